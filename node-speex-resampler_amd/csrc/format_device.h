// format_device.h -- the one device-side statement of the sample formats (SPEEXHIP_FMT_*): a sample's storage bits <->
// the internal float (one int16 step = 1.0f), and the raw loads / stores of one sample at any address the format allows.
// Shared by the converting kernels (kernels_convert.hip) and the mixing ones (kernels_mix.hip).
//
// Rounding (include/speexhip_resampler.h): halfup(v) = floor(v + 0.5) on v = y * 2^k, evaluated in fp64 -- the product is
// exact there, and v + 0.5 is exact wherever its floor depends on it.  NaN becomes the format's zero, +-inf the rails.
//
// The companded formats (ULAW, ALAW: one byte per sample) go through g711.h: decoding gives an exact integer in int16
// units, encoding is the S16 rule (with or without dither) followed by the compressor on that int16.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/speexhip_resampler.h"
#include "g711.h"

namespace speexhip {
namespace fmtdev {

constexpr uint32_t bytes_of(int f) {
  return f == SPEEXHIP_FMT_U8 || f == SPEEXHIP_FMT_ULAW || f == SPEEXHIP_FMT_ALAW ? 1u
         : f == SPEEXHIP_FMT_S16                                                    ? 2u
         : f == SPEEXHIP_FMT_S24                                                    ? 3u
                                                                                    : 4u;
}

// ---- one sample --------------------------------------------------------------------------------------------------
// `raw` = the sample's storage bits in the low bytes of a dword
template <int F>
__device__ __forceinline__ float to_internal(uint32_t raw) {
  if (F == SPEEXHIP_FMT_U8) return (static_cast<float>(raw & 0xffu) - 128.0f) * 256.0f;
  if (F == SPEEXHIP_FMT_S16) return static_cast<float>(static_cast<int16_t>(raw));
  if (F == SPEEXHIP_FMT_S24) return static_cast<float>(static_cast<int32_t>(raw << 8) >> 8) * (1.0f / 256.0f);
  if (F == SPEEXHIP_FMT_S32) return static_cast<float>(static_cast<int32_t>(raw)) * (1.0f / 65536.0f);
  if (F == SPEEXHIP_FMT_F32) return __uint_as_float(raw);
  if (F == SPEEXHIP_FMT_ULAW) return static_cast<float>(g711::ulaw_decode(raw & 0xffu));
  if (F == SPEEXHIP_FMT_ALAW) return static_cast<float>(g711::alaw_decode(raw & 0xffu));
  return __uint_as_float(raw) * 32768.0f;  // F32N
}

template <int F>
__device__ __forceinline__ uint32_t from_internal(float y) {
  if (F == SPEEXHIP_FMT_F32) return __float_as_uint(y);
  if (F == SPEEXHIP_FMT_F32N) return __float_as_uint(y * (1.0f / 32768.0f));
  if (F == SPEEXHIP_FMT_ULAW) return g711::ulaw_encode(g711::s16_of(y));
  if (F == SPEEXHIP_FMT_ALAW) return g711::alaw_encode(g711::s16_of(y));
  constexpr double scale = F == SPEEXHIP_FMT_U8 ? 1.0 / 256.0 : F == SPEEXHIP_FMT_S16 ? 1.0 : F == SPEEXHIP_FMT_S24 ? 256.0 : 65536.0;
  constexpr double bias = F == SPEEXHIP_FMT_U8 ? 128.0 : 0.0;
  constexpr double lo = F == SPEEXHIP_FMT_U8 ? 0.0 : F == SPEEXHIP_FMT_S16 ? -32768.0 : F == SPEEXHIP_FMT_S24 ? -8388608.0 : -2147483648.0;
  constexpr double hi = F == SPEEXHIP_FMT_U8 ? 255.0 : F == SPEEXHIP_FMT_S16 ? 32767.0 : F == SPEEXHIP_FMT_S24 ? 8388607.0 : 2147483647.0;
  if (y != y) return static_cast<uint32_t>(static_cast<int32_t>(bias));
  const double r = floor(static_cast<double>(y) * scale + 0.5) + bias;
  return static_cast<uint32_t>(static_cast<int32_t>(fmin(fmax(r, lo), hi)));
}

// ... with dither (dither.h): d, in LSB of the integer format F, joins v before the half-up rounding -- v = y * 2^k (exact),
// t = v + d (one fp64 rounding), floor(t + 0.5) (one more), as written: nothing contracted, nothing re-associated.  With
// d = 0 these are from_internal's bits.
template <int F>
__device__ __forceinline__ uint32_t from_internal_dither(float y, double d) {
  static_assert(F == SPEEXHIP_FMT_U8 || F == SPEEXHIP_FMT_S16 || F == SPEEXHIP_FMT_S24 || F == SPEEXHIP_FMT_S32 ||
                    F == SPEEXHIP_FMT_ULAW || F == SPEEXHIP_FMT_ALAW,
                "the integer formats are dithered, the float ones written as they are");
  // (the companded formats: d in int16 steps joins at the S16 stage, the compressor follows)
  if (F == SPEEXHIP_FMT_ULAW) return g711::ulaw_encode(g711::s16_of_dither(y, d));
  if (F == SPEEXHIP_FMT_ALAW) return g711::alaw_encode(g711::s16_of_dither(y, d));
  constexpr double scale = F == SPEEXHIP_FMT_U8 ? 1.0 / 256.0 : F == SPEEXHIP_FMT_S16 ? 1.0 : F == SPEEXHIP_FMT_S24 ? 256.0 : 65536.0;
  constexpr double bias = F == SPEEXHIP_FMT_U8 ? 128.0 : 0.0;
  constexpr double lo = F == SPEEXHIP_FMT_U8 ? 0.0 : F == SPEEXHIP_FMT_S16 ? -32768.0 : F == SPEEXHIP_FMT_S24 ? -8388608.0 : -2147483648.0;
  constexpr double hi = F == SPEEXHIP_FMT_U8 ? 255.0 : F == SPEEXHIP_FMT_S16 ? 32767.0 : F == SPEEXHIP_FMT_S24 ? 8388607.0 : 2147483647.0;
  if (y != y) return static_cast<uint32_t>(static_cast<int32_t>(bias));
  const double v = static_cast<double>(y) * scale;
  const double t = v + d;
  const double r = floor(t + 0.5) + bias;
  return static_cast<uint32_t>(static_cast<int32_t>(fmin(fmax(r, lo), hi)));
}

// ---- one sample at its address (any byte address for the 1-byte formats and s24, an element-aligned one for the rest)
template <int F>
__device__ __forceinline__ uint32_t load_raw(const char *p) {
  if (bytes_of(F) == 1) return *reinterpret_cast<const uint8_t *>(p);
  if (F == SPEEXHIP_FMT_S16) return *reinterpret_cast<const uint16_t *>(p);
  if (F == SPEEXHIP_FMT_S24) {
    const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
    return b[0] | (static_cast<uint32_t>(b[1]) << 8) | (static_cast<uint32_t>(b[2]) << 16);
  }
  return *reinterpret_cast<const uint32_t *>(p);
}
template <int F>
__device__ __forceinline__ void store_raw(char *p, uint32_t raw) {
  if (bytes_of(F) == 1) {
    *reinterpret_cast<uint8_t *>(p) = static_cast<uint8_t>(raw);
  } else if (F == SPEEXHIP_FMT_S16) {
    *reinterpret_cast<uint16_t *>(p) = static_cast<uint16_t>(raw);
  } else if (F == SPEEXHIP_FMT_S24) {
    uint8_t *b = reinterpret_cast<uint8_t *>(p);
    b[0] = static_cast<uint8_t>(raw), b[1] = static_cast<uint8_t>(raw >> 8), b[2] = static_cast<uint8_t>(raw >> 16);
  } else {
    *reinterpret_cast<uint32_t *>(p) = raw;
  }
}

}  // namespace fmtdev
}  // namespace speexhip
