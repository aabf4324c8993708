// format_device.h -- the one device-side statement of the sample formats (SPEEXHIP_FMT_*): a sample's storage bits <->
// the internal float (one int16 step = 1.0f), and the raw loads / stores of one sample at any address the format allows;
// and with_format, through which a launcher reaches its kernels' instance of a format.  Shared by the converting kernels
// (kernels_convert.hip) and the mixing ones (kernels_mix.hip).  Bytes per sample and which formats are dithered:
// sample_bytes and dithered_fmt of kernels.h, which the host reads too.
//
// Rounding (include/speexhip_resampler.h): halfup(v) = floor(v + 0.5) on v = y * 2^k, evaluated in fp64 -- the product is
// exact there, and v + 0.5 is exact wherever its floor depends on it.  NaN becomes the format's zero, +-inf the rails.
//
// The companded formats (ULAW, ALAW: one byte per sample) go through g711.h: decoding gives an exact integer in int16
// units, encoding is the S16 rule (with or without dither) followed by the compressor on that int16.
//
// The half-float formats (F16N, BF16N) and the big-endian ones (S16BE, S24BE, S32BE) go through halfbe.h.  A big-endian
// format is its little-endian twin (le_twin) behind a byte reversal: per sample here (to_internal / from_internal take
// and give the storage bits), per dword on the kernels' vector paths (swap_words, then the twin's statements).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/speexhip_resampler.h"
#include "g711.h"
#include "halfbe.h"
#include "kernels.h"

namespace speexhip {
namespace fmtdev {

// Host side: fn(std::integral_constant<int, fmt>()) for a format known at run time -- the one place a launcher turns
// fmt into the template argument of its kernels.  No such format: hipErrorInvalidValue.
template <class Fn>
hipError_t with_format(int fmt, Fn fn) {
  switch (fmt) {
#define SPEEXHIP_FORMAT_CASE(F) case F: return fn(std::integral_constant<int, F>())
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_U8);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S16);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S24);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S32);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_F32);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_F32N);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_ULAW);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_ALAW);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_F16N);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_BF16N);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S16BE);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S24BE);
    SPEEXHIP_FORMAT_CASE(SPEEXHIP_FMT_S32BE);
#undef SPEEXHIP_FORMAT_CASE
    default: return hipErrorInvalidValue;
  }
}

// ---- byte order ----------------------------------------------------------------------------------------------------
// the little-endian format a big-endian one is the byte reversal of; every other format is its own twin
constexpr int le_twin(int f) {
  return f == SPEEXHIP_FMT_S16BE   ? SPEEXHIP_FMT_S16
         : f == SPEEXHIP_FMT_S24BE ? SPEEXHIP_FMT_S24
         : f == SPEEXHIP_FMT_S32BE ? SPEEXHIP_FMT_S32
                                   : f;
}
// The vector paths: `words` dwords of whole samples of F, in storage order, become the same samples of le_twin(F) (and
// back) -- S16BE two samples per v_perm_b32, S32BE one dword reversal each; a packed S24BE sample straddles dwords and is
// reversed on its own by to_internal / from_internal (swaps_words false).
constexpr bool swaps_words(int f) { return f == SPEEXHIP_FMT_S16BE || f == SPEEXHIP_FMT_S32BE; }
template <int F, uint32_t words>
__device__ __forceinline__ void swap_words(uint32_t *w) {
  if constexpr (swaps_words(F)) {
#pragma unroll
    for (uint32_t i = 0; i < words; i++) w[i] = F == SPEEXHIP_FMT_S16BE ? halfbe::swap16x2(w[i]) : halfbe::swap32(w[i]);
  }
}
// the format whose statements a vector path runs on words that went through swap_words
constexpr int word_format(int f) { return swaps_words(f) ? le_twin(f) : f; }

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
  if (F == SPEEXHIP_FMT_F16N) return halfbe::f16n_decode(raw);
  if (F == SPEEXHIP_FMT_BF16N) return halfbe::bf16n_decode(raw);
  if (F == SPEEXHIP_FMT_S16BE) return halfbe::pcm_decode(16, halfbe::swap16(raw));
  if (F == SPEEXHIP_FMT_S24BE) return halfbe::pcm_decode(24, halfbe::swap24(raw));
  if (F == SPEEXHIP_FMT_S32BE) return halfbe::pcm_decode(32, halfbe::swap32(raw));
  return __uint_as_float(raw) * 32768.0f;  // F32N
}

// an integer format (U8, S16, S24, S32) on its way out: round(y * scale) + bias, held to [lo, hi]; NaN becomes bias
struct IntegerFormat {
  double scale, bias, lo, hi;
};
constexpr IntegerFormat integer_format(int f) {
  return f == SPEEXHIP_FMT_U8    ? IntegerFormat{1.0 / 256.0, 128.0, 0.0, 255.0}
         : f == SPEEXHIP_FMT_S16 ? IntegerFormat{1.0, 0.0, -32768.0, 32767.0}
         : f == SPEEXHIP_FMT_S24 ? IntegerFormat{256.0, 0.0, -8388608.0, 8388607.0}
                                 : IntegerFormat{65536.0, 0.0, -2147483648.0, 2147483647.0};
}

template <int F>
__device__ __forceinline__ uint32_t from_internal(float y) {
  if (F == SPEEXHIP_FMT_F32) return __float_as_uint(y);
  if (F == SPEEXHIP_FMT_F32N) return __float_as_uint(y * (1.0f / 32768.0f));
  if (F == SPEEXHIP_FMT_ULAW) return g711::ulaw_encode(g711::s16_of(y));
  if (F == SPEEXHIP_FMT_ALAW) return g711::alaw_encode(g711::s16_of(y));
  if (F == SPEEXHIP_FMT_F16N) return halfbe::f16n_encode(y);
  if (F == SPEEXHIP_FMT_BF16N) return halfbe::bf16n_encode(y);
  if (F == SPEEXHIP_FMT_S16BE) return halfbe::swap16(static_cast<uint32_t>(halfbe::pcm_of(16, y)));
  if (F == SPEEXHIP_FMT_S24BE) return halfbe::swap24(static_cast<uint32_t>(halfbe::pcm_of(24, y)));
  if (F == SPEEXHIP_FMT_S32BE) return halfbe::swap32(static_cast<uint32_t>(halfbe::pcm_of(32, y)));
  constexpr IntegerFormat k = integer_format(F);
  if (y != y) return static_cast<uint32_t>(static_cast<int32_t>(k.bias));
  const double r = floor(static_cast<double>(y) * k.scale + 0.5) + k.bias;
  return static_cast<uint32_t>(static_cast<int32_t>(fmin(fmax(r, k.lo), k.hi)));
}

// ... with dither (dither.h): d, in LSB of the integer format F, joins v before the half-up rounding -- v = y * 2^k (exact),
// t = v + d (one fp64 rounding), floor(t + 0.5) (one more), as written: nothing contracted, nothing re-associated.  With
// d = 0 these are from_internal's bits.
template <int F>
__device__ __forceinline__ uint32_t from_internal_dither(float y, double d) {
  static_assert(dithered_fmt(F), "the integer formats are dithered, the float ones written as they are");
  // (the companded formats: d in int16 steps joins at the S16 stage, the compressor follows)
  if (F == SPEEXHIP_FMT_ULAW) return g711::ulaw_encode(g711::s16_of_dither(y, d));
  if (F == SPEEXHIP_FMT_ALAW) return g711::alaw_encode(g711::s16_of_dither(y, d));
  // (the big-endian formats: the twin's dithered rule, then the reversal)
  if (F == SPEEXHIP_FMT_S16BE) return halfbe::swap16(static_cast<uint32_t>(halfbe::pcm_of_dither(16, y, d)));
  if (F == SPEEXHIP_FMT_S24BE) return halfbe::swap24(static_cast<uint32_t>(halfbe::pcm_of_dither(24, y, d)));
  if (F == SPEEXHIP_FMT_S32BE) return halfbe::swap32(static_cast<uint32_t>(halfbe::pcm_of_dither(32, y, d)));
  constexpr IntegerFormat k = integer_format(F);
  if (y != y) return static_cast<uint32_t>(static_cast<int32_t>(k.bias));
  const double v = static_cast<double>(y) * k.scale;
  const double t = v + d;
  const double r = floor(t + 0.5) + k.bias;
  return static_cast<uint32_t>(static_cast<int32_t>(fmin(fmax(r, k.lo), k.hi)));
}

// what an output pass stores for y: kDither = false from_internal, otherwise from_internal_dither with d = noise()
template <int F, bool kDither, class Noise>
__device__ __forceinline__ uint32_t encode(float y, Noise noise) {
  if constexpr (kDither)
    return from_internal_dither<F>(y, noise());
  else
    return from_internal<F>(y);
}

// ---- one sample at its address (any byte address for the 1-byte formats and s24, an element-aligned one for the rest)
template <int F>
__device__ __forceinline__ uint32_t load_raw(const char *p) {
  if (sample_bytes(F) == 1) return *reinterpret_cast<const uint8_t *>(p);
  if (sample_bytes(F) == 2) return *reinterpret_cast<const uint16_t *>(p);
  if (sample_bytes(F) == 3) {  // (packed: byte by byte)
    const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
    return b[0] | (static_cast<uint32_t>(b[1]) << 8) | (static_cast<uint32_t>(b[2]) << 16);
  }
  return *reinterpret_cast<const uint32_t *>(p);
}
template <int F>
__device__ __forceinline__ void store_raw(char *p, uint32_t raw) {
  if (sample_bytes(F) == 1) {
    *reinterpret_cast<uint8_t *>(p) = static_cast<uint8_t>(raw);
  } else if (sample_bytes(F) == 2) {
    *reinterpret_cast<uint16_t *>(p) = static_cast<uint16_t>(raw);
  } else if (sample_bytes(F) == 3) {
    uint8_t *b = reinterpret_cast<uint8_t *>(p);
    b[0] = static_cast<uint8_t>(raw), b[1] = static_cast<uint8_t>(raw >> 8), b[2] = static_cast<uint8_t>(raw >> 16);
  } else {
    *reinterpret_cast<uint32_t *>(p) = raw;
  }
}

}  // namespace fmtdev
}  // namespace speexhip
