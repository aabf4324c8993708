// g711.h -- the one statement of the companded sample formats (include/speexhip_resampler.h, "Companded formats"),
// host and device: format_device.h, and through it the converting and mixing kernels (kernels_convert.hip,
// kernels_mix.hip), and the host functions speexhip_debug_g711_decode / _encode (c_api.cpp) compile these very lines.
// G.711 mu-law (PCMU) and A-law (PCMA): one byte per sample.  Decoding gives an exact integer in int16 units, encoding
// takes the int16 the S16 output rule made.  Integer arithmetic only, no tables: a handful of shifts and one count of
// leading zeros per sample.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace speexhip {
namespace g711 {

// floor(log2(v)), v >= 1
__host__ __device__ inline uint32_t log2_floor(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 31u - static_cast<uint32_t>(__clz(static_cast<int>(v)));
#else
  return 31u - static_cast<uint32_t>(__builtin_clz(v));
#endif
}

// ---- mu-law: range +-32124; byte 0x7f is the negative zero and decodes to 0 ----------------------------------------
__host__ __device__ inline int32_t ulaw_decode(uint32_t b) {
  const uint32_t u = ~b & 0xffu, e = (u >> 4) & 7u, m = u & 15u;
  const int32_t t = static_cast<int32_t>((((m << 3) + 0x84u) << e) - 0x84u);
  return (u & 0x80u) ? -t : t;
}
// q = an int16 value
__host__ __device__ inline uint32_t ulaw_encode(int32_t q) {
  const uint32_t s = q < 0 ? 1u : 0u;
  const uint32_t a = static_cast<uint32_t>(q < 0 ? -q : q);
  const uint32_t mag = (a < 32635u ? a : 32635u) + 132u;  // 132 .. 32767: e = 0 .. 7
  const uint32_t e = log2_floor(mag) - 7u;
  const uint32_t m = (mag >> (e + 3u)) & 15u;
  return ~((s << 7) | (e << 4) | m) & 0xffu;
}

// ---- A-law: range +-32256 --------------------------------------------------------------------------------------------
__host__ __device__ inline int32_t alaw_decode(uint32_t b) {
  const uint32_t a = (b ^ 0x55u) & 0xffu, e = (a >> 4) & 7u, m = a & 15u;
  const int32_t t = static_cast<int32_t>(e == 0 ? (m << 4) + 8u : ((m << 4) + 0x108u) << (e - 1u));
  return (a & 0x80u) ? t : -t;
}
// q = an int16 value
__host__ __device__ inline uint32_t alaw_encode(int32_t q) {
  const uint32_t pos = q >= 0 ? 1u : 0u;
  const uint32_t mag = static_cast<uint32_t>(q >= 0 ? q : -q - 1) >> 3;  // 0 .. 4095
  const uint32_t e = mag < 32u ? 0u : log2_floor(mag) - 4u;                // 0 .. 7
  const uint32_t m = e == 0 ? (mag >> 1) & 15u : (mag >> e) & 15u;
  return ((pos << 7) | (e << 4) | m) ^ 0x55u;
}

// ---- the S16 stage of the encoder (the S16 row of the header's table; with d, the dithered rule) ----------------------
// q = clamp(halfup(y), -32768, 32767) in fp64; NaN -> 0, +-inf -> the rails.  d in int16 steps: v = y, t = v + d (one
// rounding), floor(t + 0.5) (one more), as written.
__host__ __device__ inline int32_t s16_of(float y) {
  if (y != y) return 0;
  const double r = floor(static_cast<double>(y) + 0.5);
  return static_cast<int32_t>(fmin(fmax(r, -32768.0), 32767.0));
}
__host__ __device__ inline int32_t s16_of_dither(float y, double d) {
  if (y != y) return 0;
  const double v = static_cast<double>(y);
  const double t = v + d;
  const double r = floor(t + 0.5);
  return static_cast<int32_t>(fmin(fmax(r, -32768.0), 32767.0));
}

}  // namespace g711
}  // namespace speexhip
