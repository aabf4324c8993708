// halfbe.h -- the one statement of the half-float and big-endian sample formats (include/speexhip_resampler.h,
// "Half-float and big-endian formats"), host and device: format_device.h, and through it the converting, mixing and
// plane kernels (kernels_convert.hip, kernels_mix.hip, kernels_sides.hip), and the host functions
// speexhip_debug_format_decode / _encode (c_api.cpp) compile these very lines.
//   F16N   IEEE binary16, +-1.0 full scale      BF16N  bfloat16 (the upper half of an fp32), +-1.0 full scale
//   S16BE / S24BE / S32BE   the S16 / S24 / S32 sample with its bytes reversed
// No tables.  Integer arithmetic where the bits are stated as integer arithmetic (bf16, the NaN codes); the binary16
// conversions are the language's own (_Float16: v_cvt_f16_f32 / v_cvt_f32_f16 on the device, round to nearest even with
// subnormals kept on both sides), which are the stated bits for everything but NaN -- that is one select.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace speexhip {
namespace halfbe {

__host__ __device__ inline uint32_t bits_of(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof(u));
  return u;
}
__host__ __device__ inline float float_of(uint32_t u) {
  float v;
  memcpy(&v, &u, sizeof(v));
  return v;
}

// ---- byte order: a sample's storage bits (low bytes of a dword) <-> the little-endian sample's ------------------------
__host__ __device__ inline uint32_t swap16(uint32_t raw) { return ((raw & 0xffu) << 8) | ((raw >> 8) & 0xffu); }
__host__ __device__ inline uint32_t swap24(uint32_t raw) { return __builtin_bswap32(raw) >> 8; }  // (raw's top byte is dropped)
__host__ __device__ inline uint32_t swap32(uint32_t raw) { return __builtin_bswap32(raw); }
// both 16-bit samples of a dword at once (the vector paths: one v_perm_b32 on the device)
__host__ __device__ inline uint32_t swap16x2(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, w, 0x02030001u);
#else
  return ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu);
#endif
}

// ---- the integer stage of the big-endian encoders: the S16 / S24 / S32 row of the header's table ------------------------
// q = clamp(halfup(y * scale), lo, hi) in fp64; NaN -> 0, +-inf -> the rails.  With d (LSB of the format): v = y * scale
// (exact), t = v + d (one rounding), floor(t + 0.5) (one more), as written.  bits = 16, 24 or 32.
__host__ __device__ constexpr double pcm_scale(int bits) { return bits == 16 ? 1.0 : bits == 24 ? 256.0 : 65536.0; }
__host__ __device__ constexpr double pcm_hi(int bits) { return bits == 16 ? 32767.0 : bits == 24 ? 8388607.0 : 2147483647.0; }
__host__ __device__ inline int32_t pcm_of(int bits, float y) {
  if (y != y) return 0;
  const double r = floor(static_cast<double>(y) * pcm_scale(bits) + 0.5);
  return static_cast<int32_t>(fmin(fmax(r, -pcm_hi(bits) - 1.0), pcm_hi(bits)));
}
__host__ __device__ inline int32_t pcm_of_dither(int bits, float y, double d) {
  if (y != y) return 0;
  const double v = static_cast<double>(y) * pcm_scale(bits);
  const double t = v + d;
  const double r = floor(t + 0.5);
  return static_cast<int32_t>(fmin(fmax(r, -pcm_hi(bits) - 1.0), pcm_hi(bits)));
}
// the little-endian sample as the internal float (the S16 / S24 / S32 decode rule)
__host__ __device__ inline float pcm_decode(int bits, uint32_t le) {
  if (bits == 16) return static_cast<float>(static_cast<int16_t>(le));
  if (bits == 24) return static_cast<float>(static_cast<int32_t>(le << 8) >> 8) * (1.0f / 256.0f);
  return static_cast<float>(static_cast<int32_t>(le)) * (1.0f / 65536.0f);
}

// ---- F16N ---------------------------------------------------------------------------------------------------------------
// x = (float)h * 32768: both steps exact for every code, subnormals included; +-inf stay, NaN stays NaN
__host__ __device__ inline float f16n_decode(uint32_t h) {
  const uint16_t code = static_cast<uint16_t>(h);
  _Float16 v;
  memcpy(&v, &code, sizeof(v));
  return static_cast<float>(v) * 32768.0f;
}
// z = y / 32768 in fp32, rounded to nearest even to binary16, subnormals kept, |z| >= 65520 -> +-inf; NaN -> 0x7E00 | sign
__host__ __device__ inline uint32_t f16n_encode(float y) {
  const float z = y * (1.0f / 32768.0f);
  const _Float16 v = static_cast<_Float16>(z);
  uint16_t code;
  memcpy(&code, &v, sizeof(code));
  return z != z ? 0x7e00u | ((bits_of(z) >> 16) & 0x8000u) : code;
}

// ---- BF16N --------------------------------------------------------------------------------------------------------------
// x = as_float(b << 16) * 32768: one fp32 product
__host__ __device__ inline float bf16n_decode(uint32_t b) { return float_of((b & 0xffffu) << 16) * 32768.0f; }
// z = y / 32768 in fp32, u = its bits: NaN -> 0x7FC0 | sign, otherwise round to nearest even on the integer (overflow
// rounds into 0x7F80 by itself)
__host__ __device__ inline uint32_t bf16n_encode(float y) {
  const float z = y * (1.0f / 32768.0f);
  const uint32_t u = bits_of(z);
  return z != z ? 0x7fc0u | ((u >> 16) & 0x8000u) : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace halfbe
}  // namespace speexhip
