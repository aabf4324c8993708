// dither.h -- the one statement of the dither noise (include/speexhip_resampler.h, "Dither"), host and device: the
// converting and mixing kernels (kernels_convert.hip, kernels_mix.hip) and the host function speexhip_debug_dither
// (c_api.cpp) compile these very lines.  The noise of an output sample is a pure function of (seed, idx), idx = the
// sample's index in its stream since position 0: counter based, nothing carried from sample to sample.
//
//   mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32, wrapping)
//   w = mix32( lo32(idx) ^ mix32( hi32(idx) ^ hi32(seed) ) ^ lo32(seed) );   a = w & 0xffff,  b = w >> 16
//   d = 0 (NONE),  (a + 0.5) / 65536 - 0.5 (RECTANGULAR),  (a - b) / 65536 (TRIANGULAR)             in LSB of the output
//
// Every d is a multiple of 2^-17 below 1 in magnitude: exact in fp64, however it is evaluated.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/speexhip_resampler.h"

namespace speexhip {
namespace dither {

__host__ __device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

inline bool known_kind(int kind) {
  return kind == SPEEXHIP_DITHER_NONE || kind == SPEEXHIP_DITHER_RECTANGULAR || kind == SPEEXHIP_DITHER_TRIANGULAR;
}

// The inner half of w: everything but lo32(idx).  It changes once per 2^32 samples of a stream.
__host__ __device__ inline uint32_t key_of(uint64_t seed, uint32_t idx_hi) {
  return mix32(idx_hi ^ static_cast<uint32_t>(seed >> 32)) ^ static_cast<uint32_t>(seed);
}
__host__ __device__ inline uint32_t word_of(uint32_t key, uint32_t idx_lo) { return mix32(idx_lo ^ key); }

// d of one random word
__host__ __device__ inline double value_of(int kind, uint32_t w) {
  const int32_t a = static_cast<int32_t>(w & 0xffffu), b = static_cast<int32_t>(w >> 16);
  if (kind == SPEEXHIP_DITHER_RECTANGULAR) return (static_cast<double>(a) + 0.5) / 65536.0 - 0.5;
  if (kind == SPEEXHIP_DITHER_TRIANGULAR) return static_cast<double>(a - b) / 65536.0;
  return 0.0;
}

// d of sample idx
__host__ __device__ inline double noise(int kind, uint64_t seed, uint64_t idx) {
  return value_of(kind, word_of(key_of(seed, static_cast<uint32_t>(idx >> 32)), static_cast<uint32_t>(idx)));
}

// A run of consecutive samples idx0 .. idx0 + n - 1 (n <= 2^32: a lane's group, the samples of a frame) crosses at most
// one 2^32 boundary of idx: the inner half is taken once for the run, a second time only when the run does cross.
struct Run {
  uint32_t lo0, key0, key1;
};
__host__ __device__ inline Run run_of(uint64_t seed, uint64_t idx0, uint32_t n) {
  Run r;
  const uint32_t hi0 = static_cast<uint32_t>(idx0 >> 32);
  r.lo0 = static_cast<uint32_t>(idx0);
  r.key0 = key_of(seed, hi0);
  r.key1 = r.key0;
  if (n != 0 && r.lo0 + (n - 1u) < r.lo0) r.key1 = key_of(seed, hi0 + 1u);  // (idx wraps at 2^64 like its halves)
  return r;
}
// d of sample j of the run
__host__ __device__ inline double noise_in(int kind, const Run &r, uint32_t j) {
  const uint32_t lo = r.lo0 + j;
  return value_of(kind, word_of(lo < r.lo0 ? r.key1 : r.key0, lo));
}

// seed of stream s of a batch
inline uint64_t stream_seed(uint64_t seed, uint32_t s) { return seed + static_cast<uint64_t>(s) * 0x9E3779B97F4A7C15ull; }

}  // namespace dither
}  // namespace speexhip
