// meter.h -- the one statement of the output meter (include/speexhip_resampler.h, "Metering"), host and device: the
// metered instances of the output passes (kernels_convert.hip, kernels_convert_many.hip, kernels_mix.hip,
// kernels_sides.hip), the kernel meter_image and the host function speexhip_debug_meter (c_api.cpp) compile these very
// lines.  For one value y that a pass is about to encode to format F, with d the dither of that sample (0: none):
//
//   nan:   y != y; nothing else is counted for that sample
//   peak:  |y| in int16 units -- the value that enters from_internal: behind the output matrix, before the dither
//   clipped_high / clipped_low (the formats of dithered_fmt only):  r > hi / r < lo,  r = floor(t + 0.5),  t = v + d,
//          v = (double)y * scale -- from_internal_dither's own statements, r being what its clamp is about to hold to
//          [lo, hi] (U8: behind the offset of 128, an exact addition); scale, lo and hi are integer_format's.  The companded formats are judged at their S16 stage (g711::s16_of: the compressor's own
//          limit is no clip), a big-endian format as its little-endian twin; +-inf clip at their rail.
//   The float formats count no clip: their callers read the peak (above 32768.0: beyond +-1.0).
//
// A lane keeps three counts and the running maximum of the bits of |y| (for non-negative, non-NaN floats the unsigned
// order of the bits is the order of the values).  Integers and a maximum: the totals do not depend on the order of
// accumulation, so a stream's totals depend on the stream alone -- not on chunking, on what shares a launch, or on the GPU.
//
// On the device a workgroup folds its lanes with commit(): __shfl_xor over the wave, the waves through LDS, then at most
// one atomic per quantity and workgroup on the stream's MeterCell -- atomicAdd on the counts that are not zero (clips are
// rare), atomicMax on the peak's bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/speexhip_resampler.h"
#include "format_device.h"
#include "kernels.h"

namespace speexhip {
namespace meter {

struct Lane {
  uint32_t hi = 0, lo = 0, nan = 0, peak = 0;  // peak: bits of the largest |y|
};

// the integer format whose rails judge F (F a dithered_fmt)
constexpr int judged_as(int f) {
  return f == SPEEXHIP_FMT_ULAW || f == SPEEXHIP_FMT_ALAW ? SPEEXHIP_FMT_S16 : fmtdev::le_twin(f);
}

template <int F>
__host__ __device__ inline void judge(Lane &m, float y, double d) {
  if (y != y) {
    m.nan++;
    return;
  }
  const uint32_t bits = __builtin_bit_cast(uint32_t, y) & 0x7fffffffu;  // |y|
  m.peak = bits > m.peak ? bits : m.peak;
  if constexpr (dithered_fmt(F)) {
    constexpr fmtdev::IntegerFormat k = fmtdev::integer_format(judged_as(F));
    const double v = static_cast<double>(y) * k.scale;
    const double t = v + d;
    const double r = floor(t + 0.5) + k.bias;  // (what the clamp is about to hold to [lo, hi]; the U8 offset is exact)
    // (sums of 0 / 1, not branches: two conditional increments become one increment through a selected address, which
    //  keeps the lane's counts in scratch memory)
    m.hi += r > k.hi ? 1u : 0u;
    m.lo += r < k.lo ? 1u : 0u;
  }
}

#if defined(__HIPCC__)
// What a metered output pass stores for y, judged on its way: fmtdev::encode's bits (kDither with kind NONE: d = 0, the
// undithered bytes).  kMeter = false IS fmtdev::encode: m is not touched.
template <int F, bool kDither, bool kMeter, class Noise>
__device__ __forceinline__ uint32_t encode(Lane &m, float y, Noise noise) {
  if constexpr (!kMeter) {
    return fmtdev::encode<F, kDither>(y, noise);
  } else if constexpr (kDither) {
    const double d = noise();
    judge<F>(m, y, d);
    return fmtdev::from_internal_dither<F>(y, d);
  } else {
    judge<F>(m, y, 0.0);
    return fmtdev::from_internal<F>(y);
  }
}

// Every lane of the workgroup (up to 256: four waves) arrives here once, with what it counted; cell is wave-uniform.
__device__ __forceinline__ void commit(const Lane &m, MeterCell *cell) {
  __shared__ uint32_t part[4][4];
  uint32_t hi = m.hi, lo = m.lo, nan = m.nan, peak = m.peak;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    hi += __shfl_xor(hi, off);
    lo += __shfl_xor(lo, off);
    nan += __shfl_xor(nan, off);
    const uint32_t other = __shfl_xor(peak, off);
    peak = other > peak ? other : peak;
  }
  const uint32_t wave = threadIdx.x >> 6, waves = (blockDim.x + 63u) >> 6;
  if ((threadIdx.x & 63u) == 0 && wave < 4) part[wave][0] = hi, part[wave][1] = lo, part[wave][2] = nan, part[wave][3] = peak;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < waves && w < 4; w++) {
      hi += part[w][0], lo += part[w][1], nan += part[w][2];
      peak = part[w][3] > peak ? part[w][3] : peak;
    }
    if (hi != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&cell->hi), static_cast<unsigned long long>(hi));
    if (lo != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&cell->lo), static_cast<unsigned long long>(lo));
    if (nan != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&cell->nan), static_cast<unsigned long long>(nan));
    if (peak != 0) atomicMax(&cell->peak_bits, peak);
  }
}
#endif

}  // namespace meter
}  // namespace speexhip
