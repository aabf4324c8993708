// bus.h -- the one statement of a mix bus's sum (include/speexhip_resampler.h, "Buses"), host and device: the kernel
// bus_sum (kernels_bus.hip) and the host function speexhip_debug_bus (c_api.cpp) compile these very lines.  A bus sample
// is the weighted sum of the streams' samples of the same frame and channel,
//
//   acc = (double)W[j][0] * (double)y'_0
//   acc = acc + (double)W[j][s] * (double)y'_s      s = 1 .. n_streams - 1, in ascending order
//   z   = (float)acc                                one rounding, nearest even
//
// y'_s the stream's float sample behind its gain (gain.h), +0.0f where the stream has ended.  A product of two floats is
// exact in fp64 (48 significant bits of 53), so the fused multiply-add below rounds exactly where a separate multiply and
// add would: once, at the sum.  Every term is included -- a zero weight is not skipped, 0 * inf is NaN -- and the first
// term is the product itself, not 0 + the product: a sum of negative zeros stays -0.0f.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace speexhip {
namespace bus {

// the streams' pointers of a bus call travel in one kernel-argument pack (kMaxPackedStreams), and so do at most as many
// bus images of its output pass
constexpr uint32_t kMaxStreams = 32, kMaxBuses = 32;

__host__ __device__ inline double first(float w, float y) { return static_cast<double>(w) * static_cast<double>(y); }
__host__ __device__ inline double add(double acc, float w, float y) {
  return fma(static_cast<double>(w), static_cast<double>(y), acc);
}
__host__ __device__ inline float finish(double acc) { return static_cast<float>(acc); }

// bus j of one sample: y[s * y_step] = stream s's (gained) sample, w = row j of W
__host__ __device__ inline float sum(const float *w, const float *y, uint64_t y_step, uint32_t n_streams) {
  double acc = first(w[0], y[0]);
  for (uint32_t s = 1; s < n_streams; s++) acc = add(acc, w[s], y[s * y_step]);
  return finish(acc);
}

}  // namespace bus
}  // namespace speexhip
