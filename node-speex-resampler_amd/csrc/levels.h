// levels.h -- the one statement of a mixer leg's level (include/speexhip_resampler.h, "Mixer levels"), host and device:
// the kernel leg_levels (kernels_levels.hip) and the host function speexhip_debug_levels (c_api.cpp) compile these very
// lines.  One record per slot and call over all C channels of the leg, measured on the leg's float value y -- the float
// call's value in int16 units BEFORE the state's gain (y_i, not y'_i of "Mixer"): a muted leg still reads as loud.
//
//   samples   produced[i] * C         (frames of THIS call; the +0.0f padding up to bus_frames is NOT measured)
//   per sample y:
//     y != y      nan += 1; nothing else for that sample
//     otherwise   peak = max(peak, |y|)                       fp32, +inf is a legal peak
//                 r = floor((double)y + 0.5)                  "Metering"'s S16 r with d = 0
//                 q = r < -32768 ? -32768 : r > 32767 ? 32767 : r
//                 energy += (uint64)(q * q)                   integer, exact; +-inf count at their rail
//
// A lane keeps the count of NaNs, the running maximum of the bits of |y| (for non-negative, non-NaN floats the unsigned
// order of the bits is the order of the values) and the energy as an fp64 FMA chain: q is an integer of at most 16 bits,
// q * q <= 2^30, so a chain of up to kLaneMost = 2^23 terms stays below 2^53 and every partial is an integer fp64 holds
// exactly.  Whoever accumulates folds a lane into a record (fold) before it has seen more than that; the record's energy
// is a uint64.  Integers and a maximum: the record does not depend on the order of the reduction, on what shares a
// launch, or on the GPU.  A call of more than 2^34 samples in one leg wraps energy mod 2^64.
//
// (The host's sanitizer program, tools/san_host.cpp, compiles these lines with a plain C++ compiler: no HIP header there.)
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPEEXHIP_LEVELS_FN __host__ __device__ inline
#else
#define SPEEXHIP_LEVELS_FN inline
#endif

#include <cmath>
#include <cstdint>

#include "../../include/speexhip_resampler.h"

namespace speexhip {
namespace levels {

constexpr uint32_t kLaneMost = 1u << 23;  // samples a lane may take between two folds

struct Lane {
  double energy = 0.0;          // sum of q * q: an integer below 2^53
  uint32_t nan = 0, peak = 0;   // peak: bits of the largest |y|
};

SPEEXHIP_LEVELS_FN void add(Lane &l, float y) {
  // (selects, not a branch around the rest: a NaN counts, and adds the bits of 0.0 to the maximum and 0 * 0 to the
  //  energy -- nothing -- so that the samples of a trip are straight-line code and their loads can be in flight together)
  const bool number = y == y;
  l.nan += number ? 0u : 1u;
  const uint32_t bits = number ? __builtin_bit_cast(uint32_t, y) & 0x7fffffffu : 0u;  // |y|
  l.peak = bits > l.peak ? bits : l.peak;
  const double r = floor(static_cast<double>(y) + 0.5);
  const double held = r < -32768.0 ? -32768.0 : r > 32767.0 ? 32767.0 : r;
  const double q = number ? held : 0.0;
  l.energy = fma(q, q, l.energy);
}

// a lane's share into a record (samples is the caller's: it knows what the leg produced)
SPEEXHIP_LEVELS_FN void fold(SpeexHipLevel &rec, const Lane &l) {
  rec.energy += static_cast<uint64_t>(l.energy);
  rec.nan += l.nan;
  const uint32_t now = __builtin_bit_cast(uint32_t, rec.peak);
  rec.peak = __builtin_bit_cast(float, l.peak > now ? l.peak : now);
}

}  // namespace levels
}  // namespace speexhip
