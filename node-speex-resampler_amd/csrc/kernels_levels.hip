// kernels_levels.hip -- leg_levels: the level of every leg of a mixer call (include/speexhip_resampler.h, "Mixer levels";
// levels.h states the record), one small reduction over the legs' float images while they are resident, behind the last
// FIR launch of the call and beside bus_sum_legs (kernels_bus_legs.hip), whose table of the legs it reads: src and frames,
// through scalar loads -- the slot is the workgroup's, so everything it selects by is wave-uniform.  The gain in the record
// is not read: a level is the leg's value BEFORE its gain.
//
// Shape ("Mixer", has the numbers).  The grid is (span, slot): a span is kSpan = 65 536 consecutive samples of a
// leg, a workgroup 256 lanes, so a lane takes at most 256 samples -- its fp64 energy chain is exact up to 2^23 (levels.h).
// Where the span's base lies on a 16-byte boundary (the images are 128-byte aligned, a span is 256 KiB) the lanes walk it
// in trips of 1024 samples, one 16-byte load a lane and trip; what is left behind the last whole trip -- and a span whose
// base is off that alignment, whole -- is read sample by sample, every lane inside the leg, its last sample at the
// furthest, keeping what is its own (as load_samples of bus_sum_legs does).  The lanes' partials are folded over the wave
// with __shfl_xor, over the four waves through LDS, and lane 0 writes the 32-byte record with ordinary stores.
//
// No atomics: for a small call the records lie in pinned HOST memory, which the kernel writes in place.  A call whose
// every leg is one span -- every tick of a bridge -- is ONE launch that writes the records where they travel from.  A
// call in which some leg has more spans writes one partial per (slot, span) into a device block (slot-major, `spans` a
// slot; a span behind a leg's end is not written and not read) and a second, tiny launch -- a wave per slot -- folds a
// slot's partials into its record.  No matrix instruction.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "levels.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(levels)

namespace {

constexpr uint32_t kLanes = 256, kWaves = kLanes / 64, kQuad = 4, kTrip = kLanes * kQuad;
constexpr uint32_t kSpan = kLevelSpan;
static_assert(kSpan % kTrip == 0, "a whole span is whole trips");
static_assert(kSpan / kLanes <= levels::kLaneMost, "a lane's energy chain stays exact");

// (a pointer read from memory is a generic one to the compiler: the images are global memory, and said to be here)
typedef const __attribute__((address_space(1))) float *GlobalFloats;
typedef float Quad __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) Quad *GlobalQuads;

// what the wave's lanes hold, folded into every lane of the wave
__device__ __forceinline__ void fold_wave(uint64_t &energy, uint32_t &nan, uint32_t &peak) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    energy += __shfl_xor(static_cast<unsigned long long>(energy), off);
    nan += __shfl_xor(nan, off);
    const uint32_t other = __shfl_xor(peak, off);
    peak = other > peak ? other : peak;
  }
}

// span blockIdx.x of the leg in slot blockIdx.y
__global__ __launch_bounds__(kLanes) void leg_levels(const LevelsArgs a) {
  __shared__ uint64_t part_energy[kWaves];
  __shared__ uint32_t part_nan[kWaves], part_peak[kWaves];
  const uint32_t slot = blockIdx.y, span = blockIdx.x;
  const BusLeg *__restrict__ leg = a.legs + slot;
  const uint64_t n = static_cast<uint64_t>(leg->frames) * a.channels;
  const uint64_t span0 = static_cast<uint64_t>(span) * kSpan;
  // (the whole workgroup: no barrier is left waiting.  Span 0 of every slot runs: an empty slot's record is written, zeros)
  if (span != 0 && span0 >= n) return;
  const uint32_t left = span0 >= n ? 0u : static_cast<uint32_t>(min(static_cast<uint64_t>(kSpan), n - span0));
  levels::Lane mine;
  if (left != 0) {
    const GlobalFloats src = (GlobalFloats)(leg->src + span0);
    const uint32_t trips = (reinterpret_cast<uintptr_t>(leg->src + span0) & 15u) == 0 ? left / kTrip : 0u;
#pragma unroll 4
    for (uint32_t t = 0; t < trips; t++) {
      const Quad v = *(GlobalQuads)(src + t * kTrip + threadIdx.x * kQuad);
      levels::add(mine, v.x);
      levels::add(mine, v.y);
      levels::add(mine, v.z);
      levels::add(mine, v.w);
    }
    for (uint32_t i = trips * kTrip + threadIdx.x; i - threadIdx.x < left; i += kLanes) {
      const float v = src[min(i, left - 1)];
      if (i < left) levels::add(mine, v);
    }
  }
  uint64_t energy = static_cast<uint64_t>(mine.energy);
  uint32_t nan = mine.nan, peak = mine.peak;
  fold_wave(energy, nan, peak);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) part_energy[wave] = energy, part_nan[wave] = nan, part_peak[wave] = peak;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kWaves; w++) {
      energy += part_energy[w], nan += part_nan[w];
      peak = part_peak[w] > peak ? part_peak[w] : peak;
    }
    SpeexHipLevel rec;
    rec.samples = a.spans == 1 ? n : left;
    rec.energy = energy;
    rec.nan = nan;
    rec.peak = __builtin_bit_cast(float, peak);
    rec.reserved = 0;
    a.dst[a.spans == 1 ? slot : static_cast<size_t>(slot) * a.spans + span] = rec;
  }
}

// wave blockIdx.x folds the partials of slot blockIdx.x (a.dst of leg_levels) into its record
__global__ __launch_bounds__(64) void fold_levels(const LevelsArgs a, SpeexHipLevel *__restrict__ records) {
  const uint32_t slot = blockIdx.x;
  const uint64_t n = static_cast<uint64_t>(a.legs[slot].frames) * a.channels;
  // (span 0 is written for every slot; behind it, the spans that begin inside the leg)
  const uint32_t have = n == 0 ? 1u : static_cast<uint32_t>((n + kSpan - 1) / kSpan);
  const SpeexHipLevel *__restrict__ part = a.dst + static_cast<size_t>(slot) * a.spans;
  uint64_t energy = 0;
  uint32_t peak = 0;
  uint64_t nan = 0;
  for (uint32_t s = threadIdx.x; s < have; s += 64) {
    energy += part[s].energy;
    nan += part[s].nan;
    const uint32_t bits = __builtin_bit_cast(uint32_t, part[s].peak);
    peak = bits > peak ? bits : peak;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    energy += __shfl_xor(static_cast<unsigned long long>(energy), off);
    nan += __shfl_xor(static_cast<unsigned long long>(nan), off);
    const uint32_t other = __shfl_xor(peak, off);
    peak = other > peak ? other : peak;
  }
  if (threadIdx.x == 0) {
    SpeexHipLevel rec;
    rec.samples = n;
    rec.energy = energy;
    rec.nan = nan;
    rec.peak = __builtin_bit_cast(float, peak);
    rec.reserved = 0;
    records[slot] = rec;
  }
}

}  // namespace

uint64_t level_spans(const BusLeg *host_legs, uint32_t n_legs, uint32_t channels) {
  uint64_t spans = 1;
  for (uint32_t s = 0; host_legs != nullptr && s < n_legs; s++)
    spans = std::max(spans, (static_cast<uint64_t>(host_legs[s].frames) * channels + kSpan - 1) / kSpan);
  return spans;
}

hipError_t launch_leg_levels(const BusLeg *legs, const BusLeg *host_legs, uint32_t n_legs, uint32_t channels, uint32_t bus_frames,
                             SpeexHipLevel *records, SpeexHipLevel *partials, size_t partials_room, hipStream_t stream,
                             uint32_t *launches) {
  if (bus_frames == 0) return hipSuccess;
  if (n_legs == 0 || n_legs > kBusMaxLegs || channels == 0 || legs == nullptr || host_legs == nullptr || records == nullptr)
    return hipErrorInvalidValue;
  for (uint32_t s = 0; s < n_legs; s++) {
    const BusLeg &leg = host_legs[s];
    if (leg.frames > bus_frames || (leg.frames != 0 && leg.src == nullptr)) return hipErrorInvalidValue;
  }
  const uint64_t spans = level_spans(host_legs, n_legs, channels);
  if (spans > 0x7fffffffull) return hipErrorInvalidValue;
  if (spans > 1 && (partials == nullptr || partials_room / sizeof(SpeexHipLevel) / n_legs < spans)) return hipErrorInvalidValue;
  LevelsArgs a;
  a.legs = legs;
  a.dst = spans == 1 ? records : partials;
  a.channels = channels;
  a.spans = static_cast<uint32_t>(spans);
  hipLaunchKernelGGL(leg_levels, dim3(a.spans, n_legs), dim3(kLanes), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (launches != nullptr) (*launches)++;
  if (spans > 1) {
    hipLaunchKernelGGL(fold_levels, dim3(n_legs), dim3(64), 0, stream, a, records);
    e = hipGetLastError();
    if (e == hipSuccess && launches != nullptr) (*launches)++;
  }
  return e;
}

}  // namespace speexhip
