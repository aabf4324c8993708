// kernels_bus_legs.hip -- bus_sum_legs: the weighted sums of a mixer's legs (include/speexhip_resampler.h, "Mixer"; bus.h
// states the sum, gain.h the gain), the one pass of a mixer call between the legs' FIR launches and the output pass over the
// buses.  It stands beside bus_sum (kernels_bus.hip), which keeps the Batch's bus call: up to 1024 legs x 1024 buses do not
// fit bus_sum's kernel-argument pack of 32 streams, nor its habit of reading every stream once per group of 8 buses.
//
// Shape ("Mixer", has the numbers).  What bounds a wide mix is not bytes but the chain it waits on: a leg's
// record, then its samples and its weights, then the fp64 adds, leg after leg in the order the rule fixes -- and a 20 ms
// tick is few workgroups, so nothing else on the CU hides that chain.  So a workgroup of 256 lanes takes one tile of
// kTile = 128 consecutive samples and one group of up to kWgBuses = 32 buses, and walks the legs in BLOCKS of kLegBlock =
// 16: the four waves fetch the block's sixteen tiles together (four legs a wave, one 8-byte load a lane and leg) and, two
// floats a lane, the block's 16 x 32 weights -- all of it in flight at once where bus_sum has one load -- multiply each
// tile by its leg's gain ONCE and lay tiles and weights in LDS (8 + 2 KiB); behind a barrier wave w sums the block into
// its own kBusGroup = 8 buses, 8 x 2 fp64 accumulators a lane (32 VGPRs), reading a leg's two samples and, at one address
// for the whole wave, its eight weights back from LDS.  The next block's loads are issued before the sums of this one and
// waited for behind them.  A leg's tile is thus read from L2 once per 32 buses, not once per 8, and gained once, not once
// per group.  (The weights came through one aligned 32-byte scalar load per leg and wave at first: each a miss of the
// scalar cache, waited for leg by leg -- a fifth of the kernel's time; DESIGN.md.)
// Everything the loop selects by is wave-uniform: the leg's record -- image pointer, frames, GainStream -- lies in DEVICE
// memory (the table rides in the call's one transfer in) and is read through scalar loads.  W is the mixer's resident
// copy: its transpose, rows of w_pitch floats (n_buses rounded up to 8, so that a group's weights of a leg are aligned
// pairs and quads), zeros behind n_buses.  A leg that has ended, an empty slot and a refused leg supply +0.0f and are
// summed like any other: a term is never skipped.  Sample indices are 64 bits, a lane's offset into its tile 32.  No matrix instruction: the rule fixes one fp64
// rounding per add in ascending order.
#include <hip/hip_runtime.h>

#include "bus.h"
#include "gain.h"
#include "kernels.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(bus_legs)

namespace {

constexpr uint32_t kLanes = 256, kWaves = kLanes / 64, kPer = 2, kTile = 64 * kPer;
constexpr uint32_t kLegBlock = 16, kLegsPerWave = kLegBlock / kWaves;
constexpr uint32_t kWgBuses = kBusGroup * kWaves;
static_assert(kLegBlock % kWaves == 0, "a block's legs are dealt to the waves in whole rounds");

// samples of a leg in the tile that begins at sample tile0 (0: the leg has ended before it, or supplies nothing at all)
__device__ __forceinline__ uint32_t samples_left(const BusLeg &leg, uint32_t channels, uint64_t tile0) {
  const uint64_t n = static_cast<uint64_t>(leg.frames) * channels;
  return tile0 >= n ? 0u : static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), n - tile0));
}

// the lane's two samples of a leg in that tile as they lie in its image, +0.0f from the leg's end on
__device__ __forceinline__ void load_samples(const BusLeg &leg, uint32_t left, uint64_t tile0, uint32_t i0, float (&e)[kPer]) {
#pragma unroll
  for (uint32_t k = 0; k < kPer; k++) e[k] = 0.0f;
  if (left == 0) return;
  // (a pointer read from memory is a generic one to the compiler: the images are global memory, and said to be here, so
  //  that the loads count against the vector-memory counter alone and not against the LDS reads' as well)
  typedef const __attribute__((address_space(1))) float *GlobalFloats;
  typedef float Pair __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) Pair *GlobalPairs;
  const GlobalFloats src = (GlobalFloats)(leg.src + tile0);
  if (left == kTile && (reinterpret_cast<uintptr_t>(leg.src + tile0) & 7u) == 0) {
    const Pair v = *(GlobalPairs)(src + i0);
    e[0] = v.x, e[1] = v.y;
  } else {
    // (a tail, or an image off the load's alignment: every lane reads inside the leg -- its last sample at the furthest --
    //  and keeps what is its own)
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const float v = src[min(i0 + k, left - 1)];
      e[k] = i0 + k < left ? v : 0.0f;
    }
  }
}

// ... multiplied by the leg's gain
__device__ __forceinline__ void gain_samples(const BusLeg &leg, uint32_t left, uint64_t tile0, uint32_t i0, float (&e)[kPer]) {
  const gain::Tile gt = gain::tile_of(leg.gain, true);
  if (gt.mode == gain::kOff || left == 0) return;
  gain::apply_group<kPer>(gt, gain::split_of(gt, tile0), i0, e);
  // (a sample behind the leg's end is +0.0f, not its product with g)
#pragma unroll
  for (uint32_t k = 0; k < kPer; k++)
    if (i0 + k >= left) e[k] = 0.0f;
}

// tile blockIdx.x of the buses [blockIdx.y * kWgBuses, + kWgBuses): wave w of the workgroup sums eight of them
__global__ __launch_bounds__(kLanes) void bus_sum_legs(const BusLegsArgs a) {
  __shared__ float stage[kLegBlock][kTile];
  __shared__ __attribute__((aligned(16))) float wstage[kLegBlock][kWgBuses];  // the block's weights of the workgroup's buses
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint64_t total = static_cast<uint64_t>(a.bus_frames) * a.channels;
  if (tile0 >= total) return;  // (the whole workgroup: no barrier is left waiting)
  // (the wave's number as a scalar: what it selects -- legs to fetch, weights to read -- stays in scalar registers)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, i0 = lane * kPer;
  const uint32_t j0 = blockIdx.y * kWgBuses + wave * kBusGroup;
  const uint32_t nb = j0 < a.n_buses ? min(kBusGroup, a.n_buses - j0) : 0u;  // (a ragged last group leaves waves without a bus)
  const uint32_t n_legs = a.n_legs;
  const BusLeg *__restrict__ legs = a.legs;
  // the lane's share of a block's weights: two of its 16 x 32, leg wl of the block, buses wc and wc + 1 of the group
  const uint32_t wl = threadIdx.x / (kWgBuses / 2), wc = (threadIdx.x % (kWgBuses / 2)) * 2;
  const uint32_t wcol = blockIdx.y * kWgBuses + wc;  // (a row ends at w_pitch, a multiple of 8: an even column's pair lies inside or outside it whole)
  typedef float Pair __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) Pair *GlobalPairs;
  double acc[kBusGroup][kPer];
#pragma unroll
  for (uint32_t b = 0; b < kBusGroup; b++)
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) acc[b][k] = 0.0;
  float next[kLegsPerWave][kPer];
  Pair wnext;
  // the wave's legs of the block that begins at leg b0, as they lie in their images: block slot wave + r * kWaves
  const auto fetch = [&](uint32_t b0) {
#pragma unroll
    for (uint32_t r = 0; r < kLegsPerWave; r++) {
      const uint32_t s = b0 + wave + r * kWaves;
      next[r][0] = next[r][1] = 0.0f;
      if (s < n_legs) load_samples(legs[s], samples_left(legs[s], a.channels, tile0), tile0, i0, next[r]);
    }
    wnext = Pair{0.0f, 0.0f};
    if (b0 + wl < n_legs && wcol < a.w_pitch) wnext = *(GlobalPairs)(a.w + static_cast<size_t>(b0 + wl) * a.w_pitch + wcol);
  };
  fetch(0);
  for (uint32_t b0 = 0; b0 < n_legs; b0 += kLegBlock) {
    const uint32_t cnt = min(kLegBlock, n_legs - b0);
    __syncthreads();  // (every wave has summed the block before: its tiles may go)
#pragma unroll
    for (uint32_t r = 0; r < kLegsPerWave; r++) {
      const uint32_t slot = wave + r * kWaves, s = b0 + slot;
      if (s < n_legs) {
        gain_samples(legs[s], samples_left(legs[s], a.channels, tile0), tile0, i0, next[r]);
        *reinterpret_cast<float2 *>(&stage[slot][i0]) = make_float2(next[r][0], next[r][1]);
      }
    }
    *reinterpret_cast<float2 *>(&wstage[wl][wc]) = make_float2(wnext.x, wnext.y);
    __syncthreads();
    if (b0 + kLegBlock < n_legs) fetch(b0 + kLegBlock);  // (in flight while this block is summed)
    if (nb == 0) continue;
#pragma unroll 4
    for (uint32_t l = 0; l < cnt; l++) {
      const uint32_t s = b0 + l;
      const float2 v = *reinterpret_cast<const float2 *>(&stage[l][i0]);
      const float e[kPer] = {v.x, v.y};
      // (the wave's eight weights of the leg: one address for all lanes, which the LDS broadcasts)
      const float4 wa = *reinterpret_cast<const float4 *>(&wstage[l][wave * kBusGroup]);
      const float4 wb = *reinterpret_cast<const float4 *>(&wstage[l][wave * kBusGroup + 4]);
      const float ws[kBusGroup] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
      if (s == 0) {
        // (the first term is the product itself, not 0 + the product: a sum of negative zeros stays -0.0f)
#pragma unroll
        for (uint32_t b = 0; b < kBusGroup; b++)
#pragma unroll
          for (uint32_t k = 0; k < kPer; k++) acc[b][k] = bus::first(ws[b], e[k]);
      } else {
#pragma unroll
        for (uint32_t b = 0; b < kBusGroup; b++)
#pragma unroll
          for (uint32_t k = 0; k < kPer; k++) acc[b][k] = bus::add(acc[b][k], ws[b], e[k]);
      }
    }
  }
  const uint32_t left = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), total - tile0));
#pragma unroll
  for (uint32_t b = 0; b < kBusGroup; b++) {
    if (b < nb) {
      float *dst = a.dst + (j0 + b) * a.dst_pitch + tile0;
      if (left == kTile && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0) {
        *reinterpret_cast<float2 *>(dst + i0) = make_float2(bus::finish(acc[b][0]), bus::finish(acc[b][1]));
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++)
          if (i0 + k < left) dst[i0 + k] = bus::finish(acc[b][k]);
      }
    }
  }
}

}  // namespace

hipError_t launch_bus_sum_legs(const BusLegsArgs &a, const BusLeg *host_legs, hipStream_t stream) {
  if (a.bus_frames == 0) return hipSuccess;
  if (a.n_legs == 0 || a.n_legs > kBusMaxLegs || a.n_buses == 0 || a.n_buses > kBusMaxBuses || a.channels == 0 ||
      a.legs == nullptr || host_legs == nullptr || a.dst == nullptr || a.w == nullptr)
    return hipErrorInvalidValue;
  if (a.w_pitch < a.n_buses || a.w_pitch % kBusGroup != 0) return hipErrorInvalidValue;  // (a group's weights: one aligned load)
  const uint64_t total = static_cast<uint64_t>(a.bus_frames) * a.channels;
  if (a.n_buses > 1 && a.dst_pitch < total) return hipErrorInvalidValue;  // (the buses would overlap)
  for (uint32_t s = 0; s < a.n_legs; s++) {
    const BusLeg &leg = host_legs[s];
    if (leg.frames > a.bus_frames || (leg.frames != 0 && leg.src == nullptr) ||
        (leg.gain.channels != 0 && leg.gain.channels != a.channels))
      return hipErrorInvalidValue;
  }
  const uint64_t tiles = (total + kTile - 1) / kTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(tiles), (a.n_buses + kWgBuses - 1) / kWgBuses), block(kLanes);
  hipLaunchKernelGGL(bus_sum_legs, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace speexhip
