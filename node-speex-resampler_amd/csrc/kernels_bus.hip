// kernels_bus.hip -- bus_sum: the weighted sums of a batch's streams (include/speexhip_resampler.h, "Buses"; bus.h states
// the sum), the pass of a bus call between the float call and the output pass.
//
// Shape.  The pass is bound by memory: a bus sample costs n_streams fp64 FMAs, a stream sample is four bytes.  A workgroup
// of 256 lanes takes one tile of 1024 consecutive samples -- four per lane, one 16-byte load per lane and stream where the
// tile is whole and the image aligned -- and one GROUP of up to kBusGroup = 8 buses: 8 x 4 fp64 accumulators are 64 VGPRs
// beside the four loaded samples, and all 32 buses at once would be 256 and spill.  The groups are the grid's y: the
// workgroups of one tile read the same stream samples, the first from HBM, the others from L2, and multiply them by the
// streams' gains again (one fp32 product a sample; a ramp's g once per frame) -- cheaper than a barrier and 128 KiB of LDS
// a tile.  The loop over the streams is wave-uniform, and so is everything it selects by: the stream's pointer, length
// and gain mode from the kernel arguments, the weights from the device copy of W through scalar loads.  A stream that
// ends inside the tile, or before it, supplies +0.0f and is summed like any other: a term is never skipped.  Sample
// indices are 64 bits (frames x channels passes 2^32), a lane's offset into its tile 32.
#include <hip/hip_runtime.h>

#include "bus.h"
#include "gain.h"
#include "kernels.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(bus)

namespace {

constexpr uint32_t kLanes = 256, kPer = 4, kTile = kLanes * kPer;

// samples of stream s in the tile that begins at sample tile0 (0: the stream has ended before it)
__device__ __forceinline__ uint32_t samples_left(const BusPack &pack, uint32_t s, uint64_t tile0) {
  const uint64_t n = static_cast<uint64_t>(pack.frames[s]) * pack.channels;
  return tile0 >= n ? 0u : static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), n - tile0));
}

// the lane's four samples of stream s in that tile as they lie in the image, +0.0f from the stream's end on
__device__ __forceinline__ void load_samples(const BusPack &pack, uint32_t s, uint64_t tile0, float (&e)[kPer]) {
#pragma unroll
  for (uint32_t k = 0; k < kPer; k++) e[k] = 0.0f;
  const uint32_t left = samples_left(pack, s, tile0);
  if (left == 0) return;
  const float *src = pack.src[s] + tile0;
  const uint32_t i0 = threadIdx.x * kPer;
  if (left == kTile && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    const float4 v = reinterpret_cast<const float4 *>(src)[threadIdx.x];
    e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
  } else {
    // (a tail, or an image off 16-byte alignment: every lane reads inside the stream -- its last sample at the furthest --
    //  and keeps what is its own)
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const float v = src[min(i0 + k, left - 1)];
      e[k] = i0 + k < left ? v : 0.0f;
    }
  }
}

// ... multiplied by the stream's gain
__device__ __forceinline__ void gain_samples(const BusPack &pack, const GainPack &gain, uint32_t s, uint64_t tile0,
                                             float (&e)[kPer]) {
  const gain::Tile gt = gain::tile_of(gain.s[s], true);
  const uint32_t left = samples_left(pack, s, tile0);
  if (gt.mode == gain::kOff || left == 0) return;
  const uint32_t i0 = threadIdx.x * kPer;
  gain::apply_group<kPer>(gt, gain::split_of(gt, tile0), i0, e);
  // (a sample behind the stream's end is +0.0f, not its product with g)
#pragma unroll
  for (uint32_t k = 0; k < kPer; k++)
    if (i0 + k >= left) e[k] = 0.0f;
}

// tile blockIdx.x of the buses [blockIdx.y * kBusGroup, + kBusGroup)
__global__ __launch_bounds__(kLanes) void bus_sum(const BusPack pack, const GainPack gain) {
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint64_t total = static_cast<uint64_t>(pack.bus_frames) * pack.channels;
  if (tile0 >= total) return;
  const uint32_t j0 = blockIdx.y * kBusGroup;
  const uint32_t nb = min(kBusGroup, pack.n_buses - j0);
  const uint32_t n_streams = pack.n_streams;
  // (the device copy of W is its transpose, rows of kMaxBuses floats, zeros behind n_buses: the group's eight weights of
  //  a stream are one aligned 32-byte scalar load)
  const float *w = pack.w + j0;
  double acc[kBusGroup][kPer];
  float e[kPer];
  load_samples(pack, 0, tile0, e);
  gain_samples(pack, gain, 0, tile0, e);
#pragma unroll
  for (uint32_t b = 0; b < kBusGroup; b++) {
    const float wb = w[b];
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) acc[b][k] = bus::first(wb, e[k]);
  }
  for (uint32_t s = 1; s < n_streams; s++) {
    load_samples(pack, s, tile0, e);
    gain_samples(pack, gain, s, tile0, e);
    float ws[kBusGroup];
#pragma unroll
    for (uint32_t b = 0; b < kBusGroup; b++) ws[b] = w[s * bus::kMaxBuses + b];
#pragma unroll
    for (uint32_t b = 0; b < kBusGroup; b++) {
      if (b < nb) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++) acc[b][k] = bus::add(acc[b][k], ws[b], e[k]);
      }
    }
  }
  const uint32_t left = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), total - tile0));
  const uint32_t i0 = threadIdx.x * kPer;
#pragma unroll
  for (uint32_t b = 0; b < kBusGroup; b++) {
    if (b < nb) {
      float *dst = pack.dst + (j0 + b) * pack.dst_pitch + tile0;
      if (left == kTile && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        reinterpret_cast<float4 *>(dst)[threadIdx.x] =
            make_float4(bus::finish(acc[b][0]), bus::finish(acc[b][1]), bus::finish(acc[b][2]), bus::finish(acc[b][3]));
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++)
          if (i0 + k < left) dst[i0 + k] = bus::finish(acc[b][k]);
      }
    }
  }
}

}  // namespace

hipError_t launch_bus_sum(const BusPack &pack, const GainPack &gain, hipStream_t stream) {
  if (pack.bus_frames == 0) return hipSuccess;
  if (pack.n_streams == 0 || pack.n_streams > bus::kMaxStreams || pack.n_buses == 0 || pack.n_buses > bus::kMaxBuses ||
      pack.channels == 0 || pack.dst == nullptr || pack.w == nullptr)
    return hipErrorInvalidValue;
  const uint64_t total = static_cast<uint64_t>(pack.bus_frames) * pack.channels;
  if (pack.n_buses > 1 && pack.dst_pitch < total) return hipErrorInvalidValue;  // (the buses would overlap)
  for (uint32_t s = 0; s < pack.n_streams; s++)
    if (pack.frames[s] > pack.bus_frames || (pack.frames[s] != 0 && pack.src[s] == nullptr) ||
        (gain.s[s].channels != 0 && gain.s[s].channels != pack.channels))
      return hipErrorInvalidValue;
  const uint64_t tiles = (total + kTile - 1) / kTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(tiles), (pack.n_buses + kBusGroup - 1) / kBusGroup), block(kLanes);
  hipLaunchKernelGGL(bus_sum, grid, block, 0, stream, pack, gain);
  return hipGetLastError();
}

}  // namespace speexhip
