// kernels_convert.hip -- sample formats <-> the internal float image: the two passes either side of a formatted call
// (engine.h, process_sides_device).  convert_in<F> reads storage of format F (u8, s16, packed s24, s32, float in +-1.0,
// G.711 mu-law and A-law)
// and writes the float image the FIR kernels read, in the library's unit (one int16 step = 1.0f); convert_out<F> reads
// the image they wrote and stores format F, rounding half up and saturating the integer formats.  Elementwise.
//
// Grid = (tile, stream); the streams' arguments (ConvertPack) travel in the kernel-argument segment.  A tile is 4096
// samples: 256 lanes x 16.
//
// Vector path (whole tiles; storage and image 16-byte aligned; step 1 -- decided per workgroup from the stream's
// arguments, so it is wave-uniform): every access is 16 bytes per lane.  A lane owns G consecutive samples per pass --
// G = 16 for the 1-byte formats u8, mu-law and A-law (one 16-byte piece of storage, four of the image) and packed s24 (three pieces of storage, unpacked /
// packed in registers with byte shifts across dword pairs, four of the image), 8 for the 2-byte formats, 4 for the
// 4-byte ones -- and a workgroup makes 16 / G passes, lane t on group pass * 256 + t.  Big-endian s16 and s32 are
// reversed per dword (format_device.h, swap_words: two s16 samples per v_perm_b32) and then are their little-endian
// twins; a packed big-endian s24 sample is reversed on its own.
//
// Element path (any byte address for the 1-byte formats and s24, any element-aligned one for the rest; partial tiles; strided samples of
// a state whose channels stand apart): sample by sample, s24 byte by byte, consecutive lanes on consecutive samples.
//
// The image convert_in writes is read by the very next kernel and convert_out's source was written by the previous
// one: plain loads and stores throughout, so that the images can stay in L2 / Infinity Cache.
//
// The bodies of both paths -- vector_tile, element_tile and stream_tile, which picks between them -- are stated in
// kernels_convert_impl.h, shared with kernels_convert_many.hip (a format per stream of one launch); this unit holds the
// instances of one format per launch and their launcher.
//
// The formats themselves -- one sample to and from the image, rounding half up, and the loads / stores of one sample --
// are stated in format_device.h, which the mixing kernels (kernels_mix.hip) share.
//
// convert_out_dither<F> (the formats of dithered_fmt; a state with dither on): convert_out with the dither of dither.h added
// before the rounding.  Instances of their own beside convert_out -- the same body, kDither = true: the same two paths,
// the same bytes from both.  Sample k of a stream has idx first + k (DitherPack; the launcher takes step 1 only), so a
// lane's group on the vector path is a run of G consecutive idx: the inner half of the generator's word, which changes
// once per 2^32 samples, is taken once per group (twice for the one group that crosses such a boundary), once per sample
// on the element path.  The kind is one per launch: wave-uniform.
//
// convert_out_meter<F> (every format; a state with the meter on): convert_out judged on its way (meter.h) -- the dithered
// body for the formats of dithered_fmt, where kind NONE gives d = 0 and the undithered bytes, the plain body for the float
// formats.  A lane counts in registers, the workgroup folds its four waves and adds into the stream's MeterCell, whose
// address travels in a third kernel argument (MeterPack).  meter_image reads a float result that no pass writes and
// judges it the same way.  The plain and dithered instances are untouched: the meter is a compile-time flag of the body.
//
// convert_out_gain<F> (every format; a state with a stream's gain on): one instance per format.  Each sample is
// multiplied by the g of its frame (gain.h) and then leaves through the metered body, which takes dither and meter at
// run time -- kind NONE: d = 0; no cell: nothing judged or committed; neither: from_internal, the same bytes without the
// fp64 sum.  The pass walks samples, not frames: a stream past its ramp has one wave-uniform g and forms no index; in a
// ramp the tile's first sample is split into frame and channel once, in 64 bits, and a lane's offset divided in 32 -- once
// per 16-byte group on the vector path, frame and channel then walking on through the group, which may straddle frames;
// once per sample on the element path.  The stream's mode and what it asks of the encoder are branched on once per group.
// gain_image does the same in place over a float result that no pass writes.
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "kernels.h"
#include "kernels_convert_impl.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(convert)

namespace {

using namespace convert_impl;  // kLanes, kTile, stream_tile: the bodies (kernels_convert_impl.h)

template <int F, bool kOut, bool kDither>
__device__ __forceinline__ void convert_tile(const ConvertPack &pack, const DitherPack *dith) {
  stream_tile<F, kOut, kDither>(pack.s[blockIdx.y], kDither ? &dith->s[blockIdx.y] : nullptr, kDither ? dith->kind : 0);
}

template <int F>
__global__ __launch_bounds__(kLanes) void convert_in(const ConvertPack pack) {
  convert_tile<F, false, false>(pack, nullptr);
}
template <int F>
__global__ __launch_bounds__(kLanes) void convert_out(const ConvertPack pack) {
  convert_tile<F, true, false>(pack, nullptr);
}
template <int F>
__global__ __launch_bounds__(kLanes) void convert_out_dither(const ConvertPack pack, const DitherPack dith) {
  convert_tile<F, true, true>(pack, &dith);
}
// the metered instance of a format (meter.h): the dithered body for the formats of dithered_fmt (kind NONE: d = 0), the
// plain one for the float formats; the stream's cell travels in the third argument
template <int F>
__global__ __launch_bounds__(kLanes) void convert_out_meter(const ConvertPack pack, const DitherPack dith, const MeterPack meter) {
  constexpr bool kDither = dithered_fmt(F);
  stream_tile<F, true, kDither, true>(pack.s[blockIdx.y], kDither ? &dith.s[blockIdx.y] : nullptr, kDither ? dith.kind : 0,
                                      meter.cell[blockIdx.y]);
}

// the gained instance of a format (gain.h): every sample times the g of its frame, then the metered body above with
// dither and meter taken at run time
template <int F>
__global__ __launch_bounds__(kLanes) void convert_out_gain(const ConvertPack pack, const DitherPack dith, const MeterPack meter,
                                                           const GainPack gain) {
  stream_tile<F, true, dithered_fmt(F), true, true>(pack.s[blockIdx.y], &dith.s[blockIdx.y], dithered_fmt(F) ? dith.kind : 0,
                                                    meter.cell[blockIdx.y], &gain.s[blockIdx.y]);
}

// gain_image: the tile blockIdx.x of stream blockIdx.y of a float result that no pass writes, multiplied in place by the
// g of each sample's frame (gain.h); 16 bytes per lane where the tile is whole and aligned, sample by sample otherwise.
// A stream with a cell is judged on the product * scale in the same pass (meter_image's rule, without its second read).
// A stream whose gain is off is not written.
__global__ __launch_bounds__(kLanes) void gain_image(const ConvertPack pack, const GainPack gain, const MeterPack meter,
                                                     const float scale) {
  const ConvertStream &s = pack.s[blockIdx.y];
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  if (s.dst == nullptr || tile0 >= s.n) return;
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), s.n - tile0));
  float *img = static_cast<float *>(s.dst) + tile0;
  MeterCell *const cell = meter.cell[blockIdx.y];
  const gain::Tile gt = gain::tile_of(gain.s[blockIdx.y], true);
  if (gt.mode == gain::kOff && cell == nullptr) return;
  const gain::Split sp = gain::split_of(gt, tile0);
  meter::Lane m;
  const auto one = [&](float y, uint32_t i) {
    const float v = gain::apply(gt, y, gain::frame_of(gt, sp, i));
    if (cell != nullptr) meter::judge<SPEEXHIP_FMT_F32>(m, v * scale, 0.0);
    return v;
  };
  if (n == kTile && (reinterpret_cast<uintptr_t>(s.dst) & 15u) == 0) {
#pragma unroll
    for (uint32_t pass = 0; pass < kTile / (kLanes * 4); pass++) {
      const uint32_t i = (pass * kLanes + threadIdx.x) * 4;
      float4 v = reinterpret_cast<const float4 *>(img)[pass * kLanes + threadIdx.x];
      v.x = one(v.x, i), v.y = one(v.y, i + 1), v.z = one(v.z, i + 2), v.w = one(v.w, i + 3);
      if (gt.mode != gain::kOff) reinterpret_cast<float4 *>(img)[pass * kLanes + threadIdx.x] = v;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < n; i += kLanes) {
      const float v = one(img[i], i);
      if (gt.mode != gain::kOff) img[i] = v;
    }
  }
  if (cell != nullptr) meter::commit(m, cell);
}

// meter_image: the tile blockIdx.x of stream blockIdx.y of a float result, read and judged, nothing written but the cell.
// Whole 16-byte aligned tiles 16 bytes per lane (lane t on group pass * 256 + t, as convert_out<F32N> reads), the rest
// sample by sample.
__global__ __launch_bounds__(kLanes) void meter_image(const ConvertPack pack, const MeterPack meter, const float scale) {
  const ConvertStream &s = pack.s[blockIdx.y];
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  if (s.src == nullptr || tile0 >= s.n) return;
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), s.n - tile0));
  const float *src = static_cast<const float *>(s.src) + tile0;
  meter::Lane m;
  if (n == kTile && (reinterpret_cast<uintptr_t>(s.src) & 15u) == 0) {
#pragma unroll
    for (uint32_t pass = 0; pass < kTile / (kLanes * 4); pass++) {
      const float4 v = reinterpret_cast<const float4 *>(src)[pass * kLanes + threadIdx.x];
      meter::judge<SPEEXHIP_FMT_F32>(m, v.x * scale, 0.0);
      meter::judge<SPEEXHIP_FMT_F32>(m, v.y * scale, 0.0);
      meter::judge<SPEEXHIP_FMT_F32>(m, v.z * scale, 0.0);
      meter::judge<SPEEXHIP_FMT_F32>(m, v.w * scale, 0.0);
    }
  } else {
    for (uint32_t i = threadIdx.x; i < n; i += kLanes) meter::judge<SPEEXHIP_FMT_F32>(m, src[i] * scale, 0.0);
  }
  meter::commit(m, meter.cell[blockIdx.y]);
}

}  // namespace

hipError_t launch_meter_image(const ConvertPack &pack, const MeterPack &meter, float scale, uint32_t n, uint64_t most,
                              hipStream_t stream) {
  if (n == 0 || most == 0) return hipSuccess;
  if (n > kMaxPackedStreams) return hipErrorInvalidValue;
  for (uint32_t j = 0; j < n; j++)
    if (pack.s[j].src != nullptr && pack.s[j].n != 0 && (meter.cell[j] == nullptr || pack.s[j].n > most)) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((most + kTile - 1) / kTile), n), block(kLanes);
  hipLaunchKernelGGL(meter_image, grid, block, 0, stream, pack, meter, scale);
  return hipGetLastError();
}

hipError_t launch_gain_image(const ConvertPack &pack, const GainPack &gain, const MeterPack *meter, float scale, uint32_t n,
                             uint64_t most, hipStream_t stream) {
  if (n == 0 || most == 0) return hipSuccess;
  if (n > kMaxPackedStreams) return hipErrorInvalidValue;
  for (uint32_t j = 0; j < n; j++)
    if (pack.s[j].dst != nullptr && pack.s[j].n != 0 && (pack.s[j].n > most || gain.s[j].channels > 0x7fffffffu)) return hipErrorInvalidValue;
  const MeterPack none = {};
  const dim3 grid(static_cast<uint32_t>((most + kTile - 1) / kTile), n), block(kLanes);
  hipLaunchKernelGGL(gain_image, grid, block, 0, stream, pack, gain, meter != nullptr ? *meter : none, scale);
  return hipGetLastError();
}

hipError_t launch_convert(int fmt, bool out, const ConvertPack &pack, const DitherPack *dith, uint32_t n, uint64_t most,
                          hipStream_t stream, const MeterPack *meter, const GainPack *gain) {
  if (n == 0 || most == 0) return hipSuccess;
  for (uint32_t j = 0; (dith != nullptr || meter != nullptr || gain != nullptr) && j < n; j++)
    if (!out || pack.s[j].step != 1 || (meter != nullptr && meter->cell[j] == nullptr) ||
        (gain != nullptr && gain->s[j].channels > 0x7fffffffu))
      return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((most + kTile - 1) / kTile), n), block(kLanes);
  return with_format(fmt, [&](auto format) -> hipError_t {
    constexpr int F = decltype(format)::value;
    // (F32 is the image's own format: nothing to convert; the float formats are not dithered)
    if constexpr (F == SPEEXHIP_FMT_F32) {
      return hipErrorInvalidValue;
    } else if (gain != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      const DitherPack none = {};    // (kind NONE)
      const MeterPack no_cells = {};  // (nothing judged)
      hipLaunchKernelGGL((convert_out_gain<F>), grid, block, 0, stream, pack, dith != nullptr ? *dith : none,
                         meter != nullptr ? *meter : no_cells, *gain);
    } else if (meter != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      DitherPack none = {};  // (kind NONE)
      hipLaunchKernelGGL((convert_out_meter<F>), grid, block, 0, stream, pack, dith != nullptr ? *dith : none, *meter);
    } else if (dith == nullptr) {
      if (out)
        hipLaunchKernelGGL((convert_out<F>), grid, block, 0, stream, pack);
      else
        hipLaunchKernelGGL((convert_in<F>), grid, block, 0, stream, pack);
    } else if constexpr (dithered_fmt(F)) {
      hipLaunchKernelGGL((convert_out_dither<F>), grid, block, 0, stream, pack, *dith);
    } else {
      return hipErrorInvalidValue;
    }
    return hipGetLastError();
  });
}

}  // namespace speexhip
