// kernels_mix.hip -- the channel mix of a mixed call (engine.h, process_sides_device), folded into the pass that converts a
// side anyway: mix_in<F> reads storage of format F with src_channels per frame and writes the float image the FIR
// kernels read with dst_channels per frame; mix_out<F> reads the image they wrote and stores format F.  Per frame:
// to_internal, the matrix, from_internal (format_device.h).  A side with a matrix runs this INSTEAD of convert_*.
//
// One frame (include/speexhip_resampler.h): output o = M[o][0] * x[0], then + M[o][i] * x[i] for i = 1 .. n-1 in that
// order, all in fp64 -- a product of two fp32 values is exact there, so fma(M, x, acc) gives the bits of a multiply and
// an add -- then one rounding to fp32.  Every term is included; nothing is clamped on the image.
//
// Grid = (tile, stream); the streams' arguments and the matrix (MixPack) travel in the kernel-argument segment, so the
// channel counts and the coefficients are wave-uniform (scalar loads); one instance per format, none per shape.  A tile
// is 512 frames: 256 lanes x 2.
//
// Tile path (mix_in only; whole tiles; storage and image 16-byte aligned -- decided per workgroup from the stream's
// arguments): every global access is 16 bytes per lane.  With runtime channel counts a lane cannot own whole 16-byte
// pieces of both sides in registers, so the workgroup copies its tile's raw storage bytes into LDS piece by piece, lane t
// then mixes frames t and t + 256 out of LDS into a second LDS area laid out as the image, and the workgroup copies that
// out piece by piece.  512 frames are whole pieces on both sides for every shape and format.  Big-endian s16 and s32 are
// reversed per dword on their way into LDS (format_device.h, swap_words) and are their little-endian twins from there.
// LDS layout: both areas are the global bytes in order, with one spare dword after every 32 (dword d lives at
// d + d / 32).  A lane's frame starts frame-stride dwords after its neighbour's -- 1, 2, 4 or 8 dwords for the common
// shapes, which unpadded would put 32 lanes on 32, 16, 8 or 4 banks; with the spare dword a stride of 2^k walks all 32
// banks (stride 8: frame 4a + b -> bank 8b + a).  The copies move their 16-byte pieces as four dword accesses, which the
// padding keeps conflict-free too (piece 8a + b -> bank 4b + a + j).
//
// Element path (mix_out always; mix_in on partial tiles and at any byte address for the 1-byte formats and s24, any element-aligned one for
// the rest): frame by frame from and to global memory, consecutive lanes on consecutive frames.  Both paths run the same
// mix_frame: the same bytes.  mix_out had a tile path of the same build; measured on whole aligned tiles it was not
// faster than this one ("Mixed calls"), so it is gone: a lane's stores already fall into lines its
// neighbours fill.
//
// mix_out_dither<F> (the formats of dithered_fmt; a state with dither on): mix_out with the dither of dither.h added before
// the rounding, instances of their own beside mix_out -- the same body, kDither = true.  Output o of frame f of a stream at position p has idx
// (p + f) * dst_channels + o: a frame is a run of consecutive idx, so the inner half of the generator's word is taken
// once per frame (twice for the one frame that crosses a 2^32 boundary of idx).
//
// mix_out_meter<F> (every format; a state with the meter on): mix_out judged on its way (meter.h), behind the matrix and
// before the dither -- the dithered body for the formats of dithered_fmt (kind NONE: d = 0), the plain one for the float
// formats; the streams' cells travel in a third kernel argument.
//
// mix_out_gain<F> (every format; a state with a stream's gain on): one instance per format.  The outputs of a frame are
// multiplied by the frame's g (gain.h) behind the matrix's rounding to fp32, then judged and dithered as the stream asks,
// both at run time.  The pass walks frames: the ramp's index is tile0 + f, no division anywhere.
//
// The image mix_in writes is read by the very next kernel and mix_out's source was written by the previous one: plain
// loads and stores throughout, so that the images can stay in L2 / Infinity Cache.
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "gain.h"
#include "kernels.h"
#include "meter.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(mix)

namespace {

using namespace fmtdev;

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTileFrames = 512;  // a multiple of 16: whole 16-byte pieces of 1..8 channels of 1..4 bytes

// where dword d of an LDS area lives: one spare dword after every 32
__host__ __device__ constexpr uint32_t pad_dword(uint32_t d) { return d + (d >> 5); }
// dwords of an area that holds `dwords` of data (+ the dword past the end that an s24 read may touch)
__host__ __device__ constexpr uint32_t area_dwords(uint32_t dwords) { return pad_dword(dwords) + 2; }

// ---- one frame -----------------------------------------------------------------------------------------------------
// get(i) = source sample i as the internal float, put(o, y) takes output o; ns, nd and the coefficients are wave-uniform
template <class Get, class Put>
__device__ __forceinline__ void mix_frame(const MixPack &pack, uint32_t ns, uint32_t nd, Get get, Put put) {
  double x[kMixMaxChannels];
#pragma unroll
  for (uint32_t i = 0; i < kMixMaxChannels; i++) x[i] = i < ns ? static_cast<double>(get(i)) : 0.0;
  for (uint32_t o = 0; o < nd; o++) {
    const float *row = pack.m + o * ns;
    double acc = static_cast<double>(row[0]) * x[0];
#pragma unroll
    for (uint32_t i = 1; i < kMixMaxChannels; i++)
      if (i < ns) acc = fma(static_cast<double>(row[i]), x[i], acc);
    put(o, static_cast<float>(acc));
  }
}

// ---- 16 bytes per lane, frames out of LDS ----------------------------------------------------------------------------
// sample s of format F out of an LDS area that holds storage bytes in order
template <int F>
__device__ __forceinline__ uint32_t lds_raw(const uint32_t *area, uint32_t s) {
  constexpr uint32_t B = sample_bytes(F);
  if (B == 4) return area[pad_dword(s)];
  if (B == 2) return area[pad_dword(s >> 1)] >> ((s & 1u) * 16);
  if (B == 1) return area[pad_dword(s >> 2)] >> ((s & 3u) * 8);
  const uint32_t a = 3 * s, k = a >> 2;  // packed s24: three bytes that may span two dwords
  const uint64_t pair = area[pad_dword(k)] | (static_cast<uint64_t>(area[pad_dword(k + 1)]) << 32);
  return static_cast<uint32_t>(pair >> ((a & 3u) * 8));
}
// mix_in: frames [tile0, tile0 + kTileFrames) of the stream; src_fb / dst_fb = bytes of a frame on either side
template <int F>
__device__ __forceinline__ void tile_path(const MixPack &pack, const MixStream &s, uint64_t tile0, uint32_t ns, uint32_t nd,
                                          uint32_t src_fb, uint32_t dst_fb, uint32_t *lds) {
  constexpr int W = word_format(F);
  const uint32_t src_dwords = kTileFrames * src_fb / 4, dst_dwords = kTileFrames * dst_fb / 4;
  uint32_t *a_src = lds, *a_dst = lds + area_dwords(src_dwords);
  const uint4 *g_src = reinterpret_cast<const uint4 *>(static_cast<const char *>(s.src) + tile0 * src_fb);
  uint4 *g_dst = reinterpret_cast<uint4 *>(static_cast<char *>(s.dst) + tile0 * dst_fb);
  for (uint32_t p = threadIdx.x; p < src_dwords / 4; p += kLanes) {
    const uint4 v = g_src[p];
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    swap_words<F, 4>(w);  // (S16BE / S32BE: reversed as dwords on their way in, the samples then the twin's)
    uint32_t *at = a_src + pad_dword(4 * p);  // (a piece never straddles a spare dword)
    at[0] = w[0], at[1] = w[1], at[2] = w[2], at[3] = w[3];
  }
  __syncthreads();
  for (uint32_t f = threadIdx.x; f < kTileFrames; f += kLanes)
    mix_frame(
        pack, ns, nd, [&](uint32_t i) { return to_internal<W>(lds_raw<W>(a_src, f * ns + i)); },
        [&](uint32_t o, float y) { a_dst[pad_dword(f * nd + o)] = __float_as_uint(y); });
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < dst_dwords / 4; p += kLanes) {
    const uint32_t *at = a_dst + pad_dword(4 * p);
    g_dst[p] = make_uint4(at[0], at[1], at[2], at[3]);
  }
}

// ---- frame by frame --------------------------------------------------------------------------------------------------
// frames [tile0, tile0 + n) of the stream; kDither (kOut only): the dithered instances; d and kind are theirs alone;
// kMeter (kOut only): the metered instances, m (meter.h) is theirs alone; kGain (kOut, kMeter and kDither =
// dithered_fmt(F) only): the gained instances, gt (gain.h) is theirs alone -- the frame's g, behind the matrix's rounding
template <int F, bool kOut, bool kDither, bool kMeter, bool kGain>
__device__ __forceinline__ void element_path(const MixPack &pack, const MixStream &s, const DitherStream *d, int kind,
                                             uint64_t tile0, uint32_t n, uint32_t ns, uint32_t nd, meter::Lane &m,
                                             const gain::Tile &gt) {
  constexpr uint32_t B = sample_bytes(F);
  for (uint32_t f = threadIdx.x; f < n; f += kLanes) {
    const uint64_t frame = tile0 + f;
    if (!kOut) {
      const char *src = static_cast<const char *>(s.src) + frame * ns * B;
      float *dst = static_cast<float *>(s.dst) + frame * nd;
      mix_frame(
          pack, ns, nd, [&](uint32_t i) { return to_internal<F>(load_raw<F>(src + i * B)); },
          [&](uint32_t o, float y) { dst[o] = y; });
    } else {
      const float *src = static_cast<const float *>(s.src) + frame * ns;
      char *dst = static_cast<char *>(s.dst) + frame * nd * B;
      const dither::Run run = kDither ? dither::run_of(d->seed, (d->first + frame) * nd, nd) : dither::Run{};
      mix_frame(
          pack, ns, nd, [&](uint32_t i) { return src[i]; },
          [&](uint32_t o, float y) {
            if constexpr (kGain)
              store_raw<F>(dst + o * B, gain::encode<F>(gt, m, y, frame, [&] { return dither::noise_in(kind, run, o); }));
            else
              store_raw<F>(dst + o * B, meter::encode<F, kDither, kMeter>(m, y, [&] { return dither::noise_in(kind, run, o); }));
          });
    }
  }
}

template <int F, bool kOut, bool kDither, bool kMeter = false, bool kGain = false>
__device__ __forceinline__ void mix_tile(const MixPack &pack, const DitherPack *dith, uint32_t *lds, const MeterPack *meter = nullptr,
                                         const GainPack *gain = nullptr) {
  const MixStream &s = pack.s[blockIdx.y];
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTileFrames;
  if (s.src == nullptr || tile0 >= s.frames) return;  // (nothing to mix, or a shorter stream of the launch)
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTileFrames), s.frames - tile0));
  const uint32_t ns = pack.src_channels, nd = pack.dst_channels;
  const DitherStream *d = kDither ? &dith->s[blockIdx.y] : nullptr;
  const int kind = kDither ? dith->kind : 0;
  const bool aligned = ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 15u) == 0;
  meter::Lane m;
  MeterCell *const cell = kGain ? meter->cell[blockIdx.y] : nullptr;
  // (kGain: dither and meter at run time -- kind NONE: d = 0, no cell: nothing judged or committed)
  const gain::Tile gt = kGain ? gain::tile_of(gain->s[blockIdx.y], cell == nullptr && kind == SPEEXHIP_DITHER_NONE) : gain::Tile{};
  if (!kOut && n == kTileFrames && aligned)
    tile_path<F>(pack, s, tile0, ns, nd, ns * sample_bytes(F), nd * 4u, lds);
  else
    element_path<F, kOut, kDither, kMeter, kGain>(pack, s, d, kind, tile0, n, ns, nd, m, gt);
  // (every lane: the early return above is the workgroup's, and so is the cell)
  if constexpr (kGain) {
    if (cell != nullptr) meter::commit(m, cell);
  } else if constexpr (kMeter) {
    meter::commit(m, meter->cell[blockIdx.y]);
  }
}

template <int F>
__global__ __launch_bounds__(kLanes) void mix_in(const MixPack pack) {
  extern __shared__ uint32_t mix_lds[];
  mix_tile<F, false, false>(pack, nullptr, mix_lds);
}
template <int F>
__global__ __launch_bounds__(kLanes) void mix_out(const MixPack pack) {
  extern __shared__ uint32_t mix_lds[];
  mix_tile<F, true, false>(pack, nullptr, mix_lds);
}
template <int F>
__global__ __launch_bounds__(kLanes) void mix_out_dither(const MixPack pack, const DitherPack dith) {
  mix_tile<F, true, true>(pack, &dith, nullptr);
}
// the metered instance of a format (meter.h): the dithered body for the formats of dithered_fmt (kind NONE: d = 0), the
// plain one for the float formats
template <int F>
__global__ __launch_bounds__(kLanes) void mix_out_meter(const MixPack pack, const DitherPack dith, const MeterPack meter) {
  mix_tile<F, true, dithered_fmt(F), true>(pack, &dith, nullptr, &meter);
}
// the gained instance of a format (gain.h): every output of a frame times the frame's g, then the metered body with
// dither and meter taken at run time
template <int F>
__global__ __launch_bounds__(kLanes) void mix_out_gain(const MixPack pack, const DitherPack dith, const MeterPack meter,
                                                       const GainPack gain) {
  mix_tile<F, true, dithered_fmt(F), true, true>(pack, &dith, nullptr, &meter, &gain);
}

}  // namespace

hipError_t launch_mix(int fmt, bool out, const MixPack &pack, const DitherPack *dith, uint32_t n, uint32_t most,
                      hipStream_t stream, const MeterPack *meter, const GainPack *gain) {
  if (n == 0 || most == 0) return hipSuccess;
  if (pack.src_channels == 0 || pack.src_channels > kMixMaxChannels || pack.dst_channels == 0 ||
      pack.dst_channels > kMixMaxChannels || ((dith != nullptr || meter != nullptr || gain != nullptr) && !out))
    return hipErrorInvalidValue;
  for (uint32_t j = 0; meter != nullptr && j < n; j++)
    if (meter->cell[j] == nullptr) return hipErrorInvalidValue;
  // the two LDS areas of mix_in's tile path (at most 33.8 KB: no opt-in needed)
  const uint32_t src_fb = pack.src_channels * sample_bytes(fmt), dst_fb = pack.dst_channels * 4u;
  const uint32_t lds = out ? 0u : (area_dwords(kTileFrames * src_fb / 4) + area_dwords(kTileFrames * dst_fb / 4)) * 4;
  const dim3 grid((most + kTileFrames - 1) / kTileFrames, n), block(kLanes);
  return with_format(fmt, [&](auto format) -> hipError_t {
    constexpr int F = decltype(format)::value;
    if (gain != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      const DitherPack none = {};    // (kind NONE)
      const MeterPack no_cells = {};  // (nothing judged)
      hipLaunchKernelGGL((mix_out_gain<F>), grid, block, 0, stream, pack, dith != nullptr ? *dith : none,
                         meter != nullptr ? *meter : no_cells, *gain);
    } else if (meter != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      DitherPack none = {};  // (kind NONE)
      hipLaunchKernelGGL((mix_out_meter<F>), grid, block, 0, stream, pack, dith != nullptr ? *dith : none, *meter);
    } else if (dith == nullptr) {
      if (out)
        hipLaunchKernelGGL((mix_out<F>), grid, block, lds, stream, pack);
      else
        hipLaunchKernelGGL((mix_in<F>), grid, block, lds, stream, pack);
    } else if constexpr (dithered_fmt(F)) {
      hipLaunchKernelGGL((mix_out_dither<F>), grid, block, 0, stream, pack, *dith);
    } else {
      return hipErrorInvalidValue;  // (the float formats are not dithered)
    }
    return hipGetLastError();
  });
}

}  // namespace speexhip
