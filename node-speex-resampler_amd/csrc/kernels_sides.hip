// kernels_sides.hip -- the pass of a planar side of a formatted or mixed call (engine.h, process_sides_device):
// planes_in<F> reads the C storage planes of a stream in format F and writes the interleaved float image the FIR kernels
// read; planes_out<F> reads the image they wrote and stores planes of format F; planes_out_dither<F> is planes_out with
// the dither of dither.h.  Conversion, the side's channel matrix (PlanePack::mixed) and the dither happen in the pass
// that transposes: a planar side costs one launch per <= 32 streams, like an interleaved one.  Per sample the statements
// are the interleaved passes' own (format_device.h, dither.h, g711.h; mix_frame in kernels_mix.hip's order: fp64,
// ascending, every term, one rounding), so the bytes are theirs, transposed.
//
// Grid = (tile, stream); the streams' arguments and the matrix (PlanePack) travel in the kernel-argument segment, so
// channel counts and coefficients are wave-uniform.  A tile is kSidesTileFrames = 1024 frames of every plane.
//
// Vector path (whole tiles; plane base, plane stride in bytes and the image 16-byte aligned; at most 8 planes; image
// frames as wide as the pass's channels -- decided per workgroup from the stream's arguments, so it is wave-uniform):
// a plane is contiguous along frames, so a work item is one 16-byte piece of one plane (three pieces of packed s24): G
// consecutive frames of a channel, G = 16 for the 1-byte formats and both s24, 8 for the 2-byte formats, 4 for the 4-byte ones.  The items
// of a tile (planes x 1024 / G) go round the 256 lanes, consecutive lanes on consecutive pieces of a plane.  Between
// the plane side and the image side the tile lives in LDS as floats, frame-major with the storage side's channel count
// per frame -- without a matrix that IS the tile of the image, which then moves between LDS and global memory linearly,
// 16 bytes per lane.  With a matrix lane t mixes frames t, t + 256, ... between LDS and the image directly, a frame's
// samples in one run per lane (kernels_mix.hip's element path, measured there to be no slower than an LDS tile).
// Big-endian s16 and s32 pieces are reversed per dword (format_device.h, swap_words) next to their load or store.
// planes_in:  plane pieces -> to_internal -> LDS | LDS -> (matrix) -> image
// planes_out: image -> (matrix) -> LDS          | LDS -> encode (+ dither) -> plane pieces
// LDS layout as in kernels_mix.hip: dword d lives at d + d / 32, so the lane stride of the plane side's accesses (G x
// channels dwords, a power of two for the common shapes) walks all banks, and a 16-byte piece of the linear copy never
// straddles a spare dword.
//
// Element path (partial tiles, planes at any element-aligned address or stride, more than 8 planes, one channel of a
// state whose channels stand apart): lane t on frames t, t + 256, ...: consecutive lanes on consecutive samples of each
// plane, a frame's samples of the image in one run per lane.  No LDS.  The same statements: the same bytes.
//
// Dither: output c of frame f of a stream at position p has idx (p + f) * planes + c, as in the interleaved passes.
//
// planes_out_meter<F> (every format; a state with the meter on): planes_out judged on its way (meter.h), on both paths --
// the dithered body for the formats of dithered_fmt (kind NONE: d = 0), the plain one for the float formats.  The samples
// and their d are the interleaved pass's, so the totals are too.
//
// planes_out_gain<F> (every format; a state with a stream's gain on): one instance per format, on both paths.  The
// outputs of a frame are multiplied by the frame's g (gain.h) behind the matrix's rounding, then judged and dithered as
// the stream asks, both at run time.  The pass walks frames: no division.
//
// The image planes_in writes is read by the very next kernel and planes_out's source was written by the previous one:
// plain loads and stores throughout, so that the images can stay in L2 / Infinity Cache.
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "gain.h"
#include "kernels.h"
#include "meter.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(sides)

namespace {

using namespace fmtdev;

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTile = kSidesTileFrames;

// frames of a plane in a work item of the vector path: whole 16-byte pieces
constexpr uint32_t group_of(int f) { return sample_bytes(f) == 1 || sample_bytes(f) == 3 ? 16u : sample_bytes(f) == 2 ? 8u : 4u; }

// where dword d of the LDS tile lives: one spare dword after every 32
__host__ __device__ constexpr uint32_t pad_dword(uint32_t d) { return d + (d >> 5); }
__host__ __device__ constexpr uint32_t area_dwords(uint32_t dwords) { return pad_dword(dwords) + 2; }

// sample j (compile-time) of an item's group, from / into the group's storage words (as in kernels_convert.hip)
template <int F>
__device__ __forceinline__ uint32_t raw_of(const uint32_t *w, uint32_t j) {
  constexpr uint32_t bits = 8 * sample_bytes(F), words = group_of(F) * sample_bytes(F) / 4;
  const uint32_t k = j * bits / 32, shift = j * bits % 32;
  const uint64_t pair = w[k] | (static_cast<uint64_t>(k + 1 < words ? w[k + 1] : 0u) << 32);
  return static_cast<uint32_t>(pair >> shift);
}
template <int F>
__device__ __forceinline__ void put_raw(uint32_t *w, uint32_t j, uint32_t raw) {
  constexpr uint32_t bits = 8 * sample_bytes(F), words = group_of(F) * sample_bytes(F) / 4;
  const uint32_t k = j * bits / 32, shift = j * bits % 32;
  const uint64_t pair = static_cast<uint64_t>(bits == 32 ? raw : raw & ((1u << (bits & 31)) - 1u)) << shift;
  w[k] |= static_cast<uint32_t>(pair);
  if (k + 1 < words) w[k + 1] |= static_cast<uint32_t>(pair >> 32);
}

// one frame through the matrix m (row-major nd x ns), kernels_mix.hip's mix_frame: output o = m[o][0] * x[0], then
// + m[o][i] * x[i] for i = 1 .. ns-1 in that order, all in fp64, then one rounding to fp32
template <class Get, class Put>
__device__ __forceinline__ void mix_frame(const float *m, uint32_t ns, uint32_t nd, Get get, Put put) {
  double x[kMixMaxChannels];
#pragma unroll
  for (uint32_t i = 0; i < kMixMaxChannels; i++) x[i] = i < ns ? static_cast<double>(get(i)) : 0.0;
  for (uint32_t o = 0; o < nd; o++) {
    const float *row = m + o * ns;
    double acc = static_cast<double>(row[0]) * x[0];
#pragma unroll
    for (uint32_t i = 1; i < kMixMaxChannels; i++)
      if (i < ns) acc = fma(static_cast<double>(row[i]), x[i], acc);
    put(o, static_cast<float>(acc));
  }
}

// ---- 16 bytes per lane on the plane side -----------------------------------------------------------------------------
// frames [tile0, tile0 + kTile) of the stream, planes -> image
template <int F>
__device__ __forceinline__ void vector_in(const PlanePack &pack, const PlaneStream &s, uint64_t tile0, uint32_t *lds) {
  constexpr uint32_t B = sample_bytes(F), G = group_of(F), words = G * B / 4, pieces = kTile / G;
  constexpr int W = word_format(F);
  const uint32_t sc = pack.storage_channels, ic = pack.image_channels;
  const char *planes = static_cast<const char *>(s.src);
  for (uint32_t item = threadIdx.x; item < sc * pieces; item += kLanes) {
    const uint32_t c = item / pieces, f0 = (item % pieces) * G;  // the item's plane and its first frame of the tile
    const uint4 *in = reinterpret_cast<const uint4 *>(planes + (c * s.plane_stride + tile0 + f0) * B);
    uint32_t w[words];
#pragma unroll
    for (uint32_t i = 0; i < words / 4; i++) {
      const uint4 v = in[i];
      w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
    }
    swap_words<F, words>(w);  // (S16BE / S32BE: reversed as dwords, the samples then the little-endian twin's)
#pragma unroll
    for (uint32_t j = 0; j < G; j++) lds[pad_dword((f0 + j) * sc + c)] = __float_as_uint(to_internal<W>(raw_of<W>(w, j)));
  }
  __syncthreads();
  float *image = static_cast<float *>(s.dst) + tile0 * ic;
  if (pack.mixed == 0) {  // (sc == ic: the LDS tile is the image's)
    uint4 *g = reinterpret_cast<uint4 *>(image);
    for (uint32_t p = threadIdx.x; p < kTile * sc / 4; p += kLanes) {
      const uint32_t *at = lds + pad_dword(4 * p);
      g[p] = make_uint4(at[0], at[1], at[2], at[3]);
    }
  } else {
    for (uint32_t f = threadIdx.x; f < kTile; f += kLanes)
      mix_frame(
          pack.m, sc, ic, [&](uint32_t i) { return __uint_as_float(lds[pad_dword(f * sc + i)]); },
          [&](uint32_t o, float y) { image[static_cast<size_t>(f) * ic + o] = y; });
  }
}

// ... image -> planes; kDither: the dithered instances, d and kind are theirs alone; kMeter: the metered instances, m
// (meter.h) is theirs alone; kGain (kMeter and kDither = dithered_fmt(F) only): the gained instances, gt (gain.h) is
// theirs alone -- the frame's g, behind the matrix's rounding
template <int F, bool kDither, bool kMeter, bool kGain>
__device__ __forceinline__ void vector_out(const PlanePack &pack, const PlaneStream &s, const DitherStream *d, int kind,
                                           uint64_t tile0, uint32_t *lds, meter::Lane &m, const gain::Tile &gt) {
  constexpr uint32_t B = sample_bytes(F), G = group_of(F), words = G * B / 4, pieces = kTile / G;
  constexpr int W = word_format(F);
  const uint32_t sc = pack.storage_channels, ic = pack.image_channels;
  const float *image = static_cast<const float *>(s.src) + tile0 * ic;
  if (pack.mixed == 0) {
    const uint4 *g = reinterpret_cast<const uint4 *>(image);
    for (uint32_t p = threadIdx.x; p < kTile * sc / 4; p += kLanes) {
      const uint4 v = g[p];
      uint32_t *at = lds + pad_dword(4 * p);
      at[0] = v.x, at[1] = v.y, at[2] = v.z, at[3] = v.w;
    }
  } else {
    for (uint32_t f = threadIdx.x; f < kTile; f += kLanes)
      mix_frame(
          pack.m, ic, sc, [&](uint32_t i) { return image[static_cast<size_t>(f) * ic + i]; },
          [&](uint32_t o, float y) { lds[pad_dword(f * sc + o)] = __float_as_uint(y); });
  }
  __syncthreads();
  char *planes = static_cast<char *>(s.dst);
  for (uint32_t item = threadIdx.x; item < sc * pieces; item += kLanes) {
    const uint32_t c = item / pieces, f0 = (item % pieces) * G;
    uint32_t w[words];
#pragma unroll
    for (uint32_t i = 0; i < words; i++) w[i] = 0;
#pragma unroll
    for (uint32_t j = 0; j < G; j++) {
      const float y = __uint_as_float(lds[pad_dword((f0 + j) * sc + c)]);
      if constexpr (kGain)
        put_raw<W>(w, j, gain::encode<W>(gt, m, y, tile0 + f0 + j, [&] { return dither::noise(kind, d->seed, (d->first + tile0 + f0 + j) * sc + c); }));
      else
        put_raw<W>(w, j, meter::encode<W, kDither, kMeter>(m, y, [&] { return dither::noise(kind, d->seed, (d->first + tile0 + f0 + j) * sc + c); }));
    }
    swap_words<F, words>(w);
    uint4 *out = reinterpret_cast<uint4 *>(planes + (c * s.plane_stride + tile0 + f0) * B);
#pragma unroll
    for (uint32_t i = 0; i < words / 4; i++) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  }
}

// ---- frame by frame --------------------------------------------------------------------------------------------------
// frames [tile0, tile0 + n) of the stream
template <int F, bool kOut, bool kDither, bool kMeter, bool kGain>
__device__ __forceinline__ void element_path(const PlanePack &pack, const PlaneStream &s, const DitherStream *d, int kind,
                                             uint64_t tile0, uint32_t n, meter::Lane &m, const gain::Tile &gt) {
  constexpr uint32_t B = sample_bytes(F);
  const uint32_t sc = pack.storage_channels, ic = pack.image_channels;
  const uint64_t plane_bytes = s.plane_stride * B;
  for (uint32_t f = threadIdx.x; f < n; f += kLanes) {
    const uint64_t frame = tile0 + f;
    if (!kOut) {
      const char *src = static_cast<const char *>(s.src) + frame * B;  // the frame's sample of plane 0
      float *dst = static_cast<float *>(s.dst) + frame * pack.image_pitch;
      const auto get = [&](uint32_t i) { return to_internal<F>(load_raw<F>(src + i * plane_bytes)); };
      if (pack.mixed == 0)
        for (uint32_t c = 0; c < sc; c++) dst[c] = get(c);
      else
        mix_frame(pack.m, sc, ic, get, [&](uint32_t o, float y) { dst[o] = y; });
    } else {
      const float *src = static_cast<const float *>(s.src) + frame * pack.image_pitch;
      char *dst = static_cast<char *>(s.dst) + frame * B;
      const dither::Run run = kDither ? dither::run_of(d->seed, (d->first + frame) * sc, sc) : dither::Run{};
      const auto put = [&](uint32_t o, float y) {
        if constexpr (kGain)
          store_raw<F>(dst + o * plane_bytes, gain::encode<F>(gt, m, y, frame, [&] { return dither::noise_in(kind, run, o); }));
        else
          store_raw<F>(dst + o * plane_bytes, meter::encode<F, kDither, kMeter>(m, y, [&] { return dither::noise_in(kind, run, o); }));
      };
      if (pack.mixed == 0)
        for (uint32_t c = 0; c < sc; c++) put(c, src[c]);
      else
        mix_frame(pack.m, ic, sc, [&](uint32_t i) { return src[i]; }, put);
    }
  }
}

template <int F, bool kOut, bool kDither, bool kMeter = false, bool kGain = false>
__device__ __forceinline__ void planes_tile(const PlanePack &pack, const DitherPack *dith, uint32_t *lds, const MeterPack *meter = nullptr,
                                            const GainPack *gain = nullptr) {
  const PlaneStream &s = pack.s[blockIdx.y];
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  if (s.src == nullptr || tile0 >= s.frames) return;  // (nothing to move, or a shorter stream of the launch)
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), s.frames - tile0));
  const DitherStream *d = kDither ? &dith->s[blockIdx.y] : nullptr;
  const int kind = kDither ? dith->kind : 0;
  const bool aligned = ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) |
                         (s.plane_stride * sample_bytes(F))) & 15u) == 0;
  const bool tiled = pack.storage_channels <= kMixMaxChannels && pack.image_channels <= kMixMaxChannels &&
                     pack.image_pitch == pack.image_channels;
  meter::Lane m;
  // (kGain: dither and meter at run time -- kind NONE: d = 0, no cell: nothing judged or committed)
  MeterCell *const cell = kGain ? meter->cell[blockIdx.y] : nullptr;
  const gain::Tile gt = kGain ? gain::tile_of(gain->s[blockIdx.y], cell == nullptr && kind == SPEEXHIP_DITHER_NONE) : gain::Tile{};
  if (n == kTile && aligned && tiled) {
    if (kOut)
      vector_out<F, kDither, kMeter, kGain>(pack, s, d, kind, tile0, lds, m, gt);
    else
      vector_in<F>(pack, s, tile0, lds);
  } else {
    element_path<F, kOut, kDither, kMeter, kGain>(pack, s, d, kind, tile0, n, m, gt);
  }
  // (every lane: the early return above is the workgroup's, and so is the cell)
  if constexpr (kGain) {
    if (cell != nullptr) meter::commit(m, cell);
  } else if constexpr (kMeter) {
    meter::commit(m, meter->cell[blockIdx.y]);
  }
}

template <int F>
__global__ __launch_bounds__(kLanes) void planes_in(const PlanePack pack) {
  extern __shared__ uint32_t sides_lds[];
  planes_tile<F, false, false>(pack, nullptr, sides_lds);
}
template <int F>
__global__ __launch_bounds__(kLanes) void planes_out(const PlanePack pack) {
  extern __shared__ uint32_t sides_lds[];
  planes_tile<F, true, false>(pack, nullptr, sides_lds);
}
template <int F>
__global__ __launch_bounds__(kLanes) void planes_out_dither(const PlanePack pack, const DitherPack dith) {
  extern __shared__ uint32_t sides_lds[];
  planes_tile<F, true, true>(pack, &dith, sides_lds);
}
// the metered instance of a format (meter.h): the dithered body for the formats of dithered_fmt (kind NONE: d = 0), the
// plain one for the float formats
template <int F>
__global__ __launch_bounds__(kLanes) void planes_out_meter(const PlanePack pack, const DitherPack dith, const MeterPack meter) {
  extern __shared__ uint32_t sides_lds[];
  planes_tile<F, true, dithered_fmt(F), true>(pack, &dith, sides_lds, &meter);
}
// the gained instance of a format (gain.h): every output of a frame times the frame's g, then the metered body with
// dither and meter taken at run time
template <int F>
__global__ __launch_bounds__(kLanes) void planes_out_gain(const PlanePack pack, const DitherPack dith, const MeterPack meter,
                                                          const GainPack gain) {
  extern __shared__ uint32_t sides_lds[];
  planes_tile<F, true, dithered_fmt(F), true, true>(pack, &dith, sides_lds, &meter, &gain);
}

}  // namespace

hipError_t launch_planes(int fmt, bool out, const PlanePack &pack, const DitherPack *dith, uint32_t n, uint32_t most,
                         hipStream_t stream, const MeterPack *meter, const GainPack *gain) {
  if (n == 0 || most == 0) return hipSuccess;
  const uint32_t sc = pack.storage_channels, ic = pack.image_channels;
  if (sc == 0 || ic == 0 || pack.image_pitch < ic || ((dith != nullptr || meter != nullptr || gain != nullptr) && !out)) return hipErrorInvalidValue;
  for (uint32_t j = 0; meter != nullptr && j < n; j++)
    if (meter->cell[j] == nullptr) return hipErrorInvalidValue;
  if (pack.mixed != 0 ? (sc > kMixMaxChannels || ic > kMixMaxChannels) : sc != ic) return hipErrorInvalidValue;
  // the LDS tile of the vector path (at most 33.8 KB: no opt-in needed); more than 8 planes take the element path alone
  const uint32_t lds = sc <= kMixMaxChannels ? area_dwords(kTile * sc) * 4 : 0u;
  const dim3 grid((most + kTile - 1) / kTile, n), block(kLanes);
  return with_format(fmt, [&](auto format) -> hipError_t {
    constexpr int F = decltype(format)::value;
    if (gain != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      const DitherPack none = {};    // (kind NONE)
      const MeterPack no_cells = {};  // (nothing judged)
      hipLaunchKernelGGL((planes_out_gain<F>), grid, block, lds, stream, pack, dith != nullptr ? *dith : none,
                         meter != nullptr ? *meter : no_cells, *gain);
    } else if (meter != nullptr) {
      if (dith != nullptr && !dithered_fmt(F)) return hipErrorInvalidValue;
      DitherPack none = {};  // (kind NONE)
      hipLaunchKernelGGL((planes_out_meter<F>), grid, block, lds, stream, pack, dith != nullptr ? *dith : none, *meter);
    } else if (dith == nullptr) {
      if (out)
        hipLaunchKernelGGL((planes_out<F>), grid, block, lds, stream, pack);
      else
        hipLaunchKernelGGL((planes_in<F>), grid, block, lds, stream, pack);
    } else if constexpr (dithered_fmt(F)) {
      hipLaunchKernelGGL((planes_out_dither<F>), grid, block, lds, stream, pack, *dith);
    } else {
      return hipErrorInvalidValue;  // (the float formats are not dithered)
    }
    return hipGetLastError();
  });
}

}  // namespace speexhip
