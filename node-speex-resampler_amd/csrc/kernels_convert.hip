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
// The formats themselves -- one sample to and from the image, rounding half up, and the loads / stores of one sample --
// are stated in format_device.h, which the mixing kernels (kernels_mix.hip) share.
//
// convert_out_dither<F> (the formats of dithered_fmt; a state with dither on): convert_out with the dither of dither.h added
// before the rounding.  Instances of their own beside convert_out -- the same body, kDither = true: the same two paths,
// the same bytes from both.  Sample k of a stream has idx first + k (DitherPack; the launcher takes step 1 only), so a
// lane's group on the vector path is a run of G consecutive idx: the inner half of the generator's word, which changes
// once per 2^32 samples, is taken once per group (twice for the one group that crosses such a boundary), once per sample
// on the element path.  The kind is one per launch: wave-uniform.
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "kernels.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(convert)

namespace {

using namespace fmtdev;  // to_internal / from_internal, load_raw / store_raw, with_format

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTile = 4096;  // samples per workgroup

// samples a lane owns per pass of the vector path: whole 16-byte pieces on both sides
constexpr uint32_t group_of(int f) { return sample_bytes(f) == 1 || sample_bytes(f) == 3 ? 16u : sample_bytes(f) == 2 ? 8u : 4u; }

// ---- 16 bytes per lane ---------------------------------------------------------------------------------------------
// sample j (compile-time) of a lane's group, from / into the group's storage words
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

// kDither (kOut only): the dithered instances; d and kind are theirs alone
template <int F, bool kOut, bool kDither>
__device__ __forceinline__ void vector_tile(const ConvertStream &s, const DitherStream *d, int kind, uint64_t tile0) {
  constexpr uint32_t B = sample_bytes(F), G = group_of(F), words = G * B / 4;
  constexpr int W = word_format(F);  // (S16BE / S32BE: the words are reversed as dwords, the samples then the twin's)
  const char *src = static_cast<const char *>(s.src);
  char *dst = static_cast<char *>(s.dst);
#pragma unroll
  for (uint32_t pass = 0; pass < kTile / (kLanes * G); pass++) {
    const uint64_t first = tile0 + static_cast<uint64_t>(pass * kLanes + threadIdx.x) * G;  // the lane's first sample
    const dither::Run run = kDither ? dither::run_of(d->seed, d->first + first, G) : dither::Run{};
    uint32_t w[words];
    float e[G];
    if (!kOut) {
      const uint4 *in = reinterpret_cast<const uint4 *>(src + first * B);
#pragma unroll
      for (uint32_t i = 0; i < words / 4; i++) {
        const uint4 v = in[i];
        w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
      }
      swap_words<F, words>(w);
#pragma unroll
      for (uint32_t j = 0; j < G; j++) e[j] = to_internal<W>(raw_of<W>(w, j));
      float4 *out = reinterpret_cast<float4 *>(dst + first * sizeof(float));
#pragma unroll
      for (uint32_t i = 0; i < G / 4; i++) out[i] = make_float4(e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]);
    } else {
      const float4 *in = reinterpret_cast<const float4 *>(src + first * sizeof(float));
#pragma unroll
      for (uint32_t i = 0; i < G / 4; i++) {
        const float4 v = in[i];
        e[4 * i] = v.x, e[4 * i + 1] = v.y, e[4 * i + 2] = v.z, e[4 * i + 3] = v.w;
      }
#pragma unroll
      for (uint32_t i = 0; i < words; i++) w[i] = 0;
#pragma unroll
      for (uint32_t j = 0; j < G; j++)
        put_raw<W>(w, j, encode<W, kDither>(e[j], [&] { return dither::noise_in(kind, run, j); }));
      swap_words<F, words>(w);
      uint4 *out = reinterpret_cast<uint4 *>(dst + first * B);
#pragma unroll
      for (uint32_t i = 0; i < words / 4; i++) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
  }
}

// ---- sample by sample ----------------------------------------------------------------------------------------------
// samples [tile0, tile0 + n) of the stream; sample k lies k * step elements into both buffers (dithered: step is 1)
template <int F, bool kOut, bool kDither>
__device__ __forceinline__ void element_tile(const ConvertStream &s, const DitherStream *d, int kind, uint64_t tile0,
                                             uint32_t n) {
  constexpr uint32_t B = sample_bytes(F);
  const char *src = static_cast<const char *>(s.src);
  char *dst = static_cast<char *>(s.dst);
  for (uint32_t i = threadIdx.x; i < n; i += kLanes) {
    const uint64_t at = kDither ? tile0 + i : (tile0 + i) * s.step;
    if (!kOut)
      *reinterpret_cast<float *>(dst + at * sizeof(float)) = to_internal<F>(load_raw<F>(src + at * B));
    else
      store_raw<F>(dst + at * B, encode<F, kDither>(*reinterpret_cast<const float *>(src + at * sizeof(float)),
                                                    [&] { return dither::noise(kind, d->seed, d->first + at); }));
  }
}

template <int F, bool kOut, bool kDither>
__device__ __forceinline__ void convert_tile(const ConvertPack &pack, const DitherPack *dith) {
  const ConvertStream &s = pack.s[blockIdx.y];
  const DitherStream *d = kDither ? &dith->s[blockIdx.y] : nullptr;
  const int kind = kDither ? dith->kind : 0;
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  if (s.src == nullptr || tile0 >= s.n) return;  // (nothing to convert, or a shorter stream of the launch)
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), s.n - tile0));
  const bool aligned = ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 15u) == 0;
  if (n == kTile && aligned && (kDither || s.step == 1))
    vector_tile<F, kOut, kDither>(s, d, kind, tile0);
  else
    element_tile<F, kOut, kDither>(s, d, kind, tile0, n);
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

}  // namespace

hipError_t launch_convert(int fmt, bool out, const ConvertPack &pack, const DitherPack *dith, uint32_t n, uint64_t most,
                          hipStream_t stream) {
  if (n == 0 || most == 0) return hipSuccess;
  for (uint32_t j = 0; dith != nullptr && j < n; j++)
    if (!out || pack.s[j].step != 1) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((most + kTile - 1) / kTile), n), block(kLanes);
  return with_format(fmt, [&](auto format) -> hipError_t {
    constexpr int F = decltype(format)::value;
    // (F32 is the image's own format: nothing to convert; the float formats are not dithered)
    if constexpr (F == SPEEXHIP_FMT_F32) {
      return hipErrorInvalidValue;
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
