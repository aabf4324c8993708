// kernels_convert_impl.h -- the bodies of the converting passes, stated once for the two units that run them:
// kernels_convert.hip (one format per launch: convert_in<F> / convert_out<F> / convert_out_dither<F>) and
// kernels_convert_many.hip (a format per stream of the launch: convert_many_in / convert_many_out).  Both reach a stream's
// tile through stream_tile<F, kOut, kDither> below, so a stream's bytes are the same from either unit by construction.
// What the two paths are and why the loads and stores are plain: the head of kernels_convert.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "gain.h"
#include "kernels.h"
#include "meter.h"

namespace speexhip {
namespace convert_impl {

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

// kDither (kOut only): the dithered instances; d and kind are theirs alone.  kMeter (kOut only): the metered instances;
// m takes what the lane's samples come to (meter.h) and is theirs alone.  kGain (kOut, kMeter and kDither = dithered_fmt(F)
// only): the gained instances; gt (gain.h) is theirs alone -- a sample is multiplied by the g of its frame, then leaves as
// its stream asks
template <int F, bool kOut, bool kDither, bool kMeter, bool kGain>
__device__ __forceinline__ void vector_tile(const ConvertStream &s, const DitherStream *d, int kind, uint64_t tile0,
                                            meter::Lane &m, const gain::Tile &gt) {
  constexpr uint32_t B = sample_bytes(F), G = group_of(F), words = G * B / 4;
  constexpr int W = word_format(F);  // (S16BE / S32BE: the words are reversed as dwords, the samples then the twin's)
  const char *src = static_cast<const char *>(s.src);
  char *dst = static_cast<char *>(s.dst);
  const gain::Split sp = kGain ? gain::split_of(gt, tile0) : gain::Split{};
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
      if constexpr (kGain) {
        // The group is multiplied, then encoded, each in one straight run: the stream's mode and what it asks of the
        // encoder are wave-uniform, so they are branched on once per group, not once per sample.
        gain::apply_group<G>(gt, sp, (pass * kLanes + threadIdx.x) * G, e);
        if (gt.plain) {
#pragma unroll
          for (uint32_t j = 0; j < G; j++) put_raw<W>(w, j, from_internal<W>(e[j]));
        } else {
#pragma unroll
          for (uint32_t j = 0; j < G; j++)
            put_raw<W>(w, j, meter::encode<W, kDither, true>(m, e[j], [&] { return dither::noise_in(kind, run, j); }));
        }
      } else {
#pragma unroll
        for (uint32_t j = 0; j < G; j++)
          put_raw<W>(w, j, meter::encode<W, kDither, kMeter>(m, e[j], [&] { return dither::noise_in(kind, run, j); }));
      }
      swap_words<F, words>(w);
      uint4 *out = reinterpret_cast<uint4 *>(dst + first * B);
#pragma unroll
      for (uint32_t i = 0; i < words / 4; i++) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
  }
}

// ---- sample by sample ----------------------------------------------------------------------------------------------
// samples [tile0, tile0 + n) of the stream; sample k lies k * step elements into both buffers (dithered: step is 1)
template <int F, bool kOut, bool kDither, bool kMeter, bool kGain>
__device__ __forceinline__ void element_tile(const ConvertStream &s, const DitherStream *d, int kind, uint64_t tile0,
                                             uint32_t n, meter::Lane &m, const gain::Tile &gt) {
  constexpr uint32_t B = sample_bytes(F);
  const char *src = static_cast<const char *>(s.src);
  char *dst = static_cast<char *>(s.dst);
  const gain::Split sp = kGain ? gain::split_of(gt, tile0) : gain::Split{};
  for (uint32_t i = threadIdx.x; i < n; i += kLanes) {
    const uint64_t at = kDither ? tile0 + i : (tile0 + i) * s.step;
    if (!kOut)
      *reinterpret_cast<float *>(dst + at * sizeof(float)) = to_internal<F>(load_raw<F>(src + at * B));
    else if constexpr (kGain)
      store_raw<F>(dst + at * B,
                   gain::encode<F>(gt, m, *reinterpret_cast<const float *>(src + at * sizeof(float)), gain::frame_of(gt, sp, i),
                                   [&] { return dither::noise(kind, d->seed, d->first + at); }));
    else
      store_raw<F>(dst + at * B,
                   meter::encode<F, kDither, kMeter>(m, *reinterpret_cast<const float *>(src + at * sizeof(float)),
                                                     [&] { return dither::noise(kind, d->seed, d->first + at); }));
  }
}

// The tile blockIdx.x of one stream: the vector path for whole tiles with storage and image 16-byte aligned and step 1,
// the element path for everything else.  s, d and kind are wave-uniform (kernel arguments selected by blockIdx.y).
// kMeter: the workgroup's totals go into *cell (wave-uniform too) behind its tile.  kGain: the gained body, the stream's
// gain in *g; dither and meter are then taken at run time -- kind NONE: d = 0, a NULL cell: nothing committed.
template <int F, bool kOut, bool kDither, bool kMeter = false, bool kGain = false>
__device__ __forceinline__ void stream_tile(const ConvertStream &s, const DitherStream *d, int kind, MeterCell *cell = nullptr,
                                            const GainStream *g = nullptr) {
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  if (s.src == nullptr || tile0 >= s.n) return;  // (nothing to convert, or a shorter stream of the launch)
  const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(kTile), s.n - tile0));
  const bool aligned = ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 15u) == 0;
  meter::Lane m;
  const gain::Tile gt = kGain ? gain::tile_of(*g, cell == nullptr && kind == SPEEXHIP_DITHER_NONE) : gain::Tile{};
  if (n == kTile && aligned && (kDither || kGain || s.step == 1))
    vector_tile<F, kOut, kDither, kMeter, kGain>(s, d, kind, tile0, m, gt);
  else
    element_tile<F, kOut, kDither, kMeter, kGain>(s, d, kind, tile0, n, m, gt);
  // (every lane of the workgroup: the early return above is the workgroup's, and so is the cell)
  if constexpr (kGain) {
    if (cell != nullptr) meter::commit(m, cell);
  } else if constexpr (kMeter) {
    meter::commit(m, cell);
  }
}

}  // namespace convert_impl
}  // namespace speexhip
