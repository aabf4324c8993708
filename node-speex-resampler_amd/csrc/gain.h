// gain.h -- the one statement of the per-stream output gain (include/speexhip_resampler.h, "Gain"), host and device: the
// gained instances of the output passes (kernels_convert.hip, kernels_convert_many.hip, kernels_mix.hip,
// kernels_sides.hip), the kernel gain_image, the engine's set_gain / get_gain and the host function speexhip_debug_gain
// (c_api.cpp) compile these very lines.  A stream's gain state is (from, to, total, done); the gain of the output frame
// that stands k frames behind the start of the ramp is
//
//   g(k) = (float)( (double)from + (double)k * step )   for k <  total     step = ((double)to - (double)from) / (double)total,
//   g(k) = to                                           for k >= total     formed once, on the host, by set_gain
//
// the product rounded once, the sum once more (never contracted: -ffp-contract=off on every unit), then nearest-even to
// fp32.  k is an integer index of the stream alone (done + the frame within the call, in 64 bits), so a gained stream's
// bytes depend on the stream alone.  Every sample of the frame becomes y * g, one fp32 product: behind the output
// matrix's rounding, before the meter's judgement, the dither and from_internal.
//
// On the device a stream of a launch is in one of three wave-uniform modes (its GainStream is a kernel argument selected
// by blockIdx.y): off -- nothing is multiplied, so an ungained stream that shares a launch keeps its bits, NaN payloads
// and signed zeros included (the selection, not a product with 1.0f, which would quiet a signalling NaN); constant --
// first >= total, one v_mul_f32 per sample and no index; ramp -- g(k) per frame.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/speexhip_resampler.h"
#include "format_device.h"
#include "kernels.h"
#include "meter.h"

namespace speexhip {
namespace gain {

// step of a ramp (host only: the device never forms it); total = 0: no ramp, nothing reads it
inline double step_of(float from, float to, uint32_t total) {
  return total == 0 ? 0.0 : (static_cast<double>(to) - static_cast<double>(from)) / static_cast<double>(total);
}

// g(k)
__host__ __device__ inline float at(double step, float from, float to, uint32_t total, uint64_t k) {
  if (k >= total) return to;
  const double p = static_cast<double>(k) * step;  // (k < 2^32: exact in fp64)
  const double s = static_cast<double>(from) + p;
  return static_cast<float>(s);
}

// off: the default, and what a ramp that ends at 1.0 returns to
inline bool is_off(float to, uint32_t total, uint32_t done) { return to == 1.0f && (total == 0 || done == total); }

#if defined(__HIPCC__)
enum : uint32_t { kOff = 0, kConstant = 1, kRamp = 2 };

// A workgroup's view of its stream's gain: wave-uniform throughout.  plain: neither dither nor meter is wanted of this
// stream (kind NONE and no cell), so its samples leave through from_internal -- the same bytes as the dithered body at
// d = 0, without its fp64 sum or the judgement.
struct Tile {
  const GainStream *s;
  uint32_t mode;
  float g;  // kConstant
  bool plain;
};
__device__ __forceinline__ Tile tile_of(const GainStream &s, bool plain) {
  Tile t;
  t.s = &s;
  t.mode = s.channels == 0 ? kOff : s.first >= s.total ? kConstant : kRamp;
  t.g = s.to;
  t.plain = plain;
  return t;
}

// y' of a sample of the frame that stands `frame` frames into the launch
__device__ __forceinline__ float apply(const Tile &t, float y, uint64_t frame) {
  if (t.mode == kOff) return y;
  const float g = t.mode == kConstant ? t.g : at(t.s->step, t.s->from, t.s->to, t.s->total, t.s->first + frame);
  return y * g;
}

// The frame of a sample of a flat (interleaved) pass, for the ramp: the tile's first sample is split once, in 64 bits
// (sample counts beyond 2^32), the lane's offset into the tile (< 4096 + channels) in 32.
struct Split {
  uint64_t q0;  // frame of the tile's first sample
  uint32_t r0;  // its channel
  uint32_t c;   // samples of a frame
};
__device__ __forceinline__ Split split_of(const Tile &t, uint64_t tile0) {
  Split sp = {0, 0, 1};
  if (t.mode == kRamp) {
    sp.c = t.s->channels;
    sp.q0 = tile0 / sp.c;
    sp.r0 = static_cast<uint32_t>(tile0 - sp.q0 * sp.c);
  }
  return sp;
}
// frame (within the launch) of the sample `i` samples into the tile; only a ramp reads it, and only a ramp divides
__device__ __forceinline__ uint64_t frame_of(const Tile &t, const Split &sp, uint32_t i) {
  return t.mode == kRamp ? sp.q0 + (sp.r0 + i) / sp.c : 0;
}

// A lane's group of G consecutive samples, the first `i0` samples into the tile, multiplied in place: one run of products
// at the constant g, or g of each sample's own frame in a ramp (a group may straddle frames); nothing when off.
template <uint32_t G>
__device__ __forceinline__ void apply_group(const Tile &t, const Split &sp, uint32_t i0, float (&e)[G]) {
  if (t.mode == kConstant) {
#pragma unroll
    for (uint32_t j = 0; j < G; j++) e[j] = e[j] * t.g;
  } else if (t.mode == kRamp) {
    // (one division for the group, then frame and channel walk on together)
    const uint32_t off = sp.r0 + i0;
    uint64_t q = sp.q0 + off / sp.c;
    uint32_t r = off % sp.c;
#pragma unroll
    for (uint32_t j = 0; j < G; j++) {
      e[j] = e[j] * at(t.s->step, t.s->from, t.s->to, t.s->total, t.s->first + q);
      if (++r == sp.c) r = 0, q++;
    }
  }
}

// What a gained output pass stores for y of frame `frame`: multiplied, then judged and dithered as its stream asks
template <int F, class Noise>
__device__ __forceinline__ uint32_t encode(const Tile &t, meter::Lane &m, float y, uint64_t frame, Noise noise) {
  const float v = apply(t, y, frame);
  if (t.plain) return fmtdev::from_internal<F>(v);
  return meter::encode<F, dithered_fmt(F), true>(m, v, noise);
}
#endif

}  // namespace gain
}  // namespace speexhip
