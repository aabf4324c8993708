// formats.cpp -- the formatted and mixed calls of engine.h: the caller names the sample format of either side
// (SPEEXHIP_FMT_*), and a side may carry a channel matrix (CallSide).  One pipeline serves them all:
// storage --the input side's pass--> float scratch image --the existing float launch--> float scratch image --the output
// side's pass--> storage (side_pass, mix.cpp).  Counters, positions and the history are the float call's, so formatted,
// mixed, interleaved, planar and per-channel calls mix freely on one state.  The state's dither (set_dither) lives here too;
// its meter (set_meter / get_meter) in engine.cpp, beside the control copies it uses.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "dither.h"
#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
// the side with its one stream at `base` (a staging buffer of a host call)
inline CallSide at(const CallSide &side, const void *base) {
  return CallSide{side.fmt, side.channels, side.mix, const_cast<void *>(base), 0};
}
// ... a planar side with its planes `pitch` samples apart in a staging image at `base`
inline CallSide planes_at(const CallSide &side, const void *base, uint64_t pitch) {
  CallSide staged = at(side, base);
  staged.layout = SPEEXHIP_LAYOUT_PLANAR;
  staged.plane_stride = pitch;
  return staged;
}
// plane c of a host side
inline char *host_plane(const CallSide &side, uint32_t c) {
  return side.planes != nullptr ? static_cast<char *>(side.planes[c])
                                : static_cast<char *>(side.base) + c * side.plane_stride * sample_bytes(side.fmt);
}
// ... all of them, each `skip` bytes in
inline std::vector<void *> host_planes(const CallSide &side, size_t skip = 0) {
  std::vector<void *> planes(side.channels);
  for (uint32_t c = 0; c < side.channels; c++) planes[c] = host_plane(side, c) + skip;
  return planes;
}
// A host side that is not planar, as one buffer: a mono side given as its one plane is that plane.
inline int flatten(CallSide *side) {
  if (side_planar(*side) || side->planes == nullptr) return SPEEXHIP_ERR_SUCCESS;
  if (side->planes[0] == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  side->base = side->planes[0];
  side->planes = nullptr;
  return SPEEXHIP_ERR_SUCCESS;
}
// a side given as plane pointers with one of them null
inline bool lacks_plane(const CallSide &side) {
  for (uint32_t c = 0; side.planes != nullptr && c < side.channels; c++)
    if (side.planes[c] == nullptr) return true;
  return false;
}
// whether the `out_bytes` written to a plane of a planar host result overlap another of its planes, or the `in_bytes`
// read from a plane of `in` (may be null: no planar input to compare)
inline bool planes_overlap(const CallSide &out, size_t out_bytes, const CallSide *in, size_t in_bytes) {
  for (uint32_t c = 0; c < out.channels; c++) {
    for (uint32_t k = 0; k < c; k++)
      if (buffers_overlap(host_plane(out, c), out_bytes, host_plane(out, k), out_bytes)) return true;
    for (uint32_t k = 0; in != nullptr && k < in->channels; k++)
      if (buffers_overlap(host_plane(out, c), out_bytes, host_plane(*in, k), in_bytes)) return true;
  }
  return false;
}
}  // namespace

// ---- dither (engine.h) -------------------------------------------------------------------------------------------------
int Batch::set_dither(int kind, uint64_t seed, uint64_t position) {
  if (!dither::known_kind(kind)) return SPEEXHIP_ERR_INVALID_ARG;
  dither_kind_ = kind;
  dither_seed_ = seed;
  dither_pos_.assign(n_streams_, position);
  bus_out_.set_dither(kind, seed, position);  // (the buses' one position, whether or not buses are on: bus.cpp)
  return SPEEXHIP_ERR_SUCCESS;
}
int Batch::get_dither(uint32_t stream, int *kind, uint64_t *seed, uint64_t *position) const {
  if (stream >= n_streams_) return SPEEXHIP_ERR_INVALID_ARG;
  if (kind != nullptr) *kind = dither_kind_;
  if (seed != nullptr) *seed = dither::stream_seed(dither_seed_, stream);
  if (position != nullptr) *position = dither_pos_.empty() ? 0 : dither_pos_[stream];
  return SPEEXHIP_ERR_SUCCESS;
}
DitherPack Batch::dither_pack(uint32_t s0, uint32_t n, uint32_t per_frame) const {
  DitherPack d;
  std::memset(&d, 0, sizeof(d));
  d.kind = dither_kind_;
  for (uint32_t j = 0; j < n; j++) {
    d.s[j].seed = dither::stream_seed(dither_seed_, s0 + j);
    d.s[j].first = (dither_pos_.empty() ? 0 : dither_pos_[s0 + j]) * per_frame;  // (mod 2^64, like idx)
  }
  return d;
}
void Batch::dither_advance(const uint32_t *produced) {
  if (dither_pos_.empty()) dither_pos_.assign(n_streams_, 0);
  for (uint32_t s = 0; s < n_streams_; s++) dither_pos_[s] += produced[s];
}

// ---- the route (sides_route.h), described and obeyed ----------------------------------------------------------------------
SidesState Batch::sides_state(bool repeated) const {
  SidesState st = {dither_on(), meter_on_, gain_on(), false, zero_mode_, n_streams_ == 1, repeated};
  for (uint32_t s = 0; s < n_streams_ && !st.split; s++) st.split = !uniform(s);
  return st;
}
void Batch::sides_moved(const SidesRoute &r, const uint32_t *produced, uint32_t per_frame) {
  if (r.counts_meter) meter_count(produced, per_frame);
  if (r.moves_gain) gain_advance(produced);
  if (r.moves_dither) dither_advance(produced);
}

// The float images of a call and its input pass: one stream after the other, whole 128-byte lines each, sized from what
// this call moves.  (The zero fallback goes through them as well: its history still takes the converted input, and its
// silence is whatever the float call writes, converted -- and dithered.)  bus: the streams' results always lie in the
// state's image, whatever the route.
int Batch::prepare_images(const CallSide &in, const uint32_t *in_len, const uint32_t *out_len, const SidesRoute &r, bool split,
                          bool bus, hipStream_t stream, SideImages *im) {
  // what the float call will do, known before anything is launched (integer arithmetic)
  const EntryRules rules = entry_rules(true);
  uint32_t most_in = 0;
  im->most_out = 0;
  for (uint32_t s = 0; s < n_streams_; s++) {
    most_in = std::max(most_in, in_len[s]);
    for (uint32_t c = 0; c < (split ? channels_ : 1u); c++)
      im->most_out = std::max(im->most_out, plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, c), rules).produced);
  }
  // a present but empty input is not silence: no frame is read, any non-null address serves
  const bool pass_in = r.pass_in && in.base != nullptr && most_in != 0;
  const size_t in_pitch = align64(static_cast<size_t>(most_in) * channels_);
  im->out_pitch = align64(static_cast<size_t>(im->most_out) * channels_);
  int rc = ensure_planar_scratch(pass_in ? in_pitch * n_streams_ * sizeof(float) : 0,
                                 bus || r.pass_out ? im->out_pitch * n_streams_ * sizeof(float) : 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (bus || pass_in || (r.pass_out && im->most_out != 0)) {
    // (the images and the cells belong to the state: a call on another stream than the previous one waits for it first)
    rc = chain_to(stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (pass_in) {
    rc = side_pass(in, true, d_planar_in_, in_pitch, in_len, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  im->in = pass_in ? static_cast<const void *>(d_planar_in_) : in.base;
  im->in_stride = pass_in ? in_pitch : in.stride;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::process_sides_device(const CallSide &in_side, uint32_t *in_len, const CallSide &out_side, uint32_t *out_len,
                                hipStream_t stream, std::vector<CallPlan> *plans_out) {
  if (!side_ok(in_side, channels_) || !side_ok(out_side, channels_)) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, n_streams_)) return SPEEXHIP_ERR_OVERFLOW;  // (engine.h; nothing touched)
  // (a side of one channel is the same bytes in either layout)
  CallSide in = in_side, out = out_side;
  if (!side_planar(in)) in.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  if (!side_planar(out)) out.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  ON_DEVICE();
  const SidesState st = sides_state();
  const SidesRoute r = route_sides_call(SidesForm::Device, side_kind(in), side_kind(out), st);
  if (r.refuse != SPEEXHIP_ERR_SUCCESS) return r.refuse;
  int rc;
  void *result = out.base;  // what a call without an output pass wrote
  std::vector<CallPlan> plans;  // of the channels of a state whose channels stand apart
  if (r.kind == SidesRoute::PlanarFloatCall) {
    rc = process_planar_device(in.base, in.stride, in.plane_stride, in_len, out.base, out.stride, out.plane_stride, out_len, true,
                               stream);
  } else if (r.kind != SidesRoute::Images) {
    rc = process_device(in.base, in.stride, in_len, out.base, out.stride, out_len, r.kind == SidesRoute::FloatCall, stream);
  } else {
    SideImages im;
    rc = prepare_images(in, in_len, out_len, r, st.split, false, stream, &im);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    if (r.pass_out) result = d_planar_out_;
    if (st.split)
      rc = process_split(im.in, in_len, result, out_len, true, stream, &plans);
    else
      rc = process_device(im.in, im.in_stride, in_len, result, r.pass_out ? im.out_pitch : out.stride, out_len, true, stream);
    if (ran(rc) && plans_out != nullptr) *plans_out = plans;
    if (ran(rc) && r.pass_out) {
      // (out_len: what the float call produced)
      const int prc = side_pass(out, false, d_planar_out_, im.out_pitch, out_len, stream, st.split ? plans.data() : nullptr);
      if (prc != SPEEXHIP_ERR_SUCCESS) return prc;
    }
  }
  if (!ran(rc)) return rc;
  if (r.finish != SidesRoute::Nothing) {
    // (the FIR wrote the caller's buffer: read once more by meter_image, or multiplied in place by gain_image, an F32N
    //  result as stored, and judged in that same pass)
    const int frc = image_result(result, out.stride, out_len, r.finish_scale, stream);
    if (frc != SPEEXHIP_ERR_SUCCESS) return frc;
  }
  sides_moved(r, out_len, out.channels);
  return rc;
}

// The formatted many-states call (engine.h): the entries as many_run takes them, which asks the route of each (many.cpp).
int Batch::process_host_many_sides(uint32_t n, Batch *const *st, const CallSide *in, uint32_t *in_len, const CallSide *out,
                                   uint32_t *out_len, const uint8_t *bad, int *codes) {
  std::vector<ManyEntry> entries(n);
  for (uint32_t i = 0; i < n; i++) {
    ManyEntry &e = entries[i];
    Batch *b = e.b = st[i];
    e.sides = true;
    if (b == nullptr || (bad != nullptr && bad[i] != 0) || !side_ok(in[i], b->channels_) || !side_ok(out[i], b->channels_) ||
        (out[i].base == nullptr && out[i].planes == nullptr)) {
      e.rc = SPEEXHIP_ERR_INVALID_ARG;
      continue;
    }
    e.in_side = in[i];
    e.out_side = out[i];
    e.in_fmt = in[i].fmt;
    e.out_fmt = out[i].fmt;
    e.in = in[i].base;  // (read where the entry is fused: one interleaved buffer a side)
    e.out = out[i].base;
  }
  return many_run(n, entries.data(), in_len, out_len, codes);
}

// process_sides_device on own_stream_ around a single-stream call's host buffers: the raw bytes of both sides move by the
// rule of host_transfer.h -- in place when pinned, through the bounce buffers when small, by the runtime's staged copy when
// large; channels that stand apart as in process_host.
int Batch::process_sides_host(const CallSide &in_side, uint32_t *in_len, const CallSide &out_side, uint32_t *out_len) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (!side_ok(in_side, channels_) || !side_ok(out_side, channels_)) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  if (side_planar(in_side) || side_planar(out_side)) return planes_host_call(in_side, in_len, out_side, out_len);
  CallSide in = in_side, out = out_side;
  if (flatten(&in) != SPEEXHIP_ERR_SUCCESS || flatten(&out) != SPEEXHIP_ERR_SUCCESS || out.base == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const SidesState st = sides_state();
  const SidesRoute r = route_sides_call(SidesForm::Host, side_kind(in), side_kind(out), st);
  if (r.refuse != SPEEXHIP_ERR_SUCCESS && !r.refuse_late) return r.refuse;
  if (r.direct) {
    const int rc = process_host(in.base, in_len, out.base, out_len, r.kind == SidesRoute::FloatCall);
    if (ran(rc)) sides_moved(r, out_len, out.channels);
    return rc;
  }
  ON_DEVICE();
  if (r.refuse != SPEEXHIP_ERR_SUCCESS) return r.refuse;
  const bool split = st.split;
  const size_t bout = sample_bytes(out.fmt);
  // (only as many output frames as this call can produce need a device buffer)
  const size_t in_bytes = static_cast<size_t>(*in_len) * in.channels * sample_bytes(in.fmt);
  const size_t out_bytes = static_cast<size_t>(will_make(*in_len, *out_len)) * out.channels * bout;
  const void *pin_in = nullptr;
  void *pin_out = nullptr;
  if (!split) pinned_sides(in.base, in_bytes, out.base, out_bytes, &pin_in, &pin_out);
  HostCallShape shape;
  shape.split = split;
  shape.in = flat_side(in.base != nullptr, pin_in != nullptr, in_bytes);
  shape.out = flat_side(true, pin_out != nullptr, out_bytes);
  HostCall call(this);
  const HostPiece piece = {in.base, 0, in_bytes};
  int rc = call.begin(route_host_call(shape), &piece, 1, pin_in, pin_out);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  std::vector<CallPlan> plans;  // (of the channels that stand apart)
  rc = process_sides_device(at(in, call.src), in_len, at(out, call.dst), out_len, own_stream_, split ? &plans : nullptr);
  if (!ran(rc)) return rc;
  const int frc = split ? call.finish_samples(out.base, channels_, channels_, bout, made_per_channel(channels_, 0, plans.data()).data())
                        : call.finish_whole(out.base, static_cast<size_t>(*out_len) * out.channels * bout);
  return frc != SPEEXHIP_ERR_SUCCESS ? frc : rc;
}

// ---- the formatted chunks call (engine.h) -----------------------------------------------------------------------------------
namespace {
// speexhip_debug_chunk_counters: FIR launches, input passes, output passes, chunks that took a call of their own
std::atomic<uint64_t> g_chunk_counters[4];
inline void count_chunks(int which, uint64_t by = 1) { g_chunk_counters[which].fetch_add(by, std::memory_order_relaxed); }

// The chunks of a call planned one after the other in integer arithmetic, and the launch groups they form -- the rule of
// process_host_chunks (engine.cpp): a capacity-bound chunk that leaves input unconsumed keeps one more frame readable and
// closes its group.
struct ChunkGroup {
  CallPlan fused;
  uint64_t in_off = 0, out_off = 0;  // frames into the staged images
  uint32_t readable = 0;             // frames at in_off the launch may read
};
struct ChunkPlans {
  std::vector<CallPlan> plans;
  std::vector<uint32_t> staged;  // frames of chunk i that travel: what it consumes, one more where it drops input
  std::vector<ChunkGroup> groups;
  uint64_t frames = 0, made = 0;  // frames staged / produced by the whole call
  uint32_t launches = 0;          // groups with anything to run
};
ChunkPlans plan_chunks(uint32_t num, uint32_t den, uint32_t n, const uint32_t *in_len, const uint32_t *out_len, StreamPos pos,
                       const EntryRules &rules) {
  ChunkPlans p;
  p.plans.resize(n);
  p.staged.resize(n);
  bool open = false;
  for (uint32_t i = 0; i < n; i++) {
    const CallPlan &plan = p.plans[i] = plan_call(num, den, in_len[i], out_len[i], pos, rules);
    pos = plan.end;
    if (!open) {
      ChunkGroup g;
      g.fused.begin = plan.begin;
      g.in_off = p.frames;
      g.out_off = p.made;
      p.groups.push_back(g);
      open = true;
    }
    const bool drops = plan.consumed < in_len[i];
    ChunkGroup &g = p.groups.back();
    g.fused.end = plan.end;
    g.fused.magic_used += plan.magic_used;
    g.fused.consumed += plan.consumed;
    g.fused.produced += plan.produced;
    p.staged[i] = plan.consumed + (drops ? 1u : 0u);
    g.readable += p.staged[i];
    p.frames += p.staged[i];
    p.made += plan.produced;
    if (drops) open = false;
  }
  for (const ChunkGroup &g : p.groups)
    if (g.fused.produced != 0 || g.fused.magic_used + g.fused.consumed != 0) p.launches++;
  return p;
}
}  // namespace

void chunk_counters(uint64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_chunk_counters[k].load(std::memory_order_relaxed);
}

int Batch::process_sides_host_chunks(uint32_t n_chunks, const CallSide &in, const void *const *in_data, uint32_t *in_len,
                                     const CallSide &out_side, uint32_t *out_len) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (!side_ok(in, channels_) || !side_ok(out_side, channels_)) return SPEEXHIP_ERR_INVALID_ARG;
  const bool pl_in = side_planar(in), pl_out = side_planar(out_side);
  CallSide out = out_side;
  if (flatten(&out) != SPEEXHIP_ERR_SUCCESS || (out.base == nullptr && out.planes == nullptr) || lacks_plane(out))
    return SPEEXHIP_ERR_INVALID_ARG;
  // entries of in_data per chunk; a present chunk has all its planes
  const uint32_t per = pl_in ? in.channels : 1u;
  const auto entry = [&](uint32_t i, uint32_t c) { return in_data != nullptr ? in_data[static_cast<size_t>(i) * per + c] : nullptr; };
  for (uint32_t i = 0; i < n_chunks; i++)
    for (uint32_t c = 1; entry(i, 0) != nullptr && c < per; c++)
      if (entry(i, c) == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  // With the meter or gain on the call on the same bytes (F32 or F32N then) is staged here without passes and finished
  // once over all chunks: the ramp's index runs on across the chunk boundaries as the dither's does.
  const SidesRoute r = route_sides_call(SidesForm::Chunks, side_kind(in), side_kind(out), sides_state());
  if (r.refuse != SPEEXHIP_ERR_SUCCESS) return r.refuse;
  const size_t bin = sample_bytes(in.fmt), bout = sample_bytes(out.fmt);
  if (r.kind == SidesRoute::OwnCalls) {  // rare states: the separate calls, one after the other, each output side behind the frames written
    int last = SPEEXHIP_ERR_SUCCESS;
    uint64_t written = 0;
    for (uint32_t i = 0; i < n_chunks; i++) {
      CallSide a = in, b = out;
      a.base = const_cast<void *>(entry(i, 0));
      a.planes = nullptr;
      if (pl_in && a.base != nullptr) a.planes = const_cast<void *const *>(in_data + static_cast<size_t>(i) * per), a.base = nullptr;
      std::vector<void *> planes;
      if (pl_out) {
        planes = host_planes(out, written * bout);
        if (out.planes != nullptr) b.planes = planes.data();
        else b.base = planes[0];
      } else {
        b.base = static_cast<char *>(out.base) + written * out.channels * bout;
      }
      last = process_sides_host(a, &in_len[i], b, &out_len[i]);
      if (!ran(last)) return last;
      written += out_len[i];
      count_chunks(3);
    }
    return last;
  }
  const ChunkPlans p = plan_chunks(filter_.num, filter_.den, n_chunks, in_len, out_len, P(0, 0), entry_rules(r.kind != SidesRoute::Int16Call));
  if (r.direct) {  // process_host_chunks on the same bytes (which serves the rare states itself)
    const int rc = process_host_chunks(n_chunks, in_data, in_len, out.base, out_len, r.kind == SidesRoute::FloatCall);
    if (!ran(rc)) return rc;
    uint32_t made = 0;
    for (uint32_t i = 0; i < n_chunks; i++) made += out_len[i];
    sides_moved(r, &made, out.channels);
    if (r.fusable) count_chunks(0, p.launches);
    else count_chunks(3, n_chunks);
    return rc;
  }
  if (p.frames > 0x7fffffffull || p.made > 0x7fffffffull) return SPEEXHIP_ERR_OVERFLOW;
  // (only so many frames are written to a plane: the sum of what the chunks will make)
  if (pl_out && planes_overlap(out, p.made * bout, nullptr, 0)) return SPEEXHIP_ERR_PTR_OVERLAP;
  ON_DEVICE();
  for (uint32_t i = 0; i < n_chunks; i++)
    if (in_len[i] != 0 && out_len[i] != 0) started_[0] = 1;
  // The staged images: the chunks' frames back to back, in the buffer or in every plane (planes whole 128-byte lines apart).
  const uint32_t frames = static_cast<uint32_t>(p.frames), made = static_cast<uint32_t>(p.made);
  const size_t in_pitch = align64(frames), out_pitch = align64(made);  // samples between two staged planes
  const size_t fb_in = pl_in ? bin : bin * in.channels;                // bytes of a frame in a piece
  HostCallShape shape;
  shape.gathered = true;  // (a silent chunk is gathered too, as zeros)
  shape.in = pl_in ? planar_side(true, frames * bin, in_pitch * bin, in.channels) : flat_side(true, false, frames * fb_in);
  shape.out = pl_out ? planar_side(true, made * bout, out_pitch * bout, out.channels) : flat_side(true, false, made * out.channels * bout);
  std::vector<HostPiece> pieces;
  pieces.reserve(static_cast<size_t>(n_chunks) * per);
  uint64_t off = 0;
  for (uint32_t i = 0; i < n_chunks; i++) {  // frames a chunk drops never reach the GPU
    for (uint32_t c = 0; c < per; c++) pieces.push_back({entry(i, c), (c * in_pitch + off) * fb_in, p.staged[i] * fb_in});
    off += p.staged[i];
  }
  HostCall call(this);
  int rc = call.begin(route_host_call(shape), pieces.data(), static_cast<uint32_t>(pieces.size()), nullptr, nullptr);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // The passes of process_sides_device, once over all chunks: conversion, matrix and dither are per sample or per frame,
  // and the dither index runs on over the chunks' output frames as the position does.
  const bool pass_in = r.pass_in && frames != 0, pass_out = r.pass_out;
  const size_t fi = channels_ * sizeof(float);  // bytes of a frame of the float images
  rc = ensure_planar_scratch(pass_in ? align64(static_cast<size_t>(frames) * channels_) * sizeof(float) : 0,
                             pass_out ? align64(static_cast<size_t>(made) * channels_) * sizeof(float) : 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (pass_in || (pass_out && made != 0)) {
    rc = chain_to(own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (pass_in) {
    rc = side_pass(pl_in ? planes_at(in, call.src, in_pitch) : at(in, call.src), true, d_planar_in_, 0, &frames, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    // (a silent chunk is zeros in the float image, as the FIR reads an absent input -- not what the format's zero bytes or
    //  a matrix's negative coefficient make of them)
    off = 0;
    for (uint32_t i = 0; i < n_chunks; off += p.staged[i], i++)
      if (entry(i, 0) == nullptr && p.staged[i] != 0) HIP_TRY(hipMemsetAsync(d_planar_in_ + off * fi, 0, p.staged[i] * fi, own_stream_));
  }
  const char *image_in = pass_in ? d_planar_in_ : static_cast<const char *>(call.src);
  char *image_out = pass_out ? d_planar_out_ : static_cast<char *>(call.dst);
  for (const ChunkGroup &g : p.groups) {
    rc = run_plans(image_in != nullptr ? image_in + g.in_off * fi : nullptr, 0, &g.readable, image_out + g.out_off * fi, 0, &g.fused,
                   true, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (pass_out) {
    rc = side_pass(pl_out ? planes_at(out, call.dst, out_pitch) : at(out, call.dst), false, d_planar_out_, 0, &made, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  } else if (r.finish != SidesRoute::Nothing) {
    rc = image_result(call.dst, 0, &made, r.finish_scale, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  sides_moved(r, &made, out.channels);
  if (pl_out) {
    rc = call.finish_planes(host_planes(out).data(), out.channels, out_pitch * bout, bout, std::vector<uint32_t>(out.channels, made).data());
  } else {
    rc = call.finish_whole(out.base, static_cast<size_t>(made) * out.channels * bout);
  }
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t i = 0; i < n_chunks; i++) {
    in_len[i] = p.plans[i].consumed;
    out_len[i] = p.plans[i].produced;
  }
  count_chunks(0, p.launches);
  count_chunks(1, pass_in ? 1 : 0);
  count_chunks(2, pass_out && made != 0 ? 1 : 0);
  return SPEEXHIP_ERR_SUCCESS;
}

// A host call with a planar side.  Each side moves by its own rule (host_transfer.h): an interleaved side as in
// process_sides_host above -- in place when pinned, through the bounce buffer when small, by the runtime's staged copy when large --
// a planar side plane by plane into an image whose planes lie whole 128-byte lines apart, as in process_planar_host (all
// planes of a side have one size, so one route serves the side).  process_sides_device then runs on the images.
int Batch::planes_host_call(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len) {
  const bool pl_in = side_planar(in), pl_out = side_planar(out);
  const SidesState st = sides_state();
  const SidesRoute r = route_sides_call(SidesForm::PlanesHost, side_kind(in), side_kind(out), st);
  if (r.refuse != SPEEXHIP_ERR_SUCCESS) return r.refuse;
  const bool split = st.split;
  CallSide in_flat = in, out_flat = out;
  if (flatten(&in_flat) != SPEEXHIP_ERR_SUCCESS || flatten(&out_flat) != SPEEXHIP_ERR_SUCCESS) return SPEEXHIP_ERR_INVALID_ARG;
  const bool present = in_flat.planes != nullptr || in_flat.base != nullptr;
  if (out_flat.planes == nullptr && out_flat.base == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  if (lacks_plane(in_flat) || lacks_plane(out_flat)) return SPEEXHIP_ERR_INVALID_ARG;
  const uint32_t frames = *in_len;
  const uint32_t most = will_make(frames, *out_len);  // only so many output frames are written (and need a device buffer)
  const size_t bin = sample_bytes(in.fmt), bout = sample_bytes(out.fmt);
  const size_t plane_in = frames * bin, plane_out = most * bout;
  if (pl_out && planes_overlap(out, plane_out, pl_in && present ? &in : nullptr, plane_in)) return SPEEXHIP_ERR_PTR_OVERLAP;
  ON_DEVICE();
  // what each side moves (payload) and the image the device call works on
  const size_t in_pitch = align64(frames), out_pitch = align64(most);
  const size_t in_payload = plane_in * in.channels, out_payload = plane_out * out.channels;
  // (channels that stand apart write different numbers of frames: the block is fetched whole and the caller handed only
  //  what each channel really wrote, so nothing is used in place there)
  const void *pin_in = nullptr;
  void *pin_out = nullptr;
  if (!split)
    pinned_sides(pl_in ? nullptr : in_flat.base, in_payload, pl_out ? nullptr : out_flat.base, out_payload, &pin_in, &pin_out);
  HostCallShape shape;
  shape.split = split;
  shape.in = pl_in ? planar_side(present, plane_in, in_pitch * bin, in.channels) : flat_side(present, pin_in != nullptr, in_payload);
  shape.out = pl_out ? planar_side(true, plane_out, out_pitch * bout, out.channels) : flat_side(true, pin_out != nullptr, out_payload);
  std::vector<HostPiece> pieces(1, HostPiece{in_flat.base, 0, in_payload});
  if (pl_in) pieces.resize(in.channels);
  for (uint32_t c = 0; pl_in && c < in.channels; c++) pieces[c] = {present ? host_plane(in, c) : nullptr, c * in_pitch * bin, plane_in};
  HostCall call(this);
  int rc = call.begin(route_host_call(shape), pieces.data(), static_cast<uint32_t>(pieces.size()), pin_in, pin_out);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  std::vector<CallPlan> plans;
  rc = process_sides_device(pl_in ? planes_at(in, call.src, in_pitch) : at(in, call.src), in_len,
                            pl_out ? planes_at(out, call.dst, out_pitch) : at(out, call.dst), out_len, own_stream_, &plans);
  if (!ran(rc)) return rc;
  // frames each channel of the result received (channels that stand apart produce different numbers of them)
  const std::vector<uint32_t> made = made_per_channel(out.channels, *out_len, split ? plans.data() : nullptr);
  int frc;
  if (pl_out) {
    frc = call.finish_planes(host_planes(out).data(), out.channels, out_pitch * bout, bout, made.data());
  } else if (split) {
    frc = call.finish_samples(out_flat.base, out.channels, out.channels, bout, made.data());
  } else {
    frc = call.finish_whole(out_flat.base, static_cast<size_t>(*out_len) * out.channels * bout);
  }
  return frc != SPEEXHIP_ERR_SUCCESS ? frc : rc;
}

}  // namespace speexhip
