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
inline bool planar(const CallSide &side) { return side_planar(side); }
// The calls that are an existing call on the same bytes: nothing is converted, nothing extra launched.  (F32N -> F32N: a
// power-of-two scale commutes exactly with the FIR.)  With dither on S16 -> S16 is no such call -- it runs as the float
// call between convert_in and the dithered convert_out -- and the float pairs, written as ever, still count their frames.
inline bool same_bytes(const CallSide &in, const CallSide &out, bool dith) {
  if (in.mix != nullptr || out.mix != nullptr || in.fmt != out.fmt || planar(in) || planar(out)) return false;
  return in.fmt == SPEEXHIP_FMT_S16 ? !dith : in.fmt == SPEEXHIP_FMT_F32 || in.fmt == SPEEXHIP_FMT_F32N;
}
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
// Both sides planar, the same float format, no matrix: the planar float call on the same bytes (F32N: a power-of-two scale
// commutes exactly with the FIR).
inline bool planar_float_call(const CallSide &in, const CallSide &out) {
  return planar(in) && planar(out) && in.mix == nullptr && out.mix == nullptr && in.fmt == out.fmt &&
         (in.fmt == SPEEXHIP_FMT_F32 || in.fmt == SPEEXHIP_FMT_F32N);
}
// plane c of a host side
inline char *host_plane(const CallSide &side, uint32_t c) {
  return side.planes != nullptr ? static_cast<char *>(side.planes[c])
                                : static_cast<char *>(side.base) + c * side.plane_stride * sample_bytes(side.fmt);
}
}  // namespace

// ---- dither (engine.h) -------------------------------------------------------------------------------------------------
int Batch::set_dither(int kind, uint64_t seed, uint64_t position) {
  if (!dither::known_kind(kind)) return SPEEXHIP_ERR_INVALID_ARG;
  dither_kind_ = kind;
  dither_seed_ = seed;
  dither_pos_.assign(n_streams_, position);
  bus_pos_ = position;  // (the buses' one position: bus.cpp)
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

int Batch::process_sides_device(const CallSide &in_side, uint32_t *in_len, const CallSide &out_side, uint32_t *out_len,
                                hipStream_t stream, std::vector<CallPlan> *plans_out) {
  if (!side_ok(in_side, channels_) || !side_ok(out_side, channels_)) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, n_streams_)) return SPEEXHIP_ERR_OVERFLOW;  // (engine.h; nothing touched)
  // (a side of one channel is the same bytes in either layout)
  CallSide in = in_side, out = out_side;
  if (!planar(in)) in.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  if (!planar(out)) out.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  ON_DEVICE();
  const bool mixed = in.mix != nullptr || out.mix != nullptr, dith = dither_on(), gained = gain_on();
  // (what the meter asks of the routes below a gained stream asks too: no shortcut past the output side)
  const bool meter = meter_on_ || gained;
  bool split = false;
  for (uint32_t s = 0; s < n_streams_; s++)
    if (!uniform(s)) {
      // (channels that stand apart produce different numbers of frames: neither an output frame of a matrix nor a dither
      //  position nor a stream of samples to meter nor a frame index of a gain is defined)
      if (n_streams_ != 1 || dith || mixed || meter) return SPEEXHIP_ERR_BAD_STATE;
      split = true;
    }
  if (same_bytes(in, out, dith || meter)) {
    // (with the meter on: F32 or F32N, the float call's bytes as ever, read once more by meter_image; with gain on:
    //  multiplied in place by gain_image, an F32N result as stored, and judged in that same pass)
    const int rc = process_device(in.base, in.stride, in_len, out.base, out.stride, out_len, in.fmt != SPEEXHIP_FMT_S16, stream);
    if (meter && ran(rc)) {
      const int mrc = image_result(out.base, out.stride, out_len, in.fmt == SPEEXHIP_FMT_F32N ? 32768.0f : 1.0f, stream);
      if (mrc != SPEEXHIP_ERR_SUCCESS) return mrc;
      if (meter_on_) meter_count(out_len, channels_);
      if (gained) gain_advance(out_len);
    }
    if (dith && ran(rc)) dither_advance(out_len);
    return rc;
  }
  // (with the meter on the planar float pairs run between planes_in and the metered planes_out)
  if (planar_float_call(in, out) && !split && !meter) {
    const int rc = process_planar_device(in.base, in.stride, in.plane_stride, in_len, out.base, out.stride, out.plane_stride,
                                         out_len, true, stream);
    if (dith && ran(rc)) dither_advance(out_len);
    return rc;
  }
  const EntryRules rules = entry_rules(true);
  // what the float call will do, known before anything is launched (integer arithmetic): sizes the images
  uint32_t most_in = 0, most_out = 0;
  for (uint32_t s = 0; s < n_streams_; s++) {
    most_in = std::max(most_in, in_len[s]);
    for (uint32_t c = 0; c < (split ? channels_ : 1u); c++)
      most_out = std::max(most_out, plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, c), rules).produced);
  }
  // a side passes through an image unless it has no matrix and its storage IS the image (interleaved F32); a present but
  // empty input is not silence: no frame is read, any non-null address serves
  const bool pass_in = (in.mix != nullptr || in.fmt != SPEEXHIP_FMT_F32 || planar(in)) && in.base != nullptr && most_in != 0;
  const bool pass_out = out.mix != nullptr || out.fmt != SPEEXHIP_FMT_F32 || planar(out);
  // The float images: one stream after the other, whole 128-byte lines each, sized from what this call moves.  (The zero
  // fallback goes through them as well: its history still takes the converted input, and its silence is whatever the
  // float call writes, converted -- and dithered.)
  const size_t in_pitch = align64(static_cast<size_t>(most_in) * channels_);
  const size_t out_pitch = align64(static_cast<size_t>(most_out) * channels_);
  int rc = ensure_planar_scratch(pass_in ? in_pitch * n_streams_ * sizeof(float) : 0,
                                 pass_out ? out_pitch * n_streams_ * sizeof(float) : 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (pass_in || (pass_out && most_out != 0)) {
    // (the images belong to the state: a call on another stream than the previous one waits for it first)
    rc = chain_to(stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (pass_in) {
    rc = side_pass(in, true, d_planar_in_, in_pitch, in_len, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  const void *image_in = pass_in ? static_cast<const void *>(d_planar_in_) : in.base;
  void *image_out = pass_out ? static_cast<void *>(d_planar_out_) : out.base;
  std::vector<CallPlan> plans;  // of the channels of a state whose channels stand apart
  if (split)
    rc = process_split(image_in, in_len, image_out, out_len, true, stream, &plans);
  else
    rc = process_device(image_in, pass_in ? in_pitch : in.stride, in_len, image_out, pass_out ? out_pitch : out.stride, out_len,
                        true, stream);
  if (!ran(rc)) return rc;
  if (plans_out != nullptr) *plans_out = plans;
  if (pass_out) {
    // (out_len: what the float call produced)
    const int prc = side_pass(out, false, d_planar_out_, out_pitch, out_len, stream, split ? plans.data() : nullptr);
    if (prc != SPEEXHIP_ERR_SUCCESS) return prc;
  } else if (meter) {
    // (interleaved F32 without a matrix: the FIR wrote the caller's buffer)
    const int mrc = image_result(out.base, out.stride, out_len, 1.0f, stream);
    if (mrc != SPEEXHIP_ERR_SUCCESS) return mrc;
  }
  if (meter_on_) meter_count(out_len, out.channels);
  if (gained) gain_advance(out_len);
  if (dith) dither_advance(out_len);
  return rc;
}

// The formatted many-states call (engine.h): which entries a launch group can serve and as what -- the rules of
// process_sides_host above, entry by entry -- then many_run (many.cpp).
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
    // fused: both sides interleaved (or of one channel) in one buffer each, no matrix
    e.fusable = !planar(in[i]) && !planar(out[i]) && in[i].mix == nullptr && out[i].mix == nullptr && in[i].planes == nullptr &&
                out[i].planes == nullptr;
    // (a metered result that no pass of kernels_convert_many.hip writes -- F32, or the float call on the same bytes --
    //  takes its own call, which runs meter_image behind it)
    if (b->meter_on_ && (out[i].fmt == SPEEXHIP_FMT_F32 || (in[i].fmt == out[i].fmt && out[i].fmt == SPEEXHIP_FMT_F32N)))
      e.fusable = false;
    if (!e.fusable) continue;
    e.in = in[i].base;
    e.out = out[i].base;
    // (a gained entry stays fused: S16 -> S16 between its two passes, a float result multiplied by gain_image in the group)
    e.kind = !same_bytes(in[i], out[i], b->dither_on() || b->meter_on_ || b->gain_on()) ? ManyEntry::Image
             : in[i].fmt == SPEEXHIP_FMT_S16            ? ManyEntry::Int16
                                                        : ManyEntry::Float;
  }
  return many_run(n, entries.data(), in_len, out_len, codes);
}

// process_sides_device on own_stream_ around a single-stream call's host buffers: the raw bytes of both sides move by the
// rule of host_transfer.h -- in place when pinned, through the bounce buffers when small, by the runtime's staged copy when
// large; channels that stand apart as in process_host.
int Batch::process_sides_host(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (!side_ok(in, channels_) || !side_ok(out, channels_)) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  if (planar(in) || planar(out)) return planes_host_call(in, in_len, out, out_len);
  // (a mono side given as its one plane)
  if (in.planes != nullptr || out.planes != nullptr) {
    if ((in.planes != nullptr && in.planes[0] == nullptr) || (out.planes != nullptr && out.planes[0] == nullptr))
      return SPEEXHIP_ERR_INVALID_ARG;
    CallSide in1 = in, out1 = out;
    if (in.planes != nullptr) in1.base = in.planes[0], in1.planes = nullptr;
    if (out.planes != nullptr) out1.base = out.planes[0], out1.planes = nullptr;
    return process_sides_host(in1, in_len, out1, out_len);
  }
  if (out.base == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const bool mixed = in.mix != nullptr || out.mix != nullptr, dith = dither_on(), split = !uniform(0);
  const bool gained = gain_on();
  if (split && (dith || meter_on_ || gained) && !mixed) return SPEEXHIP_ERR_BAD_STATE;
  // (with the meter or gain on the float pairs go on below: process_sides_device runs meter_image or gain_image behind the
  //  float call)
  if (same_bytes(in, out, dith) && !meter_on_ && !gained) {
    const int rc = process_host(in.base, in_len, out.base, out_len, in.fmt != SPEEXHIP_FMT_S16);
    if (dith && ran(rc)) dither_advance(out_len);
    return rc;
  }
  ON_DEVICE();
  if (split && mixed) return SPEEXHIP_ERR_BAD_STATE;
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
  const bool pl_in = planar(in), pl_out = planar(out_side);
  // (a mono side given as its one plane is an interleaved buffer)
  CallSide out = out_side;
  if (!pl_out && out.planes != nullptr) out.base = out.planes[0], out.planes = nullptr;
  if (out.base == nullptr && out.planes == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t c = 0; out.planes != nullptr && c < out.channels; c++)
    if (out.planes[c] == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  // entries of in_data per chunk; a present chunk has all its planes
  const uint32_t per = pl_in ? in.channels : 1u;
  const auto entry = [&](uint32_t i, uint32_t c) { return in_data != nullptr ? in_data[static_cast<size_t>(i) * per + c] : nullptr; };
  for (uint32_t i = 0; i < n_chunks; i++)
    for (uint32_t c = 1; entry(i, 0) != nullptr && c < per; c++)
      if (entry(i, c) == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const bool mixed = in.mix != nullptr || out.mix != nullptr, dith = dither_on(), gained = gain_on(), split = !uniform(0);
  const bool meter = meter_on_ || gained;  // (a gained stream asks of the routes what the meter asks)
  if (split && (dith || mixed || meter)) return SPEEXHIP_ERR_BAD_STATE;
  // same: the call on the same bytes; with the meter on (F32 or F32N then) it still goes through here, without passes,
  // and meter_image reads the result -- or gain_image multiplies it, once over all chunks: the ramp's index runs on
  // across the chunk boundaries as the dither's does
  const bool same = same_bytes(in, out, dith || meter), own_calls = split || zero_mode_;
  const size_t bin = sample_bytes(in.fmt), bout = sample_bytes(out.fmt);
  if (own_calls && (!same || meter)) {  // rare states: the separate calls, one after the other, each output side behind the frames written
    int last = SPEEXHIP_ERR_SUCCESS;
    uint64_t written = 0;
    std::vector<void *> planes(out.channels);
    for (uint32_t i = 0; i < n_chunks; i++) {
      CallSide a = in, b = out;
      a.base = const_cast<void *>(entry(i, 0));
      a.planes = nullptr;
      if (pl_in && a.base != nullptr) a.planes = const_cast<void *const *>(in_data + static_cast<size_t>(i) * per), a.base = nullptr;
      if (pl_out) {
        for (uint32_t c = 0; c < out.channels; c++) planes[c] = host_plane(out, c) + written * bout;
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
  const ChunkPlans p = plan_chunks(filter_.num, filter_.den, n_chunks, in_len, out_len, P(0, 0), entry_rules(!same || in.fmt != SPEEXHIP_FMT_S16));
  if (same && !meter) {  // process_host_chunks on the same bytes (which serves the rare states itself)
    const int rc = process_host_chunks(n_chunks, in_data, in_len, out.base, out_len, in.fmt != SPEEXHIP_FMT_S16);
    if (!ran(rc)) return rc;
    uint32_t made = 0;
    for (uint32_t i = 0; i < n_chunks; i++) made += out_len[i];
    if (dith) dither_advance(&made);
    if (own_calls) count_chunks(3, n_chunks);
    else count_chunks(0, p.launches);
    return rc;
  }
  if (p.frames > 0x7fffffffull || p.made > 0x7fffffffull) return SPEEXHIP_ERR_OVERFLOW;
  // (only so many frames are written to a plane: the sum of what the chunks will make)
  for (uint32_t c = 0; pl_out && c < out.channels; c++)
    for (uint32_t k = 0; k < c; k++)
      if (buffers_overlap(host_plane(out, c), p.made * bout, host_plane(out, k), p.made * bout)) return SPEEXHIP_ERR_PTR_OVERLAP;
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
  const bool pass_in = !same && (in.mix != nullptr || in.fmt != SPEEXHIP_FMT_F32 || pl_in) && frames != 0;
  const bool pass_out = !same && (out.mix != nullptr || out.fmt != SPEEXHIP_FMT_F32 || pl_out);
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
  } else if (meter) {
    rc = image_result(call.dst, 0, &made, out.fmt == SPEEXHIP_FMT_F32N ? 32768.0f : 1.0f, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (meter_on_) meter_count(&made, out.channels);
  if (gained) gain_advance(&made);
  if (dith) dither_advance(&made);
  if (pl_out) {
    std::vector<void *> planes(out.channels);
    for (uint32_t c = 0; c < out.channels; c++) planes[c] = host_plane(out, c);
    rc = call.finish_planes(planes.data(), out.channels, out_pitch * bout, bout, std::vector<uint32_t>(out.channels, made).data());
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
  const bool pl_in = planar(in), pl_out = planar(out);
  const bool mixed = in.mix != nullptr || out.mix != nullptr, dith = dither_on(), split = !uniform(0);
  if (split && (dith || mixed || meter_on_ || gain_on())) return SPEEXHIP_ERR_BAD_STATE;
  // (a mono side given as its one plane is an interleaved buffer)
  CallSide in_flat = in, out_flat = out;
  if ((!pl_in && in.planes != nullptr && in.planes[0] == nullptr) || (!pl_out && out.planes != nullptr && out.planes[0] == nullptr))
    return SPEEXHIP_ERR_INVALID_ARG;
  if (!pl_in && in.planes != nullptr) in_flat.base = in.planes[0];
  if (!pl_out && out.planes != nullptr) out_flat.base = out.planes[0];
  const bool present = pl_in ? in.planes != nullptr || in.base != nullptr : in_flat.base != nullptr;
  if (pl_out ? out.planes == nullptr && out.base == nullptr : out_flat.base == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t c = 0; pl_in && in.planes != nullptr && c < in.channels; c++)
    if (in.planes[c] == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t c = 0; pl_out && out.planes != nullptr && c < out.channels; c++)
    if (out.planes[c] == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const uint32_t frames = *in_len;
  const uint32_t most = will_make(frames, *out_len);  // only so many output frames are written (and need a device buffer)
  const size_t bin = sample_bytes(in.fmt), bout = sample_bytes(out.fmt);
  const size_t plane_in = frames * bin, plane_out = most * bout;
  for (uint32_t c = 0; pl_out && c < out.channels; c++) {
    for (uint32_t k = 0; k < c; k++)
      if (buffers_overlap(host_plane(out, c), plane_out, host_plane(out, k), plane_out)) return SPEEXHIP_ERR_PTR_OVERLAP;
    for (uint32_t k = 0; pl_in && present && k < in.channels; k++)
      if (buffers_overlap(host_plane(out, c), plane_out, host_plane(in, k), plane_in)) return SPEEXHIP_ERR_PTR_OVERLAP;
  }
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
    std::vector<void *> planes(out.channels);
    for (uint32_t c = 0; c < out.channels; c++) planes[c] = host_plane(out, c);
    frc = call.finish_planes(planes.data(), out.channels, out_pitch * bout, bout, made.data());
  } else if (split) {
    frc = call.finish_samples(out_flat.base, out.channels, out.channels, bout, made.data());
  } else {
    frc = call.finish_whole(out_flat.base, static_cast<size_t>(*out_len) * out.channels * bout);
  }
  return frc != SPEEXHIP_ERR_SUCCESS ? frc : rc;
}

}  // namespace speexhip
