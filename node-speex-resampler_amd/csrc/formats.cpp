// formats.cpp -- the formatted calls of engine.h: the caller names the sample format of the input and of the output
// (SPEEXHIP_FMT_*).  A formatted call is the float call on the converted input followed by the output conversion:
// storage --convert_in--> float scratch image --the existing float launch--> float scratch image --convert_out-->
// storage (kernels_convert.hip).  Counters, positions and the history are the float call's, so formatted, interleaved,
// planar and per-channel calls mix freely on one state.
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "dither.h"
#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
inline size_t line_pitch(size_t elements) { return (elements + 63) & ~static_cast<size_t>(63); }
inline size_t fmt_bytes(int fmt) {
  switch (fmt) {
    case SPEEXHIP_FMT_U8:
    case SPEEXHIP_FMT_ULAW:
    case SPEEXHIP_FMT_ALAW: return 1;
    case SPEEXHIP_FMT_S16: return 2;
    case SPEEXHIP_FMT_S24: return 3;
    case SPEEXHIP_FMT_S32:
    case SPEEXHIP_FMT_F32:
    case SPEEXHIP_FMT_F32N: return 4;
    default: return 0;
  }
}
// the pairs that are an existing call on the same bytes: nothing is converted, nothing extra launched
inline bool same_bytes_pair(int in_fmt, int out_fmt) {
  return in_fmt == out_fmt && (in_fmt == SPEEXHIP_FMT_S16 || in_fmt == SPEEXHIP_FMT_F32 || in_fmt == SPEEXHIP_FMT_F32N);
}
// (the companded formats quantise to int16 on their way out: dithered like the integer ones)
inline bool integer_fmt(int fmt) {
  return fmt == SPEEXHIP_FMT_U8 || fmt == SPEEXHIP_FMT_S16 || fmt == SPEEXHIP_FMT_S24 || fmt == SPEEXHIP_FMT_S32 ||
         fmt == SPEEXHIP_FMT_ULAW || fmt == SPEEXHIP_FMT_ALAW;
}
}  // namespace

// ---- dither (engine.h) -------------------------------------------------------------------------------------------------
int Batch::set_dither(int kind, uint64_t seed, uint64_t position) {
  if (!dither::known_kind(kind)) return SPEEXHIP_ERR_INVALID_ARG;
  dither_kind_ = kind;
  dither_seed_ = seed;
  dither_pos_.assign(n_streams_, position);
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

// The converting pass of a side without a matrix over every stream of the batch, <= 32 streams per launch: stream s is
// lens[s] frames of channels() samples at src + s * src_step and dst + s * dst_step (bytes).  to_image: convert_in (storage
// -> float image), otherwise convert_out.  Shared with the mixed calls (mix.cpp).
int Batch::convert_streams(bool to_image, int fmt, const void *src, size_t src_step, void *dst, size_t dst_step,
                           const uint32_t *lens, hipStream_t stream, bool dithered) {
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  for (uint32_t s0 = 0; s0 < n_streams_; s0 += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - s0);
    ConvertPack pack;
    std::memset(&pack, 0, sizeof(pack));
    uint64_t most = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t s = s0 + j;
      pack.s[j].src = static_cast<const char *>(src) + s * src_step;
      pack.s[j].dst = static_cast<char *>(dst) + s * dst_step;
      pack.s[j].n = static_cast<uint64_t>(lens[s]) * channels_;
      pack.s[j].step = 1;
      most = std::max(most, pack.s[j].n);
    }
    const hipError_t e = to_image   ? launch_convert_in(fmt, pack, n, most, stream)
                         : dithered ? launch_convert_out_dither(fmt, pack, dither_pack(s0, n, channels_), n, most, stream)
                                    : launch_convert_out(fmt, pack, n, most, stream);
    if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::process_fmt_device(int in_fmt, const void *d_in, uint64_t in_stride, uint32_t *in_len, int out_fmt, void *d_out,
                              uint64_t out_stride, uint32_t *out_len, hipStream_t stream, std::vector<CallPlan> *plans_out) {
  const size_t bin = fmt_bytes(in_fmt), bout = fmt_bytes(out_fmt);
  if (bin == 0 || bout == 0) return SPEEXHIP_ERR_INVALID_ARG;
  ON_DEVICE();
  EntryRules rules;
  rules.block_in = block_in();
  bool split = false;
  const bool dith = dither_on();
  for (uint32_t s = 0; s < n_streams_; s++)
    if (!uniform(s)) {
      // (with dither on: channels that stand apart produce different numbers of frames, a position is not defined)
      if (n_streams_ != 1 || dith) return SPEEXHIP_ERR_BAD_STATE;
      split = true;
    }
  // (F32N -> F32N: a power-of-two scale commutes exactly with the FIR, so the float call on the same bytes)
  // With dither on S16 -> S16 is no such pair -- it runs as the float call between convert_in and the dithered
  // convert_out -- and the float pairs, written as ever, still count their frames.
  if (same_bytes_pair(in_fmt, out_fmt) && !(dith && in_fmt == SPEEXHIP_FMT_S16)) {
    const int rc = process_device(d_in, in_stride, in_len, d_out, out_stride, out_len, in_fmt != SPEEXHIP_FMT_S16, stream);
    if (dith && (rc == SPEEXHIP_ERR_SUCCESS || rc == SPEEXHIP_ERR_ALLOC_FAILED)) dither_advance(out_len);
    return rc;
  }
  rules.float_entry = true;
  // what the float call will do, known before anything is launched (integer arithmetic): sizes the images
  uint32_t most_in = 0, most_out = 0;
  for (uint32_t s = 0; s < n_streams_; s++) {
    most_in = std::max(most_in, in_len[s]);
    for (uint32_t c = 0; c < (split ? channels_ : 1u); c++)
      most_out = std::max(most_out, plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, c), rules).produced);
  }
  const bool conv_in = in_fmt != SPEEXHIP_FMT_F32 && d_in != nullptr && most_in != 0;
  const bool conv_out = out_fmt != SPEEXHIP_FMT_F32;
  // The float images: one stream after the other, sized from what this call moves.  (The zero fallback goes through them
  // as well: its history still takes the converted input, and its silence is whatever the float call writes, converted.)
  const size_t in_pitch = line_pitch(static_cast<size_t>(most_in) * channels_);
  const size_t out_pitch = line_pitch(static_cast<size_t>(most_out) * channels_);
  int rc = ensure_planar_scratch(conv_in ? in_pitch * n_streams_ * sizeof(float) : 0,
                                 conv_out ? out_pitch * n_streams_ * sizeof(float) : 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  if (conv_in || (conv_out && most_out != 0)) {
    // (the images belong to the state: a call on another stream than the previous one waits for it first)
    rc = chain_to(stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (conv_in) {
    rc = convert_streams(true, in_fmt, d_in, in_stride * bin, d_planar_in_, in_pitch * sizeof(float), in_len, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  // (a present but empty input is not silence: no frame is read, any non-null address serves)
  const void *image_in = conv_in ? static_cast<const void *>(d_planar_in_) : d_in;
  const uint64_t image_in_stride = conv_in ? in_pitch : in_stride;
  void *image_out = conv_out ? static_cast<void *>(d_planar_out_) : d_out;
  const uint64_t image_out_stride = conv_out ? out_pitch : out_stride;
  std::vector<CallPlan> plans;  // of the channels of a state whose channels stand apart
  if (split)
    rc = process_split(image_in, in_len, image_out, out_len, true, stream, &plans);
  else
    rc = process_device(image_in, image_in_stride, in_len, image_out, image_out_stride, out_len, true, stream);
  if (rc != SPEEXHIP_ERR_SUCCESS && rc != SPEEXHIP_ERR_ALLOC_FAILED) return rc;
  if (plans_out != nullptr) *plans_out = plans;
  if (conv_out && split) {
    // channel c wrote plans[c].produced frames: each channel is a strided stream of the converting launch
    for (uint32_t c0 = 0; c0 < channels_; c0 += kChunk) {
      const uint32_t n = std::min(kChunk, channels_ - c0);
      ConvertPack pack;
      std::memset(&pack, 0, sizeof(pack));
      uint64_t most = 0;
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t c = c0 + j;
        pack.s[j].src = d_planar_out_ + c * sizeof(float);
        pack.s[j].dst = static_cast<char *>(d_out) + c * bout;
        pack.s[j].n = plans[c].produced;
        pack.s[j].step = channels_;
        most = std::max(most, pack.s[j].n);
      }
      if (hip_failed(launch_convert_out(out_fmt, pack, n, most, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
    }
  }
  if (conv_out && !split) {
    // (out_len: what the float call produced)
    const int crc = convert_streams(false, out_fmt, d_planar_out_, out_pitch * sizeof(float), d_out, out_stride * bout, out_len,
                                    stream, dith && integer_fmt(out_fmt));
    if (crc != SPEEXHIP_ERR_SUCCESS) return crc;
  }
  if (dith) dither_advance(out_len);
  return rc;
}

// A single-stream call on host buffers around a device call: the raw bytes of both sides move by the rule of
// host_transfer.h -- in place when pinned, through the bounce buffers when small, by the runtime's staged copy when large.
// device_call(src, dst) enqueues the work on own_stream_ and sets *out_len to the frames produced, out_frame_bytes each.
// Shared by the formatted and the mixed host calls.
int Batch::routed_host_call(const void *in, size_t in_bytes, void *out, size_t out_bytes, size_t out_frame_bytes,
                            const uint32_t *out_len, const std::function<int(const void *, void *)> &device_call) {
  int rc = SPEEXHIP_ERR_SUCCESS;
  DrainOnExit drain(&own_stream_);
  const void *pin_in = in != nullptr ? pinned_view_of(in, in_bytes) : nullptr;
  void *pin_out = pinned_view_of(out, out_bytes);
  if (pin_in != nullptr && pin_out != nullptr && buffers_overlap(in, in_bytes, out, out_bytes)) pin_in = nullptr;
  const bool small = small_call(in != nullptr && pin_in == nullptr ? in_bytes : 0, pin_out == nullptr ? out_bytes : 0);
  const Via in_via = route_side(in_bytes, in != nullptr, pin_in != nullptr, small);
  const Via out_via = route_side(out_bytes, true, pin_out != nullptr, small);
  Wait wait;
  wait.add(in_via, in_bytes);
  wait.add(out_via, out_bytes);
  rc = ensure_stage(device_part(in_via, in_bytes), device_part(out_via, out_bytes), pinned_part(in_via, in_bytes),
                    pinned_part(out_via, out_bytes) + (wait.sync ? 0 : 64));
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const void *src = nullptr;
  rc = stage_input(in_via, in, in_bytes, pin_in, &src);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (src == nullptr && in != nullptr) src = h_pin_out_;  // (an empty chunk, not silence)
  void *dst = out_via == Via::InPlace ? pin_out : out_via == Via::Bounce ? static_cast<void *>(h_pin_out_) : static_cast<void *>(d_stage_out_);
  rc = device_call(src, dst);
  if (rc != SPEEXHIP_ERR_SUCCESS && rc != SPEEXHIP_ERR_ALLOC_FAILED) return rc;
  const size_t made = static_cast<size_t>(*out_len) * out_frame_bytes;
  if (device_part(out_via, made) != 0)
    HIP_TRY(hipMemcpyAsync(out_via == Via::Copy ? out : h_pin_out_, d_stage_out_, made, hipMemcpyDeviceToHost, own_stream_));
  const int wrc = wait_call(own_stream_, wait, tail_word(h_pin_out_, pin_out_cap_), ++done_seq_);
  if (wrc != SPEEXHIP_ERR_SUCCESS) return wrc;
  drain.armed = false;
  if (pinned_part(out_via, made) != 0) std::memcpy(out, h_pin_out_, made);
  return rc;
}

// Host buffers: the raw bytes of both sides move exactly as process_host moves samples -- in place when pinned, through
// the bounce buffers when small, by the runtime's staged copy when large -- and the conversions run on the device.
int Batch::process_fmt_host(int in_fmt, const void *in, uint32_t *in_len, int out_fmt, void *out, uint32_t *out_len) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  const size_t bin = fmt_bytes(in_fmt), bout = fmt_bytes(out_fmt);
  if (bin == 0 || bout == 0 || out == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const bool dith = dither_on();
  const bool split = !uniform(0);
  if (dith && split) return SPEEXHIP_ERR_BAD_STATE;
  if (same_bytes_pair(in_fmt, out_fmt) && !(dith && in_fmt == SPEEXHIP_FMT_S16)) {
    const int rc = process_host(in, in_len, out, out_len, in_fmt != SPEEXHIP_FMT_S16);
    if (dith && (rc == SPEEXHIP_ERR_SUCCESS || rc == SPEEXHIP_ERR_ALLOC_FAILED)) dither_advance(out_len);
    return rc;
  }
  ON_DEVICE();
  const uint32_t frames = *in_len;
  uint32_t will_make = 0;  // only as many output frames as this call can produce need a device buffer
  for (uint32_t c = 0; c < (split ? channels_ : 1u); c++)
    will_make = std::max(will_make, produced_closed_form(filter_.num, filter_.den, frames, *out_len, P(0, c)));
  const size_t in_bytes = static_cast<size_t>(frames) * channels_ * bin;
  const size_t out_bytes = static_cast<size_t>(will_make) * channels_ * bout;
  if (split) {
    int rc = SPEEXHIP_ERR_SUCCESS;
    DrainOnExit drain(&own_stream_);
    std::vector<CallPlan> plans;
    // channels at different positions write different numbers of frames: fetch the whole block and hand the caller
    // only the samples each channel really wrote (as process_host does)
    const Via in_via = route_side(in_bytes, in != nullptr, false, false);
    rc = ensure_stage(in_bytes, out_bytes, pinned_part(in_via, in_bytes), out_bytes);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    const void *src = nullptr;
    rc = stage_input(in_via, in, in_bytes, nullptr, &src);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    if (src == nullptr && in != nullptr) src = h_pin_out_;
    rc = process_fmt_device(in_fmt, src, 0, in_len, out_fmt, d_stage_out_, 0, out_len, own_stream_, &plans);
    if (rc != SPEEXHIP_ERR_SUCCESS && rc != SPEEXHIP_ERR_ALLOC_FAILED) return rc;
    uint32_t most = 0;
    for (const CallPlan &pl : plans) most = std::max(most, pl.produced);
    const size_t bytes = static_cast<size_t>(most) * channels_ * bout;
    if (bytes != 0) HIP_TRY(hipMemcpyAsync(h_pin_out_, d_stage_out_, bytes, hipMemcpyDeviceToHost, own_stream_));
    HIP_TRY(hipStreamSynchronize(own_stream_));
    drain.armed = false;
    for (uint32_t c = 0; c < channels_; c++)
      for (uint32_t j = 0; j < plans[c].produced; j++)
        std::memcpy(static_cast<char *>(out) + (static_cast<size_t>(j) * channels_ + c) * bout,
                    h_pin_out_ + (static_cast<size_t>(j) * channels_ + c) * bout, bout);
    return rc;
  }
  return routed_host_call(in, in_bytes, out, out_bytes, channels_ * bout, out_len, [&](const void *src, void *dst) {
    return process_fmt_device(in_fmt, src, 0, in_len, out_fmt, dst, 0, out_len, own_stream_);
  });
}

}  // namespace speexhip
