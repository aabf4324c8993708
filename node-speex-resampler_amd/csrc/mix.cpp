// mix.cpp -- the mixed calls of engine.h: a formatted call whose sides may carry a channel matrix.  The state's channel
// count C is what the FIR runs on; the caller's input frames hold in_channels samples, its output frames out_channels:
// storage --mix_in (or convert_in)--> float image of C channels --the existing float launch--> float image of C
// channels --mix_out (or convert_out)--> storage.  A side with a matrix runs the mixing kernel (kernels_mix.hip)
// INSTEAD of the converting one, so a mixed call launches the float call's kernels plus at most one pass per side.
// Counters, positions and the history are the float call's for every format pair.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
inline size_t line_pitch(size_t elements) { return (elements + 63) & ~static_cast<size_t>(63); }
// a side of a mixed call: with a matrix both counts are 1..8, without one the caller's count is the state's
inline bool side_ok(const float *matrix, uint32_t caller_channels, uint32_t state_channels) {
  if (matrix == nullptr) return caller_channels == state_channels;
  return state_channels <= kMixMaxChannels && caller_channels >= 1 && caller_channels <= kMixMaxChannels;
}
}  // namespace

int Batch::process_mix_device(int in_fmt, uint32_t in_channels, const float *in_mix, const void *d_in, uint64_t in_stride,
                              uint32_t *in_len, int out_fmt, uint32_t out_channels, const float *out_mix, void *d_out,
                              uint64_t out_stride, uint32_t *out_len, hipStream_t stream) {
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0 || !side_ok(in_mix, in_channels, channels_) || !side_ok(out_mix, out_channels, channels_))
    return SPEEXHIP_ERR_INVALID_ARG;
  if (in_mix == nullptr && out_mix == nullptr)
    return process_fmt_device(in_fmt, d_in, in_stride, in_len, out_fmt, d_out, out_stride, out_len, stream);
  ON_DEVICE();
  // (channels that stand apart produce different numbers of frames: an output frame is not defined)
  for (uint32_t s = 0; s < n_streams_; s++)
    if (!uniform(s)) return SPEEXHIP_ERR_BAD_STATE;
  EntryRules rules;
  rules.block_in = block_in();
  rules.float_entry = true;
  // what the float call will do, known before anything is launched (integer arithmetic): sizes the images
  uint32_t most_in = 0, most_out = 0;
  for (uint32_t s = 0; s < n_streams_; s++) {
    most_in = std::max(most_in, in_len[s]);
    most_out = std::max(most_out, plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, 0), rules).produced);
  }
  // a side passes through an image unless it has no matrix and its storage IS the image (F32)
  const bool pass_in = (in_mix != nullptr || in_fmt != SPEEXHIP_FMT_F32) && d_in != nullptr && most_in != 0;
  const bool pass_out = out_mix != nullptr || out_fmt != SPEEXHIP_FMT_F32;
  const size_t in_pitch = line_pitch(static_cast<size_t>(most_in) * channels_);
  const size_t out_pitch = line_pitch(static_cast<size_t>(most_out) * channels_);
  int rc = ensure_planar_scratch(pass_in ? in_pitch * n_streams_ * sizeof(float) : 0,
                                 pass_out ? out_pitch * n_streams_ * sizeof(float) : 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  if (pass_in || (pass_out && most_out != 0)) {
    // (the images belong to the state: a call on another stream than the previous one waits for it first)
    rc = chain_to(stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (pass_in && in_mix == nullptr) {
    rc = convert_streams(true, in_fmt, d_in, in_stride * bin, d_planar_in_, in_pitch * sizeof(float), in_len, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  for (uint32_t s0 = 0; pass_in && in_mix != nullptr && s0 < n_streams_; s0 += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - s0);
    MixPack pack;
    std::memset(&pack, 0, sizeof(pack));
    pack.src_channels = in_channels, pack.dst_channels = channels_;
    std::memcpy(pack.m, in_mix, sizeof(float) * in_channels * channels_);
    uint32_t most = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t s = s0 + j;
      pack.s[j].src = static_cast<const char *>(d_in) + s * in_stride * bin;
      pack.s[j].dst = d_planar_in_ + s * in_pitch * sizeof(float);
      pack.s[j].frames = in_len[s];
      most = std::max(most, in_len[s]);
    }
    if (hip_failed(launch_mix_in(in_fmt, pack, n, most, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  }
  // (a present but empty input is not silence: no frame is read, any non-null address serves)
  const void *image_in = pass_in ? static_cast<const void *>(d_planar_in_) : d_in;
  const uint64_t image_in_stride = pass_in ? in_pitch : in_stride;
  void *image_out = pass_out ? static_cast<void *>(d_planar_out_) : d_out;
  const uint64_t image_out_stride = pass_out ? out_pitch : out_stride;
  rc = process_device(image_in, image_in_stride, in_len, image_out, image_out_stride, out_len, true, stream);
  if (rc != SPEEXHIP_ERR_SUCCESS && rc != SPEEXHIP_ERR_ALLOC_FAILED) return rc;
  // (out_len: what the float call produced; the zero fallback's zeros take the same way out)
  // With dither on (engine.h, set_dither) the integer formats leave through the dithered instances of either pass, at the
  // streams' positions, and every format counts the frames it produced.
  const bool dith = dither_on();
  // (every format but the two float ones: the integer formats and the companded ULAW / ALAW)
  const bool dith_out = dith && out_fmt != SPEEXHIP_FMT_F32 && out_fmt != SPEEXHIP_FMT_F32N;
  if (pass_out && out_mix == nullptr) {
    const int crc = convert_streams(false, out_fmt, d_planar_out_, out_pitch * sizeof(float), d_out, out_stride * bout, out_len,
                                    stream, dith_out);
    if (crc != SPEEXHIP_ERR_SUCCESS) return crc;
  }
  for (uint32_t s0 = 0; pass_out && out_mix != nullptr && s0 < n_streams_; s0 += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - s0);
    MixPack pack;
    std::memset(&pack, 0, sizeof(pack));
    pack.src_channels = channels_, pack.dst_channels = out_channels;
    std::memcpy(pack.m, out_mix, sizeof(float) * out_channels * channels_);
    uint32_t most = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t s = s0 + j;
      pack.s[j].src = d_planar_out_ + s * out_pitch * sizeof(float);
      pack.s[j].dst = static_cast<char *>(d_out) + s * out_stride * bout;
      pack.s[j].frames = out_len[s];
      most = std::max(most, out_len[s]);
    }
    const hipError_t e = dith_out ? launch_mix_out_dither(out_fmt, pack, dither_pack(s0, n, 1), n, most, stream)
                                  : launch_mix_out(out_fmt, pack, n, most, stream);
    if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  }
  if (dith) dither_advance(out_len);
  return rc;
}

// Host buffers: the raw bytes of both sides move as process_fmt_host moves them (routed_host_call, formats.cpp), with byte
// counts taken from the caller-side channel counts; the mixes and conversions run on the device.
int Batch::process_mix_host(int in_fmt, uint32_t in_channels, const float *in_mix, const void *in, uint32_t *in_len,
                            int out_fmt, uint32_t out_channels, const float *out_mix, void *out, uint32_t *out_len) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0 || out == nullptr || !side_ok(in_mix, in_channels, channels_) ||
      !side_ok(out_mix, out_channels, channels_))
    return SPEEXHIP_ERR_INVALID_ARG;
  if (in_mix == nullptr && out_mix == nullptr) return process_fmt_host(in_fmt, in, in_len, out_fmt, out, out_len);
  ON_DEVICE();
  if (!uniform(0)) return SPEEXHIP_ERR_BAD_STATE;
  const uint32_t frames = *in_len;
  // only as many output frames as this call can produce need a device buffer
  const uint32_t will_make = produced_closed_form(filter_.num, filter_.den, frames, *out_len, P(0, 0));
  const size_t in_bytes = static_cast<size_t>(frames) * in_channels * bin;
  const size_t out_bytes = static_cast<size_t>(will_make) * out_channels * bout;
  return routed_host_call(in, in_bytes, out, out_bytes, out_channels * bout, out_len, [&](const void *src, void *dst) {
    return process_mix_device(in_fmt, in_channels, in_mix, src, 0, in_len, out_fmt, out_channels, out_mix, dst, 0, out_len,
                              own_stream_);
  });
}

}  // namespace speexhip
