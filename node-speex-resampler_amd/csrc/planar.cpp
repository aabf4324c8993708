// planar.cpp -- the planar (one plane per channel) calls of engine.h.  A planar call is the interleaved call on the
// same frames: planes --gather--> interleaved scratch --the existing launch--> interleaved scratch --scatter-->
// planes (kernels_planar.hip).  The history stays the interleaved float `mem`, so interleaved, planar and per-channel
// calls mix freely on one state.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

// The interleaved images of a planar call: per state, grow-only, from the pool.  A grow waits for the state's own last
// call (which may still read the old image) and for nothing else.
int Batch::ensure_planar_scratch(size_t in_bytes, size_t out_bytes) {
  if (in_bytes <= planar_in_cap_ && out_bytes <= planar_out_cap_) return SPEEXHIP_ERR_SUCCESS;
  const int rc = quiesce();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const int rc_in = grow_stage(device_, &d_planar_in_, &planar_in_cap_, in_bytes, false);
  return rc_in != SPEEXHIP_ERR_SUCCESS ? rc_in : grow_stage(device_, &d_planar_out_, &planar_out_cap_, out_bytes, false);
}

int Batch::process_planar_device(const void *d_in, uint64_t in_stream_stride, uint64_t in_plane_stride, uint32_t *in_len,
                                 void *d_out, uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len,
                                 bool float_io, hipStream_t stream) {
  if (!lengths_fit(in_len, out_len, n_streams_)) return SPEEXHIP_ERR_OVERFLOW;  // (engine.h; nothing touched)
  // a mono plane is an interleaved buffer
  if (channels_ == 1) return process_device(d_in, in_stream_stride, in_len, d_out, out_stream_stride, out_len, float_io, stream);
  ON_DEVICE();
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const EntryRules rules = entry_rules(float_io);
  // channels that the per-channel calls moved apart: process_split with plane c as a stride-1 buffer
  const SplitLayout planes = {in_plane_stride, out_plane_stride, 1, 1};
  for (uint32_t s = 0; s < n_streams_; s++)
    if (!uniform(s)) {
      if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
      return process_split(d_in, in_len, d_out, out_len, float_io, stream, nullptr, &planes);
    }
  // Zero-fallback mode (the last filter change ran out of memory): the interleaved call needs no allocation there, so
  // neither may this one -- channel by channel straight on the planes, no scratch (the channels stand together, so
  // every channel reports the same lengths).  A batch has no such route and keeps the scratch images.
  if (zero_mode_ && n_streams_ == 1) return process_split(d_in, in_len, d_out, out_len, float_io, stream, nullptr, &planes);
  // planned exactly as process_device plans: `produced` is integer arithmetic, known before anything is launched
  std::vector<CallPlan> plans(n_streams_);
  std::vector<uint32_t> produced(n_streams_);
  uint32_t most_in = 0, most_out = 0;
  for (uint32_t s = 0; s < n_streams_; s++) {
    plans[s] = plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, 0), rules);
    produced[s] = plans[s].produced;
    most_in = std::max(most_in, in_len[s]);
    most_out = std::max(most_out, plans[s].produced);
  }
  // the scratch images: one stream after the other, whole 128-byte lines each, sized from what this call moves (never
  // from the capacities)
  const size_t in_pitch = align64(static_cast<size_t>(most_in) * channels_);
  const size_t out_pitch = align64(static_cast<size_t>(most_out) * channels_);
  int rc = ensure_planar_scratch(in_pitch * n_streams_ * es, out_pitch * n_streams_ * es);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t s = 0; s < n_streams_; s++)
    if (in_len[s] != 0 && out_len[s] != 0) started_[s] = 1;  // resample.c:886

  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  const bool gathers = d_in != nullptr && most_in != 0, scatters = most_out != 0;
  if (gathers || scatters) {
    // (the images belong to the state: a call on another stream than the previous one waits for it first, as the
    //  launch itself would)
    rc = chain_to(stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  // the transposing launches, <= kMaxPackedStreams streams each: planes -> image (gather) or image -> planes
  auto transpose = [&](bool gather, const void *planes, uint64_t stream_stride, uint64_t plane_stride, char *image, size_t pitch,
                       const uint32_t *frames) -> int {
    for (uint32_t s0 = 0; s0 < n_streams_; s0 += kChunk) {
      const uint32_t n = std::min(kChunk, n_streams_ - s0);
      PlanarPack pack;
      std::memset(&pack, 0, sizeof(pack));
      uint32_t most = 0;
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t s = s0 + j;
        pack.s[j].planes = static_cast<const char *>(planes) + s * stream_stride * es;
        pack.s[j].plane_stride = plane_stride;
        pack.s[j].inter = image + s * pitch * es;
        pack.s[j].frames = frames[s];
        most = std::max(most, pack.s[j].frames);
      }
      const hipError_t e = gather ? launch_planar_gather(pack, n, channels_, most, float_io, stream)
                                  : launch_planar_scatter(pack, n, channels_, most, float_io, stream);
      if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
    }
    return SPEEXHIP_ERR_SUCCESS;
  };
  if (gathers) {
    rc = transpose(true, d_in, in_stream_stride, in_plane_stride, d_planar_in_, in_pitch, in_len);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  // (a present but empty input is not silence: no frame is read, any non-null address serves)
  const void *image_in = d_in == nullptr ? nullptr : d_planar_in_ != nullptr ? static_cast<const void *>(d_planar_in_) : d_in;
  rc = run_plans(image_in, in_pitch, in_len, d_planar_out_, out_pitch, plans.data(), float_io, stream);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (scatters) {
    rc = transpose(false, d_out, out_stream_stride, out_plane_stride, d_planar_out_, out_pitch, produced.data());
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  for (uint32_t s = 0; s < n_streams_; s++) {
    in_len[s] = plans[s].consumed;
    out_len[s] = plans[s].produced;
  }
  return zero_mode_ ? SPEEXHIP_ERR_ALLOC_FAILED : SPEEXHIP_ERR_SUCCESS;
}

// Host planes: every plane moves by the routing rule of host_transfer.h into a planar image (pinned or on the device),
// the device call runs on the images, the result planes move out.  All planes of a side have one size, so one route
// serves the side.  (A plane in pinned memory is copied like a pageable one: the transposing kernels address planes as
// base + c * stride, and separate host planes have no common stride.)
int Batch::process_planar_host(const void *const *in_planes, uint32_t *in_len, void *const *out_planes, uint32_t *out_len,
                               bool float_io) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (out_planes == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const uint32_t frames = *in_len, capacity = *out_len;
  for (uint32_t c = 0; c < channels_; c++)
    if (out_planes[c] == nullptr || (in_planes != nullptr && in_planes[c] == nullptr)) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  // only as many output frames as this call can produce are written (and need a device buffer)
  const bool split = !uniform(0);
  const uint32_t most = will_make(frames, capacity);
  for (uint32_t c = 0; c < channels_; c++) {
    for (uint32_t k = 0; k < c; k++)
      if (buffers_overlap(out_planes[c], most * es, out_planes[k], most * es)) return SPEEXHIP_ERR_PTR_OVERLAP;
    for (uint32_t k = 0; in_planes != nullptr && k < channels_; k++)
      if (buffers_overlap(out_planes[c], most * es, in_planes[k], frames * es)) return SPEEXHIP_ERR_PTR_OVERLAP;
  }
  if (channels_ == 1) return process_host(in_planes ? in_planes[0] : nullptr, in_len, out_planes[0], out_len, float_io);
  ON_DEVICE();
  const size_t in_pitch = align64(frames), out_pitch = align64(most);  // elements between two planes: whole lines
  const size_t plane_in = frames * es, plane_out = most * es;
  const bool present = in_planes != nullptr;
  HostCallShape shape;
  shape.split = split;
  shape.in = planar_side(present, plane_in, in_pitch * es, channels_);
  shape.out = planar_side(true, plane_out, out_pitch * es, channels_);
  std::vector<HostPiece> pieces(channels_);
  for (uint32_t c = 0; c < channels_; c++) pieces[c] = {present ? in_planes[c] : nullptr, c * in_pitch * es, plane_in};
  HostCall call(this);
  int rc = call.begin(route_host_call(shape), pieces.data(), channels_, nullptr, nullptr);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  std::vector<CallPlan> plans;
  const SplitLayout image_planes = {in_pitch, out_pitch, 1, 1};
  if (split)
    rc = process_split(call.src, in_len, call.dst, out_len, float_io, own_stream_, &plans, &image_planes);
  else
    rc = process_planar_device(call.src, 0, in_pitch, in_len, call.dst, 0, out_pitch, out_len, float_io, own_stream_);
  if (!ran(rc)) return rc;
  // frames each plane received (channels that stand apart produce different numbers of them)
  const std::vector<uint32_t> made = made_per_channel(channels_, *out_len, split ? plans.data() : nullptr);
  const int frc = call.finish_planes(out_planes, channels_, out_pitch * es, es, made.data());
  return frc != SPEEXHIP_ERR_SUCCESS ? frc : rc;
}

}  // namespace speexhip
