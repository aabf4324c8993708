// host_call.cpp -- the mechanics of a single-state host-buffer call (engine.h, Batch::HostCall): the staging buffers, the
// input on its way in, the result on its way out, the wait and the hand-over, for every way route_host_call
// (host_transfer.h) can decide.  The entry points keep their argument checks and their device call; everything between the
// caller's memory and that call is here, once.
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
// n samples of es bytes, src_step samples apart, to places dst_step samples apart.  A long line spends all its host time
// here (2^20 frames: 3 ns per sample each way), so the common sample sizes get loops of their own with a fixed-size move.
template <size_t ES>
void copy_samples_of(char *dst, size_t dst_step, const char *src, size_t src_step, size_t n) {
  for (size_t j = 0; j < n; j++) std::memcpy(dst + j * dst_step * ES, src + j * src_step * ES, ES);
}
void copy_samples(char *dst, size_t dst_step, const char *src, size_t src_step, size_t n, size_t es) {
  if (es == 2) return copy_samples_of<2>(dst, dst_step, src, src_step, n);
  if (es == 4) return copy_samples_of<4>(dst, dst_step, src, src_step, n);
  for (size_t j = 0; j < n; j++) std::memcpy(dst + j * dst_step * es, src + j * src_step * es, es);
}
}  // namespace

// Staging buffers of the host-buffer calls (grow_stage), each taken only when a call needs it: small calls run on the
// pinned pair alone, large ones on the device pair alone (the runtime copies straight from / to the caller's memory).
int Batch::ensure_stage(size_t dev_in, size_t dev_out, size_t pin_in, size_t pin_out) {
  if (own_stream_ == nullptr) HIP_TRY(pool::stream_get(device_, &own_stream_));
  int rc = grow_stage(device_, &d_stage_in_, &stage_in_cap_, dev_in, false);
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = grow_stage(device_, &d_stage_out_, &stage_out_cap_, dev_out, false);
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = grow_stage(device_, &h_pin_in_, &pin_in_cap_, pin_in, true);
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = grow_stage(device_, &h_pin_out_, &pin_out_cap_, pin_out, true);
  return rc;
}

uint32_t Batch::will_make(uint32_t frames, uint32_t capacity) const {
  uint32_t most = 0;
  for (uint32_t c = 0; c < (uniform(0) ? 1u : channels_); c++)
    most = std::max(most, produced_closed_form(filter_.num, filter_.den, frames, capacity, P(0, c)));
  return most;
}

bool Batch::lengths_fit(const uint32_t *in_len, const uint32_t *out_len, uint32_t n) const {
  const uint64_t room = 0xffffffffull - kExtentSlack;
  const uint32_t most = filter_.den < room ? static_cast<uint32_t>(room - filter_.den) : 0u;
  for (uint32_t s = 0; s < n; s++) {
    if (in_len[s] > most) return false;
    if (out_len[s] <= most) continue;  // (every call but those that name a capacity at the very limit)
    for (uint32_t c = 0; c < channels_; c++)
      if (produced_closed_form(filter_.num, filter_.den, in_len[s], out_len[s], P(s, c)) > most) return false;
  }
  return true;
}

// The pinned lookup of both sides: the address the device sees where a side is pinned memory (pinned_view), else nullptr
// (a null side too).  A pinned result that overlaps its pinned chunk: the chunk is taken in whole before anything is
// written, as on pageable buffers -- it counts as not pinned.
void Batch::pinned_sides(const void *in, size_t in_bytes, void *out, size_t out_bytes, const void **pin_in, void **pin_out) {
  *pin_in = pinned_view(in, in_bytes);
  *pin_out = pinned_view(out, out_bytes);
  if (*pin_in != nullptr && *pin_out != nullptr && buffers_overlap(in, in_bytes, out, out_bytes)) *pin_in = nullptr;
}

int Batch::HostCall::begin(const HostRoute &route, const HostPiece *in, uint32_t n_in, const void *pinned_in,
                           void *pinned_out) {
  r = route;
  const int rc = b->ensure_stage(r.dev_in, r.dev_out, r.pin_in, r.pin_out);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  hipStream_t stream = b->own_stream_;
  if (r.in == Via::InPlace) {
    src = pinned_in;
  } else if (r.in != Via::None && r.in_image != 0) {
    for (uint32_t i = 0; i < n_in; i++) {
      const char *host = static_cast<const char *>(in[i].host);
      if (r.in == Via::Copy) {
        if (in[i].bytes != 0) HIP_TRY(hipMemcpyAsync(b->d_stage_in_ + in[i].at, host, in[i].bytes, hipMemcpyHostToDevice, stream));
      } else if (host == nullptr) {
        std::memset(b->h_pin_in_ + in[i].at, 0, in[i].bytes);
      } else if (r.strided) {
        copy_samples(b->h_pin_in_ + in[i].at, 1, host, line_step, in[i].bytes / line_es, line_es);
      } else {
        std::memcpy(b->h_pin_in_ + in[i].at, host, in[i].bytes);
      }
    }
    if (r.in == Via::Staged) HIP_TRY(hipMemcpyAsync(b->d_stage_in_, b->h_pin_in_, r.in_image, hipMemcpyHostToDevice, stream));
    src = r.in == Via::Bounce ? b->h_pin_in_ : b->d_stage_in_;
  }
  // A present but empty input is not silence: no frame is read, any non-null address serves.  (One rule for every entry
  // point: before there was one helper the take call and the interleaved call of a state whose channels stand apart passed
  // nullptr here, the per-channel and chunks calls their input staging buffer.  With no readable frame no kernel reads
  // through the address -- device_helpers.h tests `in != nullptr && frame < in_frames` -- and the planar gather is skipped
  // for 0 frames, so samples, counters and state are the same either way.)
  if (src == nullptr && r.in != Via::None) src = b->h_pin_out_;
  dst = r.out == Via::InPlace ? pinned_out : r.out == Via::Bounce ? static_cast<void *>(b->h_pin_out_) : static_cast<void *>(b->d_stage_out_);
  return SPEEXHIP_ERR_SUCCESS;
}

// The wait the route chose (wait_call): on the tail of the pinned result buffer with the state's next sequence number, or
// on a take call's own word, which is armed once.
int Batch::HostCall::wait() {
  const int rc = word != nullptr ? wait_call(b->own_stream_, r.wait, word, 1u)
                                  : wait_call(b->own_stream_, r.wait, tail_word(b->h_pin_out_, b->pin_out_cap_), ++b->done_seq_);
  if (rc == SPEEXHIP_ERR_SUCCESS) drain.armed = false;
  return rc;
}

int Batch::HostCall::finish_whole(void *out, size_t bytes) {
  if (device_part(r.out, bytes) != 0)
    HIP_TRY(hipMemcpyAsync(r.out == Via::Copy ? out : b->h_pin_out_, b->d_stage_out_, bytes, hipMemcpyDeviceToHost, b->own_stream_));
  const int rc = wait();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (pinned_part(r.out, bytes) != 0) std::memcpy(out, b->h_pin_out_, bytes);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::HostCall::finish_planes(void *const *planes, uint32_t n, size_t pitch, size_t es, const uint32_t *made) {
  for (uint32_t c = 0; r.out == Via::Copy && c < n; c++)
    if (made[c] != 0)
      HIP_TRY(hipMemcpyAsync(planes[c], b->d_stage_out_ + c * pitch, made[c] * es, hipMemcpyDeviceToHost, b->own_stream_));
  if (r.out == Via::Staged && r.out_image != 0)
    HIP_TRY(hipMemcpyAsync(b->h_pin_out_, b->d_stage_out_, r.out_image, hipMemcpyDeviceToHost, b->own_stream_));
  const int rc = wait();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t c = 0; (r.out == Via::Bounce || r.out == Via::Staged) && c < n; c++)
    if (made[c] != 0) std::memcpy(planes[c], b->h_pin_out_ + c * pitch, made[c] * es);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::HostCall::finish_samples(void *out, uint32_t n, uint32_t host_step, size_t es, const uint32_t *made) {
  const size_t bytes = static_cast<size_t>(*std::max_element(made, made + n)) * n * es;  // the block whole
  if (device_part(r.out, bytes) != 0)
    HIP_TRY(hipMemcpyAsync(b->h_pin_out_, b->d_stage_out_, bytes, hipMemcpyDeviceToHost, b->own_stream_));
  const int rc = wait();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t c = 0; c < n; c++) copy_samples(static_cast<char *>(out) + c * es, host_step, b->h_pin_out_ + c * es, n, made[c], es);
  return SPEEXHIP_ERR_SUCCESS;
}

}  // namespace speexhip
