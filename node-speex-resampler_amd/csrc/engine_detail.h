// engine_detail.h -- what the engine's translation units (engine.cpp, many.cpp, planar.cpp ...) share beside engine.h: the HIP error
// macros, the device scope of an entry point and the staging helpers of the host-buffer calls (product code).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/speexhip_resampler.h"
#include "devices.h"
#include "host_transfer.h"

namespace speexhip {
namespace detail {

// engine.cpp: text of the most recent HIP failure on this thread (last_device_error)
extern thread_local std::string g_last_error;
// false on hipSuccess; otherwise records the text speexhip_resampler_strerror(SPEEXHIP_ERR_DEVICE) reports
bool hip_failed(hipError_t e, const char *what);
#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    if (::speexhip::detail::hip_failed((expr), #expr)) return SPEEXHIP_ERR_DEVICE;     \
  } while (0)

// Every entry point runs on the batch's own device whatever the calling thread's current one is,
// and leaves the thread's current device as it found it.
class DeviceScope {
 public:
  explicit DeviceScope(int logical_device) {  // (devices.h: logical ordinals; physical = logical unless aliased)
    const int device = devices::physical(logical_device);
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = device;
    if (prev_ != device) err_ = hipSetDevice(device);
    // (a failed call leaves its code behind as the thread's "last error", and the launchers read that after their
    //  next launch: hipLaunchKernelGGL + hipGetLastError would report THIS failure for a launch that worked)
    if (err_ != hipSuccess) (void)hipGetLastError();
  }
  ~DeviceScope() {
    if (prev_ != device_now()) (void)hipSetDevice(prev_);
  }
  hipError_t error() const { return err_; }

 private:
  static int device_now() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
  }
  int prev_ = 0;
  hipError_t err_ = hipSuccess;
};
#define ON_DEVICE()                                   \
  ::speexhip::detail::DeviceScope device_scope(device_); \
  HIP_TRY(device_scope.error())

// The host-buffer calls are synchronous, and their staging buffers and the (shared) stream go on to the
// next call or to another state: on EVERY exit nothing they enqueued may still be in flight.  The normal
// path waits explicitly (and checks the result); this guard covers the early error returns.
struct DrainOnExit {
  hipStream_t *stream;  // (pointer: the stream is taken from the pool after the guard is set up)
  bool armed = true;
  explicit DrainOnExit(hipStream_t *s) : stream(s) {}
  ~DrainOnExit() {
    if (armed && *stream != nullptr) (void)hipStreamSynchronize(*stream);
  }
};

inline bool buffers_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}
inline char *tail_word(char *buf, size_t cap) { return buf == nullptr ? nullptr : buf + ((cap - 64) & ~static_cast<size_t>(63)); }
// A call that ran: ALLOC_FAILED is what the zero fallback answers after writing its silence, counters and state moved.
inline bool ran(int rc) { return rc == SPEEXHIP_ERR_SUCCESS || rc == SPEEXHIP_ERR_ALLOC_FAILED; }

// engine.cpp: the wait a host-buffer call's `Wait` chose, and the grow-only staging buffers
int wait_call(hipStream_t stream, const Wait &w, void *word, uint32_t seq);
int grow_stage(int device, char **buf, size_t *cap_now, size_t want, bool pinned);
// engine.cpp: the address the device sees when all of [p, p + bytes) is pinned memory, else nullptr
void *pinned_view(const void *p, size_t bytes);
// engine.cpp: control-plane data (histories, tables, meter cells, a bus matrix) moves through the copy engines, whole, in
// copies of at least kCtlCopyMin bytes -- the device buffers involved are allocated at least that big.  ctl_upload: host
// `src` (bytes) -> device `dst`; ctl_download: bytes [off, off + len) of the device buffer `base` of `total` bytes -> host
// `dst`.  Both wait for their copy.  dev_alloc: ALLOC_FAILED when the device is out of memory, DEVICE for anything else.
extern const size_t kCtlCopyMin;
int dev_alloc(int device, void **ptr, size_t bytes);
int ctl_upload(void *dst, const void *src, size_t bytes, hipStream_t stream);
int ctl_download(void *dst, const char *base, size_t total, size_t off, size_t len, hipStream_t stream);

}  // namespace detail
}  // namespace speexhip
