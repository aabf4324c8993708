// engine.cpp -- see engine.h.
#include "engine.h"

#include "devices.h"
#include "engine_detail.h"
#include "gain.h"
#include "host_transfer.h"
#include "pool.h"
#include "unit_workers.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

namespace speexhip {
namespace detail {
thread_local std::string g_last_error = "no HIP error recorded";
bool hip_failed(hipError_t e, const char *what) {
  if (e == hipSuccess) return false;
  g_last_error = std::string("HIP device error: ") + what + ": " + hipGetErrorString(e);
  return true;
}
}  // namespace detail
using namespace detail;  // (engine_detail.h: HIP_TRY, ON_DEVICE, DeviceScope, DrainOnExit, the staging helpers)

namespace {
std::atomic<int> g_fail_allocs{0};
}  // namespace

namespace detail {  // (engine_detail.h: the control-plane helpers that bus.cpp shares)

// Device allocation of the filter installs: ALLOC_FAILED when the device is out of memory (or the
// test hook says so) -- the caller then falls back to resampler_basic_zero like the reference
// (resample.c:785-791) --, DEVICE for anything else.
int dev_alloc(int device, void **ptr, size_t bytes) {
  *ptr = nullptr;
  // test hook: a countdown -- the allocation that brings it to zero fails
  if (g_fail_allocs.load() > 0 && g_fail_allocs.fetch_sub(1) == 1) return SPEEXHIP_ERR_ALLOC_FAILED;
  hipError_t e = pool::device_get(device, ptr, bytes);
  if (e == hipErrorOutOfMemory) {
    // (pool::device_get has already given the pool's idle buffers back and tried again.)  Table sets
    // that no state references any more are reclaimable too: evict them, empty the pool, try once more.
    (void)hipGetLastError();
    if (release_cached_tables() != 0) {
      (void)pool::release_idle();
      e = pool::device_get(device, ptr, bytes);
    }
  }
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return SPEEXHIP_ERR_ALLOC_FAILED;
  }
  if (hip_failed(e, "hipMalloc")) return SPEEXHIP_ERR_DEVICE;
  return SPEEXHIP_ERR_SUCCESS;
}

// Control-plane copies (histories of a filter change, table uploads).  The runtime performs copies of
// <= 16 KiB with a blit KERNEL, and a kernel of this stream is dispatched only once the kernels other
// states have running let go of the CUs: 2 KB beside a 5 ms launch took 5 ms, 16 385 bytes 9 us
// (tools/ubench_ctl.hip, profiles/r03_ubench_ctl.txt).  So every control copy is at least kCtlCopyMin bytes
// -- the device buffers involved are allocated at least that big -- and runs on the copy engines from / to a
// pinned image, beside whatever the device is doing.
const size_t kCtlCopyMin = 20 * 1024;
namespace {
struct PinnedImage {
  char *p = nullptr;
  size_t bytes = 0;
  ~PinnedImage() { pool::pinned_put(p); }
  hipError_t get(size_t want) {
    bytes = std::max(want, kCtlCopyMin);
    return pool::pinned_get(reinterpret_cast<void **>(&p), bytes);
  }
};
}  // namespace
// host `src` (bytes) -> device `dst` (capacity >= max(bytes, kCtlCopyMin)); waits for the copy
int ctl_upload(void *dst, const void *src, size_t bytes, hipStream_t stream) {
  PinnedImage img;
  HIP_TRY(img.get(bytes));
  std::memset(img.p, 0, img.bytes);
  if (bytes != 0) std::memcpy(img.p, src, bytes);
  HIP_TRY(hipMemcpyAsync(dst, img.p, img.bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return SPEEXHIP_ERR_SUCCESS;
}
// device buffer `base` of `total` bytes (>= kCtlCopyMin): bytes [off, off+len) -> host `dst`; waits
int ctl_download(void *dst, const char *base, size_t total, size_t off, size_t len, hipStream_t stream) {
  if (len == 0) return SPEEXHIP_ERR_SUCCESS;
  const size_t span = std::min(total, std::max(len, kCtlCopyMin));
  const size_t first = std::min(off, total - span);
  PinnedImage img;
  HIP_TRY(img.get(span));
  HIP_TRY(hipMemcpyAsync(img.p, base + first, span, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(dst, img.p + (off - first), len);
  return SPEEXHIP_ERR_SUCCESS;
}
}  // namespace detail

namespace {

const size_t kLdsBudget = 150 * 1024;  // of the CU's 160 KiB
static_assert(kStagedLdsBytes <= kLdsBudget, "the period kernel's staged-store instance asks for more LDS than the budget");
// A piecewise host call (take_in_pieces) takes 2 MB of input per piece, at most four: a piece costs ~15 us (an event,
// a cross-stream wait, a launch) and buys the overlap of its launch -- the result leaving through PCIe -- with the next
// piece's copy.  2^20 stereo frames (4.2 MB in): 1 / 2 / 3 / 4 pieces 0.1935 / 0.1879 / 0.198 / 0.224 ms per call; 8
// channels (16.8 MB in), four pieces: 0.617 -> 0.517 ms.
const size_t kPieceBytes = static_cast<size_t>(2) << 20;

}  // namespace
// Round 6 -- pinned host buffers are used in place.  Where the kernels reach a HOST buffer directly: the address the
// device sees when all of [p, p + bytes) is pinned memory -- a block of the library's slabs (speexhip_block_acquire, a
// result block of ..._take: a range check, no runtime call), or, for buffers of kDirectCopyBytes and more, memory the
// caller pinned itself (hipHostMalloc / hipHostRegister: asked of the runtime at both ends of the buffer) -- else nullptr.
// Such a buffer needs no staging: the kernel that reads it through PCIe can write its result block through PCIe at the
// same time (the link is full duplex), where copy -> launch -> copy takes the two crossings one after the other; for the
// Node wrapper this replaces the copy into the module's heap, src/index.ts:71-92.
void *detail::pinned_view(const void *p, size_t bytes) {
  if (p == nullptr || bytes == 0) return nullptr;
  if (pool::block_owns(p, bytes)) return const_cast<void *>(p);
  if (bytes < kDirectCopyBytes) return nullptr;
  auto device_side = [](const void *q) -> char * {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // (an ordinary malloc'ed pointer is an "invalid value" to older runtimes)
      return nullptr;
    }
    return a.type == hipMemoryTypeHost ? static_cast<char *>(a.devicePointer) : nullptr;
  };
  char *first = device_side(p);
  if (first == nullptr) return nullptr;
  char *last = device_side(static_cast<const char *>(p) + bytes - 1);
  return last != nullptr && static_cast<size_t>(last - first) == bytes - 1 ? first : nullptr;
}
namespace {

// The polled wait of a host-buffer call (host_transfer.h, Wait): a 32-bit stream write behind the kernel
// (hipStreamWriteValue32: performed once everything before it on the stream has completed) into pinned memory, polled by
// the caller.  The pool's streams are shared by all states -- behind another state's long launch the word will not come
// soon -- so the spin is bounded (`spin_us`, `pause` between the reads) and then the thread sleeps in the runtime, which
// also reports the error if that is what happened.  *word must not equal seq when the call is made.
int wait_done(hipStream_t stream, volatile uint32_t *word, uint32_t seq, uint32_t spin_us) {
  bool signalled = false;
  if (hipStreamWriteValue32(stream, const_cast<uint32_t *>(word), seq, 0) == hipSuccess) {
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us);
    for (uint32_t spins = 0; !signalled; spins++) {
      signalled = __atomic_load_n(const_cast<const uint32_t *>(word), __ATOMIC_ACQUIRE) == seq;
      if (signalled) break;
      __builtin_ia32_pause();
      if ((spins & 63u) == 63u && std::chrono::steady_clock::now() > deadline) break;
    }
  } else {
    (void)hipGetLastError();
  }
  if (!signalled) HIP_TRY(hipStreamSynchronize(stream));
  return SPEEXHIP_ERR_SUCCESS;
}
}  // namespace
// The wait `w` chose.  A polled one arms the completion word at `word` -- 64 bytes of pinned memory the call's kernels do
// not write: the tail of a pinned result buffer (tail_word) or the bytes behind the samples of a take block -- with a
// value other than `seq` and waits for the stream to write `seq` there.
int detail::wait_call(hipStream_t stream, const Wait &w, void *word, uint32_t seq) {
  if (w.sync) {
    HIP_TRY(hipStreamSynchronize(stream));
    return SPEEXHIP_ERR_SUCCESS;
  }
  volatile uint32_t *done = static_cast<volatile uint32_t *>(word);
  *done = seq - 1;
  return wait_done(stream, done, seq, w.spin_us());
}
// Grows a staging buffer of the host-buffer calls to `want` bytes: grow-only (like the wrapper's heap buffers,
// src/index.ts:71-87); the calls are synchronous, so nothing in flight uses a buffer that goes back to the pool here.
int detail::grow_stage(int device, char **buf, size_t *cap_now, size_t want, bool pinned) {
  if (want <= *cap_now) return SPEEXHIP_ERR_SUCCESS;
  if (pinned)
    pool::pinned_put(*buf);
  else
    pool::device_put(device, *buf);
  *buf = nullptr;
  *cap_now = 0;
  const size_t cap = pool::size_class(std::max<size_t>(want, 8192));
  if (pinned)
    HIP_TRY(pool::pinned_get(reinterpret_cast<void **>(buf), cap));
  else
    HIP_TRY(pool::device_get(device, reinterpret_cast<void **>(buf), cap));
  *cap_now = cap;
  return SPEEXHIP_ERR_SUCCESS;
}
namespace {

// The position fields of a descriptor: `n_out` outputs of filter `f` from `at`, `consumed` frames of V past the history,
// `hist_frames` frames of history read and `hist_keep` left behind.
void set_position(StreamDesc &d, const FilterSpec &f, const StreamPos &at, uint32_t n_out, uint32_t consumed,
                  uint32_t hist_frames, uint32_t hist_keep) {
  d.n_out = n_out;
  d.consumed = consumed;
  d.hist_frames = hist_frames;
  d.hist_keep = hist_keep;
  d.last0 = at.last;
  d.frac0 = at.frac;
  d.k_shift = phase_index_of(f.num, f.den, at.frac);
  d.base_shift = at.last - static_cast<int32_t>((static_cast<uint64_t>(d.k_shift) * f.num) / f.den);
  d.tile_begin = 0;
  d.m_total = static_cast<uint32_t>((static_cast<uint64_t>(d.k_shift) + n_out + f.den - 1) / f.den);
}
}  // namespace

// The exact kernel's geometry in the zero fallback: the window geometry belongs to the filter that is no longer in force.
static ExactGeometry zero_geometry(ExactGeometry geo) {
  geo.staged = false;
  geo.lds_bytes = 0;
  geo.outs_per_block = 256;
  return geo;
}

void Batch::fill_desc(StreamDesc &d, uint32_t s, uint32_t c, const void *in, void *out, uint32_t in_frames, const CallPlan &plan) const {
  d.in = in;
  d.hist = d_hist_[hist_cur_] + s * hist_elems_ + c;
  d.out = out;
  d.hist_next = d_hist_[hist_cur_ ^ 1] + s * hist_elems_ + c;
  d.in_frames = in_frames;
  set_position(d, filter_, plan.begin, plan.produced, plan.magic_used + plan.consumed, filter_.taps - 1 + plan.begin.magic,
               filter_.taps - 1 + plan.end.magic);
}

// SPEEXHIP_INIT_TRACE=1: where a state's creation goes, step by step (stderr; tools/first_call.py)
struct InitTrace {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  static bool on() {
    static const bool v = SPEEXHIP_DIAG_ENV("SPEEXHIP_INIT_TRACE") != nullptr;
    return v;
  }
  void step(const char *what) {
    if (!on()) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "speexhip init: %-40s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

const char *last_device_error() { return g_last_error.c_str(); }
void set_last_device_error(const std::string &text) { g_last_error = text; }
size_t lds_budget() { return kLdsBudget; }

// diagnostics / tests: the int16-window plan at every launch size (normally only launches that fill the chip)
// (SPEEXHIP_W16_ALWAYS=0: never -- A/B runs)
static int w16_env() {
  static const int v = [] {
    const char *e = SPEEXHIP_DIAG_ENV("SPEEXHIP_W16_ALWAYS");
    return e == nullptr ? -1 : (e[0] == '0' && e[1] == '\0' ? 0 : 1);
  }();
  return v;
}
void debug_fail_device_allocs(int n) { g_fail_allocs.store(n < 0 ? 0 : n); }

bool Batch::uniform(uint32_t s) const {
  const StreamPos &a = P(s, 0);
  for (uint32_t c = 1; c < channels_; c++) {
    const StreamPos &b = P(s, c);
    if (a.last != b.last || a.frac != b.frac || a.magic != b.magic) return false;
  }
  return true;
}

uint32_t Batch::max_magic(uint32_t s) const {
  uint32_t m = 0;
  for (uint32_t c = 0; c < channels_; c++) m = std::max(m, P(s, c).magic);
  return m;
}

Batch *Batch::create(uint32_t n_streams, uint32_t channels, uint32_t in_rate, uint32_t out_rate,
                     int quality, int *err, int device) {
  return create_frac(n_streams, channels, in_rate, out_rate, in_rate, out_rate, quality, err, device);
}

Batch *Batch::create_frac(uint32_t n_streams, uint32_t channels, uint32_t ratio_num, uint32_t ratio_den,
                          uint32_t in_rate, uint32_t out_rate, int quality, int *err, int device) {
  int e = SPEEXHIP_ERR_SUCCESS;
  // (owned until it is handed out: an exception below -- a bad_alloc in a position vector, in the design
  //  or in the tap rows; c_api.cpp maps it to a code -- must not leak the batch and what it already took)
  std::unique_ptr<Batch> b;
  // argument checks first, like the reference (resample.c:804-809)
  if (n_streams == 0 || channels == 0 || ratio_num == 0 || ratio_den == 0 || quality > 10 ||
      quality < 0) {
    e = SPEEXHIP_ERR_INVALID_ARG;
  } else {
    b.reset(new (std::nothrow) Batch());
    if (b == nullptr) {
      e = SPEEXHIP_ERR_ALLOC_FAILED;
    } else {
      b->n_streams_ = n_streams;
      b->channels_ = channels;
      b->device_ = device;  // (< 0: the placement rule decides, setup())
      e = design_filter_frac(ratio_num, ratio_den, in_rate, out_rate, quality, &b->filter_, /*fill_table=*/false);
      if (e == SPEEXHIP_ERR_SUCCESS) e = b->setup();
      if (e != SPEEXHIP_ERR_SUCCESS) b.reset();
    }
  }
  if (err) *err = e;
  return b.release();
}

int Batch::setup() {
  InitTrace trace;
  const int count = devices::count();
  trace.step("device count (first HIP call)");
  if (count <= 0) {
    g_last_error = count < 0 ? "HIP device error: hipGetDeviceCount failed (libspeexhip has no CPU fallback)"
                             : "HIP device error: no GPU visible (libspeexhip has no CPU fallback)";
    return SPEEXHIP_ERR_DEVICE;
  }
  // Which GPU: the caller's choice (..._init_on), else the process-wide rule (devices.h: SPEEXHIP_DEVICE,
  // SPEEXHIP_DEVICES=all -> state k on device k mod count, default = the thread's current device).
  if (device_ < 0) {
    device_ = devices::place_next_state();
    if (device_ < 0) {
      g_last_error = "HIP device error: SPEEXHIP_DEVICE / SPEEXHIP_DEVICES names a device this node does not have";
      return SPEEXHIP_ERR_DEVICE;
    }
  } else if (device_ >= count) {
    g_last_error = "HIP device error: device " + std::to_string(device_) + " requested, the node has " + std::to_string(count);
    device_ = -1;  // (nothing lives anywhere yet: the destructor has no device to visit)
    return SPEEXHIP_ERR_DEVICE;
  }
  ON_DEVICE();  // (everything below -- pool, tables, uploads -- runs on the state's device)
  bus_out_.bind(device_, channels_, n_streams_);
  hipDeviceProp_t prop;
  trace.step("placement + hipSetDevice");
  HIP_TRY(hipGetDeviceProperties(&prop, devices::physical(device_)));
  trace.step("hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_last_error = std::string("HIP device error: built for gfx950 (MI355X), found ") + prop.gcnArchName;
    return SPEEXHIP_ERR_DEVICE;
  }
  // (default: SPEEXHIP_MODE_FAST_FIXED -- a stream's bytes do not depend on chunking, batch size or GPU, like the
  //  reference's; 'fast' opts into launch-time re-association where it buys speed)
  const char *m = std::getenv("SPEEXHIP_MODE");
  if (m != nullptr && std::strcmp(m, "fast") == 0) mode_ = SPEEXHIP_MODE_FAST;
  if (m != nullptr && std::strcmp(m, "exact") == 0) mode_ = SPEEXHIP_MODE_EXACT;
  if (m != nullptr && std::strcmp(m, "fast_f32") == 0) mode_ = SPEEXHIP_MODE_FAST_F32;
  if (m != nullptr && std::strcmp(m, "fast_fixed") == 0) mode_ = SPEEXHIP_MODE_FAST_FIXED;

  pos_.assign(static_cast<size_t>(n_streams_) * channels_, StreamPos());
  started_.assign(n_streams_, 0);
  const FilterSpec designed = filter_;
  int rc = install_filter(designed, std::vector<float>(), designed.taps - 1);  // resample.c:721-725: silence
  trace.step("install_filter (total)");
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  devices::state_born(device_);  // (the live count the placement rule balances: devices.h, round 6)
  counted_ = true;
  return SPEEXHIP_ERR_SUCCESS;  // (install_filter waited for its own uploads)
}

DeviceTables::~DeviceTables() {
  // (whoever dropped the last reference has synchronised: ~Batch, install_filter)
  pool::device_put(device, table);
  for (void *rows : period_rows) pool::device_put(device, rows);
  pool::device_put(device, slide_rows);
  pool::device_put(device, slide64_rows);
}

namespace {
struct TablesKey {
  int device;
  uint32_t num, den, channels;
  int quality;
  bool operator==(const TablesKey &o) const {
    return device == o.device && num == o.num && den == o.den && channels == o.channels && quality == o.quality;
  }
};
struct TablesCache {
  std::mutex mu;
  std::list<std::pair<TablesKey, std::shared_ptr<const DeviceTables>>> lru;  // most recent first
};
TablesCache &tables_cache() {
  static TablesCache *c = new TablesCache();  // never destroyed, like the pool
  return *c;
}
const size_t kCachedTables = 24;                           // entries kept beyond the ones in use ...
const size_t kCachedTableBytes = static_cast<size_t>(256) << 20;  // ... and their bytes (most recent first)
const size_t kCacheableBytes = static_cast<size_t>(64) << 20;  // bigger table sets are built per state

// Design (host, double precision), plan and upload the tables of filter `g` (geometry only: num,
// den, quality, taps ...) for `channels` channels.
// Uploads run on `stream` (the installing state's control stream) and are waited for before the tables
// are published: never on the null stream, whose copies would wait for every blocking stream of the process.
int build_tables(int device, const FilterSpec &g, uint32_t channels, hipStream_t stream,
                 std::shared_ptr<const DeviceTables> *out) {
  InitTrace trace;
  FilterSpec f;
  int rc = design_filter_frac(g.num, g.den, g.in_rate, g.out_rate, g.quality, &f);
  trace.step("    filter design (host)");
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  auto t = std::make_shared<DeviceTables>();
  t->device = device;
  auto upload_bytes = [&](void **dst, const void *src, size_t bytes) -> int {
    const int arc = dev_alloc(device, dst, std::max(bytes, kCtlCopyMin));
    if (arc != SPEEXHIP_ERR_SUCCESS) return arc;
    if (bytes != 0) {
      const int urc = ctl_upload(*dst, src, bytes, stream);
      if (urc != SPEEXHIP_ERR_SUCCESS) return urc;
    }
    t->bytes += std::max(bytes, kCtlCopyMin);
    return SPEEXHIP_ERR_SUCCESS;
  };
  auto upload = [&](float **dst, const float *src, size_t count) -> int {
    return upload_bytes(reinterpret_cast<void **>(dst), src, count * sizeof(float));
  };
  rc = upload(&t->table, f.table.data(), f.table_len);
  trace.step("    first allocation + upload (sinc table)");
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // which plans the filter gets: filter_plans.h.  Their rows go up in the order of PeriodVariant, the slide rows between
  // the fp32 and the fp64 variants (the allocation-failure hook counts allocations).
  FilterPlans &plans = t->plans;
  FilterSpec folded;
  const FilterSpec &pf = plan_filter(f, channels, kLdsBudget, &plans, &folded);
  for (int v = 0; v < kPeriodVariants; v++) {
    if (v == kPeriod64 && plans.slide.usable) {
      std::vector<float> rows;
      build_slide_rows(f, plans.slide, &rows);
      rc = upload(&t->slide_rows, rows.data(), rows.size());
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    }
    if (!plans.has_rows(v)) continue;
    if (plans.period[v].a64) {
      std::vector<double> rows;
      build_period_rows64(pf, plans.period[v], &rows);
      rc = upload_bytes(&t->period_rows[v], rows.data(), rows.size() * sizeof(double));
    } else {
      std::vector<float> rows;
      build_period_rows(pf, plans.period[v], &rows);
      rc = upload_bytes(&t->period_rows[v], rows.data(), rows.size() * sizeof(float));
    }
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  if (plans.slide64.usable) {
    std::vector<double> rows;
    build_slide64_rows(f, plans.slide64, &rows);
    rc = upload_bytes(reinterpret_cast<void **>(&t->slide64_rows), rows.data(), rows.size() * sizeof(double));
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  trace.step("    plans, tap rows, their uploads");
  *out = t;
  return SPEEXHIP_ERR_SUCCESS;
}

int acquire_tables(int device, const FilterSpec &g, uint32_t channels, hipStream_t stream,
                   std::shared_ptr<const DeviceTables> *out) {
  static const bool enabled = [] {
    const char *e = std::getenv("SPEEXHIP_POOL_MB");
    return e == nullptr || std::atoi(e) != 0;
  }();
  // (an armed allocation-failure hook must see the allocations: no cache then)
  const bool cacheable = enabled && g_fail_allocs.load() <= 0;
  const TablesKey key{device, g.num, g.den, channels, g.quality};
  TablesCache &c = tables_cache();
  if (cacheable) {
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto it = c.lru.begin(); it != c.lru.end(); ++it)
      if (it->first == key) {
        c.lru.splice(c.lru.begin(), c.lru, it);
        *out = it->second;
        return SPEEXHIP_ERR_SUCCESS;
      }
  }
  std::shared_ptr<const DeviceTables> built;
  const int rc = build_tables(device, g, channels, stream, &built);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (cacheable && built->bytes <= kCacheableBytes) {
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto &e : c.lru)
      if (e.first == key) {  // another thread built the same tables meanwhile: share those
        *out = e.second;
        return SPEEXHIP_ERR_SUCCESS;
      }
    c.lru.emplace_front(key, built);
    size_t idle = 0, idle_bytes = 0;
    for (auto it = c.lru.begin(); it != c.lru.end();) {
      if (it->second.use_count() == 1 &&
          (++idle > kCachedTables || (idle_bytes += it->second->bytes) > kCachedTableBytes))
        it = c.lru.erase(it);  // nobody uses them: back to the pool
      else
        ++it;
    }
  }
  *out = built;
  return SPEEXHIP_ERR_SUCCESS;
}
}  // namespace

size_t release_cached_tables() {
  TablesCache &c = tables_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  size_t bytes = 0;
  for (auto it = c.lru.begin(); it != c.lru.end();) {
    if (it->second.use_count() == 1) {
      bytes += it->second->bytes;
      it = c.lru.erase(it);
    } else {
      ++it;
    }
  }
  return bytes;
}

// Put everything on the device that depends on the filter `f` (geometry: the tables are designed
// here on a cache miss) in place -- the shared tables, the history buffers (hist = all streams'
// lines, hist_frames_cap frames each, interleaved; empty = silence) -- and only then replace what
// the batch holds: a failed allocation leaves the batch exactly as it was (the caller decides what
// a failure means, resample.c:785-791).
int Batch::install_filter(const FilterSpec &f, const std::vector<float> &hist, uint32_t hist_frames_cap) {
  InitTrace trace;
  if (own_stream_ == nullptr) HIP_TRY(pool::stream_get(device_, &own_stream_));
  trace.step("  stream");
  std::shared_ptr<const DeviceTables> tables;
  int rc = acquire_tables(device_, f, channels_, own_stream_, &tables);
  trace.step("  tables (design, allocations, uploads)");
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  struct Fresh {
    int device = 0;
    float *hist[2] = {nullptr, nullptr};
    ~Fresh() {
      pool::device_put(device, hist[0]);
      pool::device_put(device, hist[1]);
    }
  } n;
  n.device = device_;
  const size_t hist_elems = static_cast<size_t>(hist_frames_cap) * channels_;
  const size_t hist_bytes = std::max(hist_elems * n_streams_ * sizeof(float), kCtlCopyMin);
  for (int i = 0; i < 2; i++) {
    rc = dev_alloc(device_, reinterpret_cast<void **>(&n.hist[i]), hist_bytes);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  {
    // Both buffers start from one pinned image of the histories (zeros = silence) through the copy
    // engines (see kCtlCopyMin; not hipMemsetAsync either: a fill kernel queues behind other states'
    // kernels just the same -- set_quality beside another state's 6 ms launch took 6 ms).
    PinnedImage image;
    DrainOnExit drain(&own_stream_);  // (declared behind the buffers it protects: an early return waits for the copies first)
    HIP_TRY(image.get(hist_bytes));
    std::memset(image.p, 0, hist_bytes);
    if (!hist.empty()) std::memcpy(image.p, hist.data(), hist_elems * n_streams_ * sizeof(float));
    for (int i = 0; i < 2; i++)
      HIP_TRY(hipMemcpyAsync(n.hist[i], image.p, hist_bytes, hipMemcpyHostToDevice, own_stream_));
    HIP_TRY(hipStreamSynchronize(own_stream_));  // the new buffers are in place for a launch on any stream
    drain.armed = false;
  }
  trace.step("  history buffers + their image");
  // What the batch held goes back to the pool / the cache below, so nothing in flight may still read it:
  // wait for this batch's own last call -- not for the device: other states' launches keep running.
  if (tables_ != nullptr) {
    rc = quiesce();
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  // commit: nothing below can fail
  hist_bytes_ = hist_bytes;
  std::swap(d_hist_[0], n.hist[0]);
  std::swap(d_hist_[1], n.hist[1]);  // (~Fresh releases the old history buffers)
  tables_ = tables;
  const std::vector<float> no_table;
  filter_ = f;
  filter_.table = no_table;  // the host copy of the sinc table lives only while the tables are built
  line_ = std::max(line_, f.taps - 1 + kBlockIn);  // grow-only, resample.c:709-720
  hist_elems_ = hist_elems;
  hist_cur_ = 0;
  return SPEEXHIP_ERR_SUCCESS;
}

// Wait for what THIS batch has enqueued.  Calls on one batch are ordered (a call on another stream
// than the previous one waits for it on the device, chain_to), so the previous call's stream ends
// with the batch's last piece of work; the control stream's own copies are waited for where they are
// issued.
int Batch::quiesce() {
  if (ev_pending_) {
    HIP_TRY(hipEventSynchronize(order_ev_));
    ev_pending_ = false;
  }
  if (have_last_stream_) HIP_TRY(hipStreamSynchronize(last_stream_));
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::chain_to(hipStream_t stream) {
  if (have_last_stream_ && stream != last_stream_) {
    if (order_ev_ == nullptr) HIP_TRY(pool::event_get(device_, &order_ev_));
    HIP_TRY(hipEventRecord(order_ev_, last_stream_));
    ev_pending_ = true;
  }
  if (ev_pending_) {
    HIP_TRY(hipStreamWaitEvent(stream, order_ev_, 0));
    ev_pending_ = false;  // (from here on the tail of `stream` stands for it)
  }
  last_stream_ = stream;
  have_last_stream_ = true;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::release_stream() {
  ON_DEVICE();
  if (!have_last_stream_ || last_stream_ == own_stream_) return SPEEXHIP_ERR_SUCCESS;  // (the pool's streams never die)
  if (order_ev_ == nullptr) HIP_TRY(pool::event_get(device_, &order_ev_));
  HIP_TRY(hipEventRecord(order_ev_, last_stream_));
  ev_pending_ = true;
  have_last_stream_ = false;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::fetch_history(std::vector<float> *host) {
  ON_DEVICE();
  int rc = quiesce();  // every enqueued call of this batch has left its history
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  host->assign(hist_elems_ * n_streams_, 0.f);
  if (!host->empty())
    return ctl_download(host->data(), reinterpret_cast<const char *>(d_hist_[hist_cur_]), hist_bytes_, 0,
                        host->size() * sizeof(float), own_stream_);
  return SPEEXHIP_ERR_SUCCESS;
}

// Switch every stream to the filter `next` (already designed): the tail of update_filter(),
// resample.c:703-782, per channel, on the host -- this is rare control-plane work.  Positions and
// device state change only if everything succeeded.
int Batch::adopt_filter(const FilterSpec &next) {
  ON_DEVICE();
  std::vector<float> old;
  int rc = fetch_history(&old);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const uint32_t old_taps = filter_.taps, new_taps = next.taps;
  const size_t old_stride = hist_elems_;
  std::vector<StreamPos> moved = pos_;
  std::vector<Realign> moves(pos_.size());
  uint32_t cap_frames = new_taps - 1;
  for (uint32_t s = 0; s < n_streams_; s++)
    for (uint32_t c = 0; c < channels_; c++) {
      const size_t i = static_cast<size_t>(s) * channels_ + c;
      if (started_[s]) {
        moves[i] = realign_history(old_taps, new_taps, pos_[i].magic);
        moved[i].magic = moves[i].new_magic;
        moved[i].last += moves[i].last_delta;
      }
      cap_frames = std::max(cap_frames, new_taps - 1 + moved[i].magic);
    }
  std::vector<float> fresh(static_cast<size_t>(cap_frames) * channels_ * n_streams_, 0.f);
  for (uint32_t s = 0; s < n_streams_; s++) {
    if (!started_[s]) continue;  // resample.c:721-726: nothing processed yet -> silence
    const float *src = old.data() + s * old_stride;
    float *dst = fresh.data() + static_cast<size_t>(s) * cap_frames * channels_;
    for (uint32_t c = 0; c < channels_; c++) {
      const size_t i = static_cast<size_t>(s) * channels_ + c;
      const int64_t have = static_cast<int64_t>(old_taps - 1) + pos_[i].magic;
      const uint32_t keep = new_taps - 1 + moved[i].magic;
      for (uint32_t j = 0; j < keep; j++) {
        const int64_t from = static_cast<int64_t>(j) + moves[i].shift;
        if (from < 0 || from >= have) continue;
        dst[static_cast<size_t>(j) * channels_ + c] = src[from * channels_ + c];
      }
    }
  }
  rc = install_filter(next, fresh, cap_frames);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  pos_ = moved;
  return SPEEXHIP_ERR_SUCCESS;
}

// resample.c:785-791: the new filter could not be built.  The reference keeps its old filter
// length (so its history stays where it is), has already taken the new rates / ratio / quality
// and the advances derived from them, and installs resampler_basic_zero: outputs are zeros with
// the right lengths until a later filter change succeeds.
void Batch::enter_zero_mode(const FilterSpec &n) {
  filter_.in_rate = n.in_rate;
  filter_.out_rate = n.out_rate;
  filter_.num = n.num;
  filter_.den = n.den;
  filter_.quality = n.quality;
  filter_.int_advance = n.int_advance;
  filter_.frac_advance = n.frac_advance;
  zero_mode_ = true;
}

// Common tail of set_rate_frac / set_quality: `next` was designed with result design_rc; fracs =
// every channel's phase numerator on the new denominator (set_rate_frac) or null.
int Batch::change_filter(const FilterSpec &next, int design_rc, const std::vector<uint32_t> *fracs) {
  int rc = design_rc;
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = adopt_filter(next);
  if (!ran(rc)) return rc;  // nothing was touched
  if (fracs != nullptr)
    for (size_t i = 0; i < pos_.size(); i++) pos_[i].frac = (*fracs)[i];
  if (rc == SPEEXHIP_ERR_ALLOC_FAILED) {
    enter_zero_mode(next);
    return rc;
  }
  zero_mode_ = false;
  // (a filter change that succeeded after a set_rate_frac had overflowed -- set_quality with the old ratio: what
  //  get_rate / get_ratio show is the filter in force again, not rates that never were)
  shown_valid_ = false;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::set_rate_frac(uint32_t ratio_num, uint32_t ratio_den, uint32_t in_rate, uint32_t out_rate) {
  if (ratio_num == 0 || ratio_den == 0) return SPEEXHIP_ERR_INVALID_ARG;
  // resample.c:1116-1117 (compares the given ratio with the REDUCED one it stores, as there)
  const RateView now = rates();
  if (now.in_rate == in_rate && now.out_rate == out_rate && now.num == ratio_num && now.den == ratio_den)
    return SPEEXHIP_ERR_SUCCESS;
  FilterSpec next;
  const int design_rc =
      design_filter_frac(ratio_num, ratio_den, in_rate, out_rate, filter_.quality, &next, /*fill_table=*/false);
  if (!ran(design_rc)) return design_rc;
  // phase numerators move to the new denominator (resample.c:1130-1139; next.num / next.den are set
  // even when the design failed later on).  On overflow the reference returns RESAMPLER_ERR_OVERFLOW from
  // the middle of that loop: it has ALREADY stored the new rates and the reduced ratio (:1119-1127), so
  // get_rate / get_ratio report them and a repeat of the same call is a no-op (:1116), while its filter,
  // its advances and the phase numerators of the failing and later channels are still the old ones --
  // a state in which its own processing indexes the old sinc table with numerators on two denominators.
  // Mirrored here: what a caller can SEE (rates, ratio, the no-op repeat).  Not mirrored: processing goes
  // on with the old ratio and filter, consistently, until a later set_rate succeeds (named deviation,
  // pinned by test_set_rate_overflow_leaves_the_reference_s_visible_state).
  std::vector<uint32_t> frac(pos_.size());
  for (size_t i = 0; i < pos_.size(); i++) {
    frac[i] = pos_[i].frac;
    if (!scale_phase(&frac[i], next.den, filter_.den)) {
      shown_ = RateView{in_rate, out_rate, next.num, next.den};
      shown_valid_ = true;
      return SPEEXHIP_ERR_OVERFLOW;
    }
  }
  const int rc = change_filter(next, design_rc, &frac);
  if (ran(rc)) shown_valid_ = false;  // filter_ holds the truth again
  return rc;
}

int Batch::set_quality(int quality) {
  if (quality > 10 || quality < 0) return SPEEXHIP_ERR_INVALID_ARG;
  if (quality == filter_.quality) return SPEEXHIP_ERR_SUCCESS;  // resample.c:1157-1158
  FilterSpec next;
  // the stored ratio is already reduced, so designing from it reproduces num/den
  const int design_rc =
      design_filter_frac(filter_.num, filter_.den, filter_.in_rate, filter_.out_rate, quality, &next, /*fill_table=*/false);
  if (!ran(design_rc)) return design_rc;
  return change_filter(next, design_rc, nullptr);
}

int Batch::skip_zeros() {  // resample.c:1200-1206
  for (StreamPos &p : pos_) p.last = static_cast<int32_t>(filter_.taps / 2);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::reset_mem() {  // resample.c:1208-1220
  ON_DEVICE();
  std::vector<float> h;
  int rc = fetch_history(&h);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // The reference clears the first channels*(taps-1) floats of its buffer as ONE run, but its
  // channel lines are line_ floats apart: only the lines (or parts of lines) that fall inside
  // that run are silenced, later channels keep their history.  Restated, not "fixed": the
  // outputs after a reset must be the reference's.
  const uint64_t run = static_cast<uint64_t>(channels_) * (filter_.taps - 1);
  for (uint32_t s = 0; s < n_streams_; s++) {
    float *line = h.data() + s * hist_elems_;
    for (uint32_t c = 0; c < channels_; c++) {
      const uint64_t first = static_cast<uint64_t>(c) * line_;
      for (uint32_t j = 0; j + 1 < filter_.taps && first + j < run; j++) line[static_cast<size_t>(j) * channels_ + c] = 0.f;
    }
    for (uint32_t c = 0; c < channels_; c++) P(s, c) = StreamPos();
  }
  if (!h.empty()) {
    // the whole buffer (>= kCtlCopyMin) from an image: what lies behind the histories is never read
    std::vector<float> image(hist_bytes_ / sizeof(float), 0.f);
    std::copy(h.begin(), h.end(), image.begin());
    return ctl_upload(d_hist_[hist_cur_], image.data(), hist_bytes_, own_stream_);
  }
  return SPEEXHIP_ERR_SUCCESS;
}

Batch::~Batch() {
  if (device_ < 0) return;  // setup() never got as far as a device
  if (counted_) devices::state_gone(device_);
  DeviceScope device_scope(device_);
  // everything goes back to the pool (pool.h) for the next state, once nothing in flight uses it:
  // this batch's calls are chained, so the tail of its last stream is all there is to wait for
  // (a device-wide wait here stalled a server's every other state behind one state's garbage collection)
  (void)quiesce();
  pool::event_put(device_, order_ev_);
  tables_.reset();  // shared (DeviceTables): the cache keeps them for the next state with this filter
  pool::device_put(device_, d_hist_[0]);
  pool::device_put(device_, d_hist_[1]);
  pool::device_put(device_, d_stage_in_);
  pool::device_put(device_, d_stage_out_);
  pool::device_put(device_, d_planar_in_);
  pool::device_put(device_, d_planar_out_);
  pool::device_put(device_, d_meter_);
  pool::device_put(device_, d_bus_);
  bus_out_.release();
  pool::pinned_put(h_pin_in_);
  pool::pinned_put(h_pin_out_);
  for (int i = 0; i < kMaxPieces; i++) pool::event_put(device_, piece_ev_[i]);
  pool::stream_put(device_, copy_stream_);
  pool::stream_put(device_, own_stream_);
}

// ---- the output meter (engine.h) ---------------------------------------------------------------------------------------
// The cells are control-plane data: zeroed and fetched through the copy engines (kCtlCopyMin), whole, on own_stream_.
int Batch::set_meter(int on) {
  if (on != 0 && on != 1) return SPEEXHIP_ERR_INVALID_ARG;
  if (on != 0 && d_meter_ == nullptr) {
    ON_DEVICE();
    void *cells = nullptr;
    const size_t bytes = std::max(sizeof(MeterCell) * n_streams_, kCtlCopyMin);
    int rc = dev_alloc(device_, &cells, bytes);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    const std::vector<char> zeros(bytes, 0);
    rc = ctl_upload(cells, zeros.data(), bytes, own_stream_);  // (in place before any launch on any stream)
    if (rc != SPEEXHIP_ERR_SUCCESS) {
      pool::device_put(device_, cells);
      return rc;
    }
    d_meter_ = static_cast<MeterCell *>(cells);
    meter_samples_.assign(n_streams_, 0);
  }
  meter_on_ = on != 0;
  bus_out_.set_meter(meter_on_);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::get_meter(uint32_t stream, SpeexHipMeter *m, bool reset) {
  if (!meter_request_ok(stream, n_streams_, m, reset)) return SPEEXHIP_ERR_INVALID_ARG;
  if (d_meter_ == nullptr) return read_meter(nullptr, n_streams_, stream, meter_on_, nullptr, m, reset, nullptr);
  ON_DEVICE();
  const int rc = quiesce();  // this state's own last call; its totals are in the cells behind it
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  return read_meter(d_meter_, n_streams_, stream, meter_on_, meter_samples_.data(), m, reset, own_stream_);
}

MeterPack Batch::meter_pack(uint32_t s0, uint32_t n) const {
  MeterPack p;
  std::memset(&p, 0, sizeof(p));
  for (uint32_t j = 0; j < n; j++) p.cell[j] = d_meter_ + s0 + j;
  return p;
}

void Batch::meter_count(const uint32_t *produced, uint32_t per_frame) {
  for (uint32_t s = 0; s < n_streams_; s++) meter_samples_[s] += static_cast<uint64_t>(produced[s]) * per_frame;
}

int Batch::meter_result(const void *result, uint64_t stride, const uint32_t *lens, float scale, hipStream_t stream) {
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  for (uint32_t first = 0; first < n_streams_; first += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - first);
    uint64_t most = 0;
    const ConvertPack pack = float_results_pack(static_cast<const float *>(result) + first * stride, stride, lens + first, n, channels_, &most);
    if (hip_failed(launch_meter_image(pack, meter_pack(first, n), scale, n, most, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

// ---- the output gain (engine.h) ----------------------------------------------------------------------------------------
int Batch::set_gain(uint32_t stream, float gain, uint32_t ramp_frames) {
  if (stream != UINT32_MAX && stream >= n_streams_) return SPEEXHIP_ERR_INVALID_ARG;
  if (!std::isfinite(gain)) return SPEEXHIP_ERR_INVALID_ARG;
  if (gain_.empty()) gain_.assign(n_streams_, Gain());
  for (uint32_t s = stream == UINT32_MAX ? 0 : stream; s < (stream == UINT32_MAX ? n_streams_ : stream + 1); s++) {
    Gain &g = gain_[s];
    const float now = gain::at(g.step, g.from, g.to, g.total, g.done);  // (what the next output frame would have had)
    g.from = now;
    g.to = gain;
    g.total = ramp_frames;
    g.done = 0;
    g.step = gain::step_of(g.from, g.to, g.total);
  }
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::get_gain(uint32_t stream, float *current, float *target, uint32_t *remaining) const {
  if (stream >= n_streams_) return SPEEXHIP_ERR_INVALID_ARG;
  const Gain g = gain_.empty() ? Gain() : gain_[stream];
  if (current != nullptr) *current = gain::at(g.step, g.from, g.to, g.total, g.done);
  if (target != nullptr) *target = g.to;
  if (remaining != nullptr) *remaining = g.total - g.done;
  return SPEEXHIP_ERR_SUCCESS;
}

bool Batch::gain_on() const {
  for (const Gain &g : gain_)
    if (!gain::is_off(g.to, g.total, g.done)) return true;
  return false;
}

GainPack Batch::gain_pack(uint32_t s0, uint32_t n, uint32_t per_frame) const {
  GainPack p;
  std::memset(&p, 0, sizeof(p));
  for (uint32_t j = 0; j < n && !gain_.empty(); j++) {
    const Gain &g = gain_[s0 + j];
    if (gain::is_off(g.to, g.total, g.done)) continue;  // (channels 0: not multiplied)
    p.s[j].step = g.step;
    p.s[j].first = g.done;
    p.s[j].from = g.from, p.s[j].to = g.to;
    p.s[j].total = g.total;
    p.s[j].channels = per_frame;
  }
  return p;
}

void Batch::gain_advance(const uint32_t *produced) {
  for (uint32_t s = 0; s < n_streams_ && !gain_.empty(); s++) {
    Gain &g = gain_[s];
    g.done += std::min(produced[s], g.total - g.done);  // (saturates at total)
  }
}

int Batch::image_result(void *result, uint64_t stride, const uint32_t *lens, float scale, hipStream_t stream) {
  if (!gain_on()) return meter_on_ ? meter_result(result, stride, lens, scale, stream) : SPEEXHIP_ERR_SUCCESS;
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  for (uint32_t first = 0; first < n_streams_; first += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - first);
    uint64_t most = 0;
    const ConvertPack pack = float_results_pack(static_cast<const float *>(result) + first * stride, stride, lens + first, n, channels_, &most);
    MeterPack cells;
    if (meter_on_) cells = meter_pack(first, n);
    if (hip_failed(launch_gain_image(pack, gain_pack(first, n, channels_), meter_on_ ? &cells : nullptr, scale, n, most, stream),
                   "kernel launch"))
      return SPEEXHIP_ERR_DEVICE;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

CallPlan Batch::peek(uint32_t s, uint32_t in_len, uint32_t out_capacity, bool float_io) const {
  const EntryRules rules = entry_rules(float_io);
  // (an interleaved call reports the counters of its LAST channel, resample.c:1070-1078)
  return plan_call(filter_.num, filter_.den, in_len, out_capacity, P(s, channels_ - 1), rules);
}

int Batch::set_mode(int mode) {
  if (mode != SPEEXHIP_MODE_FAST && mode != SPEEXHIP_MODE_EXACT && mode != SPEEXHIP_MODE_FAST_F32 &&
      mode != SPEEXHIP_MODE_FAST_FIXED)
    return SPEEXHIP_ERR_INVALID_ARG;
  mode_ = mode;
  return SPEEXHIP_ERR_SUCCESS;
}

void Batch::info(uint32_t s, SpeexHipInfo *o) const {
  std::memset(o, 0, sizeof(*o));
  o->in_rate = filter_.in_rate;
  o->out_rate = filter_.out_rate;
  o->num_rate = filter_.num;
  o->den_rate = filter_.den;
  o->nb_channels = channels_;
  o->quality = filter_.quality;
  o->filt_len = filter_.taps;
  o->oversample = filter_.oversample;
  o->sinc_table_length = filter_.table_len;
  o->kernel = filter_.kind;
  o->mode = mode_;
  const FilterPlans &p = tables_->plans;
  o->fast_path = p.period[kBase].usable ? 2 : (p.slide.usable ? 3 : 0);
  const bool double_kind = is_double_kind(filter_);
  // (what FAST would run: in EXACT mode too; FAST_F32 reports its own fp32-chain kernels)
  if (double_kind && mode_ != SPEEXHIP_MODE_FAST_F32 && !p.period[kBase].usable && p.slide64.usable) o->fast_path = 4;
  if (double_kind && mode_ != SPEEXHIP_MODE_FAST_F32 && p.period[kPeriod64].usable) o->fast_path = 5;
  o->accumulate_bits = mode_ == SPEEXHIP_MODE_EXACT || o->fast_path == 0 ? (double_kind ? 64 : 32)
                                                                          : (o->fast_path >= 4 ? 64 : 32);
  if (s < n_streams_) {
    o->last_sample = P(s, 0).last;
    o->samp_frac_num = P(s, 0).frac;
    o->magic_samples = P(s, 0).magic;
  }
  o->block_in = block_in();
  o->device = device_;
}

int Batch::history(uint32_t s, float *dst) {
  if (s >= n_streams_) return SPEEXHIP_ERR_INVALID_ARG;
  ON_DEVICE();
  int rc = quiesce();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const size_t n = static_cast<size_t>(filter_.taps - 1 + max_magic(s)) * channels_;
  if (n)
    return ctl_download(dst, reinterpret_cast<const char *>(d_hist_[hist_cur_]), hist_bytes_,
                        s * hist_elems_ * sizeof(float), n * sizeof(float), own_stream_);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::process_device(const void *d_in, uint64_t in_stride, uint32_t *in_len, void *d_out,
                          uint64_t out_stride, uint32_t *out_len, bool float_io, hipStream_t stream) {
  if (!lengths_fit(in_len, out_len, n_streams_)) return SPEEXHIP_ERR_OVERFLOW;  // (engine.h; nothing touched)
  ON_DEVICE();
  // the int16 entry point emits at most 1024 outputs per 160-frame block (its stack buffer,
  // resample.c:982-991); the float entry point has no such cap (resample.c:943)
  const EntryRules rules = entry_rules(float_io);
  for (uint32_t s = 0; s < n_streams_; s++)
    if (!uniform(s)) {
      // channels that the per-channel entry points moved apart: one channel at a time, as the
      // reference's interleaved call does (resample.c:1061-1082)
      if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
      return process_split(d_in, in_len, d_out, out_len, float_io, stream, nullptr);
    }
  std::vector<CallPlan> plans(n_streams_);
  for (uint32_t s = 0; s < n_streams_; s++) {
    plans[s] = plan_call(filter_.num, filter_.den, in_len[s], out_len[s], P(s, 0), rules);
    // resample.c:886: any block run marks the state as started
    if (in_len[s] != 0 && out_len[s] != 0) started_[s] = 1;
  }
  const int rc = run_plans(d_in, in_stride, in_len, d_out, out_stride, plans.data(), float_io, stream);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t s = 0; s < n_streams_; s++) {
    in_len[s] = plans[s].consumed;
    out_len[s] = plans[s].produced;
  }
  // resample.c:1081 (and :962, :1035): with resampler_basic_zero installed every call reports the failure
  return zero_mode_ ? SPEEXHIP_ERR_ALLOC_FAILED : SPEEXHIP_ERR_SUCCESS;
}

// One channel of a single-stream batch from plan.begin to plan.end on device buffers whose frames
// are in_stride / out_stride samples apart (the exact kernel on one channel; bit-exact in both
// modes).  The history ping-pong is per stream, so the channel's new line is copied back beside
// the other channels' lines.
int Batch::run_channel(uint32_t c, const void *d_in, uint32_t in_stride, uint32_t in_frames, void *d_out,
                       uint32_t out_stride, const CallPlan &plan, bool float_io, hipStream_t stream) {
  const uint32_t walked = plan.magic_used + plan.consumed;
  if (float_io) float_seen_ = true;
  if (plan.produced == 0 && walked == 0) return SPEEXHIP_ERR_SUCCESS;
  int chain_rc = chain_to(stream);
  if (chain_rc != SPEEXHIP_ERR_SUCCESS) return chain_rc;
  DescPack pack;
  std::memset(&pack, 0, sizeof(pack));
  StreamDesc &d = pack.d[0];
  // (launch_exact and its kernel read none of k_shift, base_shift, tile_begin, m_total)
  fill_desc(d, 0, c, d_in, d_out, in_frames, plan);
  const ExactStrides strides = {in_stride, out_stride, channels_};
  const ExactGeometry geo = zero_mode_ ? zero_geometry(tables_->plans.geo_ch) : tables_->plans.geo_ch;
  const hipError_t e = launch_exact(filter_, geo, tables_->table, 1, &pack, 1, plan.produced, float_io, stream, &strides, zero_mode_);
  if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  if (d.hist_keep != 0)
    HIP_TRY(hipMemcpy2DAsync(d_hist_[hist_cur_] + c, channels_ * sizeof(float), d_hist_[hist_cur_ ^ 1] + c,
                             channels_ * sizeof(float), sizeof(float), d.hist_keep, hipMemcpyDeviceToDevice,
                             stream));
  return SPEEXHIP_ERR_SUCCESS;
}

// A call on a stream whose channels stand at different positions: channel by channel with the caller's lengths
// restored before each, the lengths of the LAST channel reported (resample.c:1061-1082).  Channel c starts
// `layout.in_channel` / `layout.out_channel` samples into the device buffers and its samples lie `in_sample` /
// `out_sample` apart there: an interleaved buffer is {1, 1, channels, channels}, planes {in_plane_stride,
// out_plane_stride, 1, 1}.
int Batch::process_split(const void *d_in, uint32_t *in_len, void *d_out, uint32_t *out_len, bool float_io,
                         hipStream_t stream, std::vector<CallPlan> *plans_out, const SplitLayout *layout) {
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const SplitLayout interleaved = {1, 1, channels_, channels_};
  const SplitLayout &at = layout != nullptr ? *layout : interleaved;
  const EntryRules rules = entry_rules(float_io);
  const uint32_t want_in = *in_len, want_out = *out_len;
  if (want_in != 0 && want_out != 0) started_[0] = 1;
  for (uint32_t c = 0; c < channels_; c++) {
    const CallPlan plan = plan_call(filter_.num, filter_.den, want_in, want_out, P(0, c), rules);
    const int rc = run_channel(c, d_in ? static_cast<const char *>(d_in) + c * at.in_channel * es : nullptr, at.in_sample, want_in,
                               static_cast<char *>(d_out) + c * at.out_channel * es, at.out_sample, plan, float_io, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    P(0, c) = plan.end;
    *in_len = plan.consumed;
    *out_len = plan.produced;
    if (plans_out) plans_out->push_back(plan);
  }
  return zero_mode_ ? SPEEXHIP_ERR_ALLOC_FAILED : SPEEXHIP_ERR_SUCCESS;
}

// One launch of up to 32 stream descriptors (`descs` = pack.d): the kernel choose_launch (filter_plans.h) selects for the
// mode, the filter's plans and the launch's size.
int Batch::launch_chunk(const StreamDesc *descs, const DescPack &pack, uint32_t n, uint32_t max_out, bool float_io,
                        hipStream_t stream) {
  const DeviceTables &t = *tables_;
  const FilterPlans &p = t.plans;
  const LaunchChoice c = choose_launch(p, filter_, mode_, zero_mode_, float_io, float_seen_, w16_env(), descs, n);
  const bool fixed = mode_ == SPEEXHIP_MODE_FAST_FIXED;  // (kernels.h: no tap-range shares -- an output's bits depend on the stream alone)
  hipError_t e = hipSuccess;
  switch (c.family) {
    case KernelFamily::Zero: {
      e = launch_exact(filter_, zero_geometry(p.geo), t.table, channels_, &pack, n, max_out, float_io, stream, nullptr, true);
      break;
    }
    case KernelFamily::Exact:
      e = launch_exact(filter_, p.geo, t.table, channels_, &pack, n, max_out, float_io, stream);
      break;
    case KernelFamily::Period:
      // (the rows of the fp64 variants are doubles behind the same pointer type)
      e = launch_period(filter_, p.period[c.variant], static_cast<const float *>(t.period_rows[c.variant]),
                        c.with_fine ? &p.period[c.fine] : nullptr,
                        c.with_fine ? static_cast<const float *>(t.period_rows[c.fine]) : nullptr, channels_, descs, &pack, n,
                        c.float_io, stream, fixed);
      break;
    case KernelFamily::Slide:
      e = launch_slide(filter_, p.slide, t.slide_rows, channels_, descs, &pack, n, float_io, stream, fixed);
      break;
    case KernelFamily::Slide64:
      e = launch_slide64(filter_, p.slide64, t.slide64_rows, channels_, descs, &pack, n, float_io, stream, fixed);
      break;
  }
  if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  return SPEEXHIP_ERR_SUCCESS;
}

// Every stream from plans[s].begin to plans[s].end: one launch per 32 streams (kMaxPackedStreams: the descriptors
// of a launch travel in its kernel arguments -- no descriptor copy, no dependent load in the kernels).  in_frames[s]
// = frames readable at the stream's input pointer.
// (Until round 4 a batch of more than 32 streams was ONE launch whose descriptors went through a pinned -> device
//  ring, and every kernel existed twice -- reading its descriptor from the arguments or from the ring: half of the
//  library's code objects, half of its build time and of what a process loads at its first call, for launches that
//  are many generations long anyway; BASELINE configs[4] is 32 streams per GPU.  A launch's ragged end costs ~14 us
//  of a 32-stream launch's ~200: what a 64-stream batch pays for being two launches.)
int Batch::run_plans(const void *d_in, uint64_t in_stride, const uint32_t *in_frames, void *d_out,
                     uint64_t out_stride, const CallPlan *plans, bool float_io, hipStream_t stream) {
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  if (float_io) float_seen_ = true;  // (from here on the histories may hold non-integer samples)
  bool chained = false;
  for (uint32_t s0 = 0; s0 < n_streams_; s0 += kChunk) {
    const uint32_t n = std::min(kChunk, n_streams_ - s0);
    DescPack pack;
    std::memset(&pack, 0, sizeof(pack));
    StreamDesc *descs = pack.d;
    uint32_t max_out = 0;
    bool any_work = false;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t s = s0 + j;
      const CallPlan &plan = plans[s];
      StreamDesc &d = descs[j];
      fill_desc(d, s, 0, d_in ? static_cast<const char *>(d_in) + s * in_stride * es : nullptr,
                static_cast<char *>(d_out) + s * out_stride * es, in_frames[s], plan);
      max_out = std::max(max_out, plan.produced);
      any_work = any_work || plan.produced != 0 || d.consumed != 0;
    }
    if (!any_work) {
      // (nothing to run for these streams -- but the ping-pong below flips for the whole batch: their histories
      //  must move to the other buffer with everybody else's, which the kernels do even for an idle stream)
      bool others = false;
      for (uint32_t s = 0; s < n_streams_ && !others; s++)
        others = plans[s].produced != 0 || plans[s].magic_used + plans[s].consumed != 0;
      if (!others) continue;
    }
    if (!chained) {
      // Calls on one batch are ordered (each reads the history the previous one left and the
      // ping-pong buffers alternate): a call enqueued on another stream than the previous one
      // waits for it on the device.
      const int chain_rc = chain_to(stream);
      if (chain_rc != SPEEXHIP_ERR_SUCCESS) return chain_rc;
      chained = true;
    }
    const int lrc = launch_chunk(descs, pack, n, max_out, float_io, stream);
    if (lrc != SPEEXHIP_ERR_SUCCESS) return lrc;
  }
  if (chained) hist_cur_ ^= 1;
  for (uint32_t s = 0; s < n_streams_; s++)
    for (uint32_t c = 0; c < channels_; c++) P(s, c) = plans[s].end;
  if (!float_io) int16_call_done(plans, n_streams_);
  return SPEEXHIP_ERR_SUCCESS;
}

// Round 6 (VERDICT r5 #7b): ONE float call must not keep a state off its int16 window for good.  float_seen_ says the
// histories may hold samples an int16 image cannot (a float call put them there).  An int16 call that consumes at least
// as many frames as the history it leaves behind (taps - 1 + the pending frames) replaces every one of them with its own
// int16 input: from the next call on the int16-window plans serve again.  (THIS call still ran over the float window: it
// read the old history.)
void Batch::int16_call_done(const CallPlan *plans, uint32_t n) {
  if (!float_seen_) return;
  for (uint32_t s = 0; s < n; s++)
    if (plans[s].consumed < filter_.taps - 1 + plans[s].end.magic) return;
  float_seen_ = false;
}

// The second stream of a piecewise call: one of the pool's shared streams that is NOT this state's own one (on the
// same stream the copies and the launches would simply take turns: correct, but nothing overlaps).
bool Batch::have_copy_stream() {
  if (copy_stream_ != nullptr) return copy_stream_ != own_stream_;
  if (own_stream_ == nullptr && pool::stream_get(device_, &own_stream_) != hipSuccess) return false;
  for (int tries = 0; tries < 4; tries++) {
    hipStream_t s = nullptr;
    if (pool::stream_get(device_, &s) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    if (s != own_stream_) {
      copy_stream_ = s;
      return true;
    }
  }
  return false;
}

// A large owned-block call in `pieces` pieces (process_host_take).  Piece i: input frames [f_i, f_{i+1}) copied on
// copy_stream_, an event behind the copy, and on own_stream_ -- waiting for that event -- one launch for the outputs
// whose windows end inside the frames copied so far.  Output k of the call reads V-frames
// [last0 + (frac0 + k*num) div den, ... + taps) (stream_plan.h), so the count is closed-form; a piece's descriptor is
// the call's with the position advanced by its first output.  A tile's window may reach past the frames copied so far:
// what it stages from there only feeds outputs of later pieces, which this launch does not store.
int Batch::take_in_pieces(const void *in, uint32_t *in_len, uint32_t *out_len, bool float_io, void *blk, uint32_t pieces) {
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const uint32_t frames = *in_len;
  const EntryRules rules = entry_rules(float_io);
  const CallPlan plan = plan_call(filter_.num, filter_.den, frames, *out_len, P(0, 0), rules);
  if (frames != 0 && *out_len != 0) started_[0] = 1;
  const size_t in_bytes = static_cast<size_t>(frames) * channels_ * es;
  DrainOnExit drain(&own_stream_);
  int rc = ensure_stage(in_bytes, 0, 0, 0);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  DrainOnExit drain_copy(&copy_stream_);
  for (uint32_t i = 0; i < pieces; i++)
    if (piece_ev_[i] == nullptr) HIP_TRY(pool::event_get(device_, &piece_ev_[i]));
  rc = chain_to(own_stream_);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (float_io) float_seen_ = true;
  const uint32_t hist_frames = filter_.taps - 1 + plan.begin.magic;
  const int64_t num = filter_.num, den = filter_.den;
  // outputs (of the call's plan.produced) whose windows lie inside history + the first f input frames
  auto outputs_within = [&](uint64_t f) -> uint32_t {
    const int64_t x = static_cast<int64_t>(f) + hist_frames - filter_.taps - plan.begin.last;
    if (x < 0) return 0;
    const int64_t k = ((x + 1) * den - 1 - static_cast<int64_t>(plan.begin.frac)) / num;  // last such output
    return static_cast<uint32_t>(std::min<int64_t>(k + 1, plan.produced));
  };
  // A fast kernel runs every phase of a group over the group's whole zero-padded row (row_len >= taps steps), so an
  // output's accumulator also meets samples up to row_len - taps frames BEHIND its own window -- times zero taps.
  // Behind the frames copied so far the staging buffer holds stale pool memory (or the next piece arriving): as float
  // samples that may be Inf / NaN, and 0 * NaN = NaN.  A piece therefore only stores the outputs whose
  // whole ROW lies inside the frames copied so far: the bound moves back by the longest row any plan of this filter
  // may run (+ one loop iteration of prefetch).
  uint32_t guard = 0;
  // (kPeriod64W16 has never counted here, and need not: its launches read int16 samples, which hold no NaN.  Left out so
  //  that the pieces of a call end where they always did.)
  for (int v = 0; v < kPeriodVariants; v++) {
    const PeriodPlan &t = tables_->plans.period[v];
    if (v != kPeriod64W16 && t.usable && t.row_len > filter_.taps) guard = std::max(guard, t.row_len - filter_.taps);
  }
  for (const SlidePlan *t : {&tables_->plans.slide, &tables_->plans.slide64})
    if (t->usable && t->row_len > filter_.taps) guard = std::max(guard, t->row_len - filter_.taps + t->p * t->num);
  guard += 16;
  uint32_t done_out = 0;
  for (uint32_t i = 0; i < pieces; i++) {
    const uint64_t f0 = static_cast<uint64_t>(frames) * i / pieces, f1 = static_cast<uint64_t>(frames) * (i + 1) / pieces;
    const size_t off = static_cast<size_t>(f0) * channels_ * es, bytes = static_cast<size_t>(f1 - f0) * channels_ * es;
    if (bytes != 0) HIP_TRY(hipMemcpyAsync(d_stage_in_ + off, static_cast<const char *>(in) + off, bytes, hipMemcpyHostToDevice, copy_stream_));
    HIP_TRY(hipEventRecord(piece_ev_[i], copy_stream_));
    HIP_TRY(hipStreamWaitEvent(own_stream_, piece_ev_[i], 0));
    const bool last = i + 1 == pieces;
    const uint32_t upto = last ? plan.produced : std::max(done_out, outputs_within(f1 > guard ? f1 - guard : 0));
    const uint32_t n_out = upto > done_out ? upto - done_out : 0;
    if (n_out == 0 && !last) continue;
    // the piece's first output: the call's position advanced by done_out outputs
    const uint64_t adv = static_cast<uint64_t>(plan.begin.frac) + static_cast<uint64_t>(done_out) * filter_.num;
    StreamPos at = plan.begin;
    at.last = plan.begin.last + static_cast<int32_t>(adv / filter_.den);
    at.frac = static_cast<uint32_t>(adv % filter_.den);
    DescPack pack;
    std::memset(&pack, 0, sizeof(pack));
    StreamDesc &d = pack.d[0];
    d.in = d_stage_in_;
    d.hist = d_hist_[hist_cur_];
    d.out = static_cast<char *>(blk) + static_cast<size_t>(done_out) * channels_ * es;
    d.hist_next = d_hist_[hist_cur_ ^ 1];
    d.in_frames = frames;
    // (the history moves once, with the last piece)
    set_position(d, filter_, at, n_out, plan.magic_used + plan.consumed, hist_frames, last ? filter_.taps - 1 + plan.end.magic : 0);
    rc = launch_chunk(pack.d, pack, 1, n_out, float_io, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    done_out = upto;
  }
  hist_cur_ ^= 1;
  HIP_TRY(hipStreamSynchronize(own_stream_));  // (behind the last launch, which waited for the last copy)
  drain.armed = false;
  drain_copy.armed = false;
  for (uint32_t c = 0; c < channels_; c++) P(0, c) = plan.end;
  if (!float_io) int16_call_done(&plan, 1);
  *in_len = plan.consumed;
  *out_len = plan.produced;
  return SPEEXHIP_ERR_SUCCESS;
}

// Host buffer in, result in a pinned block the caller owns afterwards (the N-API addon wraps it in an external
// Buffer: src/index.ts:111-115 returns a fresh, caller-owned Buffer, and so does this -- without the copy into it).
// The kernel writes the block directly: small calls as before (they already wrote pinned memory, then the result
// was copied out of it: 0.18 us per KB), large ones instead of a device buffer + a copy back.  States whose
// channels stand apart and the zero fallback take the ordinary path into the block.
int Batch::process_host_take(const void *in, uint32_t *in_len, uint32_t *out_len, bool float_io, void **block) {
  *block = nullptr;
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  ON_DEVICE();
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const uint32_t frames = *in_len;
  const bool split = !uniform(0);
  const size_t in_bytes = static_cast<size_t>(frames) * channels_ * es;
  const size_t out_bytes = static_cast<size_t>(will_make(frames, *out_len)) * channels_ * es;
  // (+ 64 bytes behind the samples: the completion word)  Nothing has touched the state yet: without a block the
  // caller makes the copying call instead.
  void *blk = nullptr;
  if (!pool::block_get(&blk, out_bytes + 128)) return SPEEXHIP_ERR_NO_BLOCK;
  struct Guard {
    void *p;
    ~Guard() {
      if (p != nullptr) (void)pool::block_put(p);
    }
  } guard{blk};
  int rc;
  // Large calls in pieces (round 4): PCIe is full duplex, and with the kernel writing the result block itself the
  // two directions belong to different engines -- the input copies run on a second stream, and behind each an event
  // lets a launch for the outputs that piece completes start while the next piece is still arriving.  No kernel
  // change: a piece is a StreamDesc of the same call that begins o_i outputs later (positions advanced in integers)
  // and only the last one rolls the history.  SPEEXHIP_PIECES=1 turns it off, =n forces n (A/B, tests).
  const uint32_t env_pieces = static_cast<uint32_t>(std::max(0, diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_PIECES"), 0)));
  uint32_t pieces = env_pieces > 0 ? env_pieces : static_cast<uint32_t>(in_bytes / kPieceBytes);
  pieces = std::min<uint32_t>(pieces, env_pieces > 0 ? kMaxPieces : 4);  // (the rule: at most four; up to kMaxPieces when forced)
  // Round 6: an input the caller left in pinned memory (speexhip_block_acquire, or memory it pinned itself) is read where
  // it lies -- ONE launch whose loads and stores cross PCIe in opposite directions at the same time, no staging copy, no
  // second stream (the pieces above overlap the two directions only partly and pay ~15 us per piece for it).
  // The result is the block (InPlace); the input takes the rule of host_transfer.h.
  HostCallShape shape;
  shape.take = true;
  const void *pin_in = nullptr;
  void *no_out = nullptr;
  if (!split && !zero_mode_) pinned_sides(in, in_bytes, nullptr, 0, &pin_in, &no_out);
  shape.in = flat_side(in != nullptr, pin_in != nullptr, in_bytes);
  shape.out = flat_side(true, true, out_bytes);
  const HostRoute route = route_host_call(shape);
  if (split || zero_mode_) {
    rc = process_host(in, in_len, blk, out_len, float_io);
    if (!ran(rc)) return rc;
  } else if (route.in == Via::Copy && pieces >= 2 && frames < 0x40000000u && have_copy_stream()) {
    rc = take_in_pieces(in, in_len, out_len, float_io, blk, pieces);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  } else {
    HostCall call(this);
    const HostPiece piece = {in, 0, in_bytes};
    call.word = static_cast<char *>(blk) + align64(out_bytes);  // (behind the samples, in the block)
    rc = call.begin(route, &piece, 1, pin_in, blk);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    rc = process_device(call.src, 0, in_len, call.dst, 0, out_len, float_io, own_stream_);
    if (!ran(rc)) return rc;
    const int wrc = call.finish_whole(blk, static_cast<size_t>(*out_len) * channels_ * es);
    if (wrc != SPEEXHIP_ERR_SUCCESS) return wrc;
  }
  if (*out_len == 0) return rc;  // (the guard returns the block)
  guard.p = nullptr;
  *block = blk;
  return rc;
}

void Batch::release_block(void *block) { (void)pool::block_put(block); }

int Batch::process_host(const void *in, uint32_t *in_len, void *out, uint32_t *out_len, bool float_io) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  ON_DEVICE();
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const bool split = !uniform(0);
  // only as many output frames as this call can produce need a device buffer
  const size_t in_bytes = static_cast<size_t>(*in_len) * channels_ * es;
  const size_t out_bytes = static_cast<size_t>(will_make(*in_len, *out_len)) * channels_ * es;
  // (channels at different positions write different numbers of frames: the block is fetched whole and the caller handed
  //  only the samples each channel really wrote, so nothing is used in place there)
  const void *pin_in = nullptr;
  void *pin_out = nullptr;
  if (!split) pinned_sides(in, in_bytes, out, out_bytes, &pin_in, &pin_out);
  HostCallShape shape;
  shape.split = split;
  shape.in = flat_side(in != nullptr, pin_in != nullptr, in_bytes);
  shape.out = flat_side(true, pin_out != nullptr, out_bytes);
  HostCall call(this);
  const HostPiece piece = {in, 0, in_bytes};
  int rc = call.begin(route_host_call(shape), &piece, 1, pin_in, pin_out);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  std::vector<CallPlan> plans;
  rc = split ? process_split(call.src, in_len, call.dst, out_len, float_io, own_stream_, &plans)
             : process_device(call.src, 0, in_len, call.dst, 0, out_len, float_io, own_stream_);
  if (!ran(rc)) return rc;
  const int frc = split ? call.finish_samples(out, channels_, channels_, es, made_per_channel(channels_, 0, plans.data()).data())
                        : call.finish_whole(out, static_cast<size_t>(*out_len) * channels_ * es);
  return frc != SPEEXHIP_ERR_SUCCESS ? frc : rc;
}

// speex_resampler_process_int / _process_float (resample.c:927-1036): ONE channel, host buffers
// whose samples are in_stride_ / out_stride_ apart (resample.c:1170-1188).  The samples travel as a
// dense line; the state's other channels are not touched.
int Batch::process_channel_host(uint32_t c, const void *in, uint32_t *in_len, void *out, uint32_t *out_len,
                                bool float_io) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  if (c >= channels_) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, 1)) return SPEEXHIP_ERR_OVERFLOW;
  ON_DEVICE();
  const size_t es = float_io ? sizeof(float) : sizeof(int16_t);
  const EntryRules rules = entry_rules(float_io);
  const uint32_t frames = *in_len;
  const CallPlan plan = plan_call(filter_.num, filter_.den, frames, *out_len, P(0, c), rules);
  if (frames != 0 && *out_len != 0) started_[0] = 1;
  HostCallShape shape;
  shape.strided = true;
  shape.in = flat_side(in != nullptr, false, static_cast<size_t>(frames) * es);
  shape.out = flat_side(true, false, static_cast<size_t>(plan.produced) * es);
  HostCall call(this);
  const HostPiece line = {in, 0, shape.in.image};
  call.line_step = in_stride_;
  call.line_es = es;
  int rc = call.begin(route_host_call(shape), &line, 1, nullptr, nullptr);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  rc = run_channel(c, call.src, 1, frames, call.dst, 1, plan, float_io, own_stream_);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  rc = call.finish_samples(out, 1, out_stride_, es, &plan.produced);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  P(0, c) = plan.end;
  *in_len = plan.consumed;
  *out_len = plan.produced;
  return zero_mode_ ? SPEEXHIP_ERR_ALLOC_FAILED : SPEEXHIP_ERR_SUCCESS;
}

// A sequence of calls on one stream as one transfer and (normally) one launch.  Every output
// is a function of (history ++ the frames consumed so far) and its own index; call boundaries
// only decide the counters.  So: plan the calls one after the other on the host (integers),
// pack the frames each call really consumes back to back, and run the stream from the first
// call's begin state to the last call's end state.  One exception: a capacity-bound call that
// leaves input unconsumed -- its last outputs may still have read the first frame it then drops
// (up-sampling: several outputs share one newest frame), while the next call sees its own first
// frame in that slot.  Such a call closes a launch group: it keeps that one extra frame
// readable, and the calls after it start a new launch on the same stream.
int Batch::process_host_chunks(uint32_t n_chunks, const void *const *in, uint32_t *in_len, void *out,
                               uint32_t *out_len, bool float_io) {
  if (n_streams_ != 1) return SPEEXHIP_ERR_BAD_STATE;
  ON_DEVICE();
  const size_t fb = (float_io ? sizeof(float) : sizeof(int16_t)) * channels_;  // bytes per frame
  if (!uniform(0) || zero_mode_) {  // rare states: the separate calls, one after the other
    int last = SPEEXHIP_ERR_SUCCESS;
    char *o = static_cast<char *>(out);
    for (uint32_t i = 0; i < n_chunks; i++) {
      last = process_host(in != nullptr ? in[i] : nullptr, &in_len[i], o, &out_len[i], float_io);
      if (!ran(last)) return last;
      o += static_cast<size_t>(out_len[i]) * fb;
    }
    return last;
  }
  const EntryRules rules = entry_rules(float_io);
  struct Group {
    CallPlan fused;
    uint64_t in_off = 0, out_off = 0;  // frames into the staging buffers
    uint32_t readable = 0;             // frames at in_off the launch may read
  };
  std::vector<CallPlan> plans(n_chunks);
  std::vector<Group> groups;
  StreamPos pos = P(0, 0);
  uint64_t frames = 0, made = 0;
  bool open = false;
  for (uint32_t i = 0; i < n_chunks; i++) {
    plans[i] = plan_call(filter_.num, filter_.den, in_len[i], out_len[i], pos, rules);
    pos = plans[i].end;
    if (in_len[i] != 0 && out_len[i] != 0) started_[0] = 1;
    if (!open) {
      Group g;
      g.fused.begin = plans[i].begin;
      g.in_off = frames;
      g.out_off = made;
      groups.push_back(g);
      open = true;
    }
    Group &g = groups.back();
    g.fused.end = plans[i].end;
    g.fused.magic_used += plans[i].magic_used;
    g.fused.consumed += plans[i].consumed;
    g.fused.produced += plans[i].produced;
    g.readable += plans[i].consumed;
    frames += plans[i].consumed;
    made += plans[i].produced;
    if (plans[i].consumed < in_len[i]) {  // dropped input: one more frame stays readable
      g.readable += 1;
      frames += 1;
      open = false;
    }
    if (frames > 0x7fffffffull || made > 0x7fffffffull) return SPEEXHIP_ERR_OVERFLOW;
  }
  // Small runs -- what a Transform holds back, eight 64 KiB chunks say -- are all latency, like small single calls
  // (process_host): the kernels read the pinned bounce buffer and write the pinned result buffer straight through
  // PCIe, one wait, no copy-engine hand-overs.  (Until round 5 every coalesced run went through the device staging
  // buffers: H2D copy, launch, D2H copy -- three in-order steps of ~10 us hand-over each -- and `coalesceChunks: 8` was
  // SLOWER than the plain pipe on four of the reference's seven test tuples, profiles/r04_node_bench.json.)
  HostCallShape shape;
  shape.gathered = true;
  shape.in = flat_side(true, false, frames * fb);  // (a null chunk is gathered too, as zeros)
  shape.out = flat_side(true, false, made * fb);
  std::vector<HostPiece> pieces(n_chunks);
  size_t off = 0;
  for (uint32_t i = 0; i < n_chunks; i++) {  // frames a call drops never reach the GPU
    const size_t bytes = (plans[i].consumed + (plans[i].consumed < in_len[i] ? 1u : 0u)) * fb;
    pieces[i] = {in != nullptr ? in[i] : nullptr, off, bytes};
    off += bytes;
  }
  HostCall call(this);
  int rc = call.begin(route_host_call(shape), pieces.data(), n_chunks, nullptr, nullptr);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (const Group &g : groups) {
    rc = run_plans(static_cast<const char *>(call.src) + g.in_off * fb, 0, &g.readable, static_cast<char *>(call.dst) + g.out_off * fb,
                   0, &g.fused, float_io, own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  rc = call.finish_whole(out, made * fb);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (uint32_t i = 0; i < n_chunks; i++) {
    in_len[i] = plans[i].consumed;
    out_len[i] = plans[i].produced;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

// ---- warm-up (speexhip_warmup) ------------------------------------------------------------------------------------
// What the FIRST state of a process pays that has nothing to do with the state: the runtime's own start (the first HIP
// call, 90-180 ms), the first stream (20 ms; 160 ms when it is also the runtime's first), each further shared stream
// (~8 ms for the second to fourth state), the first copy (~8 ms: the copy engines' queues) -- against 0.04 ms of filter
// design and 0.2 ms of uploads (profiles/r05_first_call_trace.txt).  The reference pays its counterpart -- compiling
// the WASM module -- when the module is imported, behind SpeexResampler.initPromise (src/index.ts:18-19, :31); so does
// the drop-in: the addon runs this on a pool thread at import and initPromise resolves behind it.
int warm_device(int device) {
  DeviceScope scope(device);
  HIP_TRY(scope.error());
  HIP_TRY(pool::streams_prewarm(device));
  hipStream_t s = nullptr;
  HIP_TRY(pool::stream_get(device, &s));
  void *d = nullptr;
  HIP_TRY(pool::device_get(device, &d, kCtlCopyMin));
  const std::vector<char> zeros(kCtlCopyMin, 0);
  const int rc = ctl_upload(d, zeros.data(), zeros.size(), s);  // (pinned image -> device through the copy engines)
  pool::device_put(device, d);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // the code objects (kernels.h, SPEEXHIP_WARM_UNIT): one empty launch per translation unit
  warm_unit_period(s);
  warm_unit_slide_i16(s);
  warm_unit_exact(s);
  warm_unit_period64(s);
  warm_unit_slide64_i16(s);
  warm_unit_period_pp(s);
  warm_unit_period_odd(s);
  warm_unit_period_frames(s);
  warm_unit_period64_w16(s);
  warm_unit_period_w16g(s);
  warm_unit_slide_f32(s);
  warm_unit_slide64_f32(s);
  warm_unit_planar(s);
  warm_unit_convert(s);
  warm_unit_convert_many(s);
  warm_unit_mix(s);
  warm_unit_sides(s);
  warm_unit_bus(s);
  warm_unit_bus_legs(s);
  warm_unit_levels(s);
  HIP_TRY(hipStreamSynchronize(s));
  return SPEEXHIP_ERR_SUCCESS;
}

int warmup(int device) {
  const int count = devices::count();
  if (count <= 0) {
    g_last_error = "HIP device error: no GPU visible (libspeexhip has no CPU fallback)";
    return SPEEXHIP_ERR_DEVICE;
  }
  if (device >= count) return SPEEXHIP_ERR_INVALID_ARG;
  if (device >= 0) return warm_device(device);
  int list[64], n = 0;
  devices::placement_candidates(list, &n, 64);
  if (n == 0) {
    g_last_error = "HIP device error: SPEEXHIP_DEVICE / SPEEXHIP_DEVICES names a device this node does not have";
    return SPEEXHIP_ERR_DEVICE;
  }
  for (int k = 0; k < n; k++) {
    const int rc = warm_device(list[k]);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

}  // namespace speexhip
