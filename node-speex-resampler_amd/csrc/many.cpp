// many.cpp -- the host-buffer calls of many single-stream states at once (engine.h: process_host_many,
// process_host_many_sides through many_run): product code.
#include "engine.h"

#include "devices.h"
#include "engine_detail.h"
#include "host_transfer.h"
#include "pool.h"
#include "unit_workers.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

namespace speexhip {
using namespace detail;  // (engine_detail.h: HIP_TRY, DeviceScope, DrainOnExit, the staging helpers)

// ---- host-buffer calls of many single-stream states at once (engine.h) ---------------------------------------------
namespace {
// Staging of the many-states call: one per logical device, grow-only, taken from the pool and kept for the life of the
// process like the shared streams.  A call holds the lock of every device it touches from its first copy to its last.
struct ManyStage {
  std::mutex mu;
  hipStream_t stream = nullptr, copy_stream = nullptr;  // (copy_stream + events: the pipelined large path)
  std::vector<hipEvent_t> events;
  char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
  size_t d_in_cap = 0, d_out_cap = 0, h_in_cap = 0, h_out_cap = 0;
  // the float images of the entries whose storage is not the image (ManyEntry::Image): device scratch either side of the
  // FIR launch, one range per entry
  char *d_img_in = nullptr, *d_img_out = nullptr;
  size_t d_img_in_cap = 0, d_img_out_cap = 0;
  uint32_t seq = 0;
};
// speexhip_debug_many_counters: FIR launches, input passes, output passes, entries that took their own call
std::atomic<uint64_t> g_many_counters[4];
inline void count_many(int which, uint64_t by = 1) { g_many_counters[which].fetch_add(by, std::memory_order_relaxed); }
inline size_t align128(size_t v) { return (v + 127) & ~static_cast<size_t>(127); }
// (device, lane): a large call on one device runs as two halves side by side, each on a stage of its own (below)
ManyStage &many_stage(int device, int lane) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, ManyStage *> *all = new std::map<std::pair<int, int>, ManyStage *>();  // never destroyed, like the pool
  std::lock_guard<std::mutex> lock(mu);
  ManyStage *&m = (*all)[std::make_pair(device, lane)];
  if (m == nullptr) m = new ManyStage();
  return *m;
}

// The stage's copy stream: a stream of its own that carries host -> device copies and NOTHING else, made and primed here.
// Why (late in round 6; profiles/r06_engine_log.txt, r06_pinned_in_leg.txt): the runtime picks a copy engine per stream --
// for a copy in, the lowest engine free at the moment it asks; for a copy out, the engine ROCr recommends for that
// direction (0x2 on this box) -- and then KEEPS it for that stream whatever the direction of the stream's later copies.
// The pool's streams are shared with every state's own calls, which copy both ways: a copy stream that had last carried
// a state's results kept engine 0x2 for the inputs of the next many-states call, the 32 queued copies in of a call over
// pinned chunks went ahead of every copy out on that one engine, and the call took 6.0-6.3 ms instead of 4.0 (pageable
// chunks: 5.5 instead of 3.8) -- or not, depending on which calls the process had made before.  A stream that only ever
// copies in asks once, here, one stage at a time and with its copy waited for, so that the lowest engine is free when
// the next stage asks: every stage's inputs travel on engine 0x1, the results on 0x2 / 0x4.
int prime_copy_stream(int device, ManyStage &ms) {
  static std::mutex one_at_a_time;
  std::lock_guard<std::mutex> lock(one_at_a_time);
  if (ms.copy_stream != nullptr) return SPEEXHIP_ERR_SUCCESS;
  DeviceScope scope(device);
  HIP_TRY(scope.error());
  hipStream_t s = nullptr;
  HIP_TRY(pool::stream_own(device, &s));
  const size_t bytes = 64 * 1024;  // (above the 16 KiB the runtime copies with a kernel: a copy ENGINE must be asked for)
  void *h = nullptr, *d = nullptr;
  hipEvent_t e = nullptr;
  int rc = SPEEXHIP_ERR_SUCCESS;
  if (hip_failed(pool::pinned_get(&h, bytes), "hipHostMalloc") || hip_failed(pool::device_get(device, &d, bytes), "hipMalloc") ||
      hip_failed(pool::event_get(device, &e), "hipEventCreate") ||
      hip_failed(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (priming)") ||
      hip_failed(hipEventRecord(e, s), "hipEventRecord") ||
      // (the EVENT is waited for, not the stream: the stream is never synchronised, the engine it was given stays its own)
      hip_failed(hipEventSynchronize(e), "hipEventSynchronize"))
    rc = SPEEXHIP_ERR_DEVICE;
  if (e != nullptr) pool::event_put(device, e);
  if (d != nullptr) pool::device_put(device, d);
  if (h != nullptr) pool::pinned_put(h);
  if (rc != SPEEXHIP_ERR_SUCCESS) {
    (void)hipStreamDestroy(s);
    return rc;
  }
  ms.copy_stream = s;
  return SPEEXHIP_ERR_SUCCESS;
}
}  // namespace

// The fused states of ONE device: idx = their positions in the caller's arrays.
int Batch::many_on_device(int device, int lane, const std::vector<uint32_t> &idx, const ManyEntry *entries, uint32_t *in_len,
                          uint32_t *out_len, int *rcs) {
  ManyStage &ms = many_stage(device, lane);
  std::lock_guard<std::mutex> lock(ms.mu);
  DeviceScope device_scope(device);
  HIP_TRY(device_scope.error());
  if (ms.stream == nullptr) HIP_TRY(pool::stream_get(device, &ms.stream));
  DrainOnExit drain(&ms.stream);
  struct Item {
    uint32_t i;
    Batch *b;
    const ManyEntry *e;
    const void *in;                               // the caller's buffers (raw bytes of e->in_fmt / e->out_fmt)
    void *out;
    bool float_io;                                // the FIR launch's sample type: int16 direct, or float (direct or images)
    bool pass_in, pass_out;                       // the entry's storage goes through a float image on that side
    size_t img_in, img_out;                       // ... at this offset of the stage's images
    CallPlan plan;
    size_t in_bytes, out_bytes, in_off, out_off;
    const void *pin_in;                           // round 6: the caller's own buffers where they are pinned memory
    void *pin_out;                                // (pinned_view): the kernels read / write them directly
    Via in_via, out_via;                          // host_transfer.h
    bool work;
  };
  std::vector<Item> items(idx.size());
  size_t total_in = 0, total_out = 0;  // pageable bytes, as laid out in the stage
  size_t images_in = 0, images_out = 0;
  for (size_t k = 0; k < idx.size(); k++) {
    Item &it = items[k];
    it.i = idx[k];
    it.e = &entries[it.i];
    it.b = it.e->b;
    it.in = it.e->in;
    it.out = it.e->out;
    it.float_io = it.e->kind != ManyEntry::Int16;
    EntryRules rules;
    rules.block_in = it.b->block_in();
    rules.float_entry = it.float_io;
    it.plan = plan_call(it.b->filter_.num, it.b->filter_.den, in_len[it.i], out_len[it.i], it.b->P(0, 0), rules);
    // the raw bytes of either side, in the side's own format: what every size decision below goes by
    it.in_bytes = it.in != nullptr ? static_cast<size_t>(in_len[it.i]) * it.b->channels_ * sample_bytes(it.e->in_fmt) : 0;
    it.out_bytes = static_cast<size_t>(it.plan.produced) * it.b->channels_ * sample_bytes(it.e->out_fmt);
    // (formats.cpp, process_sides_device: F32 storage IS the image; a present but empty input is not silence, no frame of
    //  it is read)
    it.pass_in = it.e->kind == ManyEntry::Image && it.e->in_fmt != SPEEXHIP_FMT_F32 && it.in != nullptr && in_len[it.i] != 0;
    it.pass_out = it.e->kind == ManyEntry::Image && it.e->out_fmt != SPEEXHIP_FMT_F32;
    it.img_in = images_in;
    it.img_out = images_out;
    if (it.pass_in) images_in += align128(static_cast<size_t>(in_len[it.i]) * it.b->channels_ * sizeof(float));
    if (it.pass_out) images_out += align128(static_cast<size_t>(it.plan.produced) * it.b->channels_ * sizeof(float));
    it.pin_in = pinned_view(it.in, it.in_bytes);
    it.pin_out = pinned_view(it.out, it.out_bytes);
    if (it.pin_in != nullptr && it.pin_out != nullptr && buffers_overlap(it.in, it.in_bytes, it.out, it.out_bytes)) it.pin_in = nullptr;
    // (a pinned input whose result goes to a LARGE pageable buffer is copied like any other -- from pinned memory the copy
    //  is a plain DMA -- so that the call can take the pipelined path, inputs arriving while results leave: read in place,
    //  all the reads come first and all the pageable copies out after them, 32 x 2^20 stereo frames 5.4 ms against 4.0,
    //  profiles/r06_bench_driver_form_v2.json)
    if (it.pin_in != nullptr && it.pin_out == nullptr && it.out_bytes >= kDirectCopyBytes &&
        diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_PIN_IN_COPY"), 1) != 0)  // (A/B: 0 = read in place even then)
      it.pin_in = nullptr;
    it.work = it.plan.produced != 0 || it.plan.magic_used + it.plan.consumed != 0;
    total_in += align64(it.pin_in != nullptr ? 0 : it.in_bytes);
    total_out += align64(it.pin_out != nullptr ? 0 : it.out_bytes);
  }
  // Every side by the rule of host_transfer.h, the call's pageable totals deciding whether it is small.  Small calls (a
  // server's 10-20 ms frames, a Transform's 64 KiB chunks) run on pinned memory alone; larger ones gather their Staged
  // buffers in the pinned buffer, which travels as ONE copy each way.
  const bool small = small_call(total_in, total_out);
  Wait wait;
  bool all_big = true;  // every working state Copy both ways: the pipelined path (below)
  for (Item &it : items) {
    it.in_via = route_side(it.in_bytes, it.in != nullptr, it.pin_in != nullptr, small);
    it.out_via = route_side(it.out_bytes, true, it.pin_out != nullptr, small);
    wait.add(it.in_via, it.in_bytes);
    wait.add(it.out_via, it.out_bytes);
    if (it.work && (it.in_via != Via::Copy || it.out_via != Via::Copy)) all_big = false;
  }
  // layout: the gathered buffers first (one contiguous range = one copy), then the Copy ones
  auto through_stage = [](Via v, size_t bytes) { return v == Via::InPlace ? 0 : bytes; };
  size_t gathered_in = 0, gathered_out = 0, off_in = 0, off_out = 0;
  for (int pass = 0; pass < 2; pass++)
    for (Item &it : items) {
      if ((it.in_via == Via::Copy) == (pass == 1)) {
        it.in_off = off_in;
        off_in += align64(through_stage(it.in_via, it.in_bytes));
        if (pass == 0) gathered_in = off_in;
      }
      if ((it.out_via == Via::Copy) == (pass == 1)) {
        it.out_off = off_out;
        off_out += align64(through_stage(it.out_via, it.out_bytes));
        if (pass == 0) gathered_out = off_out;
      }
    }
  int rc = grow_stage(device, &ms.h_in, &ms.h_in_cap, gathered_in, true);
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = grow_stage(device, &ms.h_out, &ms.h_out_cap, gathered_out + 128, true);
  if (rc == SPEEXHIP_ERR_SUCCESS && !small) rc = grow_stage(device, &ms.d_in, &ms.d_in_cap, total_in, false);
  if (rc == SPEEXHIP_ERR_SUCCESS && !small) rc = grow_stage(device, &ms.d_out, &ms.d_out_cap, total_out, false);
  // (a line of slack behind the last image, as the single call's pitched images have behind every stream)
  if (rc == SPEEXHIP_ERR_SUCCESS && images_in != 0) rc = grow_stage(device, &ms.d_img_in, &ms.d_img_in_cap, images_in + 256, false);
  if (rc == SPEEXHIP_ERR_SUCCESS && images_out != 0) rc = grow_stage(device, &ms.d_img_out, &ms.d_img_out_cap, images_out + 256, false);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  char *src_base = small ? ms.h_in : ms.d_in, *dst_base = small ? ms.h_out : ms.d_out;

  // Large calls in pieces (below): a launch then carries about 16 MB of input, so that the transfer of the next
  // piece and the results of the previous one have something to overlap with.
  static const int env_pipe = diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_MANY_PIPELINE"), -1);  // A/B: 0 off
  const bool pipelined = all_big && env_pipe != 0 && total_in >= (static_cast<size_t>(32) << 20);
  // launches: the states that share (tables, mode, window format, sample type of the launch) go together, at most 32 per
  // launch
  std::vector<std::vector<Item *>> launches;
  {
    std::map<std::tuple<const void *, int, bool, bool>, std::vector<Item *>> groups;
    for (Item &it : items) {
      if (it.float_io) it.b->float_seen_ = true;
      if (in_len[it.i] != 0 && out_len[it.i] != 0) it.b->started_[0] = 1;  // resample.c:886
      if (!it.work) continue;  // nothing to run: the state stays where it is
      groups[std::make_tuple(static_cast<const void *>(it.b->tables_.get()), it.b->mode_, it.b->float_seen_, it.float_io)].push_back(&it);
    }
    for (auto &kv : groups) {
      std::vector<Item *> &g = kv.second;
      size_t per = kMaxPackedStreams;
      if (pipelined) {
        size_t bytes = 0;
        for (Item *it : g) bytes += it->in_bytes;
        const size_t pieces = std::max<size_t>(1, bytes / (static_cast<size_t>(16) << 20));
        per = std::min<size_t>(kMaxPackedStreams, std::max<size_t>(1, (g.size() + pieces - 1) / pieces));
      }
      for (size_t g0 = 0; g0 < g.size(); g0 += per)
        launches.emplace_back(g.begin() + g0, g.begin() + std::min(g.size(), g0 + per));
    }
  }
  auto commit_item = [&](Item &it) {  // counters and position of one state
    for (uint32_t c = 0; c < it.b->channels_; c++) it.b->P(0, c) = it.plan.end;
    if (!it.float_io && it.work) it.b->int16_call_done(&it.plan, 1);
    in_len[it.i] = it.plan.consumed;
    out_len[it.i] = it.plan.produced;
    // (a formatted call of a state with dither on moves its position by the frames produced, whatever the format)
    if (it.e->sides && it.b->dither_on()) it.b->dither_advance(&out_len[it.i]);
    rcs[it.i] = SPEEXHIP_ERR_SUCCESS;
  };
  // one launch of `launches[k]` on `stream`
  auto launch = [&](const std::vector<Item *> &g, hipStream_t stream) -> int {
    const uint32_t cnt = static_cast<uint32_t>(g.size());
    const bool float_io = g[0]->float_io;  // (the group's: part of its key)
    DescPack pack;
    std::memset(&pack, 0, sizeof(pack));
    // the passes either side of the launch (kernels_convert_many.hip): one each for all the formats the group's entries
    // name, over the entries whose storage is not their image
    ConvertPack to_image, from_image;
    DitherPack dith;
    uint64_t most_to = 0, most_from = 0;
    std::memset(&to_image, 0, sizeof(to_image));
    std::memset(&from_image, 0, sizeof(from_image));
    std::memset(&dith, 0, sizeof(dith));
    uint32_t max_out = 0;
    for (uint32_t j = 0; j < cnt; j++) {
      Item &it = *g[j];
      Batch *b = it.b;
      const int crc = b->chain_to(stream);  // (each state's calls stay ordered, whatever stream its last one ran on)
      if (crc != SPEEXHIP_ERR_SUCCESS) return crc;
      const void *storage_in = it.in == nullptr ? nullptr : it.pin_in != nullptr ? it.pin_in : src_base + it.in_off;
      void *storage_out = it.pin_out != nullptr ? it.pin_out : dst_base + it.out_off;
      b->fill_desc(pack.d[j], 0, 0, it.pass_in ? ms.d_img_in + it.img_in : storage_in,
                   it.pass_out ? ms.d_img_out + it.img_out : storage_out, in_len[it.i], it.plan);
      if (it.pass_in) {
        ConvertStream &c = to_image.s[j];
        c.src = storage_in, c.dst = ms.d_img_in + it.img_in;
        c.n = static_cast<uint64_t>(in_len[it.i]) * b->channels_;
        c.step = 1;
        c.reserved = convert_many_tag(it.e->in_fmt, SPEEXHIP_DITHER_NONE);
        most_to = std::max(most_to, c.n);
      }
      if (it.pass_out && it.plan.produced != 0) {
        ConvertStream &c = from_image.s[j];
        c.src = ms.d_img_out + it.img_out, c.dst = storage_out;
        c.n = static_cast<uint64_t>(it.plan.produced) * b->channels_;
        c.step = 1;
        const bool dithered = b->dither_on() && dithered_fmt(it.e->out_fmt);
        c.reserved = convert_many_tag(it.e->out_fmt, dithered ? b->dither_kind_ : SPEEXHIP_DITHER_NONE);
        if (dithered) dith.s[j] = b->dither_pack(0, 1, b->channels_).s[0];
        most_from = std::max(most_from, c.n);
      }
      max_out = std::max(max_out, it.plan.produced);
    }
    if (most_to != 0) {
      if (hip_failed(launch_convert_many(false, to_image, dith, cnt, most_to, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
      count_many(1);
    }
    const int lrc = g[0]->b->launch_chunk(pack.d, pack, cnt, max_out, float_io, stream);
    if (lrc != SPEEXHIP_ERR_SUCCESS) return lrc;
    count_many(0);
    if (most_from != 0) {
      if (hip_failed(launch_convert_many(true, from_image, dith, cnt, most_from, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
      count_many(2);
    }
    // A state moves as ONE step, the moment its launch is queued: the history ping-pong, the position and the counters
    // together.  (Until round 6 the flip happened here and the positions behind the last launch of the call: a later
    // group's failure left the earlier groups' states with a flipped history and their OLD position -- silently corrupt
    // for every later call, ADVICE r5.  Now a failure further on costs such a state this call's audio -- its code says
    // so -- and nothing else; states whose launch was never queued have not moved at all.)
    for (uint32_t j = 0; j < cnt; j++) {
      g[j]->b->hist_cur_ ^= 1;
      commit_item(*g[j]);
    }
    return SPEEXHIP_ERR_SUCCESS;
  };
  auto commit = [&]() {  // ... and the states with nothing to run: counters of an empty call, position unchanged
    for (Item &it : items)
      if (!it.work) commit_item(it);
  };

  if (pipelined && launches.size() >= 2) {
    // Large calls, pipelined (round 5).  PCIe is full duplex, but the runtime's pageable copies keep the thread that
    // issues them busy until they are staged, so one thread alone moves inputs, computes, and moves results strictly
    // one after the other: 32 streams x 2^20 stereo frames 5.8 ms, of which 0.2 are the kernel.  Here the calling
    // thread copies the inputs of launch after launch on the stage's copy stream (an event behind each launch's
    // inputs), while a second thread waits for the events, runs the launches on the stage's stream and copies each
    // launch's results out behind it: results leave while the next inputs arrive.
    if (ms.copy_stream == nullptr) {
      const int prc = prime_copy_stream(device, ms);  // (process_host_many has done this for every large unit, one after the other)
      if (prc != SPEEXHIP_ERR_SUCCESS) return prc;
    }
    while (ms.events.size() < launches.size()) {
      hipEvent_t e = nullptr;
      HIP_TRY(pool::event_get(device, &e));
      ms.events.push_back(e);
    }
    DrainOnExit drain_copy(&ms.copy_stream);
    std::mutex mu;
    std::condition_variable cv;
    size_t ready = 0;       // launches whose inputs are enqueued with their event recorded
    bool copy_failed = false;
    int worker_rc = SPEEXHIP_ERR_SUCCESS;
    std::string worker_err;
    auto helper = [&] {
      DeviceScope scope(device);
      try {
      for (size_t k = 0; k < launches.size() && worker_rc == SPEEXHIP_ERR_SUCCESS; k++) {
        {
          std::unique_lock<std::mutex> l(mu);
          cv.wait(l, [&] { return ready > k || copy_failed; });
          if (copy_failed) return;
        }
        auto fail = [&](hipError_t e, const char *what) {
          if (e == hipSuccess) return false;
          worker_err = std::string("HIP device error: ") + what + ": " + hipGetErrorString(e);
          worker_rc = SPEEXHIP_ERR_DEVICE;
          return true;
        };
        if (fail(hipStreamWaitEvent(ms.stream, ms.events[k], 0), "hipStreamWaitEvent")) return;
        const int lrc = launch(launches[k], ms.stream);
        if (lrc != SPEEXHIP_ERR_SUCCESS) {
          worker_rc = lrc;
          worker_err = g_last_error;
          return;
        }
        for (Item *it : launches[k])
          if (it->out_bytes != 0 &&
              fail(hipMemcpyAsync(it->out, ms.d_out + it->out_off, it->out_bytes, hipMemcpyDeviceToHost, ms.stream), "hipMemcpyAsync (results)"))
            return;
      }
      if (worker_rc == SPEEXHIP_ERR_SUCCESS) {
        const hipError_t e = hipStreamSynchronize(ms.stream);
        if (e != hipSuccess) {
          worker_err = std::string("HIP device error: hipStreamSynchronize: ") + hipGetErrorString(e);
          worker_rc = SPEEXHIP_ERR_DEVICE;
        }
      }
      } catch (...) {  // (a host allocation inside a launcher: no exception leaves a thread)
        worker_rc = SPEEXHIP_ERR_ALLOC_FAILED;
      }
    };
    // (the launching half runs on this (device, lane)'s persistent helper thread -- unit_workers.h; until round 6 a
    //  std::thread made and joined inside every such call.  No thread to be had: the call falls back to one thread,
    //  copies first, launches after -- the helper's loop then finds every event recorded already.)
    workers::Ticket helper_job = workers::submit(workers::key_of(device, lane, 1), helper);
    hipError_t copy_err = hipSuccess;
    for (size_t k = 0; k < launches.size() && copy_err == hipSuccess; k++) {
      for (Item *it : launches[k])
        if (it->in_bytes != 0 && copy_err == hipSuccess)
          copy_err = hipMemcpyAsync(ms.d_in + it->in_off, it->in, it->in_bytes, hipMemcpyHostToDevice, ms.copy_stream);
      if (copy_err == hipSuccess) copy_err = hipEventRecord(ms.events[k], ms.copy_stream);
      {
        std::lock_guard<std::mutex> l(mu);
        if (copy_err == hipSuccess)
          ready = k + 1;
        else
          copy_failed = true;
      }
      cv.notify_all();
    }
    if (helper_job != nullptr) {
      workers::wait(helper_job);
      if (workers::failed(helper_job)) worker_rc = SPEEXHIP_ERR_ALLOC_FAILED;
    } else {
      helper();
    }
    if (hip_failed(copy_err, "hipMemcpyAsync (inputs)")) return SPEEXHIP_ERR_DEVICE;
    if (worker_rc != SPEEXHIP_ERR_SUCCESS) {
      g_last_error = worker_err;
      return worker_rc;
    }
    drain.armed = false;
    drain_copy.armed = false;
    commit();
    return SPEEXHIP_ERR_SUCCESS;
  }

  for (const Item &it : items) {
    if (it.in_bytes == 0) continue;
    if (it.in_via == Via::Bounce || it.in_via == Via::Staged) std::memcpy(ms.h_in + it.in_off, it.in, it.in_bytes);
    if (it.in_via == Via::Copy)
      HIP_TRY(hipMemcpyAsync(ms.d_in + it.in_off, it.in, it.in_bytes, hipMemcpyHostToDevice, ms.stream));
  }
  // (not small: the gathered range holds the Staged buffers)
  if (!small && gathered_in != 0) HIP_TRY(hipMemcpyAsync(ms.d_in, ms.h_in, gathered_in, hipMemcpyHostToDevice, ms.stream));
  for (const std::vector<Item *> &g : launches) {
    rc = launch(g, ms.stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  commit();
  // results back
  if (!small && gathered_out != 0) HIP_TRY(hipMemcpyAsync(ms.h_out, ms.d_out, gathered_out, hipMemcpyDeviceToHost, ms.stream));
  for (const Item &it : items)
    if (it.out_via == Via::Copy)
      HIP_TRY(hipMemcpyAsync(it.out, ms.d_out + it.out_off, it.out_bytes, hipMemcpyDeviceToHost, ms.stream));
  if (wait.sync || !launches.empty()) {
    const int wrc = wait_call(ms.stream, wait, tail_word(ms.h_out, ms.h_out_cap), ++ms.seq);
    if (wrc != SPEEXHIP_ERR_SUCCESS) return wrc;
  }
  drain.armed = false;
  for (const Item &it : items)
    if (pinned_part(it.out_via, it.out_bytes) != 0) std::memcpy(it.out, ms.h_out + it.out_off, it.out_bytes);
  return SPEEXHIP_ERR_SUCCESS;
}

void many_counters(uint64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_many_counters[k].load(std::memory_order_relaxed);
}

// process_many_int / _float: the all-S16 / all-F32 case of many_run -- every entry the int16 call, or the float call, on
// its own bytes; the state's dither is neither read nor moved.
int Batch::process_host_many(uint32_t n, Batch *const *st, const void *const *in, uint32_t *in_len, void *const *out,
                             uint32_t *out_len, bool float_io, int *codes) {
  std::vector<ManyEntry> entries(n);
  for (uint32_t i = 0; i < n; i++) {
    ManyEntry &e = entries[i];
    e.b = st[i];
    e.in = in[i];
    e.out = out[i];
    e.in_fmt = e.out_fmt = float_io ? SPEEXHIP_FMT_F32 : SPEEXHIP_FMT_S16;
    e.kind = float_io ? ManyEntry::Float : ManyEntry::Int16;
    e.fusable = true;
    if (st[i] == nullptr || (out[i] == nullptr && out_len[i] != 0)) e.rc = SPEEXHIP_ERR_INVALID_ARG;
  }
  return many_run(n, entries.data(), in_len, out_len, codes);
}

int Batch::many_run(uint32_t n, const ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *codes) {
  std::vector<int> rcs(n, SPEEXHIP_ERR_SUCCESS);
  std::map<int, std::vector<uint32_t>> by_device;  // (ordered: two concurrent calls lock their devices in one order)
  std::vector<uint32_t> apart;                     // states that take the single call (in the caller's order)
  for (uint32_t i = 0; i < n; i++) {
    Batch *b = entries[i].b;
    if (entries[i].rc != SPEEXHIP_ERR_SUCCESS) {  // (an argument error: the state and the lengths stay as they are)
      rcs[i] = entries[i].rc;
      continue;
    }
    bool earlier = false;  // a state named twice: its second call must see the first one's end state
    for (uint32_t j = 0; j < i && !earlier; j++) earlier = entries[j].b == b;
    // (rare states -- channels moved apart by the per-channel calls, the zero fallback, batches of several streams --
    //  and the sides a launch group does not serve -- a matrix, planes of several channels -- keep their own call's rules)
    if (earlier || !entries[i].fusable || b->n_streams_ != 1 || !b->uniform(0) || b->zero_mode_)
      apart.push_back(i);
    else
      by_device[b->device_].push_back(i);
  }
  // the raw bytes entry i's sides would move at most: frames x channels x the side's sample size
  auto raw_in = [&](uint32_t i) {
    return static_cast<uint64_t>(in_len[i]) * entries[i].b->channels_ * sample_bytes(entries[i].in_fmt);
  };
  // Units of work: a device's states -- or, for a large call, two halves of them ("lanes"): one thread's pageable copies
  // do not fill a PCIe link (64 x 2^20 stereo frames on one GPU: 11.0 ms through one stage, 7.6 ms as two logical
  // devices of 32 states each, profiles/r05_host_many.txt), two stages side by side nearly do.
  struct Unit {
    int device, lane;
    std::vector<uint32_t> idx;
  };
  std::vector<Unit> units;
  static const int env_lanes = SPEEXHIP_DIAG_ENV("SPEEXHIP_MANY_LANES") ? std::atoi(SPEEXHIP_DIAG_ENV("SPEEXHIP_MANY_LANES")) : -1;  // A/B: 1 = never split
  for (auto &kv : by_device) {
    // What a lane is for: the runtime's PAGEABLE copies keep the thread that issues them busy, so the bytes that count are
    // the pageable ones of the busier direction.  Buffers in the library's pinned blocks do not count (a range check; read or
    // written in place -- or, chunks beside large pageable results, copied by a plain DMA that keeps no thread).
    // 32 x 2^20 stereo frames, one box (profiles/r06_pin_both_copy.txt, r06_pinned_in_leg.txt): pageable both ways one lane
    // 4.11, two 3.80 ms; pinned chunks + pageable results (146 MB out) 4.04 -> 3.83; both pinned 3.61 / 3.65 (nothing to
    // split).  (Until the stages had copy streams of their own -- prime_copy_stream -- the second case measured 4.02 / 4.54:
    // that was the copy engines' lottery, not the lanes.)
    uint64_t bytes_in = 0, bytes_out = 0;
    for (uint32_t i : kv.second) {
      const ManyEntry &e = entries[i];
      const uint64_t b = raw_in(i);
      if (e.in != nullptr && !pool::block_owns(e.in, b)) bytes_in += b;
      // (results: about den / num of the input's frames, capped by the caller's capacity)
      const uint64_t frames_out = std::min<uint64_t>(out_len[i], static_cast<uint64_t>(in_len[i]) * e.b->filter_.den / std::max<uint32_t>(e.b->filter_.num, 1) + 1);
      const uint64_t o = frames_out * e.b->channels_ * sample_bytes(e.out_fmt);
      if (e.out != nullptr && !pool::block_owns(e.out, o)) bytes_out += o;
    }
    const uint64_t bytes = std::max(bytes_in, bytes_out);
    // (from 128 MB: 32 x 2^20 stereo frames 4.11 -> 4.00 ms, 64 states 7.90 -> 7.14; at 67 MB nothing, 2.26 / 2.44)
    const bool split = env_lanes != 1 && kv.second.size() >= 8 && (env_lanes == 2 || bytes >= (static_cast<uint64_t>(128) << 20));  // (A/B: 2 = always)
    if (!split) {
      units.push_back(Unit{kv.first, 0, kv.second});
    } else {
      const size_t half = kv.second.size() / 2;
      units.push_back(Unit{kv.first, 0, std::vector<uint32_t>(kv.second.begin(), kv.second.begin() + half)});
      units.push_back(Unit{kv.first, 1, std::vector<uint32_t>(kv.second.begin() + half, kv.second.end())});
    }
  }
  // (the copy streams of the units that will take the pipelined path: made and primed one after the other, before any
  //  unit copies anything -- prime_copy_stream)
  for (const Unit &u : units) {
    uint64_t bytes = 0;
    for (uint32_t i : u.idx) bytes += raw_in(i);
    if (bytes >= (static_cast<uint64_t>(32) << 20)) {
      ManyStage &ms = many_stage(u.device, u.lane);
      std::lock_guard<std::mutex> lock(ms.mu);  // (the order many_on_device takes them in: the stage, then the priming)
      (void)prime_copy_stream(u.device, ms);   // (a failure shows again, with its code, in the unit's own call)
    }
  }
  std::vector<int> dev_rc(units.size(), SPEEXHIP_ERR_SUCCESS);
  std::vector<std::string> dev_err(units.size());
  auto run_device = [&](size_t slot) {
    const Unit &u = units[slot];
    try {
      dev_rc[slot] = many_on_device(u.device, u.lane, u.idx, entries, in_len, out_len, rcs.data());
    } catch (const std::bad_alloc &) {
      dev_rc[slot] = SPEEXHIP_ERR_ALLOC_FAILED;
    } catch (const std::exception &e) {  // (anything else: a code and its text, never std::terminate in a worker)
      g_last_error = std::string("internal error: ") + e.what();
      dev_rc[slot] = SPEEXHIP_ERR_DEVICE;
    } catch (...) {
      g_last_error = "internal error: unknown exception";
      dev_rc[slot] = SPEEXHIP_ERR_DEVICE;
    }
    if (dev_rc[slot] != SPEEXHIP_ERR_SUCCESS) {
      dev_err[slot] = g_last_error;  // (the text lives per thread)
      for (uint32_t i : u.idx) rcs[i] = dev_rc[slot];
    }
  };
  {
    // GPUs side by side: every further unit of the call runs on the persistent thread of its (device, lane) -- a GPU
    // is a PCIe link of its own, and the runtime's pageable copies keep the thread that issues them busy -- while the
    // calling thread runs the first one (unit_workers.h: one thread per (device, lane) for the life of the process;
    // until round 6 a std::thread per unit per CALL, 7-15 thread creations per step on an 8-GPU node).  A unit whose
    // job cannot be queued runs here, after the first.
    std::vector<workers::Ticket> tickets(units.size());
    for (size_t slot = 1; slot < units.size(); slot++)
      tickets[slot] = workers::submit(workers::key_of(units[slot].device, units[slot].lane, 0), [&run_device, slot] { run_device(slot); });
    if (!units.empty()) run_device(0);
    for (size_t slot = 1; slot < units.size(); slot++) {
      if (tickets[slot] != nullptr)
        workers::wait(tickets[slot]);
      else
        run_device(slot);
    }
    for (size_t k = 0; k < dev_rc.size(); k++)
      if (dev_rc[k] != SPEEXHIP_ERR_SUCCESS) {
        g_last_error = dev_err[k];
        break;
      }
  }
  for (uint32_t i : apart) {
    const ManyEntry &e = entries[i];
    rcs[i] = e.sides ? e.b->process_sides_host(e.in_side, &in_len[i], e.out_side, &out_len[i])
                     : e.b->process_host(e.in, &in_len[i], e.out, &out_len[i], e.kind != ManyEntry::Int16);
  }
  count_many(3, apart.size());
  int first = SPEEXHIP_ERR_SUCCESS;
  for (uint32_t i = 0; i < n; i++) {
    if (codes != nullptr) codes[i] = rcs[i];
    if (first == SPEEXHIP_ERR_SUCCESS && rcs[i] != SPEEXHIP_ERR_SUCCESS) first = rcs[i];
  }
  return first;
}

}  // namespace speexhip
