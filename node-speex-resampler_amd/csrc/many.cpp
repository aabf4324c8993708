// many.cpp -- the host-buffer calls of many single-stream states at once (engine.h: process_host_many,
// process_host_many_sides through many_run): product code.  Every decision is many_plan.h's (host only, in integers);
// here are the mechanics: the stages, the copies, the launches, the two-thread hand-over of a pipelined call.
#include "engine.h"

#include "devices.h"
#include "engine_detail.h"
#include "many_plan.h"
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
  // the float images of the entries whose storage is not the image (SidesRoute::Images): device scratch either side of the
  // FIR launch, one range per entry
  char *d_img_in = nullptr, *d_img_out = nullptr;
  size_t d_img_in_cap = 0, d_img_out_cap = 0;
  uint32_t seq = 0;
};
// speexhip_debug_many_counters: FIR launches, input passes, output passes, entries that took their own call
std::atomic<uint64_t> g_many_counters[4];
inline void count_many(int which, uint64_t by = 1) { g_many_counters[which].fetch_add(by, std::memory_order_relaxed); }
// speexhip_debug_mixer_counters: FIR launches, input passes, bus-sum launches, output passes, transfers in, transfers out
std::atomic<uint64_t> g_mixer_counters[6];
inline void count_mixer(int which, uint64_t by = 1) { g_mixer_counters[which].fetch_add(by, std::memory_order_relaxed); }
// speexhip_debug_mixer_level_launches: the launches of the levels' kernels, apart from the six above
std::atomic<uint64_t> g_mixer_level_launches;
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

// What the two threads of a pipelined call (ManyUnit::run_pipelined) hand each other
struct HandOver {
  std::mutex mu;
  std::condition_variable cv;
  size_t ready = 0;  // launches whose inputs are enqueued with their event recorded
  bool copy_failed = false;
  int worker_rc = SPEEXHIP_ERR_SUCCESS;
  std::string worker_err;
};
static_assert(kManyLaunchStates == static_cast<size_t>(kMaxPackedStreams), "the planner's launches fill a descriptor pack");
// the states of a call that one stage serves (many_run)
struct Unit {
  int device, lane;
  std::vector<uint32_t> idx;
};
}  // namespace

// The fused states of ONE unit, idx = their positions in the caller's arrays: described as ManyShapes, planned by
// plan_many_unit, carried out on the unit's stage -- grow, then the plain or the pipelined run.
struct Batch::ManyUnit {
  struct Item {
    uint32_t i;
    Batch *b;
    const ManyEntry *e;  // (in / out: the caller's buffers, raw bytes of in_fmt / out_fmt)
    bool float_io;       // the FIR launch's sample type: int16 direct, or float (direct or images)
    CallPlan plan;
    const void *pin_in;  // round 6: the caller's own buffers where they are pinned memory (pinned_sides): the kernels
    void *pin_out;       // read / write them directly
  };
  int device, lane;
  ManyStage &ms;
  uint32_t *in_len, *out_len;
  int *rcs;
  std::vector<Item> items;
  std::vector<ManyShape> shapes;  // (items[k] as the decision sees it; plan.e[k] what was decided)
  ManyUnitPlan plan;
  char *src_base = nullptr, *dst_base = nullptr;  // the stage the kernels read / write: the pinned pair of a small call, else the device pair
  MixerCall *mixer = nullptr;  // a mixer call's unit (run_mixer): the entries are its legs, the buses stand behind them

  // a FIR launch / an input pass of the unit, in the counters of the call it belongs to
  void count(int which) const { mixer != nullptr ? count_mixer(which) : count_many(which); }
  static int run(const Unit &unit, const ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs);
  static std::vector<Unit> units_of(const std::map<int, std::vector<uint32_t>> &by_device, const ManyEntry *entries,
                                    const uint32_t *in_len, const uint32_t *out_len);
  // the raw bytes `frames` frames of an entry's side are: frames x channels x the side's sample size
  static uint64_t raw_bytes(const ManyEntry &e, uint64_t frames, bool in) {
    return frames * e.b->channels_ * sample_bytes(in ? e.in_fmt : e.out_fmt);
  }
  void describe(const std::vector<uint32_t> &idx, const ManyEntry *entries);
  int grow();
  int inputs_in();
  int run_plain();
  static int run_mixer(const Unit &unit, const ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs, MixerCall &mc);
  int measure_legs(size_t records_off);
  int sum_buses(size_t bus_stride, size_t plane_stride);
  int buses_out(size_t bus_stride, size_t plane_stride, size_t records_off);
  int run_pipelined();
  void launch_behind_copies(HandOver &h);
  int launch_group(const std::vector<uint32_t> &g, hipStream_t stream);
  void commit_item(Item &it, bool work);
  void commit_idle() {  // the states with nothing to run: counters of an empty call, position unchanged
    for (size_t k = 0; k < items.size(); k++)
      if (!shapes[k].work) commit_item(items[k], false);
  }
};

void Batch::ManyUnit::describe(const std::vector<uint32_t> &idx, const ManyEntry *entries) {
  items.resize(idx.size());
  shapes.resize(idx.size());
  for (size_t k = 0; k < idx.size(); k++) {
    Item &it = items[k];
    ManyShape &s = shapes[k];
    it.i = idx[k];
    it.e = &entries[it.i];
    it.b = it.e->b;
    const SidesRoute &r = it.e->route;
    it.float_io = r.kind != SidesRoute::Int16Call;
    it.plan = plan_call(it.b->filter_.num, it.b->filter_.den, in_len[it.i], out_len[it.i], it.b->P(0, 0), it.b->entry_rules(it.float_io));
    // the raw bytes of either side, in the side's own format: what every size decision goes by
    s.in_present = it.e->in != nullptr;
    s.in_bytes = s.in_present ? raw_bytes(*it.e, in_len[it.i], true) : 0;
    s.leg = it.e->leg;
    s.out_bytes = s.leg ? 0 : raw_bytes(*it.e, it.plan.produced, false);
    // (a present but empty input is not silence, no frame of it is read)
    s.pass_in = r.pass_in && s.in_present && in_len[it.i] != 0;
    s.pass_out = r.pass_out;
    s.image_in = static_cast<size_t>(in_len[it.i]) * it.b->channels_ * sizeof(float);
    s.image_out = static_cast<size_t>(it.plan.produced) * it.b->channels_ * sizeof(float);
    pinned_sides(it.e->in, s.in_bytes, s.leg ? nullptr : it.e->out, s.out_bytes, &it.pin_in, &it.pin_out);
    s.in_pinned = it.pin_in != nullptr;
    s.out_pinned = it.pin_out != nullptr;
    s.work = it.plan.produced != 0 || it.plan.magic_used + it.plan.consumed != 0;
    // (the window format as this call will leave it: the state itself is written in run(), once the stage has grown)
    s.key = ManyKey{reinterpret_cast<uintptr_t>(it.b->tables_.get()), it.b->mode_, it.b->float_seen_ || it.float_io, it.float_io,
                    it.b->zero_mode_};
  }
}

int Batch::ManyUnit::grow() {
  const struct {
    char **buf;
    size_t *cap, want;
    bool pinned;
  } stages[] = {{&ms.h_in, &ms.h_in_cap, plan.pin_in, true},        {&ms.h_out, &ms.h_out_cap, plan.pin_out, true},
                {&ms.d_in, &ms.d_in_cap, plan.dev_in, false},       {&ms.d_out, &ms.d_out_cap, plan.dev_out, false},
                {&ms.d_img_in, &ms.d_img_in_cap, plan.dev_img_in, false}, {&ms.d_img_out, &ms.d_img_out_cap, plan.dev_img_out, false}};
  for (const auto &g : stages) {
    const int rc = grow_stage(device, g.buf, g.cap, g.want, g.pinned);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  src_base = plan.small ? ms.h_in : ms.d_in;
  dst_base = plan.small ? ms.h_out : ms.d_out;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::ManyUnit::run(const Unit &unit, const ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs) {
  ManyStage &ms = many_stage(unit.device, unit.lane);
  std::lock_guard<std::mutex> lock(ms.mu);
  DeviceScope device_scope(unit.device);
  HIP_TRY(device_scope.error());
  if (ms.stream == nullptr) HIP_TRY(pool::stream_get(unit.device, &ms.stream));
  DrainOnExit drain(&ms.stream);
  ManyUnit u{unit.device, unit.lane, ms, in_len, out_len, rcs, {}, {}, {}};
  u.describe(unit.idx, entries);
  // (A/B, the diagnostics build: a pinned input beside a large pageable result read in place all the same; no pipeline)
  static const ManySwitches switches = {diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_PIN_IN_COPY"), 1),
                                        diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_MANY_PIPELINE"), -1)};
  u.plan = plan_many_unit(u.shapes.data(), u.shapes.size(), switches);
  int rc = u.grow();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  for (const Item &it : u.items) {
    if (it.float_io) it.b->float_seen_ = true;
    if (in_len[it.i] != 0 && out_len[it.i] != 0) it.b->started_[0] = 1;  // resample.c:886
  }
  rc = u.plan.pipelined ? u.run_pipelined() : u.run_plain();
  if (rc == SPEEXHIP_ERR_SUCCESS) drain.armed = false;  // (both runs have waited for everything they queued)
  return rc;
}

// counters and position of one state
void Batch::ManyUnit::commit_item(Item &it, bool work) {
  for (uint32_t c = 0; c < it.b->channels_; c++) it.b->P(0, c) = it.plan.end;
  if (!it.float_io && work) it.b->int16_call_done(&it.plan, 1);
  in_len[it.i] = it.plan.consumed;
  out_len[it.i] = it.plan.produced;
  // (a formatted call moves the state's dither position, meter totals and gain ramp by the frames produced, whatever the
  //  format: its output pass has judged these frames into the state's cell and left them at its g)
  it.b->sides_moved(it.e->route, &out_len[it.i], it.b->channels_);
  // (resample.c:1081: the zero fallback -- among fused entries only a mixer's leg -- reports the failure with every call)
  rcs[it.i] = it.b->zero_mode_ ? SPEEXHIP_ERR_ALLOC_FAILED : SPEEXHIP_ERR_SUCCESS;
}

// One launch of the entries g (one of plan.launches) on `stream`, between its passes.
int Batch::ManyUnit::launch_group(const std::vector<uint32_t> &g, hipStream_t stream) {
  const uint32_t cnt = static_cast<uint32_t>(g.size());
  const bool float_io = items[g[0]].float_io;  // (the group's: part of its key)
  DescPack pack;
  std::memset(&pack, 0, sizeof(pack));
  // the passes either side of the launch (kernels_convert_many.hip): one each for all the formats the group's entries
  // name, over the entries whose storage is not their image
  ConvertPack to_image, from_image;
  DitherPack dith;
  MeterPack cells;  // (beside the dither seeds: the cell of each entry whose state has the meter on)
  bool metered = false;
  std::memset(&cells, 0, sizeof(cells));
  // The gain of each entry whose state has it on: gains rides beside the dither seeds into the output pass; an entry
  // whose result no pass writes (F32 storage IS the FIR's image) is multiplied in place by one gain_image over the group.
  // Either way the entry stays in its group.
  GainPack gains, image_gains;
  ConvertPack in_place;
  bool gained = false;
  uint64_t most_in_place = 0;
  std::memset(&gains, 0, sizeof(gains));
  std::memset(&image_gains, 0, sizeof(image_gains));
  std::memset(&in_place, 0, sizeof(in_place));
  uint64_t most_to = 0, most_from = 0;
  std::memset(&to_image, 0, sizeof(to_image));
  std::memset(&from_image, 0, sizeof(from_image));
  std::memset(&dith, 0, sizeof(dith));
  uint32_t max_out = 0;
  for (uint32_t j = 0; j < cnt; j++) {
    Item &it = items[g[j]];
    const ManyShape &s = shapes[g[j]];
    const ManyEntryPlan &p = plan.e[g[j]];
    Batch *b = it.b;
    const int crc = b->chain_to(stream);  // (each state's calls stay ordered, whatever stream its last one ran on)
    if (crc != SPEEXHIP_ERR_SUCCESS) return crc;
    const void *storage_in = p.in == Via::None ? nullptr : p.in == Via::InPlace ? it.pin_in : src_base + p.in_off;
    void *storage_out = p.out == Via::InPlace ? it.pin_out : dst_base + p.out_off;
    // (a mixer's leg: the FIR's image is the result, in a range of its own; no storage stands behind it)
    b->fill_desc(pack.d[j], 0, 0, s.pass_in ? ms.d_img_in + p.img_in : storage_in,
                 s.pass_out || s.leg ? ms.d_img_out + p.img_out : storage_out, in_len[it.i], it.plan);
    if (s.pass_in) {
      ConvertStream &c = to_image.s[j];
      c.src = storage_in, c.dst = ms.d_img_in + p.img_in;
      c.n = static_cast<uint64_t>(in_len[it.i]) * b->channels_;
      c.step = 1;
      c.reserved = convert_many_tag(it.e->in_fmt, SPEEXHIP_DITHER_NONE);
      most_to = std::max(most_to, c.n);
    }
    if (s.pass_out && it.plan.produced != 0) {
      ConvertStream &c = from_image.s[j];
      c.src = ms.d_img_out + p.img_out, c.dst = storage_out;
      c.n = static_cast<uint64_t>(it.plan.produced) * b->channels_;
      c.step = 1;
      const bool dithered = b->dither_on() && dithered_fmt(it.e->out_fmt);
      c.reserved = convert_many_tag(it.e->out_fmt, dithered ? b->dither_kind_ : SPEEXHIP_DITHER_NONE);
      if (dithered) dith.s[j] = b->dither_pack(0, 1, b->channels_).s[0];
      if (it.e->route.counts_meter) cells.cell[j] = b->d_meter_, metered = true;
      if (it.e->route.moves_gain) gains.s[j] = b->gain_pack(0, 1, b->channels_).s[0], gained = true;
      most_from = std::max(most_from, c.n);
    } else if (it.e->route.finish == SidesRoute::GainImage && it.plan.produced != 0) {
      ConvertStream &c = in_place.s[j];
      c.dst = storage_out;
      c.n = static_cast<uint64_t>(it.plan.produced) * b->channels_;
      c.step = 1;
      image_gains.s[j] = b->gain_pack(0, 1, b->channels_).s[0];
      most_in_place = std::max(most_in_place, c.n);
    }
    max_out = std::max(max_out, it.plan.produced);
  }
  if (most_to != 0) {
    if (hip_failed(launch_convert_many(false, to_image, dith, cnt, most_to, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
    count(1);
  }
  const int lrc = items[g[0]].b->launch_chunk(pack.d, pack, cnt, max_out, float_io, stream);
  if (lrc != SPEEXHIP_ERR_SUCCESS) return lrc;
  count(0);
  if (most_from != 0) {
    if (hip_failed(launch_convert_many(true, from_image, dith, cnt, most_from, stream, metered ? &cells : nullptr, gained ? &gains : nullptr),
                   "kernel launch"))
      return SPEEXHIP_ERR_DEVICE;
    count_many(2);
  }
  if (most_in_place != 0) {
    // (a metered F32 result is no entry of a group -- process_host_many_sides -- so nothing is judged here)
    // (the route's finish_scale is 1 for every fused entry)
    if (hip_failed(launch_gain_image(in_place, image_gains, nullptr, 1.0f, cnt, most_in_place, stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
    count_many(2);
  }
  // A state moves as ONE step, the moment its launch is queued: the history ping-pong, the position and the counters
  // together.  (Until round 6 the flip happened here and the positions behind the last launch of the call: a later
  // group's failure left the earlier groups' states with a flipped history and their OLD position -- silently corrupt
  // for every later call, ADVICE r5.  Now a failure further on costs such a state this call's audio -- its code says
  // so -- and nothing else; states whose launch was never queued have not moved at all.)
  for (uint32_t k : g) {
    items[k].b->hist_cur_ ^= 1;
    commit_item(items[k], true);
  }
  return SPEEXHIP_ERR_SUCCESS;
}

// One thread, one stream: the inputs in, the launches, the results back, the wait the plan chose.
int Batch::ManyUnit::inputs_in() {
  for (size_t k = 0; k < items.size(); k++) {
    const ManyShape &s = shapes[k];
    const ManyEntryPlan &p = plan.e[k];
    if (pinned_part(p.in, s.in_bytes) != 0) std::memcpy(ms.h_in + p.in_off, items[k].e->in, s.in_bytes);
    if (p.in == Via::Copy && s.in_bytes != 0)
      HIP_TRY(hipMemcpyAsync(ms.d_in + p.in_off, items[k].e->in, s.in_bytes, hipMemcpyHostToDevice, ms.stream));
  }
  // (not small: the gathered range holds the Staged buffers)
  if (!plan.small && plan.gathered_in != 0) HIP_TRY(hipMemcpyAsync(ms.d_in, ms.h_in, plan.gathered_in, hipMemcpyHostToDevice, ms.stream));
  return SPEEXHIP_ERR_SUCCESS;
}
int Batch::ManyUnit::run_plain() {
  const int irc = inputs_in();
  if (irc != SPEEXHIP_ERR_SUCCESS) return irc;
  for (const ManyLaunch &l : plan.launches) {
    const int rc = launch_group(l.entries, ms.stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  commit_idle();
  // results back
  if (!plan.small && plan.gathered_out != 0) HIP_TRY(hipMemcpyAsync(ms.h_out, ms.d_out, plan.gathered_out, hipMemcpyDeviceToHost, ms.stream));
  for (size_t k = 0; k < items.size(); k++)
    if (plan.e[k].out == Via::Copy)
      HIP_TRY(hipMemcpyAsync(items[k].e->out, ms.d_out + plan.e[k].out_off, shapes[k].out_bytes, hipMemcpyDeviceToHost, ms.stream));
  if (plan.wait.sync || !plan.launches.empty()) {
    const int wrc = wait_call(ms.stream, plan.wait, tail_word(ms.h_out, ms.h_out_cap), ++ms.seq);
    if (wrc != SPEEXHIP_ERR_SUCCESS) return wrc;
  }
  for (size_t k = 0; k < items.size(); k++)
    if (pinned_part(plan.e[k].out, shapes[k].out_bytes) != 0) std::memcpy(items[k].e->out, ms.h_out + plan.e[k].out_off, shapes[k].out_bytes);
  return SPEEXHIP_ERR_SUCCESS;
}

// Large calls, pipelined (round 5).  PCIe is full duplex, but the runtime's pageable copies keep the thread that
// issues them busy until they are staged, so one thread alone moves inputs, computes, and moves results strictly
// one after the other: 32 streams x 2^20 stereo frames 5.8 ms, of which 0.2 are the kernel.  Here the calling
// thread copies the inputs of launch after launch on the stage's copy stream (an event behind each launch's
// inputs), while a second thread waits for the events, runs the launches on the stage's stream and copies each
// launch's results out behind it (launch_behind_copies): results leave while the next inputs arrive.
int Batch::ManyUnit::run_pipelined() {
  const std::vector<ManyLaunch> &launches = plan.launches;
  if (ms.copy_stream == nullptr) {
    const int prc = prime_copy_stream(device, ms);  // (many_run has done this for every large unit, one after the other)
    if (prc != SPEEXHIP_ERR_SUCCESS) return prc;
  }
  while (ms.events.size() < launches.size()) {
    hipEvent_t e = nullptr;
    HIP_TRY(pool::event_get(device, &e));
    ms.events.push_back(e);
  }
  DrainOnExit drain_copy(&ms.copy_stream);
  HandOver h;
  // (the launching half runs on this (device, lane)'s persistent helper thread -- unit_workers.h; until round 6 a
  //  std::thread made and joined inside every such call.  No thread to be had: the call falls back to one thread,
  //  copies first, launches after -- the helper's loop then finds every event recorded already.)
  workers::Ticket helper_job = workers::submit(workers::key_of(device, lane, 1), [this, &h] { launch_behind_copies(h); });
  hipError_t copy_err = hipSuccess;
  for (size_t k = 0; k < launches.size() && copy_err == hipSuccess; k++) {
    for (uint32_t j : launches[k].entries)
      if (shapes[j].in_bytes != 0 && copy_err == hipSuccess)
        copy_err = hipMemcpyAsync(ms.d_in + plan.e[j].in_off, items[j].e->in, shapes[j].in_bytes, hipMemcpyHostToDevice, ms.copy_stream);
    if (copy_err == hipSuccess) copy_err = hipEventRecord(ms.events[k], ms.copy_stream);
    {
      std::lock_guard<std::mutex> l(h.mu);
      if (copy_err == hipSuccess)
        h.ready = k + 1;
      else
        h.copy_failed = true;
    }
    h.cv.notify_all();
  }
  if (helper_job != nullptr) {
    workers::wait(helper_job);
    if (workers::failed(helper_job)) h.worker_rc = SPEEXHIP_ERR_ALLOC_FAILED;
  } else {
    launch_behind_copies(h);
  }
  if (hip_failed(copy_err, "hipMemcpyAsync (inputs)")) return SPEEXHIP_ERR_DEVICE;
  if (h.worker_rc != SPEEXHIP_ERR_SUCCESS) {
    g_last_error = h.worker_err;
    return h.worker_rc;
  }
  drain_copy.armed = false;
  commit_idle();
  return SPEEXHIP_ERR_SUCCESS;
}

// The second thread of a pipelined call: launch k behind the event of its inputs, its results out behind it, on the
// stage's stream; then the wait for all of it.  Codes and the error text travel back through `h`.
void Batch::ManyUnit::launch_behind_copies(HandOver &h) {
  DeviceScope scope(device);
  auto fail = [&h](hipError_t e, const char *what) {
    if (e == hipSuccess) return false;
    h.worker_err = std::string("HIP device error: ") + what + ": " + hipGetErrorString(e);
    h.worker_rc = SPEEXHIP_ERR_DEVICE;
    return true;
  };
  try {
    for (size_t k = 0; k < plan.launches.size() && h.worker_rc == SPEEXHIP_ERR_SUCCESS; k++) {
      {
        std::unique_lock<std::mutex> l(h.mu);
        h.cv.wait(l, [&] { return h.ready > k || h.copy_failed; });
        if (h.copy_failed) return;
      }
      if (fail(hipStreamWaitEvent(ms.stream, ms.events[k], 0), "hipStreamWaitEvent")) return;
      const int lrc = launch_group(plan.launches[k].entries, ms.stream);
      if (lrc != SPEEXHIP_ERR_SUCCESS) {
        h.worker_rc = lrc;
        h.worker_err = g_last_error;
        return;
      }
      for (uint32_t j : plan.launches[k].entries)
        if (shapes[j].out_bytes != 0 &&
            fail(hipMemcpyAsync(items[j].e->out, ms.d_out + plan.e[j].out_off, shapes[j].out_bytes, hipMemcpyDeviceToHost, ms.stream),
                 "hipMemcpyAsync (results)"))
          return;
    }
    if (h.worker_rc == SPEEXHIP_ERR_SUCCESS) (void)fail(hipStreamSynchronize(ms.stream), "hipStreamSynchronize");
  } catch (...) {  // (a host allocation inside a launcher: no exception leaves a thread)
    h.worker_rc = SPEEXHIP_ERR_ALLOC_FAILED;
  }
}

void many_counters(uint64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_many_counters[k].load(std::memory_order_relaxed);
}
void mixer_counters(uint64_t out[6]) {
  for (int k = 0; k < 6; k++) out[k] = g_mixer_counters[k].load(std::memory_order_relaxed);
}
uint64_t mixer_level_launches() { return g_mixer_level_launches.load(std::memory_order_relaxed); }

// ---- the unit of a mixer call (engine.h, many_mixer; include/speexhip_resampler.h, "Mixer") -------------------------------
// The legs are staged, grouped and launched as run_plain does it -- the table of ALL the call's slots at the head of the
// range that travels in -- and stay float images on the device; behind the last launch bus_sum_legs (kernels_bus_legs.hip)
// sums every slot into the buses, their output stage (bus_out.h) encodes them into the head of the range that travels out, and
// that range goes back as one copy (a small call: the kernels wrote the pinned stage) and from there into the caller's
// bus buffers.  Never pipelined, never two lanes: a tick is small, and the buses need every leg.
// With the mixer's levels on ("Mixer levels") leg_levels (kernels_levels.hip) measures every slot's image behind the last
// FIR launch and before the sum, which it does not wait for; its records lie behind the buses in the range that travels
// out, on a 64-byte boundary, and leave with them.
int Batch::ManyUnit::run_mixer(const Unit &unit, const ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs, MixerCall &mc) {
  ManyStage &ms = many_stage(unit.device, unit.lane);
  std::lock_guard<std::mutex> lock(ms.mu);
  DeviceScope device_scope(unit.device);
  HIP_TRY(device_scope.error());
  if (ms.stream == nullptr) HIP_TRY(pool::stream_get(unit.device, &ms.stream));
  DrainOnExit drain(&ms.stream);
  ManyUnit u{unit.device, unit.lane, ms, in_len, out_len, rcs, {}, {}, {}};
  u.mixer = &mc;
  u.describe(unit.idx, entries);
  mc.bus_frames = 0;
  for (const Item &it : u.items) mc.bus_frames = std::max(mc.bus_frames, it.plan.produced);
  // The buses in the stage, as their side stores them: bus j begins j * bus_stride samples behind bus 0 (whole 64-sample
  // runs, so that every bus begins on a line whatever the format), a planar side's plane c another c * plane_stride.
  const bool planar = mc.out.layout == SPEEXHIP_LAYOUT_PLANAR;
  const size_t plane_stride = planar ? (static_cast<size_t>(mc.bus_frames) + 15) & ~static_cast<size_t>(15) : 0;
  const size_t bus_samples = planar ? plane_stride * mc.out.channels : static_cast<size_t>(mc.bus_frames) * mc.out.channels;
  const size_t bus_stride = (bus_samples + 63) & ~static_cast<size_t>(63);
  ManyExtra extra;
  extra.in_bytes = sizeof(BusLeg) * mc.n_legs;
  extra.out_bytes = bus_stride * mc.buses->n_buses() * sample_bytes(mc.out.fmt);
  // (bus_stride is whole 64-sample runs: the buses end on a 64-byte boundary, where the records begin)
  const size_t records_off = extra.out_bytes;
  if (mc.levels != nullptr) extra.out_bytes += align64(sizeof(SpeexHipLevel) * mc.n_legs);
  const ManySwitches switches = {1, 0};  // (no pipeline)
  u.plan = plan_many_unit(u.shapes.data(), u.shapes.size(), switches, extra);
  int rc = u.grow();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (mc.bus_route.pass_out) {  // (the mixer's last call has been waited for: nothing reads the old image)
    rc = mc.buses->grow_image(bus_stride * mc.buses->n_buses() * sizeof(float));
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  // The table: one record per SLOT, in slot order.  A slot without a leg that runs -- empty, refused -- stays zeros: no
  // frames, +0.0f throughout.  A leg's gain is read here, before its launch commits and moves it.
  BusLeg *table = reinterpret_cast<BusLeg *>(ms.h_in);
  std::memset(table, 0, sizeof(BusLeg) * mc.n_legs);
  for (size_t k = 0; k < u.items.size(); k++) {
    const Item &it = u.items[k];
    BusLeg &leg = table[it.i];
    leg.src = reinterpret_cast<const float *>(ms.d_img_out + u.plan.e[k].img_out);
    leg.frames = it.plan.produced;
    if (it.e->route.moves_gain) leg.gain = it.b->gain_pack(0, 1, mc.out.channels).s[0];
  }
  if (mc.levels != nullptr && mc.bus_frames != 0) {
    // (the mixer's last call has been waited for: nothing reads the old block)
    const uint64_t spans = level_spans(table, mc.n_legs, mc.out.channels);
    if (spans > 1) {
      rc = grow_stage(unit.device, mc.level_parts, mc.level_parts_cap, sizeof(SpeexHipLevel) * mc.n_legs * spans, false);
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    }
  }
  for (const Item &it : u.items) {
    it.b->float_seen_ = true;
    if (in_len[it.i] != 0 && out_len[it.i] != 0) it.b->started_[0] = 1;  // resample.c:886
  }
  rc = u.inputs_in();
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // (the stage is the call's one transfer in -- copied, or read in place by the kernels of a small call; a payload large
  //  enough to travel on its own counts beside it)
  count_mixer(4);
  for (const ManyEntryPlan &e : u.plan.e)
    if (e.in == Via::Copy) count_mixer(4);
  for (const ManyLaunch &l : u.plan.launches) {
    rc = u.launch_group(l.entries, ms.stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  u.commit_idle();
  rc = u.measure_legs(records_off);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  rc = u.sum_buses(bus_stride, plane_stride);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  rc = u.buses_out(bus_stride, plane_stride, records_off);
  if (rc == SPEEXHIP_ERR_SUCCESS) drain.armed = false;
  return rc;
}

// leg_levels over the table, into the records behind the buses in the stage that travels out (levels off: nothing)
int Batch::ManyUnit::measure_legs(size_t records_off) {
  MixerCall &mc = *mixer;
  if (mc.levels == nullptr || mc.bus_frames == 0) return SPEEXHIP_ERR_SUCCESS;
  uint32_t launches = 0;
  const hipError_t e = launch_leg_levels(reinterpret_cast<const BusLeg *>(src_base), reinterpret_cast<const BusLeg *>(ms.h_in), mc.n_legs,
                                         mc.out.channels, mc.bus_frames, reinterpret_cast<SpeexHipLevel *>(dst_base + records_off),
                                         reinterpret_cast<SpeexHipLevel *>(*mc.level_parts), *mc.level_parts_cap, ms.stream, &launches);
  g_mixer_level_launches.fetch_add(launches, std::memory_order_relaxed);
  return hip_failed(e, "kernel launch") ? SPEEXHIP_ERR_DEVICE : SPEEXHIP_ERR_SUCCESS;
}

// bus_sum_legs over the table, then the output pass over the buses, into the stage that travels out
int Batch::ManyUnit::sum_buses(size_t bus_stride, size_t plane_stride) {
  MixerCall &mc = *mixer;
  if (mc.bus_frames == 0) return SPEEXHIP_ERR_SUCCESS;
  const BusLeg *table = reinterpret_cast<const BusLeg *>(ms.h_in);
  BusLegsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.legs = reinterpret_cast<const BusLeg *>(src_base);  // (the head of the range that travelled in)
  a.w = mc.d_w;
  a.w_pitch = mc.w_pitch;
  // (an interleaved F32 side IS the buses' image: the kernel writes the stage itself)
  a.dst = reinterpret_cast<float *>(mc.bus_route.pass_out ? mc.buses->image() : dst_base);
  a.dst_pitch = bus_stride;
  a.n_legs = mc.n_legs;
  a.n_buses = mc.buses->n_buses();
  a.channels = mc.out.channels;
  a.bus_frames = mc.bus_frames;
  if (hip_failed(launch_bus_sum_legs(a, table, ms.stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  count_mixer(2);
  CallSide stage = mc.out;
  stage.base = dst_base;
  stage.stride = bus_stride;
  stage.plane_stride = plane_stride;
  uint32_t passes = 0;
  const int prc = mc.buses->encode(mc.bus_route, stage, mc.buses->image(), bus_stride, mc.bus_frames, ms.stream, &passes);
  count_mixer(3, passes);
  return prc;
}

// the buses back: the one copy of a call that is not small (the legs' records behind the buses in it, when the levels
// are on), the wait, and the stage's buses into the caller's buffers, the records into the mixer's snapshot
int Batch::ManyUnit::buses_out(size_t bus_stride, size_t plane_stride, size_t records_off) {
  const MixerCall &mc = *mixer;
  const size_t es = sample_bytes(mc.out.fmt);
  const size_t records_bytes = mc.levels != nullptr ? sizeof(SpeexHipLevel) * mc.n_legs : 0;
  const size_t out_bytes = records_bytes != 0 ? records_off + records_bytes : bus_stride * mc.buses->n_buses() * es;
  if (mc.bus_frames != 0) {
    if (!plan.small) HIP_TRY(hipMemcpyAsync(ms.h_out, ms.d_out, out_bytes, hipMemcpyDeviceToHost, ms.stream));
    count_mixer(5);
  }
  if (plan.wait.sync || !plan.launches.empty()) {
    const int wrc = wait_call(ms.stream, plan.wait, tail_word(ms.h_out, ms.h_out_cap), ++ms.seq);
    if (wrc != SPEEXHIP_ERR_SUCCESS) return wrc;
  }
  const bool planar = mc.out.layout == SPEEXHIP_LAYOUT_PLANAR;
  for (uint32_t j = 0; j < mc.buses->n_buses() && mc.bus_frames != 0; j++) {
    char *to = static_cast<char *>(mc.out.base) + j * mc.out.stride * es;
    const char *from = ms.h_out + j * bus_stride * es;
    if (!planar) {
      std::memcpy(to, from, static_cast<size_t>(mc.bus_frames) * mc.out.channels * es);
    } else {
      for (uint32_t c = 0; c < mc.out.channels; c++)
        std::memcpy(to + c * mc.out.plane_stride * es, from + c * plane_stride * es, static_cast<size_t>(mc.bus_frames) * es);
    }
  }
  if (records_bytes != 0 && mc.bus_frames != 0) std::memcpy(mc.levels, ms.h_out + records_off, records_bytes);
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::many_mixer(MixerCall &mc, uint32_t n, ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs) {
  Unit unit{mc.device, 0, {}};
  for (uint32_t i = 0; i < n; i++)
    if (entries[i].leg && entries[i].rc == SPEEXHIP_ERR_SUCCESS && entries[i].b != nullptr) unit.idx.push_back(i);
  return ManyUnit::run_mixer(unit, entries, in_len, out_len, rcs, mc);
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
    if (st[i] == nullptr || (out[i] == nullptr && out_len[i] != 0)) e.rc = SPEEXHIP_ERR_INVALID_ARG;
  }
  return many_run(n, entries.data(), in_len, out_len, codes);
}

// Units of work: a device's states, or the two lanes plan_many_lanes splits them into -- by the pageable bytes of either
// direction: buffers in the library's pinned blocks do not count (a range check).
std::vector<Unit> Batch::ManyUnit::units_of(const std::map<int, std::vector<uint32_t>> &by_device, const ManyEntry *entries,
                                            const uint32_t *in_len, const uint32_t *out_len) {
  static const int env_lanes = diag_int(SPEEXHIP_DIAG_ENV("SPEEXHIP_MANY_LANES"), -1);  // A/B: 1 = never split, 2 = always
  std::vector<Unit> units;
  for (const auto &kv : by_device) {
    const std::vector<uint32_t> &idx = kv.second;
    uint64_t bytes_in = 0, bytes_out = 0;
    for (uint32_t i : idx) {
      const ManyEntry &e = entries[i];
      const uint64_t b = raw_bytes(e, in_len[i], true);
      if (e.in != nullptr && !pool::block_owns(e.in, b)) bytes_in += b;
      // (results: about den / num of the input's frames, capped by the caller's capacity)
      const uint64_t o = raw_bytes(e, std::min<uint64_t>(out_len[i], static_cast<uint64_t>(in_len[i]) * e.b->filter_.den / std::max<uint32_t>(e.b->filter_.num, 1) + 1), false);
      if (e.out != nullptr && !pool::block_owns(e.out, o)) bytes_out += o;
    }
    const size_t first = plan_many_lanes(idx.size(), bytes_in, bytes_out, env_lanes);
    units.push_back(Unit{kv.first, 0, std::vector<uint32_t>(idx.begin(), idx.begin() + first)});
    if (first != idx.size()) units.push_back(Unit{kv.first, 1, std::vector<uint32_t>(idx.begin() + first, idx.end())});
  }
  return units;
}

int Batch::many_run(uint32_t n, ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *codes) {
  std::vector<int> rcs(n, SPEEXHIP_ERR_SUCCESS);
  std::map<int, std::vector<uint32_t>> by_device;  // (ordered: two concurrent calls lock their devices in one order)
  std::vector<uint32_t> apart;                     // states that take the single call (in the caller's order)
  for (uint32_t i = 0; i < n; i++) {
    Batch *b = entries[i].b;
    if (entries[i].rc != SPEEXHIP_ERR_SUCCESS) {  // (an argument error: the state and the lengths stay as they are)
      rcs[i] = entries[i].rc;
      continue;
    }
    if (b->n_streams_ == 1 && !b->lengths_fit(&in_len[i], &out_len[i], 1)) {  // (engine.h: likewise)
      rcs[i] = SPEEXHIP_ERR_OVERFLOW;
      continue;
    }
    bool earlier = false;  // a state named twice: its second call must see the first one's end state
    for (uint32_t j = 0; j < i && !earlier; j++) earlier = entries[j].b == b;
    // (rare states -- channels moved apart by the per-channel calls, the zero fallback, batches of several streams --
    //  and the sides a launch group does not serve -- a matrix, planes of several channels -- keep their own call's rules.
    //  An entry of process_host_many is its format on both sides of a state with nothing on: never read, never moved.)
    ManyEntry &e = entries[i];
    SidesState st = b->sides_state(earlier);
    if (!e.sides) st.dither = st.meter = st.gain = false;
    const SideKind plain_in = {e.in_fmt, false, false, false}, plain_out = {e.out_fmt, false, false, false};
    e.route = route_sides_call(SidesForm::ManyEntry, e.sides ? side_kind(e.in_side) : plain_in, e.sides ? side_kind(e.out_side) : plain_out, st);
    if (!e.route.fusable)
      apart.push_back(i);
    else
      by_device[b->device_].push_back(i);
  }
  const std::vector<Unit> units = ManyUnit::units_of(by_device, entries, in_len, out_len);
  // (the copy streams of the units that will take the pipelined path: made and primed one after the other, before any
  //  unit copies anything -- prime_copy_stream)
  for (const Unit &u : units) {
    uint64_t bytes = 0;
    for (uint32_t i : u.idx) bytes += ManyUnit::raw_bytes(entries[i], in_len[i], true);
    if (many_primes_copy_stream(bytes)) {
      ManyStage &ms = many_stage(u.device, u.lane);
      std::lock_guard<std::mutex> lock(ms.mu);  // (the order ManyUnit::run takes them in: the stage, then the priming)
      (void)prime_copy_stream(u.device, ms);   // (a failure shows again, with its code, in the unit's own call)
    }
  }
  std::vector<int> dev_rc(units.size(), SPEEXHIP_ERR_SUCCESS);
  std::vector<std::string> dev_err(units.size());
  auto run_device = [&](size_t slot) {
    const Unit &u = units[slot];
    try {
      dev_rc[slot] = ManyUnit::run(u, entries, in_len, out_len, rcs.data());
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
                     : e.b->process_host(e.in, &in_len[i], e.out, &out_len[i], e.in_fmt != SPEEXHIP_FMT_S16);
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
