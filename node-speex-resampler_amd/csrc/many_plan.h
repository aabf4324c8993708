// many_plan.h -- every decision of the many-states host call, in integers (host only: no HIP, no Batch; tools/san_host.cpp
// checks it against its tables and over random shapes).  many.cpp describes the fused entries of one unit -- the states of
// one (device, lane) -- as ManyShapes and carries out what plan_many_unit answers; plan_many_lanes splits a device's
// states into units, many_primes_copy_stream says which units get their copy stream before anything is copied.
// A mixer call (mixer.cpp) plans its legs here as well: ManyShape::leg, ManyExtra, ManyKey::zero.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "host_transfer.h"

namespace speexhip {

const size_t kManyLaunchStates = 32;                               // states per launch (device_types.h, kMaxPackedStreams)
const size_t kManyPipelineBytes = static_cast<size_t>(32) << 20;   // from here a call of large buffers runs in pieces ...
const size_t kManyPieceBytes = static_cast<size_t>(16) << 20;      // ... of about this much input per launch
const uint64_t kManyLaneBytes = static_cast<uint64_t>(128) << 20;  // from here a device's states run as two lanes

inline size_t align128(size_t v) { return (v + 127) & ~static_cast<size_t>(127); }

// What the states of one launch share, in the order the launches are queued: the filter's tables (their address), the
// mode, the window format (a float call has put samples into the history that an int16 window cannot hold) and the sample
// type of the launch -- and, among a mixer's legs, whether the state is in the zero fallback (its launch writes zeros; a
// fused entry of the many-states calls never is: such a state takes its own call).
struct ManyKey {
  uintptr_t tables = 0;
  int mode = 0;
  bool float_window = false, float_io = false;
  bool zero = false;
  bool operator<(const ManyKey &o) const {
    return std::tie(tables, mode, float_window, float_io, zero) < std::tie(o.tables, o.mode, o.float_window, o.float_io, o.zero);
  }
};

// One fused entry as the decision sees it.
struct ManyShape {
  size_t in_bytes = 0, out_bytes = 0;  // the raw bytes of either side, in the side's own format (an absent input: 0)
  bool in_present = false;
  bool in_pinned = false, out_pinned = false;  // the caller's lookup decides (Batch::pinned_sides: the overlap rule)
  bool work = false;                   // something runs for the entry; else it is routed and laid out but not launched
  bool pass_in = false, pass_out = false;      // the side's storage goes through a float image ...
  size_t image_in = 0, image_out = 0;          // ... of this many bytes
  ManyKey key;
  // a leg of a mixer call (mixer.cpp): its result STAYS its float image on the device, a range of its own among the output
  // images -- no storage, no output pass, nothing that travels back (out_bytes 0, pass_out false)
  bool leg = false;
};
// What a mixer call moves beside its legs' inputs: the table of the legs at the head of the range that travels in, the
// buses (as their side stores them) at the head of the range that travels out.  They go the gathered way, whatever their
// size: one copy each way, or the pinned stage of a small call.
struct ManyExtra {
  size_t in_bytes = 0, out_bytes = 0;
};
struct ManySwitches {     // the diagnostics build's: SPEEXHIP_PIN_IN_COPY (0 = read in place even then), _MANY_PIPELINE (0 = off)
  int pin_in_copy = 1, pipeline = -1;
};

struct ManyEntryPlan {
  Via in = Via::None, out = Via::None;
  bool demoted = false;             // a pinned input that is copied after all (below)
  size_t in_off = 0, out_off = 0;   // where the side lies in the stage (InPlace / None: nothing there)
  size_t img_in = 0, img_out = 0;   // where its float image lies
};
struct ManyLaunch {  // (a type of the project's own: the list's template code stays out of the library's dynamic symbols)
  std::vector<uint32_t> entries;
};
struct ManyUnitPlan {
  std::vector<ManyEntryPlan> e;
  size_t total_in = 0, total_out = 0;        // pageable bytes as laid out: each side on whole 64-byte lines
  size_t gathered_in = 0, gathered_out = 0;  // the leading range of the stage that travels as one copy
  size_t images_in = 0, images_out = 0;
  bool small = false, all_big = false, pipelined = false;
  Wait wait;
  size_t pin_in = 0, pin_out = 0, dev_in = 0, dev_out = 0, dev_img_in = 0, dev_img_out = 0;  // the six staging sizes (0: not needed)
  std::vector<ManyLaunch> launches;  // entry indices, in the order the launches are queued
};

inline ManyUnitPlan plan_many_unit(const ManyShape *shapes, size_t n, const ManySwitches &sw, const ManyExtra &extra = ManyExtra()) {
  ManyUnitPlan p;
  p.e.resize(n);
  p.total_in = align64(extra.in_bytes);
  p.total_out = align64(extra.out_bytes);
  for (size_t k = 0; k < n; k++) {
    const ManyShape &s = shapes[k];
    ManyEntryPlan &e = p.e[k];
    // (a pinned input whose result goes to a LARGE pageable buffer is copied like any other -- from pinned memory the copy
    //  is a plain DMA -- so that the call can take the pipelined path, inputs arriving while results leave: read in place,
    //  all the reads come first and all the pageable copies out after them, 32 x 2^20 stereo frames 5.4 ms against 4.0,
    //  profiles/r06_bench_driver_form_v2.json)
    e.demoted = s.in_pinned && !s.out_pinned && s.out_bytes >= kDirectCopyBytes && sw.pin_in_copy != 0;
    e.img_in = p.images_in;
    e.img_out = p.images_out;
    if (s.pass_in) p.images_in += align128(s.image_in);
    if (s.pass_out || s.leg) p.images_out += align128(s.image_out);
    p.total_in += align64(s.in_pinned && !e.demoted ? 0 : s.in_bytes);
    p.total_out += align64(s.out_pinned ? 0 : s.out_bytes);
  }
  // Every side by the rule of host_transfer.h, the call's pageable totals deciding whether it is small.  Small calls (a
  // server's 10-20 ms frames, a Transform's 64 KiB chunks) run on pinned memory alone; larger ones gather their Staged
  // buffers in the pinned buffer, which travels as ONE copy each way.
  p.small = small_call(p.total_in, p.total_out);
  p.all_big = true;  // every working state Copy both ways: the pipelined path
  for (size_t k = 0; k < n; k++) {
    const ManyShape &s = shapes[k];
    ManyEntryPlan &e = p.e[k];
    e.in = route_side(s.in_bytes, s.in_present, s.in_pinned && !e.demoted, p.small);
    e.out = s.leg ? Via::None : route_side(s.out_bytes, true, s.out_pinned, p.small);
    p.wait.add(e.in, s.in_bytes);
    p.wait.add(e.out, s.out_bytes);
    if (s.work && (e.in != Via::Copy || e.out != Via::Copy)) p.all_big = false;
  }
  // layout: the gathered buffers first (one contiguous range = one copy), then the Copy ones.  A small call's stage is
  // the pinned pair, a larger one's the device pair.
  auto through_stage = [&p](Via v, size_t bytes) { return align64(p.small ? pinned_part(v, bytes) : device_part(v, bytes)); };
  // (a mixer call's table and buses lie at the head of the gathered ranges)
  if (extra.in_bytes != 0) p.wait.add(p.small ? Via::Bounce : Via::Staged, extra.in_bytes);
  if (extra.out_bytes != 0) p.wait.add(p.small ? Via::Bounce : Via::Staged, extra.out_bytes);
  size_t off_in = p.gathered_in = align64(extra.in_bytes), off_out = p.gathered_out = align64(extra.out_bytes);
  for (int pass = 0; pass < 2; pass++)
    for (size_t k = 0; k < n; k++) {
      ManyEntryPlan &e = p.e[k];
      if ((e.in == Via::Copy) == (pass == 1)) {
        e.in_off = off_in;
        off_in += through_stage(e.in, shapes[k].in_bytes);
        if (pass == 0) p.gathered_in = off_in;
      }
      if ((e.out == Via::Copy) == (pass == 1)) {
        e.out_off = off_out;
        off_out += through_stage(e.out, shapes[k].out_bytes);
        if (pass == 0) p.gathered_out = off_out;
      }
    }
  p.pin_in = p.gathered_in;
  p.pin_out = p.gathered_out + 128;  // (the completion word of a polled wait lies at the buffer's tail)
  p.dev_in = p.small ? 0 : p.total_in;
  p.dev_out = p.small ? 0 : p.total_out;
  // (a line of slack behind the last image, as the single call's pitched images have behind every stream)
  p.dev_img_in = p.images_in != 0 ? p.images_in + 256 : 0;
  p.dev_img_out = p.images_out != 0 ? p.images_out + 256 : 0;

  // Large calls in pieces: a launch then carries about 16 MB of input, so that the transfer of the next piece and the
  // results of the previous one have something to overlap with.
  // (this 32 MiB test: the pageable total as laid out, and only when every working entry is Copy both ways)
  const bool in_pieces = p.all_big && sw.pipeline != 0 && p.total_in >= kManyPipelineBytes;
  // launches: the working entries that share a key go together, at most 32 per launch
  std::map<ManyKey, std::vector<uint32_t>> groups;
  for (size_t k = 0; k < n; k++)
    if (shapes[k].work) groups[shapes[k].key].push_back(static_cast<uint32_t>(k));  // (else: the state stays where it is)
  for (auto &kv : groups) {
    const std::vector<uint32_t> &g = kv.second;
    size_t per = kManyLaunchStates;
    if (in_pieces) {
      size_t bytes = 0;
      for (uint32_t k : g) bytes += shapes[k].in_bytes;
      const size_t pieces = std::max<size_t>(1, bytes / kManyPieceBytes);
      per = std::min(kManyLaunchStates, std::max<size_t>(1, (g.size() + pieces - 1) / pieces));
    }
    for (size_t g0 = 0; g0 < g.size(); g0 += per)
      p.launches.push_back(ManyLaunch{std::vector<uint32_t>(g.begin() + g0, g.begin() + std::min(g.size(), g0 + per))});
  }
  p.pipelined = in_pieces && p.launches.size() >= 2;  // (one launch: nothing to overlap with)
  return p;
}

// Units of work: a device's states -- or, for a large call, two halves of them ("lanes"): one thread's pageable copies
// do not fill a PCIe link (64 x 2^20 stereo frames on one GPU: 11.0 ms through one stage, 7.6 ms as two logical devices of
// 32 states each, profiles/r05_host_many.txt), two stages side by side nearly do.  What a lane is for: the runtime's
// PAGEABLE copies keep the thread that issues them busy, so the bytes that count are the pageable ones of the busier
// direction; the caller leaves out the buffers in the library's pinned blocks (read or written in place -- or, chunks
// beside large pageable results, copied by a plain DMA that keeps no thread).
// 32 x 2^20 stereo frames, one box (profiles/r06_pin_both_copy.txt, r06_pinned_in_leg.txt): pageable both ways one lane
// 4.11, two 3.80 ms; pinned chunks + pageable results (146 MB out) 4.04 -> 3.83; both pinned 3.61 / 3.65 (nothing to
// split).  (Until the stages had copy streams of their own the second case measured 4.02 / 4.54: that was the copy
// engines' lottery, not the lanes.)
// Returns the states of lane 0: all n, or the first half.  lanes_switch: SPEEXHIP_MANY_LANES (1 = never split, 2 = always).
inline size_t plan_many_lanes(size_t n, uint64_t pageable_in, uint64_t pageable_out, int lanes_switch) {
  const uint64_t bytes = std::max(pageable_in, pageable_out);
  // (from 128 MB: 32 x 2^20 stereo frames 4.11 -> 4.00 ms, 64 states 7.90 -> 7.14; at 67 MB nothing, 2.26 / 2.44)
  const bool split = lanes_switch != 1 && n >= 8 && (lanes_switch == 2 || bytes >= kManyLaneBytes);
  return split ? n / 2 : n;
}
// The copy stream of a unit that may take the pipelined path is made and primed before any unit copies anything.
// (this 32 MiB test: the raw input bytes of all the unit's entries, pinned, absent and small ones included)
inline bool many_primes_copy_stream(uint64_t raw_in_bytes) { return raw_in_bytes >= kManyPipelineBytes; }

}  // namespace speexhip
