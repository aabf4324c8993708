// host_transfer.h -- how a host-buffer call moves its buffers and how it waits (host only; tools/san_host.cpp checks it).
// route_host_call() at the end is the whole decision for a single-state call: every entry point describes its two sides
// (HostCallShape) and gets the way of each, the wait and the sizes of the staging buffers (HostRoute); host_call.cpp
// carries it out.  The many-states call gathers many states into one range: its decision is plan_many_unit (many_plan.h,
// host only as well and checked by the same program), built from the parts below; many.cpp carries that out.
//
// Each side of a call (its input, its result) reaches the GPU one of four ways:
//   InPlace  the buffer is pinned memory (engine.cpp, pinned_view): the kernels read / write it through PCIe;
//   Bounce   the pinned bounce buffer: a memcpy into it, the kernels read / write it through PCIe, a memcpy out of it;
//   Copy     the runtime's own staged copy straight from / to the caller's memory, into / out of a device buffer;
//   Staged   a memcpy into the pinned buffer and ONE DMA (many-states call: the small buffers gathered into one range).
// A call that used the copy engines waits on its stream; one whose kernels did all the moving polls a completion word.
#pragma once
#include <cstddef>
#include <cstdint>

namespace speexhip {

// Large buffers go straight from / to the caller's pageable memory: the HIP runtime stages such
// copies itself and does it 2.2-2.5x faster than memcpy -> pinned -> DMA in one thread (2^20
// stereo frames: 0.46 -> 0.21 ms per call, 8 channels 1.57 -> 0.63 ms).  Small ones go through
// the pinned bounce buffers (below).
// What was tried in round 2 to get below this (2^20 stereo frames, 207 us per call; tools/ubench_copy.hip):
// PCIe is full duplex -- both copies at once from pinned memory take 103 us instead of 175 -- but
//   * H2D / kernel / D2H of 2-8 pieces on three streams chained by events: +30 us per piece (a
//     cross-stream wait costs ~14 us on this stack and nothing overlapped);
//   * pieces alternating on two independent in-order streams: 189 us at 2 pieces, more beyond (a
//     copy-engine <-> kernel hand-over costs ~10 us, and kernels of two streams never ran side by side);
//   * the caller's buffers pinned for the call (hipHostRegister, ~5 us) and read / written by the
//     kernels straight through PCIe, one launch: 166 us -- and, one run in three, a stretch of stale
//     zeros near the end of the output when buffers at recycled addresses were pinned again.  Not
//     shippable; removed.
// So the call stays three in-order steps on one stream.
const size_t kDirectCopyBytes = 256 * 1024;  // host buffers at least this big skip the pinned bounce buffer

// Small calls -- a Transform's 64 KiB chunks, a realtime caller's 10-20 ms frames -- are all latency:
// the kernels read the pinned bounce buffer and write the pinned result buffer straight through PCIe
// (pool-owned hipHostMalloc memory, coherent; one launch and one wait instead of copy / launch / copy
// / wait): 480-960 stereo frames 26.5 -> 22.7 us per call, 16384 frames 41.7 -> 30.1, 65536 frames
// 70.4 -> 53.7 (tools/small_call_latency.py).
// Where it stops paying (profiles/r03_zero_copy_sweep.txt, per call, pinned alone vs copies): 256 KB of input
// 49 vs 65 us (stereo), 49 vs 66 (mono), 46 vs 65 (8 channels); 512 KB 76 vs 95, 76 vs 95, 72 vs 90; 1 MB
// 167 vs 145, 169 vs 144, 132 vs 150: the single-threaded memcpy into and out of the bounce buffers grows at
// 0.18 us per KB against 0.10 for the runtime's own staged copies -- they cross near 740 KB.  (Until late in
// round 3 the limit was 256 KB, which sent a 65536-frame stereo chunk down the slower way.)
const size_t kZeroCopyBelow = 720 * 1024;    // ... and calls whose buffers are smaller than this run on pinned memory alone

enum class Via { None, InPlace, Bounce, Copy, Staged };
inline size_t align64(size_t v) { return (v + 63) & ~static_cast<size_t>(63); }

// A call runs on pinned memory alone when its pageable bytes -- pinned sides and an absent input count 0; the
// many-states call sums its states' -- stay below kZeroCopyBelow in both directions.
inline bool small_call(size_t pageable_in, size_t pageable_out) {
  return pageable_in < kZeroCopyBelow && pageable_out < kZeroCopyBelow;
}

// Round 6: buffers the caller keeps in pinned memory (speexhip_block_acquire, hipHostMalloc, hipHostRegister) are used
// where they lie: a pinned input is read by the kernel through PCIe, a pinned output written by it -- with both pinned
// the call is one launch and one wait, the two crossings side by side.  The other side, if pageable, keeps its own
// rule: small through the bounce buffer, large by the runtime's staged copy.
inline Via route_side(size_t bytes, bool present, bool pinned, bool small) {
  if (!present) return Via::None;
  if (pinned) return Via::InPlace;
  if (small) return Via::Bounce;
  return bytes >= kDirectCopyBytes ? Via::Copy : Via::Staged;
}

// How long a polled call may spin: 300 us for the launch itself plus what its in-place `bytes` take to cross PCIe
// (~40 GB/s), 2 ms at most
inline uint32_t spin_budget_us(size_t bytes) {
  const size_t us = 300 + bytes / 40000;
  return static_cast<uint32_t>(us < 2000 ? us : 2000);
}

// The wait: hipStreamSynchronize after a small launch costs 11-12 us on this stack; a 32-bit stream write behind the
// kernel into pinned memory, polled by the caller, 8.8 (tools/ubench_sync.hip).  So a call whose sides the kernels
// move themselves (InPlace, Bounce) polls, for spin_us(); one that used the copy engines (Copy, Staged) synchronises.
struct Wait {
  bool sync = false;
  size_t in_place = 0;  // bytes of the InPlace sides
  void add(Via v, size_t bytes) {
    if (v == Via::Copy || v == Via::Staged) sync = true;
    if (v == Via::InPlace) in_place += bytes;
  }
  uint32_t spin_us() const { return spin_budget_us(in_place); }
};

// ---- the decision of a single-state host-buffer call ----------------------------------------------------------------------
// One side as the decision sees it.  A planar side (one buffer per channel) is judged plane by plane -- all planes of a side
// have one size, so one way serves the side -- and staged as an image whose planes lie whole 128-byte lines apart.
struct HostSide {
  bool present = false;  // (an absent input is silence; a result is always present)
  bool pinned = false;   // the kernels reach the buffer where it lies.  The caller's pinned lookup decides, and it is where a
                         // pinned result overlapping its pinned chunk makes the chunk count as not pinned
  bool planar = false;
  size_t judged = 0;     // bytes route_side judges: one plane, or the whole interleaved buffer
  size_t payload = 0;    // bytes of the caller's that move; they count toward small_call while pageable
  size_t image = 0;      // bytes of the staging image: planes on whole lines, else the payload
};
// an interleaved buffer (or one line) of `bytes`; the planes of a side, `plane` bytes each, `pitch` bytes apart in the image
inline HostSide flat_side(bool present, bool pinned, size_t bytes) { return HostSide{present, pinned, false, bytes, bytes, bytes}; }
inline HostSide planar_side(bool present, size_t plane, size_t pitch, size_t n) {
  return HostSide{present, false, true, plane, plane * n, pitch * n};
}
struct HostCallShape {
  HostSide in, out;
  bool split = false;     // the channels of the state stand apart: each writes its own number of frames
  bool gathered = false;  // the input is gathered from several chunks (the chunks call)
  bool strided = false;   // one channel's line with strides on both sides (the per-channel call)
  bool take = false;      // the result is a block the caller owns afterwards (the take call; its out side is pinned)
};
struct HostRoute {
  Via in = Via::None, out = Via::None;
  Wait wait;
  size_t dev_in = 0, dev_out = 0, pin_in = 0, pin_out = 0;  // what the four staging buffers must hold
  size_t in_image = 0, out_image = 0;                       // (the shape's, for the one DMA of a staged image)
  bool strided = false;                                     // (the shape's: the input is gathered sample by sample)
};
// bytes of a side that pass through a device / a pinned staging buffer
inline size_t device_part(Via v, size_t bytes) { return v == Via::Copy || v == Via::Staged ? bytes : 0; }
inline size_t pinned_part(Via v, size_t bytes) { return v == Via::Bounce || v == Via::Staged ? bytes : 0; }

// The entry points differ in small ways that their histories chose; each is one line here and is kept as it is.
inline HostRoute route_host_call(const HostCallShape &s) {
  HostRoute r;
  r.in_image = s.in.image;
  r.out_image = s.out.image;
  r.strided = s.strided;
  const bool planes = s.in.planar || s.out.planar;
  if (s.strided || (s.split && !planes)) {
    // A strided line, and interleaved buffers of a split state (the result is handed over sample by sample): never the
    // bounce way, never in place -- the input by the size rule alone, the result device -> pinned -> the caller.
    r.in = s.strided ? (s.in.present ? Via::Staged : Via::None)  // (a line is gathered sample by sample: pinned, one DMA)
                     : route_side(s.in.judged, s.in.present, false, false);
    r.out = Via::Staged;
    r.wait.sync = true;
    r.dev_in = s.in.image;  // (reserved whatever the input's way, absent included)
    r.pin_in = s.strided ? s.in.image : pinned_part(r.in, s.in.image);  // (a line's: reserved even when absent)
    r.dev_out = r.pin_out = s.out.image;
    return r;
  }
  const bool small = small_call(s.in.present && !s.in.pinned ? s.in.payload : 0, s.out.pinned ? 0 : s.out.payload);
  r.in = route_side(s.in.judged, s.in.present, s.in.pinned, small);
  r.out = route_side(s.out.judged, true, s.out.pinned, small);
  if (s.gathered && r.in == Via::Copy) r.in = Via::Staged;  // chunks are gathered in pinned memory: one DMA from there
  if (s.split && !s.out.planar && r.out == Via::Copy) r.out = Via::Staged;  // handed over sample by sample, from pinned memory
  r.wait.add(r.in, s.in.image);
  r.wait.add(r.out, s.out.image);
  if (s.gathered) r.wait.sync = true;  // the chunks call has always synchronised its stream
  r.dev_in = device_part(r.in, s.in.image);
  r.dev_out = device_part(r.out, s.out.image);
  r.pin_in = pinned_part(r.in, s.in.image);
  r.pin_out = pinned_part(r.out, s.out.image);
  // The completion word of a polled wait: 64 bytes behind the samples in the pinned result buffer.  A call with a planar
  // side reserves it whatever its wait, the chunks call whenever its result bounces; a take call's word lies in its block.
  if (s.take ? false : planes ? true : s.gathered ? r.out == Via::Bounce : !r.wait.sync) r.pin_out += 64;
  return r;
}

}  // namespace speexhip
