// host_transfer.h -- how a host-buffer call moves its buffers and how it waits (host only; tools/san_host.cpp checks it).
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

}  // namespace speexhip
