// tools/san_host.cpp -- the host-only half of the product (filter_design.cpp, stream_plan.cpp) under ASan + UBSan:
// every rate pair of a grid incl. absurd ones, random positions / pending frames / capacities up to 2^32; and the
// host-buffer calls' decision (host_transfer.h, route_host_call -- the function the product calls) against its tables.
// Built and run by tests/test_cpu_sanitizers.py (GPU sanitizers are not available on the pool).
#include <cstdio>
#include <cstdlib>
#include <random>
#include "devices.h"
#include "filter_design.h"
#include "host_transfer.h"
#include "stream_plan.h"
using namespace speexhip;
int main() {
  std::mt19937 rng(1);
  const uint32_t rates[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000, 1, 7, 4000000};
  long plans = 0, filters = 0;
  for (uint32_t a : rates) for (uint32_t b : rates) for (int q = 0; q <= 10; q += 5) {
    FilterSpec f;
    int rc = design_filter(a, b, q, &f, false);  // geometry first ...
    if (rc != 0) continue;
    if (f.table_len <= 20000) rc = design_filter(a, b, q, &f, true);  // ... tables where they are small
    if (rc != 0) continue;
    filters++;
    if (!f.table.empty() && f.den < 2000) {
      std::vector<double> row(f.taps);
      for (uint32_t ph = 0; ph < f.den; ph += (f.den / 7 + 1)) phase_taps(f, ph, row.data());
    }
    for (int k = 0; k < 40; k++) {
      StreamPos p; p.last = (int32_t)(rng() % (f.taps + 5)); p.frac = rng() % f.den; p.magic = (rng() % 4 == 0) ? rng() % 300 : 0;
      EntryRules r; r.float_entry = rng() & 1; r.block_in = 160 + (rng() % 3 == 0 ? rng() % 500 : 0);
      // (full-range lengths only where whole blocks fast-forward in closed form; extreme up-sampling
      //  walks 160-frame blocks one by one and would dominate the run time)
      const uint32_t big = f.num >= f.den ? rng() : rng() % (1u << 20);
      uint32_t in = rng() % 3 ? rng() % 5000 : big; uint32_t cap = rng() % 3 ? rng() % 6000 : rng();
      CallPlan c = plan_call(f.num, f.den, in, cap, p, r);
      if (c.consumed > in || c.produced > cap || c.end.frac >= f.den) { printf("BAD plan\n"); return 1; }
      (void)phase_index_of(f.num, f.den, p.frac);
      (void)produced_closed_form(f.num, f.den, in, cap, p);
      plans++;
    }
    for (uint32_t m = 0; m < 400; m += 37) { Realign g = realign_history(f.taps, f.taps + 8 * (rng() % 40), m); (void)g; g = realign_history(f.taps + 8 * (rng() % 40), f.taps, m); (void)g; }
    uint32_t fr = rng() % f.den; (void)scale_phase(&fr, 1 + rng() % 100000, f.den);
  }
  // the placement rule (devices_rule.cpp) on well-formed, malformed and random environment strings
  long placements = 0;
  const char *envs[] = {nullptr, "", "all", "0", "7", "8", "-1", "0,1,2", "0,,1", ",", "3, 1 ,2", "all,1", "99999", "1,99999",
                        "0,1,2,3,4,5,6,7,0,1,2,3,4,5,6,7,0,1,2,3,4,5,6,7", "x", " ", "1 2", "0x1"};
  for (int count : {-1, 0, 1, 2, 8, 64})
    for (const char *one : envs)
      for (const char *many : envs)
        for (uint64_t k : {0ull, 1ull, 7ull, 255ull, ~0ull}) {
          const int d = devices::placement_rule(count, one, many, k, static_cast<int>(k % 9) - 1);
          if (d < -1 || d >= (count > 0 ? count : 1)) { printf("BAD placement %d of %d\n", d, count); return 1; }
          placements++;
        }
  for (int n = 0; n < 20000; n++) {
    char buf[24];
    const int len = rng() % 23;
    for (int i = 0; i < len; i++) buf[i] = "0123456789, al-x"[rng() % 16];
    buf[len] = 0;
    const int d = devices::placement_rule(8, (rng() & 1) ? buf : nullptr, buf, rng(), rng() % 8);
    if (d < -1 || d >= 8) { printf("BAD placement\n"); return 1; }
    placements++;
  }
  // the host-buffer staging rule (host_transfer.h): a single-state call, both sides
  const size_t K = 1024, M = 1024 * 1024, Z = kZeroCopyBelow, D = kDirectCopyBytes;
  struct Row {
    size_t in;
    bool in_present, in_pinned;
    size_t out;
    bool out_pinned;
    Via want_in, want_out;
    bool want_sync;
    uint32_t want_spin;  // (polled rows)
  };
  const Row rows[] = {
      {64 * K, true, false, 70 * K, false, Via::Bounce, Via::Bounce, false, 300},
      {500 * K, true, false, 500 * K, false, Via::Bounce, Via::Bounce, false, 300},
      {100 * K, true, false, 800 * K, false, Via::Staged, Via::Copy, true, 0},
      {800 * K, true, false, 100 * K, false, Via::Copy, Via::Staged, true, 0},
      {4 * M, true, false, 4506 * K, false, Via::Copy, Via::Copy, true, 0},
      {D, true, false, Z, false, Via::Copy, Via::Copy, true, 0},  // (D inclusive; out exactly Z: not small)
      {D - 1, true, false, Z, false, Via::Staged, Via::Copy, true, 0},
      {D, true, false, Z - 1, false, Via::Bounce, Via::Bounce, false, 300},
      {4 * M, true, true, 4506 * K, true, Via::InPlace, Via::InPlace, false, spin_budget_us(4 * M + 4506 * K)},
      {4 * M, true, true, 500 * K, false, Via::InPlace, Via::Bounce, false, spin_budget_us(4 * M)},
      {4 * M, true, true, 800 * K, false, Via::InPlace, Via::Copy, true, 0},
      {500 * K, true, false, 1 * M, true, Via::Bounce, Via::InPlace, false, spin_budget_us(1 * M)},
      {1 * M, true, false, 1 * M, true, Via::Copy, Via::InPlace, true, 0},
      {0, false, false, 64 * K, false, Via::None, Via::Bounce, false, 300},
      {4 * M, false, false, 64 * K, false, Via::None, Via::Bounce, false, 300},  // (absent input: 0 pageable bytes)
  };
  long routes = 0;
  for (const Row &r : rows) {
    HostCallShape shape;  // (an interleaved call of a state whose channels stand together: process_host, process_sides_host)
    shape.in = flat_side(r.in_present, r.in_pinned, r.in);
    shape.out = flat_side(true, r.out_pinned, r.out);
    const HostRoute got = route_host_call(shape);
    const Wait &w = got.wait;
    if (got.in != r.want_in || got.out != r.want_out || w.sync != r.want_sync || (!w.sync && w.spin_us() != r.want_spin)) {
      printf("BAD route: in %zu out %zu -> %d / %d sync %d spin %u\n", r.in, r.out, static_cast<int>(got.in), static_cast<int>(got.out),
             w.sync, w.spin_us());
      return 1;
    }
    routes++;
  }
  // Every shape the entry points distinguish, with the sizes of the four staging buffers (device in, device out, pinned in,
  // pinned out).  Each group names the function of the commit before route_host_call existed ("Hold the device-pointer
  // calls to their ordering contract under load") that the rows were read from.
  struct Case {
    const char *name;
    HostSide in, out;
    bool split, gathered, strided, take;
    Via want_in, want_out;
    bool want_sync;
    uint32_t want_spin;  // (polled rows)
    size_t dev_in, dev_out, pin_in, pin_out;
  };
  const size_t W = 64;  // the completion word
  const bool no = false, yes = true;
  const Case cases[] = {
      // interleaved, channels together -- Batch::process_host, engine.cpp:1286-1315; Batch::routed_host_call, formats.cpp:200-233:
      // the word only for a polled wait
      {"whole small", flat_side(yes, no, 64 * K), flat_side(yes, no, 70 * K), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, 64 * K, 70 * K + W},
      {"whole up", flat_side(yes, no, 100 * K), flat_side(yes, no, 800 * K), no, no, no, no, Via::Staged, Via::Copy, true, 0, 100 * K, 800 * K, 100 * K, 0},
      {"whole down", flat_side(yes, no, 800 * K), flat_side(yes, no, 100 * K), no, no, no, no, Via::Copy, Via::Staged, true, 0, 800 * K, 100 * K, 0, 100 * K},
      {"whole D / Z-1", flat_side(yes, no, D), flat_side(yes, no, Z - 1), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, D, Z - 1 + W},
      {"whole D-1 / Z", flat_side(yes, no, D - 1), flat_side(yes, no, Z), no, no, no, no, Via::Staged, Via::Copy, true, 0, D - 1, Z, D - 1, 0},
      {"whole D / Z", flat_side(yes, no, D), flat_side(yes, no, Z), no, no, no, no, Via::Copy, Via::Copy, true, 0, D, Z, 0, 0},
      {"whole Z / small", flat_side(yes, no, Z), flat_side(yes, no, 64 * K), no, no, no, no, Via::Copy, Via::Staged, true, 0, Z, 64 * K, 0, 64 * K},
      {"whole Z-1 / small", flat_side(yes, no, Z - 1), flat_side(yes, no, 64 * K), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, Z - 1, 64 * K + W},
      {"whole pinned in", flat_side(yes, yes, 4 * M), flat_side(yes, no, 500 * K), no, no, no, no, Via::InPlace, Via::Bounce, false, spin_budget_us(4 * M), 0, 0, 0, 500 * K + W},
      {"whole pinned both", flat_side(yes, yes, 4 * M), flat_side(yes, yes, 1 * M), no, no, no, no, Via::InPlace, Via::InPlace, false, spin_budget_us(5 * M), 0, 0, 0, W},
      {"whole pinned in, copy out", flat_side(yes, yes, 4 * M), flat_side(yes, no, 800 * K), no, no, no, no, Via::InPlace, Via::Copy, true, 0, 0, 800 * K, 0, 0},
      {"whole silence", flat_side(no, no, 4 * M), flat_side(yes, no, 64 * K), no, no, no, no, Via::None, Via::Bounce, false, 300, 0, 0, 0, 64 * K + W},
      // interleaved, channels apart -- process_host, engine.cpp:1262-1285; process_sides_host, formats.cpp:266-290: the input
      // by the size rule alone (never bounced, never in place), the result device -> pinned whatever its size, a synchronise;
      // the device input buffer holds the input's bytes whatever its way
      {"split small", flat_side(yes, no, 64 * K), flat_side(yes, no, 70 * K), yes, no, no, no, Via::Staged, Via::Staged, true, 0, 64 * K, 70 * K, 64 * K, 70 * K},
      {"split D", flat_side(yes, no, D), flat_side(yes, no, 70 * K), yes, no, no, no, Via::Copy, Via::Staged, true, 0, D, 70 * K, 0, 70 * K},
      {"split D-1", flat_side(yes, no, D - 1), flat_side(yes, no, 70 * K), yes, no, no, no, Via::Staged, Via::Staged, true, 0, D - 1, 70 * K, D - 1, 70 * K},
      {"split big out", flat_side(yes, no, 64 * K), flat_side(yes, no, 4 * M), yes, no, no, no, Via::Staged, Via::Staged, true, 0, 64 * K, 4 * M, 64 * K, 4 * M},
      {"split silence", flat_side(no, no, 4 * K), flat_side(yes, no, 70 * K), yes, no, no, no, Via::None, Via::Staged, true, 0, 4 * K, 70 * K, 0, 70 * K},
      // planes on both sides -- Batch::process_planar_host, planar.cpp:138-150 (and planes_host_call below with both sides
      // planar): a plane is judged, the payload of all planes decides `small`, the image on whole lines is staged; the word
      // always; channels apart take the same ways
      {"planar small", planar_side(yes, 1000, 1024, 2), planar_side(yes, 1100, 1152, 2), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, 2048, 2304 + W},
      {"planar small, apart", planar_side(yes, 1000, 1024, 2), planar_side(yes, 1100, 1152, 2), yes, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, 2048, 2304 + W},
      {"planar plane D-1 of 4", planar_side(yes, D - 1, D, 4), planar_side(yes, D, D, 4), no, no, no, no, Via::Staged, Via::Copy, true, 0, 4 * D, 4 * D, 4 * D, W},
      {"planar plane D of 4", planar_side(yes, D, D, 4), planar_side(yes, 1000, 1024, 4), no, no, no, no, Via::Copy, Via::Staged, true, 0, 4 * D, 4096, 0, 4096 + W},
      {"planar payload Z", planar_side(yes, Z / 2, Z / 2, 2), planar_side(yes, 1000, 1024, 2), no, no, no, no, Via::Copy, Via::Staged, true, 0, Z, 2048, 0, 2048 + W},
      {"planar payload Z-2", planar_side(yes, Z / 2 - 1, Z / 2, 2), planar_side(yes, 1000, 1024, 2), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, Z, 2048 + W},
      {"planar silence", planar_side(no, 1000, 1024, 2), planar_side(yes, 1100, 1152, 2), no, no, no, no, Via::None, Via::Bounce, false, 300, 0, 0, 0, 2304 + W},
      // one planar side -- Batch::planes_host_call, formats.cpp:326-345: the interleaved side as in process_host (in place
      // when pinned), the word always; channels apart: nothing in place, the bounce way stays open, and an interleaved
      // result is handed over sample by sample, so Copy becomes Staged (formats.cpp:339)
      {"planes in", planar_side(yes, 1000, 1024, 2), flat_side(yes, no, 4000), no, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, 2048, 4000 + W},
      {"planes out, pinned in", flat_side(yes, yes, 1 * M), planar_side(yes, 1000, 1024, 2), no, no, no, no, Via::InPlace, Via::Bounce, false, spin_budget_us(1 * M), 0, 0, 0, 2048 + W},
      {"planes in, copy out", planar_side(yes, 1000, 1024, 2), flat_side(yes, no, 800 * K), no, no, no, no, Via::Staged, Via::Copy, true, 0, 2048, 800 * K, 2048, W},
      {"planes in, apart, copy out", planar_side(yes, 1000, 1024, 2), flat_side(yes, no, 800 * K), yes, no, no, no, Via::Staged, Via::Staged, true, 0, 2048, 800 * K, 2048, 800 * K + W},
      {"planes in, apart, small", planar_side(yes, 1000, 1024, 2), flat_side(yes, no, 4000), yes, no, no, no, Via::Bounce, Via::Bounce, false, 300, 0, 0, 2048, 4000 + W},
      {"planes out, apart, copy out", flat_side(yes, no, 100 * K), planar_side(yes, D, D, 4), yes, no, no, no, Via::Staged, Via::Copy, true, 0, 100 * K, 4 * D, 100 * K, W},
      // the result in a block the caller owns -- Batch::process_host_take, single-launch branch, engine.cpp:1215-1236: the
      // result in place (0 pageable bytes), no pinned result buffer: the word lies in the block
      {"take small", flat_side(yes, no, 64 * K), flat_side(yes, yes, 4 * M), no, no, no, yes, Via::Bounce, Via::InPlace, false, spin_budget_us(4 * M), 0, 0, 64 * K, 0},
      {"take Z-1", flat_side(yes, no, Z - 1), flat_side(yes, yes, 4 * M), no, no, no, yes, Via::Bounce, Via::InPlace, false, spin_budget_us(4 * M), 0, 0, Z - 1, 0},
      {"take Z", flat_side(yes, no, Z), flat_side(yes, yes, 4 * M), no, no, no, yes, Via::Copy, Via::InPlace, true, 0, Z, 0, 0, 0},
      {"take pinned in", flat_side(yes, yes, 4 * M), flat_side(yes, yes, 4 * M), no, no, no, yes, Via::InPlace, Via::InPlace, false, spin_budget_us(8 * M), 0, 0, 0, 0},
      {"take silence", flat_side(no, no, 4 * M), flat_side(yes, yes, 64 * K), no, no, no, yes, Via::None, Via::InPlace, false, spin_budget_us(64 * K), 0, 0, 0, 0},
      // gathered chunks -- Batch::process_host_chunks, engine.cpp:1424-1454: zero_copy and direct_out; the chunks are gathered in
      // pinned memory (never Copy), the wait is a synchronise, the word is reserved when the result bounces
      {"chunks small", flat_side(yes, no, 500 * K), flat_side(yes, no, 500 * K), no, yes, no, no, Via::Bounce, Via::Bounce, true, 0, 0, 0, 500 * K, 500 * K + W},
      {"chunks Z-1 / Z-1", flat_side(yes, no, Z - 1), flat_side(yes, no, Z - 1), no, yes, no, no, Via::Bounce, Via::Bounce, true, 0, 0, 0, Z - 1, Z - 1 + W},
      {"chunks Z / small", flat_side(yes, no, Z), flat_side(yes, no, 100 * K), no, yes, no, no, Via::Staged, Via::Staged, true, 0, Z, 100 * K, Z, 100 * K},
      {"chunks small / Z", flat_side(yes, no, 100 * K), flat_side(yes, no, Z), no, yes, no, no, Via::Staged, Via::Copy, true, 0, 100 * K, Z, 100 * K, 0},
      {"chunks Z / D-1", flat_side(yes, no, Z), flat_side(yes, no, D - 1), no, yes, no, no, Via::Staged, Via::Staged, true, 0, Z, D - 1, Z, D - 1},
      {"chunks Z / D", flat_side(yes, no, Z), flat_side(yes, no, D), no, yes, no, no, Via::Staged, Via::Copy, true, 0, Z, D, Z, 0},
      // one channel's strided line -- Batch::process_channel_host, engine.cpp:1333-1349: pinned then DMA both ways whatever the
      // size, a synchronise, all four buffers reserved even for silence
      {"line", flat_side(yes, no, 4 * K), flat_side(yes, no, 5 * K), no, no, yes, no, Via::Staged, Via::Staged, true, 0, 4 * K, 5 * K, 4 * K, 5 * K},
      {"line big", flat_side(yes, no, 4 * M), flat_side(yes, no, 5 * M), no, no, yes, no, Via::Staged, Via::Staged, true, 0, 4 * M, 5 * M, 4 * M, 5 * M},
      {"line silence", flat_side(no, no, 4 * K), flat_side(yes, no, 5 * K), no, no, yes, no, Via::None, Via::Staged, true, 0, 4 * K, 5 * K, 4 * K, 5 * K},
  };
  for (const Case &c : cases) {
    HostCallShape shape;
    shape.in = c.in;
    shape.out = c.out;
    shape.split = c.split;
    shape.gathered = c.gathered;
    shape.strided = c.strided;
    shape.take = c.take;
    const HostRoute got = route_host_call(shape);
    if (got.in != c.want_in || got.out != c.want_out || got.wait.sync != c.want_sync ||
        (!got.wait.sync && got.wait.spin_us() != c.want_spin) || got.dev_in != c.dev_in || got.dev_out != c.dev_out ||
        got.pin_in != c.pin_in || got.pin_out != c.pin_out) {
      printf("BAD route (%s): %d / %d sync %d spin %u, buffers %zu %zu %zu %zu\n", c.name, static_cast<int>(got.in),
             static_cast<int>(got.out), got.wait.sync, got.wait.spin_us(), got.dev_in, got.dev_out, got.pin_in, got.pin_out);
      return 1;
    }
    routes++;
  }
  if (small_call(0, Z) || !small_call(Z - 1, Z - 1) || spin_budget_us(4 * M + 4506 * K) <= 300 || spin_budget_us(1ull << 40) != 2000) {
    printf("BAD thresholds\n");
    return 1;
  }
  printf("sanitizer run ok: %ld filters, %ld plans, %ld placements, %ld routes\n", filters, plans, placements, routes);
  return 0;
}
