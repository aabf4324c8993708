// tools/san_host.cpp -- the host-only half of the product (filter_design.cpp, stream_plan.cpp) under ASan + UBSan:
// every rate pair of a grid incl. absurd ones, random positions / pending frames / capacities up to 2^32; and the
// host-buffer calls' decisions (host_transfer.h, route_host_call; many_plan.h, plan_many_unit and plan_many_lanes -- the
// functions the product calls) against their tables, the many-states one over random units as well.
// Built and run by tests/test_cpu_sanitizers.py (GPU sanitizers are not available on the pool).
#include <cstdio>
#include <cstdlib>
#include <random>
#include "devices.h"
#include "filter_design.h"
#include "host_transfer.h"
#include "many_plan.h"
#include "stream_plan.h"
using namespace speexhip;

// ---- the many-states call's decision (many_plan.h: plan_many_unit, plan_many_lanes -- the functions many.cpp calls) ----------
// The rows were read off Batch::many_on_device and Batch::many_run of the commit before the planner existed ("Formatted
// chunk coalescing and sample formats in the Node stream paths", csrc/many.cpp); each cites the lines it was read from.
namespace {
const size_t KB = 1024, MB = 1024 * 1024, Zc = kZeroCopyBelow, Dc = kDirectCopyBytes;
ManyShape many_shape(size_t in, size_t out, bool in_pinned = false, bool out_pinned = false) {
  ManyShape s;
  s.in_bytes = in, s.out_bytes = out;
  s.in_present = s.work = true;
  s.in_pinned = in_pinned, s.out_pinned = out_pinned;
  return s;
}
struct ManyWant {
  Via in, out;
  size_t in_off, out_off;
};
typedef std::vector<std::vector<uint32_t>> Launches;
Launches launches_of(const ManyUnitPlan &p) {
  Launches all;
  for (const ManyLaunch &l : p.launches) all.push_back(l.entries);
  return all;
}
bool many_is(const char *name, const ManyUnitPlan &p, const std::vector<ManyWant> &want, const Launches &launches) {
  bool ok = p.e.size() == want.size() && launches_of(p) == launches;
  for (size_t k = 0; ok && k < want.size(); k++)
    ok = p.e[k].in == want[k].in && p.e[k].out == want[k].out && p.e[k].in_off == want[k].in_off && p.e[k].out_off == want[k].out_off;
  if (ok) return true;
  printf("BAD many-states plan (%s):", name);
  for (const ManyEntryPlan &e : p.e) printf(" [%d / %d at %zu / %zu]", static_cast<int>(e.in), static_cast<int>(e.out), e.in_off, e.out_off);
  printf(", launches");
  for (const ManyLaunch &l : p.launches) printf(" %zu", l.entries.size());
  printf("\n");
  return false;
}
#define MANY_EXPECT(cond)                                            \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("BAD many-states plan (%s): not %s\n", name, #cond);    \
      return false;                                                  \
    }                                                                \
  } while (0)
ManyUnitPlan many_plan_of(const std::vector<ManyShape> &s, ManySwitches sw = ManySwitches()) { return plan_many_unit(s.data(), s.size(), sw); }

bool check_many_plans(long *rows) {
  const ManySwitches in_place_switch = {0, -1}, no_pipeline = {1, 0};
  const Via N = Via::None, I = Via::InPlace, B = Via::Bounce, C = Via::Copy, S = Via::Staged;
  const char *name;
  ManyUnitPlan p;
  std::vector<ManyShape> s;

  name = "all small";  // many.cpp:164-173 (small: every side bounces, nothing synchronises), :190-198 (the pinned pair alone)
  s.assign(5, many_shape(256, 280));
  p = many_plan_of(s);
  if (!many_is(name, p, {{B, B, 0, 0}, {B, B, 256, 320}, {B, B, 512, 640}, {B, B, 768, 960}, {B, B, 1024, 1280}}, {{0, 1, 2, 3, 4}})) return false;
  MANY_EXPECT(p.small && !p.wait.sync && p.wait.spin_us() == 300 && !p.pipelined && !p.all_big);
  MANY_EXPECT(p.total_in == 1280 && p.total_out == 1600 && p.gathered_in == 1280 && p.gathered_out == 1600);
  MANY_EXPECT(p.pin_in == 1280 && p.pin_out == 1600 + 128 && p.dev_in == 0 && p.dev_out == 0 && p.dev_img_in == 0 && p.dev_img_out == 0);
  (*rows)++;

  name = "in total exactly Z";  // :158, :164 -- the totals are the laid-out ones: two sides of Z/2 - 1 bytes lie on Z bytes
  for (size_t less : {size_t(0), size_t(1)}) {
    s.assign(2, many_shape(Zc / 2 - less, 1000));
    p = many_plan_of(s);
    if (!many_is(name, p, {{C, S, 0, 0}, {C, S, Zc / 2, 1024}}, {{0, 1}})) return false;
    MANY_EXPECT(!p.small && p.total_in == Zc && p.wait.sync && p.gathered_in == 0 && p.gathered_out == 2048 && p.pin_in == 0 && p.dev_in == Zc);
    (*rows)++;
  }
  name = "in total Z - 64";  // :164 -- small although each buffer is past kDirectCopyBytes
  s = {many_shape(Zc / 2, 1000), many_shape(Zc / 2 - 64, 1000)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{B, B, 0, 0}, {B, B, Zc / 2, 1024}}, {{0, 1}})) return false;
  MANY_EXPECT(p.small && p.pin_in == Zc - 64 && p.dev_in == 0);
  (*rows)++;
  name = "out total exactly Z";  // :159, :164
  s.assign(2, many_shape(1000, Zc / 2));
  p = many_plan_of(s);
  if (!many_is(name, p, {{S, C, 0, 0}, {S, C, 1024, Zc / 2}}, {{0, 1}})) return false;
  MANY_EXPECT(!p.small && p.total_out == Zc && p.gathered_in == 2048 && p.gathered_out == 0 && p.pin_out == 128 && p.dev_out == Zc);
  (*rows)++;

  // :168-169 (route_side: kDirectCopyBytes inclusive), :176-189 (pass 0 lays the gathered sides out from 0 in entry order,
  // pass 1 the Copy ones behind them; every side on whole 64-byte lines), :190-193
  name = "D - 1 against D; gathered first";
  s = {many_shape(Dc - 1, Dc), many_shape(Dc, Dc - 1), many_shape(Zc, 100)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{S, C, 0, Dc + 128}, {C, S, Dc, 0}, {C, S, 2 * Dc, Dc}}, {{0, 1, 2}})) return false;
  MANY_EXPECT(!p.small && p.wait.sync && !p.all_big && !p.pipelined);
  MANY_EXPECT(p.gathered_in == Dc && p.gathered_out == Dc + 128 && p.total_in == 2 * Dc + Zc && p.total_out == 2 * Dc + 128);
  MANY_EXPECT(p.pin_in == Dc && p.pin_out == Dc + 128 + 128 && p.dev_in == p.total_in && p.dev_out == p.total_out);
  (*rows)++;

  // :147-149 (the caller's lookup), :158-159 (a pinned side counts 0 pageable bytes), :168-171 (in place; its bytes make
  // the spin budget), :175 (nothing of it in the stage)
  name = "pinned in";
  s = {many_shape(4 * MB, 100 * KB, true, false), many_shape(64 * KB, 64 * KB)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{I, B, 0, 0}, {B, B, 0, 100 * KB}}, {{0, 1}})) return false;
  MANY_EXPECT(p.small && !p.wait.sync && p.wait.spin_us() == spin_budget_us(4 * MB) && p.pin_in == 64 * KB && !p.e[0].demoted);
  (*rows)++;
  name = "pinned out";
  s = {many_shape(4 * MB, 4 * MB, false, true), many_shape(64 * KB, 64 * KB)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{C, I, 64 * KB, 0}, {S, S, 0, 0}}, {{0, 1}})) return false;
  MANY_EXPECT(!p.small && p.wait.sync && p.total_out == 64 * KB && p.dev_out == 64 * KB && p.dev_in == 4 * MB + 64 * KB);
  (*rows)++;
  name = "pinned both";
  s = {many_shape(4 * MB, 4 * MB, true, true)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{I, I, 0, 0}}, {{0}})) return false;
  MANY_EXPECT(p.small && !p.wait.sync && p.wait.spin_us() == spin_budget_us(8 * MB) && p.total_in == 0 && p.total_out == 0);
  MANY_EXPECT(p.pin_in == 0 && p.pin_out == 128 && p.dev_in == 0 && p.dev_out == 0 && !p.e[0].demoted);
  (*rows)++;

  // :154-156 -- a pinned input beside a pageable result of at least kDirectCopyBytes is copied like a pageable one
  name = "pinned in demoted";
  s = {many_shape(4 * MB, Dc, true, false)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{C, C, 0, 0}}, {{0}})) return false;  // (not small: 4 MiB of input count again)
  MANY_EXPECT(p.e[0].demoted && !p.small && p.total_in == 4 * MB && p.wait.in_place == 0);
  (*rows)++;
  name = "pinned in demoted, small";
  s = {many_shape(64 * KB, Dc, true, false)};
  p = many_plan_of(s);
  if (!many_is(name, p, {{B, B, 0, 0}}, {{0}})) return false;
  MANY_EXPECT(p.e[0].demoted && p.small && p.pin_in == 64 * KB);
  (*rows)++;
  name = "pinned in, switch 0";
  p = many_plan_of({many_shape(4 * MB, Dc, true, false)}, in_place_switch);
  if (!many_is(name, p, {{I, B, 0, 0}}, {{0}})) return false;
  MANY_EXPECT(!p.e[0].demoted && p.small && p.total_in == 0);
  (*rows)++;
  name = "pinned in, smaller result";
  p = many_plan_of({many_shape(4 * MB, Dc - 1, true, false)});
  if (!many_is(name, p, {{I, B, 0, 0}}, {{0}})) return false;
  MANY_EXPECT(!p.e[0].demoted && p.small);
  (*rows)++;
  name = "pinned both is never demoted";
  p = many_plan_of({many_shape(4 * MB, 4 * MB, true, true), many_shape(Zc, Zc)});
  if (!many_is(name, p, {{I, I, 0, 0}, {C, C, 0, 0}}, {{0, 1}})) return false;
  MANY_EXPECT(!p.e[0].demoted && !p.all_big);  // (:172: a working entry that is not Copy both ways)
  (*rows)++;

  // :137 (an absent input has no bytes), :168 (route_side: absent -> None; a present input of 0 bytes takes a way)
  name = "absent and empty inputs";
  s = {many_shape(0, 1000), many_shape(0, 1000), many_shape(Zc, 1000)};
  s[0].in_present = false;
  p = many_plan_of(s);
  if (!many_is(name, p, {{N, S, 0, 0}, {S, S, 0, 1024}, {C, S, 0, 2048}}, {{0, 1, 2}})) return false;
  s.pop_back();
  p = many_plan_of(s);
  if (!many_is(name, p, {{N, B, 0, 0}, {B, B, 0, 1024}}, {{0, 1}})) return false;
  MANY_EXPECT(p.small && p.pin_in == 0);
  (*rows)++;

  // :157, :212 -- an entry with nothing to run is routed and laid out but is in no launch; :172 -- and does not decide all_big
  name = "an entry without work";
  s = {many_shape(Zc, Zc), many_shape(0, 0), many_shape(Zc, Zc)};
  s[1].work = false;
  p = many_plan_of(s);
  if (!many_is(name, p, {{C, C, 0, 0}, {S, S, 0, 0}, {C, C, Zc, Zc}}, {{0, 2}})) return false;
  MANY_EXPECT(p.all_big && !p.pipelined);
  s[0].work = s[2].work = false;
  p = many_plan_of(s);
  MANY_EXPECT(p.launches.empty() && p.wait.sync && !p.pipelined);
  (*rows)++;

  // :208-226 -- std::map over std::tuple<tables, mode, float_seen, float_io>: the groups in key order, entries in call order
  name = "two keys";
  s.assign(5, many_shape(256, 280));
  s[0].key = s[2].key = ManyKey{20, 0, false, false};
  s[1].key = s[3].key = s[4].key = ManyKey{10, 1, true, true};
  p = many_plan_of(s);
  MANY_EXPECT((launches_of(p) == Launches{{1, 3, 4}, {0, 2}}));
  {
    const ManyKey order[] = {{10, 0, false, false}, {10, 0, false, true}, {10, 0, true, false}, {10, 0, true, true}, {10, 1, false, false}, {11, 0, false, false}};
    for (size_t a = 0; a < 6; a++)
      for (size_t b = 0; b < 6; b++) MANY_EXPECT((order[a] < order[b]) == (a < b));
    for (size_t a = 0; a < 5; a++) s[a].key = order[5 - a];
    p = many_plan_of(s);
    MANY_EXPECT((launches_of(p) == Launches{{4}, {3}, {2}, {1}, {0}}));
  }
  (*rows)++;
  name = "33 entries of one key";  // :217, :224-225 -- at most 32 per launch
  s.assign(33, many_shape(256, 280));
  p = many_plan_of(s);
  MANY_EXPECT(p.launches.size() == 2 && p.launches[0].entries.size() == 32 && p.launches[1].entries == std::vector<uint32_t>{32} && p.launches[0].entries[31] == 31);
  (*rows)++;

  // :166-172 (all_big), :203 (the laid-out pageable input total at least 32 MiB, the switch), :218-223 (a group in
  // pieces of about 16 MiB of raw input: bytes / 16 MiB pieces, the entries shared out among them), :308 (two launches)
  name = "pipelined at exactly 32 MiB";
  s.assign(8, many_shape(4 * MB, 4 * MB));
  p = many_plan_of(s);
  MANY_EXPECT(p.all_big && p.pipelined && p.total_in == 32 * MB && (launches_of(p) == Launches{{0, 1, 2, 3}, {4, 5, 6, 7}}));
  MANY_EXPECT(p.e[7].in == Via::Copy && p.e[7].in_off == 28 * MB && p.gathered_in == 0 && p.dev_in == 32 * MB && p.dev_out == 32 * MB);
  (*rows)++;
  name = "64 bytes below 32 MiB";
  s[3].in_bytes -= 64;
  p = many_plan_of(s);
  MANY_EXPECT(p.all_big && !p.pipelined && p.launches.size() == 1 && p.launches[0].entries.size() == 8);
  (*rows)++;
  name = "pipelined, two keys";  // (each group 16 MiB: one piece, one launch each)
  s.assign(8, many_shape(4 * MB, 4 * MB));
  for (size_t k = 0; k < 4; k++) s[2 * k].key.mode = 1;
  p = many_plan_of(s);
  MANY_EXPECT(p.pipelined && (launches_of(p) == Launches{{1, 3, 5, 7}, {0, 2, 4, 6}}));
  (*rows)++;
  name = "pipelined, an idle small entry beside";
  s.push_back(many_shape(100, 0));
  s[8].work = false;
  p = many_plan_of(s);
  MANY_EXPECT(p.all_big && p.pipelined && p.launches.size() == 2 && p.e[8].in == Via::Staged && p.gathered_in == 128);
  (*rows)++;
  name = "not pipelined: a working entry that is not Copy both ways";
  s[8].work = true;
  p = many_plan_of(s);
  MANY_EXPECT(!p.all_big && !p.pipelined && p.launches.size() == 2 && p.launches[0].entries.size() == 5);
  (*rows)++;
  name = "not pipelined: the switch at 0";
  s.assign(8, many_shape(4 * MB, 4 * MB));
  p = many_plan_of(s, no_pipeline);
  MANY_EXPECT(p.all_big && !p.pipelined && p.launches.size() == 1);
  (*rows)++;
  name = "not pipelined: one launch";  // (:221-222: 2 pieces, but one entry)
  p = many_plan_of({many_shape(32 * MB, 32 * MB)});
  MANY_EXPECT(p.all_big && !p.pipelined && p.launches.size() == 1);
  p = many_plan_of({many_shape(16 * MB, 16 * MB), many_shape(16 * MB, 16 * MB)});
  MANY_EXPECT(p.pipelined && (launches_of(p) == Launches{{0}, {1}}));
  p = many_plan_of(std::vector<ManyShape>(40, many_shape(1 * MB, 1 * MB)));  // (40 MiB: 2 pieces of 20 entries)
  MANY_EXPECT(p.pipelined && p.launches.size() == 2 && p.launches[0].entries.size() == 20);
  p = many_plan_of(std::vector<ManyShape>(130, many_shape(Dc, Dc)));  // (32.5 MiB: 2 pieces of 65, 32 per launch at most)
  MANY_EXPECT(p.pipelined && p.launches.size() == 5 && p.launches[0].entries.size() == 32 && p.launches[4].entries.size() == 2);
  (*rows)++;

  // :141-146 (an image per side that passes through one, on whole 128-byte lines, in entry order), :195-196 (256 bytes of slack)
  name = "images";
  s.assign(4, many_shape(256, 280));
  s[0].pass_in = s[2].pass_in = s[3].pass_in = true;
  s[1].pass_out = true;
  s[0].image_in = 100, s[2].image_in = 128, s[3].image_in = 129, s[1].image_out = 1000;
  s[1].image_in = 4096;  // (no pass on that side: no image)
  p = many_plan_of(s);
  MANY_EXPECT(p.e[0].img_in == 0 && p.e[1].img_in == 128 && p.e[2].img_in == 128 && p.e[3].img_in == 256 && p.images_in == 512);
  MANY_EXPECT(p.e[1].img_out == 0 && p.e[2].img_out == 1024 && p.images_out == 1024 && p.dev_img_in == 512 + 256 && p.dev_img_out == 1024 + 256);
  (*rows)++;

  // many_run, :505-507: the pageable bytes of the busier direction, at least 8 states, at least 128 MiB; SPEEXHIP_MANY_LANES
  // 1 = never, 2 = always (still 8 states); :511 the first half is lane 0
  name = "lanes";
  const uint64_t L = static_cast<uint64_t>(128) << 20;
  MANY_EXPECT(plan_many_lanes(7, 8 * L, 8 * L, -1) == 7 && plan_many_lanes(8, L - 1, L - 1, -1) == 8 && plan_many_lanes(8, L, 0, -1) == 4);
  MANY_EXPECT(plan_many_lanes(8, 0, L, -1) == 4 && plan_many_lanes(9, L, L, -1) == 4 && plan_many_lanes(64, L / 2, L / 2, -1) == 64);
  MANY_EXPECT(plan_many_lanes(64, 8 * L, 8 * L, 1) == 64 && plan_many_lanes(8, 0, 0, 2) == 4 && plan_many_lanes(7, 8 * L, 0, 2) == 7);
  (*rows)++;
  name = "priming";  // many_run, :519-521: the raw input bytes of the unit's entries, whatever their way
  MANY_EXPECT(!many_primes_copy_stream(32 * MB - 1) && many_primes_copy_stream(32 * MB));
  (*rows)++;
  return true;
}

// Random units from a fixed seed: what must hold whatever the shapes are.
bool check_many_invariants(std::mt19937 &rng, long *units) {
  const char *name = "random";
  const size_t sizes[] = {0, 1, 63, 64, 65, 1000, 64 * KB, Dc - 1, Dc, Dc + 1, Zc / 2 - 1, Zc / 2, Zc - 1, Zc, 1 * MB, 4 * MB, 16 * MB};
  for (int round = 0; round < 4000; round++) {
    const size_t n = 1 + rng() % (round % 50 == 0 ? 140 : 12);
    const size_t top = 6 + rng() % 12;  // (most rounds stay small, some reach the pipelined sizes)
    std::vector<ManyShape> s(n);
    for (ManyShape &e : s) {
      e = many_shape(sizes[rng() % top], sizes[rng() % top], rng() % 4 == 0, rng() % 4 == 0);
      if (rng() % 8 == 0) e.in_present = false, e.in_bytes = 0, e.in_pinned = false;
      e.work = rng() % 6 != 0;
      e.pass_in = e.in_present && e.in_bytes != 0 && rng() % 3 == 0;
      e.pass_out = rng() % 3 == 0;
      e.image_in = 2 * e.in_bytes, e.image_out = 2 * e.out_bytes;
      e.key = ManyKey{static_cast<uintptr_t>(4096 * (1 + rng() % 2)), static_cast<int>(rng() % 2), rng() % 2 == 0, rng() % 2 == 0};
    }
    const ManySwitches sw = {static_cast<int>(rng() % 2), static_cast<int>(rng() % 3) - 1};
    const ManyUnitPlan p = plan_many_unit(s.data(), n, sw);
    MANY_EXPECT(p.e.size() == n);
    // the stage: offsets on 64-byte lines; the gathered sides contiguous from 0 in entry order, the Copy ones behind them
    // and apart; everything inside the buffer it passes through
    for (int side = 0; side < 2; side++) {
      const size_t gathered = side ? p.gathered_out : p.gathered_in, pin = side ? p.pin_out : p.pin_in, dev = side ? p.dev_out : p.dev_in;
      size_t next = 0;
      std::vector<std::pair<size_t, size_t>> copied;
      for (size_t k = 0; k < n; k++) {
        const Via v = side ? p.e[k].out : p.e[k].in;
        const size_t off = side ? p.e[k].out_off : p.e[k].in_off, bytes = side ? s[k].out_bytes : s[k].in_bytes;
        MANY_EXPECT(off % 64 == 0);
        MANY_EXPECT(!p.small || (v != Via::Copy && v != Via::Staged));
        MANY_EXPECT(p.small || v != Via::Bounce);
        if (v == Via::Copy) {
          MANY_EXPECT(off >= gathered && off + bytes <= dev);
          copied.push_back(std::make_pair(off, bytes));
        } else {
          MANY_EXPECT(off == next);
          if (v == Via::Bounce || v == Via::Staged) next += align64(bytes);
          MANY_EXPECT(pinned_part(v, bytes) == 0 || off + bytes <= pin);
          MANY_EXPECT(device_part(v, bytes) == 0 || off + bytes <= dev);
        }
      }
      MANY_EXPECT(next == gathered && gathered <= pin && (p.small || gathered <= dev));
      MANY_EXPECT(!side || p.pin_out >= gathered + 64);  // (the completion word behind the gathered results)
      std::sort(copied.begin(), copied.end());
      for (size_t k = 1; k < copied.size(); k++) MANY_EXPECT(copied[k - 1].first + copied[k - 1].second <= copied[k].first);
    }
    // the images: on 128-byte lines, apart, inside their buffer
    size_t img_in = 0, img_out = 0;
    for (size_t k = 0; k < n; k++) {
      MANY_EXPECT(p.e[k].img_in == img_in && p.e[k].img_out == img_out && img_in % 128 == 0 && img_out % 128 == 0);
      if (s[k].pass_in) img_in += align128(s[k].image_in);
      if (s[k].pass_out) img_out += align128(s[k].image_out);
    }
    MANY_EXPECT(img_in <= p.dev_img_in && img_out <= p.dev_img_out && (img_in == 0) == (p.dev_img_in == 0));
    // the launches: every working entry in exactly one, no other entry in any; at most 32 of one key, keys never going back
    std::vector<int> seen(n, 0);
    for (size_t g = 0; g < p.launches.size(); g++) {
      const std::vector<uint32_t> &l = p.launches[g].entries;
      MANY_EXPECT(!l.empty() && l.size() <= 32);
      for (uint32_t k : l) {
        MANY_EXPECT(k < n && s[k].work && seen[k]++ == 0);
        MANY_EXPECT(!(s[k].key < s[l[0]].key) && !(s[l[0]].key < s[k].key));
      }
      MANY_EXPECT(g == 0 || !(s[l[0]].key < s[p.launches[g - 1].entries[0]].key));
    }
    for (size_t k = 0; k < n; k++) MANY_EXPECT(seen[k] == (s[k].work ? 1 : 0));
    MANY_EXPECT(!p.pipelined || (p.all_big && p.launches.size() >= 2 && sw.pipeline != 0 && p.total_in >= (32 * MB)));
    (*units)++;
  }
  return true;
}
}  // namespace

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
  long many_rows = 0, many_random = 0;
  if (!check_many_plans(&many_rows) || !check_many_invariants(rng, &many_random)) return 1;
  printf("sanitizer run ok: %ld filters, %ld plans, %ld placements, %ld routes, %ld many-states rows, %ld random many-states units\n",
         filters, plans, placements, routes, many_rows, many_random);
  return 0;
}
