// tools/san_host.cpp -- the host-only half of the product (filter_design.cpp, stream_plan.cpp) under ASan + UBSan:
// every rate pair of a grid incl. absurd ones, random positions / pending frames / capacities up to 2^32; and the
// host-buffer calls' decisions (host_transfer.h, route_host_call; many_plan.h, plan_many_unit and plan_many_lanes -- the
// functions the product calls; sides_route.h, route_sides_call) against their tables, the many-states one over random units
// and the formatted calls' one over its whole input space as well; and the statement of a mixer leg's level (levels.h) at
// its decision points and over random floats.
// Built and run by tests/test_cpu_sanitizers.py (GPU sanitizers are not available on the pool).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include "devices.h"
#include "filter_design.h"
#include "host_transfer.h"
#include "levels.h"
#include "many_plan.h"
#include "sides_route.h"
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
  // The legs of a mixer call (mixer.cpp, many.cpp: run_mixer): the table at the head of the range that travels in, the
  // buses at the head of the range that travels out, every leg's result an image range of its own and no storage
  name = "mixer legs, a small tick";
  s.assign(3, many_shape(160, 0));
  for (ManyShape &leg : s) leg.leg = true, leg.pass_in = true, leg.image_in = 640, leg.image_out = 3840;
  s[1].pass_in = false;  // (an F32 leg: its storage is its input image)
  s[2].key.zero = true;  // (the zero fallback: a launch of its own)
  {
    ManyExtra extra;
    extra.in_bytes = 3 * 64, extra.out_bytes = 5 * 960 * 2;
    p = plan_many_unit(s.data(), s.size(), no_pipeline, extra);
    MANY_EXPECT(p.small && !p.pipelined && !p.wait.sync && (launches_of(p) == Launches{{0, 1}, {2}}));
    MANY_EXPECT(p.e[0].in == B && p.e[0].out == N && p.e[0].in_off == 192 && p.e[1].in_off == 192 + 192 && p.e[2].in_off == 192 + 384);
    MANY_EXPECT(p.e[0].img_out == 0 && p.e[1].img_out == 3840 && p.e[2].img_out == 7680 && p.images_out == 3 * 3840 && p.dev_img_out == 3 * 3840 + 256);
    MANY_EXPECT(p.e[1].img_in == 640 && p.e[2].img_in == 640 && p.images_in == 1280);
    MANY_EXPECT(p.gathered_in == 192 + 3 * 192 && p.pin_in == p.gathered_in && p.dev_in == 0);
    MANY_EXPECT(p.gathered_out == 9600 && p.pin_out == 9600 + 128 && p.dev_out == 0 && p.total_out == 9600);
    (*rows)++;
    name = "mixer legs, buses too large for the pinned stage alone";
    extra.out_bytes = 1 * MB;
    p = plan_many_unit(s.data(), s.size(), no_pipeline, extra);
    MANY_EXPECT(!p.small && !p.pipelined && p.wait.sync && p.e[0].in == S && p.e[0].out == N && p.e[0].in_off == 192);
    MANY_EXPECT(p.gathered_in == 192 + 3 * 192 && p.dev_in == p.gathered_in && p.pin_in == p.gathered_in);
    MANY_EXPECT(p.gathered_out == 1 * MB && p.dev_out == 1 * MB && p.pin_out == 1 * MB + 128);
    (*rows)++;
    name = "mixer legs, a payload that travels on its own";
    s[0].in_bytes = Dc;
    p = plan_many_unit(s.data(), s.size(), no_pipeline, extra);
    MANY_EXPECT(!p.small && !p.pipelined && p.e[0].in == C && p.e[1].in == S && p.e[1].in_off == 192 && p.e[0].in_off == p.gathered_in);
    MANY_EXPECT(p.gathered_in == 192 + 2 * 192 && p.dev_in == p.gathered_in + Dc);
    (*rows)++;
  }
  {
    const ManyKey zero_last[] = {{10, 0, true, true, false}, {10, 0, true, true, true}, {10, 1, false, false, false}};
    for (size_t a = 0; a < 3; a++)
      for (size_t b = 0; b < 3; b++) MANY_EXPECT((zero_last[a] < zero_last[b]) == (a < b));
  }
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

// ---- the route of a formatted call (sides_route.h: route_sides_call -- the function formats.cpp, many.cpp and bus.cpp call) ----
// The rows were read off the commit before the rule existed ("Mix buses: weighted sums of a batch's streams in one device
// call"): csrc/formats.cpp, many.cpp and bus.cpp; each cites the lines it was read from.
struct RouteRow {
  const char *name;  // (with the lines it was read from)
  SidesForm form;
  SideKind in, out;
  SidesState st;
  int refuse;
  bool late;
  SidesRoute::Kind kind;
  bool direct, pass_in, pass_out;
  SidesRoute::Finish finish;
  float scale;
  bool dither, meter, gain, fusable;  // moves_dither, counts_meter, moves_gain, fusable
};
bool check_sides_routes(long *rows, long *walked) {
  const int S16 = SPEEXHIP_FMT_S16, F32 = SPEEXHIP_FMT_F32, F32N = SPEEXHIP_FMT_F32N, S24 = SPEEXHIP_FMT_S24, U8 = SPEEXHIP_FMT_U8;
  const int OK = SPEEXHIP_ERR_SUCCESS, BAD = SPEEXHIP_ERR_BAD_STATE, ARG = SPEEXHIP_ERR_INVALID_ARG;
  const auto flat = [](int fmt) { return SideKind{fmt, false, false, false}; };
  const auto mix = [](int fmt) { return SideKind{fmt, true, false, false}; };
  const auto planar = [](int fmt) { return SideKind{fmt, false, true, false}; };
  const auto ptrs = [](int fmt) { return SideKind{fmt, false, false, true}; };  // a mono side given as its one plane
  // the state flags: dither, meter, gain, split, zero_mode, single_stream, repeated
  const SidesState one = {false, false, false, false, false, true, false}, batch = {false, false, false, false, false, false, false};
  const auto with = [](SidesState s, const char *flags) {
    for (const char *f = flags; *f != 0; f++) {
      if (*f == 'd') s.dither = true;
      if (*f == 'm') s.meter = true;
      if (*f == 'g') s.gain = true;
      if (*f == 's') s.split = true;
      if (*f == 'z') s.zero_mode = true;
      if (*f == 'r') s.repeated = true;
    }
    return s;
  };
  const SidesForm Dev = SidesForm::Device, Host = SidesForm::Host, Planes = SidesForm::PlanesHost, Chunks = SidesForm::Chunks,
                  Many = SidesForm::ManyEntry, Bus = SidesForm::Bus, Leg = SidesForm::MixerLeg;
  const SidesRoute::Kind I16 = SidesRoute::Int16Call, Flt = SidesRoute::FloatCall, PFl = SidesRoute::PlanarFloatCall,
                         Img = SidesRoute::Images, Own = SidesRoute::OwnCalls;
  const SidesRoute::Finish None = SidesRoute::Nothing, MeterI = SidesRoute::MeterImage, GainI = SidesRoute::GainImage;
  const bool n = false, y = true;
  const RouteRow table[] = {
      // ---- Device: formats.cpp, process_sides_device
      {"device s16 same, :104-116", Dev, flat(S16), flat(S16), batch, OK, n, I16, n, n, n, None, 1, n, n, n, n},
      {"device f32 same, :104-116", Dev, flat(F32), flat(F32), batch, OK, n, Flt, n, n, n, None, 1, n, n, n, n},
      {"device f32 same dithered still counts, :114", Dev, flat(F32), flat(F32), with(batch, "d"), OK, n, Flt, n, n, n, None, 1, y, n, n, n},
      {"device s16 dithered is images, :25-28, :134-135", Dev, flat(S16), flat(S16), with(batch, "d"), OK, n, Img, n, y, y, None, 1, y, n, n, n},
      {"device s16 metered is images, :95, :104", Dev, flat(S16), flat(S16), with(batch, "m"), OK, n, Img, n, y, y, None, 1, n, y, n, n},
      {"device s16 gained is images, :95, :104", Dev, flat(S16), flat(S16), with(batch, "g"), OK, n, Img, n, y, y, None, 1, n, n, y, n},
      {"device f32n same metered, :108-113", Dev, flat(F32N), flat(F32N), with(batch, "m"), OK, n, Flt, n, n, n, MeterI, 32768, n, y, n, n},
      {"device f32 same gained, :108-113", Dev, flat(F32), flat(F32), with(batch, "g"), OK, n, Flt, n, n, n, GainI, 1, n, n, y, n},
      {"device f32n same gained metered dithered, :108-114", Dev, flat(F32N), flat(F32N), with(batch, "dmg"), OK, n, Flt, n, n, n, GainI, 32768, y, y, y, n},
      {"device s16 to f32 metered: meter_image, :134-135, :167-170", Dev, flat(S16), flat(F32), with(batch, "m"), OK, n, Img, n, y, n, MeterI, 1, n, y, n, n},
      {"device s16 to f32 gained: gain_image, :167-173", Dev, flat(S16), flat(F32), with(batch, "g"), OK, n, Img, n, y, n, GainI, 1, n, n, y, n},
      {"device f32 to s16, :134-135", Dev, flat(F32), flat(S16), batch, OK, n, Img, n, n, y, None, 1, n, n, n, n},
      {"device f32 to f32n, :134-135", Dev, flat(F32), flat(F32N), batch, OK, n, Img, n, n, y, None, 1, n, n, n, n},
      {"device matrix in on f32, :26, :134", Dev, mix(F32), flat(F32), batch, OK, n, Img, n, y, n, None, 1, n, n, n, n},
      {"device matrix out on f32 metered, :135, :163", Dev, flat(F32), mix(F32), with(batch, "m"), OK, n, Img, n, n, y, None, 1, n, y, n, n},
      {"device planar f32 pair, :118-123", Dev, planar(F32), planar(F32), batch, OK, n, PFl, n, n, n, None, 1, n, n, n, n},
      {"device planar f32n pair dithered moves, :121", Dev, planar(F32N), planar(F32N), with(batch, "d"), OK, n, PFl, n, n, n, None, 1, y, n, n, n},
      {"device planar f32 pair metered: passes, :117-118", Dev, planar(F32), planar(F32), with(batch, "m"), OK, n, Img, n, y, y, None, 1, n, y, n, n},
      {"device planar f32 pair gained: passes, :95, :118", Dev, planar(F32), planar(F32), with(batch, "g"), OK, n, Img, n, y, y, None, 1, n, n, y, n},
      {"device planar f32 pair split: passes, :118", Dev, planar(F32), planar(F32), with(one, "s"), OK, n, Img, n, y, y, None, 1, n, n, n, n},
      {"device planar s16 to f32n, :134-135", Dev, planar(S16), flat(F32N), batch, OK, n, Img, n, y, y, None, 1, n, n, n, n},
      {"device planar f32 to flat f32, :26, :134-135", Dev, planar(F32), flat(F32), batch, OK, n, Img, n, y, n, None, 1, n, n, n, n},
      {"device split one stream, :97-103, :156-157", Dev, flat(S16), flat(F32), with(one, "s"), OK, n, Img, n, y, n, None, 1, n, n, n, n},
      {"device split same bytes, :101-107", Dev, flat(S16), flat(S16), with(one, "s"), OK, n, I16, n, n, n, None, 1, n, n, n, n},
      {"device split of a batch, :101", Dev, flat(S16), flat(F32), with(batch, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"device split dithered, :101", Dev, flat(S16), flat(F32), with(one, "sd"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"device split matrix, :101", Dev, mix(S16), flat(F32), with(one, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"device split metered, :101", Dev, flat(F32), flat(F32), with(one, "sm"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"device split gained, :95, :101", Dev, flat(F32), flat(F32), with(one, "sg"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      // ---- Host: formats.cpp, process_sides_host
      {"host s16 same: process_host, :237-241", Host, flat(S16), flat(S16), one, OK, n, I16, y, n, n, None, 1, n, n, n, n},
      {"host f32n same dithered: process_host, moves, :237-239", Host, flat(F32N), flat(F32N), with(one, "d"), OK, n, Flt, y, n, n, None, 1, y, n, n, n},
      {"host same, split: process_host serves it, :234, :237", Host, flat(F32), flat(F32), with(one, "s"), OK, n, Flt, y, n, n, None, 1, n, n, n, n},
      {"host f32 same metered goes on, :235-237, :108-113", Host, flat(F32), flat(F32), with(one, "m"), OK, n, Flt, n, n, n, MeterI, 1, n, y, n, n},
      {"host f32n same gained goes on, :235-237, :108-113", Host, flat(F32N), flat(F32N), with(one, "g"), OK, n, Flt, n, n, n, GainI, 32768, n, n, y, n},
      {"host s16 dithered: images, :237, :134-135", Host, flat(S16), flat(S16), with(one, "d"), OK, n, Img, n, y, y, None, 1, y, n, n, n},
      {"host s16 to f32, :260", Host, flat(S16), flat(F32), one, OK, n, Img, n, y, n, None, 1, n, n, n, n},
      {"host split served, :250-262", Host, flat(S16), flat(F32), with(one, "s"), OK, n, Img, n, y, n, None, 1, n, n, n, n},
      {"host split dithered, no matrix: early, :234", Host, flat(S16), flat(S16), with(one, "sd"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"host split metered same bytes: early, :234", Host, flat(F32), flat(F32), with(one, "sm"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"host split gained: early, :234", Host, flat(S16), flat(F32), with(one, "sg"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"host split matrix: late, :242-243", Host, mix(S16), flat(F32), with(one, "s"), BAD, y, Img, n, n, n, None, 1, n, n, n, n},
      {"host split matrix dithered: late, :234, :243", Host, flat(S16), mix(S16), with(one, "sd"), BAD, y, Img, n, n, n, None, 1, n, n, n, n},
      {"host planar side: planes_host_call, :221, :474-475", Host, planar(S16), flat(F32N), with(one, "s"), OK, n, Img, n, y, y, None, 1, n, n, n, n},
      // ---- PlanesHost: formats.cpp, planes_host_call
      {"planes planar f32 pair, :519, :118", Planes, planar(F32), planar(F32), one, OK, n, PFl, n, n, n, None, 1, n, n, n, n},
      {"planes s16 to planar f32 metered, :519, :163", Planes, flat(S16), planar(F32), with(one, "m"), OK, n, Img, n, y, y, None, 1, n, y, n, n},
      {"planes split dithered, :475", Planes, planar(S16), flat(S16), with(one, "sd"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"planes split matrix: not late, :475", Planes, planar(S16), mix(S16), with(one, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"planes split metered, :475", Planes, planar(F32), planar(F32), with(one, "sm"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"planes split gained, :475", Planes, planar(F32), planar(F32), with(one, "sg"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      // ---- Chunks: formats.cpp, process_sides_host_chunks
      {"chunks s16 same: process_host_chunks, :376-384", Chunks, flat(S16), flat(S16), one, OK, n, I16, y, n, n, None, 1, n, n, n, y},
      {"chunks f32 same dithered, :376-381", Chunks, flat(F32), flat(F32), with(one, "d"), OK, n, Flt, y, n, n, None, 1, y, n, n, y},
      {"chunks same, split: process_host_chunks all the same, :352, :376, :382", Chunks, flat(F32), flat(F32), with(one, "s"), OK, n, Flt, y, n, n, None, 1, n, n, n, n},
      {"chunks same, zero mode, :350, :382", Chunks, flat(S16), flat(S16), with(one, "z"), OK, n, I16, y, n, n, None, 1, n, n, n, n},
      {"chunks not same, split: own calls, :352-374", Chunks, flat(S16), flat(F32), with(one, "s"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"chunks not same, zero mode dithered: own calls, :350-352", Chunks, flat(S16), flat(S16), with(one, "zd"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"chunks same metered, zero mode: own calls, :352", Chunks, flat(F32), flat(F32), with(one, "zm"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"chunks same gained, zero mode: own calls, :345, :352", Chunks, flat(F32N), flat(F32N), with(one, "zg"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"chunks f32n same metered: staged, no passes, :414-415, :443-447", Chunks, flat(F32N), flat(F32N), with(one, "m"), OK, n, Flt, n, n, n, MeterI, 32768, n, y, n, y},
      {"chunks f32 same gained dithered, :443-449", Chunks, flat(F32), flat(F32), with(one, "gd"), OK, n, Flt, n, n, n, GainI, 1, y, n, y, y},
      {"chunks s16 to f32 metered, :414-415, :443-444", Chunks, flat(S16), flat(F32), with(one, "m"), OK, n, Img, n, y, n, MeterI, 1, n, y, n, y},
      {"chunks s24 to u8 dithered, :414-415, :449", Chunks, flat(S24), flat(U8), with(one, "d"), OK, n, Img, n, y, y, None, 1, y, n, n, y},
      {"chunks planar f32 pair: passes, no planar float call, :350, :414-415", Chunks, planar(F32), planar(F32), one, OK, n, Img, n, y, y, None, 1, n, n, n, y},
      {"chunks matrix out, :415", Chunks, flat(F32), mix(F32), one, OK, n, Img, n, n, y, None, 1, n, n, n, y},
      {"chunks split dithered, :346", Chunks, flat(F32), flat(F32), with(one, "sd"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"chunks split matrix, :346", Chunks, mix(S16), flat(S16), with(one, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"chunks split gained, :345-346", Chunks, flat(F32), flat(F32), with(one, "sg"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      // ---- ManyEntry: formats.cpp, process_host_many_sides; many.cpp
      {"many s16 same: int16, formats :207-208", Many, flat(S16), flat(S16), one, OK, n, I16, n, n, n, None, 1, n, n, n, y},
      {"many f32n same: float, formats :207-209", Many, flat(F32N), flat(F32N), one, OK, n, Flt, n, n, n, None, 1, n, n, n, y},
      {"many f32 same dithered moves, many :231", Many, flat(F32), flat(F32), with(one, "d"), OK, n, Flt, n, n, n, None, 1, y, n, n, y},
      {"many s16 dithered: image, formats :207, many :170-171", Many, flat(S16), flat(S16), with(one, "d"), OK, n, Img, n, y, y, None, 1, y, n, n, y},
      {"many s16 metered: image, formats :207, many :233, :294", Many, flat(S16), flat(S16), with(one, "m"), OK, n, Img, n, y, y, None, 1, n, y, n, y},
      {"many s16 to f32: image, many :170-171", Many, flat(S16), flat(F32), one, OK, n, Img, n, y, n, None, 1, n, n, n, y},
      {"many f32 to s24 gained stays fused, many :295", Many, flat(F32), flat(S24), with(one, "g"), OK, n, Img, n, n, y, None, 1, n, n, y, y},
      {"many f32 same gained stays fused: gain_image, formats :206, many :297-304", Many, flat(F32), flat(F32), with(one, "g"), OK, n, Flt, n, n, n, GainI, 1, n, n, y, y},
      {"many f32n same gained: gain_image at 1, many :322", Many, flat(F32N), flat(F32N), with(one, "g"), OK, n, Flt, n, n, n, GainI, 1, n, n, y, y},
      {"many s16 to f32 gained: gain_image, many :297", Many, flat(S16), flat(F32), with(one, "g"), OK, n, Img, n, y, n, GainI, 1, n, n, y, y},
      {"many f32 to f32n metered stays fused, formats :201", Many, flat(F32), flat(F32N), with(one, "m"), OK, n, Img, n, n, y, None, 1, n, y, n, y},
      {"many f32 result metered: own call, formats :199-202", Many, flat(S16), flat(F32), with(one, "m"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many f32n same metered: own call, formats :201", Many, flat(F32N), flat(F32N), with(one, "mg"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many matrix: own call, formats :197", Many, mix(S16), flat(S16), one, OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many planar: own call, formats :197", Many, flat(S16), planar(S16), one, OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many planes pointer: own call, formats :197-198", Many, ptrs(S16), flat(S16), one, OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many named twice: own call, many :517-521", Many, flat(S16), flat(S16), with(one, "r"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many split: own call, many :521", Many, flat(S16), flat(S16), with(one, "s"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many zero mode: own call, many :521", Many, flat(F32), flat(F32), with(one, "z"), OK, n, Own, n, n, n, None, 1, n, n, n, n},
      {"many batch of several: own call, many :521", Many, flat(F32), flat(F32), batch, OK, n, Own, n, n, n, None, 1, n, n, n, n},
      // ---- Bus: bus.cpp, process_bus_device
      {"bus f32 to f32: no same-bytes route, :139-142", Bus, flat(F32), flat(F32), batch, OK, n, Img, n, n, n, None, 1, n, n, n, n},
      {"bus planar f32 pair: no planar float route, :141-142", Bus, planar(F32), planar(F32), batch, OK, n, Img, n, y, y, None, 1, n, n, n, n},
      {"bus s16 to s16 dithered: the bus position, :182, :199", Bus, flat(S16), flat(S16), with(batch, "d"), OK, n, Img, n, y, y, None, 1, y, n, n, n},
      {"bus f32 side metered: meter_image, :184-197", Bus, flat(S16), flat(F32), with(batch, "m"), OK, n, Img, n, y, n, MeterI, 1, n, y, n, n},
      {"bus f32 side gained: never gain_image, gain moves, :178-198", Bus, flat(S16), flat(F32), with(batch, "g"), OK, n, Img, n, y, n, None, 1, n, n, y, n},
      {"bus f32 side gained metered: meter_image only, :184, :196-198", Bus, mix(S16), flat(F32), with(batch, "gm"), OK, n, Img, n, y, n, MeterI, 1, n, y, y, n},
      {"bus f32n side metered: the pass, :142, :181-183", Bus, flat(F32), flat(F32N), with(batch, "m"), OK, n, Img, n, n, y, None, 1, n, y, n, n},
      {"bus matrix on the sum, :122", Bus, flat(S16), mix(S16), batch, ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"bus split, :129-131", Bus, flat(S16), flat(S16), with(one, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      // ---- MixerLeg: mixer.cpp, Mixer::process (written with the rule; `out` is the leg's float image)
      {"leg s16: the input pass, no output pass", Leg, flat(S16), flat(F32), one, OK, n, Img, n, y, n, None, 1, n, n, n, y},
      {"leg f32: no same-bytes route, no pass at all", Leg, flat(F32), flat(F32), one, OK, n, Img, n, n, n, None, 1, n, n, n, y},
      {"leg f32n: the input pass", Leg, flat(F32N), flat(F32), one, OK, n, Img, n, y, n, None, 1, n, n, n, y},
      {"leg gained: gain moves, never gain_image", Leg, flat(U8), flat(F32), with(one, "g"), OK, n, Img, n, y, n, None, 1, n, n, y, y},
      {"leg dithered metered gained: only gain moves", Leg, flat(S24), flat(F32), with(one, "dmg"), OK, n, Img, n, y, n, None, 1, n, n, y, y},
      {"leg in the zero fallback joins its group", Leg, flat(S16), flat(F32), with(one, "zg"), OK, n, Img, n, y, n, None, 1, n, n, y, y},
      {"leg matrix", Leg, mix(S16), flat(F32), one, ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg planar of several channels", Leg, planar(S16), flat(F32), one, ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg plane pointers", Leg, ptrs(S16), flat(F32), one, ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg of a batch of several streams", Leg, flat(S16), flat(F32), batch, ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg named by an earlier slot", Leg, flat(S16), flat(F32), with(one, "r"), ARG, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg split", Leg, flat(S16), flat(F32), with(one, "s"), BAD, n, Img, n, n, n, None, 1, n, n, n, n},
      {"leg split and named twice: the argument error first", Leg, flat(S16), flat(F32), with(one, "sr"), ARG, n, Img, n, n, n, None, 1, n, n, n, n},
  };
  for (const RouteRow &w : table) {
    const SidesRoute r = route_sides_call(w.form, w.in, w.out, w.st);
    if (r.refuse != w.refuse || r.refuse_late != w.late || r.kind != w.kind || r.direct != w.direct || r.pass_in != w.pass_in ||
        r.pass_out != w.pass_out || r.finish != w.finish || r.finish_scale != w.scale || r.moves_dither != w.dither ||
        r.counts_meter != w.meter || r.moves_gain != w.gain || r.fusable != w.fusable) {
      printf("BAD sides route (%s): refuse %d late %d kind %d direct %d passes %d / %d finish %d at %g, moves %d %d %d, fusable %d\n", w.name,
             r.refuse, r.refuse_late, static_cast<int>(r.kind), r.direct, r.pass_in, r.pass_out, static_cast<int>(r.finish), r.finish_scale,
             r.moves_dither, r.counts_meter, r.moves_gain, r.fusable);
      return false;
    }
    (*rows)++;
  }
  // The whole input space: what holds of every route, whatever the table says.
  const int fmts[] = {SPEEXHIP_FMT_U8,   SPEEXHIP_FMT_S16,  SPEEXHIP_FMT_S24,   SPEEXHIP_FMT_S32,   SPEEXHIP_FMT_F32,   SPEEXHIP_FMT_F32N, SPEEXHIP_FMT_ULAW,
                      SPEEXHIP_FMT_ALAW, SPEEXHIP_FMT_F16N, SPEEXHIP_FMT_BF16N, SPEEXHIP_FMT_S16BE, SPEEXHIP_FMT_S24BE, SPEEXHIP_FMT_S32BE};
  const auto is_float = [](int fmt) { return fmt == SPEEXHIP_FMT_F32 || fmt == SPEEXHIP_FMT_F32N; };
#define ROUTE_EXPECT(cond)                                                                                                     \
  do {                                                                                                                         \
    if (!(cond)) {                                                                                                             \
      printf("BAD sides route: not %s (form %d, %d%s%s -> %d%s%s, state %x)\n", #cond, static_cast<int>(form), in.fmt,          \
             in.mix ? " mix" : "", in.planar ? " planar" : "", out.fmt, out.mix ? " mix" : "", out.planar ? " planar" : "", bits); \
      return false;                                                                                                            \
    }                                                                                                                          \
  } while (0)
  for (SidesForm form : {Dev, Host, Planes, Chunks, Many, Bus, Leg})
    for (int fi : fmts) for (int fo : fmts)
      for (int sides = 0; sides < 64; sides++)  // mix, planar, planes of either side
        for (int bits = 0; bits < 128; bits++) {
          if (form != Many && form != Leg && (sides & (4 | 32)) != 0) continue;  // (only the many-states and the mixer call ask for plane pointers)
          const SideKind in ={fi, (sides & 1) != 0, (sides & 2) != 0, (sides & 4) != 0};
          const SideKind out = {fo, (sides & 8) != 0, (sides & 16) != 0, (sides & 32) != 0};
          const SidesState st = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0};
          const SidesRoute r = route_sides_call(form, in, out, st);
          (*walked)++;
          const bool delegates = r.kind == SidesRoute::OwnCalls;  // (the next form down asks again)
          if (r.refuse != SPEEXHIP_ERR_SUCCESS || delegates) {
            // a refused route names no passes -- nor does one that hands the call on; neither moves anything
            ROUTE_EXPECT(!r.pass_in && !r.pass_out && r.finish == SidesRoute::Nothing && !r.direct && !r.fusable);
            ROUTE_EXPECT(!r.moves_dither && !r.counts_meter && !r.moves_gain);
            continue;
          }
          ROUTE_EXPECT(!r.refuse_late);
          if (form == Leg) {
            // a leg that runs: one interleaved buffer of a single-stream state; the float call into its image behind at most
            // an input pass -- never an output pass, never a finish: the bus-sum kernel reads the image and gains it; of
            // the state only the gain moves
            ROUTE_EXPECT(!in.mix && !in.planar && !in.planes && st.single_stream && !st.repeated && !st.split);
            ROUTE_EXPECT(r.kind == SidesRoute::Images && !r.pass_out && r.finish == SidesRoute::Nothing && !r.direct && r.fusable);
            ROUTE_EXPECT(r.pass_in == (fi != SPEEXHIP_FMT_F32));
            ROUTE_EXPECT(!r.moves_dither && !r.counts_meter && r.moves_gain == st.gain && r.finish_scale == 1.0f);
            continue;
          }
          if (r.kind == SidesRoute::Int16Call)
            ROUTE_EXPECT(fi == SPEEXHIP_FMT_S16 && fo == SPEEXHIP_FMT_S16 && !st.dither && !st.meter && !st.gain && !in.mix && !out.mix);
          if (r.kind != SidesRoute::Images) ROUTE_EXPECT(!r.pass_in && !r.pass_out);
          if (r.kind == SidesRoute::FloatCall) ROUTE_EXPECT(fi == fo && is_float(fi) && !in.mix && !out.mix && !in.planar && !out.planar);
          if (r.finish != SidesRoute::Nothing) ROUTE_EXPECT(!r.pass_out && is_float(fo));
          if (r.finish_scale != 1.0f) ROUTE_EXPECT(r.finish_scale == 32768.0f && r.finish != SidesRoute::Nothing && fi == SPEEXHIP_FMT_F32N && fo == fi && r.kind == SidesRoute::FloatCall);
          // pass_out and finish together cover every call with the meter on, and every one with gain on -- but a bus
          // call's, whose streams bus_sum gains before it sums them
          if (st.meter || (st.gain && form != Bus)) ROUTE_EXPECT(r.pass_out || r.finish != SidesRoute::Nothing);
          if (r.kind == SidesRoute::PlanarFloatCall) ROUTE_EXPECT(in.planar && out.planar && fi == fo && is_float(fi) && !in.mix && !out.mix);
          // whatever counts the meter or moves gain has an output pass or a finish (the bus call's gain as above)
          if (r.counts_meter || (r.moves_gain && form != Bus)) ROUTE_EXPECT(r.pass_out || r.finish != SidesRoute::Nothing);
          // ... and every call that is obeyed here moves exactly what the state has on; the host's own calls only the dither
          ROUTE_EXPECT(r.moves_dither == st.dither);
          if (!r.direct) ROUTE_EXPECT(r.counts_meter == st.meter && r.moves_gain == st.gain);
          if (r.direct) ROUTE_EXPECT((form == Host || form == Chunks) && !st.meter && !st.gain && r.kind != SidesRoute::Images && r.kind != SidesRoute::PlanarFloatCall);
          if (r.fusable) ROUTE_EXPECT(form == Chunks || form == Many);  // (and a mixer's leg, above)
          if (form == Many) ROUTE_EXPECT(r.fusable && !in.planar && !out.planar && !in.mix && !out.mix && !in.planes && !out.planes && r.finish != SidesRoute::MeterImage);
          if (form == Bus) ROUTE_EXPECT(r.kind == SidesRoute::Images && r.finish != SidesRoute::GainImage);
        }
#undef ROUTE_EXPECT
  return true;
}

// ---- a mixer leg's level (levels.h: the lines the kernel leg_levels and speexhip_debug_levels compile) ----------------------
// At its decision points against the step the header states, and over random floats -- every bit pattern, so NaNs of
// either sign, infinities and denormals among them -- against a reference in integers: the step through long double, the
// energy in uint64, the peak by comparing values.  Folded as the users fold: sample by sample (c_api.cpp) and a lane of
// 256 at a time (the kernel).
bool check_levels(std::mt19937 &rng, long *points, long *random) {
  struct Point {
    float y;
    int q;  // the step; 1 << 30: a NaN
  };
  const float inf = std::numeric_limits<float>::infinity();
  const Point at[] = {{0.5f, 1},          {-0.5f, 0},         {1.5f, 2},           {-1.5f, -1},   {0.49999997f, 0}, {-0.50000006f, -1},
                      {32766.5f, 32767},  {32767.5f, 32767},  {-32768.5f, -32768}, {inf, 32767},  {-inf, -32768},   {-0.0f, 0},
                      {1e30f, 32767},     {1e-42f, 0},        {-1e30f, -32768},    {32767.0f, 32767}, {-32768.0f, -32768},
                      {std::numeric_limits<float>::quiet_NaN(), 1 << 30}};
  for (const Point &p : at) {
    levels::Lane lane;
    levels::add(lane, p.y);
    SpeexHipLevel rec = {};
    levels::fold(rec, lane);
    const bool nan = p.q == 1 << 30;
    const uint64_t energy = nan ? 0 : static_cast<uint64_t>(static_cast<int64_t>(p.q) * p.q);
    const float peak = nan ? 0.0f : std::fabs(p.y);
    if (rec.energy != energy || rec.nan != (nan ? 1u : 0u) || rec.peak != peak || std::signbit(rec.peak) || rec.samples != 0 || rec.reserved != 0) {
      printf("BAD level at %a: energy %llu nan %llu peak %a\n", p.y, static_cast<unsigned long long>(rec.energy),
             static_cast<unsigned long long>(rec.nan), rec.peak);
      return false;
    }
    (*points)++;
  }
  for (int round = 0; round < 200; round++) {
    const uint32_t n = 1 + rng() % 3000;
    const int kind = round % 3;  // every bit pattern; audio around the rails; whispers around the ties
    SpeexHipLevel by_sample = {}, by_lane = {};
    uint64_t energy = 0, nans = 0;
    float peak = 0.0f;
    levels::Lane lane;
    uint32_t in_lane = 0;
    for (uint32_t i = 0; i < n; i++) {
      float y;
      if (kind == 0) {
        const uint32_t bits = rng();
        memcpy(&y, &bits, sizeof(y));
      } else {
        y = (static_cast<float>(rng()) / 4294967296.0f - 0.5f) * (kind == 1 ? 80000.0f : 6.0f);
        if (kind == 2 && rng() % 8 == 0) y = std::floor(y) + 0.5f;  // (an exact tie)
      }
      if (y != y) {
        nans++;
      } else {
        const long double r = std::floor(static_cast<long double>(y) + 0.5L);
        const int64_t q = r < -32768.0L ? -32768 : r > 32767.0L ? 32767 : static_cast<int64_t>(r);
        energy += static_cast<uint64_t>(q * q);
        if (std::fabs(y) > peak) peak = std::fabs(y);
      }
      levels::Lane one;
      levels::add(one, y);
      levels::fold(by_sample, one);
      levels::add(lane, y);
      if (++in_lane == 256 || i + 1 == n) {
        levels::fold(by_lane, lane);
        lane = levels::Lane();
        in_lane = 0;
      }
      (*random)++;
    }
    for (const SpeexHipLevel *rec : {&by_sample, &by_lane})
      if (rec->energy != energy || rec->nan != nans || rec->peak != peak) {
        printf("BAD level over %u random floats of kind %d: energy %llu (want %llu) nan %llu (%llu) peak %a (%a)\n", n, kind,
               static_cast<unsigned long long>(rec->energy), static_cast<unsigned long long>(energy),
               static_cast<unsigned long long>(rec->nan), static_cast<unsigned long long>(nans), rec->peak, peak);
        return false;
      }
  }
  // a lane at the limit of its chain: kLaneMost samples at the rail are 2^23 * 2^30 = 2^53, which fp64 still holds
  levels::Lane full;
  for (uint32_t i = 0; i < levels::kLaneMost; i++) levels::add(full, -40000.0f);
  SpeexHipLevel rec = {};
  levels::fold(rec, full);
  if (rec.energy != (1ull << 53) || rec.peak != 40000.0f) {
    printf("BAD level of a full lane: energy %llu\n", static_cast<unsigned long long>(rec.energy));
    return false;
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
  long sides_rows = 0, sides_walked = 0;
  if (!check_sides_routes(&sides_rows, &sides_walked)) return 1;
  long level_points = 0, level_random = 0;
  if (!check_levels(rng, &level_points, &level_random)) return 1;
  printf("sanitizer run ok: %ld filters, %ld plans, %ld placements, %ld routes, %ld many-states rows, %ld random many-states units, "
         "%ld sides routes, %ld walked, %ld level points, %ld random level samples\n",
         filters, plans, placements, routes, many_rows, many_random, sides_rows, sides_walked, level_points, level_random);
  return 0;
}
