"""Which code a configuration runs, read from the host planner alone -- and the short list of configurations that,
with the curated *_CASES lists of test_gpu_parity.py, meets every plan feature the rate grid reaches.

The FIR kernels are judged per sample against tests/exact_model.py on hand-picked (channels, in, out, quality) tuples.
Which kernel instance a tuple runs is the host planner's choice (plan_period*, plan_slide*, period_view,
launch_period_plan): it keys on the kernel kind, the channel layout, the phases per wave and whether den leaves a
short last phase group, the bank padding, the fine plan, the int16 window, the folded view, the slide shape and
whether an fp64 twin exists.  features() names those choices as pairs; universe() is their union over the grid
RATES x RATES x QUALITIES x CHANNELS; curated() is what the hand-picked lists hold; choose() is a deterministic greedy
cover of the rest, committed as tests/plan_cover_cases.json (python tests/plan_cover.py writes it) and run on the GPU by
tests/test_gpu_plan_cover.py.  tests/test_cpu_plan_cover.py proves without a GPU that the list still covers the
universe.  Nothing here needs a GPU: speexhip.design_filter, debug_plan, debug_plan64 and debug_launch_shape are host
code.

Pairs (tuples; the first element names the family):
  period (fast_path 2), for each feature F of
        ("kind", kernel) ("r", r) ("pad", pad != 0) ("fine", fine_plan) ("w16", w16_lane_periods != 0)
        ("fold", den <= 6) ("ragged", r, den' % r) ("p64", debug_plan64's fast_path) ("one_period_tile", lane_periods == 1)
        ("rowpar", row_len % 2)                         [den' = the den the plan sees: k den on a folded view]
      ("period", class) + F, and ("period", kind) + F for every F but kind;
  slide (fast_path 3), with shape = (num, den, periods per lane, tap steps per iteration):
      ("slide", shape, "1" | "2" | "even" | "odd" channels), ("slide", shape, "fp64" | "fp32"), ("slide", kind, class);
  exact (fast_path 0): ("exact", kind, class);
  launch: debug_launch_shape for an int16 and a float call of F frames on S streams gives
        ("launch_r", r, den' % r) ("w16", int16_window) ("pp", phase_pairs) ("splits", min(splits, 3)) ("touch", touch)
      each as ("launch", class) + F.  One-state cases are probed at (1, frames_for(case)), batches at BATCH_PROBE.
class: "1", "2", "odd" (3, 5, 7), "isa" (4, 6, 8, 10, 12, 16), "gen" (the rest).
"""
import ast
import json
import os
import sys
from math import gcd

if __name__ == "__main__":      # as a script: the paths tests/conftest.py gives the tests
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "oracle"), os.path.join(_root, "node-speex-resampler_amd", "python")]

import speexhip

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_FILE = os.path.join(HERE, "plan_cover_cases.json")

# the 20 rates of test_cpu_host_logic.test_planner_invariants_over_rates_qualities_and_channel_counts
RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 40000, 44100, 48000, 56000, 64000, 72000, 80000,
         88200, 96000, 128000, 160000, 176400, 192000]
QUALITIES = tuple(range(11))
CHANNELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)
KINDS = ("direct_single", "direct_double", "interpolate_single", "interpolate_double")

MAX_CASES = 160
FRAME_CAP = 120000
BATCH_PROBE = (32, 65536)           # streams x frames of the launches no one-state call reaches
# the one-state schedule of a cover case (test_gpu_exact_model._one_state): calls of these sizes, call 3 capacity-bound
BOUND_CALL, SEED = 3, 40
EXACT_SEED = 77
# the long calls of the curated lists' own exact-model tests (test_gpu_exact_model.py), for their launch pairs
CURATED_LONG_CALL = {"LAYOUT_CASES": 30011, "PERIOD64_CASES": 30011, "FOLDED_CASES": 50011}
DEFAULT_LONG_CALL = 21011


def first_call(num, den):
    """Frames of a cover case's first call: three, or the next of 2, 4, 5, 7 where three leave the stream on phase 0
    again (3:n and 4:3 do), so that the long call starts between two input frames.  (1:n and n:1 ratios are on phase 0
    after any whole number of frames.)"""
    for n in (3, 2, 4, 5, 7):
        if -(-n * den // num) * num % den:
            return n
    return 3


def sizes_of(num, den, frames):
    """a cover case's calls: a few frames, the long call, an empty one, a capacity-bound one"""
    return (first_call(num, den), frames, 0, frames // 3)


def exact_sizes_of(frames):
    return (1, frames // 3, 0, frames - frames // 3)


def channel_class(ch):
    if ch in (1, 2):
        return str(ch)
    if ch in (3, 5, 7):
        return "odd"
    return "isa" if ch in (4, 6, 8, 10, 12, 16) else "gen"


def _parity(ch):
    return str(ch) if ch in (1, 2) else "odd" if ch % 2 else "even"


_DESIGN, _PLAN, _SHAPE = {}, {}, {}


def design(i, o, q):
    """-> {"num", "den", "taps", "kind"} or None where the library refuses the filter.  (The filter is a function of the
    reduced ratio alone: memoised on it.)"""
    g = gcd(i, o)
    key = (i // g, o // g, q)
    if key not in _DESIGN:
        try:
            info, _ = speexhip.design_filter(key[0], key[1], q, want_table=False)
        except ValueError:
            _DESIGN[key] = None
        else:
            assert (info["num_rate"], info["den_rate"]) == key[:2], (key, info)
            _DESIGN[key] = {"num": key[0], "den": key[1], "taps": info["filt_len"], "kind": KINDS[info["kernel"]]}
    return _DESIGN[key]


def plans(ch, i, o, q):
    """-> (design, debug_plan, debug_plan64) or None"""
    d = design(i, o, q)
    if d is None:
        return None
    key = (ch, d["num"], d["den"], q)
    if key not in _PLAN:
        _PLAN[key] = (speexhip.debug_plan(d["num"], d["den"], q, ch), speexhip.debug_plan64(d["num"], d["den"], q, ch))
    return (d,) + _PLAN[key]


def view_den(d, plan):
    """the den a period plan sees: period_view folds den <= 6 to k den, k = 5 (10 for den = 1)"""
    if plan["fast_path"] != 2 or d["den"] > 6:
        return d["den"]
    return d["den"] * (10 if d["den"] == 1 else 5)


def info_fast_path(plan, plan64):
    """fast_path as Resampler.info() reports it in the default mode"""
    return plan64["fast_path"] if plan64["fast_path"] in (4, 5) else plan["fast_path"]


def launch_shape(ch, d, q, streams, frames, float_io):
    key = (ch, d["num"], d["den"], q, streams, frames, float_io)
    if key not in _SHAPE:
        _SHAPE[key] = speexhip.debug_launch_shape(d["num"], d["den"], q, ch, streams, frames, float_io)
    return _SHAPE[key]


def plan_features(ch, i, o, q):
    """the pairs the plan alone decides (no launch) -> set, or None where the library refuses the filter"""
    got = plans(ch, i, o, q)
    if got is None:
        return None
    d, plan, plan64 = got
    cls, kind = channel_class(ch), d["kind"]
    if plan["fast_path"] == 2:
        r, den = plan["r_or_p"], view_den(d, plan)
        feats = [("kind", kind), ("r", r), ("pad", plan["pad"] != 0), ("fine", plan["fine_plan"]),
                 ("w16", plan["w16_lane_periods"] != 0), ("fold", d["den"] <= 6), ("ragged", r, den % r),
                 ("p64", plan64["fast_path"]), ("one_period_tile", plan["lane_periods"] == 1),
                 ("rowpar", plan["row_len"] % 2)]
        return {("period", cls) + f for f in feats} | {("period", kind) + f for f in feats if f[0] != "kind"}
    if plan["fast_path"] == 3:
        shape = (d["num"], d["den"], plan["r_or_p"], plan["steps_per_iteration"])
        return {("slide",) + shape + (_parity(ch),), ("slide",) + shape + ("fp64" if plan64["fast_path"] == 4 else "fp32",),
                ("slide", kind, cls)}
    assert plan["fast_path"] == 0, plan
    return {("exact", kind, cls)}


def launch_features(ch, i, o, q, streams, frames):
    """the pairs of an int16 and a float launch of `frames` frames on each of `streams` streams (period kernel on the
    single kinds: debug_launch_shape models no other launch)"""
    d, plan, _ = plans(ch, i, o, q)
    out = set()
    if plan["fast_path"] != 2:
        return out
    cls, den = channel_class(ch), view_den(d, plan)
    for float_io in (False, True):
        s = launch_shape(ch, d, q, streams, frames, float_io)
        if not s["r"]:
            continue
        for f in (("launch_r", s["r"], den % s["r"]), ("w16", s["int16_window"]), ("pp", s["phase_pairs"]),
                  ("splits", min(s["splits"], 3)), ("touch", s["touch"])):
            out.add(("launch", cls) + f)
    return out


def tile_periods(ch, i, o, q):
    """the most periods a tile of this period case holds, over the plans its int16 and float calls may take"""
    d, plan, plan64 = plans(ch, i, o, q)
    lp = [plan["lane_periods"], plan["w16_lane_periods"]]
    if plan64["fast_path"] in (5, 6):
        lp += [plan64["lane_periods"], plan64["last"]]
    return max(lp)


def tiles_of(ch, i, o, q, frames):
    """the fewest tiles a first call of `frames` frames has, over its int16 and its float launch: debug_launch_shape's
    where it models the launch, else ceil(periods / periods per tile) as launch_period_plan counts them"""
    d, plan, plan64 = plans(ch, i, o, q)
    counts = [s["tiles"] for s in (launch_shape(ch, d, q, 1, frames, fl) for fl in (False, True)) if s["r"]]
    if not counts:
        periods = -(-(frames * d["den"] // d["num"]) // view_den(d, plan))
        counts = [-(-periods // tile_periods(ch, i, o, q))]
    return min(counts)


def min_outputs(ch, i, o, q):
    """outputs after which every phase index of a period case has fallen in two tiles"""
    d, plan, _ = plans(ch, i, o, q)
    den = view_den(d, plan)
    return 2 * tile_periods(ch, i, o, q) * den + den


def frames_for(ch, i, o, q):
    """The long call of a cover case.  Period cases: the smallest F = 1000 k + 11 with F > 2 taps + 64, at least 3 tiles
    and min_outputs() outputs, at most FRAME_CAP.  Slide and exact cases: max(21011, 3 taps + 75)."""
    d, plan, _ = plans(ch, i, o, q)
    if plan["fast_path"] != 2:
        return max(21011, 3 * d["taps"] + 75)

    def ok(k):
        f = 1000 * k + 11
        return (f > 2 * d["taps"] + 64 and tiles_of(ch, i, o, q, f) >= 3 and
                f * d["den"] // d["num"] >= min_outputs(ch, i, o, q))
    # (from the first size the two arithmetic conditions allow, upwards: the tiles need not grow with the frames -- a
    #  longer launch may take the int16 window, whose tiles hold more periods)
    need = max(2 * d["taps"] + 65, -(-min_outputs(ch, i, o, q) * d["num"] // d["den"]))
    last = (FRAME_CAP - 11) // 1000
    for k in range(max(1, -(-(need - 11) // 1000)), last):
        if ok(k):
            return 1000 * k + 11
    return 1000 * last + 11


def features(ch, i, o, q):
    """every pair a one-state cover case of this configuration meets, or None where the library refuses the filter"""
    f = plan_features(ch, i, o, q)
    if f is None:
        return None
    return f | launch_features(ch, i, o, q, 1, frames_for(ch, i, o, q))


def batch_features(ch, i, o, q):
    return launch_features(ch, i, o, q, *BATCH_PROBE)


def grid():
    """one configuration per (reduced ratio, quality, channels) the grid holds, in grid order: the plan is a function
    of the reduced ratio, so 48000 -> 16000 stands for 24000 -> 8000 and 96000 -> 32000 too"""
    seen = set()
    for i in RATES:
        for o in RATES:
            g = gcd(i, o)
            if (i // g, o // g) in seen:
                continue
            seen.add((i // g, o // g))
            for q in QUALITIES:
                if design(i, o, q) is None:
                    continue
                for ch in CHANNELS:
                    yield (ch, i, o, q)


_UNIVERSE = {}


def universe():
    """-> {"one": pairs one-state cases reach, "batch": launch pairs only a BATCH_PROBE launch reaches}"""
    if not _UNIVERSE:
        one, batch = set(), set()
        for c in grid():
            one |= features(*c)
            batch |= batch_features(*c)
        _UNIVERSE.update(one=one, batch=batch - one)
    return _UNIVERSE


def _module_lists(filename, pick):
    """{name: value} of the module-level list assignments of tests/<filename> whose name `pick` accepts, read with ast
    (importing the GPU test modules needs a GPU)"""
    with open(os.path.join(HERE, filename)) as f:
        tree = ast.parse(f.read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and pick(node.targets[0].id):
            out[node.targets[0].id] = ast.literal_eval(node.value)
    return out


def curated_cases():
    """{list name: [(ch, in, out, quality), ...]} of test_gpu_parity.py's *_CASES lists"""
    lists = _module_lists("test_gpu_parity.py", lambda n: n.endswith("_CASES"))
    return {name: [tuple(t[:4]) for t in v] for name, v in lists.items()}


def curated_batches():
    """(ch, in, out, quality, streams, frames) of the batch lists of test_gpu_exact_model.py"""
    lists = _module_lists("test_gpu_exact_model.py", lambda n: n in ("BATCHES", "PHASE_PAIR_BATCHES"))
    return [tuple(t[:6]) for name in sorted(lists) for t in lists[name]]


def curated():
    """the pairs the curated lists hold: the plan pairs of every tuple, the launch pairs of its own long call, and the
    launch pairs of the batches"""
    got = set()
    for name, cases in sorted(curated_cases().items()):
        for c in cases:
            f = plan_features(*c)
            if f is not None:
                got |= f | launch_features(*c, 1, CURATED_LONG_CALL.get(name, DEFAULT_LONG_CALL))
    for (ch, i, o, q, streams, frames) in curated_batches():
        # (a batch of more than 32 streams runs in launches of 32)
        got |= plan_features(ch, i, o, q) | launch_features(ch, i, o, q, min(streams, 32), frames)
    return got


def _cost(c):
    d = design(*c[1:])
    return d["taps"] * max(d["num"], d["den"]) * c[0]


def oracle_stream(c, frames, kind, exact=False):
    """the oracle over the schedule tests/test_gpu_plan_cover.py runs for a one-state case (kind "int16" or "float";
    exact: the exact-kernel cases' schedule) -> (outputs, the input the stream has read)"""
    import numpy as np

    import exact_model as em
    import oracle as orc
    ch, i, o, q = c
    ref = orc.Oracle(ch, i, o, q)
    sizes = exact_sizes_of(frames) if exact else sizes_of(ref.num, ref.den, frames)
    got, fed = [], []
    for call, n in enumerate(sizes):
        if exact:
            x, cap = em.samples(n, ch, EXACT_SEED + call, ref.taps), 1 << 20
        else:
            x = em.samples(n, ch, SEED + 7 * call + ch, ref.taps, tone=call == 3)
            cap = max(1, n * o // i // 2) if call == BOUND_CALL else 1 << 20
        y, u = ref.process_float(x.astype(np.float32), cap) if kind == "float" else ref.process(x, cap)
        got.append(y), fed.append(x[: u + 1] if call == len(sizes) - 1 else x[:u])      # (as _one_state does)
    return np.concatenate(got), np.concatenate(fed)


_ORACLE = {}


def oracle_alone(c):
    """The oracle by itself on the case's own input: (a) on both streams and (c) wherever n >= 20 000, against the fp32
    bound (the reference's kernels round every product to fp32, the double ones too) -> (failures, stats).  The
    reference's interpolating kernels blend four SUMS, not the rows (exact_model.reference_abs_rows): on a short
    filter a sample or two in 100 000 may leave the bound over mag.  Such an input cannot tell the kernel's error from
    the reference's, and choose() passes the configuration over."""
    import numpy as np

    import exact_model as em
    if c not in _ORACLE:
        exact = plans(*c)[1]["fast_path"] == 0
        frames = frames_for(*c)
        model = em.Model(*c)
        gotf, fed = oracle_stream(c, frames, "float", exact)
        got16, fed16 = oracle_stream(c, frames, "int16", exact)
        assert np.array_equal(fed, fed16) and got16.shape == gotf.shape and gotf.shape[0] > 0
        assert np.any(np.all(fed[:frames] == 0, axis=1)), "no silence in the long call"
        truth, mag = model.truth(fed, gotf.shape[0])
        fails, stats = em.judge_float(model, fed, gotf, truth, mag, 32, None, tile=model.num)
        fails += ["int16 (a) " + m for m in em.hard_int16(model, fed, got16, truth, mag, 32, tile=model.num)]
        _ORACLE[c] = (fails, stats)
    return _ORACLE[c]


def _greedy(todo, candidates, accept=None):
    """([(case, pairs it is there for)], [cases passed over]): the case that holds most of what is left, ties to the
    smaller filter, then to the smaller tuple; one that `accept` turns down is passed over for good"""
    todo, picked, passed = set(todo), [], []
    live = {c: f & todo for c, f in candidates.items() if f & todo}
    while todo:
        best = min(live, key=lambda c: (-len(live[c]), _cost(c), c))
        if accept is not None and not accept(best):
            passed.append(best)
            del live[best]
            continue
        gain = live[best]
        picked.append((best, sorted(gain, key=repr)))
        todo -= gain
        live = {c: f - gain for c, f in live.items() if f - gain}
    return picked, passed


def choose():
    """the committed file's content: a greedy cover of universe() - curated() by one-state cases on whose input the
    oracle itself passes, then of the launch pairs that are left by BATCH_PROBE launches"""
    u, have = universe(), curated()
    cases = []
    picked, passed = _greedy(u["one"] - have, {c: features(*c) for c in grid()}, lambda c: not oracle_alone(c)[0])
    for c, pairs in picked:
        d, plan, plan64 = plans(*c)
        e = {"case": list(c), "fast_path": info_fast_path(plan, plan64), "frames": frames_for(*c)}
        if plan["fast_path"] == 2:
            e["tiles"] = tiles_of(*c, e["frames"])
        e["pairs"] = [list(p) for p in pairs]
        cases.append(e)
    batches = []
    for c, pairs in _greedy(u["batch"] - have, {c: batch_features(*c) for c in grid()})[0]:
        d, plan, plan64 = plans(*c)
        batches.append({"case": list(c), "fast_path": info_fast_path(plan, plan64), "streams": BATCH_PROBE[0],
                        "frames": BATCH_PROBE[1], "pairs": [list(p) for p in pairs]})
    return {"cases": cases, "batches": batches, "passed_over": [{"case": list(c)} for c in passed]}


def committed():
    with open(CASES_FILE) as f:
        return json.load(f)


def pairs_of(entry):
    return {tuple(p) for p in entry["pairs"]}


def family_of(entry):
    return {0: "cover exact", 2: "cover period", 5: "cover period", 3: "cover slide", 4: "cover slide"}[entry["fast_path"]]


def dumps(doc):
    """one entry per line: a planner change shows as the lines it moves"""
    def block(key):
        return '  "%s": [\n%s\n  ]' % (key, ",\n".join("    " + json.dumps(e) for e in doc[key]))
    return "{\n" + ",\n".join(block(k) for k in ("cases", "batches", "passed_over")) + "\n}\n"


if __name__ == "__main__":
    doc = choose()
    with open(CASES_FILE, "w") as f:
        f.write(dumps(doc))
    u, have = universe(), curated()
    print("universe %d one-state + %d batch-only pairs; curated lists hold %d; %d cases + %d batches written" % (
        len(u["one"]), len(u["batch"]), len((u["one"] | u["batch"]) & have), len(doc["cases"]), len(doc["batches"])))
