"""tests/plan_cover_cases.json, proved without a GPU: with the curated *_CASES lists it meets every pair of (channel
class or kernel kind) x (plan feature) that the rate grid reaches (tests/plan_cover.py); every case still has the pairs
and the fast_path it is listed for -- a planner change fails here instead of silently moving a case onto another
kernel; the schedules are big enough to be able to fail, shown by two defects of a short last phase group planted at
the smallest such case's own size; and on every case's own input the oracle alone passes the hard check and the bias
check, so whatever tests/test_gpu_plan_cover.py finds is the kernel's."""
import ast
import os

import numpy as np
import pytest

import exact_model as em
import oracle as orc
import plan_cover as pc
import speexhip

BIG = 1 << 20
DOC = pc.committed()
CASES = DOC["cases"]
_ID = lambda e: "-".join(str(v) for v in e["case"])


def test_the_grid_is_the_planner_invariant_test_s_rates():
    with open(os.path.join(pc.HERE, "test_cpu_host_logic.py")) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef)
          and n.name == "test_planner_invariants_over_rates_qualities_and_channel_counts"][0]
    rates = [ast.literal_eval(n.value) for n in ast.walk(fn)
             if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "rates"]
    assert rates == [pc.RATES] and len(pc.RATES) == 20
    assert pc.QUALITIES == tuple(range(11)) and pc.CHANNELS == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)
    assert {pc.channel_class(c) for c in pc.CHANNELS} == {"1", "2", "odd", "isa", "gen"}


def test_the_kind_names_are_the_oracle_s():
    assert pc.KINDS == orc.KIND_NAMES
    for c in [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (2, 44100, 48000, 1), (2, 44100, 48000, 10)]:
        o = orc.Oracle(*c)
        d = pc.design(*c[1:])
        assert (d["kind"], d["taps"], d["num"], d["den"]) == (o.kind, o.taps, o.num, o.den), c


def test_the_curated_lists_are_read_whole():
    lists = pc.curated_cases()
    assert set(lists) == {"SLIDE_CASES", "EXACT_FALLBACK_CASES", "FOLDED_CASES", "N_TO_ONE_CASES", "LAYOUT_CASES",
                          "PERIOD64_CASES"}
    assert sum(len(v) for v in lists.values()) >= 150 and len(pc.curated_batches()) >= 15
    assert set(pc.CURATED_LONG_CALL) <= set(lists)


def test_the_committed_cases_and_the_curated_lists_cover_the_universe():
    u, have = pc.universe(), pc.curated()
    every = u["one"] | u["batch"]
    assert len(CASES) + len(DOC["batches"]) <= pc.MAX_CASES
    assert len({tuple(e["case"]) for e in CASES}) == len(CASES)
    mine = set()
    for e in CASES:
        c = tuple(e["case"])
        d, plan, plan64 = pc.plans(*c)
        got = pc.features(*c)
        assert pc.pairs_of(e) and pc.pairs_of(e) <= got, (c, sorted(pc.pairs_of(e) - got, key=repr))
        assert e["fast_path"] == pc.info_fast_path(plan, plan64), (c, plan, plan64)
        assert e["frames"] == pc.frames_for(*c), c
        mine |= got
    for e in DOC["batches"]:
        c = tuple(e["case"])
        d, plan, plan64 = pc.plans(*c)
        assert (e["streams"], e["frames"]) == pc.BATCH_PROBE and e["fast_path"] == pc.info_fast_path(plan, plan64) == 2
        got = pc.batch_features(*c)
        assert pc.pairs_of(e) and pc.pairs_of(e) <= got, (c, sorted(pc.pairs_of(e) - got, key=repr))
        mine |= got
    left = every - have - mine
    print("universe: %d pairs (%d of plans, %d of launches); the curated lists hold %d; %d cases and %d batches hold the "
          "other %d" % (len(every), sum(p[0] != "launch" for p in every), sum(p[0] == "launch" for p in every),
                        len(every & have), len(CASES), len(DOC["batches"]), len(every - have)))
    assert not left, sorted(left, key=repr)
    # every case is there for something the curated lists and the cases before it do not hold
    seen = set(have)
    for e in CASES + DOC["batches"]:
        assert not pc.pairs_of(e) & seen, e["case"]
        seen |= pc.pairs_of(e)
    # the universe is what the issue counted, give or take the features added since: all five families, all four kinds
    assert {p[0] for p in every} == {"period", "slide", "exact", "launch"}
    assert len(every) >= 477


def test_choose_reproduces_the_committed_file():
    with open(pc.CASES_FILE) as f:
        assert pc.dumps(pc.choose()) == f.read(), "run python tests/plan_cover.py and commit tests/plan_cover_cases.json"


def test_every_schedule_is_big_enough_to_be_able_to_fail():
    for e in CASES:
        c = tuple(e["case"])
        ch, i, o, q = c
        d, plan, plan64 = pc.plans(*c)
        frames = e["frames"]
        assert frames > 2 * d["taps"] + 64, c                 # a stretch of silence longer than the filter fits
        if plan["fast_path"] != 2:
            assert "tiles" not in e and frames == max(21011, 3 * d["taps"] + 75), c
            continue
        assert frames % 1000 == 11 and frames <= pc.FRAME_CAP
        assert e["tiles"] == pc.tiles_of(*c, frames) >= 3, c
        # every phase index falls in two tiles of the long call, whichever plan the launch takes
        den = pc.view_den(d, plan)
        for lp in (plan["lane_periods"], plan["w16_lane_periods"], plan64["lane_periods"] if plan64["fast_path"] == 5 else 0):
            assert frames * d["den"] // d["num"] >= 2 * lp * den + den, (c, lp)
        # the long call starts off phase 0: the frames before it left the stream between two input frames -- on every
        # ratio but 1:n, which is on phase 0 after any whole number of frames
        first = pc.sizes_of(d["num"], d["den"], frames)[0]
        used, k0, last, frac = speexhip.plan_call(d["num"], d["den"], first, BIG, 0, 0)
        assert used == first and k0 > 0 and (frac != 0) == (d["num"] != 1 and d["den"] != 1), (c, k0, frac)
        # (and no smaller size of the recipe would do)
        smaller = frames - 1000
        assert smaller < 0 or not (smaller > 2 * d["taps"] + 64 and pc.tiles_of(*c, smaller) >= 3 and
                                   smaller * d["den"] // d["num"] >= pc.min_outputs(*c)), c


@pytest.mark.parametrize("entry", CASES, ids=_ID)
def test_the_oracle_alone_passes_on_the_case_s_own_input(entry):
    """(a) on both streams and (c) wherever n >= 20 000 (em.bias_ok judges no fewer), against the fp32 bound"""
    c = tuple(entry["case"])
    fails, stats = pc.oracle_alone(c)
    print("%s: n %d rms(e) %.3f max|e| %.2f bias %.1f sigma" % (c, stats["n"], stats["rms"], stats["max"], stats["z"]))
    assert not fails, (c, fails)


def test_the_configurations_passed_over_are_those_on_which_the_reference_leaves_its_own_bound():
    """... by a sample or two of an interpolating kind (four blended sums): never a direct kind, never the int16 stream"""
    for e in DOC["passed_over"]:
        c = tuple(e["case"])
        fails, stats = pc.oracle_alone(c)
        assert fails and all(f.startswith("(a)") for f in fails), (c, fails)
        assert pc.design(*c[1:])["kind"].startswith("interpolate") and stats["rms"] < 1.0, (c, stats)
    assert len(DOC["passed_over"]) <= 16


def _smallest_ragged_case():
    ragged = []
    for e in CASES:
        d, plan, _ = pc.plans(*e["case"])
        if plan["fast_path"] == 2 and pc.view_den(d, plan) % plan["r_or_p"]:
            ragged.append((pc._cost(tuple(e["case"])), e["case"], e))
    return min(ragged)[2]


@pytest.mark.parametrize("defect", [None, "the last phase group takes the row of phase den - 1",
                                    "the last tap of the last phase group dropped"])
def test_a_defect_of_the_short_last_phase_group_fails_at_the_case_s_own_size(defect):
    """The smallest committed case whose den leaves a short last phase group, as the documented fp32 chain over the
    case's own float stream: clean it passes every check, with either defect planted in the den % r phases of the
    last group it fails (a).  This is what shows the sizes of frames_for() are not too small."""
    e = _smallest_ragged_case()
    c = tuple(e["case"])
    d, plan, _ = pc.plans(*c)
    r, den = plan["r_or_p"], d["den"]
    assert den == pc.view_den(d, plan) and 0 < den % r < r
    model = em.Model(*c)
    want, fed = pc.oracle_stream(c, e["frames"], "float")
    n = want.shape[0]
    truth, mag = model.truth(fed, n)
    rows, first = model.rows.copy(), den - den % r
    if defect and defect.startswith("the last phase group takes"):
        rows[first:] = rows[den - 1]
    elif defect:
        rows[first:, -1] = 0.0
    got = em.chain32(model, fed, n, rows=rows)
    yard = em.chain32(model, fed, n) if model.double_kind else want
    fails, _ = em.judge_float(model, fed, got, truth, mag, 32, yard, tile=model.num)
    got16 = np.clip(np.floor(got.astype(np.float64) + 0.5), -32768, 32767).astype(np.int16)
    fails += ["(a, int16) " + m for m in em.hard_int16(model, fed, got16, truth, mag, 32, tile=model.num)]
    if defect is None:
        assert not fails, (c, fails)
    else:
        assert any(f.startswith("(a)") for f in fails), (c, defect, fails)
        # ... and in the phases of the last group alone
        bad = np.abs(got.astype(np.float64) - truth) > em.bound32(truth, mag, model.taps)
        phases = model.where(np.nonzero(bad.any(axis=1))[0])[1]
        assert phases.size and phases.min() >= first, (c, defect, np.unique(phases)[:8])
