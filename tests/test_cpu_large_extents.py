"""The tools of the large-extent GPU tests, on the CPU: the virtual input, the window judge's teeth, and the planner at
in_len up to 2^32 - 1 against the reference's block loop restated in Python integers (tests/large_extents.py)."""
import re
import time

import numpy as np
import pytest

import exact_model as em
import large_extents as le
import speexhip

P = le.P


# ---- 1. the virtual input ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float"])
def test_slice_equals_a_materialised_pattern(kind):
    ch = 3
    # silent ranges: one across 2^32, one across a multiple of P, one that a slice only touches with its first frame
    f32 = (1 << 32) // ch
    silent = [(f32 - 20, 41), (5 * P // ch - 3, 90), (1000, 1)]
    v = le.VirtualInput(ch, kind, silent)
    assert v.tile.shape == (P,) and v.tile.dtype == (np.int16 if kind == "int16" else np.float32)
    assert len(np.unique(v.tile[:4096])) > 2000                     # noise, not a constant
    for n0, count in (((1 << 32) - 700, 1500), (5 * P - 400, 1000), (0, 4000), (P - 1, 2 * P // 1000), ((1 << 31) - 5, 10),
                      (1000 * ch + 1, 5), (7 * P, 0)):
        n = n0 + np.arange(count, dtype=np.int64)
        want = v.tile[n % P].copy()
        for s in range(count):                                       # the definition, sample by sample
            f = (n0 + s) // ch
            if any(a <= f < a + c for a, c in silent):
                want[s] = 0
        got = v.slice(n0, count)
        assert got.dtype == v.tile.dtype and got.tobytes() == want.tobytes(), (kind, n0, count)
    assert (v.frames(f32 - 20, 41) == 0).all() and v.frames(f32 - 21, 1).any() and v.frames(f32 + 21, 1).any()
    # a read that wraps at 2^31 or 2^32 lands on other samples
    w = le.VirtualInput(ch, kind)
    for shift in (1 << 31, 1 << 32):
        assert (w.slice(shift + 12345, 4096) != w.slice(12345, 4096)).mean() > 0.99


# ---- 2. the judge has teeth ----------------------------------------------------------------------------------------------
class _Displaced:
    """the input as a kernel reads it whose sample index wraps: sample n >= mark comes from n - mark"""

    def __init__(self, vin, mark):
        self.vin, self.mark, self.channels = vin, mark, vin.channels

    def slice(self, n0, count):
        below = max(0, min(count, self.mark - n0))
        parts = [self.vin.slice(n0, below)] if below else []
        if count - below:
            parts.append(self.vin.slice(n0 + below - self.mark, count - below))
        return np.concatenate(parts)

    def frames(self, f0, count):
        return self.slice(f0 * self.channels, count * self.channels).reshape(count, self.channels)


def _first_failing(fails):
    m = re.search(r"first \[([0-9, ]+)\]", " ".join(fails))
    assert m, fails
    return [int(t) for t in m.group(1).split(",")]


def _render(model, vin, k0, w, kind, rows=None):
    """what a correct kernel (or one with `rows` for taps) stores for outputs [k0, k0 + w)"""
    seg, fed, _ = le.window_segment(model, vin, k0, w)
    truth, _ = seg.truth(fed, w, rows=rows)
    return em.halfup(truth).astype(np.int16) if kind == "int16" else truth.astype(np.float32)


@pytest.mark.parametrize("kind", ["int16", "float"])
def test_the_window_judge_has_teeth(kind):
    ch, i, o, q, w = 2, 44100, 48000, 5, 3000
    model = em.Model(ch, i, o, q)
    num, den, taps = model.num, model.den, model.taps
    sil = le.silence_frames(taps)
    marks = {"2^31": 1 << 31, "2^32": 1 << 32}
    frames = {name: x // ch for name, x in marks.items()}
    vin = le.VirtualInput(ch, kind, [(f + 5, sil) for f in frames.values()])
    for name, x in marks.items():
        f = frames[name]
        k0 = f * den // num - w // 2
        good = _render(model, vin, k0, w, kind)
        assert not le.judge_window(model, 32, vin, k0, good), name
        # a wrapped read: everything from sample x on comes from x lower
        bad = _render(model, _Displaced(vin, x), k0, w, kind)
        fails = le.judge_window(model, 32, vin, k0, bad)
        assert fails, "a read that wraps at %s went through" % name
        first = _first_failing(fails)[0]
        pos = (k0 + first) * num // den                 # line position: the window is input frames (pos - taps, pos]
        assert pos - taps < f <= pos, (name, first, pos, f)  # the first output whose window holds sample x, none before
    # a wrapped store: the window holds what belongs 2^32 / ch frames earlier
    # (the outputs right behind the crossing: those in front of it have no place 2^32 samples earlier)
    kc = (1 << 32) // ch
    good = _render(model, vin, kc + 100, w, kind)
    assert not le.judge_window(model, 32, vin, kc + 100, good)
    stale = _render(model, vin, 100, w, kind)
    fails = le.judge_window(model, 32, vin, kc + 100, stale)
    assert fails and _first_failing(fails)[0] < 4, fails
    # one edge tap dropped: the whole sample inside the silent stretch, 10^-7 of it elsewhere
    f = frames["2^32"]
    k0 = f * den // num - w // 2
    good = _render(model, vin, k0, w, "float")
    pos = (k0 + np.arange(w)) * num // den                  # the window of an output: input frames [pos - (taps - 1), pos]
    silent_frames = np.minimum(pos, f + 5 + sil - 1) - np.maximum(pos - (taps - 1), f + 5) + 1
    edge = (silent_frames >= taps - 4) & (silent_frames < taps)     # all but a few frames of the window are silent
    assert 4 <= edge.sum() <= 16
    for tap in (0, taps - 1):
        rows = model.rows.copy()
        rows[:, tap] = 0.0
        bad = good.copy()
        bad[edge] = _render(model, vin, k0, w, "float", rows=rows)[edge]
        fails = le.judge_window(model, 32, vin, k0, bad)
        assert fails, "tap %d dropped went through" % tap
        assert all(edge[k] for k in _first_failing(fails)), (tap, fails)


def test_windows_name_what_a_case_cannot_reach():
    taps, num, den = 80, 147, 160
    frames = le.frames_to_cross(2, num, den, 8192, in_mark=1 << 31, out_mark=1 << 31)
    assert frames % 2 == 1
    n_out = frames * den // num
    wins, absent, silent = le.windows(2, num, den, taps, frames, n_out, 8192)
    assert [n for n, _, _ in wins] == ["first", "last", "in 2^31", "out 2^31"]
    assert [n for n, _ in absent] == ["in 2^32", "out 2^32"]       # stereo cannot reach 2^32 samples in 2^31 - 1 frames
    assert all(k0 >= 0 and k0 + w <= n_out for _, k0, w in wins)
    assert len(silent) == 3 and all(n == taps + 17 for _, n in silent)
    # every silent range lies inside the input span of its window
    for (name, k0, w), (a, n) in zip([wins[0], wins[1], wins[2]], silent):
        assert k0 * num // den < a and a + n < (k0 + w) * num // den, name
    wins, absent, _ = le.windows(8, num, den, taps, (1 << 29) + 30001, ((1 << 29) + 30001) * den // num, 8192, float_io=True)
    assert not absent and len(wins) == 8


# ---- 3. the planner at the limits ----------------------------------------------------------------------------------------
IN_LENS = [(1 << 31) - 1, 1 << 31, 3 * (1 << 30) + 1, (1 << 32) - 1]
CAPACITIES = [1, 100000, (1 << 31) - 1, (1 << 32) - 1]
RATIOS = [(147, 160), (160, 147), (6, 1), (1, 2), (192, 1), (1, 192), (640, 147), (44100, 44101)]   # in : out = num : den


def test_the_restated_block_loop_equals_the_per_output_loop_on_small_calls():
    """the restatement itself, against the reference's loop output by output, where that loop is affordable"""
    rng = np.random.RandomState(4)
    for num, den in RATIOS + [(3, 2), (441, 160)]:
        for float_entry in (False, True):
            for _ in range(12):
                in_len, cap = int(rng.randint(0, 5000)), int(rng.choice([0, 1, 7, 1000, 1024, 1025, 40000, 1 << 31]))
                frac, magic = int(rng.randint(0, den)), int(rng.choice([0, 0, 3, 40]))
                last = int(rng.choice([0, 0, 1, num // den + 2]))
                block_in = int(rng.choice([160, 160, 97]))
                a = le.reference_plan(num, den, in_len, cap, float_entry, block_in, last, frac, magic)
                b = le.naive_plan(num, den, in_len, cap, float_entry, block_in, last, frac, magic)
                assert a == b, ((num, den), float_entry, in_len, cap, block_in, last, frac, magic)


def test_the_planner_at_the_limits_of_its_counters():
    t0 = time.time()
    n = 0
    for num, den in RATIOS:
        for in_len in IN_LENS:
            for cap in CAPACITIES:
                want = le.reference_plan(num, den, in_len, cap)
                assert speexhip.plan_call(num, den, in_len, cap, 0, 0) == want[:4], ((num, den), in_len, cap)
                for float_entry in (False, True):
                    want = le.reference_plan(num, den, in_len, cap, float_entry)
                    got = speexhip.plan_call_ex(num, den, in_len, cap, float_entry, 160, 0, 0, 0)
                    assert got == want, ((num, den), in_len, cap, float_entry)
                    n += 1
                    # nothing is lost: a call that is not capacity-bound consumes all it was given
                    if got[1] < cap:
                        assert got[0] == in_len
                    assert 0 <= got[2] and got[3] < den
        # a start in the middle of a stream, and pending frames (drained first: inside the block loop by the int16 entry,
        # up front by the float one), at both ends of the range
        for float_entry in (False, True):
            for in_len, cap, last, frac, magic in (((1 << 32) - 1, (1 << 32) - 1, num // den + 1, den - 1, 0),
                                                   ((1 << 31) + 7, (1 << 31) - 1, 2, den // 2, 0),
                                                   ((1 << 32) - 1, (1 << 32) - 1, 0, den // 3, 40),
                                                   (1 << 31, 3, 1, 0, 200)):
                want = le.reference_plan(num, den, in_len, cap, float_entry, 160, last, frac, magic)
                got = speexhip.plan_call_ex(num, den, in_len, cap, float_entry, 160, last, frac, magic)
                assert got == want, ((num, den), in_len, cap, float_entry, last, frac, magic)
                n += 1
    took = time.time() - t0
    print("\n[large extents] planner: %d calls compared in %.2f s" % (n, took))
    assert n == 8 * 4 * 4 * 2 + 8 * 2 * 4      # (about two seconds: whole blocks are skipped along the cycle of positions)


def test_sentinel_ranges_surround_regions_and_their_wrapped_aliases():
    s = le.SENTINELS
    stride = (1 << 32) + 5
    regions = [(0, 9000), (stride, 9000)]
    total = stride + 9000
    r = le.sentinel_ranges(regions, total)
    assert r[0] == (-s, 0) and r[-1] == (total, total + s)
    # the alias of stream 1 (element 5) lies inside stream 0's region: what is left of its sentinels is the gap behind
    assert (9000, 9005 + s) in r and (stride - s, stride) in r
    for lo, hi in r:
        assert lo < hi and all(hi <= a or lo >= a + n for a, n in regions)
    assert all(r[i][1] < r[i + 1][0] for i in range(len(r) - 1))
