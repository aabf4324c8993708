"""The mixer call held to its header (include/speexhip_resampler.h, "Mixer") where test_gpu_mixer.py's noise cannot: the order
of the sum in a kernel that walks its legs in blocks of 16 dealt to four waves, the weights of every bus group, ramps where a
128-sample tile starts in mid-frame and a lane's pair straddles frames, leg ends on, beside and inside tile edges, the limits
(1024 x 1024), and the promises without a test.  The method is test_gpu_bus_edges.py's, unchanged.  Expected bytes never come
from the call under test: a TWIN state per leg runs the same input through process_many_sides with F32 interleaved out and
no gain (test_gpu_mixer.twin_floats), gain_model / bus_model / halfbe_model / dither_model / meter_model do the rest, and
bytes, totals, positions, counters and the bits of get_gain are compared for equality.  No tolerance.  The one allowance is
test_gpu_bus.py's (same_storage: for the float formats a model NaN is matched by any NaN); only the run with the infinite leg
uses it, under its condition that at most 5 % of a bus is NaN in the model.  Every other input is finite and the model
asserts that it made no NaN.

What a wrong kernel would have to change is PLANTED in the model first -- bus_model's defects, LEG_DEFECTS for this kernel's
blocks and waves, the ramp defects with this kernel's tile (128) and lane group (2), wrong weight indexing -- and must change
the model's output on the twins' floats of the very case: a condition, not a tolerance; a case that cannot tell the defect
from the rule fails.  The shares print with -s; DESIGN.md section 4 records them.

Every output buffer is host memory filled with Resampler.SENTINEL_BYTE, the buses a gap apart and a planar side's planes a
gap apart: behind bus_frames of every bus and plane, and in every gap, the sentinel must still be there after the call."""
import collections
import functools

import numpy as np
import pytest

import bus_model as bm
import dither_model as dm
import gain_model as gm
import halfbe_model as hm
import meter_model as mm
import speexhip
import test_gpu_bus as tb
import test_gpu_mixer as tm

pytestmark = pytest.mark.gpu

F32, S16, ULAW, S24 = tm.F32, tm.S16, tm.ULAW, tm.S24
INTER, PLANAR = tm.INTER, tm.PLANAR
START = tm.START
SENT = speexhip.Resampler.SENTINEL_BYTE
TILE, GROUP = 128, 2          # samples of a bus_sum_legs workgroup, samples of a lane
GAP, PLANE_GAP = 5, 3         # samples between two buses' buffers, between two planes
MONO_RUNS = ((F32, INTER), (S16, INTER))
WIDE_RUNS = MONO_RUNS + ((S24, PLANAR),)

Result = collections.namedtuple("Result", "got bus_frames used made codes rc")


def noise(seed, shape, scale=0.9):
    return (np.random.default_rng(seed).uniform(-scale, scale, shape) * 32767.0).astype(np.float32)


def f32_chunks(x):
    """(legs, frames, ch) float32 in int16 units: one F32 chunk of bytes per leg"""
    out = [np.ascontiguousarray(x[i]).view(np.uint8).reshape(-1) for i in range(len(x))]
    for c in out:
        c.setflags(write=False)
    return out


def frozen(ys):
    for y in ys:
        if y is not None:
            y.setflags(write=False)
    return tuple(ys)


def twins_once(case, lens, chunks, mode=None):
    """the case's one call through fresh twins: (floats per slot, consumed)"""
    twins = case.states(mode)
    try:
        ys, used = tm.twin_floats(case, twins, lens, chunks)
    finally:
        tm.close_all(twins)
    return frozen(ys), tuple(used)


def sizes(ys):
    return [0 if y is None else y.size for y in ys]


# ---- the model ------------------------------------------------------------------------------------------------------------
def frames_of(n_samples, ch, defect=None):
    """the frame whose g multiplies flat sample n of a leg's image -- with one of the kernel's ramp defects planted:
      ignores_r0    the frame of sample i of a tile taken as tile0 // C + i // C: the tile's first channel forgotten
      group_first   g of the first of a lane's two samples used for both"""
    n = np.arange(n_samples)
    if defect == "ignores_r0":
        tile0 = n // TILE * TILE
        return tile0 // ch + (n - tile0) // ch
    if defect == "group_first":
        return (n // GROUP * GROUP) // ch
    assert defect in (None, "past_end"), defect
    return n // ch


def gained_rows(ch, ys, gfull, frames, defect=None):
    """(n_legs, frames * ch) float32: every slot behind its gain (gfull[i]: g of each of the bus's frames, None: off), +0.0f
    behind its end and for a slot without floats -- with "past_end" planted, the product of +0.0f and g behind a leg's end"""
    rows = np.zeros((len(ys), frames * ch), np.float32)
    for s, y in enumerate(ys):
        if y is None:
            continue
        if gfull is None or gfull[s] is None:
            rows[s, : y.size] = y
            continue
        g = np.asarray(gfull[s], np.float32)
        assert g.shape == (frames,)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            rows[s, : y.size] = y * g[frames_of(y.size, ch, defect)]
            if defect == "past_end":
                rows[s, y.size:] = np.float32(0.0) * g[frames_of(frames * ch, ch)[y.size:]]
    return rows


def model(w, ch, ys, gfull=None, defect=None, gain_defect=None, nan_ok=False, wide=False):
    """(n_buses, bus_frames * ch) float32 of the slots' floats ys (None: a slot that supplies nothing), and bus_frames"""
    n = sizes(ys)
    frames = max(n) // ch
    rows = gained_rows(ch, ys, gfull, frames, gain_defect)
    if gain_defect is None and gfull is not None:   # (the rule's rows are gain_model's own products)
        own = [np.zeros(0, np.float32) if y is None else y if gfull[s] is None else gm.apply(y, gfull[s][: y.size // ch], ch)
               for s, y in enumerate(ys)]
        assert rows.tobytes() == bm.pad(own, frames, ch).tobytes()
    if defect in bm.LEG_DEFECTS:
        z = bm.buses_legs(w, rows, defect)
    elif defect is None and wide:
        z = bm.buses_wide(w, rows)
    else:
        z = bm.buses(w, rows, defect, bm.live_of(n, frames * ch))
    if defect is None and gain_defect is None:
        if nan_ok:
            assert np.isnan(z).any(), "the buses hold no NaN"
            assert all(np.isnan(zj).mean() <= 0.05 for zj in z), "more than 5 % of a bus is NaN in the model"
        else:
            assert not np.isnan(z).any(), "a finite input made a NaN in the model"
    return z, frames


def ramps(models, made, frames):
    """g of each of the bus's `frames` frames per slot (None: the gain is off), and the models moved by what each produced"""
    out = []
    for mo, n in zip(models, made):
        out.append(None if mo is None or mo.off() else gm.g(mo.frm, mo.to, mo.total, mo.done, frames))
        if mo is not None:
            mo.take(n)
    return out


def differs(z, want):
    """the largest share of a bus's samples that differ in their bits"""
    return max(bm.changed(a, b) for a, b in zip(z, want))


def must_change(what, bad, z, bar=0.0):
    share = differs(bad, z)
    print("%-40s: up to %5.1f %% of a bus's samples change" % (what, 100 * share))
    assert share > bar if bar == 0.0 else share >= bar, "the twins' floats do not tell %s from the rule" % what
    return share


# ---- the call, into sentinels ---------------------------------------------------------------------------------------------
def in_sides(case, legs, chunks):
    return [None if legs[i] is None else
            speexhip.make_side(case.fmts[i], case.ch, data=None if chunks[i] is None else chunks[i].ctypes.data) for i in range(case.n)]


def run(m, case, legs, lens, chunks, fmt, layout=INTER, caps=None, sides=None):
    """one mixer call into a host buffer of sentinels: the buses' bytes (n_buses, bytes; planar: plane after plane) and what
    the call returned.  Whatever lies outside [0, bus_frames) of every bus and plane must still hold the sentinel."""
    caps = case.caps(lens) if caps is None else list(caps)
    ch, nb = case.ch, hm.nbytes(fmt)
    cap = max(caps + [1])
    planar = layout == PLANAR and ch > 1
    plane = cap + PLANE_GAP
    stride = (plane * ch if planar else cap * ch) + GAP
    buf = np.full(case.n_buses * stride * nb, SENT, np.uint8)
    out_side = speexhip.make_side(fmt, ch, layout=layout, data=buf.ctypes.data, plane_stride=plane, stream_stride=stride)
    sides = in_sides(case, legs, chunks) if sides is None else sides
    rc, used, made, bus_frames, codes = m.process_sides(legs, sides, list(lens), out_side, caps)
    assert bus_frames is not None, "the call did not set bus_frames (code %d)" % rc
    assert bus_frames <= cap
    written = np.zeros(buf.size, bool)
    got = []
    for j in range(case.n_buses):
        base = j * stride * nb
        parts = [(base + k * plane * nb, bus_frames * nb) for k in range(ch)] if planar else [(base, bus_frames * ch * nb)]
        got.append(np.concatenate([buf[a: a + n] for a, n in parts]))
        for a, n in parts:
            written[a: a + n] = True
    stray = np.flatnonzero(~written & (buf != SENT))
    assert stray.size == 0, "%d bytes written outside the buses' frames, the first at byte %d (bus stride %d bytes, %d frames)" % (
        stray.size, stray[0], stride * nb, bus_frames)
    return Result(np.stack(got), bus_frames, used, made, codes, rc)


def run_and_check(case, lens, chunks, ys, z, frames, runs, what, gains=None, used_want=None):
    """fresh legs and a fresh mixer per output format: the call equals the model"""
    for fmt, layout in runs:
        legs, m = case.states(), tm.mixer_of(case)
        try:
            if gains is not None:
                gains(legs)
            r = run(m, case, legs, lens, chunks, fmt, layout)
            assert r.rc == 0 and r.codes == [0] * case.n, (r.rc, r.codes)
            assert r.bus_frames == frames and [v * case.ch for v in r.made] == sizes(ys)
            if used_want is not None:
                assert r.used == list(used_want)
            tm.check_buses(case, fmt, layout, r.got, z, dm.NONE, 0, "%s format %d layout %d" % (what, fmt, layout))
        finally:
            m.close()
            tm.close_all(legs)


def counters_of(fn):
    c0 = speexhip.debug_mixer_counters()
    out = fn()
    c1 = speexhip.debug_mixer_counters()
    return out, {k: c1[k] - c0[k] for k in c0}


# ---- A. the order of the sum ------------------------------------------------------------------------------------------------
ORDER_FRAMES = 603          # (thirds of 201 input frames: the q7 filter is 128 long, and a pair needs a stretch of outputs to itself)
ORDER_KEY = (1, 8000, 16000, 7)
SEVEN = bm.ORDER_DEFECTS + ("round_each_add",) + bm.LEG_DEFECTS


@functools.lru_cache(maxsize=None)
def order_case():
    x = bm.order_layout_legs(bm.LEGS_48, bm.PAIRS_48, ORDER_FRAMES).reshape(bm.LEGS_48, ORDER_FRAMES, 1)
    case = tm.Case(1, [ORDER_KEY] * bm.LEGS_48, [F32] * bm.LEGS_48, bm.order_weights_legs(bm.LEGS_48, bm.PAIRS_48, 8))
    lens = (ORDER_FRAMES,) * bm.LEGS_48
    chunks = f32_chunks(x)
    ys, used = twins_once(case, lens, chunks)
    return case, lens, chunks, ys, used


def stretch_masks(ys, pairs):
    """per pair, the samples of the twins' floats where the pair is huge and everybody else is small: its stretch as the
    filter left it"""
    y = np.abs(np.stack(ys))
    masks = []
    for a, b in pairs:
        others = np.delete(y, (a, b), axis=0)
        masks.append((y[a] > 2.0 ** 55) & (others.max(axis=0) < 2.0 ** 15))
    return masks


def order_preconditions(case, ys, pairs, least):
    """the layout survived the filter; the stretches (least = None: the whole bus as one, where the filter is longer than a
    stretch and the pairs' reaches overlap)"""
    n = ys[0].size
    assert all(y.size == n for y in ys if y is not None) and np.isfinite(np.stack([y for y in ys if y is not None])).all()
    for a, b in pairs:      # the negations survived the filter exactly
        assert ys[b].tobytes() == (-ys[a]).tobytes(), "leg %d is not the negation of leg %d" % (b, a)
    if least is None:
        return [np.ones(n, bool)]
    filled = [np.zeros(n, np.float32) if y is None else y for y in ys]
    masks = stretch_masks(filled, pairs)
    print("order stretches as the filter left them: %s of %d samples" % ([int(k.sum()) for k in masks], n))
    assert all(k.sum() >= least for k in masks), "a pair has no stretch of its own behind the filter"
    return masks


def order_defects(case, ys, z, masks, defects):
    for defect in defects:
        bad, _ = model(case.w[:2], 1, ys, defect=defect)
        share = [max(bm.changed(bad[j][k], z[j][k]) for j in (0, 1)) for k in masks]
        print("order %4d legs, %-16s: %s %% of rows 0 / 1 change per stretch" % (case.n, defect, " / ".join("%5.1f" % (100 * s) for s in share)))
        assert max(share) >= 0.01, "the twins' floats do not tell %s from the rule" % defect


def test_the_sum_runs_in_ascending_slot_order_across_blocks_and_waves():
    case, lens, chunks, ys, used = order_case()
    masks = order_preconditions(case, ys, bm.PAIRS_48, 64)
    z, frames = model(case.w, 1, ys)
    assert frames == ys[0].size > 700
    assert z[2:5].tobytes() == np.zeros((3, frames), np.float32).tobytes(), "a pair alone is not +0.0"
    order_defects(case, ys, z, masks, SEVEN)
    run_and_check(case, lens, chunks, ys, z, frames, MONO_RUNS, "order", used_want=used)


# ---- B. the weights of every group ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights_case():
    n, n_buses, frames = 20, 41, 320
    w = np.random.default_rng(2041).uniform(-1.5, 1.5, (n_buses, n)).astype(np.float32)
    w[37] = 0.0
    case = tm.Case(1, [(1, 16000, 48000, 5)] * n, [F32] * n, w)
    lens = (frames,) * n
    x = noise(20, (n, frames, 1))
    ys, used = twins_once(case, lens, f32_chunks(x))
    return case, lens, x, ys, used


def test_weights_reach_every_wave_and_workgroup_row_untransposed():
    case, lens, x, ys, used = weights_case()
    w = case.w
    z, frames = model(w, 1, ys)
    assert frames == 960 and not w[37].any() and not z[37].any()
    wt = w.copy()
    wt[:20, :20] = w[:20, :20].T
    must_change("weights, W transposed where it can be", model(wt, 1, ys)[0], z)
    for group in (32, 8):
        must_change("weights, bus j reads bus j mod %d" % group, model(w[np.arange(41) % group], 1, ys)[0], z)
    run_and_check(case, lens, f32_chunks(x), ys, z, frames, MONO_RUNS, "weights", used_want=used)


# ---- C. signed zeros; a zero weight on an infinite leg ----------------------------------------------------------------------
SIGNS_W = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
INF_W = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)


@functools.lru_cache(maxsize=None)
def signs_case():
    case = tm.Case(1, [ORDER_KEY] * 2, [F32] * 2, SIGNS_W)
    x = noise(1, (2, 160, 1))
    ys, used = twins_once(case, (0, 160), f32_chunks(x))
    return case, x, ys


@pytest.mark.parametrize("first_slot", ("fed nothing", "empty", "refused"))
def test_signed_zeros_with_a_first_slot_that_supplies_nothing(first_slot):
    case, x, ys = signs_case()
    assert ys[0].size == 0 and ys[1].size > 300 and (ys[1] != 0).all()
    neg = ys[1] < 0
    assert 0.2 < neg.mean() < 0.8
    z, frames = model(case.w, 1, ys)
    # -1 on the slot that supplies +0.0f, 0 on the live leg: -0 + -0 = -0, -0 + +0 = +0; +1 on it: +0 + either = +0
    assert z[0].tobytes() == np.where(neg, np.float32(-0.0), np.float32(0.0)).astype(np.float32).tobytes()
    assert z[1].tobytes() == np.zeros(neg.size, np.float32).tobytes() and z[2].tobytes() == ys[1].tobytes()
    for defect in ("zero_plus_first", "skip_zero_weight", "skip_ended"):
        must_change("signs, " + defect, model(case.w, 1, ys, defect=defect)[0], z)
    chunks = f32_chunks(x)
    A = speexhip.ERR_INVALID_ARG
    for fmt, layout in MONO_RUNS + ((ULAW, INTER),):
        legs, m = case.states(), tm.mixer_of(case)
        try:
            call_legs, sides, lens = list(legs), in_sides(case, legs, chunks), [0, 160]
            if first_slot == "empty":
                call_legs[0], sides[0] = None, None
            elif first_slot == "refused":
                sides[0].channels, lens[0] = 2, 160
            before = tm.position_of(legs[0])
            r = run(m, case, call_legs, lens, chunks, fmt, layout, caps=[384, 384], sides=sides)
            want_code = A if first_slot == "refused" else 0
            assert r.codes == [want_code, 0] and r.rc == want_code
            assert r.bus_frames == frames and r.made[1] == frames and r.used[1] == 160
            assert (r.used[0], r.made[0]) == ((160, 384) if first_slot == "refused" else (0, 0))
            assert tm.position_of(legs[0]) == before
            tm.check_buses(case, fmt, layout, r.got, z, dm.NONE, 0, "signs, slot 0 %s, format %d" % (first_slot, fmt))
        finally:
            m.close()
            tm.close_all(legs)


def test_a_zero_weight_on_an_infinite_leg_is_nan():
    ch, fi, fo, q, frames_in, fed, _ = tb.CASES["stereo"]
    x = tb.noise("stereo")
    case = tm.Case(ch, [(ch, fi, fo, q)] * 3, [F32] * 3, INF_W)
    chunks = f32_chunks(x)
    ys, used = twins_once(case, fed, chunks)
    assert np.isinf(ys[2]).any() and np.isfinite(ys[1]).all()
    z, frames = model(case.w, ch, ys, nan_ok=True)
    bad, _ = model(case.w, ch, ys, defect="skip_zero_weight")
    inf_at = np.zeros(frames * ch, bool)
    inf_at[: ys[2].size] = np.isinf(ys[2])
    assert np.isnan(z[0][inf_at]).all() and not np.isnan(bad[0][inf_at & ~np.isnan(bm.pad(ys, frames, ch)[0])]).any()
    print("inf, skip_zero_weight: %.2f %% of bus 0 changes; %.2f %% of bus 0 is NaN in the model" % (
        100 * bm.changed(bad[0], z[0]), 100 * np.isnan(z[0]).mean()))
    assert bm.changed(bad[0], z[0]) > 0
    run_and_check(case, fed, chunks, ys, z, frames, WIDE_RUNS, "inf", used_want=used)


# ---- D. ramps where tiles start in mid-frame ------------------------------------------------------------------------------------
RAMP_SLOTS = 18
RAMP_FED = (1500, 1500, 1201, 0, 1500) + (1500,) * (RAMP_SLOTS - 5)
# slot: (gain, ramp frames).  0: a ramp that ends inside the call in mid-tile; 1: a constant; 2: a ramp still in flight when
# the leg ends, negative by then; 3: a ramp on the leg fed nothing; 4: a negative constant; 17 (second block, wave 1): a ramp
# in flight at the end of the call; everybody else off
RAMP_GAINS = {0: (0.3, 1777), 1: (0.5, 0), 2: (-0.5, 4000), 3: (0.7, 900), 4: (-1.0, 0), 17: (2.0, 100000)}
ALONE = 3   # the bus that weights the short negative-gained leg (slot 2) alone


def ramp_gains(n, table, legs=None):
    """the gains of `table` set on legs (None: on the models alone): the models"""
    models = [gm.State() for _ in range(n)]
    for s, (gain, ramp) in table.items():
        models[s].set(gain, ramp)
        if legs is not None:
            assert legs[s].set_gain(gain, ramp) == 0
    return models


@functools.lru_cache(maxsize=None)
def ramp_case():
    """3 channels 16k -> 48k q5.  The input is noise around a level of its own sign per leg, so that behind the end of the
    short leg every live leg's GAINED sample is negative: on bus ALONE -- 1 on slot 2, -1 on the slot that was fed nothing,
    0 on everybody else -- every term but slot 2's is then -0.0, and slot 2's own term decides the sign of the sum: +0.0f by
    the rule, -0.0f if the kernel multiplied the +0.0f behind the leg's end by its (negative) g."""
    ch, frames = 3, 1500
    rng = np.random.default_rng(318)
    w = rng.uniform(-1.5, 1.5, (5, RAMP_SLOTS)).astype(np.float32)
    w[ALONE] = 0.0
    w[ALONE, 2], w[ALONE, 3] = 1.0, -1.0
    level = np.full(RAMP_SLOTS, -12000.0, np.float32)
    level[4] = 12000.0        # (its gain is negative)
    x = (level[:, None, None] + noise(319, (RAMP_SLOTS, frames, ch), 0.1)).astype(np.float32)
    case = tm.Case(ch, [(ch, 16000, 48000, 5)] * RAMP_SLOTS, [F32] * RAMP_SLOTS, w)
    ys, used = twins_once(case, RAMP_FED, f32_chunks(x))
    return case, x, ys, used


def check_ramp_defects(name, w, ch, ys, gfull, z, past_end_bus=None):
    for defect in ("ignores_r0", "group_first"):
        must_change("%s, ramp %s" % (name, defect), model(w, ch, ys, gfull, gain_defect=defect)[0], z, 0.01)
    if past_end_bus is not None:
        bad, _ = model(w, ch, ys, gfull, gain_defect="past_end")
        must_change("%s, ramp past_end" % name, bad[past_end_bus: past_end_bus + 1], z[past_end_bus: past_end_bus + 1])


@functools.lru_cache(maxsize=None)
def ramp_model():
    case, x, ys, used = ramp_case()
    ch = case.ch
    made = [y.size // ch for y in ys]
    frames, total = max(made), max(made) * ch
    assert all(made[i] == frames for i in range(RAMP_SLOTS) if i not in (2, 3)) and made[3] == 0
    # whole tiles and a tail; every tile but each third starts in mid-frame; slot 2 ends inside a tile, in mid-pair of a
    # lane or not, before the bus does; slot 0's ramp ends in mid-tile
    assert total // TILE >= 4 and total % TILE != 0 and TILE % ch == 2
    assert 0 < made[2] < frames and (made[2] * ch) % TILE != 0 and made[2] * ch > TILE
    assert 1777 < frames and (1777 * ch) % TILE not in (0, TILE - 1) and made[2] < 4000
    models = ramp_gains(RAMP_SLOTS, RAMP_GAINS)
    gfull = ramps(models, made, frames)
    assert gfull[5] is None and (np.diff(gfull[0]) != 0).sum() > 1000 and models[3].done == 0 and models[2].done == made[2]
    assert models[17].done < models[17].total and gfull[2][made[2]] < 0
    # behind slot 2's end every live leg's gained sample is negative (the docstring of ramp_case)
    rows = gained_rows(ch, ys, gfull, frames)
    tail = slice(made[2] * ch, total)
    assert (np.delete(rows, (2, 3), axis=0)[:, tail] < 0).all(), "a live leg is not negative behind the short leg's end"
    z, _ = model(case.w, ch, ys, gfull)
    assert z[ALONE][tail].tobytes() == np.zeros(total - made[2] * ch, np.float32).tobytes()
    check_ramp_defects("18 x 5 of 3 channels", case.w, ch, ys, gfull, z, past_end_bus=ALONE)
    return z, frames, made, tuple(mo.report() for mo in models)


@pytest.mark.parametrize("fmt_name,layout", (("f32", INTER), ("s16", INTER), ("s24", PLANAR)))
def test_ramps_of_three_channels_in_and_behind_the_legs(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, x, ys, used = ramp_case()
    z, frames, made_want, reports = ramp_model()
    legs, m = case.states(), tm.mixer_of(case)
    try:
        ramp_gains(RAMP_SLOTS, RAMP_GAINS, legs)
        r = run(m, case, legs, RAMP_FED, f32_chunks(x), fmt, layout)
        assert r.rc == 0 and r.codes == [0] * RAMP_SLOTS and r.made == made_want and r.bus_frames == frames and r.used == list(used)
        tm.check_buses(case, fmt, layout, r.got, z, dm.NONE, 0, "ramps " + fmt_name)
        for s in range(RAMP_SLOTS):
            assert tm.report(legs[s]) == reports[s], "get_gain of leg %d after the call" % s
        assert legs[3].get_gain()["remaining"] == 900, "the ramp of a leg that was fed nothing moved"
    finally:
        m.close()
        tm.close_all(legs)


@pytest.mark.parametrize("fmt_name,layout", (("f32", INTER), ("s16", INTER), ("s24", PLANAR)))
def test_two_calls_of_the_ramped_legs_give_what_one_gives(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, x, ys, used = ramp_case()
    z, frames, made_want, reports = ramp_model()
    kind, cut, ch = dm.TRIANGULAR, 700, case.ch

    def go(cuts):
        legs, m = case.states(), tm.mixer_of(case, kind, meter=True)
        try:
            ramp_gains(RAMP_SLOTS, RAMP_GAINS, legs)
            pieces, total = [], 0
            for lo, hi in cuts:
                lens = [max(0, min(f, hi) - lo) for f in RAMP_FED]
                r = run(m, case, legs, lens, f32_chunks(x[:, lo:hi]), fmt, layout)
                assert r.rc == 0 and r.used == lens
                if (lo, hi) == (0, cut):    # the cut is where every leg that is fed has produced the same count
                    assert len(set(v for i, v in enumerate(r.made) if i != 3)) == 1 and r.made[3] == 0
                pieces.append(r.got.reshape(case.n_buses, ch if layout == PLANAR else 1, -1))
                total += r.bus_frames
            meters = [m.get_bus_meter(j) for j in range(case.n_buses)]
            return (np.concatenate(pieces, axis=2).reshape(case.n_buses, -1), total, meters, m.bus_position(),
                    tuple(tm.report(st) for st in legs))
        finally:
            m.close()
            tm.close_all(legs)

    one, two = go(((0, 1500),)), go(((0, cut), (cut, 1500)))
    for res, what in ((one, "one call"), (two, "two calls")):
        assert res[1] == frames and res[3] == START + frames and res[4] == reports, what
        tm.check_buses(case, fmt, layout, res[0], z, kind, START, what)
        for j in range(case.n_buses):
            d = dm.values(kind, dm.stream_seed(tm.SEED, case.n + j), START * ch, z[j].size) if mm.clips(fmt) else None
            got = dict(res[2][j])
            assert got.pop("on") is True and mm.same(got, mm.totals(fmt, z[j], d)), "%s: bus %d meter" % (what, j)
    assert one[0].tobytes() == two[0].tobytes()       # (finite input: the float formats too)


@pytest.mark.parametrize("ch,key,n,n_buses,frames_in", ((5, (5, 44100, 48000, 5), 3, 33, 400), (7, (7, 16000, 48000, 5), 2, 2, 300)))
def test_a_ramp_and_a_constant_at_five_and_seven_channels(ch, key, n, n_buses, frames_in):
    rng = np.random.default_rng(500 + ch)
    w = rng.uniform(-1.5, 1.5, (n_buses, n)).astype(np.float32)
    case = tm.Case(ch, [key] * n, [F32] * n, w)
    x = noise(600 + ch, (n, frames_in, ch))
    lens, chunks = (frames_in,) * n, f32_chunks(x)
    ys, used = twins_once(case, lens, chunks)
    made = [y.size // ch for y in ys]
    frames = max(made)
    assert TILE % ch in (2, 3) and frames * ch // TILE >= 2 and (frames * ch) % TILE != 0
    table = {0: (0.25, frames - 37), 1: (-0.75, 0)}
    models = ramp_gains(n, table)
    gfull = ramps(models, made, frames)
    assert models[0].done == models[0].total < frames
    z, _ = model(w, ch, ys, gfull)
    check_ramp_defects("%d x %d of %d channels" % (n, n_buses, ch), w, ch, ys, gfull, z)
    for fmt, layout in WIDE_RUNS:
        legs, m = case.states(), tm.mixer_of(case)
        try:
            ramp_gains(n, table, legs)
            r = run(m, case, legs, lens, chunks, fmt, layout)
            assert r.rc == 0 and r.made == made and r.bus_frames == frames and r.used == list(used)
            tm.check_buses(case, fmt, layout, r.got, z, dm.NONE, 0, "%d channels format %d" % (ch, fmt))
            assert [tm.report(st) for st in legs] == [mo.report() for mo in models]
        finally:
            m.close()
            tm.close_all(legs)


# ---- E. leg ends at tile edges -------------------------------------------------------------------------------------------------
EDGE_KEY = (1, 48000, 48000, 3)
EDGE_FED = (384, 128, 127, 129, 256, 1, 0, 300, 383)


def edge_case(fed, n_buses, seed, zero_row=None):
    n = len(fed)
    w = np.random.default_rng(seed).uniform(-1.5, 1.5, (n_buses, n)).astype(np.float32)
    if zero_row is not None:
        w[zero_row] = 0.0
    case = tm.Case(1, [EDGE_KEY] * n, [F32] * n, w)
    x = noise(seed + 1, (n, max(max(fed), 1), 1))
    chunks = f32_chunks(x)
    ys, used = twins_once(case, fed, chunks)
    # at this ratio a leg produces exactly what it is fed, from its first frame on
    assert sizes(ys) == list(fed) and list(used) == list(fed), (sizes(ys), fed)
    return case, chunks, ys, used


@pytest.mark.parametrize("name,fed", (("whole tiles", EDGE_FED), ("a tail of one", (385,) + EDGE_FED[1:]), ("under a tile", (100, 37)),
                                      ("one frame", (1,))))
def test_legs_that_end_on_beside_and_inside_tile_edges(name, fed):
    n_buses = 3 if len(fed) > 1 else 1
    case, chunks, ys, used = edge_case(fed, n_buses, 700 + len(fed), zero_row=2 if name == "whole tiles" else None)
    z, frames = model(case.w, 1, ys)
    assert frames == max(fed)
    if name == "whole tiles":
        assert frames % TILE == 0 and frames // TILE == 3
        # bus 2 weights nobody: every ended leg's +0.0f decides its sign (+0.0f throughout); a kernel that skips ended legs
        # leaves -0.0f wherever the legs still live are both negative
        assert z[2].tobytes() == np.zeros(frames, np.float32).tobytes()
        must_change("edges, skip_ended", model(case.w, 1, ys, defect="skip_ended")[0], z)
    run_and_check(case, fed, chunks, ys, z, frames, MONO_RUNS, "edges " + name, used_want=used)


@pytest.mark.parametrize("n,n_buses", ((1, 9), (16, 8), (17, 32), (33, 33)))
def test_small_shapes_of_legs_and_buses(n, n_buses):
    fed = tuple(200 - (i % 3) for i in range(n))
    case, chunks, ys, used = edge_case(fed, n_buses, 800 + n)
    z, frames = model(case.w, 1, ys)
    assert frames == 200
    run_and_check(case, fed, chunks, ys, z, frames, MONO_RUNS, "%d x %d" % (n, n_buses), used_want=used)


# ---- F. a call that makes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ("fed nothing", "refused"))
def test_a_call_that_makes_nothing_moves_nothing(how):
    n, frames_in, fmt, kind = 4, 320, S16, dm.TRIANGULAR
    w = np.random.default_rng(900).uniform(-1.5, 1.5, (3, n)).astype(np.float32)
    case = tm.Case(1, [(1, 16000, 48000, 5)] * n, [F32] * n, w)
    x = noise(901, (n, frames_in, 1))
    chunks, lens = f32_chunks(x), (frames_in,) * n
    ys, used = twins_once(case, lens, chunks)
    model_g = gm.State()
    model_g.set(0.5, 1000)
    made = [y.size for y in ys]
    z, frames = model(w, 1, ys, ramps([None, model_g, None, None], made, max(made)))
    legs, m, fresh_legs, fresh = case.states(), tm.mixer_of(case, kind, meter=True), case.states(), tm.mixer_of(case, kind, meter=True)
    try:
        for group in (legs, fresh_legs):
            assert group[1].set_gain(0.5, 1000) == 0
        state = lambda: ([tm.position_of(st) for st in legs], [tm.report(st) for st in legs], [sorted(st.info().items()) for st in legs],
                         m.bus_position(), [sorted(m.get_bus_meter(j).items()) for j in range(3)])
        before = state()
        sides = in_sides(case, legs, chunks)
        if how == "refused":
            for s in sides:
                s.channels = 2
            sides[0].fmt = 99       # (the first refusal: the code the call returns)
        r = run(m, case, legs, [0] * n if how == "fed nothing" else lens, chunks, fmt, caps=[1024] * n, sides=sides)
        A = speexhip.ERR_INVALID_ARG
        assert r.bus_frames == 0 and r.got.size == 0
        if how == "fed nothing":
            assert r.rc == 0 and r.codes == [0] * n and r.made == [0] * n and r.used == [0] * n
        else:
            assert r.rc == A and r.codes == [A] * n and r.made == [1024] * n and r.used == list(lens)
        assert state() == before, "a call that made nothing moved something"
        assert m.bus_position() == START
        # the next ordinary call: the model's, and a fresh mixer's
        a = run(m, case, legs, lens, chunks, fmt)
        b = run(fresh, case, fresh_legs, lens, chunks, fmt)
        assert a.rc == 0 and a.made == made and a.bus_frames == frames
        tm.check_buses(case, fmt, INTER, a.got, z, kind, START, "behind a call that made nothing")
        assert a.got.tobytes() == b.got.tobytes() and m.bus_position() == fresh.bus_position() == START + frames
        tm.check_meters(m, case, fmt, z, kind, START, frames, "behind a call that made nothing")
        assert [tm.report(st) for st in legs] == [tm.report(st) for st in fresh_legs] and tm.report(legs[1]) == model_g.report()
    finally:
        m.close()
        fresh.close()
        tm.close_all(legs, fresh_legs)


# ---- G. the transfer routes ----------------------------------------------------------------------------------------------------
def pinned_copies(chunks):
    """the chunks in pinned blocks of the library: (views, the blocks to close)"""
    blocks, views = [], []
    for c in chunks:
        if c is None or c.size == 0:
            views.append(c)
            continue
        b = speexhip.PinnedBlock(c.size)
        blocks.append(b)
        v = b.array(np.uint8, (c.size,))
        v[:] = c
        views.append(v)
    return views, blocks


def test_large_payloads_travel_on_their_own_and_pinned_chunks_are_read_in_place():
    n, big, little, fmt = 4, 70000, 1000, S16
    w = np.array([[1.0, -0.5, 0.25, 1.0], [0.3, 0.3, 0.3, -1.5]], np.float32)
    case = tm.Case(1, [(1, 44100, 48000, 3)] * n, [F32] * n, w)
    lens = (big, big, big, little)
    x = noise(1000, (n, big, 1), 0.4)
    chunks = [c[: f * 4] for c, f in zip(f32_chunks(x), lens)]
    # (each large payload is at least 256 KiB, and the call's pageable bytes are past what runs on pinned memory alone)
    assert all(c.size >= 256 * 1024 for c in chunks[:3]) and sum(c.size for c in chunks) > 720 * 1024
    ys, used = twins_once(case, lens, chunks)
    z, frames = model(w, 1, ys)
    assert ys[3].size < ys[0].size == frames

    def go(these):
        legs, m = case.states(), tm.mixer_of(case)
        try:
            r, d = counters_of(lambda: run(m, case, legs, lens, these, fmt))
            assert r.rc == 0 and r.used == list(used) and r.made == sizes(ys) and r.bus_frames == frames
            tm.check_buses(case, fmt, INTER, r.got, z, dm.NONE, 0, "routes")
            return r, d
        finally:
            m.close()
            tm.close_all(legs)

    # the gathered stage (the table and the small payload) and one transfer for each payload that travels on its own
    r, d = go(chunks)
    assert (d["transfers_in"], d["transfers_out"], d["bus_sum_launches"], d["fir_launches"], d["out_passes"]) == (4, 1, 1, 1, 1), d
    views, blocks = pinned_copies(chunks)
    try:
        rp, dp = go(views)
    finally:
        for b in blocks:
            b.close()
    # read in place: nothing travels beside the stage
    assert (dp["transfers_in"], dp["transfers_out"], dp["bus_sum_launches"], dp["fir_launches"], dp["out_passes"]) == (1, 1, 1, 1, 1), dp
    assert rp.got.tobytes() == r.got.tobytes()


def test_a_small_tick_of_pinned_chunks_equals_itself_with_pageable_chunks():
    case, lens, x, ys, used = weights_case()
    z, frames = model(case.w, 1, ys)
    chunks = f32_chunks(x)
    views, blocks = pinned_copies(chunks)
    try:
        got = []
        for these in (chunks, views):
            legs, m = case.states(), tm.mixer_of(case)
            try:
                r, d = counters_of(lambda: run(m, case, legs, lens, these, S16))
                assert r.rc == 0 and r.bus_frames == frames and r.used == list(used)
                assert (d["transfers_in"], d["transfers_out"], d["bus_sum_launches"]) == (1, 1, 1), d
                tm.check_buses(case, S16, INTER, r.got, z, dm.NONE, 0, "small tick")
                got.append(r.got.tobytes())
            finally:
                m.close()
                tm.close_all(legs)
        assert got[0] == got[1]
    finally:
        for b in blocks:
            b.close()


# ---- H. slots, modes, control calls ----------------------------------------------------------------------------------------------
SIX_KEY = (1, 16000, 48000, 5)


def six(seed=1100):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.5, 1.5, (6, 6)).astype(np.float32)
    assert not np.array_equal(w, w.T)
    case = tm.Case(1, [SIX_KEY] * 6, [S16] * 6, w)
    x = [tm.raw_of(S16, 640, seed + 1 + i) for i in range(6)]     # per STATE: two ticks of 320 frames
    half = lambda i, t: x[i][t * 640: (t + 1) * 640]
    return case, half


@pytest.mark.parametrize("fmt", (F32, S16))
def test_the_caller_names_the_state_in_every_slot_with_every_call(fmt):
    case, half = six()
    states, twins = case.states(), case.states()
    m = tm.mixer_of(case)
    try:
        models = [gm.State() for _ in range(6)]
        models[1].set(0.3, 1500)        # crosses the ticks, and changes its slot between them
        assert states[1].set_gain(0.3, 1500) == 0
        slots = ([0, 1, 2, 3, 4, 5], [0, 4, None, 3, 1, 5])
        for t, names in enumerate(slots):
            by_slot = lambda things: [None if i is None else things[i] for i in names]
            chunks = [None if i is None else half(i, t) for i in names]
            lens = [0 if i is None else 320 for i in names]
            ys, used = tm.twin_floats(case, by_slot(twins), lens, chunks)
            made = sizes(ys)
            # the weights follow the slots, the gain and the stream position the states
            z, frames = model(case.w, 1, ys, ramps(by_slot(models), made, max(made)))
            r = run(m, case, by_slot(states), lens, chunks, fmt)
            assert r.rc == 0 and r.codes == [0] * 6 and r.made == made and r.used == used and r.bus_frames == frames == 960
            tm.check_buses(case, fmt, INTER, r.got, z, dm.NONE, 0, "tick %d" % t)
        assert models[1].done == 1500 and 0 < models[1].total - 960 < 960
        for i in range(6):
            assert tm.report(states[i]) == models[i].report(), "get_gain of state %d" % i
            assert tm.position_of(states[i]) == tm.position_of(twins[i]), "state %d" % i
    finally:
        m.close()
        tm.close_all(states, twins)


@pytest.mark.parametrize("fmt", (F32, S16))
def test_legs_of_two_modes_in_one_call(fmt):
    case, half = six(1200)
    make = lambda: [speexhip.Resampler(*SIX_KEY, mode=speexhip.MODE_EXACT if i < 3 else None) for i in range(6)]
    legs, twins = make(), make()
    m = tm.mixer_of(case)
    try:
        assert [st.info()["mode"] == speexhip.MODE_EXACT for st in legs] == [True] * 3 + [False] * 3
        chunks, lens = [half(i, 0) for i in range(6)], [320] * 6
        ys, used = tm.twin_floats(case, twins, lens, chunks)
        z, frames = model(case.w, 1, ys)
        r, d = counters_of(lambda: run(m, case, legs, lens, chunks, fmt))
        assert r.rc == 0 and r.made == sizes(ys) and r.used == used and r.bus_frames == frames
        assert d["fir_launches"] == 2 and d["bus_sum_launches"] == 1, d
        tm.check_buses(case, fmt, INTER, r.got, z, dm.NONE, 0, "two modes")
    finally:
        m.close()
        tm.close_all(legs, twins)


def test_a_leg_with_a_control_call_between_two_ticks():
    case, half = six(1300)
    legs, twins = case.states(), case.states()
    m = tm.mixer_of(case)
    try:
        for t in range(2):
            lens = [320] * 6
            if t == 1:      # leg 2 is an 8 kHz leg from here on: 20 ms are 160 frames
                for st in (legs[2], twins[2]):
                    assert st.set_rate(8000, 48000) == 0
                lens[2] = 160
            chunks = [half(i, t) for i in range(6)]
            caps = [1100] * 6
            ys, used = tm.twin_floats(case, twins, lens, chunks, caps)
            made = sizes(ys)
            z, frames = model(case.w, 1, ys)
            r = run(m, case, legs, lens, chunks, S16, caps=caps)
            assert r.rc == 0 and r.made == made and r.used == used and r.bus_frames == frames
            tm.check_buses(case, S16, INTER, r.got, z, dm.NONE, 0, "tick %d" % t)
        print("behind set_rate(8000, 48000) the leg makes %d frames of its 160, the others %d" % (made[2], made[0]))
        assert made[2] > 0 and made[0] == 960
        for i in range(6):
            assert tm.position_of(legs[i]) == tm.position_of(twins[i]), "leg %d" % i
    finally:
        m.close()
        tm.close_all(legs, twins)


def test_set_weights_between_two_ticks_starts_the_buses_again():
    case, half = six(1400)
    kind, fmt = dm.TRIANGULAR, S16
    w2 = np.random.default_rng(1401).uniform(-1.5, 1.5, (6, 6)).astype(np.float32)
    legs, twins = case.states(), case.states()
    m = tm.mixer_of(case, kind, meter=True)
    try:
        for t, (w, position) in enumerate(((case.w, START), (w2, 0))):
            chunks, lens = [half(i, t) for i in range(6)], [320] * 6
            ys, used = tm.twin_floats(case, twins, lens, chunks)
            z, frames = model(w, 1, ys)
            if t == 1:
                states_before = [(tm.position_of(st), tm.report(st)) for st in legs]
                assert m.set_weights(w2) == 0 and np.array_equal(m.get_weights(), w2)
                assert m.get_dither() == (kind, tm.SEED, 0), "set_weights did not zero the bus position, or touched the dither"
                assert [(tm.position_of(st), tm.report(st)) for st in legs] == states_before
            r = run(m, case, legs, lens, chunks, fmt)
            assert r.rc == 0 and r.bus_frames == frames and r.used == used
            tm.check_buses(case, fmt, INTER, r.got, z, kind, position, "tick %d" % t)
            assert m.bus_position() == position + frames
            tm.check_meters(m, case, fmt, z, kind, position, frames, "tick %d" % t)     # (tick 1: its totals alone)
    finally:
        m.close()
        tm.close_all(legs, twins)


# ---- I. the limits ---------------------------------------------------------------------------------------------------------------
LIMIT_FRAMES = 160


@functools.lru_cache(maxsize=None)
def limits_case():
    n = bm.LIMIT
    x = bm.limits_layout(LIMIT_FRAMES).reshape(n, LIMIT_FRAMES, 1)
    keys = [None if i == bm.LIMIT_EMPTY else (1, 8000, 16000, 5) for i in range(n)]
    case = tm.Case(1, keys, [F32] * n, bm.order_weights_legs(n, bm.LIMIT_PAIRS, n))
    chunks = f32_chunks(x)
    chunks[bm.LIMIT_EMPTY] = chunks[bm.LIMIT_SILENT] = None
    lens = tuple(0 if k is None else LIMIT_FRAMES for k in keys)
    ys, used = twins_once(case, lens, chunks)
    assert ys[bm.LIMIT_EMPTY] is None and ys[bm.LIMIT_SILENT].size > 0 and not ys[bm.LIMIT_SILENT].any()
    masks = order_preconditions(case, ys, bm.LIMIT_PAIRS, None)
    z, frames = model(case.w, 1, ys, wide=True)
    assert z[2:5].tobytes() == np.zeros((3, frames), np.float32).tobytes(), "a pair alone is not +0.0"
    assert z[:6].tobytes() == model(case.w[:6], 1, ys)[0].tobytes()
    order_defects(case, ys, z, masks, ("descending",) + bm.LEG_DEFECTS)
    return case, lens, chunks, ys, used, z, frames


@pytest.mark.parametrize("fmt", (S16, F32))
def test_the_limits_1024_slots_and_1024_buses(fmt):
    """The header's limits in one call: 64 blocks of legs, a grid of 32 workgroup rows, 32 launch groups.  Read off
    many_plan.h and host_transfer.h: a call is SMALL -- its kernels read and write the pinned stage, nothing is copied -- when
    its pageable bytes stay under 720 KiB each way.  In: the table of 1024 records of 64 bytes and 1022 payloads of 640
    bytes, 719 616.  Out, the buses on whole 64-sample runs: 655 360 bytes of S16 -- small -- and 1 310 720 of F32 -- not
    small, the stage is copied each way.  The counters are the same either way: the stage is the one transfer."""
    case, lens, chunks, ys, used, z, frames = limits_case()
    assert case.n == speexhip.MIXER_MAX_LEGS and case.n_buses == speexhip.MIXER_MAX_BUSES
    bytes_in, bytes_out = 64 * case.n + sum(c.size for c in chunks if c is not None), case.n_buses * 320 * hm.nbytes(fmt)
    assert bytes_in < 720 * 1024 and (bytes_out < 720 * 1024) == (fmt == S16) and frames == 320
    legs, m = case.states(), tm.mixer_of(case)
    try:
        r, d = counters_of(lambda: run(m, case, legs, lens, chunks, fmt))
        assert r.rc == 0 and r.codes == [0] * case.n and r.used == list(used)
        assert r.bus_frames == frames and r.made == sizes(ys)
        assert d["bus_sum_launches"] == 1 and d["transfers_in"] == 1 and d["transfers_out"] == 1, d
        assert d["out_passes"] == (0 if fmt == F32 else 32) and d["fir_launches"] == 32, d
        tm.check_buses(case, fmt, INTER, r.got, z, dm.NONE, 0, "limits format %d" % fmt)
    finally:
        m.close()
        tm.close_all(legs)
