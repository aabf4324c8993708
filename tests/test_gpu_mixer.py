"""The mixer (include/speexhip_resampler.h, "Mixer") on the GPU, by the discipline of test_gpu_bus.py: the expected bytes
never come from the call under test.  A TWIN state per leg runs the same input through speexhip_resampler_process_many_sides
with F32 interleaved out and no gain -- an existing path; in the default mode a stream's floats do not depend on what
shares its launch -- gain_model.py multiplies the twin's floats by g of each output frame, bus_model.py sums the slots in
float64 in ascending order (+0.0 for an empty slot, a refused leg and behind a leg's end), halfbe_model.py and
dither_model.py encode the buses with the dither of the bus seeds at the bus position, meter_model.py judges them.  Bytes,
totals, positions, counters and the bits of get_gain are compared for EQUALITY.

The one allowance, the one test_gpu_bus.py documents: for the float output formats, where the model's value is NaN the
library's must be a NaN and its bits are not compared.

Shapes, the smallest that reach every branch.
  "tick": mono, 41 slots x 41 buses, mix-minus -- past one pack of 32 on both sides, three blocks of 16 legs with a ragged
    last one, two groups of 32 buses with a ragged group of ONE bus (and three waves without any); one 20 ms tick per leg,
    the legs cycling through 8k -> 48k q7 mu-law, 8k -> 48k q5 A-law, 16k -> 48k q7 S16BE, 44.1k -> 48k q7 S16 and
    48k -> 48k q3 F32N (160, 160, 320, 882, 960 frames); slot 7 empty, slot 9 present and silent.  Finite inputs, no NaN
    in the model.  Every ratio turns its 20 ms into exactly 960 frames, on the first call as on every other -- a state
    produces from its first input frame on, whatever its filter's length (asserted: it is the library's and the
    reference's counter rule) -- so in that call no leg ends before the bus does.  A SECOND call of the same mixer is
    therefore part of the case: the 44.1k legs bring 10 ms (441 frames, 480 out), everybody else 20 ms; its produced differ
    between the ratios (asserted), so legs end before the bus does, in launch groups of mixed lengths.
  "wide": stereo, 34 legs x 3 buses, all 44.1k -> 48k q7, 3000 frames, leg 1 fed 2990, F32 in -- about 6530 samples a leg:
    whole 128-sample tiles and a tail; one NaN in leg 0 channel 0 and one +inf in leg 2 channel 1, placed as in
    test_gpu_bus.py: each spreads over about 70 of about 3265 frames of one channel, about 1.1 % of a bus's samples; at
    most 5 % of any bus is NaN in the model (asserted)."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bus_model as bm
import dither_model as dm
import gain_model as gm
import halfbe_model as hm
import meter_model as mm
import speexhip
from golden_util import ROOT
from test_gpu_bus import FLOATS, SEED, as_layout, encode, same_storage

pytestmark = pytest.mark.gpu

F32, F32N, S16, U8, S24 = speexhip.FMT_F32, speexhip.FMT_F32N, speexhip.FMT_S16, speexhip.FMT_U8, speexhip.FMT_S24
ULAW, ALAW, S16BE, F16N = speexhip.FMT_ULAW, speexhip.FMT_ALAW, speexhip.FMT_S16BE, speexhip.FMT_F16N
INTER, PLANAR = speexhip.LAYOUT_INTERLEAVED, speexhip.LAYOUT_PLANAR
START = 4242
OUT_RATE = 48000
N = 41
# the tick's leg kinds: (in_rate, quality, input format, frames of one 20 ms tick)
KINDS = ((8000, 7, ULAW, 160), (8000, 5, ALAW, 160), (16000, 7, S16BE, 320), (44100, 7, S16, 882), (48000, 3, F32N, 960))
EMPTY, SILENT = 7, 9


def raw_of(fmt, samples, seed):
    """`samples` finite samples of format fmt as raw bytes: any bytes for the integer and companded formats, audio-sized
    values for the float ones"""
    rng = np.random.RandomState(seed)
    if fmt in (F32, F32N):
        v = (rng.standard_normal(samples) * 6000.0).astype(np.float32)
        return (v if fmt == F32 else v / np.float32(32768.0)).view(np.uint8).copy()
    return rng.randint(0, 256, samples * speexhip.fmt_bytes(fmt)).astype(np.uint8)


class Case:
    """the slots of one mixer: key[i] = (channels, in_rate, out_rate, quality) or None, the input format and the chunks of
    every call (None: a silent leg of lens[i] frames)"""

    def __init__(self, ch, keys, fmts, w):
        self.ch, self.keys, self.fmts, self.w = ch, keys, fmts, np.ascontiguousarray(w, np.float32)
        self.n, self.n_buses = len(keys), self.w.shape[0]

    def states(self, mode=None):
        return [None if k is None else speexhip.Resampler(*k, mode=mode) for k in self.keys]

    def caps(self, lens):
        return [0 if k is None else f * k[2] // k[1] + 64 for k, f in zip(self.keys, lens)]


def close_all(*lists):
    for states in lists:
        for st in states:
            if st is not None:
                st.close()


@functools.lru_cache(maxsize=None)
def tick(call=0):
    """(the case, the lengths and the chunks of call `call`): call 0 a whole tick for everybody, call 1 half a tick for the
    44.1k legs"""
    keys = [None if i == EMPTY else (1, KINDS[i % 5][0], OUT_RATE, KINDS[i % 5][1]) for i in range(N)]
    fmts = [KINDS[i % 5][2] for i in range(N)]
    lens = [0 if i == EMPTY else KINDS[i % 5][3] // (2 if call == 1 and i % 5 == 3 else 1) for i in range(N)]
    chunks = [None if i in (EMPTY, SILENT) else raw_of(fmts[i], lens[i], 9000 + 100 * call + i) for i in range(N)]
    for c in chunks:
        if c is not None:
            c.setflags(write=False)
    return Case(1, keys, fmts, bm.mix_minus(N)), tuple(lens), tuple(chunks)


WIDE_LEGS = 34
WIDE_W = np.stack([np.ones(WIDE_LEGS), np.where(np.arange(WIDE_LEGS) % 3 == 1, -0.5, 0.75), 1.0 - (np.arange(WIDE_LEGS) == 2)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide():
    frames = 3000
    keys = [(2, 44100, OUT_RATE, 7)] * WIDE_LEGS
    rng = np.random.default_rng(79)
    x = (rng.uniform(-0.5, 0.5, (WIDE_LEGS, frames, 2)) * 32767.0).astype(np.float32)
    x[0, frames // 8, 0] = np.nan
    x[2, frames - frames // 16, 1] = np.inf
    x.setflags(write=False)
    lens = [frames] * WIDE_LEGS
    lens[1] = 2990
    return Case(2, keys, [F32] * WIDE_LEGS, WIDE_W), tuple(lens), x


def wide_chunks(lo, hi):
    case, lens, x = wide()
    cut = [max(0, min(f, hi) - lo) for f in lens]
    return cut, [np.ascontiguousarray(x[i, lo: lo + cut[i]]).view(np.uint8).reshape(-1) for i in range(WIDE_LEGS)]


def twin_floats(case, twins, lens, chunks, caps=None):
    """per slot the flat interleaved float32 result of the slot's input in its ungained twin, through
    speexhip_resampler_process_many_sides with F32 out (None for a slot without a twin); (floats, consumed)"""
    caps = case.caps(lens) if caps is None else caps
    idx = [i for i, t in enumerate(twins) if t is not None]
    outs = {i: np.zeros(max(caps[i], 1) * case.ch, np.float32) for i in idx}
    a = [speexhip.make_side(case.fmts[i], case.ch, data=None if chunks[i] is None else chunks[i].ctypes.data) for i in idx]
    b = [speexhip.make_side(F32, case.ch, data=outs[i].ctypes.data) for i in idx]
    rc, used, made, codes = speexhip.process_many_sides([twins[i] for i in idx], a, [lens[i] for i in idx], b, [caps[i] for i in idx])
    assert rc in (0, speexhip.ERR_ALLOC_FAILED), rc
    ys, consumed = [None] * case.n, [0] * case.n
    for k, i in enumerate(idx):
        ys[i] = outs[i][: made[k] * case.ch].copy()
        consumed[i] = used[k]
    return ys, consumed


@functools.lru_cache(maxsize=None)
def tick_floats():
    """the twins' floats and consumed frames of the tick's two calls: ((ys, used), (ys, used))"""
    twins = tick()[0].states()
    calls = []
    try:
        for call in range(2):
            case, lens, chunks = tick(call)
            ys, used = twin_floats(case, twins, lens, chunks)
            for y in ys:
                if y is not None:
                    y.setflags(write=False)
            calls.append((tuple(ys), tuple(used)))
    finally:
        close_all(twins)
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def wide_floats():
    case, lens, x = wide()
    twins = case.states()
    try:
        ys, used = twin_floats(case, twins, lens, wide_chunks(0, 3000)[1])
    finally:
        close_all(twins)
    for y in ys:
        y.setflags(write=False)
    return tuple(ys), tuple(used)


def model_buses(case, ys, gains=None, nan_ok=False):
    """(n_buses, bus_frames * ch) float32 of the slots' floats ys (None: +0.0 throughout), slot i behind gains[i]"""
    ch = case.ch
    gained = [np.zeros(0, np.float32) if y is None else y if gains is None or gains[i] is None else gm.apply(y, gains[i], ch)
              for i, y in enumerate(ys)]
    frames = max(y.size for y in gained) // ch
    z = bm.buses(case.w, bm.pad(gained, frames, ch))
    if nan_ok:
        assert np.isnan(z).any(), "the buses hold no NaN"
        assert all(np.isnan(zj).mean() <= 0.05 for zj in z), "more than 5 % of a bus is NaN in the model"
    else:
        assert not np.isnan(z).any(), "a finite input made a NaN in the model"
    return z, frames


def mixer_of(case, kind=dm.NONE, meter=False, position=START):
    m = speexhip.Mixer(case.n, case.n_buses, case.ch)
    if meter:
        assert m.set_meter(1) == 0
    assert m.set_weights(case.w) == 0
    if kind != dm.NONE:
        assert m.set_dither(kind, SEED, position) == 0     # (behind set_weights, which zeroes the bus position)
    return m


def mix(m, case, legs, lens, chunks, fmt, layout=INTER, caps=None):
    """one mixer call: (the buses' bytes (n_buses, bytes) -- planar: plane after plane --, bus_frames, used, made, codes)"""
    caps = case.caps(lens) if caps is None else caps
    cap_arg = [(lens[i], caps[i]) if chunks[i] is None else caps[i] for i in range(case.n)]
    buses, bus_frames, used, made, codes = m.process(legs, chunks, case.fmts, fmt, cap_arg, "planar" if layout == PLANAR else "interleaved")
    return np.ascontiguousarray(buses).view(np.uint8).reshape(case.n_buses, -1), bus_frames, used, made, codes


def check_buses(case, fmt, layout, got, z, kind, position, what):
    for j in range(case.n_buses):
        want = as_layout(fmt, encode(fmt, z[j], kind, case.ch, case.n, j, position), case.ch, layout)
        same_storage(fmt, got[j], want, z[j], case.ch, layout, "%s bus %d" % (what, j))


def check_meters(m, case, fmt, z, kind, position, bus_frames, what):
    clipped = 0
    for j in range(case.n_buses):
        d = dm.values(kind, dm.stream_seed(SEED, case.n + j), position * case.ch, z[j].size) if mm.clips(fmt) and kind != dm.NONE else None
        want = mm.totals(fmt, z[j], d)
        got = m.get_bus_meter(j)
        assert got.pop("on") is True and mm.same(got, want), "%s bus %d: meter %r, model %r" % (what, j, got, want)
        assert got["samples"] == bus_frames * case.ch
        clipped += want["clipped_high"] + want["clipped_low"]
    return clipped


def position_of(st):
    i = st.info()
    return (i["last_sample"], i["samp_frac_num"], i["magic_samples"], st._lines().tobytes())


# ---- 1. the tick: five kinds of leg, 41 x 41, every output format ------------------------------------------------------
@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("u8", INTER), ("ulaw", INTER), ("s24", PLANAR), ("f32", INTER), ("f16n", INTER)))
def test_a_tick_of_mixed_legs_equals_the_model_on_the_twins_floats(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, lens, chunks = tick()
    ys, twin_used = tick_floats()[0]
    z, frames = model_buses(case, ys)
    made_want = [0 if y is None else y.size for y in ys]
    # (module docstring: every ratio makes 960 frames of its first 20 ms; the second call below is the ragged one)
    assert [made_want[i] for i in range(N) if i != EMPTY] == [960] * (N - 1) and frames == 960
    assert not ys[SILENT].any() and ys[SILENT].size > 0
    legs, m = case.states(), mixer_of(case)
    try:
        c0 = speexhip.debug_mixer_counters()
        got, bus_frames, used, made, codes = mix(m, case, legs, lens, chunks, fmt, layout)
        c1 = speexhip.debug_mixer_counters()
        assert codes == [0] * N and bus_frames == frames and made == made_want and used == list(twin_used)
        check_buses(case, fmt, layout, got, z, dm.NONE, 0, "tick " + fmt_name)
        assert m.bus_position() == 0, "the bus position moved without dither"
        # the second call: the 44.1k legs end half way through the bus
        case2, lens2, chunks2 = tick(1)
        ys2, twin_used2 = tick_floats()[1]
        z2, frames2 = model_buses(case, ys2)
        made2 = [0 if y is None else y.size for y in ys2]
        assert len(set(made2[i] for i in range(5))) > 1 and min(v for i, v in enumerate(made2) if i != EMPTY) < frames2, \
            "every leg produced the bus's length: no leg ends before the bus"
        got2, bus_frames2, used2, made_got2, codes2 = mix(m, case, legs, lens2, chunks2, fmt, layout)
        assert codes2 == [0] * N and bus_frames2 == frames2 and made_got2 == made2 and used2 == list(twin_used2)
        check_buses(case, fmt, layout, got2, z2, dm.NONE, 0, "second tick " + fmt_name)
        # counters: one bus-sum launch, one transfer each way, one output pass per 32 buses (none for an interleaved F32
        # side, which the kernel writes itself), one FIR launch per launch group -- a group is up to 32 working legs of one
        # (filter, mode, window format): the five kinds, eight legs each (seven where a slot is empty)
        d = {k: c1[k] - c0[k] for k in c0}
        assert d["bus_sum_launches"] == 1 and d["transfers_in"] == 1 and d["transfers_out"] == 1, d
        assert d["out_passes"] == (0 if fmt == F32 else 2), d
        assert d["fir_launches"] == 5, d
        # four of the five kinds pass through an input image; the silent leg has nothing to convert
        assert d["in_passes"] == 5, d
    finally:
        m.close()
        close_all(legs)


# ---- 2. the wide case: whole tiles and a tail, stereo, NaN and inf ----------------------------------------------------
@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("s24", PLANAR), ("f32", INTER), ("f32", PLANAR)))
def test_wide_stereo_legs_with_tiles_a_tail_and_bad_samples(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, lens, x = wide()
    ys, twin_used = wide_floats()
    z, frames = model_buses(case, ys, nan_ok=True)
    assert ys[1].size < ys[0].size, "leg 1 does not end before the bus"
    assert frames * 2 > 3 * 128 and (frames * 2) % 128 != 0, "no whole tiles and a tail"
    legs, m = case.states(), mixer_of(case)
    try:
        got, bus_frames, used, made, codes = mix(m, case, legs, lens, wide_chunks(0, 3000)[1], fmt, layout)
        assert codes == [0] * WIDE_LEGS and bus_frames == frames and made == [y.size // 2 for y in ys] and used == list(twin_used)
        check_buses(case, fmt, layout, got, z, dm.NONE, 0, "wide %s layout %d" % (fmt_name, layout))
    finally:
        m.close()
        close_all(legs)


# ---- 3. gain ------------------------------------------------------------------------------------------------------------
def report(st):
    g = st.get_gain()
    return (np.float32(g["current"]).tobytes(), np.float32(g["target"]).tobytes(), g["remaining"])


@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("f32", INTER)))
def test_legs_are_gained_before_they_are_summed(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, lens, x = wide()
    ys, _ = wide_floats()
    models = [gm.State() for _ in ys]
    legs, m = case.states(), mixer_of(case)
    try:
        # leg 0: a ramp that ends at an odd frame inside the call; leg 1: muted; leg 33 (the ragged last block of legs): a
        # ramp still in flight at the end of the call; everybody else: off
        for i, (gain, ramp) in {0: (0.3, 1777), 1: (0.0, 0), 33: (2.0, 100000)}.items():
            assert legs[i].set_gain(gain, ramp) == 0
            models[i].set(gain, ramp)
        gains = [mo.take(y.size // 2) if i in (0, 1, 33) else None for i, (mo, y) in enumerate(zip(models, ys))]
        assert (np.diff(gains[0]) != 0).sum() > 1000 and models[0].done == models[0].total and models[33].done < models[33].total
        z, frames = model_buses(case, ys, gains, nan_ok=True)
        got, bus_frames, used, made, codes = mix(m, case, legs, lens, wide_chunks(0, 3000)[1], fmt, layout)
        assert codes == [0] * WIDE_LEGS
        check_buses(case, fmt, layout, got, z, dm.NONE, 0, "gained " + fmt_name)
        for i, mo in enumerate(models):
            assert report(legs[i]) == mo.report(), "get_gain of leg %d after the call" % i
    finally:
        m.close()
        close_all(legs)


# ---- 4. dither and meter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,fmt_name,layout", (("tick", "s16", INTER), ("tick", "ulaw", INTER), ("wide", "u8", PLANAR), ("wide", "f32", INTER)))
def test_buses_are_dithered_from_the_bus_seeds_and_judged_into_their_own_cells(which, fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    kind = dm.TRIANGULAR
    if which == "tick":
        case, lens, chunks = tick()
        ys = tick_floats()[0][0]
    else:
        case, lens, x = wide()
        ys, chunks = wide_floats()[0], wide_chunks(0, 3000)[1]
    z, frames = model_buses(case, ys, nan_ok=which == "wide")
    legs = case.states()
    m = mixer_of(case, kind, meter=True)
    try:
        # the legs' own dither and meter are ON: a mixer call must neither read nor move them
        for i, st in enumerate(legs):
            if st is not None:
                assert st.set_dither(dm.RECTANGULAR, 77 + i, 1000 + i) == 0 and st.set_meter(1) == 0
        assert m.get_dither() == (kind, SEED, START) and m.bus_position() == START
        got, bus_frames, used, made, codes = mix(m, case, legs, lens, chunks, fmt, layout)
        assert bus_frames == frames
        check_buses(case, fmt, layout, got, z, kind, START, "dithered %s %s" % (which, fmt_name))
        assert m.bus_position() == START + bus_frames
        clipped = check_meters(m, case, fmt, z, kind, START, bus_frames, which + " " + fmt_name)
        if mm.clips(fmt):
            assert clipped > 0, "the weights do not sum beyond full scale"
        for i, st in enumerate(legs):
            if st is not None:
                assert st.get_dither() == (dm.RECTANGULAR, 77 + i, 1000 + i), "leg %d: its own dither position moved" % i
                ms = st.get_meter()
                assert ms.pop("on") is True and mm.same(ms, mm.ZERO), "leg %d: its own meter totals moved" % i
        # reset clears that bus only; set_weights zeroes cells, totals and the bus position
        first = m.get_bus_meter(0, reset=True)
        again = m.get_bus_meter(0)
        again.pop("on")
        assert mm.same(again, mm.ZERO) and first["samples"] == bus_frames * case.ch
        assert m.get_bus_meter(1)["samples"] == bus_frames * case.ch
        assert m.set_weights(case.w) == 0 and m.bus_position() == 0
        last = m.get_bus_meter(1)
        last.pop("on")
        assert mm.same(last, mm.ZERO) and np.array_equal(m.get_weights(), case.w)
    finally:
        m.close()
        close_all(legs)


# ---- 5. two calls equal one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("s24", PLANAR), ("f32", INTER)))
def test_two_calls_give_the_bytes_position_and_totals_of_one(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    case, lens, x = wide()
    kind, cut, ch = dm.TRIANGULAR, 1700, 2

    def run(cuts):
        legs = case.states()
        m = mixer_of(case, kind, meter=True)
        try:
            assert legs[1].set_gain(0.25, 2500) == 0     # crosses the boundary between the calls
            pieces, total = [], 0
            for lo, hi in cuts:
                cut_lens, chunks = wide_chunks(lo, hi)
                got, bus_frames, used, made, codes = mix(m, case, legs, cut_lens, chunks, fmt, layout)
                assert codes == [0] * WIDE_LEGS and used == cut_lens
                if (lo, hi) == (0, cut):
                    assert len(set(made)) == 1, "the cut is not where every leg has produced the same count"
                pieces.append(got.reshape(case.n_buses, ch if layout == PLANAR else 1, -1))
                total += bus_frames
            meters = [m.get_bus_meter(j) for j in range(case.n_buses)]
            return np.concatenate(pieces, axis=2).reshape(case.n_buses, -1), total, meters, m.bus_position(), report(legs[1])
        finally:
            m.close()
            close_all(legs)

    one = run(((0, 3000),))
    two = run(((0, cut), (cut, 3000)))
    assert one[1] == two[1] and one[3] == two[3] == START + one[1] and one[4] == two[4]
    ys, _ = wide_floats()
    model = gm.State()
    model.set(0.25, 2500)
    gains = [None] * WIDE_LEGS
    gains[1] = model.take(ys[1].size // ch)
    assert model.report() == one[4]
    z, n = model_buses(case, ys, gains, nan_ok=True)
    assert n == one[1]
    for res, what in ((one, "one call"), (two, "two calls")):
        check_buses(case, fmt, layout, res[0], z, kind, START, what)
        for j in range(case.n_buses):
            d = dm.values(kind, dm.stream_seed(SEED, case.n + j), START * ch, z[j].size) if mm.clips(fmt) else None
            got = dict(res[2][j])
            assert got.pop("on") is True and mm.same(got, mm.totals(fmt, z[j], d)), "%s: bus %d meter" % (what, j)
    assert one[0].tobytes() == two[0].tobytes() or fmt in FLOATS


# ---- 6. every per-leg outcome; the call-level errors ---------------------------------------------------------------------
def test_every_per_leg_outcome_and_a_refused_leg_counts_as_zero():
    """8 slots x 3 buses, mono 16k -> 48k q5 S16: 0 good, 1 empty, 2 a short struct_size, 3 an unknown format, 4 a matrix, 5
    the wrong channel count, 6 named by an earlier slot (slot 0's state), 7 good and gained.  Then, one call each beside a
    good leg: a planar side of two channels, a state whose channel count is not the mixer's, lengths that fail "Extents", a
    state whose channels stand apart, a batch of several streams, the zero fallback.  (A leg on another device: the test
    below, in a process of its own.)"""
    L = speexhip.lib()
    n, frames = 8, 320
    key = (1, 16000, OUT_RATE, 5)
    w = np.array([[1.0] * n, [0.5, 1, 1, 1, 1, 1, 1, -2.0], [0.0] * 7 + [1.0]], np.float32)
    case = Case(1, [key] * n, [S16] * n, w)
    cap = case.caps([frames] * n)[0]
    chunks = [raw_of(S16, frames, 300 + i) for i in range(n)]

    def sides():
        s = [speexhip.make_side(S16, 1, data=chunks[i].ctypes.data) for i in range(n)]
        s[1] = None
        s[2].struct_size = C.sizeof(speexhip.Side) - 8
        s[3].fmt = 99
        mix1 = np.ones((1, 1), np.float32)
        s[4] = speexhip.make_side(S16, 1, mix=mix1, data=chunks[4].ctypes.data)
        s[5].channels = 2
        return s, mix1

    legs, twins = case.states(), case.states()
    m = mixer_of(case)
    out = np.zeros((case.n_buses, cap), np.int16)
    out_side = speexhip.make_side(S16, 1, data=out.ctypes.data, stream_stride=cap)
    try:
        assert legs[7].set_gain(0.5, 0) == 0
        call_legs = list(legs)
        call_legs[1] = None
        call_legs[6] = legs[0]
        before = [position_of(st) for st in legs]
        s, keep = sides()
        rc, used, made, bus_frames, codes = m.process_sides(call_legs, s, [frames] * n, out_side, [cap] * n)
        A = speexhip.ERR_INVALID_ARG
        assert codes == [0, 0, A, A, A, A, A, 0] and rc == A
        for i in (2, 3, 4, 5, 6):
            assert (used[i], made[i]) == (frames, cap), "slot %d: a refused leg's lengths were touched" % i
        assert (used[1], made[1]) == (0, 0), "an empty slot's lengths are not 0"
        for i in (1, 2, 3, 4, 5, 6):
            assert position_of(legs[i]) == before[i], "slot %d: a refused leg's state moved" % i
        ys, twin_used = twin_floats(case, [twins[0]] + [None] * 6 + [twins[7]], [frames] * n, chunks)
        assert (used[0], used[7]) == (twin_used[0], twin_used[7]) and made[0] * 1 == ys[0].size and made[7] == ys[7].size
        gains = [None] * 7 + [gm.g(np.float32(0.5), np.float32(0.5), 0, 0, ys[7].size)]
        z, nf = model_buses(case, ys, gains)
        assert bus_frames == nf
        for j in range(case.n_buses):
            assert out[j, :nf].tobytes() == np.ascontiguousarray(hm.raw(S16, hm.from_internal(S16, z[j]))).tobytes(), "bus %d" % j
        assert position_of(legs[0]) == position_of(twins[0]) and position_of(legs[7]) == position_of(twins[7])
    finally:
        m.close()
        close_all(legs, twins)

    # ---- one leg at a time beside a good one: 2 slots x 1 bus
    small = Case(1, [key, key], [S16, S16], np.ones((1, 2), np.float32))
    good = raw_of(S16, frames, 555)

    def one_bad(bad_leg, bad_side, bad_len, want, runs, silent_twin=None):
        """slot 0 good, slot 1 the leg in question; returns nothing, asserts everything"""
        legs0, twin0 = speexhip.Resampler(*key), speexhip.Resampler(*key)
        mx = mixer_of(small)
        ob = np.zeros((1, cap), np.int16)
        os_ = speexhip.make_side(S16, 1, data=ob.ctypes.data, stream_stride=cap)
        try:
            info_before = bad_leg.info() if hasattr(bad_leg, "info") else None
            rc, used, made, bf, codes = mx.process_sides([legs0, bad_leg], [speexhip.make_side(S16, 1, data=good.ctypes.data), bad_side],
                                                         [frames, bad_len[0]], os_, [cap, bad_len[1]])
            assert codes == [0, want] and rc == want, (codes, rc, want)
            y0, _ = twin_floats(small, [twin0, None], [frames, 0], [good, None])
            if not runs:
                assert (used[1], made[1]) == tuple(bad_len), "a refused leg's lengths were touched"
                if info_before is not None:
                    assert bad_leg.info() == info_before, "a refused leg's state moved"
                ys = [y0[0], None]
            else:
                ys = [y0[0], silent_twin]
            z, nf = model_buses(small, ys)
            assert bf == nf and ob[0, :nf].tobytes() == np.ascontiguousarray(hm.raw(S16, hm.from_internal(S16, z[0]))).tobytes()
        finally:
            mx.close()
            legs0.close()
            twin0.close()

    other = raw_of(S16, 2 * frames, 556)
    # a planar layout of more than one channel (its channel count is not the mixer's either way)
    st = speexhip.Resampler(2, 16000, OUT_RATE, 5)
    try:
        one_bad(st, speexhip.make_side(S16, 2, layout=PLANAR, data=other.ctypes.data, plane_stride=frames), (frames, cap), speexhip.ERR_INVALID_ARG, False)
        # a state whose channel count is not the mixer's, behind a side that claims the mixer's
        one_bad(st, speexhip.make_side(S16, 1, data=other.ctypes.data), (frames, cap), speexhip.ERR_INVALID_ARG, False)
    finally:
        st.close()
    # lengths that fail "Extents"
    st = speexhip.Resampler(*key)
    try:
        one_bad(st, speexhip.make_side(S16, 1, data=other.ctypes.data), (0xFFFFFFF0, 0xFFFFFFF0), speexhip.ERR_OVERFLOW, False)
    finally:
        st.close()
    # a state whose channels the per-channel calls moved apart: BAD_STATE.  (The mixer here is stereo, and the ratio one
    # at which 300 and 150 frames leave two different positions.)
    stereo_key = (2, 44100, OUT_RATE, 5)
    small2 = Case(2, [stereo_key, stereo_key], [S16, S16], np.ones((1, 2), np.float32))
    st, ok, tw = speexhip.Resampler(*stereo_key), speexhip.Resampler(*stereo_key), speexhip.Resampler(*stereo_key)
    mx = mixer_of(small2)
    try:
        xs = (np.arange(600, dtype=np.int16).reshape(300, 2) * 37) % 9000
        st.channel_call("int", 0, xs[:300, 0], 1000)
        st.channel_call("int", 1, xs[:150, 1], 1000)
        assert len(set(st.positions())) == 2, "the channels do not stand apart"
        before = position_of(st)
        ob = np.zeros((1, cap * 2), np.int16)
        os_ = speexhip.make_side(S16, 2, data=ob.ctypes.data, stream_stride=cap * 2)
        a = [speexhip.make_side(S16, 2, data=other.ctypes.data), speexhip.make_side(S16, 2, data=other.ctypes.data)]
        rc, used, made, bf, codes = mx.process_sides([ok, st], a, [frames, frames], os_, [cap, cap])
        assert codes == [0, speexhip.ERR_BAD_STATE] and rc == speexhip.ERR_BAD_STATE and (used[1], made[1]) == (frames, cap)
        assert position_of(st) == before
        y0, _ = twin_floats(small2, [tw, None], [frames, 0], [other, None])
        z, nf = model_buses(small2, [y0[0], None])
        assert bf == nf and ob[0, : nf * 2].tobytes() == np.ascontiguousarray(hm.raw(S16, hm.from_internal(S16, z[0]))).tobytes()
    finally:
        mx.close()
        close_all([st, ok, tw])
    # a batch of several streams in a slot (the two handle types wrap the same object: the library must refuse, not run it)
    b = speexhip.Batch(2, 1, 16000, OUT_RATE, 5)
    try:
        one_bad(b, speexhip.make_side(S16, 1, data=other.ctypes.data), (frames, cap), speexhip.ERR_INVALID_ARG, False)
    finally:
        b.close()
    # the zero fallback: runs -- counters move, zeros are summed -- and reports ALLOC_FAILED as in every call
    st, tw = speexhip.Resampler(*key), speexhip.Resampler(*key)
    try:
        for s_ in (st, tw):
            L.speexhip_debug_fail_device_allocs(1)
            rc = s_.set_rate(32000, OUT_RATE)
            L.speexhip_debug_fail_device_allocs(0)
            assert rc == speexhip.ERR_ALLOC_FAILED
        yz, used_z = twin_floats(small, [None, tw], [0, frames], [None, other[: frames * 2]], caps=[0, cap])
        assert yz[1].size > 0 and not yz[1].any()
        legs0, twin0 = speexhip.Resampler(*key), speexhip.Resampler(*key)
        mx = mixer_of(small)
        try:
            ob = np.zeros((1, cap), np.int16)
            os_ = speexhip.make_side(S16, 1, data=ob.ctypes.data, stream_stride=cap)
            a = [speexhip.make_side(S16, 1, data=good.ctypes.data), speexhip.make_side(S16, 1, data=other.ctypes.data)]
            rc, used, made, bf, codes = mx.process_sides([legs0, st], a, [frames, frames], os_, [cap, cap])
            assert codes == [0, speexhip.ERR_ALLOC_FAILED] and rc == speexhip.ERR_ALLOC_FAILED
            assert used[1] == used_z[1] and made[1] == yz[1].size and position_of(st) == position_of(tw)
            y0, _ = twin_floats(small, [twin0, None], [frames, 0], [good, None])
            z, nf = model_buses(small, [y0[0], yz[1]])
            assert bf == nf and ob[0, :nf].tobytes() == np.ascontiguousarray(hm.raw(S16, hm.from_internal(S16, z[0]))).tobytes()
        finally:
            mx.close()
            legs0.close()
            twin0.close()
    finally:
        L.speexhip_debug_fail_device_allocs(0)
        st.close()
        tw.close()


def test_call_level_errors_leave_everything_untouched_and_init_refuses_its_limits():
    L = speexhip.lib()
    for args in ((1025, 1, 1), (0, 1, 1), (1, 1025, 1), (1, 0, 1), (1, 1, 0), (1, 1, 9)):
        err = C.c_int(0)
        assert not L.speexhip_mixer_init(*args, C.byref(err)) and err.value == speexhip.ERR_INVALID_ARG, args
    with pytest.raises(ValueError):
        speexhip.Mixer(1025, 2, 1)
    n, frames = 3, 320
    key = (1, 16000, OUT_RATE, 5)
    case = Case(1, [key] * n, [S16] * n, bm.mix_minus(n))
    cap = case.caps([frames] * n)[0]
    chunks = [raw_of(S16, frames, 40 + i) for i in range(n)]
    legs = case.states()
    m = speexhip.Mixer(n, n, 1)
    out = np.zeros((n, cap), np.int16)
    try:
        sides = [speexhip.make_side(S16, 1, data=c.ctypes.data) for c in chunks]
        good_out = speexhip.make_side(S16, 1, data=out.ctypes.data, stream_stride=cap)
        before = [position_of(st) for st in legs]

        def refused(code, out_side, what, null=None):
            hs = (C.c_void_p * n)(*[st._h for st in legs])
            a = (speexhip.Side * n)()
            for i in range(n):
                C.memmove(C.byref(a[i]), C.byref(sides[i]), C.sizeof(speexhip.Side))
            il, ol, codes = (C.c_uint32 * n)(*([frames] * n)), (C.c_uint32 * n)(*([cap] * n)), (C.c_int * n)(*([-7] * n))
            bf = C.c_uint32(12345)
            args = {"m": m._h, "legs": hs, "in": a, "in_len": il, "out_len": ol, "out": None if out_side is None else C.byref(out_side),
                    "bus_frames": C.byref(bf), "codes": codes}
            if null is not None:
                args[null] = None
            rc = L.speexhip_mixer_process(*[args[k] for k in ("m", "legs", "in", "in_len", "out_len", "out", "bus_frames", "codes")])
            assert rc == code, "%s: code %d" % (what, rc)
            assert list(il) == [frames] * n and list(ol) == [cap] * n and bf.value == 12345 and list(codes) == [-7] * n, what + ": touched"
            assert [position_of(st) for st in legs] == before, what + ": a state moved"

        refused(speexhip.ERR_BAD_STATE, good_out, "no weights set")
        bad = case.w.copy()
        bad[1, 2] = np.inf
        assert m.set_weights(bad) == speexhip.ERR_INVALID_ARG and m.get_weights() is None
        refused(speexhip.ERR_BAD_STATE, good_out, "still no weights")
        assert m.set_weights(case.w) == 0
        bad[1, 2] = np.nan
        assert m.set_weights(bad) == speexhip.ERR_INVALID_ARG and np.array_equal(m.get_weights(), case.w)   # the mixer as it was
        for name in ("m", "legs", "in", "in_len", "out_len", "out", "bus_frames"):
            refused(speexhip.ERR_INVALID_ARG, good_out, "NULL " + name, null=name)
        mix1 = np.ones((1, 1), np.float32)
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(S16, 1, mix=mix1, data=out.ctypes.data, stream_stride=cap), "out->mix")
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(S16, 2, data=out.ctypes.data, stream_stride=cap), "out channels")
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(99, 1, data=out.ctypes.data, stream_stride=cap), "out format")
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(S16, 1, layout=7, data=out.ctypes.data, stream_stride=cap), "out layout")
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(S16, 1, data=None, stream_stride=cap), "out data NULL")
        short = speexhip.make_side(S16, 1, data=out.ctypes.data, stream_stride=cap)
        short.struct_size -= 8
        refused(speexhip.ERR_INVALID_ARG, short, "out struct_size")
        planes = (C.c_void_p * 1)(out.ctypes.data)
        refused(speexhip.ERR_INVALID_ARG, speexhip.make_side(S16, 1, layout=PLANAR, data=out.ctypes.data, stream_stride=cap, planes=planes),
                "out planes")
        # NULL weights turn the mixer off; and the call still works afterwards, on the states the refused ones left
        assert m.set_weights(None) == 0 and m.get_weights() is None
        refused(speexhip.ERR_BAD_STATE, good_out, "turned off")
        assert m.set_weights(case.w) == 0
        rc, used, made, bf, codes = m.process_sides(legs, sides, [frames] * n, good_out, [cap] * n)
        assert rc == 0 and codes == [0] * n and bf == max(made) > 0
        # codes may be NULL
        hs = (C.c_void_p * n)(*[st._h for st in legs])
        a = (speexhip.Side * n)()
        for i in range(n):
            C.memmove(C.byref(a[i]), C.byref(sides[i]), C.sizeof(speexhip.Side))
        il, ol, bfc = (C.c_uint32 * n)(*([frames] * n)), (C.c_uint32 * n)(*([cap] * n)), C.c_uint32(0)
        assert L.speexhip_mixer_process(m._h, hs, a, il, ol, C.byref(good_out), C.byref(bfc), None) == 0 and bfc.value > 0
    finally:
        m.close()
        close_all(legs)


def test_a_leg_on_another_device_is_refused():
    """needs two logical devices: a child process with SPEEXHIP_ALIAS_DEVICES=2 (this box's one GPU twice)"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import speexhip
m = speexhip.Mixer(2, 1, 1, device=0)
assert m.set_weights(np.ones((1, 2), np.float32)) == 0
a, b = speexhip.Resampler(1, 16000, 48000, 5, device=0), speexhip.Resampler(1, 16000, 48000, 5, device=1)
assert a.info()["device"] == 0 and b.info()["device"] == 1
x = (np.arange(320) %% 100).astype(np.int16)
before = b.info()
buses, bus_frames, used, made, codes = m.process([a, b], [x, x], speexhip.FMT_S16, speexhip.FMT_S16, 1100)
assert codes == [0, speexhip.ERR_INVALID_ARG], codes
assert (used[1], made[1]) == (320, 1100) and b.info() == before and bus_frames == made[0] > 0
print("other device ok")
''' % os.path.join(ROOT, "node-speex-resampler_amd", "python")
    env = dict(os.environ, SPEEXHIP_ALIAS_DEVICES="2")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and "other device ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]


# ---- 7. existing calls unchanged ------------------------------------------------------------------------------------------
def test_a_legs_own_sides_call_after_mixer_calls_equals_an_untouched_twin():
    """a leg that has been through two mixer calls and a twin that has been through the same input by process_many_sides
    are the same state: the next process_sides call of each gives the same bytes, dither included"""
    case, lens, chunks = tick()
    legs, twins = case.states(), case.states()
    m = mixer_of(case)
    try:
        for st in legs + twins:
            if st is not None:
                assert st.set_dither(dm.TRIANGULAR, 99, 5) == 0
        for step in range(2):
            got, bus_frames, used, made, codes = mix(m, case, legs, lens, chunks, S16)
            ys, twin_used = twin_floats(case, twins, lens, chunks)
            assert codes == [0] * N and used == twin_used and made == [0 if y is None else y.size for y in ys]
        for i in (0, 1, 2, 3, 4, SILENT, 40):
            # (the twins' F32 results moved their dither positions; a leg's did not move: set both where the twin's is)
            pos = twins[i].get_dither()[2]
            assert legs[i].get_dither() == (dm.TRIANGULAR, 99, 5) and legs[i].set_dither(dm.TRIANGULAR, 99, pos) == 0
            assert position_of(legs[i]) == position_of(twins[i]), i
            x = raw_of(S16, 500, 1234 + i).view(np.int16)
            a, _ = legs[i].process_sides(x.reshape(-1, 1), S16, U8, 4000)
            b, _ = twins[i].process_sides(x.reshape(-1, 1), S16, U8, 4000)
            assert a.size > 0 and a.tobytes() == b.tobytes(), "leg %d" % i
    finally:
        m.close()
        close_all(legs, twins)


# ---- 8. Node --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_mixer():
    pkg = os.path.join(ROOT, "node-speex-resampler_amd")
    run = subprocess.run(["node", os.path.join(pkg, "test", "test_mixer.js")], capture_output=True, text=True, timeout=300, cwd=pkg)
    assert run.returncode == 0 and "mixer ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
