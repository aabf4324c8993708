"""The bus call held to its header (include/speexhip_resampler.h, "Buses") where test_gpu_bus.py's noise cannot: the order
of the sum, the gain's ramp inside bus_sum at odd channel counts, the shapes nobody ran, and the promises without a test.
The method is test_gpu_bus.py's.  Expected bytes never come from the code under test: an ungained twin batch without
buses gives each stream's float32 image through process_sides_device in the same mode and through the same control calls,
gain_model / bus_model / halfbe_model / dither_model / meter_model do the rest, and bytes, totals, positions and get_gain
bits are compared for equality.  No tolerance.  The one allowance is test_gpu_bus.py's, unchanged (same_storage: for the
float formats a model NaN is matched by any NaN), and only the runs on its stereo input use it -- the zero weight on the
infinite stream and the mode runs -- under its condition that at most 5 % of a bus is NaN in the model.  Every other input
is finite and the model asserts that it made no NaN.

What a wrong kernel would have to change is PLANTED in the model first (bus_model.buses(defect=), the ramp defects below)
and must change the model's output on the twin's floats of the very case -- a condition, not a tolerance: a case that
cannot tell the defect from the rule fails instead of passing.  Measured shares: DESIGN.md section 4.

Every output buffer is filled with Resampler.SENTINEL_BYTE; behind bus_frames of every bus and plane, and between the
buses' strides, it must still be there after the call.  Interleaved F32 buses are written by bus_sum itself, straight
into the caller's buffer: `aligned` strides (a multiple of four samples: the 16-byte store of whole tiles on every bus)
and strides one sample off (the element path on every odd bus) are both run.

Shapes (the sizes, the smallest that reach the branch): order -- mono 8k -> 16k q7, 32 streams x 4 buses, 400 frames;
signs -- 2 streams, the first fed nothing; triple -- 3 channels 16k -> 48k q5, 1500 frames, 5 streams fed (1500, 1500,
1201, 0, 1500): 1024 mod 3 = 1, so every tile starts in another channel and every lane's four samples straddle frames;
six -- 6 channels 44.1k -> 48k q5, 400 frames, 2 streams x 11 buses: 1024 mod 6 = 4, more buses than streams, a second
bus group of 3; solo 1 x 1; nine 2 x 9; matrix -- 4 mono streams 48k -> 16k q5 fed stereo S16 planes through [[0.5, 0.5]]."""
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

pytestmark = pytest.mark.gpu

F32, S16, ULAW = tb.F32, tb.S16, tb.ULAW
INTER, PLANAR = tb.INTER, tb.PLANAR
SEED, START = tb.SEED, tb.START
SENT = speexhip.Resampler.SENTINEL_BYTE
TILE = 1024          # samples of a bus_sum workgroup, four per lane

Case = collections.namedtuple("Case", "name ch fi fo q frames fed w x in_fmt in_layout in_mix")

SIGNS_W = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
INF_W = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
TRIPLE_FED = (1500, 1500, 1201, 0, 1500)
IN_MIX = np.array([[0.5, 0.5]], np.float32)


def _noise(seed, shape, scale=0.9):
    return (np.random.default_rng(seed).uniform(-scale, scale, shape) * 32767.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(4711)
    if name == "order":
        x = bm.order_layout(400).reshape(bm.ORDER_STREAMS, 400, 1)
        c = Case(name, 1, 8000, 16000, 7, 400, (400,) * 32, bm.ORDER_W, x, F32, INTER, None)
    elif name == "signs":
        c = Case(name, 1, 8000, 16000, 7, 160, (0, 160), SIGNS_W, _noise(1, (2, 160, 1)), F32, INTER, None)
    elif name in ("stereo", "inf"):
        ch, fi, fo, q, frames, fed, w = tb.CASES["stereo"]
        c = Case(name, ch, fi, fo, q, frames, fed, INF_W if name == "inf" else w, tb.noise("stereo"), F32, INTER, None)
    elif name == "triple":
        c = Case(name, 3, 16000, 48000, 5, 1500, TRIPLE_FED, tb.TRIPLE_W, tb.noise("triple"), F32, INTER, None)
    elif name == "six":
        w = rng.uniform(-1.5, 1.5, (11, 2)).astype(np.float32)
        w[4] = 0.0
        c = Case(name, 6, 44100, 48000, 5, 400, (400, 400), w, _noise(2, (2, 400, 6)), F32, INTER, None)
    elif name == "solo":
        c = Case(name, 1, 8000, 16000, 7, 160, (160,), np.array([[-0.5]], np.float32), _noise(3, (1, 160, 1)), F32, INTER, None)
    elif name == "nine":
        w = rng.uniform(-1.5, 1.5, (9, 2)).astype(np.float32)
        c = Case(name, 1, 8000, 16000, 7, 160, (160, 160), w, _noise(4, (2, 160, 1)), F32, INTER, None)
    elif name == "matrix":
        w = rng.uniform(-1.5, 1.5, (3, 4)).astype(np.float32)
        c = Case(name, 1, 48000, 16000, 5, 480, (480,) * 4, w, _noise(5, (4, 480, 2)), S16, PLANAR, IN_MIX)
    elif name == "mono":
        ch, fi, fo, q, frames, fed, w = tb.CASES["mono"]
        c = Case(name, ch, fi, fo, q, frames, fed, w, tb.noise("mono"), F32, INTER, None)
    else:
        raise KeyError(name)
    assert c.x.shape[:2] == (len(c.fed), c.frames) and c.w.shape[1] == len(c.fed)
    if name not in ("stereo", "inf"):
        assert np.isfinite(c.x).all()
    return c


def make(c, mode=None, kind=dm.NONE, meter=False, w=None, buses=True):
    b = speexhip.Batch(len(c.fed), c.ch, c.fi, c.fo, c.q, mode=mode)
    if kind != dm.NONE:
        assert b.set_dither(kind, SEED, START) == 0
    if meter:
        assert b.set_meter(1) == 0
    if buses:
        assert b.set_buses(c.w if w is None else w) == 0
        if kind != dm.NONE:     # (set_buses zeroed the bus position)
            assert b.bus_position() == 0 and b.set_dither(kind, SEED, START) == 0 and b.bus_position() == START
    return b


def lens_of(c, lo, hi):
    return [max(0, min(f, hi) - lo) for f in c.fed]


def in_side_of(c, lo, hi):
    """the input side of frames [lo, hi) of the case: its Side and the tensor that owns the bytes"""
    import torch
    x = c.x[:, lo:hi]
    S, frames, n_in = x.shape
    arranged = x if c.in_layout == INTER else np.ascontiguousarray(x.transpose(0, 2, 1))
    raw = hm.raw(c.in_fmt, hm.from_internal(c.in_fmt, arranged.reshape(-1)))
    t = torch.from_numpy(raw.copy()).cuda()
    return speexhip.make_side(c.in_fmt, n_in, c.in_layout, c.in_mix, t.data_ptr(), frames, frames * n_in), t


def float_call(t, c, lo=0, hi=None, lens=None, cap=None):
    """one sides call, F32 out, of the twin t over frames [lo, hi): the flat interleaved floats of every stream"""
    hi = c.frames if hi is None else hi
    lens = lens_of(c, lo, hi) if lens is None else list(lens)
    cap = tb.wcap(hi - lo, c.fi, c.fo) if cap is None else cap
    in_side, keep = in_side_of(c, lo, hi)
    out_side, buf = tb.out_buffer(F32, len(c.fed), cap, c.ch, INTER)
    used, made = t.process_sides_device(in_side, lens, out_side, cap)
    assert used == lens
    raw = tb.fetched(F32, buf, len(c.fed), cap, c.ch, INTER, max(made))
    outs = [raw[s, : made[s] * c.ch * 4].copy().view(np.float32) for s in range(len(c.fed))]
    for y in outs:
        y.setflags(write=False)
    return outs


@functools.lru_cache(maxsize=None)
def twin(name, mode=None):
    """the case's whole input through a fresh ungained twin without buses, in `mode`.  Computed once."""
    c = case(name)
    t = make(c, mode, buses=False)
    try:
        return tuple(float_call(t, c))
    finally:
        t.close()


# ---- the model ------------------------------------------------------------------------------------------------------------
def frames_of(n_samples, ch, defect=None):
    """the frame whose g multiplies flat sample n of a stream's image -- with one of the kernel's ramp defects planted:
      ignores_r0    the frame of sample i of a tile taken as tile0 // C + i // C: the tile's first channel forgotten
      group_first   g of the first of a lane's four samples used for all four"""
    n = np.arange(n_samples)
    if defect == "ignores_r0":
        tile0 = n // TILE * TILE
        return tile0 // ch + (n - tile0) // ch
    if defect == "group_first":
        return (n // 4 * 4) // ch
    assert defect in (None, "past_end"), defect
    return n // ch


def gained_rows(c, ys, gfull, frames, defect=None):
    """(n_streams, frames * ch) float32: every stream behind its gain (gfull[s]: g of each of the bus's frames, None: off),
    +0.0f behind its end -- with "past_end" planted, the product of +0.0f and g there instead"""
    rows = np.zeros((len(ys), frames * c.ch), np.float32)
    for s, y in enumerate(ys):
        if gfull is None or gfull[s] is None:
            rows[s, : y.size] = y
            continue
        g = np.asarray(gfull[s], np.float32)
        assert g.shape == (frames,)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            rows[s, : y.size] = y * g[frames_of(y.size, c.ch, defect)]
            if defect == "past_end":
                rows[s, y.size:] = np.float32(0.0) * g[frames_of(frames * c.ch, c.ch)[y.size:]]
    return rows


def model(c, ys, gfull=None, w=None, defect=None, gain_defect=None, nan_ok=False):
    """(n_buses, bus_frames * ch) float32 of the twin's floats ys, and bus_frames"""
    frames = max(y.size for y in ys) // c.ch
    rows = gained_rows(c, ys, gfull, frames, gain_defect)
    live = bm.live_of([y.size for y in ys], frames * c.ch)
    z = bm.buses(c.w if w is None else w, rows, defect, live)
    if defect is None and gain_defect is None:
        if nan_ok:
            assert np.isnan(z).any(), "the buses hold no NaN"
            assert all(np.isnan(zj).mean() <= 0.05 for zj in z), "more than 5 % of a bus is NaN in the model"
        else:
            assert not np.isnan(z).any(), "a finite input made a NaN in the model"
    return z, frames


def ramps(models, made, frames):
    """g of each of the bus's `frames` frames per stream (None: the stream's gain is off), and the models moved by what
    each stream produced"""
    out = []
    for m, n in zip(models, made):
        out.append(None if m.off() else gm.g(m.frm, m.to, m.total, m.done, frames))
        m.take(n)
    return out


def differs(z, want):
    """the largest share of a bus's samples that differ in their bits"""
    return max(bm.changed(a, b) for a, b in zip(z, want))


# ---- the call, into sentinels -------------------------------------------------------------------------------------------
def stride_of(cap, ch, aligned):
    """samples between two buses: the capacity and a gap, a multiple of four samples or one sample off it"""
    stride = cap * ch + 8
    stride += (-stride) % 4
    return stride if aligned else stride + 1


def run(b, c, fmt, layout, lo=0, hi=None, lens=None, aligned=True, cap=None, want_rc=0):
    """one bus call of b over frames [lo, hi) of the case into a buffer of sentinels: (the buses' bytes (n_buses, bytes),
    produced, bus_frames).  Whatever the call did not produce must still hold the sentinel."""
    import torch
    hi = c.frames if hi is None else hi
    lens = lens_of(c, lo, hi) if lens is None else list(lens)
    cap = tb.wcap(hi - lo, c.fi, c.fo) if cap is None else cap
    n_buses, nb = len(b.get_buses()), hm.nbytes(fmt)
    stride = stride_of(cap, c.ch, aligned)
    in_side, keep = in_side_of(c, lo, hi)
    buf = torch.full((n_buses * stride * nb,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out_side = speexhip.make_side(fmt, c.ch, layout, None, buf.data_ptr(), cap, stride)
    rc, used, made, bus_frames = b.bus_call(in_side, lens, out_side, cap)
    torch.cuda.synchronize()
    assert rc == want_rc, "code %d" % rc
    assert used == lens and bus_frames == max(made) <= cap
    raw = buf.cpu().numpy()
    written = np.zeros(raw.size, bool)
    got = []
    for j in range(n_buses):
        base = j * stride * nb
        if layout == INTER or c.ch == 1:
            parts = [(base, bus_frames * c.ch * nb)]
        else:
            parts = [(base + k * cap * nb, bus_frames * nb) for k in range(c.ch)]
        got.append(np.concatenate([raw[a: a + n] for a, n in parts]))
        for a, n in parts:
            written[a: a + n] = True
    stray = np.flatnonzero(~written & (raw != SENT))
    assert stray.size == 0, "%d bytes written outside the buses' frames, the first at byte %d (bus stride %d bytes, %d frames)" % (
        stray.size, stray[0], stride * nb, bus_frames)
    return np.stack(got), made, bus_frames


def check(c, fmt, layout, got, z, what, kind=dm.NONE, position=0):
    assert got.shape[0] == z.shape[0]
    for j in range(z.shape[0]):
        want = tb.as_layout(fmt, tb.encode(fmt, z[j], kind, c.ch, len(c.fed), j, position), c.ch, layout)
        tb.same_storage(fmt, got[j], want, z[j], c.ch, layout, "%s %s bus %d" % (c.name, what, j))


def totals(c, fmt, j, calls, kind):
    """bus j's meter totals over consecutive calls: (z of the call, bus position at its start) each"""
    out = dict(mm.ZERO)
    for z, position in calls:
        d = None
        if mm.clips(fmt) and kind != dm.NONE:
            d = dm.values(kind, dm.stream_seed(SEED, len(c.fed) + j), position * c.ch, z[j].size)
        out = mm.add(out, mm.totals(fmt, z[j], d))
    return out


def check_meters(b, c, fmt, calls, kind, what):
    for j in range(len(b.get_buses())):
        m = b.get_bus_meter(j)
        want = totals(c, fmt, j, calls, kind)
        assert m.pop("on") is True and mm.same(m, want), "%s %s: bus %d meter %r, model %r" % (c.name, what, j, m, want)


def stream_state(b):
    """what a bus-state control call must leave alone: every stream's counters, gain and dither"""
    return [(tuple(sorted(b.info(s).items())), tb.report(b, s), b.get_dither(s), b.lines(s).tobytes()) for s in range(b.n_streams)]


FORMAT_RUNS = ((F32, INTER, True), (F32, INTER, False), (S16, INTER, True))


# ---- A. the order of the sum, signed zeros, 0 * inf ---------------------------------------------------------------------
def test_the_sum_runs_in_ascending_order_in_fp64_with_one_rounding():
    c = case("order")
    ys = twin("order")
    n = ys[0].size
    assert all(y.size == n for y in ys) and n > 700
    # the layout survived the filter: exact negations, the huge pair of each half, everybody else small
    assert ys[1].tobytes() == (-ys[0]).tobytes() and ys[31].tobytes() == (-ys[30]).tobytes()
    assert np.isfinite(np.stack(ys)).all()
    # (the filter is 128 input frames long and as many output frames late: what the first half's huge pair reaches ends
    #  about 140 outputs before the stream does, what the second half's reaches begins behind output 400)
    first, second = slice(0, 300), slice(n - 100, n)
    assert np.median(np.abs(ys[0][first])) > 2.0 ** 55 and np.median(np.abs(ys[30][second])) > 2.0 ** 55
    assert max(np.abs(ys[s][first]).max() for s in range(2, 32)) < 2.0 ** 15
    assert max(np.abs(ys[s][second]).max() for s in range(0, 30)) < 2.0 ** 15
    z, frames = model(c, ys)
    assert frames == n and z[2:].tobytes() == np.zeros((2, n), np.float32).tobytes(), "a pair alone is not +0.0"
    for defect in bm.ORDER_DEFECTS + ("round_each_add",):
        bad, _ = model(c, ys, defect=defect)
        share = [max(bm.changed(bad[j][part], z[j][part]) for j in (0, 1)) for part in (first, second)]
        print("order, %-16s: %5.1f %% / %5.1f %% of a bus's samples change (first / second half)" % (defect, 100 * share[0], 100 * share[1]))
        assert max(share) >= 0.01, "the twin's floats do not tell %s from the rule" % defect
    for fmt, layout, aligned in FORMAT_RUNS:
        b = make(c)
        try:
            got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
            assert bus_frames == frames and made == [n] * 32
            check(c, fmt, layout, got, z, "format %d aligned %d" % (fmt, aligned))
        finally:
            b.close()


def test_signed_zeros_with_a_stream_that_has_ended():
    c = case("signs")
    ys = twin("signs")
    assert ys[0].size == 0 and ys[1].size > 300 and (ys[1] != 0).all()
    neg = ys[1] < 0
    assert 0.2 < neg.mean() < 0.8
    z, frames = model(c, ys)
    # -1 on the ended stream, 0 on the live one: -0 + -0 = -0, -0 + +0 = +0; +1 on the ended stream: +0 + either = +0
    assert z[0].tobytes() == np.where(neg, np.float32(-0.0), np.float32(0.0)).astype(np.float32).tobytes()
    assert z[1].tobytes() == np.zeros(neg.size, np.float32).tobytes() and z[2].tobytes() == ys[1].tobytes()
    for defect in ("zero_plus_first", "skip_zero_weight", "skip_ended"):
        bad, _ = model(c, ys, defect=defect)
        print("signs, %-16s: %5.1f %% of a bus's samples change" % (defect, 100 * differs(bad, z)))
        assert differs(bad, z) > 0, "the twin's floats do not tell %s from the rule" % defect
    for fmt, layout, aligned in FORMAT_RUNS + ((ULAW, INTER, True),):
        b = make(c)
        try:
            got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
            assert made == [0, frames] and bus_frames == frames
            check(c, fmt, layout, got, z, "format %d aligned %d" % (fmt, aligned))
        finally:
            b.close()


def test_a_zero_weight_on_an_infinite_stream_is_nan():
    c = case("inf")
    ys = twin("inf")
    assert np.isinf(ys[2]).any() and np.isfinite(ys[1]).all()
    z, frames = model(c, ys, nan_ok=True)
    bad, _ = model(c, ys, defect="skip_zero_weight")
    inf_at = np.zeros(frames * c.ch, bool)
    inf_at[: ys[2].size] = np.isinf(ys[2])
    assert np.isnan(z[0][inf_at]).all() and not np.isnan(bad[0][inf_at & ~np.isnan(bm.pad(ys, frames, c.ch)[0])]).any()
    print("inf, skip_zero_weight: %.2f %% of bus 0 changes" % (100 * bm.changed(bad[0], z[0])))
    assert bm.changed(bad[0], z[0]) > 0
    for fmt, layout, aligned in FORMAT_RUNS:
        b = make(c)
        try:
            got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
            assert bus_frames == frames
            check(c, fmt, layout, got, z, "format %d aligned %d" % (fmt, aligned))
        finally:
            b.close()


# ---- B. ramps inside bus_sum at odd channel counts -------------------------------------------------------------------------
def triple_gains(b=None):
    """the gains of B's triple case set on b (None: on the models alone): the models"""
    models = [gm.State() for _ in TRIPLE_FED]
    # 0: a ramp that ends inside the call, in mid-tile; 1: a constant; 2: a ramp still in flight when the stream ends;
    # 3: a ramp pending on a stream that is fed nothing; 4: off
    for s, (gain, ramp) in {0: (0.3, 1777), 1: (-1.0, 0), 2: (0.5, 4000), 3: (-0.7, 900)}.items():
        models[s].set(gain, ramp)
        if b is not None:
            assert b.set_gain(gain, ramp, stream=s) == 0
    return models


def check_ramp_defects(c, ys, gfull, z):
    assert gained_rows(c, ys, gfull, z.shape[1] // c.ch).tobytes() == bm.pad(
        [y if g is None else gm.apply(y, g[: y.size // c.ch], c.ch) for y, g in zip(ys, gfull)], z.shape[1] // c.ch, c.ch).tobytes()
    for defect in ("ignores_r0", "group_first"):
        bad, _ = model(c, ys, gfull, gain_defect=defect)
        print("%s, ramp %-12s: %5.1f %% of a bus's samples change" % (c.name, defect, 100 * differs(bad, z)))
        assert differs(bad, z) >= 0.01, "the twin's floats do not tell the ramp defect %s from the rule" % defect
    # the product with g behind a stream's end instead of +0.0f: -0.0f terms where g is negative, which no sum here
    # shows -- every bus holds a non-zero or a +0.0 term beside them.  Bit-neutral, and said so.
    bad, _ = model(c, ys, gfull, gain_defect="past_end")
    assert bad.tobytes() == z.tobytes()


@functools.lru_cache(maxsize=None)
def triple_model(mode=None):
    c = case("triple")
    ys = twin("triple", mode)
    made = [y.size // c.ch for y in ys]
    frames = max(made)
    total = frames * c.ch
    assert made[0] == made[1] == made[4] == frames and made[3] == 0
    # whole tiles and a tail; stream 2 ends inside a tile, before the bus does; stream 0's ramp ends in mid-tile, inside
    # the call; stream 2's is in flight at its end; every tile but the first starts in another channel than 0
    assert total // TILE >= 4 and total % TILE != 0 and TILE % c.ch == 1
    assert 0 < made[2] < frames and (made[2] * c.ch) % TILE != 0 and made[2] * c.ch > TILE
    assert 1777 < frames and (1777 * c.ch) % TILE not in (0, TILE - 1) and made[2] < 4000
    models = triple_gains()
    gfull = ramps(models, made, frames)
    assert gfull[4] is None and (np.diff(gfull[0]) != 0).sum() > 1000 and models[3].done == 0 and models[2].done == made[2]
    z, _ = model(c, ys, gfull)
    check_ramp_defects(c, ys, gfull, z)
    return z, frames, made, tuple(m.report() for m in models)


@pytest.mark.parametrize("fmt_name,layout,aligned", (("f32", INTER, True), ("f32", INTER, False), ("s16", PLANAR, True), ("s24", INTER, True)))
def test_ramps_of_three_channels_in_and_behind_the_streams(fmt_name, layout, aligned):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("triple")
    z, frames, made_want, reports = triple_model()
    b = make(c)
    try:
        triple_gains(b)
        got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
        assert made == made_want and bus_frames == frames
        check(c, fmt, layout, got, z, "gained %s aligned %d" % (fmt_name, aligned))
        for s in range(len(c.fed)):
            assert tb.report(b, s) == reports[s], "get_gain of stream %d after the call" % s
        assert b.get_gain(3)["remaining"] == 900, "the ramp of a stream that was fed nothing moved"
    finally:
        b.close()


@pytest.mark.parametrize("fmt_name,layout", (("f32", INTER), ("s16", PLANAR), ("s24", INTER)))
def test_two_calls_of_the_gained_triple_give_what_one_gives(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("triple")
    z, frames, made_want, reports = triple_model()
    kind, cut = dm.TRIANGULAR, 700

    def go(cuts):
        b = make(c, kind=kind, meter=True)
        try:
            triple_gains(b)
            pieces, total = [], 0
            for lo, hi in cuts:
                got, made, bus_frames = run(b, c, fmt, layout, lo=lo, hi=hi, aligned=False)
                pieces.append(got.reshape(len(c.w), c.ch if layout == PLANAR else 1, -1))
                total += bus_frames
            meters = [b.get_bus_meter(j) for j in range(len(c.w))]
            return (np.concatenate(pieces, axis=2).reshape(len(c.w), -1), total, meters, b.bus_position(),
                    tuple(tb.report(b, s) for s in range(len(c.fed))))
        finally:
            b.close()

    one, two = go(((0, c.frames),)), go(((0, cut), (cut, c.frames)))
    for res, what in ((one, "one call"), (two, "two calls")):
        assert res[1] == frames and res[3] == START + frames and res[4] == reports, what
        check(c, fmt, layout, res[0], z, what, kind, START)
        for j in range(len(c.w)):
            m = dict(res[2][j])
            assert m.pop("on") is True and mm.same(m, totals(c, fmt, j, ((z, START),), kind)), "%s: bus %d meter" % (what, j)
    assert one[0].tobytes() == two[0].tobytes()       # (finite input: the float formats too)


@pytest.mark.parametrize("fmt_name,layout,aligned", (("f32", INTER, False), ("f32", INTER, True), ("s16", PLANAR, True), ("u8", INTER, True)))
def test_six_channels_eleven_buses_of_two_streams(fmt_name, layout, aligned):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("six")
    ys = twin("six")
    made_want = [y.size // c.ch for y in ys]
    frames = max(made_want)
    assert TILE % c.ch == 4 and frames * c.ch // TILE >= 2 and (frames * c.ch) % TILE != 0
    assert len(c.w) == 11 > len(c.fed) and not c.w[4].any()
    models = [gm.State(), gm.State()]
    models[0].set(0.25, 300)
    gfull = ramps(models, made_want, frames)
    assert models[0].done == 300 < frames
    z, _ = model(c, ys, gfull)
    check_ramp_defects(c, ys, gfull, z)
    b = make(c)
    try:
        assert b.set_gain(0.25, 300, stream=0) == 0
        got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
        assert made == made_want and bus_frames == frames
        check(c, fmt, layout, got, z, "%s aligned %d" % (fmt_name, aligned))
        assert [tb.report(b, s) for s in range(2)] == [m.report() for m in models]
    finally:
        b.close()


# ---- C. shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("solo", "nine", "matrix"))
def test_small_shapes(name):
    c = case(name)
    ys = twin(name)
    z, frames = model(c, ys)
    assert frames > 100
    if name == "matrix":
        assert c.x.shape[2] == 2 and c.ch == 1 and c.in_layout == PLANAR and c.in_fmt == S16
    for fmt, layout, aligned in FORMAT_RUNS:
        b = make(c)
        try:
            got, made, bus_frames = run(b, c, fmt, layout, aligned=aligned)
            assert bus_frames == frames and made == [y.size // c.ch for y in ys]
            check(c, fmt, layout, got, z, "format %d aligned %d" % (fmt, aligned))
        finally:
            b.close()


def peek(b, s, n_in, cap):
    i = b.info(s)
    return speexhip.plan_call_ex(i["num_rate"], i["den_rate"], n_in, cap, True, i["block_in"], i["last_sample"],
                                 i["samp_frac_num"], i["magic_samples"])


@pytest.mark.parametrize("fmt_name", ("f32", "s16"))
def test_a_call_that_feeds_nothing(fmt_name):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("nine")
    kind = dm.TRIANGULAR
    b, t = make(c, kind=kind, meter=True), make(c, buses=False)
    try:
        assert b.set_gain(0.5, 1000, stream=1) == 0
        # on a fresh batch: nothing is produced, written or moved
        before = (stream_state(b), b.get_buses().tobytes(), b.bus_position())
        got, made, bus_frames = run(b, c, fmt, INTER, lens=(0, 0), aligned=False)
        assert made == [0, 0] and bus_frames == 0 and got.size == 0
        assert (stream_state(b), b.get_buses().tobytes(), b.bus_position()) == before
        check_meters(b, c, fmt, (), kind, "nothing fed")
        # behind a real call and a change of quality: what the plan says is pending, and no more
        model_g = gm.State()
        model_g.set(0.5, 1000)
        ys = float_call(t, c)
        made1 = [y.size for y in ys]
        z1, frames1 = model(c, ys, ramps([gm.State(), model_g], made1, max(made1)))
        got, made, bus_frames = run(b, c, fmt, INTER, aligned=False)
        check(c, fmt, INTER, got, z1, "first call", kind, START)
        for bb in (b, t):
            assert bb.set_quality(3) == 0
        want = [peek(b, s, 0, 64)[1] for s in range(2)]
        print("nothing fed behind set_quality: the plan produces", want)
        assert max(want) > 0, "nothing is pending: the call would show nothing"
        ys = float_call(t, c, lens=(0, 0), cap=64)
        assert [y.size for y in ys] == want
        got, made, bus_frames = run(b, c, fmt, INTER, lens=(0, 0), aligned=False, cap=64)
        assert made == want and bus_frames == max(want)
        z2, frames2 = model(c, ys, ramps([gm.State(), model_g], want, max(want)))
        check(c, fmt, INTER, got, z2, "nothing fed", kind, START + frames1)
        assert b.bus_position() == START + frames1 + bus_frames
        check_meters(b, c, fmt, ((z1, START), (z2, START + frames1)), kind, "nothing fed")
        assert tb.report(b, 1) == model_g.report()
    finally:
        b.close()
        t.close()


@pytest.mark.parametrize("fmt_name", ("alaw", "bf16n", "s16be", "s24be"))
def test_the_remaining_formats_dithered_on_the_mix_minus(fmt_name):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("mono")
    kind = dm.TRIANGULAR
    z, frames = model(c, twin("mono"))
    b = make(c, kind=kind, meter=True)
    try:
        got, made, bus_frames = run(b, c, fmt, INTER, aligned=False)
        assert bus_frames == frames
        check(c, fmt, INTER, got, z, fmt_name, kind, START)
        assert b.bus_position() == START + frames
        check_meters(b, c, fmt, ((z, START),), kind, fmt_name)
    finally:
        b.close()


# ---- D. promises ------------------------------------------------------------------------------------------------------------------
def test_the_zero_fallbacks_zeros_are_gained_and_summed_like_any_value():
    c = case("stereo")
    L = speexhip.lib()
    finite = np.where(np.isfinite(c.x), c.x, np.float32(1.0)).astype(np.float32)
    # (every stream fed alike: one that ended early would supply +0.0f, not its product with -1)
    c = c._replace(x=finite, w=np.ones((2, 3), np.float32), fed=(c.frames,) * 3)
    b = make(c)
    try:
        assert b.set_gain(-1.0, 0) == 0
        L.speexhip_debug_fail_device_allocs(1)
        rc = b.set_rate_frac(2, 3, 32000, 48000)
        L.speexhip_debug_fail_device_allocs(0)
        assert rc == speexhip.ERR_ALLOC_FAILED
        cap = c.frames * 3 // 2 + 64
        for gain_off, fmts in ((None, (F32, S16, ULAW)), (1, (F32,))):
            if gain_off is not None:
                assert b.set_gain(1.0, 0, stream=gain_off) == 0
            for fmt in fmts:
                for aligned in (True, False):
                    want = [peek(b, s, n, cap)[:2] for s, n in enumerate(c.fed)]
                    assert all(used == n for (used, _), n in zip(want, c.fed))
                    got, made, bus_frames = run(b, c, fmt, INTER, aligned=aligned, cap=cap, want_rc=speexhip.ERR_ALLOC_FAILED)
                    assert made == [p for _, p in want] and bus_frames > 0
                    if fmt == F32:    # -1 * +0.0f three times: -0.0f; with one stream's gain off a +0.0f term: +0.0f
                        one = np.float32(-0.0 if gain_off is None else 0.0)
                        sample = np.full(1, one, np.float32).view(np.uint8)
                    else:
                        sample = hm.zero(fmt)
                    for j in range(2):
                        assert got[j].tobytes() == np.tile(sample, bus_frames * c.ch).tobytes(), "format %d bus %d" % (fmt, j)
    finally:
        L.speexhip_debug_fail_device_allocs(0)
        b.close()


@pytest.mark.parametrize("fmt_name", ("s16", "f32"))
def test_control_calls_leave_the_bus_state_alone(fmt_name):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("triple")._replace(fed=(1500,) * 5)
    kind, cut = dm.TRIANGULAR, 700
    b, t = make(c, kind=kind, meter=True), make(c, buses=False)
    try:
        models = [gm.State() for _ in c.fed]
        models[0].set(0.3, 5000)
        assert b.set_gain(0.3, 5000, stream=0) == 0
        ys = float_call(t, c, 0, cut)
        made1 = [y.size // c.ch for y in ys]
        z1, frames1 = model(c, ys, ramps(models, made1, max(made1)))
        got, made, bus_frames = run(b, c, fmt, INTER, 0, cut)
        check(c, fmt, INTER, got, z1, "first call", kind, START)
        bus_state = lambda: (b.get_buses().tobytes(), b.bus_position(), [sorted(b.get_bus_meter(j).items()) for j in range(len(c.w))])
        before = bus_state()
        assert before[1] == START + frames1
        for bb in (b, t):
            assert bb.set_rate_frac(160, 441, 16000, 44100) == 0
            assert bb.set_quality(4) == 0
            assert bb.reset_mem() == 0
            assert bb.skip_zeros() == 0
            assert bb.set_meter(0) == 0 and bb.set_meter(1) == 0
        assert b.set_gain(0.5, 100, stream=1) == 0
        models[1].set(0.5, 100)
        assert bus_state() == before, "a control call touched the bus state"
        cap = (c.frames - cut) * 3 + 64
        ys = float_call(t, c, cut, c.frames, cap=cap)
        made2 = [y.size // c.ch for y in ys]
        z2, frames2 = model(c, ys, ramps(models, made2, max(made2)))
        got, made, bus_frames = run(b, c, fmt, INTER, cut, c.frames, cap=cap, aligned=False)
        assert made == made2 and bus_frames == frames2 > 1000
        check(c, fmt, INTER, got, z2, "second call", kind, START + frames1)
        assert b.bus_position() == START + frames1 + frames2
        check_meters(b, c, fmt, ((z1, START), (z2, START + frames1)), kind, "both calls")
        assert [tb.report(b, s) for s in range(len(c.fed))] == [m.report() for m in models]
    finally:
        b.close()
        t.close()


def test_set_buses_again_in_mid_stream_with_more_buses():
    c = case("six")
    kind, cut, fmt = dm.TRIANGULAR, 200, S16
    b, t = make(c, kind=kind, meter=True, w=c.w[:2]), make(c, buses=False)
    try:
        ys = float_call(t, c, 0, cut)
        z1, frames1 = model(c, ys, w=c.w[:2])
        got, made, bus_frames = run(b, c, fmt, PLANAR, 0, cut)
        check(c, fmt, PLANAR, got, z1, "two buses", kind, START)
        check_meters(b, c, fmt, ((z1, START),), kind, "two buses")
        assert b.bus_position() == START + frames1
        streams = stream_state(b)
        assert b.set_buses(c.w) == 0    # (eleven: the image of the buses grows)
        assert np.array_equal(b.get_buses(), c.w) and b.bus_position() == 0
        check_meters(b, c, fmt, (), kind, "behind set_buses")
        assert stream_state(b) == streams, "set_buses touched a stream"
        ys = float_call(t, c, cut, c.frames)
        z2, frames2 = model(c, ys)
        got, made, bus_frames = run(b, c, fmt, PLANAR, cut, c.frames)
        assert bus_frames == frames2
        check(c, fmt, PLANAR, got, z2, "eleven buses", kind, 0)
        check_meters(b, c, fmt, ((z2, 0),), kind, "eleven buses")
        assert b.bus_position() == frames2
        assert [b.get_dither(s)[2] for s in range(2)] == [START, START]
    finally:
        b.close()
        t.close()


def test_a_sides_call_between_two_bus_calls():
    c = case("triple")._replace(fed=(1500,) * 5)
    kind, fmt = dm.TRIANGULAR, S16
    S = len(c.fed)
    b, t = make(c, kind=kind), make(c, buses=False)
    try:
        models = [gm.State() for _ in c.fed]
        models[2].set(0.2, 6000)        # crosses all three calls
        assert b.set_gain(0.2, 6000, stream=2) == 0
        ys = float_call(t, c, 0, 500)
        made1 = [y.size // c.ch for y in ys]
        z1, frames1 = model(c, ys, ramps(models, made1, max(made1)))
        got, made, bus_frames = run(b, c, fmt, INTER, 0, 500)
        check(c, fmt, INTER, got, z1, "first bus call", kind, START)
        assert [b.get_dither(s)[2] for s in range(S)] == [START] * S and b.bus_position() == START + frames1
        # the sides call: every stream encoded for itself, behind its gain, from its own seed and position
        ys = float_call(t, c, 500, 1000)
        made2 = [y.size // c.ch for y in ys]
        g2 = ramps(models, made2, max(made2))
        cap = tb.wcap(500, c.fi, c.fo)
        in_side, keep = in_side_of(c, 500, 1000)
        out_side, buf = tb.out_buffer(fmt, S, cap, c.ch, INTER)
        used, made = b.process_sides_device(in_side, [500] * S, out_side, cap)
        assert made == made2
        raw = tb.fetched(fmt, buf, S, cap, c.ch, INTER, max(made))
        for s in range(S):
            y = ys[s] if g2[s] is None else gm.apply(ys[s], g2[s][: made2[s]], c.ch)
            want = hm.raw(fmt, hm.from_internal_dither(fmt, y, kind, dm.stream_seed(SEED, s), START, c.ch))
            assert raw[s, : want.size].tobytes() == want.tobytes(), "sides call, stream %d" % s
        assert [b.get_dither(s)[2] for s in range(S)] == [START + n for n in made2], "stream positions: the sides call alone"
        assert b.bus_position() == START + frames1, "the sides call moved the bus position"
        ys = float_call(t, c, 1000, 1500)
        made3 = [y.size // c.ch for y in ys]
        z3, frames3 = model(c, ys, ramps(models, made3, max(made3)))
        got, made, bus_frames = run(b, c, fmt, INTER, 1000, 1500, aligned=False)
        check(c, fmt, INTER, got, z3, "second bus call", kind, START + frames1)
        assert b.bus_position() == START + frames1 + frames3
        assert [b.get_dither(s)[2] for s in range(S)] == [START + n for n in made2]
        assert models[2].done == made1[2] + made2[2] + made3[2]
        assert [tb.report(b, s) for s in range(S)] == [m.report() for m in models], "the gains move by all three calls"
    finally:
        b.close()
        t.close()


# ---- E. modes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (speexhip.MODE_EXACT, speexhip.MODE_FAST_F32))
@pytest.mark.parametrize("fmt_name", ("s16", "f32"))
def test_the_other_modes(mode, fmt_name):
    fmt, _ = mm.FORMATS[fmt_name]
    c = case("stereo")
    z, frames = model(c, twin("stereo", mode), nan_ok=True)
    b = make(c, mode)
    try:
        assert b.info(0)["mode"] == mode
        got, made, bus_frames = run(b, c, fmt, INTER, aligned=False)
        assert bus_frames == frames
        check(c, fmt, INTER, got, z, "mode %d %s" % (mode, fmt_name))
    finally:
        b.close()
    c = case("triple")
    z, frames, made_want, reports = triple_model(mode)
    b = make(c, mode)
    try:
        triple_gains(b)
        got, made, bus_frames = run(b, c, fmt, INTER, aligned=False)
        assert made == made_want and bus_frames == frames
        check(c, fmt, INTER, got, z, "mode %d %s" % (mode, fmt_name))
        assert tuple(tb.report(b, s) for s in range(len(c.fed))) == reports
    finally:
        b.close()
