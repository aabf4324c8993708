"""Mix buses (include/speexhip_resampler.h, "Buses") on the GPU.  The expected bytes never come from the code under test:
a twin batch makes the same call through process_sides_device with F32 out, no gain and no buses -- a stream's floats do
not depend on what shares its launch -- gain_model.py multiplies the twin's floats by g of each output frame, bus_model.py
sums them in float64 in ascending order, the format models (halfbe_model.py, dither_model.py) encode the buses with the
dither of the bus seeds at the bus position, and meter_model.py judges them.  Bytes, totals, positions and the bits of
get_gain are compared for equality.

The one allowance: for the float output formats, where the model's value is NaN the library's value must be a NaN and its
bits are not compared -- which payload survives a sum of NaNs, and the sign of a generated NaN, are the implementation's
choice (the allowance test_gpu_gain.py documents for the gain's products).  The stereo input carries one NaN (stream 0,
channel 0) and one +inf (stream 2, channel 1); a 64-tap q7 filter spreads each over about 70 of 3265 frames of one channel,
about 1.1 % of a bus's samples per bad sample, and the test asserts that at most 5 % of any bus's samples are NaN in the
model.  The mono and triple inputs are finite and their model output has no NaN.  Integer and companded formats get no
allowance: NaN is the format's zero, compared exactly.

Shapes, the smallest that reach every branch: 44.1k -> 48k stereo q7, 3000 frames, 3 streams x 2 buses with stream 1 fed
2990 frames -- about 3265 output frames: whole 1024-sample tiles and a tail, and a stream that ends before the bus does;
8k -> 16k mono q7, 160 frames, 32 streams x 32 buses mix-minus -- full packs, every bus group, under one tile; 16k -> 48k
of three channels q5, 1500 frames, 5 streams x 3 buses -- frames that straddle a lane's 16-byte group."""
import ctypes as C
import functools

import numpy as np
import pytest

import bus_model as bm
import dither_model as dm
import gain_model as gm
import halfbe_model as hm
import meter_model as mm
import speexhip

pytestmark = pytest.mark.gpu

F32, F32N, S16, ULAW = speexhip.FMT_F32, speexhip.FMT_F32N, speexhip.FMT_S16, speexhip.FMT_ULAW
FLOATS = (F32, F32N, speexhip.FMT_F16N, speexhip.FMT_BF16N)
SEED = 0x5EEDFACE12345678
START = 4242
INTER, PLANAR = speexhip.LAYOUT_INTERLEAVED, speexhip.LAYOUT_PLANAR
FORMATS = ("s16", "u8", "s24", "s32be", "ulaw", "f32", "f32n", "f16n")

# name: (channels, in_rate, out_rate, quality, frames, frames fed per stream, W)
STEREO_W = np.array([[1.0, 1.0, 1.0], [0.75, -0.5, 1.25]], np.float32)   # sums beyond full scale
TRIPLE_W = np.array([[1.0, 0.5, 0.0, -1.0, 0.25], [0.0, 0.0, 1.0, 0.0, 0.0], [-0.125, 3.0, 1.0, 1.0, 1.0]], np.float32)
CASES = {
    "stereo": (2, 44100, 48000, 7, 3000, (3000, 2990, 3000), STEREO_W),
    "mono": (1, 8000, 16000, 7, 160, (160,) * 32, bm.mix_minus(32)),
    "triple": (3, 16000, 48000, 5, 1500, (1500,) * 5, TRIPLE_W),
}


def wcap(frames, fi, fo):
    return frames * fo // fi + 64


@functools.lru_cache(maxsize=None)
def noise(name):
    """(streams, frames, ch) float32 in int16 units; the stereo case with one NaN and one +inf"""
    ch, fi, fo, q, frames, fed, w = CASES[name]
    rng = np.random.default_rng(77 + ch)
    scale = 1.3 if name == "stereo" else 0.9
    x = (rng.uniform(-scale, scale, (len(fed), frames, ch)) * 32767.0).astype(np.float32)
    if name == "stereo":
        x[0, frames // 8, 0] = np.nan
        x[2, frames - frames // 16, 1] = np.inf
    x.setflags(write=False)
    return x


def batch(name, kind=dm.NONE, meter=False, buses=True):
    ch, fi, fo, q, frames, fed, w = CASES[name]
    b = speexhip.Batch(len(fed), ch, fi, fo, q)
    if kind != dm.NONE:
        assert b.set_dither(kind, SEED, START) == 0
    if meter:
        assert b.set_meter(1) == 0
    if buses:
        assert b.set_buses(w) == 0    # (behind set_dither: set_buses zeroes the bus position)
    return b


def storage(fmt, x, layout):
    """(streams, frames, ch) float32 -> the input side's bytes on the device, its Side and the tensor that owns them"""
    import torch
    S, frames, ch = x.shape
    arranged = x if layout == INTER else np.ascontiguousarray(x.transpose(0, 2, 1))
    raw = hm.raw(fmt, hm.from_internal(fmt, arranged.reshape(-1)))
    t = torch.from_numpy(raw.copy()).cuda()
    side = speexhip.make_side(fmt, ch, layout, None, t.data_ptr(), frames, frames * ch)
    return side, t


def out_buffer(fmt, items, cap, ch, layout):
    import torch
    t = torch.zeros(items * cap * ch * hm.nbytes(fmt), dtype=torch.uint8, device="cuda")
    return speexhip.make_side(fmt, ch, layout, None, t.data_ptr(), cap, cap * ch), t


def fetched(fmt, t, items, cap, ch, layout, frames):
    """the first `frames` frames of every item of an output buffer: (items, bytes) -- planar: plane after plane"""
    import torch
    torch.cuda.synchronize()
    nb = hm.nbytes(fmt)
    raw = t.cpu().numpy()
    if layout == INTER or ch == 1:
        return raw.reshape(items, cap * ch * nb)[:, : frames * ch * nb].copy()
    return np.ascontiguousarray(raw.reshape(items, ch, cap * nb)[:, :, : frames * nb]).reshape(items, -1)


@functools.lru_cache(maxsize=None)
def twin_floats(name, in_fmt=F32, in_layout=INTER):
    """per stream, the flat interleaved float32 result of the case's input in an ungained twin batch without buses: what
    the bus call sums.  Computed once."""
    ch, fi, fo, q, frames, fed, w = CASES[name]
    S, cap = len(fed), wcap(frames, fi, fo)
    t = batch(name, buses=False)
    try:
        in_side, keep = storage(in_fmt, noise(name), in_layout)
        out_side, buf = out_buffer(F32, S, cap, ch, INTER)
        used, made = t.process_sides_device(in_side, list(fed), out_side, cap)
        assert used == list(fed)
        raw = fetched(F32, buf, S, cap, ch, INTER, max(made))
        outs = [raw[s, : made[s] * ch * 4].copy().view(np.float32) for s in range(S)]
    finally:
        t.close()
    for y in outs:
        y.setflags(write=False)
    return tuple(outs)


def model_buses(name, ys, gains=None):
    """(n_buses, bus_frames * ch) float32 of the twin's floats ys, stream s behind gains[s] (None: not multiplied)"""
    ch, w = CASES[name][0], CASES[name][6]
    gained = [y if gains is None or gains[s] is None else gm.apply(y, gains[s], ch) for s, y in enumerate(ys)]
    frames = max(y.size for y in ys) // ch
    z = bm.buses(w, bm.pad(gained, frames, ch))
    if name == "stereo":
        assert np.isnan(z).any(), "the stereo buses hold no NaN"
        assert all(np.isnan(zj).mean() <= 0.05 for zj in z), "more than 5 % of a bus is NaN in the model"
    else:
        assert not np.isnan(z).any(), "a finite input made a NaN in the model"
    return z, frames


def encode(fmt, zj, kind, ch, n_streams, j, position):
    """the model's storage bytes of bus j's floats, from bus position `position` on"""
    if kind == dm.NONE or not hm.dithered(fmt):
        st = hm.from_internal(fmt, zj)
    else:
        st = hm.from_internal_dither(fmt, zj, kind, dm.stream_seed(SEED, n_streams + j), position, ch)
    return np.ascontiguousarray(hm.raw(fmt, st))


def as_layout(fmt, inter_bytes, ch, layout):
    if layout == INTER or ch == 1:
        return inter_bytes
    b = hm.nbytes(fmt)
    return np.ascontiguousarray(np.asarray(inter_bytes, np.uint8).reshape(-1, ch, b).transpose(1, 0, 2)).reshape(-1)


def same_storage(fmt, got, want, zj, ch, layout, what):
    """bytes equal; for the float formats a sample whose model value is NaN is matched by any NaN (module docstring)"""
    got, want = np.asarray(got, np.uint8).reshape(-1), np.asarray(want, np.uint8).reshape(-1)
    assert got.size == want.size, "%s: %d bytes, model %d" % (what, got.size, want.size)
    nan = np.isnan(np.asarray(zj, np.float32).reshape(-1))
    if fmt in FLOATS and nan.any():
        if not (layout == INTER or ch == 1):
            nan = np.ascontiguousarray(nan.reshape(-1, ch).T).reshape(-1)
        b = hm.nbytes(fmt)
        vg = hm.to_internal(fmt, got.view(hm.dtype(fmt)))
        assert np.isnan(vg[nan]).all(), what + ": no NaN where the model has one"
        keep = np.repeat(~nan, b)
        got, want = got[keep], want[keep]
    if got.tobytes() != want.tobytes():
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first difference at byte %d of %d (%d differ)" % (what, at, got.size, int((got != want).sum())))


def bus_call(b, name, fmt, layout, in_fmt=F32, in_layout=INTER, lo=0, hi=None):
    """one bus call of b over frames [lo, hi) of the case's input: (the buses' bytes (n_buses, bytes), produced, bus_frames)"""
    ch, fi, fo, q, frames, fed, w = CASES[name]
    hi = frames if hi is None else hi
    lens = [max(0, min(f, hi) - lo) for f in fed]
    cap = wcap(hi - lo, fi, fo)
    in_side, keep = storage(in_fmt, noise(name)[:, lo:hi], in_layout)
    out_side, buf = out_buffer(fmt, len(w), cap, ch, layout)
    used, made, bus_frames = b.process_bus_device(in_side, lens, out_side, cap)
    assert used == lens and bus_frames == max(made)
    return fetched(fmt, buf, len(w), cap, ch, layout, bus_frames), made, bus_frames


def check_buses(name, fmt, layout, got, z, kind, position, what):
    ch, w = CASES[name][0], CASES[name][6]
    for j in range(len(w)):
        want = as_layout(fmt, encode(fmt, z[j], kind, ch, w.shape[1], j, position), ch, layout)
        same_storage(fmt, got[j], want, z[j], ch, layout, "%s bus %d" % (what, j))


# ---- 1. every output format, both layouts, a planar and a mu-law input side ------------------------------------------
@pytest.mark.parametrize("fmt_name", FORMATS)
def test_every_format_and_layout_equals_the_model_on_the_twins_floats(fmt_name):
    fmt, _ = mm.FORMATS[fmt_name]
    runs = (("stereo", F32, INTER, (INTER, PLANAR)), ("mono", ULAW, INTER, (INTER,)), ("triple", F32, PLANAR, (INTER, PLANAR)))
    for name, in_fmt, in_layout, layouts in runs:
        ys = twin_floats(name, in_fmt, in_layout)
        z, frames = model_buses(name, ys)
        if name == "stereo":
            assert len(ys[1]) < len(ys[0]), "stream 1 does not end before the bus"
            assert frames * 2 > 3 * 1024 and (frames * 2) % 1024 != 0, "no whole tiles and a tail"
        for layout in layouts:
            b = batch(name)
            try:
                got, made, bus_frames = bus_call(b, name, fmt, layout, in_fmt, in_layout)
                assert bus_frames == frames and made == [y.size // CASES[name][0] for y in ys]
                check_buses(name, fmt, layout, got, z, dm.NONE, 0, "%s %s layout %d" % (name, fmt_name, layout))
                assert b.bus_position() == 0, "the bus position moved without dither"
            finally:
                b.close()


def test_process_bus_tensor_gives_the_buses_of_a_tensor():
    import torch
    name = "triple"
    ch, fi, fo, q, frames, fed, w = CASES[name]
    z, n = model_buses(name, twin_floats(name))
    b = batch(name, buses=False)
    try:
        x = torch.from_numpy(noise(name).copy()).cuda()
        out, bus_frames, made = b.process_bus_tensor(x, weights=w, out_dtype=torch.int16)
        assert bus_frames == n and tuple(out.shape) == (len(w), n, ch) and np.array_equal(b.get_buses(), w)
        check_buses(name, S16, INTER, np.ascontiguousarray(out.cpu().numpy()).view(np.uint8).reshape(len(w), -1), z, dm.NONE, 0, "tensor")
    finally:
        b.close()
    b = batch(name)     # (a fresh stream; weights=None: the matrix the batch already has)
    try:
        out, bus_frames, made = b.process_bus_tensor(x, out_dtype=torch.float32, normalized=False, out_layout="planar")
        assert tuple(out.shape) == (len(w), ch, n)
        got = np.ascontiguousarray(out.cpu().numpy()).view(np.uint8).reshape(len(w), -1)
        check_buses(name, F32, PLANAR, got, z, dm.NONE, 0, "tensor, planar")
    finally:
        b.close()


# ---- 2. gain: a ramp in flight, a muted stream, a stream that is off -------------------------------------------------
def report(b, s):
    g = b.get_gain(s)
    return (np.float32(g["current"]).tobytes(), np.float32(g["target"]).tobytes(), g["remaining"])


@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("f32", INTER), ("s24", PLANAR)))
def test_streams_are_gained_before_they_are_summed(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    name = "stereo"
    ch = CASES[name][0]
    ys = twin_floats(name)
    models = [gm.State() for _ in ys]
    b = batch(name)
    try:
        # stream 0: a ramp that ends at an odd frame inside the call; stream 1: muted; stream 2: off
        for s, (gain, ramp) in {0: (0.3, 1777), 1: (0.0, 0)}.items():
            assert b.set_gain(gain, ramp, stream=s) == 0
            models[s].set(gain, ramp)
        gains = [m.take(y.size // ch) for m, y in zip(models, ys)]
        gains[2] = None
        assert (np.diff(gains[0]) != 0).sum() > 1000 and models[0].done == models[0].total
        z, frames = model_buses(name, ys, gains)
        got, made, bus_frames = bus_call(b, name, fmt, layout)
        check_buses(name, fmt, layout, got, z, dm.NONE, 0, "gained %s" % fmt_name)
        for s, m in enumerate(models):
            assert report(b, s) == m.report(), "get_gain of stream %d after the call" % s
    finally:
        b.close()


# ---- 3. dither and meter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("u8", PLANAR), ("ulaw", INTER), ("f32", INTER), ("f32n", PLANAR)))
def test_buses_are_dithered_from_the_bus_seeds_and_judged_into_their_own_cells(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    kind = dm.TRIANGULAR
    for name in ("stereo", "mono"):
        ch, w = CASES[name][0], CASES[name][6]
        S = w.shape[1]
        ys = twin_floats(name)
        z, frames = model_buses(name, ys)
        b = batch(name, kind, meter=True)
        try:
            assert b.bus_position() == 0, "set_buses did not zero the bus position"
            assert b.set_dither(kind, SEED, START) == 0 and b.bus_position() == START
            got, made, bus_frames = bus_call(b, name, fmt, layout)
            check_buses(name, fmt, layout, got, z, kind, START, "dithered %s %s" % (name, fmt_name))
            assert b.bus_position() == START + bus_frames
            clipped = 0
            for j in range(len(w)):
                d = dm.values(kind, dm.stream_seed(SEED, S + j), START * ch, z[j].size) if mm.clips(fmt) else None
                want = mm.totals(fmt, z[j], d)
                m = b.get_bus_meter(j)
                assert m.pop("on") is True and mm.same(m, want), "%s bus %d: meter %r, model %r" % (name, j, m, want)
                assert m["samples"] == bus_frames * ch
                clipped += want["clipped_high"] + want["clipped_low"]
            if mm.clips(fmt):
                assert clipped > 0, "the weights do not sum beyond full scale"
            # nothing of the streams is encoded: their dither positions and meter totals have not moved
            for s in range(S):
                assert b.get_dither(s) == (kind, dm.stream_seed(SEED, s), START)
                ms = b.get_meter(s)
                assert ms.pop("on") is True and mm.same(ms, mm.ZERO)
            # reset clears that bus only
            first = b.get_bus_meter(0, reset=True)
            again = b.get_bus_meter(0)
            again.pop("on")
            assert mm.same(again, mm.ZERO) and first["samples"] == bus_frames * ch
            if len(w) > 1:
                assert b.get_bus_meter(1)["samples"] == bus_frames * ch
        finally:
            b.close()


# ---- 4. chunk independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name,layout", (("s16", INTER), ("s24", PLANAR), ("f32", INTER)))
def test_two_calls_give_the_bytes_and_totals_of_one(fmt_name, layout):
    fmt, _ = mm.FORMATS[fmt_name]
    name, cut = "stereo", 1700
    ch, fi, fo, q, frames, fed, w = CASES[name]
    S, kind = len(fed), dm.TRIANGULAR
    nb = hm.nbytes(fmt)

    def run(cuts):
        b = batch(name, kind, meter=True)
        try:
            assert b.set_dither(kind, SEED, START) == 0
            assert b.set_gain(0.25, 2500, stream=1) == 0     # crosses the boundary between the calls
            pieces, total = [], 0
            for lo, hi in cuts:
                got, made, bus_frames = bus_call(b, name, fmt, layout, lo=lo, hi=hi)
                pieces.append(got.reshape(len(w), ch if layout == PLANAR else 1, -1))
                total += bus_frames
            meters = [b.get_bus_meter(j) for j in range(len(w))]
            return np.concatenate(pieces, axis=2).reshape(len(w), -1), total, meters, b.bus_position(), report(b, 1)
        finally:
            b.close()

    one = run(((0, frames),))
    two = run(((0, cut), (cut, frames)))
    assert one[1] == two[1] and one[3] == two[3] == START + one[1]
    assert one[4] == two[4]
    # the model, on the twin's floats of the whole stream: a stream's floats do not depend on how it is cut into calls
    ys = twin_floats(name)
    model = gm.State()
    model.set(0.25, 2500)
    gains = [None, model.take(ys[1].size // ch), None]
    assert model.report() == one[4]
    # (the first of the two calls feeds all streams alike; stream 1's 2990 frames are 1700 + 1290 there)
    z, n = model_buses(name, ys, gains)
    assert n == one[1]
    for res, what in ((one, "one call"), (two, "two calls")):
        check_buses(name, fmt, layout, res[0], z, kind, START, what)
        for j in range(len(w)):
            d = dm.values(kind, dm.stream_seed(SEED, S + j), START * ch, z[j].size) if mm.clips(fmt) else None
            m = dict(res[2][j])
            assert m.pop("on") is True and mm.same(m, mm.totals(fmt, z[j], d)), "%s: bus %d meter" % (what, j)
    assert one[0].tobytes() == two[0].tobytes() or fmt in FLOATS


# ---- 5. errors leave everything untouched ------------------------------------------------------------------------------
def snapshot(b, n_in, cap):
    """info and the next call's counters of every stream, with the bus state beside them"""
    out = []
    for s in range(b.n_streams):
        i = b.info(s)
        peek = speexhip.plan_call_ex(i["num_rate"], i["den_rate"], n_in, cap, True, i["block_in"], i["last_sample"],
                                     i["samp_frac_num"], i["magic_samples"])
        out.append((tuple(sorted(i.items())), peek, report(b, s), b.get_dither(s)))
    w = b.get_buses()
    return out, None if w is None else w.tobytes(), b.bus_position()


def test_errors_leave_the_state_and_the_lengths_untouched():
    import torch
    name = "stereo"
    ch, fi, fo, q, frames, fed, w = CASES[name]
    S, cap = len(fed), wcap(frames, fi, fo)
    L = speexhip.lib()
    x = noise(name)
    in_side, keep = storage(F32, x, INTER)
    out_side, buf = out_buffer(S16, len(w), cap, ch, INTER)
    b = batch(name, buses=False)
    try:
        # a first call, so that the state is not a fresh one
        assert b.set_gain(0.5, 100000, stream=0) == 0
        side_s, buf_s = out_buffer(S16, S, cap, ch, INTER)
        b.process_sides_device(in_side, 100, side_s, cap)
        before = snapshot(b, frames, cap)

        def refused(code, call, what):
            rc, used, made, bus_frames = call()
            assert rc == code, "%s: code %d" % (what, rc)
            assert used == list(fed) and made == [cap] * S and bus_frames == 0, what + ": lengths touched"
            assert snapshot(b, frames, cap) == before, what + ": state touched"

        refused(speexhip.ERR_BAD_STATE, lambda: b.bus_call(in_side, list(fed), out_side, cap), "no buses")
        assert b.set_buses(np.ones((33, S), np.float32)) == speexhip.ERR_INVALID_ARG
        bad = w.copy()
        bad[1, 2] = np.nan
        assert b.set_buses(bad) == speexhip.ERR_INVALID_ARG
        bad[1, 2] = np.inf
        assert b.set_buses(bad) == speexhip.ERR_INVALID_ARG
        assert b.get_buses() is None and snapshot(b, frames, cap) == before
        refused(speexhip.ERR_BAD_STATE, lambda: b.bus_call(in_side, list(fed), out_side, cap), "still no buses")
        many = speexhip.Batch(33, 1, 8000, 16000, 3)
        try:
            assert many.set_buses(np.ones((1, 33), np.float32)) == speexhip.ERR_INVALID_ARG and many.get_buses() is None
        finally:
            many.close()
        assert b.set_buses(w) == 0 and np.array_equal(b.get_buses(), w)
        before = snapshot(b, frames, cap)
        # a refused set_buses leaves the matrix that was there
        assert b.set_buses(np.ones((33, S), np.float32)) == speexhip.ERR_INVALID_ARG and snapshot(b, frames, cap) == before
        mix = np.eye(ch, dtype=np.float32)
        mixed = speexhip.make_side(S16, ch, INTER, mix, buf.data_ptr(), cap, cap * ch)
        refused(speexhip.ERR_INVALID_ARG, lambda: b.bus_call(in_side, list(fed), mixed, cap), "out->mix")
        wide = speexhip.make_side(S16, ch + 1, INTER, None, buf.data_ptr(), cap, cap * ch)
        refused(speexhip.ERR_INVALID_ARG, lambda: b.bus_call(in_side, list(fed), wide, cap), "wrong channels")

        def null_frames():
            il, ol = (C.c_uint32 * S)(*fed), (C.c_uint32 * S)(*([cap] * S))
            rc = L.speexhip_batch_process_bus_device(b._h, C.byref(in_side), il, C.byref(out_side), ol, None, None)
            return rc, list(il), list(ol), 0
        refused(speexhip.ERR_INVALID_ARG, null_frames, "NULL bus_frames")
        # ... and the call still works, on the state the refused ones left
        rc, used, made, bus_frames = b.bus_call(in_side, list(fed), out_side, cap)
        assert rc == 0 and used == list(fed) and bus_frames == max(made) > 0
        torch.cuda.synchronize()
    finally:
        b.close()


def test_a_sides_call_is_the_same_bytes_with_and_without_buses():
    name = "stereo"
    ch, fi, fo, q, frames, fed, w = CASES[name]
    S, cap = len(fed), wcap(frames, fi, fo)
    in_side, keep = storage(F32, noise(name), INTER)
    b, plain = batch(name, dm.TRIANGULAR, buses=False), batch(name, dm.TRIANGULAR, buses=False)
    try:
        for step in range(2):
            outs = []
            for bb in (b, plain):
                side, buf = out_buffer(S16, S, cap, ch, INTER)
                used, made = bb.process_sides_device(in_side, list(fed), side, cap)
                outs.append((used, made, fetched(S16, buf, S, cap, ch, INTER, max(made)).tobytes()))
            assert outs[0] == outs[1], "call %d" % step
            assert [b.get_dither(s) for s in range(S)] == [plain.get_dither(s) for s in range(S)]
            assert b.set_buses(w) == 0    # (the second round: with buses set)
    finally:
        b.close()
        plain.close()
