"""The per-stream output gain (include/speexhip_resampler.h, "Gain") on the GPU.  The expected bytes never come from the
code under test: a twin state makes the same call with output format F32 and no gain -- a formatted call being the float
call plus a conversion, and a stream's floats not depending on how it is cut into calls -- the numpy model
(gain_model.py) multiplies the twin's floats by g of each output frame, and the format models (halfbe_model.py) encode
the products, with the dither of the stream's position; meter_model.py judges them.  Bytes, counters, meter totals and
the bits of get_gain are compared for equality.  One allowance, for the float formats alone and only where the product
MAKES a NaN of a value that was none (inf * 0): there the library's value must be a NaN, but its sign and payload are not
compared -- IEEE 754 leaves the NaN an invalid operation generates to the implementation, and the CPU under numpy and the
GPU choose different signs.  A NaN that the gain merely passes on (NaN * g) is compared bit for bit like any value.

Shapes: 44.1k -> 48k stereo q7 with 3000 input frames gives about 3265 frames -- one whole 4096-sample convert tile and
a tail, three 1024-frame plane tiles, six 512-frame mix tiles; 8k -> 16k mono q7 with 160 frames stays under one tile;
16k -> 48k of three channels q5 with 1500 frames gives 13 500 samples -- three convert tiles and a tail, with frames that
straddle a lane's 16-byte group.  The input is the meter tests' noise at 1.3 x full scale with one NaN and one +inf."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import dither_model as dm
import gain_model as gm
import halfbe_model as hm
import meter_model as mm
import speexhip

pytestmark = pytest.mark.gpu

STEREO = (2, 44100, 48000, 7, 3000)
MONO = (1, 8000, 16000, 7, 160)
TRIPLE = (3, 16000, 48000, 5, 1500)
CONFIGS = (STEREO, MONO, TRIPLE)
SEED = 0x5EEDFACE12345678
START = 4242          # dither position the dithered states start at
F32, F32N, S16 = speexhip.FMT_F32, speexhip.FMT_F32N, speexhip.FMT_S16
DOWNMIX = ((0.75, 0.75),)                 # stereo -> mono: sums beyond full scale
ROTATE = ((0.75, 0.75), (-0.75, 0.75))     # stereo -> stereo
FLOATS = (F32, F32N, speexhip.FMT_F16N, speexhip.FMT_BF16N)


def wcap(frames, fi, fo):
    return frames * fo // fi + 64


@functools.lru_cache(maxsize=None)
def noise(cfg, salt=0):
    """(frames, ch) float32 in int16 units: noise at 1.3 x full scale, one NaN early in the stream, one +inf late"""
    ch, fi, fo, q, frames = cfg
    rng = np.random.default_rng(1000 + 7 * ch + salt)
    x = (rng.uniform(-1.3, 1.3, (frames, ch)) * 32767.0).astype(np.float32)
    x[frames // 8, 0] = np.nan
    x[frames - frames // 16, ch - 1] = np.inf
    x.setflags(write=False)
    return x


def make(cfg, kind=dm.NONE, meter=False):
    ch, fi, fo, q, _ = cfg
    r = speexhip.Resampler(ch, fi, fo, q)
    if kind != dm.NONE:
        assert r.set_dither(kind, SEED, START) == 0
    if meter:
        assert r.set_meter(1) == 0
    return r


@functools.lru_cache(maxsize=None)
def twin_floats(cfg, out_mix=None, salt=0):
    """what the output pass of a call on noise(cfg) encodes before the gain: an ungained twin's F32 result, flat,
    interleaved.  Computed once."""
    ch, fi, fo, q, frames = cfg
    t = make(cfg)
    try:
        rc, used, made, out = t.mix_call(noise(cfg, salt), F32, F32, None, out_mix, wcap(frames, fi, fo))
        assert rc == 0 and used == frames
        n_out = ch if out_mix is None else len(out_mix)
        y = out[: made * n_out].copy()
    finally:
        t.close()
    assert np.isnan(y).any() and np.isinf(y).any(), "the twin's floats hold no NaN / no infinity"
    y.setflags(write=False)
    return y


class Gained(np.ndarray):
    """the model's values (or their storage bytes) with `born`: per sample, whether the product made a NaN of a value
    that was none.  Views keep it."""
    born = None

    def __array_finalize__(self, obj):
        self.born = getattr(obj, "born", None)


def gained(y, gains, c_out):
    """gain_model.apply, remembering where a NaN was born"""
    yg = gm.apply(y, gains, c_out).view(Gained)
    yg.born = np.isnan(yg) & ~np.isnan(np.asarray(y, np.float32).reshape(-1))
    return yg


def encode(fmt, yg, kind, c_out, position=START, seed=SEED):
    """the model's storage bytes of gained floats yg (a stream from output frame `position` on)"""
    if kind == dm.NONE or not hm.dithered(fmt):
        st = hm.from_internal(fmt, yg)
    else:
        st = hm.from_internal_dither(fmt, yg, kind, seed, position, c_out)
    out = np.ascontiguousarray(hm.raw(fmt, st)).view(Gained)
    out.born = getattr(yg, "born", None)
    return out


def same_storage(fmt, got, want, what):
    """bytes equal; for the float formats a NaN born of the product is matched by any NaN (module docstring)"""
    born = getattr(want, "born", None)
    got, want = np.asarray(got, np.uint8).reshape(-1), np.asarray(want, np.uint8).reshape(-1)
    assert got.size == want.size, "%s: %d bytes, model %d" % (what, got.size, want.size)
    if fmt in FLOATS and born is not None and born.any():
        b = hm.nbytes(fmt)
        vg = hm.to_internal(fmt, got.view(hm.dtype(fmt)))
        assert born.size == vg.size and np.isnan(vg[born]).all(), what + ": no NaN where the product makes one"
        keep = np.repeat(~born, b)
        got, want = got[keep], want[keep]
    if got.tobytes() != want.tobytes():
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first difference at byte %d of %d (%d differ)" % (what, at, got.size, int((got != want).sum())))


def stored(fmt, out, samples):
    return hm.raw(fmt, out)[: samples * hm.nbytes(fmt)]


def report(r, stream=None):
    g = r.get_gain() if stream is None else r.get_gain(stream)
    return (np.float32(g["current"]).tobytes(), np.float32(g["target"]).tobytes(), g["remaining"])


# ---- the ramps the tests draw from --------------------------------------------------------------------------------
# a scenario: the stream's input cut into calls (frames of the leading pieces; the rest is the last call) and the
# set_gain(gain, ramp_frames) made before piece i
def tile_edge(cfg):
    """output frames at which a tile of the flat converting pass ends on a frame boundary"""
    ch = cfg[0]
    return {1: 64, 2: 2048, 3: 4096}[ch]   # (mono stays under a tile: any frame)


def scenario(cfg, name):
    ch, fi, fo, q, frames = cfg
    short = frames // 11               # a short first call: some 300 output frames of the stereo stream
    if name in ("half", "minus", "mute"):
        return (), {0: ({"half": 0.5, "minus": -1.0, "mute": 0.0}[name], 0)}
    if name == "one":
        return (), {0: (0.25, 1)}
    if name == "mid":
        # begins before the main call and ends at an odd frame inside its first tile, in mid-lane-group
        probe = make(cfg)
        try:
            made0 = probe.peek(short, wcap(short, fi, fo), float_entry=True)[1]
        finally:
            probe.close()
        return (short,), {0: (0.3, made0 + (777 if frames > 1000 else 77))}
    if name == "edge":
        return (), {0: (1.5, tile_edge(cfg))}
    if name == "long":
        return (frames // 2,), {0: (-0.5, 100000)}
    raise KeyError(name)


def drive(r, cfg, x, in_fmt, out_fmt, cuts, events, model, call=None, c_out=None):
    """the stream x through r in the scenario's calls (c_out: samples of an output frame, the state's channels unless a
    matrix says otherwise); returns (the output's bytes, the gains of its frames)"""
    ch, fi, fo, q, _ = cfg
    at, outs, gains = 0, [], []
    bounds = list(cuts) + [len(x) - sum(cuts)]
    for i, n in enumerate(bounds):
        if i in events:
            assert r.set_gain(*events[i]) == 0
            model.set(*events[i])
        piece = x[at: at + n]
        at += n
        if call is None:
            rc, used, made, out = r.fmt_call(piece, in_fmt, out_fmt, wcap(n, fi, fo))
        else:
            rc, used, made, out = call(r, piece, wcap(n, fi, fo))
        assert rc == 0 and used == n, (rc, used, n)
        outs.append(stored(out_fmt, out, made * (ch if c_out is None else c_out)))
        gains.append(model.take(made))
        assert report(r) == model.report(), "get_gain after call %d" % i
    return np.concatenate(outs), np.concatenate(gains)


# ---- 1. every output format through the formatted host call ------------------------------------------------------------
@pytest.mark.parametrize("kind", (dm.NONE, dm.TRIANGULAR), ids=("plain", "triangular"))
@pytest.mark.parametrize("ramp", ("half", "mid"))
@pytest.mark.parametrize("name", mm.NAMES)
def test_every_format_equals_the_model_on_the_twins_floats(name, ramp, kind):
    fmt, _ = mm.FORMATS[name]
    for cfg in CONFIGS:
        ch, fi, fo, q, frames = cfg
        y, x = twin_floats(cfg), noise(cfg)
        cuts, events = scenario(cfg, ramp)
        r, model = make(cfg, kind), gm.State()
        try:
            got, gains = drive(r, cfg, x, F32, fmt, cuts, events, model)
            what = "%s %s %s %s" % (cfg, name, ramp, dm.KIND_NAMES[kind])
            assert gains.size == y.size // ch, what
            if ramp == "mid":
                assert model.done == model.total and (np.diff(gains) != 0).sum() > 50, what + ": the ramp did not run"
            same_storage(fmt, got, encode(fmt, gained(y, gains, ch), kind, ch), what)
        finally:
            r.close()


def test_s16_to_s16_follows_the_float_entrys_counters_while_gain_is_on():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x = np.full((frames, ch), 32767, np.int16)
    x[::2] = -32768      # a full-scale square wave: the filter overshoots
    r, probe, twin = make(cfg), make(cfg), make(cfg)
    try:
        cap = 3000        # (too small for the whole input: the two entries' counter rules differ)
        assert r.set_gain(0.5, 1000) == 0
        want = probe.peek(frames, cap, float_entry=True)
        rc, used, made, out = r.fmt_call(x, S16, S16, cap)
        assert rc == 0 and (used, made) == tuple(want)
        y, _ = twin.process_fmt(x, S16, F32, cap)
        gains = gm.g(1.0, 0.5, 1000, 0, made)
        same_storage(S16, stored(S16, out, made * ch), encode(S16, gained(y, gains, ch), dm.NONE, ch), "s16 -> s16")
    finally:
        for s in (r, probe, twin):
            s.close()


# ---- 2. a device call off 16-byte alignment ----------------------------------------------------------------------------
def test_device_call_off_alignment_takes_the_element_path_to_the_same_bytes():
    import torch
    for cfg, ramp in ((STEREO, "edge"), (TRIPLE, "one"), (TRIPLE, "edge")):
        ch, fi, fo, q, frames = cfg
        y, x = twin_floats(cfg), noise(cfg)
        cap = wcap(frames, fi, fo)
        src = torch.from_numpy(x.copy()).cuda()
        _, events = scenario(cfg, ramp)
        for fmt_name, off in (("s16", 0), ("s16", 2), ("s24", 1), ("ulaw", 3), ("f32n", 4), ("f32", 0), ("f32", 4)):
            fmt, _ = mm.FORMATS[fmt_name]
            dst = torch.zeros(64 + cap * ch * speexhip.fmt_bytes(fmt), dtype=torch.uint8, device="cuda")
            r, model = make(cfg, dm.TRIANGULAR), gm.State()
            try:
                assert r.set_gain(*events[0]) == 0
                model.set(*events[0])
                used, made = r.process_fmt_device(F32, src.data_ptr(), frames, fmt, dst.data_ptr() + off, cap,
                                                  torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert (used, made) == (frames, y.size // ch)
                gains = model.take(made)
                assert report(r) == model.report()
                got = dst.cpu().numpy()[off: off + made * ch * speexhip.fmt_bytes(fmt)]
                same_storage(fmt, got, encode(fmt, gained(y, gains, ch), dm.TRIANGULAR, ch),
                             "%s %s %s off %d" % (cfg, ramp, fmt_name, off))
            finally:
                r.close()


# ---- 3. mixed and planar outputs: the gain sits behind the matrix ------------------------------------------------------
def planar_bytes(fmt, out, made):
    """the planes of a planar result, plane after plane, as bytes"""
    b = hm.nbytes(fmt)
    raw = np.ascontiguousarray(out).view(np.uint8).reshape(out.shape[0], -1)
    return raw[:, : made * b]


def as_planes(fmt, inter_bytes, c_out):
    b = hm.nbytes(fmt)
    born = getattr(inter_bytes, "born", None)
    out = np.ascontiguousarray(np.asarray(inter_bytes, np.uint8).reshape(-1, c_out, b).transpose(1, 0, 2)).reshape(c_out, -1).view(Gained)
    out.born = None if born is None else np.ascontiguousarray(born.reshape(-1, c_out).T).reshape(-1)
    return out


@pytest.mark.parametrize("name", ("s16", "s24", "u8", "ulaw", "f32n", "f32", "bf16n"))
def test_mixed_and_planar_outputs_equal_the_model(name):
    fmt, _ = mm.FORMATS[name]
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, cap = noise(cfg), wcap(frames, fi, fo)
    for kind, ramp in ((dm.NONE, "long"), (dm.TRIANGULAR, "edge"), (dm.NONE, "minus")):
        cuts, events = scenario(cfg, ramp)
        # stereo -> mono through out_mix, interleaved (mix_out)
        y = twin_floats(cfg, DOWNMIX)
        r, model = make(cfg, kind), gm.State()
        try:
            got, gains = drive(r, cfg, x, F32, fmt, cuts, events, model, c_out=1,
                               call=lambda s, p, c: s.mix_call(p, F32, fmt, None, DOWNMIX, c))
            same_storage(fmt, got, encode(fmt, gained(y, gains, 1), kind, 1),
                         "%s downmix %s %s" % (name, ramp, dm.KIND_NAMES[kind]))
        finally:
            r.close()
        # a planar output, without and with a matrix (planes_out), in one call
        for out_mix in (None, ROTATE):
            y = twin_floats(cfg, out_mix)
            r, model = make(cfg, kind), gm.State()
            try:
                assert r.set_gain(*events[0]) == 0
                model.set(*events[0])
                rc, used, made, out = r.sides_call(x, F32, fmt, cap, None, "planar", None, out_mix)
                assert (rc, used, made) == (0, frames, y.size // ch)
                want = encode(fmt, gained(y, model.take(made), ch), kind, ch)
                what = "%s planar mix=%s %s %s" % (name, out_mix is not None, ramp, dm.KIND_NAMES[kind])
                same_storage(fmt, planar_bytes(fmt, out, made), as_planes(fmt, want, ch), what)
                assert report(r) == model.report(), what
            finally:
                r.close()


def test_three_planes_equal_the_model():
    cfg = TRIPLE
    ch, fi, fo, q, frames = cfg
    x, y, cap = noise(cfg), twin_floats(cfg), wcap(frames, fi, fo)
    for name, kind, ramp in (("s16", dm.TRIANGULAR, "edge"), ("s24", dm.NONE, "one"), ("f32", dm.NONE, "half")):
        fmt, _ = mm.FORMATS[name]
        _, events = scenario(cfg, ramp)
        r, model = make(cfg, kind), gm.State()
        try:
            assert r.set_gain(*events[0]) == 0
            model.set(*events[0])
            rc, used, made, out = r.sides_call(x, F32, fmt, cap, None, "planar")
            assert (rc, used, made) == (0, frames, y.size // ch)
            want = encode(fmt, gained(y, model.take(made), ch), kind, ch)
            same_storage(fmt, planar_bytes(fmt, out, made), as_planes(fmt, want, ch), "three planes %s %s" % (name, ramp))
        finally:
            r.close()


# ---- 4. the pairs no output pass writes: gain_image ----------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (F32, F32N), ids=("f32", "f32n"))
def test_float_pairs_are_multiplied_in_place_and_judged_in_the_same_pass(fmt):
    import torch
    scale = np.float32(1.0 if fmt == F32 else 1.0 / 32768.0)
    for cfg, ramp in ((STEREO, "mid"), (STEREO, "edge"), (MONO, "one"), (TRIPLE, "long"), (TRIPLE, "mute")):
        ch, fi, fo, q, frames = cfg
        x = noise(cfg) * scale
        cap = wcap(frames, fi, fo)
        cuts, events = scenario(cfg, ramp)
        twin = make(cfg)
        try:
            rc, used, made_all, out = twin.fmt_call(x, fmt, fmt, cap)   # the stored floats, ungained
            assert rc == 0 and used == frames
            y = out[: made_all * ch].copy()
        finally:
            twin.close()
        # host, with the meter on
        r, model = make(cfg, meter=True), gm.State()
        try:
            got, gains = drive(r, cfg, x, fmt, fmt, cuts, events, model)
            want = gained(y, gains, ch)      # (F32N: the stored value times g)
            what = "%s %s fmt %d" % (cfg, ramp, fmt)
            same_storage(F32, got, want.view(np.uint8), what)
            m = r.get_meter()
            assert m.pop("on") is True
            with np.errstate(over="ignore", invalid="ignore"):
                judged = want * np.float32(32768.0) if fmt == F32N else want
            assert mm.same(m, mm.totals(fmt, judged)), "%s: meter %r, model %r" % (what, m, mm.totals(fmt, judged))
        finally:
            r.close()
        # device, in one call, off and on 16-byte alignment
        src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        for off in (0, 4):
            dst = torch.zeros(64 + cap * ch * 4, dtype=torch.uint8, device="cuda")
            r, model = make(cfg), gm.State()
            try:
                assert r.set_gain(*events[0]) == 0
                model.set(*events[0])
                used, made = r.process_fmt_device(fmt, src.data_ptr(), frames, fmt, dst.data_ptr() + off, cap,
                                                  torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert (used, made) == (frames, made_all)
                want = gained(y, model.take(made), ch)
                same_storage(F32, dst.cpu().numpy()[off: off + made * ch * 4], want.view(np.uint8), "%s device off %d" % (what, off))
            finally:
                r.close()


def test_planar_float_pairs_go_through_the_plane_passes():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    y, x = twin_floats(cfg), noise(cfg)
    planes = np.ascontiguousarray(x.T)
    _, events = scenario(cfg, "edge")
    for fmt, scale in ((F32, 1.0), (F32N, 1.0 / 32768.0)):
        r, model = make(cfg, meter=True), gm.State()
        try:
            assert r.set_gain(*events[0]) == 0
            model.set(*events[0])
            rc, used, made, out = r.sides_call(planes * np.float32(scale), fmt, fmt, wcap(frames, fi, fo), "planar", "planar")
            assert (rc, used, made) == (0, frames, y.size // ch)
            yg = gained(y, model.take(made), ch)
            same_storage(fmt, planar_bytes(fmt, out, made), as_planes(fmt, encode(fmt, yg, dm.NONE, ch), ch), "planar pair %d" % fmt)
            m = r.get_meter()
            m.pop("on")
            assert mm.same(m, mm.totals(fmt, yg)), (m, mm.totals(fmt, yg))
        finally:
            r.close()


# ---- 5. chunking and launch invariance -----------------------------------------------------------------------------------
def cut(x):
    """the stream in pieces of 1, 159 and the rest"""
    return [x[:1], x[1:160], x[160:]]


@pytest.mark.parametrize("name,kind,ramp", (("s16", dm.TRIANGULAR, "edge"), ("ulaw", dm.NONE, "long"), ("f32", dm.NONE, "mid"),
                                            ("s24", dm.NONE, "one")))
def test_bytes_gain_and_totals_do_not_depend_on_chunking_or_on_what_shares_a_launch(name, kind, ramp):
    fmt, _ = mm.FORMATS[name]
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, y = noise(cfg), twin_floats(cfg)
    gain, total = scenario(cfg, ramp)[1][0]
    model = gm.State()
    model.set(gain, total)
    yg = gained(y, model.take(y.size // ch), ch)
    want_bytes = encode(fmt, yg, kind, ch)
    want_meter = mm.totals(fmt, yg, None if kind == dm.NONE or not mm.clips(fmt) else
                           speexhip.debug_dither(kind, SEED, START * ch, yg.size))
    want_report = model.report()
    states = []

    def fresh(on=True):
        r = make(cfg, kind if on else dm.NONE, meter=on)
        states.append(r)
        if on:
            assert r.set_gain(gain, total) == 0
        return r

    def check(r, got, what):
        same_storage(fmt, got, want_bytes, what)
        assert report(r) == want_report, what + ": get_gain"
        m = r.get_meter()
        assert m.pop("on") is True and mm.same(m, want_meter), "%s: meter %r, model %r" % (what, m, want_meter)

    try:
        whole = fresh()
        out, _ = whole.process_fmt(x, F32, fmt, wcap(frames, fi, fo))
        check(whole, hm.raw(fmt, out), "one call")
        parts = fresh()
        outs = [parts.process_fmt(p, F32, fmt, wcap(len(p), fi, fo))[0] for p in cut(x)]
        check(parts, np.concatenate([hm.raw(fmt, o) for o in outs]), "three calls")
        chunked = fresh()
        ps = cut(x)
        outs, used = chunked.process_chunks_fmt(ps, F32, fmt, [wcap(len(p), fi, fo) for p in ps])
        assert used == [len(p) for p in ps]
        check(chunked, np.concatenate([hm.raw(fmt, o) for o in outs]), "chunks call")
        # a many-states call of 7: entry 0 is the stream, the rest short ungained neighbours in other formats
        others = (speexhip.FMT_S24, speexhip.FMT_ULAW, S16, F32N, speexhip.FMT_S32, speexhip.FMT_U8)
        short = noise(cfg, 1)[:500]
        group = [fresh() if i == 0 else fresh(False) for i in range(7)]
        chunks = [x if i == 0 else short for i in range(7)]
        out_fmts = [fmt if i == 0 else others[i % len(others)] for i in range(7)]
        before = speexhip.many_counters()
        outs, used, codes = speexhip.process_many_fmt(group, chunks, F32, out_fmts, [wcap(len(c), fi, fo) for c in chunks])
        after = speexhip.many_counters()
        assert used == [len(c) for c in chunks] and not any(codes)
        # (a METERED F32 result takes its own call, as before this feature; gain alone takes no entry out of a group)
        own = 1 if fmt == F32 else 0
        assert after["own_calls"] - before["own_calls"] == own and after["fir_launches"] - before["fir_launches"] == 1
        check(group[0], hm.raw(fmt, outs[0]), "many-states entry")
        # the neighbours' bytes are those of separate ungained calls
        for i in range(1, 7):
            alone = fresh(False)
            o, _ = alone.process_fmt(short, F32, out_fmts[i], wcap(500, fi, fo))
            assert hm.raw(out_fmts[i], outs[i]).tobytes() == hm.raw(out_fmts[i], o).tobytes(), "neighbour %d" % i
            assert report(group[i]) == gm.State().report()
    finally:
        for r in states:
            r.close()


# ---- 6. a batch: every stream at its own gain ------------------------------------------------------------------------------
def test_batch_streams_each_at_their_own_gain_and_ramp_stage():
    import torch
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    lens = [0, 1, 159, frames, frames]
    S = len(lens)
    xs = np.stack([noise(cfg, 10 + s) for s in range(S)])
    cap = wcap(frames, fi, fo)
    kind = dm.TRIANGULAR
    b, plain = speexhip.Batch(S, ch, fi, fo, q), speexhip.Batch(S, ch, fi, fo, q)
    twins = [make(cfg) for _ in range(S)]
    models = [gm.State() for _ in range(S)]
    sets = {0: (0.5, 100), 1: (0.5, 0), 2: (0.25, 1000), 4: (-1.0, 2048)}   # stream 3 stays at unity
    try:
        for bb in (b, plain):
            assert bb.set_dither(kind, SEED, START) == 0
        for s, (gain, ramp) in sets.items():
            assert b.set_gain(gain, ramp, stream=s) == 0
            models[s].set(gain, ramp)
        assert b.set_gain(0.5, 0, stream=S) == speexhip.ERR_INVALID_ARG
        x = torch.from_numpy(xs).cuda()
        pos = [START] * S
        for call in range(2):
            out, made = b.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=torch.int16)
            out_p, made_p = plain.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=torch.int16)
            assert made == made_p
            out, out_p = out.cpu().numpy(), out_p.cpu().numpy()
            for s in range(S):
                yt, used = twins[s].process_fmt(xs[s, : lens[s]], F32, F32, cap)
                assert used == lens[s] and made[s] == yt.size // ch
                gains = models[s].take(made[s])
                want = encode(S16, gained(yt, gains, ch), kind, ch, pos[s], dm.stream_seed(SEED, s))
                got = np.ascontiguousarray(out[s, : made[s]]).view(np.uint8)
                same_storage(S16, got, want, "call %d stream %d" % (call, s))
                pos[s] += made[s]
                assert report(b, s) == models[s].report(), "call %d stream %d: get_gain" % (call, s)
            # the unity stream's bytes are those of the ungained batch; the idle stream's ramp has not moved
            assert out[3, : made[3]].tobytes() == out_p[3, : made[3]].tobytes()
            assert report(b, 0) == (np.float32(1.0).tobytes(), np.float32(0.5).tobytes(), 100)
        assert models[2].done > 0 and models[4].done == models[4].total
        # ... NaN payloads and signed zeros included: F32 out, where the unity stream is not multiplied at all
        odd = xs.copy()
        odd[3, 100, 0] = np.frombuffer(np.uint32(0x7FA12345).tobytes(), np.float32)[0]   # a signalling NaN with a payload
        xo = torch.from_numpy(odd).cuda()
        o1, m1 = b.process_tensor(xo, out_capacity=cap, in_frames=lens, out_dtype=torch.float32, out_format=F32, in_format=F32)
        o2, m2 = plain.process_tensor(xo, out_capacity=cap, in_frames=lens, out_dtype=torch.float32, out_format=F32, in_format=F32)
        assert m1 == m2
        assert o1[3, : m1[3]].cpu().numpy().tobytes() == o2[3, : m2[3]].cpu().numpy().tobytes()
        with pytest.raises(RuntimeError):
            b.get_gain(S)
    finally:
        b.close()
        plain.close()
        for t in twins:
            t.close()


# ---- 7. the many-states call: per-entry gains, entries stay fused ----------------------------------------------------------
def test_many_states_entries_keep_their_group_with_gain_on():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, y = noise(cfg), twin_floats(cfg)
    cap = wcap(frames, fi, fo)
    fmts = (S16, speexhip.FMT_ULAW, speexhip.FMT_S24, speexhip.FMT_U8, F32N, speexhip.FMT_S32BE)
    gains = ((0.5, 0), (0.3, 1077), (-1.0, 2048), None, (0.0, 1), (1.5, 100000))   # entry 3 is not gained
    group = [make(cfg) for _ in fmts]
    alone = [make(cfg) for _ in fmts]
    try:
        for r, a, g in zip(group, alone, gains):
            if g is not None:
                assert r.set_gain(*g) == 0 and a.set_gain(*g) == 0
        before = speexhip.many_counters()
        outs, used, codes = speexhip.process_many_fmt(group, [x] * len(fmts), F32, list(fmts), [cap] * len(fmts))
        after = speexhip.many_counters()
        assert used == [frames] * len(fmts) and not any(codes)
        delta = {k: after[k] - before[k] for k in after}
        assert delta == {"fir_launches": 1, "in_passes": 0, "out_passes": 1, "own_calls": 0}, delta
        for i, fmt in enumerate(fmts):
            o, _ = alone[i].process_fmt(x, F32, fmt, cap)
            assert hm.raw(fmt, outs[i]).tobytes() == hm.raw(fmt, o).tobytes(), "entry %d differs from its separate call" % i
            model = gm.State()
            if gains[i] is not None:
                model.set(*gains[i])
            want = encode(fmt, gained(y, model.take(y.size // ch), ch), dm.NONE, ch)
            same_storage(fmt, hm.raw(fmt, outs[i]), want, "entry %d" % i)
            assert report(group[i]) == model.report() == report(alone[i])
        # entries whose gained result no pass of the group writes stay fused as well: S16 -> S16 between its two passes,
        # F32 -> F32 multiplied in place by one more kernel over the group
        xi = np.clip(np.nan_to_num(x, nan=0.0, posinf=32767.0), -32768, 32767).astype(np.int16)
        a, bq = make(cfg), make(cfg)
        ta, tb = make(cfg), make(cfg)
        group += [a, bq, ta, tb]
        assert a.set_gain(0.5, 777) == 0 and bq.set_gain(-0.25, 0) == 0
        before = speexhip.many_counters()
        outs, used, codes = speexhip.process_many_fmt([a, bq], [xi, x], [S16, F32], [S16, F32], [cap, cap])
        after = speexhip.many_counters()
        assert used == [frames, frames] and not any(codes)
        assert after["own_calls"] == before["own_calls"] and after["fir_launches"] - before["fir_launches"] == 1
        ya, _ = ta.process_fmt(xi, S16, F32, cap)
        same_storage(S16, hm.raw(S16, outs[0]), encode(S16, gained(ya, gm.g(1.0, 0.5, 777, 0, ya.size // ch), ch), dm.NONE, ch),
                     "fused s16 -> s16")
        same_storage(F32, hm.raw(F32, outs[1]), gained(y, np.full(y.size // ch, -0.25, np.float32), ch).view(np.uint8),
                     "fused f32 -> f32")
    finally:
        for r in group + alone:
            r.close()


# ---- 8. the switch -----------------------------------------------------------------------------------------------------------
def test_what_does_not_touch_the_gain_and_the_return_to_off():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    r, twin = make(cfg), make(cfg)
    try:
        assert report(r) == gm.State().report()
        assert r.set_gain(0.5, 1000) == 0
        model = gm.State()
        model.set(0.5, 1000)
        for bad in (np.nan, np.inf, -np.inf):
            assert r.set_gain(bad, 10) == speexhip.ERR_INVALID_ARG and report(r) == model.report()
        # the calls that are never gained, and the control calls
        xi = np.full((500, ch), 1000, np.int16)
        out, _ = r.process(xi, 600)
        out_t, _ = twin.process(xi, 600)
        assert out.tobytes() == out_t.tobytes(), "the int16 call was gained"
        xf = noise(cfg)[:400].copy()
        assert r.process_float(xf[:100], 200)[0].tobytes() == twin.process_float(xf[:100], 200)[0].tobytes()
        assert r.set_rate(48000, 44100) == 0 and r.set_quality(5) == 0
        r.skip_zeros()
        r.reset_mem()
        assert r.set_dither(dm.TRIANGULAR, 1, 2) == 0 and r.set_dither(dm.NONE, 0, 0) == 0
        assert r.set_meter(1) == 0 and r.set_meter(0) == 0
        assert report(r) == model.report()
        # NULL pointers are allowed one by one
        cur = C.c_float()
        assert speexhip.lib().speexhip_resampler_get_gain(r._h, C.byref(cur), None, None) == 0 and cur.value == 1.0
        assert speexhip.lib().speexhip_resampler_get_gain(r._h, None, None, None) == 0
    finally:
        r.close()
        twin.close()
    # after a ramp back to 1.0 an S16 -> S16 call is the int16 call again: its bytes and its counter rule
    r, twin, probe = make(cfg), make(cfg), make(cfg)
    try:
        x = np.full((frames, ch), 32767, np.int16)
        x[::2] = -32768
        a, bq, c = x[:1000], x[1000:2000], x[2000:]
        assert r.set_gain(0.5, 0) == 0
        r.process_fmt(a, S16, S16, 1200)
        assert r.set_gain(1.0, 10) == 0
        r.process_fmt(bq, S16, S16, 1200)
        assert report(r) == gm.State().report(), "a ramp that ended at 1.0 did not return the state to off"
        for t in (twin, probe):
            t.process_fmt(a, S16, F32, 1200)
            t.process_fmt(bq, S16, F32, 1200)
        cap = 900   # (too small: the int16 entry's counter rule shows)
        want = probe.peek(len(c), cap, float_entry=False)
        rc, used, made, out = r.fmt_call(c, S16, S16, cap)
        assert rc == 0 and (used, made) == tuple(want)
        out_t, used_t = twin.process(c, cap)
        assert used_t == used and stored(S16, out, made * ch).tobytes() == np.ascontiguousarray(out_t).view(np.uint8).tobytes()
    finally:
        for s in (r, twin, probe):
            s.close()


def test_the_calls_that_are_never_gained_neither_apply_the_gain_nor_move_the_ramp():
    """int16, float, planar, per-channel, chunks_int / _float, many_int / _float and take calls on states with a ramp in
    flight: the bytes of ungained twins, and get_gain's bits the same before and after each."""
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    rng = np.random.default_rng(77)
    xf = (rng.uniform(-1.0, 1.0, (600, ch)) * 30000.0).astype(np.float32)
    xi = xf.astype(np.int16)
    r, r2, t, t2 = make(cfg), make(cfg), make(cfg), make(cfg)
    try:
        assert r.set_gain(0.5, 100000) == 0 and r2.set_gain(-2.0, 7) == 0
        model, model2 = gm.State(), gm.State()
        model.set(0.5, 100000)
        model2.set(-2.0, 7)
        before = (report(r), report(r2))
        assert before == (model.report(), model2.report())

        def both(what, call):
            a, b = call(r, r2), call(t, t2)
            flat_a = [np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else v for v in a]
            flat_b = [np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else v for v in b]
            assert flat_a == flat_b, what + ": a gained state's result differs from an ungained twin's"
            assert (report(r), report(r2)) == before, what + ": get_gain moved"

        def flatten(outs, *rest):
            return list(outs) + list(rest)

        both("int16 call", lambda s, _: list(s.process(xi[:200], 300)))
        both("float call", lambda s, _: list(s.process_float(xf[:200], 300)))
        both("planar int16 call", lambda s, _: list(s.process_planar(np.ascontiguousarray(xi[200:400].T), 300)))
        both("planar float call", lambda s, _: list(s.process_planar(np.ascontiguousarray(xf[200:400].T), 300, float_io=True)))
        # (both channels by the same amount: the channels stand together again behind the pair of calls)
        both("per-channel calls", lambda s, _: [v for c in range(ch) for v in s.channel_call("float", c, xf[400:500, c], 200)])
        both("chunks_int", lambda s, _: flatten(*s.process_chunks([xi[:1], xi[1:160], xi[160:300]], [8, 200, 200])))
        both("chunks_float", lambda s, _: flatten(*s.process_chunks([xf[:1], xf[1:160], xf[160:300]], [8, 200, 200], np.float32)))
        both("many_int", lambda s, s2: flatten(*speexhip.process_many([s, s2], [xi[300:500], xi[:333]], [300, 400])))
        both("many_float", lambda s, s2: flatten(*speexhip.process_many([s, s2], [xf[300:500], xf[:333]], [300, 400], np.float32)))
        both("int16 take", lambda s, _: list(s.process_take(xi[500:], 200)))
        both("float take", lambda s, _: list(s.process_take(xf[500:], 200, float_io=True)))
        # the ramps stand where they stood: the next formatted call starts them at index 0
        for s, tw, m in ((r, t, model), (r2, t2, model2)):
            yt, _ = tw.process_fmt(xf[:300], F32, F32, 400)
            out, _ = s.process_fmt(xf[:300], F32, S16, 400)
            same_storage(S16, hm.raw(S16, out), encode(S16, gained(yt, m.take(yt.size // ch), ch), dm.NONE, ch), "behind them")
            assert report(s) == m.report()
    finally:
        for s in (r, r2, t, t2):
            s.close()


def test_s16_to_s16_of_a_batch_with_one_gained_stream_follows_the_state():
    """The routes follow the state: while one stream's gain is on, S16 -> S16 of every stream of the batch runs as the
    float call between the two conversions -- the ungained stream too, with the float entry's counters and the bytes of
    that call, unmultiplied.  The two entries' counter rules part where frames are pending behind a change to a shorter
    filter and a call brings no input: the float entry drains them, the int16 entry makes nothing."""
    import torch
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x = np.full((2, frames, ch), 32767, np.int16)
    x[:, ::2] = -32768      # a full-scale square wave: the filter overshoots
    x[1, ::3] = 12345
    cap = wcap(frames, fi, fo)
    b = speexhip.Batch(2, ch, fi, fo, q)
    probe, twins = make(cfg), [make(cfg), make(cfg)]
    models = [gm.State(), gm.State()]
    try:
        assert b.set_gain(0.5, 100000, stream=1) == 0
        models[1].set(0.5, 100000)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.zeros((2, cap, ch), dtype=torch.int16, device="cuda")
        for in_frames, room in ((frames, cap), (0, 64)):
            want = tuple(probe.peek(in_frames, room, float_entry=True))
            if in_frames == 0:
                assert b.info(0)["magic_samples"] > 0 and want[1] > 0
                assert want != tuple(probe.peek(in_frames, room, float_entry=False)), "the set-up does not tell the two rules apart"
            used, made = b.process_fmt_device(S16, d_in.data_ptr(), frames * ch, in_frames, S16, d_out.data_ptr(), cap * ch, room,
                                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            for s in range(2):
                assert (used[s], made[s]) == want, "stream %d, %d frames in" % (s, in_frames)
                rc, used_t, made_t, y = twins[s].fmt_call(x[s, :in_frames], S16, F32, room)
                assert rc == 0 and (used_t, made_t) == want
                gains = models[s].take(made[s])
                same_storage(S16, np.ascontiguousarray(out[s, : made[s]]).view(np.uint8),
                             encode(S16, gained(y[: made_t * ch], gains, ch), dm.NONE, ch), "stream %d, %d frames in" % (s, in_frames))
                assert report(b, s) == models[s].report()
            probe.process_fmt(x[0, :in_frames], S16, F32, room)
            if in_frames:
                # a shorter filter: frames of the history become pending
                assert b.set_quality(3) == 0 and probe.set_quality(3) == 0 and all(t.set_quality(3) == 0 for t in twins)
    finally:
        b.close()
        for s in [probe] + twins:
            s.close()


# ---- 9. while gain is on -----------------------------------------------------------------------------------------------------
def test_channels_moved_apart_return_bad_state_while_gain_is_on():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    try:
        assert r.set_gain(0.5, 100) == 0
        rc, _, _, _ = r.channel_call("float", 0, np.zeros(300, np.float32), 400)
        assert rc == 0
        before = (r.positions(), r.history().tobytes(), report(r))
        raw = np.zeros(1000 * ch, np.float32)
        out = np.full(1200 * ch, 0x5A5A, np.int16)
        L = speexhip.lib()
        for device in (False, True):
            il, ol = C.c_uint32(1000), C.c_uint32(1200)
            if device:
                rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, F32, None, C.byref(il), S16,
                                                                         C.c_void_p(out.ctypes.data), C.byref(ol), None)
            else:
                rc = L.speexhip_resampler_process_interleaved_fmt(r._h, F32, C.c_void_p(raw.ctypes.data), C.byref(il),
                                                                  S16, C.c_void_p(out.ctypes.data), C.byref(ol))
            assert rc == speexhip.ERR_BAD_STATE and (il.value, ol.value) == (1000, 1200), device
        rc, _, _, _ = r.fmt_call(raw, F32, F32, 1200)
        assert rc == speexhip.ERR_BAD_STATE
        assert (out == 0x5A5A).all() and (r.positions(), r.history().tobytes(), report(r)) == before
        # with the gain back at unity the same state is served channel by channel, as ever
        assert r.set_gain(1.0, 0) == 0
        rc, _, made, _ = r.fmt_call(raw, F32, S16, 1200)
        assert rc == 0 and made > 0
    finally:
        r.close()


def test_zero_fallback_zeros_are_multiplied_like_any_value():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    try:
        assert r.set_gain(-1.0, 0) == 0
        speexhip.lib().speexhip_debug_fail_device_allocs(1)
        rc = r.set_rate(32000, 48000)
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        assert rc == speexhip.ERR_ALLOC_FAILED
        x = np.full(2000 * ch, 40000.0, np.float32)
        for fmt in (F32, speexhip.FMT_U8, S16, speexhip.FMT_ULAW):
            rc, used, made, out = r.fmt_call(x, F32, fmt, 2500)
            assert rc == speexhip.ERR_ALLOC_FAILED and made > 0
            got = stored(fmt, out, made * ch)
            if fmt == F32:
                want = np.full(made * ch, -0.0, np.float32).view(np.uint8)   # 0 * negative is -0.0f, stored as it is
            else:
                want = np.tile(hm.zero(fmt), made * ch)
            assert got.tobytes() == want.tobytes(), "zero fallback, format %d" % fmt
    finally:
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        r.close()


# ---- 10. a new target in mid-ramp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("s16", "f32"))
def test_retarget_in_mid_ramp_is_continuous(name):
    fmt, _ = mm.FORMATS[name]
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, y = noise(cfg), twin_floats(cfg)
    r, model = make(cfg), gm.State()
    try:
        events = {0: (0.2, 3000), 1: (0.9, 500), 2: (-0.3, 0)}
        firsts = []

        def call(s, p, c):
            # (straight behind set_gain: current is debug_gain at the ramp's index, and the new ramp's `from`)
            g = s.get_gain()
            want = speexhip.debug_gain(model.frm, model.to, model.total, model.done, 1)[0]
            assert np.float32(g["current"]).tobytes() == np.float32(want).tobytes()
            # (a ramp begins at the gain the next frame would have had; ramp_frames = 0 is a step at that frame)
            assert np.float32(g["current"]).tobytes() == np.float32(model.frm if model.total else model.to).tobytes()
            firsts.append(np.float32(g["current"]))
            return s.fmt_call(p, F32, fmt, c)

        got, gains = drive(r, cfg, x, F32, fmt, (1000, 1000), events, model, call=call)
        same_storage(fmt, got, encode(fmt, gained(y, gains, ch), dm.NONE, ch), "retarget " + name)
        # the first re-target took the ramp where it stood (between 1.0 and 0.2); the second is a step
        assert np.float32(0.2) < firsts[1] < np.float32(1.0) and firsts[2] == np.float32(-0.3)
        assert (gains == firsts[1]).any() and gains[-1] == np.float32(-0.3)
    finally:
        r.close()


# ---- 11. the Node binding ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_gain_harness():
    """setGain / getGain on the class, the batch and the Transform (test/test_gain.js)"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "node-speex-resampler_amd", "test", "test_gain.js")
    p = subprocess.run(["node", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ALL NODE GAIN TESTS PASSED" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
