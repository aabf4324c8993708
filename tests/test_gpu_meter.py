"""The output meter (include/speexhip_resampler.h, "Metering") on the GPU: clip counts and peak level of what the
formatted, mixed and sides calls encode.  The expected totals never come from the meter under test: a twin state makes the
same call with output format F32 (and the same matrix), a formatted call being the float call plus a conversion, so the
twin's floats are the values the pass encoded; numpy applies the rule to them (meter_model.py), with the dither of
speexhip_debug_dither at the stream's position.  Counts and the peak's bits must match exactly.

Shapes: 44.1k -> 48k stereo q7 with 3000 input frames gives about 3265 frames -- one whole aligned 4096-sample tile of
the convert pass and a ragged tail, three whole 1024-frame tiles of the planes pass and a tail, six 512-frame tiles of the
mix pass and a tail -- and 8k -> 16k mono q7 with 160 frames stays under one tile.  The input is seeded noise at
1.3 x 32767 with one NaN and one +inf mid-stream, so both rails clip and every class of sample occurs."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import dither_model as dm
import meter_model as mm
import speexhip

pytestmark = pytest.mark.gpu

STEREO = (2, 44100, 48000, 7, 3000)
MONO = (1, 8000, 16000, 7, 160)
CONFIGS = (STEREO, MONO)
SEED = 0x5EEDFACE12345678
START = 4242          # dither position the metered states start at
F32, F32N = speexhip.FMT_F32, speexhip.FMT_F32N
DOWNMIX = ((0.75, 0.75),)                 # stereo -> mono: sums beyond full scale
ROTATE = ((0.75, 0.75), (-0.75, 0.75))     # stereo -> stereo


def wcap(frames, fi, fo):
    return frames * fo // fi + 64


@functools.lru_cache(maxsize=None)
def noise(cfg, salt=0):
    """(frames, ch) float32 in int16 units: noise at 1.3 x full scale, one NaN early in the stream, one +inf late"""
    ch, fi, fo, q, frames = cfg
    rng = np.random.default_rng(1000 + 7 * ch + salt)
    x = (rng.uniform(-1.3, 1.3, (frames, ch)) * 32767.0).astype(np.float32)
    # (q7 is 128 taps: in the 160-frame stream the two must stand this far apart for outputs that see the infinity alone)
    x[frames // 8, 0] = np.nan
    x[frames - frames // 16, ch - 1] = np.inf
    x.setflags(write=False)
    return x


def make(cfg, meter=False, kind=dm.NONE, position=START):
    ch, fi, fo, q, _ = cfg
    r = speexhip.Resampler(ch, fi, fo, q)
    if kind != dm.NONE:
        assert r.set_dither(kind, SEED, position) == 0
    if meter:
        assert r.set_meter(1) == 0
    return r


@functools.lru_cache(maxsize=None)
def twin_floats(cfg, out_mix=None, salt=0):
    """what the output pass of a call on noise(cfg) encodes: the twin's F32 result, flat, interleaved.  Computed once."""
    ch, fi, fo, q, frames = cfg
    t = make(cfg)
    try:
        rc, used, made, out = t.mix_call(noise(cfg, salt), F32, F32, None, out_mix, wcap(frames, fi, fo))
        assert rc == 0 and used == frames
        n_out = ch if out_mix is None else len(out_mix)
        y = out[: made * n_out].copy()
    finally:
        t.close()
    # the set-up: all three classes, and an infinity, really are among the samples
    assert np.isnan(y).any() and np.isinf(y).any(), "the twin's floats hold no NaN / no infinity"
    s16 = mm.totals(speexhip.FMT_S16, y)
    assert s16["clipped_high"] > 0 and s16["clipped_low"] > 0, "the twin's floats do not clip both rails"
    y.setflags(write=False)
    return y


def dither_of(fmt, kind, n, first_index, seed=SEED):
    if kind == dm.NONE or not mm.clips(fmt):
        return None
    return speexhip.debug_dither(kind, seed, first_index, n)


def expected(fmt, y, kind, c_out, position=START, seed=SEED):
    return mm.totals(fmt, y, dither_of(fmt, kind, y.size, position * c_out, seed))


def check(got, want, what):
    assert mm.same(got, want), "%s: meter %r, model %r" % (what, got, want)


# ---- 1. every output format through the formatted host call ------------------------------------------------------------
CASES = list(mm.NAMES) + ["f32n_from_f32n"]


@pytest.mark.parametrize("kind", (dm.NONE, dm.TRIANGULAR), ids=("plain", "triangular"))
@pytest.mark.parametrize("case", CASES)
def test_every_format_matches_the_model_on_the_twins_floats(case, kind):
    name = "f32n" if case == "f32n_from_f32n" else case
    fmt, _ = mm.FORMATS[name]
    for cfg in CONFIGS:
        ch, fi, fo, q, frames = cfg
        y = twin_floats(cfg)
        x = noise(cfg)
        in_fmt = F32
        if case == "f32n_from_f32n":   # (the float call on the same bytes: the result is read by meter_image, as stored * 32768)
            in_fmt, x = F32N, x * np.float32(1.0 / 32768.0)
        metered, plain = make(cfg, True, kind), make(cfg, False, kind)
        try:
            rc, used, made, out = metered.fmt_call(x, in_fmt, fmt, wcap(frames, fi, fo))
            rc_p, used_p, made_p, out_p = plain.fmt_call(x, in_fmt, fmt, wcap(frames, fi, fo))
            what = "%s %s %s" % (cfg, case, dm.KIND_NAMES[kind])
            assert (rc, used, made) == (rc_p, used_p, made_p) == (0, frames, y.size // ch), what
            assert out.tobytes() == out_p.tobytes(), what + ": the meter changed the bytes"
            got = metered.get_meter()
            assert got.pop("on") is True
            check(got, expected(fmt, y, kind, ch), what)
            assert got["samples"] == made * ch
            off = plain.get_meter()
            assert off.pop("on") is False and mm.same(off, mm.ZERO), what + ": a state with the meter off counted"
        finally:
            metered.close()
            plain.close()


def test_device_call_off_alignment_takes_the_element_path_to_the_same_totals():
    import torch
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    y, x = twin_floats(cfg), noise(cfg)
    cap = wcap(frames, fi, fo)
    src = torch.from_numpy(x.copy()).cuda()
    for fmt_name, off in (("s16", 0), ("s16", 2), ("s24", 1), ("f32", 0), ("f32", 4)):
        fmt, _ = mm.FORMATS[fmt_name]
        dst = torch.zeros(64 + cap * ch * speexhip.fmt_bytes(fmt), dtype=torch.uint8, device="cuda")
        r = make(cfg, True, dm.TRIANGULAR)
        try:
            used, made = r.process_fmt_device(F32, src.data_ptr(), frames, fmt, dst.data_ptr() + off, cap,
                                              torch.cuda.current_stream().cuda_stream)
            got = r.get_meter()   # (no synchronise: the read waits for the state's own call)
            assert got.pop("on") and (used, made) == (frames, y.size // ch)
            check(got, expected(fmt, y, dm.TRIANGULAR, ch), "%s off %d" % (fmt_name, off))
        finally:
            r.close()


# ---- 2. a mixed call and a planar output -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("s16", "s24", "u8", "ulaw", "f32n"))
def test_mixed_and_planar_outputs_match_the_model(name):
    fmt, _ = mm.FORMATS[name]
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, cap = noise(cfg), wcap(frames, fi, fo)
    for kind in (dm.NONE, dm.TRIANGULAR):
        # stereo -> mono through out_mix, interleaved
        y = twin_floats(cfg, DOWNMIX)
        r = make(cfg, True, kind)
        try:
            rc, used, made, _ = r.mix_call(x, F32, fmt, None, DOWNMIX, cap)
            assert (rc, used, made) == (0, frames, y.size)
            got = r.get_meter()
            got.pop("on")
            check(got, expected(fmt, y, kind, 1), "%s downmix %s" % (name, dm.KIND_NAMES[kind]))
        finally:
            r.close()
        # a planar output, without and with a matrix: the interleaved call's totals
        for out_mix in (None, ROTATE):
            y = twin_floats(cfg, out_mix)
            inter, planar = make(cfg, True, kind), make(cfg, True, kind)
            try:
                rc, used, made, _ = inter.sides_call(x, F32, fmt, cap, None, None, None, out_mix)
                assert (rc, used, made) == (0, frames, y.size // ch)
                rc, used, made, _ = planar.sides_call(x, F32, fmt, cap, None, "planar", None, out_mix)
                assert (rc, used, made) == (0, frames, y.size // ch)
                a, b = inter.get_meter(), planar.get_meter()
                what = "%s planar mix=%s %s" % (name, out_mix is not None, dm.KIND_NAMES[kind])
                assert a == b, what
                a.pop("on")
                check(a, expected(fmt, y, kind, ch), what)
            finally:
                inter.close()
                planar.close()


def test_planar_float_pairs_are_metered_through_the_plane_passes():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    y, x = twin_floats(cfg), noise(cfg)
    planes = np.ascontiguousarray(x.T)
    for fmt, scale in ((F32, 1.0), (F32N, 1.0 / 32768.0)):
        r, plain = make(cfg, True), make(cfg)
        try:
            rc, used, made, out = r.sides_call(planes * np.float32(scale), fmt, fmt, wcap(frames, fi, fo), "planar", "planar")
            rc_p, _, made_p, out_p = plain.sides_call(planes * np.float32(scale), fmt, fmt, wcap(frames, fi, fo), "planar", "planar")
            assert (rc, used, made) == (0, frames, y.size // ch) and (rc_p, made_p) == (0, made)
            assert out.tobytes() == out_p.tobytes()
            got = r.get_meter()
            got.pop("on")
            check(got, expected(fmt, y, dm.NONE, ch), "planar float pair %d" % fmt)
        finally:
            r.close()
            plain.close()


# ---- 3. chunk and launch invariance ------------------------------------------------------------------------------------
CUTS = (1, 159, 160, 1000, 777)   # and the rest: six ragged calls


def pieces(x):
    at, out = 0, []
    for n in CUTS:
        out.append(x[at: at + n])
        at += n
    out.append(x[at:])
    return out


@pytest.mark.parametrize("name,kind", (("s16", dm.TRIANGULAR), ("u8", dm.NONE), ("f32", dm.NONE)))
def test_totals_do_not_depend_on_chunking_or_on_what_shares_a_launch(name, kind):
    fmt, _ = mm.FORMATS[name]
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, y = noise(cfg), twin_floats(cfg)
    want = expected(fmt, y, kind, ch)
    states = []

    def fresh(meter=True, k=kind):
        states.append(make(cfg, meter, k))
        return states[-1]

    def totals(r):
        got = r.get_meter()
        assert got.pop("on")
        return got

    try:
        # one call
        whole = fresh()
        whole.process_fmt(x, F32, fmt, wcap(frames, fi, fo))
        check(totals(whole), want, "one call")
        # six ragged calls
        parts = fresh()
        for p in pieces(x):
            _, used = parts.process_fmt(p, F32, fmt, wcap(len(p), fi, fo))
            assert used == len(p)
        check(totals(parts), want, "six calls")
        # the chunks call
        chunked = fresh()
        ps = pieces(x)
        _, used = chunked.process_chunks_fmt(ps, F32, fmt, [wcap(len(p), fi, fo) for p in ps])
        assert used == [len(p) for p in ps]
        check(totals(chunked), want, "chunks call")
        # many-states calls of 7 and 33 states, formats mixed so that entries are fused: entry 0 is the stream, entry 2 the
        # stream into S24 (metered as well), the rest short neighbours with the meter off
        others = (speexhip.FMT_S24, speexhip.FMT_ULAW, speexhip.FMT_S16, F32N, speexhip.FMT_S32, speexhip.FMT_U8)
        short = noise(cfg, 1)[:500]
        for n in (7, 33):
            before = speexhip.many_counters()
            group = [fresh() if i in (0, 2) else fresh(False, dm.NONE) for i in range(n)]
            chunks = [x if i in (0, 2) else short for i in range(n)]
            out_fmts = [fmt if i == 0 else speexhip.FMT_S24 if i == 2 else others[i % len(others)] for i in range(n)]
            caps = [wcap(len(c), fi, fo) for c in chunks]
            _, used, codes = speexhip.process_many_fmt(group, chunks, F32, out_fmts, caps)
            assert used == [len(c) for c in chunks] and not any(codes)
            after = speexhip.many_counters()
            # (a metered F32 result has no pass to be judged in: that entry takes its own call, behind the fused ones)
            own = 1 if fmt == F32 else 0
            assert after["fir_launches"] - before["fir_launches"] == (n - own + 31) // 32 and \
                after["own_calls"] - before["own_calls"] == own, \
                "entries were not fused as expected: %r -> %r" % (before, after)
            check(totals(group[0]), want, "many-states call of %d" % n)
            check(totals(group[2]), expected(speexhip.FMT_S24, y, kind, ch), "many-states call of %d, entry 2" % n)
            for i in range(n):
                if i not in (0, 2):
                    off = group[i].get_meter()
                    assert off.pop("on") is False and mm.same(off, mm.ZERO), "neighbour %d of %d counted" % (i, n)
        # an entry that takes its own call (a matrix side) is metered by that call
        a, b = fresh(), fresh(False, dm.NONE)
        ym = twin_floats(cfg, DOWNMIX)
        cap = wcap(frames, fi, fo)
        xin = np.ascontiguousarray(x)
        outs = [np.zeros(cap * speexhip.fmt_bytes(fmt), np.uint8), np.zeros(cap * ch * 2, np.uint8)]
        mix, _ = speexhip._mix_matrix(DOWNMIX, ch, False)
        in_sides = [speexhip.make_side(F32, ch, data=xin.ctypes.data) for _ in range(2)]
        out_sides = [speexhip.make_side(fmt, 1, mix=mix, data=outs[0].ctypes.data),
                     speexhip.make_side(speexhip.FMT_S16, ch, data=outs[1].ctypes.data)]
        before = speexhip.many_counters()
        rc, used, made, codes = speexhip.process_many_sides([a, b], in_sides, [frames, frames], out_sides, [cap, cap])
        assert rc == 0 and not any(codes) and used == [frames, frames] and made[0] == ym.size
        assert speexhip.many_counters()["own_calls"] - before["own_calls"] == 1, "the matrix entry did not take its own call"
        check(totals(a), expected(fmt, ym, kind, 1), "many-states entry with a matrix")
        off = b.get_meter()
        assert off.pop("on") is False and mm.same(off, mm.ZERO)
    finally:
        for r in states:
            r.close()


# ---- 4. the batch device form ------------------------------------------------------------------------------------------
def test_batch_streams_are_metered_each_into_its_own_cell():
    import torch
    ch, fi, fo, q, frames = STEREO
    lens = [0, 1, 159, frames, frames]
    S = len(lens)
    xs = np.stack([noise(STEREO, 10 + s) for s in range(S)])
    cap = wcap(frames, fi, fo)
    kind = dm.TRIANGULAR
    b = speexhip.Batch(S, ch, fi, fo, q)
    twins = [make(STEREO) for _ in range(S)]
    try:
        assert b.set_dither(kind, SEED, START) == 0 and b.set_meter(1) == 0
        x = torch.from_numpy(xs).cuda()
        want = [dict(mm.ZERO) for _ in range(S)]
        pos = [START] * S
        first = None
        for call in range(2):
            ys = []
            for s in range(S):
                yt, used = twins[s].process_fmt(xs[s, : lens[s]], F32, F32, cap)
                assert used == lens[s]
                ys.append(yt)
            out, made = b.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=torch.int16)
            got = [b.get_meter(s) for s in range(S)]   # (straight behind the asynchronous call: no synchronise)
            assert made == [y.size // ch for y in ys]
            for s in range(S):
                this = mm.totals(speexhip.FMT_S16, ys[s], dither_of(speexhip.FMT_S16, kind, ys[s].size, pos[s] * ch,
                                                                    dm.stream_seed(SEED, s)))
                want[s] = mm.add(want[s], this)
                pos[s] += made[s]
                assert got[s].pop("on") is True
                check(got[s], want[s], "call %d stream %d" % (call, s))
            assert mm.same(got[0], mm.ZERO), "the idle stream counted"
            if call == 0:
                # reset clears one stream only
                first = b.get_meter(3, reset=True)
                first.pop("on")
                check(first, want[3], "the totals a reset returns")
                cleared = b.get_meter(3)
                assert cleared.pop("on") is True and mm.same(cleared, mm.ZERO)
                kept = b.get_meter(4)
                kept.pop("on")
                check(kept, want[4], "the neighbour of a reset stream")
                want[3] = dict(mm.ZERO)
        assert want[3]["samples"] > 0 and want[4]["samples"] > want[3]["samples"]
        with pytest.raises(RuntimeError):
            b.get_meter(S)
    finally:
        b.close()
        for t in twins:
            t.close()


# ---- 5. the switch -----------------------------------------------------------------------------------------------------
def test_totals_survive_the_switch_and_the_control_calls():
    cfg = STEREO
    ch, fi, fo, q, frames = cfg
    x, y = noise(cfg), twin_floats(cfg)
    want = expected(speexhip.FMT_S16, y, dm.NONE, ch)
    r = make(cfg, True)
    try:
        for bad in (-1, 2, 77):
            assert r.set_meter(bad) == speexhip.ERR_INVALID_ARG and r.get_meter()["on"] is True
        r.process_fmt(x, F32, speexhip.FMT_S16, wcap(frames, fi, fo))
        assert r.set_meter(0) == 0
        got = r.get_meter()
        assert got.pop("on") is False
        check(got, want, "after set_meter(0)")
        # with the meter off nothing is counted, and the calls that are never metered never are
        r.process_fmt(x, F32, speexhip.FMT_S16, wcap(frames, fi, fo))
        assert r.set_meter(1) == 0
        r.process(np.full((500, ch), 32767, np.int16), 600)
        r.process_float(x[:500], 600)
        assert r.set_rate(48000, 44100) == 0 and r.set_quality(5) == 0
        r.skip_zeros()
        r.reset_mem()
        assert r.set_dither(dm.TRIANGULAR, 1, 2) == 0 and r.set_dither(dm.NONE, 0, 0) == 0
        got = r.get_meter()
        assert got.pop("on") is True
        check(got, want, "after the control calls")
        # reset through the single-state call; m may be NULL with reset
        assert speexhip.lib().speexhip_resampler_get_meter(r._h, None, 1) == 0
        assert speexhip.lib().speexhip_resampler_get_meter(r._h, None, 0) == speexhip.ERR_INVALID_ARG
        got = r.get_meter()
        assert got.pop("on") is True and mm.same(got, mm.ZERO)
    finally:
        r.close()


def test_s16_to_s16_runs_as_the_float_call_while_the_meter_is_on():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = np.full((3000, ch), 32767, np.int16)
    x[::2] = -32768      # a full-scale square wave: the filter overshoots
    r, probe, twin = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    try:
        assert r.set_meter(1) == 0
        cap = 4000
        want = probe.peek(3000, cap, float_entry=True)
        rc, used, made, out = r.fmt_call(x, speexhip.FMT_S16, speexhip.FMT_S16, cap)
        assert rc == 0 and (used, made) == tuple(want)
        y, _ = twin.process_fmt(x, speexhip.FMT_S16, F32, cap)
        got = r.get_meter()
        got.pop("on")
        check(got, mm.totals(speexhip.FMT_S16, y), "s16 -> s16")
        assert got["samples"] == made * ch and got["peak"] > 0
    finally:
        for s in (r, probe, twin):
            s.close()


def test_channels_moved_apart_return_bad_state_while_the_meter_is_on():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    try:
        assert r.set_meter(1) == 0
        rc, _, _, _ = r.channel_call("float", 0, np.zeros(300, np.float32), 400)
        assert rc == 0
        before = (r.positions(), r.history().tobytes())
        raw = np.zeros(1000 * ch, np.float32)
        out = np.full(1200 * ch, 0x5A5A, np.int16)
        L = speexhip.lib()
        for device in (False, True):
            il, ol = C.c_uint32(1000), C.c_uint32(1200)
            if device:
                rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, F32, None, C.byref(il), speexhip.FMT_S16,
                                                                         C.c_void_p(out.ctypes.data), C.byref(ol), None)
            else:
                rc = L.speexhip_resampler_process_interleaved_fmt(r._h, F32, C.c_void_p(raw.ctypes.data), C.byref(il),
                                                                  speexhip.FMT_S16, C.c_void_p(out.ctypes.data), C.byref(ol))
            assert rc == speexhip.ERR_BAD_STATE and (il.value, ol.value) == (1000, 1200), device
        rc, _, _, _ = r.fmt_call(raw, F32, F32, 1200)
        assert rc == speexhip.ERR_BAD_STATE
        assert (out == 0x5A5A).all() and (r.positions(), r.history().tobytes()) == before
        got = r.get_meter()
        assert got.pop("on") is True and mm.same(got, mm.ZERO)
        # with the meter off the same state is served channel by channel, as ever
        assert r.set_meter(0) == 0
        rc, _, made, _ = r.fmt_call(raw, F32, speexhip.FMT_S16, 1200)
        assert rc == 0 and made > 0
    finally:
        r.close()


def test_zero_fallback_zeros_count_as_samples_and_clip_nothing():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    try:
        assert r.set_meter(1) == 0
        speexhip.lib().speexhip_debug_fail_device_allocs(1)
        rc = r.set_rate(32000, 48000)
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        assert rc == speexhip.ERR_ALLOC_FAILED
        x = np.full(2000 * ch, 40000.0, np.float32)
        made_all = 0
        for fmt in (speexhip.FMT_S16, speexhip.FMT_U8, F32):
            rc, used, made, out = r.fmt_call(x, F32, fmt, 2500)
            assert rc == speexhip.ERR_ALLOC_FAILED and made > 0
            made_all += made
        got = r.get_meter()
        assert got.pop("on") is True
        check(got, dict(mm.ZERO, samples=made_all * ch), "zero fallback")
    finally:
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        r.close()


# ---- 6. the Node binding -----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_meter_harness():
    """setMeter / getMeter on the class, the batch and the Transform (test/test_meter.js)"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "node-speex-resampler_amd", "test", "test_meter.js")
    p = subprocess.run(["node", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ALL NODE METER TESTS PASSED" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
