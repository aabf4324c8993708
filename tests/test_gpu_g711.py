"""G.711 mu-law and A-law in the formatted, mixed and batch calls, on the GPU.  The rule under test: a call with a
companded format on either side IS the float call on the decoded (and mixed) input followed by the output mix and the
encoder -- the S16 output rule, dithered or not, then the G.711 compressor.  Decoder, encoder, mix and dither are exact
statements (g711_model.py, sample_formats.py, channel_mix.py, dither_model.py), so every comparison with a twin state
driven through the existing float call is equality of bytes."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest

import channel_mix as cm
import dither_model as dm
import g711_model as gm
import oracle as orc
import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_formats import storage_of
from test_gpu_planar import MODES, same_state, wcap

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 8000, 16000, 7), (2, 44100, 48000, 7), (1, 8000, 48000, 3)]
SENTINEL = speexhip.Resampler.SENTINEL_BYTE
SEED = 0xDEADBEEFCAFEF00D
FMT_IDS = [gm.name(f) for f in gm.ALL]
KIND_IDS = [dm.KIND_NAMES[k] for k in dm.KINDS]


def storage(fmt, n, seed, quiet=False, all_codes=False):
    """n samples of format fmt, the companded ones included: the bytes of full-scale LCG noise (or of a quiet stretch)
    through the model's encoder; all_codes: the first 256 samples are the 256 codes"""
    if fmt not in gm.COMPANDED:
        return storage_of(fmt, n, seed, quiet)
    codes = gm.from_internal(fmt, storage_of(sf.F32, n, seed, quiet))
    if all_codes:
        assert n >= 256
        codes[:256] = np.arange(256, dtype=np.uint8)
    return codes


def frames_of(fmt, raw, ch):
    return raw.size // gm.per_sample(fmt) // ch


def check_tail(out, fmt, made, c_out, what):
    raw = out.view(np.uint8)
    assert (raw[made * c_out * gm.nbytes(fmt):] == SENTINEL).all(), what + ": written past produced"


def device_call(r, in_fmt, raw, out_fmt, cap, c_in, c_out, in_off, out_off, torch, in_mix=None, out_mix=None):
    """formatted / mixed device call with the input `in_off` and the output `out_off` bytes off a 16-byte boundary, guard
    bytes around the output (checked); returns (consumed, produced, output bytes)"""
    src = torch.zeros(64 + raw.nbytes + 64, dtype=torch.uint8, device="cuda")
    src[16 + in_off: 16 + in_off + raw.nbytes] = torch.from_numpy(raw.view(np.uint8).copy()).cuda()
    room = cap * c_out * gm.nbytes(out_fmt)
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    frames = frames_of(in_fmt, raw, c_in)
    stream = torch.cuda.current_stream().cuda_stream
    if in_mix is None and out_mix is None:
        used, made = r.process_fmt_device(in_fmt, src.data_ptr() + 16 + in_off, frames, out_fmt,
                                          dst.data_ptr() + 16 + out_off, cap, stream)
    else:
        used, made = r.process_mix_device(in_fmt, src.data_ptr() + 16 + in_off, frames, out_fmt,
                                          dst.data_ptr() + 16 + out_off, cap, in_mix, out_mix, stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    n = made * c_out * gm.nbytes(out_fmt)
    lo = 16 + out_off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "bytes outside the produced samples written"
    return used, made, flat[lo: lo + n].copy()


# ---- 1. the twin, byte for byte --------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", gm.ALL, ids=FMT_IDS)
@pytest.mark.parametrize("mode", ("default", "exact"))
def test_companded_call_equals_the_float_twin(mode, in_fmt):
    """a companded input to every output format, every other input to the two companded outputs (ULAW <-> ALAW and
    ULAW -> ULAW among them): counters, bytes, the untouched tail, position and final state are the float twin's"""
    out_fmts = gm.ALL if in_fmt in gm.COMPANDED else gm.COMPANDED
    for cfg in CONFIGS:
        ch, fi, fo, q = cfg
        # (frames or None for silence, capacity, silent frames, quiet)
        calls = [(1, 8, 0, False), (15, 100, 0, False), (16, 100, 0, False), (17, 110, 0, False),
                 (160, wcap(160, fi, fo), 0, False), (4097, wcap(4097, fi, fo), 0, True),
                 (0, 64, 0, False),                       # an empty call
                 (None, 600, 480, False),                 # silence
                 (5000, 777, 0, False),                   # a capacity that binds
                 (20000, wcap(20000, fi, fo), 0, False)]
        mk = lambda: speexhip.Resampler(ch, fi, fo, q, mode=MODES[mode])
        states = {o: mk() for o in out_fmts}
        twin = mk()
        got = {o: [] for o in out_fmts}
        fed = []
        try:
            for i, (frames, cap, silent, quiet) in enumerate(calls):
                raw = None if frames is None else storage(in_fmt, frames * ch, 31 * ch + q + 17 * i, quiet,
                                                          all_codes=in_fmt in gm.COMPANDED and frames * ch >= 256)
                x = None if raw is None else gm.to_internal(in_fmt, raw)
                rc_t, used_t, made_t, out_t = twin.raw_call("float", x, cap, silent)
                y = out_t[:made_t].reshape(-1)
                if raw is not None and in_fmt in gm.COMPANDED:
                    fed.append(raw[: used_t * ch])
                for o, r in states.items():
                    what = "%s mode=%s %s->%s call %d (%s frames, cap %d)" % (cfg, mode, gm.name(in_fmt), gm.name(o), i, frames, cap)
                    rc, used, made, out = r.fmt_call(raw, in_fmt, o, cap, silent)
                    assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
                    per = ch * gm.per_sample(o)
                    assert out[: made * per].tobytes() == gm.from_internal(o, y).tobytes(), what + ": samples"
                    check_tail(out, o, made, ch, what)
                    assert r.position() == twin.position(), what
                    got[o].append(out[: made * per].copy())
            for o, r in states.items():
                same_state(r, twin, "%s mode=%s %s->%s" % (cfg, mode, gm.name(in_fmt), gm.name(o)))
        finally:
            for r in list(states.values()) + [twin]:
                r.close()
        if in_fmt in gm.COMPANDED:
            assert np.unique(np.concatenate(fed)).size == 256, (cfg, "the input holds every code")
        # full-scale noise reaches both rails of each companded output
        for o in gm.COMPANDED:
            codes = np.concatenate(got[o])
            lo, hi = gm.RAILS[o]
            assert (codes == lo).any() and (codes == hi).any(), (cfg, mode, gm.name(in_fmt), gm.name(o))


# ---- 2. addressing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(gm.ULAW, gm.ALAW), (gm.ALAW, gm.ULAW)], ids=["ulaw-alaw", "alaw-ulaw"])
def test_companded_addressing_offsets_tails_and_guards(pair):
    """whole 4096-sample tiles plus a tail, both sides at byte offsets 0..15 off a 16-byte boundary: offset 0 takes the
    16-bytes-per-lane path, every other the element path -- one answer"""
    import torch
    in_fmt, out_fmt = pair
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37
    cap = wcap(frames, fi, fo)
    raw = storage(in_fmt, frames * ch, 77 + in_fmt, all_codes=True)
    t = speexhip.Resampler(*cfg)
    y, used_t = t.process_float(gm.to_internal(in_fmt, raw).reshape(-1, ch), cap)
    want = gm.from_internal(out_fmt, y).tobytes()
    assert y.shape[0] * ch > 2 * 4096      # (whole tiles on the way out as well)
    for off in range(16):
        r = speexhip.Resampler(*cfg)
        used, made, got = device_call(r, in_fmt, raw, out_fmt, cap, ch, ch, off, off, torch)
        what = (gm.name(in_fmt), gm.name(out_fmt), off)
        assert (used, made) == (used_t, y.shape[0]), what
        assert got.tobytes() == want, what
        same_state(r, t, str(what))
        r.close()
    # one side aligned, the other not: each pass chooses for itself
    for in_off, out_off in ((0, 5), (9, 0)):
        r = speexhip.Resampler(*cfg)
        used, made, got = device_call(r, in_fmt, raw, out_fmt, cap, ch, ch, in_off, out_off, torch)
        assert (used, made) == (used_t, y.shape[0]) and got.tobytes() == want, (in_off, out_off)
        r.close()
    t.close()


# ---- 3. batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(gm.ULAW, sf.F32N), (sf.S16, gm.ALAW)], ids=["ulaw-f32n", "s16-alaw"])
def test_companded_batch_equals_single_states(pair):
    import torch
    in_fmt, out_fmt = pair
    S, ch, fi, fo, q, T = 5, 2, 44100, 48000, 7, 9000
    bi, bo = gm.nbytes(in_fmt), gm.nbytes(out_fmt)
    lens = [T - 611 * s for s in range(S)]
    cap = wcap(T, fi, fo)
    raws = [storage(in_fmt, T * ch, 900 + s, all_codes=True) for s in range(S)]
    in_stride, out_stride = T * ch + 5, cap * ch + 3   # samples; odd strides put the streams at every alignment
    src = torch.zeros(S * in_stride * bi, dtype=torch.uint8, device="cuda")
    for s in range(S):
        src[s * in_stride * bi: s * in_stride * bi + raws[s].nbytes] = torch.from_numpy(raws[s].view(np.uint8).copy()).cuda()
    dst = torch.full((S * out_stride * bo,), SENTINEL, dtype=torch.uint8, device="cuda")
    b = speexhip.Batch(S, ch, fi, fo, q)
    used, made = b.process_fmt_device(in_fmt, src.data_ptr(), in_stride, lens, out_fmt, dst.data_ptr(), out_stride, cap,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    for s in range(S):
        r = speexhip.Resampler(ch, fi, fo, q)
        want, used_r = r.process_fmt(raws[s][: lens[s] * ch], in_fmt, out_fmt, cap)
        t = speexhip.Resampler(ch, fi, fo, q)
        y, _ = t.process_float(gm.to_internal(in_fmt, raws[s][: lens[s] * ch]).reshape(-1, ch), cap)
        assert want.tobytes() == gm.from_internal(out_fmt, y).tobytes(), s     # (the single state is the model's)
        n = want.nbytes
        assert (used[s], made[s] * ch * bo) == (used_r, n), s
        lo = s * out_stride * bo
        assert flat[lo: lo + n].tobytes() == want.tobytes(), s
        assert (flat[lo + n: lo + out_stride * bo] == SENTINEL).all(), s
        assert b.lines(s).tobytes() == r._lines().tobytes(), s
        r.close()
        t.close()
    b.close()


def test_process_tensor_takes_named_formats():
    import torch
    S, ch, fi, fo, q, T = 3, 1, 8000, 16000, 7, 6000
    cap = wcap(T, fi, fo)
    # (input format, in_format=, out_format=, out_dtype=, normalized, the output format that makes)
    cases = [(gm.ULAW, gm.ULAW, None, torch.float32, True, sf.F32N),
             (gm.ALAW, gm.ALAW, gm.ULAW, None, False, gm.ULAW),
             (sf.S16, None, gm.ALAW, None, False, gm.ALAW),
             (gm.ULAW, gm.ULAW, gm.ULAW, None, False, gm.ULAW),
             (sf.U8, None, None, None, False, sf.U8)]            # without the keywords: what it was
    for in_fmt, in_format, out_format, out_dtype, normalized, out_fmt in cases:
        raws = [storage(in_fmt, T * ch, 500 + s, all_codes=in_fmt in gm.COMPANDED) for s in range(S)]
        x = torch.from_numpy(np.stack(raws).reshape(S, T, ch)).cuda()
        b = speexhip.Batch(S, ch, fi, fo, q)
        out, made = b.process_tensor(x, out_capacity=cap, out_dtype=out_dtype, normalized=normalized, in_format=in_format,
                                     out_format=out_format)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.shape == (S, max(made), ch) and got.dtype == gm.dtype(out_fmt)
        for s in range(S):
            t = speexhip.Resampler(ch, fi, fo, q)
            y, _ = t.process_float(gm.to_internal(in_fmt, raws[s]).reshape(-1, ch), cap)
            assert made[s] == y.shape[0]
            assert got[s, : made[s]].tobytes() == gm.from_internal(out_fmt, y).tobytes(), (gm.name(in_fmt), gm.name(out_fmt), s)
            assert b.lines(s).tobytes() == t._lines().tobytes(), s
            t.close()
        b.close()
    b = speexhip.Batch(1, 1, fi, fo, q)
    with pytest.raises(ValueError):      # a format names its storage type
        b.process_tensor(torch.zeros((1, 100, 1), dtype=torch.int16, device="cuda"), in_format=gm.ULAW)
    b.close()


# ---- 4. mixed calls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(gm.ULAW, sf.F32N, True), (gm.ULAW, gm.ALAW, True), (sf.S16, gm.ALAW, False),
                                  (gm.ULAW, gm.ALAW, False)],
                         ids=["2-1-1-ulaw-f32n", "2-1-1-ulaw-alaw", "1-1-2-s16-alaw", "1-1-2-ulaw-alaw"])
def test_companded_mixed_calls_equal_the_model_around_the_float_twin(case):
    """(in, state, out) channels (2, 1, 1) with a companded input -- mix_in's tile path on whole 512-frame tiles and its
    element path on the tail and off alignment -- and (1, 1, 2) with a companded output"""
    import torch
    in_fmt, out_fmt, down = case
    fi, fo, q = 8000, 16000, 7
    in_mix, out_mix = (cm.STEREO_TO_MONO, None) if down else (None, cm.MONO_TO_STEREO)
    c_in, c_out = (2, 1) if down else (1, 2)
    frames = 512 * 2 + 37
    cap = wcap(frames, fi, fo)
    r, t = speexhip.Resampler(1, fi, fo, q), speexhip.Resampler(1, fi, fo, q)
    for i, (route, in_off, out_off) in enumerate((("host", 0, 0), ("device", 0, 0), ("device", 3, 7), ("device", 0, 1))):
        raw = storage(in_fmt, frames * c_in, 60 + i, all_codes=in_fmt in gm.COMPANDED)
        x = gm.to_internal(in_fmt, raw)
        xin = x if in_mix is None else cm.mix(in_mix, x).reshape(-1)
        rc_t, used_t, made_t, out_t = t.raw_call("float", xin, cap)
        y = out_t[:made_t].reshape(-1)
        yout = y if out_mix is None else cm.mix(out_mix, y).reshape(-1)
        want = gm.from_internal(out_fmt, yout)
        what = (gm.name(in_fmt), gm.name(out_fmt), c_in, c_out, route, in_off, out_off)
        if route == "host":
            rc, used, made, out = r.mix_call(raw, in_fmt, out_fmt, in_mix, out_mix, cap)
            assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
            assert out[: made * c_out].tobytes() == want.tobytes(), what
            check_tail(out, out_fmt, made, c_out, str(what))
        else:
            used, made, got = device_call(r, in_fmt, raw, out_fmt, cap, c_in, c_out, in_off, out_off, torch, in_mix, out_mix)
            assert (used, made) == (used_t, made_t), what
            assert got.tobytes() == want.view(np.uint8).tobytes(), what
        same_state(r, t, str(what))
    r.close()
    t.close()


# ---- 5. dither -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dm.KINDS, ids=KIND_IDS)
def test_dithered_companded_outputs_equal_the_model(kind):
    """the noise joins at the int16 stage, at the stream's position: host calls, both paths of the device call, and a
    mixed call whose index runs over the output frame's samples"""
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37
    cap = wcap(frames, fi, fo)
    raw = storage_of(sf.F32, frames * ch, 91)
    t = speexhip.Resampler(*cfg)
    y, used_t = t.process_float(raw.reshape(-1, ch), cap)
    start = 77777
    for o in gm.COMPANDED:
        want = gm.from_internal_dither(o, y, kind, SEED, start, ch)
        assert want.tobytes() != gm.from_internal(o, y).tobytes()
        for off in (None, 0, 1):   # host; device aligned (16 bytes per lane); one byte off (element path)
            r = speexhip.Resampler(*cfg)
            assert r.set_dither(kind, SEED, start) == 0
            what = (dm.KIND_NAMES[kind], gm.name(o), off)
            if off is None:
                rc, used, made, out = r.fmt_call(raw, sf.F32, o, cap)
                assert rc == 0
                got = out[: made * ch]
                check_tail(out, o, made, ch, str(what))
            else:
                used, made, got = device_call(r, sf.F32, raw, o, cap, ch, ch, 0, off, torch)
            assert (used, made) == (used_t, y.shape[0]), what
            assert got.tobytes() == want.tobytes(), what
            assert r.get_dither() == (kind, SEED, start + made), what      # the position advances
            same_state(r, t, str(what))
            r.close()
    t.close()
    # mixed: a mono state, 1 -> 2 out_mix, and a 2 -> 1 in_mix with a companded input
    fi, fo = 8000, 16000
    for in_fmt, in_mix, out_mix in ((sf.S16, None, cm.MONO_TO_STEREO), (gm.ALAW, cm.STEREO_TO_MONO, None)):
        c_in = 1 if in_mix is None else 2
        c_out = 1 if out_mix is None else 2
        for o in gm.COMPANDED:
            r, t = speexhip.Resampler(1, fi, fo, q), speexhip.Resampler(1, fi, fo, q)
            r.set_dither(kind, SEED, 5)
            pos = 5
            for i, n in enumerate((333, 1500)):
                rawm = storage(in_fmt, n * c_in, 70 + i)
                x = gm.to_internal(in_fmt, rawm)
                xin = x if in_mix is None else cm.mix(in_mix, x).reshape(-1)
                rc_t, used_m, made_m, out_t = t.raw_call("float", xin, wcap(n, fi, fo))
                ym = out_t[:made_m].reshape(-1)
                yout = ym if out_mix is None else cm.mix(out_mix, ym).reshape(-1)
                rc, used, made, out = r.mix_call(rawm, in_fmt, o, in_mix, out_mix, wcap(n, fi, fo))
                assert (rc, used, made) == (0, used_m, made_m)
                assert out[: made * c_out].tobytes() == gm.from_internal_dither(o, yout, kind, SEED, pos, c_out).tobytes(), \
                    (dm.KIND_NAMES[kind], gm.name(in_fmt), gm.name(o), i)
                pos += made
                assert r.get_dither() == (kind, SEED, pos)
            r.close()
            t.close()


def test_dithered_companded_bytes_do_not_depend_on_the_chunking():
    ch, fi, fo, q = 1, 8000, 16000, 7
    frames = 6000
    x = storage(gm.ULAW, frames * ch, 23, all_codes=True)
    cuts = [1, 159, 160, 17, 4097, 16]
    cuts.append(frames - sum(cuts))
    assert len(cuts) == 7 and cuts[-1] > 0
    for o in gm.COMPANDED:
        for kind in dm.KINDS:
            whole, parts = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
            whole.set_dither(kind, 11, 0)
            parts.set_dither(kind, 11, 0)
            a, used = whole.process_fmt(x, gm.ULAW, o, wcap(frames, fi, fo))
            assert used == frames
            got, at = [], 0
            for n in cuts:
                b, used = parts.process_fmt(x[at * ch: (at + n) * ch], gm.ULAW, o, wcap(n, fi, fo))
                assert used == n
                got.append(b)
                at += n
            assert np.concatenate(got).tobytes() == a.tobytes(), (gm.name(o), dm.KIND_NAMES[kind])
            assert whole.get_dither() == parts.get_dither() == (kind, 11, a.size // ch)
            same_state(whole, parts, "whole against parts")
            whole.close()
            parts.close()


def test_channels_moved_apart_with_companded_formats():
    """BAD_STATE with dither on, the state untouched; channel by channel without it"""
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    r.set_dither(dm.TRIANGULAR, 1, 10)
    rc, _, _, _ = r.channel_call("float", 0, np.zeros(300, np.float32), 400)
    assert rc == 0
    before = (r.positions(), r.history().tobytes())
    raw = storage(gm.ULAW, 1000 * ch, 2)
    for in_fmt, out_fmt in ((gm.ULAW, gm.ALAW), (sf.F32, gm.ULAW)):
        rc, used, made, out = r.fmt_call(raw if in_fmt == gm.ULAW else storage_of(sf.F32, 1000 * ch, 2), in_fmt, out_fmt, 1200)
        assert rc == speexhip.ERR_BAD_STATE and (used, made) == (1000, 1200), gm.name(out_fmt)
        assert (out.view(np.uint8) == SENTINEL).all()
    assert r.get_dither() == (dm.TRIANGULAR, 1, 10)
    assert (r.positions(), r.history().tobytes()) == before
    # without dither: each channel is the float per-channel call on the decoded samples, encoded
    assert r.set_dither(dm.NONE, 0, 0) == 0
    t = speexhip.Resampler(ch, fi, fo, q)
    t.channel_call("float", 0, np.zeros(300, np.float32), 400)
    rc, used, made, out = r.fmt_call(raw, gm.ULAW, gm.ALAW, 1200)
    assert rc == 0
    x = gm.to_internal(gm.ULAW, raw).reshape(-1, ch)
    got = out.reshape(1200, ch)
    for c in range(ch):
        rc_c, used_c, made_c, out_c = t.channel_call("float", c, np.ascontiguousarray(x[:, c]), 1200)
        assert rc_c == 0
        assert got[:made_c, c].tobytes() == gm.from_internal(gm.ALAW, out_c[:made_c]).tobytes(), c
        assert (got[made_c:, c] == SENTINEL).all(), c
    assert (used, made) == (used_c, made_c)      # (the call reports the last channel's lengths)
    assert r.positions() == t.positions()
    r.close()
    t.close()


# ---- 6. edges --------------------------------------------------------------------------------------------------------
def test_zero_fallback_writes_the_formats_zero():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = storage(gm.ALAW, 3000 * ch, 5)
    for out_fmt in gm.COMPANDED:
        p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
        try:
            p.process_fmt(x, gm.ALAW, out_fmt, wcap(3000, fi, fo))
            t.process_float(gm.to_internal(gm.ALAW, x).reshape(-1, ch), wcap(3000, fi, fo))
            for r in (p, t):
                speexhip.lib().speexhip_debug_fail_device_allocs(1)
                rc = r.set_rate(32000, 48000)
                speexhip.lib().speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            y = storage(gm.ALAW, 2000 * ch, 6)
            rc_t, used_t, made_t, out_t = t.raw_call("float", gm.to_internal(gm.ALAW, y).reshape(-1, ch), 2500)
            rc_p, used_p, made_p, out_p = p.fmt_call(y, gm.ALAW, out_fmt, 2500)
            assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
            assert not out_t[:made_t].any()
            assert (out_p[: made_p * ch] == gm.ZERO[out_fmt]).all(), gm.name(out_fmt)      # 0xFF / 0xD5
            check_tail(out_p, out_fmt, made_p, ch, gm.name(out_fmt))
            assert p.positions() == t.positions()
        finally:
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            p.close()
            t.close()


def test_non_finite_float_input_to_companded_outputs():
    """+-inf and NaN out of the FIR: the rails and the format's zero (the direct filter of test_gpu_formats.py)"""
    ch, fi, fo, q = 1, 16000, 48000, 7
    n = 6000
    x = orc.lcg_pcm(n, 8).astype(np.float32)
    x[1000], x[2500], x[4000], x[4001] = np.inf, -np.inf, np.inf, -np.inf
    t = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    y, _ = t.process_float(x.reshape(-1, 1), wcap(n, fi, fo))
    t.close()
    y = y.reshape(-1)
    assert np.isposinf(y).any() and np.isneginf(y).any() and np.isnan(y).any()
    for out_fmt in gm.COMPANDED:
        for kind in (dm.NONE, dm.TRIANGULAR):
            r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
            r.set_dither(kind, 3, 0)
            got, _ = r.process_fmt(x, sf.F32, out_fmt, wcap(n, fi, fo))
            r.close()
            assert got.tobytes() == gm.from_internal_dither(out_fmt, y, kind, 3, 0, 1).tobytes(), gm.name(out_fmt)
            lo, hi = gm.RAILS[out_fmt]
            assert (got[np.isnan(y)] == gm.ZERO[out_fmt]).all()
            assert (got[np.isposinf(y)] == hi).all() and (got[np.isneginf(y)] == lo).all()


def test_formats_6_and_15_are_still_unknown():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    raw = storage(gm.ULAW, 2000 * ch, 3)
    r.process_fmt(raw, gm.ULAW, gm.ALAW, 2300)
    t.process_fmt(raw, gm.ULAW, gm.ALAW, 2300)
    before = (r.positions(), r.history().tobytes())
    L = speexhip.lib()
    buf = np.zeros(2300 * ch * 4, np.uint8)
    m = cm.STEREO_TO_MONO
    for in_fmt, out_fmt in ((6, gm.ULAW), (gm.ALAW, 15), (15, 6), (7, gm.ALAW), (gm.ULAW, 18)):
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = L.speexhip_resampler_process_interleaved_fmt(r._h, in_fmt, C.c_void_p(raw.ctypes.data), C.byref(il), out_fmt,
                                                          C.c_void_p(buf.ctypes.data), C.byref(ol))
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
        rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, in_fmt, None, C.byref(il), out_fmt,
                                                                 C.c_void_p(buf.ctypes.data), C.byref(ol), None)
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
        rc = L.speexhip_resampler_process_interleaved_mix(r._h, in_fmt, ch, None, C.c_void_p(raw.ctypes.data), C.byref(il),
                                                          out_fmt, 1, C.c_void_p(m.ctypes.data), C.c_void_p(buf.ctypes.data),
                                                          C.byref(ol))
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
    assert not buf.any()
    assert (r.positions(), r.history().tobytes()) == before
    got, _ = r.process_fmt(raw, gm.ULAW, gm.ALAW, 2300)      # ... and the stream goes on as its twin's
    want, _ = t.process_fmt(raw, gm.ULAW, gm.ALAW, 2300)
    assert got.tobytes() == want.tobytes()
    r.close()
    t.close()


def test_companded_host_routes_give_the_device_calls_bytes():
    """pageable (small: the bounce buffers; large: the runtime's staged copy) and speexhip_block_acquire blocks on both
    sides, against the device-pointer call"""
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    for in_fmt, out_fmt, frames in ((gm.ULAW, gm.ALAW, 3000), (gm.ALAW, sf.F32N, 200000), (sf.S16, gm.ULAW, 400000)):
        raw = storage(in_fmt, frames * ch, 60 + frames % 7, all_codes=in_fmt in gm.COMPANDED)
        cap = wcap(frames, fi, fo)
        rd = speexhip.Resampler(*cfg)
        used_d, made_d, want = device_call(rd, in_fmt, raw, out_fmt, cap, ch, ch, 0, 0, torch)
        out_bytes = cap * ch * gm.nbytes(out_fmt)
        what = (gm.name(in_fmt), gm.name(out_fmt), frames)
        r = speexhip.Resampler(*cfg)
        got, used = r.process_fmt(raw, in_fmt, out_fmt, cap)
        assert used == used_d and got.view(np.uint8).tobytes() == want.tobytes(), what + ("pageable",)
        same_state(r, rd, "pageable")
        r.close()
        r = speexhip.Resampler(*cfg)
        with speexhip.PinnedBlock(raw.nbytes) as bin_, speexhip.PinnedBlock(out_bytes) as bout:
            a_in, a_out = bin_.array(np.uint8, (raw.nbytes,)), bout.array(np.uint8, (out_bytes,))
            a_in[:] = raw.view(np.uint8)
            a_out[:] = SENTINEL
            il, ol = C.c_uint32(frames), C.c_uint32(cap)
            rc = speexhip.lib().speexhip_resampler_process_interleaved_fmt(
                r._h, in_fmt, C.c_void_p(a_in.ctypes.data), C.byref(il), out_fmt, C.c_void_p(a_out.ctypes.data), C.byref(ol))
            assert (rc, il.value, ol.value) == (0, used_d, made_d), what + ("blocks",)
            assert a_out[: want.nbytes].tobytes() == want.tobytes() and (a_out[want.nbytes:] == SENTINEL).all(), what + ("blocks",)
        same_state(r, rd, "blocks")
        r.close()
        rd.close()


# ---- 7. Node ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_process_chunk_format_with_companded_formats():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_g711.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL G711 NODE TESTS PASSED" in res.stdout


# ---- 8. cost ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_companded_batch_call_is_not_slower_than_decoding_with_torch():
    """8 kHz -> 16 kHz mono q7, 32 streams x 2^20 frames, device-resident, mu-law in and float32 in +-1.0 out.  Yardstick:
    what a caller does today in the same process on the same buffers -- a 256-entry float table gathered in torch
    (lut[x.long()]), the float batch call, out.mul_(1 / 32768).  The formatted call may be slower than that route by no
    more than the route's own run-to-run spread (max / min of five medians)."""
    import torch
    S, ch, fi, fo, q, T = 32, 1, 8000, 16000, 7, 1 << 20
    cap = wcap(T, fi, fo)
    x = torch.randint(0, 256, (S, T, ch), dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(gm.decode(gm.ULAW, np.arange(256, dtype=np.uint8))).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    fmt, flt = speexhip.Batch(S, ch, fi, fo, q), speexhip.Batch(S, ch, fi, fo, q)
    out_f = torch.empty((S, cap, ch), dtype=torch.float32, device="cuda")
    out_d = torch.empty((S, cap, ch), dtype=torch.float32, device="cuda")

    def formatted_call():
        return fmt.process_fmt_device(gm.ULAW, x.data_ptr(), T * ch, T, sf.F32N, out_f.data_ptr(), cap * ch, cap, stream)

    def diy_call():
        xf = lut[x.long()]
        _, made = flt.process_device(xf.data_ptr(), T * ch, T, out_d.data_ptr(), cap * ch, cap, stream, float_io=True)
        return out_d[:, : made[0]].mul_(1.0 / 32768.0)

    # (one answer from both routes before either is timed)
    _, made = formatted_call()
    want = diy_call()
    torch.cuda.synchronize()
    assert torch.equal(out_f[:, : made[0]], want)

    def median_ms(fn, reps=7):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    for _ in range(2):
        formatted_call()
        diy_call()
    diy, mine = [], []
    for _ in range(5):  # interleaved in time, so that a clock change hits both
        diy.append(median_ms(diy_call))
        mine.append(median_ms(formatted_call))
    spread = max(diy) / min(diy)
    print("mu-law formatted %.3f ms (medians %s), torch route %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(diy), ["%.3f" % v for v in diy], spread))
    fmt.close()
    flt.close()
    assert statistics.median(mine) <= statistics.median(diy) * spread
