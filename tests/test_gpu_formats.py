"""Formatted calls on the GPU: the caller names the sample format of the input and of the output (u8, s16, packed s24,
s32, float in int16 units, float in +-1.0).  The rule under test: a formatted call IS the float call on the converted
input followed by the output conversion -- both conversions are exact statements (sample_formats.py), so every comparison
with a twin state driven through the float call is equality of bytes.  S16 -> S16 is the int16 call and F32N -> F32N the
float call on the same bytes."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest

import exact_model as em
import oracle as orc
import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_planar import FAMILIES, MODES, same_state, wcap

pytestmark = pytest.mark.gpu

# one configuration per kernel family, stereo, plus mono, 3 and 8 channels on the BASELINE ratio
CONFIGS = [f[:4] for f in FAMILIES] + [(1, 44100, 48000, 7), (3, 44100, 48000, 7), (8, 44100, 48000, 7)]
SENTINEL = speexhip.Resampler.SENTINEL_BYTE


def storage_of(fmt, n, seed, quiet=False):
    """n samples of format fmt: full-scale LCG noise with fraction bits (the wide formats carry them), or a quiet stretch
    of amplitude <= 100 int16 steps"""
    pcm = orc.lcg_pcm(n, seed).astype(np.float64)
    frac = (orc.lcg_pcm(n, seed + 1000).astype(np.float64) + 32768.0) / 65536.0
    target = (pcm % 201 - 100 + frac * 0.5) if quiet else pcm + frac
    if fmt in (sf.F32, sf.F32N):
        x = target.astype(np.float32)
        return x if fmt == sf.F32 else x / np.float32(32768.0)
    return sf.from_internal(fmt, target.astype(np.float32)) if fmt != sf.S32 else \
        sf.store(sf.S32, np.clip(np.floor(target * 65536.0 + 0.5), -(1 << 31), (1 << 31) - 1).astype(np.int64))


def frames_of(fmt, storage, ch):
    return sf.samples_in(fmt, storage) // ch


def check_tail(out, fmt, made, ch, what):
    raw = out.view(np.uint8)
    assert (raw[made * ch * sf.BYTES[fmt]:] == SENTINEL).all(), what + ": written past produced"


def twin_of_pair(in_fmt, out_fmt):
    """which existing call the pair IS: 'int' / 'same' (the float call on the same bytes) for the identity pairs, else
    'float' on to_internal(input)"""
    if in_fmt == out_fmt == sf.S16:
        return "int"
    if in_fmt == out_fmt == sf.F32N:
        return "same"
    return "float"


def run_pairs(cfg, mode, in_fmt, calls, seed, out_fmts=sf.ALL):
    """One formatted state per output format against the twins, call after call.  calls: (frames or None for silence,
    capacity, silent frames, quiet).  Returns {out_fmt: all bytes produced} and the float twin's output."""
    ch, fi, fo, q = cfg
    mk = lambda: speexhip.Resampler(ch, fi, fo, q, mode=mode)
    states = {o: mk() for o in out_fmts}
    twins = {kind: mk() for kind in set(twin_of_pair(in_fmt, o) for o in out_fmts)}
    got = {o: [] for o in out_fmts}
    floats = []
    try:
        for i, (frames, cap, silent, quiet) in enumerate(calls):
            raw = None if frames is None else storage_of(in_fmt, frames * ch, seed + 17 * i, quiet)
            ref = {}
            for kind, t in twins.items():
                if kind == "int":
                    ref[kind] = t.raw_call("int", raw, cap, silent)
                else:
                    x = None if raw is None else (raw if kind == "same" else sf.to_internal(in_fmt, raw))
                    ref[kind] = t.raw_call("float", x, cap, silent)
            if "float" in ref:
                floats.append(ref["float"][3][: ref["float"][2]].reshape(-1))
            for o, r in states.items():
                what = "%s mode=%s %s->%s call %d (%s frames, cap %d)" % (cfg, mode, sf.NAMES[in_fmt], sf.NAMES[o], i, frames, cap)
                kind = twin_of_pair(in_fmt, o)
                rc_t, used_t, made_t, out_t = ref[kind]
                rc, used, made, out = r.fmt_call(raw, in_fmt, o, cap, silent)
                assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
                y = out_t[:made_t].reshape(-1)
                want = y if kind != "float" else sf.from_internal(o, y)
                per = ch * (3 if o == sf.S24 else 1)
                assert out[: made * per].tobytes() == want.tobytes(), what + ": samples"
                check_tail(out, o, made, ch, what)
                assert r.position() == twins[kind].position(), what
                got[o].append(out[: made * per].copy())
        for o, r in states.items():
            same_state(r, twins[twin_of_pair(in_fmt, o)], "%s mode=%s %s->%s" % (cfg, mode, sf.NAMES[in_fmt], sf.NAMES[o]))
    finally:
        for r in list(states.values()) + list(twins.values()):
            r.close()
    return {o: np.concatenate(v) for o, v in got.items()}, (np.concatenate(floats) if floats else np.zeros(0, np.float32))


def ties(y, scale):
    v = y.astype(np.float64) * scale
    return int((v - np.floor(v) == 0.5).sum())


# ---- 1. the twin, byte for byte --------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", sf.ALL, ids=sf.NAMES)
@pytest.mark.parametrize("mode", list(MODES))
def test_formatted_call_equals_the_float_twin_for_every_pair(mode, in_fmt):
    for cfg in CONFIGS:
        ch, fi, fo, q = cfg
        calls = [(1, 8, 0, False), (15, 40, 0, False), (16, 40, 0, False), (17, 40, 0, False), (160, wcap(160, fi, fo), 0, False),
                 (4097, wcap(4097, fi, fo), 0, True),     # the quiet stretch
                 (0, 64, 0, False),                       # no input
                 (None, 600, 480, False),                 # silence
                 (5000, 777, 0, False),                   # a capacity that binds
                 (300000, wcap(300000, fi, fo), 0, False)]
        got, y = run_pairs(cfg, MODES[mode], in_fmt, calls, seed=31 * ch + q)
        # both rails of every integer output are reached, and the half-up rule meets exact ties -- of the S24 and S32
        # scales, by chance; every encoder's ties, rails and thresholds by construction: test_gpu_decision_points.py
        for o, lo, hi in ((sf.U8, 0, 255), (sf.S16, -32768, 32767), (sf.S24, -(1 << 23), (1 << 23) - 1),
                          (sf.S32, -(1 << 31), (1 << 31) - 1)):
            if in_fmt == o == sf.S16:
                continue  # (the int16 call: its own test below)
            v = sf.integers(o, got[o])
            assert v.min() == lo and v.max() == hi, (cfg, mode, sf.NAMES[in_fmt], sf.NAMES[o], int(v.min()), int(v.max()))
        assert ties(y, 65536.0) > 0 and ties(y, 256.0) > 0, (cfg, mode, sf.NAMES[in_fmt], ties(y, 65536.0), ties(y, 256.0))


# ---- 2. the three identity pairs -------------------------------------------------------------------------------------
def test_identity_pairs_are_the_existing_calls():
    ch, fi, fo, q = 2, 44100, 48000, 7
    calls = [(160, wcap(160, fi, fo), 0, False), (5000, 777, 0, False), (20000, wcap(20000, fi, fo), 0, False),
             (None, 600, 480, False), (4097, wcap(4097, fi, fo), 0, True)]
    # (8 kHz -> 96 kHz: a 160-frame block makes more than the 1024 outputs the int entry emits per block)
    for cfg in ((ch, fi, fo, q), (1, 8000, 96000, 3)):
        for mode in (None, speexhip.MODE_EXACT):
            for fmt in (sf.S16, sf.F32, sf.F32N):
                run_pairs(cfg, mode, fmt, calls, seed=5, out_fmts=(fmt,))
    # the int entry's capacity-bound behaviour differs from the float entry's: S16 -> S16 has the int one
    a, b = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    x = orc.lcg_pcm(5000 * ch, 3)
    rc, used, made, _ = a.fmt_call(x, sf.S16, sf.S16, 777)
    assert (rc, used, made) == (0,) + b.peek(5000, 777, False)
    rc, used, made, _ = b.fmt_call(x, sf.S16, sf.F32N, 777)
    assert (rc, used, made) == (0,) + speexhip.Resampler(ch, fi, fo, q).peek(5000, 777, True)
    a.close()
    b.close()


# ---- 3. addressing ---------------------------------------------------------------------------------------------------
def _device_call(cfg, in_fmt, out_fmt, raw, cap, in_off, out_off, torch):
    """formatted device call with the input `in_off` bytes and the output `out_off` bytes off a 16-byte boundary, guard
    bytes around the output (checked); returns (consumed, produced, output bytes, state)"""
    ch, fi, fo, q = cfg
    r = speexhip.Resampler(ch, fi, fo, q)
    src = torch.zeros(64 + raw.nbytes + 64, dtype=torch.uint8, device="cuda")
    src[16 + in_off: 16 + in_off + raw.nbytes] = torch.from_numpy(raw.view(np.uint8).copy()).cuda()
    room = cap * ch * sf.BYTES[out_fmt]
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    used, made = r.process_fmt_device(in_fmt, src.data_ptr() + 16 + in_off, frames_of(in_fmt, raw, ch), out_fmt,
                                      dst.data_ptr() + 16 + out_off, cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    n = made * ch * sf.BYTES[out_fmt]
    lo = 16 + out_off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "bytes outside the produced samples written"
    return used, made, flat[lo: lo + n].copy(), r


def test_formatted_addressing_offsets_tails_and_guards():
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37  # whole 4096-sample tiles and a tail that ends inside a 16-byte piece, on both sides
    cap = wcap(frames, fi, fo)
    # byte offsets 0..15 for the byte-addressed formats, element offsets 0..3 for the rest
    cases = [(sf.U8, sf.U8, range(16)), (sf.S24, sf.S24, range(16)), (sf.S16, sf.S32, range(4)),
             (sf.S32, sf.F32N, range(4)), (sf.F32N, sf.S16, range(4))]
    for in_fmt, out_fmt, offsets in cases:
        raw = storage_of(in_fmt, frames * ch, 77 + in_fmt)
        t = speexhip.Resampler(*cfg)
        y, used_t = t.process_float(sf.to_internal(in_fmt, raw).reshape(-1, ch), cap)
        want = sf.from_internal(out_fmt, y).view(np.uint8).tobytes()
        for e in offsets:
            bytewise = in_fmt in (sf.U8, sf.S24)
            off, out_off = (e, e) if bytewise else (e * sf.BYTES[in_fmt], e * sf.BYTES[out_fmt])
            used, made, got, r = _device_call(cfg, in_fmt, out_fmt, raw, cap, off, out_off, torch)
            what = (sf.NAMES[in_fmt], sf.NAMES[out_fmt], off, out_off)
            assert (used, made) == (used_t, y.shape[0]), what
            # (offset 0: whole tiles take the 16-bytes-per-lane path, every other offset the element path -- one answer)
            assert got.tobytes() == want, what
            same_state(r, t, str(what))
            r.close()
        t.close()


# ---- 4. batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(sf.S16, sf.F32N), (sf.S24, sf.S32)], ids=["s16-f32n", "s24-s32"])
def test_formatted_batch_equals_single_states(pair):
    import torch
    in_fmt, out_fmt = pair
    S, ch, fi, fo, q, T = 5, 2, 44100, 48000, 7, 9000
    bi, bo = sf.BYTES[in_fmt], sf.BYTES[out_fmt]
    lens = [T - 611 * s for s in range(S)]
    cap = wcap(T, fi, fo)
    raws = [storage_of(in_fmt, T * ch, 900 + s) for s in range(S)]
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
        want, used_r = r.process_fmt(raws[s][: lens[s] * ch * (3 if in_fmt == sf.S24 else 1)], in_fmt, out_fmt, cap)
        n = want.nbytes
        assert (used[s], made[s] * ch * bo) == (used_r, n), s
        lo = s * out_stride * bo
        assert flat[lo: lo + n].tobytes() == want.tobytes(), s
        assert (flat[lo + n: lo + out_stride * bo] == SENTINEL).all(), s
        assert b.lines(s).tobytes() == r._lines().tobytes(), s
        r.close()
    b.close()


def test_process_tensor_converts_sample_types():
    import torch
    S, ch, fi, fo, q, T = 3, 2, 44100, 48000, 7, 6000
    cap = wcap(T, fi, fo)
    for in_fmt, out_dtype, normalized, out_fmt in ((sf.S32, None, False, sf.S32), (sf.U8, None, False, sf.U8),
                                                   (sf.S16, torch.float32, True, sf.F32N), (sf.S32, torch.int16, False, sf.S16),
                                                   (sf.U8, torch.float32, False, sf.F32)):
        raws = [storage_of(in_fmt, T * ch, 500 + s) for s in range(S)]
        x = torch.from_numpy(np.stack(raws).reshape(S, T, ch)).cuda()
        b = speexhip.Batch(S, ch, fi, fo, q)
        out, made = b.process_tensor(x, out_capacity=cap, out_dtype=out_dtype, normalized=normalized)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.shape == (S, max(made), ch) and got.dtype == sf.DTYPE[out_fmt]
        for s in range(S):
            r = speexhip.Resampler(ch, fi, fo, q)
            want, _ = r.process_fmt(raws[s], in_fmt, out_fmt, cap)
            assert got[s, : made[s]].tobytes() == want.tobytes(), (sf.NAMES[in_fmt], sf.NAMES[out_fmt], s)
            r.close()
        b.close()


# ---- 5. against the oracle -------------------------------------------------------------------------------------------
def test_formatted_call_against_the_oracle():
    ch, fi, fo, q = 2, 44100, 48000, 7
    frames = 30000
    cap = wcap(frames, fi, fo)
    model = em.Model(ch, fi, fo, q)
    x = em.with_silence(orc.lcg_pcm(frames * ch, 12).reshape(frames, ch), model.taps)
    want, want_used = orc.Oracle(ch, fi, fo, q).process_float(x.astype(np.float32), cap)
    # exact mode: bit for bit
    r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    got, used = r.process_fmt(x, sf.S16, sf.F32N, cap)
    r.close()
    assert used == want_used
    assert got.tobytes() == (want.reshape(-1) / np.float32(32768.0)).tobytes()
    # the default mode: judged against the exact model like a float call of that family (the margin
    # test_gpu_exact_model.py uses for the period family: em.MARGIN, no exception listed there)
    r = speexhip.Resampler(ch, fi, fo, q)
    bits = r.info()["accumulate_bits"]
    got, used = r.process_fmt(x, sf.S16, sf.F32N, cap)
    r.close()
    gotf = (got * np.float32(32768.0)).reshape(-1, ch)   # exact: a power of two
    assert used == want_used and gotf.shape == want.shape
    truth, mag = model.truth(x[:used], gotf.shape[0])
    fails, stats = em.judge_float(model, x[:used], gotf, truth, mag, bits, want, em.MARGIN, tile=model.num)
    print("s16 -> f32n, default mode: n %d rms(e) %.3f yardstick %.3f max|e| %.2f" % (
        stats["n"], stats["rms"], stats.get("yard", 0.0), stats["max"]))
    assert not fails, fails
    # S32 input with 24 significant bits is the same samples as S24
    s24 = sf.integers(sf.S24, storage_of(sf.S24, frames * ch, 4))
    a, b = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    for out_fmt in (sf.S24, sf.S32, sf.F32N):
        ya, ua = a.process_fmt(sf.store(sf.S24, s24), sf.S24, out_fmt, cap)
        yb, ub = b.process_fmt(sf.store(sf.S32, s24 * 256), sf.S32, out_fmt, cap)
        assert ua == ub and ya.tobytes() == yb.tobytes(), sf.NAMES[out_fmt]
    same_state(a, b, "s24 and s32 with 24 significant bits")
    a.close()
    b.close()


# ---- 6. state mixing and errors --------------------------------------------------------------------------------------
def test_mixing_formatted_interleaved_planar_and_per_channel_calls():
    """One state through formatted, interleaved int, planar and per-channel calls in turn, against the oracle driven by
    the same sequence (formatted -> the float call on the converted samples, converted back).  After an uneven per-channel
    call the formatted call goes channel by channel: it reports the last channel's lengths and writes each channel's own
    number of frames."""
    ch, fi, fo, q = 2, 44100, 48000, 5
    r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    o = orc.Oracle(ch, fi, fo, q)
    seq = [("fmt", 700, sf.S24, sf.S32), ("inter", 1500), ("fmt", 4500, sf.U8, sf.S16), ("planar", 900), ("chan", 400),
           ("fmt", 1, sf.S16, sf.F32N), ("uneven", 300), ("fmt", 2000, sf.S32, sf.S24), ("fmt", 5000, sf.F32N, sf.U8),
           ("inter", 800), ("fmt", 1200, sf.S16, sf.F32N)]
    for i, step in enumerate(seq):
        what, n = step[0], step[1]
        cap = wcap(n, fi, fo)
        x = orc.lcg_pcm(n * ch, 300 + i).reshape(n, ch)
        if what in ("chan", "uneven"):
            for c in range(ch):
                m = n if what == "chan" or c == 0 else n // 2
                a = r.channel_call("int", c, x[:m, c], cap)
                bref = o.channel_call("int", c, x[:m, c], cap)
                assert a[:3] == bref[:3] and a[3][: a[2]].tobytes() == bref[3][: bref[2]].tobytes(), (i, c)
        elif what == "inter":
            rc, used, made, out = r.raw_call("int", x, cap)
            rc_o, used_o, made_o, out_o = o.raw_call("int", x, cap)
            assert (rc, used, made) == (rc_o, used_o, made_o) and out[:made].tobytes() == out_o[:made_o].tobytes(), i
        elif what == "planar":
            rc, used, made, outs = r.planar_call("int", [np.ascontiguousarray(x[:, c]) for c in range(ch)], cap)
            rc_o, used_o, made_o, out_o = o.raw_call("int", x, cap)
            assert (rc, used, made) == (rc_o, used_o, made_o), i
            for c in range(ch):
                assert outs[c].tobytes() == np.ascontiguousarray(out_o[:, c]).tobytes(), (i, c)
        else:
            in_fmt, out_fmt = step[2], step[3]
            raw = storage_of(in_fmt, n * ch, 300 + i)
            rc, used, made, out = r.fmt_call(raw, in_fmt, out_fmt, cap)
            rc_o, used_o, made_o, out_o = o.raw_call("float", sf.to_internal(in_fmt, raw).reshape(-1, ch), cap)
            assert (rc, used, made) == (rc_o, used_o, made_o), (i, step)
            # (channels that stand apart write different numbers of frames: compare, per channel, what the oracle wrote
            #  -- everything that is not its sentinel -- and require the rest untouched)
            per = 3 if out_fmt == sf.S24 else 1
            got = out.reshape(cap, ch, per)
            for c in range(ch):
                wrote = int((out_o[:, c] != np.float32(orc.SENTINEL_F32)).sum())
                assert (out_o[:wrote, c] != np.float32(orc.SENTINEL_F32)).all()
                want = sf.from_internal(out_fmt, out_o[:wrote, c])
                assert got[:wrote, c].tobytes() == want.tobytes(), (i, step, c)
                assert (np.ascontiguousarray(got[wrote:, c]).view(np.uint8) == SENTINEL).all(), (i, step, c, "written past the channel's frames")
        assert r.positions() == o.positions(), (i, step)
    r.close()


def test_formatted_call_in_zero_fallback_mode():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = storage_of(sf.S24, 3000 * ch, 5)
    for out_fmt in sf.ALL:
        p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
        try:
            p.process_fmt(x, sf.S24, out_fmt, wcap(3000, fi, fo))
            t.process_float(sf.to_internal(sf.S24, x).reshape(-1, ch), wcap(3000, fi, fo))
            for r in (p, t):
                speexhip.lib().speexhip_debug_fail_device_allocs(1)
                rc = r.set_rate(32000, 48000)
                speexhip.lib().speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            y = storage_of(sf.S24, 2000 * ch, 6)
            rc_t, used_t, made_t, out_t = t.raw_call("float", sf.to_internal(sf.S24, y).reshape(-1, ch), 2500)
            rc_p, used_p, made_p, out_p = p.fmt_call(y, sf.S24, out_fmt, 2500)
            assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
            per = ch * (3 if out_fmt == sf.S24 else 1)
            assert not out_t[:made_t].any()
            assert out_p[: made_p * per].tobytes() == sf.from_internal(out_fmt, out_t[:made_t]).tobytes(), sf.NAMES[out_fmt]
            if out_fmt in (sf.U8, sf.S16, sf.S24, sf.S32):  # the format's zero: 128 for u8
                assert (sf.integers(out_fmt, out_p[: made_p * per]) == sf.ZERO[out_fmt]).all(), sf.NAMES[out_fmt]
            check_tail(out_p, out_fmt, made_p, ch, sf.NAMES[out_fmt])
            assert p.positions() == t.positions()
        finally:
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            p.close()
            t.close()


def test_non_finite_float_input_to_integer_outputs():
    """+-inf reach the FIR as they are; every output they touch is +-inf or NaN in the float call -- the integer formats
    clamp infinities to their rails and write their zero for NaN, sample by sample as sample_formats.from_internal says.
    (A filter of the direct kind: one infinite sample times a tap is an infinity of the tap's sign, two of opposite sign
    under one window a NaN; the interpolating kinds blend four infinite sums and give NaN alone.)"""
    ch, fi, fo, q = 1, 16000, 48000, 7
    n = 6000
    x = orc.lcg_pcm(n, 8).astype(np.float32)
    x[1000], x[2500], x[4000], x[4001] = np.inf, -np.inf, np.inf, -np.inf
    t = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    y, _ = t.process_float(x.reshape(-1, 1), wcap(n, fi, fo))
    t.close()
    y = y.reshape(-1)
    assert np.isposinf(y).any() and np.isneginf(y).any() and np.isnan(y).any()
    for out_fmt in (sf.U8, sf.S16, sf.S24, sf.S32):
        r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
        got, _ = r.process_fmt(x, sf.F32, out_fmt, wcap(n, fi, fo))
        r.close()
        assert got.tobytes() == sf.from_internal(out_fmt, y).tobytes(), sf.NAMES[out_fmt]
        v = sf.integers(out_fmt, got)
        assert (v[np.isnan(y)] == sf.ZERO[out_fmt]).all()


def test_formatted_argument_errors_leave_the_state_untouched():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    raw = storage_of(sf.S24, 2000 * ch, 3)
    r.process_fmt(raw, sf.S24, sf.S32, 2300)
    t.process_fmt(raw, sf.S24, sf.S32, 2300)
    before = (r.positions(), r.history().tobytes())
    L = speexhip.lib()
    buf = np.zeros(2300 * ch, np.int32)
    for in_fmt, out_fmt, out_ptr in ((6, sf.S16, buf.ctypes.data), (sf.S16, -1, buf.ctypes.data), (99, 99, buf.ctypes.data),
                                     (sf.S24, sf.S32, None)):
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = L.speexhip_resampler_process_interleaved_fmt(r._h, in_fmt, C.c_void_p(raw.ctypes.data), C.byref(il), out_fmt,
                                                          C.c_void_p(out_ptr), C.byref(ol))
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, in_fmt, None, C.byref(il), out_fmt, C.c_void_p(out_ptr),
                                                                 C.byref(ol), None)
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
    assert not buf.any()
    assert (r.positions(), r.history().tobytes()) == before
    got, _ = r.process_fmt(raw, sf.S24, sf.S32, 2300)      # ... and the stream goes on as its twin's
    want, _ = t.process_fmt(raw, sf.S24, sf.S32, 2300)
    assert got.tobytes() == want.tobytes()
    r.close()
    t.close()


# ---- 7. host routes --------------------------------------------------------------------------------------------------
def test_formatted_host_routes_give_the_device_calls_bytes():
    """pageable (small: the bounce buffers; large: the runtime's staged copy), speexhip_block_acquire blocks on both sides
    and a caller-pinned buffer of 256 KB and more, against the device-pointer call"""
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    for in_fmt, out_fmt, frames in ((sf.S24, sf.F32N, 3000), (sf.S24, sf.F32N, 200000), (sf.S16, sf.S32, 150000)):
        raw = storage_of(in_fmt, frames * ch, 60 + frames % 7)
        cap = wcap(frames, fi, fo)
        used_d, made_d, want, rd = _device_call(cfg, in_fmt, out_fmt, raw, cap, 0, 0, torch)
        out_bytes = cap * ch * sf.BYTES[out_fmt]
        what = (sf.NAMES[in_fmt], sf.NAMES[out_fmt], frames)
        # pageable
        r = speexhip.Resampler(*cfg)
        got, used = r.process_fmt(raw, in_fmt, out_fmt, cap)
        assert used == used_d and got.view(np.uint8).tobytes() == want.tobytes(), what + ("pageable",)
        same_state(r, rd, "pageable")
        r.close()
        # pinned blocks of the library, both sides in place
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
        # memory the caller pinned itself (used in place from 256 KB)
        if raw.nbytes >= 256 * 1024:
            r = speexhip.Resampler(*cfg)
            h_in = torch.from_numpy(raw.view(np.uint8).copy()).pin_memory()
            h_out = torch.full((out_bytes,), SENTINEL, dtype=torch.uint8).pin_memory()
            il, ol = C.c_uint32(frames), C.c_uint32(cap)
            rc = speexhip.lib().speexhip_resampler_process_interleaved_fmt(
                r._h, in_fmt, C.c_void_p(h_in.data_ptr()), C.byref(il), out_fmt, C.c_void_p(h_out.data_ptr()), C.byref(ol))
            assert (rc, il.value, ol.value) == (0, used_d, made_d), what + ("caller-pinned",)
            flat = h_out.numpy()
            assert flat[: want.nbytes].tobytes() == want.tobytes() and (flat[want.nbytes:] == SENTINEL).all(), what + ("caller-pinned",)
            same_state(r, rd, "caller-pinned")
            r.close()
        rd.close()


# ---- 8. Node ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_process_chunk_format():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_formats.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL FORMAT NODE TESTS PASSED" in res.stdout


# ---- 9. cost ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_formatted_batch_call_is_not_slower_than_converting_with_torch():
    """44.1k -> 48k stereo q7, 32 streams x 2^20 frames, device-resident, s16 in and float32 in +-1.0 out.  Yardstick: what
    a caller does today in the same process on the same buffers -- x.to(torch.float32), the float batch call,
    out.mul_(1 / 32768).  The formatted call may be slower than that route by no more than the route's own run-to-run
    spread (max / min of five medians)."""
    import torch
    S, ch, fi, fo, q, T = 32, 2, 44100, 48000, 7, 1 << 20
    cap = wcap(T, fi, fo)
    x = torch.randint(-20000, 20000, (S, T, ch), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fmt, flt = speexhip.Batch(S, ch, fi, fo, q), speexhip.Batch(S, ch, fi, fo, q)
    out_f = torch.empty((S, cap, ch), dtype=torch.float32, device="cuda")
    out_d = torch.empty((S, cap, ch), dtype=torch.float32, device="cuda")

    def formatted_call():
        fmt.process_fmt_device(sf.S16, x.data_ptr(), T * ch, T, sf.F32N, out_f.data_ptr(), cap * ch, cap, stream)

    def diy_call():
        xf = x.to(torch.float32)
        _, made = flt.process_device(xf.data_ptr(), T * ch, T, out_d.data_ptr(), cap * ch, cap, stream, float_io=True)
        return out_d[:, : made[0]].mul_(1.0 / 32768.0)

    def median_ms(fn, reps=7):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    for _ in range(3):
        formatted_call()
        diy_call()
    diy, mine = [], []
    for _ in range(5):  # interleaved in time, so that a clock change hits both
        diy.append(median_ms(diy_call))
        mine.append(median_ms(formatted_call))
    spread = max(diy) / min(diy)
    print("formatted %.3f ms (medians %s), torch route %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(diy), ["%.3f" % v for v in diy], spread))
    fmt.close()
    flt.close()
    assert statistics.median(mine) <= statistics.median(diy) * spread
