"""Mixed calls on the GPU: a formatted call whose input frames and output frames may hold another number of channels than
the state, with a matrix on that side (in_mix before the FIR, out_mix after it).  The rule under test: a mixed call IS
to_internal, the input mix, the float call of the state, the output mix, from_internal -- the conversions
(sample_formats.py) and the mix (channel_mix.py) are exact statements, so every comparison with a twin state of C channels
driven through the float call is equality of bytes."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest

import channel_mix as cm
import exact_model as em
import oracle as orc
import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_formats import SENTINEL, storage_of
from test_gpu_planar import FAMILIES, MODES, same_state, wcap

pytestmark = pytest.mark.gpu

TILE = 512  # frames of a workgroup's tile (kernels_mix.hip)
# caller in -> C -> caller out
SHAPES = [(2, 1, 1), (1, 1, 2), (6, 2, 2), (2, 2, 6), (8, 1, 8), (3, 2, 5), (8, 8, 8)]
PAIRS = [(sf.S16, sf.S16), (sf.S16, sf.F32N), (sf.S24, sf.S32), (sf.U8, sf.U8), (sf.F32, sf.F32), (sf.F32N, sf.S16)]
INTEGER_RAILS = {sf.U8: (0, 255), sf.S16: (-32768, 32767), sf.S24: (-(1 << 23), (1 << 23) - 1),
                 sf.S32: (-(1 << 31), (1 << 31) - 1)}


def matrices(shape, seed=1, loud=True):
    """(in_mix, out_mix) of a shape: a side has a matrix where its counts differ (both sides of 8 -> 8 -> 8 have one).
    Coefficients: float32 noise in +-1 with all 24 bits; loud: row 0 of the last matrix is a gain of 2 on one channel, so
    that full-scale noise reaches both rails of every integer output."""
    n_in, c, n_out = shape
    rng = np.random.RandomState(1000 * seed + 100 * n_in + 10 * c + n_out)
    in_mix = rng.uniform(-1.0, 1.0, (c, n_in)).astype(np.float32) if (n_in != c or n_in == 8) else None
    out_mix = rng.uniform(-1.0, 1.0, (n_out, c)).astype(np.float32) if (n_out != c or n_out == 8) else None
    if loud:
        last = out_mix if out_mix is not None else in_mix
        last[0, :] = 0.0
        last[0, 0] = 2.0
    return in_mix, out_mix


def model(in_fmt, raw, in_mix, c):
    """the float image the state's float call sees"""
    x = sf.to_internal(in_fmt, raw)
    return cm.mix(in_mix, x) if in_mix is not None else x.reshape(-1, c)


def model_out(out_fmt, y, out_mix):
    """storage bytes of the float call's output y (frames, C)"""
    z = cm.mix(out_mix, y) if out_mix is not None else y
    return sf.from_internal(out_fmt, np.ascontiguousarray(z).reshape(-1)).view(np.uint8).tobytes()


def out_bytes_of(out, out_fmt, made, n_out):
    return out.view(np.uint8)[: made * n_out * sf.BYTES[out_fmt]].tobytes()


def check_tail(out, out_fmt, made, n_out, what):
    assert (out.view(np.uint8)[made * n_out * sf.BYTES[out_fmt]:] == SENTINEL).all(), what + ": written past produced"


def run_twin(cfg, mode, shape, pair, calls, seed):
    """One mixed state against its float twin of C channels, call after call.  calls: (frames or None for silence,
    capacity, silent frames).  Returns all bytes produced."""
    fi, fo, q = cfg
    n_in, c, n_out = shape
    in_fmt, out_fmt = pair
    in_mix, out_mix = matrices(shape)
    r, t = speexhip.Resampler(c, fi, fo, q, mode=mode), speexhip.Resampler(c, fi, fo, q, mode=mode)
    got = []
    try:
        for i, (frames, cap, silent) in enumerate(calls):
            what = "%s mode=%s %s %s->%s call %d (%s frames, cap %d)" % (cfg, mode, shape, sf.NAMES[in_fmt], sf.NAMES[out_fmt],
                                                                         i, frames, cap)
            raw = None if frames is None else storage_of(in_fmt, frames * n_in, seed + 17 * i)
            x = None if raw is None else model(in_fmt, raw, in_mix, c)
            rc_t, used_t, made_t, out_t = t.raw_call("float", x, cap, silent)
            rc, used, made, out = r.mix_call(raw, in_fmt, out_fmt, in_mix, out_mix, cap, silent)
            assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
            assert out_bytes_of(out, out_fmt, made, n_out) == model_out(out_fmt, out_t[:made_t], out_mix), what + ": samples"
            check_tail(out, out_fmt, made, n_out, what)
            assert r.position() == t.position(), what
            got.append(out.view(np.uint8)[: made * n_out * sf.BYTES[out_fmt]].copy())
        same_state(r, t, "%s mode=%s %s %s->%s" % (cfg, mode, shape, sf.NAMES[in_fmt], sf.NAMES[out_fmt]))
    finally:
        r.close()
        t.close()
    return np.concatenate(got).view(sf.DTYPE[out_fmt])


# ---- 1. the twin, byte for byte --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", range(len(FAMILIES)), ids=["path%d" % f[4] for f in FAMILIES])
@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_call_equals_the_float_twin(mode, family):
    _, fi, fo, q, _ = FAMILIES[family]
    for shape in SHAPES:
        for pair in PAIRS:
            calls = [(1, 8, 0), (15, 40, 0), (16, 40, 0), (17, 40, 0), (160, wcap(160, fi, fo), 0),
                     (3 * TILE + 37, wcap(3 * TILE + 37, fi, fo), 0),   # whole tiles and a tail
                     (0, 64, 0),                                        # no input
                     (None, 600, 480),                                  # silence
                     (5000, 777, 0),                                    # a capacity that binds
                     (20000, wcap(20000, fi, fo), 0)]
            if family == 0 and shape == (6, 2, 2) and pair == (sf.S16, sf.F32N):
                calls.append((300000, wcap(300000, fi, fo), 0))
            got = run_twin((fi, fo, q), MODES[mode], shape, pair, calls, seed=31 * shape[0] + q)
            # a gain of 2 on full-scale noise: both rails of every integer output are reached
            if pair[1] in INTEGER_RAILS:
                v = sf.integers(pair[1], got)
                assert (int(v.min()), int(v.max())) == INTEGER_RAILS[pair[1]], (mode, family, shape, sf.NAMES[pair[1]])


# ---- 2. addressing ---------------------------------------------------------------------------------------------------
def _device_call(cfg, shape, pair, mats, raw, cap, in_off, out_off, torch):
    """mixed device call with the input `in_off` bytes and the output `out_off` bytes off a 16-byte boundary, guard bytes
    around the output (checked); returns (consumed, produced, output bytes, state)"""
    c, fi, fo, q = cfg
    n_in, _, n_out = shape
    in_fmt, out_fmt = pair
    r = speexhip.Resampler(c, fi, fo, q)
    src = torch.zeros(64 + raw.nbytes + 64, dtype=torch.uint8, device="cuda")
    src[16 + in_off: 16 + in_off + raw.nbytes] = torch.from_numpy(raw.view(np.uint8).copy()).cuda()
    room = cap * n_out * sf.BYTES[out_fmt]
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    used, made = r.process_mix_device(in_fmt, src.data_ptr() + 16 + in_off, sf.samples_in(in_fmt, raw) // n_in, out_fmt,
                                      dst.data_ptr() + 16 + out_off, cap, mats[0], mats[1],
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    n = made * n_out * sf.BYTES[out_fmt]
    lo = 16 + out_off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "bytes outside the produced samples written"
    return used, made, flat[lo: lo + n].copy(), r


def test_mixed_addressing_offsets_tails_and_guards():
    """6 -> 2 -> 2 puts the matrix on the input side (mix_in beside convert_out), 2 -> 2 -> 6 on the output side (convert_in
    beside mix_out): byte-wise and 2-byte stores of mix_out at every offset too."""
    import torch
    frames = 3 * TILE + 37
    cap = wcap(frames, 44100, 48000)
    in_side = [((sf.U8, sf.U8), range(16)), ((sf.S24, sf.S24), range(16)), ((sf.S16, sf.S32), range(4)),
               ((sf.S32, sf.F32N), range(4)), ((sf.F32N, sf.S16), range(4)), ((sf.F32, sf.F32), range(4))]
    out_side = [((sf.U8, sf.U8), range(16)), ((sf.S24, sf.S24), range(16)), ((sf.F32, sf.S16), range(4)),
                ((sf.S16, sf.F32N), range(4))]
    for shape, cases in (((6, 2, 2), in_side), ((2, 2, 6), out_side)):
        n_in, c, n_out = shape
        cfg = (c, 44100, 48000, 7)
        mats = matrices(shape)
        assert (mats[0] is None) != (mats[1] is None)
        for pair, offsets in cases:
            in_fmt, out_fmt = pair
            raw = storage_of(in_fmt, frames * n_in, 77 + in_fmt)
            t = speexhip.Resampler(*cfg)
            y, used_t = t.process_float(model(in_fmt, raw, mats[0], c), cap)
            want = model_out(out_fmt, y, mats[1])
            first = None
            for e in offsets:
                bytewise = in_fmt in (sf.U8, sf.S24)
                off, out_off = (e, e) if bytewise else (e * sf.BYTES[in_fmt], e * sf.BYTES[out_fmt])
                used, made, got, r = _device_call(cfg, shape, pair, mats, raw, cap, off, out_off, torch)
                what = (shape, sf.NAMES[in_fmt], sf.NAMES[out_fmt], off, out_off)
                assert (used, made) == (used_t, y.shape[0]), what
                # (mix_in, offset 0: whole tiles take the 16-bytes-per-lane path, every other offset the element path -- one
                # answer; mix_out goes frame by frame at every offset)
                first = got.tobytes() if first is None else first
                assert got.tobytes() == first, what
                assert got.tobytes() == want, what
                same_state(r, t, str(what))
                r.close()
            t.close()


# ---- 3. batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 2, 6)], ids=["2-1-1", "2-2-6"])
@pytest.mark.parametrize("pair", [(sf.S16, sf.F32N), (sf.S24, sf.S32)], ids=["s16-f32n", "s24-s32"])
def test_mixed_batch_equals_single_states(pair, shape):
    import torch
    in_fmt, out_fmt = pair
    n_in, c, n_out = shape
    S, fi, fo, q, T = 5, 44100, 48000, 7, 9000
    bi, bo = sf.BYTES[in_fmt], sf.BYTES[out_fmt]
    in_mix, out_mix = matrices(shape)
    lens = [T - 611 * s for s in range(S)]
    cap = wcap(T, fi, fo)
    raws = [storage_of(in_fmt, T * n_in, 900 + s) for s in range(S)]
    in_stride, out_stride = T * n_in + 5, cap * n_out + 3   # samples; odd strides put the streams at every alignment
    src = torch.zeros(S * in_stride * bi, dtype=torch.uint8, device="cuda")
    for s in range(S):
        src[s * in_stride * bi: s * in_stride * bi + raws[s].nbytes] = torch.from_numpy(raws[s].view(np.uint8).copy()).cuda()
    dst = torch.full((S * out_stride * bo,), SENTINEL, dtype=torch.uint8, device="cuda")
    b = speexhip.Batch(S, c, fi, fo, q)
    used, made = b.process_mix_device(in_fmt, src.data_ptr(), in_stride, lens, out_fmt, dst.data_ptr(), out_stride, cap,
                                      in_mix, out_mix, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    for s in range(S):
        r = speexhip.Resampler(c, fi, fo, q)
        want, used_r = r.process_mix(raws[s].view(np.uint8)[: lens[s] * n_in * bi].view(sf.DTYPE[in_fmt]), in_fmt, out_fmt, cap,
                                     in_mix, out_mix)
        n = want.nbytes
        assert (used[s], made[s] * n_out * bo) == (used_r, n), s
        lo = s * out_stride * bo
        assert flat[lo: lo + n].tobytes() == want.tobytes(), s
        assert (flat[lo + n: lo + out_stride * bo] == SENTINEL).all(), s
        assert b.lines(s).tobytes() == r._lines().tobytes(), s
        r.close()
    b.close()


# ---- 4. process_tensor -----------------------------------------------------------------------------------------------
def test_process_tensor_with_mixes():
    import torch
    S, fi, fo, q, T = 3, 44100, 48000, 7, 6000
    cap = wcap(T, fi, fo)
    for shape, in_fmt, out_dtype, normalized, out_fmt in (((2, 1, 1), sf.S16, torch.float32, True, sf.F32N),
                                                          ((1, 1, 2), sf.S16, None, False, sf.S16),
                                                          ((6, 2, 2), sf.S32, torch.int16, False, sf.S16),
                                                          ((2, 2, 6), sf.U8, torch.float32, False, sf.F32)):
        n_in, c, n_out = shape
        in_mix, out_mix = matrices(shape, loud=False)
        raws = [storage_of(in_fmt, T * n_in, 500 + s) for s in range(S)]
        x = torch.from_numpy(np.stack(raws).reshape(S, T, n_in)).cuda()
        b = speexhip.Batch(S, c, fi, fo, q)
        out, made = b.process_tensor(x, out_capacity=cap, out_dtype=out_dtype, normalized=normalized, in_mix=in_mix,
                                     out_mix=out_mix)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.shape == (S, max(made), n_out) and got.dtype == sf.DTYPE[out_fmt], shape
        for s in range(S):
            r = speexhip.Resampler(c, fi, fo, q)
            want, _ = r.process_mix(raws[s], in_fmt, out_fmt, cap, in_mix, out_mix)
            assert got[s, : made[s]].tobytes() == want.tobytes(), (shape, s)
            r.close()
        b.close()


# ---- 5. against the oracle -------------------------------------------------------------------------------------------
def test_mixed_call_against_the_oracle():
    fi, fo, q = 44100, 48000, 7
    frames = 20000
    cap = wcap(frames, fi, fo)
    mdl = em.Model(1, fi, fo, q)
    stereo = np.stack([em.with_silence(orc.lcg_pcm(frames, 12 + k).reshape(frames, 1), mdl.taps).reshape(-1) for k in (0, 1)],
                      axis=1).astype(np.int16)
    mono = cm.mix(cm.STEREO_TO_MONO, stereo.astype(np.float32))          # the modelled mix: (frames, 1) float32
    want, want_used = orc.Oracle(1, fi, fo, q).process_float(mono, cap)
    # exact mode: bit for bit
    r = speexhip.Resampler(1, fi, fo, q, mode=speexhip.MODE_EXACT)
    got, used = r.process_mix(stereo, sf.S16, sf.F32N, cap, in_mix=cm.STEREO_TO_MONO)
    r.close()
    assert used == want_used
    assert got.tobytes() == (want.reshape(-1) / np.float32(32768.0)).tobytes()
    # the default mode: judged against the exact model like a float call of that family (em.MARGIN, as the formatted
    # call's test does)
    r = speexhip.Resampler(1, fi, fo, q)
    bits = r.info()["accumulate_bits"]
    got, used = r.process_mix(stereo, sf.S16, sf.F32N, cap, in_mix=cm.STEREO_TO_MONO)
    r.close()
    gotf = (got * np.float32(32768.0)).reshape(-1, 1)   # exact: a power of two
    assert used == want_used and gotf.shape == want.shape
    truth, mag = mdl.truth(mono[:used], gotf.shape[0])
    fails, stats = em.judge_float(mdl, mono[:used], gotf, truth, mag, bits, want, em.MARGIN, tile=mdl.num)
    print("stereo s16 -> mono f32n, default mode: n %d rms(e) %.3f yardstick %.3f max|e| %.2f" % (
        stats["n"], stats["rms"], stats.get("yard", 0.0), stats["max"]))
    assert not fails, fails


# ---- 6. no mix is the formatted call ---------------------------------------------------------------------------------
def test_no_mix_is_the_formatted_call():
    ch, fi, fo, q = 2, 44100, 48000, 7
    for in_fmt, out_fmt in ((sf.S16, sf.S16), (sf.S24, sf.S32), (sf.F32N, sf.F32N), (sf.U8, sf.F32)):
        a, b = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
        for i, (frames, cap) in enumerate(((160, 200), (5000, 777), (3 * TILE + 37, 2000))):   # 777: a capacity that binds
            raw = storage_of(in_fmt, frames * ch, 40 + i)
            ra = a.mix_call(raw, in_fmt, out_fmt, None, None, cap)
            rb = b.fmt_call(raw, in_fmt, out_fmt, cap)
            assert ra[:3] == rb[:3] and ra[0] == 0, (sf.NAMES[in_fmt], sf.NAMES[out_fmt], i)
            assert ra[3].tobytes() == rb[3].tobytes(), (sf.NAMES[in_fmt], sf.NAMES[out_fmt], i)
        same_state(a, b, "no mix")
        a.close()
        b.close()
    # S16 -> S16 without a matrix has the int16 call's counters, with one the float call's
    x = orc.lcg_pcm(5000 * ch, 3)
    a, b, p = (speexhip.Resampler(ch, fi, fo, q) for _ in range(3))
    eye = np.eye(2, dtype=np.float32)
    rc, used, made, _ = a.mix_call(x, sf.S16, sf.S16, None, None, 777)
    assert (rc, used, made) == (0,) + p.peek(5000, 777, False)
    rc, used, made, _ = b.mix_call(x, sf.S16, sf.S16, eye, None, 777)
    assert (rc, used, made) == (0,) + p.peek(5000, 777, True)
    # (on a fresh state the two entries count alike.)  They part where frames are pending -- a filter shortened
    # mid-stream -- and a call brings no input: the int16 entry leaves them, the float entry drains them up front.
    assert p.raw_call("int", x, 777)[:3] == (0, used, made)
    for r in (a, b, p):
        assert r.set_quality(0) == 0
        assert r.info()["magic_samples"] > 0
    none = np.zeros(0, np.int16)
    as_int, as_float = p.peek(0, 50, False), p.peek(0, 50, True)
    assert as_int != as_float and as_float[1] > 0
    assert a.mix_call(none, sf.S16, sf.S16, None, None, 50)[:3] == (0,) + as_int
    assert b.mix_call(none, sf.S16, sf.S16, eye, None, 50)[:3] == (0,) + as_float
    for r in (a, b, p):
        r.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def _raw_mix(L, h, device, in_fmt, n_in, in_mix, in_ptr, il, out_fmt, n_out, out_mix, out_ptr, ol):
    mp = lambda m: None if m is None else C.c_void_p(m.ctypes.data)
    if device:
        return L.speexhip_resampler_process_interleaved_mix_device(h, in_fmt, n_in, mp(in_mix), C.c_void_p(in_ptr), C.byref(il),
                                                                   out_fmt, n_out, mp(out_mix), C.c_void_p(out_ptr), C.byref(ol), None)
    return L.speexhip_resampler_process_interleaved_mix(h, in_fmt, n_in, mp(in_mix), C.c_void_p(in_ptr), C.byref(il), out_fmt,
                                                        n_out, mp(out_mix), C.c_void_p(out_ptr), C.byref(ol))


def test_mixed_argument_errors_leave_the_state_untouched():
    import torch
    ch, fi, fo, q = 2, 44100, 48000, 7
    in_mix, out_mix = matrices((6, 2, 2), loud=False)[0], matrices((2, 2, 6), loud=False)[1]
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    raw = storage_of(sf.S24, 2000 * 6, 3)
    for s in (r, t):
        s.process_mix(raw, sf.S24, sf.S32, 2300, in_mix, out_mix)
    before = (r.positions(), r.history().tobytes())
    L = speexhip.lib()
    buf = np.zeros(2300 * 8, np.int32)
    d_in = torch.zeros(raw.nbytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(buf.nbytes, dtype=torch.uint8, device="cuda")
    wide = np.zeros(9 * 9, np.float32)
    good = (sf.S24, 6, in_mix, sf.S32, 6, out_mix)
    cases = [
        (sf.S24, 0, wide, sf.S32, 6, out_mix, True), (sf.S24, 9, wide, sf.S32, 6, out_mix, True),   # caller channels 0, 9
        (sf.S24, 6, in_mix, sf.S32, 0, wide, True), (sf.S24, 6, in_mix, sf.S32, 9, wide, True),
        (sf.S24, 6, None, sf.S32, 6, out_mix, True), (sf.S24, 6, in_mix, sf.S32, 6, None, True),    # NULL matrix, count != C
        (sf.S24, 1, None, sf.S32, 2, None, True),
        (6, 6, in_mix, sf.S32, 6, out_mix, True), (sf.S24, 6, in_mix, -1, 6, out_mix, True),        # unknown formats
        (99, 6, in_mix, 99, 6, out_mix, True),
        good + (False,),                                                                            # out == NULL
    ]
    for in_fmt, n_in, mi, out_fmt, n_out, mo, have_out in cases:
        for device in (False, True):
            il, ol = C.c_uint32(2000), C.c_uint32(2300)
            in_ptr = d_in.data_ptr() if device else raw.ctypes.data
            out_ptr = (d_out.data_ptr() if device else buf.ctypes.data) if have_out else None
            rc = _raw_mix(L, r._h, device, in_fmt, n_in, mi, in_ptr, il, out_fmt, n_out, mo, out_ptr, ol)
            assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, n_in, out_fmt, n_out, device)
    torch.cuda.synchronize()
    assert not buf.any() and not d_out.cpu().numpy().any()
    assert (r.positions(), r.history().tobytes()) == before
    # C = 9 with a matrix
    r9 = speexhip.Resampler(9, fi, fo, q)
    before9 = (r9.positions(), r9.history().tobytes())
    for mi, n_in, mo, n_out in ((wide, 2, None, 9), (None, 9, wide, 2), (wide, 9, wide, 9)):
        il, ol = C.c_uint32(100), C.c_uint32(200)
        rc = _raw_mix(L, r9._h, False, sf.S16, n_in, mi, raw.ctypes.data, il, sf.S16, n_out, mo, buf.ctypes.data, ol)
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (100, 200)
    assert (r9.positions(), r9.history().tobytes()) == before9 and not buf.any()
    r9.close()
    # a state whose channels the per-channel calls moved apart
    u = speexhip.Resampler(ch, fi, fo, q)
    x = orc.lcg_pcm(300, 9)
    u.channel_call("int", 0, x, 400)
    u.channel_call("int", 1, x[:150], 400)
    before_u = (u.positions(), u.history().tobytes())
    assert before_u[0][0] != before_u[0][1]
    for device in (False, True):
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = _raw_mix(L, u._h, device, sf.S24, 6, in_mix, d_in.data_ptr() if device else raw.ctypes.data, il, sf.S32, 6, out_mix,
                      d_out.data_ptr() if device else buf.ctypes.data, ol)
        assert rc == speexhip.ERR_BAD_STATE and (il.value, ol.value) == (2000, 2300), device
    assert (u.positions(), u.history().tobytes()) == before_u and not buf.any()
    u.close()
    got, _ = r.process_mix(raw, sf.S24, sf.S32, 2300, in_mix, out_mix)      # ... and the stream goes on as its twin's
    want, _ = t.process_mix(raw, sf.S24, sf.S32, 2300, in_mix, out_mix)
    assert got.tobytes() == want.tobytes()
    same_state(r, t, "after the errors")
    r.close()
    t.close()


# ---- 8. the zero fallback --------------------------------------------------------------------------------------------
def test_mixed_call_in_zero_fallback_mode():
    fi, fo, q = 44100, 48000, 7
    n_in, c, n_out = shape = (6, 2, 6)
    in_mix, out_mix = matrices(shape, loud=False)
    x = storage_of(sf.S24, 3000 * n_in, 5)
    for out_fmt in sf.ALL:
        p, t = speexhip.Resampler(c, fi, fo, q), speexhip.Resampler(c, fi, fo, q)
        try:
            p.process_mix(x, sf.S24, out_fmt, wcap(3000, fi, fo), in_mix, out_mix)
            t.process_float(model(sf.S24, x, in_mix, c), wcap(3000, fi, fo))
            for r in (p, t):
                speexhip.lib().speexhip_debug_fail_device_allocs(1)
                rc = r.set_rate(32000, 48000)
                speexhip.lib().speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            y = storage_of(sf.S24, 2000 * n_in, 6)
            rc_t, used_t, made_t, out_t = t.raw_call("float", model(sf.S24, y, in_mix, c), 2500)
            rc_p, used_p, made_p, out_p = p.mix_call(y, sf.S24, out_fmt, in_mix, out_mix, 2500)
            assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
            assert not out_t[:made_t].any()
            assert out_bytes_of(out_p, out_fmt, made_p, n_out) == model_out(out_fmt, out_t[:made_t], out_mix), sf.NAMES[out_fmt]
            per = n_out * (3 if out_fmt == sf.S24 else 1)
            if out_fmt in INTEGER_RAILS:  # the format's zero: 128 for u8
                assert (sf.integers(out_fmt, out_p[: made_p * per]) == sf.ZERO[out_fmt]).all(), sf.NAMES[out_fmt]
            else:
                assert not out_p[: made_p * per].any(), sf.NAMES[out_fmt]
            check_tail(out_p, out_fmt, made_p, n_out, sf.NAMES[out_fmt])
            assert p.positions() == t.positions()
        finally:
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            p.close()
            t.close()


# ---- 9. host routes --------------------------------------------------------------------------------------------------
def test_mixed_host_routes_give_the_device_calls_bytes():
    """pageable (small: the bounce buffers; large: the runtime's staged copy), speexhip_block_acquire blocks on both sides
    and a caller-pinned buffer of 256 KB and more, against the device-pointer call"""
    import torch
    fi, fo, q = 44100, 48000, 7
    for shape, in_fmt, out_fmt, frames in (((6, 2, 2), sf.S24, sf.F32N, 3000), ((2, 1, 1), sf.S16, sf.F32N, 20000),
                                           ((6, 2, 2), sf.S24, sf.F32N, 20000), ((2, 2, 6), sf.S16, sf.S32, 20000)):
        n_in, c, n_out = shape
        cfg = (c, fi, fo, q)
        mats = matrices(shape, loud=False)
        raw = storage_of(in_fmt, frames * n_in, 60 + frames % 7)
        cap = wcap(frames, fi, fo)
        used_d, made_d, want, rd = _device_call(cfg, shape, (in_fmt, out_fmt), mats, raw, cap, 0, 0, torch)
        out_bytes = cap * n_out * sf.BYTES[out_fmt]
        what = (shape, sf.NAMES[in_fmt], sf.NAMES[out_fmt], frames)
        L = speexhip.lib()
        # pageable
        r = speexhip.Resampler(*cfg)
        got, used = r.process_mix(raw, in_fmt, out_fmt, cap, mats[0], mats[1])
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
            rc = _raw_mix(L, r._h, False, in_fmt, n_in, mats[0], a_in.ctypes.data, il, out_fmt, n_out, mats[1], a_out.ctypes.data, ol)
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
            rc = _raw_mix(L, r._h, False, in_fmt, n_in, mats[0], h_in.data_ptr(), il, out_fmt, n_out, mats[1], h_out.data_ptr(), ol)
            assert (rc, il.value, ol.value) == (0, used_d, made_d), what + ("caller-pinned",)
            flat = h_out.numpy()
            assert flat[: want.nbytes].tobytes() == want.tobytes() and (flat[want.nbytes:] == SENTINEL).all(), what + ("caller-pinned",)
            same_state(r, rd, "caller-pinned")
            r.close()
        rd.close()


# ---- 10. call kinds mixed on one state -------------------------------------------------------------------------------
def test_mixing_mixed_formatted_interleaved_planar_and_per_channel_calls():
    """One stereo state through mixed, formatted, interleaved int, planar and per-channel calls in turn, in EXACT mode,
    against the oracle driven by the same sequence (mixed -> the float call on the modelled input mix, the modelled output
    mix of what it gave)."""
    ch, fi, fo, q = 2, 44100, 48000, 5
    r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    o = orc.Oracle(ch, fi, fo, q)
    seq = [("mix", 700, (6, 2, 2), sf.S24, sf.S32), ("inter", 1500), ("mix", 4500, (2, 2, 6), sf.U8, sf.S16), ("planar", 900),
           ("chan", 400), ("mix", 1, (3, 2, 5), sf.S16, sf.F32N), ("fmt", 2000, sf.S32, sf.S24), ("mix", 5000, (8, 2, 2), sf.F32N, sf.U8),
           ("inter", 800), ("mix", 1200, (1, 2, 1), sf.S16, sf.F32N)]
    for i, step in enumerate(seq):
        what, n = step[0], step[1]
        cap = wcap(n, fi, fo)
        x = orc.lcg_pcm(n * ch, 300 + i).reshape(n, ch)
        if what == "chan":
            for c in range(ch):
                a = r.channel_call("int", c, x[:, c], cap)
                bref = o.channel_call("int", c, x[:, c], cap)
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
        elif what == "fmt":
            in_fmt, out_fmt = step[2], step[3]
            raw = storage_of(in_fmt, n * ch, 300 + i)
            rc, used, made, out = r.fmt_call(raw, in_fmt, out_fmt, cap)
            rc_o, used_o, made_o, out_o = o.raw_call("float", sf.to_internal(in_fmt, raw).reshape(-1, ch), cap)
            assert (rc, used, made) == (rc_o, used_o, made_o), (i, step)
            assert out_bytes_of(out, out_fmt, made, ch) == model_out(out_fmt, out_o[:made_o], None), (i, step)
        else:
            shape, in_fmt, out_fmt = step[2], step[3], step[4]
            n_in, _, n_out = shape
            in_mix, out_mix = matrices(shape, seed=2, loud=False)
            raw = storage_of(in_fmt, n * n_in, 300 + i)
            rc, used, made, out = r.mix_call(raw, in_fmt, out_fmt, in_mix, out_mix, cap)
            rc_o, used_o, made_o, out_o = o.raw_call("float", model(in_fmt, raw, in_mix, ch), cap)
            assert (rc, used, made) == (rc_o, used_o, made_o) and rc == 0, (i, step)
            assert out_bytes_of(out, out_fmt, made, n_out) == model_out(out_fmt, out_o[:made_o], out_mix), (i, step)
            check_tail(out, out_fmt, made, n_out, str((i, step)))
        assert r.positions() == o.positions(), (i, step)
    r.close()


# ---- 11. Node --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_process_chunk_mix():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_mix.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL MIX NODE TESTS PASSED" in res.stdout


# ---- 12. cost --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_mixed_batch_call_is_not_slower_than_mixing_with_torch():
    """48k -> 16k q7, 32 streams x 2^20 frames, device-resident, stereo s16 in and mono float32 in +-1.0 out.  Yardstick: what
    a caller does today in the same process on the same buffers -- x.to(torch.float32) mixed to mono with torch, the mono
    float batch call, out.mul_(1 / 32768).  The mixed call may be slower than that route by no more than the route's own
    run-to-run spread (max / min of five medians)."""
    import torch
    S, fi, fo, q, T = 32, 48000, 16000, 7, 1 << 20
    cap = wcap(T, fi, fo)
    x = torch.randint(-20000, 20000, (S, T, 2), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    mixed, flt = speexhip.Batch(S, 1, fi, fo, q), speexhip.Batch(S, 1, fi, fo, q)
    out_m = torch.empty((S, cap, 1), dtype=torch.float32, device="cuda")
    out_d = torch.empty((S, cap, 1), dtype=torch.float32, device="cuda")

    def mixed_call():
        mixed.process_mix_device(sf.S16, x.data_ptr(), T * 2, T, sf.F32N, out_m.data_ptr(), cap, cap, cm.STEREO_TO_MONO, None,
                                 stream)

    def diy_call():
        xf = x.to(torch.float32).mean(dim=2)    # (S, T): 0.5 * l + 0.5 * r
        _, made = flt.process_device(xf.data_ptr(), T, T, out_d.data_ptr(), cap, cap, stream, float_io=True)
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
        mixed_call()
        diy_call()
    diy, mine = [], []
    for _ in range(5):  # interleaved in time, so that a clock change hits both
        diy.append(median_ms(diy_call))
        mine.append(median_ms(mixed_call))
    spread = max(diy) / min(diy)
    print("mixed %.3f ms (medians %s), torch route %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(diy), ["%.3f" % v for v in diy], spread))
    mixed.close()
    flt.close()
    assert statistics.median(mine) <= statistics.median(diy) * spread
