"""Layouts: planar or interleaved per side of a formatted or mixed call (the sides calls), on the GPU.  The rule under
test: a call with a planar side IS the mixed call on the same samples arranged as interleaved frames -- counters, return
codes, the value of every sample, the dither index, the history and position left behind -- so every comparison is
equality of bytes with a twin state driven through the existing mix_call / fmt_call on the transposed samples."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest

import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_formats import SENTINEL, storage_of
from test_gpu_planar import FAMILIES, same_state, wcap

pytestmark = pytest.mark.gpu

TILE = 1024  # frames of a workgroup's tile (kSidesTileFrames, kernels.h)
ULAW, ALAW = speexhip.FMT_ULAW, speexhip.FMT_ALAW
FMTS = tuple(sf.ALL) + (ULAW, ALAW)
NAME = dict(zip(sf.ALL, sf.NAMES))
NAME.update({ULAW: "ulaw", ALAW: "alaw"})
P, I = "planar", "interleaved"
COMBOS = [(P, P), (P, I), (I, P)]
FRAMES = [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
BASE = (44100, 48000, 7)
SURROUND_TO_STEREO = np.array([[1, 0, 0.7071, 0.5, 0.7071, 0], [0, 1, 0.7071, 0.5, 0, 0.7071]], np.float32)


def nbytes(fmt):
    return speexhip.fmt_bytes(fmt)


def storage(fmt, n, seed):
    """n samples of any format as its storage array (G.711: every byte value occurs)"""
    if fmt in (ULAW, ALAW):
        return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)
    return storage_of(fmt, n, seed)


def planes_of(fmt, raw, n_ch):
    """interleaved storage -> (n_ch, T) planes of the storage type (S24: (n_ch, 3 T) bytes)"""
    b = nbytes(fmt)
    by = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, n_ch, b)
    return np.ascontiguousarray(by.transpose(1, 0, 2)).reshape(n_ch, -1).view(speexhip.fmt_dtype(fmt))


def frames_of_planes(fmt, planes, made):
    """the first `made` frames of (n_ch, stride) planes as the bytes of interleaved frames"""
    b = nbytes(fmt)
    by = np.ascontiguousarray(planes).view(np.uint8).reshape(planes.shape[0], -1, b)
    return np.ascontiguousarray(by[:, :made].transpose(1, 0, 2)).tobytes()


def planes_tail_untouched(fmt, planes, made):
    b = nbytes(fmt)
    return bool((np.ascontiguousarray(planes).view(np.uint8).reshape(planes.shape[0], -1)[:, made * b:] == SENTINEL).all())


def twin_mixes(c, in_fmt, out_fmt, in_mix, out_mix):
    """the matrices that make the existing mixed call this sides call's twin: with a planar side S16 -> S16 runs by the
    float entry's rules, which the mixed call takes with a matrix -- the identity leaves every sample as it is"""
    if in_mix is None and out_mix is None and in_fmt == out_fmt == sf.S16:
        return np.eye(c, dtype=np.float32), None
    return in_mix, out_mix


def got_bytes(out, fmt, layout, made, n_out):
    if layout == P and n_out > 1:
        return frames_of_planes(fmt, out, made)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)[: made * n_out * nbytes(fmt)].tobytes()


def tail_ok(out, fmt, layout, made, n_out):
    if layout == P and n_out > 1:
        return planes_tail_untouched(fmt, out, made)
    return bool((np.ascontiguousarray(out).view(np.uint8).reshape(-1)[made * n_out * nbytes(fmt):] == SENTINEL).all())


def one_call(r, t, raw, c, in_fmt, out_fmt, li, lo, in_mix, out_mix, cap, silent, what, **kw):
    """the sides call on r against the mixed call on t; returns the produced bytes"""
    n_in = c if in_mix is None else in_mix.shape[1]
    n_out = c if out_mix is None else out_mix.shape[0]
    tm_in, tm_out = twin_mixes(c, in_fmt, out_fmt, in_mix, out_mix)
    rc_t, used_t, made_t, out_t = t.mix_call(raw, in_fmt, out_fmt, tm_in, tm_out, cap, silent)
    x = raw if raw is None or li == I else planes_of(in_fmt, raw, n_in)
    rc, used, made, out = r.sides_call(x, in_fmt, out_fmt, cap, li, lo, in_mix, out_mix, silent, **kw)
    assert (rc, used, made) == (rc_t, used_t, made_t), what
    want = out_t.view(np.uint8)[: made_t * n_out * nbytes(out_fmt)].tobytes()
    got = got_bytes(out, out_fmt, lo, made, n_out)
    assert got == want, what + ": samples"
    assert tail_ok(out, out_fmt, lo, made, n_out), what + ": written past produced"
    assert r.position() == t.position(), what
    return got


def calls_for(fi, fo):
    calls = [(n, wcap(n, fi, fo), 0) for n in FRAMES]
    return calls + [(3000, 777, 0),   # a capacity that binds
                    (0, 64, 0),       # no input
                    (None, 600, 480)]  # silence


def run_pair(cfg, mode, c, in_fmt, out_fmt, in_mix=None, out_mix=None, combos=COMBOS, dither=None, seed=1):
    fi, fo, q = cfg
    n_in = c if in_mix is None else in_mix.shape[1]
    for li, lo in combos:
        r, t = speexhip.Resampler(c, fi, fo, q, mode=mode), speexhip.Resampler(c, fi, fo, q, mode=mode)
        try:
            if dither is not None:
                assert r.set_dither(dither, 77, 5) == 0 and t.set_dither(dither, 77, 5) == 0
            for i, (frames, cap, silent) in enumerate(calls_for(fi, fo)):
                what = "%s mode=%s c=%d %s->%s %s->%s call %d (%s frames, cap %d)" % (
                    cfg, mode, c, NAME[in_fmt], NAME[out_fmt], li, lo, i, frames, cap)
                raw = None if frames is None else storage(in_fmt, frames * n_in, seed + 17 * i)
                one_call(r, t, raw, c, in_fmt, out_fmt, li, lo, in_mix, out_mix, cap, silent, what)
            same_state(r, t, "%s %s->%s %s->%s" % (cfg, NAME[in_fmt], NAME[out_fmt], li, lo))
            assert r.get_dither() == t.get_dither()
        finally:
            r.close()
            t.close()


# ---- 1. every format pair ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", FMTS, ids=[NAME[f] for f in FMTS])
@pytest.mark.parametrize("mode", ["fast_fixed", "exact"])
def test_sides_call_equals_the_mixed_twin_for_every_pair(mode, in_fmt):
    m = {"fast_fixed": speexhip.MODE_FAST_FIXED, "exact": speexhip.MODE_EXACT}[mode]
    for out_fmt in FMTS:
        run_pair(BASE, m, 2, in_fmt, out_fmt, seed=3 + in_fmt)


@pytest.mark.parametrize("family", [1, 2], ids=["slide", "fp64"])
def test_sides_call_on_the_slide_and_fp64_kernels(family):
    ch, fi, fo, q, _ = FAMILIES[family]
    run_pair((fi, fo, q), None, ch, sf.S16, sf.F32N, seed=9)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 6, 8, 12])
def test_sides_call_for_every_channel_count(c):
    run_pair(BASE, None, c, sf.S16, sf.F32N, seed=20 + c)
    run_pair(BASE, None, c, sf.F32N, sf.S24, seed=40 + c)


# ---- 2. addressing -----------------------------------------------------------------------------------------------------
def device_sides(cfg, c, in_fmt, out_fmt, raw, frames, cap, in_mix, out_mix, in_off, in_stride, out_off, out_stride, torch,
                 dither=None):
    """both sides planar on device buffers: planes `in_stride` / `out_stride` samples apart, plane 0 `in_off` / `out_off`
    samples into a 16-byte aligned buffer whose every other byte is SENTINEL.  Returns (used, made, the whole output
    buffer, the state)."""
    fi, fo, q = cfg
    n_in = c if in_mix is None else in_mix.shape[1]
    n_out = c if out_mix is None else out_mix.shape[0]
    bi, bo = nbytes(in_fmt), nbytes(out_fmt)
    host = np.full((in_off + n_in * in_stride) * bi + 64, SENTINEL, np.uint8)
    pl = planes_of(in_fmt, raw, n_in).view(np.uint8).reshape(n_in, -1)
    for ch in range(n_in):
        at = (in_off + ch * in_stride) * bi
        host[at: at + frames * bi] = pl[ch]
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full(((out_off + n_out * out_stride) * bo + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    r = speexhip.Resampler(c, fi, fo, q)
    if dither is not None:
        r.set_dither(dither, 77, 5)
    mi = None if in_mix is None else np.ascontiguousarray(in_mix, np.float32)
    mo = None if out_mix is None else np.ascontiguousarray(out_mix, np.float32)
    a = speexhip.make_side(in_fmt, n_in, speexhip.LAYOUT_PLANAR, mi, d_in.data_ptr() + in_off * bi, in_stride)
    b = speexhip.make_side(out_fmt, n_out, speexhip.LAYOUT_PLANAR, mo, d_out.data_ptr() + out_off * bo, out_stride)
    used, made = r.process_sides_device(a, frames, b, cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return used, made, d_out.cpu().numpy(), r


def test_sides_addressing_vector_path_element_path_and_guards():
    import torch
    fi, fo, q = BASE
    frames = 2 * TILE + 5
    cap = wcap(frames, fi, fo)
    stride_a = 4096  # whole 16-byte pieces of every format, > cap
    for c, in_fmt, out_fmt, in_mix, out_mix in ((2, sf.S16, sf.F32N, None, None), (2, sf.U8, sf.S24, None, None),
                                                (2, sf.F32N, ULAW, None, None), (2, sf.S24, sf.S16, None, None),
                                                (2, sf.S32, sf.F32, SURROUND_TO_STEREO, None)):
        n_in = c if in_mix is None else in_mix.shape[1]
        raw = storage(in_fmt, frames * n_in, 70 + in_fmt)
        t = speexhip.Resampler(c, fi, fo, q)
        tm_in, tm_out = twin_mixes(c, in_fmt, out_fmt, in_mix, out_mix)
        rc_t, used_t, made_t, out_t = t.mix_call(raw, in_fmt, out_fmt, tm_in, tm_out, cap)
        want = out_t.view(np.uint8)[: made_t * c * nbytes(out_fmt)].tobytes()
        bo = nbytes(out_fmt)
        for in_off, in_stride, out_off, out_stride in ((0, stride_a, 0, stride_a), (1, stride_a + 1, 1, stride_a + 1)):
            what = (NAME[in_fmt], NAME[out_fmt], in_off, out_off)
            used, made, buf, r = device_sides(BASE, c, in_fmt, out_fmt, raw, frames, cap, in_mix, out_mix, in_off, in_stride,
                                              out_off, out_stride, torch)
            assert (used, made) == (used_t, made_t), what
            touched = np.zeros(buf.size, bool)
            got = []
            for ch in range(c):
                at = (out_off + ch * out_stride) * bo
                got.append(buf[at: at + made * bo].reshape(made, bo))
                touched[at: at + made * bo] = True
            assert np.stack(got, axis=1).tobytes() == want, what
            # every byte beyond `produced` in each plane, and between planes, is untouched
            assert (buf[~touched] == SENTINEL).all(), what
            same_state(r, t, str(what))
            r.close()
        t.close()


def test_host_form_with_separate_planes_equals_the_device_form():
    import torch
    fi, fo, q = BASE
    for frames in (300, 2 * TILE + 5, 200000):   # the bounce buffers, and the runtime's staged copy
        cap = wcap(frames, fi, fo)
        raw = storage(sf.S16, frames * 2, 81)
        used_d, made_d, buf, rd = device_sides(BASE, 2, sf.S16, sf.F32N, raw, frames, cap, None, None, 0, 262144, 0, 262144,
                                               torch)
        want = np.stack([buf[ch * 262144 * 4: ch * 262144 * 4 + made_d * 4] for ch in range(2)])
        r = speexhip.Resampler(2, fi, fo, q)
        rc, used, made, out = r.sides_call(planes_of(sf.S16, raw, 2), sf.S16, sf.F32N, cap, P, P, separate_planes=True)
        assert (rc, used, made) == (0, used_d, made_d), frames
        assert out.view(np.uint8).reshape(2, -1)[:, : made * 4].tobytes() == want.tobytes(), frames
        assert planes_tail_untouched(sf.F32N, out, made)
        same_state(r, rd, "separate planes %d" % frames)
        r.close()
        rd.close()


# ---- 3. with a matrix --------------------------------------------------------------------------------------------------
MATRIX_CASES = {
    "6-planes-to-stereo": (2, SURROUND_TO_STEREO, None, sf.S16),
    "2-to-mono": (1, np.array([[0.5, 0.5]], np.float32), None, sf.S16),
    "stereo-to-6-planes": (2, None, np.random.RandomState(5).uniform(-1, 1, (6, 2)).astype(np.float32), sf.F32N),
}


@pytest.mark.parametrize("case", list(MATRIX_CASES))
def test_sides_call_with_a_matrix(case):
    c, in_mix, out_mix, in_fmt = MATRIX_CASES[case]
    for out_fmt in (sf.F32N, sf.S16, sf.S24):
        run_pair(BASE, None, c, in_fmt, out_fmt, in_mix, out_mix, seed=11)


# ---- 4. dither ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["triangular", "rectangular"])
def test_dithered_planar_output_is_the_dithered_interleaved_output_transposed(kind):
    k = {"triangular": speexhip.DITHER_TRIANGULAR, "rectangular": speexhip.DITHER_RECTANGULAR}[kind]
    up = MATRIX_CASES["stereo-to-6-planes"][2]
    for out_fmt in (sf.U8, sf.S16, ULAW):
        for out_mix in (None, up):
            run_pair(BASE, None, 2, sf.F32N, out_fmt, None, out_mix, combos=[(P, P), (I, P)], dither=k, seed=5)


def test_dithered_stream_cut_into_calls_equals_one_call():
    fi, fo, q = BASE
    frames = 7 * 700 + 3
    raw = storage(sf.S16, frames * 2, 91)
    pl = planes_of(sf.S16, raw, 2)
    for out_fmt, out_mix in ((sf.U8, None), (sf.S16, MATRIX_CASES["stereo-to-6-planes"][2])):
        n_out = 2 if out_mix is None else 6
        whole = speexhip.Resampler(2, fi, fo, q)
        whole.set_dither(speexhip.DITHER_TRIANGULAR, 9, 0)
        one, used = whole.process_sides(pl, sf.S16, out_fmt, wcap(frames, fi, fo), P, P, None, out_mix)
        assert used == frames
        cut = speexhip.Resampler(2, fi, fo, q)
        cut.set_dither(speexhip.DITHER_TRIANGULAR, 9, 0)
        parts, at = [], 0
        for i in range(7):
            n = 700 if i < 6 else frames - at
            got, used = cut.process_sides(pl[:, at: at + n], sf.S16, out_fmt, wcap(n, fi, fo), P, P, None, out_mix)
            assert used == n
            parts.append(got)
            at += n
        assert np.concatenate(parts, axis=1).tobytes() == one.tobytes() and one.shape[0] == n_out
        assert cut.get_dither() == whole.get_dither()
        same_state(cut, whole, "seven calls")
        whole.close()
        cut.close()


# ---- 5. batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_matrix_and_dither", [False, True], ids=["plain", "matrix-dither"])
def test_sides_batch_equals_single_states(with_matrix_and_dither):
    """33 streams: the second chunk of the pack loop runs; unequal lengths, one idle stream"""
    import torch
    fi, fo, q = BASE
    S, c, T = 33, 2, 2 * TILE + 5
    in_mix = SURROUND_TO_STEREO if with_matrix_and_dither else None
    out_fmt = sf.S16 if with_matrix_and_dither else sf.F32N
    n_in = 6 if with_matrix_and_dither else 2
    lens = [T - 61 * s for s in range(S)]
    lens[4] = 0
    cap = wcap(T, fi, fo)
    x = np.stack([planes_of(sf.S16, storage(sf.S16, T * n_in, 200 + s), n_in) for s in range(S)])  # (S, n_in, T)
    d_in = torch.from_numpy(x).cuda()
    pitch = 4096
    bo = nbytes(out_fmt)
    d_out = torch.full((S, c, pitch * bo), SENTINEL, dtype=torch.uint8, device="cuda")
    b = speexhip.Batch(S, c, fi, fo, q)
    if with_matrix_and_dither:
        b.set_dither(speexhip.DITHER_TRIANGULAR, 1234, 3)
    mi = None if in_mix is None else np.ascontiguousarray(in_mix)
    a = speexhip.make_side(sf.S16, n_in, speexhip.LAYOUT_PLANAR, mi, d_in.data_ptr(), T, n_in * T)
    o = speexhip.make_side(out_fmt, c, speexhip.LAYOUT_PLANAR, None, d_out.data_ptr(), pitch, c * pitch)
    used, made = b.process_sides_device(a, lens, o, cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for s in range(S):
        t = speexhip.Resampler(c, fi, fo, q)
        if with_matrix_and_dither:
            kind, seed, _ = b.get_dither(s)
            t.set_dither(kind, seed, 3)
        raw = np.ascontiguousarray(x[s][:, : lens[s]].T).reshape(-1)
        rc, used_t, made_t, out_t = t.mix_call(raw, sf.S16, out_fmt, in_mix, None, cap)
        assert (rc, used[s], made[s]) == (0, used_t, made_t), s
        assert frames_of_planes(out_fmt, out[s], made[s]) == out_t.view(np.uint8)[: made_t * c * bo].tobytes(), s
        assert planes_tail_untouched(out_fmt, out[s], made[s]), s
        assert b.lines(s)[: t.taps - 1].tobytes() == t.history().tobytes(), s
        if with_matrix_and_dither:
            assert b.get_dither(s)[2] == t.get_dither()[2], s
        t.close()
    assert made[4] == 0
    b.close()


# ---- 6. process_tensor -------------------------------------------------------------------------------------------------
def test_process_tensor_with_layouts():
    import torch
    fi, fo, q = BASE
    S, c, T = 3, 2, 2 * TILE + 5
    mk = lambda ch=c: speexhip.Batch(S, ch, fi, fo, q)
    xf = (torch.rand((S, c, T), device="cuda") * 2 - 1).contiguous()
    # (B, C, T) float32 in +-1.0, planar both ways
    a, b = mk(), mk()
    got, made = a.process_tensor(xf, normalized=True, in_layout="planar", out_layout="planar")
    want, made_w = b.process_tensor(xf.transpose(1, 2).contiguous(), normalized=True)
    assert made == made_w and got.shape == (S, c, max(made)) and torch.equal(got, want.transpose(1, 2))
    # ... a non-contiguous view with a dense last dimension
    wide = (torch.rand((S, c + 1, T + 24), device="cuda") * 2 - 1)
    view = wide[:, 1:, 8: 8 + T]
    assert not view.is_contiguous()
    got, made = a.process_tensor(view, normalized=True, in_layout="planar", out_layout="planar")
    want, made_w = b.process_tensor(view.transpose(1, 2).contiguous(), normalized=True)
    assert made == made_w and torch.equal(got, want.transpose(1, 2))
    a.close(), b.close()
    # (B, T, C) int16 -> (B, C, T') float32 normalized
    xi = torch.randint(-30000, 30000, (S, T, c), dtype=torch.int16, device="cuda")
    a, b = mk(), mk()
    got, made = a.process_tensor(xi, out_dtype=torch.float32, normalized=True, in_layout="interleaved", out_layout="planar")
    want, made_w = b.process_tensor(xi, out_dtype=torch.float32, normalized=True)
    assert made == made_w and got.shape == (S, c, max(made)) and torch.equal(got, want.transpose(1, 2))
    a.close(), b.close()
    # uint8 mu-law (B, 1, T)
    xu = torch.randint(0, 256, (S, 1, T), dtype=torch.uint8, device="cuda")
    a, b = mk(1), mk(1)
    got, made = a.process_tensor(xu, out_dtype=torch.float32, normalized=True, in_format=ULAW, in_layout="planar",
                                 out_layout="planar")
    want, made_w = b.process_tensor(xu.transpose(1, 2).contiguous(), out_dtype=torch.float32, normalized=True, in_format=ULAW)
    assert made == made_w and torch.equal(got, want.transpose(1, 2))
    a.close(), b.close()
    # both layouts None: what the function did before, against the explicit calls
    a, b = mk(), mk()
    xs = torch.randint(-30000, 30000, (S, c, T), dtype=torch.int16, device="cuda")
    got, made = a.process_tensor(xs)
    cap = (T * a.info()["den_rate"] + a.info()["num_rate"] - 1) // a.info()["num_rate"] + 1
    out = torch.empty((S, c, cap), dtype=torch.int16, device="cuda")
    _, made_w = b.process_planar_device(xs.data_ptr(), xs.stride(0), xs.stride(1), T, out.data_ptr(), out.stride(0),
                                        out.stride(1), cap, torch.cuda.current_stream().cuda_stream)
    assert made == made_w and torch.equal(got, out[:, :, : max(made_w)])
    got, made = a.process_tensor(xi, out_dtype=torch.float32, normalized=True)
    out = torch.empty((S, cap, c), dtype=torch.float32, device="cuda")
    _, made_w = b.process_fmt_device(sf.S16, xi.data_ptr(), xi.stride(0), T, sf.F32N, out.data_ptr(), out.stride(0), cap,
                                     torch.cuda.current_stream().cuda_stream)
    assert made == made_w and torch.equal(got, out[:, : max(made_w)])
    a.close(), b.close()


# ---- 7. forwarding and edges -------------------------------------------------------------------------------------------
def test_both_layouts_interleaved_is_the_mixed_call():
    # (8 kHz -> 96 kHz: a 160-frame block makes more than the 1024 outputs the int entry emits per block)
    for c, fi, fo, q, in_fmt, out_fmt, in_mix in ((2, 44100, 48000, 7, sf.S16, sf.S16, None), (1, 8000, 96000, 3, sf.S16, sf.S16, None),
                                                  (2, 44100, 48000, 7, sf.S24, sf.F32N, None),
                                                  (2, 44100, 48000, 7, sf.S16, sf.U8, SURROUND_TO_STEREO)):
        n_in = c if in_mix is None else 6
        r, t = speexhip.Resampler(c, fi, fo, q), speexhip.Resampler(c, fi, fo, q)
        for i, (frames, cap) in enumerate(((700, wcap(700, fi, fo)), (5000, 777), (160, wcap(160, fi, fo)), (333, 100), (0, 64))):
            if frames == 0:
                # a shorter filter mid-stream leaves pending frames: the float entry drains them without input, the int16
                # entry does not -- the two entries' counters differ here
                assert r.set_quality(1) == 0 and t.set_quality(1) == 0 and r.info()["magic_samples"] > 0
                assert r.peek(frames, cap, False) != r.peek(frames, cap, True)
            raw = storage(in_fmt, frames * n_in, 50 + i)
            by_int, by_float = r.peek(frames, cap, False), r.peek(frames, cap, True)
            rc_t, used_t, made_t, out_t = t.mix_call(raw, in_fmt, out_fmt, in_mix, None, cap)
            rc, used, made, out = r.sides_call(raw, in_fmt, out_fmt, cap, I, I, in_mix, None)
            assert (rc, used, made) == (rc_t, used_t, made_t) and out.tobytes() == out_t.tobytes(), (NAME[in_fmt], i)
            # S16 -> S16 without matrix and dither keeps the int16 call's counter rule
            assert (used, made) == (by_int if in_fmt == out_fmt == sf.S16 else by_float), (NAME[in_fmt], i)
        same_state(r, t, NAME[in_fmt])
        r.close(), t.close()


def test_both_planar_float_pairs_are_the_planar_float_call():
    fi, fo, q = BASE
    for fmt in (sf.F32, sf.F32N):
        r, t = speexhip.Resampler(2, fi, fo, q), speexhip.Resampler(2, fi, fo, q)
        for i, frames in enumerate((TILE + 1, 17, 2 * TILE + 5)):
            cap = wcap(frames, fi, fo)
            pl = planes_of(fmt, storage(fmt, frames * 2, 60 + i), 2)
            rc_t, used_t, made_t, out_t = t.planar_call("float", list(pl), cap)
            rc, used, made, out = r.sides_call(pl, fmt, fmt, cap, P, P)
            assert (rc, used, made) == (rc_t, used_t, made_t), (NAME[fmt], i)
            assert out[:, :made].tobytes() == np.stack([o[:made_t] for o in out_t]).tobytes(), (NAME[fmt], i)
            assert planes_tail_untouched(fmt, out, made)
        same_state(r, t, NAME[fmt])
        r.close(), t.close()


def test_channels_moved_apart():
    fi, fo, q = 44100, 48000, 5
    ch = 2
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    x = storage(sf.S16, 300 * ch, 3).reshape(-1, ch)
    for s in (r, t):   # an uneven per-channel call: channel 1 takes half the frames
        s.channel_call("int", 0, x[:300, 0], 400)
        s.channel_call("int", 1, x[:150, 1], 400)
    assert r.positions() == t.positions() and len(set(map(tuple, r.positions()))) > 1
    # with a matrix or dither on: BAD_STATE, the state untouched
    before = (r.positions(), r.history().tobytes())
    raw = storage(sf.S16, 1500 * ch, 4)
    rc, used, made, _ = r.sides_call(planes_of(sf.S16, raw, ch), sf.S16, sf.F32N, 2000, P, P, np.eye(2, dtype=np.float32), None)
    assert (rc, used, made) == (speexhip.ERR_BAD_STATE, 1500, 2000)
    r.set_dither(speexhip.DITHER_TRIANGULAR, 1, 0)
    rc, used, made, _ = r.sides_call(planes_of(sf.S16, raw, ch), sf.S16, sf.F32N, 2000, P, P)
    assert (rc, used, made) == (speexhip.ERR_BAD_STATE, 1500, 2000)
    r.set_dither(speexhip.DITHER_NONE, 0, 0)
    assert (r.positions(), r.history().tobytes()) == before
    # served channel by channel: plane c holds what channel c produced in the interleaved formatted call
    for lo in (P, I):
        rr, tt = (r, t) if lo == P else (speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q))
        if lo == I:
            for s in (rr, tt):
                s.channel_call("int", 0, x[:300, 0], 400)
                s.channel_call("int", 1, x[:150, 1], 400)
        cap = 2000
        rc_t, used_t, made_t, out_t = tt.fmt_call(raw, sf.S16, sf.F32N, cap)
        rc, used, made, out = rr.sides_call(planes_of(sf.S16, raw, ch), sf.S16, sf.F32N, cap, P, lo)
        assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0
        want = out_t.view(np.uint8).reshape(cap, ch, 4)
        got = out.view(np.uint8).reshape(ch, cap, 4).transpose(1, 0, 2) if lo == P else out.view(np.uint8).reshape(cap, ch, 4)
        assert np.ascontiguousarray(got).tobytes() == want.tobytes()   # (each plane's own `produced`, sentinel beyond)
        wrote = [(want[:, c] != SENTINEL).any(axis=1).sum() for c in range(ch)]
        assert wrote[0] != wrote[1]
        assert rr.positions() == tt.positions()
        if lo == I:
            rr.close(), tt.close()
    r.close(), t.close()


def test_sides_call_in_zero_fallback_mode():
    fi, fo, q = BASE
    zero = {sf.U8: 128, ULAW: 0xFF, ALAW: 0xD5}
    for out_fmt in (sf.U8, sf.S16, sf.F32N, ULAW, ALAW):
        p, t = speexhip.Resampler(2, fi, fo, q), speexhip.Resampler(2, fi, fo, q)
        try:
            for r in (p, t):
                speexhip.lib().speexhip_debug_fail_device_allocs(1)
                rc = r.set_rate(32000, 48000)
                speexhip.lib().speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            raw = storage(sf.S24, 2000 * 2, 6)
            rc_t, used_t, made_t, out_t = t.mix_call(raw, sf.S24, out_fmt, None, None, 2500)
            rc, used, made, out = p.sides_call(planes_of(sf.S24, raw, 2), sf.S24, out_fmt, 2500, P, P)
            assert rc == speexhip.ERR_ALLOC_FAILED and (rc, used, made) == (rc_t, used_t, made_t) and made > 0
            assert frames_of_planes(out_fmt, out, made) == out_t.view(np.uint8)[: made * 2 * nbytes(out_fmt)].tobytes()
            written = out.view(np.uint8).reshape(2, -1)[:, : made * nbytes(out_fmt)]
            if out_fmt in zero:
                assert (written == zero[out_fmt]).all()
            else:
                assert not written.any()
            assert planes_tail_untouched(out_fmt, out, made) and p.positions() == t.positions()
        finally:
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            p.close()
            t.close()


def test_sides_argument_errors_leave_the_state_untouched():
    fi, fo, q = BASE
    r, t = speexhip.Resampler(2, fi, fo, q), speexhip.Resampler(2, fi, fo, q)
    raw = storage(sf.S16, 2000 * 2, 3)
    pl = planes_of(sf.S16, raw, 2)
    for s in (r, t):
        s.process_sides(pl, sf.S16, sf.F32N, 2300, P, P)
    before = (r.positions(), r.history().tobytes())
    L = speexhip.lib()
    out = np.zeros((2, 2300), np.float32)
    nine = np.zeros((2, 9), np.float32)
    ptrs_null = (C.c_void_p * 2)(pl[0].ctypes.data, None)

    def sides():
        a = speexhip.make_side(sf.S16, 2, speexhip.LAYOUT_PLANAR, None, pl.ctypes.data, 2000)
        b = speexhip.make_side(sf.F32N, 2, speexhip.LAYOUT_PLANAR, None, out.ctypes.data, 2300)
        return a, b

    def broken(what, change):
        a, b = sides()
        change(a, b)
        return what, a, b

    cases = [broken("bad layout", lambda a, b: setattr(a, "layout", 2)),
             broken("bad out layout", lambda a, b: setattr(b, "layout", -1)),
             broken("short struct_size", lambda a, b: setattr(a, "struct_size", C.sizeof(speexhip.Side) - 8)),
             broken("bad format", lambda a, b: setattr(a, "fmt", 6)),
             broken("NULL plane", lambda a, b: (setattr(a, "data", None),
                                                setattr(a, "planes", C.cast(ptrs_null, C.POINTER(C.c_void_p))))),
             broken("NULL out", lambda a, b: setattr(b, "data", None)),
             broken("9 channels on a matrix side", lambda a, b: (setattr(a, "channels", 9), setattr(a, "mix", nine.ctypes.data)))]
    for what, a, b in cases:
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = L.speexhip_resampler_process_sides(r._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), what
        if what != "NULL plane":
            il, ol = C.c_uint32(2000), C.c_uint32(2300)
            rc = L.speexhip_resampler_process_sides_device(r._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol), None)
            assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), what
    # overlapping host output planes
    a, b = sides()
    b.plane_stride = 100
    il, ol = C.c_uint32(2000), C.c_uint32(2300)
    rc = L.speexhip_resampler_process_sides(r._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
    assert rc == speexhip.ERR_PTR_OVERLAP and (il.value, ol.value) == (2000, 2300)
    assert not out.any()
    assert (r.positions(), r.history().tobytes()) == before
    got, _ = r.process_sides(pl, sf.S16, sf.F32N, 2300, P, P)   # ... and the stream goes on as its twin's
    want, _ = t.process_sides(pl, sf.S16, sf.F32N, 2300, P, P)
    assert got.tobytes() == want.tobytes()
    r.close(), t.close()


def test_mixing_sides_formatted_planar_and_interleaved_calls_on_one_state():
    fi, fo, q = 44100, 48000, 5
    ch = 2
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    seq = [("sides", 700, sf.S24, sf.S32, P, P), ("inter", 1500), ("sides", 4500, sf.U8, sf.S16, I, P), ("planar", 900),
           ("fmt", 1200, sf.S16, sf.F32N), ("sides", 1, sf.S16, sf.F32N, P, I), ("sides", 2 * TILE + 5, ULAW, sf.F32N, P, P),
           ("inter", 800), ("sides", 1200, sf.F32N, sf.F32N, P, P), ("sides", 333, sf.S16, sf.S16, P, P)]
    for i, step in enumerate(seq):
        kind, n = step[0], step[1]
        cap = wcap(n, fi, fo)
        if kind == "sides":
            raw = storage(step[2], n * ch, 300 + i)
            one_call(r, t, raw, ch, step[2], step[3], step[4], step[5], None, None, cap, 0, str((i, step)))
        elif kind == "fmt":
            raw = storage(step[2], n * ch, 300 + i)
            a, b = r.fmt_call(raw, step[2], step[3], cap), t.fmt_call(raw, step[2], step[3], cap)
            assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes(), i
        else:
            x = storage(sf.S16, n * ch, 300 + i).reshape(n, ch)
            if kind == "inter":
                a, b = r.raw_call("int", x, cap), t.raw_call("int", x, cap)
                assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes(), i
            else:
                a = r.planar_call("int", [np.ascontiguousarray(x[:, c]) for c in range(ch)], cap)
                b = t.planar_call("int", [np.ascontiguousarray(x[:, c]) for c in range(ch)], cap)
                assert a[:3] == b[:3] and np.stack(a[3]).tobytes() == np.stack(b[3]).tobytes(), i
        assert r.positions() == t.positions(), (i, step)
    same_state(r, t, "mixed kinds of calls")
    r.close(), t.close()


# ---- 8. Node -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_process_chunk_sides():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_sides.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL SIDES NODE TESTS PASSED" in res.stdout


# ---- 9. cost -----------------------------------------------------------------------------------------------------------
def _medians(fns, torch, reps=7, rounds=5):
    def median_ms(fn):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    for _ in range(3):
        for fn in fns:
            fn()
    got = [[] for _ in fns]
    for _ in range(rounds):  # interleaved in time, so that a clock change hits all
        for k, fn in enumerate(fns):
            got[k].append(median_ms(fn))
    return got


@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_planar_normalized_call_is_not_slower_than_todays_routes():
    """44.1k -> 48k stereo q7, 32 streams x 2^20 frames, device-resident, (B, C, T) float32 in +-1.0 in and out.
    Yardsticks, in the same process on the same tensors: (a) transpose(1, 2).contiguous(), the interleaved formatted
    F32N -> F32N call, transpose back; (b) x * 32768, the planar float call, out / 32768.  The sides call may be slower
    than the faster of them by no more than that route's own run-to-run spread (max / min of its five medians)."""
    import torch
    S, ch, fi, fo, q, T = 32, 2, 44100, 48000, 7, 1 << 20
    x = (torch.rand((S, ch, T), device="cuda") * 2 - 1).contiguous()
    mine_b, a_b, b_b = (speexhip.Batch(S, ch, fi, fo, q) for _ in range(3))

    def sides_call():
        return mine_b.process_tensor(x, normalized=True, in_layout="planar", out_layout="planar")[0]

    def route_a():
        out, _ = a_b.process_tensor(x.transpose(1, 2).contiguous(), normalized=True)
        return out.transpose(1, 2).contiguous()

    def route_b():
        out, _ = b_b.process_tensor(x * 32768.0)
        return out / 32768.0

    mine, ra, rb = _medians([sides_call, route_a, route_b], torch)
    best = ra if statistics.median(ra) <= statistics.median(rb) else rb
    spread = max(best) / min(best)
    print("sides %.3f ms (medians %s), transpose route %.3f ms (medians %s), scale route %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(ra), ["%.3f" % v for v in ra],
        statistics.median(rb), ["%.3f" % v for v in rb], spread))
    for b in (mine_b, a_b, b_b):
        b.close()
    assert statistics.median(mine) <= statistics.median(best) * spread
