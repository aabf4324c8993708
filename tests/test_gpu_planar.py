"""Planar (one plane per channel) calls on the GPU.  The rule under test: a planar call IS the interleaved call on the
same frames -- the same counters, the same samples in every mode, the same state left behind -- so every comparison
with a twin state driven through the interleaved calls is exact equality."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest

import oracle as orc
import speexhip
from golden_util import ROOT

pytestmark = pytest.mark.gpu

MODES = {"exact": speexhip.MODE_EXACT, "default": None, "fast": speexhip.MODE_FAST, "fast_f32": speexhip.MODE_FAST_F32}
# one configuration per kernel family info().fast_path reports: (channels, in, out, quality, fast_path) -- the BASELINE
# stereo config, a SLIDE_CASES row, its quality-10 form, a quality-10 row of the period kernel and a ratio no fast kernel takes
FAMILIES = [(2, 44100, 48000, 7, 2), (2, 16000, 48000, 7, 3), (2, 24000, 48000, 10, 4), (2, 44100, 48000, 10, 5),
            (2, 47999, 48000, 4, 0)]
CHANNEL_COUNTS = [1, 2, 3, 4, 5, 6, 8, 11, 16]  # (4, 6, 8 and 2: the kernels' vector instantiations)


def samples(frames, ch, seed, kind):
    x = orc.lcg_pcm(frames * ch, seed).reshape(frames, ch)
    return x if kind == "int" else (x.astype(np.float32) / np.float32(3.0))


def same_state(a, b, what):
    assert a.positions() == b.positions(), what
    assert a.info()["magic_samples"] == b.info()["magic_samples"], what
    assert a.history().tobytes() == b.history().tobytes(), what + ": history"


def twin_run(cfg, mode, kind, calls, seed=1):
    """calls: (frames or None for silence, capacity, silent_frames).  Planar state against its interleaved twin."""
    ch, fi, fo, q = cfg
    p, t = speexhip.Resampler(ch, fi, fo, q, mode=mode), speexhip.Resampler(ch, fi, fo, q, mode=mode)
    try:
        for i, (frames, cap, silent) in enumerate(calls):
            what = "%s mode=%s %s call %d (%s frames, cap %d)" % (cfg, mode, kind, i, frames, cap)
            x = None if frames is None else samples(frames, ch, seed + i, kind)
            rc_t, used_t, made_t, out_t = t.raw_call(kind, x, cap, silent)
            planes = None if x is None else [np.ascontiguousarray(x[:, c]) for c in range(ch)]
            rc_p, used_p, made_p, out_p = p.planar_call(kind, planes, cap, silent)
            assert (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and rc_t == 0, what
            got = np.stack([o[:made_p] for o in out_p], axis=1)
            assert got.tobytes() == out_t[:made_t].tobytes(), what + ": samples"
            fill = p.SENTINEL_I16 if kind == "int" else p.SENTINEL_F32
            for o in out_p:  # written only up to `produced`
                assert (o[made_p:] == o.dtype.type(fill)).all(), what + ": plane written past produced"
            assert p.position() == t.position(), what
        same_state(p, t, "%s mode=%s %s" % (cfg, mode, kind))
    finally:
        p.close()
        t.close()


def wcap(frames, fi, fo):
    return int(np.ceil(frames * fo / fi)) + 8


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("mode", list(MODES))
def test_planar_equals_interleaved_twin_in_every_family_and_mode(mode, kind):
    for ch, fi, fo, q, path in FAMILIES:
        r = speexhip.Resampler(ch, fi, fo, q, mode=MODES[mode])
        # (FAST_F32 reports its own fp32-chain kernels on the double kinds: the slide / period kernel instead of 4 / 5)
        assert r.info()["fast_path"] == ({4: 3, 5: 2}.get(path, path) if mode == "fast_f32" else path), (ch, fi, fo, q)
        r.close()
        big = 300000 if path == 2 else 40000
        calls = [(1, 8, 0), (160, wcap(160, fi, fo), 0), (16384, wcap(16384, fi, fo), 0), (big, wcap(big, fi, fo), 0),
                 (5000, 777, 0),            # a capacity that binds
                 (None, 600, 480),          # silence
                 (480, 0, 0),               # n_out == 0
                 (0, 64, 0),                # no input
                 (2048, wcap(2048, fi, fo), 0)]
        twin_run((ch, fi, fo, q), MODES[mode], kind, calls, seed=11 * path + 3)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("ch", CHANNEL_COUNTS)
def test_planar_equals_interleaved_twin_for_every_channel_count(ch, kind):
    fi, fo, q = 48000, 44100, 5
    calls = [(1, 4, 0), (160, wcap(160, fi, fo), 0), (16384, wcap(16384, fi, fo), 0), (4100, 1000, 0), (None, 300, 256),
             (300000 if ch in (2, 8) else 20000, wcap(300000, fi, fo), 0), (333, 0, 0), (4097, wcap(4097, fi, fo), 0)]
    for mode in (None, speexhip.MODE_EXACT):
        twin_run((ch, fi, fo, q), mode, kind, calls, seed=100 + ch)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_planar_against_the_oracle(kind):
    """Independent of the interleaved path: EXACT equals the oracle bit for bit, the default mode within +-1 LSB."""
    for ch, fi, fo, q in ((2, 44100, 48000, 7), (6, 48000, 44100, 5), (3, 16000, 48000, 7)):
        x = samples(30000, ch, 5 + ch, "int")  # (the +-1 LSB contract is stated on PCM values)
        xin = x if kind == "int" else x.astype(np.float32)
        cap = wcap(30000, fi, fo)
        o = orc.Oracle(ch, fi, fo, q)
        want, want_used = (o.process(x, cap) if kind == "int" else o.process_float(xin, cap))
        for mode, tol in ((speexhip.MODE_EXACT, 0), (None, 1)):
            r = speexhip.Resampler(ch, fi, fo, q, mode=mode)
            got, used = r.process_planar(xin.T, cap, float_io=kind == "float")
            r.close()
            assert used == want_used and got.shape == (ch, want.shape[0])
            if tol == 0:
                assert got.T.tobytes() == want.tobytes(), (ch, fi, fo, q, kind)
            else:
                assert np.abs(got.T.astype(np.float64) - want.astype(np.float64)).max() <= tol, (ch, fi, fo, q, kind)


def _device_planar_vs_twin(ch, kind, frames, offset, stride_pad, torch, lines=False):
    """device planes at `offset` elements from a 16-byte boundary, plane stride frames + stride_pad (lines: rounded up to
    whole 128-byte lines); guards around"""
    fi, fo, q = 44100, 48000, 7
    dt = torch.int16 if kind == "int" else torch.float32
    x = samples(frames, ch, 40 + offset + stride_pad, kind)
    cap = wcap(frames, fi, fo)
    p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    try:
        want, used_t = (t.process(x, cap) if kind == "int" else t.process_float(x, cap))
        made = want.shape[0]
        in_stride, out_stride = frames + stride_pad, made + stride_pad
        if lines:
            in_stride, out_stride = (in_stride + 63) & ~63, (out_stride + 63) & ~63
        src = torch.zeros(16 + offset + ch * in_stride, dtype=dt, device="cuda")
        planes_in = src[16 + offset:].as_strided((ch, frames), (in_stride, 1))
        planes_in.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
        guard = 77
        dst = torch.full((16 + offset + ch * out_stride + 64,), guard, dtype=dt, device="cuda")
        base = 16 + offset
        es = 2 if kind == "int" else 4
        assert (src.data_ptr() % 16, dst.data_ptr() % 16) == (0, 0)
        used, got_made = p.process_planar_device(src.data_ptr() + base * es, in_stride, frames, dst.data_ptr() + base * es,
                                                 out_stride, cap, torch.cuda.current_stream().cuda_stream, kind == "float")
        torch.cuda.synchronize()
        assert (used, got_made) == (used_t, made)
        flat = dst.cpu().numpy()
        for c in range(ch):
            lo = base + c * out_stride
            assert flat[lo: lo + made].tobytes() == np.ascontiguousarray(want[:, c]).tobytes(), (ch, kind, offset, stride_pad, c)
            assert (flat[lo + made: lo + out_stride] == guard).all(), "gap after plane %d written" % c
        assert (flat[:base] == guard).all() and (flat[base + ch * out_stride:] == guard).all(), "guard region written"
        same_state(p, t, "device planes")
    finally:
        p.close()
        t.close()


def test_planar_addressing_offsets_strides_and_guards():
    import torch
    for kind in ("int", "float"):
        for offset in (0, 1, 3, 7):
            _device_planar_vs_twin(2, kind, 5000, offset, 0 if offset else 8, torch)
        for pad in (0, 1, 24):  # stride == frames, frames + 1, a padded stride
            _device_planar_vs_twin(4, kind, 4096 + 37, 0, pad, torch)
        _device_planar_vs_twin(2, kind, 8192, 0, 0, torch)   # whole tiles: the vector path end to end
        _device_planar_vs_twin(5, kind, 3000, 3, 5, torch)
    # separate, non-contiguous host planes with a guard after each
    ch, fi, fo, q = 3, 44100, 48000, 7
    x = samples(7000, ch, 9, "int")
    cap = wcap(7000, fi, fo)
    p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    want, used_t = t.process(x, cap)
    store = np.zeros((ch, 3, 7000), np.int16)
    store[:, 1, :] = x.T
    outs = [np.full(cap + 50, 0x1111 * (c + 1), np.int16) for c in range(ch)]
    rc, used, made, _ = p.planar_call("int", [store[c, 1] for c in range(ch)], cap, out_planes=outs)
    assert (rc, used, made) == (0, used_t, want.shape[0])
    for c in range(ch):
        assert outs[c][:made].tobytes() == np.ascontiguousarray(want[:, c]).tobytes()
        assert (outs[c][made:] == 0x1111 * (c + 1)).all()
    same_state(p, t, "host planes")
    p.close()
    t.close()


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("ch", [2, 4, 6, 8])
def test_planar_vector_path_on_aligned_device_planes(ch, kind):
    """The 16-bytes-per-lane instantiations of both kernels, on purpose: device planes whose base and stride are
    multiples of 16 bytes and several whole tiles of frames (a tile is 2048 int16 / 1024 float frames) plus a ragged end
    -- so gather AND scatter run their vector path on the whole tiles and the element path on the last one."""
    import torch
    _device_planar_vs_twin(ch, kind, 5 * 2048 + 333, 0, 0, torch, lines=True)
    _device_planar_vs_twin(ch, kind, 4 * 2048, 0, 64, torch, lines=True)


@pytest.mark.parametrize("ch", [2, 8])
@pytest.mark.parametrize("B", [1, 4, 32, 33])
def test_planar_batch_tensor_equals_single_states(B, ch):
    import torch
    fi, fo, q, T = 44100, 48000, 7, 6000
    for kind in ("int", "float"):
        x = np.stack([samples(T, ch, 1000 + s, kind) for s in range(B)])              # (B, T, ch)
        lens = [T - 37 * (s % 5) for s in range(B)]                                   # per-stream in_len
        d = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()        # (B, ch, T)
        b = speexhip.Batch(B, ch, fi, fo, q)
        cap = wcap(T, fi, fo)
        out, made = b.process_tensor(d, out_capacity=cap, in_frames=lens)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.shape == (B, ch, max(made))
        for s in range(B):
            r = speexhip.Resampler(ch, fi, fo, q)
            want, _ = (r.process(x[s, : lens[s]], cap) if kind == "int" else r.process_float(x[s, : lens[s]], cap))
            assert made[s] == want.shape[0]
            assert got[s, :, : made[s]].tobytes() == np.ascontiguousarray(want.T).tobytes(), (B, ch, kind, s)
            assert b.lines(s).tobytes() == r._lines().tobytes(), (B, ch, kind, s)
            r.close()
        b.close()


def test_process_tensor_on_a_strided_view():
    import torch
    ch, fi, fo, q, T = 2, 44100, 48000, 7, 9000
    x = samples(T, ch, 77, "float")
    big = torch.zeros((3, 5, T + 40), dtype=torch.float32, device="cuda")
    view = big[1, 1:5:2, 8: 8 + T]                                  # (2, T): plane stride 2 * (T + 40), offset 8
    view.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
    assert view.stride() == (2 * (T + 40), 1) and not view.is_contiguous()
    b = speexhip.Batch(1, ch, fi, fo, q)
    out, made = b.process_tensor(view)
    torch.cuda.synchronize()
    r = speexhip.Resampler(ch, fi, fo, q)
    want, _ = r.process_float(x, wcap(T, fi, fo) + 64)
    assert out.dim() == 2 and made == [want.shape[0]]
    assert out.cpu().numpy().tobytes() == np.ascontiguousarray(want.T).tobytes()
    with pytest.raises(ValueError):
        b.process_tensor(big[1, 1:3, ::2])
    r.close()
    b.close()


def test_mixing_interleaved_planar_and_per_channel_calls():
    """One state through interleaved, planar and per-channel calls in turn equals the oracle driven by the same sequence
    (planar -> interleaved there); after an uneven per-channel call the planar call goes channel by channel and reports the
    last channel's lengths."""
    ch, fi, fo, q = 2, 44100, 48000, 5
    for kind in ("int", "float"):
        r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
        o = orc.Oracle(ch, fi, fo, q)
        seq = [("inter", 700), ("planar", 1500), ("chan", 400), ("planar", 1), ("inter", 160), ("planar", 5000),
               ("uneven", 300), ("planar", 2000), ("planar", 900), ("inter", 800)]
        for i, (what, n) in enumerate(seq):
            x = samples(n, ch, 300 + i, kind)
            cap = wcap(n, fi, fo)
            if what == "chan" or what == "uneven":
                for c in range(ch):
                    m = n if what == "chan" or c == 0 else n // 2
                    a = r.channel_call(kind, c, x[:m, c], cap)
                    bref = o.channel_call(kind, c, x[:m, c], cap)
                    assert a[:3] == bref[:3] and a[3][: a[2]].tobytes() == bref[3][: bref[2]].tobytes(), (kind, i, c)
                continue
            rc_o, used_o, made_o, out_o = o.raw_call(kind, x, cap)
            if what == "inter":
                rc, used, made, out = r.raw_call(kind, x, cap)
                assert (rc, used, made) == (rc_o, used_o, made_o)
                assert out[:made].tobytes() == out_o[:made_o].tobytes(), (kind, i)
            else:
                rc, used, made, outs = r.planar_call(kind, [np.ascontiguousarray(x[:, c]) for c in range(ch)], cap)
                assert (rc, used, made) == (rc_o, used_o, made_o), (kind, i, what)
                # (channels that stand apart write different numbers of frames; both sides pre-fill with the same
                #  sentinel, so whole planes compare: what was written and what was left alone)
                assert (r.SENTINEL_I16, r.SENTINEL_F32) == (orc.SENTINEL_I16, orc.SENTINEL_F32)
                for c in range(ch):
                    assert outs[c].tobytes() == np.ascontiguousarray(out_o[:, c]).tobytes(), (kind, i, c)
            assert r.positions() == o.positions(), (kind, i, what)
        r.close()


def test_planar_call_in_zero_fallback_mode():
    ch, fi, fo, q = 2, 44100, 48000, 7
    p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    try:
        x = samples(3000, ch, 5, "int")
        p.process_planar(x.T, wcap(3000, fi, fo))
        t.process(x, wcap(3000, fi, fo))
        for r in (p, t):
            speexhip.lib().speexhip_debug_fail_device_allocs(1)
            rc = r.set_rate(32000, 48000)
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            assert rc == speexhip.ERR_ALLOC_FAILED
        y = samples(2000, ch, 6, "int")
        rc_t, used_t, made_t, out_t = t.raw_call("int", y, 2500)
        rc_p, used_p, made_p, out_p = p.planar_call("int", [np.ascontiguousarray(y[:, c]) for c in range(ch)], 2500)
        assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
        for o in out_p:
            assert (o[:made_p] == 0).all() and (o[made_p:] == p.SENTINEL_I16).all()
        assert p.positions() == t.positions()
    finally:
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        p.close()
        t.close()


def test_planar_argument_errors_leave_the_state_untouched():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    x = samples(2000, ch, 3, "int")
    planes = [np.ascontiguousarray(x[:, c]) for c in range(ch)]
    r.process_planar(x.T, 2300)
    t.process(x, 2300)
    before = (r.positions(), r.history().tobytes())
    buf = np.zeros(6000, np.int16)
    rc, _, _, _ = r.planar_call("int", planes, 2300, out_planes=[buf[:2300], buf[1000:3300]])      # output planes overlap
    assert rc == speexhip.ERR_PTR_OVERLAP
    both = np.zeros(4000, np.int16)
    both[:2000] = planes[0]
    rc, _, _, _ = r.planar_call("int", [both[:2000], planes[1]], 2300, out_planes=[both[1000:3300], buf[:2300]])  # in / out
    assert rc == speexhip.ERR_PTR_OVERLAP
    rc, _, _, _ = r.planar_call("int", planes, 2300, out_planes=[buf[:2300], None])
    assert rc == speexhip.ERR_INVALID_ARG
    il, ol = C.c_uint32(2000), C.c_uint32(2300)
    ins = (C.c_void_p * 2)(planes[0].ctypes.data, None)
    outs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 2 * 3000)
    assert speexhip.lib().speexhip_resampler_process_planar_int(r._h, ins, C.byref(il), outs, C.byref(ol)) == speexhip.ERR_INVALID_ARG
    assert speexhip.lib().speexhip_resampler_process_planar_int(r._h, ins, C.byref(il), None, C.byref(ol)) == speexhip.ERR_INVALID_ARG
    assert (il.value, ol.value) == (2000, 2300)
    assert (r.positions(), r.history().tobytes()) == before
    got, _ = r.process_planar(x.T, 2300)      # ... and the stream goes on as its twin's
    want, _ = t.process(x, 2300)
    assert got.T.tobytes() == want.tobytes()
    r.close()
    t.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_process_chunk_planar():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_planar.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL PLANAR NODE TESTS PASSED" in res.stdout


@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_planar_batch_call_is_not_slower_than_transposing_with_torch():
    """44.1k -> 48k stereo q7, 32 streams x 2^20 frames, int16, device-resident.  Yardstick: what a caller does today --
    permute(...).contiguous() in, the interleaved batch call, permute(...).contiguous() out -- in the same process on the
    same buffers.  The planar call may be slower than that route by no more than the route's own run-to-run spread
    (max / min of five medians)."""
    import torch
    S, ch, fi, fo, q, T = 32, 2, 44100, 48000, 7, 1 << 20
    cap = wcap(T, fi, fo)
    x = torch.randint(-20000, 20000, (S, ch, T), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    planar, inter = speexhip.Batch(S, ch, fi, fo, q), speexhip.Batch(S, ch, fi, fo, q)
    pitch = (cap + 63) & ~63  # rows of whole 128-byte lines, as Batch.process_tensor lays its result out
    out_p = torch.empty((S, ch, pitch), dtype=torch.int16, device="cuda")
    out_i = torch.empty((S, cap, ch), dtype=torch.int16, device="cuda")
    assert x.data_ptr() % 16 == 0 and out_p.data_ptr() % 16 == 0

    def planar_call():
        planar.process_planar_device(x.data_ptr(), ch * T, T, T, out_p.data_ptr(), ch * pitch, pitch, cap, stream)

    def diy_call():
        xi = x.permute(0, 2, 1).contiguous()
        _, made = inter.process_device(xi.data_ptr(), T * ch, T, out_i.data_ptr(), cap * ch, cap, stream)
        return out_i[:, : made[0]].permute(0, 2, 1).contiguous()

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
        planar_call()
        diy_call()
    diy, mine = [], []
    for _ in range(5):  # interleaved in time, so that a clock change hits both
        diy.append(median_ms(diy_call))
        mine.append(median_ms(planar_call))
    spread = max(diy) / min(diy)
    print("planar %.3f ms (medians %s), torch route %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(diy), ["%.3f" % v for v in diy], spread))
    planar.close()
    inter.close()
    assert statistics.median(mine) <= statistics.median(diy) * spread
