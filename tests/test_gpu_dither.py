"""Dither of the integer output formats of the formatted and mixed calls, on the GPU.  The rule under test: with dither
on, a formatted (mixed) call IS the float call on the converted (and mixed) input, followed by the output mix and the
dithered output conversion at the stream's running position -- the noise is a pure function of (seed, sample index) and
every step is an exact statement (sample_formats.py, channel_mix.py, dither_model.py), so every comparison with a twin state
driven through the existing float call is equality of bytes.  With dither off every call is what it was."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import channel_mix as cm
import dither_model as dm
import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_formats import storage_of
from test_gpu_planar import MODES, same_state, wcap

pytestmark = pytest.mark.gpu

SENTINEL = speexhip.Resampler.SENTINEL_BYTE
INT_FMTS = (sf.U8, sf.S16, sf.S24, sf.S32)
SEED = 0xDEADBEEFCAFEF00D
KIND_IDS = [dm.KIND_NAMES[k] for k in dm.KINDS]


def per_sample(fmt):
    """elements of the storage array per sample"""
    return 3 if fmt == sf.S24 else 1


def check_tail(out, fmt, made, c_out, what):
    raw = out.view(np.uint8)
    assert (raw[made * c_out * sf.BYTES[fmt]:] == SENTINEL).all(), what + ": written past produced"


# ---- 1. the twin and the model, byte for byte ------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", (sf.F32, sf.S16), ids=("f32", "s16"))
@pytest.mark.parametrize("kind", dm.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("mode", ("default", "exact"))
def test_dithered_call_equals_the_model_on_the_float_twin(mode, kind, in_fmt):
    for cfg in ((2, 44100, 48000, 7), (1, 44100, 48000, 7), (3, 44100, 48000, 7)):
        ch, fi, fo, q = cfg
        # (frames or None for silence, capacity, silent frames, quiet): whole 4096-sample tiles, partial ones, one sample
        calls = [(1, 8, 0, False), (15, 40, 0, False), (17, 40, 0, False), (4097, wcap(4097, fi, fo), 0, True), (0, 64, 0, False),
                 (None, 600, 480, False), (5000, 777, 0, False), (20000, wcap(20000, fi, fo), 0, False)]
        mk = lambda: speexhip.Resampler(ch, fi, fo, q, mode=MODES[mode])
        start = 1000 * ch + 7
        twin = mk()
        states = {o: mk() for o in INT_FMTS}
        try:
            for r in states.values():
                assert r.set_dither(kind, SEED, start) == 0
                assert r.get_dither() == (kind, SEED, start)
            pos = start
            for i, (frames, cap, silent, quiet) in enumerate(calls):
                raw = None if frames is None else storage_of(in_fmt, frames * ch, 40 + 17 * i + ch, quiet)
                x = None if raw is None else sf.to_internal(in_fmt, raw)
                rc_t, used_t, made_t, out_t = twin.raw_call("float", x, cap, silent)
                y = out_t[:made_t].reshape(-1)
                for o, r in states.items():
                    what = "%s mode=%s %s %s->%s call %d (%s frames, cap %d)" % (
                        cfg, mode, dm.KIND_NAMES[kind], sf.NAMES[in_fmt], sf.NAMES[o], i, frames, cap)
                    rc, used, made, out = r.fmt_call(raw, in_fmt, o, cap, silent)
                    assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
                    want = dm.from_internal(o, y, kind, SEED, pos, ch)
                    assert out[: made * ch * per_sample(o)].tobytes() == want.tobytes(), what + ": samples"
                    check_tail(out, o, made, ch, what)
                    assert r.get_dither() == (kind, SEED, pos + made), what
                pos += made_t
            for o, r in states.items():
                same_state(r, twin, "%s mode=%s %s->%s" % (cfg, mode, sf.NAMES[in_fmt], sf.NAMES[o]))
        finally:
            for r in list(states.values()) + [twin]:
                r.close()


def device_call(r, in_fmt, raw, out_fmt, cap, c_in, c_out, out_off, torch, in_mix=None, out_mix=None):
    """formatted / mixed device call with the output `out_off` bytes off a 16-byte boundary and guard bytes around it
    (checked); returns (consumed, produced, output bytes)"""
    src = torch.zeros(64 + raw.nbytes + 64, dtype=torch.uint8, device="cuda")
    src[16: 16 + raw.nbytes] = torch.from_numpy(raw.view(np.uint8).copy()).cuda()
    room = cap * c_out * sf.BYTES[out_fmt]
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    frames = sf.samples_in(in_fmt, raw) // c_in
    stream = torch.cuda.current_stream().cuda_stream
    if in_mix is None and out_mix is None:
        used, made = r.process_fmt_device(in_fmt, src.data_ptr() + 16, frames, out_fmt, dst.data_ptr() + 16 + out_off, cap, stream)
    else:
        used, made = r.process_mix_device(in_fmt, src.data_ptr() + 16, frames, out_fmt, dst.data_ptr() + 16 + out_off, cap,
                                          in_mix, out_mix, stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    n = made * c_out * sf.BYTES[out_fmt]
    lo = 16 + out_off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "bytes outside the produced samples written"
    return used, made, flat[lo: lo + n].copy()


@pytest.mark.parametrize("kind", dm.KINDS, ids=KIND_IDS)
def test_vector_and_element_paths_give_the_models_bytes(kind):
    """device buffers: 16-byte aligned (whole tiles take the 16-bytes-per-lane path) and one byte -- one element for the
    formats that need their alignment -- off it (every tile takes the element path)"""
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37
    cap = wcap(frames, fi, fo)
    raw = storage_of(sf.F32, frames * ch, 91)
    t = speexhip.Resampler(*cfg)
    y, used_t = t.process_float(raw.reshape(-1, ch), cap)
    start = 77777
    for o in INT_FMTS:
        want = dm.from_internal(o, y, kind, SEED, start, ch).view(np.uint8).tobytes()
        for off in (0, 1 if o in (sf.U8, sf.S24) else sf.BYTES[o]):
            r = speexhip.Resampler(*cfg)
            r.set_dither(kind, SEED, start)
            used, made, got = device_call(r, sf.F32, raw, o, cap, ch, ch, off, torch)
            what = (dm.KIND_NAMES[kind], sf.NAMES[o], off)
            assert (used, made) == (used_t, y.shape[0]), what
            assert got.tobytes() == want, what
            assert r.get_dither()[2] == start + made, what
            same_state(r, t, str(what))
            r.close()
    t.close()


# ---- 2. chunk independence -------------------------------------------------------------------------------------------
def test_dithered_bytes_do_not_depend_on_the_chunking():
    ch, fi, fo, q = 2, 44100, 48000, 7
    frames = 30000
    x = storage_of(sf.F32, frames * ch, 23).reshape(frames, ch)
    cuts = [1, 159, 160, 4097]
    cuts.append(frames - sum(cuts))
    for o in (sf.S16, sf.U8):
        for kind in dm.KINDS:
            whole, parts = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
            whole.set_dither(kind, 11, 0)
            parts.set_dither(kind, 11, 0)
            a, used = whole.process_fmt(x, sf.F32, o, wcap(frames, fi, fo))
            assert used == frames
            got, at = [], 0
            for n in cuts:
                b, used = parts.process_fmt(x[at: at + n], sf.F32, o, wcap(n, fi, fo))
                assert used == n
                got.append(b)
                at += n
            assert np.concatenate(got).tobytes() == a.tobytes(), (sf.NAMES[o], dm.KIND_NAMES[kind])
            assert whole.get_dither() == parts.get_dither()
            same_state(whole, parts, "whole against parts")
            whole.close()
            parts.close()


# ---- 3. the 2^32 boundary of the sample index ------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, (1 << 31) - 1000), (3, (1 << 31) - 1000), (3, (1 << 32) // 3 - 1000)],
                         ids=["stereo", "three-channels", "three-channels-crossing"])
def test_sample_index_crosses_two_to_the_32(case):
    """idx = position * C + ...: stereo from position 2^31 - 1000 crosses idx = 2^32 after 1000 frames, three channels from
    2^32 / 3 - 1000 likewise; three channels from 2^31 - 1000 run wholly above it (hi32(idx) = 1).  Host call (staged
    buffers) and aligned device call: the crossing lies inside a whole tile of the 16-bytes-per-lane path."""
    import torch
    ch, start = case
    fi, fo, q = 44100, 48000, 7
    frames = 5000
    cap = wcap(frames, fi, fo)
    raw = storage_of(sf.F32, frames * ch, 300 + ch)
    t = speexhip.Resampler(ch, fi, fo, q)
    y, _ = t.process_float(raw.reshape(-1, ch), cap)
    t.close()
    assert y.shape[0] >= 5000
    first, last = start * ch, (start + y.shape[0]) * ch - 1
    if case != (3, (1 << 31) - 1000):
        assert first < (1 << 32) <= last
    for o in INT_FMTS:
        want = dm.from_internal(o, y, dm.TRIANGULAR, SEED, start, ch)
        r = speexhip.Resampler(ch, fi, fo, q)
        r.set_dither(dm.TRIANGULAR, SEED, start)
        got, _ = r.process_fmt(raw, sf.F32, o, cap)
        assert got.tobytes() == want.tobytes(), (sf.NAMES[o], "host")
        assert r.get_dither()[2] == start + y.shape[0]
        r.close()
        r = speexhip.Resampler(ch, fi, fo, q)
        r.set_dither(dm.TRIANGULAR, SEED, start)
        _, made, got = device_call(r, sf.F32, raw, o, cap, ch, ch, 0, torch)
        assert made == y.shape[0] and got.tobytes() == want.view(np.uint8).tobytes(), (sf.NAMES[o], "device")
        r.close()


# ---- 4. mixed calls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dm.KINDS, ids=KIND_IDS)
def test_mixed_calls_dither_the_output_frames(kind):
    """a 2 -> 1 in_mix and a 1 -> 2 out_mix on a mono state; the index runs over the OUTPUT frame's samples"""
    import torch
    fi, fo, q = 44100, 48000, 7
    for in_mix, out_mix in ((cm.STEREO_TO_MONO, None), (None, cm.MONO_TO_STEREO)):
        c_in = 1 if in_mix is None else in_mix.shape[1]
        c_out = 1 if out_mix is None else out_mix.shape[0]
        for o in (sf.S16, sf.U8):
            r, t = speexhip.Resampler(1, fi, fo, q), speexhip.Resampler(1, fi, fo, q)
            start = (1 << 32) // c_out - 700   # (the second call crosses idx = 2^32)
            r.set_dither(kind, SEED, start)
            pos = start
            for i, (frames, cap) in enumerate(((333, wcap(333, fi, fo)), (6000, wcap(6000, fi, fo)), (5000, 777))):
                raw = storage_of(sf.S16, frames * c_in, 60 + i)
                x = sf.to_internal(sf.S16, raw)
                xin = x if in_mix is None else cm.mix(in_mix, x).reshape(-1)
                rc_t, used_t, made_t, out_t = t.raw_call("float", xin, cap)
                y = out_t[:made_t].reshape(-1)
                yout = y if out_mix is None else cm.mix(out_mix, y).reshape(-1)
                want = dm.from_internal(o, yout, kind, SEED, pos, c_out)
                what = (dm.KIND_NAMES[kind], sf.NAMES[o], c_in, c_out, i)
                if i < 2:
                    rc, used, made, out = r.mix_call(raw, sf.S16, o, in_mix, out_mix, cap)
                    assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
                    assert out[: made * c_out].tobytes() == want.tobytes(), what
                    check_tail(out, o, made, c_out, str(what))
                else:   # the device form, one byte / element off alignment
                    used, made, got = device_call(r, sf.S16, raw, o, cap, c_in, c_out, sf.BYTES[o], torch, in_mix, out_mix)
                    assert (used, made) == (used_t, made_t), what
                    assert got.tobytes() == want.view(np.uint8).tobytes(), what
                pos += made
                assert r.get_dither() == (kind, SEED, pos), what
            same_state(r, t, "mixed")
            r.close()
            t.close()


# ---- 5. batches ------------------------------------------------------------------------------------------------------
def test_batch_streams_have_their_own_seeds_and_positions():
    import torch
    S, ch, fi, fo, q, T = 3, 2, 44100, 48000, 7, 9000
    kind, seed, start = dm.TRIANGULAR, SEED, 5
    cap = wcap(T, fi, fo)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    b = speexhip.Batch(S, ch, fi, fo, q)
    assert b.set_dither(kind, seed, start) == 0
    twins = [speexhip.Resampler(ch, fi, fo, q) for _ in range(S)]
    pos = [start] * S
    for s in range(S):
        assert b.get_dither(s) == (kind, dm.stream_seed(seed, s), start)

    def settle(what, got_of, made, ys, c_out, o, mix=None):
        for s in range(S):
            y = ys[s].reshape(-1) if mix is None else cm.mix(mix, ys[s]).reshape(-1)
            want = dm.from_internal(o, y, kind, dm.stream_seed(seed, s), pos[s], c_out)
            assert made[s] == ys[s].shape[0], (what, s)
            assert got_of(s).tobytes() == want.view(np.uint8).tobytes(), (what, s)
            pos[s] += made[s]
            assert b.get_dither(s) == (kind, dm.stream_seed(seed, s), pos[s]), (what, s)

    # formatted, ragged lengths, f32 -> s16
    lens = [T - 611 * s for s in range(S)]
    raws = [storage_of(sf.F32, T * ch, 700 + s) for s in range(S)]
    src = torch.from_numpy(np.stack(raws)).cuda()
    dst = torch.full((S, cap * ch * 2 + 6), SENTINEL, dtype=torch.uint8, device="cuda")
    used, made = b.process_fmt_device(sf.F32, src.data_ptr(), T * ch, lens, sf.S16, dst.data_ptr(), dst.stride(0) // 2, cap,
                                      stream())
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    ys = [twins[s].process_float(raws[s][: lens[s] * ch].reshape(-1, ch), cap)[0] for s in range(S)]
    assert used == lens
    settle("fmt", lambda s: flat[s, : made[s] * ch * 2], made, ys, ch, sf.S16)
    for s in range(S):
        assert (flat[s, made[s] * ch * 2:] == SENTINEL).all(), s

    # mixed, a second call that continues the positions: 2 -> 1 out_mix to u8
    lens = [1234, 4097, 2 * 4096]
    raws = [storage_of(sf.S16, T * ch, 800 + s) for s in range(S)]
    src = torch.from_numpy(np.stack(raws)).cuda()
    dst = torch.full((S, cap + 5), SENTINEL, dtype=torch.uint8, device="cuda")
    used, made = b.process_mix_device(sf.S16, src.data_ptr(), T * ch, lens, sf.U8, dst.data_ptr(), dst.stride(0), cap,
                                      None, cm.STEREO_TO_MONO, stream())
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    ys = [twins[s].process_float(sf.to_internal(sf.S16, raws[s][: lens[s] * ch]).reshape(-1, ch), cap)[0] for s in range(S)]
    assert used == lens
    settle("mix", lambda s: flat[s, : made[s]], made, ys, 1, sf.U8, cm.STEREO_TO_MONO)
    for s in range(S):
        assert (flat[s, made[s]:] == SENTINEL).all(), s

    # process_tensor, float32 -> int16
    raws = [storage_of(sf.F32, 3000 * ch, 900 + s) for s in range(S)]
    x = torch.from_numpy(np.stack(raws).reshape(S, 3000, ch)).cuda()
    out, made = b.process_tensor(x, out_capacity=wcap(3000, fi, fo), out_dtype=torch.int16)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ys = [twins[s].process_float(raws[s].reshape(-1, ch), wcap(3000, fi, fo))[0] for s in range(S)]
    settle("tensor", lambda s: np.ascontiguousarray(got[s, : made[s]]), made, ys, ch, sf.S16)
    for s in range(S):
        assert b.lines(s).tobytes() == twins[s]._lines().tobytes(), s
        twins[s].close()
    b.close()


def _batch_of_33():
    """one launch's 32 streams plus one: streams 0 and 32 are the long ones (2500 frames: one whole 4096-sample convert
    tile and a tail, four whole 512-frame mix tiles and a tail -- and 32 rows of any length start 16-byte aligned, so
    both take the 16-bytes-per-lane paths), the others short and ragged: the second launch's longest stream is not the
    first's, and each launch has whole tiles and element tails"""
    S, T = 33, 2500
    return S, T, [T if s in (0, S - 1) else 300 + 7 * s for s in range(S)]


def test_second_launch_of_a_batch_of_33_streams_with_dither():
    """three calls on one batch, positions continuing: formatted f32 -> s16 (dithered convert_out), mixed s16 stereo -> u8
    mono (convert_in, dithered mix_out), mixed u8 mono -> s24 on the stereo state (mix_in, dithered convert_out); every
    stream against its own float twin, the mix model and the dither model at the stream's seed and running position"""
    import torch
    S, T, lens = _batch_of_33()
    ch, fi, fo, q = 2, 44100, 48000, 7
    kind, seed, start = dm.TRIANGULAR, SEED, 12345
    cap = wcap(T, fi, fo)
    b = speexhip.Batch(S, ch, fi, fo, q)
    assert b.set_dither(kind, seed, start) == 0
    twins = [speexhip.Resampler(ch, fi, fo, q) for _ in range(S)]
    pos = [start] * S
    # (input format, its channels, in_mix, output format, its channels, out_mix)
    calls = ((sf.F32, 2, None, sf.S16, 2, None),
             (sf.S16, 2, None, sf.U8, 1, cm.STEREO_TO_MONO),
             (sf.U8, 1, cm.MONO_TO_STEREO, sf.S24, 2, None))
    for i, (in_fmt, c_in, in_mix, o, c_out, out_mix) in enumerate(calls):
        bo = sf.BYTES[o]
        raws = [storage_of(in_fmt, T * c_in, 1300 + 50 * i + s) for s in range(S)]
        src = torch.from_numpy(np.stack(raws)).cuda()
        row = cap * c_out * bo + 2 * bo   # bytes of a stream's row: room for cap frames and two samples of sentinel
        dst = torch.full((S, row), SENTINEL, dtype=torch.uint8, device="cuda")
        args = (in_fmt, src.data_ptr(), T * c_in, lens, o, dst.data_ptr(), row // bo, cap)
        stream = torch.cuda.current_stream().cuda_stream
        if in_mix is None and out_mix is None:
            used, made = b.process_fmt_device(*args, stream)
        else:
            used, made = b.process_mix_device(*args, in_mix, out_mix, stream)
        torch.cuda.synchronize()
        flat = dst.cpu().numpy()
        assert used == lens, i
        for s in range(S):
            x = sf.to_internal(in_fmt, raws[s][: lens[s] * c_in])
            xin = x if in_mix is None else cm.mix(in_mix, x)
            y, used_t = twins[s].process_float(xin.reshape(-1, ch), cap)
            yout = y if out_mix is None else cm.mix(out_mix, y)
            want = dm.from_internal(o, yout, kind, dm.stream_seed(seed, s), pos[s], c_out).view(np.uint8)
            assert (used[s], made[s]) == (used_t, y.shape[0]), (i, s)
            assert want.size == made[s] * c_out * bo and flat[s, : want.size].tobytes() == want.tobytes(), (i, s)
            assert (flat[s, want.size:] == SENTINEL).all(), (i, s)
            pos[s] += made[s]
            assert b.get_dither(s) == (kind, dm.stream_seed(seed, s), pos[s]), (i, s)
    for s in range(S):
        assert b.lines(s).tobytes() == twins[s]._lines().tobytes(), s
        twins[s].close()
    b.close()


def test_second_launch_of_a_batch_of_33_streams_without_dither():
    """s24 -> u8, formatted, no matrix, on a fresh batch: convert_in and the plain convert_out, every stream against a
    single state given the same call (as test_formatted_batch_equals_single_states)"""
    import torch
    S, T, lens = _batch_of_33()
    ch, fi, fo, q = 2, 44100, 48000, 7
    cap = wcap(T, fi, fo)
    raws = [storage_of(sf.S24, T * ch, 1500 + s) for s in range(S)]
    src = torch.from_numpy(np.stack(raws)).cuda()
    row = cap * ch + 2
    dst = torch.full((S, row), SENTINEL, dtype=torch.uint8, device="cuda")
    b = speexhip.Batch(S, ch, fi, fo, q)
    used, made = b.process_fmt_device(sf.S24, src.data_ptr(), T * ch, lens, sf.U8, dst.data_ptr(), row, cap,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    for s in range(S):
        r = speexhip.Resampler(ch, fi, fo, q)
        want, used_r = r.process_fmt(raws[s][: lens[s] * ch * 3], sf.S24, sf.U8, cap)
        assert (used[s], made[s] * ch) == (used_r, want.size), s
        assert flat[s, : want.size].tobytes() == want.tobytes(), s
        assert (flat[s, want.size:] == SENTINEL).all(), s
        assert b.lines(s).tobytes() == r._lines().tobytes(), s
        assert b.get_dither(s) == (dm.NONE, dm.stream_seed(0, s), 0), s
        r.close()
    b.close()


# ---- 6. off is what it was -------------------------------------------------------------------------------------------
def test_dither_off_is_the_undithered_call():
    ch, fi, fo, q = 2, 44100, 48000, 7
    calls = [(160, wcap(160, fi, fo)), (5000, 777), (20000, wcap(20000, fi, fo))]
    for setter in (None, lambda r: r.set_dither(dm.NONE, 99, 12345)):
        a, b, tf, ti = (speexhip.Resampler(ch, fi, fo, q) for _ in range(4))
        for r in (a, b):
            if setter is not None:
                assert setter(r) == 0
        for i, (frames, cap) in enumerate(calls):
            xf = storage_of(sf.F32, frames * ch, 10 + i)
            rc_t, used_t, made_t, out_t = tf.raw_call("float", xf, cap)
            rc, used, made, out = a.fmt_call(xf, sf.F32, sf.S16, cap)
            assert (rc, used, made) == (rc_t, used_t, made_t)
            assert out[: made * ch].tobytes() == sf.from_internal(sf.S16, out_t[:made_t]).tobytes(), i
            xi = storage_of(sf.S16, frames * ch, 20 + i)
            rc_t, used_t, made_t, out_t = ti.raw_call("int", xi, cap)
            rc, used, made, out = b.fmt_call(xi, sf.S16, sf.S16, cap)
            assert (rc, used, made) == (rc_t, used_t, made_t)
            assert out[: made * ch].tobytes() == out_t[:made_t].tobytes(), i
        # the position of a state without dither does not move
        assert a.get_dither() == ((dm.NONE, 0, 0) if setter is None else (dm.NONE, 99, 12345))
        same_state(a, tf, "f32->s16, off")
        same_state(b, ti, "s16->s16, off")
        for r in (a, b, tf, ti):
            r.close()


def test_s16_to_s16_follows_the_int_call_when_off_and_the_float_call_when_on():
    """8 kHz -> 96 kHz: a 160-frame block makes 1920 outputs, more than the 1024 the int entry emits per block (it goes
    round its loop twice and ends on the same count as the float entry here).  Off: the int16 call, bytes and counters.
    On: the float twin's counters and the model's bytes on the float twin's output."""
    cfg = (1, 8000, 96000, 3)
    x = storage_of(sf.S16, 160, 4)
    off, ti, on, tf = (speexhip.Resampler(*cfg) for _ in range(4))
    rc_t, used_t, made_t, out_t = ti.raw_call("int", x, 4000)
    rc, used, made, out = off.fmt_call(x, sf.S16, sf.S16, 4000)
    assert (rc, used, made) == (rc_t, used_t, made_t) and out[:made].tobytes() == out_t[:made_t].tobytes()
    assert on.set_dither(dm.TRIANGULAR, 3, 0) == 0
    rc_f, used_f, made_f, out_f = tf.raw_call("float", sf.to_internal(sf.S16, x), 4000)
    rc, used, made, out = on.fmt_call(x, sf.S16, sf.S16, 4000)
    assert (rc, used, made) == (rc_f, used_f, made_f)
    assert out[:made].tobytes() == dm.from_internal(sf.S16, out_f[:made_f], dm.TRIANGULAR, 3, 0, 1).tobytes()
    assert on.get_dither() == (dm.TRIANGULAR, 3, made)
    # a capacity that binds, where the two entries may count differently: the counters are the float entry's
    pos = made
    x = storage_of(sf.S16, 5000, 5)
    want = tf.peek(5000, 777, True)
    rc_f, used_f, made_f, out_f = tf.raw_call("float", sf.to_internal(sf.S16, x), 777)
    rc, used, made, out = on.fmt_call(x, sf.S16, sf.S16, 777)
    print("s16->s16 with dither, 5000 frames into 777: consumed, produced", (used, made), "float entry", (used_f, made_f))
    assert (rc, used, made) == (rc_f, used_f, made_f) == (0,) + want
    assert out[:made].tobytes() == dm.from_internal(sf.S16, out_f[:made_f], dm.TRIANGULAR, 3, pos, 1).tobytes()
    assert on.get_dither() == (dm.TRIANGULAR, 3, pos + made)
    same_state(on, tf, "s16->s16, on")
    same_state(off, ti, "s16->s16, off")
    for r in (off, ti, on, tf):
        r.close()


# ---- 7. float outputs ------------------------------------------------------------------------------------------------
def test_float_outputs_are_written_as_ever_and_count_their_frames():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = storage_of(sf.F32, 6000 * ch, 8)
    cap = wcap(6000, fi, fo)
    for in_fmt, o in ((sf.F32, sf.F32N), (sf.F32N, sf.F32N), (sf.F32, sf.F32)):
        xin = x if in_fmt == sf.F32 else x / np.float32(32768.0)
        plain, dith = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
        dith.set_dither(dm.RECTANGULAR, 1, 40)
        pos = 40
        for _ in range(2):
            a, used_a = plain.process_fmt(xin, in_fmt, o, cap)
            b, used_b = dith.process_fmt(xin, in_fmt, o, cap)
            assert used_a == used_b and a.tobytes() == b.tobytes(), (sf.NAMES[in_fmt], sf.NAMES[o])
            pos += a.size // ch
            assert dith.get_dither() == (dm.RECTANGULAR, 1, pos)
        # ... and the next integer call finds its noise at that position
        y, _ = plain.process_float(x.reshape(-1, ch), cap)
        got, _ = dith.process_fmt(x, sf.F32, sf.S24, cap)
        assert got.tobytes() == dm.from_internal(sf.S24, y, dm.RECTANGULAR, 1, pos, ch).tobytes()
        plain.close()
        dith.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------
def test_unknown_kind_is_refused_and_control_calls_leave_dither_alone():
    r = speexhip.Resampler(2, 44100, 48000, 7)
    assert r.set_dither(dm.TRIANGULAR, 17, 4) == 0
    for kind in (-1, 3, 77):
        assert r.set_dither(kind, 1, 2) == speexhip.ERR_INVALID_ARG
        assert r.get_dither() == (dm.TRIANGULAR, 17, 4)
    r.process_fmt(storage_of(sf.F32, 2000, 1), sf.F32, sf.U8, 1200)
    before = r.get_dither()
    assert before[2] > 4
    r.set_rate(48000, 44100)
    r.set_quality(5)
    r.skip_zeros()
    r.reset_mem()
    # the calls outside the formatted and mixed ones do not move the position either
    r.process(np.zeros((500, 2), np.int16), 600)
    r.process_float(np.zeros((500, 2), np.float32), 600)
    assert r.get_dither() == before
    r.close()
    b = speexhip.Batch(2, 2, 44100, 48000, 7)
    assert b.set_dither(9, 1, 2) == speexhip.ERR_INVALID_ARG and b.get_dither(1) == (dm.NONE, dm.stream_seed(0, 1), 0)
    b.close()


def test_channels_moved_apart_return_bad_state_with_dither_on():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    r.set_dither(dm.TRIANGULAR, 1, 10)
    rc, _, _, _ = r.channel_call("float", 0, np.zeros(300, np.float32), 400)
    assert rc == 0
    before = (r.positions(), r.history().tobytes())
    raw = storage_of(sf.F32, 1000 * ch, 2)
    out = np.full(1200 * ch, 0x5A5A, np.int16)
    L = speexhip.lib()
    for device in (False, True):
        il, ol = C.c_uint32(1000), C.c_uint32(1200)
        if device:
            rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, sf.F32, None, C.byref(il), sf.S16,
                                                                     C.c_void_p(out.ctypes.data), C.byref(ol), None)
        else:
            rc = L.speexhip_resampler_process_interleaved_fmt(r._h, sf.F32, C.c_void_p(raw.ctypes.data), C.byref(il), sf.S16,
                                                              C.c_void_p(out.ctypes.data), C.byref(ol))
        assert rc == speexhip.ERR_BAD_STATE and (il.value, ol.value) == (1000, 1200), device
    assert (out == 0x5A5A).all()
    assert r.get_dither() == (dm.TRIANGULAR, 1, 10)
    assert (r.positions(), r.history().tobytes()) == before
    # without dither the same state is served channel by channel, as ever
    assert r.set_dither(dm.NONE, 0, 0) == 0
    rc, _, _, _ = r.fmt_call(raw, sf.F32, sf.S16, 1200)
    assert rc == 0
    r.close()


def test_zero_fallback_zeros_are_dithered():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = storage_of(sf.S16, 3000 * ch, 5)
    p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    try:
        p.set_dither(dm.TRIANGULAR, SEED, 0)
        got, _ = p.process_fmt(x, sf.S16, sf.U8, wcap(3000, fi, fo))
        t.process_float(sf.to_internal(sf.S16, x).reshape(-1, ch), wcap(3000, fi, fo))
        pos = got.size // ch
        for r in (p, t):
            speexhip.lib().speexhip_debug_fail_device_allocs(1)
            rc = r.set_rate(32000, 48000)
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            assert rc == speexhip.ERR_ALLOC_FAILED
        y = storage_of(sf.S16, 2000 * ch, 6)
        rc_t, used_t, made_t, out_t = t.raw_call("float", sf.to_internal(sf.S16, y).reshape(-1, ch), 2500)
        rc_p, used_p, made_p, out_p = p.fmt_call(y, sf.S16, sf.U8, 2500)
        assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
        assert not out_t[:made_t].any()
        want = dm.from_internal(sf.U8, np.zeros(made_t * ch, np.float32), dm.TRIANGULAR, SEED, pos, ch)
        assert out_p[: made_p * ch].tobytes() == want.tobytes()
        assert set(np.unique(want).tolist()) == {127, 128, 129}, "TPDF on the format's zero reaches both neighbours"
        check_tail(out_p, sf.U8, made_p, ch, "zero fallback")
        assert p.get_dither()[2] == pos + made_p
        assert p.positions() == t.positions()
    finally:
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        p.close()
        t.close()


# ---- 9. Node ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_set_dither_gives_the_python_bindings_bytes(tmp_path):
    ch, fi, fo, q = 2, 44100, 48000, 7
    cuts = [480, 4097, 1, 9000]
    pcm = storage_of(sf.S16, sum(cuts) * ch, 44)
    src, dst = tmp_path / "in.s16le", tmp_path / "out.u8"
    src.write_bytes(pcm.tobytes())
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_dither.js")
    res = subprocess.run(["node", script, str(src), str(dst), ",".join(map(str, cuts))], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL DITHER NODE TESTS PASSED" in res.stdout
    told = json.loads(res.stdout.strip().splitlines()[-2])
    # the same state through the Python binding, with the wrapper's grow-only capacity rule (reference src/index.ts:80-95)
    r = speexhip.Resampler(ch, fi, fo, q)
    r.set_dither(dm.TRIANGULAR, 5, 0)
    got, at, room = [], 0, 0
    for n in cuts:
        room = max(room, -(-(n * ch * 4 * fo) // fi))
        # (the rule's capacity may bind and leave a frame unread: the wrapper drops it, and so does this loop)
        out, used = r.process_fmt(pcm[at * ch: (at + n) * ch], sf.S16, sf.U8, room // ch // 4)
        got.append(out)
        at += n
    want = np.concatenate(got)
    assert dst.read_bytes() == want.tobytes()
    assert told == {"kind": "triangular", "seed": "5", "position": str(want.size // ch)}
    assert r.get_dither() == (dm.TRIANGULAR, 5, want.size // ch)
    r.close()
