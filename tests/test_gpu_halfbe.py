"""Half-float (F16N, BF16N) and big-endian (S16BE, S24BE, S32BE) sample formats in the formatted, mixed, sides and batch
calls, on the GPU.  The rule under test: a call with one of these formats on either side IS the float call on the decoded
(and mixed) input followed by the output mix and the encoder.  Decoder, encoder, mix and dither are exact statements
(halfbe_model.py, sample_formats.py, channel_mix.py, dither_model.py), so every comparison with a twin state driven
through the existing float call is equality of bytes; there are no tolerances in this file."""
import ctypes as C
import json
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
import halfbe_model as hm
import oracle as orc
import sample_formats as sf
import speexhip
from golden_util import ROOT
from test_gpu_formats import storage_of
from test_gpu_g711 import storage as old_storage
from test_gpu_planar import MODES, same_state, wcap
from test_gpu_sides import device_sides, frames_of_planes, planes_of

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 8000, 16000, 7), (2, 44100, 48000, 7), (1, 8000, 48000, 3)]
SENTINEL = speexhip.Resampler.SENTINEL_BYTE
SEED = 0xDEADBEEFCAFEF00D
START = (1 << 32) - 5
FMT_IDS = [hm.name(f) for f in hm.ALL]
NEW_IDS = [hm.name(f) for f in hm.NEW]
KINDS = (dm.NONE,) + tuple(dm.KINDS)
KIND_IDS = [dm.KIND_NAMES[k] for k in KINDS]
CODES = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def finite_codes(fmt):
    """the 16-bit codes of a half format whose decode is finite"""
    with np.errstate(all="ignore"):
        return CODES[np.isfinite(hm.to_internal(fmt, CODES.view(hm.dtype(fmt))))]


def non_finite_codes(fmt):
    with np.errstate(all="ignore"):
        return CODES[~np.isfinite(hm.to_internal(fmt, CODES.view(hm.dtype(fmt))))]


def storage(fmt, n, seed, quiet=False, codes=None):
    """n samples of any of the thirteen formats as its flat storage array: full-scale LCG noise (or a quiet stretch)
    through the model's encoder; codes: 16-bit codes that replace the first samples of a half format"""
    if fmt not in hm.NEW:
        return old_storage(fmt, n, seed, quiet, all_codes=fmt in (gm.ULAW, gm.ALAW) and n >= 256)
    if fmt in hm.BIG:
        return hm.be_of(fmt, storage_of(hm.LE_TWIN[fmt], n, seed, quiet))
    st = hm.from_internal(fmt, storage_of(sf.F32, n, seed, quiet)).copy()
    if codes is not None:
        k = min(n, codes.size)
        st.view(np.uint16)[:k] = codes[:k]
    return st


def raw_bytes(fmt, st):
    return hm.raw(fmt, st)


def frames_of(fmt, st, ch):
    return raw_bytes(fmt, st).size // hm.nbytes(fmt) // ch


def check_tail(out, fmt, made, c_out, what):
    assert (out.view(np.uint8)[made * c_out * hm.nbytes(fmt):] == SENTINEL).all(), what + ": written past produced"


def produced(out, fmt, made, c_out):
    return out.view(np.uint8)[: made * c_out * hm.nbytes(fmt)].tobytes()


def device_call(r, in_fmt, st, out_fmt, cap, c_in, c_out, in_off, out_off, torch, in_mix=None, out_mix=None):
    """formatted / mixed device call with the input `in_off` and the output `out_off` bytes off a 16-byte boundary, guard
    bytes around the output (checked); returns (consumed, produced, output bytes)"""
    raw = raw_bytes(in_fmt, st)
    src = torch.zeros(64 + raw.nbytes + 64, dtype=torch.uint8, device="cuda")
    src[16 + in_off: 16 + in_off + raw.nbytes] = torch.from_numpy(raw.copy()).cuda()
    room = cap * c_out * hm.nbytes(out_fmt)
    dst = torch.full((64 + room + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    frames = frames_of(in_fmt, st, c_in)
    stream = torch.cuda.current_stream().cuda_stream
    if in_mix is None and out_mix is None:
        used, made = r.process_fmt_device(in_fmt, src.data_ptr() + 16 + in_off, frames, out_fmt,
                                          dst.data_ptr() + 16 + out_off, cap, stream)
    else:
        used, made = r.process_mix_device(in_fmt, src.data_ptr() + 16 + in_off, frames, out_fmt,
                                          dst.data_ptr() + 16 + out_off, cap, in_mix, out_mix, stream)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    n = made * c_out * hm.nbytes(out_fmt)
    lo = 16 + out_off
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "bytes outside the produced samples written"
    return used, made, flat[lo: lo + n].copy()


# ---- 1. the float twin, byte for byte --------------------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", hm.ALL, ids=FMT_IDS)
@pytest.mark.parametrize("mode", ("default", "exact"))
def test_new_format_call_equals_the_float_twin(mode, in_fmt):
    """a new input to every output format, every old input to the five new outputs: counters, bytes, the untouched tail,
    position and final state are the float twin's.  Half-float inputs carry every code over the configurations, the ones
    that do not decode to a finite value in a call of their own at the end."""
    out_fmts = hm.ALL if in_fmt in hm.NEW else hm.NEW
    half_in = in_fmt in hm.HALF
    todo = finite_codes(in_fmt) if half_in else None
    fed = []
    rails = {o: [False, False] for o in hm.BIG}
    for cfg in CONFIGS:
        ch, fi, fo, q = cfg
        # (frames or None for silence, capacity, silent frames, quiet, codes)
        calls = [(1, 8, 0, False, None), (15, 100, 0, False, None), (16, 100, 0, False, None), (17, 110, 0, False, None),
                 (160, wcap(160, fi, fo), 0, False, None), (4097, wcap(4097, fi, fo), 0, True, None),
                 (0, 64, 0, False, None),                       # an empty call
                 (None, 600, 480, False, None),                 # silence
                 (5000, 777, 0, False, None),                   # a capacity that binds
                 (20000, wcap(20000, fi, fo), 0, False, "finite")]
        if half_in:
            calls.append((4200, wcap(4200, fi, fo), 0, False, "non-finite"))
        mk = lambda: speexhip.Resampler(ch, fi, fo, q, mode=MODES[mode])
        states = {o: mk() for o in out_fmts}
        twin = mk()
        try:
            for i, (frames, cap, silent, quiet, which) in enumerate(calls):
                codes = None
                if half_in and which == "finite":
                    codes, todo = todo[: frames * ch], todo[frames * ch:]
                elif half_in and which == "non-finite":
                    codes = non_finite_codes(in_fmt)
                st = None if frames is None else storage(in_fmt, frames * ch, 31 * ch + q + 17 * i, quiet, codes)
                with np.errstate(all="ignore"):
                    x = None if st is None else hm.to_internal(in_fmt, st)
                rc_t, used_t, made_t, out_t = twin.raw_call("float", x, cap, silent)
                y = out_t[:made_t].reshape(-1)
                if half_in and st is not None:
                    assert used_t == frames or which is None
                    fed.append(st.view(np.uint16)[: used_t * ch])
                for o, r in states.items():
                    what = "%s mode=%s %s->%s call %d (%s frames, cap %d)" % (cfg, mode, hm.name(in_fmt), hm.name(o), i, frames, cap)
                    rc, used, made, out = r.fmt_call(st, in_fmt, o, cap, silent)
                    assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
                    with np.errstate(all="ignore"):
                        want = hm.from_internal(o, y)
                    assert produced(out, o, made, ch) == raw_bytes(o, want).tobytes(), what + ": samples"
                    check_tail(out, o, made, ch, what)
                    assert r.position() == twin.position(), what
                    if o in hm.BIG and made:
                        v = sf.integers(hm.LE_TWIN[o], hm.le_of(o, want))
                        bits = 8 * hm.nbytes(o)
                        rails[o][0] |= bool((v == -(1 << (bits - 1))).any())
                        rails[o][1] |= bool((v == (1 << (bits - 1)) - 1).any())
            for o, r in states.items():
                same_state(r, twin, "%s mode=%s %s->%s" % (cfg, mode, hm.name(in_fmt), hm.name(o)))
        finally:
            for r in list(states.values()) + [twin]:
                r.close()
    if half_in:
        assert todo.size == 0 and np.unique(np.concatenate(fed)).size == 65536, "the input holds every code"
    # full-scale noise reaches both rails of the big-endian outputs
    if in_fmt not in hm.HALF and in_fmt not in (gm.ULAW, gm.ALAW, sf.U8):
        for o in hm.BIG:
            assert rails[o] == [True, True], (mode, hm.name(in_fmt), hm.name(o))


# ---- 2. the little-endian twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_big_endian_call_is_the_little_endian_call_byte_reversed(kind):
    """S16BE / S24BE / S32BE -> F32N and F32 -> each of them against the little-endian call on a twin state, dither off and
    on: the bytes are the twin's with every sample reversed, the position advances alike"""
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 4096 + 4097
    cap = wcap(frames, fi, fo)
    for be in hm.BIG:
        le = hm.LE_TWIN[be]
        for in_be, out_be in ((True, False), (False, True)):
            r, t = speexhip.Resampler(*cfg), speexhip.Resampler(*cfg)
            if kind != dm.NONE:
                assert r.set_dither(kind, SEED, START) == 0 and t.set_dither(kind, SEED, START) == 0
            st_le = storage_of(le if in_be else sf.F32, frames * ch, 40 + be)
            st = hm.be_of(be, st_le) if in_be else st_le
            in_r, out_r = (be, sf.F32N) if in_be else (sf.F32, be)
            in_t, out_t = (le, sf.F32N) if in_be else (sf.F32, le)
            what = (dm.KIND_NAMES[kind], hm.name(in_r), hm.name(out_r))
            rc, used, made, out = r.fmt_call(st, in_r, out_r, cap)
            rc_t, used_t, made_t, out_tw = t.fmt_call(st_le, in_t, out_t, cap)
            assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0 and made > 4096, what
            got, want = produced(out, out_r, made, ch), produced(out_tw, out_t, made, ch)
            if out_be:
                want = hm.reverse(be, np.frombuffer(want, np.uint8)).tobytes()
                assert got != produced(out_tw, out_t, made, ch), what
            assert got == want, what
            check_tail(out, out_r, made, ch, str(what))
            assert r.get_dither() == t.get_dither(), what
            if kind != dm.NONE:
                assert r.get_dither() == (kind, SEED, START + made), what      # (across 2^32)
            same_state(r, t, str(what))
            r.close()
            t.close()


def test_s16be_to_s16be_follows_the_float_entrys_counters():
    """no identity pair among the new formats: S16BE -> S16BE decodes, filters and encodes by the float entry's rules.  One
    160-frame input with capacity 2000 at 8 k -> 96 k makes more than a sides tile of frames."""
    ch, fi, fo, q = 1, 8000, 96000, 7
    r, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
    for i in range(3):
        st = storage(hm.S16BE, 160 * ch, 5 + i)
        x = hm.to_internal(hm.S16BE, st)
        rc_t, used_t, made_t, out_t = t.raw_call("float", x, 2000)
        rc, used, made, out = r.fmt_call(st, hm.S16BE, hm.S16BE, 2000)
        assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0 and made > 1024, i
        assert produced(out, hm.S16BE, made, ch) == raw_bytes(hm.S16BE, hm.from_internal(hm.S16BE, out_t[:made_t].reshape(-1))).tobytes()
        assert r.position() == t.position(), i
    same_state(r, t, "s16be -> s16be")
    r.close()
    t.close()


# ---- 3. addressing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(hm.S24BE, hm.S24BE), (hm.S16BE, hm.F16N), (hm.BF16N, hm.S32BE), (hm.F16N, hm.BF16N),
                                  (hm.S32BE, hm.S16BE)], ids=["s24be-s24be", "s16be-f16n", "bf16n-s32be", "f16n-bf16n", "s32be-s16be"])
def test_new_format_addressing_offsets_tails_and_guards(pair):
    """whole 4096-sample tiles plus a tail; offset 0 takes the 16-bytes-per-lane path, every other allowed offset (any byte
    for S24BE, element-aligned ones for the rest) the element path on the same data -- one answer"""
    import torch
    in_fmt, out_fmt = pair
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37
    cap = wcap(frames, fi, fo)
    st = storage(in_fmt, frames * ch, 77 + in_fmt, codes=CODES[::7] if in_fmt in hm.HALF else None)
    if in_fmt in hm.HALF:      # (finite samples only)
        ok = np.isin(st.view(np.uint16), finite_codes(in_fmt))
        st.view(np.uint16)[~ok] = 0
    t = speexhip.Resampler(*cfg)
    y, used_t = t.process_float(hm.to_internal(in_fmt, st).reshape(-1, ch), cap)
    with np.errstate(all="ignore"):
        want = raw_bytes(out_fmt, hm.from_internal(out_fmt, y)).tobytes()
    assert y.shape[0] * ch > 2 * 4096      # (whole tiles on the way out as well)
    offs = lambda f: {2: (0, 2, 6, 14), 3: (0, 1, 2, 3), 4: (0, 4, 12)}[hm.nbytes(f)]
    pairs = [(a, 0) for a in offs(in_fmt)] + [(0, b) for b in offs(out_fmt)[1:]] + [(offs(in_fmt)[-1], offs(out_fmt)[-1])]
    for in_off, out_off in pairs:
        r = speexhip.Resampler(*cfg)
        used, made, got = device_call(r, in_fmt, st, out_fmt, cap, ch, ch, in_off, out_off, torch)
        what = (hm.name(in_fmt), hm.name(out_fmt), in_off, out_off)
        assert (used, made) == (used_t, y.shape[0]), what
        assert got.tobytes() == want, what
        same_state(r, t, str(what))
        r.close()
    t.close()


# ---- 4. the mix pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(hm.S16BE, hm.F16N, True), (hm.BF16N, hm.S24BE, False)], ids=["2-1-1-s16be-f16n", "1-1-2-bf16n-s24be"])
def test_new_format_mixed_calls_equal_the_model_around_the_float_twin(case):
    """S16BE stereo -> mono F16N with [[0.5, 0.5]] -- mix_in's tile path on whole 512-frame tiles, its element path on the
    tail and off alignment -- and mono BF16N -> stereo S24BE: channel_mix.py around the float twin, 4097 frames"""
    import torch
    in_fmt, out_fmt, down = case
    fi, fo, q = 8000, 16000, 7
    in_mix, out_mix = (cm.STEREO_TO_MONO, None) if down else (None, cm.MONO_TO_STEREO)
    assert np.array_equal(cm.STEREO_TO_MONO, np.float32([[0.5, 0.5]]))
    c_in, c_out = (2, 1) if down else (1, 2)
    frames = 4097
    cap = wcap(frames, fi, fo)
    r, t = speexhip.Resampler(1, fi, fo, q), speexhip.Resampler(1, fi, fo, q)
    in_offs = {2: (2, 6), 3: (3, 1), 4: (4, 12)}
    o_in, o_out = in_offs[hm.nbytes(in_fmt)], in_offs[hm.nbytes(out_fmt)]
    for i, (route, in_off, out_off) in enumerate((("host", 0, 0), ("device", 0, 0), ("device", o_in[0], o_out[0]),
                                                  ("device", 0, o_out[1]), ("device", o_in[1], 0))):
        st = storage(in_fmt, frames * c_in, 60 + i, codes=finite_codes(in_fmt)[i::5] if in_fmt in hm.HALF else None)
        with np.errstate(all="ignore"):
            x = hm.to_internal(in_fmt, st)
            xin = x if in_mix is None else cm.mix(in_mix, x).reshape(-1)
        rc_t, used_t, made_t, out_t = t.raw_call("float", xin, cap)
        y = out_t[:made_t].reshape(-1)
        with np.errstate(all="ignore"):
            yout = y if out_mix is None else cm.mix(out_mix, y).reshape(-1)
            want = raw_bytes(out_fmt, hm.from_internal(out_fmt, yout)).tobytes()
        what = (hm.name(in_fmt), hm.name(out_fmt), c_in, c_out, route, in_off, out_off)
        if route == "host":
            rc, used, made, out = r.mix_call(st, in_fmt, out_fmt, in_mix, out_mix, cap)
            assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0, what
            assert produced(out, out_fmt, made, c_out) == want, what
            check_tail(out, out_fmt, made, c_out, str(what))
        else:
            used, made, got = device_call(r, in_fmt, st, out_fmt, cap, c_in, c_out, in_off, out_off, torch, in_mix, out_mix)
            assert (used, made) == (used_t, made_t), what
            assert got.tobytes() == want, what
        same_state(r, t, str(what))
    r.close()
    t.close()


# ---- 5. the planar pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", hm.NEW, ids=NEW_IDS)
def test_planes_of_each_new_format_equal_the_interleaved_call_transposed(fmt):
    """(C, T) device planes of the format in and out, C = 2 and 3, T = 1025 and 3000 (one whole 1024-frame tile and a tail;
    two and a tail), plane strides that are multiples of 16 bytes (the vector path) and ones that are not (the element
    path), with a matrix, and with dither for the big-endian formats"""
    import torch
    base = (44100, 48000, 7)
    fi, fo, q = base
    fold = np.float32([[1.0, 0.5, 0.0], [0.0, 0.5, 1.0]])      # 3 planes in, a stereo state
    widen = np.float32([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])   # a stereo state, 3 planes out
    shapes = [(c, T, None, None, None) for c in (2, 3) for T in (1025, 3000)]
    shapes += [(2, 3000, fold, None, None), (2, 1025, None, widen, None)]
    if fmt in hm.BIG:
        shapes += [(2, 3000, None, None, dm.TRIANGULAR), (3, 1025, None, None, dm.RECTANGULAR), (2, 3000, None, widen, dm.TRIANGULAR)]
    for c, T, in_mix, out_mix, dither in shapes:
        n_in = c if in_mix is None else in_mix.shape[1]
        n_out = c if out_mix is None else out_mix.shape[0]
        cap = wcap(T, fi, fo)
        st = storage(fmt, T * n_in, 3 * c + T + fmt, codes=finite_codes(fmt)[c::3] if fmt in hm.HALF else None)
        t = speexhip.Resampler(c, fi, fo, q)
        if dither is not None:
            t.set_dither(dither, 77, 5)
        rc_t, used_t, made_t, out_t = t.mix_call(st, fmt, fmt, in_mix, out_mix, cap)
        assert rc_t == 0 and made_t > 1024
        bo = hm.nbytes(fmt)
        want = produced(out_t, fmt, made_t, n_out)
        # strides in samples: 4096 is whole 16-byte pieces of every format; + 1 (and plane 0 one sample in) is not
        for in_off, in_stride, out_off, out_stride in ((0, 4096, 0, 4096), (1, 4097, 1, 4097), (0, 4096, 1, 4097)):
            what = (hm.name(fmt), c, T, in_mix is not None, out_mix is not None, dither, in_off, out_off)
            used, made, buf, r = device_sides(base, c, fmt, fmt, st, T, cap, in_mix, out_mix, in_off, in_stride, out_off,
                                              out_stride, torch, dither)
            assert (used, made) == (used_t, made_t), what
            touched = np.zeros(buf.size, bool)
            got = []
            for ch in range(n_out):
                at = (out_off + ch * out_stride) * bo
                got.append(buf[at: at + made * bo].reshape(made, bo))
                touched[at: at + made * bo] = True
            assert np.stack(got, axis=1).tobytes() == want, what
            assert (buf[~touched] == SENTINEL).all(), what
            same_state(r, t, str(what))
            assert r.get_dither() == t.get_dither(), what
            r.close()
        t.close()


def test_host_planes_of_the_new_formats():
    """the host form of the sides call, planar in and planar out, against the host mixed call"""
    fi, fo, q = 44100, 48000, 7
    for in_fmt, out_fmt in ((hm.S16BE, hm.BF16N), (hm.F16N, hm.S24BE), (hm.S24BE, hm.S32BE), (hm.S32BE, hm.F16N)):
        r, t = speexhip.Resampler(2, fi, fo, q), speexhip.Resampler(2, fi, fo, q)
        for T in (17, 1025, 3000):
            st = storage(in_fmt, T * 2, T + in_fmt)
            cap = wcap(T, fi, fo)
            rc_t, used_t, made_t, out_t = t.mix_call(st, in_fmt, out_fmt, None, None, cap)
            rc, used, made, out = r.sides_call(planes_of(in_fmt, st, 2), in_fmt, out_fmt, cap, "planar", "planar")
            assert (rc, used, made) == (rc_t, used_t, made_t) and rc == 0
            assert frames_of_planes(out_fmt, out, made) == produced(out_t, out_fmt, made_t, 2), (hm.name(in_fmt), hm.name(out_fmt), T)
            res, _ = speexhip.Resampler(2, fi, fo, q).process_sides(planes_of(in_fmt, st, 2), in_fmt, out_fmt, cap, "planar", "planar")
            assert res.shape[0] == 2 and res.dtype == hm.dtype(out_fmt)
        same_state(r, t, "host planes")
        r.close()
        t.close()


# ---- 6. batches and tensors ----------------------------------------------------------------------------------------------
def bits_of(tensor, torch):
    """the 16-bit codes of a float16 / bfloat16 tensor, as a numpy uint16 array"""
    return tensor.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def half_tensor(bits, dtype, torch):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(dtype).cuda()


@pytest.mark.parametrize("fmt", hm.HALF, ids=[hm.name(f) for f in hm.HALF])
@pytest.mark.parametrize("layout", ("interleaved", "planar"))
def test_process_tensor_in_half_precision(layout, fmt):
    """3 streams of (4097, 0, 160) frames: float16 / bfloat16 in and out, interleaved and planar, equal single states'
    results, and on finite data the F32N result cast by torch -- an independent statement of round-to-nearest-even"""
    import torch
    tdt = torch.float16 if fmt == hm.F16N else torch.bfloat16
    S, ch, fi, fo, q, T = 3, 2, 44100, 48000, 7, 4097
    lens = [4097, 0, 160]
    cap = wcap(T, fi, fo)
    planar = layout == "planar"
    kw = dict(in_layout="planar", out_layout="planar") if planar else {}
    sts = [storage(fmt, T * ch, 500 + s, quiet=(s == 2)) for s in range(S)]
    s16 = [storage_of(sf.S16, T * ch, 700 + s) for s in range(S)]

    def tensor_of(arrs, dtype):
        a = np.stack([np.ascontiguousarray(v).reshape(T, ch) for v in arrs])            # (S, T, ch)
        if planar:
            a = np.ascontiguousarray(a.transpose(0, 2, 1))
        return half_tensor(a, dtype, torch) if dtype in (torch.float16, torch.bfloat16) else torch.from_numpy(a).cuda()

    def frames_first(arr, s, made):
        a = arr[s]
        return np.ascontiguousarray((a.T if planar else a)[:made])

    # (x, out_dtype, normalized, in_fmt, out_fmt, sources)
    cases = [(tensor_of([v.view(np.uint16) for v in sts], tdt), None, False, fmt, fmt, sts),
             (tensor_of(s16, torch.int16), tdt, True, sf.S16, fmt, s16),
             (tensor_of([v.view(np.uint16) for v in sts], tdt), torch.float32, True, fmt, sf.F32N, sts)]
    for x, out_dtype, normalized, in_fmt, out_fmt, src in cases:
        b = speexhip.Batch(S, ch, fi, fo, q)
        out, made = b.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=out_dtype, normalized=normalized, **kw)
        # the F32N result of the same input, on a twin batch
        b32 = speexhip.Batch(S, ch, fi, fo, q)
        out32, made32 = b32.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=torch.float32, normalized=True, **kw)
        torch.cuda.synchronize()
        assert made == made32 and made[1] == 0 and made[0] > 4096
        assert out.dtype == (tdt if out_fmt == fmt else torch.float32)
        assert tuple(out.shape) == ((S, ch, max(made)) if planar else (S, max(made), ch))
        got = bits_of(out, torch) if out_fmt == fmt else out.cpu().numpy()
        for s in range(S):
            what = (layout, hm.name(in_fmt), hm.name(out_fmt), s)
            r = speexhip.Resampler(ch, fi, fo, q)
            want, used = r.process_fmt(src[s][: lens[s] * ch], in_fmt, out_fmt, cap)
            assert made[s] * ch == want.size, what
            assert frames_first(got, s, made[s]).tobytes() == want.tobytes(), what
            assert b.lines(s).tobytes() == r._lines().tobytes(), what
            r.close()
        if out_fmt == fmt:
            cast = out32.to(tdt)
            for s in range(S):
                n = made[s]
                a = out[s, :, :n] if planar else out[s, :n]
                c = cast[s, :, :n] if planar else cast[s, :n]
                assert torch.isfinite(out32[s, :, :n] if planar else out32[s, :n]).all()
                assert torch.equal(a.contiguous().view(torch.int16), c.contiguous().view(torch.int16)), (layout, hm.name(fmt), s)
        b.close()
        b32.close()


def test_process_tensor_takes_big_endian_formats_and_mixes():
    import torch
    S, fi, fo, q, T = 3, 8000, 16000, 7, 4097
    lens = [4097, 0, 160]
    cap = wcap(T, fi, fo)
    # RTP L16 stereo in, mono bfloat16 planes out; mono float16 in, big-endian s32 stereo out
    for in_fmt, out_fmt, in_mix, out_mix, out_dtype in ((hm.S16BE, hm.BF16N, cm.STEREO_TO_MONO, None, torch.bfloat16),
                                                         (hm.F16N, hm.S32BE, None, cm.MONO_TO_STEREO, None)):
        c_in = 2 if in_mix is not None else 1
        c_out = 2 if out_mix is not None else 1
        sts = [storage(in_fmt, T * c_in, 300 + s) for s in range(S)]
        host = np.stack([raw_bytes(in_fmt, v).view(np.int16).reshape(T, c_in) for v in sts])
        x = torch.from_numpy(host).cuda()
        if in_fmt == hm.F16N:
            x = x.view(torch.float16)
        b = speexhip.Batch(S, 1, fi, fo, q)
        out, made = b.process_tensor(x, out_capacity=cap, in_frames=lens, out_dtype=out_dtype, in_mix=in_mix, out_mix=out_mix,
                                     in_format=in_fmt if in_fmt in hm.BIG else None,
                                     out_format=out_fmt if out_fmt in hm.BIG else None,
                                     in_layout="interleaved", out_layout="planar")
        torch.cuda.synchronize()
        assert out.dtype == (torch.bfloat16 if out_fmt == hm.BF16N else torch.int32)
        raw = out.contiguous().view(torch.uint8).cpu().numpy().reshape(S, c_out, -1)
        for s in range(S):
            r = speexhip.Resampler(1, fi, fo, q)
            want, _ = r.process_mix(sts[s][: lens[s] * c_in], in_fmt, out_fmt, cap, in_mix, out_mix)
            bo = hm.nbytes(out_fmt)
            got = np.ascontiguousarray(raw[s].reshape(c_out, -1, bo)[:, : made[s]].transpose(1, 0, 2))
            assert got.tobytes() == raw_bytes(out_fmt, want).tobytes(), (hm.name(in_fmt), hm.name(out_fmt), s)
            r.close()
        b.close()
    b = speexhip.Batch(1, 1, fi, fo, q)
    with pytest.raises(ValueError):      # a format names its storage type
        b.process_tensor(torch.zeros((1, 100, 1), dtype=torch.float32, device="cuda"), in_format=hm.S16BE)
    b.close()


# ---- 7. edges ------------------------------------------------------------------------------------------------------------
def test_non_finite_float_input_to_every_new_output():
    ch, fi, fo, q = 1, 16000, 48000, 7
    n = 6000
    x = orc.lcg_pcm(n, 8).astype(np.float32)
    x[1000], x[2500], x[4000], x[4001] = np.inf, -np.inf, np.inf, -np.inf
    t = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
    y, _ = t.process_float(x.reshape(-1, 1), wcap(n, fi, fo))
    t.close()
    y = y.reshape(-1)
    assert np.isposinf(y).any() and np.isneginf(y).any() and np.isnan(y).any()
    for out_fmt in hm.NEW:
        for kind in (dm.NONE, dm.TRIANGULAR):
            r = speexhip.Resampler(ch, fi, fo, q, mode=speexhip.MODE_EXACT)
            r.set_dither(kind, 3, 0)
            got, _ = r.process_fmt(x, sf.F32, out_fmt, wcap(n, fi, fo))
            r.close()
            with np.errstate(all="ignore"):
                want = hm.from_internal_dither(out_fmt, y, kind, 3, 0, 1)
            assert raw_bytes(out_fmt, got).tobytes() == raw_bytes(out_fmt, want).tobytes(), (hm.name(out_fmt), kind)
            if out_fmt in hm.BIG:
                v = sf.integers(hm.LE_TWIN[out_fmt], hm.le_of(out_fmt, got))
                bits = 8 * hm.nbytes(out_fmt)
                assert (v[np.isnan(y)] == 0).all() and (v[np.isposinf(y)] == (1 << (bits - 1)) - 1).all() \
                    and (v[np.isneginf(y)] == -(1 << (bits - 1))).all()
            else:
                codes = got.view(np.uint16)
                inf, nan = (0x7C00, 0x7E00) if out_fmt == hm.F16N else (0x7F80, 0x7FC0)
                assert (codes[np.isposinf(y)] == inf).all() and (codes[np.isneginf(y)] == (inf | 0x8000)).all()
                assert ((codes[np.isnan(y)] & 0x7FFF) == nan).all()      # canonical, whatever the FIR's payload


def test_zero_fallback_writes_each_formats_zero():
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = storage(hm.S16BE, 3000 * ch, 5)
    for out_fmt in hm.NEW:
        p, t = speexhip.Resampler(ch, fi, fo, q), speexhip.Resampler(ch, fi, fo, q)
        try:
            p.process_fmt(x, hm.S16BE, out_fmt, wcap(3000, fi, fo))
            t.process_float(hm.to_internal(hm.S16BE, x).reshape(-1, ch), wcap(3000, fi, fo))
            for r in (p, t):
                speexhip.lib().speexhip_debug_fail_device_allocs(1)
                rc = r.set_rate(32000, 48000)
                speexhip.lib().speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            y = storage(hm.S16BE, 2000 * ch, 6)
            rc_t, used_t, made_t, out_t = t.raw_call("float", hm.to_internal(hm.S16BE, y).reshape(-1, ch), 2500)
            rc_p, used_p, made_p, out_p = p.fmt_call(y, hm.S16BE, out_fmt, 2500)
            assert rc_t == speexhip.ERR_ALLOC_FAILED and (rc_p, used_p, made_p) == (rc_t, used_t, made_t) and made_p > 0
            assert not out_t[:made_t].any()
            got = out_p.view(np.uint8)[: made_p * ch * hm.nbytes(out_fmt)]
            assert not got.any(), hm.name(out_fmt)      # every format's zero is all bytes 0: +0 for the half formats
            assert got.tobytes() == np.tile(hm.zero(out_fmt), made_p * ch).tobytes()
            check_tail(out_p, out_fmt, made_p, ch, hm.name(out_fmt))
            assert p.positions() == t.positions()
        finally:
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            p.close()
            t.close()


def test_channels_moved_apart_with_the_new_formats():
    """BAD_STATE with dither on, the state untouched; channel by channel without it"""
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    r.set_dither(dm.TRIANGULAR, 1, 10)
    rc, _, _, _ = r.channel_call("float", 0, np.zeros(300, np.float32), 400)
    assert rc == 0
    before = (r.positions(), r.history().tobytes())
    raw = storage(hm.S24BE, 1000 * ch, 2)
    for in_fmt, out_fmt in ((hm.S24BE, hm.S16BE), (hm.S24BE, hm.F16N)):
        rc, used, made, out = r.fmt_call(raw, in_fmt, out_fmt, 1200)
        assert rc == speexhip.ERR_BAD_STATE and (used, made) == (1000, 1200), hm.name(out_fmt)
        assert (out.view(np.uint8) == SENTINEL).all()
    assert r.get_dither() == (dm.TRIANGULAR, 1, 10)
    assert (r.positions(), r.history().tobytes()) == before
    assert r.set_dither(dm.NONE, 0, 0) == 0
    x = hm.to_internal(hm.S24BE, raw).reshape(-1, ch)
    for out_fmt in (hm.S16BE, hm.BF16N):
        t = speexhip.Resampler(ch, fi, fo, q)
        t.channel_call("float", 0, np.zeros(300, np.float32), 400)
        r2 = speexhip.Resampler(ch, fi, fo, q)
        r2.channel_call("float", 0, np.zeros(300, np.float32), 400)
        rc, used, made, out = r2.fmt_call(raw, hm.S24BE, out_fmt, 1200)
        assert rc == 0
        got = out.view(np.uint8).reshape(1200, ch, hm.nbytes(out_fmt))
        for c in range(ch):
            rc_c, used_c, made_c, out_c = t.channel_call("float", c, np.ascontiguousarray(x[:, c]), 1200)
            assert rc_c == 0
            assert got[:made_c, c].tobytes() == raw_bytes(out_fmt, hm.from_internal(out_fmt, out_c[:made_c])).tobytes(), c
            assert (got[made_c:, c] == SENTINEL).all(), c
        assert (used, made) == (used_c, made_c)      # (the call reports the last channel's lengths)
        assert r2.positions() == t.positions()
        r2.close()
        t.close()
    r.close()


def test_dither_leaves_half_float_output_as_it_is_and_advances_the_position():
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    frames = 2 * 4096 + 37
    cap = wcap(frames, fi, fo)
    raw = storage_of(sf.F32, frames * ch, 91)
    for o in hm.HALF:
        plain = speexhip.Resampler(*cfg)
        want, used_t = plain.process_fmt(raw, sf.F32, o, cap)
        for kind in dm.KINDS:
            for off in (None, 0, 2):   # host; device aligned (16 bytes per lane); one element off (element path)
                r = speexhip.Resampler(*cfg)
                assert r.set_dither(kind, SEED, START) == 0
                if off is None:
                    rc, used, made, out = r.fmt_call(raw, sf.F32, o, cap)
                    assert rc == 0
                    got = produced(out, o, made, ch)
                else:
                    used, made, got = device_call(r, sf.F32, raw, o, cap, ch, ch, 0, off, torch)
                    got = got.tobytes()
                assert got == raw_bytes(o, want).tobytes(), (hm.name(o), kind, off)
                assert r.get_dither() == (kind, SEED, START + made)
                same_state(r, plain, "dither on, half-float out")
                r.close()
        plain.close()


def test_formats_18_19_22_23_27_are_still_unknown():
    ch, fi, fo, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, fi, fo, q)
    raw = storage(hm.S16BE, 2000 * ch, 3)
    r.process_fmt(raw, hm.S16BE, hm.F16N, 2300)
    before = (r.positions(), r.history().tobytes())
    L = speexhip.lib()
    buf = np.zeros(2300 * ch * 4, np.uint8)
    for in_fmt, out_fmt in ((18, hm.F16N), (hm.S16BE, 19), (22, 23), (27, hm.S32BE), (hm.BF16N, 32)):
        il, ol = C.c_uint32(2000), C.c_uint32(2300)
        rc = L.speexhip_resampler_process_interleaved_fmt(r._h, in_fmt, C.c_void_p(raw.ctypes.data), C.byref(il), out_fmt,
                                                          C.c_void_p(buf.ctypes.data), C.byref(ol))
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
        rc = L.speexhip_resampler_process_interleaved_fmt_device(r._h, in_fmt, None, C.byref(il), out_fmt,
                                                                 C.c_void_p(buf.ctypes.data), C.byref(ol), None)
        assert rc == speexhip.ERR_INVALID_ARG and (il.value, ol.value) == (2000, 2300), (in_fmt, out_fmt)
    assert not buf.any()
    assert (r.positions(), r.history().tobytes()) == before
    r.close()


# ---- 8. host routes --------------------------------------------------------------------------------------------------------
def test_new_format_host_routes_give_the_device_calls_bytes():
    """pageable (small: the bounce buffers; large: the runtime's staged copy) and speexhip_block_acquire blocks on both
    sides, against the device-pointer call: one pair per new format"""
    import torch
    cfg = (2, 44100, 48000, 7)
    ch, fi, fo, q = cfg
    for in_fmt, out_fmt, frames in ((hm.S16BE, sf.F32N, 3000), (sf.S16, hm.F16N, 200000), (hm.BF16N, hm.S24BE, 3000),
                                    (hm.S24BE, hm.BF16N, 200000), (hm.F16N, hm.S32BE, 3000), (hm.S32BE, hm.S16BE, 200000)):
        st = storage(in_fmt, frames * ch, 60 + frames % 7 + in_fmt)
        raw = raw_bytes(in_fmt, st)
        cap = wcap(frames, fi, fo)
        rd = speexhip.Resampler(*cfg)
        used_d, made_d, want = device_call(rd, in_fmt, st, out_fmt, cap, ch, ch, 0, 0, torch)
        out_bytes = cap * ch * hm.nbytes(out_fmt)
        what = (hm.name(in_fmt), hm.name(out_fmt), frames)
        r = speexhip.Resampler(*cfg)
        got, used = r.process_fmt(st, in_fmt, out_fmt, cap)
        assert used == used_d and raw_bytes(out_fmt, got).tobytes() == want.tobytes(), what + ("pageable",)
        same_state(r, rd, "pageable")
        r.close()
        r = speexhip.Resampler(*cfg)
        with speexhip.PinnedBlock(raw.nbytes) as bin_, speexhip.PinnedBlock(out_bytes) as bout:
            a_in, a_out = bin_.array(np.uint8, (raw.nbytes,)), bout.array(np.uint8, (out_bytes,))
            a_in[:] = raw
            a_out[:] = SENTINEL
            il, ol = C.c_uint32(frames), C.c_uint32(cap)
            rc = speexhip.lib().speexhip_resampler_process_interleaved_fmt(
                r._h, in_fmt, C.c_void_p(a_in.ctypes.data), C.byref(il), out_fmt, C.c_void_p(a_out.ctypes.data), C.byref(ol))
            assert (rc, il.value, ol.value) == (0, used_d, made_d), what + ("blocks",)
            assert a_out[: want.nbytes].tobytes() == want.tobytes() and (a_out[want.nbytes:] == SENTINEL).all(), what + ("blocks",)
        same_state(r, rd, "blocks")
        r.close()
        rd.close()


# ---- 9. Node ---------------------------------------------------------------------------------------------------------------
NODE_NAME = {sf.S16: "s16le", sf.F32N: "f32le-normalized", hm.S16BE: "s16be", hm.S24BE: "s24be", hm.S32BE: "s32be",
             hm.F16N: "f16le-normalized", hm.BF16N: "bf16le-normalized"}


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_calls_with_the_new_formats_equal_the_python_results(tmp_path):
    """processChunkFormat, processChunkMix and processChunkSides on 's16be' and 'f16le-normalized' (and the other three
    names once each) against what this binding makes of the same stream cut into the same chunks"""
    chunks = [160, 4097, 1, 17, 3000]
    total = sum(chunks)
    manifest = []

    def case(name, call, ch, rates, in_fmt, out_fmt, in_mix=None, out_mix=None, planar_in=False, planar_out=False, dither=None):
        fi, fo = rates
        c_in = ch if in_mix is None else in_mix.shape[1]
        c_out = ch if out_mix is None else out_mix.shape[0]
        st = storage(in_fmt, total * c_in, 900 + len(manifest))
        raw = raw_bytes(in_fmt, st)
        r = speexhip.Resampler(ch, fi, fo, 7)
        if dither is not None:
            r.set_dither(dither, 12345, 7)
        got, at, room = [], 0, 0
        bi = hm.nbytes(in_fmt)
        for n in chunks:
            part = raw[at * c_in * bi: (at + n) * c_in * bi].view(hm.dtype(in_fmt))
            # index.js's capacity rule (processChunkFloat's on these frames: bytes of float32, grow-only)
            room = max(room, -(-(n * ch * 4 * fo) // fi))
            cap = room // ch // 4
            if call == "format":
                out, used = r.process_fmt(part, in_fmt, out_fmt, cap)
            else:
                out, used = r.process_mix(part, in_fmt, out_fmt, cap, in_mix, out_mix)
            got.append(raw_bytes(out_fmt, out).tobytes())
            at += n
        r.close()
        (tmp_path / (name + ".in")).write_bytes(raw.tobytes())
        (tmp_path / (name + ".want")).write_bytes(b"".join(got))
        manifest.append({"name": name, "call": call, "channels": ch, "inRate": fi, "outRate": fo, "quality": 7,
                         "inFormat": NODE_NAME[in_fmt], "outFormat": NODE_NAME[out_fmt], "inChannels": c_in, "outChannels": c_out,
                         "inMix": None if in_mix is None else in_mix.tolist(), "outMix": None if out_mix is None else out_mix.tolist(),
                         "planarIn": planar_in, "planarOut": planar_out, "chunks": chunks, "input": name + ".in",
                         "expected": name + ".want",
                         "dither": None if dither is None else {"kind": dm.KIND_NAMES[dither], "seed": "12345", "position": "7"}})

    case("format-s16be-f32n", "format", 1, (8000, 16000), hm.S16BE, sf.F32N)
    case("format-s16-f16n", "format", 2, (44100, 48000), sf.S16, hm.F16N)
    case("format-f16n-s16be-dither", "format", 2, (44100, 48000), hm.F16N, hm.S16BE, dither=dm.TRIANGULAR)
    case("format-s24be-bf16n", "format", 1, (8000, 16000), hm.S24BE, hm.BF16N)
    case("format-bf16n-s32be", "format", 1, (8000, 16000), hm.BF16N, hm.S32BE)
    case("mix-s16be-f16n", "mix", 1, (48000, 16000), hm.S16BE, hm.F16N, in_mix=cm.STEREO_TO_MONO)
    case("mix-f16n-s16be", "mix", 1, (8000, 16000), hm.F16N, hm.S16BE, out_mix=cm.MONO_TO_STEREO)
    case("sides-s16be-f16n-planes", "sides", 2, (44100, 48000), hm.S16BE, hm.F16N, planar_out=True)
    case("sides-f16n-planes-s16be-planes", "sides", 2, (44100, 48000), hm.F16N, hm.S16BE, planar_in=True, planar_out=True)
    case("sides-s16be-planes-f16n", "sides", 1, (48000, 16000), hm.S16BE, hm.F16N, in_mix=cm.STEREO_TO_MONO, planar_in=True)
    (tmp_path / "manifest.json").write_text(json.dumps(manifest))
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_halfbe.js")
    res = subprocess.run(["node", script, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "ALL HALFBE NODE TESTS PASSED" in res.stdout


# ---- 10. cost --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_half_float_batch_call_is_not_slower_than_casting_with_torch():
    """8 kHz -> 16 kHz mono q7, 32 streams x 2^20 frames, device-resident, s16 in.  Route A: the formatted call with F16N
    out.  Route B, what a caller did before in the same process on the same buffers: the F32N call, then
    out.to(torch.float16).  Equal bits first; then route A may be slower than route B by no more than route B's own
    run-to-run spread (max / min of five medians)."""
    import torch
    S, ch, fi, fo, q, T = 32, 1, 8000, 16000, 7, 1 << 20
    cap = wcap(T, fi, fo)
    x = torch.randint(-32768, 32768, (S, T, ch), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    a, b = speexhip.Batch(S, ch, fi, fo, q), speexhip.Batch(S, ch, fi, fo, q)
    out_a = torch.empty((S, cap, ch), dtype=torch.float16, device="cuda")
    out_b = torch.empty((S, cap, ch), dtype=torch.float32, device="cuda")

    def route_a():
        return a.process_fmt_device(sf.S16, x.data_ptr(), T * ch, T, hm.F16N, out_a.data_ptr(), cap * ch, cap, stream)

    def route_b():
        _, made = b.process_fmt_device(sf.S16, x.data_ptr(), T * ch, T, sf.F32N, out_b.data_ptr(), cap * ch, cap, stream)
        return out_b[:, : made[0]].to(torch.float16)

    _, made = route_a()
    want = route_b()
    torch.cuda.synchronize()
    assert torch.equal(out_a[:, : made[0]].view(torch.int16), want.view(torch.int16))

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
        route_a()
        route_b()
    theirs, mine = [], []
    for _ in range(5):  # interleaved in time, so that a clock change hits both
        theirs.append(median_ms(route_b))
        mine.append(median_ms(route_a))
    spread = max(theirs) / min(theirs)
    print("F16N out %.3f ms (medians %s), F32N + torch cast %.3f ms (medians %s), spread %.3f" % (
        statistics.median(mine), ["%.3f" % v for v in mine], statistics.median(theirs), ["%.3f" % v for v in theirs], spread))
    a.close()
    b.close()
    assert statistics.median(mine) <= statistics.median(theirs) * spread
