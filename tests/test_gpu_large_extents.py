"""Calls that cross 2^31 and 2^32 samples, on the GPU (tests/large_extents.py has the tools and the reasoning).

Group 1, far apart: tiny calls whose streams or planes lie more than 2^32 elements apart (torch.empty, untouched but for
the few thousand frames of each stream): every output judged in full as test_gpu_exact_model._judge does, and sentinels
around each region the call may write AND around its 32-bit-wrapped alias.  The exact kernel is among them.

Group 2, long calls: one stream through process_device in the default mode, long enough for the sample index of the
input, of the output or of both to cross 2^31 and 2^32 inside ONE call, judged three ways --
  (A) every window of large_extents.windows() against the exact model (judge_window), after the window's input has been
      read back from the device and compared with the virtual input; counters and position against plan_call;
  (B) the whole output, on the device, equal to the same stream fed to a second state in pieces none of which reaches
      sample index 2^30 -- the regime the rest of the suite covers (the contract of
      test_fast_fixed_mode_bytes_do_not_depend_on_chunking_or_batch_size);
  (C) sentinels in front of and behind the output;
then one more call of 9001 frames on the same state, judged in full: it reads the history rolled from the far end.

Lengths from 2^31 frames are accepted (one long case and a silent host call have more).  What the 32-bit counts below a
call cannot hold -- the launchers' round-up sums, the slide kernels' k_shift + n_out -- one host rule refuses, within
2^16 + den frames of 2^32: the two tests before the last.

Run with -s for the windows judged, the windows a case cannot have, and the bytes each case needs."""
import time
from math import gcd

import numpy as np
import pytest

import dither_model as dm
import exact_model as em
import float_inputs as fi
import g711_model as gm
import large_extents as le
import oracle as orc
import sample_formats as sf
import speexhip
from test_gpu_exact_model import _expect_bits, _judge
from test_gpu_formats import storage_of

pytestmark = pytest.mark.gpu

FAR = (1 << 32) + 5           # elements between two streams (or planes): odd, so the second lies at every misalignment
FAR_ALIGNED = (1 << 32) + 8   # ... and with both planes on 16 bytes: the vector path
TAIL = 9001                   # frames of the call that follows a long one


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _ratio(i, o):
    g = gcd(i, o)
    return i // g, o // g


def _ragged_frames(model, q):
    """more than two tiles of the plan and not a multiple of one (the exact kernel: of its 256 outputs a workgroup)"""
    w = le.window_frames(model.num, model.den, q, model.channels)
    if speexhip.debug_plan(model.num, model.den, q, model.channels)["fast_path"] == 0:
        return (2 * 256 + 190) * model.num // model.den + 7
    tile = w // 3 if w > 8192 else 2048
    return (2 * tile + tile // 3) * model.num // model.den + 7


def _noise(kind, frames, ch, seed, taps):
    """a stream's samples: int16 noise, or real float data (float_inputs kind A), with a stretch of silence"""
    if kind == "float":
        return fi.make("A", frames, ch, seed, taps)
    return em.with_silence(orc.lcg_pcm(frames * ch, seed).reshape(frames, ch), taps)


# ---- group 1: far apart ----------------------------------------------------------------------------------------------
# (channels, in, out, quality, fast_path): a period case, a slide case, an fp64 case and the exact fallback
FAR_BATCHES = [(2, 44100, 48000, 7, 2), (2, 48000, 8000, 7, 3), (2, 44100, 48000, 10, 5), (2, 192000, 1000, 8, 0)]


@pytest.mark.parametrize("ch,i,o,q,fast_path", FAR_BATCHES)
def test_batch_streams_more_than_2_to_32_elements_apart(ch, i, o, q, fast_path):
    torch = _torch()
    model = em.Model(ch, i, o, q)
    S, F = 2, _ragged_frames(model, q)
    lens = [F, F - 997]
    cap = F * o // i + 64
    name = "%s, 2 streams %d elements apart" % ((ch, i, o, q), FAR)
    got, fed, want = {}, {}, {}
    for kind in ("int16", "float"):
        fl = kind == "float"
        dt, es = (torch.float32, 4) if fl else (torch.int16, 2)
        le.gate(torch, pytest, name + " " + kind, 2 * (FAR + cap * ch + 2 * le.SENTINELS) * es)
        d_in = out = b = None
        try:
            xs = [_noise(kind, lens[s], ch, 300 + 11 * s + q, model.taps) for s in range(S)]
            d_in = torch.empty(FAR + F * ch + 64, dtype=dt, device="cuda")
            for s in range(S):
                d_in[s * FAR: s * FAR + lens[s] * ch].copy_(torch.from_numpy(xs[s].reshape(-1)))
            out = le.Guarded(torch, dt, FAR + cap * ch, [(s * FAR, cap * ch) for s in range(S)])
            b = speexhip.Batch(S, ch, i, o, q)
            info = b.info()
            assert info["fast_path"] == fast_path, (name, info)
            bits = _expect_bits(info, model)
            used, made = b.process_device(d_in.data_ptr(), FAR, lens, out.ptr, FAR, cap, _stream(torch), fl)
            torch.cuda.synchronize()
            out.check(name + " " + kind, [m * ch for m in made])
            for s in range(S):
                ref = orc.Oracle(ch, i, o, q)
                w, wu = ref.process_float(xs[s], cap) if fl else ref.process(xs[s], cap)
                assert (used[s], made[s]) == (wu, w.shape[0]), (name, kind, s)
                got[kind, s] = out.at(s * FAR, made[s] * ch).cpu().numpy().reshape(made[s], ch)
                fed[kind, s], want[kind, s] = xs[s][:wu], w
                if fast_path == 0:      # the exact kernel: the oracle's bytes
                    assert np.array_equal(got[kind, s], w), (name, kind, s)
        finally:
            if b is not None:
                b.close()
            if out is not None:
                out.free()
            del d_in, out
            le.release(torch)
    for s in range(S):
        _judge("far apart", "%s stream %d" % (name, s), model, bits, fed["int16", s], got["int16", s], got["float", s],
               want["float", s], fedf=fed["float", s])


def _planar_call(torch, model, rates, q, kind, in_stride, out_stride, name):
    """one planar device call of a few thousand frames with the given plane strides -> (fed, got[frames, ch], oracle's)"""
    ch, fl = model.channels, kind == "float"
    dt, es = (torch.float32, 4) if fl else (torch.int16, 2)
    i, o = rates
    F = _ragged_frames(model, q)
    cap = F * o // i + 64
    le.gate(torch, pytest, name, ((ch - 1) * (in_stride + out_stride) + F + cap + 2 * le.SENTINELS) * es)
    d_in = out = r = None
    try:
        x = _noise(kind, F, ch, 500 + ch, model.taps)
        d_in = torch.empty((ch - 1) * in_stride + F + 64, dtype=dt, device="cuda")
        for c in range(ch):
            d_in[c * in_stride: c * in_stride + F].copy_(torch.from_numpy(np.ascontiguousarray(x[:, c])))
        out = le.Guarded(torch, dt, (ch - 1) * out_stride + cap, [(c * out_stride, cap) for c in range(ch)])
        r = speexhip.Resampler(ch, i, o, q)
        assert r.info()["fast_path"] == 2
        used, made = r.process_planar_device(d_in.data_ptr(), in_stride, F, out.ptr, out_stride, cap, _stream(torch), fl)
        torch.cuda.synchronize()
        out.check(name, [made] * ch)
        ref = orc.Oracle(ch, i, o, q)
        w, wu = ref.process_float(x, cap) if fl else ref.process(x, cap)
        assert (used, made) == (wu, w.shape[0]) and r.position() == ref.position(), name
        got = np.stack([out.at(c * out_stride, made).cpu().numpy() for c in range(ch)], axis=1)
        return x[:wu], got, w
    finally:
        if r is not None:
            r.close()
        if out is not None:
            out.free()
        del d_in, out
        le.release(torch)


@pytest.mark.parametrize("ch,stride", [(2, FAR_ALIGNED), (3, FAR)], ids=["2ch-vector-path", "3ch-element-path"])
def test_planes_more_than_2_to_32_elements_apart(ch, stride):
    """int16 and float planes `stride` elements apart on both sides -- except the float planes of the three-channel case,
    which take the far stride one side at a time (both at once: 2 x 2 x 2^32 x 4 bytes, 69 GiB)."""
    torch = _torch()
    i, o, q = 44100, 48000, 7
    model = em.Model(ch, i, o, q)
    near = 40000
    fed, got16, _ = _planar_call(torch, model, (i, o), q, "int16", stride, stride, "%d int16 planes %d apart" % (ch, stride))
    sides = [(stride, stride)] if ch == 2 else [(stride, near), (near, stride)]
    for in_stride, out_stride in sides:
        name = "%d float planes %d / %d apart" % (ch, in_stride, out_stride)
        fedf, gotf, wantf = _planar_call(torch, model, (i, o), q, "float", in_stride, out_stride, name)
        _judge("far apart", name, model, 32, fed, got16, gotf, wantf, fedf=fedf)


def test_sides_call_with_planes_more_than_2_to_32_samples_apart():
    """both sides planar, mu-law in, S16 out, 2 channels: the decode, the float call and the encoder of test_gpu_g711"""
    torch = _torch()
    ch, i, o, q = 2, 44100, 48000, 7
    model = em.Model(ch, i, o, q)
    F = _ragged_frames(model, q)
    cap = F * o // i + 64
    name = "sides, 2 mu-law planes %d samples apart -> 2 S16 planes %d apart" % (FAR, FAR_ALIGNED)
    le.gate(torch, pytest, name, FAR + 2 * FAR_ALIGNED + 4 * cap + F)
    d_in = out = r = t = None
    try:
        codes = le.VirtualInput(ch, "ulaw", [(F // 3, le.silence_frames(model.taps))]).frames(0, F)
        d_in = torch.empty(FAR + F + 64, dtype=torch.uint8, device="cuda")
        for c in range(ch):
            d_in[c * FAR: c * FAR + F].copy_(torch.from_numpy(np.ascontiguousarray(codes[:, c])))
        out = le.Guarded(torch, torch.int16, FAR_ALIGNED + cap, [(c * FAR_ALIGNED, cap) for c in range(ch)])
        r, t = speexhip.Resampler(ch, i, o, q), speexhip.Resampler(ch, i, o, q)
        a = speexhip.make_side(gm.ULAW, ch, speexhip.LAYOUT_PLANAR, None, d_in.data_ptr(), FAR)
        b = speexhip.make_side(sf.S16, ch, speexhip.LAYOUT_PLANAR, None, out.ptr, FAR_ALIGNED)
        used, made = r.process_sides_device(a, F, b, cap, _stream(torch))
        torch.cuda.synchronize()
        out.check(name, [made] * ch)
        y, used_t = t.process_float(gm.to_internal(gm.ULAW, codes.reshape(-1)).reshape(-1, ch), cap)
        assert (used, made) == (used_t, y.shape[0]) and r.position() == t.position()
        got = np.stack([out.at(c * FAR_ALIGNED, made).cpu().numpy() for c in range(ch)], axis=1)
        assert got.tobytes() == gm.from_internal(sf.S16, y).tobytes(), name
    finally:
        for s in (r, t):
            if s is not None:
                s.close()
        if out is not None:
            out.free()
        del d_in, out
        le.release(torch)


def test_formatted_batch_streams_more_than_2_to_32_samples_apart():
    """packed S24 in (3 bytes a sample: the second stream begins 12 GiB in), S16 out: test_gpu_formats' expectation, the
    float call on the converted input and the output conversion"""
    torch = _torch()
    S, ch, i, o, q = 2, 2, 44100, 48000, 7
    model = em.Model(ch, i, o, q)
    F = _ragged_frames(model, q)
    lens = [F, F - 611]
    cap = F * o // i + 64
    name = "formatted batch, 2 S24 streams %d samples apart -> S16" % FAR
    le.gate(torch, pytest, name, 3 * (FAR + F * ch) + 2 * (FAR + cap * ch))
    d_in = out = b = None
    try:
        raws = [storage_of(sf.S24, lens[s] * ch, 900 + s) for s in range(S)]
        d_in = torch.empty(3 * (FAR + F * ch) + 64, dtype=torch.uint8, device="cuda")
        for s in range(S):
            d_in[3 * s * FAR: 3 * s * FAR + raws[s].nbytes].copy_(torch.from_numpy(raws[s].view(np.uint8).copy()))
        out = le.Guarded(torch, torch.int16, FAR + cap * ch, [(s * FAR, cap * ch) for s in range(S)])
        b = speexhip.Batch(S, ch, i, o, q)
        used, made = b.process_fmt_device(sf.S24, d_in.data_ptr(), FAR, lens, sf.S16, out.ptr, FAR, cap, _stream(torch))
        torch.cuda.synchronize()
        out.check(name, [m * ch for m in made])
        for s in range(S):
            t = speexhip.Resampler(ch, i, o, q)
            y, used_t = t.process_float(sf.to_internal(sf.S24, raws[s]).reshape(-1, ch), cap)
            t.close()
            assert (used[s], made[s]) == (used_t, y.shape[0]), s
            got = out.at(s * FAR, made[s] * ch).cpu().numpy()
            assert got.tobytes() == sf.from_internal(sf.S16, y).tobytes(), (name, s)
    finally:
        if b is not None:
            b.close()
        if out is not None:
            out.free()
        del d_in, out
        le.release(torch)


# ---- group 2: long calls ---------------------------------------------------------------------------------------------
def _piece_frames(ch, num, den):
    """input frames of a piece in which neither side's sample index reaches 2^30"""
    most = ((1 << 30) - (1 << 16)) // ch
    return (most if den <= num else most * num // den) - 77


def _read_back(d_in, vin, f_lo, f_hi, what):
    """the device holds what the virtual input says, frames [f_lo, f_hi): torch's fill is not trusted"""
    ch = vin.channels
    assert d_in[f_lo * ch: f_hi * ch].cpu().numpy().tobytes() == vin.slice(f_lo * ch, (f_hi - f_lo) * ch).tobytes(), \
        what + ": the device input differs from the virtual input"


class _Long:
    """One long call, set up: the plan, the windows, the virtual input on the device, the output behind sentinels."""

    def __init__(self, torch, name, ch, i, o, q, kind, frames, fast_path, bits, extra_bytes=0, vin_kind=None):
        self.torch, self.name, self.kind, self.cfg = torch, name, kind, (ch, i, o, q)
        self.fl = kind == "float"
        self.model = model = em.Model(ch, i, o, q)
        num, den = model.num, model.den
        self.w = le.window_frames(num, den, q, ch)
        self.F = frames
        cap = frames * den // num + 64
        assert cap < 1 << 32
        self.plan = speexhip.plan_call_ex(num, den, frames, cap, self.fl, 160, 0, 0, 0)
        assert self.plan[0] == frames
        self.n_out, self.cap = self.plan[1], cap
        self.wins, self.absent, silent = le.windows(ch, num, den, model.taps, frames, self.n_out, self.w, self.fl)
        silent.append((frames + 3000, le.silence_frames(model.taps)))      # ... and one in the call that follows
        self.vin = le.VirtualInput(ch, vin_kind or kind, silent)
        self.dt, self.es = (torch.float32, 4) if self.fl else (torch.int16, 2)
        in_es = 1 if vin_kind == "ulaw" else self.es
        self.piece = _piece_frames(ch, num, den)
        self.piece_cap = self.piece * den // num + 64
        assert self.piece * ch < 1 << 30 and self.piece_cap * ch < 1 << 30
        self.need = le.need_bytes((frames + TAIL) * ch, in_es, cap * ch, self.es, self.piece_cap * ch, extra_bytes)
        le.gate(torch, pytest, name, self.need)
        for wname, why in self.absent:
            print("[large extents] %s: no window '%s': %s" % (name, wname, why))
        self.fast_path, self.bits = fast_path, bits
        self.d_in = self.out = self.scratch = None

    def allocate(self):
        torch, ch = self.torch, self.cfg[0]
        in_dt = torch.uint8 if self.vin.kind == "ulaw" else self.dt
        self.d_in = torch.empty((self.F + TAIL) * ch, dtype=in_dt, device="cuda")
        self.vin.fill(self.d_in)
        self.out = le.Guarded(torch, self.dt, self.cap * ch, [(0, self.cap * ch)])
        self.scratch = torch.empty(self.piece_cap * ch, dtype=self.dt, device="cuda")

    def state(self):
        r = speexhip.Resampler(*self.cfg)
        info = r.info()
        assert info["mode"] == speexhip.MODE_FAST_FIXED and info["fast_path"] == self.fast_path, (self.name, info)
        assert _expect_bits(info, self.model) == self.bits, (self.name, info)
        return r

    def judge_windows(self):
        """(A)"""
        ch, model = self.cfg[0], self.model
        for wname, k0, w in self.wins:
            t0 = time.time()
            seg, fed, pos0 = le.window_segment(model, self.vin, k0, w)
            _read_back(self.d_in, self.vin, max(0, pos0 - (model.taps - 1)), pos0 + fed.shape[0], wname)
            got = self.out.at(k0 * ch, w * ch).cpu().numpy().reshape(w, ch)
            fails = le.judge_window(model, self.bits, self.vin, k0, got)
            print("[large extents] %s: window '%s', outputs [%d, %d) from input frame %d (sample %d): %s (%.1f s)" % (
                self.name, wname, k0, k0 + w, pos0, pos0 * ch, "FAILED" if fails else "ok", time.time() - t0))
            assert not fails, (self.name, wname, fails)

    def pieces(self, call, check=None):
        """(B): the stream in pieces of at most self.piece frames through call(first frame, frames, scratch, capacity) ->
        (consumed, produced), each piece's output equal to its part of the long call's, on the device"""
        torch, ch = self.torch, self.cfg[0]
        at = done = n = 0
        while at < self.F:
            frames = min(self.piece, self.F - at)
            used, made = call(at, frames, self.scratch, self.piece_cap)
            torch.cuda.synchronize()
            assert used == frames, (self.name, at, used, frames)
            assert torch.equal(self.scratch[: made * ch], self.out.at(done * ch, made * ch)), \
                "%s: piece %d (input frames from %d, outputs from %d) differs from the long call" % (self.name, n, at, done)
            if check is not None:
                check(done, made)
            at, done, n = at + frames, done + made, n + 1
        assert done == self.n_out, (self.name, done, self.n_out)
        print("[large extents] %s: (B) %d pieces of <= %d frames equal the long call's %d outputs" % (self.name, n, self.piece, done))

    def free(self):
        if self.out is not None:
            self.out.free()
        self.d_in = self.out = self.scratch = None
        self.vin.release()
        le.release(self.torch)


def _long_interleaved(name, ch, i, o, q, kind, frames, fast_path, bits):
    torch = _torch()
    L = _Long(torch, name, ch, i, o, q, kind, frames, fast_path, bits, extra_bytes=TAIL * 4 * ch * 4)
    model, fl, es = L.model, L.fl, L.es
    num, den = model.num, model.den
    r = r2 = out2 = None
    try:
        L.allocate()
        r, r2 = L.state(), L.state()
        sp = _stream(torch)
        t0 = time.time()
        used, made = r.process_device(L.d_in.data_ptr(), L.F, L.out.ptr, L.cap, sp, fl)
        torch.cuda.synchronize()
        print("[large extents] %s: %d frames in, %d out, %.2f s" % (name, used, made, time.time() - t0))
        assert (used, made) + r.position() == L.plan[:4], (name, used, made, r.position(), L.plan)
        L.out.check(name, [made * ch])                                                   # (C)
        L.judge_windows()                                                                # (A)
        L.pieces(lambda at, n, scratch, cap: r2.process_device(L.d_in.data_ptr() + at * ch * es, n, scratch.data_ptr(), cap, sp, fl))
        assert r2.position() == r.position() and r2.history().tobytes() == r.history().tobytes(), name
        # the call that follows: the history was rolled from the far end of the long input
        cap2 = TAIL * den // num + 64
        want2 = speexhip.plan_call_ex(num, den, TAIL, cap2, fl, 160, L.plan[2], L.plan[3], 0)
        out2 = le.Guarded(torch, L.dt, cap2 * ch, [(0, cap2 * ch)])
        used2, made2 = r.process_device(L.d_in.data_ptr() + L.F * ch * es, TAIL, out2.ptr, cap2, sp, fl)
        torch.cuda.synchronize()
        assert (used2, made2) + r.position() == want2[:4] and used2 == TAIL, (name, used2, made2, want2)
        out2.check(name + ", the call that follows", [made2 * ch])
        _read_back(L.d_in, L.vin, L.F - (model.taps - 1), L.F + TAIL, "the call that follows")
        seg = model.segment(L.vin.frames(L.F - (model.taps - 1), model.taps - 1), (L.plan[2], L.plan[3]))
        fed = L.vin.frames(L.F, TAIL)
        got = out2.at(0, made2 * ch).cpu().numpy().reshape(made2, ch)
        truth, mag = seg.truth(fed, made2)
        fails = em.judge_float(seg, fed, got, truth, mag, L.bits, None)[0] if fl else em.hard_int16(seg, fed, got, truth, mag, L.bits)
        assert not fails, (name, "the call that follows", fails)
    finally:
        for s in (r, r2):
            if s is not None:
                s.close()
        if out2 is not None:
            out2.free()
        L.free()


def _frames(ch, i, o, q, in_mark=None, out_mark=None):
    num, den = _ratio(i, o)
    return le.frames_to_cross(ch, num, den, le.window_frames(num, den, q, ch), in_mark, out_mark)


M31, M32 = 1 << 31, 1 << 32
# (id, channels, in, out, quality, kind, frames (None: from the marks), input mark, output mark, fast_path, accumulate bits)
LONG_CASES = [
    ("period-fp32-pair-frames", 8, 44100, 48000, 5, "int16", None, M32, M32, 2, 32),
    ("period-fp32-float-window", 8, 44100, 48000, 5, "float", None, M32, M32, 2, 32),
    ("period-fp64", 8, 44100, 48000, 9, "int16", None, M32, M32, 5, 64),
    ("slide", 8, 48000, 8000, 7, "int16", None, M32, None, 3, 32),
    ("slide-upsampling", 8, 24000, 48000, 5, "int16", None, M31, M32, 3, 32),
    ("slide-fp64", 8, 96000, 8000, 10, "int16", None, M32, None, 4, 64),
    ("int16-window-loop", 9, 48000, 11025, 7, "int16", None, M32, None, 2, 32),
    ("mono-rows-frame-limit", 1, 44100, 48000, 7, "int16", 0x7FFFFFFF, None, None, 2, 32),
    # Lengths from 2^31 frames (include/speexhip_resampler.h, "Extents"): the device-pointer calls take them
    ("more-than-2-to-31-frames", 1, 48000, 8000, 5, "int16", M31 + (1 << 20), None, None, 3, 32),
]


@pytest.mark.parametrize("case", LONG_CASES, ids=[c[0] for c in LONG_CASES])
def test_one_long_call(case):
    name, ch, i, o, q, kind, frames, in_mark, out_mark, fast_path, bits = case
    frames = frames or _frames(ch, i, o, q, in_mark, out_mark)
    assert frames % 2 == 1 or frames == M31 + (1 << 20)
    _long_interleaved("%s %s %s" % (name, (ch, i, o, q), kind), ch, i, o, q, kind, frames, fast_path, bits)


def test_one_long_planar_call_equals_the_interleaved_call_transposed():
    """planar gather / scatter: int16 planes of the (8, 48000, 8000, 7) input, each 2^29+ frames long"""
    torch = _torch()
    ch, i, o, q = 8, 48000, 8000, 7
    name = "planar %s int16" % ((ch, i, o, q),)
    frames = _frames(ch, i, o, q, M32, None)
    stride = (frames + 15) // 8 * 8                      # planes on 16 bytes: the vector path
    L = _Long(torch, name, ch, i, o, q, "int16", frames, 3, 32, extra_bytes=ch * stride * 2 + frames // 6 * ch * 2 + (1 << 20))
    r = p = planes = outp = None
    try:
        L.allocate()
        sp = _stream(torch)
        planes = torch.empty(ch * stride, dtype=torch.int16, device="cuda")
        planes.view(ch, stride)[:, : frames].copy_(L.d_in[: frames * ch].view(frames, ch).t())
        ostride = (L.cap + 15) // 8 * 8
        outp = le.Guarded(torch, torch.int16, ch * ostride, [(c * ostride, L.cap) for c in range(ch)])
        r, p = L.state(), L.state()
        used, made = r.process_device(L.d_in.data_ptr(), frames, L.out.ptr, L.cap, sp, False)
        used_p, made_p = p.process_planar_device(planes.data_ptr(), stride, frames, outp.ptr, ostride, L.cap, sp, False)
        torch.cuda.synchronize()
        assert (used, made) == (used_p, made_p) == L.plan[:2] and p.position() == r.position() == L.plan[2:4], name
        outp.check(name, [made] * ch)
        L.out.check(name, [made * ch])
        L.judge_windows()                                # (the interleaved output, so that this test stands alone)
        got = outp.at(0, ch * ostride).view(ch, ostride)[:, :made]
        assert torch.equal(got, L.out.at(0, made * ch).view(made, ch).t()), name + ": the planes differ from the interleaved call's"
        assert p.history().tobytes() == r.history().tobytes(), name
        # the planes read back where the input crosses 2^32 samples -- plane c, frame f is interleaved sample f ch + c
        f = M32 // ch
        back = planes.view(ch, stride)[:, f - 64: f + 64].t().contiguous().cpu().numpy()
        assert back.tobytes() == L.vin.frames(f - 64, 128).tobytes()
    finally:
        for s in (r, p):
            if s is not None:
                s.close()
        if outp is not None:
            outp.free()
        del planes, outp
        L.free()


def test_one_long_formatted_call_with_dither():
    """mu-law in, S16 out with TPDF dither, (8, 48000, 8000, 7): the convert passes and the dither's 64-bit index.  (B)
    against pieces; the windows as test_gpu_g711 expects them -- decode, the float call, the encoder with the noise of
    the window's own position -- with the float call made in the same pieces on a twin."""
    torch = _torch()
    ch, i, o, q = 8, 48000, 8000, 7
    name = "formatted %s mu-law -> S16, TPDF" % ((ch, i, o, q),)
    frames = _frames(ch, i, o, q, M32, None)
    seed, start = 0xDEADBEEFCAFEF00D, (1 << 32) - 12345          # (the dither index crosses 2^32 x channels early on)
    num, den = _ratio(i, o)
    piece = _piece_frames(ch, num, den)
    # inside the library: the decoded input and the float output of the whole call; here: the twin's float output, and a
    # piece decoded with torch (an int64 index and the floats)
    extra = frames * ch * 4 + 2 * (frames // 6 + 64) * ch * 4 + piece * ch * 12
    L = _Long(torch, name, ch, i, o, q, "int16", frames, 3, 32, extra_bytes=extra, vin_kind="ulaw")
    r = r2 = t = y = lut = None
    try:
        L.allocate()
        sp = _stream(torch)
        r, r2, t = L.state(), L.state(), L.state()
        for s in (r, r2):
            assert s.set_dither(speexhip.DITHER_TRIANGULAR, seed, start) == 0
        used, made = r.process_fmt_device(gm.ULAW, L.d_in.data_ptr(), frames, sf.S16, L.out.ptr, L.cap, sp)
        torch.cuda.synchronize()
        # (the formatted call runs the float entry's plan)
        want = speexhip.plan_call_ex(num, den, frames, L.cap, True, 160, 0, 0, 0)
        assert (used, made) + r.position() == want[:4], (name, used, made, want)
        assert r.get_dither() == (speexhip.DITHER_TRIANGULAR, seed, start + made)
        assert made == L.n_out                                   # (the windows were laid out for that many outputs)
        L.out.check(name, [made * ch])
        y = torch.empty(made * ch, dtype=torch.float32, device="cuda")
        lut = torch.from_numpy(gm.to_internal(gm.ULAW, np.arange(256, dtype=np.uint8))).cuda()
        fscratch = torch.empty(L.piece_cap * ch, dtype=torch.float32, device="cuda")

        def call(at, n, scratch, cap):
            got = r2.process_fmt_device(gm.ULAW, L.d_in.data_ptr() + at * ch, n, sf.S16, scratch.data_ptr(), cap, sp)
            x = lut[L.d_in[at * ch: (at + n) * ch].long()]
            call.twin = t.process_device(x.data_ptr(), n, fscratch.data_ptr(), cap, sp, True)
            torch.cuda.synchronize()
            del x
            return got

        def keep(done, n_made):
            assert call.twin[1] == n_made
            y[done * ch: (done + n_made) * ch].copy_(fscratch[: n_made * ch])

        L.pieces(call, keep)
        assert r2.get_dither() == r.get_dither() and r2.history().tobytes() == r.history().tobytes() == t.history().tobytes()
        for wname, k0, w in L.wins:
            pos0 = k0 * num // den
            _read_back(L.d_in, L.vin, max(0, pos0 - (L.model.taps - 1)), pos0 + w * num // den + 1, wname)
            got = L.out.at(k0 * ch, w * ch).cpu().numpy()
            yw = y[k0 * ch: (k0 + w) * ch].cpu().numpy()
            expect = dm.from_internal(sf.S16, yw, dm.TRIANGULAR, seed, start + k0, ch)
            assert expect.tobytes() != sf.from_internal(sf.S16, yw).tobytes()
            print("[large extents] %s: window '%s', outputs [%d, %d), dither index from %d" % (name, wname, k0, k0 + w, (start + k0) * ch))
            assert got.tobytes() == expect.tobytes(), (name, wname)
    finally:
        for s in (r, r2, t):
            if s is not None:
                s.close()
        del y, lut
        L.free()


# ---- what the 32-bit counts below a call cannot hold -----------------------------------------------------------------
# Found by reading, beyond what real input in 45 GiB can reach: the launchers round a frame or period count up to whole
# tiles in 32 bits (count + tile - 1: the exact kernel's 256 outputs, the planar passes' 2048 frames, the period and slide
# launchers' periods when den = 1), and the slide kernels end a call at k_shift + n_out in 32 bits.  One host rule
# (engine.h, Batch::lengths_fit): a call's in_len and the outputs it can make stay kExtentSlack + den below 2^32, or the
# call returns OVERFLOW before it touches anything.
SLACK = 1 << 16     # Batch::kExtentSlack


def _most(den):
    return 0xFFFFFFFF - SLACK - den


def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError) as e:
        fn(*args, **kw)
    assert str(e.value) == speexhip.strerror(speexhip.ERR_OVERFLOW), e.value


@pytest.mark.parametrize("mode", [None, speexhip.MODE_EXACT], ids=["default", "exact"])
def test_an_input_length_the_launchers_cannot_round_up_is_refused(mode):
    """As the issue words it: a silent (NULL) input and a capacity of 16, so nothing large runs.  Every entry point refuses
    in_len beyond the rule with OVERFLOW and leaves positions, history, dither position and the output alone; the
    largest in_len the rule admits runs, and makes its 16 outputs."""
    torch = _torch()
    sp = _stream(torch)
    for ch in (1, 2):
        i, o, q = 48000, 8000, 5
        most = _most(1)
        r = speexhip.Resampler(ch, i, o, q, mode=mode)
        out = None
        try:
            r.process(orc.lcg_pcm(700 * ch, 9).reshape(700, ch), 200)       # a history that is not silence
            assert r.set_dither(speexhip.DITHER_TRIANGULAR, 7, 100) == 0
            before = (r.positions(), r.history().tobytes(), r.get_dither())
            out = le.Guarded(torch, torch.int16, 4096, [(0, 4096)])
            for in_len in (most + 1, 0xFFFFFFFF):
                _refused(r.process_device, 0, in_len, out.ptr, 16, sp, False)
                _refused(r.process_device, 0, in_len, out.ptr, 16, sp, True)
                _refused(r.process_planar_device, 0, 1 << 33, in_len, out.ptr, 64, 16, sp, False)
                _refused(r.process_fmt_device, gm.ULAW, 0, in_len, sf.S16, out.ptr, 16, sp)
                _refused(r.process, None, 16, null_frames=in_len)
                _refused(r.process_float, None, 16, null_frames=in_len)
                _refused(r.process_planar, None, 16, False, in_len)
                _refused(r.process_fmt, None, gm.ULAW, sf.S16, 16, in_len)
                torch.cuda.synchronize()
                assert (r.positions(), r.history().tobytes(), r.get_dither()) == before and out.untouched(0, 4096), (ch, in_len)
            want = speexhip.plan_call_ex(6, 1, most, 16, False, 160, *r.positions()[0])
            used, made = r.process_device(0, most, out.ptr, 16, sp, False)
            torch.cuda.synchronize()
            assert (used, made) + r.position() == want[:4] and made == 16, (used, made, want)
            out.check("in_len %d" % most, [16 * ch])
            assert out.at(0, 16 * ch).any().item()         # (the history's tail rings into the silence)
        finally:
            r.close()
            if out is not None:
                out.free()
            del out
            le.release(torch)


def test_an_output_count_the_kernels_cannot_hold_is_refused_and_the_largest_that_fits_runs():
    """The quantity is a count of OUTPUTS, so this test cannot keep to the issue's capacity of 16: the refused calls name a
    capacity at the limit (and run nothing), and the accepting side runs 2^32 - 65538 mono outputs, 8 GiB, from phase
    index 1 of a 1:2 stream through the slide kernel -- silence in, an output buffer with the full room either way."""
    torch = _torch()
    ch, i, o, q = 1, 24000, 48000, 5
    name = "output count at the limit %s" % ((ch, i, o, q),)
    in_len, most = M31 + 64, _most(2)
    le.gate(torch, pytest, name, (0xFFFFFFFF + 2 * le.SENTINELS) * 2 + (1 << 32))
    out = r = e = None
    try:
        r, e = speexhip.Resampler(ch, i, o, q), speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
        assert r.info()["fast_path"] == 3
        y, used = r.process(orc.lcg_pcm(3, 5).reshape(3, 1), 5)        # five outputs of a 1:2 stream: the next has phase 1
        assert y.shape[0] == 5 and r.position()[1] == 1, (used, y.shape, r.position())
        before = (r.positions(), r.history().tobytes(), e.positions(), e.history().tobytes())
        out = le.Guarded(torch, torch.int16, 0xFFFFFFFF, [(0, 0xFFFFFFFF)])
        sp = _stream(torch)
        for cap in (most + 1, 0xFFFFFFFF):
            assert speexhip.plan_call_ex(1, 2, in_len, cap, False, 160, r.position()[0], 1, 0)[1] == cap
            for s in (r, e):        # (the exact kernel's launcher at phase 0: 2^32 - 1 outputs rounded up to no block at all)
                _refused(s.process_device, 0, in_len, out.ptr, cap, sp, False)
                _refused(s.process, None, cap, null_frames=in_len)
        torch.cuda.synchronize()
        assert (r.positions(), r.history().tobytes(), e.positions(), e.history().tobytes()) == before, name
        assert out.untouched(0, 0xFFFFFFFF), name
        # a capacity at the limit that the input cannot fill is no reason to refuse
        want = speexhip.plan_call_ex(1, 2, 100, 0xFFFFFFFF, False, 160, 0, 0, 0)
        assert e.process_device(0, 100, out.ptr, 0xFFFFFFFF, sp, False) == want[:2]
        # the largest count that fits, from phase index 1
        want = speexhip.plan_call_ex(1, 2, in_len, most, False, 160, r.position()[0], 1, 0)
        used, made = r.process_device(0, in_len, out.ptr, most, sp)
        torch.cuda.synchronize()
        assert (used, made) + r.position() == want[:4] and made == most, (used, made, want)
        out.check(name, [made])
        # silence behind three frames of history: zeros from the filter's length on, to the last output
        taps = r.info()["filt_len"]
        for lo in (4 * taps, M31 - 4096, made - 8192):
            assert not out.at(lo, 8192).any().item(), (name, lo)
        print("[large extents] %s: OVERFLOW from %d outputs on, %d outputs run from phase index 1" % (name, most + 1, made))
    finally:
        for s in (r, e):
            if s is not None:
                s.close()
        if out is not None:
            out.free()
        del out
        le.release(torch)


# ---- lengths from 2^31 frames on a host call --------------------------------------------------------------------------
def test_a_silent_host_call_of_more_than_2_to_31_frames():
    """The host-buffer calls take such lengths too (include/speexhip_resampler.h, "Extents"; their piecewise route,
    whose positions are int32, is entered below 2^30 frames only).  Silence and a capacity of 16: nothing large runs."""
    for fl in (False, True):
        r = speexhip.Resampler(1, 48000, 8000, 5)
        try:
            want = speexhip.plan_call_ex(6, 1, M31 + 5, 16, fl, 160, 0, 0, 0)
            y, used = (r.process_float if fl else r.process)(None, 16, null_frames=M31 + 5)
            assert (used, y.shape[0]) + r.position() == want[:4] and not y.any(), (fl, used, y.shape, want)
        finally:
            r.close()
