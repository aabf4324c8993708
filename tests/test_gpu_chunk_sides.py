"""The formatted chunks call (speexhip_resampler_process_chunks_sides / _fmt) on the GPU, as twin tests: one state runs
ONE chunks call, its twin the separate speexhip_resampler_process_sides calls, each output side beginning at the frames
already written.  They must agree on bytes (whole buffers, the sentinel beyond what was written included), per-chunk
counters, positions, history, magic_samples and dither position -- exactly in the default mode and in EXACT; in FAST and
FAST_F32, where the launch's shape may move a sample's last bit, int16 results within test_gpu_parity's +-1 LSB of the twin
with counters and state still equal.

The chunk lists are the smallest that can go wrong: 0, 1, 3, 5, 160 and 4097 frames (a whole 4096-sample tile and a ragged
tail; with packed S24 the chunk boundaries fall inside a 16-sample group), a NULL chunk, a capacity of 0, a capacity-bound
chunk that drops input (sized with speexhip_plan_call_ex before the GPU is touched), 40 chunks in one call."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import speexhip
from golden_util import ROOT

pytestmark = pytest.mark.gpu

U8, S16, S24, S32, F32, F32N = range(6)
ULAW, ALAW, F16N, BF16N, S16BE, S24BE, S32BE = 16, 17, 20, 21, 24, 25, 26
SENTINEL = 0xA5
NONE, RECT, TRI = speexhip.DITHER_NONE, speexhip.DITHER_RECTANGULAR, speexhip.DITHER_TRIANGULAR
# one configuration per kernel family (tests/test_gpu_planar.py), and telephony
CONFIGS = {"period": (2, 44100, 48000, 7), "slide": (2, 16000, 48000, 7), "slide64": (2, 24000, 48000, 10),
           "period64": (2, 44100, 48000, 10), "exact": (2, 47999, 48000, 4), "telephony": (1, 8000, 16000, 7)}
# (input format, output format, dither kind)
PAIRS = {"s16": (S16, S16, NONE), "f32": (F32, F32, NONE), "f32n": (F32N, F32N, NONE), "ulaw_f32n": (ULAW, F32N, NONE),
         "s24_s16_tri": (S24, S16, TRI), "s16be_bf16n": (S16BE, BF16N, NONE), "f32n_u8_rect": (F32N, U8, RECT)}
MODES = {"default": None, "exact": speexhip.MODE_EXACT}
FAST_MODES = {"fast": speexhip.MODE_FAST, "fast_f32": speexhip.MODE_FAST_F32}
DROP_FRAMES, DROP_CAP = 160, 7   # the capacity-bound chunk: every configuration here makes more than 7 frames of 160


def storage(fmt, samples, seed):
    """`samples` samples of format fmt as raw bytes: any bytes for the integer and companded formats, finite audio-sized
    values for the float ones"""
    rng = np.random.RandomState(seed)
    if fmt in (F32, F32N, F16N, BF16N):
        v = (rng.standard_normal(samples) * 6000.0).astype(np.float32)
        if fmt == F32:
            return v.view(np.uint8).copy()
        v = v / np.float32(32768.0)
        if fmt == F32N:
            return v.view(np.uint8).copy()
        if fmt == F16N:
            return v.astype(np.float16).view(np.uint8).copy()
        return (v.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()
    return rng.randint(0, 256, samples * speexhip.fmt_bytes(fmt)).astype(np.uint8)


def state_of(st):
    """everything a call leaves behind in a state"""
    return (st.positions(), st._lines().tobytes(), st.get_dither())


def addr(a):
    """the address of an array (an empty chunk is still a present one: any address that is not NULL)"""
    return a.ctypes.data or 1


class Shape:
    """The two sides of a call and its chunks.  chunks[i]: None (silence) or the chunk's bytes -- one array when the input
    side is interleaved (or mono), one per plane (separate allocations) when it is planar."""

    def __init__(self, st_channels, in_fmt, out_fmt, frames, caps, seed, in_planar=False, out_planar=False, in_mix=None,
                 out_mix=None, out_planes_apart=False, silent=()):
        self.in_fmt, self.out_fmt, self.frames, self.caps = in_fmt, out_fmt, list(frames), list(caps)
        self.in_mix = None if in_mix is None else np.ascontiguousarray(in_mix, np.float32)
        self.out_mix = None if out_mix is None else np.ascontiguousarray(out_mix, np.float32)
        self.n_in = st_channels if in_mix is None else self.in_mix.shape[1]
        self.n_out = st_channels if out_mix is None else self.out_mix.shape[0]
        self.in_planar = in_planar and self.n_in > 1
        self.out_planar = out_planar and self.n_out > 1
        self.out_planes_apart = out_planes_apart and self.out_planar
        self.per = self.n_in if self.in_planar else 1
        self.chunks = []
        for i, f in enumerate(self.frames):
            if i in silent:
                self.chunks.append(None)
            elif self.in_planar:
                self.chunks.append([storage(in_fmt, f, seed + 10 * i + c) for c in range(self.n_in)])
            else:
                self.chunks.append([storage(in_fmt, f * self.n_in, seed + 10 * i)])
        self.room = max(sum(self.caps), 1)
        self.bo = speexhip.fmt_bytes(out_fmt)

    def in_layout(self):
        return speexhip.LAYOUT_PLANAR if self.in_planar else speexhip.LAYOUT_INTERLEAVED

    def out_layout(self):
        return speexhip.LAYOUT_PLANAR if self.out_planar else speexhip.LAYOUT_INTERLEAVED

    def in_ptrs(self):
        ptrs = []
        for ch in self.chunks:
            ptrs += [None] * self.per if ch is None else [addr(p) for p in ch]
        return ptrs

    def new_out(self):
        """the output buffers, every byte SENTINEL: one block, or one array per plane"""
        if self.out_planes_apart:
            return [np.full(self.room * self.bo, SENTINEL, np.uint8) for _ in range(self.n_out)]
        if self.out_planar:
            return np.full((self.n_out, self.room * self.bo), SENTINEL, np.uint8)
        return np.full(self.room * self.n_out * self.bo, SENTINEL, np.uint8)

    def out_side(self, out, written, keep):
        """the output side that begins `written` frames into `out`"""
        if self.out_planes_apart:
            ptrs = (C.c_void_p * self.n_out)(*[p.ctypes.data + written * self.bo for p in out])
            keep.append(ptrs)
            return speexhip.make_side(self.out_fmt, self.n_out, self.out_layout(), self.out_mix, planes=ptrs)
        if self.out_planar:
            return speexhip.make_side(self.out_fmt, self.n_out, self.out_layout(), self.out_mix,
                                      data=out.ctypes.data + written * self.bo, plane_stride=self.room)
        return speexhip.make_side(self.out_fmt, self.n_out, self.out_layout(), self.out_mix,
                                  data=out.ctypes.data + written * self.n_out * self.bo)

    @staticmethod
    def bytes_of(out):
        return b"".join(p.tobytes() for p in out) if isinstance(out, list) else out.tobytes()


def chunks_call(st, sh, out=None):
    """ONE chunks call; (rc, consumed, produced, out)"""
    out = sh.new_out() if out is None else out
    keep = []
    a = speexhip.make_side(sh.in_fmt, sh.n_in, sh.in_layout(), sh.in_mix)
    b = sh.out_side(out, 0, keep)
    rc, used, made = st.process_chunks_sides(a, sh.in_ptrs(), sh.frames, b, sh.caps)
    return rc, used, made, out


def separate_calls(st, sh):
    """the separate process_sides calls, each output side behind the frames written; (codes, consumed, produced, out)"""
    out = sh.new_out()
    codes, used, made, written = [], [], [], 0
    L = speexhip.lib()
    for i, ch in enumerate(sh.chunks):
        keep = []
        if ch is None:
            a = speexhip.make_side(sh.in_fmt, sh.n_in, sh.in_layout(), sh.in_mix)
        elif sh.in_planar:
            ptrs = (C.c_void_p * sh.n_in)(*[addr(p) for p in ch])
            a = speexhip.make_side(sh.in_fmt, sh.n_in, sh.in_layout(), sh.in_mix, planes=ptrs)
        else:
            a = speexhip.make_side(sh.in_fmt, sh.n_in, sh.in_layout(), sh.in_mix, data=addr(ch[0]))
        b = sh.out_side(out, written, keep)
        il, ol = C.c_uint32(sh.frames[i]), C.c_uint32(sh.caps[i])
        codes.append(L.speexhip_resampler_process_sides(st._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol)))
        used.append(il.value)
        made.append(ol.value)
        written += ol.value
    return codes, used, made, out


def make_pair(key, mode, dither=NONE, seed=77, position=(1 << 32) - 900):
    pair = [speexhip.Resampler(*key, mode=mode) for _ in range(2)]
    for st in pair:
        if dither != NONE:
            assert st.set_dither(dither, seed, position) == 0
    return pair


def basic_list(key):
    """frames and capacities of the basic chunk list; index 6 is silent, 7 has capacity 0, 8 drops input"""
    ch, fi, fo, q = key
    frames = [0, 1, 3, 5, 160, 4097, 97, 50, DROP_FRAMES, 33, 160]
    caps = [f * fo // fi + 64 for f in frames]
    caps[7], caps[8] = 0, DROP_CAP
    return frames, caps


def assert_drop_chunk_drops(key, frames, caps, float_entry, index=8):
    """on the CPU, before the GPU is used: the capacity-bound chunk consumes fewer frames than it is given"""
    ch, fi, fo, q = key
    info, _ = speexhip.design_filter(fi, fo, q, want_table=False)
    last = frac = magic = 0
    for i, (f, cap) in enumerate(zip(frames, caps)):
        used, made, last, frac, magic = speexhip.plan_call_ex(info["num_rate"], info["den_rate"], f, cap, float_entry, 160, last,
                                                              frac, magic)
        if i == index:
            assert used < f and made == cap, (key, i, used, f, made, cap)
            return
    raise AssertionError("no chunk %d" % index)


def assert_twins_agree(st, tw, sh, tag, lsb=0):
    before = state_of(st)
    assert before == state_of(tw), tag
    rc, used, made, out = chunks_call(st, sh)
    codes, used_t, made_t, out_t = separate_calls(tw, sh)
    assert rc == (codes[-1] if codes else 0) and all(c == codes[-1] for c in codes), (tag, rc, codes)
    assert (used, made) == (used_t, made_t), (tag, used, used_t, made, made_t)
    if lsb == 0:
        assert Shape.bytes_of(out) == Shape.bytes_of(out_t), tag
    else:
        assert sh.out_fmt == S16 and not isinstance(out, list)
        diff = np.abs(out.reshape(-1).view(np.int16).astype(np.int32) - out_t.reshape(-1).view(np.int16).astype(np.int32))
        print(tag, "max |diff| vs the twin:", diff.max(), "LSB,", int((diff != 0).sum()), "of", diff.size, "samples differ")
        assert diff.max() <= lsb, (tag, diff.max())
    assert state_of(st) == state_of(tw), tag
    return used, made


# ---- 1. every kernel family, every format pair ------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_one_chunks_call_equals_the_separate_calls(config, pair):
    key = CONFIGS[config]
    in_fmt, out_fmt, dither = PAIRS[pair]
    frames, caps = basic_list(key)
    assert_drop_chunk_drops(key, frames, caps, float_entry=pair != "s16")
    for mode in sorted(MODES):
        st, tw = make_pair(key, MODES[mode], dither)
        try:
            for step in range(2):   # (the second call starts from a full history and a position inside the stream)
                sh = Shape(key[0], in_fmt, out_fmt, frames, caps, 1000 * step + 31, silent=(6,))
                used, made = assert_twins_agree(st, tw, sh, (config, pair, mode, step))
                assert used[8] < frames[8] and made[8] == DROP_CAP and made[7] == 0 and made[5] > 4000
        finally:
            st.close(), tw.close()


def test_the_identity_pairs_are_process_chunks_int_and_float():
    key = CONFIGS["period"]
    ch = key[0]
    frames, caps = basic_list(key)
    for fmt, dtype in ((S16, np.int16), (F32, np.float32), (F32N, np.float32)):
        st, tw = make_pair(key, None)
        try:
            sh = Shape(ch, fmt, fmt, frames, caps, 5, silent=(6,))
            rc, used, made, out = chunks_call(st, sh)
            chunks = [None if c is None else c[0].view(dtype).reshape(-1, ch) for c in sh.chunks]
            outs, used_t = tw.process_chunks(chunks, [(frames[i], caps[i]) if c is None else caps[i] for i, c in enumerate(chunks)],
                                             dtype=dtype)
            assert rc == 0 and used == used_t and made == [o.shape[0] for o in outs]
            assert out[: sum(made) * ch * sh.bo].tobytes() == b"".join(o.tobytes() for o in outs)
            assert not (out[sum(made) * ch * sh.bo:] != SENTINEL).any()
            assert state_of(st) == state_of(tw)
        finally:
            st.close(), tw.close()


# ---- 2. sides: planar, matrices ---------------------------------------------------------------------------------------
SIDES = {
    "planar_in_out": ("period", dict(in_planar=True, out_planar=True), S24, F32N, NONE),
    "planar_out_planes_apart": ("slide", dict(in_planar=True, out_planar=True, out_planes_apart=True), ULAW, S16, TRI),
    "planar_in_only": ("period64", dict(in_planar=True), F32N, S24BE, RECT),
    "planar_f32_both": ("period", dict(in_planar=True, out_planar=True), F32, F32, NONE),
    "stereo_to_mono_in_matrix": ("telephony", dict(in_mix=[[0.5, 0.5]]), S16, F32N, NONE),
    "mono_to_stereo_out_matrix": ("telephony", dict(out_mix=[[1.0], [-0.75]], out_planar=True), ALAW, S16, TRI),
    "both_matrices": ("period", dict(in_mix=[[1.0, -0.5, 0.25], [0.0, 0.5, -1.0]], out_mix=[[0.5, 0.5]]), U8, F16N, NONE),
}


@pytest.mark.parametrize("case", sorted(SIDES))
def test_planar_sides_and_matrices_equal_the_separate_calls(case):
    config, kw, in_fmt, out_fmt, dither = SIDES[case]
    key = CONFIGS[config]
    frames, caps = basic_list(key)
    assert_drop_chunk_drops(key, frames, caps, float_entry=True)
    for mode in sorted(MODES):
        st, tw = make_pair(key, MODES[mode], dither)
        try:
            for step in range(2):
                sh = Shape(key[0], in_fmt, out_fmt, frames, caps, 2000 * step + 7, silent=(6,), **kw)
                used, made = assert_twins_agree(st, tw, sh, (case, mode, step))
                assert used[8] < frames[8] and made[5] > 4000
        finally:
            st.close(), tw.close()


def test_forty_chunks_in_one_call():
    key = CONFIGS["slide"]
    ch, fi, fo, q = key
    frames = [(160, 1, 333, 7, 480)[i % 5] for i in range(40)]
    caps = [f * fo // fi + 64 for f in frames]
    caps[13] = 5      # (two chunks that drop input: three launch groups)
    caps[29] = 5
    assert_drop_chunk_drops(key, frames, caps, True, index=13)
    for in_fmt, out_fmt, dither in ((ULAW, F32N, NONE), (S24, S16, TRI)):
        st, tw = make_pair(key, None, dither)
        try:
            sh = Shape(ch, in_fmt, out_fmt, frames, caps, 99, silent=(3, 20))
            c0 = speexhip.chunk_counters()
            used, made = assert_twins_agree(st, tw, sh, ("forty", in_fmt))
            c1 = speexhip.chunk_counters()
            assert c1["fir_launches"] - c0["fir_launches"] == 3 and c1["own_calls"] == c0["own_calls"]
            assert used[13] < frames[13] and used[29] < frames[29]
        finally:
            st.close(), tw.close()


def test_the_thin_form_is_the_sides_form_on_interleaved_sides():
    key = CONFIGS["telephony"]
    frames, caps = basic_list(key)
    st, tw = make_pair(key, None)
    try:
        sh = Shape(1, ULAW, F32N, frames, caps, 3, silent=(6,))
        outs, used = st.process_chunks_fmt([None if c is None else c[0] for c in sh.chunks], ULAW, F32N,
                                           [(frames[i], caps[i]) if c is None else caps[i] for i, c in enumerate(sh.chunks)])
        rc, used_t, made_t, out_t = chunks_call(tw, sh)
        assert rc == 0 and used == used_t and [o.size for o in outs] == made_t
        assert b"".join(o.tobytes() for o in outs) == out_t[: sum(made_t) * 4].tobytes()
        assert state_of(st) == state_of(tw)
    finally:
        st.close(), tw.close()


# ---- 3. the opt-in modes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(FAST_MODES))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fast_modes_agree_with_the_twin_within_one_lsb(config, mode):
    key = CONFIGS[config]
    frames, caps = basic_list(key)
    for in_fmt, dither in ((S16, NONE), (S24, TRI)):
        st, tw = make_pair(key, FAST_MODES[mode], dither)
        try:
            for step in range(2):
                sh = Shape(key[0], in_fmt, S16, frames, caps, 3000 * step + 11, silent=(6,))
                assert_twins_agree(st, tw, sh, (config, mode, in_fmt, step), lsb=1)
        finally:
            st.close(), tw.close()


# ---- 4. rare states ---------------------------------------------------------------------------------------------------
def move_channels_apart(*states):
    x = (np.arange(600, dtype=np.int16).reshape(300, 2) * 37) % 9000
    for s in states:
        s.channel_call("int", 0, x[:300, 0], 400)
        s.channel_call("int", 1, x[:150, 1], 400)
        assert len(set(s.positions())) == 2


def test_a_state_whose_channels_stand_apart_runs_the_separate_calls():
    key = CONFIGS["period"]
    frames, caps = basic_list(key)
    for in_fmt, out_fmt, kw in ((S16, S16, {}), (ULAW, F32N, {}), (S24, S16, dict(in_planar=True, out_planar=True))):
        st, tw = make_pair(key, None)
        try:
            move_channels_apart(st, tw)
            sh = Shape(2, in_fmt, out_fmt, frames, caps, 41, silent=(6,), **kw)
            c0 = speexhip.chunk_counters()
            assert_twins_agree(st, tw, sh, ("apart", in_fmt, out_fmt))
            c1 = speexhip.chunk_counters()
            assert c1["own_calls"] - c0["own_calls"] == len(frames) and c1["fir_launches"] == c0["fir_launches"]
        finally:
            st.close(), tw.close()


def test_channels_apart_with_a_matrix_or_dither_is_bad_state_and_untouched():
    key = CONFIGS["period"]
    frames, caps = [160, 33], [300, 100]
    for kw, dither in ((dict(out_mix=[[0.5, 0.5]]), NONE), (dict(in_mix=[[1.0], [1.0]]), NONE), ({}, TRI)):
        st, tw = make_pair(key, None, dither)
        try:
            move_channels_apart(st, tw)
            before = state_of(st)
            sh = Shape(2, S16, U8, frames, caps, 1, **kw)
            rc, used, made, out = chunks_call(st, sh)
            assert rc == speexhip.ERR_BAD_STATE and (used, made) == (frames, caps), (kw, rc)
            assert state_of(st) == before and not (out != SENTINEL).any()
        finally:
            st.close(), tw.close()


def test_the_zero_fallback_runs_the_separate_calls():
    key = CONFIGS["period"]
    frames, caps = basic_list(key)
    L = speexhip.lib()
    for in_fmt, out_fmt, dither, kw in ((S16, S16, NONE, {}), (ULAW, U8, RECT, {}), (F32N, S24, NONE, dict(out_planar=True))):
        st, tw = make_pair(key, None, dither)
        try:
            for s in (st, tw):
                s.process(np.zeros((200, 2), np.int16) + 500, 400)
                L.speexhip_debug_fail_device_allocs(1)
                rc = s.set_rate(32000, 48000)
                L.speexhip_debug_fail_device_allocs(0)
                assert rc == speexhip.ERR_ALLOC_FAILED
            sh = Shape(2, in_fmt, out_fmt, frames, caps, 17, silent=(6,), **kw)
            before = state_of(st)
            rc, used, made, out = chunks_call(st, sh)
            codes, used_t, made_t, out_t = separate_calls(tw, sh)
            assert rc == speexhip.ERR_ALLOC_FAILED and codes == [speexhip.ERR_ALLOC_FAILED] * len(frames)
            assert (used, made) == (used_t, made_t) and sum(made) > 4000
            assert Shape.bytes_of(out) == Shape.bytes_of(out_t) and state_of(st) == state_of(tw) != before
        finally:
            L.speexhip_debug_fail_device_allocs(0)
            st.close(), tw.close()


# ---- 5. argument errors -----------------------------------------------------------------------------------------------
def test_an_argument_error_leaves_every_length_and_the_state_untouched():
    key = CONFIGS["period"]
    frames, caps = [160, 33, 4097, 5, 160, 97, 160], [300, 100, 4600, 70, 300, 200, 300]
    st, tw = make_pair(key, None, TRI)
    try:
        warm = Shape(2, S24, S16, [500], [700], 2)
        assert_twins_agree(st, tw, warm, "warm")
        before = state_of(st)

        def refused(sh, a, b, ptrs, want=speexhip.ERR_INVALID_ARG, out=None):
            rc, used, made = st.process_chunks_sides(a, ptrs, sh.frames, b, sh.caps)
            assert rc == want and (used, made) == (sh.frames, sh.caps), (rc, used, made)
            assert state_of(st) == before
            assert out is None or not (np.asarray(out) != SENTINEL).any()

        # a planar chunk in the middle of the list without its second plane
        sh = Shape(2, S24, S16, frames, caps, 3, in_planar=True)
        out, keep = sh.new_out(), []
        ptrs = sh.in_ptrs()
        ptrs[2 * 3 + 1] = None
        refused(sh, speexhip.make_side(S24, 2, sh.in_layout()), sh.out_side(out, 0, keep), ptrs, out=out)
        # an unknown format or layout, a short struct_size, a channel count that is not the state's, no output buffer
        sh = Shape(2, S24, S16, frames, caps, 3)
        for case in ("in_fmt", "out_fmt", "layout", "struct_size", "channels", "mix_channels", "no_out"):
            out = sh.new_out()
            a, b = speexhip.make_side(S24, 2), sh.out_side(out, 0, keep)
            if case == "in_fmt":
                a.fmt = 9
            elif case == "out_fmt":
                b.fmt = 99
            elif case == "layout":
                a.layout = 2
            elif case == "struct_size":
                a.struct_size = C.sizeof(speexhip.Side) - 8
            elif case == "channels":
                b.channels = 3
            elif case == "mix_channels":
                m = np.ones((2, 9), np.float32)
                a = speexhip.make_side(S24, 9, mix=m)
            else:
                b.data = None
            refused(sh, a, b, sh.in_ptrs(), out=out)
        # output planes that overlap in the frames the call writes
        sh = Shape(2, S24, S16, frames, caps, 3, out_planar=True)
        out = sh.new_out()
        b = speexhip.make_side(S16, 2, speexhip.LAYOUT_PLANAR, data=out.ctypes.data, plane_stride=1000)   # (> 5000 frames are made)
        refused(sh, speexhip.make_side(S24, 2), b, sh.in_ptrs(), want=speexhip.ERR_PTR_OVERLAP, out=out)
        ptrs_o = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data + 64)
        b = speexhip.make_side(S16, 2, speexhip.LAYOUT_PLANAR, planes=ptrs_o)
        refused(sh, speexhip.make_side(S24, 2), b, sh.in_ptrs(), want=speexhip.ERR_PTR_OVERLAP, out=out)
        # the thin form: an unknown format
        il, ol = (C.c_uint32 * 2)(10, 10), (C.c_uint32 * 2)(20, 20)
        flat = np.full(4096, SENTINEL, np.uint8)
        ptrs2 = (C.c_void_p * 2)(flat.ctypes.data, flat.ctypes.data)
        rc = speexhip.lib().speexhip_resampler_process_chunks_fmt(st._h, 2, 9, ptrs2, il, S16, C.c_void_p(flat.ctypes.data), ol)
        assert rc == speexhip.ERR_INVALID_ARG and list(il) == [10, 10] and list(ol) == [20, 20] and state_of(st) == before
        # ... and the state goes on as its twin's
        sh = Shape(2, S24, S16, frames, caps, 3)
        assert_twins_agree(st, tw, sh, "after errors")
    finally:
        st.close(), tw.close()


# ---- 6. launches ------------------------------------------------------------------------------------------------------
def test_twelve_chunks_cost_one_launch_and_one_pass_a_side():
    key = CONFIGS["telephony"]
    frames = [160, 320, 1, 4097, 160, 160, 33, 480, 160, 5, 160, 160]
    caps = [f * 2 + 64 for f in frames]
    for in_fmt, out_fmt, passes in ((ULAW, F32N, (1, 1)), (S16, S16, (0, 0)), (F32, S16, (0, 1))):
        st = speexhip.Resampler(*key)
        try:
            sh = Shape(1, in_fmt, out_fmt, frames, caps, 8)
            c0 = speexhip.chunk_counters()
            rc, used, made, out = chunks_call(st, sh)
            c1 = speexhip.chunk_counters()
            d = {k: c1[k] - c0[k] for k in c0}
            assert rc == 0 and used == frames, (rc, used)
            assert d["fir_launches"] == 1 and d["in_passes"] <= 1 and d["out_passes"] <= 1 and d["own_calls"] == 0, d
            assert (d["in_passes"], d["out_passes"]) == passes, d
            # the same call with one chunk that drops input: two launches
            caps2 = list(caps)
            caps2[4] = 9
            assert_drop_chunk_drops(key, frames, caps2, float_entry=(in_fmt, out_fmt) != (S16, S16), index=4)
            sh2 = Shape(1, in_fmt, out_fmt, frames, caps2, 9)
            rc, used, made, out = chunks_call(st, sh2)
            c2 = speexhip.chunk_counters()
            d = {k: c2[k] - c1[k] for k in c1}
            assert rc == 0 and used[4] < frames[4]
            assert d["fir_launches"] == 2 and d["in_passes"] <= 1 and d["out_passes"] <= 1 and d["own_calls"] == 0, d
        finally:
            st.close()


# ---- 7. pinned chunks -------------------------------------------------------------------------------------------------
def test_pinned_chunks_and_pageable_chunks_give_the_same_bytes():
    key = CONFIGS["period"]
    frames, caps = basic_list(key)
    st, tw = make_pair(key, None, TRI)
    blocks = []
    try:
        sh = Shape(2, S24, S16, frames, caps, 61, silent=(6,))
        pinned = Shape(2, S24, S16, frames, caps, 61, silent=(6,))
        for i, ch in enumerate(pinned.chunks):
            if ch is not None and ch[0].size:
                blk = speexhip.PinnedBlock(ch[0].size)
                blocks.append(blk)
                view = blk.array(np.uint8, (ch[0].size,))
                view[:] = ch[0]
                pinned.chunks[i] = [view]
        blk = speexhip.PinnedBlock(sh.new_out().size)
        blocks.append(blk)
        out_p = blk.array(np.uint8, (sh.new_out().size,))
        out_p[:] = SENTINEL
        rc_p, used_p, made_p, out_p = chunks_call(st, pinned, out=out_p)
        rc, used, made, out = chunks_call(tw, sh)
        assert rc_p == rc == 0 and (used_p, made_p) == (used, made)
        assert out_p.tobytes() == out.tobytes() and state_of(st) == state_of(tw)
    finally:
        for blk in blocks:
            blk.close()
        st.close(), tw.close()


# ---- 8. Node ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_transform_formats_and_formatted_chunks():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_chunk_formats.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "chunk formats: ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


# ---- 9. time ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_one_chunks_call_is_not_slower_than_sixteen_separate_calls():
    """16 chunks of 4096 frames, mono 8000 -> 16000 q7, mu-law in, f32n out: the median of one process_chunks_fmt call
    against the median of the 16 separate process_interleaved_fmt calls, 60 repetitions each, interleaved in one process so
    that both see the same box.  The coalesced call runs a strict subset of the separate calls' launches and waits: no
    margin."""
    key, n, frames, cap, reps = CONFIGS["telephony"], 16, 4096, 8192 + 64, 60
    st, tw = make_pair(key, None)
    L = speexhip.lib()
    try:
        raws = [storage(ULAW, frames, i) for i in range(n)]
        out = np.zeros(n * cap * 4, np.uint8)
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
        il, ol = (C.c_uint32 * n)(), (C.c_uint32 * n)()
        a, b = C.c_uint32(), C.c_uint32()

        def coalesced():
            for i in range(n):
                il[i], ol[i] = frames, cap
            assert L.speexhip_resampler_process_chunks_fmt(st._h, n, ULAW, ptrs, il, F32N, C.c_void_p(out.ctypes.data), ol) == 0

        def one_by_one():
            at = out.ctypes.data
            for i in range(n):
                a.value, b.value = frames, cap
                assert L.speexhip_resampler_process_interleaved_fmt(tw._h, ULAW, ptrs[i], C.byref(a), F32N, C.c_void_p(at), C.byref(b)) == 0
                at += b.value * 4

        t_one, t_apart = [], []
        for rep in range(reps + 10):
            t0 = time.perf_counter()
            coalesced()
            t1 = time.perf_counter()
            one_by_one()
            t2 = time.perf_counter()
            if rep >= 10:
                t_one.append(t1 - t0)
                t_apart.append(t2 - t1)
        one_us, apart_us = np.median(t_one) * 1e6, np.median(t_apart) * 1e6
        clock = speexhip.device_clock()
        print("16 x 4096-frame mu-law -> f32n: one chunks call %.1f us, 16 separate calls %.1f us (medians of %d), clock %.3f GHz"
              % (one_us, apart_us, reps, clock[0]))
        assert one_us <= apart_us, (one_us, apart_us)
    finally:
        st.close(), tw.close()
