"""Every host-buffer entry point on every route its buffers can take (csrc/host_transfer.h): the call on one state
against the device-pointer form of the same call on a twin state.  A host call is the device call between two
transfers, so every comparison is equality: the produced bytes, the counters, the return code, the history, every
channel's position and the dither position; behind the produced frames the caller's buffer keeps its sentinel fill.

The sizes are the smallest that reach each route with stereo s16 at quality 3: 64 frames (bounce / bounce), 1:8
up-sampling of 26 000 frames (staged in, copied out), 8:1 down-sampling of 205 000 frames (copied in, staged out),
44.1k -> 48k of 205 000 frames (copied both ways); blocks of the library on either side and on both (in place);
caller-pinned memory of exactly 256 KB (in place) and of one byte less (not).  Plus a present but empty input,
silence (a null input), capacity 0 and a state whose channels a per-channel call moved apart."""
import ctypes as C

import numpy as np
import pytest
import torch

import speexhip
from speexhip import (ERR_BAD_STATE, ERR_INVALID_ARG, ERR_PTR_OVERLAP, FMT_S16, FMT_S32, FMT_U8, LAYOUT_INTERLEAVED,
                      LAYOUT_PLANAR, make_side)

pytestmark = pytest.mark.gpu

CH, Q, SENT = 2, 3, 0xA5
MIX_IN = np.array([[1.0], [0.5]], np.float32)  # a mono side feeding the two channels

# name -> (in_rate, out_rate, frames)
SIZES = {"bounce": (44100, 48000, 64), "staged_copy": (8000, 64000, 26000), "copy_staged": (64000, 8000, 205000),
         "copy_copy": (44100, 48000, 205000)}


def cap_for(fi, fo, frames):
    return frames * fo // fi + 64


def u32(v):
    return C.c_uint32(int(v))


class Mem:
    """the host buffers of one case: pageable, blocks of the library on the named sides, or pinned by the caller"""

    def __init__(self, kind):
        self.kind, self.blocks, self.keep = kind, [], []

    def get(self, nbytes, side):
        n = max(int(nbytes), 1)
        if self.kind in ("block_both", "block_" + side):
            b = speexhip.PinnedBlock(n)
            self.blocks.append(b)
            return b.array(np.uint8, (n,))
        if self.kind == "pinned":
            t = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            self.keep.append(t)
            return t.numpy()
        a = np.empty(n, np.uint8)
        self.keep.append(a)  # (the calls get addresses: the arrays live as long as the case)
        return a

    def close(self):
        for b in self.blocks:
            b.close()


def state_of(r):
    torch.cuda.synchronize()
    return r.positions(), r._lines().tobytes(), r.get_dither()


class Entry:
    """One entry point.  in_parts(x): the call's input as storage arrays, one per buffer (x: (frames, CH) int16);
    out_frame_bytes: bytes of one frame in each output buffer; host / dev: the call itself on addresses, returning
    (rc, consumed, produced) -- lists where the entry makes several calls."""
    name = ""
    float_io = False
    mode = None
    n_out = 1
    out_frame_bytes = 2 * CH
    splits = True  # serves a state whose channels stand apart (else: BAD_STATE)
    sentinel = True
    ch = CH  # channels of the state

    def in_parts(self, x):
        return [x]

    def setup(self, r):
        pass


def _host_il(fn_name, ctype):
    def call(self, r, ins, n, outs, cap):
        il, ol = u32(n), u32(cap)
        fn = getattr(speexhip.lib(), fn_name)
        rc = fn(r._h, C.cast(ins[0], C.POINTER(ctype)), C.byref(il), C.cast(outs[0], C.POINTER(ctype)), C.byref(ol))
        return rc, il.value, ol.value
    return call


def _dev_il(fn_name):
    def call(self, t, d_in, n, d_out, cap, in_pitch, out_pitch):
        il, ol = u32(n), u32(cap)
        rc = getattr(speexhip.lib(), fn_name)(t._h, C.c_void_p(d_in), C.byref(il), C.c_void_p(d_out), C.byref(ol), None)
        return rc, il.value, ol.value
    return call


class Int(Entry):
    name = "int"
    host = _host_il("speexhip_resampler_process_interleaved_int", C.c_int16)
    dev = _dev_il("speexhip_resampler_process_interleaved_int_device")


class Float(Entry):
    name, float_io, out_frame_bytes = "float", True, 4 * CH
    host = _host_il("speexhip_resampler_process_interleaved_float", C.c_float)
    dev = _dev_il("speexhip_resampler_process_interleaved_float_device")

    def in_parts(self, x):
        return [x.astype(np.float32)]


class Take(Int):
    """the result in a block of the library: nothing to fill with a sentinel, and a split state's unwritten samples are
    whatever the block held"""
    name, sentinel = "take", False

    def host(self, r, ins, n, outs, cap):
        il, ol, blk = u32(n), u32(cap), C.POINTER(C.c_int16)()
        rc = speexhip.lib().speexhip_resampler_process_interleaved_int_take(r._h, C.c_void_p(ins[0]), C.byref(il), C.byref(ol),
                                                                            C.byref(blk))
        if blk:
            # (two frames more than reported: on a split state another channel may have written a frame more than the
            #  last one; the block has that room behind its samples)
            C.memmove(outs[0], blk, min(cap, ol.value + 2) * 2 * CH)
            speexhip.lib().speexhip_block_release(C.cast(blk, C.c_void_p))
        return rc, il.value, ol.value


class Chunks(Int):
    """three calls as one: the twin makes the three device calls one after the other"""
    name = "chunks"

    @staticmethod
    def cuts(n):
        return [n // 3, n // 3, n - 2 * (n // 3)]

    def host(self, r, ins, n, outs, cap):
        cuts = self.cuts(n)
        ptrs = (C.c_void_p * 3)()
        off = 0
        for i, k in enumerate(cuts):
            ptrs[i] = ins[0] + off * 2 * CH if ins[0] else None
            off += k
        il, ol = (C.c_uint32 * 3)(*cuts), (C.c_uint32 * 3)(cap, cap, cap)
        rc = speexhip.lib().speexhip_resampler_process_chunks_int(r._h, 3, ptrs, il, C.c_void_p(outs[0]), ol)
        return rc, list(il), list(ol)

    def dev(self, t, d_in, n, d_out, cap, in_pitch, out_pitch):
        used, made, rc, off = [], [], 0, 0
        for k in self.cuts(n):
            il, ol = u32(k), u32(cap)
            rc = speexhip.lib().speexhip_resampler_process_interleaved_int_device(
                t._h, C.c_void_p(d_in + off * 2 * CH if d_in else None), C.byref(il), C.c_void_p(d_out + sum(made) * 2 * CH),
                C.byref(ol), None)
            off += k
            used.append(il.value)
            made.append(ol.value)
        return rc, used, made


class Channel(Int):
    """the per-channel call on every channel in turn, strides = the channel count: together the interleaved call, which
    reports its last channel's counters.  It runs the exact kernel, so both states are in the exact mode.  per_channel:
    every channel's own (rc, consumed, produced) -- the same for all unless the channels stand apart."""
    name, mode = "channel", speexhip.MODE_EXACT

    def host(self, r, ins, n, outs, cap):
        L = speexhip.lib()
        L.speexhip_resampler_set_input_stride(r._h, CH)
        L.speexhip_resampler_set_output_stride(r._h, CH)
        res = []
        for c in range(CH):
            il, ol = u32(n), u32(cap)
            rc = L.speexhip_resampler_process_int(r._h, c, C.cast(ins[0] + 2 * c if ins[0] else None, C.POINTER(C.c_int16)),
                                                  C.byref(il), C.cast(outs[0] + 2 * c, C.POINTER(C.c_int16)), C.byref(ol))
            res.append((rc, il.value, ol.value))
        self.per_channel = res
        return res[-1]


class Planar(Entry):
    name, n_out, out_frame_bytes, ctype = "planar_int", CH, 2, C.c_int16
    fn = "speexhip_resampler_process_planar_int"

    def in_parts(self, x):
        x = x.astype(np.float32) if self.float_io else x
        return [np.ascontiguousarray(x[:, c]) for c in range(CH)]

    def host(self, r, ins, n, outs, cap):
        il, ol = u32(n), u32(cap)
        a = (C.c_void_p * CH)(*ins) if ins[0] else None
        rc = getattr(speexhip.lib(), self.fn)(r._h, a, C.byref(il), (C.c_void_p * CH)(*outs), C.byref(ol))
        return rc, il.value, ol.value

    def dev(self, t, d_in, n, d_out, cap, in_pitch, out_pitch):
        il, ol = u32(n), u32(cap)
        rc = getattr(speexhip.lib(), self.fn + "_device")(t._h, C.c_void_p(d_in), in_pitch, C.byref(il), C.c_void_p(d_out),
                                                           out_pitch, C.byref(ol), None)
        return rc, il.value, ol.value


class PlanarFloat(Planar):
    name, float_io, out_frame_bytes = "planar_float", True, 4
    fn = "speexhip_resampler_process_planar_float"


class Sides(Entry):
    """the sides call: layouts, formats and matrices per side.  On the host a planar side is given as separate planes."""
    in_fmt, out_fmt, in_planar, out_planar, in_mix, in_channels, mono_plane = FMT_S16, FMT_S16, False, False, None, CH, False

    def __init__(self, name, **kw):
        self.name = name
        for k, v in kw.items():
            setattr(self, k, v)
        self.n_out = self.ch if self.out_planar else 1
        self.out_frame_bytes = speexhip.fmt_bytes(self.out_fmt) * (1 if self.out_planar else self.ch)
        self.splits = self.in_mix is None

    def in_parts(self, x):
        if self.in_fmt == FMT_U8:
            x = ((x >> 8) + 128).astype(np.uint8)
        if self.in_channels == 1:
            return [np.ascontiguousarray(x[:, 0])]
        return [np.ascontiguousarray(x[:, c]) for c in range(CH)] if self.in_planar else [x]

    def _side(self, fmt, channels, planar, mix, ptrs, pitch, host):
        if ptrs[0] is None:
            return make_side(fmt, channels, LAYOUT_PLANAR if planar else LAYOUT_INTERLEAVED, mix)
        if host and (planar or self.mono_plane and channels == 1):
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            self._keep.append(arr)
            return make_side(fmt, channels, LAYOUT_PLANAR, mix, planes=arr)
        return make_side(fmt, channels, LAYOUT_PLANAR if planar else LAYOUT_INTERLEAVED, mix, data=ptrs[0], plane_stride=pitch)

    def _call(self, fn, h, ins, n, outs, cap, in_pitch, out_pitch, host, *stream):
        self._keep = []
        a = self._side(self.in_fmt, self.in_channels, self.in_planar, self.in_mix, ins, in_pitch, host)
        b = self._side(self.out_fmt, self.ch, self.out_planar, None, outs, out_pitch, host)
        il, ol = u32(n), u32(cap)
        rc = fn(h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol), *stream)
        return rc, il.value, ol.value

    def host(self, r, ins, n, outs, cap):
        return self._call(speexhip.lib().speexhip_resampler_process_sides, r._h, ins, n, outs, cap, 0, 0, True)

    def dev(self, t, d_in, n, d_out, cap, in_pitch, out_pitch):
        return self._call(speexhip.lib().speexhip_resampler_process_sides_device, t._h, [d_in], n, [d_out], cap, in_pitch,
                          out_pitch, False, None)


class Fmt(Sides):
    def host(self, r, ins, n, outs, cap):
        il, ol = u32(n), u32(cap)
        rc = speexhip.lib().speexhip_resampler_process_interleaved_fmt(r._h, self.in_fmt, C.c_void_p(ins[0]), C.byref(il),
                                                                       self.out_fmt, C.c_void_p(outs[0]), C.byref(ol))
        return rc, il.value, ol.value


class Mix(Sides):
    def host(self, r, ins, n, outs, cap):
        il, ol = u32(n), u32(cap)
        rc = speexhip.lib().speexhip_resampler_process_interleaved_mix(
            r._h, self.in_fmt, 1, C.c_void_p(MIX_IN.ctypes.data), C.c_void_p(ins[0]), C.byref(il), self.out_fmt, CH, None,
            C.c_void_p(outs[0]), C.byref(ol))
        return rc, il.value, ol.value


ENTRIES = [Int(), Float(), Take(), Chunks(), Channel(), Planar(), PlanarFloat(),
           Fmt("fmt", out_fmt=FMT_S32),
           Mix("mix", in_mix=MIX_IN, in_channels=1),
           Sides("sides_planar_in", in_planar=True),
           Sides("sides_planar_out", out_planar=True),
           Sides("sides_planar_both", in_planar=True, out_planar=True, out_fmt=FMT_S32),
           Sides("sides_mono_plane", in_mix=MIX_IN, in_channels=1, mono_plane=True)]
BY_NAME = {e.name: e for e in ENTRIES}

_inputs = {}


def samples(frames):
    """(frames, CH) int16, made once per length and left as it is"""
    if frames not in _inputs:
        x = np.random.RandomState(frames + 1).randint(-20000, 20000, (max(frames, 1), CH)).astype(np.int16)
        x.setflags(write=False)
        _inputs[frames] = x
    return _inputs[frames][:frames]


def run_pair(entry, rates, frames, cap, kind="pageable", present=True, split=False, expect=None, setup=None):
    """the host call on one state, the device call on its twin; everything the two leave behind must be equal"""
    fi, fo = rates
    r, t = (speexhip.Resampler(entry.ch, fi, fo, Q, mode=entry.mode) for _ in range(2))
    mem = Mem(kind)
    try:
        for s in (r, t):
            if setup is not None:
                setup(s)
            if split:  # one per-channel call that runs out of room moves channel 0 away from channel 1
                rc, _, _, _ = s.channel_call("int", 0, samples(64)[:37, 0], 37 * fo // fi - 3)
                assert rc == 0
        if split:
            assert len(set(r.positions())) > 1
        before = state_of(r)
        parts = entry.in_parts(samples(frames))
        ins, d_in, in_pitch = [None] * len(parts), 0, 0
        if present:
            ins = []
            for p in parts:
                a = mem.get(p.nbytes, "in")
                a[: p.nbytes] = p.reshape(-1).view(np.uint8)
                ins.append(a.ctypes.data)
            in_pitch = parts[0].shape[0]
            # (an empty input is still an address)
            d_in = torch.from_numpy(np.concatenate([p.reshape(-1).view(np.uint8) for p in parts] + [np.zeros(16, np.uint8)])).cuda()
        n_calls = 3 if entry.name == "chunks" else 1
        out_bytes = max(cap, 1) * n_calls * entry.out_frame_bytes
        outs = [mem.get(out_bytes, "out") for _ in range(entry.n_out)]
        for o in outs:
            o[:] = SENT
        rc, used, made = entry.host(r, ins, frames, [o.ctypes.data for o in outs], cap)
        if expect is not None:
            assert rc == expect, (rc, expect)
            assert state_of(r) == before, "a refused call touched the state"
            assert all((o == SENT).all() for o in outs), "a refused call wrote to the result"
            return
        d_out = torch.full((entry.n_out * out_bytes,), SENT, dtype=torch.uint8, device="cuda")
        rc_t, used_t, made_t = entry.dev(t, d_in.data_ptr() if present else 0, frames, d_out.data_ptr(), cap, in_pitch,
                                         out_bytes // entry.out_frame_bytes)
        torch.cuda.synchronize()
        assert (rc, used, made) == (rc_t, used_t, made_t)
        total = sum(made) if isinstance(made, list) else made
        want = d_out.cpu().numpy().reshape(entry.n_out, out_bytes)
        if entry.n_out == 1 and not entry.float_io and entry.out_frame_bytes == 2 * CH:
            # frames the twin wrote to each channel of an interleaved s16 result: up to the last sample that lost its fill
            cols = want[0].view(np.int16).reshape(-1, CH)
            wrote = [int(np.flatnonzero(cols[:, c] != np.int16(SENT * 0x101 - 0x10000)).max(initial=-1)) + 1 for c in range(CH)]
        if entry.name == "channel":
            if split:  # every channel's own counters: nothing left unread, as many frames as the twin wrote there
                for c, (rc_c, used_c, made_c) in enumerate(entry.per_channel):
                    assert (rc_c, used_c, made_c) == (rc_t, frames, wrote[c]), "channel %d" % c
            else:
                assert all(res == entry.per_channel[0] for res in entry.per_channel)
        if split and not entry.sentinel:
            # (a result block is not filled beforehand: of each channel the frames it wrote, as many as the twin's)
            got = outs[0][: cols.size * 2].view(np.int16).reshape(-1, CH)
            for c in range(CH):
                assert wrote[c] > 0 and got[: wrote[c], c].tobytes() == cols[: wrote[c], c].tobytes(), "samples of channel %d" % c
        for c, o in enumerate(outs):
            n = total * entry.out_frame_bytes
            if split and entry.sentinel:
                # (each channel wrote its own number of frames, one more or less than the call reports: the samples no
                #  channel wrote keep the fill in both buffers)
                assert o.tobytes() == want[c, : o.size].tobytes(), "samples of buffer %d" % c
                n += 2 * entry.out_frame_bytes
            elif not split:
                assert o[:n].tobytes() == want[c, :n].tobytes(), "samples of buffer %d" % c
            if entry.sentinel:
                assert (o[n:] == SENT).all(), "written behind the produced frames of buffer %d" % c
        assert state_of(r) == state_of(t)
    finally:
        mem.close()
        r.close()
        t.close()


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_pageable_buffers_on_every_route(entry, size):
    fi, fo, frames = SIZES[size]
    run_pair(entry, (fi, fo), frames, cap_for(fi, fo, frames))


@pytest.mark.parametrize("size", ["bounce", "copy_copy"])
@pytest.mark.parametrize("kind", ["block_in", "block_out", "block_both"])
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_blocks_of_the_library_are_used_in_place(entry, kind, size):
    fi, fo, frames = SIZES[size]
    run_pair(entry, (fi, fo), frames, cap_for(fi, fo, frames), kind=kind)


@pytest.mark.parametrize("nbytes", [256 * 1024, 256 * 1024 - 1])
def test_caller_pinned_memory_at_the_in_place_threshold(nbytes):
    """an input of exactly 256 KB in memory the caller pinned is read where it lies, one byte less is staged: a mono u8
    state, one byte per frame, a result of a size of its own (and stereo s16 at the exact size)"""
    fmt = Fmt("fmt_u8", ch=1, in_channels=1, in_fmt=FMT_U8, out_fmt=FMT_S16)
    run_pair(fmt, (44100, 48000), nbytes, cap_for(44100, 48000, nbytes), kind="pinned")
    if nbytes % (2 * CH) == 0:
        run_pair(BY_NAME["int"], (44100, 48000), nbytes // (2 * CH), cap_for(44100, 48000, nbytes // (2 * CH)), kind="pinned")


EDGES = {"empty": dict(frames=0, cap=64), "silence": dict(frames=480, cap=600, present=False), "capacity_0": dict(frames=64, cap=0)}


@pytest.mark.parametrize("kind", ["pageable", "block_both"])
@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_empty_input_silence_and_no_room(entry, edge, kind):
    run_pair(entry, (44100, 48000), kind=kind, **EDGES[edge])


@pytest.mark.parametrize("size", ["bounce", "staged_copy", "copy_copy"])
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_channels_that_stand_apart(entry, size):
    """after a per-channel call the channels of a state stand apart: served channel by channel where the entry point can,
    BAD_STATE (and nothing touched) where a matrix needs whole frames"""
    fi, fo, frames = SIZES[size]
    run_pair(entry, (fi, fo), frames, cap_for(fi, fo, frames), split=True, expect=None if entry.splits else ERR_BAD_STATE)


@pytest.mark.parametrize("strides", [(0, 1), (1, 0), (0, 0), (0, 3)])
def test_per_channel_call_with_a_stride_of_zero(strides):
    """speex_resampler_set_input_stride / _output_stride take any value, 0 included: with an input stride of 0 every frame
    reads the caller's first sample -- and nothing behind it -- and with an output stride of 0 every sample lands on the
    first, the last one staying.  The twin takes the same frames written out, strides of 1."""
    in_stride, out_stride = strides
    frames, cap, c, L = 300, 400, 1, speexhip.lib()
    r, t = (speexhip.Resampler(CH, 44100, 48000, Q) for _ in range(2))
    try:
        x = samples(frames)[:, 0].copy()
        x[1:] += 77  # (what lies behind the first sample is not the first sample)
        line = np.repeat(x[:1], frames) if in_stride == 0 else x
        rc_t, used_t, made_t, want = t.channel_call("int", c, line, cap)
        L.speexhip_resampler_set_input_stride(r._h, in_stride)
        L.speexhip_resampler_set_output_stride(r._h, out_stride)
        out = np.full(cap * 3 + 1, r.SENTINEL_I16, np.int16)
        il, ol = u32(frames), u32(cap)
        rc = L.speexhip_resampler_process_int(r._h, c, C.cast(x.ctypes.data, C.POINTER(C.c_int16)), C.byref(il),
                                              C.cast(out.ctypes.data, C.POINTER(C.c_int16)), C.byref(ol))
        assert (rc, il.value, ol.value) == (rc_t, used_t, made_t) and made_t > 0
        if out_stride == 0:
            assert out[0] == want[made_t - 1] and (out[1:] == r.SENTINEL_I16).all()
        else:
            assert (out[: made_t * out_stride: out_stride] == want[:made_t]).all()
            rest = np.ones(out.size, bool)
            rest[: made_t * out_stride: out_stride] = False
            assert (out[rest] == r.SENTINEL_I16).all()
        L.speexhip_resampler_set_input_stride(r._h, 1)
        L.speexhip_resampler_set_output_stride(r._h, 1)
        assert state_of(r) == state_of(t)
    finally:
        r.close()
        t.close()


def test_dither_refuses_channels_that_stand_apart():
    run_pair(BY_NAME["fmt"], (44100, 48000), 64, 128, split=True, expect=ERR_BAD_STATE,
             setup=lambda s: s.set_dither(speexhip.DITHER_TRIANGULAR, 7, 3))


def test_argument_errors_leave_the_state_alone():
    r = speexhip.Resampler(CH, 44100, 48000, Q)
    try:
        before = state_of(r)
        x, L = samples(1024), speexhip.lib()
        out = np.full(4096, SENT, np.uint8)
        il, ol = u32(64), u32(100)
        # a channel the state does not have
        rc = L.speexhip_resampler_process_int(r._h, CH, C.cast(x.ctypes.data, C.POINTER(C.c_int16)), C.byref(il),
                                              C.cast(out.ctypes.data, C.POINTER(C.c_int16)), C.byref(ol))
        assert rc == ERR_INVALID_ARG
        planes_in = (C.c_void_p * CH)(x.ctypes.data, x.ctypes.data + 1024)
        # a result plane missing; result planes that overlap
        for outs, code in (((C.c_void_p * CH)(out.ctypes.data, None), ERR_INVALID_ARG),
                           ((C.c_void_p * CH)(out.ctypes.data, out.ctypes.data + 8), ERR_PTR_OVERLAP)):
            il, ol = u32(32), u32(100)
            assert L.speexhip_resampler_process_planar_int(r._h, planes_in, C.byref(il), outs, C.byref(ol)) == code
            arr = (C.c_void_p * CH)(*outs)
            a = make_side(FMT_S16, CH, LAYOUT_INTERLEAVED, data=x.ctypes.data)
            b = make_side(FMT_S32, CH, LAYOUT_PLANAR, planes=arr)
            il, ol = u32(32), u32(100)
            assert L.speexhip_resampler_process_sides(r._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol)) == code
        # no result buffer
        a, b = make_side(FMT_S16, CH, data=x.ctypes.data), make_side(FMT_S32, CH)
        il, ol = u32(32), u32(100)
        assert L.speexhip_resampler_process_sides(r._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol)) == ERR_INVALID_ARG
        assert state_of(r) == before and (out == SENT).all()
    finally:
        r.close()
