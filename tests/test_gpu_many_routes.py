"""The many-states host calls (speexhip_resampler_process_many_int / _float / _fmt) on every route their buffers can take
(csrc/many_plan.h decides, csrc/many.cpp carries out): one call on a set of states against the separate single-state host
calls (process_interleaved_int / _float, process_sides) on twin states, each call made twice so that the second starts from
a real position.  Entry i of a many-states call IS that single call, so every comparison is equality, in the default mode
and in EXACT: the produced bytes, the consumed and produced counts, the per-entry codes, every channel's position, the
history and the dither position; behind the produced frames the caller's buffer keeps its sentinel fill.

Each case also holds the call to its launches: the deltas of speexhip.many_counters() -- FIR launches, input passes,
output passes, entries that took their own call -- are literals, read off a run of this file against the library of the
commit before the planner existed; the file passes unchanged with that library and with this one.

Quality 3, stereo s16 unless a case says otherwise; the frame counts are those of test_gpu_host_routes.py, the smallest
that reach each route: 64 frames (bounce), 26 000 at 1:8 up (staged in, copied out), 205 000 at 8:1 down (copied in, staged
out), 205 000 at 44.1k -> 48k (copied both ways); 2^20 frames x 8 states is the 32 MiB from which a call is pipelined."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import speexhip
from golden_util import ROOT
from speexhip import FMT_F32, FMT_F32N, FMT_S16, FMT_ULAW

pytestmark = pytest.mark.gpu

CH, Q, SENT = 2, 3, 0xA5
CD, UP, DOWN, BACK = (44100, 48000), (8000, 64000), (64000, 8000), (48000, 44100)
MODES = {"default": None, "exact": speexhip.MODE_EXACT}
DIAG_LIB = os.path.join(ROOT, "node-speex-resampler_amd", "ab", "libspeexhip_diag.so")


class E:
    """One entry of a call: state `st` of the case, `frames` frames of in_fmt (null: a NULL input, silence) into room for
    `cap` frames of out_fmt (None: what the rates make of the frames, and 64).  mem_in / mem_out: "page" = pageable memory,
    "block" = a pinned block of the library, "shared" (both) = one block for both sides, the result overlapping the chunk."""

    def __init__(self, st, frames, cap=None, in_fmt=FMT_S16, out_fmt=FMT_S16, mem_in="page", mem_out="page", null=False):
        self.st, self.frames, self.cap, self.in_fmt, self.out_fmt = st, frames, cap, in_fmt, out_fmt
        self.mem_in, self.mem_out, self.null = mem_in, mem_out, null


def same(n, frames, **kw):
    return [E(i, frames, **kw) for i in range(n)]


def move_apart(s, rates):
    """one per-channel call that runs out of room moves channel 0 away from channel 1"""
    rc, _, _, _ = s.channel_call("int", 0, raw(FMT_S16, 37, 5).view(np.int16), 37 * rates[1] // rates[0] - 3)
    assert rc == 0 and len(set(s.positions())) > 1


def with_dither(s, rates):
    assert s.set_dither(speexhip.DITHER_TRIANGULAR, 7, 3) == 0


# name -> (rates of each state, [(entry point, entries) of each call], setup of each state or None,
#          (FIR launches, input passes, output passes, own calls) of all the calls together)
CASES = {
    "small": ([CD] * 5, [("int", same(5, 64))] * 2, None, (2, 0, 0, 0)),
    "small_float": ([CD] * 5, [("float", same(5, 64, in_fmt=FMT_F32, out_fmt=FMT_F32))] * 2, None, (2, 0, 0, 0)),
    "gathered_and_copied": ([CD] * 4, [("int", [E(0, 5000), E(1, 205000), E(2, 5000), E(3, 5000)])] * 2, None, (2, 0, 0, 0)),
    "staged_in_copied_out": ([UP] * 2, [("int", same(2, 26000))] * 2, None, (2, 0, 0, 0)),
    "copied_in_staged_out": ([DOWN] * 2, [("int", same(2, 205000))] * 2, None, (2, 0, 0, 0)),
    "block_in_small": ([CD] * 3, [("int", same(3, 64, mem_in="block"))] * 2, None, (2, 0, 0, 0)),
    "block_out_small": ([CD] * 3, [("int", same(3, 64, mem_out="block"))] * 2, None, (2, 0, 0, 0)),
    "block_both_small": ([CD] * 3, [("int", same(3, 64, mem_in="block", mem_out="block"))] * 2, None, (2, 0, 0, 0)),
    # (a pinned chunk beside a pageable result of 892 KB, at least 256 KiB: copied like a pageable one)
    "block_in_large_result": ([CD] * 3, [("int", same(3, 205000, mem_in="block"))] * 2, None, (2, 0, 0, 0)),
    # (... beside one of 113 KB: read in place; a large pageable entry beside it keeps the call from being small)
    "block_in_smaller_result": ([CD] * 2, [("int", [E(0, 26000, mem_in="block"), E(1, 205000)])] * 2, None, (2, 0, 0, 0)),
    "block_out_large": ([CD] * 3, [("int", same(3, 205000, mem_out="block"))] * 2, None, (2, 0, 0, 0)),
    "block_both_large": ([CD] * 3, [("int", same(3, 205000, mem_in="block", mem_out="block"))] * 2, None, (2, 0, 0, 0)),
    "block_shared_by_both_sides": ([CD] * 3, [("int", [E(0, 64, mem_in="shared", mem_out="shared"), E(1, 64),
                                                       E(2, 205000, mem_in="shared", mem_out="shared")])] * 2, None, (2, 0, 0, 0)),
    # a NULL input, a present input of 0 frames, capacity 0, nothing to run at all, beside an ordinary entry
    "edge_entries": ([CD] * 5, [("int", [E(0, 480, cap=600, null=True), E(1, 0, cap=64), E(2, 64, cap=0), E(3, 0, cap=0),
                                          E(4, 64)])] * 2, None, (2, 0, 0, 0)),
    "edge_entries_large": ([CD] * 5, [("int", [E(0, 480, cap=600, null=True), E(1, 0, cap=64), E(2, 64, cap=0), E(3, 0, cap=0),
                                                E(4, 205000)])] * 2, None, (2, 0, 0, 0)),
    "a_state_named_twice": ([CD] * 2, [("int", [E(0, 64), E(1, 64), E(0, 480)])] * 2, None, (2, 0, 0, 2)),
    "channels_moved_apart": ([CD] * 2, [("int", same(2, 64))] * 2, [None, move_apart], (2, 0, 0, 2)),
    "two_filters": ([CD, BACK, CD, BACK], [("int", same(4, 64))] * 2, None, (4, 0, 0, 0)),
    "thirty_three_states": ([CD] * 33, [("int", same(33, 64))] * 2, None, (4, 0, 0, 0)),
    "three_formats": ([CD] * 3, [("fmt", [E(0, 64), E(1, 64, in_fmt=FMT_F32, out_fmt=FMT_F32),
                                          E(2, 64, in_fmt=FMT_ULAW, out_fmt=FMT_F32N)])] * 2, [None, None, with_dither], (4, 2, 2, 0)),
    "three_formats_large": ([CD] * 3, [("fmt", [E(0, 205000), E(1, 205000, in_fmt=FMT_F32, out_fmt=FMT_F32),
                                                E(2, 205000, in_fmt=FMT_ULAW, out_fmt=FMT_F32N)])] * 2, [None, None, with_dither],
                            (4, 2, 2, 0)),
    # (states 0 and 1 have taken float samples into their histories, state 2 has not: two launches of the int16 call)
    "int16_after_float": ([CD] * 3, [("float", same(2, 64, in_fmt=FMT_F32, out_fmt=FMT_F32)), ("int", same(3, 64))], None, (3, 0, 0, 0)),
    "pipelined_two_groups": ([CD, BACK] * 4, [("int", same(8, 1 << 20))] * 2, None, (4, 0, 0, 0)),
}
# the cases of a process that splits every call of eight or more states into two lanes (test_two_lanes)
LANE_CASES = {
    "lanes_small": ([CD] * 9, [("int", same(9, 64))] * 2, None, (4, 0, 0, 0)),
    "lanes_copied": ([CD] * 9, [("int", same(9, 70000))] * 2, None, (4, 0, 0, 0)),
}

_raws = {}


def raw(fmt, samples, seed):
    """`samples` samples of a format as bytes, made once and left as they are: audio-sized values for s16 and f32, any
    bytes for mu-law"""
    key = (fmt, samples, seed) if samples <= 1 << 19 else None  # (the largest are made again: 10 ms, not 4 MB kept each)
    if key not in _raws:
        rng = np.random.default_rng(1000 * seed + fmt)
        if fmt == FMT_S16:
            v = rng.integers(-20000, 20000, samples, dtype=np.int16)
        elif fmt == FMT_F32:
            v = (rng.standard_normal(samples, dtype=np.float32) * np.float32(6000.0))
        else:
            assert fmt == FMT_ULAW
            v = rng.integers(0, 256, samples, dtype=np.uint8)
        v = v.view(np.uint8)
        v.setflags(write=False)
        if key is None:
            return v
        _raws[key] = v
    return _raws[key]


def u32(v):
    return C.c_uint32(int(v))


def state_of(r):
    torch.cuda.synchronize()
    return r.positions(), r._lines().tobytes(), r.get_dither()


class Buffers:
    """the caller's memory of one call: per entry the chunk (None: a NULL input) and the room for the result, filled with
    the sentinel"""

    def __init__(self, entries, rates, seed):
        self.blocks, self.ins, self.outs, self.caps = [], [], [], []
        for k, e in enumerate(entries):
            fi, fo = rates[e.st]
            cap = e.frames * fo // fi + 64 if e.cap is None else e.cap
            x = raw(e.in_fmt, e.frames * CH, seed + k)
            out_bytes = max(cap, 1) * CH * speexhip.fmt_bytes(e.out_fmt)
            if e.mem_in == "shared":  # the result starts in the last quarter of the chunk
                at = (x.size * 3 // 4 + 63) & ~63
                whole = self.block(at + out_bytes)
                whole[:] = SENT
                a, o = whole[: x.size], whole[at:]
            else:
                a = self.block(max(x.size, 1)) if e.mem_in == "block" else np.empty(max(x.size, 1), np.uint8)
                o = self.block(out_bytes) if e.mem_out == "block" else np.empty(out_bytes, np.uint8)
                o[:] = SENT
            a[: x.size] = x
            self.ins.append(None if e.null else a)
            self.outs.append(o)
            self.caps.append(cap)

    def block(self, nbytes):
        b = speexhip.PinnedBlock(nbytes)
        self.blocks.append(b)
        return b.array(np.uint8, (nbytes,))

    def close(self):
        for b in self.blocks:
            b.close()


def many_call(api, states, entries, buf):
    """(rc, consumed, produced, codes) of the one many-states call"""
    n = len(entries)
    ins = [None if a is None else a.ctypes.data for a in buf.ins]
    outs = [o.ctypes.data for o in buf.outs]
    lens = [e.frames for e in entries]
    if api == "fmt":
        return speexhip.many_fmt_call(states, [e.in_fmt for e in entries], ins, lens, [e.out_fmt for e in entries], outs, buf.caps)
    hs, ia, oa = (C.c_void_p * n)(*[s._h for s in states]), (C.c_void_p * n)(*ins), (C.c_void_p * n)(*outs)
    il, ol, codes = (C.c_uint32 * n)(*lens), (C.c_uint32 * n)(*buf.caps), (C.c_int * n)()
    fn = speexhip.lib().speexhip_resampler_process_many_int if api == "int" else speexhip.lib().speexhip_resampler_process_many_float
    rc = fn(n, hs, ia, il, oa, ol, codes)
    return rc, list(il), list(ol), list(codes)


def single_call(api, tw, e, x, cap):
    """the entry as a single-state host call of the twin, on pageable memory of its own: (rc, consumed, produced, result)"""
    out = np.full(max(cap, 1) * CH * speexhip.fmt_bytes(e.out_fmt), SENT, np.uint8)
    il, ol, L = u32(e.frames), u32(cap), speexhip.lib()
    if api == "fmt":
        a = speexhip.make_side(e.in_fmt, CH, data=None if x is None else x.ctypes.data)
        b = speexhip.make_side(e.out_fmt, CH, data=out.ctypes.data)
        rc = L.speexhip_resampler_process_sides(tw._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
    else:
        fn, ct = ((L.speexhip_resampler_process_interleaved_int, C.c_int16) if api == "int" else
                  (L.speexhip_resampler_process_interleaved_float, C.c_float))
        rc = fn(tw._h, C.cast(None if x is None else x.ctypes.data, C.POINTER(ct)), C.byref(il), C.cast(out.ctypes.data, C.POINTER(ct)),
                C.byref(ol))
    return rc, il.value, ol.value, out


def run_case(case, mode):
    rates, calls, setup, want = case
    states, twins = ([speexhip.Resampler(CH, fi, fo, Q, mode=mode) for fi, fo in rates] for _ in range(2))
    try:
        for group in (states, twins):
            for j, s in enumerate(group):
                if setup is not None and setup[j] is not None:
                    setup[j](s, rates[j])
        c0 = speexhip.many_counters()
        for step, (api, entries) in enumerate(calls):
            buf = Buffers(entries, rates, 10 * step)
            try:
                rc, used, made, codes = many_call(api, [states[e.st] for e in entries], entries, buf)
                assert rc == 0, (step, rc, codes)
                for k, e in enumerate(entries):  # (a state named twice: its twin takes the calls in the caller's order)
                    x = None if e.null else np.array(raw(e.in_fmt, e.frames * CH, 10 * step + k))
                    rc_t, used_t, made_t, out_t = single_call(api, twins[e.st], e, x, buf.caps[k])
                    assert (codes[k], used[k], made[k]) == (rc_t, used_t, made_t), (step, k)
                    n = made[k] * CH * speexhip.fmt_bytes(e.out_fmt)
                    assert buf.outs[k][:n].tobytes() == out_t[:n].tobytes(), "samples of entry %d, call %d" % (k, step)
                    assert (buf.outs[k][n:] == SENT).all() and (out_t[n:] == SENT).all(), "written behind the frames of entry %d" % k
                for j in range(len(states)):
                    assert state_of(states[j]) == state_of(twins[j]), (step, j)
            finally:
                buf.close()
        c1 = speexhip.many_counters()
        got = tuple(c1[k] - c0[k] for k in ("fir_launches", "in_passes", "out_passes", "own_calls"))
        print("counters of the calls:", got)
        assert got == want
    finally:
        for s in states + twins:
            s.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_every_route_equals_the_single_calls(name, mode):
    run_case(CASES[name], MODES[mode])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_lanes(mode):
    """SPEEXHIP_MANY_LANES=2 (the diagnostics build, a child process) splits every call of at least eight states into two
    units, each on a stage and a thread of its own: nine states run as four and five."""
    if os.environ.get("SPEEXHIP_MANY_LANES") == "2":
        for name in LANE_CASES:
            run_case(LANE_CASES[name], MODES[mode])
        return
    assert os.path.exists(DIAG_LIB), "ab/libspeexhip_diag.so not built (make -C node-speex-resampler_amd diag)"
    env = dict(os.environ, SPEEXHIP_LIB_PATH=DIAG_LIB, SPEEXHIP_MANY_LANES="2")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "test_two_lanes and " + mode], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0 and "1 passed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
