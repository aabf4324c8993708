"""The formatted many-states call (speexhip_resampler_process_many_sides / _fmt) on the GPU: entry i IS
speexhip_resampler_process_sides on states[i] -- bytes, counters, history, position, dither position and code -- so every
comparison here is byte equality with a twin state fed the same bytes by separate calls.  No tolerance anywhere: neither
the default mode's bytes nor the exact mode's depend on what shares a launch.

Sizes are the smallest that reach both paths of the pass (kernels_convert_many.hip): a telephony frame (160), a whole
4096-sample tile plus a ragged tail, several tiles; 40 states make launches of 32 + 8."""
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
ALL = (U8, S16, S24, S32, F32, F32N, ULAW, ALAW, F16N, BF16N, S16BE, S24BE, S32BE)
SENTINEL = 0xA5
CONFIGS = {"slide": (1, 8000, 16000, 7), "period": (2, 44100, 48000, 7), "fp64": (1, 48000, 16000, 10)}
MODES = {"default": None, "exact": speexhip.MODE_EXACT}


def storage(fmt, samples, seed):
    """`samples` samples of format fmt as raw bytes (uint8): any bytes for the integer and companded formats, finite
    audio-sized values for the float ones"""
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
    i = st.info()
    return (i["last_sample"], i["samp_frac_num"], i["magic_samples"], st._lines().tobytes(), st.get_dither())


def separate(st, in_fmt, raw, frames, out_fmt, cap, room=None):
    """speexhip_resampler_process_sides on interleaved sides: raw = the input's bytes (None: silence of `frames` frames).
    Returns (rc, consumed, produced, the whole output buffer, SENTINEL beyond what was written)."""
    ch = st.channels
    out = np.full(max(cap if room is None else room, 1) * ch * speexhip.fmt_bytes(out_fmt), SENTINEL, np.uint8)
    a = speexhip.make_side(in_fmt, ch, data=None if raw is None else raw.ctypes.data)
    b = speexhip.make_side(out_fmt, ch, data=out.ctypes.data)
    il, ol = C.c_uint32(frames), C.c_uint32(cap)
    rc = speexhip.lib().speexhip_resampler_process_sides(st._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
    return rc, il.value, ol.value, out


def fused(states, in_fmts, raws, frames, out_fmts, caps, out_bufs=None):
    """speexhip_resampler_process_many_fmt over pageable buffers (or out_bufs); (rc, consumed, produced, codes, outs)"""
    outs = out_bufs or [np.full(max(caps[i], 1) * st.channels * speexhip.fmt_bytes(out_fmts[i]), SENTINEL, np.uint8)
                        for i, st in enumerate(states)]
    rc, used, made, codes = speexhip.many_fmt_call(states, in_fmts, [None if r is None else r.ctypes.data for r in raws],
                                                   frames, out_fmts, [o.ctypes.data for o in outs], caps)
    return rc, used, made, codes, outs


def make_states(key, n, mode):
    return [speexhip.Resampler(*key, mode=mode) for _ in range(n)]


def close_all(*lists):
    for states in lists:
        for st in states:
            st.close()


def entry_plan(key, n, step, seed):
    """formats, lengths, inputs and capacities of the n entries of one step: formats cycle over all 13 on each side
    independently, lengths over the five sizes; some inputs are NULL, some capacities tight"""
    ch, fi, fo, _ = key
    sizes = (0, 1, 160, 4096 // ch + 37, 3 * 4096 // ch)
    in_fmts = [ALL[i % 13] for i in range(n)]
    out_fmts = [ALL[(3 * i + 1 + step) % 13] for i in range(n)]
    frames = [sizes[(i + 2 * step) % 5] for i in range(n)]
    raws = [None if i % 11 == 5 else storage(in_fmts[i], frames[i] * ch, seed + 100 * step + i) for i in range(n)]
    caps = [frames[i] * fo // fi + 64 for i in range(n)]
    caps = [max(1, c // 3) if i % 7 == 3 else c for i, c in enumerate(caps)]
    return in_fmts, out_fmts, frames, raws, caps


def assert_entries_equal(states, twins, in_fmts, raws, frames, out_fmts, caps, got, tag):
    rc, used, made, codes, outs = got
    for i, (st, tw) in enumerate(zip(states, twins)):
        rc_t, used_t, made_t, out_t = separate(tw, in_fmts[i], raws[i], frames[i], out_fmts[i], caps[i])
        assert (codes[i], used[i], made[i]) == (rc_t, used_t, made_t), (tag, i, in_fmts[i], out_fmts[i], frames[i], caps[i])
        assert outs[i].tobytes() == out_t.tobytes(), (tag, i, in_fmts[i], out_fmts[i], frames[i], made[i])
        assert state_of(st) == state_of(tw), (tag, i)


# ---- 1. equality with separate calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_forty_states_of_thirteen_formats_equal_the_separate_calls(config, mode):
    key, n = CONFIGS[config], 40
    states, twins = make_states(key, n, MODES[mode]), make_states(key, n, MODES[mode])
    try:
        for step in range(3):
            in_fmts, out_fmts, frames, raws, caps = entry_plan(key, n, step, 7000)
            got = fused(states, in_fmts, raws, frames, out_fmts, caps)
            assert got[0] == 0
            assert_entries_equal(states, twins, in_fmts, raws, frames, out_fmts, caps, got, (config, mode, step))
    finally:
        close_all(states, twins)


# ---- 2. identity kinds -----------------------------------------------------------------------------------------------
def test_same_format_entries_are_the_int16_and_float_calls():
    """S16 -> S16 is process_many_int, F32 -> F32 process_many_float, F32N -> F32N the float call on the same bytes.  After a
    change to a shorter filter the states hold pending frames, and entry 0 of the second step brings an empty chunk: the
    float rule drains the pending frames into the room given, the int16 rule produces nothing (picked with plan_call_ex)."""
    key = CONFIGS["period"]
    ch, fi, fo, q = key
    lens = [[1500, 160, 4096 // ch + 37, 3 * 4096 // ch, 0], [0, 160, 4096 // ch + 37, 1, 3 * 4096 // ch]]
    n = len(lens[0])
    for fmt, dtype in ((S16, np.int16), (F32, np.float32), (F32N, np.float32)):
        states, twins = make_states(key, n, None), make_states(key, n, None)
        try:
            for step in range(2):
                caps = [100 if f == 0 else f * fo // fi + 64 for f in lens[step]]
                want_counters = None
                if step == 1:
                    for st in states + twins:
                        assert st.set_quality(3) == 0
                    i0 = states[0].info()
                    assert i0["magic_samples"] > 0
                    plans = [speexhip.plan_call_ex(i0["num_rate"], i0["den_rate"], 0, caps[0], fe, i0["block_in"], i0["last_sample"],
                                                   i0["samp_frac_num"], i0["magic_samples"])[:2] for fe in (0, 1)]
                    assert plans[0] != plans[1] and plans[1][1] > 0, plans
                    want_counters = plans[0 if fmt == S16 else 1]
                raws = [storage(fmt, f * ch, 31 * step + i) for i, f in enumerate(lens[step])]
                rc, used, made, codes, outs = fused(states, [fmt] * n, raws, lens[step], [fmt] * n, caps)
                assert rc == 0 and codes == [0] * n
                if fmt == F32N:   # the float call on the same bytes
                    want = [tw.process_float(r.view(np.float32).reshape(-1, ch), caps[i]) for i, (tw, r) in enumerate(zip(twins, raws))]
                    w_out, w_used = [w[0] for w in want], [w[1] for w in want]
                else:
                    w_out, w_used, w_codes = speexhip.process_many(twins, [r.view(dtype).reshape(-1, ch) for r in raws], caps, dtype=dtype)
                    assert w_codes == [0] * n
                for i in range(n):
                    assert (used[i], made[i]) == (w_used[i], w_out[i].shape[0]), (fmt, step, i)
                    assert outs[i][: made[i] * ch * dtype().itemsize].tobytes() == w_out[i].tobytes(), (fmt, step, i)
                    assert not (outs[i][made[i] * ch * dtype().itemsize:] != SENTINEL).any(), (fmt, step, i)
                    assert state_of(states[i]) == state_of(twins[i]), (fmt, step, i)
                if want_counters is not None:
                    assert (used[0], made[0]) == tuple(want_counters), (fmt, used[0], made[0], want_counters)
        finally:
            close_all(states, twins)


# ---- 3. dither -------------------------------------------------------------------------------------------------------
def test_each_state_is_dithered_at_its_own_kind_seed_and_position():
    key = CONFIGS["slide"]
    ch = key[0]
    kinds = (speexhip.DITHER_NONE, speexhip.DITHER_RECTANGULAR, speexhip.DITHER_TRIANGULAR)
    out_cycle = (U8, S16, S24BE, ULAW, F32N, F16N)   # (the float outputs are not dithered, their position moves all the same)
    n = 36
    states, twins = make_states(key, n, None), make_states(key, n, None)
    try:
        for i in range(n):
            for st in (states[i], twins[i]):
                assert st.set_dither(kinds[i % 3], 1000 + 17 * i, (1 << 32) - 700 + 4001 * i if i % 4 == 0 else 13 * i) == 0
        for step in range(2):
            in_fmts = [(S16, F32, ALAW)[(i + step) % 3] for i in range(n)]
            out_fmts = [out_cycle[(i // 3 + step) % len(out_cycle)] for i in range(n)]
            frames = [(160, 4096 + 37, 3 * 4096)[i % 3] for i in range(n)]
            raws = [storage(in_fmts[i], frames[i] * ch, 500 + 50 * step + i) for i in range(n)]
            caps = [f * 2 + 64 for f in frames]
            before = [st.get_dither()[2] for st in states]
            got = fused(states, in_fmts, raws, frames, out_fmts, caps)
            assert got[0] == 0
            assert_entries_equal(states, twins, in_fmts, raws, frames, out_fmts, caps, got, ("dither", step))
            for i, st in enumerate(states):
                moved = got[2][i] if kinds[i % 3] != speexhip.DITHER_NONE else 0
                assert st.get_dither()[2] == (before[i] + moved) % (1 << 64) and got[2][i] > 0, (step, i)
    finally:
        close_all(states, twins)


# ---- 4. entries that take their own call -----------------------------------------------------------------------------
def test_entries_a_launch_cannot_serve_take_their_own_call_in_order():
    key = CONFIGS["period"]
    ch, fi, fo, q = key
    n = 12
    L = speexhip.lib()
    states, twins = make_states(key, n, None), make_states(key, n, None)
    try:
        x = (np.arange(600, dtype=np.int16).reshape(300, 2) * 37) % 9000
        for s in (states[2], twins[2]):       # channels moved apart by per-channel calls
            s.channel_call("int", 0, x[:300, 0], 400)
            s.channel_call("int", 1, x[:150, 1], 400)
        for s in (states[4], twins[4]):       # the zero fallback
            L.speexhip_debug_fail_device_allocs(1)
            rc = s.set_rate(32000, 48000)
            L.speexhip_debug_fail_device_allocs(0)
            assert rc == speexhip.ERR_ALLOC_FAILED
        frames = 2000
        order = list(range(n)) + [6]          # state 6 named twice: its second entry sees the first one's end state
        m = len(order)
        in_fmts = [ALL[(2 * k + 1) % 13] for k in range(m)]
        out_fmts = [ALL[(5 * k + 2) % 13] for k in range(m)]
        raws = [storage(in_fmts[k], frames * ch, 900 + k) for k in range(m)]
        cap = frames * fo // fi + 64
        mono_mix = np.array([[0.5, 0.5]], np.float32)      # output side: 1 x 2
        bo = [speexhip.fmt_bytes(f) for f in out_fmts]

        def sides_for(k, out):
            a = speexhip.make_side(in_fmts[k], ch, data=raws[k].ctypes.data)
            if k == 8:     # a planar stereo output side
                b = speexhip.make_side(out_fmts[k], ch, layout=speexhip.LAYOUT_PLANAR, data=out.ctypes.data, plane_stride=cap)
            elif k == 10:  # an output side with a matrix: stereo -> mono
                b = speexhip.make_side(out_fmts[k], 1, mix=mono_mix, data=out.ctypes.data)
            else:
                b = speexhip.make_side(out_fmts[k], ch, data=out.ctypes.data)
            return a, b

        outs = [np.full(cap * ch * bo[k], SENTINEL, np.uint8) for k in range(m)]
        sides = [sides_for(k, outs[k]) for k in range(m)]
        c0 = speexhip.many_counters()
        rc, used, made, codes = speexhip.process_many_sides([states[j] for j in order], [s[0] for s in sides], [frames] * m,
                                                           [s[1] for s in sides], [cap] * m)
        c1 = speexhip.many_counters()
        assert c1["own_calls"] - c0["own_calls"] == 5
        # the same calls one by one: the fused ones first, then the own calls in the caller's order -- for a state named
        # once the order does not matter, the state named twice runs its entries in the caller's order either way
        for k, j in enumerate(order):
            out_t = np.full(cap * ch * bo[k], SENTINEL, np.uint8)
            a, b = sides_for(k, out_t)
            il, ol = C.c_uint32(frames), C.c_uint32(cap)
            rc_t = L.speexhip_resampler_process_sides(twins[j]._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
            assert (codes[k], used[k], made[k]) == (rc_t, il.value, ol.value), (k, j)
            assert outs[k].tobytes() == out_t.tobytes(), (k, j)
            if k == 4:
                assert rc_t == speexhip.ERR_ALLOC_FAILED and made[k] > 0
            else:
                assert rc_t == 0 and made[k] > 0, (k, rc_t)
        assert rc == speexhip.ERR_ALLOC_FAILED     # the first code that is not SUCCESS
        for j in range(n):
            assert state_of(states[j]) == state_of(twins[j]), j
    finally:
        L.speexhip_debug_fail_device_allocs(0)
        close_all(states, twins)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------
def test_an_entrys_argument_error_leaves_its_state_and_lengths_untouched():
    key = CONFIGS["slide"]
    ch, fi, fo, q = key
    n, frames = 6, 500
    cap = frames * 2 + 64
    states, twins = make_states(key, n, None), make_states(key, n, None)
    try:
        in_fmts, out_fmts = [ULAW, S16, ALAW, S24, U8, F32N], [F32N, S16, S16BE, ULAW, S32, F16N]
        for step in range(2):
            raws = [storage(in_fmts[i], frames * ch, 40 * step + i) for i in range(n)]
            for case in ("format", "null_out", "struct_size", "channels"):
                bad = {"format": 1, "null_out": 2, "struct_size": 3, "channels": 4}[case]
                before = state_of(states[bad])
                outs = [np.full(cap * ch * speexhip.fmt_bytes(out_fmts[i]), SENTINEL, np.uint8) for i in range(n)]
                a = [speexhip.make_side(in_fmts[i], ch, data=raws[i].ctypes.data) for i in range(n)]
                b = [speexhip.make_side(out_fmts[i], ch, data=outs[i].ctypes.data) for i in range(n)]
                if case == "format":
                    a[bad].fmt = 9
                elif case == "null_out":
                    b[bad].data = None
                elif case == "struct_size":
                    b[bad].struct_size = C.sizeof(speexhip.Side) - 8
                else:
                    a[bad].channels = ch + 1
                rc, used, made, codes = speexhip.process_many_sides(states, a, [frames] * n, b, [cap] * n)
                assert rc == speexhip.ERR_INVALID_ARG and codes[bad] == speexhip.ERR_INVALID_ARG, (case, codes)
                assert (used[bad], made[bad]) == (frames, cap) and state_of(states[bad]) == before, case
                assert not (outs[bad] != SENTINEL).any()
                for i in range(n):
                    if i == bad:
                        continue
                    rc_t, used_t, made_t, out_t = separate(twins[i], in_fmts[i], raws[i], frames, out_fmts[i], cap)
                    assert (codes[i], used[i], made[i]) == (rc_t, used_t, made_t) and rc_t == 0, (case, i)
                    assert outs[i].tobytes() == out_t.tobytes() and state_of(states[i]) == state_of(twins[i]), (case, i)
                # (the twin of the entry that sat out stays level with it)
            if step == 0:
                got = fused(states, in_fmts, raws, [frames] * n, out_fmts, [cap] * n)
                assert_entries_equal(states, twins, in_fmts, raws, [frames] * n, out_fmts, [cap] * n, got, "after errors")
        # the thin form: an unknown format there
        rc, used, made, codes, outs = fused(states[:2], [9, S16], [raws[0], raws[1]], [frames] * 2, [S16, S16], [cap] * 2)
        assert rc == speexhip.ERR_INVALID_ARG and codes == [speexhip.ERR_INVALID_ARG, 0] and (used[0], made[0]) == (frames, cap)
    finally:
        close_all(states, twins)


# ---- 6. routes -------------------------------------------------------------------------------------------------------
def test_pinned_blocks_and_pageable_buffers_in_one_call():
    key, n = CONFIGS["period"], 40
    ch = key[0]
    states, twins = make_states(key, n, None), make_states(key, n, None)
    blocks = []
    try:
        for step in range(2):
            in_fmts, out_fmts, frames, raws, caps = entry_plan(key, n, step, 9000)
            outs = []
            for i in range(n):
                if raws[i] is not None and raws[i].size and i % 3 == 0:     # the chunk in a pinned block
                    blk = speexhip.PinnedBlock(raws[i].size)
                    blocks.append(blk)
                    view = blk.array(np.uint8, (raws[i].size,))
                    view[:] = raws[i]
                    raws[i] = view
                size = max(caps[i], 1) * ch * speexhip.fmt_bytes(out_fmts[i])
                if i % 4 == 1:                                              # the result in a pinned block
                    blk = speexhip.PinnedBlock(size)
                    blocks.append(blk)
                    o = blk.array(np.uint8, (size,))
                    o[:] = SENTINEL
                else:
                    o = np.full(size, SENTINEL, np.uint8)
                outs.append(o)
            got = fused(states, in_fmts, raws, frames, out_fmts, caps, out_bufs=outs)
            assert got[0] == 0
            assert_entries_equal(states, twins, in_fmts, raws, frames, out_fmts, caps, got, ("pinned", step))
    finally:
        for blk in blocks:
            blk.close()
        close_all(states, twins)


def test_a_large_pageable_call_takes_the_pipelined_path():
    """34 states x 2^18 stereo frames, half s16 and half s24 (42.6 MB of pageable input: more than the 32 MB from which
    the call runs in pieces), f32n results"""
    key, n, frames = CONFIGS["period"], 34, 1 << 18
    ch, fi, fo, q = key
    states, twins = make_states(key, n, None), make_states(key, n, None)
    try:
        in_fmts = [S16 if i % 2 == 0 else S24 for i in range(n)]
        base = {f: storage(f, frames * ch + 64 * 3 * 4, 77) for f in (S16, S24)}
        b = {f: speexhip.fmt_bytes(f) for f in (S16, S24)}
        raws = [base[f][i * b[f]: i * b[f] + frames * ch * b[f]] for i, f in enumerate(in_fmts)]   # (shifted: the states differ)
        raws = [np.ascontiguousarray(r) for r in raws]
        cap = frames * fo // fi + 64
        assert sum(r.size for r in raws) > 32 << 20
        c0 = speexhip.many_counters()
        got = fused(states, in_fmts, raws, [frames] * n, [F32N] * n, [cap] * n)
        c1 = speexhip.many_counters()
        assert got[0] == 0 and c1["own_calls"] == c0["own_calls"]
        assert c1["fir_launches"] - c0["fir_launches"] >= 2 and c1["in_passes"] - c0["in_passes"] == c1["fir_launches"] - c0["fir_launches"]
        for i in (0, 1, 16, 17, 32, 33):
            rc_t, used_t, made_t, out_t = separate(twins[i], in_fmts[i], raws[i], frames, F32N, cap)
            assert (got[3][i], got[1][i], got[2][i]) == (rc_t, used_t, made_t), i
            assert got[4][i].tobytes() == out_t.tobytes(), i
            assert state_of(states[i]) == state_of(twins[i]), i
    finally:
        close_all(states, twins)


# ---- 7. fusion -------------------------------------------------------------------------------------------------------
def test_forty_states_of_five_formats_cost_two_launches_and_two_passes_a_side():
    key, n, frames = CONFIGS["slide"], 40, 160
    states = make_states(key, n, None)
    try:
        in_fmts = [(ULAW, ALAW, S16BE, S16, U8)[i % 5] for i in range(n)]
        # (no entry is S16 -> S16: that pair is the int16 call, a launch group of its own kind)
        out_fmts = [(F32N, S16, ULAW, ALAW, S24)[(i + 1) % 5] for i in range(n)]
        assert all(p != (S16, S16) for p in zip(in_fmts, out_fmts)) and len(set(in_fmts)) == len(set(out_fmts)) == 5
        raws = [storage(in_fmts[i], frames, i) for i in range(n)]
        c0 = speexhip.many_counters()
        rc, used, made, codes, outs = fused(states, in_fmts, raws, [frames] * n, out_fmts, [400] * n)
        c1 = speexhip.many_counters()
        assert rc == 0 and codes == [0] * n and min(made) > 0
        d = {k: c1[k] - c0[k] for k in c0}
        print("counters of the call:", d)
        assert d["fir_launches"] == 2 and d["in_passes"] <= 2 and d["out_passes"] <= 2 and d["own_calls"] == 0, d
        assert d["in_passes"] >= 1 and d["out_passes"] >= 1
    finally:
        close_all(states)


# ---- 8. Node ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_batch_formatted_chunks_equal_the_single_instances():
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test_many_formats.js")
    res = subprocess.run(["node", script], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "many formats: ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


# ---- 9. time ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("SPEEXHIP_PERF_GATE") == "0", reason="SPEEXHIP_PERF_GATE=0")
def test_one_fused_call_is_not_slower_than_thirty_two_separate_calls():
    """32 mono 8000 -> 16000 q7 legs, 160-frame mu-law payloads, f32n results: the median of one fused call against the
    median of the 32 separate process_interleaved_fmt calls, 300 steps each, interleaved so that both see the same box."""
    key, n, frames, cap, steps = CONFIGS["slide"], 32, 160, 400, 300
    states, twins = make_states(key, n, None), make_states(key, n, None)
    L = speexhip.lib()
    try:
        raws = [storage(ULAW, frames, i) for i in range(n)]
        outs = [np.zeros(cap * 4, np.uint8) for _ in range(n)]
        hs, ins, ops = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        fi_, fo_ = (C.c_int * n)(*[ULAW] * n), (C.c_int * n)(*[F32N] * n)
        il, ol, codes = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int * n)()
        for i in range(n):
            hs[i], ins[i], ops[i] = states[i]._h, raws[i].ctypes.data, outs[i].ctypes.data

        def one_fused():
            for i in range(n):
                il[i], ol[i] = frames, cap
            assert L.speexhip_resampler_process_many_fmt(n, hs, fi_, ins, il, fo_, ops, ol, codes) == 0

        a, b = C.c_uint32(), C.c_uint32()

        def one_by_one():
            for i in range(n):
                a.value, b.value = frames, cap
                assert L.speexhip_resampler_process_interleaved_fmt(twins[i]._h, ULAW, ins[i], C.byref(a), F32N, ops[i], C.byref(b)) == 0

        t_fused, t_apart = [], []
        for step in range(steps + 20):
            t0 = time.perf_counter()
            one_fused()
            t1 = time.perf_counter()
            one_by_one()
            t2 = time.perf_counter()
            if step >= 20:
                t_fused.append(t1 - t0)
                t_apart.append(t2 - t1)
        fused_us, apart_us = np.median(t_fused) * 1e6, np.median(t_apart) * 1e6
        print("32 x 160-frame mu-law -> f32n: fused %.1f us, 32 separate calls %.1f us (medians of %d)" % (fused_us, apart_us, steps))
        assert fused_us <= apart_us, (fused_us, apart_us)
    finally:
        close_all(states, twins)
