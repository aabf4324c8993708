"""Every scenario of tests/test_gpu_async_order.py can fail: for every adjacent pair of calls (N, N+1) of every script the
GPU file runs, call N+1 made on the state "as if call N had not run yet on the device" -- stated on the oracle alone,
async_order.stale_pairs -- differs from the correct call N+1 in its output (in the history it leaves where it produces no
output; in what it returns where it is a read).  A script or pair for which the two agree -- a chunk of silence would do
it -- is rejected here, so a green GPU run cannot be a run that had nothing to see.  No GPU needed."""
import numpy as np
import pytest

import async_order as ao
import oracle as orc

SCRIPTS = ao.all_scripts()


def _id(entry):
    script = entry[0]
    if isinstance(script, tuple):
        script = script[0]
    return "%s-%s" % (script.name.replace(" ", "_").replace(":", ""), script.family)


def test_a_copied_oracle_state_is_independent_and_equal():
    """Oracle.clone / set_lines, the two hooks the stale states are made with"""
    for filt in ((2, 44100, 48000, 7), (1, 24000, 48000, 10), (2, 192000, 1000, 8)):
        ch = filt[0]
        a = orc.Oracle(*filt)
        a.process(ao.pcm(3000, ch, 1), 1 << 16)
        a.set_quality(filt[3] - 2)             # (pending frames, another filter length)
        a.process_float(ao.floats(700, ch, 2), 5)
        b = a.clone()
        state = lambda o: (o.position(), o.positions(), [o.history(c).tobytes() + o.pending(c).tobytes() for c in range(ch)])
        assert state(a) == state(b)
        x = ao.floats(2000, ch, 3)
        yb, ub = b.process_float(x, 1 << 16)
        assert state(a) != state(b)            # the copy moved alone
        ya, ua = a.process_float(x, 1 << 16)
        assert ua == ub and ya.tobytes() == yb.tobytes() and state(a) == state(b)
        # set_lines: the lines change, positions and counts stay
        c2 = a.clone()
        fresh = np.arange(a.taps - 1, dtype=np.float32)
        c2.set_lines(0, fresh)
        assert c2.history(0).tobytes() == fresh.tobytes() and c2.positions() == a.positions()
        if ch > 1:
            assert c2.history(1).tobytes() == a.history(1).tobytes()
        assert a.history(0).tobytes() != fresh.tobytes()


def test_device_buffer_layouts_round_trip():
    """lay_in / take_out, the numpy half of the GPU runner: planar and interleaved sides, packed samples, several streams"""
    sf = ao.sf
    for in_fmt, layout, n_ch in ((sf.S16, ao.P, 3), (sf.S24, ao.P, 2), (sf.S24, ao.I, 2), (sf.F32, ao.I, 2)):
        xs = [ao._storage(in_fmt, 50 - 7 * s, n_ch, s) for s in range(3)]
        call = ao.Call("sides", xs, 40, "A", in_fmt, in_fmt, None, None, layout, layout)
        host, g = ao.lay_in(call, n_ch)
        assert host.size == g.in_bytes and (g.planar_in, g.planar_out) == (layout == ao.P, layout == ao.P)
        rows = host.reshape(3, -1)
        for s in range(3):
            frames, b = 50 - 7 * s, g.bi
            raw = xs[s].view(np.uint8).reshape(frames, n_ch, b)
            for c in range(n_ch):
                for f in (0, frames - 1):
                    at = (c * g.in_plane + f) * b if layout == ao.P else (f * n_ch + c) * b
                    assert rows[s, at: at + b].tobytes() == raw[f, c].tobytes(), (in_fmt, layout, s, c, f)
        # an output buffer in which stream s produced 10 + s frames, frame f of channel c = the byte value f + c
        made = [10, 11, 12]
        out = np.full((3, g.out_row * g.bo), ao.SENTINEL, np.uint8)
        for s in range(3):
            for f in range(made[s]):
                for c in range(n_ch):
                    at = (c * g.out_plane + f) * g.bo if layout == ao.P else (f * n_ch + c) * g.bo
                    out[s, at: at + g.bo] = f + c
        got, clean = ao.take_out(g, out.reshape(-1), made)
        assert clean
        for s in range(3):
            want = np.repeat((np.arange(made[s])[:, None] + np.arange(n_ch)[None, :]).astype(np.uint8), g.bo)
            assert got[s] == want.tobytes(), (in_fmt, layout, s)
        out[1, -1] = 0
        assert not ao.take_out(g, out.reshape(-1), made)[1]


def test_the_stale_state_check_rejects_a_script_that_cannot_fail():
    """silence after silence: stale and correct agree, and stale_pairs says so"""
    ch, fi, fo, q = ao.FAMILIES["period"][:4]
    quiet = ao.Script("quiet", "period", [ao.Call("int", np.zeros((3000, ch), np.int16), ao.wcap(3000, fi, fo), "A"),
                                         ao.Call("int", np.zeros((3000, ch), np.int16), ao.wcap(3000, fi, fo), "B"),
                                         ao.Call("int", ao.pcm(3000, ch, 1), ao.wcap(3000, fi, fo), "A")])
    pairs = ao.stale_pairs(quiet)
    assert [d for _, _, d in pairs] == [False, False]   # (the third call: both older histories are silence too)
    loud = ao.Script("loud", "period", [ao.Call("int", ao.pcm(3000, ch, 2), ao.wcap(3000, fi, fo), "A"),
                                       ao.Call("int", np.zeros((3000, ch), np.int16), ao.wcap(3000, fi, fo), "B")])
    assert [d for _, _, d in ao.stale_pairs(loud)] == [True]


def test_the_scripts_cover_what_the_scenarios_name():
    names = {(s[0] if isinstance(s, tuple) else s).name for s, _ in SCRIPTS}
    for want in ("hops", "batch hops", "int16 window", "images", "rights", "ticks", "ticks alternating", "ticks batch",
                 "release", "release and destroy", "recycle: closed"):
        assert want in names, want
    assert {"blocking %s" % h for h in ao.BLOCKING} <= names and {"control %s" % c for c in ao.CONTROLS} <= names
    hops = ao.hops("slide")
    frames = [c.frames(0, 2) for c in hops.calls()]
    assert 0 in frames and 1 in frames and {c.stream for c in hops.calls()} == {"A", "B", "C", "D"}
    assert [c.stream for c in hops.calls() if c.frames(0, 2) == 0] == ["D"]
    batch = ao.batch_hops("period")
    assert batch.n_streams == 40 and all(c.frames(ao.BATCH_IDLE, 2) == 0 for c in batch.calls())
    assert len({c.frames(s, 2) for c in batch.calls() for s in range(40)}) > 40      # ragged
    for c in hops.calls() + batch.calls():
        assert all(n in (0, 1) or 2000 <= n <= 4000 for n in (c.frames(s, 2) for s in range(len(c.xs)))), c
    ticks = ao.ticks("period")
    at = ticks.ops.index(ao.DELAY)
    assert len(ticks.ops) - at - 1 == 128 and all(c.frames(0, 2) == 480 for c in ticks.ops[at + 1:])
    img = ao.images("period")
    kinds = [(c.kind, c.in_fmt, c.out_fmt, c.in_layout, c.out_layout) for c in img.calls()]
    assert {k[0] for k in kinds} == {"sides", "fmt", "mix", "planar_int", "planar_float"}
    assert ("fmt", ao.sf.S24, ao.sf.F32, ao.I, ao.I) in kinds and ("fmt", ao.sf.F32, ao.sf.S16, ao.I, ao.I) in kinds
    sides = [c for c in img.calls() if c.kind == "sides"][0]
    assert (sides.in_layout, sides.out_layout) == (ao.P, ao.I) and sides.in_mix is not None and sides.out_mix is not None
    assert img.dither[0] == ao.dm.TRIANGULAR


@pytest.mark.parametrize("entry", SCRIPTS, ids=[_id(e) for e in SCRIPTS])
def test_every_adjacent_pair_of_every_script_is_sensitive_to_a_stale_state(entry):
    script, how = entry
    if how == "recycle":
        assert ao.recycled_differs(*script), script
        return
    pairs = ao.stale_pairs(script)
    work = [op for op in script.ops if isinstance(op, ao.Call)]
    assert pairs, script
    blind = [(idx, s, script.ops[idx]) for idx, s, differs in pairs if not differs]
    assert not blind, (script, blind)
    # every work call but a stream's first is the second of a judged pair, and every read is judged
    ch = script.filt[0]
    for s in range(script.n_streams):
        judged = {idx for idx, t, _ in pairs if t == s}
        calls = [idx for idx, op in enumerate(script.ops) if isinstance(op, ao.Call) and ao.is_work(op, s, ch)]
        reads = [idx for idx, op in enumerate(script.ops) if isinstance(op, ao.Ctl) and op.op in ("history", "pending")]
        assert judged == set(calls[1:]) | {r for r in reads if calls and r > calls[0]}, (script, s)
    assert len(work) >= 1
