"""Ordering under load: the second half of the device-pointer contract (include/speexhip_resampler.h) -- "the call returns
without waiting for the GPU ... calls on one state are ordered: the next call, on whatever stream, first waits for this one
on the device ... control calls and destroy wait on the host ... d_in must stay valid until the stream has executed the
call" -- with the previous call provably NOT yet run when the next one is made.

The method.  Every scenario puts a DELAY on stream A first: a bounded run of plain device-to-device copies of one large
tensor (never a kernel that waits for the host; DELAY_MS, at most 200 ms), an event right behind it.  Then the whole script
(tests/async_order.py) is issued without any host synchronisation, so every call is enqueued while the first cannot have
started.  Two hard assertions keep a scenario from passing because nothing was in flight:
  1. still in flight -- the event behind the delay is still pending after the script's last non-blocking call (before its
     first blocking call, where it has one);
  2. really concurrent -- two HIP streams on one hardware queue order themselves; the streams A, B, C used here passed a
     probe pair by pair (delay on one, a tiny op on the other, synchronise the other, the delay still pending), chosen from
     at most 8 fresh streams; no concurrent pair = failure, not a skip.
What is compared: in MODE_EXACT every call's bytes, counters and position equal oracle.Oracle's (async_order.Model); in the
default mode the bytes equal those of the same script on a fresh state with a synchronise after every call (default-mode
bytes are a function of the stream alone) and lie within test_gpu_parity's bars of the oracle; after the final
synchronise history, pending frames, position and dither position equal the oracle's.  That each script CAN fail is
tests/test_cpu_async_order.py's business.  Run with -s for the enqueue time and the delay of every script (DESIGN.md,
"Ordering under load")."""
import ctypes as C
import time

import numpy as np
import pytest

import async_order as ao
import speexhip
import test_gpu_parity as par

pytestmark = pytest.mark.gpu

DELAY_MS = 60.0     # >= 10 x the enqueue time of the longest script (1.8 ms measured: DESIGN.md 4a); never above MAX_DELAY_MS
PROBE_MS = 15.0
MAX_DELAY_MS = 200.0
FAMILY_NAMES = list(ao.FAMILIES)


class Rig:
    """the streams and the delay, made once per run of this file"""

    def __init__(self):
        import torch
        self.torch = torch
        self.why = None
        n = 256 << 20
        self.src = torch.ones(n, dtype=torch.uint8, device="cuda")
        self.dst = torch.empty_like(self.src)
        self.tiny = torch.zeros(64, device="cuda")
        self.log = []
        cands = [torch.cuda.Stream() for _ in range(8)]
        # how long one copy takes: warm, then time 16 of them
        with torch.cuda.stream(cands[0]):
            for _ in range(4):
                self.dst.copy_(self.src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(16):
                self.dst.copy_(self.src)
            e1.record()
        torch.cuda.synchronize()
        self.copy_ms = e0.elapsed_time(e1) / 16
        self.last = None
        self.A = cands[0]
        self.B = self.C = self.D = None
        good = []
        for x in cands[1:]:
            if not self.concurrent(self.A, x):
                continue
            for y in good:
                if self.concurrent(y, x):
                    self.B, self.C = y, x
                    break
            if self.B is not None:
                break
            good.append(x)
        if self.B is None:
            self.why = ("no three mutually concurrent streams among 8 fresh ones (%d of 7 run beside the first): every "
                        "pair of streams shares a hardware queue, a missing wait could not show" % len(good))
            return
        self.D = [x for x in cands if x not in (self.A, self.B, self.C)][0]

    def streams(self):
        return {"A": self.A, "B": self.B, "C": self.C, "D": self.D}

    def delay(self, stream, ms=DELAY_MS):
        """`ms` of copies on `stream`; -> the event behind them"""
        torch = self.torch
        copies = max(1, int(np.ceil(ms / self.copy_ms)))
        assert copies * self.copy_ms <= MAX_DELAY_MS, (copies, self.copy_ms)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            start.record()
            for _ in range(copies):
                self.dst.copy_(self.src)
            end.record()
        self.last = (start, end)
        return end

    def delay_ms(self):
        """how long the last delay ran (after a synchronise)"""
        ms = self.last[0].elapsed_time(self.last[1])
        assert ms <= MAX_DELAY_MS, "the delay ran %.1f ms" % ms
        return ms

    def concurrent(self, a, b):
        """does work on b run while a is busy?"""
        torch = self.torch
        torch.cuda.synchronize()
        ev = self.delay(a, PROBE_MS)
        with torch.cuda.stream(b):
            self.tiny.add_(1.0)
        b.synchronize()
        pending = not ev.query()
        torch.cuda.synchronize()
        return pending


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    if r.log:
        worst = max(r.log, key=lambda e: e[1])
        print("\nordering under load: %d delayed scripts, one copy %.3f ms; longest enqueue %.3f ms (%s), its delay %.1f ms; "
              "shortest delay %.1f ms" % (len(r.log), r.copy_ms, worst[1], worst[0], worst[2], min(e[2] for e in r.log)))


# ---- the expected results: once per script -----------------------------------------------------------------------------
_EXPECTED = {}


def expected(script):
    """per op: a Call -> [(consumed, produced, bytes) per stream], a Ctl -> the oracle's answer; and the models at the end"""
    key = (script.name, script.family)
    if key not in _EXPECTED:
        models = [ao.Model(script.filt, script.dither, s) for s in range(script.n_streams)]
        res = []
        for op in script.ops:
            if op == ao.DELAY:
                res.append(None)
            elif isinstance(op, ao.Ctl):
                res.append([m.ctl(op) for m in models][0])
            else:
                res.append([m.run(op, s) for s, m in enumerate(models)])
        _EXPECTED[key] = (res, models)
    return _EXPECTED[key]


# ---- one script on the library -----------------------------------------------------------------------------------------
def make_state(script, mode):
    ch, fi, fo, q = script.filt
    if script.streams is None:
        st = speexhip.Resampler(ch, fi, fo, q, mode=mode)
    else:
        st = speexhip.Batch(script.streams, ch, fi, fo, q, mode=mode)
    if script.dither is not None:
        assert st.set_dither(*script.dither) == 0
    return st


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def issue(st, batch, call, ch, d_in, d_out, g, stream_ptr, scribble):
    """the C call itself on this runner's own argument arrays; scribble: every host argument is overwritten with garbage
    the moment the call has returned.  -> (consumed, produced) per stream"""
    lib = speexhip.lib()
    S = g.streams
    il = (C.c_uint32 * S)(*[call.frames(s, ch) for s in range(S)])
    ol = (C.c_uint32 * S)(*([call.cap] * S))
    mi = None if call.in_mix is None else np.array(call.in_mix, np.float32)
    mo = None if call.out_mix is None else np.array(call.out_mix, np.float32)
    pin, pout, sp, h = C.c_void_p(d_in), C.c_void_p(d_out), C.c_void_p(stream_ptr), st._h
    fi, fo = int(call.in_fmt), int(call.out_fmt)
    a = b = None
    k = call.kind
    if k in ("int", "float"):
        name = "int" if k == "int" else "float"
        if batch:
            rc = getattr(lib, "speexhip_batch_process_interleaved_%s_device" % name)(h, pin, g.in_row, il, pout, g.out_row, ol, sp)
        else:
            rc = getattr(lib, "speexhip_resampler_process_interleaved_%s_device" % name)(h, pin, il, pout, ol, sp)
    elif k in ("planar_int", "planar_float"):
        name = "int" if k == "planar_int" else "float"
        if batch:
            rc = getattr(lib, "speexhip_batch_process_planar_%s_device" % name)(h, pin, g.in_row, g.in_plane, il, pout, g.out_row,
                                                                               g.out_plane, ol, sp)
        else:
            rc = getattr(lib, "speexhip_resampler_process_planar_%s_device" % name)(h, pin, g.in_plane, il, pout, g.out_plane, ol, sp)
    elif k == "fmt":
        if batch:
            rc = lib.speexhip_batch_process_interleaved_fmt_device(h, fi, pin, g.in_row, il, fo, pout, g.out_row, ol, sp)
        else:
            rc = lib.speexhip_resampler_process_interleaved_fmt_device(h, fi, pin, il, fo, pout, ol, sp)
    elif k == "mix":
        if batch:
            rc = lib.speexhip_batch_process_interleaved_mix_device(h, fi, g.n_in, _ptr(mi), pin, g.in_row, il, fo, g.n_out, _ptr(mo),
                                                                   pout, g.out_row, ol, sp)
        else:
            rc = lib.speexhip_resampler_process_interleaved_mix_device(h, fi, g.n_in, _ptr(mi), pin, il, fo, g.n_out, _ptr(mo), pout,
                                                                       ol, sp)
    else:
        assert k == "sides", k
        layout = lambda planar: speexhip.LAYOUT_PLANAR if planar else speexhip.LAYOUT_INTERLEAVED
        a = speexhip.make_side(fi, g.n_in, layout(g.planar_in), mi, d_in, g.in_plane if g.planar_in else 0, g.in_row)
        b = speexhip.make_side(fo, g.n_out, layout(g.planar_out), mo, d_out, g.out_plane if g.planar_out else 0, g.out_row)
        fn = lib.speexhip_batch_process_sides_device if batch else lib.speexhip_resampler_process_sides_device
        rc = fn(h, C.byref(a), il, C.byref(b), ol, sp)
    assert rc == 0, (call, speexhip.strerror(rc))
    used, made = list(il), list(ol)
    if scribble:
        for arr in (il, ol):
            for s in range(S):
                arr[s] = 0xDEADBEEF
        for m in (mi, mo):
            if m is not None:
                m[...] = np.float32(-3.0e38)
        for side in (a, b):
            if side is not None:
                C.memset(C.byref(side), 0xFF, C.sizeof(side))
    return used, made


def issue_host(st, call, ch, idle):
    """one of the blocking host-buffer calls -> (consumed, produced, bytes)"""
    x, cap, host = call.xs[0], call.cap, call.host
    frames = x.reshape(-1, ch) if call.kind != "fmt" else None
    if host == "process":
        out, used = st.process(frames, cap)
    elif host == "process_float":
        out, used = st.process_float(frames, cap)
    elif host == "process_take":
        out, used = st.process_take(frames, cap)
    elif host == "process_chunks":
        half = frames.shape[0] // 2
        outs, useds = st.process_chunks([frames[:half], frames[half:]], [cap, cap])
        out, used = np.concatenate(outs), sum(useds)
    elif host == "process_planar":
        planes, used = st.process_planar(np.ascontiguousarray(frames.T), cap)
        out = np.ascontiguousarray(planes.T)
    elif host == "process_fmt":
        flat, used = st.process_fmt(x, call.in_fmt, call.out_fmt, cap)
        return used, flat.size // (ch * (3 if call.out_fmt == ao.sf.S24 else 1)), flat.view(np.uint8).tobytes()
    else:
        assert host == "process_many", host
        outs, useds, codes = speexhip.process_many([st, idle], [frames, np.zeros((0, ch), np.int16)], [cap, 8])
        assert codes == [0, 0] and useds[1] == 0 and outs[1].shape[0] == 0
        out, used = outs[0], useds[0]
    return used, out.shape[0], out.tobytes()


class Run:
    """a script's state and device buffers; calls are made one by one so that a scenario can put its own steps between"""

    def __init__(self, rig, script, mode, streams=None):
        torch = rig.torch
        self.rig, self.script, self.mode, self.torch = rig, script, mode, torch
        self.ch = script.filt[0]
        self.batch = script.streams is not None
        self.st = make_state(script, mode)
        self.streams = dict(rig.streams(), **(streams or {}))
        self.bufs, self.got = {}, {}
        for idx, op in enumerate(script.ops):
            if isinstance(op, ao.Call) and op.host is None:
                host, g = ao.lay_in(op, self.ch)
                self.bufs[idx] = (torch.from_numpy(host).cuda(),
                                  torch.full((g.out_bytes,), ao.SENTINEL, dtype=torch.uint8, device="cuda"), g)
        self.idle = None
        self.ev = self.t0 = None
        self.checked = False
        torch.cuda.synchronize()

    def delay(self, stream="A"):
        self.torch.cuda.synchronize()
        self.ev = self.rig.delay(self.streams[stream])
        self.t0 = time.perf_counter()

    def in_flight(self):
        """hard assertion 1: made after the last non-blocking call, or right before the first blocking one"""
        if self.ev is None or self.checked:
            return
        pending, dt = not self.ev.query(), (time.perf_counter() - self.t0) * 1e3
        self.checked = True
        self.enqueue_ms = dt
        assert pending, "%s: the delay had run out %.2f ms after it was enqueued: nothing was in flight" % (self.script, dt)

    def call(self, idx, scribble=False, d_in=None, d_out=None):
        op = self.script.ops[idx]
        if op.host is not None:
            self.in_flight()
            if op.host == "process_many" and self.idle is None:
                self.idle = speexhip.Resampler(*self.script.filt, mode=self.mode)
            self.got[idx] = issue_host(self.st, op, self.ch, self.idle)
            return
        din, dout, g = self.bufs[idx]
        used, made = issue(self.st, self.batch, op, self.ch, (d_in if d_in is not None else din).data_ptr(),
                           (d_out if d_out is not None else dout).data_ptr(), g, self.streams[op.stream].cuda_stream, scribble)
        self.got[idx] = (used, made)

    def ctl(self, idx):
        op = self.script.ops[idx]
        if op.op == "release_stream":
            self.st.release_stream()
            self.got[idx] = 0
            return
        self.in_flight()
        self.got[idx] = self.st._lines() if op.op in ("history", "pending") else getattr(self.st, op.op)(*op.args)

    def play(self, ordered=False, scribble=False, start=0):
        """the whole script (from op `start`): ordered = a synchronise after every call and no delay (the default mode's
        second opinion)"""
        for idx, op in enumerate(self.script.ops):
            if idx < start:
                continue
            if op == ao.DELAY:
                if not ordered:
                    self.delay()
            elif isinstance(op, ao.Ctl):
                self.ctl(idx)
            else:
                self.call(idx, scribble)
                if ordered:
                    self.torch.cuda.synchronize()
        return self.finish()

    def finish(self, outputs=None):
        """the in-flight check if no blocking call made it, the final synchronise, the outputs; -> per op results"""
        self.in_flight()
        self.torch.cuda.synchronize()
        if self.ev is not None:
            self.rig.log.append((repr(self.script), self.enqueue_ms, self.rig.delay_ms()))
            print("%s: enqueued in %.3f ms behind a delay of %.1f ms" % (self.script, self.enqueue_ms, self.rig.log[-1][2]))
        res = []
        for idx, op in enumerate(self.script.ops):
            if idx not in self.got:
                res.append(None)
            elif isinstance(op, ao.Call) and op.host is None:
                used, made = self.got[idx]
                raw = (outputs[idx] if outputs is not None else self.bufs[idx][1]).cpu().numpy()
                outs, clean = ao.take_out(self.bufs[idx][2], raw, made)
                assert clean, (self.script, idx, "bytes beyond the produced frames were written")
                res.append([(used[s], made[s], outs[s]) for s in range(len(outs))])
            elif isinstance(op, ao.Call):
                res.append([self.got[idx]])
            else:
                res.append(self.got[idx])
        return res

    def lines(self, s):
        return self.st.lines(s) if self.batch else self.st._lines()

    def position(self, s):
        if self.batch:
            i = self.st.info(s)
            return i["last_sample"], i["samp_frac_num"]
        return self.st.position()

    def close(self):
        self.st.close()
        if self.idle is not None:
            self.idle.close()


def judge(run, got, second=None):
    """every op's result against the oracle's (and, in the default mode, against the ordered second run), then the state"""
    script, mode = run.script, run.mode
    want, models = expected(script)
    bar = ao.float_bar(script)
    for idx, op in enumerate(script.ops):
        tag = "%s op %d %s" % (script, idx, op)
        if op == ao.DELAY:
            continue
        if isinstance(op, ao.Ctl):
            if op.op in ("history", "pending"):
                assert got[idx].shape == want[idx].shape and np.array_equal(got[idx], want[idx]), tag
            else:
                assert got[idx] == want[idx], (tag, got[idx], want[idx])
            continue
        for s, ((used, made, data), (w_used, w_made, w_data)) in enumerate(zip(got[idx], want[idx])):
            assert (used, made) == (w_used, w_made), (tag, s, used, made, w_used, w_made)
            if mode == speexhip.MODE_EXACT:
                assert data == w_data, "%s stream %d: bytes differ from the oracle's" % (tag, s)
            else:
                assert second is not None
                assert data == second[idx][s][2], "%s stream %d: bytes differ from the ordered run's" % (tag, s)
                ao.close_to_oracle(op.out_fmt, data, w_data, bar, par.assert_close, "%s stream %d" % (tag, s))
    for s, m in enumerate(models):
        assert run.position(s) == m.position(), (script, s, run.position(s), m.position())
        lines = run.lines(s)
        assert lines.shape == m.lines().shape and np.array_equal(lines, m.lines()), (script, s, "history / pending frames")
        if script.dither is not None:
            assert run.st.get_dither(*([s] if run.batch else []))[2] == m.pos, (script, s, "dither position")


def fast_path_of(run):
    return (run.st.info(0) if run.batch else run.st.info())["fast_path"]


def go(rig, script, scribble=False):
    """the standard scenario: the script behind the delay, judged; in the default mode also played in order"""
    assert rig.why is None, rig.why     # hard assertion 2
    mode = script.mode
    second = None
    if mode != speexhip.MODE_EXACT:
        ordered = Run(rig, script, mode)
        second = ordered.play(ordered=True)
        ordered.close()
    run = Run(rig, script, mode)
    if script.family in ao.FAMILIES:
        assert fast_path_of(run) == ao.FAMILIES[script.family][4], (script, fast_path_of(run))
    got = run.play(scribble=scribble)
    judge(run, got, second)
    run.close()


# ---- 1. stream hops, one state -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_stream_hops_on_one_state(rig, family):
    go(rig, ao.hops(family))


# ---- 2. stream hops, batches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_stream_hops_of_a_batch_of_two_launches(rig, family):
    go(rig, ao.batch_hops(family))


def test_a_call_behind_a_launch_over_the_int16_window(rig):
    ch, fi, fo, q, streams, frames = ao.INT16_WINDOW
    probe = speexhip.Resampler(ch, fi, fo, q)
    info = probe.info()
    probe.close()
    assert speexhip.debug_launch_shape(info["num_rate"], info["den_rate"], q, ch, streams, frames)["int16_window"]
    go(rig, ao.int16_window())


# ---- 3. shared images --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [None, 3], ids=["resampler", "batch"])
@pytest.mark.parametrize("family", ao.IMAGE_FAMILIES)
def test_calls_that_share_the_state_s_images(rig, family, streams):
    go(rig, ao.images(family, streams))


# ---- 4. the caller's rights, in stream order ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_caller_reuses_its_buffers_in_stream_order(rig, family):
    """one input and one output buffer for every call: behind each call, on its stream, the output is copied away and the
    next chunk copied over the input"""
    assert rig.why is None, rig.why
    torch = rig.torch
    script = ao.rights(family)

    def play(ordered):
        run = Run(rig, script, script.mode)
        calls = [i for i, op in enumerate(script.ops) if isinstance(op, ao.Call)]
        d_in = torch.zeros(max(run.bufs[i][2].in_bytes for i in calls), dtype=torch.uint8, device="cuda")
        d_out = torch.full((max(run.bufs[i][2].out_bytes for i in calls),), ao.SENTINEL, dtype=torch.uint8, device="cuda")
        saved = {i: torch.empty(run.bufs[i][2].out_bytes, dtype=torch.uint8, device="cuda") for i in calls}
        d_in[: run.bufs[calls[0]][2].in_bytes].copy_(run.bufs[calls[0]][0])
        torch.cuda.synchronize()
        if not ordered:
            run.delay()
        for n, i in enumerate(calls):
            run.call(i, d_in=d_in, d_out=d_out)
            with torch.cuda.stream(rig.A):
                saved[i].copy_(d_out[: saved[i].numel()])
                d_out.fill_(ao.SENTINEL)
                if n + 1 < len(calls):
                    nxt = run.bufs[calls[n + 1]][0]
                    d_in[: nxt.numel()].copy_(nxt)
            if ordered:
                torch.cuda.synchronize()
        return run, run.finish(outputs=saved)

    second = None
    if script.mode != speexhip.MODE_EXACT:
        ordered, second = play(True)
        ordered.close()
    run, got = play(False)
    judge(run, got, second)
    run.close()


# ---- 5. host arguments die at return -----------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [None, 3], ids=["resampler", "batch"])
@pytest.mark.parametrize("family", ao.IMAGE_FAMILIES)
def test_host_arguments_may_be_overwritten_when_the_call_has_returned(rig, family, streams):
    """lengths, capacities, matrices and Side structures (a Batch's per-stream arrays) turn to garbage while the call they
    were given to has not run"""
    go(rig, ao.images(family, streams), scribble=True)


def test_host_arguments_of_a_batch_of_two_launches(rig):
    go(rig, ao.batch_hops("period"), scribble=True)


# ---- 6. many calls, no sync --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one stream", "two streams", "batch of 8"])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_128_ticks_without_a_synchronise(rig, family, shape):
    go(rig, ao.ticks(family, alternate=shape == "two streams", streams=8 if shape == "batch of 8" else None))


# ---- 7. a blocking call behind an in-flight one ------------------------------------------------------------------------
@pytest.mark.parametrize("host", ao.BLOCKING)
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_a_blocking_call_behind_a_call_in_flight(rig, family, host):
    """A host-buffer call runs on a stream of the library's own (one of four that its states share in turn), which no
    probe from outside can reach.  So the script's first call -- the same kind of call, before the delay -- is the probe:
    made behind a delay on A, it must return with that delay still pending; a state whose stream shares A's
    hardware queue is dropped for the next one."""
    assert rig.why is None, rig.why
    torch = rig.torch
    script = ao.blocking(family, host)
    assert script.ops[0].host == host and script.ops[1] == ao.DELAY
    second = None
    if script.mode != speexhip.MODE_EXACT:
        ordered = Run(rig, script, script.mode)
        second = ordered.play(ordered=True)
        ordered.close()
    beside = False
    for _ in range(4):
        run = Run(rig, script, script.mode)
        torch.cuda.synchronize()
        ev = rig.delay(rig.A)
        t0 = time.perf_counter()
        run.call(0)
        beside = not ev.query()
        print("%s: the probe call took %.2f ms, the delay behind it is %s" % (script, (time.perf_counter() - t0) * 1e3,
                                                                              "still pending" if beside else "over"))
        if beside:
            break
        torch.cuda.synchronize()
        run.close()
    assert beside, "%s: none of 4 fresh states runs its host-buffer calls beside stream A" % script
    got = run.play(start=1)
    judge(run, got, second)
    run.close()


# ---- 8. control calls behind an in-flight call -------------------------------------------------------------------------
@pytest.mark.parametrize("what", ao.CONTROLS)
@pytest.mark.parametrize("family", ao.IMAGE_FAMILIES)
def test_a_control_call_behind_a_call_in_flight(rig, family, what):
    go(rig, ao.control(family, what))


# ---- 9. release_stream under load --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_release_stream_under_load(rig, family):
    """every call's stream handed back at once, the next call elsewhere, nobody synchronises"""
    go(rig, ao.release(family, False))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_release_stream_then_destroy_under_load(rig, family):
    """the call runs on a stream of its own that is released and destroyed while the call is in flight; the next call runs
    on B.  (hipStreamDestroy may wait for the stream: the in-flight check is made right before it.)"""
    assert rig.why is None, rig.why
    torch = rig.torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    script = ao.release(family, True)
    second = None
    if script.mode != speexhip.MODE_EXACT:
        ordered = Run(rig, script, script.mode, {"X": rig.A})
        second = ordered.play(ordered=True)
        ordered.close()
    raw, x = None, None
    for _ in range(4):     # a fresh stream that runs beside B
        raw = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(raw)) == 0
        x = torch.cuda.ExternalStream(raw.value)
        if rig.concurrent(x, rig.B):
            break
        assert hip.hipStreamDestroy(raw) == 0
        raw = None
    assert raw is not None, "no fresh stream runs beside stream B: a missing wait could not show"
    run = Run(rig, script, script.mode, {"X": x})
    at = script.ops.index(ao.DELAY)
    run.delay("X")
    run.call(at + 1)
    run.ctl(at + 2)
    run.in_flight()
    assert hip.hipStreamDestroy(raw) == 0
    print("%s: the delay is %s after hipStreamDestroy" % (script, "done" if run.ev.query() else "still pending"))
    run.call(at + 3)
    got = run.finish()
    judge(run, got, second)
    run.close()


# ---- 10. destroy and recycle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_a_state_made_from_the_buffers_of_one_closed_in_flight_starts_from_silence(rig, family):
    assert rig.why is None, rig.why
    closed, fresh = ao.recycle(family)
    second = None
    if fresh.mode != speexhip.MODE_EXACT:
        ordered = Run(rig, fresh, fresh.mode)
        second = ordered.play(ordered=True)
        ordered.close()
    speexhip.lib().speexhip_release_cached_memory()    # (the pool holds nothing but what the closed state hands back)
    old = Run(rig, closed, closed.mode)
    old.delay()
    old.call(closed.ops.index(ao.DELAY) + 1)
    old.in_flight()         # close() waits on the host: the check comes first
    old.st.close()
    new = Run(rig, fresh, fresh.mode)
    new.call(fresh.ops.index(ao.DELAY) + 1)
    got = new.finish()
    old.finish()
    judge(new, got, second)
    new.close()
