"""Ordering under load: the scripts of tests/test_gpu_async_order.py, their oracle model and the proof that every one of
them can fail (tests/test_cpu_async_order.py).  Nothing here needs a GPU.

The contract (include/speexhip_resampler.h, the device-pointer calls): a call returns without waiting for the GPU; calls on
one state are ordered -- the next call, on whatever stream, first waits for this one on the device; control calls, the
history read and destroy wait for the state's last call on the host; the caller's host arguments are dead at return.

A SCRIPT is a list of ops on one state (a Resampler, or a Batch of `streams` streams):
  DELAY            where the GPU runner puts the delay on stream A (every op behind it is issued while it is pending)
  Call             a sample call: device-pointer (on the stream labelled A / B / C / D / X) or, with host=..., one of the
                   blocking host-buffer calls
  Ctl              a control call or a state read
What a call must produce comes from oracle.Oracle alone (Model below): the int16 and float entry points as they are, the
formatted / mixed / sides calls as the float call between sample_formats, channel_mix and dither_model.

"Can fail": for every adjacent pair of work calls (N, N+1) `stale_pairs` builds the state "everything as after N, history
as it was before N" -- what call N+1 reads when it does not wait for call N: the host's bookkeeping is always current, the
device's buffers are not -- on a copy of the oracle's state (Oracle.clone, Oracle.set_lines), and the stale outcome of N+1
must differ from the correct one."""
import numpy as np

import channel_mix as cm
import dither_model as dm
import oracle as orc
import sample_formats as sf

MODE_EXACT = 1
SENTINEL = 0xA5
I, P = "interleaved", "planar"

# one filter per kernel family: (channels, in, out, quality, info()["fast_path"], mode; None = the default mode)
FAMILIES = {
    "period": (2, 44100, 48000, 7, 2, None),
    "slide": (2, 48000, 8000, 7, 3, None),
    "fp64-slide": (1, 24000, 48000, 10, 4, None),
    "fp64-period": (2, 44100, 48000, 10, 5, None),
    "folded": (2, 56000, 48000, 4, 2, None),          # a row of test_gpu_parity.FOLDED_CASES
    "exact-fallback": (2, 192000, 1000, 8, 0, None),  # a row of test_gpu_parity.EXACT_FALLBACK_CASES (without its length)
    "period-exact": (2, 44100, 48000, 7, 2, MODE_EXACT),
}
IMAGE_FAMILIES = ("period", "fp64-period", "period-exact")   # scenarios about images or control calls
INT16_WINDOW = (2, 48000, 11025, 7, 32, 65536)               # channels, in, out, quality, streams, frames

# Float outputs against the oracle in the default mode, as a fraction of the largest sample in the window -- here full
# scale, in int16 units: the samples are full-scale noise.  test_gpu_parity's bars: 2e-6 where it names the filter
# (test_float_entry_point_exact_and_fast, test_mid_stream_control_scripts_fast_mode: the period kernel's 44.1k -> 48k), 4e-6
# for the folded view's float call and for "any rate, any quality" (test_random_control_soak_against_the_oracle), which is
# what the slide family's 768 taps and the filters a control script changes to come under.
FLOAT_BAR = {"folded": 4e-6, "slide": 4e-6}
FLOAT_BAR_DEFAULT = 2e-6
FULL_SCALE = 32768.0


def float_bar(script):
    if script.name.startswith("control"):
        return 4e-6
    return FLOAT_BAR.get(script.family, FLOAT_BAR_DEFAULT)

DELAY = "delay"
DITHER = (dm.TRIANGULAR, 77, 5)


def wcap(frames, fi, fo):
    return int(np.ceil(frames * fo / fi)) + 8


def pcm(frames, ch, seed):
    """full-scale white noise: no window of it is silent"""
    return orc.lcg_pcm(frames * ch, seed).reshape(frames, ch)


def floats(frames, ch, seed):
    """float samples in int16 units that are no integers"""
    return pcm(frames, ch, seed).astype(np.float32) * np.float32(0.999)


def matrix(rows, cols, seed):
    """a mix matrix whose rows have absolute sum 1: full-scale frames stay inside full scale"""
    m = np.random.RandomState(seed).uniform(-1.0, 1.0, (rows, cols))
    return (m / np.abs(m).sum(axis=1, keepdims=True)).astype(np.float32)


class Ctl:
    def __init__(self, op, *args):
        self.op, self.args = op, args

    def __repr__(self):
        return "Ctl(%s%s)" % (self.op, self.args)


class Call:
    """kind: int | float (the interleaved entry points), planar_int | planar_float, fmt | mix | sides.  xs: one flat storage
    array of whole interleaved frames per stream (a planar side is laid out by the runner); cap: frames of room."""

    def __init__(self, kind, xs, cap, stream="A", in_fmt=None, out_fmt=None, in_mix=None, out_mix=None, in_layout=I,
                 out_layout=I, host=None):
        self.kind, self.cap, self.stream, self.host = kind, int(cap), stream, host
        self.xs = [np.ascontiguousarray(x).reshape(-1) for x in (xs if isinstance(xs, list) else [xs])]
        self.in_mix, self.out_mix = in_mix, out_mix
        if kind in ("int", "planar_int"):
            in_fmt = out_fmt = sf.S16
        elif kind in ("float", "planar_float"):
            in_fmt = out_fmt = sf.F32
        if kind.startswith("planar"):
            in_layout = out_layout = P
        self.in_fmt, self.out_fmt, self.in_layout, self.out_layout = in_fmt, out_fmt, in_layout, out_layout
        self.entry = "int" if kind in ("int", "planar_int") else "float" if kind in ("float", "planar_float") else "image"

    def channels_in(self, ch):
        return ch if self.in_mix is None else self.in_mix.shape[1]

    def channels_out(self, ch):
        return ch if self.out_mix is None else self.out_mix.shape[0]

    def frames(self, s, ch):
        return sf.samples_in(self.in_fmt, self.xs[s]) // self.channels_in(ch)

    def __repr__(self):
        return "Call(%s%s on %s)" % (self.kind, " via %s" % self.host if self.host else "", self.stream)


class Script:
    def __init__(self, name, family, ops, streams=None, dither=None, filt=None):
        self.name, self.family, self.ops, self.streams, self.dither = name, family, ops, streams, dither
        self.filt = filt if filt is not None else FAMILIES[family][:4]
        self.mode = FAMILIES[family][5] if family in FAMILIES else None
        if DELAY not in ops:
            self.ops = [DELAY] + list(ops)

    @property
    def n_streams(self):
        return 1 if self.streams is None else self.streams

    def calls(self):
        return [op for op in self.ops if isinstance(op, Call)]

    def __repr__(self):
        return "Script(%s, %s)" % (self.name, self.family)


# ---- the oracle's statement of a call ----------------------------------------------------------------------------------
class Model:
    """one stream of a state: oracle.Oracle plus the dither position of the formatted calls"""

    def __init__(self, filt, dither=None, stream=0):
        self.filt, self.ch = filt, filt[0]
        self.o = orc.Oracle(*filt)
        kind, seed, pos = dither if dither is not None else (dm.NONE, 0, 0)
        self.kind, self.seed, self.pos = kind, dm.stream_seed(seed, stream), pos

    def run(self, call, s=0):
        """-> (consumed, produced, the produced frames as interleaved bytes of the output format)"""
        x, o, ch = call.xs[s], self.o, self.ch
        if call.host == "process_chunks":   # two consecutive int16 calls, as one launch
            half = (x.size // ch // 2) * ch
            ya, ua = o.process(x[:half].reshape(-1, ch), call.cap)
            yb, ub = o.process(x[half:].reshape(-1, ch), call.cap)
            return ua + ub, ya.shape[0] + yb.shape[0], ya.tobytes() + yb.tobytes()
        if call.entry == "int":
            y, used = o.process(x.reshape(-1, ch), call.cap)
            out = y.tobytes()
        elif call.entry == "float":
            y, used = o.process_float(x.reshape(-1, ch), call.cap)
            out = y.tobytes()
        else:
            xf = sf.to_internal(call.in_fmt, x)
            xf = cm.mix(call.in_mix, xf) if call.in_mix is not None else xf.reshape(-1, ch)
            y, used = o.process_float(xf, call.cap)
            z = cm.mix(call.out_mix, y) if call.out_mix is not None else y
            flat = np.ascontiguousarray(z).reshape(-1)
            out = dm.from_internal(call.out_fmt, flat, self.kind, self.seed, self.pos, z.shape[1]).view(np.uint8).tobytes()
            if self.kind != dm.NONE:
                self.pos += y.shape[0]
        return used, y.shape[0], out

    def ctl(self, op):
        """a control call on the oracle -> its return value (history / pending: the lines)"""
        if op.op in ("history", "pending"):
            return self.lines()
        if op.op == "release_stream":   # (the state's own bookkeeping: nothing the reference knows of)
            return 0
        return getattr(self.o, op.op)(*op.args)

    def position(self):
        return self.o.position()

    def lines(self):
        """(taps - 1 + pending, channels): what speexhip's _lines() / Batch.lines() return"""
        cols = [np.concatenate([self.o.history(c), self.o.pending(c)]) for c in range(self.ch)]
        return np.stack(cols, axis=1)

    def with_lines(self, lines):
        """a copy of this state -- positions, counts, filter, dither position -- over other lines: the state a call meets
        that reads what an earlier call left"""
        m = object.__new__(Model)
        m.filt, m.ch, m.kind, m.seed, m.pos = self.filt, self.ch, self.kind, self.seed, self.pos
        m.o = self.o.clone()
        for c in range(self.ch):
            m.o.set_lines(c, lines[:, c])
        return m


def is_work(call, s, ch):
    """a call that enqueues something for stream s (an empty call, or one without room, touches nothing)"""
    return call.frames(s, ch) != 0 and call.cap != 0


def stale_pairs(script):
    """For every adjacent pair of work calls (N, N+1) of the script, per stream: (index of N+1 among the ops, stream,
    differs).  `differs`: call N+1 made on "everything as after call N, but the lines -- history and pending frames -- as
    they were before call N" comes out different from the correct call N+1 (its produced bytes; the lines it leaves where
    it produces nothing), AND so does the same with the lines as they were before call N-1, which is what the history
    ping-pong's other buffer holds while call N has not run.  A control op between N and N+1 is made on the stale states
    too, and a read (history, pending) must itself differ there: its own entry.  reset_mem is the other way round -- the
    late call N writes its history after the reset -- so its stale state is the reset state over the lines call N left."""
    out = []
    for s in range(script.n_streams):
        m = Model(script.filt, script.dither, s)
        twins, older = [], None     # older: the lines before the last work call
        for idx, op in enumerate(script.ops):
            if op == DELAY:
                continue
            if isinstance(op, Ctl):
                if op.op == "reset_mem":
                    left = m.lines()
                    m.ctl(op)
                    twins = [m.with_lines(left)] if twins else []
                    continue
                want = m.ctl(op)
                got = [t.ctl(op) for t in twins]
                if op.op in ("history", "pending") and twins:
                    out.append((idx, s, all(g.shape != want.shape or not np.array_equal(g, want) for g in got)))
                continue
            if not is_work(op, s, m.ch):
                continue
            before = m.lines()
            stale = [(t.run(op, s), t.lines()) for t in twins]
            used, made, data = m.run(op, s)
            after = m.lines()
            if twins:
                out.append((idx, s, all((d != data) if made else not np.array_equal(ln, after) for (_, _, d), ln in stale)))

            def fit(lines):   # (the rows this state's lines hold now)
                res = np.zeros_like(after)
                k = min(res.shape[0], lines.shape[0])
                res[:k] = lines[:k]
                return res
            twins = [m.with_lines(fit(before))] + ([m.with_lines(fit(older))] if older is not None else [])
            older = before
    return out


def recycled_differs(closed, fresh):
    """10.: the first call of a fresh state must differ when the closed state's late call leaves its history (or its call's
    input history ping-pong) in the recycled buffers"""
    a = Model(closed.filt)
    a.run(closed.calls()[0])
    m = Model(fresh.filt)
    t = m.with_lines(a.lines())
    call = fresh.calls()[0]
    return t.run(call)[2] != m.run(call)[2]


def close_to_oracle(fmt, got, want, bar, assert_close, name):
    """default-mode bytes against the oracle's: int16 by test_gpu_parity.assert_close, float samples within `bar` of full
    scale; another integer format holds the same FIR value at 2^k steps per int16 step, so it may differ by the float bar
    in its own steps plus one for the rounding"""
    assert len(got) == len(want), name
    if fmt == sf.S16:
        assert_close(np.frombuffer(got, np.int16), np.frombuffer(want, np.int16), name)
    elif fmt in (sf.F32, sf.F32N):
        g, w = np.frombuffer(got, np.float32).astype(np.float64), np.frombuffer(want, np.float32).astype(np.float64)
        lim = bar * (FULL_SCALE if fmt == sf.F32 else 1.0)
        assert np.abs(g - w).max(initial=0.0) <= lim, "%s: %.3g > %.3g" % (name, np.abs(g - w).max(), lim)
    else:
        g, w = (sf.integers(fmt, np.frombuffer(b, sf.DTYPE[fmt])) for b in (got, want))
        lim = int(np.ceil(bar * FULL_SCALE * sf._INT[fmt][0])) + 1
        assert np.abs(g - w).max(initial=0) <= lim, "%s: %d > %d steps" % (name, np.abs(g - w).max(), lim)


# ---- device buffers of a call: numpy only, so that the layout is checked without a GPU --------------------------------
class Geometry:
    """strides in samples of the side's format: a stream's row, a plane inside it (planar sides), and the output's bytes"""


def geometry(call, ch):
    g = Geometry()
    g.streams = len(call.xs)
    g.n_in, g.n_out = call.channels_in(ch), call.channels_out(ch)
    g.bi, g.bo = sf.BYTES[call.in_fmt], sf.BYTES[call.out_fmt]
    g.in_plane = max(max(call.frames(s, ch) for s in range(g.streams)), 1)
    g.in_row = g.in_plane * g.n_in + 3            # (odd rows: the streams of a batch lie at every alignment)
    g.out_plane = max(call.cap, 1) + 1
    g.out_row = g.out_plane * g.n_out + 5
    g.planar_in = call.in_layout == P and g.n_in > 1
    g.planar_out = call.out_layout == P and g.n_out > 1
    g.in_bytes, g.out_bytes = g.streams * g.in_row * g.bi, g.streams * g.out_row * g.bo
    return g


def lay_in(call, ch):
    """-> (the input buffer of all streams as bytes, its Geometry)"""
    g = geometry(call, ch)
    host = np.zeros((g.streams, g.in_row * g.bi), np.uint8)
    for s, x in enumerate(call.xs):
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        frames = call.frames(s, ch)
        if g.planar_in:
            planes = raw.reshape(frames, g.n_in, g.bi).transpose(1, 0, 2).reshape(g.n_in, frames * g.bi)
            for c in range(g.n_in):
                host[s, c * g.in_plane * g.bi: c * g.in_plane * g.bi + frames * g.bi] = planes[c]
        else:
            host[s, : raw.size] = raw
    return host.reshape(-1), g


def take_out(g, raw, made):
    """the output buffer's bytes -> (per stream: the produced frames as interleaved bytes, whether every other byte still
    holds SENTINEL)"""
    rows = np.asarray(raw, np.uint8).reshape(g.streams, g.out_row * g.bo)
    outs, untouched = [], np.ones(rows.shape, bool)
    for s in range(g.streams):
        n = int(made[s])
        if g.planar_out:
            planes = []
            for c in range(g.n_out):
                at = c * g.out_plane * g.bo
                planes.append(rows[s, at: at + n * g.bo].reshape(n, g.bo))
                untouched[s, at: at + n * g.bo] = False
            outs.append(np.stack(planes, axis=1).tobytes())
        else:
            outs.append(rows[s, : n * g.n_out * g.bo].tobytes())
            untouched[s, : n * g.n_out * g.bo] = False
    return outs, bool((rows[untouched] == SENTINEL).all())


# ---- the scripts -------------------------------------------------------------------------------------------------------
def _fam(family):
    ch, fi, fo, q = FAMILIES[family][:4]
    return ch, fi, fo, q


def hops(family):
    """1. stream hops, one state: int16 and float calls A -> B -> A -> C, an empty call on a fourth stream and a 1-frame call
    in between"""
    ch, fi, fo, q = _fam(family)
    c = lambda n: wcap(n, fi, fo)
    return Script("hops", family, [
        Call("int", pcm(3000, ch, 11), c(3000), "A"),
        Call("float", floats(2500, ch, 12), c(2500), "B"),
        Call("int", pcm(0, ch, 13), 64, "D"),
        Call("int", pcm(1, ch, 14), 8, "A"),
        Call("float", floats(3500, ch, 15), c(3500), "C"),
        Call("int", pcm(2000, ch, 16), c(2000), "B"),
        Call("float", floats(1, ch, 17), 8, "A"),
        Call("int", pcm(4000, ch, 18), c(4000), "C"),
    ])


BATCH_STREAMS, BATCH_IDLE = 40, 17


def _ragged(kind, base, ch, seed, streams=BATCH_STREAMS, idle=BATCH_IDLE, step=37):
    gen = pcm if kind == "int" else floats
    return [gen(0 if s == idle else base - step * s, ch, seed + s) for s in range(streams)]


def batch_hops(family):
    """2. stream hops, a batch of 40 (launches of 32 + 8), ragged lengths, one idle stream, A -> B -> A"""
    ch, fi, fo, q = _fam(family)
    return Script("batch hops", family, [
        Call("int", _ragged("int", 4000, ch, 100), wcap(4000, fi, fo), "A"),
        Call("float", _ragged("float", 3600, ch, 200), wcap(3600, fi, fo), "B"),
        Call("int", _ragged("int", 3800, ch, 300), wcap(3800, fi, fo), "A"),
    ], streams=BATCH_STREAMS)


def int16_window():
    """2. a launch that takes the int16 window, followed by a call on B"""
    ch, fi, fo, q, streams, frames = INT16_WINDOW
    return Script("int16 window", None, [
        Call("int", [pcm(frames, ch, 400 + s) for s in range(streams)], wcap(frames, fi, fo), "A"),
        Call("int", [pcm(3000 - 11 * s, ch, 500 + s) for s in range(streams)], wcap(3000, fi, fo), "B"),
    ], streams=streams, filt=(ch, fi, fo, q))


def _storage(fmt, frames, n_ch, seed):
    """full-scale noise in any of the formats used here"""
    x = pcm(frames, n_ch, seed).reshape(-1)
    if fmt == sf.S16:
        return x
    if fmt == sf.S24:
        return sf.pack_s24(x.astype(np.int64) * 256 + (np.arange(x.size) % 251))
    if fmt in (sf.F32, sf.F32N):
        v = x.astype(np.float32) * np.float32(0.999)
        return v if fmt == sf.F32 else v / np.float32(32768.0)
    raise ValueError(fmt)


def images(family, streams=None, large=4000, small=300):
    """3. shared images: planar, formatted, mixed and sides calls, a large call on A, a small one on B, then small and
    large on C; an input-pass-only call (interleaved F32 out), an output-pass-only call (interleaved F32 in); triangular
    dither on"""
    ch, fi, fo, q = _fam(family)
    n = 1 if streams is None else streams
    m_in3, m_out3 = matrix(ch, 3, 1), matrix(3, ch, 2)
    m_in6, m_out1 = matrix(ch, 6, 3), matrix(1, ch, 4)

    def xs(fmt, frames, n_ch, seed):
        return [_storage(fmt, frames - 53 * s, n_ch, seed + s) for s in range(n)]

    c = lambda f: wcap(f, fi, fo)
    return Script("images%s" % (" batch" if streams else ""), family, [
        Call("sides", xs(sf.S16, large, 3, 600), c(large), "A", sf.S16, sf.S16, m_in3, m_out3, P, I),
        Call("fmt", xs(sf.S24, small, ch, 610), c(small), "B", sf.S24, sf.F32),                 # input pass only
        Call("mix", xs(sf.S16, small, 6, 620), c(small), "C", sf.S16, sf.F32N, m_in6, None),
        Call("fmt", xs(sf.F32, large, ch, 630), c(large), "C", sf.F32, sf.S16),                 # output pass only
        Call("planar_int", xs(sf.S16, 2500, ch, 640), c(2500), "A"),
        Call("mix", xs(sf.F32N, small, ch, 650), c(small), "B", sf.F32N, sf.U8, None, m_out1),
        Call("planar_float", xs(sf.F32, 2000, ch, 660), c(2000), "C"),
        Call("sides", xs(sf.S24, large, 3, 670), c(large), "A", sf.S24, sf.S24, m_in3, m_out3, P, I),
    ], streams=streams, dither=DITHER)


def rights(family):
    """4. the caller's rights, in stream order: one stream, one input and one output buffer for all calls"""
    ch, fi, fo, q = _fam(family)
    ops = []
    for k in range(6):
        n = 3000 + 100 * k
        ops.append(Call("int", pcm(n, ch, 700 + k), wcap(n, fi, fo), "A") if k % 2 == 0 else
                   Call("float", floats(n, ch, 700 + k), wcap(n, fi, fo), "A"))
    return Script("rights", family, ops)


TICKS, TICK, WARM = 128, 480, 16384


def ticks(family, alternate=False, streams=None):
    """6. many calls, no sync: 128 back-to-back calls of 480 frames (10 ms at 48 kHz) on one stream or alternating between
    two, int16 and float in turn.  One call comes first, before the delay: on the longest filter here (30 720 taps) the first
    ticks of a stream lie so far out on the filter's skirt that a float call cannot tell one history from another."""
    ch, fi, fo, q = _fam(family)
    n = 1 if streams is None else streams
    ops = [Call("int", [pcm(WARM, ch, 990 + s) for s in range(n)], wcap(WARM, fi, fo), "A"), DELAY]
    for k in range(TICKS):
        kind = "int" if k % 2 == 0 else "float"
        gen = pcm if kind == "int" else floats
        ops.append(Call(kind, [gen(TICK, ch, 1000 + 16 * k + s) for s in range(n)], wcap(TICK, fi, fo),
                        "B" if alternate and k % 2 else "A"))
    return Script("ticks%s%s" % (" alternating" if alternate else "", " batch" if streams else ""), family, ops, streams=streams)


BLOCKING = ("process", "process_float", "process_chunks", "process_take", "process_planar", "process_fmt", "process_many")


def blocking(family, host):
    """7. a blocking call behind an in-flight one.  The same kind of call comes first, before the delay, and larger: it
    grows whatever the call grows on first use (a grow waits for the state on the host, which would hide a missing device
    wait), and it is the GPU runner's probe that this state's own stream runs beside stream A."""
    ch, fi, fo, q = _fam(family)

    def host_call(n, seed):
        if host == "process_float":
            return Call("float", floats(n, ch, seed), wcap(n, fi, fo), host=host)
        if host == "process_fmt":
            return Call("fmt", _storage(sf.S24, n, ch, seed), wcap(n, fi, fo), in_fmt=sf.S24, out_fmt=sf.F32N, host=host)
        return Call("planar_int" if host == "process_planar" else "int", pcm(n, ch, seed), wcap(n, fi, fo), host=host)

    return Script("blocking %s" % host, family, [host_call(3500, 799), DELAY,
                                                 Call("float", floats(3000, ch, 800), wcap(3000, fi, fo), "A"),
                                                 host_call(2500, 801)])


CONTROLS = ("set_quality", "set_rate_frac", "reset_mem", "skip_zeros", "history", "pending")


def control(family, what):
    """8. a control call behind an in-flight call, then a device call on B"""
    ch, fi, fo, q = _fam(family)
    pre, cap = [], wcap(3000, fi, fo)
    if what == "pending":
        # pending frames exist after a filter got shorter; a call whose capacity binds leaves some of them behind
        pre, cap = [Call("int", pcm(3000, ch, 900), wcap(3000, fi, fo), "A"), Ctl("set_quality", q - 3)], 8
    op = {"set_quality": Ctl("set_quality", q - 2), "set_rate_frac": Ctl("set_rate_frac", 3, 2, 48000, 32000),
          "reset_mem": Ctl("reset_mem"), "skip_zeros": Ctl("skip_zeros"), "history": Ctl("history"),
          "pending": Ctl("pending")}[what]
    return Script("control %s" % what, family, pre + [
        DELAY,
        Call("int", pcm(3000, ch, 901), cap, "A"),
        op,
        Call("float", floats(2500, ch, 902), wcap(2500, 2, 3), "B"),   # (room for any of the ratios above)
    ])


def release(family, destroy):
    """9. release_stream under load: every call's stream is handed back at once (destroy: and destroyed, each call on a
    stream of its own, labelled X) and the next call runs elsewhere; a control call and a host-buffer call in between, as in
    test_a_caller_may_destroy_the_stream_of_a_device_pointer_call_after_release_stream"""
    ch, fi, fo, q = _fam(family)
    c = lambda n: wcap(n, fi, fo)
    if destroy:
        return Script("release and destroy", family, [
            Call("int", pcm(3000, ch, 950), c(3000), "X"), Ctl("release_stream"),
            Call("float", floats(2500, ch, 951), c(2500), "B"),
        ])
    return Script("release", family, [
        Call("int", pcm(3000, ch, 950), c(3000), "A"), Ctl("release_stream"),
        Call("float", floats(2500, ch, 951), c(2500), "B"), Ctl("release_stream"),
        Call("int", pcm(2000, ch, 952), c(2000), "A"), Ctl("release_stream"),
        Call("int", pcm(2200, ch, 953), c(2200), host="process"),
        Call("float", floats(2100, ch, 954), c(2100), "B"), Ctl("release_stream"),
        Ctl("set_quality", q - 2),
        Call("int", pcm(2300, ch, 955), wcap(2300, fi, fo), "A"),
    ])


def recycle(family):
    """10. destroy and recycle: (the call of the state that is closed while it is in flight, the first call of the state
    made right afterwards)"""
    ch, fi, fo, q = _fam(family)
    return (Script("recycle: closed", family, [Call("float", floats(3000, ch, 970), wcap(3000, fi, fo), "A")]),
            Script("recycle: fresh", family, [Call("int", pcm(2500, ch, 971), wcap(2500, fi, fo), "B")]))


def all_scripts():
    """every script the GPU file runs, for the CPU companion: (script, how it is judged)"""
    res = []
    for family in FAMILIES:
        res += [(hops(family), "pairs"), (batch_hops(family), "pairs"), (rights(family), "pairs"),
                (ticks(family), "pairs"), (ticks(family, alternate=True), "pairs"), (ticks(family, streams=8), "pairs"),
                (release(family, False), "pairs"), (release(family, True), "pairs")]
        res += [(blocking(family, host), "pairs") for host in BLOCKING]
        res.append((recycle(family), "recycle"))
    res.append((int16_window(), "pairs"))
    for family in IMAGE_FAMILIES:
        res += [(images(family), "pairs"), (images(family, streams=3), "pairs")]
        res += [(control(family, what), "control") for what in CONTROLS]
    return res
