"""Streams fed in small calls: the call schedules, the driver that cuts one array by them, and the fp32 chain computed
call by call as a kernel computes it -- shared by the CPU and the GPU tests, no GPU used.

The exact-model suite's streams are three or four calls, one of them tens of thousands of frames long.  A real caller
makes hundreds of calls of a few hundred frames, often fewer than taps - 1, each starting on another phase.  That is
where a kernel's start handling has its corners (engine.cpp set_position):
  k_shift    = the phase index of samp_frac_num (the k with k num % den == frac), anywhere in [0, den);
  base_shift = last - k_shift num // den, negative when the virtual window -- period 0, phase 0 -- starts before the
               history: silence there, and every phase lane below k_shift masked;
  m_total    = 1, or two periods for a few outputs that straddle one period boundary;
  n_out      = 0: only the history roll runs;  consumed < taps - 1: the roll keeps old history.

The resubmission rule.  A capacity-bound call computes its last outputs from frames it then reports as not consumed
(resample.c: *in_len = last_sample), so a stream in pieces is well defined only if the caller hands the unconsumed frames
in again at the head of the next call.  cut() therefore cuts ONE array X and advances by `used`; samples are never
drawn per call.  Cut this way the oracle's and the reference's pieces equal their one-call output byte for byte
(tests/test_cpu_streaming.py).

schedule() builds the calls with the library's own integer bookkeeping (speexhip.plan_call_ex, host only), so the
conditions test_cpu_streaming.py asserts hold by construction:
  1. a phase walk: min(den, 160) calls of capacity 1 -- gcd(num, den) = 1, so each starts on the next phase index;
  2. a second walk of as many calls whose capacities cycle through 2 .. 12 and den - k_shift + {-1, 0, 1} (the outputs
     stop just before, on and just past the first period boundary), an unbounded small call after every second one,
     then calls that start on the phase indices den - 2, den - 1, 0 and 1;
  3. about 100 calls by size class -- 0 frames, 1 frame, 2 .. taps/4, 1 .. taps - 2, taps - 2 .. taps, taps .. 3 taps --
     every fifth bound to half its output, one of capacity 0 with frames; decimators: calls that make no output;
  4. one closing long call, so that the float stream has em.BIAS_MIN_SAMPLES samples.
"""
import functools
from types import SimpleNamespace

import numpy as np

import exact_model as em
import oracle as orc

BIG = 1 << 20
WALK = 160

DEFECTS = ("history roll off by one frame when consumed < taps - 1",
           "a zero-output call does not roll",
           "an idle call leaves the history in the other ping-pong buffer",
           "phase lanes below k_shift stored",
           "the first partial period dropped",
           "start phase 0 after a capacity-bound call",
           "unconsumed frames counted as consumed")
# Not in DEFECTS: a correct mask hides it.  Only lanes below k_shift read in front of the history, and they are not
# stored; it shows together with "phase lanes below k_shift stored" (test_cpu_streaming.py asserts both halves).
CLAMPED_FRONT = "frames before the history read as the history's first frame"

# The one-state cases of tests/test_gpu_exact_model_streaming.py, by family: the smallest of test_gpu_parity.py's lists
# that reach each instance.  test_cpu_streaming.py asserts the schedule's conditions on every one of them.
FAMILIES = {
    "slide": [(1, 16000, 48000, 5), (2, 16000, 48000, 7), (2, 8000, 40000, 7), (1, 8000, 40000, 5), (2, 48000, 32000, 7),
              (2, 32000, 12000, 7), (3, 48000, 40000, 4), (6, 40000, 48000, 2), (1, 48000, 48000, 6), (1, 24000, 48000, 10),
              (1, 48000, 40000, 9), (2, 48000, 8000, 7), (1, 40000, 8000, 10)],
    "period": [(2, 44100, 48000, 7), (1, 48000, 44100, 7), (3, 48000, 44100, 4), (8, 48000, 44100, 5), (2, 32000, 44100, 7),
               (2, 48000, 11025, 7), (1, 48000, 11025, 7), (7, 22050, 16000, 8), (10, 44100, 48000, 7),
               (16, 48000, 11025, 5), (9, 48000, 11025, 7)],
    "period fp64": [(1, 44100, 48000, 10), (2, 44100, 48000, 10), (2, 48000, 44100, 10), (2, 44100, 8000, 10)],
    "folded": [(2, 56000, 48000, 4), (2, 72000, 16000, 7), (1, 88000, 8000, 5), (1, 64000, 12000, 7)],
}
FALLBACK = (2, 192000, 1000, 8)     # 40 calls of at most 4096 frames: case(*FALLBACK, **FALLBACK_SCHEDULE)
FALLBACK_SCHEDULE = {"walk": 6, "classes": 32, "long_call": False, "max_frames": 4096}
# MODE_FAST and MODE_FAST_F32: three of test_gpu_exact_model.py's FAST_SHARES_CASES / FAST_F32_CASES each, with fast_path
FAST_CASES = [(2, 48000, 11025, 7, 2), (1, 192000, 8000, 7, 3), (2, 44100, 8000, 10, 5)]
FAST_F32_CASES = [(1, 24000, 48000, 10, 3), (2, 44100, 48000, 10, 2), (1, 48000, 8000, 10, 3)]
BATCH_SCHEDULE = {"walk": 22, "classes": 60}    # 120 calls and the closing long one


def phase_index(num, den, frac):
    """the k in [0, den) with k num % den == frac (stream_plan.cpp phase_index_of)"""
    return frac * pow(num, -1, den) % den if den > 1 else 0


class _Walker:
    """(frames, capacity) calls and where each starts, by speexhip.plan_call_ex (the float entry's bookkeeping; the
    int16 entry's counters are asserted equal by the tests)."""

    def __init__(self, num, den, block_in):
        import speexhip
        self._plan = speexhip.plan_call_ex
        self.num, self.den, self.block_in = num, den, block_in
        self.last = self.frac = 0
        self.calls, self.log = [], []

    def peek(self, frames, cap):
        """-> (consumed, produced, last', frac')"""
        return self._plan(self.num, self.den, frames, cap, True, self.block_in, self.last, self.frac, 0)[:4]

    def add(self, frames, cap):
        used, made, last, frac = self.peek(frames, cap)
        self.calls.append((frames, cap))
        self.log.append({"frames": frames, "cap": cap, "start": (self.last, self.frac), "used": used, "made": made})
        self.last, self.frac = last, frac
        return used, made

    @property
    def k(self):
        return phase_index(self.num, self.den, self.frac)

    def bound(self, cap, extra=0):
        """a call that capacity `cap` binds: frames for more outputs than that"""
        self.add(self.last + cap * self.num // self.den + self.num // self.den + 3 + extra, cap)


def schedule(model, block_in, walk=WALK, classes=102, long_call=True, max_frames=None):
    """-> SimpleNamespace(calls [(frames, capacity)], log [dict(frames, cap, start (last, frac), used, made)],
    parts {name: range of call indices}).  walk, classes: calls of parts 1 / 2 and of part 3; max_frames clips every
    call (the 192:1 fallback, whose filter has 30 720 taps)."""
    num, den, taps, ch = model.num, model.den, model.taps, model.channels
    w = _Walker(num, den, block_in)
    clip = (lambda f: f) if max_frames is None else (lambda f: min(f, max_frames))
    parts, n_walk = {}, min(den, walk)
    # 1. the phase walk
    for k in range(n_walk):
        w.add(num // den + 2 + k % 3, 1)
    parts["phase walk"] = range(0, len(w.calls))
    # 2. the second walk
    first = len(w.calls)
    for j in range(n_walk):
        cap = 2 + (j // 2) % 11 if j % 2 == 0 else max(1, den - w.k + (-1, 0, 1)[(j // 2) % 3])
        w.bound(cap, j % 3)
        if j % 2:
            w.add(1 + (5 * j) % 17, BIG)
    if den > 2:     # starts on the phase indices den - 2, den - 1, 0 and 1
        w.bound((den - 2 - w.k) % den or den)
        for _ in range(4):
            w.bound(1)
    w.bound(den - w.k + 1)      # lanes k_shift .. den: the last output alone lies past the period boundary
    parts["second walk"] = range(first, len(w.calls))
    # 3. size classes
    first = len(w.calls)
    sizes = [(0, 0), (1, 1), (2, max(2, taps // 4)), (1, taps - 2), (taps - 2, taps), (taps, 3 * taps)]
    seed = 12345 + 7 * num + den
    for n in range(classes):
        seed = (seed * 1664525 + 1013904223) & 0xFFFFFFFF
        lo, hi = sizes[n % 6]
        frames = clip(lo + (seed >> 8) % (hi - lo + 1))
        cap = BIG
        if n % 5 == 4:
            cap = max(1, frames * den // num // 2)
        if n == classes // 2 - (classes // 2) % 6 + 2:      # (a call of class 2 .. taps/4)
            cap = 0
        w.add(frames, cap)
    if num > den:   # calls with frames that make no output: one frame where the position stands past it
        found = 0
        for _ in range(200):
            if found >= 6:
                break
            if w.last >= 1:
                assert w.add(1, BIG)[1] == 0
                found += 1
                continue
            f = next((f for f in range(2, 64) if w.peek(f, BIG)[2] >= 1), None)
            w.add(3 if f is None else f, BIG)
    parts["size classes"] = range(first, len(w.calls))
    # 4. the closing long call
    if long_call:
        first = len(w.calls)
        w.add(clip(-(-em.BIAS_MIN_SAMPLES // ch) * num // den + 2 * taps + 64), BIG)
        parts["long call"] = range(first, len(w.calls))
    return SimpleNamespace(calls=w.calls, log=w.log, parts=parts)


def make_input(model, sched, seed=91):
    """X: lcg_pcm noise over everything the schedule submits, with stretches of silence longer than the filter
    (em.with_silence) placed so that a window enters silence in one call and leaves it in a later one and a call lies
    wholly inside: one in the second walk, one among the size classes, one in the long call."""
    ch, taps = model.channels, model.taps
    offs = np.concatenate([[0], np.cumsum([c["used"] for c in sched.log])])
    total = max(int(offs[n]) + c["frames"] for n, c in enumerate(sched.log))
    x = orc.lcg_pcm(total * ch, seed + ch).reshape(total, ch)
    for part in ("second walk", "size classes"):
        picks = [n for n in sched.parts.get(part, ()) if 0 < sched.log[n]["frames"] <= taps // 4 + 17
                 and sched.log[n]["cap"] == BIG and offs[n] >= 3]
        if picks:
            n = picks[len(picks) // 2]
            x = em.with_silence(x, taps, at=int(offs[n]) - 3)
    for n in sched.parts.get("long call", ()):
        if sched.log[n]["frames"] > 2 * taps + 64:
            x = em.with_silence(x, taps, at=int(offs[n]) + sched.log[n]["frames"] // 3)
    return x


def cut(X, calls, call, position=None, after=None):
    """Drives a state through `calls` with the resubmission rule: call(frames of X from the stream's offset, capacity)
    -> (output, used); the offset advances by `used`.  position() (optional) is read before every call; after(n, rec)
    (optional) runs after call n.  -> list of dict(out, used, made, start, offset, frames, cap)."""
    off, recs = 0, []
    for n, (frames, cap) in enumerate(calls):
        start = None if position is None else tuple(position())
        y, used = call(X[off: off + frames], cap)
        rec = {"out": y, "used": used, "made": y.shape[0], "start": start, "offset": off, "frames": frames, "cap": cap}
        recs.append(rec)
        off += used
        if after is not None:
            after(n, rec)
    return recs


def consumed(recs):
    return sum(r["used"] for r in recs)


def joined(recs):
    return np.concatenate([r["out"] for r in recs])


def chunked_chain32(model, X, calls, defect=None, stored_lanes=False):
    """em.chain32 computed CALL BY CALL, as a kernel computes it: every call reads V = history ++ input, places its
    outputs on the lanes k_shift .. k_shift + n_out - 1 of a virtual window that starts base_shift frames into V
    (silence in front of V), and leaves V[consumed : consumed + taps - 1] as the next history in the other ping-pong
    buffer.  The counters are the reference's rule in closed form.  defect: one of DEFECTS or CLAMPED_FRONT;
    stored_lanes: "phase lanes below k_shift stored" on top of it.
    -> SimpleNamespace(outs [float32 per call], used, starts, fed, history)."""
    assert defect is None or defect in DEFECTS or defect == CLAMPED_FRONT, defect
    num, den, taps, ch = model.num, model.den, model.taps, model.channels
    stored_lanes = stored_lanes or defect == DEFECTS[3]
    H, pad = taps - 1, num + 1      # (a lane below k_shift starts up to k_shift num // den < num frames before V)
    Xf = np.asarray(X, np.float64).reshape(-1, ch)
    bufs, cur = [np.zeros((H, ch)), np.zeros((H, ch))], 0
    last = frac = off = base = 0
    after_bound = False
    blocks, where, phases, keeps, counts, used, starts = [], [], [], [], [], [], []
    for frames, cap in calls:
        if defect == DEFECTS[5] and after_bound:
            frac = 0
        starts.append((last, frac))
        frames = min(frames, Xf.shape[0] - off)     # (a defect that consumes too much runs out of input early)
        hist = bufs[cur]
        V = np.concatenate([hist, Xf[off: off + frames]])
        room = frames - last
        n_out = min(cap, 0 if room <= 0 else -(-(room * den - frac) // num))
        t = frac + n_out * num
        last_after, frac_next = last + t // den, t % den
        eaten = min(last_after, frames)
        after_bound = eaten < frames
        if defect == DEFECTS[6] and after_bound:
            eaten = frames
        last_next = max(last_after - eaten, 0)
        k = phase_index(num, den, frac)
        lanes = (0 if stored_lanes else k) + np.arange(n_out, dtype=np.int64)
        keep = np.ones(n_out, bool)
        if defect == DEFECTS[4] and k > 0:
            keep = lanes >= den
        front = np.zeros((pad, ch))
        if defect == CLAMPED_FRONT:
            front[:] = V[0]
        blocks.append(np.concatenate([front, V, np.zeros((1, ch))]))
        where.append(base + pad + (last - k * num // den) + lanes * num // den)
        phases.append(lanes * num % den)
        keeps.append(keep), counts.append(n_out), used.append(eaten)
        base += blocks[-1].shape[0]
        rolled = V[eaten: eaten + H]
        if defect == DEFECTS[0] and 0 < eaten < H:
            rolled = blocks[-1][pad + eaten + 1: pad + eaten + 1 + H]
        if defect == DEFECTS[1] and n_out == 0 and eaten > 0:
            rolled = hist
        if not (defect == DEFECTS[2] and n_out == 0 and eaten == 0):
            bufs[cur ^ 1] = rolled
        cur ^= 1
        off, last, frac = off + eaten, last_next, frac_next
    G = np.concatenate(blocks)
    pos, phase, keep = np.concatenate(where), np.concatenate(phases), np.concatenate(keeps)
    rows32 = model.rows.astype(np.float32).astype(np.float64)
    s = np.zeros((pos.size, ch), np.float32)
    for j in range(taps):
        s = (rows32[phase, j][:, None] * G[pos + j] + s.astype(np.float64)).astype(np.float32)
    s[~keep] = 0
    outs = np.split(s, np.cumsum(counts)[:-1]) if counts else []
    return SimpleNamespace(outs=outs, used=used, starts=starts, fed=np.asarray(X).reshape(-1, ch)[:off],
                           history=bufs[cur].astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(ch, i, o, q, walk=WALK, classes=102, long_call=True, max_frames=None):
    """model, schedule and input of one filter, made once: SimpleNamespace(key, model, block_in, sched, calls, X, Xf)"""
    model = em.Model(ch, i, o, q)
    block_in = orc.Oracle(ch, i, o, q).block_in()
    sched = schedule(model, block_in, walk, classes, long_call, max_frames)
    X = make_input(model, sched)
    X.setflags(write=False)
    Xf = X.astype(np.float32)
    Xf.setflags(write=False)
    return SimpleNamespace(key=(ch, i, o, q), model=model, block_in=block_in, sched=sched, calls=sched.calls, X=X, Xf=Xf)


def batch_case(ch, i, o, q):
    """case() with about 120 calls and the closing long one, whatever den is: the batch tests' schedule"""
    c = case(ch, i, o, q, **BATCH_SCHEDULE)
    short = 121 - len(c.calls)
    return c if short <= 0 else case(ch, i, o, q, BATCH_SCHEDULE["walk"], BATCH_SCHEDULE["classes"] + short)


def history_of(o):
    """[taps - 1, channels] float32 of an oracle or a reference"""
    return np.stack([o.history(c) for c in range(o.channels)], axis=1)


def run_on(make, key, X, calls, kind, every=16):
    """The schedule cut on a fresh `make(*key)` (oracle.Oracle / oracle.Reference) -> the records of cut(), each with
    "end" (the position after the call) and, after every `every`-th call and the last, "history"."""
    o = make(*key)
    fn = o.process_float if kind == "float" else o.process

    def after(n, rec):
        rec["end"] = tuple(o.position())
        if n % every == every - 1 or n == len(calls) - 1:
            rec["history"] = history_of(o)
    return cut(X, calls, fn, position=o.position, after=after)


@functools.lru_cache(maxsize=None)
def oracle_run(ch, i, o, q, kind, walk=WALK, classes=102, long_call=True, max_frames=None):
    """the oracle over case(...)'s stream, computed once and shared: the counters, positions and histories the GPU tests
    compare with, and the float yardstick"""
    c = case(ch, i, o, q, walk, classes, long_call, max_frames)
    return run_on(orc.Oracle, c.key, c.Xf if kind == "float" else c.X, c.calls, kind)


def one_call(make, key, x, kind):
    """a fresh state fed x in one call -> (output, used)"""
    st = make(*key)
    return (st.process_float if kind == "float" else st.process)(x, max(BIG, x.shape[0] * 8))


def conditions(model, log):
    """What a schedule's calls met, from their start positions and counters (log: dicts with start, used, made,
    frames): the figures test_cpu_streaming.py asserts."""
    num, den, H = model.num, model.den, model.taps - 1
    phases, fracs, eaten = set(), set(), 0
    none_out = short_rolls = bound = straddle = 0
    for c in log:
        k = phase_index(num, den, c["start"][1])
        if c["made"]:
            phases.add(k), fracs.add(c["start"][1])
            straddle += (k + c["made"] - 1) // den == 1
        none_out += c["frames"] > 0 and c["made"] == 0
        short_rolls += eaten >= H and 0 < c["used"] < H
        bound += c["made"] == c["cap"] and c["used"] < c["frames"]
        eaten += c["used"]
    return SimpleNamespace(phases=phases, fracs=fracs, none_out=none_out, short_rolls=short_rolls, bound=bound,
                           straddle=straddle)


def samples_with_signal(model, fed, n_out):
    """how many of the stream's output samples have a window that is not all silence (mag > 0)"""
    line = model.line(fed)
    nz = np.concatenate([[0], np.cumsum(np.any(line != 0, axis=1))])
    pos, _ = model.geometry(n_out)
    return int((nz[pos + model.taps] - nz[pos] > 0).sum()) * model.channels
