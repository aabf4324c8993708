"""Control scripts for the exact model's segments (tests/exact_model.py): streams whose filter, position and pending
frames change mid-stream, recorded once on the oracle and shared by the CPU and the GPU tests.

A script is a start (channels, in_rate, out_rate, quality) and a list of ops.  Every op begins a SEGMENT; the stream's
start is segment 0.  An op is ("set_quality", q), ("set_rate", in, out), ("set_rate_frac", num, den, in, out),
("skip_zeros",) or ("reset_mem",); ("short",) + op marks a segment that makes its pending-bound call alone, so that
the NEXT op meets pending frames that are partly drained.

Calls of a segment, in this order (frames, capacity):
  0. where the op left pending frames: a call whose capacity is half of what the pending frames alone yield.  It comes
     first because any call with room drains every pending frame before it takes input (resample.c:904-922);
  1. a 1-frame call;
  2. a call bound by its capacity to half its output, so that what follows starts on a non-zero phase.  Its input opens
     with taps + 17 frames of silence: the outputs there see the head through their first taps alone;
  3. an empty call;
  4. a long call of 21 011 frames with with_silence's stretch -- more where the float stream would otherwise make fewer
     than em.BIAS_MIN_SAMPLES samples in the segment, so that (b) and (c) are judged on every filter a script visits.
One segment per script (the first full one with pending frames, else segment 1) makes calls 0 to 2 as ONE coalesced
call of three chunks, the first of fewer frames than there are pending frames.

Streams.  "int16" and "float" are two states fed the same int16-valued samples.  "mixed" is one state whose calls
alternate between the int16 and the float entry point, the float calls on tests/float_inputs.py kinds P and A (real
fractions and full mantissas); its long calls are float calls, so every op is followed by an int16 call over a head
that holds fractions in the segments that start with one.
"""
import functools

import numpy as np

import exact_model as em
import float_inputs as fi
import oracle as orc

BIG = 1 << 20
LONG = 21011

SCRIPTS = {
    # period kernel, fp32 and fp64; grow, shrink, a partly drained shrink that grows and shrinks again
    "period": (2, 44100, 48000, 7, [("set_quality", 10), ("short", "set_quality", 3), ("set_quality", 10),
                                    ("set_quality", 3), ("set_rate", 48000, 44100), ("skip_zeros",), ("reset_mem",)]),
    # slide kernel, fp32 and fp64; n:1; a phase-pair period plan; a ratio that is not the rates' own
    "slide": (1, 24000, 48000, 5, [("set_quality", 10), ("set_rate", 48000, 8000), ("set_rate", 44100, 8000),
                                   ("set_rate_frac", 3, 2, 48000, 32000)]),
    # the period kernel on a folded view, fp64 and fp32, and a ratio that needs no folding between
    "folded": (2, 72000, 16000, 10, [("set_quality", 7), ("set_rate", 44100, 48000), ("set_rate", 72000, 16000)]),
    # into the exact kernel and out of it: a fast kernel starts from a history the exact kernel wrote
    "exact fallback": (4, 48000, 44100, 5, [("set_rate", 192000, 1000), ("set_rate", 48000, 44100)]),
    # frames of 8 channels
    "wide frames": (8, 48000, 44100, 5, [("set_quality", 9), ("set_rate", 48000, 11025)]),
    # int16 and float calls on one state, over the filters that have an int16-window plan
    "mixed data": (2, 48000, 11025, 7, [("short", "set_quality", 5), ("set_quality", 7), ("set_quality", 5),
                                        ("set_rate", 44100, 16000), ("skip_zeros",)]),
}
MIXED = ("mixed data",)
# (CPU tests only) a cutoff change at equal length and equal den: the previous filter's rows FIT the segment
EXTRA = {
    "equal length, direct": (2, 48000, 39000, 5, [("set_rate_frac", 17, 13, 51000, 39000)]),
    "equal length, interpolating": (2, 48000, 47000, 7, [("set_rate_frac", 50, 47, 50000, 47000)]),
}


def apply_op(state, op):
    """op on an oracle, a reference or a speexhip.Resampler -> its return code"""
    op = op[1:] if op[0] == "short" else op
    return getattr(state, op[0])(*op[1:])


def _pcm(frames, ch, seed):
    return orc.lcg_pcm(frames * ch, seed).reshape(frames, ch)


def head_of(o):
    """history ++ pending of a live oracle: [taps - 1 + pending, channels] float32"""
    return np.stack([np.concatenate([o.history(c), o.pending(c)]) for c in range(o.channels)], axis=1)


def plan_calls(o, short, chunked):
    """[(frames, capacity, group)] for the segment that begins where the oracle `o` stands (group: the calls that share
    one coalesced call, or None)"""
    num, den, taps, ch, m = o.num, o.den, o.taps, o.channels, len(o.pending())
    calls = []
    if m and not chunked:
        calls.append((40, max(1, m * den // num // 2), None))
    if short:
        return calls
    n2 = max(3001, 2 * taps + 101)
    half = max(1, n2 * den // num // 2)
    if chunked:     # (capacities that do not bind, but finite: a coalesced call's output buffer holds their sum)
        room = (n2 + m + taps) * den // num + 64
        calls += [(max(m // 2, 1), room, 0), (1, room, 0), (n2, half, 0)]
    else:
        calls += [(1, BIG, None), (n2, half, None)]
    calls.append((0, BIG, None))
    enough = -(-em.BIAS_MIN_SAMPLES // ch) * num // den + 2 * taps + 64
    calls.append((max(LONG, enough), BIG, None))
    return calls


def _chunk_segment(name):
    """the segment that makes its first calls as one coalesced call: the first full one that an op leaves pending frames
    (found on an oracle that takes one frame and the ops: what an op leaves pending depends on the filters' lengths), else 1"""
    ch, i, o_rate, q, ops = (SCRIPTS.get(name) or EXTRA[name])
    o = orc.Oracle(ch, i, o_rate, q)
    o.process(np.zeros((1, ch), np.int16), BIG)     # (a state that has not started keeps no memory across an op)
    for s, op in enumerate(ops, 1):
        apply_op(o, op)
        if op[0] != "short" and len(o.pending()):
            return s
    return 1


@functools.lru_cache(maxsize=None)
def record(name, stream="float", make=orc.Oracle):
    """The script `name` run on `make` over one stream -> list of segments, each a dict:
         op, short, chunked, quality, rate, ratio, key (the filter), model (em.Model of the segment, from this state),
         head, start, calls [dict(io, x, cap, group, used, want, position, head)] (state after each call),
         fed (float32, all input consumed), want (all output), n_float (float samples made).
    Cached: the GPU tests of every mode judge against one run."""
    ch, i, o_rate, q, ops = (SCRIPTS.get(name) or EXTRA[name])
    o = make(ch, i, o_rate, q)
    mixed = stream == "mixed"
    segments, chunk_at, group_io = [], _chunk_segment(name), None
    for s, op in enumerate([None] + list(ops)):
        if op is not None:
            assert apply_op(o, op) == 0, (name, op)
        short = op is not None and op[0] == "short"
        m = len(o.pending())
        chunked = s == chunk_at
        model = em.Model.of(o).segment_of(o)
        seg = {"index": s, "op": op, "short": short, "chunked": chunked, "quality": o.quality(), "rate": o.rate(),
               "ratio": o.ratio(), "key": (o.num, o.den, o.taps, o.kind, o.quality()), "model": model,
               "head": head_of(o), "start": o.position(), "calls": []}
        assert seg["head"].shape[0] == o.taps - 1 + m and model.pending == m
        for j, (frames, cap, group) in enumerate(plan_calls(o, short, chunked)):
            seed = 1000 * s + 10 * j + ch
            long_call = frames >= LONG
            io = stream if not mixed else "float" if long_call or (s + j) % 2 else "int16"
            if group is not None:       # (a coalesced call has one sample type)
                group_io = io if j == 0 else group_io
                io = group_io
            if mixed and io == "float":
                x = fi.make("P" if s % 2 == 0 else "A", frames, ch, seed, o.taps)
                if s % 2:
                    x = x * np.float32(3000.0)      # kind A at the loudness of the int16 calls around it
            else:
                x = _pcm(frames, ch, seed)
            if long_call:
                x = em.with_silence(x, o.taps)
            elif frames > 2 * o.taps:
                x = em.with_silence(x, o.taps, at=0)
            if io == "float":
                x = x.astype(np.float32)
                want, used = o.process_float(x, cap)
            else:
                want, used = o.process(x, cap)
            seg["calls"].append({"io": io, "x": x, "cap": cap, "group": group, "used": used, "want": want,
                                 "position": o.position(), "head": head_of(o)})
        seg["fed"] = np.concatenate([c["x"][: c["used"]].astype(np.float32) for c in seg["calls"]] or
                                    [np.zeros((0, ch), np.float32)])
        seg["n_float"] = sum(c["want"].size for c in seg["calls"] if c["io"] == "float")
        segments.append(seg)
    return segments


def streams_of(name):
    return ("mixed",) if name in MIXED else ("int16", "float")


def truth_of(seg):
    """(truth, mag) of every output of the segment, computed once"""
    if "truth" not in seg:
        seg["truth"] = seg["model"].truth(seg["fed"], sum(c["want"].shape[0] for c in seg["calls"]))
    return seg["truth"]


def judge(seg, outs, bits, yardstick=None, margin=em.MARGIN):
    """(a) on every output of the segment, (b) and (c) on the float calls' where they make em.BIAS_MIN_SAMPLES samples.
    outs: the output of every call, int16 from the int16 calls and float32 from the float calls; yardstick: the same of
    the yardstick (None: (b) is not judged).  The outputs of the other type are masked with values that pass, as
    test_gpu_exact_model_float._judge_mixed does.  -> (failures, stats of the float samples or None)"""
    model, fed = seg["model"], seg["fed"]
    truth, mag = truth_of(seg)
    assert [o.shape for o in outs] == [c["want"].shape for c in seg["calls"]]
    g16, gf = em.halfup(truth).astype(np.int16), truth.astype(np.float32)
    yf, isf, at = gf.copy(), np.zeros(truth.shape[0], bool), 0
    for n, (c, y) in enumerate(zip(seg["calls"], outs)):
        fl = c["io"] == "float"
        assert y.dtype == (np.float32 if fl else np.int16), (n, y.dtype)
        (gf if fl else g16)[at: at + y.shape[0]] = y
        if fl:
            isf[at: at + y.shape[0]] = True
            if yardstick is not None:
                yf[at: at + y.shape[0]] = yardstick[n]
        at += y.shape[0]
    fails, stats = [], None
    if not isf.all():
        fails += ["int16 (a) " + m for m in em.hard_int16(model, fed, g16, truth, mag, bits, tile=model.num)]
    if isf.any():
        fails += ["float (a) " + m for m in em.hard_float(model, fed, gf, truth, mag, bits, tile=model.num)]
        e = em.errors(gf[isf], truth[isf], mag[isf])
        stats = {"n": int(e.size), "rms": em.rms(e), "max": float(np.abs(e).max(initial=0.0)), "z": 0.0, "judged": False}
        if e.size >= em.BIAS_MIN_SAMPLES:
            stats["judged"] = True
            if yardstick is not None:
                stats["yard"] = em.rms(em.errors(yf[isf], truth[isf], mag[isf]))
                if not stats["rms"] <= margin * stats["yard"]:
                    fails.append("(b) rms(e) = %.4g > %.2f x %.4g, the yardstick's" % (stats["rms"], margin, stats["yard"]))
            ok, stats["z"] = em.bias_ok(e)
            if not ok:
                fails.append("(c) mean(e) = %.4g is %.1f sigma from 0 on %d samples" % (float(np.mean(e)), stats["z"], e.size))
    return fails, stats


def split(seg, values):
    """values[n_out, ch] float32 cut into the segment's calls, the int16 calls' share rounded half-up"""
    outs, at = [], 0
    for c in seg["calls"]:
        v = values[at: at + c["want"].shape[0]]
        outs.append(v.astype(np.float32) if c["io"] == "float" else em.halfup(v.astype(np.float64)).astype(np.int16))
        at += c["want"].shape[0]
    return outs


def outputs(seg, key="want"):
    """the segment's outputs of the calls' `key`, concatenated (one type of call only)"""
    return np.concatenate([c[key] for c in seg["calls"]])
