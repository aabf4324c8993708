"""Every kernel family on REAL float samples, and int16 / float calls mixed on one stream, against the exact model.

test_gpu_exact_model.py feeds its float streams the int16 stream's own samples: 16-bit mantissas, no fractions, every
channel equally loud.  Here the float stream of every case of its lists runs one of the kinds of tests/float_inputs.py
(the same checks, yardsticks and margins -- exact_model.py needs nothing new for them):
  A  full float32 mantissas            a window or a table staged through a narrower type
  B  2^-24 .. 1 per sample             a relative error that does not scale (an absolute epsilon)
  C  odd channels 2^-20 quieter        a leak of 2^-22 x the neighbour across a packed FMA, a row mapping, a staged store
  G  passages of 997 frames 2^-20 down the same in time: a floor, a flush
  E  x 2^100                           a clamp to the int16 range, or a rounding to integers, on the float path
  P  x 12000, with fractions           what an int16 window loses (the mixed streams below)
  D  x 2^-125                          gradual underflow: the reference keeps subnormals; judged by (a) alone with the
                                       bounds' underflow term (taps 2^-149)
rotating A, B, C, G, E by case index, and every kind on one case of each family.

Mixed entry points.  The int16-window plans are right only while the histories hold PCM values; Batch::float_seen_ keeps
them off a stream from its first float call until int16 calls have replaced the whole history.  Every float entry point
of the binding is walked through int16, float (kind P), an int16 call of silence that consumes taps - 2, taps - 1 or
taps frames (the boundary of that rule), and int16 calls again, each int16 output inside its interval of the exact
value.  A launch takes the int16 window only where it fills the chip: that is asserted (debug_launch_shape) for the
entry points that bring neighbours -- process_many and Batch -- on the single kinds.  ONE state needs calls of 640 000
to 1 280 000 frames for it (18 of them per entry point and case), and debug_launch_shape does not model the double
kinds: those run here over whatever plan the launch rule picks and meet the int16 window in the diagnostics child of
test_gpu_parity.test_int16_window_on_small_launches_too (SPEEXHIP_W16_ALWAYS), which runs this file's mixed tests.
(That debug_launch_shape stops at the double kinds is a gap of the tool, not a size limit: the fp64 batch takes
period64_w16_ by the same launch rule, and nothing here can assert that it did.  Nor can the child assert more than its
environment: no info field says which window a launch ran over.)
What these scripts catch is a float entry point that does not set the flag (removing one assignment fails them with
ordinary wrong numbers).  What they cannot catch is the clear of int16_call_done being off by ONE: behind taps - 2 frames
of silence the one surviving float frame reaches the outputs through the filter's first tap alone, about 1e-5, so the
fraction an int16 image would lose is 5e-6 LSB and the int16 output rounds to the same value either way.  The three
silence lengths stay, as the boundary a larger first tap would make visible.

Non-finite samples.  One NaN and one +Inf mid-stream on float calls, one instance of each family, against the oracle
and a control run with the sample zeroed: see the test's docstring.
Run with -s for the per-family figures.
"""
import os
from math import gcd

import numpy as np
import pytest

import exact_model as em
import float_inputs as fi
import oracle as orc
import speexhip
import test_gpu_exact_model as xm
import test_gpu_parity as par

pytestmark = pytest.mark.gpu

EVERY_KIND = "ABCGEP"


def _maker(kind):
    return lambda frames, ch, seed, taps: fi.make(kind, frames, ch, seed, taps)


def _walk(family, cases, run):
    """run(case, kind, underflow) on every case with its kind by index, then every kind (and D) on the first case that has
    a channel to be quiet next to"""
    for n, case in enumerate(cases):
        run(case, fi.kind_for(n, case[0]), False)
    every = next((c for c in cases if c[0] >= 2), cases[0])
    for kind in EVERY_KIND:
        if kind != "C" or every[0] >= 2:
            run(every, kind, False)
    run(every, "D", True)
    xm._report(family)


def _state(family, fast_path, **kw):
    def run(case, kind, underflow):
        ch, i, o, q = case[:4]
        xm._one_state(family, ch, i, o, q, fast_path(*case), float_samples=_maker(kind), streams=("float",),
                      underflow=underflow, label=" kind " + kind, **kw)
    return run


def test_exact_model_float_slide_shapes():
    _walk("float slide", par.SLIDE_CASES, _state("float slide", lambda ch, i, o, q: 4 if q >= 9 else 3, bound_call=3))


def test_exact_model_float_n_to_one_decimators():
    _walk("float slide n:1", par.N_TO_ONE_CASES,
          _state("float slide n:1", lambda ch, i, o, q: 4 if q >= 9 else 3, sizes=(1, 40011, 0, 24000)))


def test_exact_model_float_fp64_slide_shapes():
    cases = [(ch, i, o, 10 if (n + ch) % 2 else 9) for n, (i, o) in enumerate(par._SLIDE64_RATIOS) for ch in (1, 2, 3)]
    folded = lambda ch, i, o, q: 5 if (i, o) in ((56000, 16000), (72000, 16000)) and ch == 2 else 4
    _walk("float slide fp64", cases, _state("float slide fp64", folded, bound_call=3))


def test_exact_model_float_period_layouts():
    cases = list(par.LAYOUT_CASES) + [(9, 44100, 48000, 10, "fp32 chain")]
    fp = lambda ch, i, o, q, chain=None: 2 if chain else (5 if q >= 9 and ch in (1, 2, 4, 6, 8) else 2)
    _walk("float period", cases, _state("float period", fp, sizes=(3, 30011, 0, 21234)))


def test_exact_model_float_fp64_period_layouts():
    _walk("float period fp64", par.PERIOD64_CASES,
          _state("float period fp64", lambda ch, i, o, q: 5, sizes=(3, 30011, 0, 21234), bound_call=3))


def test_exact_model_float_folded_views():
    fp = lambda ch, i, o, q: 5 if q >= 9 and ch in (1, 2, 4, 6, 8) and i != 192000 else 2
    _walk("float folded", par.FOLDED_CASES, _state("float folded", fp, sizes=(3, 50011, 0, 1, 30001)))


def test_exact_model_float_fast_mode_tap_range_shares():
    _walk("float FAST shares", xm.FAST_SHARES_CASES,
          _state("float FAST shares", lambda ch, i, o, q, fp: fp, sizes=(3, 60011, 0, 41234), mode=speexhip.MODE_FAST))


def test_exact_model_float_fast_f32_mode_on_the_double_kinds():
    _walk("float FAST_F32", xm.FAST_F32_CASES, _state("float FAST_F32", lambda ch, i, o, q, fp: fp, mode=speexhip.MODE_FAST_F32))


@pytest.mark.parametrize("n", range(len(xm.BATCHES)))
def test_exact_model_float_batches_that_fill_the_chip(n):
    ch, i, o, q, S, F, fast_path, _ = xm.BATCHES[n]
    kind = fi.kind_for(n, ch)
    xm._batch("float batch", ch, i, o, q, S, F, fast_path, float_samples=_maker(kind), streams=("float",), label=" kind " + kind)
    xm._report("float batch")


@pytest.mark.parametrize("kind", EVERY_KIND + "D")
def test_exact_model_float_batch_of_every_kind(kind):
    ch, i, o, q, S, F, fast_path, _ = xm.BATCHES[2]
    xm._batch("float batch", ch, i, o, q, S, F, fast_path, picks=(0, S - 1), float_samples=_maker(kind), streams=("float",),
              underflow=kind == "D", label=" kind " + kind)
    xm._report("float batch")


@pytest.mark.parametrize("row", range(len(xm.BASELINE_ROWS)))
def test_exact_model_float_baseline_rows_at_full_size_in_the_default_mode(row):
    """cfg2 x 1 is the staged-store instance with float I/O"""
    name, ch, i, o, q, fast_path = xm.BASELINE_ROWS[row]
    frames = 1 << 20
    model = em.Model(ch, i, o, q)
    kinds = EVERY_KIND + "D" if name == "cfg2" else fi.kind_for(row, ch)
    for kind in kinds:
        xf = fi.make(kind, frames, ch, 12345, model.taps)
        cap, _ = orc.wrapper_capacity(xf.size * 2, i, o, ch)
        r = speexhip.Resampler(ch, i, o, q)
        info = r.info()
        assert info["mode"] == speexhip.MODE_FAST_FIXED and info["fast_path"] == fast_path, info
        bits = xm._expect_bits(info, model)
        gotf, used = r.process_float(xf, cap)
        r.close()
        wantf, wu = orc.Oracle(ch, i, o, q).process_float(xf, cap)
        assert used == wu and gotf.shape == wantf.shape
        xm._judge("float baseline, full size", "%s kind %s" % (name, kind), model, bits, None, None, gotf, wantf, fedf=xf[:used],
                  underflow=kind == "D")
    xm._report("float baseline, full size")


# ---- int16 and float calls mixed on one stream, through every float entry point ----
MIXED_CASES = [(2, 48000, 11025, 7), (4, 48000, 11025, 5), (2, 44100, 16000, 7), (2, 48000, 11025, 10)]
ENTRY_POINTS = ["process_float", "process_into", "process_take", "process_chunks", "channel_call", "process_many",
                "resampler_process_device", "batch_process_device"]
NEIGHBOURS = 8      # states of a process_many call, streams of a Batch


def _window_forced():
    """the diagnostics child: the int16 window at every launch size"""
    return os.environ.get("SPEEXHIP_W16_ALWAYS") == "1" and os.path.samefile(speexhip.LIB_PATH, par.DIAG_LIB)


class _Rig:
    """S streams of one filter behind one float entry point: int16(xs) / float(xs) -> [(output, consumed)] per stream"""

    def __init__(self, entry, ch, i, o, q, cap):
        self.entry, self.ch, self.cap = entry, ch, cap
        self.batch = entry == "batch_process_device"
        self.S = NEIGHBOURS if entry in ("process_many", "batch_process_device") else 1
        if self.batch:
            self.b = speexhip.Batch(self.S, ch, i, o, q)
        else:
            self.states = [speexhip.Resampler(ch, i, o, q) for _ in range(self.S)]

    def info(self, s):
        return self.b.info(s) if self.batch else self.states[s].info()

    def _device(self, xs, fl):
        import torch
        sp = torch.cuda.current_stream().cuda_stream
        n, cap, ch = xs[0].shape[0], self.cap, self.ch
        d_in = torch.from_numpy(np.ascontiguousarray(np.stack(xs))).cuda()
        d_out = torch.zeros((self.S, cap, ch), dtype=torch.float32 if fl else torch.int16, device="cuda")
        if self.batch:
            used, made = self.b.process_device(d_in.data_ptr(), max(n, 1) * ch, n, d_out.data_ptr(), cap * ch, cap, sp, fl)
        else:
            u, m = self.states[0].process_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, sp, fl)
            used, made = [u], [m]
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        return [(out[s, : made[s]].copy(), used[s]) for s in range(self.S)]

    def int16(self, xs):
        if self.entry in ("resampler_process_device", "batch_process_device"):
            return self._device(xs, False)
        if self.entry == "process_many":
            outs, used, codes = speexhip.process_many(self.states, xs, [self.cap] * self.S)
            assert not any(codes), codes
            return list(zip(outs, used))
        return [self.states[0].process(xs[0], self.cap)]

    def float(self, xs):
        r, x, cap = self.states[0] if not self.batch else None, xs[0], self.cap
        if self.entry in ("resampler_process_device", "batch_process_device"):
            return self._device(xs, True)
        if self.entry == "process_many":
            outs, used, codes = speexhip.process_many(self.states, xs, [cap] * self.S, dtype=np.float32)
            assert not any(codes), codes
            return list(zip(outs, used))
        if self.entry == "process_float":
            return [r.process_float(x, cap)]
        if self.entry == "process_take":
            return [r.process_take(x, cap, float_io=True)]
        if self.entry == "process_into":
            out = np.zeros((cap, self.ch), np.float32)
            used, made = r.process_into(np.ascontiguousarray(x), out, float_io=True)
            return [(out[:made].copy(), used)]
        if self.entry == "process_chunks":
            a, b = x.shape[0] // 3, 2 * x.shape[0] // 3
            outs, used = r.process_chunks([x[:a], x[a:b], x[b:]], [cap] * 3, dtype=np.float32)
            assert used == [a, b - a, x.shape[0] - b]
            return [(np.concatenate(outs), sum(used))]
        assert self.entry == "channel_call"
        cols, used = [], set()
        for c in range(self.ch):
            rc, u, m, out = r.channel_call("float", c, x[:, c], cap)
            assert rc == 0
            cols.append(out[:m].copy()), used.add(u)
        assert len(used) == 1 and len({c.shape for c in cols}) == 1
        return [(np.stack(cols, axis=1), used.pop())]

    def close(self):
        for st in [self.b] if self.batch else self.states:
            st.close()


def _long_call(ch, i, o, q, S, single_kind):
    """frames of the long int16 calls: the smallest size at which the launch takes the int16 window, where that can be had"""
    if S == 1 or not single_kind:
        return 24000, False
    g = gcd(i, o)
    for frames in (24000, 48000, 96000, 192000):
        if speexhip.debug_launch_shape(i // g, o // g, q, ch, S, frames)["int16_window"]:
            return frames, True
    return 24000, False


@pytest.mark.parametrize("entry", ENTRY_POINTS)
@pytest.mark.parametrize("ch,i,o,q", MIXED_CASES)
def test_exact_model_mixed_entry_points(ch, i, o, q, entry):
    model = em.Model(ch, i, o, q)
    taps = model.taps
    assert speexhip.debug_plan(i, o, q, ch)["w16_lane_periods"] > 0 or model.double_kind
    S = NEIGHBOURS if entry in ("process_many", "batch_process_device") else 1
    L, fills = _long_call(ch, i, o, q, S, not model.double_kind)
    # the precondition: the int16 calls of steps 1, 4 and 5 run over the int16 window (see the module docstring for the
    # one-state entry points and the double kinds in the product build)
    forced = _window_forced()
    if S > 1 and not model.double_kind:
        assert forced or fills, "no launch size takes the int16 window"
    print("%s %s: long calls of %d frames x %d streams; int16 window %s" % (
        entry, (ch, i, o, q), L, S, "forced" if forced else "by the launch rule" if fills else "not asserted"))
    cap = L * o // i + 64
    picks = sorted({0, S - 1})
    worst = 0.0
    for n in (taps - 2, taps - 1, taps):
        rig = _Rig(entry, ch, i, o, q, cap)
        refs = {s: orc.Oracle(ch, i, o, q) for s in picks}
        bits = xm._expect_bits(rig.info(0), model)
        assert bits == 64 or not model.double_kind
        # per-channel calls run the exact kernel whatever the state's fast path (Batch::run_channel): the reference's own
        # arithmetic -- fp32-rounded products on the double kinds too --, so their outputs EQUAL the oracle's and are
        # judged with the fp32 bound, as test_exact_model_exact_fallback judges that kernel
        float_bits = 32 if entry == "channel_call" else bits
        log = {s: {"fed": [], "got": [], "want": [], "float": []} for s in picks}
        step = 0
        for nf in (taps // 3, 3 * taps):             # the float call: fewer than taps - 1 frames, and more
            script = [("int16", lambda s: orc.lcg_pcm(L * ch, 100 + step + s).reshape(L, ch)),
                      ("float", lambda s: fi.make("P", nf, ch, 200 + step + s)),
                      ("int16", lambda s: np.zeros((n, ch), np.int16)),
                      ("int16", lambda s: em.with_silence(orc.lcg_pcm(L * ch, 300 + step + s).reshape(L, ch), taps, at=0)),
                      ("int16", lambda s: orc.lcg_pcm(L * ch, 400 + step + s).reshape(L, ch))]
            for io, make in script:
                xs = [make(s) for s in range(S)]
                res = rig.float(xs) if io == "float" else rig.int16(xs)
                for s in picks:
                    y, used = res[s]
                    w, wu = refs[s].process_float(xs[s], cap) if io == "float" else refs[s].process(xs[s], cap)
                    assert used == wu == xs[s].shape[0] and y.shape == w.shape, (entry, n, step, s, used, wu, y.shape, w.shape)
                    inf = rig.info(s)
                    assert (inf["last_sample"], inf["samp_frac_num"]) == refs[s].position(), (entry, n, step, s)
                    if io == "float" and entry == "channel_call":
                        assert np.array_equal(y, w), (entry, n, step, s)
                    log[s]["fed"].append(xs[s].astype(np.float32)), log[s]["got"].append(y), log[s]["want"].append(w)
                    log[s]["float"].append(io == "float")
                step += 1
        rig.close()
        for s in picks:
            worst = max(worst, _judge_mixed("%s %s n %d stream %d" % (entry, (ch, i, o, q), n, s), model, bits, float_bits, log[s]))
    print("[exact model] mixed %s %s: float calls' worst rms(e) / yardstick %.2f" % (entry, (ch, i, o, q), worst))


def _judge_mixed(name, model, bits, float_bits, log):
    """hard_int16 on the outputs of the int16 calls, (a) and (b) on those of the float calls ((c) needs 20 000 samples),
    against the truth of the whole stream.  Outputs of the other type are masked with values that pass."""
    fed = np.concatenate(log["fed"])
    n_out = sum(y.shape[0] for y in log["got"])
    truth, mag = model.truth(fed, n_out)
    g16 = em.halfup(truth).astype(np.int16)
    gf = truth.astype(np.float32)
    at, segs = 0, []
    for y, w, fl in zip(log["got"], log["want"], log["float"]):
        (gf if fl else g16)[at: at + y.shape[0]] = y
        if fl:
            segs.append((at, at + y.shape[0], w))
        at += y.shape[0]
    fails = ["int16 (a) " + m for m in em.hard_int16(model, fed, g16, truth, mag, bits, tile=model.num)]
    fails += ["float (a) " + m for m in em.hard_float(model, fed, gf, truth, mag, float_bits, tile=model.num)]
    ratio = 0.0
    for a, b, w in segs:
        mine, yard = em.rms(em.errors(gf[a:b], truth[a:b], mag[a:b])), em.rms(em.errors(w, truth[a:b], mag[a:b]))
        margin = 1.0 if float_bits == 64 else em.MARGIN
        ratio = max(ratio, mine / yard if yard else 0.0)
        if not mine <= margin * yard:
            fails.append("float (b) outputs %d..%d: rms(e) = %.4g > %.2f x %.4g" % (a, b, mine, margin, yard))
    assert not fails, (name, fails)
    return ratio


# ---- one NaN, one +Inf ----
# (family, channels, in, out, quality, fast_path, streams, frames of the first call)
NON_FINITE_CASES = [("period, one generation (r = 5 shares, staged stores)", 2, 44100, 48000, 7, 2, 1, 20011),
                    ("period, padded 8-channel window", 8, 48000, 44100, 5, 2, 1, 20011),
                    ("slide", 2, 48000, 8000, 7, 3, 1, 20011),
                    ("period fp64", 2, 44100, 48000, 10, 5, 1, 20011),
                    ("slide fp64", 1, 24000, 48000, 10, 4, 1, 20011),
                    ("folded", 2, 72000, 16000, 7, 2, 1, 20011),
                    ("batch, r = 10, several generations", 2, 44100, 48000, 7, 2, 40, 200000)]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _float_calls(ch, i, o, q, fast_path, S, xs, sizes):
    """float calls of `sizes` frames over xs[s] on S streams (one state, or a Batch through device pointers)
    -> ([output per stream], [(consumed, produced) per call and stream], [position per stream])"""
    cap = max(sizes) * o // i + 64
    outs, counters, off = [[] for _ in range(S)], [], 0
    if S == 1:
        r = speexhip.Resampler(ch, i, o, q)
        assert r.info()["fast_path"] == fast_path, r.info()
        for n in sizes:
            y, u = r.process_float(xs[0][off: off + n], cap)
            assert u == n
            outs[0].append(y), counters.append([(u, y.shape[0])])
            off += n
        pos = [r.position()]
        r.close()
    else:
        import torch
        sp = torch.cuda.current_stream().cuda_stream
        b = speexhip.Batch(S, ch, i, o, q)
        assert b.info()["fast_path"] == fast_path, b.info()
        d_out = torch.zeros((S, cap, ch), dtype=torch.float32, device="cuda")
        for n in sizes:
            d_in = torch.from_numpy(np.ascontiguousarray(xs[:, off: off + n])).cuda()
            used, made = b.process_device(d_in.data_ptr(), n * ch, n, d_out.data_ptr(), cap * ch, cap, sp, True)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert used == [n] * S
            for s in range(S):
                outs[s].append(out[s, : made[s]].copy())
            counters.append(list(zip(used, made)))
            off += n
        pos = [(b.info(s)["last_sample"], b.info(s)["samp_frac_num"]) for s in range(S)]
        b.close()
    return [np.concatenate(v) for v in outs], counters, pos


@pytest.mark.parametrize("family,ch,i,o,q,fast_path,S,first", NON_FINITE_CASES)
def test_exact_model_non_finite_samples_poison_what_the_reference_poisons_and_no_more_than_twice_the_filter(
        family, ch, i, o, q, fast_path, S, first):
    """One NaN, then one +Inf, in one channel of one stream at frame p of a float stream that float calls continue until
    the sample has left the history; against the oracle on the same input and a control run with that sample zeroed.
    Every output the oracle makes non-finite is non-finite; every other channel and stream is bit-identical to the
    control; so is every output whose window lies more than taps frames clear of p; an output outside the oracle's mask is
    non-finite (the spill: a zero padding tap times the sample, 0 x NaN) or bit-identical to the control; counters and
    positions are equal.  The spill is printed."""
    model = em.Model(ch, i, o, q)
    taps, num, den = model.taps, model.num, model.den
    sizes = [first, taps // 2, 2 * taps + 5] + ([0] if S == 1 else []) + [3001]
    total = sum(sizes)
    xs = np.stack([fi.make("A", total, ch, 900 + s, taps) for s in range(S)])
    s0, c0, p = S // 3, ch - 1, 2 * first // 3 + 7
    assert first // 3 + taps + 17 < p - 2 * taps and p + 2 * taps < first       # mid-stream, clear of the silence
    control = xs.copy()
    control[s0, p, c0] = 0
    got0, counters0, pos0 = _float_calls(ch, i, o, q, fast_path, S, control, sizes)
    for value in (np.float32(np.nan), np.float32(np.inf)):
        x = control.copy()
        x[s0, p, c0] = value
        got, counters, pos = _float_calls(ch, i, o, q, fast_path, S, x, sizes)
        ref, off, want = orc.Oracle(ch, i, o, q), 0, []
        for call, n in enumerate(sizes):
            w, wu = ref.process_float(x[s0, off: off + n], 1 << 20)
            assert (wu, w.shape[0]) == counters[call][s0], (family, value, call)
            want.append(w)
            off += n
        want = np.concatenate(want)
        assert counters == counters0 and pos == pos0 and pos[s0] == ref.position(), (family, value)
        for s in range(S):
            if s != s0:
                assert _bits_equal(got[s], got0[s]), (family, value, "stream", s)
        g, g0 = got[s0], got0[s0]
        assert g.shape == g0.shape == want.shape
        for c in range(ch):
            if c != c0:
                assert _bits_equal(g[:, c], g0[:, c]) and np.isfinite(want[:, c]).all(), (family, value, "channel", c)
        k = np.arange(g.shape[0], dtype=np.int64)
        newest = k * num // den                     # the window of output k: input frames newest - (taps - 1) .. newest
        covers = (newest - (taps - 1) <= p) & (p <= newest)
        theirs, ours = ~np.isfinite(want[:, c0]), ~np.isfinite(g[:, c0])
        assert theirs.any() and not (theirs & ~covers).any(), (family, value)
        assert ours[theirs].all(), (family, value, "finite where the reference is not", int((theirs & ~ours).sum()))
        same = g[:, c0].view(np.uint32) == g0[:, c0].view(np.uint32)
        clear = (newest < p - taps) | (newest - (taps - 1) > p + taps)
        assert same[clear].all(), (family, value, "poison more than taps frames clear of the sample", k[clear & ~same][:6])
        assert (ours | same)[~theirs].all(), (family, value, "a finite output changed", k[~theirs & ~ours & ~same][:6])
        spill = ours & ~theirs
        before = int((p - newest[spill & (newest < p)]).max(initial=0))
        after = int((newest[spill & (newest >= p)] - (taps - 1) - p).max(initial=0))
        print("[exact model] non-finite %-52s %4s: reference poisons %d outputs, spill %d outputs (reaching %d frames before "
              "the window, %d behind)" % (family, "NaN" if np.isnan(value) else "+Inf", int(theirs.sum()), int(spill.sum()),
                                          before, after))
