"""The exact value of every output sample, in numpy, and the three checks built on it.

The oracle restates the reference, and the reference is an fp32 computation with rounding error of its own: a
comparison with it cannot see anything below ~0.05 LSB.  This module evaluates the SAME sum exactly (float64, and
rational arithmetic for the few samples a check flags), so that a kernel's error can be measured in units of the fp32
rounding unit u = 2^-24.

Definition.  The taps of a phase are `rows[phase, j]`, j < taps:
  * direct kinds: the reference's fp32 table rows (resample.c:671-678);
  * interpolating kinds: the reference's four FLOAT blend weights (resample.c:318-328; three in float with the constants
    0.16667 and 0.33333, the one at index 2 through a double expression) combined with the fp32 table IN DOUBLE:
    w0 t[-2] + w1 t[-1] + w2 t[0] + w3 t[1] at t = table + 4 + (j + 1) oversample - phase oversample / den
    (filter_design.cpp phase_blend / phase_taps state the same).
Output k of a stream sits at pos = k num // den, phase = k num % den, over the line zeros(taps - 1) ++ (all input the
stream has consumed):  truth[k, c] = sum_j rows[phase, j] line[pos + j, c],  mag[k, c] = sum_j |rows| |line|.
The reference and the product differ from this only by the rounding of products and sums.  The model works per STREAM:
give it the concatenation of what each call consumed and the number of outputs made so far -- multi-call, ragged and
capacity-bound streams need no history logic.

Segments.  A stream is a sequence of segments: one begins at the stream's start or right after a control call
(set_rate, set_rate_frac, set_quality, skip_zeros, reset_mem) that returned, and ends at the next control call.  Within
a segment the definition above holds with
  line = head ++ (all input consumed in the segment),  head = history ++ pending per channel: the taps - 1 frames of
         history and the pending ("magic") frames a shortened filter left buffered, both read from the oracle after
         the control call (Oracle.history(c), Oracle.pending(c): float32, so exact);
  output k of the segment at pos = last0 + (frac0 + k num) // den, phase = (frac0 + k num) % den, where
         (last0, frac0) = Oracle.position() at the segment's start;
  rows:  those of the oracle's filter as it now is (Model.of(o): any set_rate_frac ratio, not only the rates' own).
Model.of(o).segment_of(o) reads all of it from a live oracle; a segment with head = zeros(taps - 1) and start (0, 0)
IS the stream of the first paragraph, byte for byte.  A segment has ONE position: channels that per-channel calls
moved apart stay out of scope.

Input (tests/float_inputs.py).  The model takes any float32 line: a product of two 24-bit numbers is exact in a double
and the rational arbiter settles the rest, so real float data -- full mantissas, fractions, channels and passages 2^20
apart in loudness, samples far outside the int16 range -- is judged by the same three checks and the same bounds as
int16-valued data.  Only gradual underflow (kind D) needs a term of its own: bound32 / bound64 (underflow=True).

Checks, with e = (got - truth) / (u mag) over the samples with mag > 0:
  (a) hard, per sample: hard_float / hard_int16;
  (b) accuracy against a yardstick on the same input: rms(e) (compare with the oracle's or chain32's);
  (c) bias: |mean e| <= 5 rms(e) / sqrt(n) on n >= 20 000 samples (bias_ok).
"""
from fractions import Fraction

import numpy as np

import oracle as orc

U = 2.0 ** -24
BIAS_MIN_SAMPLES = 20000
BIAS_SIGMAS = 5.0
_RECHECK_LIMIT = 512     # flagged samples recomputed exactly; more than that flagged is a failure as it stands


def blend_weights(frac_num, den):
    """The reference's cubic weights for the sub-step frac_num / den, as IT computes them: float arithmetic, one rounding
    per operation, left to right; the weight at index 2 from a double expression narrowed to float."""
    f32 = np.float32
    f = f32(frac_num) / f32(den)
    a, b, h = f32(0.16667), f32(0.33333), f32(0.5)
    w0 = (-a) * f + a * f * f * f
    w1 = f + h * f * f - h * f * f * f
    w3 = (-b) * f + h * f * f - a * f * f * f
    w2 = f32(1.0 - float(w0) - float(w1) - float(w3))
    return [float(w0), float(w1), float(w2), float(w3)]


def phase_rows(o):
    """rows[phase, j] as float64 for a designed filter `o` (oracle.Oracle or oracle.Reference)."""
    table = o.table().astype(np.float64)
    n, den = o.taps, o.den
    if o.kind.startswith("direct"):
        return table.reshape(den, n).copy()
    rows = np.empty((den, n), np.float64)
    j = np.arange(n)
    for phase in range(den):
        w = blend_weights((phase * o.oversample) % den, den)
        t = 4 + (j + 1) * o.oversample - (phase * o.oversample) // den
        rows[phase] = w[0] * table[t - 2] + w[1] * table[t - 1] + w[2] * table[t] + w[3] * table[t + 1]
    return rows


def reference_abs_rows(o):
    """sum_i |w_i| |t_i[phase, j]|: what the REFERENCE's interpolating kernels are conditioned by.  They do not sum over
    the blended row: they run four dot products over the table (resample.c:463-481) and blend the four sums, so their
    rounding error scales with sum_i |w_i| sum_j |t_i| |x| -- which is `mag` within a few per cent where neighbouring
    samples are equally loud, and many times `mag` where one loud sample sits on a zero crossing of the blended row
    (float_inputs kind B).  The product blends the ROWS (in double) and runs one dot product: its bound is over `mag`.
    Direct kinds: |rows|."""
    table = np.abs(o.table().astype(np.float64))
    n, den = o.taps, o.den
    if o.kind.startswith("direct"):
        return table.reshape(den, n).copy()
    rows = np.empty((den, n), np.float64)
    j = np.arange(n)
    for phase in range(den):
        w = np.abs(blend_weights((phase * o.oversample) % den, den))
        t = 4 + (j + 1) * o.oversample - (phase * o.oversample) // den
        rows[phase] = w[0] * table[t - 2] + w[1] * table[t - 1] + w[2] * table[t] + w[3] * table[t + 1]
    return rows


def with_silence(x, taps, at=None):
    """x with taps + 17 frames of silence from frame `at` (default: a third of the way in).  Outputs whose window enters
    the stretch see the input through their first taps alone, those that leave it through their last taps alone (as at a
    stream's start): mag is tiny there, so an edge tap that is dropped, or a window slot fetched one off where the tap
    is tiny, is the whole sample instead of 10^-7 of it."""
    x = np.array(x)
    at = x.shape[0] // 3 if at is None else at
    x[at: at + taps + 17] = 0
    return x


def samples(frames, ch, seed, taps, tone=False):
    """One call's int16 samples, as the one-state streams of the GPU tests feed them: noise with a stretch of silence
    longer than the filter wherever one fits, or (tone) a low-amplitude tonal signal."""
    if tone:
        return orc.tone_pcm(frames, ch, seed=seed)
    x = orc.lcg_pcm(frames * ch, seed).reshape(frames, ch)
    return with_silence(x, taps) if frames > 2 * taps + 64 else x


def ulp32(v):
    """the spacing of float32 around the real value v (array): 2^(exponent - 23), subnormal spacing below 2^-126"""
    _, ex = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(ex - 24, -149))


def halfup(v):
    """the reference's float -> int16 (arch.h:208-209): floor(v + .5), saturated"""
    return np.clip(np.floor(v + 0.5), -32768, 32767).astype(np.int64)


class Model:
    """The exact model of one filter: Model(channels, in_rate, out_rate, quality).truth(consumed_input, outputs_made)."""

    def __init__(self, channels, in_rate, out_rate, quality, make=orc.Oracle):
        self._adopt(make(channels, in_rate, out_rate, quality), channels)

    def _adopt(self, o, channels):
        self.channels, self.num, self.den, self.taps, self.kind = channels, o.num, o.den, o.taps, o.kind
        self.double_kind = o.kind.endswith("double")
        self.rows = phase_rows(o)
        self.head = np.zeros((self.taps - 1, channels))
        self.last0, self.frac0 = 0, 0

    @classmethod
    def of(cls, o):
        """The model of a live oracle's (or reference's) filter as it now is, whatever calls set its ratio and quality;
        a stream's start: head zeros(taps - 1), position (0, 0)."""
        m = cls.__new__(cls)
        m._adopt(o, o.channels)
        return m

    def segment(self, head, start):
        """This filter over a segment: head[taps - 1 + pending, ch] (history ++ pending) and start = (last0, frac0)."""
        m = self.__class__.__new__(self.__class__)
        m.__dict__.update(self.__dict__)
        m.head = np.array(head, np.float64).reshape(-1, self.channels)
        assert m.head.shape[0] >= self.taps - 1, "a head holds taps - 1 frames of history at least"
        m.last0, m.frac0 = int(start[0]), int(start[1])
        return m

    def segment_of(self, o):
        """The segment that begins where the live oracle `o` stands: its history, pending frames and position."""
        cols = [np.concatenate([o.history(c), o.pending(c)]) for c in range(self.channels)]
        return self.segment(np.stack(cols, axis=1), o.position())

    @property
    def pending(self):
        return self.head.shape[0] - (self.taps - 1)

    def line(self, x):
        x = np.asarray(x, np.float64).reshape(-1, self.channels)
        return np.concatenate([self.head, x])

    def where(self, k):
        """(pos, phase) of output k (an int or an int64 array) of the segment"""
        t = self.frac0 + k * self.num
        return self.last0 + t // self.den, t % self.den

    def geometry(self, n_out):
        return self.where(np.arange(n_out, dtype=np.int64))

    def truth(self, x, n_out, rows=None):
        """-> (truth[n_out, ch], mag[n_out, ch]) in float64.  Outputs of one residue r = k % den share a phase and their
        windows start num frames apart: a strided view of the line per residue, one contraction each.
        (`rows` replaces the model's taps: how the tests plant defects.)"""
        rows = self.rows if rows is None else rows
        line = self.line(x)
        absline = np.abs(line)
        ch, n, num, den = self.channels, self.taps, self.num, self.den
        truth = np.zeros((n_out, ch))
        mag = np.zeros((n_out, ch))
        if n_out:
            last = self.where(n_out - 1)[0] + n
            assert last <= line.shape[0], "the stream made output %d before consuming frame %d" % (n_out - 1, last - n)
        fs, cs = line.strides
        for r in range(min(den, n_out)):
            count = (n_out - r + den - 1) // den
            start, phase = self.where(r)
            row = rows[phase]
            for src, dst, taps in ((line, truth, row), (absline, mag, np.abs(row))):
                win = np.lib.stride_tricks.as_strided(src[start:], (count, n, ch), (num * fs, fs, cs), writeable=False)
                dst[r::den] = np.einsum("j,njc->nc", taps, win)
        return truth, mag

    def exact_sample(self, x, k, c):
        """truth[k, c] as a Fraction (no rounding at all): the arbiter for samples a float64 check flags"""
        line = self.line(x)
        pos, phase = self.where(k)
        row = self.rows[phase]
        return sum((Fraction(float(row[j])) * Fraction(float(line[pos + j, c])) for j in range(self.taps)), Fraction(0))


def chain32(model, x, n_out, rows=None, shift=None):
    """The contract DESIGN section 4 documents for the fp32 instances: rows rounded once to fp32, ONE sequential fp32 FMA
    chain per output (tap 0 first), float32 out.  (An FMA is emulated as an exact product -- 24 x 24 bits fit a double --
    added in double and narrowed; the double rounding that differs from a true FMA has probability ~2^-29 per step.)
    `rows` replaces the model's and `shift[phase]` moves that phase's window start: how the tests plant defects."""
    rows32 = np.asarray(model.rows if rows is None else rows, np.float64).astype(np.float32).astype(np.float64)
    line = model.line(x)
    pos, phase = model.geometry(n_out)
    if shift is not None:
        pos = pos + np.asarray(shift)[phase]
    s = np.zeros((n_out, model.channels), np.float32)
    for j in range(model.taps):
        s = (rows32[phase, j][:, None] * line[pos + j] + s.astype(np.float64)).astype(np.float32)
    return s


UNDERFLOW = 2.0 ** -149     # the spacing of float32 below 2^-126


def bound32(truth, mag, taps, underflow=False):
    """(a) for fp32-accumulate instances: the textbook bound of a length-`taps` fp32 dot product in any order, with or
    without FMA, over rows rounded once to fp32, then narrowed.
    `underflow` (opt-in, input kind D): the textbook bound charges every rounding u x |value|, which is nothing for a
    value in the subnormal range -- there each of the up to 2 taps roundings (products and sums) may be off by half the
    subnormal spacing, 2^-150, whatever the value: taps 2^-149 in all."""
    return (taps + 2) * U * mag + 0.5 * ulp32(truth) + (taps * UNDERFLOW if underflow else 0.0)


def bound64(truth, mag, taps, underflow=False):
    """what an fp64-accumulate instance may be off by after narrowing to float32 (`underflow`: as bound32's)"""
    return taps * 2.0 ** -52 * mag + 0.5 * ulp32(truth) + (taps * UNDERFLOW if underflow else 0.0)


def errors(got, truth, mag):
    """e = (got - truth) / (u mag) over the samples with mag > 0, flat"""
    m = mag > 0
    return (np.asarray(got, np.float64)[m] - truth[m]) / (U * mag[m])


def rms(e):
    return float(np.sqrt(np.mean(np.square(e)))) if e.size else 0.0


def bias_ok(e):
    """(c): -> (ok, mean / (rms / sqrt(n))).  Comparisons of fewer than BIAS_MIN_SAMPLES samples pass unjudged."""
    if e.size < BIAS_MIN_SAMPLES or rms(e) == 0.0:
        return True, 0.0
    z = float(np.mean(e)) / (rms(e) / np.sqrt(e.size))
    return abs(z) <= BIAS_SIGMAS, z


def _describe(model, idx, got, truth, mag, tile=None):
    k, c = (int(v) for v in idx)
    pos, phase = model.where(k)
    return "output %d ch %d (phase %d, pos %d%s): got %r, truth %.17g, mag %.6g, e = %.3g" % (
        k, c, phase, pos, "" if not tile else ", pos %% %d = %d" % (tile, pos % tile), got[k, c], truth[k, c], mag[k, c],
        (float(got[k, c]) - truth[k, c]) / (U * mag[k, c]) if mag[k, c] > 0 else float("nan"))


def _worst_phase(model, bad):
    k = np.nonzero(bad.any(axis=1))[0]
    phases = model.where(k)[1]
    vals, counts = np.unique(phases, return_counts=True)
    return "%d samples fail; worst phase %d (%d of them); first %s" % (
        int(bad.sum()), int(vals[np.argmax(counts)]), int(counts.max()), [int(v) for v in k[:6]])


def hard_float(model, x, got, truth, mag, bits, tile=None, underflow=False):
    """(a) on a float call's output -> list of failure messages (empty: passed).
    bits 32: |got - truth| <= (taps + 2) u mag + 1/2 ulp32(truth).
    bits 64: got is a float32 neighbour of truth, and the correctly rounded one unless truth lies within
             taps 2^-52 mag of the midpoint of its two neighbours.
    underflow (input kind D): |got - truth| <= the instance's bound with its underflow term, for either `bits`."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == truth.shape, (got.dtype, got.shape, truth.shape)
    g = got.astype(np.float64)
    if bits == 32 or underflow:
        slack = (bound32 if bits == 32 else bound64)(truth, mag, model.taps, underflow)
        bad = ~(np.abs(g - truth) <= slack)

        def still_bad(k, c):
            t = model.exact_sample(x, k, c)
            return abs(Fraction(float(g[k, c])) - t) > Fraction(float(slack[k, c]))
    else:
        near = truth.astype(np.float32)
        below = np.where(near.astype(np.float64) <= truth, near, np.nextafter(near, np.float32(-np.inf)))
        above = np.nextafter(below, np.float32(np.inf))
        mid = 0.5 * (below.astype(np.float64) + above.astype(np.float64))
        room = model.taps * 2.0 ** -52 * mag
        # (the float64 truth carries up to taps 2^-53 mag = room / 2 of its own error: it settles the samples that are
        #  clearly outside the midpoint zone or clearly inside it, the arbiter the rest)
        off = np.abs(truth - mid)
        bad = ~((got == near) & (off > 1.5 * room) | ((got == below) | (got == above)) & (off <= 0.5 * room))

        def still_bad(k, c):
            t = model.exact_sample(x, k, c)
            lo, hi = Fraction(float(below[k, c])), Fraction(float(above[k, c]))
            if t < lo:      # the float64 truth sat on the wrong side of a float32 value
                lo, hi = Fraction(float(np.nextafter(below[k, c], np.float32(-np.inf)))), lo
            elif t > hi:
                lo, hi = hi, Fraction(float(np.nextafter(above[k, c], np.float32(np.inf))))
            gv, m = Fraction(float(g[k, c])), (lo + hi) / 2
            if gv not in (lo, hi):
                return True
            right = lo if t < m else hi if t > m else gv
            return gv != right and abs(t - m) > Fraction(float(room[k, c]))
    return _settle(model, bad, still_bad, got, truth, mag, tile)


def hard_int16(model, x, got, truth, mag, bits, tile=None):
    """(a) on an int16 call's output: got in [halfup(truth - B), halfup(truth + B)], both ends saturated -- so a sample
    may differ from halfup(truth) only where the truth is within B of a rounding boundary, and the rails are the clamp
    of the interval, not an exemption."""
    got = np.asarray(got)
    assert got.dtype == np.int16 and got.shape == truth.shape, (got.dtype, got.shape, truth.shape)
    slack = (bound32 if bits == 32 else bound64)(truth, mag, model.taps)
    g = got.astype(np.int64)
    bad = ~((g >= halfup(truth - slack)) & (g <= halfup(truth + slack)))

    def still_bad(k, c):
        t, b = model.exact_sample(x, k, c), Fraction(float(slack[k, c]))
        lo, hi = ((v + Fraction(1, 2)).__floor__() for v in (t - b, t + b))
        return not max(-32768, min(32767, lo)) <= int(g[k, c]) <= max(-32768, min(32767, hi))
    return _settle(model, bad, still_bad, got, truth, mag, tile)


def _settle(model, bad, still_bad, got, truth, mag, tile):
    if not bad.any():
        return []
    idx = np.argwhere(bad)
    if len(idx) <= _RECHECK_LIMIT:
        idx = [i for i in idx if still_bad(int(i[0]), int(i[1]))]
        if not idx:
            return []
        bad = np.zeros_like(bad)
        for i in idx:
            bad[i[0], i[1]] = True
    return [_worst_phase(model, bad)] + [_describe(model, i, got, truth, mag, tile) for i in idx[:4]]


MARGIN = 1.5    # (b): rms(e_kernel) <= MARGIN rms(e_yardstick); an fp64-accumulate instance gets 1.0 against the oracle


def judge_float(model, x, got, truth, mag, bits, yardstick, margin=MARGIN, tile=None, underflow=False):
    """(a), (b) and (c) on one float comparison -> (failures, stats).  `yardstick`: the float32 output of the oracle or
    of chain32 on the same input (None: (b) is not judged).  underflow: (a) alone, with the bounds' underflow term --
    e = error / (u mag) means nothing where the error is an absolute 2^-150 per rounding."""
    fails = ["(a) " + m for m in hard_float(model, x, got, truth, mag, bits, tile, underflow)]
    if underflow:
        return fails, {"n": int((mag > 0).sum()), "rms": 0.0, "max": 0.0, "z": 0.0}
    e = errors(got, truth, mag)
    stats = {"n": int(e.size), "rms": rms(e), "max": float(np.abs(e).max(initial=0.0))}
    if yardstick is not None:
        stats["yard"] = rms(errors(yardstick, truth, mag))
        if not stats["rms"] <= margin * stats["yard"]:
            fails.append("(b) rms(e) = %.4g > %.2f x %.4g, the yardstick's" % (stats["rms"], margin, stats["yard"]))
    ok, stats["z"] = bias_ok(e)
    if not ok:
        fails.append("(c) mean(e) = %.4g is %.1f sigma from 0 on %d samples" % (float(np.mean(e)), stats["z"], e.size))
    return fails, stats
