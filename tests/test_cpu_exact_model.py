"""Pins tests/exact_model.py without a GPU and proves that its checks bite: the oracle (and the reference's own C where it
is built) passes the hard check (a) and the bias check (c) on all four kernel kinds; a multi-call ragged stream has the
one-call truth; every planted defect of the documented fp32 chain fails a check while the clean chain passes them all.
The same on real float input (tests/float_inputs.py): the oracle and the clean chain pass on every kind with the bounds
as they stand, and each kind's own defect -- an int16 or float16 image of the window, a 2^-22 leak between channels, a
clamp, a flush of quiet passages or of subnormals -- fails the hard check."""
import numpy as np
import pytest

import exact_model as em
import float_inputs as fi
import oracle as orc

FRAMES = 30000
CASES = [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (8, 48000, 44100, 5), (1, 24000, 48000, 5), (2, 48000, 11025, 7),
         (1, 48000, 8000, 10), (2, 44100, 48000, 10), (2, 44100, 48000, 1), (1, 16000, 48000, 7), (2, 192000, 8000, 10)]


def _input(source, frames, ch, seed=5):
    return orc.lcg_pcm(frames * ch, seed).reshape(frames, ch) if source == "lcg" else orc.tone_pcm(frames, ch, seed=seed)


@pytest.mark.parametrize("source", ["lcg", "tone"])
@pytest.mark.parametrize("ch,i,o,q", CASES)
def test_the_oracle_and_the_reference_pass_the_hard_and_the_bias_check(ch, i, o, q, source):
    x = _input(source, FRAMES, ch)
    xf = x.astype(np.float32)
    model = em.Model(ch, i, o, q)
    kinds = set()
    for make in [orc.Oracle] + ([orc.Reference] if orc.have_reference() else []):
        assert np.array_equal(em.phase_rows(make(ch, i, o, q)), model.rows)
        got, used = make(ch, i, o, q).process_float(xf, 1 << 20)
        truth, mag = model.truth(xf[:used], got.shape[0])
        # (the reference's kernels round every product to fp32, the double ones too: the fp32 bound is theirs)
        fails, stats = em.judge_float(model, xf[:used], got, truth, mag, 32, None)
        print("%s %s %s %s: rms(e) %.3f max|e| %.2f bias %.2f sigma" % (make.__name__, (ch, i, o, q), source, model.kind,
                                                                       stats["rms"], stats["max"], stats["z"]))
        assert not fails, fails
        # measured: <= 11.7 on the single kinds (the bound is taps + 2 >= 18), <= 1.31 on the double kinds
        assert stats["max"] <= (2.0 if model.double_kind else model.taps + 2)
        got16, used16 = make(ch, i, o, q).process(x, 1 << 20)
        assert used16 == used and got16.shape == truth.shape
        fails = em.hard_int16(model, x[:used], got16, truth, mag, 32)
        assert not fails, fails
        kinds.add(model.kind)
    assert kinds <= set(orc.KIND_NAMES)


def test_the_cases_cover_all_four_kinds():
    assert {em.Model(*c).kind for c in CASES} == set(orc.KIND_NAMES)


def test_saturated_samples_are_judged_as_the_clamp_of_the_interval():
    ch, i, o, q = 2, 44100, 48000, 7
    x = _input("lcg", FRAMES, ch, seed=12345)
    model = em.Model(ch, i, o, q)
    got, used = orc.Oracle(ch, i, o, q).process(x, 1 << 20)
    truth, mag = model.truth(x[:used], got.shape[0])
    assert got.min() == -32768 and got.max() == 32767 and truth.max() > 32768 and truth.min() < -32769
    assert not em.hard_int16(model, x[:used], got, truth, mag, 32)
    # a rail sample pulled off its rail, and a sample pushed onto it, both fail
    for (value, moved) in ((32767, 32766), (-32768, -32767)):
        bad = got.copy()
        k, c = np.argwhere((got == value) & (np.abs(truth) > 32800))[0]
        bad[k, c] = moved
        assert em.hard_int16(model, x[:used], bad, truth, mag, 32)
    bad = got.copy()
    k, c = np.argwhere(np.abs(truth) < 30000)[0]
    bad[k, c] = 32767
    assert em.hard_int16(model, x[:used], bad, truth, mag, 32)


@pytest.mark.parametrize("ch,i,o,q", [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (2, 48000, 11025, 7), (3, 48000, 8000, 9)])
def test_a_multi_call_ragged_stream_has_the_one_call_truth(ch, i, o, q):
    total = 26000
    x = _input("lcg", total, ch, seed=9)
    xf = x.astype(np.float32)
    model = em.Model(ch, i, o, q)
    one, used_one = orc.Oracle(ch, i, o, q).process_float(xf, 1 << 20)
    assert used_one == total
    truth_one, mag_one = model.truth(xf, one.shape[0])
    ref = orc.Oracle(ch, i, o, q)
    outs, consumed, off = [], [], 0
    # ragged sizes, an empty call, a 1-frame call and a capacity-bound call (which leaves input behind)
    for (n, cap) in [(1, 1 << 20), (4999, 1 << 20), (0, 1 << 20), (7000, 7000 * o // i // 3), (9001, 1 << 20), (333, 1 << 20)]:
        y, u = ref.process_float(xf[off: off + n], cap)
        assert u <= n and y.shape[0] <= cap
        if cap < 1 << 20:
            assert u < n and y.shape[0] == cap
        outs.append(y)
        consumed.append(xf[off: off + u])
        off += u
    got, fed = np.concatenate(outs), np.concatenate(consumed)
    assert np.array_equal(fed, xf[:off]) and 0 < got.shape[0] < one.shape[0]
    truth, mag = model.truth(fed, got.shape[0])
    assert np.array_equal(truth, truth_one[: got.shape[0]]) and np.array_equal(mag, mag_one[: got.shape[0]])
    assert np.array_equal(got, one[: got.shape[0]])      # the reference does not depend on chunking
    fails, _ = em.judge_float(model, fed, got, truth, mag, 32, None)
    assert not fails, fails
    # ... and the model refuses an output the stream cannot have made yet
    with pytest.raises(AssertionError):
        model.truth(fed, got.shape[0] + 1)


def _to_pcm(v, truncate=False):
    v = v.astype(np.float64)
    return np.clip(np.trunc(v) if truncate else np.floor(v + 0.5), -32768, 32767).astype(np.int16)


def _setup(ch, i, o, q, source="lcg"):
    """Noise with one stretch of silence longer than the filter.  A stream starts on a line of zeros, so its first outputs
    see the input through the LAST taps alone; the outputs behind the stretch do so again, and those that enter it see
    the input through the FIRST taps alone -- there mag is tiny and a lost or misplaced edge tap is the whole sample."""
    model = em.Model(ch, i, o, q)
    x = em.with_silence(_input(source, FRAMES, ch, seed=3), model.taps)
    xf = x.astype(np.float32)
    want, used = orc.Oracle(ch, i, o, q).process_float(xf, 1 << 20)
    n = want.shape[0] - model.den      # (room for the defect that reads one frame further)
    truth, mag = model.truth(xf, n)
    return model, xf, want[:n], truth, mag, n


def _all_checks(model, xf, got, truth, mag, bits, yard):
    fails, stats = em.judge_float(model, xf, got, truth, mag, bits, yard, margin=em.MARGIN if bits == 32 else 1.0)
    fails += ["(a, int16) " + m for m in em.hard_int16(model, xf, _to_pcm(got), truth, mag, bits)]
    return fails, stats


# the two cases whose dropped last tap today's bars let through, an up-sampler and a direct-kind decimator
DEFECT_CASES = [(1, 24000, 48000, 10), (2, 48000, 11025, 7), (2, 44100, 48000, 7), (2, 48000, 8000, 5)]


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
def test_the_clean_fp32_chain_passes_every_check(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup(ch, i, o, q)
    clean = em.chain32(model, xf, n)
    # the yardstick of (b): the oracle on the single kinds; on a double kind the chain is its own (an fp32 instance there
    # is judged against chain32 -- the oracle's double kernels are 8x closer)
    yard = clean if model.double_kind else oracle_out
    fails, stats = _all_checks(model, xf, clean, truth, mag, 32, yard)
    print("chain32 %s: rms(e) %.3f (oracle %.3f) max|e| %.2f bias %.2f sigma" % (
        (ch, i, o, q), stats["rms"], em.rms(em.errors(oracle_out, truth, mag)), stats["max"], stats["z"]))
    assert not fails, fails


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
@pytest.mark.parametrize("defect", ["last tap dropped", "first tap dropped", "window one frame off in one phase",
                                    "truncation instead of half-up"])
def test_every_planted_defect_of_the_fp32_chain_fails_a_check(ch, i, o, q, defect):
    model, xf, oracle_out, truth, mag, n = _setup(ch, i, o, q)
    yard = em.chain32(model, xf, n) if model.double_kind else oracle_out
    rows, shift, got16 = model.rows.copy(), None, None
    if defect == "last tap dropped":
        rows[:, -1] = 0.0
    elif defect == "first tap dropped":
        rows[:, 0] = 0.0
    elif defect == "window one frame off in one phase":
        shift = np.zeros(model.den, np.int64)
        shift[model.den // 2] = 1
    got = em.chain32(model, xf, n, rows=rows, shift=shift)
    if defect == "truncation instead of half-up":
        fails = ["(a, int16) " + m for m in em.hard_int16(model, xf, _to_pcm(got, truncate=True), truth, mag, 32)]
    else:
        fails, _ = _all_checks(model, xf, got, truth, mag, 32, yard)
    assert fails, defect + " went through"
    assert any(f.startswith("(a") for f in fails), (defect, fails)     # each of these is a per-sample matter


@pytest.mark.parametrize("ch,i,o,q", [c for c in DEFECT_CASES if c[0] > 1] + [(8, 48000, 44100, 5)])
def test_a_channel_taken_from_its_neighbour_fails_the_hard_check(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup(ch, i, o, q)
    got = em.chain32(model, xf, n)
    got[:, ch - 2] = got[:, ch - 1]
    fails, _ = _all_checks(model, xf, got, truth, mag, 32, oracle_out)
    assert any(f.startswith("(a)") for f in fails) and any(f.startswith("(a, int16)") for f in fails), fails


def test_bias_or_noise_inside_the_per_sample_bound_fails_the_statistical_checks_alone():
    """What only (b) and (c) see: errors that stay inside the per-sample bound."""
    ch, i, o, q = 2, 44100, 48000, 7
    model, xf, oracle_out, truth, mag, n = _setup(ch, i, o, q)
    clean = em.chain32(model, xf, n)
    assert not em.judge_float(model, xf, clean, truth, mag, 32, oracle_out)[0]
    up = np.nextafter(clean, np.float32(np.inf))                         # every sample rounded up once more
    fails, _ = em.judge_float(model, xf, up, truth, mag, 32, oracle_out)
    assert fails and all(f.startswith("(c)") or f.startswith("(b)") for f in fails) and any(f.startswith("(c)") for f in fails), fails
    rng = np.random.RandomState(1)
    noisy = (clean.astype(np.float64) + rng.standard_normal(clean.shape) * 3.0 * em.U * mag).astype(np.float32)
    fails, _ = em.judge_float(model, xf, noisy, truth, mag, 32, oracle_out)
    assert any(f.startswith("(b)") for f in fails), fails


@pytest.mark.parametrize("ch,i,o,q", [(2, 44100, 48000, 10), (1, 24000, 48000, 10), (2, 44100, 8000, 9)])
def test_claiming_64_bit_accumulation_takes_64_bit_accuracy(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup(ch, i, o, q)
    assert model.double_kind
    # the correctly rounded truth passes as an fp64 instance and is no worse than the oracle
    honest = truth.astype(np.float32)
    fails, stats = _all_checks(model, xf, honest, truth, mag, 64, oracle_out)
    assert not fails, fails
    # an "fp64" instance that sums in fp32
    fails, _ = _all_checks(model, xf, em.chain32(model, xf, n), truth, mag, 64, oracle_out)
    assert any(f.startswith("(a)") for f in fails) and any(f.startswith("(b)") for f in fails), fails
    # the oracle itself (fp32-rounded products) is not an fp64 instance either
    assert em.hard_float(model, xf, oracle_out, truth, mag, 64)
    # rows rounded to fp32 under an fp64 sum: only the interpolating kinds have rows that are not fp32 already
    rows32 = model.rows.astype(np.float32).astype(np.float64)
    got = model.truth(xf, n, rows=rows32)[0].astype(np.float32)
    if model.kind == "interpolate_double":
        assert not np.array_equal(rows32, model.rows)
        assert em.hard_float(model, xf, got, truth, mag, 64), "fp32 rows went through as an fp64 instance"
    else:
        assert np.array_equal(rows32, model.rows) and not em.hard_float(model, xf, got, truth, mag, 64)


def test_blend_weights_are_the_reference_s_float_arithmetic():
    # f = 0: the row is the table itself; the weights sum to 1 within the float rounding of the one at index 2
    assert em.blend_weights(0, 160) == [0.0, 0.0, 1.0, 0.0]
    for (fn, den) in [(1, 160), (53, 147), (639, 640)]:
        w = em.blend_weights(fn, den)
        assert all(float(np.float32(v)) == v for v in w) and abs(sum(w) - 1.0) < 2.0 ** -24


# ---- real float input (tests/float_inputs.py) ----
FLOAT_KINDS = "ABCGEP"      # (D: gradual underflow, judged with the underflow term, below)


REFERENCE_OVER_ITS_OWN_CONDITIONING = (2, 44100, 48000, 1, "B")


def _kinds_of(cases, kinds=FLOAT_KINDS):
    return [c + (k,) for c in cases for k in kinds if k != "C" or c[0] >= 2]


@pytest.mark.parametrize("ch,i,o,q,kind", _kinds_of(CASES))
def test_the_oracle_and_the_reference_pass_on_every_float_kind(ch, i, o, q, kind):
    model = em.Model(ch, i, o, q)
    xf = fi.make(kind, FRAMES, ch, 1, model.taps)
    for make in [orc.Oracle] + ([orc.Reference] if orc.have_reference() else []):
        got, used = make(ch, i, o, q).process_float(xf, 1 << 20)
        assert used == FRAMES
        truth, mag = model.truth(xf, got.shape[0])
        if (ch, i, o, q, kind) == REFERENCE_OVER_ITS_OWN_CONDITIONING:
            # The reference blends four SUMS, not the rows: its error scales with em.reference_abs_rows, not with mag.
            # Measured with mag itself: this case fails (a) on 11 samples of 65 000, max|e| 138.9 against taps + 2 = 18 -- a
            # loud sample on a zero crossing of the blended row.  The bound over the reference's own conditioning is the
            # textbook one for what it computes.  Every other case and kind is judged over mag, as the product always is.
            assert model.kind == "interpolate_single"
            mag = model.truth(xf, got.shape[0], rows=em.reference_abs_rows(make(ch, i, o, q)))[1]
        fails, stats = em.judge_float(model, xf, got, truth, mag, 32, None)
        print("%s %s kind %s %s: rms(e) %.3f max|e| %.2f bias %.2f sigma" % (make.__name__, (ch, i, o, q), kind, model.kind,
                                                                             stats["rms"], stats["max"], stats["z"]))
        assert not fails, fails
        if kind == "E":
            assert np.abs(got).max() > 2.0 ** 90 and np.isfinite(got).all()


@pytest.mark.parametrize("ch,i,o,q", CASES)
def test_the_oracle_and_the_reference_keep_subnormals(ch, i, o, q):
    """Kind D: without the underflow term the ORACLE fails (a) -- a gap of the bound, not of the reference --, with it the
    oracle passes and an output flushed to zero below 2^-126 does not."""
    model = em.Model(ch, i, o, q)
    xf = fi.make("D", FRAMES, ch, 1, model.taps)
    assert 0 < np.abs(xf[xf != 0]).min() < 2.0 ** -126 < np.abs(xf).max()
    for make in [orc.Oracle] + ([orc.Reference] if orc.have_reference() else []):
        got, used = make(ch, i, o, q).process_float(xf, 1 << 20)
        truth, mag = model.truth(xf, got.shape[0])
        fails, _ = em.judge_float(model, xf, got, truth, mag, 32, None, underflow=True)
        assert not fails, fails
        assert ((got != 0) & (np.abs(got) < 2.0 ** -126)).any()
    flushed = np.where(np.abs(got) < 2.0 ** -126, np.float32(0), got)
    assert em.hard_float(model, xf, flushed, truth, mag, 32, underflow=True), "a flush to zero went through"
    # ... and what claims fp64 accumulation: the correctly rounded truth passes, its flush does not
    honest = truth.astype(np.float32)
    assert not em.hard_float(model, xf, honest, truth, mag, 64, underflow=True)
    assert em.hard_float(model, xf, np.where(np.abs(honest) < 2.0 ** -126, np.float32(0), honest), truth, mag, 64, underflow=True)


def test_the_underflow_term_is_opt_in_and_what_the_docstring_derives():
    truth, mag = np.array([[1.0, 2.0 ** -130]]), np.array([[3.0, 2.0 ** -128]])
    for bound in (em.bound32, em.bound64):
        assert np.array_equal(bound(truth, mag, 64, True), bound(truth, mag, 64) + 64 * 2.0 ** -149)
        assert (bound(truth, mag, 64, True) > bound(truth, mag, 64))[0, 1]
        assert np.array_equal(bound(truth, mag, 64), bound(truth, mag, 64, underflow=False))
    assert np.array_equal(em.bound32(truth, mag, 64), (64 + 2) * em.U * mag + 0.5 * em.ulp32(truth))
    assert np.array_equal(em.bound64(truth, mag, 64), 64 * 2.0 ** -52 * mag + 0.5 * em.ulp32(truth))


def _setup_kind(ch, i, o, q, kind, seed=1):
    model = em.Model(ch, i, o, q)
    xf = fi.make(kind, FRAMES, ch, seed, model.taps)
    want, used = orc.Oracle(ch, i, o, q).process_float(xf, 1 << 20)
    n = want.shape[0] - model.den
    truth, mag = model.truth(xf, n)
    return model, xf, want[:n], truth, mag, n


@pytest.mark.parametrize("ch,i,o,q,kind", _kinds_of(DEFECT_CASES))
def test_the_clean_fp32_chain_passes_every_check_on_every_float_kind(ch, i, o, q, kind):
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, kind)
    clean = em.chain32(model, xf, n)
    yard = clean if model.double_kind else oracle_out
    fails, stats = _all_checks(model, xf, clean, truth, mag, 32, yard)
    print("chain32 %s kind %s: rms(e) %.3f (oracle %.3f) max|e| %.2f bias %.2f sigma" % (
        (ch, i, o, q), kind, stats["rms"], em.rms(em.errors(oracle_out, truth, mag)), stats["max"], stats["z"]))
    assert not fails, fails


def _a_fails(fails):
    return [f for f in fails if f.startswith("(a)")], [f for f in fails if f.startswith("(a, int16)")]


# As an fp32 chain, the cases whose int16 OUTPUT shows an int16 image of kind P input: error 0.28 LSB rms against a bound
# (median) of 0.24 and 0.11 LSB.  Not (2, 48000, 11025, 7): 0.13 against 0.48; nor (2, 48000, 8000, 5): 0.11 against 0.38.
INT16_IMAGE_SHOWS_ON_INT16_OUTPUT = {(1, 24000, 48000, 10), (2, 44100, 48000, 7)}
# ... and of the mixed streams (case, float frames) those whose fp32 chain fails hard_int16 behind the float frames
MIXED_FP32_CHAIN_FAILS = {((2, 44100, 16000, 7), "fewer than taps - 1"), ((2, 44100, 16000, 7), "more"),
                          ((4, 48000, 11025, 5), "more")}


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
def test_an_int16_window_on_float_data_fails_the_hard_check(ch, i, o, q):
    """kind P: input frames rounded to integers -- half a tap per frame at most, 0.13 to 0.28 LSB rms in all, which the
    +-1 LSB bars cannot see.  The float output fails (a) on every case.  The int16 output fails it wherever the bound is
    tighter than that error (INT16_IMAGE_SHOWS_ON_INT16_OUTPUT lists those cases); measured here: it is NOT on (2, 48000, 11025, 7) -- 560 taps, a bound of 0.48 LSB (median)
    at kind P's amplitude against an error of 0.13 LSB rms, 0 of 13 500 samples outside their interval -- so what an
    fp32 instance of that filter does to int16 output through an int16 image is inside its own textbook bound, and
    only its float output (and the fp64 instances, whose bound is the rounding itself) can show it."""
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, "P")
    got = em.chain32(model, np.rint(xf), n)
    fl, i16 = _a_fails(_all_checks(model, xf, got, truth, mag, 32, None)[0])
    err = float(np.std(got.astype(np.float64) - truth))
    bound = float(np.median(em.bound32(truth, mag, model.taps)))
    print("int16 image %s: error %.3f LSB rms, bound %.3f LSB (median); float fails %d, int16 fails %d" % (
        (ch, i, o, q), err, bound, len(fl), len(i16)))
    assert fl, "the int16 image went through on float output"
    assert bool(i16) == ((ch, i, o, q) in INT16_IMAGE_SHOWS_ON_INT16_OUTPUT), "int16 output: %d failures" % len(i16)
    # as an fp64 instance (bound: the rounding itself) every case fails on both outputs
    got64 = model.truth(np.rint(xf), n)[0].astype(np.float32)
    fl, i16 = _a_fails(_all_checks(model, xf, got64, truth, mag, 64, None)[0])
    assert fl and i16, (fl, i16)


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
def test_a_float16_window_fails_the_hard_check(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, "A")
    got = em.chain32(model, xf.astype(np.float16).astype(np.float32), n)
    assert _a_fails(_all_checks(model, xf, got, truth, mag, 32, None)[0])[0]


@pytest.mark.parametrize("ch,i,o,q", [c for c in DEFECT_CASES if c[0] > 1] + [(8, 48000, 44100, 5)])
def test_a_leak_of_2_to_the_minus_22_shows_only_next_to_a_quiet_channel(ch, i, o, q):
    """why kind C exists: between equally loud channels the leak is 4 u, inside the (taps + 2) u mag bound"""
    for kind, caught in (("A", False), ("C", True)):
        model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, kind)
        got = em.chain32(model, xf, n)
        got[:, 1] += np.float32(2.0 ** -22) * got[:, 0]
        assert bool(em.hard_float(model, xf, got, truth, mag, 32)) == caught, (kind, caught)


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
def test_a_clamp_to_the_int16_range_on_the_float_path_fails(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, "E")
    got = np.clip(em.chain32(model, xf, n), -32768, 32767).astype(np.float32)
    assert em.hard_float(model, xf, got, truth, mag, 32)
    # ... and so does a rounding to integers where the float output is small
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, "P")
    assert em.hard_float(model, xf, np.rint(em.chain32(model, xf, n)), truth, mag, 32)


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES)
def test_quiet_passages_flushed_to_zero_fail(ch, i, o, q):
    model, xf, oracle_out, truth, mag, n = _setup_kind(ch, i, o, q, "G")
    flushed = xf.copy()
    flushed[fi.quiet_frames(FRAMES)] = 0
    assert em.hard_float(model, xf, em.chain32(model, flushed, n), truth, mag, 32)
    # the same as an absolute floor on the output
    got = em.chain32(model, xf, n)
    assert em.hard_float(model, xf, np.where(np.abs(got) < 2.0 ** -16, np.float32(0), got), truth, mag, 32)


@pytest.mark.parametrize("ch,i,o,q", [(2, 48000, 11025, 7), (4, 48000, 11025, 5), (2, 44100, 16000, 7), (2, 48000, 11025, 10)])
@pytest.mark.parametrize("float_frames", ["fewer than taps - 1", "more"])
def test_a_mixed_stream_whose_float_frames_went_through_an_int16_image_fails(ch, i, o, q, float_frames):
    """The line of a stream of int16, float (kind P) and int16 calls.  Clean, the int16 outputs behind the float frames pass
    hard_int16; computed from a line whose float frames were rounded to integers (an int16 window over a history that holds
    fractions) they fail -- as an fp64 instance on every case, as an fp32 chain where its bound is tighter than the
    image's error (see test_an_int16_window_on_float_data_fails_the_hard_check: of the 500-tap filters' few hundred
    samples behind the float frames none need leave an interval 0.5 LSB wide)."""
    model = em.Model(ch, i, o, q)
    taps = model.taps
    nf = taps // 3 if float_frames.startswith("fewer") else 3 * taps
    head = _input("lcg", 9000, ch, seed=21).astype(np.float32)
    mid = fi.make("P", nf, ch, 5)
    tail = em.with_silence(_input("lcg", 9000, ch, seed=22), taps, at=0).astype(np.float32)
    line = np.concatenate([head, mid, tail])
    dirty = np.concatenate([head, np.rint(mid), tail])
    n_out = (line.shape[0] - 1) * model.den // model.num
    first = -(-(9000 + nf) * model.den // model.num)       # the outputs of the int16 call behind the float frames
    truth, mag = model.truth(line, n_out)
    for (src, must_fail) in ((line, False), (dirty, True)):
        fails64 = _hard_int16_tail(model, line, _to_pcm(model.truth(src, n_out)[0]), truth, mag, first, 64)
        assert bool(fails64) == must_fail, (must_fail, fails64)
        fails32 = _hard_int16_tail(model, line, _to_pcm(em.chain32(model, src, n_out)), truth, mag, first, 32)
        print("%s %s, float frames %s: fp32 chain fails %d" % ((ch, i, o, q), "dirty" if must_fail else "clean", float_frames, len(fails32)))
        assert bool(fails32) == (must_fail and ((ch, i, o, q), float_frames) in MIXED_FP32_CHAIN_FAILS), fails32


def _hard_int16_tail(model, line, got, truth, mag, first, bits):
    """hard_int16 on the outputs from `first` on (the others are masked as correct)"""
    masked = got.copy()
    masked[:first] = em.halfup(truth[:first]).astype(np.int16)
    return em.hard_int16(model, line, masked, truth, mag, bits)
