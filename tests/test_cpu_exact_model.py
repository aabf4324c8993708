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


# ---- segments: streams after mid-stream control calls (tests/control_scripts.py) ----
import control_scripts as cs

ALL_SCRIPTS = list(cs.SCRIPTS) + list(cs.EXTRA)


def _legacy_truth(model, x, n_out):
    """truth and mag as Model.truth computed them before it knew segments: a stream from its start"""
    line = np.concatenate([np.zeros((model.taps - 1, model.channels)), np.asarray(x, np.float64)])
    absline, (fs, cs_) = np.abs(line), line.strides
    truth, mag = np.zeros((n_out, model.channels)), np.zeros((n_out, model.channels))
    for r in range(min(model.den, n_out)):
        count = (n_out - r + model.den - 1) // model.den
        start, row = r * model.num // model.den, model.rows[r * model.num % model.den]
        for src, dst, taps in ((line, truth, row), (absline, mag, np.abs(row))):
            win = np.lib.stride_tricks.as_strided(src[start:], (count, model.taps, model.channels),
                                                  (model.num * fs, fs, cs_), writeable=False)
            dst[r::model.den] = np.einsum("j,njc->nc", taps, win)
    return truth, mag


def _legacy_chain32(model, x, n_out):
    rows32 = model.rows.astype(np.float32).astype(np.float64)
    line = np.concatenate([np.zeros((model.taps - 1, model.channels)), np.asarray(x, np.float64)])
    k = np.arange(n_out, dtype=np.int64)
    pos, phase = k * model.num // model.den, k * model.num % model.den
    s = np.zeros((n_out, model.channels), np.float32)
    for j in range(model.taps):
        s = (rows32[phase, j][:, None] * line[pos + j] + s.astype(np.float64)).astype(np.float32)
    return s


@pytest.mark.parametrize("ch,i,o,q", DEFECT_CASES + [(8, 48000, 44100, 5), (2, 44100, 48000, 10)])
def test_a_segment_with_a_zero_head_at_the_start_is_the_stream_model_bit_for_bit(ch, i, o, q):
    xf = _input("lcg", 9000, ch, seed=4).astype(np.float32)
    model = em.Model(ch, i, o, q)
    n = (9000 - 1) * model.den // model.num
    want = _legacy_truth(model, xf, n) + (_legacy_chain32(model, xf, n),)
    live = orc.Oracle(ch, i, o, q)
    for m in (model, model.segment(np.zeros((model.taps - 1, ch)), (0, 0)), em.Model.of(live), em.Model.of(live).segment_of(live)):
        assert (m.last0, m.frac0, m.pending) == (0, 0, 0) and np.array_equal(m.rows, model.rows)
        truth, mag = m.truth(xf, n)
        assert truth.tobytes() == want[0].tobytes() and mag.tobytes() == want[1].tobytes()
        assert em.chain32(m, xf, n).tobytes() == want[2].tobytes()
        assert m.exact_sample(xf, n - 1, ch - 1) == model.exact_sample(xf, n - 1, ch - 1)


def test_a_model_of_a_live_oracle_follows_set_rate_frac_and_set_quality():
    o = orc.Oracle(2, 44100, 48000, 7)
    assert o.set_rate_frac(3, 2, 48000, 32000) == 0 and o.set_quality(10) == 0
    m, fresh = em.Model.of(o), orc.Oracle(2, 48000, 32000, 10, ratio=(3, 2))
    assert (m.num, m.den, m.taps, m.kind) == (3, 2, fresh.taps, fresh.kind) and np.array_equal(m.rows, em.phase_rows(fresh))


def test_the_scripts_use_every_op_and_cover_all_four_kinds():
    ops = {(op[1] if op[0] == "short" else op[0]) for s in cs.SCRIPTS.values() for op in s[4]}
    assert ops == {"set_rate", "set_rate_frac", "set_quality", "skip_zeros", "reset_mem"}
    quals = [(a["quality"], b["quality"]) for n in cs.SCRIPTS for a, b in zip(cs.record(n, cs.streams_of(n)[-1]),
                                                                               cs.record(n, cs.streams_of(n)[-1])[1:])]
    assert any(a < b for a, b in quals) and any(a > b for a, b in quals)
    assert {g["key"][3] for n in cs.SCRIPTS for g in cs.record(n, cs.streams_of(n)[-1])} == set(orc.KIND_NAMES)
    # a capacity-bound call leaves pending frames partly drained before the next op, which grows or shrinks the filter
    partly = [(n, g["index"]) for n in cs.SCRIPTS for g in cs.record(n, cs.streams_of(n)[-1])
              if g["short"] and 0 < g["calls"][-1]["head"].shape[0] - (g["key"][2] - 1) < g["model"].pending]
    assert len(partly) >= 2, partly
    # one coalesced call per script, its first chunk shorter than the pending count wherever a script leaves pending frames
    for n in cs.SCRIPTS:
        chunked = [g for g in cs.record(n, cs.streams_of(n)[-1]) if g["chunked"]]
        assert len(chunked) == 1 and [c["group"] for c in chunked[0]["calls"]][:3] == [0, 0, 0]
        if any(g["model"].pending and not g["short"] for g in cs.record(n, cs.streams_of(n)[-1])):
            assert 0 < chunked[0]["calls"][0]["x"].shape[0] < chunked[0]["model"].pending, n
    # the mixed stream: an int16 call right after an op over a head that holds fractions, and the other way round
    firsts = [(g["calls"][0]["io"], bool((g["head"] != np.rint(g["head"])).any())) for g in cs.record("mixed data", "mixed")[1:]]
    assert ("int16", True) in firsts and any(io == "float" for io, _ in firsts), firsts


def test_every_filter_a_script_visits_has_a_segment_long_enough_for_the_statistics():
    """what the GPU tests assert of their own runs, on the oracle alone: (b) and (c) are computed on every distinct filter"""
    for name in cs.SCRIPTS:
        segs = cs.record(name, cs.streams_of(name)[-1])
        judged = {g["key"] for g in segs if (cs.judge(g, [c["want"] for c in g["calls"]], 32)[1] or {}).get("judged")}
        assert judged == {g["key"] for g in segs}, (name, {g["key"] for g in segs} - judged)


@pytest.mark.parametrize("name", ALL_SCRIPTS)
def test_the_oracle_the_reference_and_the_clean_chain_pass_on_every_segment(name):
    for stream in cs.streams_of(name):
        segs = cs.record(name, stream)
        others = [cs.record(name, stream, orc.Reference)] if orc.have_reference() else []
        for n, seg in enumerate(segs):
            model, tag = seg["model"], (name, stream, seg["index"], seg["op"])
            want = [c["want"] for c in seg["calls"]]
            for other in others:                    # the reference's own C: the same segment, and the same judgement
                ref = other[n]
                assert ref["start"] == seg["start"] and np.array_equal(ref["head"], seg["head"]), tag
                assert np.array_equal(ref["fed"], seg["fed"]) and np.array_equal(ref["model"].rows, model.rows), tag
                fails, _ = cs.judge(seg, [c["want"] for c in ref["calls"]], 32, want)
                assert not fails, (tag, "reference", fails)
            fails, stats = cs.judge(seg, want, 32, [c["want"] for c in others[0][n]["calls"]] if others else None)
            assert not fails, (tag, "oracle", fails)
            truth, _ = cs.truth_of(seg)
            clean = cs.split(seg, em.chain32(model, seg["fed"], truth.shape[0]))
            fails, cstats = cs.judge(seg, clean, 32, clean if model.double_kind else want)
            assert not fails, (tag, "chain32", fails)
            if stats:
                print("%s: %d float samples, rms(e) oracle %.3f chain32 %.3f, bias %.1f / %.1f sigma%s" % (
                    tag, stats["n"], stats["rms"], cstats["rms"], stats["z"], cstats["z"], "" if stats["judged"] else " ((a) alone)"))


def _segment(name, index, stream="float"):
    seg = cs.record(name, stream)[index]
    truth, mag = cs.truth_of(seg)
    return seg, seg["model"], truth.shape[0] - seg["model"].den - 2     # (room for the defects that read further)


def _judge_planted(seg, got, bits=32):
    """the checks on the first len(got) outputs of the segment's float stream -> failures"""
    model, (truth, mag) = seg["model"], cs.truth_of(seg)
    n = got.shape[0]
    yard = cs.outputs(seg)[:n] if bits == 64 or not model.double_kind else em.chain32(model, seg["fed"], n)
    fails, _ = em.judge_float(model, seg["fed"], got, truth[:n], mag[:n], bits, yard, margin=em.MARGIN if bits == 32 else 1.0)
    return fails


# (script, segment): what the segment starts with
START_SEGMENTS = [("period", 3), ("period", 5), ("folded", 2), ("slide", 4), ("wide frames", 2)]
PENDING_SEGMENTS = [("period", 4), ("folded", 1), ("folded", 2), ("slide", 3), ("slide", 4), ("exact fallback", 2)]
GROWN_SEGMENTS = [("period", 1), ("slide", 1), ("wide frames", 1)]


@pytest.mark.parametrize("defect", ["start phase taken as 0", "frac0 + 1", "frac0 - 1", "last0 + 1", "last0 - 1"])
@pytest.mark.parametrize("name,index", START_SEGMENTS)
def test_a_wrong_start_of_a_segment_fails_the_hard_check(name, index, defect):
    seg, model, n = _segment(name, index)
    last0, frac0 = seg["start"]
    assert frac0 >= 1 and last0 >= 1, "the segment must start off the grid for these defects to exist"
    start = {"start phase taken as 0": (last0, 0), "frac0 + 1": (last0, frac0 + 1), "frac0 - 1": (last0, frac0 - 1),
             "last0 + 1": (last0 + 1, frac0), "last0 - 1": (last0 - 1, frac0)}[defect]
    assert not _judge_planted(seg, em.chain32(model, seg["fed"], n))
    fails = _judge_planted(seg, em.chain32(model.segment(model.head, start), seg["fed"], n))
    assert any(f.startswith("(a)") for f in fails), (defect, fails)


@pytest.mark.parametrize("defect", ["pending frames dropped", "pending frames behind the new input",
                                    "one pending frame from the neighbouring slot"])
@pytest.mark.parametrize("name,index", PENDING_SEGMENTS)
def test_misplaced_pending_frames_fail_the_hard_check(name, index, defect):
    seg, model, n = _segment(name, index)
    t, m, fed = model.taps, model.pending, seg["fed"]
    assert m >= 2
    if defect == "pending frames dropped":
        bad = model.segment(model.head[: t - 1], seg["start"])
        n = min(n, (fed.shape[0] - t - m) * model.den // model.num)
    elif defect == "pending frames behind the new input":
        bad, fed = model.segment(model.head[: t - 1], seg["start"]), np.concatenate([fed, model.head[t - 1:]])
    else:
        head = model.head.copy()
        head[t - 1 + m // 2] = head[t + m // 2]
        bad = model.segment(head, seg["start"])
    fails = _judge_planted(seg, em.chain32(bad, fed, n))
    assert any(f.startswith("(a)") for f in fails), (defect, fails)


@pytest.mark.parametrize("name,index", GROWN_SEGMENTS)
def test_a_grown_history_padded_at_the_back_fails_the_hard_check(name, index):
    seg, model, n = _segment(name, index)
    before = cs.record(name, "float")[index - 1]["model"]
    assert model.taps > before.taps and model.pending == 0
    pad = int(np.argmax(np.abs(model.head).sum(axis=1) > 0))       # the frames of silence the op put in FRONT
    assert pad > 0 and not model.head[:pad].any() and model.head[-1].any()
    bad = model.segment(np.concatenate([model.head[pad:], model.head[:pad]]), seg["start"])
    fails = _judge_planted(seg, em.chain32(bad, seg["fed"], n))
    assert any(f.startswith("(a)") for f in fails), fails


def test_no_two_qualities_share_a_filter_length():
    """... so the rows of the filter before a set_quality never FIT the segment after it: only a cutoff change at equal
    length (set_rate_frac between 16:13 and 17:13, 48:47 and 50:47) lets a launch run the previous filter's rows"""
    for (i, o) in ((48000, 48000), (44100, 48000), (48000, 44100), (48000, 8000)):
        assert len({orc.Oracle(1, i, o, q).taps for q in range(11)}) == 11


@pytest.mark.parametrize("name", list(cs.EXTRA))
def test_the_previous_filter_s_rows_fail_the_hard_check(name):
    seg, model, n = _segment(name, 1)
    before = cs.record(name, "float")[0]["model"]
    assert before.rows.shape == model.rows.shape and not np.array_equal(before.rows, model.rows)
    assert not _judge_planted(seg, em.chain32(model, seg["fed"], n))
    fails = _judge_planted(seg, em.chain32(model, seg["fed"], n, rows=before.rows))
    assert any(f.startswith("(a)") for f in fails), fails


def test_64_bit_accumulation_claimed_after_quality_3_to_10_over_the_fp32_chain_fails():
    seg, model, n = _segment("period", 3)
    assert cs.record("period", "float")[2]["quality"] == 3 and seg["quality"] == 10 and model.double_kind
    chain = em.chain32(model, seg["fed"], n)
    assert not _judge_planted(seg, chain, 32)
    fails = _judge_planted(seg, chain, 64)
    assert any(f.startswith("(a)") for f in fails) and any(f.startswith("(b)") for f in fails), fails
    # ... while what does accumulate in 64 bits passes as such
    assert not _judge_planted(seg, cs.truth_of(seg)[0][:n].astype(np.float32), 64)


# the segments of "mixed data" on which an int16 image of the HEAD fails (a): the 352- and 224-tap filters whose first calls
# read the head through many taps.  Not segments 1, 2 and 5: one call that makes 14 samples from pending frames alone; 560
# taps, whose fp32 bound (0.5 LSB at this loudness) is wider than the image's error (0.2 LSB rms -- see
# test_an_int16_window_on_float_data_fails_the_hard_check); a skip_zeros that moved the start past most of the head.
INT16_IMAGE_OF_THE_HEAD_SHOWS = {3, 4}


def test_a_head_that_passed_through_an_int16_image_fails_the_hard_check_on_float_data():
    """float_inputs kinds P and A across a control call: the head of the segment holds fractions"""
    shown = set()
    for seg in cs.record("mixed data", "mixed")[1:]:
        model, (truth, _) = seg["model"], cs.truth_of(seg)
        assert (seg["head"] != np.rint(seg["head"])).any()
        clean = cs.split(seg, em.chain32(model, seg["fed"], truth.shape[0]))
        assert not cs.judge(seg, clean, 32)[0]
        image = model.segment(np.rint(model.head), seg["start"])
        fails, _ = cs.judge(seg, cs.split(seg, em.chain32(image, seg["fed"], truth.shape[0])), 32)
        assert all(f.startswith(("float (a)", "int16 (a)")) for f in fails), fails
        if any(f.startswith("float (a)") for f in fails):
            shown.add(seg["index"])
    assert shown == INT16_IMAGE_OF_THE_HEAD_SHOWS, shown
