"""Pins tests/exact_model.py without a GPU and proves that its checks bite: the oracle (and the reference's own C where it
is built) passes the hard check (a) and the bias check (c) on all four kernel kinds; a multi-call ragged stream has the
one-call truth; every planted defect of the documented fp32 chain fails a check while the clean chain passes them all."""
import numpy as np
import pytest

import exact_model as em
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
