"""Streams fed in small calls, without a GPU (tests/streaming.py): the schedules meet the conditions they were built for
on every case the GPU tests use; the oracle and the reference's C cut by a schedule equal their one-call output byte
for byte and pass the exact model's checks; the fp32 chain computed call by call equals em.chain32 bit for bit, and every
planted defect of its start and roll handling fails."""
import numpy as np
import pytest

import exact_model as em
import oracle as orc
import streaming as st

GPU_CASES = sorted({key for cases in st.FAMILIES.values() for key in cases}
                   | {c[:4] for c in st.FAST_CASES + st.FAST_F32_CASES})
# one per kind, three decimators (calls that make no output exist only where num > den) and an interpolator
KIND_CASES = [(2, 48000, 32000, 7), (1, 48000, 40000, 9), (1, 48000, 44100, 7), (1, 44100, 48000, 10)]
MAKERS = [orc.Oracle] + ([orc.Reference] if orc.have_reference() else [])


def _schedule_conditions(c):
    model, log = c.model, c.sched.log
    num, den, taps = model.num, model.den, model.taps
    met = st.conditions(model, log)
    if den <= st.WALK:
        assert met.fracs == set(range(den)), (c.key, sorted(set(range(den)) - met.fracs))
    else:
        assert len(met.fracs) >= st.WALK and {0, 1, den - 2, den - 1} <= met.phases, (c.key, len(met.fracs))
    if num > den:
        assert met.none_out >= 5, (c.key, met.none_out)
    assert met.short_rolls >= 20 and met.bound >= 10 and met.straddle >= 1, (c.key, met)
    assert any(r["frames"] > 0 and r["cap"] == 0 for r in log) and any(r["frames"] == 0 for r in log), c.key
    # every size class, and walk calls of one output for each start phase
    sizes = [r["frames"] for n, r in enumerate(log) if n in c.sched.parts["size classes"]]
    for lo, hi in ((0, 0), (1, 1), (2, max(2, taps // 4)), (taps - 2, taps), (taps + 1, 3 * taps)):
        assert any(lo <= f <= hi for f in sizes), (c.key, lo, hi)
    walk = [log[n] for n in c.sched.parts["phase walk"]]
    assert len(walk) == min(den, st.WALK) and all(r["made"] == 1 for r in walk), c.key
    assert len({r["start"][1] for r in walk}) == len(walk), c.key


@pytest.mark.parametrize("key", GPU_CASES)
def test_the_schedule_meets_its_conditions_on_every_gpu_case(key):
    c = st.case(*key)
    _schedule_conditions(c)
    # the oracle, driven by cut(), stands where the schedule's bookkeeping says -- int16 and float entry alike
    runs = {kind: st.oracle_run(*key, kind) for kind in ("int16", "float")}
    for kind, recs in runs.items():
        assert [(r["start"], r["used"], r["made"]) for r in recs] == [(r["start"], r["used"], r["made"]) for r in c.sched.log], (key, kind)
    # the silence: a window enters it in one call and leaves it in a later one, and a call lies wholly inside
    recs = runs["int16"]
    inside = [n for n, r in enumerate(recs) if r["frames"] > 0 and not c.X[r["offset"]: r["offset"] + r["frames"]].any()]
    assert inside, key
    quiet = np.concatenate([~c.X.any(axis=1), [False]])

    def eats(frame):
        return next(n for n, r in enumerate(recs) if r["offset"] <= frame < r["offset"] + r["used"])

    def enters_before_and_leaves_after(n):
        a = b = recs[n]["offset"]
        while a > 0 and quiet[a - 1]:
            a -= 1
        while quiet[b]:
            b += 1
        return b - a > c.model.taps and eats(a) < n < eats(b)
    assert any(enters_before_and_leaves_after(n) for n in inside), key
    # the float stream is long enough for (c)
    made = sum(r["made"] for r in recs)
    assert st.samples_with_signal(c.model, c.X[: st.consumed(recs)], made) >= em.BIAS_MIN_SAMPLES, key


def test_the_fallback_and_the_batch_schedules():
    c = st.case(*st.FALLBACK, **st.FALLBACK_SCHEDULE)
    assert 38 <= len(c.calls) <= 42 and max(f for f, _ in c.calls) <= 4096 and c.model.taps == 30720
    met = st.conditions(c.model, c.sched.log)
    assert met.none_out >= 5 and met.bound >= 3 and any(r["frames"] == 0 for r in c.sched.log)
    for key in [(2, 44100, 48000, 7), (2, 48000, 8000, 7), (1, 24000, 48000, 10), (2, 44100, 48000, 10), (2, 72000, 16000, 7)]:
        c = st.batch_case(*key)
        assert 118 <= len(c.calls) <= 128 and c.sched.parts["long call"], (key, len(c.calls))


def test_the_kind_cases_cover_all_four_kinds():
    assert {st.case(*key).model.kind for key in KIND_CASES} == set(orc.KIND_NAMES)


@pytest.mark.parametrize("key", KIND_CASES)
def test_the_oracle_and_the_reference_in_pieces_equal_their_one_call_output(key):
    c = st.case(*key)
    model = c.model
    bits = 32       # (the reference's kernels round every product to fp32, the double ones too: the fp32 bound is theirs)
    for make in MAKERS:
        got = {}
        for kind, X in (("int16", c.X), ("float", c.Xf)):
            recs = st.run_on(make, key, X, c.calls, kind)
            n = st.consumed(recs)
            one, used = st.one_call(make, key, X[:n], kind)
            pieces = st.joined(recs)
            assert used == n and pieces.dtype == one.dtype and pieces.tobytes() == one.tobytes(), (key, make.__name__, kind)
            got[kind] = (pieces, n)
        assert got["int16"][1] == got["float"][1]
        fed = c.X[: got["float"][1]]
        truth, mag = model.truth(fed, got["float"][0].shape[0])
        assert not em.hard_int16(model, fed, got["int16"][0], truth, mag, bits), (key, make.__name__)
        yard = em.chain32(model, fed, truth.shape[0])
        fails, stats = em.judge_float(model, fed, got["float"][0], truth, mag, bits, yard)
        assert not fails and stats["n"] >= em.BIAS_MIN_SAMPLES, (key, make.__name__, fails, stats)


_CLEAN = {}


def _clean(key):
    """(chunked chain, em.chain32 of the whole stream, truth, mag), once per case"""
    if key not in _CLEAN:
        c = st.case(*key)
        run = st.chunked_chain32(c.model, c.Xf, c.calls)
        n_out = sum(y.shape[0] for y in run.outs)
        _CLEAN[key] = (run, em.chain32(c.model, run.fed, n_out), c.model.truth(run.fed, n_out))
    return _CLEAN[key]


@pytest.mark.parametrize("key", KIND_CASES)
def test_the_chain_computed_call_by_call_is_chain32_bit_for_bit(key):
    c = st.case(*key)
    run, whole, (truth, mag) = _clean(key)
    ref = st.oracle_run(*key, "float")
    assert run.used == [r["used"] for r in ref] and run.starts == [r["start"] for r in ref], key
    assert [y.shape[0] for y in run.outs] == [r["made"] for r in ref], key
    assert np.concatenate(run.outs).tobytes() == whole.tobytes(), key
    assert np.array_equal(run.history, ref[-1]["history"]), key
    assert not em.hard_float(c.model, run.fed, whole, truth, mag, 32), key
    assert not em.hard_int16(c.model, run.fed, em.halfup(whole).astype(np.int16), truth, mag, 32), key


def _hard(model, run):
    """(a) on a defective run, float and int16, against the model over what the run says it consumed"""
    got = np.concatenate(run.outs)
    try:
        truth, mag = model.truth(run.fed, got.shape[0])
    except AssertionError as err:       # more outputs than the consumed input can place: failed before any sample
        return [str(err)], [str(err)]
    return (em.hard_float(model, run.fed, got, truth, mag, 32),
            em.hard_int16(model, run.fed, em.halfup(got).astype(np.int16), truth, mag, 32))


@pytest.mark.parametrize("defect", st.DEFECTS)
@pytest.mark.parametrize("key", KIND_CASES)
def test_every_planted_defect_fails(key, defect):
    c = st.case(*key)
    if defect == st.DEFECTS[1] and c.model.num < c.model.den:
        # an interpolator's call makes no output only where it consumes nothing: there is no roll to leave out
        assert not any(r["made"] == 0 and r["used"] > 0 for r in c.sched.log)
        return
    _, whole, _ = _clean(key)
    run = st.chunked_chain32(c.model, c.Xf, c.calls, defect)
    got = np.concatenate(run.outs)
    assert got.tobytes() != whole.tobytes(), (key, defect)
    hard_f, hard_i = _hard(c.model, run)
    assert hard_f and hard_i, (key, defect)


@pytest.mark.parametrize("key", KIND_CASES)
def test_a_clamped_front_shows_only_through_lanes_that_are_stored(key):
    """Frames before the history read as the history's first frame, not as silence: only the phase lanes below k_shift
    read there, so with a correct mask no stored sample changes -- the model says so, and a GPU test cannot see this
    defect alone.  With those lanes stored it changes what they store."""
    c = st.case(*key)
    _, whole, _ = _clean(key)
    alone = st.chunked_chain32(c.model, c.Xf, c.calls, st.CLAMPED_FRONT)
    assert np.concatenate(alone.outs).tobytes() == whole.tobytes(), key
    stored = np.concatenate(st.chunked_chain32(c.model, c.Xf, c.calls, st.DEFECTS[3]).outs)
    both = st.chunked_chain32(c.model, c.Xf, c.calls, st.CLAMPED_FRONT, stored_lanes=True)
    assert np.concatenate(both.outs).tobytes() != stored.tobytes(), key
    assert all(_hard(c.model, both)), key
