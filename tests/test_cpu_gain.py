"""The gain rule on the host (include/speexhip_resampler.h, "Gain"): speexhip_debug_gain compiles the very statement the
kernels compile (csrc/gain.h) and must equal the numpy model (gain_model.py) bit for bit at its decision points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gain_model as gm
import speexhip

U32 = 2 ** 32 - 1


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def both(frm, to, total, first, n):
    got = speexhip.debug_gain(frm, to, total, first, n)
    want = gm.g(frm, to, total, first, n)
    assert got.dtype == np.float32 and same_bits(got, want), (frm, to, total, first, n, got, want)
    return got


RAMPS = (
    (1.0, 0.5, 480), (0.0, 1.0, 441), (1.0, 0.0, 48000), (0.3, 0.7, 1), (0.25, 0.25, 100),   # from == to
    (0.5, -0.5, 1000),           # through zero
    (1.0, -1.0, 3),              # to a negative target
    (-0.75, -0.1, 77),
    (1.0, 1.0000001, U32),       # a step below one fp32 ulp of from
    (16777216.0, 16777217.0, 1 << 20),
    (1e-30, 3e38, 12345), (0.1, 0.2, U32),
)


@pytest.mark.parametrize("frm,to,total", RAMPS)
def test_debug_gain_equals_the_model_at_the_decision_points(frm, to, total):
    # k = 0 is `from` exactly; total - 1, total, total + 1 around the end of the ramp
    head = both(frm, to, total, 0, min(total + 3, 64))
    assert same_bits(head[0], np.float32(frm))
    tail = both(frm, to, total, max(total - 2, 0), 6)
    end = total - max(total - 2, 0)
    assert same_bits(tail[end:], np.full(6 - end, to, np.float32)), "g(k) for k >= total is not the target"
    # a window in the middle, and one that begins beyond 2^32
    both(frm, to, total, total // 2, 33)
    far = both(frm, to, total, 2 ** 32 + 5, 9)
    assert same_bits(far, np.full(9, to, np.float32))
    assert same_bits(both(frm, to, total, 2 ** 63 + 1, 2), np.full(2, to, np.float32))


def test_total_zero_is_the_target_from_the_first_frame_on():
    for to in (0.5, -1.0, 0.0, 1.0):
        got = both(0.125, to, 0, 0, 5)
        assert same_bits(got, np.full(5, to, np.float32))


def test_total_one_is_from_then_to():
    got = both(0.3, 0.7, 1, 0, 3)
    assert same_bits(got, np.array([0.3, 0.7, 0.7], np.float32))


def test_the_longest_ramp_near_its_end():
    got = both(0.1, 0.2, U32, U32 - 4, 8)
    assert same_bits(got[4:], np.full(4, 0.2, np.float32))
    both(-1.0, 1.0, U32, 2 ** 31 - 2, 5)   # through zero at the middle of the index range
    both(-1.0, 1.0, U32, 2 ** 31 + 2 ** 30, 5)


def test_a_step_below_one_ulp_still_ends_on_the_target():
    frm = np.float32(1.0)
    to = np.nextafter(frm, np.float32(2.0))
    got = both(frm, to, 1000, 0, 1002)
    assert set(got.tobytes()[i: i + 4] for i in range(0, got.nbytes, 4)) == {frm.tobytes(), to.tobytes()}
    assert np.all(np.diff(got) >= 0) and same_bits(got[-2:], [to, to])


def test_zero_is_signed_as_the_sum_leaves_it():
    got = both(-0.5, 0.5, 2, 0, 3)   # the middle: -0.5 + 1 * 0.5 = +0.0
    assert same_bits(got, np.array([-0.5, 0.0, 0.5], np.float32))
    got = both(0.5, -0.0, 0, 0, 1)   # a target of -0.0 is kept
    assert got.tobytes() == np.float32(-0.0).tobytes()


def test_the_chain_of_two_retargets_is_continuous():
    """set_gain's rule: the new `from` is the old g(done).  The chain is followed through the library's statement and
    through the model; both must give the same ramps."""
    m = gm.State()
    frm, to, total, done = np.float32(1.0), np.float32(1.0), 0, 0
    for gain, ramp, run in ((0.25, 1000, 333), (-0.5, 64, 17), (1.0, 10, 25)):
        frm = speexhip.debug_gain(frm, to, total, done, 1)[0]   # what the next output frame would have had
        to, total, done = np.float32(gain), ramp, 0
        m.set(gain, ramp)
        assert (frm.tobytes(), to.tobytes(), total, done) == (np.float32(m.frm).tobytes(), np.float32(m.to).tobytes(), m.total, m.done)
        got = speexhip.debug_gain(frm, to, total, done, run)
        assert same_bits(got, m.take(run))
        assert same_bits(got[0], frm), "a new target in mid-ramp jumped"
        done = min(total, done + run)
        assert done == m.done
    assert m.off()


def test_arguments():
    L = speexhip.lib()
    assert L.speexhip_debug_gain(1.0, 0.5, 10, 0, 4, None) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_gain(1.0, 0.5, 10, 0, 0, None) == 0
    assert speexhip.debug_gain(1.0, 0.5, 10, 0, 0).size == 0
    for name in ("speexhip_resampler_set_gain", "speexhip_resampler_get_gain", "speexhip_batch_set_gain",
                 "speexhip_batch_get_gain", "speexhip_debug_gain"):
        assert name in speexhip.EXPORTS and getattr(L, name)
    assert L.speexhip_resampler_set_gain(None, C.c_float(0.5), 0) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_batch_get_gain(None, 0, None, None, None) == speexhip.ERR_INVALID_ARG
