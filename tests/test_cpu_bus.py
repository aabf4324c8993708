"""The bus rule on the host (include/speexhip_resampler.h, "Buses"): speexhip_debug_bus compiles the very statement the
kernel compiles (csrc/bus.h) and must equal the numpy model (bus_model.py) bit for bit -- on random data at the pack
sizes, and at the points where a wrong sum shows: cancelling pairs and negative zeros, values 2^24 apart (a wrong order
or an fp32 accumulator loses the small ones), inf * 0.  Then the defects that bus_model.buses(defect=) can plant, on
synthetic arrays of the layouts test_gpu_bus_edges.py feeds the kernel: each must change the model's output there (the
shares are printed with -s).  No GPU."""
import os
import re

import numpy as np
import pytest

import bus_model as bm
import speexhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def both(w, y):
    got = speexhip.debug_bus(w, y)
    want = bm.buses(w, y)
    assert got.dtype == np.float32 and got.shape == want.shape
    # (NaN bits: where both are NaN the payload is the implementation's; everything else bit for bit)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), "NaN where the model has none, or none where it has one"
    assert same_bits(np.where(nan, 0, got), np.where(nan, 0, want)), (w, y, got, want)
    return got


@pytest.mark.parametrize("n_buses", (1, 2, 32))
@pytest.mark.parametrize("n_streams", (1, 3, 32))
def test_debug_bus_equals_the_model_on_random_data(n_streams, n_buses):
    rng = np.random.default_rng(100 * n_streams + n_buses)
    w = rng.uniform(-2.0, 2.0, (n_buses, n_streams)).astype(np.float32)
    y = (rng.uniform(-1.3, 1.3, (n_streams, 257)) * 32767.0).astype(np.float32)
    got = both(w, y)
    assert not np.isnan(got).any()


def test_cancelling_pairs_and_negative_zeros():
    # +a and -a under equal weights cancel to +0.0; a zero weight on a negative sample is -0.0, and a sum of -0.0 terms
    # stays -0.0 because the first term is the product itself, not 0 + the product
    y = np.array([[1.5, -0.0, -3.0, 7.0], [-1.5, -0.0, -3.0, -7.0], [0.0, -0.0, -1.0, 0.0]], np.float32)
    w = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, -1.0, 0.0], [-1.0, -1.0, -1.0]], np.float32)
    got = both(w, y)
    assert same_bits(got[0], np.array([0.0, -0.0, -7.0, 0.0], np.float32))
    assert same_bits(got[1], np.array([0.0, -0.0, -0.0, 0.0], np.float32))   # 0 * 1.5 + 0 * -1.5 = +0 + -0 = +0
    assert same_bits(got[3, 1], np.float32(0.0))                              # -1 * -0.0 three times: +0.0


def test_values_2_to_the_24_apart_catch_a_wrong_order_or_a_narrow_accumulator():
    # 2^24 + 1 + 1 - 2^24: fp32 accumulation loses both ones; fp64 in ascending order keeps them
    big = np.float32(2.0 ** 24)
    y = np.array([[big], [1.0], [1.0], [-big]], np.float32)
    w = np.ones((1, 4), np.float32)
    assert same_bits(both(w, y), np.array([[2.0]], np.float32))
    # ... and a sum whose fp64 value depends on the order: 2^60 + 1 + ... (31 ones) - 2^60
    huge = np.float32(2.0 ** 60)
    y = np.concatenate([[huge], np.ones(30, np.float32), [-huge]]).astype(np.float32).reshape(32, 1)
    w = np.ones((2, 32), np.float32)
    w[1] = -1.0
    got = both(w, y)
    # ascending order: every 1 is below half an ulp of 2^60 (ulp 2^8) and is lost one by one
    assert same_bits(got, np.array([[0.0], [0.0]], np.float32))
    # the same ones first: 30 survives
    y2 = np.concatenate([np.ones(30, np.float32), [huge], [-huge]]).astype(np.float32).reshape(32, 1)
    assert same_bits(both(w[:1], y2), np.array([[0.0]], np.float32))          # 2^60 + 30 rounds to 2^60
    y3 = np.concatenate([[huge], [-huge], np.ones(30, np.float32)]).astype(np.float32).reshape(32, 1)
    assert same_bits(both(w[:1], y3), np.array([[30.0]], np.float32))
    # one rounding to fp32, from the fp64 sum: 2^24 + 1 is a tie in fp32 and goes to even, 2^24 + 1 + 2^-20 goes up
    y = np.array([[big], [1.0], [2.0 ** -20]], np.float32)
    got = both(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]], np.float32), y)
    assert same_bits(got, np.array([[big], [big + 2.0]], np.float32))


def test_a_zero_weight_is_not_skipped():
    y = np.array([[np.inf, -np.inf, np.nan, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)
    w = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]], np.float32)
    got = both(w, y)
    assert np.isnan(got[0, :3]).all() and same_bits(got[0, 3], np.float32(1.0))   # 0 * inf = NaN
    assert same_bits(got[1, :2], np.array([np.inf, -np.inf], np.float32))
    assert same_bits(got[2, :2], np.array([np.inf, -np.inf], np.float32)) and np.isnan(got[2, 2])


def test_overflow_of_the_sum_rounds_to_infinity_once():
    m = np.finfo(np.float32).max
    y = np.array([[m], [m], [-m]], np.float32)
    got = both(np.array([[1.0, 1.0, -1.0], [1.0, 1.0, 1.0]], np.float32), y)
    assert same_bits(got, np.array([[np.inf], [m]], np.float32))   # 3 max overflows fp32; max + max - max does not in fp64


def test_mix_minus_is_ones_minus_identity():
    w = bm.mix_minus(4)
    y = np.arange(1, 9, dtype=np.float32).reshape(4, 2)
    got = both(w, y)
    assert same_bits(got, (y.sum(0)[None, :] - y).astype(np.float32))


# ---- planted defects: what the crafted layouts of test_gpu_bus_edges.py can tell from the rule -------------------------
SIGNS_W = np.array([[-1.0, 0.0], [1.0, 0.0]], np.float32)    # stream 0 has ended, stream 1 is live


def signs_layout(n=320, seed=5):
    """(2, n) float32 and its live mask: stream 0 ended before the first sample, stream 1 noise of both signs"""
    y = np.zeros((2, n), np.float32)
    y[1] = (np.random.default_rng(seed).uniform(-0.9, 0.9, n) * 32767.0).astype(np.float32)
    return y, bm.live_of([0, n], n)


def inf_layout(n=400, seed=6):
    """(3, n) float32 with one +inf in stream 2, under weights that put 0 on it and 0 on the others"""
    y = (np.random.default_rng(seed).uniform(-1.3, 1.3, (3, n)) * 32767.0).astype(np.float32)
    y[2, n - n // 16] = np.inf
    return y, np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)


def test_the_defect_engine_without_a_defect_is_the_rule():
    # (_defective with no known defect name walks the streams in ascending order, fp64, first term the product itself)
    y = bm.order_layout(800)
    want = bm.buses(bm.ORDER_W, y)
    got = np.stack([bm._defective(bm.ORDER_W[j], y.astype(np.float64), None, np.ones(y.shape, bool)) for j in range(4)])
    assert same_bits(got, want)
    assert same_bits(both(bm.ORDER_W, y), want)


def test_every_order_defect_shows_on_the_order_layout():
    n = 800
    y = bm.order_layout(n)
    assert same_bits(y[1], -y[0]) and same_bits(y[31], -y[30])
    assert np.abs(y[0, : n // 2]).mean() > 2.0 ** 57 and np.abs(y[30, n // 2:]).mean() > 2.0 ** 57
    assert np.abs(y[2:30]).max() <= 2.0 ** 12 and np.abs(y[0, n // 2:]).max() <= 2.0 ** 12
    assert np.isfinite(y).all()
    want = both(bm.ORDER_W, y)
    assert np.isfinite(want).all()
    # rows 2 and 3: a pair alone among zero weights is +0.0, never -0.0
    assert same_bits(want[2:], np.zeros((2, n), np.float32))
    for defect in bm.ORDER_DEFECTS + ("round_each_add",):
        z = bm.buses(bm.ORDER_W, y, defect)
        first = max(bm.changed(z[j, : n // 2], want[j, : n // 2]) for j in (0, 1))
        second = max(bm.changed(z[j, n // 2:], want[j, n // 2:]) for j in (0, 1))
        print("order layout, %-16s: %5.1f %% / %5.1f %% of a bus's samples change (first / second half)"
              % (defect, 100 * first, 100 * second))
        assert max(first, second) >= 0.01, defect
    for defect in ("skip_zero_weight", "zero_plus_first", "skip_ended"):
        # (finite sums far from zero: none of these shows here -- their own rows below do)
        assert same_bits(bm.buses(bm.ORDER_W[:2], y, defect), want[:2]), defect


def test_the_other_defects_show_on_their_own_rows():
    y, live = signs_layout()
    want = both(SIGNS_W, y)
    neg = y[1] < 0
    assert 0.2 < neg.mean() < 0.8 and (y[1] != 0).all()
    # -0 + -0 = -0 and -0 + +0 = +0: the sign of the live sample; +0 + either zero = +0
    assert same_bits(want[0], np.where(neg, np.float32(-0.0), np.float32(0.0)))
    assert same_bits(want[1], np.zeros(y.shape[1], np.float32))
    shares = {}
    for defect, row, where in (("zero_plus_first", 0, neg), ("skip_zero_weight", 0, ~neg), ("skip_ended", 1, neg)):
        z = bm.buses(SIGNS_W, y, defect, live)
        diff = z.view(np.uint32)[row] != want.view(np.uint32)[row]
        assert diff.any() and (diff == where).all(), defect
        shares[defect] = diff.mean()
    y, w = inf_layout()
    want = both(w, y)
    at = int(np.flatnonzero(np.isinf(y[2]))[0])
    assert np.isnan(want[0, at]) and np.isnan(want[0]).sum() == 1 and not np.isnan(want[1]).any() and np.isinf(want[1, at])
    z = bm.buses(w, y, "skip_zero_weight")
    assert not np.isnan(z).any(), "a skipped zero weight makes no NaN"
    shares["skip_zero_weight (0 * inf)"] = bm.changed(z[0], want[0])
    assert shares["skip_zero_weight (0 * inf)"] > 0
    for k, v in shares.items():
        print("%-28s: %5.1f %% of the row's samples change" % (k, 100 * v))


def test_arguments_and_exports():
    L = speexhip.lib()
    one = np.ones(1, np.float32)
    ptr = one.ctypes.data
    assert L.speexhip_debug_bus(1, 1, None, ptr, 1, ptr) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_bus(0, 1, ptr, ptr, 1, ptr) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_bus(1, 0, ptr, ptr, 1, ptr) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_bus(1, 1, ptr, None, 1, ptr) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_bus(1, 1, ptr, None, 0, None) == 0
    assert speexhip.debug_bus(np.ones((2, 3), np.float32), np.zeros((3, 0), np.float32)).shape == (2, 0)
    names = ("speexhip_batch_set_buses", "speexhip_batch_get_buses", "speexhip_batch_process_bus_device",
             "speexhip_batch_get_bus_meter", "speexhip_batch_get_bus_position", "speexhip_debug_bus")
    with open(os.path.join(ROOT, "include", "speexhip_resampler.h")) as f:
        header = f.read()
    for name in names:
        assert name in speexhip.EXPORTS and getattr(L, name)
        assert re.search(r"SPEEXHIP_API int %s\(" % name, header), "the header does not export " + name
    assert L.speexhip_batch_set_buses(None, 1, ptr) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_batch_get_bus_position(None, None) == speexhip.ERR_INVALID_ARG


def test_the_makefile_names_the_new_units():
    with open(os.path.join(ROOT, "node-speex-resampler_amd", "Makefile")) as f:
        text = f.read()
    src = text[text.index("SRC ="): text.index("OBJ =")]
    assert "csrc/bus.cpp" in src and "csrc/kernels_bus.hip" in src
    for name in ("bus.h", "bus.cpp", "kernels_bus.hip"):
        assert os.path.exists(os.path.join(ROOT, "node-speex-resampler_amd", "csrc", name))
