"""The output meter's rule (include/speexhip_resampler.h, "Metering") on the host: speexhip_debug_meter runs the very
statement the kernels compile (csrc/meter.h), and is held here against its numpy restatement (meter_model.py) for all
13 formats, on a vector built from every decision point of the rule.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import meter_model as mm
import speexhip

F32_MAX = np.finfo(np.float32).max
F32_TINY = np.finfo(np.float32).tiny


def neighbours(v):
    """v as a float32 and the float32 values either side of it"""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def decision_points():
    """every format's two thresholds -- the y at which r leaves the rails: (hi + 0.5 - offset) / scale and
    (lo - 0.5 - offset) / scale -- with their float32 neighbours, the special values, and seeded noise at 1.5 x full scale"""
    pts = []
    for rails in mm.RAILS.values():
        if rails is None:
            continue
        scale, offset, lo, hi = rails
        for edge in ((hi + 0.5 - offset) / scale, (lo - 0.5 - offset) / scale, (hi - offset) / scale, (lo - offset) / scale):
            pts += neighbours(edge)
    pts += [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, F32_MAX, -F32_MAX, 32768.0, -32768.0]
    pts += [F32_TINY, -F32_TINY, F32_TINY / 4, -F32_TINY / 4, np.float32(1e-45), np.float32(-1e-45)]  # (subnormals)
    rng = np.random.default_rng(20240607)
    noise = (rng.uniform(-1.5, 1.5, 4096) * 32767.0).astype(np.float32)
    return np.concatenate([np.array(pts, np.float32), noise])


Y = decision_points()


def test_the_entry_points_are_exported_and_bound():
    names = ("speexhip_resampler_set_meter", "speexhip_resampler_get_meter", "speexhip_batch_set_meter",
             "speexhip_batch_get_meter", "speexhip_debug_meter")
    lib = speexhip.lib()
    for name in names:
        assert name in speexhip.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 or fn.restype is C.c_int, name
        assert fn.argtypes, name
    assert C.sizeof(speexhip.Meter) == 48
    for cls, method in ((speexhip.Resampler, "set_meter"), (speexhip.Resampler, "get_meter"), (speexhip.Batch, "set_meter"),
                        (speexhip.Batch, "get_meter")):
        assert callable(getattr(cls, method))


def test_the_vector_holds_every_class_for_every_clipping_format():
    assert np.isnan(Y).sum() == 2 and np.isinf(Y).sum() == 2
    for name in mm.NAMES:
        fmt, rails = mm.FORMATS[name]
        want = mm.totals(fmt, Y)
        if rails is not None:
            assert want["clipped_high"] > 0 and want["clipped_low"] > 0, name
        assert want["peak"] == np.inf and want["nan"] == 2


@pytest.mark.parametrize("name", mm.NAMES)
def test_debug_meter_equals_the_restatement(name):
    fmt, rails = mm.FORMATS[name]
    got = speexhip.debug_meter(fmt, Y)
    want = mm.totals(fmt, Y)
    assert mm.same(got, want), (name, got, want)
    if rails is None:
        assert got["clipped_high"] == 0 and got["clipped_low"] == 0
    # (the finite part alone: the peak is then a finite float whose bits must match)
    finite = Y[np.isfinite(Y)]
    got, want = speexhip.debug_meter(fmt, finite), mm.totals(fmt, finite)
    assert mm.same(got, want) and got["nan"] == 0 and np.isfinite(got["peak"]), (name, got, want)
    # (thresholds one by one: a miscounted neighbour cannot hide behind another)
    for i in range(0, 60):
        one = Y[i: i + 1]
        assert mm.same(speexhip.debug_meter(fmt, one), mm.totals(fmt, one)), (name, float(one[0]))


@pytest.mark.parametrize("kind", (speexhip.DITHER_RECTANGULAR, speexhip.DITHER_TRIANGULAR), ids=("rectangular", "triangular"))
@pytest.mark.parametrize("name", [n for n in mm.NAMES if mm.FORMATS[n][1] is not None])
def test_debug_meter_with_dither_equals_the_restatement(name, kind):
    fmt, _ = mm.FORMATS[name]
    d = speexhip.debug_dither(kind, 0x0123456789ABCDEF, (1 << 32) - 1000, Y.size)
    got, want = speexhip.debug_meter(fmt, Y, d), mm.totals(fmt, Y, d)
    assert mm.same(got, want), (name, got, want)
    # (d = 0 given explicitly is no dither)
    assert mm.same(speexhip.debug_meter(fmt, Y, np.zeros(Y.size)), mm.totals(fmt, Y))


def test_mu_laws_own_limit_is_no_clip():
    y = np.array([32635.0, 32700.0, 32767.0, -32700.0, -32768.0], np.float32)
    for name in ("ulaw", "alaw"):
        got = speexhip.debug_meter(mm.FORMATS[name][0], y)
        assert got["clipped_high"] == 0 and got["clipped_low"] == 0 and got["peak"] == 32768.0, (name, got)
    got = speexhip.debug_meter(speexhip.FMT_ULAW, np.array([32767.5, -32768.5, -32768.51], np.float32))
    assert (got["clipped_high"], got["clipped_low"]) == (1, 1), got   # (-32768.5 rounds half up to -32768)


def test_an_empty_vector_and_a_silent_one():
    got = speexhip.debug_meter(speexhip.FMT_S16, np.zeros(0, np.float32))
    assert mm.same(got, mm.ZERO)
    got = speexhip.debug_meter(speexhip.FMT_U8, np.zeros(100, np.float32))
    assert mm.same(got, dict(mm.ZERO, samples=100))


def test_argument_rules():
    lib = speexhip.lib()
    y = np.zeros(4, np.float32)
    d = np.zeros(4, np.float64)
    py, pd = C.c_void_p(y.ctypes.data), C.c_void_p(d.ctypes.data)
    m = speexhip.Meter()
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, py, None, 4, C.byref(m)) == 0 and m.samples == 4
    # a short struct_size: nothing is written
    short = speexhip.Meter()
    short.struct_size = C.sizeof(speexhip.Meter) - 4
    short.samples = 77
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, py, None, 4, C.byref(short)) == speexhip.ERR_INVALID_ARG
    assert short.samples == 77
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, py, None, 4, None) == speexhip.ERR_INVALID_ARG
    # a larger one (a caller compiled against a later header): this version's fields, struct_size kept
    big = speexhip.Meter()
    big.struct_size = C.sizeof(speexhip.Meter) + 16
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, py, None, 4, C.byref(big)) == 0
    assert big.struct_size == C.sizeof(speexhip.Meter) + 16 and big.samples == 4
    # unknown formats
    for fmt in (-1, 6, 15, 18, 27, 255):
        assert lib.speexhip_debug_meter(fmt, py, None, 4, C.byref(m)) == speexhip.ERR_INVALID_ARG, fmt
    # dither for a float format
    for name in ("f32", "f32n", "f16n", "bf16n"):
        assert lib.speexhip_debug_meter(mm.FORMATS[name][0], py, pd, 4, C.byref(m)) == speexhip.ERR_INVALID_ARG, name
        assert lib.speexhip_debug_meter(mm.FORMATS[name][0], py, None, 4, C.byref(m)) == 0, name
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, None, None, 4, C.byref(m)) == speexhip.ERR_INVALID_ARG
    assert lib.speexhip_debug_meter(speexhip.FMT_S16, None, None, 0, C.byref(m)) == 0
    # null states
    assert lib.speexhip_resampler_set_meter(None, 1) == speexhip.ERR_INVALID_ARG
    assert lib.speexhip_resampler_get_meter(None, C.byref(m), 0) == speexhip.ERR_INVALID_ARG
    assert lib.speexhip_batch_set_meter(None, 1) == speexhip.ERR_INVALID_ARG
    assert lib.speexhip_batch_get_meter(None, 0, C.byref(m), 0) == speexhip.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        speexhip.debug_meter(speexhip.FMT_F32, y, d)
