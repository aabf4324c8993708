"""CPU checks of the dither of the formatted and mixed calls' integer outputs: the entry points are declared, listed,
exported and bound; the library's host statement of the noise (speexhip_debug_dither, the lines the kernels compile) equals
the numpy model (dither_model.py) bit for bit; the model's noise has the moments and the independence the header promises;
and the point of it all -- dither turns the harmonic distortion of a requantised sine into noise."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dither_model as dm
import sample_formats as sf
import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
DITHER = ["speexhip_resampler_set_dither", "speexhip_resampler_get_dither", "speexhip_batch_set_dither",
          "speexhip_batch_get_dither", "speexhip_debug_dither"]
SEEDS = (0, 1, 0xDEADBEEFCAFEF00D)
BASES = (0, (1 << 32) - 5000, 123456789012)   # the second one crosses the 2^32 boundary of idx


def test_dither_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", header))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in DITHER:
        assert name in declared, name + " not declared in the header"
        assert name in speexhip.EXPORTS, name + " not in EXPORTS"
        assert name in exported and hasattr(lib, name), name + " not exported"
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert [len(getattr(lib, n).argtypes) for n in DITHER] == [4, 4, 4, 5, 5]
    assert not declared - exported, "spelled in the header but not exported: %s" % sorted(declared - exported)
    assert "ABI note: 0.5 -> 0.6" in header and "ABI note: 0.6 -> 0.7" in header and "ABI note: 0.7 + dither" in header
    assert b"0.7.0" in lib.speexhip_version()
    for name, value in (("SPEEXHIP_DITHER_NONE", 0), ("SPEEXHIP_DITHER_RECTANGULAR", 1), ("SPEEXHIP_DITHER_TRIANGULAR", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert (speexhip.DITHER_NONE, speexhip.DITHER_RECTANGULAR, speexhip.DITHER_TRIANGULAR) == (0, 1, 2)


def test_dither_kernels_are_built_for_gfx950_and_share_one_statement():
    blob = open(speexhip.LIB_PATH, "rb").read()
    for kernel in (b"convert_out_ditherILi", b"mix_out_ditherILi"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    # the undithered instances are still there, beside them
    for kernel in (b"convert_outILi", b"mix_outILi"):
        assert kernel in blob, kernel
    for unit in ("kernels_convert.hip", "kernels_mix.hip", "c_api.cpp"):
        assert '#include "dither.h"' in open(os.path.join(PKG, "csrc", unit)).read(), unit


def test_bindings_offer_dither():
    for cls in (speexhip.Resampler, speexhip.Batch):
        for n in ("set_dither", "get_dither"):
            assert callable(getattr(cls, n, None)), "%s.%s" % (cls.__name__, n)
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert dts.count("setDither(") >= 2 and dts.count("getDither(") >= 2
    napi = open(os.path.join(PKG, "napi", "speex_hip_napi.c")).read()
    assert "speexhip_resampler_set_dither" in napi and "speexhip_resampler_get_dither" in napi


@pytest.mark.parametrize("kind", dm.KINDS, ids=[dm.KIND_NAMES[k] for k in dm.KINDS])
def test_library_statement_equals_the_model_bit_for_bit(kind):
    n = 1 << 16
    for seed in SEEDS:
        for base in BASES:
            got = speexhip.debug_dither(kind, seed, base, n)
            want = dm.values(kind, seed, base, n)
            assert got.tobytes() == want.tobytes(), (dm.KIND_NAMES[kind], hex(seed), base)
    # the end of the index space wraps like its halves
    got = speexhip.debug_dither(kind, 7, (1 << 64) - 100, 300)
    assert got.tobytes() == dm.values(kind, 7, (1 << 64) - 100, 300).tobytes()


def test_library_statement_none_and_unknown_kinds():
    assert not speexhip.debug_dither(dm.NONE, 5, 12345, 4096).any()
    assert not dm.values(dm.NONE, 5, 12345, 4096).any()
    d = np.full(8, 3.0)
    for kind in (-1, 3, 99):
        rc = speexhip.lib().speexhip_debug_dither(kind, 0, 0, 8, d.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == speexhip.ERR_INVALID_ARG and (d == 3.0).all(), kind


def test_mix32_is_the_stated_function():
    """by hand, in Python integers"""
    def ref(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    xs = [0, 1, 2, 0xFFFFFFFF, 0x80000000, 0xDEADBEEF, 123456789]
    assert dm.mix32(np.uint32(xs)).tolist() == [ref(x) for x in xs]
    seed, idx = 0xDEADBEEFCAFEF00D, (5 << 32) | 77
    w = ref((idx & 0xFFFFFFFF) ^ ref((idx >> 32) ^ (seed >> 32)) ^ (seed & 0xFFFFFFFF))
    assert dm.words(seed, idx, 1).tolist() == [w]
    a, b = w & 0xFFFF, w >> 16
    assert dm.values(dm.RECTANGULAR, seed, idx, 1)[0] == (a + 0.5) / 65536 - 0.5
    assert dm.values(dm.TRIANGULAR, seed, idx, 1)[0] == (a - b) / 65536


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("kind", dm.KINDS, ids=[dm.KIND_NAMES[k] for k in dm.KINDS])
def test_model_statistics(kind):
    """2^20 consecutive indices: the standard error of the mean is sqrt(var / n) <= 0.0004, of a correlation 1 / sqrt(n) =
    0.001"""
    n = 1 << 20
    var, bound = ((1.0 / 12.0), 0.5) if kind == dm.RECTANGULAR else ((1.0 / 6.0), 1.0)
    for seed in SEEDS:
        for base in BASES:
            d = dm.values(kind, seed, base, n)
            what = (dm.KIND_NAMES[kind], hex(seed), base)
            other = dm.values(kind, dm.stream_seed(seed, 1), base, n)   # stream 1 of a batch against stream 0
            figures = (d.mean(), d.var() / var, corr(d[:-1], d[1:]), corr(d[0::2], d[1::2]), corr(d, other))
            print(what, "mean %.5f var ratio %.4f lag-1 %.4f even/odd %.4f streams %.4f" % figures)
            assert abs(figures[0]) < 0.005, what
            assert abs(figures[1] - 1.0) < 0.01, what
            assert d.min() > -bound and d.max() < bound, what
            assert max(abs(f) for f in figures[2:]) < 0.01, what


def test_dither_turns_harmonic_distortion_into_noise():
    """180 * sin(2 pi 441 t / 48000) in int16 units is 0.7 LSB of u8 (one LSB = 256).  2^18 samples hold 441 * 2^18 / 48000 =
    2408.448 cycles: the harmonic is read at the sine's own frequency times three, a whole-record correlation."""
    n = 1 << 18
    t = np.arange(n, dtype=np.float64)
    y = (180.0 * np.sin(2.0 * np.pi * 441.0 * t / 48000.0)).astype(np.float32)
    ideal = y.astype(np.float64) / 256.0 + 128.0

    def h3(stored):
        err = sf.integers(sf.U8, stored).astype(np.float64) - ideal
        ph = 2.0 * np.pi * 3.0 * 441.0 * t / 48000.0
        return 2.0 * abs(np.dot(err, np.exp(-1j * ph))) / n

    plain = h3(sf.from_internal(sf.U8, y))
    assert sf.from_internal(sf.U8, y).tobytes() == dm.quantise(sf.U8, y, np.zeros(n)).tobytes()
    rect = h3(dm.from_internal(sf.U8, y, dm.RECTANGULAR, 1, 0, 1))
    tri = h3(dm.from_internal(sf.U8, y, dm.TRIANGULAR, 1, 0, 1))
    print("third harmonic, LSB: half-up %.5f rectangular %.5f triangular %.5f" % (plain, rect, tri))
    assert plain > 0.1
    assert rect < 0.01 and tri < 0.01


def test_model_quantise_is_from_internal_without_dither_and_keeps_the_edges():
    y = np.float32([0.0, -0.0, 0.5, -0.5, 127.9, 1e9, -1e9, np.inf, -np.inf, np.nan, 32767.4, -32768.6, 255.5])
    for fmt in (sf.U8, sf.S16, sf.S24, sf.S32):
        assert dm.quantise(fmt, y, np.zeros(y.size)).tobytes() == sf.from_internal(fmt, y).tobytes()
        for kind in dm.KINDS:
            q = sf.integers(fmt, dm.from_internal(fmt, y, kind, 3, 10, 1))
            lo, hi = sf._INT[fmt][1], sf._INT[fmt][2]
            assert q[7] == hi and q[8] == lo and q[9] == sf.ZERO[fmt] and q[5] == hi and q[6] == lo
    # float formats pass the model untouched
    for fmt in (sf.F32, sf.F32N):
        assert dm.from_internal(fmt, y, dm.TRIANGULAR, 3, 10, 1).tobytes() == sf.from_internal(fmt, y).tobytes()
    # d moves a value across a rounding boundary exactly where v + d says so: y = 10.25, d = +0.25 -> t = 10.5 -> 11
    assert sf.integers(sf.S16, dm.quantise(sf.S16, np.float32([10.25, 10.25]), np.float64([0.25, 0.2499]))).tolist() == [11, 10]
