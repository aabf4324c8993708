"""CPU checks of the half-float and big-endian sample formats (F16N, BF16N, S16BE, S24BE, S32BE in the formatted, mixed
and sides calls): the enum values in the header and the binding, speexhip_sample_bytes, the two host debug entry points,
gfx950 instances of the three kernel units for all five formats -- and the formats themselves: the library's host
statement (csrc/halfbe.h, the lines the kernels compile) against the numpy one (halfbe_model.py), byte for byte, on every
16-bit code, seeded values, exact ties, the overflow threshold, subnormals, non-finite values and dithered values."""
import os
import re
import subprocess

import numpy as np
import pytest

import dither_model as dm
import halfbe_model as hm
import sample_formats as sf
import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
DEBUG = ["speexhip_debug_format_decode", "speexhip_debug_format_encode"]
LIB_FMT = {hm.F16N: "F16N", hm.BF16N: "BF16N", hm.S16BE: "S16BE", hm.S24BE: "S24BE", hm.S32BE: "S32BE"}
UNKNOWN = [-1] + list(range(6, 16)) + [18, 19, 22, 23, 27, 32, 99]
CODES = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def header():
    return open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()


def same(got, want):
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


# ---- names, sizes, symbols ---------------------------------------------------------------------------------------------
def test_enum_values_in_the_header_and_the_binding():
    h = header()
    assert (hm.F16N, hm.BF16N, hm.S16BE, hm.S24BE, hm.S32BE) == (20, 21, 24, 25, 26)
    for fmt, nm in LIB_FMT.items():
        assert re.search(r"SPEEXHIP_FMT_%s = %d\b" % (nm, fmt), h), nm
        assert getattr(speexhip, "FMT_" + nm) == fmt
    assert "Half-float and big-endian formats" in h and "6..15 stay invalid" in h
    assert len(speexhip.FMT_BYTES) == len(speexhip.FMT_DTYPE) == 6


def test_sample_bytes_of_the_new_formats_and_of_the_unknown_ones():
    lib = speexhip.lib()
    assert [lib.speexhip_sample_bytes(f) for f in hm.NEW] == [2, 2, 2, 3, 4]
    want_dtype = {hm.F16N: np.float16, hm.BF16N: np.uint16, hm.S16BE: ">i2", hm.S24BE: np.uint8, hm.S32BE: ">i4"}
    for f in hm.NEW:
        assert speexhip.fmt_bytes(f) == lib.speexhip_sample_bytes(f) == hm.nbytes(f), hm.name(f)
        assert np.dtype(speexhip.fmt_dtype(f)) == np.dtype(want_dtype[f]) == hm.dtype(f), hm.name(f)
    for f in hm.OLD:
        assert speexhip.fmt_bytes(f) == lib.speexhip_sample_bytes(f) == hm.nbytes(f)
    for unknown in UNKNOWN:
        assert lib.speexhip_sample_bytes(unknown) == 0, unknown
        with pytest.raises(ValueError):
            speexhip.fmt_bytes(unknown)
        with pytest.raises(ValueError):
            speexhip.fmt_dtype(unknown)


def test_debug_entry_points_are_declared_listed_and_exported():
    h = header()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", h))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for nm in DEBUG:
        assert nm in declared, nm + " not declared in the header"
        assert nm in speexhip.EXPORTS, nm + " not in EXPORTS"
        assert nm in exported and hasattr(lib, nm), nm + " not exported"
    assert [len(getattr(lib, n).argtypes) for n in DEBUG] == [4, 5]
    assert re.search(r"ABI note: 0\.7 \+ halfbe adds five enum values and two entry points; SpeexHipInfo, the error codes\s+"
                     r"(\* )?and the version string are unchanged", h)
    assert "0.7.0" in lib.speexhip_version().decode()
    # any other format: INVALID_ARG, nothing written; and no dither for the half formats
    raw, x = np.zeros(16, np.uint8), np.full(4, 7.0, np.float32)
    for fmt in list(hm.OLD) + UNKNOWN:
        assert lib.speexhip_debug_format_decode(fmt, raw.ctypes.data, 4, x.ctypes.data) == speexhip.ERR_INVALID_ARG
        assert lib.speexhip_debug_format_encode(fmt, x.ctypes.data, None, 4, raw.ctypes.data) == speexhip.ERR_INVALID_ARG
    d = np.zeros(4, np.float64)
    for fmt in hm.HALF:
        assert lib.speexhip_debug_format_encode(fmt, x.ctypes.data, d.ctypes.data, 4, raw.ctypes.data) == speexhip.ERR_INVALID_ARG
    assert (x == 7.0).all() and not raw.any()


def test_library_holds_gfx950_kernels_for_all_five_formats():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/kernels_sides.hip" in mk and "$(wildcard csrc/*.h)" in mk
    assert os.path.exists(os.path.join(PKG, "csrc", "halfbe.h"))
    blob = open(speexhip.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for kernel in ("convert_in", "convert_out", "mix_in", "mix_out", "planes_in", "planes_out"):
        for fmt in hm.NEW:
            sym = ("%sILi%dEE" % (kernel, fmt)).encode()
            assert sym in blob, sym
    for kernel in ("convert_out_dither", "mix_out_dither", "planes_out_dither"):
        for fmt in hm.NEW:
            sym = ("%sILi%dEE" % (kernel, fmt)).encode()
            assert (sym in blob) == (fmt in hm.BIG), sym     # (the half formats are float formats: never dithered)


def test_node_files_name_the_new_formats():
    for rel in ("index.js", "index.d.ts"):
        text = open(os.path.join(PKG, rel)).read()
        for nm in ("'s16be'", "'s24be'", "'s32be'", "'f16le-normalized'", "'bf16le-normalized'"):
            assert nm in text, (rel, nm)


# ---- decode ------------------------------------------------------------------------------------------------------------
def test_library_decode_equals_the_model_on_every_16_bit_code():
    for fmt in (hm.F16N, hm.BF16N, hm.S16BE):
        storage = CODES.view(hm.dtype(fmt))
        x = speexhip.debug_format_decode(fmt, storage)
        assert x.dtype == np.float32 and x.size == 65536 and same(x, hm.to_internal(fmt, storage)), hm.name(fmt)
    # known answers: 1.0 is 32768 int16 steps; the smallest binary16 subnormal is 2^-24 (exact after the scaling)
    assert speexhip.debug_format_decode(hm.F16N, np.array([0x3C00, 0xBC00, 0x0001, 0x7C00], np.uint16).view(np.float16)).tolist() \
        == [32768.0, -32768.0, 2.0 ** -9, np.inf]
    assert speexhip.debug_format_decode(hm.BF16N, np.array([0x3F80, 0xBF80, 0x0001], np.uint16)).tolist() \
        == [32768.0, -32768.0, float(np.array([0x10000], np.uint32).view(np.float32)[0]) * 32768.0]
    assert speexhip.debug_format_decode(hm.S16BE, np.array([0x12, 0x34, 0x80, 0x00, 0x7F, 0xFF], np.uint8).view(">i2")).tolist() \
        == [0x1234, -32768.0, 32767.0]
    assert np.isnan(speexhip.debug_format_decode(hm.F16N, np.array([0x7E00, 0xFE01], np.uint16).view(np.float16))).all()


def edge_integers(bits):
    top = 1 << (bits - 1)
    return [0, 1, -1, 2, -2, 255, 256, -256, 0x1234, -0x1234, top - 1, top - 2, -top, -top + 1, top >> 1, -(top >> 1), 0x00FF00, 0xFF]


def test_library_decode_of_the_wide_big_endian_formats_equals_the_model():
    rng = np.random.RandomState(2425)
    for fmt, bits in ((hm.S24BE, 24), (hm.S32BE, 32)):
        top = 1 << (bits - 1)
        v = np.concatenate([np.array(edge_integers(bits), np.int64), rng.randint(-top, top, 50000).astype(np.int64)])
        storage = hm.be_of(fmt, sf.store(hm.LE_TWIN[fmt], v))
        x = speexhip.debug_format_decode(fmt, storage)
        assert x.size == v.size and same(x, hm.to_internal(fmt, storage)), hm.name(fmt)
        assert same(x, sf.to_internal(hm.LE_TWIN[fmt], sf.store(hm.LE_TWIN[fmt], v))), hm.name(fmt)   # the LE rule
    assert speexhip.debug_format_decode(hm.S24BE, np.array([0x80, 0, 0, 0x7F, 0xFF, 0xFF, 0, 1, 0], np.uint8)).tolist() \
        == [-32768.0, 8388607 / 256.0, 1.0]
    assert speexhip.debug_format_decode(hm.S32BE, np.array([0x80, 0, 0, 0, 0, 1, 0, 0], np.uint8).view(">i4")).tolist() \
        == [-32768.0, 1.0]


# ---- round trips ---------------------------------------------------------------------------------------------------------
def test_every_half_float_code_round_trips_through_decode_and_encode():
    h = CODES.view(np.float16)
    keep = ~np.isnan(h)
    assert keep.sum() == 65536 - 2 * 1023
    back = speexhip.debug_format_encode(hm.F16N, speexhip.debug_format_decode(hm.F16N, h))
    assert same(back[keep], h[keep])
    # NaN codes come back canonical, by sign
    assert set(back.view(np.uint16)[~keep].tolist()) == {0x7E00, 0xFE00}
    assert (back.view(np.uint16)[~keep] & 0x8000 == CODES[~keep] & 0x8000).all()
    # bfloat16: every code whose decode is finite -- all but those with exponent field >= 0xF0, where the * 32768 overflows
    x = speexhip.debug_format_decode(hm.BF16N, CODES)
    finite = np.isfinite(x)
    left_out = ((CODES >> 7) & 0xFF) >= 0xF0
    assert left_out.sum() == 4096 and (finite == ~left_out).all()
    back = speexhip.debug_format_encode(hm.BF16N, x)
    assert same(back[finite], CODES[finite])
    for fmt in (hm.S16BE,):
        st = CODES.view(hm.dtype(fmt))
        assert same(speexhip.debug_format_encode(fmt, speexhip.debug_format_decode(fmt, st)), st)


# ---- encode --------------------------------------------------------------------------------------------------------------
def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def half_ties(fmt):
    """float32 y whose z = y / 32768 lies exactly half way between two neighbours of the half format: odd and even lower
    neighbours, normal and (F16N) subnormal results"""
    if fmt == hm.BF16N:
        hi = np.array([0x3F80, 0x3F81, 0x4000, 0x40FF, 0x0080, 0x0081, 0x7F7E, 0x7F7F, 0x3EFF], np.uint32)
        z = f32((hi << 16) | 0x8000)
    else:
        # binary16 has 10 fraction bits: in fp32 a tie has fraction bit 12 set and the 12 below clear
        mant = np.array([0, 1, 2, 3, 0x3FE, 0x3FF], np.uint32)
        exps = np.array([127 - 14, 127 - 1, 127, 127 + 14, 127 + 15], np.uint32)     # (127 + 15: ties up to 65520)
        z = f32(((exps[:, None] << 23) | (mant[None, :] << 13) | 0x1000).reshape(-1))
        # subnormal results: multiples of 2^-25 that are odd
        z = np.concatenate([z, (np.array([1, 3, 5, 2045, 2047], np.float32) * np.float32(2.0 ** -25))])
    z = np.concatenate([z, -z])
    y = z * np.float32(32768.0)
    ok = np.isfinite(y)
    assert (y[ok] * np.float32(1.0 / 32768.0) == z[ok]).all()
    return y[ok]


def half_inputs(fmt):
    rng = np.random.RandomState(2021 + fmt)
    full = rng.uniform(-32768.0, 32768.0, 200000).astype(np.float32)
    quiet = (rng.uniform(-32768.0, 32768.0, 200000) * 2.0 ** -20).astype(np.float32)
    wide = f32(rng.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32))     # every exponent, NaNs among them
    edges = np.float32([65504.0 * 32768.0, 65519.996 * 32768.0, 65520.0 * 32768.0, -65504.0 * 32768.0, -65520.0 * 32768.0,
                        3.0e38, -3.0e38, 0.0, -0.0, np.inf, -np.inf])
    big = f32([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF])                   # z near the fp32 / bf16 maximum
    # z = y / 32768 subnormal in fp32 (kept, not flushed), and y itself subnormal
    sub = f32([0x07800000, 0x07FFFFFF, 0x08000000, 0x07000001, 0x00000001, 0x007FFFFF, 0x87800000, 0x80000001, 0x03812345])
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA55AA5, 0xFFA55AA5])
    return np.concatenate([full, quiet, wide, edges, big, sub, nans, half_ties(fmt)])


@pytest.mark.parametrize("fmt", hm.HALF, ids=[hm.name(f) for f in hm.HALF])
def test_library_encode_of_the_half_formats_equals_the_model(fmt):
    y = half_inputs(fmt)
    got = speexhip.debug_format_encode(fmt, y)
    want = hm.from_internal(fmt, y)
    bad = np.nonzero(got.view(np.uint16) != want.view(np.uint16))[0]
    assert bad.size == 0, [(hex(y[i:i + 1].view(np.uint32)[0]), hex(got.view(np.uint16)[i]), hex(want.view(np.uint16)[i])) for i in bad[:8]]
    enc = lambda v: speexhip.debug_format_encode(fmt, np.asarray(v, np.float32)).view(np.uint16).tolist()
    # ties go to even; NaN is canonical by sign whatever its payload; +-0 keep their sign; +-inf stay
    if fmt == hm.F16N:
        assert enc([65504.0 * 32768.0, 65520.0 * 32768.0, -65520.0 * 32768.0]) == [0x7BFF, 0x7C00, 0xFC00]
        assert enc(f32([0x38801000, 0x38803000]) * np.float32(32768.0)) == [0x0400, 0x0402]      # (1 + 2^-11) 2^-14 ...
        assert enc(np.float32([2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25]) * np.float32(32768.0)) == [0x0001, 0x0000, 0x0002]
        canon = (0x7E00, 0xFE00)
    else:
        assert enc(f32([0x3F808000, 0x3F818000]) * np.float32(32768.0)) == [0x3F80, 0x3F82]
        assert enc(f32([0x7F7F8000])) == [0x7800]      # z = y / 32768 stays finite
        assert enc(f32([0x47FF8000]) * np.float32(1.0)) == [0x4080]
        canon = (0x7FC0, 0xFFC0)
    assert enc(f32([0x7FC00000, 0x7F800001, 0x7FA55AA5, 0xFFC00000, 0xFF800001, 0xFFFFFFFF])) == [canon[0]] * 3 + [canon[1]] * 3
    assert enc([0.0, -0.0]) == [0x0000, 0x8000]
    assert enc([np.inf, -np.inf]) == ([0x7C00, 0xFC00] if fmt == hm.F16N else [0x7F80, 0xFF80])
    assert enc([32768.0, -32768.0, 16384.0]) == ([0x3C00, 0xBC00, 0x3800] if fmt == hm.F16N else [0x3F80, 0xBF80, 0x3F00])


def pcm_inputs(fmt):
    rng = np.random.RandomState(77 + fmt)
    full = rng.uniform(-33000.0, 33000.0, 200000).astype(np.float32)
    quiet = (rng.uniform(-32768.0, 32768.0, 200000) * 2.0 ** -20).astype(np.float32)
    lsb = {hm.S16BE: 1.0, hm.S24BE: 1.0 / 256.0, hm.S32BE: 1.0 / 65536.0}[fmt]
    steps = np.array([-1.5, -1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5]) * lsb
    around = np.array([0.0, 1.0, -1.0, 1000.0, -1000.0, 32767.0, -32768.0, 32767.0 + 1 - lsb, 12345.0])
    edges = (around[:, None] + steps[None, :]).reshape(-1).astype(np.float32)
    rails = np.float32([32767.49, 32767.5, 32768.0, 40000.0, 1e9, 3e38, -32768.5, -32768.51, -32769.0, -40000.0, -1e9, -3e38,
                        -0.0, np.inf, -np.inf, np.nan, -np.nan])
    return np.concatenate([full, quiet, edges, rails])


@pytest.mark.parametrize("fmt", hm.BIG, ids=[hm.name(f) for f in hm.BIG])
def test_library_encode_of_the_big_endian_formats_equals_the_model(fmt):
    y = pcm_inputs(fmt)
    twin = hm.LE_TWIN[fmt]
    got = speexhip.debug_format_encode(fmt, y)
    assert got.dtype == hm.dtype(fmt) and same(got, hm.from_internal(fmt, y)), hm.name(fmt)
    assert same(hm.le_of(fmt, got), sf.from_internal(twin, y))           # the little-endian rule, bytes reversed
    values = lambda v: sf.integers(twin, hm.le_of(fmt, speexhip.debug_format_encode(fmt, np.asarray(v, np.float32)))).tolist()
    bits = 8 * hm.nbytes(fmt)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert values([np.inf, -np.inf, np.nan, -np.nan, 1e9, -1e9]) == [hi, lo, 0, 0, hi, lo]      # the rails, NaN -> 0
    k = 1 << (bits - 16)
    # ties go up, negative ones too: -0.5 LSB -> 0, -1.5 LSB -> -1, 0.5 LSB -> 1
    assert values(np.float32([-0.5, -1.5, 0.5]) / np.float32(k)) == [0, -1, 1]
    assert values([1.0, -1.0, 32767.0, -32768.0]) == [k, -k, 32767 * k, lo]
    # the bytes themselves: most significant first
    assert hm.raw(fmt, speexhip.debug_format_encode(fmt, np.float32([0x1234]))).tolist() == [0x12, 0x34] + [0] * (hm.nbytes(fmt) - 2)
    # all three dither kinds, d from the library's own generator (which is the model's)
    for kind in (dm.NONE,) + tuple(dm.KINDS):
        d = speexhip.debug_dither(kind, 0x1234567890ABCDEF, (1 << 32) - 1000, y.size)
        assert same(d, dm.values(kind, 0x1234567890ABCDEF, (1 << 32) - 1000, y.size))
        got_d = speexhip.debug_format_encode(fmt, y, d)
        assert same(got_d, hm.quantise(fmt, y, d)), (hm.name(fmt), dm.KIND_NAMES[kind])
        assert same(hm.le_of(fmt, got_d), dm.quantise(twin, y, d))
        assert same(got_d, got) == (kind == dm.NONE)       # (the noise does move samples; d = 0 does not)
