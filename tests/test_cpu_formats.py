"""CPU checks of the formatted calls (sample formats u8, s16, packed s24, s32, float in int16 units and in +-1.0, input
and output named independently): the entry points are declared, listed and exported; both ABI notes stand in the header;
speexhip_sample_bytes; the Makefile builds the two new files and the library holds both converting kernels for gfx950;
the Node binding declares processChunkFormat; and the numpy statement of the formats (sample_formats.py) round-trips and
rounds half up."""
import os
import re
import subprocess

import numpy as np

import sample_formats as sf
import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
FORMATTED = ["speexhip_sample_bytes", "speexhip_resampler_process_interleaved_fmt",
             "speexhip_resampler_process_interleaved_fmt_device", "speexhip_batch_process_interleaved_fmt_device"]


def test_formatted_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", header))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in FORMATTED:
        assert name in declared, name + " not declared in the header"
        assert name in speexhip.EXPORTS, name + " not in EXPORTS"
        assert name in exported and hasattr(lib, name), name + " not exported"
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert [len(getattr(lib, n).argtypes) for n in FORMATTED] == [1, 7, 8, 10]
    assert "ABI note: 0.4 -> 0.5" in header and "ABI note: 0.5 -> 0.6" in header
    for i, name in enumerate(("U8", "S16", "S24", "S32", "F32", "F32N")):
        assert re.search(r"SPEEXHIP_FMT_%s = %d\b" % (name, i), header), name
        assert getattr(speexhip, "FMT_" + name) == i == getattr(sf, name)


def test_sample_bytes():
    lib = speexhip.lib()
    assert [lib.speexhip_sample_bytes(f) for f in range(6)] == [1, 2, 3, 4, 4, 4] == list(sf.BYTES) == list(speexhip.FMT_BYTES)
    for unknown in (-1, 6, 99, 1 << 20):
        assert lib.speexhip_sample_bytes(unknown) == 0


def test_convert_kernels_are_built_for_gfx950_with_the_library():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/kernels_convert.hip" in mk and "csrc/formats.cpp" in mk
    blob = open(speexhip.LIB_PATH, "rb").read()
    for kernel in (b"convert_inILi", b"convert_outILi", b"warm_kernel_convert"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob


def test_bindings_offer_the_formatted_calls():
    for cls, names in ((speexhip.Resampler, ("process_fmt", "process_fmt_device", "fmt_call")),
                       (speexhip.Batch, ("process_fmt_device", "process_tensor"))):
        for n in names:
            assert callable(getattr(cls, n, None)), "%s.%s" % (cls.__name__, n)
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert re.search(r"processChunkFormat\(chunk: Buffer, inFormat: SampleFormat, outFormat: SampleFormat\): Buffer;", dts)
    for name in ("u8", "s16le", "s24le", "s32le", "f32le", "f32le-normalized"):
        assert "'%s'" % name in dts, name
    assert "processChunkFormat(chunk, inFormat, outFormat)" in open(os.path.join(PKG, "index.js")).read()
    assert '"processFormat"' in open(os.path.join(PKG, "napi", "speex_hip_napi.c")).read()


def test_numpy_formats_round_trip():
    # every representable value of the small formats
    for fmt, values in ((sf.U8, np.arange(256)), (sf.S16, np.arange(-32768, 32768))):
        storage = sf.store(fmt, values)
        assert sf.from_internal(fmt, sf.to_internal(fmt, storage)).tobytes() == storage.tobytes(), sf.NAMES[fmt]
    # the rails and a random million of the wide ones
    rng = np.random.RandomState(24)
    for fmt, bits in ((sf.S24, 24), (sf.S32, 32)):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        values = np.concatenate([np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi], np.int64),
                                 rng.randint(lo, hi + 1, 1000000, dtype=np.int64)])
        if fmt == sf.S32:
            # float32 holds 24 significant bits: the round trip is exact on values that have no more -- and lands on the
            # nearest float32 (ties to even, saturated) on the rest
            exact = (values >> 8) << 8
            storage = sf.store(fmt, exact)
            assert sf.from_internal(fmt, sf.to_internal(fmt, storage)).tobytes() == storage.tobytes()
            back = sf.integers(fmt, sf.from_internal(fmt, sf.to_internal(fmt, sf.store(fmt, values))))
            want = np.clip(values.astype(np.int32).astype(np.float32).astype(np.float64), lo, hi).astype(np.int64)
            assert np.array_equal(back, want)
        else:
            storage = sf.store(fmt, values)
            assert storage.dtype == np.uint8 and storage.size == 3 * values.size
            assert np.array_equal(sf.unpack_s24(storage), values)
            assert sf.from_internal(fmt, sf.to_internal(fmt, storage)).tobytes() == storage.tobytes()
    x = rng.standard_normal(1000).astype(np.float32)
    assert sf.from_internal(sf.F32N, sf.to_internal(sf.F32N, x)).tobytes() == x.tobytes()
    assert sf.to_internal(sf.F32N, np.float32([1.0, -0.5])).tolist() == [32768.0, -16384.0]
    assert sf.to_internal(sf.U8, np.uint8([0, 128, 255])).tolist() == [-32768.0, 0.0, 32512.0]
    assert sf.to_internal(sf.S24, sf.pack_s24([-(1 << 23), 1, 255])).tolist() == [-32768.0, 1 / 256.0, 255 / 256.0]


def test_numpy_formats_round_ties_upward_and_saturate():
    assert sf.halfup([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, -2.500001, 2.499999]).tolist() == [-2, -1, 0, 1, 2, 3, -3, 2]
    y = np.float32([-2.5, -0.5, 0.5, 2.5, 40000.0, -40000.0, np.inf, -np.inf, np.nan])
    assert sf.from_internal(sf.S16, y).tolist() == [-2, 0, 1, 3, 32767, -32768, 32767, -32768, 0]
    assert sf.integers(sf.S24, sf.from_internal(sf.S24, y / np.float32(256))).tolist() == \
        [-2, 0, 1, 3, 40000, -40000, (1 << 23) - 1, -(1 << 23), 0]
    assert sf.from_internal(sf.S32, y / np.float32(65536)).tolist() == \
        [-2, 0, 1, 3, 40000, -40000, (1 << 31) - 1, -(1 << 31), 0]
    assert sf.from_internal(sf.S32, np.float32([32768.0, -32768.0, 32767.5])).tolist() == [(1 << 31) - 1, -(1 << 31), 32767.5 * 65536]
    # U8: one step = 256 int16 steps; ties upward, 128 is zero, NaN -> 128
    yu = np.float32([-128.0, -384.0, 128.0, 127.9, 40000.0, -40000.0, np.nan, np.inf, -np.inf])
    assert sf.from_internal(sf.U8, yu).tolist() == [128, 127, 129, 128, 255, 0, 128, 255, 0]
    # the float formats never saturate
    big = np.float32([1e9, -1e9, np.inf])
    assert sf.from_internal(sf.F32, big).tobytes() == big.tobytes()
    assert sf.from_internal(sf.F32N, big).tolist() == (big / np.float32(32768)).tolist()
