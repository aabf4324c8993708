"""CPU checks of the planar (one plane per channel) calls: the six entry points are declared, listed and exported; the
Node typings declare processChunkPlanar; kernels_planar.hip is part of the library (cross-compiled for gfx950 by
`make all`); and the LDS swizzles of its vector path are free of bank conflicts under a model of ds_write_b128 and
ds_read_b128 (lane groups and bank widths from the microarchitecture notes the kernel's header quotes)."""
import os
import re
import subprocess

import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
PLANAR = ["speexhip_resampler_process_planar_int", "speexhip_resampler_process_planar_float",
          "speexhip_resampler_process_planar_int_device", "speexhip_resampler_process_planar_float_device",
          "speexhip_batch_process_planar_int_device", "speexhip_batch_process_planar_float_device"]


def test_planar_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", header))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in PLANAR:
        assert name in declared, name + " not declared in the header"
        assert name in speexhip.EXPORTS, name + " not in EXPORTS"
        assert name in exported and hasattr(lib, name), name + " not exported"
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert len(getattr(lib, PLANAR[4]).argtypes) == 10 and len(getattr(lib, PLANAR[2]).argtypes) == 8
    assert "ABI note: 0.4 -> 0.5" in header


def test_bindings_offer_the_planar_methods():
    for cls, names in ((speexhip.Resampler, ("process_planar", "process_planar_device", "planar_call")),
                       (speexhip.Batch, ("process_planar_device", "process_tensor"))):
        for n in names:
            assert callable(getattr(cls, n, None)), "%s.%s" % (cls.__name__, n)
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert re.search(r"processChunkPlanar\(channels: Int16Array\[\]\): Int16Array\[\];", dts)
    assert re.search(r"processChunkPlanar\(channels: Float32Array\[\]\): Float32Array\[\];", dts)
    assert "processChunkPlanar(channels)" in open(os.path.join(PKG, "index.js")).read()
    assert '"processPlanar"' in open(os.path.join(PKG, "napi", "speex_hip_napi.c")).read()


def test_planar_kernels_are_built_for_gfx950_with_the_library():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/kernels_planar.hip" in mk and "csrc/planar.cpp" in mk
    # the device code of the library holds both kernels, for both sample types
    blob = open(speexhip.LIB_PATH, "rb").read()
    for kernel in (b"planar_gatherIs", b"planar_gatherIf", b"planar_scatterIs", b"planar_scatterIf"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob


# ---- the LDS layout of the vector path -------------------------------------------------------------------------------
# 16-byte chunks.  ds_write_b128: groups of 8 contiguous lanes, banks (a / 4) % 32 -> chunk % 8;
# ds_read_b128: four groups of 16 lanes, banks (a / 4) % 64 -> chunk % 16.
READ_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(8 * i, 8 * i + 8)) for i in range(8)]


def _ways(chunk_of_lane, groups, chunks_per_row):
    worst = 1
    for g in groups:
        rows = {}
        for lane in g:
            rows.setdefault(chunk_of_lane(lane) % chunks_per_row, set()).add(chunk_of_lane(lane))
        worst = max(worst, max(len(v) for v in rows.values()))
    return worst


def test_planar_lds_swizzles_are_conflict_free():
    src = open(os.path.join(PKG, "csrc", "kernels_planar.hip")).read()
    table = src[src.index("constexpr Swizzle kSwizzle[]"):]
    table = table[: table.index("};")]
    rows = [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", table)]
    assert sorted((r[0], r[1]) for r in rows) == [(c, s) for c in (2, 4, 6, 8) for s in (0, 1)]
    lanes = 256
    for channels, scatter, a, m, b, n in rows:
        assert m < (1 << a) and n < (1 << b), "the swizzle must be a bijection (it may only mix higher bits into lower ones)"

        def swz(q):
            return q ^ ((q >> a) & m) ^ ((q >> b) & n)

        assert sorted(swz(q) for q in range(lanes * channels)) == list(range(lanes * channels))
        strided_groups, strided_row = (READ_GROUPS, 16) if scatter else (WRITE_GROUPS, 8)
        linear_groups, linear_row = (WRITE_GROUPS, 8) if scatter else (READ_GROUPS, 16)
        for wave in range(lanes // 64):
            for k in range(channels):
                assert _ways(lambda l: swz((wave * 64 + l) * channels + k), strided_groups, strided_row) == 1, (channels, scatter, k)
                assert _ways(lambda l: swz(k * lanes + wave * 64 + l), linear_groups, linear_row) == 1, (channels, scatter, k)
