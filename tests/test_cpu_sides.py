"""Layouts (the sides calls) without a GPU: the entry points are declared, listed and exported, the ABI note stands, the
new kernel unit is built for gfx950 and warmed up, the bindings offer the methods and keywords, and the ctypes Side is
the header's struct."""
import ctypes as C
import inspect
import os
import re
import subprocess

import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
ENTRY_POINTS = ["speexhip_resampler_process_sides", "speexhip_resampler_process_sides_device",
                "speexhip_batch_process_sides_device"]
FORMATS = (0, 1, 2, 3, 4, 5, 16, 17)
DITHERED = (0, 1, 2, 3, 16, 17)


def header():
    return open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()


def test_entry_points_are_declared_listed_and_exported():
    h = header()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", h))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for nm in ENTRY_POINTS:
        assert nm in declared, nm + " not declared in the header"
        assert nm in speexhip.EXPORTS, nm + " not in EXPORTS"
        assert nm in exported and hasattr(lib, nm), nm + " not exported"
    assert [len(getattr(lib, n).argtypes) for n in ENTRY_POINTS] == [5, 6, 6]
    assert "0.7.0" in lib.speexhip_version().decode()


def test_abi_note_and_the_enum_stand_in_the_header():
    h = header()
    assert re.search(r"\* Layouts: a side of a call", h)
    assert re.search(r"ABI note: 0\.7 \+ layouts adds one enum, one struct and three entry points; SpeexHipInfo, the error\s+"
                     r"\* codes and the version string are unchanged", h)
    assert re.search(r"SPEEXHIP_LAYOUT_INTERLEAVED = 0, SPEEXHIP_LAYOUT_PLANAR = 1", h)
    assert (speexhip.LAYOUT_INTERLEAVED, speexhip.LAYOUT_PLANAR) == (0, 1)
    for field in ("struct_size", "fmt", "channels", "layout", "mix", "data", "plane_stride", "stream_stride", "planes"):
        assert re.search(r"\b%s;" % field, h[h.index("typedef struct SpeexHipSide"):h.index("} SpeexHipSide;")]), field


def test_new_unit_is_built_for_gfx950_and_warmed_up():
    mk = open(os.path.join(PKG, "Makefile")).read()
    src = re.search(r"^SRC = (.*?)\n(?!\s)", mk, re.S | re.M).group(1)
    assert "csrc/kernels_sides.hip" in src            # product and diag builds both come from SRC
    assert "DIAG_OBJ = $(patsubst csrc/%,build/diag/%.o,$(SRC))" in mk
    unit = open(os.path.join(PKG, "csrc", "kernels_sides.hip")).read()
    assert "SPEEXHIP_WARM_UNIT(sides)" in unit
    assert "warm_unit_sides(s);" in open(os.path.join(PKG, "csrc", "engine.cpp")).read()
    assert re.search(r"constexpr uint32_t kSidesTileFrames = 1024;", open(os.path.join(PKG, "csrc", "kernels.h")).read())
    blob = open(speexhip.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"warm_kernel_sides" in blob
    # (the Itanium mangling of a template argument: ILi<format>E)
    for fmt in FORMATS:
        for kernel in ("planes_in", "planes_out"):
            assert ("%sILi%dEE" % (kernel, fmt)).encode() in blob, (kernel, fmt)
    for fmt in DITHERED:
        assert ("planes_out_ditherILi%dEE" % fmt).encode() in blob, fmt
    # the existing passes keep their names
    for kernel in ("convert_in", "convert_out", "convert_out_dither", "mix_in", "mix_out", "mix_out_dither"):
        assert ("%sILi1EE" % kernel).encode() in blob, kernel
    assert b"planar_gather" in blob and b"planar_scatter" in blob


def test_bindings_offer_the_methods_and_keywords():
    for cls, names in ((speexhip.Resampler, ("sides_call", "process_sides", "process_sides_device")),
                       (speexhip.Batch, ("process_sides_device",))):
        for nm in names:
            assert callable(getattr(cls, nm)), (cls.__name__, nm)
    sig = inspect.signature(speexhip.Batch.process_tensor)
    for kw in ("in_layout", "out_layout", "normalized", "out_dtype", "in_mix", "out_mix", "in_format", "out_format"):
        assert kw in sig.parameters, kw
    assert sig.parameters["in_layout"].default is None and sig.parameters["out_layout"].default is None
    doc = speexhip.Batch.process_tensor.__doc__
    assert "in_layout='planar'" in doc and "no transpose" in doc
    for rel, words in (("index.js", ("processChunkSides",)), ("index.d.ts", ("processChunkSides", "planar")),
                       (os.path.join("napi", "speex_hip_napi.c"), ("speexhip_resampler_process_sides",)),
                       (os.path.join("test", "test_sides.js"), ("ALL SIDES NODE TESTS PASSED",))):
        text = open(os.path.join(PKG, rel)).read()
        for w in words:
            assert w in text, (rel, w)


def test_ctypes_side_is_the_headers_struct(tmp_path):
    src = tmp_path / "side_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "speexhip_resampler.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(SpeexHipSide), offsetof(SpeexHipSide, mix), '
                   'offsetof(SpeexHipSide, data), offsetof(SpeexHipSide, plane_stride), offsetof(SpeexHipSide, planes)); '
                   'return 0; }\n')
    exe = tmp_path / "side_size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = speexhip.Side
    assert got == [C.sizeof(S), S.mix.offset, S.data.offset, S.plane_stride.offset, S.planes.offset]
    side = speexhip.make_side(speexhip.FMT_S16, 2, speexhip.LAYOUT_PLANAR, plane_stride=480)
    assert side.struct_size == C.sizeof(S) and (side.fmt, side.channels, side.layout, side.plane_stride) == (1, 2, 1, 480)


def test_argument_errors_need_no_device():
    """what the C layer refuses before it reaches a state's device: NULL handles and sides it cannot read"""
    lib = speexhip.lib()
    a, b = speexhip.make_side(1, 2), speexhip.make_side(1, 2)
    il, ol = C.c_uint32(10), C.c_uint32(20)
    for fn, extra in ((lib.speexhip_resampler_process_sides, ()), (lib.speexhip_resampler_process_sides_device, (None,)),
                      (lib.speexhip_batch_process_sides_device, (None,))):
        assert fn(None, C.byref(a), C.byref(il), C.byref(b), C.byref(ol), *extra) == speexhip.ERR_INVALID_ARG
    assert (il.value, ol.value) == (10, 20)
