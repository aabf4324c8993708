"""The formatted chunks call without a GPU: the three symbols (speexhip_resampler_process_chunks_sides / _fmt,
speexhip_debug_chunk_counters) are exported, declared and bound; the Node layer names its new methods and options; the
counters have their four keys and an argument error moves none of them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
SYMBOLS = ("speexhip_resampler_process_chunks_sides", "speexhip_resampler_process_chunks_fmt", "speexhip_debug_chunk_counters")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_three_symbols_are_exported_declared_and_bound():
    header = read(ROOT, "include", "speexhip_resampler.h")
    nm = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    lib = speexhip.lib()
    for name in SYMBOLS:
        assert re.search(r"SPEEXHIP_API\s+\w+\s+" + name + r"\s*\(", header), name
        assert name in speexhip.EXPORTS and name in exported and hasattr(lib, name), name
    assert "0.7 + chunk sides" in header
    for method in ("process_chunks_sides", "process_chunks_fmt"):
        assert callable(getattr(speexhip.Resampler, method))


def test_the_node_layer_names_the_new_methods_and_options():
    js, dts = read(PKG, "index.js"), read(PKG, "index.d.ts")
    node_test = read(PKG, "test", "test_chunk_formats.js")
    napi = read(PKG, "napi", "speex_hip_napi.c")
    for name in ("processChunksFormat", "processChunksFormatAsync", "processChunkFormatAsync", "flushFormat", "inFormat",
                 "outFormat"):
        assert name in js and name in dts and name in node_test, name
    for name in ('"processChunksFormat"', '"processChunksFormatAsync"', "speexhip_resampler_process_chunks_fmt"):
        assert name in napi, name
    for option in ("coalesceChunks", "async", "pipeline", "pinned", "flushTail"):
        assert option in node_test, option


def test_chunk_counters_have_four_keys_and_an_argument_error_leaves_them():
    before = speexhip.chunk_counters()
    assert sorted(before) == ["fir_launches", "in_passes", "out_passes", "own_calls"]
    assert all(isinstance(v, int) and v >= 0 for v in before.values())
    L = speexhip.lib()
    n = 3
    raw = np.zeros(64, np.uint8)
    out = np.zeros(1024, np.uint8)
    ptrs = (C.c_void_p * n)(*[raw.ctypes.data] * n)
    il, ol = (C.c_uint32 * n)(8, 8, 8), (C.c_uint32 * n)(16, 16, 16)
    a = speexhip.make_side(speexhip.FMT_ULAW, 1)
    b = speexhip.make_side(speexhip.FMT_F32N, 1, data=out.ctypes.data)
    # a NULL state is INVALID_ARG, in both forms; so are NULL length arrays
    assert L.speexhip_resampler_process_chunks_sides(None, n, C.byref(a), ptrs, il, C.byref(b), ol) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_resampler_process_chunks_fmt(None, n, speexhip.FMT_ULAW, ptrs, il, speexhip.FMT_F32N,
                                                   C.c_void_p(out.ctypes.data), ol) == speexhip.ERR_INVALID_ARG
    assert list(il) == [8, 8, 8] and list(ol) == [16, 16, 16] and not out.any()
    assert speexhip.chunk_counters() == before
    L.speexhip_debug_chunk_counters(None)   # (a NULL array is ignored)
