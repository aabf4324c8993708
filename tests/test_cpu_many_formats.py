"""The formatted many-states call without a GPU: the entry points and the counter function are declared, listed and
exported, the calls refuse what they must before any device is touched, the new kernel unit and the shared bodies are
built for gfx950 with the library, and SpeexResamplerBatch.processChunksFormat checks its arguments before any state."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
ENTRY_POINTS = ["speexhip_resampler_process_many_sides", "speexhip_resampler_process_many_fmt", "speexhip_debug_many_counters"]


def test_entry_points_are_declared_listed_and_exported():
    h = open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", h))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for nm in ENTRY_POINTS:
        assert nm in declared, nm + " not declared in the header"
        assert nm in speexhip.EXPORTS, nm + " not in EXPORTS"
        assert nm in exported and hasattr(lib, nm), nm + " not exported"
    assert [len(getattr(lib, n).argtypes) for n in ENTRY_POINTS] == [7, 9, 1]
    assert re.search(r"\* Many states, formatted:", h)
    assert re.search(r"ABI note: 0\.7 \+ many formats adds these three entry points", h)
    assert "NOT fused" in h     # matrices and planar layouts are correct through the call, and the header says they are not fused


def test_empty_call_and_null_state_without_a_device():
    assert speexhip.many_fmt_call([], [], [], [], [], [], []) == (0, [], [], [])
    assert speexhip.process_many_sides([], [], [], [], []) == (0, [], [], [])
    inv = speexhip.ERR_INVALID_ARG
    rc, used, made, codes = speexhip.many_fmt_call([None, None], speexhip.FMT_ULAW, [None, None], [160, 5], speexhip.FMT_F32N,
                                                   [None, None], [400, 7])
    assert (rc, codes) == (inv, [inv, inv]) and (used, made) == ([160, 5], [400, 7])     # the lengths stay as they were
    side = speexhip.make_side(speexhip.FMT_S16, 1)
    rc, used, made, codes = speexhip.process_many_sides([None], [side], [3], [side], [9])
    assert (rc, codes, used, made) == (inv, [inv], [3], [9])
    # NULL arrays with n > 0
    L = speexhip.lib()
    assert L.speexhip_resampler_process_many_fmt(1, None, None, None, None, None, None, None, None) == inv
    assert L.speexhip_resampler_process_many_sides(1, None, None, None, None, None, None) == inv
    assert L.speexhip_resampler_process_many_fmt(0, None, None, None, None, None, None, None, None) == 0


def test_counters_start_and_stay_at_rest_without_a_launch():
    before = speexhip.many_counters()
    assert sorted(before) == ["fir_launches", "in_passes", "out_passes", "own_calls"]
    speexhip.many_fmt_call([None], 1, [None], [0], 1, [None], [0])
    assert speexhip.many_counters() == before      # an argument error launches nothing and takes no call of its own
    speexhip.lib().speexhip_debug_many_counters(None)   # (a NULL destination is ignored)


def test_the_new_unit_shares_the_bodies_and_is_built_for_gfx950():
    mk = open(os.path.join(PKG, "Makefile")).read()
    src = re.search(r"^SRC = (.*?)\n(?!\s)", mk, re.S | re.M).group(1)
    assert "csrc/kernels_convert_many.hip" in src and "csrc/kernels_convert.hip" in src
    one = open(os.path.join(PKG, "csrc", "kernels_convert.hip")).read()
    many = open(os.path.join(PKG, "csrc", "kernels_convert_many.hip")).read()
    impl = open(os.path.join(PKG, "csrc", "kernels_convert_impl.h")).read()
    for unit in (one, many):
        assert '#include "kernels_convert_impl.h"' in unit and "stream_tile<" in unit
        assert "void vector_tile(" not in unit and "void element_tile(" not in unit     # stated once, in the shared header
    assert "void vector_tile(" in impl and "void element_tile(" in impl and "void stream_tile(" in impl
    assert "SPEEXHIP_WARM_UNIT(convert_many)" in many
    assert "warm_unit_convert_many(s);" in open(os.path.join(PKG, "csrc", "engine.cpp")).read()
    blob = open(speexhip.LIB_PATH, "rb").read()
    for kernel in (b"convert_many_in", b"convert_many_out", b"warm_kernel_convert_many"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob


def test_bindings_offer_the_calls():
    for nm in ("process_many_fmt", "process_many_sides", "many_fmt_call", "many_counters"):
        assert callable(getattr(speexhip, nm, None)), nm
    for rel, words in (("index.js", ("processChunksFormat(", "processChunksFormatAsync(", "processManyFormat(", "processManyFormatAsync(")),
                       ("index.d.ts", ("processChunksFormat(", "processChunksFormatAsync(")),
                       (os.path.join("napi", "speex_hip_napi.c"), ("speexhip_resampler_process_many_fmt", '"processManyFormat"',
                                                                   '"processManyFormatAsync"'))):
        text = open(os.path.join(PKG, rel)).read()
        for w in words:
            assert w in text, (rel, w)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_batch_formatted_step_checks_its_arguments_before_any_state():
    if not os.path.exists(os.path.join(PKG, "speex_hip_napi.node")):
        pytest.skip("addon not built")
    js = r"""
const R = require(process.argv[1]);
const addon = require(require('path').join(require('path').dirname(process.argv[1]), 'speex_hip_napi.node'));
const out = {};
const grab = (k, f) => { try { const v = f(); out[k] = v === undefined ? 'no throw' : v; } catch (e) { out[k] = e.constructor.name + ': ' + e.message; } };
R.default.initPromise.then(async () => {
  const b = new R.SpeexResamplerBatch(3, 1, 8000, 16000, 7, { devices: [0] });
  const three = () => [Buffer.alloc(8), Buffer.alloc(8), Buffer.alloc(8)];
  grab('count', () => b.processChunksFormat([Buffer.alloc(8)], 'mulaw', 'f32le-normalized'));
  grab('align', () => b.processChunksFormat([Buffer.alloc(8), Buffer.alloc(7), Buffer.alloc(9)], ['mulaw', 's16be', 's24le'], 'f32le-normalized'));
  grab('align24', () => b.processChunksFormat([Buffer.alloc(8), Buffer.alloc(8), Buffer.alloc(8)], ['mulaw', 's16be', 's24le'], 'f32le-normalized'));
  grab('name', () => b.processChunksFormat(three(), ['mulaw', 'pcmu', 'alaw'], 'f32le-normalized'));
  grab('outName', () => b.processChunksFormat(three(), 'mulaw', 'f64'));
  grab('names', () => b.processChunksFormat(three(), ['mulaw', 'alaw'], 'f32le-normalized'));
  grab('allNull', () => JSON.stringify(b.processChunksFormat([null, null, null], 'mulaw', 's16le')));
  out.untouched = b.streams.every((r) => !r._resamplerPtr);
  out.asyncName = await b.processChunksFormatAsync(three(), 'mulaw', 'nope').then(() => 'resolved', (e) => e.message);
  grab('manyTypes', () => addon.processManyFormat(1, 2, 3, 4, 5, 6));
  grab('manyFew', () => addon.processManyFormat([], [], [], []));
  grab('manyEmpty', () => addon.processManyFormat([], [], [], [], [], []).length);
  console.log(JSON.stringify(out));
});
"""
    res = subprocess.run(["node", "-e", js, os.path.join(PKG, "index.js")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout)
    assert "one chunk (or null) per stream: 3" in out["count"]
    assert out["align"] == "Error: Chunk length should be a multiple of channels * 2 bytes"
    assert out["align24"] == "Error: Chunk length should be a multiple of channels * 3 bytes"
    assert out["name"] == "Error: Unknown sample format: pcmu" and out["outName"] == "Error: Unknown sample format: f64"
    assert "one format name, or one per stream: 3" in out["names"]
    assert out["allNull"] == "[null,null,null]"
    assert out["untouched"] is True          # every refusal came before any stream's native state was made
    assert out["asyncName"] == "Unknown sample format: nope"
    assert out["manyTypes"].startswith("TypeError") and out["manyFew"].startswith("TypeError") and out["manyEmpty"] == 0
