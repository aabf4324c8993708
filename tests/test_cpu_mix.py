"""CPU checks of the mixed calls (a channel matrix before the FIR and / or after it, folded into the formatted call's two
passes): the three entry points are declared, listed and exported; both ABI notes stand in the header; the Makefile
builds the new files and the library holds both mixing kernels for gfx950; the bindings offer the methods; and the numpy
statement of the mix (channel_mix.py) is the rule the header states -- fp64 products, sums in ascending order, one
rounding."""
import os
import re
import subprocess

import numpy as np

import channel_mix as cm
import speexhip
from golden_util import ROOT

PKG = os.path.join(ROOT, "node-speex-resampler_amd")
MIXED = ["speexhip_resampler_process_interleaved_mix", "speexhip_resampler_process_interleaved_mix_device",
         "speexhip_batch_process_interleaved_mix_device"]


def test_mixed_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "speexhip_resampler.h")).read()
    declared = set(re.findall(r"\b(speexhip_\w+)\s*\(", header))
    lib = speexhip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", speexhip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in MIXED:
        assert name in declared, name + " not declared in the header"
        assert name in speexhip.EXPORTS, name + " not in EXPORTS"
        assert name in exported and hasattr(lib, name), name + " not exported"
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert [len(getattr(lib, n).argtypes) for n in MIXED] == [11, 12, 14]
    assert "ABI note: 0.5 -> 0.6" in header and "ABI note: 0.6 -> 0.7" in header
    assert b"0.7.0" in lib.speexhip_version()


def test_mix_kernels_are_built_for_gfx950_with_the_library():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/kernels_mix.hip" in mk and "csrc/mix.cpp" in mk
    blob = open(speexhip.LIB_PATH, "rb").read()
    for kernel in (b"mix_inILi", b"mix_outILi", b"warm_kernel_mix"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    # one statement of the formats for both kernel files
    for unit in ("kernels_convert.hip", "kernels_mix.hip"):
        assert '#include "format_device.h"' in open(os.path.join(PKG, "csrc", unit)).read(), unit


def test_bindings_offer_the_mixed_calls():
    for cls, names in ((speexhip.Resampler, ("mix_call", "process_mix", "process_mix_device")),
                       (speexhip.Batch, ("process_mix_device", "process_tensor"))):
        for n in names:
            assert callable(getattr(cls, n, None)), "%s.%s" % (cls.__name__, n)
    import inspect
    params = inspect.signature(speexhip.Batch.process_tensor).parameters
    assert "in_mix" in params and "out_mix" in params
    assert params["in_mix"].default is None and params["out_mix"].default is None
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert "processChunkMix(" in dts


def test_numpy_mix_identity_scale_and_average():
    rng = np.random.RandomState(7)
    x = (rng.standard_normal((1000, 5)) * 9000.0).astype(np.float32)
    # an identity matrix returns the input bits (the other terms add exact zeros)
    assert cm.mix(np.eye(5, dtype=np.float32), x).tobytes() == x.tobytes()
    # a single power-of-two coefficient is an exact scale
    M = np.zeros((1, 5), np.float32)
    M[0, 3] = 0.25
    assert cm.mix(M, x).reshape(-1).tobytes() == (x[:, 3] * np.float32(0.25)).tobytes()
    # [[0.5, 0.5]] on (a, a) returns a
    a = x[:, 0]
    assert cm.mix(cm.STEREO_TO_MONO, np.stack([a, a], axis=1)).reshape(-1).tobytes() == a.tobytes()
    # shapes: (frames, outputs), whatever the shape the frames come in
    assert cm.mix(cm.SURROUND_TO_STEREO, x[:, :3].reshape(-1)).shape == (500, 2)
    assert cm.mix(cm.MONO_TO_STEREO, a).shape == (1000, 2)


def test_numpy_mix_sums_in_ascending_order():
    """One frame by hand: M = [1, 1, 1], x = (1, 2^60, -2^60).  Ascending: 1 + 2^60 rounds to 2^60 in fp64 (53 bits), and
    2^60 - 2^60 = 0.  Descending: -2^60 + 2^60 = 0, and 0 + 1 = 1.  The rule is the ascending one."""
    M = np.float32([[1.0, 1.0, 1.0]])
    x = np.float32([1.0, 2.0 ** 60, -(2.0 ** 60)])
    assert (np.float64(1.0) + np.float64(2.0 ** 60)) - np.float64(2.0 ** 60) == 0.0
    assert (np.float64(-(2.0 ** 60)) + np.float64(2.0 ** 60)) + np.float64(1.0) == 1.0
    assert cm.mix(M, x).tolist() == [[0.0]]
    assert cm.mix_descending(M, x).tolist() == [[1.0]]
    # ... and one where the difference is a last-place one after the rounding to float32.  M = [1, 1, 24929],
    # x = (c, c, 673) with c = 3 * 2^-31: the product 24929 * 673 = 2^24 + 1 is exact in fp64 and lies halfway between the
    # float32 neighbours 2^24 and 2^24 + 2; an fp64 step there is 2^-28.  Ascending: c + c = 0.75 steps, which rounds the
    # sum up to 2^24 + 1 + 2^-28 -- above the halfway point, float32 2^24 + 2.  Descending: c alone is 0.375 steps and is
    # lost twice; the sum stays 2^24 + 1, and the tie goes to the even float32, 2^24.
    M = np.float32([[1.0, 1.0, 24929.0]])
    c = np.float32(3.0 * 2.0 ** -31)
    x = np.float32([c, c, 673.0])
    assert np.float64(M[0, 2]) * np.float64(x[2]) == 2.0 ** 24 + 1.0
    assert cm.mix(M, x).tolist() == [[2.0 ** 24 + 2.0]]
    assert cm.mix_descending(M, x).tolist() == [[2.0 ** 24]]
    # a product is taken in fp64, not rounded to fp32 first: 3 * (1/3 in fp32) is not 1 in fp32 arithmetic's way
    third = np.float32(1.0) / np.float32(3.0)
    want = np.float32(np.float64(np.float32(3.0)) * np.float64(third) + np.float64(np.float32(2.0 ** -24)) * np.float64(third))
    assert cm.mix(np.float32([[3.0, 2.0 ** -24]]), np.float32([third, third]))[0, 0] == want
