"""The mixer's levels on the host (include/speexhip_resampler.h, "Mixer levels"): the header declares the record and the
four entry points, the Makefile names the kernel's unit, the Python binding exports every symbol -- and the statement
itself: speexhip_debug_levels compiles the very lines the kernel compiles (csrc/levels.h) and must equal the numpy model
(levels_model.py) field for field at the points where a wrong level shows, and over random floats at an amplitude where
the rounding decides most of the energy (3) and at one where the rails do (40 000).  Then the defects that
levels_model.record(defect=) can plant: each must change the model's record on a stated synthetic input (the shares are
printed with -s).  Last, the RFC 6464 value.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import levels_model as lm
import speexhip
from golden_util import ROOT

ALL = ("speexhip_mixer_set_levels", "speexhip_mixer_get_levels", "speexhip_debug_levels", "speexhip_debug_mixer_level_launches")


def lib_record(y):
    return lm.of_struct(speexhip.debug_levels(y)[0])


def test_the_header_declares_the_record_and_the_four_symbols():
    with open(os.path.join(ROOT, "include", "speexhip_resampler.h")) as f:
        text = f.read()
    assert re.search(r"SPEEXHIP_API int speexhip_mixer_set_levels\(SpeexHipMixer \*m, int on\)", text)
    assert re.search(r"SPEEXHIP_API int speexhip_mixer_get_levels\(SpeexHipMixer \*m, uint32_t first_slot, uint32_t count, void \*levels,\s+uint32_t struct_size\)", text)
    assert re.search(r"SPEEXHIP_API int speexhip_debug_levels\(const float \*y, uint32_t n, SpeexHipLevel \*l\)", text)
    assert re.search(r"SPEEXHIP_API uint64_t speexhip_debug_mixer_level_launches\(void\)", text)
    assert re.search(r"typedef struct SpeexHipLevel \{\s*uint64_t samples, energy, nan;\s*float peak;\s*uint32_t reserved;\s*\} SpeexHipLevel;", text)
    assert "Mixer levels" in text and "2^34" in text
    assert speexhip.LEVEL_DTYPE.itemsize == 32
    assert [speexhip.LEVEL_DTYPE.fields[k][1] for k in ("samples", "energy", "nan", "peak")] == [0, 8, 16, 24]


def test_the_library_and_the_binding_export_them():
    L = speexhip.lib()
    for name in ALL:
        assert name in speexhip.EXPORTS and getattr(L, name)
    for name in ("set_levels", "get_levels"):
        assert callable(getattr(speexhip.Mixer, name))
    assert callable(speexhip.audio_level)
    # NULL handles: an argument error, never a crash (host only: nothing here reaches a device)
    rec = np.zeros(1, speexhip.LEVEL_DTYPE)
    assert L.speexhip_mixer_set_levels(None, 1) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_get_levels(None, 0, 1, C.c_void_p(rec.ctypes.data), 32) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_levels(None, 0, None) == speexhip.ERR_INVALID_ARG
    y = np.ones(1, np.float32)
    assert L.speexhip_debug_levels(None, 1, C.c_void_p(rec.ctypes.data)) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_debug_levels(C.c_void_p(y.ctypes.data), 0, C.c_void_p(rec.ctypes.data)) == 0 and lm.same(lm.of_struct(rec[0]), lm.ZERO)
    assert isinstance(speexhip.debug_mixer_level_launches(), int)


def test_the_makefile_and_the_warm_up_name_the_new_unit():
    pkg = os.path.join(ROOT, "node-speex-resampler_amd")
    with open(os.path.join(pkg, "Makefile")) as f:
        text = f.read()
    assert "csrc/kernels_levels.hip" in text[text.index("SRC ="): text.index("OBJ =")]
    with open(os.path.join(pkg, "csrc", "engine.cpp")) as f:
        assert "warm_unit_levels(s);" in f.read()
    with open(os.path.join(pkg, "csrc", "kernels_levels.hip")) as f:
        kernel = f.read()
    assert "SPEEXHIP_WARM_UNIT(levels)" in kernel and not re.search(r"atomic[A-Z_]", kernel), "the records may lie in pinned host memory"


# ---- the statement at its decision points -------------------------------------------------------------------------------
DENORMAL = np.float32(1e-42)
POINTS = {
    "+0.5": (0.5, 1), "-0.5": (-0.5, 0), "+1.5": (1.5, 2), "-1.5": (-1.5, -1),
    "just under +0.5": (0.49999997, 0), "just under -0.5": (-0.50000006, -1),
    "32766.5": (32766.5, 32767), "32767.5": (32767.5, 32767), "-32768.5": (-32768.5, -32768),
    "+inf": (np.inf, 32767), "-inf": (-np.inf, -32768), "-0.0": (-0.0, 0), "1e30": (1e30, 32767), "a denormal": (DENORMAL, 0),
}


@pytest.mark.parametrize("name", sorted(POINTS))
def test_debug_levels_at_a_decision_point(name):
    value, q = POINTS[name]
    y = np.array([value], np.float32)
    want = lm.record(y)
    assert want == {"samples": 1, "energy": q * q, "nan": 0, "peak": np.abs(y[0])}, "the model itself, at " + name
    got = lib_record(y)
    assert lm.same(got, want), "%s: library %r, model %r" % (name, got, want)
    assert np.signbit(got["peak"]) == 0


def test_debug_levels_of_a_nan_counts_it_and_nothing_else():
    for y in (np.array([np.nan], np.float32), np.array([3.0, np.nan, -7.25, np.nan], np.float32)):
        want = lm.record(y)
        assert want["nan"] == int(np.isnan(y).sum()) and want["samples"] == y.size
        assert lm.same(lib_record(y), want)
    assert lm.same(lm.record(np.array([3.0, np.nan, -7.25, np.nan], np.float32)), {"samples": 4, "energy": 9 + 49, "nan": 2, "peak": np.float32(7.25)})


@pytest.mark.parametrize("amplitude", (3.0, 40000.0))
def test_debug_levels_equals_the_model_over_random_floats(amplitude):
    y = (np.random.default_rng(int(amplitude)).uniform(-amplitude, amplitude, 10000)).astype(np.float32)
    want = lm.record(y)
    assert want["energy"] > 0 and want["nan"] == 0
    if amplitude > 32768:
        assert (np.abs(y) > 32768).mean() > 0.1, "the rails decide nothing here"
    got = lib_record(y)
    assert lm.same(got, want), (got, want)


def test_debug_levels_accumulates_into_its_record():
    rng = np.random.default_rng(11)
    a, b = (rng.uniform(-900, 900, 777)).astype(np.float32), (rng.uniform(-20000, 20000, 1234)).astype(np.float32)
    b[5] = np.nan
    rec = speexhip.debug_levels(a)
    rec = speexhip.debug_levels(b, into=rec)
    assert lm.same(lm.of_struct(rec[0]), lm.record(np.concatenate([a, b])))


def test_all_points_at_once_and_in_any_order():
    y = np.array([v for v, _ in POINTS.values()] + [np.nan], np.float32)
    want = lm.record(y)
    assert want["nan"] == 1 and np.isinf(want["peak"]) and want["energy"] == sum(q * q for _, q in POINTS.values())
    assert lm.same(lib_record(y), want) and lm.same(lib_record(y[::-1]), want)


# ---- planted defects ----------------------------------------------------------------------------------------------------
def defect_inputs():
    """per defect: (the stated input, the record() arguments that go with it, the fields that must change)"""
    rng = np.random.default_rng(6464)
    noise = rng.uniform(-3.0, 3.0, 4000).astype(np.float32)
    ties = (np.arange(-50, 50, dtype=np.float32) + np.float32(0.5))                 # every tie: half of them go the other way
    excursion = np.concatenate([rng.uniform(-100, 100, 500), [-20000.0]]).astype(np.float32)
    loud = np.full(5000, 32767.0, np.float32)         # 32767^2 has 30 significant bits: float32 holds neither it nor the sums
    holes = noise.copy()
    holes[::97] = np.nan
    return {
        "truncate": (noise, {}, ("energy",)),
        "half_even": (ties, {}, ("energy",)),
        "post_gain": (noise, {"gain": np.float32(0.25)}, ("energy", "peak")),
        "padded": (noise, {"padded": noise.size + 960}, ("samples",)),
        "signed_peak": (excursion, {}, ("peak",)),
        "fp32_energy": (loud, {}, ("energy",)),
        "nan_as_zero_sample": (holes, {}, ("nan",)),
    }


def test_every_defect_changes_the_models_record_on_its_stated_input():
    inputs = defect_inputs()
    assert tuple(inputs) == lm.DEFECTS
    for defect, (y, kwargs, fields) in inputs.items():
        right, wrong = lm.record(y), lm.record(y, defect=defect, **kwargs)
        assert lm.same(lib_record(y), right), "the library is not the rule on the input of " + defect
        assert lm.changed(wrong, right) == fields, (defect, lm.changed(wrong, right))
        if defect in ("truncate", "half_even"):
            share = (lm.steps(y, defect) != lm.steps(y)).mean()
        elif defect == "post_gain":
            share = (lm.steps(y * kwargs["gain"]) != lm.steps(y)).mean()
        elif defect == "nan_as_zero_sample":
            share = np.isnan(y).mean()
        else:
            share = None
        print("%-20s: %-16s change; energy %d -> %d%s" % (defect, ", ".join(fields), right["energy"], wrong["energy"],
              "" if share is None else "; %.1f %% of the samples' steps differ" % (100 * share)))
        if share is not None:
            assert share >= 0.01, defect


def test_the_other_defects_do_not_show_where_they_cannot():
    # whole numbers inside the rails, no NaN, a positive peak: only a different sample count or a gain can tell
    y = np.arange(1, 200, dtype=np.float32)
    for defect in ("truncate", "half_even", "signed_peak", "fp32_energy", "nan_as_zero_sample"):
        assert lm.same(lm.record(y, defect=defect), lm.record(y)), defect


# ---- RFC 6464 -----------------------------------------------------------------------------------------------------------
def test_audio_level():
    n = 48000
    square = np.where(np.arange(n) % 2 == 0, 32767.0, -32768.0).astype(np.float32)
    sine = (32767.0 * np.sin(2 * np.pi * 997.0 * np.arange(n) / 48000.0)).astype(np.float32)
    for y, want in ((square, 0), (sine, 3), (np.zeros(n, np.float32), 127), (np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32), 90)):
        rec = speexhip.debug_levels(y)[0]
        assert speexhip.audio_level(rec) == want == lm.audio_level(lm.record(y)), (speexhip.audio_level(rec), want)
    assert speexhip.audio_level({"energy": 5, "samples": 0}) == 127 and speexhip.audio_level({"energy": 0, "samples": 9}) == 127
    assert speexhip.audio_level({"energy": 1, "samples": 10 ** 9}) == 127          # (the clamp: about 180 dB down)
