"""The committed cover of the host planner's choices (tests/plan_cover.py, tests/plan_cover_cases.json) against the exact
model, per sample: one small state per case, in the default mode, judged by (a), (b) and (c) exactly as the curated
families of test_gpu_exact_model.py are.  tests/test_cpu_plan_cover.py proves without a GPU that the list, with the
curated lists, meets every (channel class or kernel kind) x (plan feature) pair the rate grid reaches, that each
schedule is big enough to be able to fail, and that the oracle alone passes on each case's own input.  Run with -s for
the per-family figures."""
from math import gcd

import pytest

import plan_cover as pc
import speexhip
import test_gpu_exact_model as xm

pytestmark = pytest.mark.gpu

DOC = pc.committed()
_ID = lambda e: "-".join(str(v) for v in e["case"])


@pytest.mark.parametrize("entry", DOC["cases"], ids=_ID)
def test_plan_cover_case(entry):
    ch, i, o, q = entry["case"]
    family, frames = pc.family_of(entry), entry["frames"]
    if entry["fast_path"] == 0:
        # the exact kernel: bytes equal to the oracle's, and the oracle inside (a)
        xm._exact_kernel(family, ch, i, o, q, frames)
    else:
        g = gcd(i, o)
        xm._one_state(family, ch, i, o, q, entry["fast_path"], sizes=pc.sizes_of(i // g, o // g, frames),
                      bound_call=pc.BOUND_CALL, seed=pc.SEED)
    xm._report(family)


@pytest.mark.parametrize("entry", DOC["batches"], ids=_ID)
def test_plan_cover_batch(entry):
    """the launch pairs no one-state call reaches: 32 streams that fill the chip"""
    ch, i, o, q = entry["case"]
    g = gcd(i, o)
    shapes = [speexhip.debug_launch_shape(i // g, o // g, q, ch, entry["streams"], entry["frames"], fl) for fl in (False, True)]
    for pair in entry["pairs"]:
        family, cls, feature, value = pair
        assert (family, cls) == ("launch", pc.channel_class(ch)) and feature in ("touch", "pp", "w16"), pair
        key = {"touch": "touch", "pp": "phase_pairs", "w16": "int16_window"}[feature]
        assert any(s[key] == value for s in shapes), (entry["case"], pair, shapes)
    xm._batch("cover batch", ch, i, o, q, entry["streams"], entry["frames"], entry["fast_path"])
    xm._report("cover batch")
