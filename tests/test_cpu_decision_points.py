"""CPU checks of tests/decision_points.py, for every filter, format and dither kind test_gpu_decision_points.py uses:
the crafted streams make what they plan (the oracle's float output and exact_model.chain32's contract equal the target
at every planned output), the classes straddle what they claim under the numpy models, the library's host compile of the
encoders agrees with the models on the crafted streams, and every planted defect -- planted in the model, never in the
library -- changes bytes of the crafted streams' expected output.  Run with -s for the planted-defect table: bytes
changed on the crafted stream next to bytes changed on the FIR of 20 000 frames of noise."""
import numpy as np
import pytest

import decision_points as dp
import dither_model as dm
import exact_model as em
import g711_model as gm
import halfbe_model as hm
import oracle as orc
import sample_formats as sf
import speexhip
from test_gpu_formats import storage_of

CFGS = [f[0] for f in dp.FILTERS]
CFG_IDS = ["%dch-%d-%d-q%d" % c for c in CFGS]
KINDS = (dm.NONE,) + tuple(dm.KINDS)
_Y = {}


def wcap(frames, fi, fo):
    return int(np.ceil(frames * fo / fi)) + 8


def outputs(cfg):
    """[(x, plan, y)] of a filter: y = the oracle's float output of the crafted stream -- on the interpolating filter
    with the planned outputs replaced by exact_model.chain32's, the fast kernels' contract there"""
    if cfg not in _Y:
        ch, fi, fo, q = cfg
        model, parts = dp.crafted(cfg)
        out = []
        for x, plan in parts:
            y, used = orc.Oracle(ch, fi, fo, q).process_float(x, wcap(x.shape[0], fi, fo))
            assert used == x.shape[0]
            ks, cs = np.array([p[1] for p in plan]), np.array([p[2] for p in plan])
            if not model.kind.startswith("direct"):
                y = y.copy()
                y[ks, cs] = dp.chain32_at(model, x, ks, cs)
            out.append((x, plan, y))
        _Y[cfg] = out
    return _Y[cfg]


def same_bits(a, b):
    return np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)


# ---- 1. the crafting condition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_crafted_streams_make_what_they_plan(cfg):
    ch, fi, fo, q = cfg
    model, parts = dp.crafted(cfg)
    wanted = dp.wanted_for()
    asked, made, missed = dp.counts([(w[0], 0, 0, 0) for w in wanted]), {}, {}
    for x, plan, y in outputs(cfg):
        assert x.shape[0] <= dp.MAX_FRAMES and x.dtype == np.float32
        nz = x[x != 0]
        assert np.isfinite(nz).all() and (np.abs(nz) >= np.float32(2.0 ** -126)).all() and nz.size == len(plan)
        at = np.sort(np.nonzero(x.any(axis=1))[0])
        assert np.diff(at).min() >= model.taps + 3
        ks, cs = np.array([p[1] for p in plan]), np.array([p[2] for p in plan])
        tg = np.array([p[3] for p in plan], np.float32)
        assert ks.max() < y.shape[0]
        # the oracle's own loops on the direct kinds (exact mode's values too), the fp32 chain on every kind
        if model.kind.startswith("direct"):
            assert same_bits(y[ks, cs], tg).all(), "the oracle's float output is not the target at a planned output"
        assert same_bits(dp.chain32_at(model, x, ks, cs), tg).all()
        for label, n in dp.counts(plan).items():
            made[label] = made.get(label, 0) + n
        for label, _ in plan.missed:
            missed[label] = missed.get(label, 0) + 1
    assert sum(made.values()) + sum(missed.values()) == len(wanted)
    for label, n in asked.items():
        if label[2] in dp.SINGLE:
            assert made.get(label, 0) == n, ("every one of a few-valued class is made", label, made.get(label, 0), n)
        else:
            assert missed.get(label, 0) <= 0.02 * n, (label, missed.get(label, 0), n)
    print("%s: %d targets in %d stream(s) of %s frames, %d not made" % (
        cfg, len(wanted), len(parts), [p[0].shape[0] for p in parts], sum(missed.values())))


def test_chain32_at_is_chain32_at_the_chosen_outputs():
    cfg = (2, 44100, 48000, 7)
    model = em.Model(*cfg)
    x, plan = dp.craft(model, 2, dp.wanted_for((sf.S16, hm.F16N), ())[:60], dp.START * 2)
    n_out = max(p[1] for p in plan) + 1
    full = em.chain32(model, x, n_out)
    ks, cs = np.array([p[1] for p in plan]), np.array([p[2] for p in plan])
    assert same_bits(full[ks, cs], dp.chain32_at(model, x, ks, cs)).all()
    assert same_bits(full[ks, cs], [p[3] for p in plan]).all()


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_every_class_lies_in_whole_tiles_of_an_aligned_pass(cfg):
    """what the GPU file asserts of its device routes, from the plan alone: an aligned call takes the 16-bytes-per-lane
    path on whole tiles and holds every class there; the call offset by one sample takes the element path on all of it"""
    ch = cfg[0]
    classes = set(w[0] for w in dp.wanted_for())
    seen = {"convert": set(), "sides": set()}
    for x, plan, y in outputs(cfg):
        made = y.shape[0]
        for name, kw in (("convert", dict(tile_samples=dp.CONVERT_TILE)), ("sides", dict(tile_frames=dp.SIDES_TILE))):
            seen[name] |= set(dp.counts(plan, dp.in_whole_tiles(plan, ch, made, **kw)))
    for name in seen:
        assert seen[name] == classes, (name, classes - seen[name])


# ---- 2. the classes straddle what they claim ---------------------------------------------------------------------------
def code_of(fmt, y, d=None):
    """the model's bytes of single values: one row of bytes per value"""
    y = np.asarray(y, np.float32).reshape(-1)
    st = hm.from_internal(fmt, y) if d is None else hm.quantise(fmt, y, d)
    return hm.raw(fmt, st).reshape(y.size, -1)


def differ(a, b):
    return (a != b).any(axis=1)


FAMILY_FMT = {hm.name(f): f for f in hm.ALL}


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_classes_straddle_what_they_claim(cfg):
    ch = cfg[0]
    checked = {}
    for x, plan, y in outputs(cfg):
        by = {}
        for label, k, c, t in plan:
            by.setdefault(label, []).append((k, c, t))
        for (fam, kind, name), pts in by.items():
            if fam == "all":
                continue
            fmt = FAMILY_FMT[fam]
            t = np.array([p[2] for p in pts], np.float32)
            lo, hi = dp.below(t), dp.above(t)
            what = (cfg, fam, kind, name)
            if kind != "none":
                knd = dm.RECTANGULAR if kind == "rectangular" else dm.TRIANGULAR
                d = np.array([dm.values(knd, dp.SEEDS[knd], dp.START * ch + k * ch + c, 1)[0] for k, c, _ in pts])
                other = hi if name == "bracket_lo" else lo
                assert differ(code_of(fmt, t, d), code_of(fmt, other, d)).all(), what
            elif name in ("tie", "boundary_hi"):            # half-up: the tie goes up, its lower neighbour does not
                assert differ(code_of(fmt, t), code_of(fmt, lo)).all(), what
                assert not differ(code_of(fmt, t), code_of(fmt, hi)).any() or fam == "s32", what
            elif name in ("below_tie", "boundary_lo"):
                assert differ(code_of(fmt, t), code_of(fmt, hi)).all(), what
            elif name in ("tie_even", "tie_odd", "carry", "z_subnormal_tie"):
                # a tie of round-to-nearest-even separates its neighbours and goes with one of them: the one towards
                # zero when the kept mantissa is even, the other when it is odd
                a, b, m = code_of(fmt, lo), code_of(fmt, hi), code_of(fmt, t)
                assert differ(a, b).all(), what
                inner = np.where(t > 0, lo, hi)
                with_inner = ~differ(m, code_of(fmt, inner))
                if name == "tie_even":
                    assert with_inner.all(), what
                elif name in ("tie_odd", "carry"):
                    assert not with_inner.any(), what
                else:
                    assert with_inner.any() and not with_inner.all(), what
            elif name in ("rail_in", "rail_at", "rail_out"):
                st = dp.stage(fmt)
                scale, q_lo, q_hi = dp.INT_RULE[st]
                q = dp.halfup_of(st, t)
                inside = (q >= q_lo) & (q <= q_hi)
                if name == "rail_in":
                    # (s32: float32 steps by 128 at the top -- the last value inside is 2^31 - 128)
                    assert inside.all() and ((q == q_lo) | (q == q_hi) | (fam == "s32")).all(), what
                elif name == "rail_out":
                    assert not inside.any() and ((q == q_lo - 1) | (q == q_hi + 1) | (fam == "s32")).all(), what
                else:                                       # half-up: the top tie is out, the bottom one in
                    assert (inside == (t < 0)).all(), what
                rails = code_of(fmt, np.float32([-1e30, 1e30]))
                at_rail = np.isin(np.clip(q, q_lo, q_hi), (q_lo, q_hi))      # (a saturating encoder: one code for all three)
                assert not differ(code_of(fmt, t), rails[(t > 0).astype(int)])[at_rail].any() and at_rail.sum() >= 1, what
            elif name == "min_sub":
                assert hm.from_internal(fmt, t).view(np.uint16).tolist() == [0x0000, 0x0001, 0x0002], what
            elif name == "overflow":
                assert hm.from_internal(fmt, t).view(np.uint16).tolist() == [0x7C00, 0x7BFF, 0x7BFF], what
            elif name == "z_subnormal":
                z = t.astype(np.float64) / 32768.0
                assert ((np.abs(z) < 2.0 ** -126) & (np.abs(t) >= np.float32(2.0 ** -126))).all(), what
            else:
                continue
            checked[(fam, kind, name)] = checked.get((fam, kind, name), 0) + len(pts)
    names = set(k[2] for k in checked)
    assert {"tie", "below_tie", "boundary_hi", "boundary_lo", "bracket_lo", "bracket_hi", "tie_even", "tie_odd", "carry",
            "z_subnormal_tie", "rail_in", "rail_at", "rail_out", "min_sub", "overflow", "z_subnormal"} <= names
    # the one output where the two orders of the dithered sum part
    pin = [p for _, plan, _ in outputs(cfg) for p in plan if p[0][2] == "reassoc"]
    assert len(pin) == 1
    _, k, c, t = pin[0]
    d = dm.values(dm.TRIANGULAR, dp.SEEDS[dm.TRIANGULAR], dp.START * ch + k * ch + c, 1)
    assert d[0] == -0.5 and dm.quantise(sf.S16, [t], d)[0] == 0 and np.floor(float(t) + (d[0] + 0.5)) == -1


# ---- 3. the host compile of the encoders ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_host_hooks_agree_with_the_models_on_the_crafted_streams(cfg):
    """speexhip_debug_format_encode (the five half-float and big-endian formats) and speexhip_debug_g711_encode, without
    dither and with both kinds at the GPU tests' seeds and position.  U8, S16, S24 and S32 have no host compile:
    format_device.h's statement of them runs on the device alone."""
    ch = cfg[0]
    for x, plan, y in outputs(cfg):
        flat = y.reshape(-1)
        for fmt in hm.NEW + gm.COMPANDED:
            hook = speexhip.debug_g711_encode if fmt in gm.COMPANDED else speexhip.debug_format_encode
            with np.errstate(all="ignore"):
                assert hm.raw(fmt, hook(fmt, flat)).tobytes() == hm.raw(fmt, hm.from_internal(fmt, flat)).tobytes(), hm.name(fmt)
            if not hm.dithered(fmt):
                continue
            for kind in dm.KINDS:
                d = speexhip.debug_dither(kind, dp.SEEDS[kind], (dp.START * ch) & dm.M64, flat.size)
                want = hm.from_internal_dither(fmt, flat, kind, dp.SEEDS[kind], dp.START, ch)
                assert hm.raw(fmt, hook(fmt, flat, d)).tobytes() == hm.raw(fmt, want).tobytes(), (hm.name(fmt), kind)


def test_encode_without_a_defect_is_the_models():
    cfg = CFGS[0]
    ch = cfg[0]
    y = outputs(cfg)[0][2].reshape(-1)
    for fmt in hm.ALL:
        for kind in KINDS:
            with np.errstate(all="ignore"):
                want = hm.from_internal_dither(fmt, y, kind, dp.SEEDS.get(kind, 0), dp.START, ch)
                got = dp.encode(fmt, y, kind, dp.SEEDS.get(kind, 0), dp.START, ch)
            assert got.tobytes() == hm.raw(fmt, want).tobytes(), (hm.name(fmt), kind)


# ---- 4. planted defects ----------------------------------------------------------------------------------------------------
def noise_output():
    """the float twin's output test_gpu_halfbe feeds its encoders: the FIR of 20 000 frames of full-scale noise"""
    ch, fi, fo, q = 2, 44100, 48000, 7
    x = sf.to_internal(sf.F32, storage_of(sf.F32, 20000 * ch, 31 * ch + q)).reshape(-1, ch)
    y, _ = orc.Oracle(ch, fi, fo, q).process_float(x, wcap(20000, fi, fo))
    return y.reshape(-1), ch


def changed(fmt, y, kind, ch, defect):
    seed = dp.SEEDS.get(kind, 0)
    with np.errstate(all="ignore"):
        a = dp.encode(fmt, y, kind, seed, dp.START, ch)
        b = dp.encode(fmt, y, kind, seed, dp.START, ch, defect=defect)
    return int((a != b).sum())


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_every_planted_defect_changes_the_crafted_streams_bytes(cfg):
    ch = cfg[0]
    noise, noise_ch = noise_output()
    ys = [y.reshape(-1) for _, _, y in outputs(cfg)]
    print("\n%s: bytes changed by a defect planted in the model -- crafted stream | 20 000 frames of noise" % (cfg,))
    for defect in dp.DEFECTS:
        fams, kind = dp.DEFECT_SCOPE[defect]
        for fmt in fams:
            on_crafted = sum(changed(fmt, y, kind, ch, defect) for y in ys)
            on_noise = changed(fmt, noise, kind, noise_ch, defect)
            print("  %-24s %-6s %-11s %8d | %d" % (defect, hm.name(fmt), dm.KIND_NAMES[kind], on_crafted, on_noise))
            assert on_crafted > 0, (defect, hm.name(fmt))
