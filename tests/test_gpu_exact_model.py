"""Every kernel family against the EXACT value of each output sample (tests/exact_model.py), per sample.

test_gpu_parity.py pins "+-1 LSB of the reference" -- the north-star contract, with bars as wide as the reference's own
fp32 error makes them.  This file pins "as accurate as the reference against the truth": with u = 2^-24 and
e = (got - truth) / (u mag),
  (a) every sample inside the textbook bound of its instance (fp32 chain: (taps + 2) u mag + 1/2 ulp; fp64 accumulate:
      the correctly rounded float32 unless the truth sits on a midpoint; int16: the interval of the same bound, rounded
      half-up and saturated),
  (b) on float calls rms(e) <= MARGIN x the yardstick's on the same input -- the oracle on the single kinds, chain32 (the
      documented fp32 chain) for fp32 instances of the double kinds, and 1.0 x the oracle for fp64 instances,
  (c) no bias: |mean e| <= 5 rms(e) / sqrt(n) wherever n >= 20 000.
Each case runs one int16 and one float stream (the same int16-valued samples, as tools/num_check.py does) of ragged calls
with a 1-frame and an empty call; the long call carries a stretch of silence longer than the filter, where single edge
taps decide whole samples.  The case lists are test_gpu_parity.py's.  Run with -s for the per-family figures.
test_gpu_exact_model_float.py runs the same lists with real float data on the float stream (the sample-maker argument of
_one_state and _batch).
"""
import os
from math import gcd

import numpy as np
import pytest

import exact_model as em
import oracle as orc
import speexhip
import test_gpu_parity as par

pytestmark = pytest.mark.gpu

BIG = 1 << 20
# (b): margins other than em.MARGIN = 1.5, by family, each with its measurement and the reason.  None so far.
MARGINS = {}

_FIGURES = {}


def _note(family, stats, differing=None):
    f = _FIGURES.setdefault(family, {"cases": 0, "rms": 0.0, "ratio": 0.0, "max": 0.0, "z": 0.0, "int16": 0.0})
    if stats is not None:
        f["cases"] += 1
        f["rms"], f["max"], f["z"] = max(f["rms"], stats["rms"]), max(f["max"], stats["max"]), max(f["z"], abs(stats["z"]))
        if stats.get("yard"):
            f["ratio"] = max(f["ratio"], stats["rms"] / stats["yard"])
    if differing is not None:
        f["int16"] = max(f["int16"], differing)


def _report(family):
    f = _FIGURES.get(family)
    if f:
        print("\n[exact model] %-28s %3d float comparisons: worst rms(e) %.3f (%.2f x yardstick), max|e| %.2f, bias %.1f sigma; "
              "int16 samples off halfup(truth) <= %.2e" % (family, f["cases"], f["rms"], f["ratio"], f["max"], f["z"], f["int16"]))


_samples = em.samples


def _judge(family, name, model, bits, fed, got16, gotf, wantf, fedf=None, underflow=False, statistics=True,
           truth_mag=None):
    """(a) on the int16 stream, (a) (b) (c) on the float stream.  Both streams consumed the same samples `fed`, unless the
    float stream had a sample maker of its own: `fedf` is what it consumed then (got16 None: there was no int16 stream).
    underflow: the float stream is judged by (a) alone, with the bounds' underflow term (float_inputs kind D).
    statistics False: (a) alone, with no yardstick and no figures noted (a segment of a few samples, whose rms says
    nothing).  truth_mag: model.truth(fed, outputs) where the caller has it already.  -> the float comparison's stats ("yard" in them: (b) was judged)."""
    fails, differing = [], None
    if got16 is not None:
        assert got16.shape == gotf.shape, (name, got16.shape, gotf.shape)
        truth, mag = truth_mag or model.truth(fed, got16.shape[0])
        fails = ["int16 (a) " + m for m in em.hard_int16(model, fed, got16, truth, mag, bits, tile=model.num)]
        differing = float((got16.astype(np.int64) != em.halfup(truth)).mean()) if got16.size else 0.0
    if fedf is None:
        fedf = fed
    else:
        truth, mag = model.truth(fedf, gotf.shape[0])
    if underflow or not statistics:
        yard, margin = None, em.MARGIN
    elif bits == 64:
        yard, margin = wantf, 1.0           # no worse than the reference's double kernels
    elif model.double_kind:
        yard, margin = em.chain32(model, fedf, gotf.shape[0]), MARGINS.get(family, em.MARGIN)
    else:
        yard, margin = wantf, MARGINS.get(family, em.MARGIN)
    ffails, stats = em.judge_float(model, fedf, gotf, truth, mag, bits, yard, margin, tile=model.num, underflow=underflow)
    _note(family, None if underflow or not statistics else stats, differing)
    print("%s %s bits %d: n %d rms(e) %.3f yardstick %.3f max|e| %.2f bias %.1f sigma%s%s" % (
        family, name, bits, stats["n"], stats["rms"], stats.get("yard", 0.0), stats["max"], stats["z"],
        "" if differing is None else ", int16 off halfup(truth) %.2e" % differing,
        " ((a) alone, with the underflow term)" if underflow else ""))
    assert not fails + ffails, (family, name, fails + ffails)
    return stats


def _expect_bits(info, model):
    bits = info["accumulate_bits"]
    assert bits == (64 if info["fast_path"] in (4, 5) or (info["fast_path"] == 0 and model.double_kind) else 32), info
    return bits


def _one_state(family, ch, i, o, q, fast_path, sizes=(1, 21011, 0, 9000), mode=None, bound_call=None, seed=40,
               float_samples=None, streams=("int16", "float"), underflow=False, label=""):
    """One int16 and one float stream of `sizes` frames per call through two states of one filter.  float_samples(frames,
    ch, seed, taps) makes the float stream's samples (default: the int16 stream's own, as float32)."""
    model = em.Model(ch, i, o, q)
    name = "%s mode %s%s" % ((ch, i, o, q), mode, label)
    outs = {}
    for kind in streams:
        r, ref = speexhip.Resampler(ch, i, o, q, mode=mode), orc.Oracle(ch, i, o, q)
        info = r.info()
        assert info["fast_path"] == fast_path, (name, info["fast_path"])
        bits = _expect_bits(info, model)
        got, want, fed = [], [], []
        for call, frames in enumerate(sizes):
            x = _samples(frames, ch, seed + 7 * call + ch, model.taps, tone=call == 3)
            cap = max(1, frames * o // i // 2) if call == bound_call else BIG
            if kind == "float":
                if float_samples is not None:
                    x = float_samples(frames, ch, seed + 7 * call + ch, model.taps)
                y, u = r.process_float(x.astype(np.float32), cap)
                w, wu = ref.process_float(x.astype(np.float32), cap)
            else:
                y, u = r.process(x, cap)
                w, wu = ref.process(x, cap)
            assert u == wu and y.shape == w.shape and r.position() == ref.position(), (name, kind, call)
            # (a capacity-bound call may end between two outputs of one input frame: the stream has read that frame
            #  and not consumed it.  After the last call nothing else takes its place: it belongs to the line.)
            got.append(y), want.append(w), fed.append(x[: u + 1] if call == len(sizes) - 1 else x[:u])
        outs[kind] = (np.concatenate(got), np.concatenate(want), np.concatenate(fed))
        r.close()
    if float_samples is None:
        assert np.array_equal(outs["int16"][2], outs["float"][2]), name
        _judge(family, name, model, bits, outs["int16"][2], outs["int16"][0], outs["float"][0], outs["float"][1])
    else:
        i16 = outs.get("int16", (None, None, None))
        _judge(family, name, model, bits, i16[2], i16[0], outs["float"][0], outs["float"][1], fedf=outs["float"][2],
               underflow=underflow)
    return outs


def _batch(family, ch, i, o, q, S, F, fast_path, mode=None, picks=None, int16_window=None, float_samples=None,
           streams=("int16", "float"), underflow=False, label=""):
    """S streams x two ragged calls through Batch.process_device, int16 and float; three streams judged.
    float_samples: as _one_state's."""
    import torch
    model = em.Model(ch, i, o, q)
    name = "%s x %d streams x %d%s" % ((ch, i, o, q), S, F, label)
    if int16_window is not None:
        g = gcd(i, o)
        shape = speexhip.debug_launch_shape(i // g, o // g, q, ch, S, F)
        assert shape["int16_window"] == int16_window, (name, shape)
    picks = sorted(set(picks or (0, S // 2, S - 1)))
    base = em.with_silence(orc.lcg_pcm(F * ch, 700 + ch + q).reshape(F, ch), model.taps)
    xs = np.stack([np.roll(base, 13 * s, axis=0) for s in range(S)])
    xsf = None
    if float_samples is not None:
        basef = float_samples(F, ch, 700 + ch + q, model.taps)
        xsf = np.stack([np.roll(basef, 13 * s, axis=0) for s in range(S)])
    cap = F * o // i + 64
    sp = torch.cuda.current_stream().cuda_stream
    outs = {}
    for kind in streams:
        fl = kind == "float"
        if fl and xsf is not None:
            xs = xsf
        b = speexhip.Batch(S, ch, i, o, q, mode=mode)
        info = b.info()
        assert info["fast_path"] == fast_path, (name, info["fast_path"])
        bits = _expect_bits(info, model)
        d_in = torch.from_numpy(np.ascontiguousarray(xs, np.float32) if fl else xs).cuda()
        d_out = torch.zeros((S, cap, ch), dtype=torch.float32 if fl else torch.int16, device="cuda")
        refs = {s: orc.Oracle(ch, i, o, q) for s in picks}
        acc = {s: ([], [], []) for s in picks}
        for call in range(2):
            lens = [F - 997 * (s % 7) - call for s in range(S)] if call == 0 else [F // 2 + 13 * s for s in range(S)]
            used, made = b.process_device(d_in.data_ptr(), F * ch, lens, d_out.data_ptr(), cap * ch, cap, sp, fl)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            for s in picks:
                x = xs[s, : lens[s]]
                w, wu = refs[s].process_float(x.astype(np.float32), cap) if fl else refs[s].process(x, cap)
                assert (used[s], made[s]) == (wu, w.shape[0]), (name, kind, call, s)
                acc[s][0].append(out[s, : made[s]].copy()), acc[s][1].append(w), acc[s][2].append(x[:wu])
        outs[kind] = {s: tuple(np.concatenate(v) for v in acc[s]) for s in picks}
        b.close()
    for s in picks:
        if float_samples is not None:
            i16 = outs["int16"][s] if "int16" in outs else (None, None, None)
            _judge(family, "%s stream %d" % (name, s), model, bits, i16[2], i16[0], outs["float"][s][0], outs["float"][s][1],
                   fedf=outs["float"][s][2], underflow=underflow)
            continue
        assert np.array_equal(outs["int16"][s][2], outs["float"][s][2])
        _judge(family, "%s stream %d" % (name, s), model, bits, outs["int16"][s][2], outs["int16"][s][0], outs["float"][s][0],
               outs["float"][s][1])


def test_exact_model_slide_shapes():
    for (ch, i, o, q) in par.SLIDE_CASES:
        _one_state("slide", ch, i, o, q, 4 if q >= 9 else 3, bound_call=3)
    _report("slide")


def test_exact_model_n_to_one_decimators():
    for (ch, i, o, q) in par.N_TO_ONE_CASES:
        _one_state("slide n:1", ch, i, o, q, 4 if q >= 9 else 3, sizes=(1, 40011, 0, 24000))
    _report("slide n:1")


def test_exact_model_fp64_slide_shapes():
    for n, (i, o) in enumerate(par._SLIDE64_RATIOS):
        for ch in (1, 2, 3):
            folded = (i, o) in ((56000, 16000), (72000, 16000)) and ch == 2
            _one_state("slide fp64", ch, i, o, 10 if (n + ch) % 2 else 9, 5 if folded else 4, bound_call=3)
    _report("slide fp64")


def test_exact_model_period_layouts():
    for (ch, i, o, q) in par.LAYOUT_CASES:
        _one_state("period", ch, i, o, q, 5 if q >= 9 and ch in (1, 2, 4, 6, 8) else 2, sizes=(3, 30011, 0, 21234))
    # frames without an ISA loop on a double kind: the fp32 chain, reported as such and judged against chain32
    _one_state("period", 9, 44100, 48000, 10, 2)
    _report("period")


def test_exact_model_fp64_period_layouts():
    for (ch, i, o, q) in par.PERIOD64_CASES:
        _one_state("period fp64", ch, i, o, q, 5, sizes=(3, 30011, 0, 21234), bound_call=3)
    _report("period fp64")


def test_exact_model_folded_views():
    for (ch, i, o, q) in par.FOLDED_CASES:
        fp64 = q >= 9 and ch in (1, 2, 4, 6, 8) and i != 192000
        _one_state("folded", ch, i, o, q, 5 if fp64 else 2, sizes=(3, 50011, 0, 1, 30001))
    _report("folded")


def test_exact_model_exact_fallback():
    """192:1: no fast kernel holds the filter.  The exact kernel's output must EQUAL the oracle's, and the oracle (the
    reference's fp32-rounded products) must pass (a) with the fp32 bound."""
    for (ch, i, o, q, frames) in par.EXACT_FALLBACK_CASES:
        _exact_kernel("exact fallback", ch, i, o, q, frames)
    _report("exact fallback")


def _exact_kernel(family, ch, i, o, q, frames):
    """One int16 and one float stream of `frames` frames through the exact kernel: bytes equal to the oracle's call by
    call, and the oracle inside (a)."""
    model = em.Model(ch, i, o, q)
    for kind in ("int16", "float"):
        r, ref = speexhip.Resampler(ch, i, o, q), orc.Oracle(ch, i, o, q)
        assert r.info()["fast_path"] == 0 and r.info()["accumulate_bits"] == (64 if model.double_kind else 32)
        got, fed = [], []
        for call, n in enumerate((1, frames // 3, 0, frames - frames // 3)):
            x = _samples(n, ch, 77 + call, model.taps)
            if kind == "float":
                y, u = r.process_float(x.astype(np.float32), BIG)
                w, wu = ref.process_float(x.astype(np.float32), BIG)
            else:
                y, u = r.process(x, BIG)
                w, wu = ref.process(x, BIG)
            assert u == wu and np.array_equal(y, w), ((ch, i, o, q), kind, call)
            got.append(y), fed.append(x[:u])
        got, fed = np.concatenate(got), np.concatenate(fed)
        truth, mag = model.truth(fed, got.shape[0])
        if kind == "float":
            fails, stats = em.judge_float(model, fed, got, truth, mag, 32, None)
            _note(family, stats)
        else:
            fails = em.hard_int16(model, fed, got, truth, mag, 32)
        assert not fails, ((ch, i, o, q), kind, fails)
        r.close()


# (channels, in, out, quality, streams, frames, fast_path, int16 window expected or None = not asserted)
BATCHES = [(2, 44100, 48000, 7, 40, 200000, 2, None),      # r = 10 plan, several generations
           (2, 48000, 11025, 7, 32, 131072, 2, True),      # int16 window on a launch that fills the chip
           (4, 32000, 11025, 7, 32, 65536, 2, None),       # widest windows, shares from the generation model
           (1, 32000, 11025, 7, 32, 131072, 2, None),
           (8, 48000, 44100, 5, 32, 100000, 2, None),      # bank-padded window
           (2, 48000, 11025, 10, 32, 65536, 5, None),      # fp64 period kernel, int16 window
           (2, 44100, 48000, 10, 32, 150000, 5, None),     # fp64 period kernel, r = 10
           (1, 24000, 48000, 10, 32, 100000, 4, None),     # fp64 slide kernel
           (2, 48000, 8000, 7, 32, 100000, 3, None),       # slide kernel
           (8, 96000, 8000, 10, 24, 96000, 4, None),       # slide workgroups shrunk to the LDS
           (10, 44100, 48000, 7, 32, 100000, 2, None),     # frames of channel pairs
           (9, 48000, 11025, 7, 32, 100000, 2, True)]      # C++ loop over the int16 window


@pytest.mark.parametrize("ch,i,o,q,S,F,fast_path,w16", BATCHES)
def test_exact_model_batches_that_fill_the_chip(ch, i, o, q, S, F, fast_path, w16):
    _batch("batch", ch, i, o, q, S, F, fast_path, int16_window=w16)
    _report("batch")


# (channels, in, out, quality, streams, frames)
PHASE_PAIR_BATCHES = [(1, 44100, 8000, 7, 8, 131072), (2, 48000, 22050, 7, 8, 131072), (3, 44100, 16000, 5, 6, 100000)]


def test_exact_model_mono_phase_pair_plans_by_the_rule():
    """batches of wide-window decimators that the launch rule runs over phase pairs (period_launch_prefers_pp)"""
    for (ch, i, o, q, S, F) in PHASE_PAIR_BATCHES:
        g = gcd(i, o)
        assert speexhip.debug_launch_shape(i // g, o // g, q, ch, S, F)["phase_pairs"] or ch == 3, (ch, i, o, q)
        _batch("phase pairs", ch, i, o, q, S, F, 2)
    _report("phase pairs")


FAST_SHARES_CASES = [(2, 48000, 11025, 7, 2), (2, 44100, 8000, 5, 2), (4, 48000, 11025, 7, 2), (2, 192000, 24000, 7, 3),
                     (1, 192000, 8000, 7, 3), (1, 96000, 12000, 10, 4), (2, 48000, 11025, 10, 5), (2, 44100, 8000, 10, 5),
                     (12, 96000, 11025, 8, 2)]
FAST_F32_CASES = [(1, 24000, 48000, 10, 3), (2, 44100, 48000, 10, 2), (2, 48000, 44100, 9, 2), (1, 48000, 8000, 10, 3),
                  (2, 48000, 11025, 10, 2), (2, 16000, 48000, 9, 3)]
BASELINE_ROWS = [("cfg2", 2, 44100, 48000, 7, 2), ("cfg3", 1, 24000, 48000, 10, 4), ("cfg4", 8, 48000, 44100, 5, 2),
                 ("f3", 1, 24000, 48000, 5, 3)]


def test_exact_model_fast_mode_tap_range_shares():
    """MODE_FAST: small launches of long filters add their sums in tap-range shares (re-associated: still inside (a), and
    (b) leaves them their margin)."""
    for (ch, i, o, q, fp) in FAST_SHARES_CASES:
        _one_state("FAST shares", ch, i, o, q, fp, sizes=(3, 60011, 0, 41234), mode=speexhip.MODE_FAST)
    _report("FAST shares")


def test_exact_model_fast_f32_mode_on_the_double_kinds():
    """MODE_FAST_F32: the fp32 chain on quality 9 and 10, judged as what it says it is -- against chain32."""
    for (ch, i, o, q, fp) in FAST_F32_CASES:
        _one_state("FAST_F32", ch, i, o, q, fp, mode=speexhip.MODE_FAST_F32)
    _report("FAST_F32")


@pytest.mark.parametrize("name,ch,i,o,q,fast_path", BASELINE_ROWS)
def test_exact_model_baseline_rows_at_full_size_in_the_default_mode(name, ch, i, o, q, fast_path):
    """BASELINE.json configs[1..3] and SURVEY F3, one 2^20-frame call, NO mode named."""
    frames = 1 << 20
    model = em.Model(ch, i, o, q)
    x = orc.lcg_pcm(frames * ch, 12345).reshape(frames, ch)
    xf = x.astype(np.float32)
    cap, _ = orc.wrapper_capacity(x.size * 2, i, o, ch)
    r = speexhip.Resampler(ch, i, o, q)
    info = r.info()
    assert info["mode"] == speexhip.MODE_FAST_FIXED and info["fast_path"] == fast_path, info
    bits = _expect_bits(info, model)
    got16, used = r.process(x, cap)
    r.close()
    r = speexhip.Resampler(ch, i, o, q)
    gotf, usedf = r.process_float(xf, cap)
    r.close()
    wantf, wu = orc.Oracle(ch, i, o, q).process_float(xf, cap)
    assert used == usedf == wu
    if name == "cfg2":      # full-scale noise hits both rails: (a) judges them as the clamp of its interval
        assert got16.min() == -32768 and got16.max() == 32767
    _judge("baseline, full size", name, model, bits, x[:used], got16, gotf, wantf)
    _report("baseline, full size")


def test_exact_model_is_wired_into_the_diagnostics_children():
    """The instances only the diagnostics build can force (SPEEXHIP_W16_ALWAYS, SPEEXHIP_PP) run this file's period tests
    through the child-process tests of test_gpu_parity.py: their -k expressions must go on naming them."""
    import inspect
    for fn in (par.test_int16_window_on_small_launches_too, par.test_phase_pair_plans_for_mono_on_every_launch):
        src = inspect.getsource(fn)
        assert "exact_model_period_layouts" in src and "EXACT_MODEL_FILE" in src, fn.__name__
    # ... and the mixed int16 / float streams of test_gpu_exact_model_float.py, whose one-state entry points meet the int16
    # window nowhere else
    src = inspect.getsource(par.test_int16_window_on_small_launches_too)
    assert "exact_model_mixed_entry_points" in src and "EXACT_MODEL_FLOAT_FILE" in src
    assert par.EXACT_MODEL_FLOAT_FILE.endswith("test_gpu_exact_model_float.py") and os.path.exists(par.EXACT_MODEL_FLOAT_FILE)
    # ... and the period streams in small calls of test_gpu_exact_model_streaming.py: every start phase on the int16
    # window and on phase pairs, which small launches take in those children alone
    for fn in (par.test_int16_window_on_small_launches_too, par.test_phase_pair_plans_for_mono_on_every_launch):
        src = inspect.getsource(fn)
        assert "exact_model_streaming_period" in src and "EXACT_MODEL_STREAMING_FILE" in src, fn.__name__
    assert par.EXACT_MODEL_STREAMING_FILE.endswith("test_gpu_exact_model_streaming.py")
    assert os.path.exists(par.EXACT_MODEL_STREAMING_FILE)
    import test_gpu_exact_model_streaming as xs
    assert hasattr(xs, "test_exact_model_streaming_period") and xs.DEFAULT == speexhip.MODE_FAST_FIXED
