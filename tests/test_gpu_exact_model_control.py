"""Streams after mid-stream control calls against the exact value of each output sample, per SEGMENT.

test_gpu_exact_model.py and test_gpu_exact_model_float.py judge streams that start at (0, 0), keep their filter and hold
no pending frames.  Here set_rate, set_rate_frac, set_quality, skip_zeros and reset_mem come between the calls, and every
segment -- from one control call to the next -- is judged by the same checks (a), (b), (c) over the line
head ++ input from its own start (tests/exact_model.py, "Segments"; the scripts and the calls of a segment are
tests/control_scripts.py's, recorded once on the oracle).  In the default mode (no mode named), MODE_FAST and
MODE_FAST_F32:
  * after every op and every call: consumed, shapes, position, pending count, history and pending frames equal the
    oracle's; after every op fast_path and accumulate_bits equal those of a FRESH state of the same filter and mode;
  * (a) on every segment, int16 and float; (b) and (c) on every segment whose float stream makes em.BIAS_MIN_SAMPLES
    samples -- and every filter a script visits has such a segment: asserted, not assumed;
  * one segment per script makes its first calls as one coalesced call whose first chunk is shorter than the pending
    count (the fused launch's magic_used);
  * batches: streams of one launch that hold DIFFERENT pending counts, on the fast kernels, and a launch that fills the
    chip over the int16 window before and after a filter change.
Run with -s for the per-family figures: "control, one state" and "control, batch".
"""
import numpy as np
import pytest

import control_scripts as cs
import exact_model as em
import oracle as orc
import speexhip
import test_gpu_exact_model as xm

pytestmark = pytest.mark.gpu

MODES = [None, speexhip.MODE_FAST, speexhip.MODE_FAST_F32]
ONE, BATCH = "control, one state", "control, batch"


def _fresh_info(ch, seg, mode):
    r = speexhip.Resampler(ch, seg["rate"][0], seg["rate"][1], seg["quality"], mode=mode, ratio=seg["ratio"])
    info = r.info()
    r.close()
    assert (info["num_rate"], info["den_rate"], info["filt_len"]) == seg["key"][:3], (info, seg["key"])
    return info


def _same_state(r, position, head, taps, tag):
    assert r.position() == tuple(position), (tag, r.position(), position)
    assert r.info()["magic_samples"] == head.shape[0] - (taps - 1), tag
    assert np.array_equal(r.history(), head[: taps - 1]), tag
    for c in range(head.shape[1]):
        assert np.array_equal(r.pending(c), head[taps - 1:, c]), (tag, c)


def _run(name, stream, mode):
    """the script on one state over one stream -> per segment (info, [output of every call])"""
    ch, i, o, q, _ = cs.SCRIPTS[name]
    r = speexhip.Resampler(ch, i, o, q, mode=mode)
    done = []
    for seg in cs.record(name, stream):
        tag, taps = (name, stream, mode, seg["index"], seg["op"]), seg["key"][2]
        if seg["op"] is not None:
            assert cs.apply_op(r, seg["op"]) == 0, tag
        _same_state(r, seg["start"], seg["head"], taps, tag)
        info, fresh = r.info(), _fresh_info(ch, seg, mode)
        assert (info["fast_path"], info["accumulate_bits"]) == (fresh["fast_path"], fresh["accumulate_bits"]), (tag, info, fresh)
        xm._expect_bits(info, seg["model"])
        outs, calls, j = [], seg["calls"], 0
        while j < len(calls):
            c = calls[j]
            if c["group"] is None:
                y, used = (r.process_float if c["io"] == "float" else r.process)(c["x"], c["cap"])
                got, j = [(y, used)], j + 1
            else:
                group = [g for g in calls if g["group"] == c["group"]]
                ys, used = r.process_chunks([g["x"] for g in group], [g["cap"] for g in group],
                                            np.float32 if c["io"] == "float" else np.int16)
                got, j = list(zip(ys, used)), j + len(group)
            for (y, used), c in zip(got, calls[j - len(got): j]):
                assert used == c["used"] and y.shape == c["want"].shape and y.dtype == c["want"].dtype, (tag, used, y.shape)
                outs.append(y)
            # (the state is observable between calls only: after a coalesced call it is that of its last chunk)
            _same_state(r, calls[j - 1]["position"], calls[j - 1]["head"], taps, tag)
        done.append((info, outs))
    r.close()
    return done


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(cs.SCRIPTS))
def test_exact_model_control_scripts_on_one_state(name, mode):
    streams = cs.streams_of(name)
    runs = {stream: _run(name, stream, mode) for stream in streams}
    segs = cs.record(name, streams[-1])
    judged = set()
    for n, seg in enumerate(segs):
        model, label = seg["model"], "%s mode %s segment %d %s" % (name, mode, n, seg["op"])
        info, outs = runs[streams[-1]][n]
        bits = info["accumulate_bits"]
        want = [c["want"] for c in seg["calls"]]
        if name in cs.MIXED:
            # one state, int16 and float calls: the outputs of the other type masked, as _judge_mixed does; its filters
            # are single kinds, so the oracle is the yardstick
            assert not model.double_kind
            fails, stats = cs.judge(seg, outs, bits, want, xm.MARGINS.get(ONE, em.MARGIN))
            print("%s %s bits %d: %s" % (ONE, label, bits, stats))
            assert not fails, (label, fails)
            if stats and stats["judged"]:
                xm._note(ONE, stats)
                judged.add(seg["key"])
            continue
        seg16 = cs.record(name, "int16")[n]
        assert np.array_equal(seg16["fed"], seg["fed"]) and np.array_equal(seg16["head"], seg["head"]), label
        assert runs["int16"][n][0] == info
        gotf, wantf = np.concatenate(outs), np.concatenate(want)
        enough = int((cs.truth_of(seg)[1] > 0).sum()) >= em.BIAS_MIN_SAMPLES
        stats = xm._judge(ONE, label, model, bits, seg["fed"], np.concatenate(runs["int16"][n][1]), gotf, wantf,
                          statistics=enough, truth_mag=cs.truth_of(seg))
        if enough:
            assert "yard" in stats and stats["n"] >= em.BIAS_MIN_SAMPLES
            judged.add(seg["key"])
    # (b) and (c) were computed on every distinct filter the script visits
    assert judged == {seg["key"] for seg in segs}, (name, mode, {seg["key"] for seg in segs} - judged)
    xm._report(ONE)


def test_the_control_scripts_reach_every_fast_path():
    """fresh states of every judged segment's filter, default mode: the scripts meet the exact kernel (0), the period (2)
    and the slide kernel (3) and their fp64 instances (4 slide, 5 period)"""
    seen = {_fresh_info(cs.SCRIPTS[name][0], seg, None)["fast_path"]
            for name in cs.SCRIPTS for seg in cs.record(name, cs.streams_of(name)[-1]) if not seg["short"]}
    assert seen == {0, 2, 3, 4, 5}, seen


# ---- batches ----
def _batch_script(family, ch, i, o, q, S, F, mode, plan, picks, label, int16_window_step=None):
    """plan: ("op", method, args...) and ("step", [frames per stream], [capacity per stream]) in turn, on an int16 and a
    float Batch with per-stream oracles alongside; every stream of `picks` judged per segment."""
    import torch
    sp = torch.cuda.current_stream().cuda_stream
    cap = F * 2 + 64
    logs, infos = {}, {}
    for kind in ("int16", "float"):
        fl = kind == "float"
        b = speexhip.Batch(S, ch, i, o, q, mode=mode)
        refs = {s: orc.Oracle(ch, i, o, q) for s in picks}
        d_out = torch.zeros((S, cap, ch), dtype=torch.float32 if fl else torch.int16, device="cuda")
        segs = [{"info": b.info(), "rate": (i, o), "q": q,
                 "models": {s: em.Model.of(refs[s]).segment_of(refs[s]) for s in picks}, "calls": {s: [] for s in picks}}]
        step_no = 0
        for item in plan:
            if item[0] == "op":
                assert getattr(b, item[1])(*item[2:]) == 0, item
                for s in picks:
                    assert getattr(refs[s], item[1])(*item[2:]) == 0, item
                models = {}
                for s in picks:         # heads and starts per stream, from the batch, equal to the oracle's
                    inf, lines, ref = b.info(s), b.lines(s), refs[s]
                    assert (inf["last_sample"], inf["samp_frac_num"]) == ref.position(), (label, item, s)
                    assert inf["magic_samples"] == len(ref.pending()) and np.array_equal(lines, cs.head_of(ref)), (label, item, s)
                    models[s] = em.Model.of(ref).segment(lines, (inf["last_sample"], inf["samp_frac_num"]))
                ref = refs[picks[0]]
                segs.append({"info": b.info(), "rate": ref.rate(), "q": ref.quality(), "models": models,
                             "calls": {s: [] for s in picks}})
                continue
            _, lens, caps = item
            base = em.with_silence(orc.lcg_pcm(F * ch, 700 + ch + q + step_no).reshape(F, ch), segs[-1]["models"][picks[0]].taps)
            xs = np.stack([np.roll(base, 13 * s, axis=0) for s in range(S)])
            if kind == "int16" and step_no == int16_window_step:
                inf = b.info()
                shape = speexhip.debug_launch_shape(inf["num_rate"], inf["den_rate"], inf["quality"], ch, S, min(lens))
                assert shape["int16_window"], (label, shape)
            d_in = torch.from_numpy(np.ascontiguousarray(xs, np.float32) if fl else xs).cuda()
            used, made = b.process_device(d_in.data_ptr(), F * ch, lens, d_out.data_ptr(), cap * ch, caps, sp, fl)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            for s in picks:
                x = xs[s, : lens[s]]
                w, wu = refs[s].process_float(x.astype(np.float32), caps[s]) if fl else refs[s].process(x, caps[s])
                assert (used[s], made[s]) == (wu, w.shape[0]), (label, kind, step_no, s)
                inf = b.info(s)
                assert (inf["last_sample"], inf["samp_frac_num"]) == refs[s].position(), (label, kind, step_no, s)
                assert inf["magic_samples"] == len(refs[s].pending()) and np.array_equal(b.lines(s), cs.head_of(refs[s]))
                segs[-1]["calls"][s].append((out[s, : made[s]].copy(), w, x[:wu].astype(np.float32)))
            step_no += 1
        b.close()
        logs[kind] = segs
    judged = set()
    for n, (seg16, segf) in enumerate(zip(logs["int16"], logs["float"])):
        info = segf["info"]
        assert seg16["info"] == info
        fresh = speexhip.Batch(S, ch, segf["rate"][0], segf["rate"][1], segf["q"], mode=mode)
        want = fresh.info()
        fresh.close()
        assert all(info[k] == want[k] for k in ("num_rate", "den_rate", "filt_len", "fast_path", "accumulate_bits")), (label, n, info, want)
        key = (info["num_rate"], info["den_rate"], info["filt_len"], info["quality"])
        for s in picks:
            model = segf["models"][s]
            assert np.array_equal(seg16["models"][s].head, model.head) and seg16["models"][s].last0 == model.last0
            if not segf["calls"][s]:
                continue
            got16, _, fed16 = (np.concatenate(v) for v in zip(*seg16["calls"][s]))
            gotf, wantf, fed = (np.concatenate(v) for v in zip(*segf["calls"][s]))
            assert np.array_equal(fed16, fed)
            bits = xm._expect_bits(info, model)
            truth_mag = model.truth(fed, gotf.shape[0])
            enough = int((truth_mag[1] > 0).sum()) >= em.BIAS_MIN_SAMPLES
            stats = xm._judge(family, "%s segment %d stream %d" % (label, n, s), model, bits, fed, got16, gotf, wantf,
                              statistics=enough, truth_mag=truth_mag)
            if enough:
                assert "yard" in stats
                judged.add(key)
        assert key in judged, (label, "segment", n, "no stream long enough for (b) and (c)")
    xm._report(family)


@pytest.mark.parametrize("mode", MODES)
def test_exact_model_control_small_batch_with_ragged_pending_counts(mode):
    """test_gpu_parity.test_batch_mid_stream_quality_change_with_ragged_streams' steps (there: MODE_EXACT, bit for bit) on the
    fast kernels: the [3, 0, 50, 50] step leaves every stream of the next launch another pending count."""
    F, S = 25000, 4
    full, big = [F, F - 997, F - 2 * 997, F - 3 * 997], [2 * F] * 4
    plan = [("step", [6000, 5000, 300, 0], [8000, 100, 8000, 8000]), ("step", full, big),
            ("op", "set_quality", 3), ("step", [40, 40, 40, 40], [3, 0, 50, 50]), ("step", full, big),
            ("op", "set_quality", 10), ("step", [3000, 10, 3000, 1], big), ("step", full, big),
            ("op", "set_rate_frac", 3, 2, 48000, 32000), ("step", [3000, 3000, 3000, 3000], [8000, 8000, 5, 8000]), ("step", full, big),
            ("op", "skip_zeros"), ("step", full, big), ("op", "reset_mem"), ("step", full, big)]
    _batch_script(BATCH, 2, 44100, 48000, 8, S, F, mode, plan, list(range(S)), "small batch mode %s" % mode)


def test_exact_model_control_batch_that_fills_the_chip():
    """xm.BATCHES' (2, 48000 -> 11025, q7, 32 streams) at 65 536 frames: the int16 window before a filter change, the fp64
    kernel after it, and back to a period ratio through set_rate_frac"""
    ch, i, o, q, S, F = 2, 48000, 11025, 7, 32, 65536
    assert (ch, i, o, q, S) in [row[:5] for row in xm.BATCHES]
    ragged = [F - 997 * (s % 7) for s in range(S)]
    plan = [("step", ragged, [F] * S), ("op", "set_quality", 10), ("step", ragged[3:] + ragged[:3], [F] * S),
            ("op", "set_rate_frac", 160, 147, 48000, 44100), ("step", [F] * S, [2 * F] * S)]
    _batch_script(BATCH, ch, i, o, q, S, F, None, plan, [0, S // 2, S - 1], "32 streams", int16_window_step=0)
