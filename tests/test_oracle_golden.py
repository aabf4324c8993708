"""Pin the oracle (oracle/speex_oracle.c) to the reference: every golden vector produced by
the reference itself (native C + shipped WASM, tests/golden/make_golden.py) must be reproduced
BIT-FOR-BIT by the restatement -- lengths, counters, table bits and output bytes."""
import os

import numpy as np
import pytest

import oracle as orc
from golden_util import ROOT, drive, make_input, sha1


def test_lcg_generator_matches_scalar_definition():
    s, ref = 12345, []
    for _ in range(1000):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        v = s >> 16
        ref.append(v - 65536 if v >= 32768 else v)
    assert orc.lcg_pcm(1000, 12345).tolist() == ref


def test_golden_inputs_regenerate(golden):
    for c in golden["cases"]:
        if c["frames"] <= 100000:
            assert sha1(make_input(c)) == c["input_sha1"], c["name"]


def test_oracle_reproduces_every_golden_case(golden):
    for c in golden["cases"]:
        x = make_input(c)
        assert sha1(x) == c["input_sha1"], c["name"]
        o = orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
        assert (o.num, o.den, o.taps, o.oversample, o.kind, o.table_len) == (
            c["num"], c["den"], c["taps"], c["oversample"], c["kind"], c["table_len"]), c["name"]
        assert sha1(o.table()) == c["table_sha1"], c["name"] + ": filter table bits differ"
        out, calls = drive(o, c, x)
        assert out.shape[0] == c["out_frames"], c["name"]
        assert calls[: len(c["calls"])] == c["calls"], c["name"] + ": per-call counters differ"
        assert sha1(out) == c["out_sha1"], c["name"] + ": output bytes differ"
        if "out_full" in c:
            assert out.reshape(-1).tolist() == c["out_full"], c["name"]
        assert out[:8].reshape(-1).tolist() == c["head"] and out[-8:].reshape(-1).tolist() == c["tail"]


def test_oracle_bookkeeping_matches_planner_goldens(golden):
    for p in golden["planner"]:
        o = orc.Oracle(1, p["in_rate"], p["out_rate"], p["quality"])
        for (f, cap, used, n_out, pos, ph) in p["calls"]:
            out, u = o.process(np.zeros((f, 1), np.int16), cap)
            assert (u, out.shape[0]) + o.position() == (used, n_out, pos, ph), (p["in_rate"], p["out_rate"])


def test_oracle_error_paths():
    for args in [(0, 44100, 48000, 7), (2, 0, 48000, 7), (2, 44100, 0, 7), (2, 44100, 48000, 11),
                 (2, 44100, 48000, -1)]:
        with pytest.raises(ValueError, match="Invalid argument."):
            orc.Oracle(*args)
    orc.Oracle(1, 8000, 8000, 0)  # quality 0 is accepted (reference resample.c:804)


def test_oracle_equals_reference_build_on_random_configs():
    """40 random configurations x 4 calls: the oracle against the reference's native C -- the digests it recorded
    (tests/golden/golden_random_configs.json, make_golden_standalone.py), and the live build too when oracle/_ref is
    there."""
    import json
    from make_golden_standalone import random_config_trials, record_digest, run_random_trial
    with open(os.path.join(ROOT, "tests", "golden", "golden_random_configs.json")) as f:
        recorded = json.load(f)["trials"]
    trials = random_config_trials()
    assert len(trials) == len(recorded) == 40
    for trial, ((ch, i, o, q, calls), want) in enumerate(zip(trials, recorded)):
        assert record_digest(run_random_trial(orc.Oracle, ch, i, o, q, calls)) == want, (trial, ch, i, o, q)
        if not orc.have_reference():
            continue
        a, r = orc.Oracle(ch, i, o, q), orc.Reference(ch, i, o, q)
        assert np.array_equal(a.table().view(np.uint32), r.table().view(np.uint32))
        for f, cap, seed in calls:
            x = orc.lcg_pcm(f * ch, seed).reshape(f, ch)
            oa, ua = a.process(x, cap)
            orr, ur = r.process(x, cap)
            assert ua == ur and np.array_equal(oa, orr) and a.position() == r.position()
            for c in range(ch):
                assert np.array_equal(a.history(c), r.history(c))


def test_oracle_on_the_reference_fixture_files(golden):
    """The reference's own resources/*.pcm: the first 64 KiB of each, stored under tests/golden/resources/, against
    the output frames and sha1 the reference's native C gives on them (golden_resources.json), for every
    configuration golden.json lists for the whole files (whose digests are from SURVEY section 4)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "golden_resources.json")) as f:
        fx = json.load(f)
    assert [{k: c[k] for k in ("file", "channels", "in_rate", "out_rate", "quality")} for c in fx["cases"]] == \
        [{k: r[k] for k in ("file", "channels", "in_rate", "out_rate", "quality")} for r in golden["resources"]]
    for r in fx["cases"]:
        raw = np.fromfile(os.path.join(ROOT, "tests", "golden", "resources", r["file"]), dtype=np.uint8)
        assert raw.size == fx["excerpt_bytes"] and sha1(raw) == fx["files"][r["file"]], r["file"]
        raw = raw[: raw.size - raw.size % (2 * r["channels"])]
        x = raw.view(np.int16).reshape(-1, r["channels"])
        assert x.shape[0] == r["in_frames"]
        spec = dict(channels=r["channels"], in_rate=r["in_rate"], out_rate=r["out_rate"], chunks="whole")
        out, _ = drive(orc.Oracle(r["channels"], r["in_rate"], r["out_rate"], r["quality"]), spec, x)
        assert out.shape[0] == r["out_frames"] and sha1(out) == r["sha1"], r
        # the reference test's only assertion (src/test.ts:40): durations agree within 10 ms
        assert abs(x.shape[0] / r["in_rate"] - out.shape[0] / r["out_rate"]) < 0.01


def test_oracle_float_entry_point_matches_the_reference_goldens(golden):
    """speex_resampler_process_interleaved_float (native reference; the WASM build does not export
    it): bit-identical float32 bytes, counters and positions, incl. capacity-bound calls and the
    8k->48k case where one 160-frame block emits more than 1024 outputs (float path only)."""
    from make_golden import float_input
    for c in golden["float_cases"]:
        x = float_input(c["frames"], c["channels"], c["seed"])
        o = orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
        assert o.kind == c["kind"]
        outs, off = [], 0
        for (n, cap, used, made, pos, ph) in c["calls"]:
            y, u = o.process_float(x[off: off + n], cap)
            assert (u, y.shape[0]) + o.position() == (used, made, pos, ph), c["name"]
            outs.append(y)
            off += u
        out = np.concatenate(outs)
        assert out.shape[0] == c["out_frames"] and sha1(out) == c["out_sha1"], c["name"]


def test_oracle_mid_stream_control_matches_the_reference_goldens(golden):
    """set_rate / set_rate_frac / set_quality / skip_zeros / reset_mem between processing calls
    (reference deps/speex/resample.c:703-782, 904-922, 1084-1220): 40 scripts x 24 ops recorded
    on the native reference; the restatement must reproduce every return code, counter,
    output digest and visible state, incl. the pending ("magic") frames."""
    from make_golden import apply_op
    n_pending = 0
    for c in golden["control_cases"]:
        o = orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
        for k, (op, want) in enumerate(zip(c["ops"], c["results"])):
            row, _ = apply_op(o, op, c["channels"])
            assert row == want, (c["name"], k, op)
            n_pending += row[-8] > 0
    assert n_pending > 100  # the scripts really exercise the pending-frame paths


def test_oracle_equals_reference_build_on_random_control_scripts():
    """Same ops on the reference build and on the restatement, beyond the committed scripts: against the digests
    the reference recorded (tests/golden/golden_random_configs.json, make_golden_standalone.py) and, when
    oracle/_ref is there, against the live build (full output bytes and histories compared, not digests)."""
    import json
    from make_golden import apply_op
    from make_golden_standalone import random_control_scripts, record_digest, run_control_script
    with open(os.path.join(ROOT, "tests", "golden", "golden_random_configs.json")) as f:
        recorded = json.load(f)["control_scripts"]
    scripts = random_control_scripts()
    assert len(scripts) == len(recorded) == 25
    for seed, ((args, ops), want) in enumerate(zip(scripts, recorded)):
        assert record_digest(run_control_script(orc.Oracle, args, ops)) == want, (seed, args)
    if not orc.have_reference():
        return
    for seed, (args, ops) in enumerate(scripts):
        ch = args[0]
        a, b = orc.Reference(*args), orc.Oracle(*args)
        for op in ops:
            ra, ya = apply_op(a, op, ch)
            rb, yb = apply_op(b, op, ch)
            assert ra == rb, (seed, op)
            if ya is not None:
                assert ya.tobytes() == yb.tobytes()
            for c in range(ch):
                assert a.history(c).tobytes() == b.history(c).tobytes()
                assert a.pending(c).tobytes() == b.pending(c).tobytes()


def test_restatement_reproduces_the_per_channel_and_failed_filter_scripts():
    """the per-channel entry points with strides (resample.c:927-1036,
    1170-1188), interleaved calls on states whose channels stand apart (:1061-1082) and the
    resampler_basic_zero fallback after a filter change that cannot build its filter (:561-591,
    785-791) -- 624 ops recorded from the reference (tests/golden/make_golden_channels.py): return
    codes, counters, digests of the whole sentinel-filled output buffers, every channel's position."""
    import json
    from make_golden_channels import apply_channel_op
    with open(os.path.join(ROOT, "tests", "golden", "golden_channels.json")) as f:
        doc = json.load(f)
    assert doc["sentinels"] == [orc.SENTINEL_I16, orc.SENTINEL_F32]
    ops = zero_ops = 0
    for c in doc["scripts"]:
        eng = orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
        for k, (op, want) in enumerate(zip(c["ops"], c["results"])):
            got = apply_channel_op(eng, op, c["channels"])
            assert got == want, (c["name"], k, op, got, want)
            ops += 1
            zero_ops += op[0] in ("int", "float", "int_ch", "float_ch") and want[0] == 1
    assert ops == 624 and zero_ops >= 50
    if orc.have_reference():  # dev container / prebuilt _ref: the recorded rows ARE the reference's
        c = doc["scripts"][3]
        eng = orc.Reference(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
        for op, want in zip(c["ops"], c["results"]):
            assert apply_channel_op(eng, op, c["channels"]) == want
