"""Streams fed in small calls, and batches with idle streams, against the exact model (tests/streaming.py).

The other exact-model files feed three or four calls, one of them tens of thousands of frames long: a filter meets about
three start positions and almost never a call shorter than its own history.  Here every case is ONE array cut into some
hundreds of calls by streaming.schedule() with the resubmission rule (the unconsumed frames of a capacity-bound call head
the next one): every start phase with one output, capacities that end just before, on and past the first period
boundary, calls of 0 and 1 frame, of fewer frames than taps - 1, of capacity 0, calls that make no output, silence that a
window enters in one call and leaves in a later one.  tests/test_cpu_streaming.py asserts that the schedules meet all of
this on every case used here.

One state, default mode (named: MODE_FAST_FIXED, so that the diagnostics children, which set SPEEXHIP_MODE=fast, run the
same thing), an int16 and a float stream of the same samples:
  * after every call the counters and position() equal the oracle's; history() after every 16th call and the last;
  * the concatenated bytes EQUAL those of a fresh state fed X[:consumed] in one call (chunking invariance);
  * (a), (b), (c) on the concatenated stream with the suite's margins and yardsticks; fast_path and accumulate_bits.
MODE_FAST and MODE_FAST_F32: the model's checks only (FAST is documented as not chunking-invariant).
Batches: Batch.process_device with streams idle by lens = 0, by caps = 0, a whole launch group idle beside a working
one, every stream idle, and one stream idle for 1, 2 and 3 consecutive calls (both ping-pong parities).
Converted calls: process_fmt, process_mix and process_planar in pieces EQUAL one call.
Run with -s for the per-family figures ("Streams in small calls").
"""
import numpy as np
import pytest

import exact_model as em
import oracle as orc
import sample_formats as sf
import speexhip
import streaming as st
import test_gpu_exact_model as xm
import test_gpu_parity as par

pytestmark = pytest.mark.gpu

DEFAULT = speexhip.MODE_FAST_FIXED
FAMILY = "streaming, %s"


def _expected_fast_path(family, ch, q):
    if family == "slide":
        return 4 if q >= 9 else 3
    if family == "period fp64":
        return 5
    return 5 if q >= 9 and ch in (1, 2, 4, 6, 8) else 2


def _state_stream(c, kind, mode, fast_path, name):
    """one state through the case's schedule -> (records of cut(), info); counters, positions and histories asserted
    equal to the oracle's on the way"""
    ch, i, o, q = c.key
    ref = st.oracle_run(ch, i, o, q, kind)
    r = speexhip.Resampler(ch, i, o, q, mode=mode)
    info = r.info()
    assert info["fast_path"] == fast_path, (name, info["fast_path"])

    def after(n, rec):
        want = ref[n]
        tag = (name, kind, "call", n, "start", rec["start"], "frames", rec["frames"], "cap", rec["cap"],
               "n_out", want["made"], "consumed", want["used"])
        assert rec["start"] == want["start"], tag
        assert (rec["used"], rec["made"]) == (want["used"], want["made"]), tag + (rec["used"], rec["made"])
        assert r.position() == want["end"], tag
        if "history" in want:
            assert np.array_equal(r.history(), want["history"]), tag
    recs = st.cut(c.Xf if kind == "float" else c.X, c.calls, r.process_float if kind == "float" else r.process,
                  position=r.position, after=after)
    r.close()
    return recs, info


def _first_difference(recs, one):
    """the call in which the pieces first differ from the one-call output (its start and counters name the corner)"""
    at = 0
    for n, r in enumerate(recs):
        if not np.array_equal(r["out"], one[at: at + r["made"]]):
            return ("call", n, "start", r["start"], "frames", r["frames"], "cap", r["cap"], "n_out", r["made"],
                    "consumed", r["used"], "first sample", int(np.argwhere(r["out"] != one[at: at + r["made"]])[0][0]))
        at += r["made"]
    return None


def _streaming(family, key, fast_path, mode=DEFAULT, invariant=True):
    ch, i, o, q = key
    c = st.case(ch, i, o, q)
    model = c.model
    name = "%s mode %s in %d calls" % (key, mode, len(c.calls))
    outs, bits = {}, None
    for kind in ("int16", "float"):
        recs, info = _state_stream(c, kind, mode, fast_path, name)
        bits = xm._expect_bits(info, model)
        n = st.consumed(recs)
        pieces = st.joined(recs)
        if invariant:
            one = speexhip.Resampler(ch, i, o, q, mode=mode)
            X = c.Xf if kind == "float" else c.X
            whole, used = (one.process_float if kind == "float" else one.process)(X[:n], pieces.shape[0] + 64)
            one.close()
            assert used == n and whole.shape == pieces.shape, (name, kind, used, n, whole.shape, pieces.shape)
            assert pieces.tobytes() == whole.tobytes(), (name, kind, _first_difference(recs, whole))
        outs[kind] = (pieces, n)
    assert outs["int16"][1] == outs["float"][1], name
    fed = c.X[: outs["float"][1]]
    wantf = st.joined(st.oracle_run(ch, i, o, q, "float"))
    stats = xm._judge(FAMILY % family, name, model, bits, fed, outs["int16"][0], outs["float"][0], wantf)
    assert stats["n"] >= em.BIAS_MIN_SAMPLES and "yard" in stats, (name, stats)


def test_the_cases_come_from_the_existing_lists():
    lists = {"slide": par.SLIDE_CASES + par.N_TO_ONE_CASES, "period": par.LAYOUT_CASES + [row[1:5] for row in xm.BASELINE_ROWS],
             "period fp64": par.PERIOD64_CASES, "folded": par.FOLDED_CASES}
    for family, cases in st.FAMILIES.items():
        assert set(cases) <= set(lists[family]), (family, set(cases) - set(lists[family]))
    assert st.FALLBACK in [c[:4] for c in par.EXACT_FALLBACK_CASES]
    assert set(st.FAST_CASES) <= set(xm.FAST_SHARES_CASES) and set(st.FAST_F32_CASES) <= set(xm.FAST_F32_CASES)


def test_exact_model_streaming_slide():
    for key in st.FAMILIES["slide"]:
        _streaming("slide", key, _expected_fast_path("slide", key[0], key[3]))
    xm._report(FAMILY % "slide")


def test_exact_model_streaming_period():
    for key in st.FAMILIES["period"]:
        _streaming("period", key, _expected_fast_path("period", key[0], key[3]))
    xm._report(FAMILY % "period")


def test_exact_model_streaming_period_fp64():
    for key in st.FAMILIES["period fp64"]:
        _streaming("period fp64", key, 5)
    xm._report(FAMILY % "period fp64")


def test_exact_model_streaming_folded():
    for key in st.FAMILIES["folded"]:
        _streaming("folded", key, _expected_fast_path("folded", key[0], key[3]))
    xm._report(FAMILY % "folded")


def test_exact_model_streaming_exact_fallback():
    """192:1, 40 calls of at most 4096 frames: every call's output and the history after it EQUAL the oracle's (no
    model: the filter has 30 720 taps, and the oracle passes (a) in test_gpu_exact_model.py)."""
    ch, i, o, q = st.FALLBACK
    c = st.case(ch, i, o, q, **st.FALLBACK_SCHEDULE)
    for kind in ("int16", "float"):
        r, ref = speexhip.Resampler(ch, i, o, q, mode=DEFAULT), orc.Oracle(ch, i, o, q)
        assert r.info()["fast_path"] == 0
        fn, ref_fn = (r.process_float, ref.process_float) if kind == "float" else (r.process, ref.process)
        want = []

        def call(x, cap):
            want.append(ref_fn(x, cap))
            return fn(x, cap)

        def after(n, rec):
            tag = (kind, "call", n, "start", rec["start"], "frames", rec["frames"], "cap", rec["cap"])
            assert (rec["used"], r.position()) == (want[n][1], ref.position()), tag
            assert rec["out"].dtype == want[n][0].dtype and rec["out"].tobytes() == want[n][0].tobytes(), tag
            assert np.array_equal(r.history(), st.history_of(ref)), tag
        recs = st.cut(c.Xf if kind == "float" else c.X, c.calls, call, position=r.position, after=after)
        assert sum(rec["made"] for rec in recs) > 100 and [rec["start"] for rec in recs] == [l["start"] for l in c.sched.log]
        r.close()


@pytest.mark.parametrize("ch,i,o,q,fast_path", st.FAST_CASES)
def test_exact_model_streaming_fast_mode(ch, i, o, q, fast_path):
    _streaming("MODE_FAST", (ch, i, o, q), fast_path, mode=speexhip.MODE_FAST, invariant=False)
    xm._report(FAMILY % "MODE_FAST")


@pytest.mark.parametrize("ch,i,o,q,fast_path", st.FAST_F32_CASES)
def test_exact_model_streaming_fast_f32_mode(ch, i, o, q, fast_path):
    _streaming("MODE_FAST_F32", (ch, i, o, q), fast_path, mode=speexhip.MODE_FAST_F32, invariant=False)
    xm._report(FAMILY % "MODE_FAST_F32")


# ---- batches with idle streams ----
GROUP = 32      # streams per launch group (kMaxPackedStreams)
LENS0, CAPS0 = "lens = 0", "caps = 0"


def _idle_mask(S, n_calls):
    """{call: {stream: LENS0 | CAPS0}}: who idles when, and how"""
    mask = {}

    def put(call, streams, how=None):
        if call < n_calls - 1:      # (never the closing long call)
            for s in streams:
                mask.setdefault(call, {})[s] = how or (LENS0 if (call + s) % 2 else CAPS0)
    for call in range(5, n_calls, 20):
        put(call, [s for s in range(S) if s % 3 == 1], LENS0)
    for call in range(10, n_calls, 20):
        put(call, [s for s in range(S) if s % 3 == 2], CAPS0)
    if S > GROUP:
        put(30, range(GROUP)), put(31, range(GROUP))            # all of group 0 idle while group 1 works, twice ...
        put(33, range(GROUP, S))                                # ... and the reverse
        put(36, range(GROUP), CAPS0), put(37, range(GROUP, S), LENS0)
    put(40, range(S))                                           # every stream idle: no launch, no flip
    put(41, range(S), CAPS0), put(42, range(S), LENS0)
    lone = [3] + ([GROUP + 3] if S > GROUP + 3 else [])
    for first, run in ((50, 1), (60, 2), (70, 3), (80, 1), (83, 2)):    # one stream idle for 1, 2 and 3 calls
        for call in range(first, first + run):
            put(call, lone)
    return mask


def _batch_with_idle_streams(key, S, fast_path, judged):
    import torch
    ch, i, o, q = key
    c = st.batch_case(ch, i, o, q)
    model, calls = c.model, c.calls
    n_calls = len(calls)
    mask = _idle_mask(S, n_calls)
    name = "%s x %d streams in %d calls" % (key, S, n_calls)
    # stream s: the schedule rotated by 7 s calls (the long call stays last), its own samples
    rot = [[calls[(n + 7 * s) % (n_calls - 1)] for n in range(n_calls - 1)] + [calls[-1]] for s in range(S)]
    total = sum(f for f, _ in calls) + 64
    Xs = [np.roll(np.resize(c.X, (total, ch)), 131 * s, axis=0) for s in range(S)]
    F = max(f for f, _ in calls)
    cap_buf = F * model.den // model.num + 64
    sp = torch.cuda.current_stream().cuda_stream
    result = {}
    for kind in ("int16", "float"):
        fl = kind == "float"
        b = speexhip.Batch(S, ch, i, o, q, mode=DEFAULT)
        info = b.info()
        assert info["fast_path"] == fast_path, (name, info["fast_path"])
        bits = xm._expect_bits(info, model)
        refs = [orc.Oracle(ch, i, o, q) for _ in range(S)]
        offs, got, want = [0] * S, [[] for _ in range(S)], [[] for _ in range(S)]
        host = np.zeros((S, max(F, 1), ch), np.float32 if fl else np.int16)
        d_out = torch.zeros((S, cap_buf, ch), dtype=torch.float32 if fl else torch.int16, device="cuda")
        idled = set()       # streams that idled in the previous call: their history is checked once more
        for n in range(n_calls):
            lens, caps = [], []
            for s in range(S):
                frames, cap = rot[s][n]
                how = mask.get(n, {}).get(s)
                frames, cap = (0 if how == LENS0 else frames), (0 if how == CAPS0 else min(cap, cap_buf))
                host[s, :frames] = Xs[s][offs[s]: offs[s] + frames]
                lens.append(frames), caps.append(cap)
            d_in = torch.from_numpy(host).cuda()
            used, made = b.process_device(d_in.data_ptr(), host.shape[1] * ch, lens, d_out.data_ptr(), cap_buf * ch, caps, sp, fl)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            idle_now = set()
            for s in range(S):
                x = host[s, : lens[s]]
                w, wu = refs[s].process_float(x, caps[s]) if fl else refs[s].process(x, caps[s])
                tag = (name, kind, "call", n, "stream", s, "lens", lens[s], "caps", caps[s], mask.get(n, {}).get(s))
                assert (used[s], made[s]) == (wu, w.shape[0]), tag + (used[s], made[s], wu, w.shape[0])
                inf = b.info(s)
                assert (inf["last_sample"], inf["samp_frac_num"]) == refs[s].position(), tag
                if wu == 0 and w.shape[0] == 0:
                    idle_now.add(s)
                if s in idle_now or s in idled or n == n_calls - 1:
                    assert np.array_equal(b.lines(s), st.history_of(refs[s])), tag
                got[s].append(out[s, : made[s]].copy()), want[s].append(w)
                offs[s] += wu
            idled = idle_now
            if n in mask:
                assert set(mask[n]) <= idle_now, (name, n)
        b.close()
        for s in range(S):
            pieces = np.concatenate(got[s])
            one = speexhip.Resampler(ch, i, o, q, mode=DEFAULT)
            X = Xs[s][: offs[s]]
            whole, u = (one.process_float(X.astype(np.float32), pieces.shape[0] + 64) if fl
                        else one.process(X, pieces.shape[0] + 64))
            one.close()
            assert u == offs[s] and pieces.tobytes() == whole.tobytes(), (name, kind, "stream", s)
        result[kind] = (got, want, list(offs), bits)
    for s in judged:
        g16, gf = np.concatenate(result["int16"][0][s]), np.concatenate(result["float"][0][s])
        assert result["int16"][2][s] == result["float"][2][s]
        xm._judge(FAMILY % "batch", "%s stream %d" % (name, s), model, result["float"][3], Xs[s][: result["float"][2][s]],
                  g16, gf, np.concatenate(result["float"][1][s]))


def test_exact_model_streaming_batch_of_two_launch_groups_with_idle_streams():
    """40 streams = launch groups of 32 + 8; judged: one of each group that idled while the other group worked, and the
    stream that idles alone"""
    _batch_with_idle_streams((2, 44100, 48000, 7), 40, 2, judged=(0, 3, 39))
    xm._report(FAMILY % "batch")


@pytest.mark.parametrize("ch,i,o,q,fast_path", [(2, 48000, 8000, 7, 3), (1, 24000, 48000, 10, 4), (2, 44100, 48000, 10, 5),
                                                (2, 72000, 16000, 7, 2)])
def test_exact_model_streaming_small_batches_with_idle_streams(ch, i, o, q, fast_path):
    _batch_with_idle_streams((ch, i, o, q), 5, fast_path, judged=(0, 3, 4))
    xm._report(FAMILY % "batch")


# ---- converted calls: the pieces EQUAL one call ----
N_CONVERTED = 120


def _converted(key, make_call, X, per_frame):
    """the first N_CONVERTED calls of the case's schedule and a closing unbounded call (so that the last outputs rest on
    consumed frames), through make_call(state) -> call(x, cap) -> (flat output, used); per_frame: output samples per
    frame.  -> (states' pieces == one call) asserted; returns frames made."""
    ch, i, o, q = key
    c = st.case(ch, i, o, q)
    calls = c.calls[:N_CONVERTED] + [(c.model.taps + 5, st.BIG)]
    outs = []
    for cut_it in (True, False):
        r = speexhip.Resampler(ch, i, o, q, mode=DEFAULT)
        call = make_call(r)

        def framed(x, cap, call=call):
            y, used = call(x, cap)
            return np.asarray(y).reshape(-1, per_frame), used
        if cut_it:
            recs = st.cut(X, calls, framed)
            n, pieces = st.consumed(recs), st.joined(recs)
            outs.append(pieces)
            made = pieces.shape[0]
            assert made >= N_CONVERTED and sum(1 for rec in recs if rec["used"] < rec["frames"]) >= 10, key
            after = getattr(call, "after", None)
            if after:
                after(r, made)
        else:
            whole, used = framed(X[:n], outs[0].shape[0] + 64)
            assert used == n and whole.shape == outs[0].shape, (key, used, n, whole.shape, outs[0].shape)
            assert whole.tobytes() == outs[0].tobytes(), (key, _first_difference(recs, whole))
        r.close()
    return made


def test_streaming_formatted_calls_s24_to_f32n():
    key = (2, 44100, 48000, 7)
    c = st.case(*key)
    X24 = (c.X.astype(np.int32) << 8) | (c.X.astype(np.int32) & 0xFF)       # (low bytes in use)

    def make(r):
        return lambda x, cap: r.process_fmt(sf.pack_s24(x), speexhip.FMT_S24, speexhip.FMT_F32N, cap)
    _converted(key, make, X24, key[0])


def test_streaming_formatted_calls_f32_to_u8_with_triangular_dither():
    key = (1, 48000, 11025, 7)
    c = st.case(*key)

    def make(r):
        assert r.set_dither(speexhip.DITHER_TRIANGULAR, 77, 0) == 0

        def call(x, cap):
            return r.process_fmt(x, speexhip.FMT_F32, speexhip.FMT_U8, cap)

        def after(state, made):
            assert state.get_dither() == (speexhip.DITHER_TRIANGULAR, 77, made), (state.get_dither(), made)
        call.after = after
        return call
    _converted(key, make, c.Xf, key[0])


def test_streaming_mixed_calls_downmix_before_and_upmix_after():
    key = (1, 48000, 44100, 7)
    c = st.case(*key)
    stereo = np.stack([c.Xf[:, 0], np.roll(c.Xf[:, 0], 977) * np.float32(0.5)], axis=1)
    in_mix, out_mix = [[0.5, 0.25]], [[1.0], [0.5]]

    def make(r):
        return lambda x, cap: r.process_mix(x, speexhip.FMT_F32, speexhip.FMT_F32, cap, in_mix=in_mix, out_mix=out_mix)
    _converted(key, make, stereo, 2)


def test_streaming_planar_calls_of_three_channels():
    key = (3, 48000, 44100, 4)
    c = st.case(*key)

    def make(r):
        def call(x, cap):
            y, used = r.process_planar(np.ascontiguousarray(x.T), cap)
            return np.ascontiguousarray(y.T), used
        return call
    _converted(key, make, c.X, key[0])
