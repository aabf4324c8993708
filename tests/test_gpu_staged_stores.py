"""The period kernel's staged stores (kernels_period_impl.h, fir_tile_staged): a one-stream stereo launch of one generation
writes its output through an LDS image as whole 16-byte pieces instead of per-lane 20-byte runs.  Only where the bytes
are written changes, so in the default mode -- whose bytes do not depend on the batch a stream runs in -- a one-stream
call (staged) must give the same bytes as the same stream inside a 32-stream batch (per-lane stores), touch nothing
outside [0, n_out), and stay within +-1 LSB of the oracle.  41.4k -> 36.3k (138:121; den = 121, not a multiple of R = 5,
25 groups in shares of 13) covers a share whose phases run past den and the padding phases of the last group."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-speex-resampler_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

CH, FI, FO, Q = 2, 44100, 48000, 7  # BASELINE configs[1]
FRAMES = 1 << 20
SENTINEL = 0x5A5A
DIAG_LIB = os.path.join(ROOT, "node-speex-resampler_amd", "ab", "libspeexhip_diag.so")


def _signal(frames, seed, float_io):
    import oracle as orc
    x = orc.lcg_pcm(frames * CH, seed).reshape(frames, CH)
    return x.astype(np.float32) if float_io else x


def _run(n_streams, fi, fo, prior, cap, offset_bytes, float_io):
    """Stream 0 of an n_streams batch: an optional first call of `prior` frames, then FRAMES frames into a buffer that
    starts `offset_bytes` into a sentinel-filled allocation.  Returns (the first call's output, the second call's
    allocation as bytes, frames made, sample dtype)."""
    import torch
    import speexhip
    dt_t = torch.float32 if float_io else torch.int16
    es = 4 if float_io else 2
    sp = torch.cuda.current_stream().cuda_stream
    b = speexhip.Batch(n_streams, CH, fi, fo, Q)
    try:
        firsts = None
        if prior:
            xs = np.stack([_signal(prior, 7 + s, float_io) for s in range(n_streams)])
            d_in = torch.from_numpy(xs).cuda()
            pcap = prior * 2
            d_out = torch.zeros((n_streams, pcap, CH), dtype=dt_t, device="cuda")
            _, made = b.process_device(d_in.data_ptr(), prior * CH, prior, d_out.data_ptr(), pcap * CH, pcap, sp,
                                       float_io=float_io)
            torch.cuda.synchronize()
            firsts = d_out[0, : made[0]].cpu().numpy()
        xs = np.stack([_signal(FRAMES, 1000 + s, float_io) for s in range(n_streams)])
        d_in = torch.from_numpy(xs).cuda()
        stride = (cap + 16) * CH  # samples per stream's allocation
        alloc = torch.empty((n_streams * stride * es + 256,), dtype=torch.uint8, device="cuda")
        alloc.view(torch.int16).fill_(SENTINEL)
        pad = -alloc.data_ptr() % 256  # stream 0's buffer starts offset_bytes past a 256-byte boundary
        _, made = b.process_device(d_in.data_ptr(), FRAMES * CH, FRAMES, alloc.data_ptr() + pad + offset_bytes, stride, cap,
                                   sp, float_io=float_io)
        torch.cuda.synchronize()
        return firsts, alloc[pad: pad + stride * es].cpu().numpy(), made[0], (np.float32 if float_io else np.int16)
    finally:
        b.close()


CASES = [  # (id, in rate, out rate, prior frames, output capacity in frames, byte offset of the output buffer, float I/O)
    ("cfg2", FI, FO, 0, 1 << 21, 0, False),
    ("k_shift", FI, FO, 1001, 1 << 21, 0, False),
    ("n_out_mid_period", FI, FO, 1001, 1_000_003, 0, False),
    ("aligned4_not16", FI, FO, 1001, 1 << 21, 4, False),
    ("aligned2_fallback", FI, FO, 1001, 1 << 21, 2, False),
    ("float_io", FI, FO, 1001, 1_000_003, 4, True),
    ("den121", 41400, 36300, 1001, 1 << 21, 0, False),
    ("den121_n_out_mid_period", 41400, 36300, 1001, 900_001, 4, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_stream_equals_batched_bytes(case):
    _, fi, fo, prior, cap, off, float_io = case
    f1, raw1, made1, dt = _run(1, fi, fo, prior, cap, off, float_io)
    f32, raw32, made32, _ = _run(32, fi, fo, prior, cap, off, float_io)
    assert made1 == made32 and made1 > 0
    if cap < FRAMES * 2:
        assert made1 == cap  # the call ends inside a period
    if prior:
        assert np.array_equal(f1.view(np.uint8), f32.view(np.uint8))
    end = off + made1 * CH * np.dtype(dt).itemsize
    assert np.array_equal(raw1[off:end], raw32[off:end]), "staged stores changed the output bytes"
    # nothing in front of the buffer or behind the last frame made is written
    sent = np.frombuffer(np.array([SENTINEL], np.int16).tobytes(), np.uint8)
    for raw in (raw1, raw32):
        assert np.array_equal(raw[:off], np.resize(sent, off))
        assert np.array_equal(raw[end:], np.resize(sent, raw.size - end))
    if not float_io:  # +-1 LSB of the reference
        import oracle as orc
        o = orc.Oracle(CH, fi, fo, Q)
        if prior:
            o.process(_signal(prior, 7, False), prior * 2)
        want, _ = o.process(_signal(FRAMES, 1000, False), cap)
        got = np.frombuffer(raw1[off:end].tobytes(), np.int16).reshape(-1, CH)
        assert got.shape == want.shape
        assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1


PROBE = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(sys.argv[1], "node-speex-resampler_amd", "python"))
import speexhip
off, float_io, fi, fo, cap = int(sys.argv[2]), sys.argv[3] == "1", int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
frames = 1 << 20
d_in = torch.zeros((frames, 2), dtype=torch.float32 if float_io else torch.int16, device="cuda")
alloc = torch.zeros(((cap + 16) * 2 * 4 + 256,), dtype=torch.uint8, device="cuda")
b = speexhip.Batch(1, 2, fi, fo, 7)
b.process_device(d_in.data_ptr(), frames * 2, frames, alloc.data_ptr() + (-alloc.data_ptr() % 256) + off, (cap + 16) * 2, cap,
                 torch.cuda.current_stream().cuda_stream, float_io=float_io)
torch.cuda.synchronize()
b.close()
"""


@pytest.mark.parametrize("off,float_io,fi,fo,cap,staged", [
    (0, False, FI, FO, 1 << 21, 1), (4, False, FI, FO, 1 << 21, 1), (0, False, FI, FO, 1_000_003, 1),
    (2, False, FI, FO, 1 << 21, 0), (4, True, FI, FO, 1_000_003, 1), (4, False, 41400, 36300, 900_001, 1)])
def test_one_stream_launch_takes_the_staged_instance(off, float_io, fi, fo, cap, staged):
    """The diagnostics build's plan line (SPEEXHIP_PLAN_VERBOSE) names the instance the launch took."""
    assert os.path.exists(DIAG_LIB), "ab/libspeexhip_diag.so not built (make -C node-speex-resampler_amd diag)"
    env = dict(os.environ, SPEEXHIP_LIB_PATH=DIAG_LIB, SPEEXHIP_PLAN_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", PROBE, ROOT, str(off), "1" if float_io else "0", str(fi), str(fo), str(cap)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("period launch: r=5 ")]
    assert lines, r.stderr[-2000:]
    assert all(ln.endswith("staged=%d" % staged) for ln in lines), lines
