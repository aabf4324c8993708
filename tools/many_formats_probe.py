"""Diagnostics: one fused formatted many-states call against the same entries as separate formatted calls -- the pair of
medians DESIGN.md and profiles/many_formats_fused.txt quote, with the box's clock.  Two cases:
  telephony  32 mono 8000 -> 16000 q7 legs, 160-frame mu-law payloads, f32n results (a gateway's 20 ms tick)
  large      32 stereo 44100 -> 48000 q7 states, 2^20-frame s16 chunks, f32n results
  python tools/many_formats_probe.py [--steps N] [--large-steps M]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-speex-resampler_amd", "python"))
import speexhip  # noqa: E402


def measure(key, in_fmt, out_fmt, n, frames, steps, warm):
    ch, fi, fo, q = key
    L = speexhip.lib()
    cap = frames * fo // fi + 64
    states = [speexhip.Resampler(*key) for _ in range(n)]
    twins = [speexhip.Resampler(*key) for _ in range(n)]
    rng = np.random.RandomState(5)
    raws = [rng.randint(0, 256, frames * ch * speexhip.fmt_bytes(in_fmt)).astype(np.uint8) for _ in range(n)]
    outs = [np.zeros(cap * ch * speexhip.fmt_bytes(out_fmt), np.uint8) for _ in range(n)]
    hs, ins, ops = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    fa, fb = (C.c_int * n)(*[in_fmt] * n), (C.c_int * n)(*[out_fmt] * n)
    il, ol, codes = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int * n)()
    for i in range(n):
        hs[i], ins[i], ops[i] = states[i]._h, raws[i].ctypes.data, outs[i].ctypes.data
    a, b = C.c_uint32(), C.c_uint32()
    t_fused, t_apart = [], []
    before = speexhip.many_counters()
    for step in range(steps + warm):
        for i in range(n):
            il[i], ol[i] = frames, cap
        t0 = time.perf_counter()
        rc = L.speexhip_resampler_process_many_fmt(n, hs, fa, ins, il, fb, ops, ol, codes)
        t1 = time.perf_counter()
        assert rc == 0, rc
        for i in range(n):
            a.value, b.value = frames, cap
            rc = L.speexhip_resampler_process_interleaved_fmt(twins[i]._h, in_fmt, ins[i], C.byref(a), out_fmt, ops[i], C.byref(b))
            assert rc == 0, rc
        t2 = time.perf_counter()
        if step >= warm:
            t_fused.append(t1 - t0)
            t_apart.append(t2 - t1)
    after = speexhip.many_counters()
    for st in states + twins:
        st.close()
    per_call = {k: (after[k] - before[k]) / float(steps + warm) for k in after}
    return np.median(t_fused) * 1e6, np.median(t_apart) * 1e6, per_call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--large-steps", type=int, default=12)
    args = ap.parse_args()
    ghz, ghz_min = speexhip.device_clock()
    print("box: %.3f GHz under load (slowest workgroup %.3f)" % (ghz, ghz_min))
    f, s, c = measure((1, 8000, 16000, 7), speexhip.FMT_ULAW, speexhip.FMT_F32N, 32, 160, args.steps, 20)
    print("telephony  32 x 160-frame mono mu-law -> f32n, 8000 -> 16000 q7: fused %.1f us, 32 separate calls %.1f us "
          "(medians of %d steps); per fused call: %s" % (f, s, args.steps, c))
    f, s, c = measure((2, 44100, 48000, 7), speexhip.FMT_S16, speexhip.FMT_F32N, 32, 1 << 20, args.large_steps, 2)
    print("large      32 x 2^20-frame stereo s16 -> f32n, 44100 -> 48000 q7: fused %.2f ms, 32 separate calls %.2f ms "
          "(medians of %d steps); per fused call: %s" % (f / 1e3, s / 1e3, args.large_steps, c))


if __name__ == "__main__":
    main()
