#!/usr/bin/env python3
"""What the output gain costs: same-box A/B of the formatted batch device call with every stream's gain off, with a
constant gain on and with a ramp in flight (one that outlasts the run), and -- given --parent-lib, a libspeexhip.so built
from the parent commit -- the parent, which has no gain.  With the gain off the kernels are the parent's, so those two
legs must agree within the run-to-run spread; a constant gain adds one multiply a sample to a pass that moves 6 bytes a
sample; the ramp adds the frame index (a 32-bit division a sample in the flat converting pass) and two fp64 operations.
Two workloads:

  bulk   32 streams x 2^20 stereo frames, 44.1k -> 48k q7, F32 -> S16   (bandwidth-bound: the pass reads 4 and writes 2 bytes a sample)
  tick   32 streams x 160 mono frames, 8k -> 16k q5, mu-law -> mu-law    (a telephony tick: launch-bound)

Every leg runs in a child process of its own (the library is chosen at load time), the legs alternate round after round,
and the medians over the rounds are printed with the chip clock of speexhip_debug_device_clock.

  python tools/gain_bench.py [--rounds 5] [--parent-lib PATH] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-speex-resampler_amd", "python"))


def child(mode):
    import torch
    import speexhip
    res = {"clock_ghz": speexhip.device_clock()}
    stream = torch.cuda.current_stream().cuda_stream

    def run(name, S, ch, fi, fo, q, frames, in_fmt, out_fmt, in_dtype, out_dtype, calls, warm):
        b = speexhip.Batch(S, ch, fi, fo, q)
        if mode == "constant":
            assert b.set_gain(0.5, 0) == 0
        if mode == "ramp":
            assert b.set_gain(0.5, 0xFFFFFFFF) == 0   # (in flight through every call of the run)
        cap = frames * fo // fi + 64
        if in_dtype == torch.float32:
            x = (torch.rand((S, frames, ch), device="cuda") * 2.6 - 1.3) * 32767.0   # clips both rails
        else:
            x = torch.randint(0, 256, (S, frames, ch), dtype=torch.uint8, device="cuda")
        y = torch.empty((S, cap, ch), dtype=out_dtype, device="cuda")
        call = lambda: b.process_fmt_device(in_fmt, x.data_ptr(), frames * ch, frames, out_fmt, y.data_ptr(), cap * ch, cap, stream)
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        per = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / calls * 1e6)
        res[name + "_us"] = min(per)
        if mode != "off":
            g = b.get_gain(0)
            res[name + "_gain"] = [float(g["current"]), float(g["target"]), g["remaining"]]
            assert (g["remaining"] != 0) == (mode == "ramp"), g
        b.close()

    run("bulk", 32, 2, 44100, 48000, 7, 1 << 20, speexhip.FMT_F32, speexhip.FMT_S16, torch.float32, torch.int16, 10, 3)
    run("tick", 32, 1, 8000, 16000, 5, 160, speexhip.FMT_ULAW, speexhip.FMT_ULAW, torch.uint8, torch.uint8, 500, 50)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("off", "constant", "ramp"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    legs = [("branch, gain off", "off", None), ("branch, constant gain", "constant", None), ("branch, ramp in flight", "ramp", None)]
    if a.parent_lib:
        legs.insert(0, ("parent (no gain)", "off", os.path.abspath(a.parent_lib)))
    rows = {name: {"bulk_us": [], "tick_us": []} for name, _, _ in legs}
    clock = None
    for _ in range(a.rounds):
        for name, mode, lib in legs:
            env = dict(os.environ)
            if lib:
                env["SPEEXHIP_LIB_PATH"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:
                sys.exit("leg %r failed (%d):\n%s" % (name, p.returncode, p.stderr[-2000:]))
            d = json.loads(p.stdout.strip().splitlines()[-1])
            clock = d["clock_ghz"]
            for k in ("bulk_us", "tick_us"):
                rows[name][k].append(d[k])
    lines = ["# tools/gain_bench.py: medians of %d alternating rounds, us per call; clock (GHz, min) %s" % (a.rounds, clock),
             "%-24s %14s %14s" % ("leg", "bulk 32x2^20", "tick 32x160")]
    for name, _, _ in legs:
        lines.append("%-24s %14.1f %14.2f" % (name, statistics.median(rows[name]["bulk_us"]), statistics.median(rows[name]["tick_us"])))
    lines.append("# every round: " + json.dumps(rows))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
