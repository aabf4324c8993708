#!/usr/bin/env python3
"""tools/planar_bench.py -- what the two extra passes of a planar call cost (profiles/planar_overhead.txt is a run of it).

Per row (configuration, sample type, streams x 2^20 frames, device-resident), medians of repeated runs of K back-to-back
calls between two device synchronisations:
  (a) the interleaved device call of the PARENT commit's library (--parent-lib PATH, loaded in a child process through
      SPEEXHIP_LIB_PATH) beside the same call of this library: the interleaved path did not move;
  (b) the planar call on output rows of whole 128-byte lines (and, last column, on rows one element longer, which
      sends the scatter down its element path); (b) - (a) beside its floor = bytes moved by gather and scatter / 6.3 TB/s (the measured copy rate
      of the chip) + two dependent-kernel boundaries of 1.8 us;
  (c) the caller's do-it-yourself route: torch permute(...).contiguous() in, the interleaved call, permute(...).contiguous() out;
  (d) host-fed: the planar host call against one per-channel call per channel with stride 1 (what a C caller with
      planes does today; parent library), float stereo chunks of 2^20 and 16384 frames.
Prints the chip clock (speexhip_debug_device_clock) first.  Every leg runs in a child process of its own."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-speex-resampler_amd", "python"))

ROWS = [("44.1k->48k stereo q7", 2, 44100, 48000, 7, "int"), ("44.1k->48k stereo q7", 2, 44100, 48000, 7, "float"),
        ("48k->44.1k 8ch q5", 8, 48000, 44100, 5, "int")]
STREAMS = (1, 32)
FRAMES = 1 << 20
COPY_RATE, BOUNDARY_US = 6.3e12, 1.8


def median_us(fn, sync, k, reps=9, warm=2):
    for _ in range(warm):
        fn()
    sync()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / k * 1e6)
    return statistics.median(out)


def device_legs(legs):
    import numpy as np
    import torch
    import speexhip
    res = {"clock_ghz": speexhip.device_clock()}
    stream = torch.cuda.current_stream().cuda_stream
    for name, ch, fi, fo, q, kind in ROWS:
        dt, fl = (torch.int16, False) if kind == "int" else (torch.float32, True)
        for S in STREAMS:
            T = FRAMES
            cap = T * fo // fi + 64
            k = 20 if S == 1 else 3
            key = "%s %s S=%d" % (name, kind, S)
            x = (torch.randn((S, ch, T), device="cuda") * 8000).to(dt)
            row = {}
            if "interleaved" in legs:
                b = speexhip.Batch(S, ch, fi, fo, q)
                xi = x.permute(0, 2, 1).contiguous()
                out = torch.empty((S, cap, ch), dtype=dt, device="cuda")
                row["interleaved_us"] = median_us(lambda: b.process_device(xi.data_ptr(), T * ch, T, out.data_ptr(), cap * ch, cap, stream, fl),
                                                  torch.cuda.synchronize, k)
                b.close()
                del xi, out
            if "planar" in legs:
                es = 4 if fl else 2
                # rows of whole 128-byte lines (what Batch.process_tensor allocates): both kernels on their 16-bytes-per-
                # lane path; then rows one element longer: plane bases off 16 bytes, the scatter element by element
                for label, pitch in (("planar_us", (cap + 63) & ~63), ("planar_unaligned_us", ((cap + 63) & ~63) + 1)):
                    b = speexhip.Batch(S, ch, fi, fo, q)
                    out = torch.empty((S, ch, pitch), dtype=dt, device="cuda")
                    made = []
                    row[label] = median_us(lambda: made.append(b.process_planar_device(x.data_ptr(), ch * T, T, T, out.data_ptr(), ch * pitch, pitch, cap, stream, fl)[1][0]),
                                           torch.cuda.synchronize, k)
                    b.close()
                    del out
                moved = 2 * S * ch * es * (T + made[-1])
                row["floor_us"] = moved / COPY_RATE * 1e6 + 2 * BOUNDARY_US
            if "diy" in legs:
                b = speexhip.Batch(S, ch, fi, fo, q)
                out = torch.empty((S, cap, ch), dtype=dt, device="cuda")

                def diy():
                    xi = x.permute(0, 2, 1).contiguous()
                    _, m = b.process_device(xi.data_ptr(), T * ch, T, out.data_ptr(), cap * ch, cap, stream, fl)
                    return out[:, : m[0]].permute(0, 2, 1).contiguous()
                row["diy_us"] = median_us(diy, torch.cuda.synchronize, k)
                b.close()
                del out
            res[key] = row
            del x
            torch.cuda.empty_cache()
    return res


def host_legs(legs):
    import numpy as np
    import speexhip
    res = {}
    ch, fi, fo, q = 2, 44100, 48000, 7
    for frames in (FRAMES, 16384):
        x = (np.random.RandomState(1).randn(ch, frames) * 8000).astype(np.float32)
        cap = frames * fo // fi + 64
        planes = [np.ascontiguousarray(x[c]) for c in range(ch)]
        outs = [np.zeros(cap, np.float32) for _ in range(ch)]
        r = speexhip.Resampler(ch, fi, fo, q)
        k = 5 if frames > 100000 else 50
        row = {}
        if "host_planar" in legs:
            row["host_planar_us"] = median_us(lambda: r.planar_call("float", planes, cap, out_planes=outs), lambda: None, k)
        if "host_per_channel" in legs:
            import ctypes as C
            L = speexhip.lib()
            pf = C.POINTER(C.c_float)

            def per_channel():
                for c in range(ch):
                    il, ol = C.c_uint32(frames), C.c_uint32(cap)
                    rc = L.speexhip_resampler_process_float(r._h, c, planes[c].ctypes.data_as(pf), C.byref(il), outs[c].ctypes.data_as(pf), C.byref(ol))
                    assert rc == 0
            row["host_per_channel_us"] = median_us(per_channel, lambda: None, k)
        r.close()
        res["host float stereo %d frames" % frames] = row
    return res


def child(lib, legs):
    env = dict(os.environ)
    if lib:
        env["SPEEXHIP_LIB_PATH"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", ",".join(legs)], env=env, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit("leg %s failed:\n%s" % (legs, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    if "--child" in sys.argv:
        legs = sys.argv[sys.argv.index("--child") + 1].split(",")
        res = device_legs(legs) if not legs[0].startswith("host") else host_legs(legs)
        print(json.dumps(res))
        return
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    mine = child(None, ["interleaved", "planar", "diy"])
    old = child(parent, ["interleaved"]) if parent else {}
    print("chip clock under load: median %.3f GHz, slowest workgroup %.3f GHz" % tuple(mine.pop("clock_ghz")))
    old.pop("clock_ghz", None)
    print("device-resident, %d frames per stream; us per call (median of 9 runs of K back-to-back calls)" % FRAMES)
    print("%-36s %12s %12s %10s %10s %10s %8s %10s %14s" % ("row", "(a) parent", "(a) this", "(b) planar", "(b)-(a)", "floor", "ratio", "(c) torch",
                                                            "(b) odd stride"))
    for key, row in mine.items():
        a_old = old.get(key, {}).get("interleaved_us", float("nan"))
        extra = row["planar_us"] - row["interleaved_us"]
        print("%-36s %12.1f %12.1f %10.1f %10.1f %10.1f %8.2f %10.1f %14.1f" % (key, a_old, row["interleaved_us"], row["planar_us"], extra,
                                                                             row["floor_us"], extra / row["floor_us"], row["diy_us"],
                                                                             row["planar_unaligned_us"]))
    host_new = child(None, ["host_planar"])
    host_old = child(parent, ["host_per_channel"])
    print("host-fed (d): us per call; planar host call (this commit) | one per-channel call per channel, stride 1 (%s library)" %
          ("parent" if parent else "this"))
    for key in host_new:
        print("%-36s %12.1f %12.1f" % (key, host_new[key]["host_planar_us"], host_old[key]["host_per_channel_us"]))


if __name__ == "__main__":
    main()
