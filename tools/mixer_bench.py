#!/usr/bin/env python3
"""A record, not a gate: what one 20 ms tick of a wideband bridge costs through the mixer (speexhip.Mixer.process) and
through the route the library offered before it -- speexhip.process_many_fmt to F32 host buffers, then the caller's own
summing loop and encoder, here in numpy, written to give the same bytes (float64, ascending slot order, one rounding;
floor(v + 0.5), the rails, big-endian int16).

  python tools/mixer_bench.py [--legs 32,256,1024] [--ticks 40] [--warmup 5] [--loop-ticks 3] [--out profiles/mixer.txt]
  python tools/mixer_bench.py --trace-only --legs 256     # the mixer's ticks alone, for a kernel-trace run of its own
  python tools/mixer_bench.py --levels                    # with the legs' levels on ("Mixer levels"): every timed tick is
                                                          # process + get_levels; the route before measures them in numpy
  python tools/mixer_bench.py --route-levels              # the route before alone measures them (any build of the library)

Legs: mono, cycling 8 kHz mu-law, 8 kHz A-law and 16 kHz S16BE (RTP L16), all resampled to 16 kHz, q5; n legs x n buses,
mix-minus; the buses leave as S16BE.  Every tick is timed with a host clock around the synchronous call; medians and the
fastest tick are printed, with the clock the chip holds (speexhip_debug_device_clock) and the mixer's counters per tick.
The first tick of the route before is compared with the mixer's, byte for byte, at every size."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-speex-resampler_amd", "python"))
import speexhip  # noqa: E402

OUT_RATE, QUALITY = 16000, 5
KINDS = ((8000, speexhip.FMT_ULAW, 160), (8000, speexhip.FMT_ALAW, 160), (16000, speexhip.FMT_S16BE, 320))


def legs_of(n):
    return [speexhip.Resampler(1, KINDS[i % 3][0], OUT_RATE, QUALITY) for i in range(n)]


def payloads(n, tick):
    rng = np.random.RandomState(1000 + tick)
    return [rng.randint(0, 256, KINDS[i % 3][2] * speexhip.fmt_bytes(KINDS[i % 3][1])).astype(np.uint8) for i in range(n)]


def mix_minus(n):
    return np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)


def callers_route(states, chunks, fmts, w, cap, levels=False):
    """the route before the mixer: n float results in host memory, the sum and the encoder in the caller's code"""
    t0 = time.perf_counter()
    typed = [c.view(speexhip.fmt_dtype(f)) for c, f in zip(chunks, fmts)]   # (the payload's bytes as the format's samples)
    outs, used, codes = speexhip.process_many_fmt(states, typed, fmts, speexhip.FMT_F32, [cap] * len(states))
    t1 = time.perf_counter()
    if levels:
        numpy_levels(outs)
    t_levels = time.perf_counter() - t1
    t1 = time.perf_counter()
    frames = max(o.size for o in outs)
    y = np.zeros((len(outs), frames), np.float64)
    for s, o in enumerate(outs):
        y[s, : o.size] = o
    acc = w[:, 0, None].astype(np.float64) * y[0]
    for s in range(1, len(outs)):                     # ascending order, one float64 add a term: the header's rule
        acc += w[:, s, None].astype(np.float64) * y[s]
    z = acc.astype(np.float32).astype(np.float64)
    q = np.clip(np.floor(z + 0.5), -32768.0, 32767.0)
    buses = np.where(np.isnan(q), 0.0, q).astype(">i2")
    t2 = time.perf_counter()
    return buses, t1 - t0 - t_levels, t2 - t1, t_levels


def numpy_levels(outs):
    """the levels of the legs' floats in the caller's code: the header's record ("Mixer levels"), one per leg"""
    rec = np.zeros(len(outs), speexhip.LEVEL_DTYPE)
    for s, o in enumerate(outs):
        nan = np.isnan(o)
        v = np.where(nan, np.float32(0.0), o)
        q = np.clip(np.floor(v.astype(np.float64) + 0.5), -32768.0, 32767.0).astype(np.int64)
        rec[s] = (o.size, int((q * q).sum()), int(nan.sum()), np.abs(v).max() if o.size else 0.0, 0)
    return rec


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %8.3f  fastest %8.3f ms" % (float(np.median(a)), float(a[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="32,256,1024")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-ticks", type=int, default=3, help="ticks of the route before the mixer (its numpy loop is slow)")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--levels", action="store_true", help="the legs' levels on: a tick is process + get_levels")
    ap.add_argument("--route-levels", action="store_true", help="the route before measures the levels in numpy (implied by --levels)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if speexhip.device_count() <= 0:
        raise SystemExit("mixer_bench needs a GPU: there is no CPU fallback and no CPU timing is worth printing")
    say("mixer_bench: %s; device clock under load %.2f GHz (slowest workgroup %.2f)" % ((speexhip.lib().speexhip_version().decode(),) + speexhip.device_clock()))
    for n in [int(v) for v in args.legs.split(",")]:
        fmts = [KINDS[i % 3][1] for i in range(n)]
        cap = 320 + 64
        w = mix_minus(n)
        legs = legs_of(n)
        m = speexhip.Mixer(n, n, 1)
        assert m.set_weights(w) == 0
        if args.levels:
            assert m.set_levels(1) == 0
        l0 = speexhip.debug_mixer_level_launches() if args.levels else 0
        first = None
        times = []
        c0 = speexhip.debug_mixer_counters()
        for tick in range(args.warmup + args.ticks):
            chunks = payloads(n, tick)
            t0 = time.perf_counter()
            buses, bus_frames, used, made, codes = m.process(legs, chunks, fmts, speexhip.FMT_S16BE, cap)
            if args.levels:
                recs = m.get_levels()
            dt = time.perf_counter() - t0
            assert codes == [0] * n
            if tick == 0:
                first = buses.copy()
            if tick >= args.warmup:
                times.append(1e3 * dt)
        c1 = speexhip.debug_mixer_counters()
        per_tick = {k: (c1[k] - c0[k]) / float(args.warmup + args.ticks) for k in c0}
        say("%4d legs x %4d buses  mixer.process%s %s   (bus_frames %d)" % (n, n, " + levels " if args.levels else "          ", stats(times), bus_frames))
        if args.levels:
            per_tick["level_launches"] = (speexhip.debug_mixer_level_launches() - l0) / float(args.warmup + args.ticks)
            assert int(recs["samples"].min()) == bus_frames and int(recs["energy"].min()) > 0
        say("      per tick: " + ", ".join("%s %.1f" % kv for kv in per_tick.items()))
        m.close()
        for st in legs:
            st.close()
        if args.trace_only:
            continue
        states = legs_of(n)
        many, loop, lev = [], [], []
        for tick in range(args.loop_ticks):
            want, t_many, t_loop, t_lev = callers_route(states, payloads(n, tick), fmts, w, cap, args.levels or args.route_levels)
            lev.append(1e3 * t_lev)
            if tick == 0:
                same = want.view(np.uint8).reshape(n, -1).tobytes() == np.ascontiguousarray(first).view(np.uint8).tobytes()
                say("      first tick: the route before gives %s bytes" % ("the same" if same else "DIFFERENT"))
            many.append(1e3 * t_many)
            loop.append(1e3 * t_loop)
        for st in states:
            st.close()
        say("%4d legs x %4d buses  process_many_fmt to F32  %s" % (n, n, stats(many)))
        say("%4d legs x %4d buses  + numpy sum and encoder  %s" % (n, n, stats(loop)))
        if args.levels or args.route_levels:
            say("%4d legs x %4d buses  + numpy levels           %s" % (n, n, stats(lev)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
