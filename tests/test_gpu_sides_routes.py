"""The route of a formatted call (csrc/sides_route.h), pinned from outside: a small grid of calls through the public
Python wrappers, every form x side pair x state, each compared for equality with what the commit BEFORE the rule existed
("Mix buses: weighted sums of a batch's streams in one device call") did with the same call: return code, lengths, a sha1
of the whole output buffer (sentinel bytes behind the result included), dither position, the gain ramp's remaining frames,
the meter's samples and clip counts, and what the call added to speexhip_debug_chunk_counters / _many_counters.

The expected values (tests/golden/sides_routes.json) are recorded results: this file run at that commit with
SPEEXHIP_SIDES_ROUTES_RECORD=<path of the json to write>.  Nothing in them is written by hand or made by the code under test.

The grid: 44100 -> 48000, quality 3, two channels, FAST_FIXED (bytes depend on the stream alone), 64 input frames into room
for 128.  Forms: device and bus (two buses) on a batch of three streams; host, planes-host (the pair's result handed over
as separate planes, so that every pair reaches the call with a planar side), chunks (20 / 24 / 20 frames) and many-entry
(three entries, the first state named again by the third) on states of one stream.  Pairs: S16 -> S16, F32 -> F32,
F32N -> F32N, S16 -> F32, F32 -> S16, planar F32 -> planar F32, planar S16 -> interleaved F32N, and one with a matrix on
either side (a mono S16 input side into the state's two channels, its two channels into a three-channel S16 output side).
State: dither off / TPDF, meter off / on, gain off / a ramp of 40 frames to 1.5 (it ends inside the call), channels
together / apart (one per-channel host call of 5 frames on channel 0 first).  A batch has no per-channel call, so the
device form's apart cases run on a state of one stream -- the only kind whose channels can stand apart -- and the bus
form has none.  Two more calls per form where it applies: an input that is present and empty, and no input at all."""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import speexhip
from golden_util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "sides_routes.json")
RECORD = os.environ.get("SPEEXHIP_SIDES_ROUTES_RECORD")
S16, F32, F32N = speexhip.FMT_S16, speexhip.FMT_F32, speexhip.FMT_F32N
INTER, PLANAR = speexhip.LAYOUT_INTERLEAVED, speexhip.LAYOUT_PLANAR
CH, FI, FO, Q, FRAMES, CAP, STREAMS = 2, 44100, 48000, 3, 64, 128, 3
CHUNKS, CHUNK_CAPS = (20, 24, 20), (40, 48, 40)
SENTINEL = 0xA5
IN_MIX = np.array([[1.0], [-0.5]], np.float32)                       # the state's 2 channels from a mono side
OUT_MIX = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]], np.float32)  # a side of 3 channels from the state's 2
WEIGHTS = np.array([[1.0, 1.0, 1.0], [0.75, -0.5, 1.25]], np.float32)
FORMS = ("device", "host", "planes_host", "chunks", "many", "bus")
# name: (in fmt, in layout, in matrix, out fmt, out layout, out matrix)
PAIRS = {
    "s16-s16": (S16, INTER, None, S16, INTER, None),
    "f32-f32": (F32, INTER, None, F32, INTER, None),
    "f32n-f32n": (F32N, INTER, None, F32N, INTER, None),
    "s16-f32": (S16, INTER, None, F32, INTER, None),
    "f32-s16": (F32, INTER, None, S16, INTER, None),
    "pf32-pf32": (F32, PLANAR, None, F32, PLANAR, None),
    "ps16-f32n": (S16, PLANAR, None, F32N, INTER, None),
    "matrix": (S16, INTER, IN_MIX, S16, INTER, OUT_MIX),
}


def case_ids(form):
    """the grid of one form: '<pair>/<d><m><g><a>' with a letter where the flag is set, and the two input cases"""
    ids = []
    for pair in PAIRS:
        for d, m, g, a in itertools.product((0, 1), repeat=4):
            if a and form == "bus":
                continue
            ids.append("%s/%s%s%s%s" % (pair, "d" if d else "-", "m" if m else "-", "g" if g else "-", "a" if a else "-"))
    return ids + ["s16-f32/empty", "s16-f32/null", "f32-s16/empty", "f32-s16/null"]


def samples(seed, frames, channels):
    """int16 noise near full scale, so that a gain of 1.5 clips some of it"""
    return np.random.default_rng(1000 + seed).integers(-30000, 30000, (frames, channels)).astype(np.int16)


def storage(x, fmt, layout):
    """frames x channels of int16 as the bytes of a side"""
    a = x.T if layout == PLANAR else x
    a = a.astype(np.int16) if fmt == S16 else a.astype(np.float32) / np.float32(32768.0 if fmt == F32N else 1.0)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


class Sides:
    """the two Side structures of a call of `items` streams (or buses) in host or device memory, kept alive"""

    def __init__(self, pair, device, items=1, out_items=None, seed=0, frames=FRAMES, cap=CAP, present=True, separate_out=False):
        fi, li, mi, fo, lo, mo = PAIRS[pair]
        self.keep = [mi, mo]
        n_in = CH if mi is None else mi.shape[1]
        n_out = CH if mo is None else mo.shape[0]
        out_items = items if out_items is None else out_items
        raw = np.concatenate([storage(samples(seed + s, max(frames, 1), n_in), fi, li) for s in range(items)])
        per_in = max(frames, 1) * n_in
        self.out_bytes = cap * n_out * speexhip.fmt_bytes(fo)
        self.out = np.full(out_items * self.out_bytes, SENTINEL, np.uint8)
        if device:
            import torch
            self.d_in, self.d_out = torch.from_numpy(raw).cuda(), torch.from_numpy(self.out).cuda()
            in_ptr, out_ptr = self.d_in.data_ptr(), self.d_out.data_ptr()
        else:
            self.d_out = None
            self.keep.append(raw)
            in_ptr, out_ptr = raw.ctypes.data, self.out.ctypes.data
        self.in_ptr, self.in_frame_bytes = in_ptr, speexhip.fmt_bytes(fi) * (1 if li == PLANAR else n_in)
        self.in_planes, self.in_plane_bytes = (n_in if li == PLANAR else 1), max(frames, 1) * speexhip.fmt_bytes(fi)
        self.a = speexhip.make_side(fi, n_in, li, mi, in_ptr if present else None, max(frames, 1), per_in)
        if separate_out and not device:
            lo = PLANAR
            plane = cap * speexhip.fmt_bytes(fo)
            ptrs = (C.c_void_p * n_out)(*[out_ptr + c * plane for c in range(n_out)])
            self.keep.append(ptrs)
            self.b = speexhip.make_side(fo, n_out, lo, mo, planes=ptrs)
        else:
            self.b = speexhip.make_side(fo, n_out, lo, mo, out_ptr, cap, cap * n_out)

    def digest(self):
        if self.d_out is not None:
            import torch
            torch.cuda.synchronize()
            self.out = self.d_out.cpu().numpy()
        return hashlib.sha1(self.out.tobytes()).hexdigest()


def prepare(state, flags, batch):
    """the state flags of a case on a Resampler or a Batch"""
    d, m, g, a = (c != "-" for c in flags)
    if a:
        rc = state.channel_call("int", 0, samples(99, 5, 1), 16)[0]
        assert rc == 0
    if d:
        assert state.set_dither(speexhip.DITHER_TRIANGULAR, 0x1234ABCD, 7) == 0
    if m:
        assert state.set_meter(1) == 0
    if g:
        assert state.set_gain(1.5, 40) == 0


def readout(state, streams=None):
    """dither position, gain remaining, meter samples and clip counts of every stream"""
    if streams is None:
        m = state.get_meter()
        return [[state.get_dither()[2], state.get_gain()["remaining"], m["samples"], m["clipped_high"], m["clipped_low"]]]
    out = []
    for s in range(streams):
        m = state.get_meter(s)
        out.append([state.get_dither(s)[2], state.get_gain(s)["remaining"], m["samples"], m["clipped_high"], m["clipped_low"]])
    return out


def counters():
    c, m = speexhip.chunk_counters(), speexhip.many_counters()
    return [c[k] for k in sorted(c)] + [m[k] for k in sorted(m)]


def run_case(form, case):
    pair, flags = case.split("/")
    frames, present = FRAMES, True
    if flags in ("empty", "null"):
        frames, present, flags = (0, True, "----") if flags == "empty" else (FRAMES, False, "----")
    apart = flags[3] == "a"
    mode = speexhip.MODE_FAST_FIXED
    before = counters()
    got = {}
    if form in ("device", "bus") and not apart:
        b = speexhip.Batch(STREAMS, CH, FI, FO, Q, mode=mode)
        if form == "bus":
            assert b.set_buses(WEIGHTS) == 0  # (first: it zeroes the bus position that set_dither sets)
        prepare(b, flags, True)
        if form == "bus":
            sides = Sides(pair, True, STREAMS, out_items=2, frames=frames, present=present)
            rc, used, made, bus_frames = b.bus_call(sides.a, frames, sides.b, CAP)
            got["bus"] = [bus_frames, b.bus_position()] + [[m["samples"], m["clipped_high"], m["clipped_low"]]
                                                           for m in (b.get_bus_meter(j) for j in range(2))]
        else:
            sides = Sides(pair, True, STREAMS, frames=frames, present=present)
            try:
                used, made = b.process_sides_device(sides.a, frames, sides.b, CAP)
                rc = 0
            except RuntimeError as e:
                rc, used, made = str(e), [], []
        got.update(rc=rc, used=list(used), made=list(made), sha1=sides.digest(), state=readout(b, STREAMS))
        b.close()
    elif form == "many":
        states = [speexhip.Resampler(CH, FI, FO, Q, mode=mode) for _ in range(2)]
        for r in states:
            prepare(r, flags, False)
        order = [states[0], states[1], states[0]]
        sides = [Sides(pair, False, seed=10 * i, frames=frames, present=present) for i in range(3)]
        rc, used, made, codes = speexhip.process_many_sides(order, [s.a for s in sides], [frames] * 3, [s.b for s in sides], [CAP] * 3)
        got.update(rc=[rc] + codes, used=used, made=made, sha1=[s.digest() for s in sides], state=[readout(r)[0] for r in states])
        for r in states:
            r.close()
    else:
        r = speexhip.Resampler(CH, FI, FO, Q, mode=mode)
        prepare(r, flags, False)
        if form == "device":  # (channels apart: a state of one stream)
            sides = Sides(pair, True, frames=frames, present=present)
            try:
                used, made = r.process_sides_device(sides.a, frames, sides.b, CAP)
                rc = 0
            except RuntimeError as e:
                rc, used, made = str(e), 0, 0
        elif form == "chunks":
            sides = Sides(pair, False, frames=sum(CHUNKS), present=present)
            lens = [0, 0, 0] if frames == 0 else list(CHUNKS)
            ptrs, off = [], 0
            for n in CHUNKS:
                ptrs += [sides.in_ptr + p * sides.in_plane_bytes + off * sides.in_frame_bytes if present else None
                         for p in range(sides.in_planes)]
                off += n
            rc, used, made = r.process_chunks_sides(sides.a, ptrs, lens, sides.b, list(CHUNK_CAPS))
        else:
            sides = Sides(pair, False, frames=frames, present=present, separate_out=form == "planes_host")
            il, ol = C.c_uint32(frames), C.c_uint32(CAP)
            rc = speexhip.lib().speexhip_resampler_process_sides(r._h, C.byref(sides.a), C.byref(il), C.byref(sides.b), C.byref(ol))
            used, made = il.value, ol.value
        got.update(rc=rc, used=used, made=made, sha1=sides.digest(), state=readout(r))
        r.close()
    got["counters"] = [x - y for x, y in zip(counters(), before)]
    return got


@pytest.mark.parametrize("form", FORMS)
def test_every_route_does_what_it_did_before_the_rule(form):
    got = {case: run_case(form, case) for case in case_ids(form)}
    got = json.loads(json.dumps(got))  # (tuples and numpy integers as the file holds them)
    if RECORD:
        held = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                held = json.load(f)
        held[form] = got
        with open(RECORD, "w") as f:
            json.dump(held, f, indent=0, sort_keys=True)
        return
    with open(GOLDEN) as f:
        want = json.load(f)[form]
    assert sorted(got) == sorted(want)
    wrong = ["%s: %s, recorded %s" % (case, got[case], want[case]) for case in sorted(got) if got[case] != want[case]]
    assert not wrong, "%d of %d cases differ:\n%s" % (len(wrong), len(got), "\n".join(wrong[:20]))
