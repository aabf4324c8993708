"""The mixer's levels on the GPU (include/speexhip_resampler.h, "Mixer levels"), by the discipline of test_gpu_mixer.py:
the expected records never come from the call under test.  A TWIN per leg -- an identically built Resampler, never
gained -- is fed the same bytes through process_fmt(..., FMT_F32, capacity), an existing path, and levels_model.py makes
the record of the twin's floats.  Every comparison is for EQUALITY: energy is a sum of integers, peak a maximum.

Cases (the smallest shapes that reach every path of kernels_levels.hip and of the snapshot):
  A  seven mono 8k -> 16k legs, capacities 0, 1, 3, 4, 1023, 1024, 1025: no trip, a tail alone, one whole trip of 1024
     samples, a trip and a tail; samples is what the leg produced, not the bus's length; one launch; a small call.
  B  C = 3 with 53 frames, C = 7, C = 8; and one mono call of an 8k mu-law q5 leg, a 16k S16BE q7 leg, a 48k F32 q10 leg
     (the fp64 kernel) and a leg in MODE_EXACT.
  C  1024 slots x 8 frames: every 7th slot empty, one leg refused, one silent, one in the zero fallback; read back through
     windows and with struct_size 40.
  D  stereo legs that produce 32 767, 32 768, 32 769 and 100 000 frames -- 1, 1, 2 and 4 spans of 65 536 samples -- the
     peak of the longest in its last frame; two launches; a copied call.
  E  legs behind gain 0.25 over a 100-frame ramp and behind gain 0, three ticks, in two mixers, one with the levels on:
     the records are the UNGAINED twins', and nothing else of the call differs between the mixers.
  F  +inf, -inf and NaN in F32 inputs, and a leg of -0.0.
  G  F32 noise of amplitude 3 behind gain 0.25 beside a longer leg: every defect of the model changes the record on the
     twin's floats, then the library equals the right model.  Two defects need a sample of their own in that noise: a NaN,
     and a tie -- a filter's output of noise never lands on one, so the leg begins with 400 frames of a constant found by
     bisection that makes one output frame exactly 0.5.  fp32_energy needs the sum of the squares past 2^24: 8 million
     samples, 123 spans.
  H  the snapshot: overwritten by a second tick, kept by a call-level error, cleared by a change of the switch; BAD_STATE
     while off, INVALID_ARG for windows out of range."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import dither_model as dm
import levels_model as lm
import speexhip
from golden_util import ROOT

pytestmark = pytest.mark.gpu

F32, S16, ULAW, S16BE = speexhip.FMT_F32, speexhip.FMT_S16, speexhip.FMT_ULAW, speexhip.FMT_S16BE
SMALL = 720 * 1024           # host_transfer.h: a call whose pageable bytes stay below this each way runs on pinned memory
SPAN = 65536
SEED = 0x1234ABCD5678


def noise_s16(frames, ch, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, frames * ch).astype(np.int16)


def noise_f32(frames, ch, seed, amplitude=6000.0):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, frames * ch).astype(np.float32)


def close_all(*things):
    for t in things:
        for st in (t if isinstance(t, (list, tuple)) else [t]):
            if st is not None:
                st.close()


def twin_floats(twin, x, fmt, cap, null_frames=0):
    """(the flat float32 result of x in the twin, consumed, the call's code)"""
    rc, used, made, out = twin.fmt_call(None if x is None else np.asarray(x).reshape(-1).view(speexhip.fmt_dtype(fmt)), fmt, F32, cap, null_frames)
    assert rc in (0, speexhip.ERR_ALLOC_FAILED), rc
    return out[: made * twin.channels].copy(), used, rc


def mixer_of(n, ch, levels=True, n_buses=1, kind=dm.NONE, meter=False):
    m = speexhip.Mixer(n, n_buses, ch)
    if meter:
        assert m.set_meter(1) == 0
    assert m.set_weights(np.ones((n_buses, n), np.float32)) == 0
    if kind != dm.NONE:
        assert m.set_dither(kind, SEED, 77) == 0
    if levels:
        assert m.set_levels(1) == 0
    return m


def tick(m, legs, chunks, fmts, caps, out_fmt=S16):
    """one call: (buses, bus_frames, used, made, codes, the mixer counters it moved, the level launches it made)"""
    c0, l0 = speexhip.debug_mixer_counters(), speexhip.debug_mixer_level_launches()
    buses, bus_frames, used, made, codes = m.process(legs, chunks, fmts, out_fmt, caps)
    c1, l1 = speexhip.debug_mixer_counters(), speexhip.debug_mixer_level_launches()
    return buses, bus_frames, used, made, codes, {k: c1[k] - c0[k] for k in c0}, l1 - l0


def records(m, first=0, count=None):
    return [lm.of_struct(r) for r in m.get_levels(first, count)]


def check(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert lm.same(g, w), "%s, slot %d: library %r, model %r" % (what, i, g, w)


def nbytes_in(n, chunks):
    return 64 * n + sum(0 if c is None else (np.asarray(c).nbytes + 63) // 64 * 64 for c in chunks)


def nbytes_out(n, n_buses, bus_frames, ch, es, levels=True):
    return (bus_frames * ch + 63) // 64 * 64 * es * n_buses + ((32 * n + 63) // 64 * 64 if levels else 0)


# ---- A. vector tails and the one-trip edge --------------------------------------------------------------------------------
CAPS_A = (0, 1, 3, 4, 1023, 1024, 1025)


def test_a_tails_and_the_one_trip_edge():
    n = len(CAPS_A)
    chunks = [noise_s16(1000, 1, 100 + i) for i in range(n)]
    legs, twins = [speexhip.Resampler(1, 8000, 16000, 5) for _ in range(n)], [speexhip.Resampler(1, 8000, 16000, 5) for _ in range(n)]
    m = mixer_of(n, 1)
    try:
        # (a fresh state's first frames are the filter's run-in, next to nothing: every state has run before, so that a
        #  leg of one frame is one frame of signal)
        for i, st in enumerate(legs + twins):
            st.process_fmt(noise_s16(300, 1, 90 + i % n), S16, F32, 600)
        ys = [twin_floats(twins[i], chunks[i], S16, CAPS_A[i])[0] for i in range(n)]
        assert [y.size for y in ys] == list(CAPS_A), "plenty of input: every twin fills its capacity"
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, chunks, S16, list(CAPS_A))
        assert codes == [0] * n and made == list(CAPS_A) and bus_frames == 1025
        want = [lm.record(y) for y in ys]
        assert [w["samples"] for w in want] == list(CAPS_A) and all(w["energy"] > 0 for w in want[1:])
        check(records(m), want, "A")
        # (I) a small call: both byte sums stay under the limit, the records lie in the pinned stage; one launch, and the
        # transfers of the call are what they are without the levels
        assert nbytes_in(n, chunks) < SMALL and nbytes_out(n, 1, bus_frames, 1, 2) < SMALL
        assert launches == 1 and (d["transfers_in"], d["transfers_out"], d["bus_sum_launches"], d["fir_launches"]) == (1, 1, 1, 1), d
    finally:
        close_all(m, legs, twins)


# ---- B. channel counts, formats, qualities and modes ---------------------------------------------------------------------
@pytest.mark.parametrize("ch,frames", ((3, 53), (7, 300), (8, 300)))
def test_b_channel_counts(ch, frames):
    n = 3
    chunks = [noise_f32(frames, ch, 200 + 10 * ch + i) for i in range(n)]
    caps = [frames * 2] * n
    legs, twins = [speexhip.Resampler(ch, 44100, 48000, 7) for _ in range(n)], [speexhip.Resampler(ch, 44100, 48000, 7) for _ in range(n)]
    m = mixer_of(n, ch)
    try:
        ys = [twin_floats(twins[i], chunks[i], F32, caps[i])[0] for i in range(n)]
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, chunks, F32, caps)
        assert codes == [0] * n and [y.size for y in ys] == [f * ch for f in made] and min(made) > 0
        check(records(m), [lm.record(y) for y in ys], "B, %d channels" % ch)
        assert launches == 1
    finally:
        close_all(m, legs, twins)


def test_b_formats_qualities_and_modes_in_one_call():
    kinds = ((8000, 5, ULAW, 160, None), (16000, 7, S16BE, 320, None), (48000, 10, F32, 960, None), (16000, 7, S16BE, 320, speexhip.MODE_EXACT))
    n = len(kinds)
    chunks = []
    for i, (rate, q, fmt, frames, mode) in enumerate(kinds):
        chunks.append(noise_f32(frames, 1, 300 + i) if fmt == F32 else np.random.default_rng(300 + i).integers(0, 256, frames * speexhip.fmt_bytes(fmt)).astype(np.uint8))
    fmts, caps = [k[2] for k in kinds], [1100] * n
    legs = [speexhip.Resampler(1, k[0], 48000, k[1], mode=k[4]) for k in kinds]
    twins = [speexhip.Resampler(1, k[0], 48000, k[1], mode=k[4]) for k in kinds]
    m = mixer_of(n, 1)
    try:
        ys = [twin_floats(twins[i], chunks[i], fmts[i], caps[i])[0] for i in range(n)]
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, chunks, fmts, caps)
        assert codes == [0] * n and made == [y.size for y in ys] and min(made) > 0
        assert d["fir_launches"] >= 3, "the qualities and the modes did not take launches of their own"
        check(records(m), [lm.record(y) for y in ys], "B, mixed")
    finally:
        close_all(m, legs, twins)


# ---- C. the grid's edge: 1024 slots -----------------------------------------------------------------------------------------
REFUSED, SILENT, ZEROED = 3, 10, 17


def raw_levels(m, first, count, struct_size):
    buf = np.full(max(count, 1) * struct_size, 0xAB, np.uint8)
    rc = speexhip.lib().speexhip_mixer_get_levels(m._h, first, count, C.c_void_p(buf.ctypes.data), struct_size)
    return rc, buf[: count * struct_size].reshape(count, struct_size)


def test_c_1024_slots_of_every_kind():
    n, frames, cap = speexhip.MIXER_MAX_LEGS, 8, 40
    empty = [i % 7 == 6 for i in range(n)]
    assert not (empty[REFUSED] or empty[SILENT] or empty[ZEROED])
    legs, twins = [], []
    for i in range(n):
        ch = 2 if i == REFUSED else 1
        legs.append(None if empty[i] else speexhip.Resampler(ch, 8000, 16000, 5))
        twins.append(None if empty[i] or i == REFUSED else speexhip.Resampler(1, 8000, 16000, 5))
    m = mixer_of(n, 1)
    try:
        for st in (legs[ZEROED], twins[ZEROED]):
            speexhip.lib().speexhip_debug_fail_device_allocs(1)
            rc = st.set_rate(8000, 24000)
            speexhip.lib().speexhip_debug_fail_device_allocs(0)
            assert rc == speexhip.ERR_ALLOC_FAILED
        chunks = [None if empty[i] or i == SILENT else noise_s16(frames, 2 if i == REFUSED else 1, 1000 + i) for i in range(n)]
        caps = [(frames, cap) if i == SILENT else cap for i in range(n)]
        want = []
        for i in range(n):
            if twins[i] is None:
                want.append(dict(lm.ZERO))
                continue
            y, used, rc = twin_floats(twins[i], chunks[i], S16, cap, frames)
            assert (rc == speexhip.ERR_ALLOC_FAILED) == (i == ZEROED)
            want.append(lm.record(y))
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, chunks, S16, caps)
        assert codes[REFUSED] == speexhip.ERR_INVALID_ARG and codes[ZEROED] == speexhip.ERR_ALLOC_FAILED
        assert all(c == 0 for i, c in enumerate(codes) if i not in (REFUSED, ZEROED))
        for i in (SILENT, ZEROED):
            assert want[i]["samples"] == made[i] > 0 and want[i]["energy"] == 0 and want[i]["peak"] == 0, "slot %d of the model" % i
        assert [w["samples"] for w in want] == [0 if empty[i] or i == REFUSED else made[i] for i in range(n)]
        assert launches == 1 and d["bus_sum_launches"] == 1 and d["transfers_out"] == 1
        check(records(m), want, "C")
        # windows, and records 40 bytes apart: the first 32 of each written, the rest untouched
        for first, count in ((0, 1), (1023, 1), (5, 13), (1000, 24), (0, 0), (1024, 0)):
            check(records(m, first, count), want[first: first + count], "C, window %d + %d" % (first, count))
        rc, raw = raw_levels(m, 2, 20, 40)
        assert rc == 0 and (raw[:, 32:] == 0xAB).all()
        check([lm.of_struct(r) for r in np.ascontiguousarray(raw[:, :32]).view(speexhip.LEVEL_DTYPE).reshape(-1)], want[2:22], "C, struct_size 40")
    finally:
        speexhip.lib().speexhip_debug_fail_device_allocs(0)
        close_all(m, legs, twins)


# ---- D. span crossing ---------------------------------------------------------------------------------------------------------
FRAMES_D = (32767, 32768, 32769, 100000)


@functools.lru_cache(maxsize=None)
def spans_case():
    """24k -> 48k stereo: an impulse at input frame p peaks at output frame 2 p + d.  One probe finds d; the longest leg's
    input then carries one impulse, or two neighbours whose common maximum lies between them, so that its largest |y| is
    its LAST output frame.  (chunks, the twins' floats)"""
    last = FRAMES_D[-1] - 1
    in_frames = [f // 2 + 64 for f in FRAMES_D]
    probe = np.zeros((in_frames[-1], 2), np.float32)
    probe[40000] = 20000.0
    t = speexhip.Resampler(2, 24000, 48000, 5)
    y = twin_floats(t, probe, F32, FRAMES_D[-1])[0].reshape(-1, 2)
    t.close()
    d = int(np.abs(y[:, 0]).argmax()) - 2 * 40000
    chunks = [noise_f32(f, 2, 400 + i, 100.0).reshape(f, 2) for i, f in enumerate(in_frames)]
    p = (last - d) // 2
    chunks[-1][p] += 20000.0
    if (last - d) % 2:
        chunks[-1][p + 1] += 20000.0
    ys = []
    for i, f in enumerate(FRAMES_D):
        t = speexhip.Resampler(2, 24000, 48000, 5)
        ys.append(twin_floats(t, chunks[i], F32, f)[0])
        t.close()
    for a in chunks + ys:
        a.setflags(write=False)
    return tuple(chunks), tuple(ys)


def test_d_legs_of_one_two_and_four_spans():
    chunks, ys = spans_case()
    n = len(FRAMES_D)
    assert [y.size for y in ys] == [2 * f for f in FRAMES_D]
    assert [-(-y.size // SPAN) for y in ys] == [1, 1, 2, 4]
    assert int(np.abs(ys[-1]).argmax()) // 2 == FRAMES_D[-1] - 1, "the longest leg's peak is not in its last frame"
    legs = [speexhip.Resampler(2, 24000, 48000, 5) for _ in range(n)]
    m = mixer_of(n, 2)
    try:
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, list(chunks), F32, list(FRAMES_D))
        assert codes == [0] * n and made == list(FRAMES_D) and bus_frames == FRAMES_D[-1]
        want = [lm.record(y) for y in ys]
        assert want[-1]["peak"] == np.abs(ys[-1][-2:]).max() > 10000
        check(records(m), want, "D")
        # (I) a copied call: the payloads alone are past the limit; the records leave in the one copy out the buses make
        assert nbytes_in(n, chunks) >= SMALL
        assert launches == 2 and (d["transfers_out"], d["bus_sum_launches"]) == (1, 1), d
        assert d["transfers_in"] == 1 + sum(c.nbytes >= 256 * 1024 for c in chunks), d
    finally:
        close_all(m, legs)


# ---- E. pre-gain, and nothing else of the call changes ------------------------------------------------------------------------
def test_e_gained_legs_read_ungained_and_the_buses_do_not_change():
    n, frames, cap, kind = 4, 320, 700, dm.TRIANGULAR
    gains = ((0.25, 100), (0.0, 0), None, (0.25, 100))
    mixers = [mixer_of(n, 1, levels=on, n_buses=2, kind=kind, meter=True) for on in (True, False)]
    sets = [[speexhip.Resampler(1, 16000, 48000, 7) for _ in range(n)] for _ in range(3)]      # on, off, the ungained twins
    try:
        for legs in sets[:2]:
            for st, g in zip(legs, gains):
                if g is not None:
                    assert st.set_gain(*g) == 0
        position = 77
        for t in range(3):
            chunks = [noise_s16(frames, 1, 500 + 10 * t + i) for i in range(n)]
            ys = [twin_floats(sets[2][i], chunks[i], S16, cap)[0] for i in range(n)]
            runs = [tick(mixers[k], sets[k], chunks, S16, cap) for k in range(2)]
            (b0, f0, u0, m0, c0, d0, l0), (b1, f1, u1, m1, c1, d1, l1) = runs
            assert b0.tobytes() == b1.tobytes() and (f0, u0, m0, c0) == (f1, u1, m1, c1) and c0 == [0] * n
            assert d0 == d1 and (l0, l1) == (1, 0), "the six counters differ, or the levels' launches are not apart"
            position += f0
            assert mixers[0].get_dither() == mixers[1].get_dither() and mixers[0].bus_position() == position and f0 > 0
            for j in range(2):
                assert mixers[0].get_bus_meter(j) == mixers[1].get_bus_meter(j)
            want = [lm.record(y) for y in ys]
            assert m0 == [y.size for y in ys] and all(w["energy"] > 0 for w in want)
            check(records(mixers[0]), want, "E, tick %d" % t)
            # (the muted leg reads as loud as its ungained twin: post-gain it would be silence)
            assert lm.record(ys[1], defect="post_gain", gain=np.float32(0.0))["energy"] == 0
        for a, b in zip(sets[0], sets[1]):
            assert a.get_gain() == b.get_gain()
    finally:
        close_all(mixers, *sets)


# ---- F. values that are no numbers ----------------------------------------------------------------------------------------------
def test_f_infinities_nan_and_negative_zero():
    n, frames, cap = 4, 400, 900
    chunks = [noise_f32(frames, 1, 600 + i) for i in range(3)] + [np.full(frames, -0.0, np.float32)]
    chunks[0][200], chunks[1][200], chunks[2][200] = np.inf, -np.inf, np.nan
    legs, twins = [speexhip.Resampler(1, 16000, 32000, 5) for _ in range(n)], [speexhip.Resampler(1, 16000, 32000, 5) for _ in range(n)]
    m = mixer_of(n, 1)
    try:
        ys = [twin_floats(twins[i], chunks[i], F32, cap)[0] for i in range(n)]
        want = [lm.record(y) for y in ys]
        assert np.isinf(want[0]["peak"]) and np.isinf(want[1]["peak"]) and want[2]["nan"] > 0 and want[2]["nan"] < ys[2].size
        assert (ys[0] == np.inf).any() and (ys[1] == -np.inf).any(), "no infinity of either sign reaches a rail"
        assert want[0]["energy"] >= 32767 ** 2 and want[3] == {"samples": ys[3].size, "energy": 0, "nan": 0, "peak": np.float32(0.0)}
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, chunks, F32, cap, out_fmt=F32)
        assert codes == [0] * n and made == [y.size for y in ys]
        got = records(m)
        check(got, want, "F")
        assert not np.signbit(got[3]["peak"])
    finally:
        close_all(m, legs, twins)


# ---- G. the rounding rule and the pre-gain rule, on data where they matter --------------------------------------------------------
G_FRAMES = 7_400_000        # fp32_energy shows only once the sum of the steps' squares -- about 2.9 a sample -- is past 2^24


LEAD, TIE_AT = 400, 350     # output frame 350 of a fresh 44.1k -> 48k q5 state reads input frames of the lead-in alone


def tie_lead_in():
    """A tie is a single float: no filter's output of noise lands on one (about 1e-7 a sample at this amplitude), and
    half_even differs from the rule on ties alone.  So the noise leg begins with LEAD frames of one constant c, found
    here by bisection over the bits of c, such that output frame TIE_AT of a fresh twin is EXACTLY 0.5 -- the rule's step
    there is 1, half_even's 0.  (c, the tries)"""
    def out_of(bits):
        t = speexhip.Resampler(1, 44100, 48000, 5)
        y = twin_floats(t, np.full(LEAD, np.uint32(bits).view(np.float32), np.float32), F32, TIE_AT + 1)[0]
        t.close()
        assert y.size == TIE_AT + 1
        return y[TIE_AT]
    lo, hi = int(np.float32(0.3).view(np.uint32)), int(np.float32(0.8).view(np.uint32))
    assert out_of(lo) < 0.5 < out_of(hi)
    tries = 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        tries += 1
        if out_of(mid) < 0.5:
            lo = mid
        else:
            hi = mid
    for bits in range(hi - 8, hi + 9):
        tries += 1
        if out_of(bits) == np.float32(0.5):
            return np.uint32(bits).view(np.float32), tries
    raise AssertionError("no constant in %d ulps of %r makes output frame %d a tie" % (8, np.uint32(hi).view(np.float32), TIE_AT))


@functools.lru_cache(maxsize=None)
def noise_case():
    """mono 44.1k -> 48k: (the input of the noise leg, its twin's floats, its capacity).  The input is the lead-in of
    tie_lead_in and then uniform noise of amplitude 3, whose sign is chosen so that the largest |y| is a NEGATIVE value:
    signed_peak can show."""
    c, tries = tie_lead_in()
    print("G: a lead-in of %d frames of %r makes output frame %d a tie (%d tries)" % (LEAD, c, TIE_AT, tries))
    noise = noise_f32(G_FRAMES, 1, 700, 3.0)
    noise[-5000] = np.nan       # (and one value that is no number: it spreads over a filter's length of output frames)
    cap = (LEAD + G_FRAMES) * 48000 // 44100 - 1000
    for sign in (1.0, -1.0):
        x = np.concatenate([np.full(LEAD, c, np.float32), noise * np.float32(sign)])
        t = speexhip.Resampler(1, 44100, 48000, 5)
        y = twin_floats(t, x, F32, cap)[0]
        t.close()
        if -np.nanmin(y) > np.nanmax(y):
            break
    assert y[TIE_AT] == np.float32(0.5)
    x.setflags(write=False), y.setflags(write=False)
    return x, y, cap


def test_g_every_defect_shows_on_the_twins_floats_and_the_library_is_the_rule():
    x, y, cap = noise_case()
    gain = np.float32(0.25)
    right = lm.record(y)
    assert y.size == cap and np.nanmax(np.abs(y)) < 8 and -np.nanmin(y) > np.nanmax(y) and 0 < np.isnan(y).sum() < 1000
    legs = [speexhip.Resampler(1, 44100, 48000, 5) for _ in range(2)]
    assert legs[0].set_gain(float(gain), 0) == 0
    m = mixer_of(2, 1)
    try:
        # (the longer leg is present and silent: it costs no payload, and the bus is longer than the noise)
        buses, bus_frames, used, made, codes, d, launches = tick(m, legs, [x, None], F32, [cap, (LEAD + G_FRAMES + 4410, cap + 4800)])
        assert codes == [0, 0] and made[0] == cap and bus_frames == made[1] > cap
        for defect in lm.DEFECTS:
            wrong = lm.record(y, defect=defect, gain=gain, padded=bus_frames)
            fields = lm.changed(wrong, right)
            print("G %-20s: %s change (energy %d -> %d)" % (defect, ", ".join(fields) or "NOTHING", right["energy"], wrong["energy"]))
            assert fields, "the defect %s does not show on this case's floats" % defect
        got = records(m)[0]
        assert lm.same(got, right), "G: library %r, model %r" % (got, right)
        assert launches == 2
    finally:
        close_all(m, legs)


def test_g_a_nan_among_the_noise_is_counted_and_is_no_zero_sample():
    # (the one defect finite noise cannot show: the same noise, short, with NaNs in the input)
    x = noise_f32(2000, 1, 702, 3.0)
    x[::250] = np.nan
    leg, twin = speexhip.Resampler(1, 44100, 48000, 5), speexhip.Resampler(1, 44100, 48000, 5)
    m = mixer_of(1, 1)
    try:
        y = twin_floats(twin, x, F32, 2100)[0]
        right, wrong = lm.record(y), lm.record(y, defect="nan_as_zero_sample")
        assert lm.changed(wrong, right) == ("nan",) and 0 < right["nan"] < y.size
        tick(m, [leg], [x], F32, 2100, out_fmt=F32)
        check(records(m), [right], "G, NaN")
    finally:
        close_all(m, leg, twin)


# ---- H. the snapshot --------------------------------------------------------------------------------------------------------------
def test_h_the_snapshot():
    n, frames, cap = 3, 160, 400
    legs, twins = [speexhip.Resampler(1, 8000, 16000, 5) for _ in range(n)], [speexhip.Resampler(1, 8000, 16000, 5) for _ in range(n)]
    m = mixer_of(n, 1, levels=False)
    L = speexhip.lib()
    zeros = [dict(lm.ZERO)] * n
    try:
        # off: BAD_STATE, whatever the call before it; arguments are checked first
        rec = np.zeros(n, speexhip.LEVEL_DTYPE)
        ptr = C.c_void_p(rec.ctypes.data)
        assert L.speexhip_mixer_get_levels(m._h, 0, n, ptr, 32) == speexhip.ERR_BAD_STATE
        assert L.speexhip_mixer_get_levels(m._h, 0, n, None, 32) == speexhip.ERR_INVALID_ARG
        assert L.speexhip_mixer_set_levels(m._h, 2) == speexhip.ERR_INVALID_ARG and L.speexhip_mixer_set_levels(m._h, -1) == speexhip.ERR_INVALID_ARG
        chunks = [noise_s16(frames, 1, 800 + i) for i in range(n)]
        ys = [twin_floats(twins[i], chunks[i], S16, cap)[0] for i in range(n)]
        *_, d, launches = tick(m, legs, chunks, S16, cap)
        assert launches == 0 and L.speexhip_mixer_get_levels(m._h, 0, n, ptr, 32) == speexhip.ERR_BAD_STATE
        # on: zeros before any call
        assert m.set_levels(1) == 0
        check(records(m), zeros, "H, before any call")
        for first, count, size in ((0, n + 1, 32), (n, 1, 32), (n + 1, 0, 32), (1, 0xFFFFFFFF, 32), (0, n, 31), (0, n, 0)):
            assert L.speexhip_mixer_get_levels(m._h, first, count, ptr, size) == speexhip.ERR_INVALID_ARG, (first, count, size)
        # a tick, and a second one that overwrites it
        for t in (1, 2):
            chunks = [noise_s16(frames, 1, 800 + 10 * t + i) for i in range(n)]
            ys = [twin_floats(twins[i], chunks[i], S16, cap)[0] for i in range(n)]
            *_, d, launches = tick(m, legs, chunks, S16, cap)
            want = [lm.record(y) for y in ys]
            check(records(m), want, "H, tick %d" % t)
        # control calls of the buses do not touch it; setting the switch to what it is does not either
        assert m.set_meter(1) == 0 and m.set_dither(dm.TRIANGULAR, 5, 9) == 0 and m.set_weights(np.full((1, n), 0.5, np.float32)) == 0
        assert m.set_levels(1) == 0
        check(records(m), want, "H, behind control calls")
        # a call-level error -- bus_frames == NULL -- touches nothing
        hs = (C.c_void_p * n)(*[st._h for st in legs])
        sides = (speexhip.Side * n)()
        for i in range(n):
            C.memmove(C.byref(sides[i]), C.byref(speexhip.make_side(S16, 1, data=chunks[i].ctypes.data)), C.sizeof(speexhip.Side))
        il, ol, codes = (C.c_uint32 * n)(*[frames] * n), (C.c_uint32 * n)(*[cap] * n), (C.c_int * n)()
        out = np.zeros(cap, np.int16)
        out_side = speexhip.make_side(S16, 1, data=out.ctypes.data, stream_stride=cap)
        assert L.speexhip_mixer_process(m._h, hs, sides, il, ol, C.byref(out_side), None, codes) == speexhip.ERR_INVALID_ARG
        assert list(il) == [frames] * n and list(ol) == [cap] * n
        check(records(m), want, "H, behind a call-level error")
        # a call in which nothing is produced: bus_frames 0, nothing launched, zeros
        *_, bus_frames, used, made, codes2, d, launches = tick(m, legs, [np.zeros(0, np.int16)] * n, S16, cap)
        assert bus_frames == 0 and launches == 0
        check(records(m), zeros, "H, behind an empty call")
        # a change of the switch clears it
        *_, d, launches = tick(m, legs, chunks, S16, cap)
        assert launches == 1 and records(m)[0]["samples"] > 0
        assert m.set_levels(0) == 0 and L.speexhip_mixer_get_levels(m._h, 0, n, ptr, 32) == speexhip.ERR_BAD_STATE
        assert m.set_levels(1) == 0
        check(records(m), zeros, "H, behind off and on")
    finally:
        close_all(m, legs, twins)


# ---- Node ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_mixer_levels():
    pkg = os.path.join(ROOT, "node-speex-resampler_amd")
    run = subprocess.run(["node", os.path.join(pkg, "test", "test_mixer_levels.js")], capture_output=True, text=True, timeout=300, cwd=pkg)
    assert run.returncode == 0 and "mixer levels ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
