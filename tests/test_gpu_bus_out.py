"""The buses of a Batch and the buses of a Mixer leave the device through one output stage (csrc/bus_out.h): the same
streams behind the same W, dither, meter and gain give the same bytes, lengths, position and totals through either call.
Neither call is the other's reference elsewhere -- test_gpu_bus.py and test_gpu_mixer.py hold each to bus_model.py -- so
equality here says that the two agree tick by tick, which the header promises and nothing else compares.

Shapes: 3 streams x 2 channels, 44.1k -> 48k q3, 5 buses (mix-minus and the sum of everything), three ticks of 441
frames, the last with stream 2 fed nothing: about 480 output frames a tick, under one tile, and a stream that ends before
the bus does.  Sides: the converting pass, the plane pass, no pass (meter_image) and the float plane pass."""
import functools

import numpy as np
import pytest

import bus_model as bm
import speexhip

pytestmark = pytest.mark.gpu

F32, F32N, S16, S24 = speexhip.FMT_F32, speexhip.FMT_F32N, speexhip.FMT_S16, speexhip.FMT_S24
INTER, PLANAR = speexhip.LAYOUT_INTERLEAVED, speexhip.LAYOUT_PLANAR
N, CH, BUSES, FRAMES, CAP = 3, 2, 5, 441, 544
KEY = (44100, 48000, 3)
SEED, START = 0x0DDBA11C0FFEE123, 977
W = np.concatenate([bm.mix_minus(N), np.ones((1, N), np.float32), np.ones((1, N), np.float32)]).astype(np.float32)
FED = ((FRAMES,) * N, (FRAMES,) * N, (FRAMES, FRAMES, 0))
SIDES = {"s16": (S16, INTER), "s24_planar": (S24, PLANAR), "f32": (F32, INTER), "f32n_planar": (F32N, PLANAR)}


@functools.lru_cache(maxsize=None)
def ticks():
    """(tick, stream, frames * channels) float32 within +-0.9 of full scale: three streams sum beyond the rails"""
    x = np.random.default_rng(2024).uniform(-0.9, 0.9, (len(FED), N, FRAMES * CH)).astype(np.float32)
    x.setflags(write=False)
    return x


def set_up(obj, weights_call):
    assert obj.set_dither(speexhip.DITHER_TRIANGULAR, SEED, START) == 0
    assert obj.set_meter(1) == 0
    assert weights_call(W) == 0
    assert obj.set_dither(speexhip.DITHER_TRIANGULAR, SEED, START) == 0   # (the weights zeroed the position)


def batch_tick(b, x, fed, fmt, layout):
    """one bus call of the batch on device buffers: (bytes per bus, bus_frames, produced per stream)"""
    import torch
    es = speexhip.fmt_bytes(fmt)
    t_in = torch.from_numpy(x.copy()).cuda()
    t_out = torch.zeros(BUSES * CAP * CH * es, dtype=torch.uint8, device="cuda")
    a = speexhip.make_side(F32N, CH, INTER, None, t_in.data_ptr(), 0, FRAMES * CH)
    o = speexhip.make_side(fmt, CH, layout, None, t_out.data_ptr(), CAP, CAP * CH)
    used, made, bus_frames = b.process_bus_device(a, list(fed), o, CAP)
    torch.cuda.synchronize()
    assert used == list(fed)
    raw = t_out.cpu().numpy()
    if layout == INTER:
        got = raw.reshape(BUSES, CAP * CH * es)[:, : bus_frames * CH * es]
    else:
        got = raw.reshape(BUSES, CH, CAP * es)[:, :, : bus_frames * es].reshape(BUSES, -1)
    return got.tobytes(), bus_frames, made


def mixer_tick(mx, legs, x, fed, fmt, layout):
    chunks = [x[s, : fed[s] * CH].tobytes() for s in range(N)]
    buses, bus_frames, used, made, codes = mx.process(legs, chunks, F32N, fmt, CAP, "planar" if layout == PLANAR else "interleaved")
    assert codes == [0] * N and used == list(fed)
    return np.ascontiguousarray(buses).view(np.uint8).reshape(BUSES, -1).tobytes(), bus_frames, made


@pytest.mark.parametrize("side", sorted(SIDES))
def test_a_batch_and_a_mixer_give_the_same_buses_position_and_totals(side):
    fmt, layout = SIDES[side]
    b = speexhip.Batch(N, CH, *KEY)
    legs = [speexhip.Resampler(CH, *KEY) for _ in range(N)]
    mx = speexhip.Mixer(N, BUSES, CH)
    try:
        set_up(b, b.set_buses)
        set_up(mx, mx.set_weights)
        assert b.set_gain(0.5, 64, stream=1) == 0 and legs[1].set_gain(0.5, 64) == 0
        assert b.bus_position() == START == mx.bus_position()
        total = 0
        for k, fed in enumerate(FED):
            got_b, frames_b, made_b = batch_tick(b, ticks()[k], fed, fmt, layout)
            got_m, frames_m, made_m = mixer_tick(mx, legs, ticks()[k], fed, fmt, layout)
            assert frames_b == frames_m and frames_b > 0, "tick %d" % k
            assert made_b == made_m, "tick %d" % k
            assert got_b == got_m, "tick %d: the buses' bytes differ" % k
            assert b.bus_position() == mx.bus_position(), "tick %d" % k
            for j in range(BUSES):
                mb, mm = b.get_bus_meter(j), mx.get_bus_meter(j)
                assert mb == mm and mb["on"] == 1 and mb["samples"] > 0, "tick %d bus %d: %r, %r" % (k, j, mb, mm)
            total += frames_b
        assert made_b[2] < made_b[0], "stream 2 was to end before the bus"
        assert b.bus_position() == START + total      # (the position counts frames whatever the format)
        assert b.get_bus_meter(BUSES - 1)["peak"] > 0
        # reset of one bus: that bus's totals are zero, its neighbour's untouched, in both
        before = b.get_bus_meter(3)
        for obj in (b, mx):
            was = obj.get_bus_meter(2, reset=True)
            assert was["samples"] > 0
            now = obj.get_bus_meter(2)
            assert (now["samples"], now["clipped_high"], now["clipped_low"], now["nan"], now["peak"]) == (0, 0, 0, 0, 0.0)
            assert obj.get_bus_meter(3) == before
        # the weights again: position and totals zero, in both
        assert b.set_buses(W) == 0 and mx.set_weights(W) == 0
        for obj in (b, mx):
            assert obj.bus_position() == 0
            for j in range(BUSES):
                m = obj.get_bus_meter(j)
                assert (m["samples"], m["clipped_high"], m["clipped_low"], m["nan"], m["peak"]) == (0, 0, 0, 0, 0.0)
    finally:
        mx.close()
        b.close()
        for s_ in legs:
            s_.close()
