"""The mixer on the host (include/speexhip_resampler.h, "Mixer"): the header declares its eleven entry points and its two
limits, the Makefile names its units, the Python binding exports every symbol -- and the sum itself, which the mixer's
kernel compiles from csrc/bus.h as bus_sum does, still equals the numpy model (bus_model.py) bit for bit at a width no
Batch reaches: 41 slots x 41 buses, one more than a pack of 32 on both sides with a ragged group of one bus, on the
"order" layout of bus_model.py widened to 41 streams.  Every order defect the model can plant changes some bus there (the
shares are printed with -s).  No GPU."""
import os
import re

import numpy as np

import bus_model as bm
import speexhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INT_CALLS = ("speexhip_mixer_set_weights", "speexhip_mixer_get_weights", "speexhip_mixer_set_dither", "speexhip_mixer_get_dither",
             "speexhip_mixer_set_meter", "speexhip_mixer_get_bus_meter", "speexhip_mixer_process")
ALL = ("speexhip_mixer_init", "speexhip_mixer_init_on", "speexhip_mixer_destroy") + INT_CALLS + ("speexhip_debug_mixer_counters",)
N = 41


def header():
    with open(os.path.join(ROOT, "include", "speexhip_resampler.h")) as f:
        return f.read()


def test_the_header_declares_the_eleven_symbols_and_the_two_limits():
    text = header()
    assert len(ALL) == 11
    for name in INT_CALLS:
        assert re.search(r"SPEEXHIP_API int %s\(SpeexHipMixer \*m" % name, text), "the header does not declare " + name
    assert re.search(r"SPEEXHIP_API SpeexHipMixer \*speexhip_mixer_init\(uint32_t n_legs, uint32_t n_buses, uint32_t channels, int \*err\)", text)
    assert re.search(r"SPEEXHIP_API SpeexHipMixer \*speexhip_mixer_init_on\(int device, uint32_t n_legs", text)
    assert re.search(r"SPEEXHIP_API void speexhip_mixer_destroy\(SpeexHipMixer \*m\)", text)
    assert re.search(r"SPEEXHIP_API void speexhip_debug_mixer_counters\(uint64_t out\[6\]\)", text)
    assert re.search(r"typedef struct SpeexHipMixer_ SpeexHipMixer;", text)
    assert re.search(r"#define SPEEXHIP_MIXER_MAX_LEGS\s+1024\b", text) and re.search(r"#define SPEEXHIP_MIXER_MAX_BUSES\s+1024\b", text)
    assert speexhip.MIXER_MAX_LEGS == speexhip.MIXER_MAX_BUSES == 1024
    # the sentence that ended the bus work stays, and the pointer to this section follows it
    at = text.index("A host-fed bus call and a bus over many separate states are not part of this version.")
    assert '"Mixer"' in text[at: at + 300]


def test_the_library_and_the_binding_export_them():
    L = speexhip.lib()
    for name in ALL:
        assert name in speexhip.EXPORTS and getattr(L, name)
    # NULL handles: an argument error, never a crash (host only: nothing here reaches a device)
    assert L.speexhip_mixer_set_weights(None, None) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_get_weights(None, None) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_set_dither(None, 0, 0, 0) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_get_dither(None, None, None, None) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_set_meter(None, 1) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_get_bus_meter(None, 0, None, 0) == speexhip.ERR_INVALID_ARG
    assert L.speexhip_mixer_process(None, None, None, None, None, None, None, None) == speexhip.ERR_INVALID_ARG
    L.speexhip_mixer_destroy(None)
    counters = speexhip.debug_mixer_counters()
    assert list(counters) == ["fir_launches", "in_passes", "bus_sum_launches", "out_passes", "transfers_in", "transfers_out"]
    assert all(isinstance(v, int) and v >= 0 for v in counters.values())
    for name in ("set_weights", "get_weights", "set_dither", "get_dither", "set_meter", "get_bus_meter", "bus_position", "close",
                 "process"):
        assert callable(getattr(speexhip.Mixer, name))


def test_the_makefile_names_the_new_units():
    with open(os.path.join(ROOT, "node-speex-resampler_amd", "Makefile")) as f:
        text = f.read()
    src = text[text.index("SRC ="): text.index("OBJ =")]
    assert "csrc/mixer.cpp" in src and "csrc/kernels_bus_legs.hip" in src
    for name in ("mixer.h", "mixer.cpp", "kernels_bus_legs.hip"):
        assert os.path.exists(os.path.join(ROOT, "node-speex-resampler_amd", "csrc", name))
    # the kernel compiles the statements of bus.h and gain.h; it does not restate them
    with open(os.path.join(ROOT, "node-speex-resampler_amd", "csrc", "kernels_bus_legs.hip")) as f:
        kernel = f.read()
    for call in ("bus::first(", "bus::add(", "bus::finish(", "gain::tile_of(", "gain::apply_group<"):
        assert call in kernel, call
    assert "fma(" not in kernel and "mfma" not in kernel.lower()


def wide_order_layout(frames):
    """bus_model's order layout widened to 41 streams: its 32 as they are -- the cancelling pairs in streams 0, 1 and 30,
    31 -- and nine more streams of 2^12 behind them, so that the second pair no longer ends the sum"""
    y = bm.order_layout(frames)
    rng = np.random.default_rng(4141)
    more = (rng.uniform(-1.0, 1.0, (N - bm.ORDER_STREAMS, frames)) * 2.0 ** 12).astype(np.float32)
    return np.concatenate([y, more])


def wide_weights():
    """41 buses: the sum of everything, its negation, the two pairs alone, then mix-minus rows"""
    w = bm.mix_minus(N)
    w[0], w[1] = 1.0, -1.0
    w[2], w[3] = 0.0, 0.0
    w[2, :2] = 1.0
    w[3, 30:32] = 1.0
    return w


def test_debug_bus_equals_the_model_at_41_by_41_and_every_order_defect_shows():
    frames = 800
    y, w = wide_order_layout(frames), wide_weights()
    assert y.shape == (N, frames) and w.shape == (N, N) and np.isfinite(y).all()
    got = speexhip.debug_bus(w, y)
    want = bm.buses(w, y)
    assert got.dtype == np.float32 and got.shape == (N, frames)
    assert np.isfinite(want).all()
    assert got.tobytes() == want.tobytes(), "speexhip_debug_bus differs from the model at 41 x 41"
    assert want[2:4].tobytes() == np.zeros((2, frames), np.float32).tobytes()   # a pair alone among zero weights: +0.0
    for defect in bm.ORDER_DEFECTS:
        z = bm.buses(w, y, defect)
        shares = [bm.changed(z[j], want[j]) for j in range(N)]
        print("41 x 41 order layout, %-16s: up to %5.1f %% of a bus's samples change, %d of %d buses"
              % (defect, 100 * max(shares), sum(s > 0 for s in shares), N))
        assert max(shares) >= 0.01, defect


# ---- the model's own additions for the mixer's kernel (bus_model.py: buses_wide, LEG_DEFECTS, the layouts for any leg count)
def test_buses_wide_is_buses_bit_for_bit():
    rng = np.random.default_rng(5)
    for n_buses, n_legs, n in ((130, 70, 33), (41, 41, 257), (1, 1, 5), (3, 17, 64)):
        w = rng.uniform(-1.5, 1.5, (n_buses, n_legs)).astype(np.float32)
        w[n_buses // 2] = 0.0
        y = (rng.uniform(-1.0, 1.0, (n_legs, n)) * 2.0 ** rng.integers(0, 40, (n_legs, 1))).astype(np.float32)
        y[0, :2] = (-0.0, np.inf)
        assert bm.buses_wide(w, y).tobytes() == bm.buses(w, y).tobytes(), (n_buses, n_legs)
    y, w = wide_order_layout(100), wide_weights()
    assert bm.buses_wide(w, y).tobytes() == bm.buses(w, y).tobytes()


def test_the_wave_dealt_order_and_the_defects_on_an_input_that_cannot_tell():
    assert bm.wave_dealt_order(20)[:16] == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    assert bm.wave_dealt_order(20)[16:] == [16, 17, 18, 19] and bm.wave_dealt_order(22)[16:] == [16, 20, 17, 21, 18, 19]
    # small integers sum exactly in any order: neither defect may change a bit there (they reorder, nothing else)
    rng = np.random.default_rng(6)
    w = rng.integers(-3, 4, (5, 37)).astype(np.float32)
    y = rng.integers(-1000, 1000, (37, 50)).astype(np.float32)
    for defect in bm.LEG_DEFECTS:
        assert bm.buses_legs(w, y, defect).tobytes() == bm.buses(w, y).tobytes(), defect


def stretch_shares(bad, want, frames, n_pairs):
    """per stretch of the layout, the larger share of rows 0 and 1 that the defect changed"""
    lo, hi = bm.order_stretches(n_pairs, frames)
    return [max(bm.changed(bad[j][a:b], want[j][a:b]) for j in (0, 1)) for a, b in zip(lo, hi)]


def test_every_order_defect_shows_on_the_48_leg_layout_and_debug_bus_equals_the_model():
    frames = 402
    y = bm.order_layout_legs(bm.LEGS_48, bm.PAIRS_48, frames)
    w = bm.order_weights_legs(bm.LEGS_48, bm.PAIRS_48, 8)
    assert np.isfinite(y).all() and y.shape == (48, frames) and w.shape == (8, 48)
    for a, b in bm.PAIRS_48:
        assert y[b].tobytes() == (-y[a]).tobytes()
    want = bm.buses(w, y)
    assert want[2:5].tobytes() == np.zeros((3, frames), np.float32).tobytes(), "a pair alone is not +0.0"
    assert bm.buses_wide(w, y).tobytes() == want.tobytes()
    assert speexhip.debug_bus(w, y).tobytes() == want.tobytes(), "speexhip_debug_bus differs from the model on the 48-leg layout"
    shares = {}
    for defect in bm.ORDER_DEFECTS + ("round_each_add",) + bm.LEG_DEFECTS:
        bad = bm.buses_legs(w, y, defect) if defect in bm.LEG_DEFECTS else bm.buses(w, y, defect)
        shares[defect] = stretch_shares(bad, want, frames, 3)
        print("48-leg layout, %-16s: %s %% of rows 0 / 1 change per stretch" % (defect, " / ".join("%5.1f" % (100 * s) for s in shares[defect])))
        assert bad[2:5].tobytes() == want[2:5].tobytes() or defect in ("fp32_accumulator", "round_each_add")
    # the pair across the first block edge is block_partials' alone; wave_dealt sees the pair that begins a block
    assert shares["block_partials"][1] == 1.0 and shares["block_partials"][2] == 1.0
    assert shares["wave_dealt"][0] == 1.0 and shares["wave_dealt"][1] == 0.0 and shares["wave_dealt"][2] >= 0.2
    for defect in bm.ORDER_DEFECTS + ("round_each_add",):
        assert max(shares[defect]) >= 0.75, defect


def test_the_order_defects_show_at_the_mixers_limits_and_debug_bus_equals_the_model():
    frames = 160
    y = bm.limits_layout(frames)
    w = bm.order_weights_legs(bm.LIMIT, bm.LIMIT_PAIRS, bm.LIMIT)
    assert y.shape == (1024, frames) and w.shape == (1024, 1024) and not y[[bm.LIMIT_EMPTY, bm.LIMIT_SILENT]].any()
    want = bm.buses_wide(w, y)
    assert np.isfinite(want).all() and want[2:5].tobytes() == np.zeros((3, frames), np.float32).tobytes()
    assert want[:7].tobytes() == bm.buses(w[:7], y).tobytes()
    assert speexhip.debug_bus(w, y).tobytes() == want.tobytes(), "speexhip_debug_bus differs from the model at 1024 x 1024"
    for defect in ("descending",) + bm.LEG_DEFECTS:
        bad = bm.buses_legs(w[:2], y, defect) if defect in bm.LEG_DEFECTS else bm.buses(w[:2], y, defect)
        shares = stretch_shares(bad, want, frames, 3)
        print("1024-leg layout, %-16s: %s %% of rows 0 / 1 change per stretch" % (defect, " / ".join("%5.1f" % (100 * s) for s in shares)))
        assert max(shares) >= 0.01, defect
