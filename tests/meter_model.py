"""The output meter restated in numpy (include/speexhip_resampler.h, "Metering"), for the tests to hold the library
against.  For one value y (float32, int16 units) on its way to format F, with d its dither (float64, in LSB of F; 0: none):

  nan    y != y, and nothing else is counted for that sample
  peak   the largest |y| among the rest, as a float32 (0 when there is none)
  clips  the formats that are dithered only -- integer, companded, big-endian:  v = float64(y) * scale,  t = v + d,
         r = floor(t + 0.5) + offset;  r > hi counts as clipped_high, r < lo as clipped_low.  The companded formats are
         judged as S16, a big-endian format as its little-endian twin; the float formats count none.

Every step is one IEEE operation on float64 in numpy as in the library, so the totals are compared for equality."""
import numpy as np

import speexhip

# every format: name -> (FMT_*, (scale, offset, lo, hi) or None for a float format)
_U8 = (1.0 / 256.0, 128.0, 0.0, 255.0)
_S16 = (1.0, 0.0, -32768.0, 32767.0)
_S24 = (256.0, 0.0, -8388608.0, 8388607.0)
_S32 = (65536.0, 0.0, -2147483648.0, 2147483647.0)
FORMATS = {
    "u8": (speexhip.FMT_U8, _U8), "s16": (speexhip.FMT_S16, _S16), "s24": (speexhip.FMT_S24, _S24),
    "s32": (speexhip.FMT_S32, _S32), "f32": (speexhip.FMT_F32, None), "f32n": (speexhip.FMT_F32N, None),
    "ulaw": (speexhip.FMT_ULAW, _S16), "alaw": (speexhip.FMT_ALAW, _S16), "f16n": (speexhip.FMT_F16N, None),
    "bf16n": (speexhip.FMT_BF16N, None), "s16be": (speexhip.FMT_S16BE, _S16), "s24be": (speexhip.FMT_S24BE, _S24),
    "s32be": (speexhip.FMT_S32BE, _S32),
}
NAMES = tuple(FORMATS)
RAILS = {fmt: rails for fmt, rails in FORMATS.values()}
KEYS = ("samples", "clipped_high", "clipped_low", "nan", "peak")


def clips(fmt):
    """whether the format counts clips (the formats that are dithered)"""
    return RAILS[fmt] is not None


def totals(fmt, y, d=None):
    """the meter's totals over y on its way to fmt, as get_meter reports them (without 'on')"""
    y = np.asarray(y, np.float32).reshape(-1)
    nan = np.isnan(y)
    ok = y[~nan]
    out = {"samples": int(y.size), "clipped_high": 0, "clipped_low": 0, "nan": int(nan.sum()),
           "peak": float(np.abs(ok).max()) if ok.size else 0.0}
    if RAILS[fmt] is not None:
        scale, offset, lo, hi = RAILS[fmt]
        dd = np.zeros(y.size, np.float64) if d is None else np.asarray(d, np.float64).reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            v = ok.astype(np.float64) * scale
            t = v + dd[~nan]
            r = np.floor(t + 0.5) + offset
        out["clipped_high"] = int((r > hi).sum())
        out["clipped_low"] = int((r < lo).sum())
    return out


def add(a, b):
    """the totals of two runs of a stream, one after the other"""
    out = {k: a[k] + b[k] for k in ("samples", "clipped_high", "clipped_low", "nan")}
    out["peak"] = max(a["peak"], b["peak"])
    return out


def same(got, want):
    """counts equal and the peak's bits equal"""
    return all(int(got[k]) == int(want[k]) for k in ("samples", "clipped_high", "clipped_low", "nan")) and \
        np.float32(got["peak"]).tobytes() == np.float32(want["peak"]).tobytes()


ZERO = {"samples": 0, "clipped_high": 0, "clipped_low": 0, "nan": 0, "peak": 0.0}
