"""The level of a mixer's leg (include/speexhip_resampler.h, "Mixer levels"; csrc/levels.h) in numpy, and the defects a
wrong implementation could have.  One record over the flat float32 values y of a leg's call (int16 units, all channels,
BEFORE the state's gain):

  samples  y.size
  nan      the samples with y != y; they count for nothing else
  peak     max |y| as a float32 (+inf is a legal peak; 0.0 when there is no number)
  energy   sum of q * q, q = clamp(floor(float64(y) + 0.5), -32768, 32767): Python integers, exact, mod 2^64

record(y) is that.  record(y, defect=..., gain=..., padded=...) plants one of DEFECTS:

  truncate            q = trunc(y): toward zero, not floor(y + 0.5)
  half_even           q = rint(y): ties to even, not upward
  post_gain           measured on float32(y * gain) (gain: a float32 per sample, or one for all), not on y
  padded              samples = padded: the +0.0f up to the bus's length counted as the leg's
  signed_peak         peak = max(y, 0), not max |y|: a negative excursion is missed
  fp32_energy         energy accumulated in float32, sample after sample, and converted at the end
  nan_as_zero_sample  a NaN is not counted: it is taken for a sample of 0.0

Records are dicts of Python ints and one numpy float32; same() compares them for equality, the peak by its bits."""
import math

import numpy as np

DEFECTS = ("truncate", "half_even", "post_gain", "padded", "signed_peak", "fp32_energy", "nan_as_zero_sample")
FIELDS = ("samples", "energy", "nan", "peak")
ZERO = {"samples": 0, "energy": 0, "nan": 0, "peak": np.float32(0.0)}


def steps(y, defect=None):
    """q of every sample as int64 (0 where y is a NaN)"""
    y = np.asarray(y, np.float32).reshape(-1)
    nan = np.isnan(y)
    v = np.where(nan, np.float32(0.0), y).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(v) if defect == "truncate" else np.rint(v) if defect == "half_even" else np.floor(v + 0.5)
    return np.clip(r, -32768.0, 32767.0).astype(np.int64)


def record(y, defect=None, gain=None, padded=None):
    assert defect is None or defect in DEFECTS, defect
    y = np.asarray(y, np.float32).reshape(-1)
    if defect == "post_gain":
        with np.errstate(invalid="ignore", over="ignore"):
            y = (y * np.asarray(gain, np.float32)).astype(np.float32)
    nan = np.isnan(y)
    numbers = np.where(nan, np.float32(0.0), y)
    q = steps(y, defect)
    if defect == "fp32_energy":
        # (accumulate is sequential: one float32 rounding per sample, in order)
        energy = int(np.add.accumulate((q * q).astype(np.float32), dtype=np.float32)[-1]) if q.size else 0
    else:
        energy = int((q * q).astype(np.uint64).sum(dtype=np.uint64))   # (integers below 2^30 each: exact, mod 2^64)
    peak = np.float32(0.0)
    if y.size:
        peak = np.float32(max(numbers.max(), np.float32(0.0))) if defect == "signed_peak" else np.float32(np.abs(numbers).max())
    return {"samples": int(padded) if defect == "padded" else int(y.size), "energy": energy,
            "nan": 0 if defect == "nan_as_zero_sample" else int(nan.sum()), "peak": peak}


def same(a, b):
    return all(int(a[k]) == int(b[k]) for k in ("samples", "energy", "nan")) and \
        np.float32(a["peak"]).view(np.uint32) == np.float32(b["peak"]).view(np.uint32)


def changed(a, b):
    """the fields in which two records differ"""
    return tuple(k for k in FIELDS if not same({**ZERO, k: a[k]}, {**ZERO, k: b[k]}))


def of_struct(rec):
    """a record of speexhip.LEVEL_DTYPE as the model's dict"""
    return {"samples": int(rec["samples"]), "energy": int(rec["energy"]), "nan": int(rec["nan"]), "peak": np.float32(rec["peak"])}


def audio_level(rec):
    """RFC 6464: -dBov of the RMS against full scale 2^15, 0 .. 127; 127 for no energy or no samples"""
    if int(rec["energy"]) == 0 or int(rec["samples"]) == 0:
        return 127
    return min(127, max(0, round(-10.0 * math.log10(int(rec["energy"]) / (int(rec["samples"]) * 2.0 ** 30)))))
