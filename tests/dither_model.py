"""The dither of the formatted and mixed calls' integer outputs, stated in numpy (include/speexhip_resampler.h, "Dither";
csrc/dither.h is the C statement).  The noise of an output sample is a pure function of (seed, idx):

  mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32, wrapping)
  idx = (position + f) * C_out + c            (uint64, wrapping)
  w   = mix32( lo32(idx) ^ mix32( hi32(idx) ^ hi32(seed) ) ^ lo32(seed) );   a = w & 0xffff,  b = w >> 16
  d   = 0 (NONE),  (a + 0.5) / 65536 - 0.5 (RECTANGULAR),  (a - b) / 65536 (TRIANGULAR)        in LSB of the output format

and a float32 FIR value y becomes v = float64(y) * 2^k (exact), t = v + d, q = floor(t + 0.5), each one float64 rounding,
then the U8 offset and the clamp; NaN -> the format's zero."""
import numpy as np

import sample_formats as sf

NONE, RECTANGULAR, TRIANGULAR = 0, 1, 2
KINDS = (RECTANGULAR, TRIANGULAR)
KIND_NAMES = {NONE: "none", RECTANGULAR: "rectangular", TRIANGULAR: "triangular"}
STREAM_STEP = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def words(seed, first_index, n):
    """the generator's uint32 word of idx = first_index .. first_index + n - 1 (mod 2^64)"""
    seed = int(seed) & M64
    idx = np.uint64(int(first_index) & M64) + np.arange(n, dtype=np.uint64)   # (uint64 arithmetic wraps)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    inner = mix32(hi ^ np.uint32(seed >> 32))
    return mix32(lo ^ inner ^ np.uint32(seed & 0xFFFFFFFF))


def values(kind, seed, first_index, n):
    """d of idx = first_index .. first_index + n - 1, float64, in LSB"""
    if kind == NONE:
        return np.zeros(n, np.float64)
    assert kind in KINDS
    w = words(seed, first_index, n)
    a = (w & np.uint32(0xFFFF)).astype(np.float64)
    b = (w >> np.uint32(16)).astype(np.float64)
    if kind == RECTANGULAR:
        return (a + 0.5) / 65536.0 - 0.5
    return (a - b) / 65536.0


def stream_seed(seed, s):
    """seed of stream s of a batch"""
    return (int(seed) + s * STREAM_STEP) & M64


def quantise(fmt, y, d):
    """float32 FIR values y with dither d (LSB) -> flat storage of the integer format fmt"""
    scale, lo, hi, offset = sf._INT[fmt]
    y = np.asarray(y, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = y.astype(np.float64) * scale
        t = v + np.asarray(d, np.float64)
        r = np.floor(t + 0.5) + offset
        r = np.where(np.isnan(r), float(sf.ZERO[fmt]), np.clip(r, lo, hi))
    return sf.store(fmt, r.astype(np.int64))


def from_internal(fmt, y, kind, seed, position, c_out):
    """the output conversion of a call that starts at output frame `position`: y = the float32 frames it produced, c_out
    samples each.  Float formats are written as without dither."""
    y = np.asarray(y, np.float32).reshape(-1)
    if fmt in (sf.F32, sf.F32N):
        return sf.from_internal(fmt, y)
    return quantise(fmt, y, values(kind, seed, (int(position) * c_out) & M64, y.size))
