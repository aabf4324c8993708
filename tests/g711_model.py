"""The companded sample formats of the formatted and mixed calls, stated in numpy (include/speexhip_resampler.h,
"Companded formats"; csrc/g711.h is the C statement): G.711 mu-law and A-law, one byte per sample.

decode(fmt, bytes) -> float32, exact integers in int16 units;
encode(fmt, q)     -> bytes of int16 values q;
from_internal(fmt, y) = encode(the S16 output rule on y), from_internal_dither with the dithered S16 rule.

to_internal / from_internal / from_internal_dither here take EVERY format: the six of sample_formats.py go to that module
(and to dither_model.py), so a test can walk all eight with one set of functions."""
import numpy as np

import dither_model as dm
import sample_formats as sf

ULAW, ALAW = 16, 17
COMPANDED = (ULAW, ALAW)
ALL = sf.ALL + COMPANDED
_NAMES = {ULAW: "ulaw", ALAW: "alaw"}
ZERO = {ULAW: 0xFF, ALAW: 0xD5}              # what q = 0 encodes to: NaN, the zero fallback's silence
RAILS = {ULAW: (0x00, 0x80), ALAW: (0x2A, 0xAA)}   # (q = -32768, q = 32767)
PEAK = {ULAW: 32124, ALAW: 32256}            # the largest decoded magnitude


def name(fmt):
    return _NAMES[fmt] if fmt in COMPANDED else sf.NAMES[fmt]


def nbytes(fmt):
    return 1 if fmt in COMPANDED else sf.BYTES[fmt]


def dtype(fmt):
    return np.uint8 if fmt in COMPANDED else sf.DTYPE[fmt]


def per_sample(fmt):
    """elements of the flat storage array per sample (packed S24: 3 bytes)"""
    return 3 if fmt == sf.S24 else 1


def _log2_floor(v):
    """floor(log2(v)) of positive integers (an int64 array), by comparison: no floating point"""
    out = np.zeros(v.shape, np.int64)
    for k in range(1, 32):
        out[v >= (1 << k)] = k
    return out


def decode(fmt, codes):
    b = np.asarray(codes, np.uint8).reshape(-1).astype(np.int64)
    if fmt == ULAW:
        u = ~b & 0xFF
        e, m = (u >> 4) & 7, u & 15
        t = (((m << 3) + 0x84) << e) - 0x84
        return np.where(u & 0x80, -t, t).astype(np.float32)
    assert fmt == ALAW
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.float32)


def encode(fmt, q):
    q = np.asarray(q).reshape(-1).astype(np.int64)
    assert q.size == 0 or (q.min() >= -32768 and q.max() <= 32767)
    if fmt == ULAW:
        s = (q < 0).astype(np.int64)
        mag = np.minimum(np.abs(q), 32635) + 132
        e = _log2_floor(mag) - 7
        m = (mag >> (e + 3)) & 15
        return (~((s << 7) | (e << 4) | m) & 0xFF).astype(np.uint8)
    assert fmt == ALAW
    pos = (q >= 0).astype(np.int64)
    mag = np.where(q >= 0, q, -q - 1) >> 3
    e = np.where(mag < 32, 0, _log2_floor(np.maximum(mag, 1)) - 4)
    m = np.where(e == 0, (mag >> 1) & 15, (mag >> e) & 15)
    return (((pos << 7) | (e << 4) | m) ^ 0x55).astype(np.uint8)


def to_internal(fmt, storage):
    return decode(fmt, storage) if fmt in COMPANDED else sf.to_internal(fmt, storage)


def from_internal(fmt, y):
    if fmt in COMPANDED:
        return encode(fmt, sf.from_internal(sf.S16, y))
    return sf.from_internal(fmt, y)


def quantise(fmt, y, d):
    """float32 FIR values y with dither d (in int16 steps for the companded formats) -> flat storage"""
    if fmt in COMPANDED:
        return encode(fmt, dm.quantise(sf.S16, y, d))
    return dm.quantise(fmt, y, d)


def from_internal_dither(fmt, y, kind, seed, position, c_out):
    """the output conversion of a call of a state with dither on that starts at output frame `position`"""
    if fmt in COMPANDED:
        return encode(fmt, dm.from_internal(sf.S16, y, kind, seed, position, c_out))
    return dm.from_internal(fmt, y, kind, seed, position, c_out)
