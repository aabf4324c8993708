"""The sample formats of the formatted calls, stated in numpy (include/speexhip_resampler.h, "Sample formats").  The
library's internal unit is one int16 step = 1.0f.  Storage arrays are flat: uint8 for U8 and for packed S24 (3 bytes per
sample, little endian), int16, int32, float32 for the rest.

to_internal(fmt, storage) -> float32 samples the float entry point would be fed;
from_internal(fmt, y)     -> storage of a float32 FIR output: halfup(v) = floor(v + 0.5) in fp64 on v = y * 2^k (the
                             product is exact), saturating, NaN -> the format's zero; the float formats only scale."""
import numpy as np

U8, S16, S24, S32, F32, F32N = range(6)
ALL = (U8, S16, S24, S32, F32, F32N)
NAMES = ("u8", "s16", "s24", "s32", "f32", "f32n")
BYTES = (1, 2, 3, 4, 4, 4)
DTYPE = (np.uint8, np.int16, np.uint8, np.int32, np.float32, np.float32)
ZERO = (128, 0, 0, 0, 0.0, 0.0)
# integer formats: (2^k of "from a FIR value", lowest, highest, offset)
_INT = {U8: (1.0 / 256.0, 0, 255, 128), S16: (1.0, -32768, 32767, 0), S24: (256.0, -(1 << 23), (1 << 23) - 1, 0),
        S32: (65536.0, -(1 << 31), (1 << 31) - 1, 0)}


def pack_s24(values):
    """int array in -2^23 .. 2^23-1 -> uint8 array of 3 bytes per sample, little endian"""
    v = np.asarray(values).astype(np.int64) & 0xFFFFFF
    out = np.empty((v.size, 3), np.uint8)
    flat = v.reshape(-1)
    out[:, 0], out[:, 1], out[:, 2] = flat & 0xFF, (flat >> 8) & 0xFF, (flat >> 16) & 0xFF
    return out.reshape(-1)


def unpack_s24(raw):
    """uint8 array of 3 bytes per sample -> int32 array, sign extended"""
    b = np.asarray(raw, np.uint8).reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)


def integers(fmt, storage):
    """the integer sample values of an integer format's storage (U8: the stored byte)"""
    return unpack_s24(storage) if fmt == S24 else np.asarray(storage, DTYPE[fmt]).reshape(-1).astype(np.int64)


def store(fmt, values):
    """integer (or float, for F32 / F32N) sample values -> the format's flat storage array"""
    return pack_s24(values) if fmt == S24 else np.asarray(values).astype(DTYPE[fmt]).reshape(-1)


def halfup(v):
    return np.floor(np.asarray(v, np.float64) + 0.5)


def to_internal(fmt, storage):
    if fmt == U8:
        return ((np.asarray(storage, np.uint8).reshape(-1).astype(np.int32) - 128) * 256).astype(np.float32)
    if fmt == S16:
        return np.asarray(storage, np.int16).reshape(-1).astype(np.float32)
    if fmt == S24:
        return unpack_s24(storage).astype(np.float32) / np.float32(256.0)
    if fmt == S32:
        return np.asarray(storage, np.int32).reshape(-1).astype(np.float32) / np.float32(65536.0)  # astype: nearest even
    x = np.asarray(storage, np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        return x if fmt == F32 else x * np.float32(32768.0)


def from_internal(fmt, y):
    y = np.asarray(y, np.float32).reshape(-1)
    if fmt == F32:
        return y.copy()
    if fmt == F32N:
        with np.errstate(under="ignore", invalid="ignore"):
            return y / np.float32(32768.0)
    scale, lo, hi, offset = _INT[fmt]
    with np.errstate(invalid="ignore"):
        r = halfup(y.astype(np.float64) * scale) + offset
        r = np.where(np.isnan(r), float(ZERO[fmt]), np.clip(r, lo, hi))
    return store(fmt, r.astype(np.int64))


def samples_in(fmt, storage):
    """number of samples a flat storage array holds"""
    return np.asarray(storage).size // (3 if fmt == S24 else 1)
