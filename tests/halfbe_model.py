"""The half-float and big-endian sample formats of the formatted, mixed and sides calls, stated in numpy
(include/speexhip_resampler.h, "Half-float and big-endian formats"; csrc/halfbe.h is the C statement).

  F16N   IEEE binary16 in +-1.0:   x = float32(h) * 32768;  h = binary16(y / 32768), nearest even, subnormals kept,
         NaN -> 0x7E00 | sign.     Storage: np.float16.
  BF16N  bfloat16 in +-1.0:        x = as_float(b << 16) * 32768;  u = bits(y / 32768): NaN -> 0x7FC0 | sign, otherwise
         (u + 0x7FFF + ((u >> 16) & 1)) >> 16.   Storage: np.uint16, the bits (numpy has no bfloat16).
  S16BE / S24BE / S32BE   the S16 / S24 / S32 sample with its bytes reversed: byteswap of the little-endian model.
         Storage: '>i2', uint8 (3 bytes per sample), '>i4'.

to_internal / from_internal / quantise / from_internal_dither here take EVERY format: the eight of g711_model.py go to
that module, so a test can walk all thirteen with one set of functions."""
import numpy as np

import dither_model as dm
import g711_model as gm
import sample_formats as sf

F16N, BF16N, S16BE, S24BE, S32BE = 20, 21, 24, 25, 26
HALF = (F16N, BF16N)
BIG = (S16BE, S24BE, S32BE)
NEW = HALF + BIG
OLD = gm.ALL
ALL = OLD + NEW
LE_TWIN = {S16BE: sf.S16, S24BE: sf.S24, S32BE: sf.S32}
_NAMES = {F16N: "f16n", BF16N: "bf16n", S16BE: "s16be", S24BE: "s24be", S32BE: "s32be"}
_BYTES = {F16N: 2, BF16N: 2, S16BE: 2, S24BE: 3, S32BE: 4}
_DTYPE = {F16N: np.dtype(np.float16), BF16N: np.dtype(np.uint16), S16BE: np.dtype(">i2"), S24BE: np.dtype(np.uint8),
          S32BE: np.dtype(">i4")}


def name(fmt):
    return _NAMES[fmt] if fmt in NEW else gm.name(fmt)


def nbytes(fmt):
    return _BYTES[fmt] if fmt in NEW else gm.nbytes(fmt)


def dtype(fmt):
    return _DTYPE[fmt] if fmt in NEW else np.dtype(gm.dtype(fmt))


def per_sample(fmt):
    """elements of the flat storage array per sample (the packed 24-bit formats: 3 bytes)"""
    return nbytes(fmt) // dtype(fmt).itemsize


def dithered(fmt):
    return fmt not in HALF and fmt not in (sf.F32, sf.F32N)


def raw(fmt, storage):
    """the bytes of a storage array, as a flat uint8 array"""
    return np.ascontiguousarray(storage, dtype=dtype(fmt)).reshape(-1).view(np.uint8)


def reverse(fmt, storage_bytes):
    """each sample's bytes reversed: uint8 in, uint8 out"""
    b = np.asarray(storage_bytes, np.uint8).reshape(-1, nbytes(fmt))
    return np.ascontiguousarray(b[:, ::-1]).reshape(-1)


def be_of(fmt, le_storage):
    """storage of the little-endian twin -> storage of the big-endian format fmt"""
    twin = LE_TWIN[fmt]
    le = np.ascontiguousarray(le_storage, dtype=sf.DTYPE[twin]).reshape(-1).view(np.uint8)
    return reverse(fmt, le).view(dtype(fmt))


def le_of(fmt, be_storage):
    """storage of the big-endian format fmt -> storage of its little-endian twin"""
    return reverse(fmt, raw(fmt, be_storage)).view(sf.DTYPE[LE_TWIN[fmt]])


# ---- the half formats ------------------------------------------------------------------------------------------------
def f16_bits(z):
    """float32 z -> binary16 codes (uint16): astype is round-to-nearest-even with subnormals; NaN canonical by sign"""
    z = np.asarray(z, np.float32).reshape(-1)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        h = z.astype(np.float16).view(np.uint16)
    sign = ((z.view(np.uint32) >> np.uint32(16)) & np.uint32(0x8000)).astype(np.uint16)
    return np.where(np.isnan(z), np.uint16(0x7E00) | sign, h).astype(np.uint16)


def bf16_bits(z):
    """float32 z -> bfloat16 codes (uint16) by the integer formula"""
    u = np.asarray(z, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = np.uint64(0x7FC0) | ((u >> np.uint64(16)) & np.uint64(0x8000))
    return np.where(np.isnan(np.asarray(z, np.float32).reshape(-1)), nan, r).astype(np.uint16)


def _scaled_down(y):
    """z = y * (1 / 32768) in fp32, subnormal results kept"""
    with np.errstate(under="ignore", invalid="ignore"):
        return np.asarray(y, np.float32).reshape(-1) * np.float32(1.0 / 32768.0)


def to_internal(fmt, storage):
    if fmt == F16N:
        h = np.ascontiguousarray(storage, dtype=np.float16).reshape(-1)
        with np.errstate(over="ignore", invalid="ignore"):
            return h.astype(np.float32) * np.float32(32768.0)
    if fmt == BF16N:
        b = np.ascontiguousarray(storage, dtype=np.uint16).reshape(-1)
        with np.errstate(over="ignore", invalid="ignore"):
            return (b.astype(np.uint32) << np.uint32(16)).view(np.float32) * np.float32(32768.0)
    if fmt in BIG:
        return sf.to_internal(LE_TWIN[fmt], le_of(fmt, storage))
    return gm.to_internal(fmt, storage)


def from_internal(fmt, y):
    if fmt == F16N:
        return f16_bits(_scaled_down(y)).view(np.float16)
    if fmt == BF16N:
        return bf16_bits(_scaled_down(y))
    if fmt in BIG:
        return be_of(fmt, sf.from_internal(LE_TWIN[fmt], y))
    return gm.from_internal(fmt, y)


def quantise(fmt, y, d):
    """float32 FIR values y with dither d (LSB of the format) -> flat storage; the float formats take no dither"""
    if fmt in BIG:
        return be_of(fmt, dm.quantise(LE_TWIN[fmt], y, d))
    if not dithered(fmt):
        return from_internal(fmt, y)
    return gm.quantise(fmt, y, d)


def from_internal_dither(fmt, y, kind, seed, position, c_out):
    """the output conversion of a call of a state with dither on that starts at output frame `position`"""
    if fmt in BIG:
        return be_of(fmt, dm.from_internal(LE_TWIN[fmt], y, kind, seed, position, c_out))
    if fmt in HALF:
        return from_internal(fmt, y)
    return gm.from_internal_dither(fmt, y, kind, seed, position, c_out)


def zero(fmt):
    """the bytes of one sample of the format's zero (NaN for the integer formats, the zero fallback's silence)"""
    return raw(fmt, from_internal(fmt, np.zeros(1, np.float32)))
