"""ctypes binding of libspeexhip.so (include/speexhip_resampler.h) plus a Python mirror of the
reference's host class (``SpeexResampler.processChunk``, reference src/index.ts:21-117) so that
the parity tests and bench.py can drive the HIP path without Node.

There is NO fallback: if the library is missing or no MI355X is usable, calls raise.
"""
import ctypes as C
import math
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (SPEEXHIP_LIB_PATH: same-box A/B of two builds of the library, tools/ab.sh and tools/lease.sh lib-ab)
LIB_PATH = os.environ.get("SPEEXHIP_LIB_PATH") or os.path.join(PKG_DIR, "libspeexhip.so")

MODE_FAST, MODE_EXACT, MODE_FAST_F32, MODE_FAST_FIXED = 0, 1, 2, 3
KERNEL_NAMES = ("direct_single", "direct_double", "interpolate_single", "interpolate_double")
# reference codes (deps/speex/speex_resampler.h:104-113) + 6 = HIP failure
ERR_SUCCESS, ERR_ALLOC_FAILED, ERR_BAD_STATE, ERR_INVALID_ARG, ERR_PTR_OVERLAP, ERR_OVERFLOW = 0, 1, 2, 3, 4, 5
ERR_DEVICE = 6
ERR_NO_BLOCK = 7  # the ..._take calls: no pinned result block free right now, state untouched
# sample formats of the formatted calls (SPEEXHIP_FMT_*); S24 is packed: 3 bytes per sample, a uint8 array here
FMT_U8, FMT_S16, FMT_S24, FMT_S32, FMT_F32, FMT_F32N = range(6)
FMT_BYTES = (1, 2, 3, 4, 4, 4)
FMT_DTYPE = (np.uint8, np.int16, np.uint8, np.int32, np.float32, np.float32)  # numpy storage type of each format
# companded formats (G.711 mu-law / A-law, one byte per sample) start at 16; 6..15 stay invalid
FMT_ULAW, FMT_ALAW = 16, 17
# half-float formats in +-1.0 (binary16; bfloat16, whose numpy storage is its bits: numpy has no bfloat16) and big-endian
# PCM (S24BE packed: 3 bytes per sample, a uint8 array here); 18, 19, 22, 23 stay invalid
FMT_F16N, FMT_BF16N = 20, 21
FMT_S16BE, FMT_S24BE, FMT_S32BE = 24, 25, 26
_MORE_FORMATS = {FMT_ULAW: (1, np.uint8), FMT_ALAW: (1, np.uint8), FMT_F16N: (2, np.float16), FMT_BF16N: (2, np.uint16),
                 FMT_S16BE: (2, np.dtype(">i2")), FMT_S24BE: (3, np.uint8), FMT_S32BE: (4, np.dtype(">i4"))}


def fmt_bytes(fmt):
    """bytes of one sample of a format (FMT_*), the companded, half-float and big-endian ones included"""
    if fmt in _MORE_FORMATS:
        return _MORE_FORMATS[fmt][0]
    if not 0 <= fmt < len(FMT_BYTES):
        raise ValueError("unknown sample format %r" % (fmt,))
    return FMT_BYTES[fmt]


def fmt_dtype(fmt):
    """numpy storage type of a format (FMT_*), the companded, half-float and big-endian ones included"""
    if fmt in _MORE_FORMATS:
        return _MORE_FORMATS[fmt][1]
    if not 0 <= fmt < len(FMT_DTYPE):
        raise ValueError("unknown sample format %r" % (fmt,))
    return FMT_DTYPE[fmt]


def _per_sample(fmt):
    """elements of a format's numpy storage array per sample (the packed 24-bit formats: 3 bytes)"""
    return fmt_bytes(fmt) // np.dtype(fmt_dtype(fmt)).itemsize


# dither of the integer output formats of the formatted and mixed calls (SPEEXHIP_DITHER_*), a property of the state
DITHER_NONE, DITHER_RECTANGULAR, DITHER_TRIANGULAR = range(3)

EXPORTS = [
    "speexhip_resampler_init", "speexhip_resampler_destroy",
    "speexhip_resampler_process_interleaved_int", "speexhip_resampler_process_interleaved_float",
    "speexhip_resampler_process_interleaved_float_device",
    "speexhip_batch_process_interleaved_float_device", "speexhip_resampler_get_rate",
    "speexhip_resampler_strerror", "speexhip_resampler_process_interleaved_int_device",
    "speexhip_resampler_set_mode", "speexhip_resampler_get_info", "speexhip_resampler_get_history",
    "speexhip_batch_init", "speexhip_batch_destroy", "speexhip_batch_set_mode",
    "speexhip_batch_get_info", "speexhip_batch_process_interleaved_int_device",
    "speexhip_design_filter", "speexhip_plan_call", "speexhip_version",
    # mid-stream control
    "speexhip_resampler_init_frac", "speexhip_resampler_set_rate", "speexhip_resampler_set_rate_frac",
    "speexhip_resampler_get_ratio", "speexhip_resampler_set_quality", "speexhip_resampler_get_quality",
    "speexhip_resampler_get_input_latency", "speexhip_resampler_get_output_latency",
    "speexhip_resampler_skip_zeros", "speexhip_resampler_reset_mem",
    "speexhip_batch_set_rate_frac", "speexhip_batch_set_quality", "speexhip_batch_skip_zeros",
    "speexhip_batch_reset_mem", "speexhip_batch_get_history",
    "speexhip_design_filter_frac", "speexhip_plan_call_ex", "speexhip_plan_filter_change",
    # chunk coalescing
    "speexhip_resampler_process_chunks_int", "speexhip_resampler_process_chunks_float",
    "speexhip_resampler_peek",
    # per-channel entry points + strides (rest of row N2), the zero fallback's test hook (row a6)
    "speexhip_resampler_process_int", "speexhip_resampler_process_float",
    "speexhip_resampler_set_input_stride", "speexhip_resampler_get_input_stride",
    "speexhip_resampler_set_output_stride", "speexhip_resampler_get_output_stride",
    "speexhip_resampler_get_channel_position", "speexhip_debug_fail_device_allocs",
    "speexhip_release_cached_memory", "speexhip_debug_plan",
    "speexhip_resampler_release_stream", "speexhip_batch_release_stream", "speexhip_debug_device_clock",
    "speexhip_resampler_process_interleaved_int_take", "speexhip_resampler_process_interleaved_float_take",
    "speexhip_block_release", "speexhip_debug_plan64", "speexhip_debug_launch_shape",
    # round 5: device placement, many states per call
    "speexhip_device_count", "speexhip_resampler_init_on", "speexhip_batch_init_on",
    "speexhip_resampler_process_many_int", "speexhip_resampler_process_many_float",
    "speexhip_resampler_get_info2", "speexhip_debug_placement", "speexhip_warmup",
    # round 6: pinned blocks the caller fills (inputs used in place)
    "speexhip_block_acquire", "speexhip_debug_pcie_peak", "speexhip_debug_placement_live", "speexhip_debug_live_states",
    # planar (one plane per channel) calls
    "speexhip_resampler_process_planar_int", "speexhip_resampler_process_planar_float",
    "speexhip_resampler_process_planar_int_device", "speexhip_resampler_process_planar_float_device",
    "speexhip_batch_process_planar_int_device", "speexhip_batch_process_planar_float_device",
    # sample formats: u8, packed s24, s32, float in +-1.0; input and output named independently
    "speexhip_sample_bytes", "speexhip_resampler_process_interleaved_fmt",
    "speexhip_resampler_process_interleaved_fmt_device", "speexhip_batch_process_interleaved_fmt_device",
    # channel mixing in the formatted calls: a matrix before the FIR and / or after it
    "speexhip_resampler_process_interleaved_mix", "speexhip_resampler_process_interleaved_mix_device",
    "speexhip_batch_process_interleaved_mix_device",
    # dither of the integer output formats of the formatted and mixed calls
    "speexhip_resampler_set_dither", "speexhip_resampler_get_dither", "speexhip_batch_set_dither",
    "speexhip_batch_get_dither", "speexhip_debug_dither",
    # companded formats: G.711 mu-law and A-law in the formatted and mixed calls
    "speexhip_debug_g711_decode", "speexhip_debug_g711_encode",
    # half-float (binary16, bfloat16 in +-1.0) and big-endian (s16, packed s24, s32) formats
    "speexhip_debug_format_decode", "speexhip_debug_format_encode",
    # layouts: planar or interleaved per side of a formatted or mixed call
    "speexhip_resampler_process_sides", "speexhip_resampler_process_sides_device", "speexhip_batch_process_sides_device",
    # many states, formatted: a format per state in one fused call
    "speexhip_resampler_process_many_sides", "speexhip_resampler_process_many_fmt", "speexhip_debug_many_counters",
    # chunk coalescing, formatted: a side per direction
    "speexhip_resampler_process_chunks_sides", "speexhip_resampler_process_chunks_fmt", "speexhip_debug_chunk_counters",
    # metering: clip counts and peak level of the formatted, mixed and sides calls' outputs
    "speexhip_resampler_set_meter", "speexhip_resampler_get_meter", "speexhip_batch_set_meter", "speexhip_batch_get_meter",
    "speexhip_debug_meter",
    # gain: per-stream volume with click-free ramps in the formatted, mixed and sides calls
    "speexhip_resampler_set_gain", "speexhip_resampler_get_gain", "speexhip_batch_set_gain", "speexhip_batch_get_gain",
    "speexhip_debug_gain",
    # buses: weighted sums of a batch's streams in one device call
    "speexhip_batch_set_buses", "speexhip_batch_get_buses", "speexhip_batch_process_bus_device",
    "speexhip_batch_get_bus_meter", "speexhip_batch_get_bus_position", "speexhip_debug_bus",
    # mixer: mix buses over many separate states in one host call
    "speexhip_mixer_init", "speexhip_mixer_init_on", "speexhip_mixer_destroy", "speexhip_mixer_set_weights",
    "speexhip_mixer_get_weights", "speexhip_mixer_set_dither", "speexhip_mixer_get_dither", "speexhip_mixer_set_meter",
    "speexhip_mixer_get_bus_meter", "speexhip_mixer_process", "speexhip_debug_mixer_counters",
    # mixer levels: per-leg level records of every tick, measured on the device
    "speexhip_mixer_set_levels", "speexhip_mixer_get_levels", "speexhip_debug_levels", "speexhip_debug_mixer_level_launches",
]
MIXER_MAX_LEGS = MIXER_MAX_BUSES = 1024
# SpeexHipLevel: one slot's record of one mixer call (32 bytes)
LEVEL_DTYPE = np.dtype([("samples", np.uint64), ("energy", np.uint64), ("nan", np.uint64), ("peak", np.float32),
                        ("reserved", np.uint32)])


class Meter(C.Structure):
    """SpeexHipMeter: a stream's totals since the last reset"""
    _fields_ = [("struct_size", C.c_uint32), ("on", C.c_uint32), ("samples", C.c_uint64), ("clipped_high", C.c_uint64),
                ("clipped_low", C.c_uint64), ("nan", C.c_uint64), ("peak", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(Meter)

    def as_dict(self):
        return {"on": bool(self.on), "samples": int(self.samples), "clipped_high": int(self.clipped_high),
                "clipped_low": int(self.clipped_low), "nan": int(self.nan), "peak": float(self.peak)}

# layout of a side of the sides calls (SPEEXHIP_LAYOUT_*)
LAYOUT_INTERLEAVED, LAYOUT_PLANAR = 0, 1


def _layout(name):
    """'interleaved' / 'planar' (or a LAYOUT_* value, or None = interleaved) as a LAYOUT_* value"""
    if name is None:
        return LAYOUT_INTERLEAVED
    if name in (LAYOUT_INTERLEAVED, LAYOUT_PLANAR) and not isinstance(name, str):
        return int(name)
    try:
        return {"interleaved": LAYOUT_INTERLEAVED, "planar": LAYOUT_PLANAR}[name]
    except KeyError:
        raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (name,))


def _mix_matrix(m, channels, is_input):
    """a mixed call's matrix as (row-major float32 array or None, the caller-side channel count): in_mix is
    channels x in_channels, out_mix is out_channels x channels"""
    if m is None:
        return None, channels
    a = np.ascontiguousarray(m, dtype=np.float32)
    if a.ndim != 2 or a.shape[0 if is_input else 1] != channels:
        raise ValueError("%s must be %s for a state of %d channels" % (
            ("in_mix", "(channels x in_channels)") if is_input else ("out_mix", "(out_channels x channels)"), channels))
    return a, a.shape[1 if is_input else 0]


def _mix_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Info(C.Structure):
    _fields_ = [("in_rate", C.c_uint32), ("out_rate", C.c_uint32), ("num_rate", C.c_uint32),
                ("den_rate", C.c_uint32), ("nb_channels", C.c_uint32), ("quality", C.c_int32),
                ("filt_len", C.c_uint32), ("oversample", C.c_uint32),
                ("sinc_table_length", C.c_uint32), ("kernel", C.c_int32), ("mode", C.c_int32),
                ("fast_path", C.c_int32), ("last_sample", C.c_int32), ("samp_frac_num", C.c_uint32),
                ("device", C.c_int32), ("magic_samples", C.c_uint32), ("block_in", C.c_uint32),
                ("accumulate_bits", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Side(C.Structure):
    """SpeexHipSide: one side of a sides call"""
    _fields_ = [("struct_size", C.c_uint32), ("fmt", C.c_int32), ("channels", C.c_uint32), ("layout", C.c_int32),
                ("mix", C.c_void_p), ("data", C.c_void_p), ("plane_stride", C.c_uint64), ("stream_stride", C.c_uint64),
                ("planes", C.POINTER(C.c_void_p))]


def make_side(fmt, channels, layout=LAYOUT_INTERLEAVED, mix=None, data=None, plane_stride=0, stream_stride=0, planes=None):
    """A Side: mix = a float32 array (kept alive by the caller) or None; data = an address or None; planes = a ctypes
    array of addresses (host form) or None."""
    side = Side()
    side.struct_size = C.sizeof(Side)
    side.fmt, side.channels, side.layout = int(fmt), int(channels), int(layout)
    side.mix = None if mix is None else mix.ctypes.data
    side.data = data
    side.plane_stride, side.stream_stride = int(plane_stride), int(stream_stride)
    if planes is not None:
        side.planes = C.cast(planes, C.POINTER(C.c_void_p))
    return side


_lib = None


def lib():
    """Load libspeexhip.so or raise (the product path never degrades to a CPU implementation)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libspeexhip.so not built: run `python __graft_entry__.py` or "
                               "`make -C node-speex-resampler_amd` (no CPU fallback exists)")
        # One HIP runtime per process: PyTorch-ROCm preloads its bundled libamdhip64.so.7 by path;
        # if ours pulled in /opt/rocm's copy first there would be two runtimes and the second
        # to initialise sees no device.  Loading torch first makes both share one copy.
        # (SPEEXHIP_PY_NO_TORCH=1, tools only: load the library behind /opt/rocm's runtime, as the Node addon does --
        #  the two runtimes differ, e.g. in whether pinned copies of opposite directions overlap, profiles/r06_runtime_ab.txt)
        if os.environ.get("SPEEXHIP_PY_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        u32, i32, p = C.c_uint32, C.c_int, C.c_void_p
        pu32, pi16 = C.POINTER(C.c_uint32), C.POINTER(C.c_int16)
        L.speexhip_resampler_init.restype = p
        L.speexhip_resampler_init.argtypes = [u32, u32, u32, i32, C.POINTER(C.c_int)]
        L.speexhip_resampler_destroy.argtypes = [p]
        L.speexhip_resampler_process_interleaved_int.restype = i32
        L.speexhip_resampler_process_interleaved_int.argtypes = [p, pi16, pu32, pi16, pu32]
        L.speexhip_resampler_process_interleaved_int_device.restype = i32
        L.speexhip_resampler_process_interleaved_int_device.argtypes = [p, p, pu32, p, pu32, p]
        pf32 = C.POINTER(C.c_float)
        L.speexhip_resampler_process_interleaved_float.restype = i32
        L.speexhip_resampler_process_interleaved_float.argtypes = [p, pf32, pu32, pf32, pu32]
        L.speexhip_resampler_process_interleaved_float_device.restype = i32
        L.speexhip_resampler_process_interleaved_float_device.argtypes = [p, p, pu32, p, pu32, p]
        L.speexhip_batch_process_interleaved_float_device.restype = i32
        L.speexhip_batch_process_interleaved_float_device.argtypes = [p, p, C.c_uint64, pu32, p,
                                                                      C.c_uint64, pu32, p]
        L.speexhip_resampler_get_rate.argtypes = [p, pu32, pu32]
        L.speexhip_resampler_strerror.restype = C.c_char_p
        L.speexhip_resampler_strerror.argtypes = [i32]
        L.speexhip_resampler_set_mode.restype = i32
        L.speexhip_resampler_set_mode.argtypes = [p, i32]
        L.speexhip_resampler_get_info.restype = i32
        L.speexhip_resampler_get_info.argtypes = [p, C.POINTER(Info)]
        L.speexhip_resampler_get_history.restype = i32
        L.speexhip_resampler_get_history.argtypes = [p, C.POINTER(C.c_float)]
        L.speexhip_batch_init.restype = p
        L.speexhip_batch_init.argtypes = [u32, u32, u32, u32, i32, C.POINTER(C.c_int)]
        L.speexhip_batch_destroy.argtypes = [p]
        L.speexhip_batch_set_mode.restype = i32
        L.speexhip_batch_set_mode.argtypes = [p, i32]
        # (an older build of the library loaded through SPEEXHIP_LIB_PATH for a same-box A/B lacks the entry points
        #  of later rounds: they stay unbound there)
        if hasattr(L, "speexhip_block_release") or "SPEEXHIP_LIB_PATH" not in os.environ:
            for fn, st in ((L.speexhip_resampler_process_interleaved_int_take, C.c_int16),
                           (L.speexhip_resampler_process_interleaved_float_take, C.c_float)):
                fn.restype = i32
                fn.argtypes = [p, C.c_void_p, pu32, pu32, C.POINTER(C.POINTER(st))]
            L.speexhip_block_release.restype = None
            L.speexhip_block_release.argtypes = [C.c_void_p]
            L.speexhip_debug_device_clock.restype = i32
            L.speexhip_debug_device_clock.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
            L.speexhip_resampler_release_stream.restype = i32
            L.speexhip_resampler_release_stream.argtypes = [p]
            L.speexhip_batch_release_stream.restype = i32
            L.speexhip_batch_release_stream.argtypes = [p]
        L.speexhip_batch_get_info.restype = i32
        L.speexhip_batch_get_info.argtypes = [p, u32, C.POINTER(Info)]
        L.speexhip_batch_process_interleaved_int_device.restype = i32
        L.speexhip_batch_process_interleaved_int_device.argtypes = [p, p, C.c_uint64, pu32, p,
                                                                    C.c_uint64, pu32, p]
        L.speexhip_design_filter.restype = i32
        L.speexhip_design_filter.argtypes = [u32, u32, i32, C.POINTER(Info), C.POINTER(C.c_float), u32]
        L.speexhip_plan_call.restype = i32
        L.speexhip_plan_call.argtypes = [u32, u32, u32, u32, C.POINTER(C.c_int32), pu32, pu32, pu32]
        L.speexhip_version.restype = C.c_char_p
        pi32 = C.POINTER(C.c_int32)
        L.speexhip_resampler_init_frac.restype = p
        L.speexhip_resampler_init_frac.argtypes = [u32, u32, u32, u32, u32, i32, C.POINTER(C.c_int)]
        L.speexhip_resampler_set_rate.argtypes = [p, u32, u32]
        L.speexhip_resampler_set_rate_frac.argtypes = [p, u32, u32, u32, u32]
        L.speexhip_resampler_get_ratio.argtypes = [p, pu32, pu32]
        L.speexhip_resampler_set_quality.argtypes = [p, i32]
        L.speexhip_resampler_get_quality.argtypes = [p, C.POINTER(C.c_int)]
        for f in (L.speexhip_resampler_get_input_latency, L.speexhip_resampler_get_output_latency,
                  L.speexhip_resampler_skip_zeros, L.speexhip_resampler_reset_mem,
                  L.speexhip_batch_skip_zeros, L.speexhip_batch_reset_mem):
            f.restype = i32
            f.argtypes = [p]
        L.speexhip_batch_set_rate_frac.argtypes = [p, u32, u32, u32, u32]
        L.speexhip_batch_set_quality.argtypes = [p, i32]
        L.speexhip_batch_get_history.argtypes = [p, u32, C.POINTER(C.c_float)]
        L.speexhip_design_filter_frac.restype = i32
        L.speexhip_design_filter_frac.argtypes = [u32, u32, u32, u32, i32, C.POINTER(Info),
                                                  C.POINTER(C.c_float), u32]
        L.speexhip_plan_call_ex.restype = i32
        L.speexhip_plan_call_ex.argtypes = [u32, u32, u32, u32, i32, u32, pi32, pu32, pu32, pu32, pu32]
        L.speexhip_plan_filter_change.restype = i32
        L.speexhip_plan_filter_change.argtypes = [u32, u32, u32, C.POINTER(C.c_int64), pu32, pi32, pu32, u32, u32]
        for f in (L.speexhip_resampler_process_chunks_int, L.speexhip_resampler_process_chunks_float):
            f.restype = i32
            f.argtypes = [p, u32, C.POINTER(C.c_void_p), pu32, p, pu32]
        L.speexhip_resampler_peek.restype = i32
        L.speexhip_resampler_peek.argtypes = [p, u32, u32, i32, pu32, pu32]
        L.speexhip_resampler_process_int.restype = i32
        L.speexhip_resampler_process_int.argtypes = [p, u32, pi16, pu32, pi16, pu32]
        L.speexhip_resampler_process_float.restype = i32
        L.speexhip_resampler_process_float.argtypes = [p, u32, pf32, pu32, pf32, pu32]
        for f in (L.speexhip_resampler_set_input_stride, L.speexhip_resampler_set_output_stride):
            f.restype = None
            f.argtypes = [p, u32]
        for f in (L.speexhip_resampler_get_input_stride, L.speexhip_resampler_get_output_stride):
            f.restype = None
            f.argtypes = [p, pu32]
        L.speexhip_resampler_get_channel_position.restype = i32
        L.speexhip_resampler_get_channel_position.argtypes = [p, u32, pi32, pu32, pu32]
        L.speexhip_debug_fail_device_allocs.restype = None
        L.speexhip_debug_fail_device_allocs.argtypes = [i32]
        L.speexhip_debug_plan.restype = C.c_int
        L.speexhip_debug_plan.argtypes = [u32, u32, i32, u32, C.POINTER(u32)]
        L.speexhip_release_cached_memory.restype = C.c_uint64
        L.speexhip_release_cached_memory.argtypes = []
        if hasattr(L, "speexhip_resampler_process_many_int") or "SPEEXHIP_LIB_PATH" not in os.environ:
            L.speexhip_device_count.restype = i32
            L.speexhip_device_count.argtypes = []
            L.speexhip_resampler_init_on.restype = p
            L.speexhip_resampler_init_on.argtypes = [i32, u32, u32, u32, i32, C.POINTER(C.c_int)]
            L.speexhip_batch_init_on.restype = p
            L.speexhip_batch_init_on.argtypes = [i32, u32, u32, u32, u32, i32, C.POINTER(C.c_int)]
            for f in (L.speexhip_resampler_process_many_int, L.speexhip_resampler_process_many_float):
                f.restype = i32
                f.argtypes = [u32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), pu32, C.POINTER(C.c_void_p), pu32,
                              C.POINTER(C.c_int)]
            L.speexhip_resampler_get_info2.restype = i32
            L.speexhip_resampler_get_info2.argtypes = [p, C.c_void_p, u32]
            L.speexhip_warmup.restype = i32
            L.speexhip_warmup.argtypes = [i32]
            L.speexhip_debug_placement.restype = i32
            L.speexhip_debug_placement.argtypes = [i32, C.c_char_p, C.c_char_p, C.c_uint64, i32]
        if hasattr(L, "speexhip_block_acquire") or "SPEEXHIP_LIB_PATH" not in os.environ:
            L.speexhip_block_acquire.restype = C.c_void_p
            L.speexhip_block_acquire.argtypes = [C.c_uint64]
            L.speexhip_debug_placement_live.restype = i32
            L.speexhip_debug_placement_live.argtypes = [i32, C.c_char_p, C.c_char_p, C.c_uint64, i32, C.POINTER(C.c_uint32)]
            L.speexhip_debug_live_states.restype = C.c_uint32
            L.speexhip_debug_live_states.argtypes = [i32]
            L.speexhip_debug_pcie_peak.restype = i32
            L.speexhip_debug_pcie_peak.argtypes = [C.c_uint64, i32, C.POINTER(C.c_double)]
        if hasattr(L, "speexhip_resampler_process_planar_int") or "SPEEXHIP_LIB_PATH" not in os.environ:
            u64 = C.c_uint64
            for f in (L.speexhip_resampler_process_planar_int, L.speexhip_resampler_process_planar_float):
                f.restype = i32
                f.argtypes = [p, C.POINTER(C.c_void_p), pu32, C.POINTER(C.c_void_p), pu32]
            for f in (L.speexhip_resampler_process_planar_int_device, L.speexhip_resampler_process_planar_float_device):
                f.restype = i32
                f.argtypes = [p, p, u64, pu32, p, u64, pu32, p]
            for f in (L.speexhip_batch_process_planar_int_device, L.speexhip_batch_process_planar_float_device):
                f.restype = i32
                f.argtypes = [p, p, u64, u64, pu32, p, u64, u64, pu32, p]
        if hasattr(L, "speexhip_sample_bytes") or "SPEEXHIP_LIB_PATH" not in os.environ:
            u64 = C.c_uint64
            L.speexhip_sample_bytes.restype = u32
            L.speexhip_sample_bytes.argtypes = [i32]
            L.speexhip_resampler_process_interleaved_fmt.restype = i32
            L.speexhip_resampler_process_interleaved_fmt.argtypes = [p, i32, p, pu32, i32, p, pu32]
            L.speexhip_resampler_process_interleaved_fmt_device.restype = i32
            L.speexhip_resampler_process_interleaved_fmt_device.argtypes = [p, i32, p, pu32, i32, p, pu32, p]
            L.speexhip_batch_process_interleaved_fmt_device.restype = i32
            L.speexhip_batch_process_interleaved_fmt_device.argtypes = [p, i32, p, u64, pu32, i32, p, u64, pu32, p]
        if hasattr(L, "speexhip_resampler_process_interleaved_mix") or "SPEEXHIP_LIB_PATH" not in os.environ:
            u64 = C.c_uint64
            L.speexhip_resampler_process_interleaved_mix.restype = i32
            L.speexhip_resampler_process_interleaved_mix.argtypes = [p, i32, u32, p, p, pu32, i32, u32, p, p, pu32]
            L.speexhip_resampler_process_interleaved_mix_device.restype = i32
            L.speexhip_resampler_process_interleaved_mix_device.argtypes = [p, i32, u32, p, p, pu32, i32, u32, p, p, pu32, p]
            L.speexhip_batch_process_interleaved_mix_device.restype = i32
            L.speexhip_batch_process_interleaved_mix_device.argtypes = [p, i32, u32, p, p, u64, pu32, i32, u32, p, p, u64,
                                                                        pu32, p]
        if hasattr(L, "speexhip_resampler_set_dither") or "SPEEXHIP_LIB_PATH" not in os.environ:
            u64, pu64 = C.c_uint64, C.POINTER(C.c_uint64)
            L.speexhip_resampler_set_dither.restype = i32
            L.speexhip_resampler_set_dither.argtypes = [p, i32, u64, u64]
            L.speexhip_resampler_get_dither.restype = i32
            L.speexhip_resampler_get_dither.argtypes = [p, C.POINTER(C.c_int), pu64, pu64]
            L.speexhip_batch_set_dither.restype = i32
            L.speexhip_batch_set_dither.argtypes = [p, i32, u64, u64]
            L.speexhip_batch_get_dither.restype = i32
            L.speexhip_batch_get_dither.argtypes = [p, u32, C.POINTER(C.c_int), pu64, pu64]
            L.speexhip_debug_dither.restype = i32
            L.speexhip_debug_dither.argtypes = [i32, u64, u64, u32, C.POINTER(C.c_double)]
        if hasattr(L, "speexhip_debug_g711_decode") or "SPEEXHIP_LIB_PATH" not in os.environ:
            L.speexhip_debug_g711_decode.restype = i32
            L.speexhip_debug_g711_decode.argtypes = [i32, p, u32, p]
            L.speexhip_debug_g711_encode.restype = i32
            L.speexhip_debug_g711_encode.argtypes = [i32, p, p, u32, p]
        if hasattr(L, "speexhip_debug_format_decode") or "SPEEXHIP_LIB_PATH" not in os.environ:
            L.speexhip_debug_format_decode.restype = i32
            L.speexhip_debug_format_decode.argtypes = [i32, p, u32, p]
            L.speexhip_debug_format_encode.restype = i32
            L.speexhip_debug_format_encode.argtypes = [i32, p, p, u32, p]
        if hasattr(L, "speexhip_resampler_process_sides") or "SPEEXHIP_LIB_PATH" not in os.environ:
            ps = C.POINTER(Side)
            L.speexhip_resampler_process_sides.restype = i32
            L.speexhip_resampler_process_sides.argtypes = [p, ps, pu32, ps, pu32]
            L.speexhip_resampler_process_sides_device.restype = i32
            L.speexhip_resampler_process_sides_device.argtypes = [p, ps, pu32, ps, pu32, p]
            L.speexhip_batch_process_sides_device.restype = i32
            L.speexhip_batch_process_sides_device.argtypes = [p, ps, pu32, ps, pu32, p]
        if hasattr(L, "speexhip_resampler_process_many_sides") or "SPEEXHIP_LIB_PATH" not in os.environ:
            ps, pp, pi = C.POINTER(Side), C.POINTER(C.c_void_p), C.POINTER(C.c_int)
            L.speexhip_resampler_process_many_sides.restype = i32
            L.speexhip_resampler_process_many_sides.argtypes = [u32, pp, ps, pu32, ps, pu32, pi]
            L.speexhip_resampler_process_many_fmt.restype = i32
            L.speexhip_resampler_process_many_fmt.argtypes = [u32, pp, pi, pp, pu32, pi, pp, pu32, pi]
            L.speexhip_debug_many_counters.restype = None
            L.speexhip_debug_many_counters.argtypes = [C.POINTER(C.c_uint64)]
        if hasattr(L, "speexhip_resampler_process_chunks_sides") or "SPEEXHIP_LIB_PATH" not in os.environ:
            ps, pp = C.POINTER(Side), C.POINTER(C.c_void_p)
            L.speexhip_resampler_process_chunks_sides.restype = i32
            L.speexhip_resampler_process_chunks_sides.argtypes = [p, u32, ps, pp, pu32, ps, pu32]
            L.speexhip_resampler_process_chunks_fmt.restype = i32
            L.speexhip_resampler_process_chunks_fmt.argtypes = [p, u32, i32, pp, pu32, i32, p, pu32]
            L.speexhip_debug_chunk_counters.restype = None
            L.speexhip_debug_chunk_counters.argtypes = [C.POINTER(C.c_uint64)]
        if hasattr(L, "speexhip_resampler_set_meter") or "SPEEXHIP_LIB_PATH" not in os.environ:
            pm = C.POINTER(Meter)
            L.speexhip_resampler_set_meter.restype = i32
            L.speexhip_resampler_set_meter.argtypes = [p, i32]
            L.speexhip_resampler_get_meter.restype = i32
            L.speexhip_resampler_get_meter.argtypes = [p, pm, i32]
            L.speexhip_batch_set_meter.restype = i32
            L.speexhip_batch_set_meter.argtypes = [p, i32]
            L.speexhip_batch_get_meter.restype = i32
            L.speexhip_batch_get_meter.argtypes = [p, u32, pm, i32]
            L.speexhip_debug_meter.restype = i32
            L.speexhip_debug_meter.argtypes = [i32, p, p, u32, pm]
        if hasattr(L, "speexhip_resampler_set_gain") or "SPEEXHIP_LIB_PATH" not in os.environ:
            pf = C.POINTER(C.c_float)
            L.speexhip_resampler_set_gain.restype = i32
            L.speexhip_resampler_set_gain.argtypes = [p, C.c_float, u32]
            L.speexhip_resampler_get_gain.restype = i32
            L.speexhip_resampler_get_gain.argtypes = [p, pf, pf, pu32]
            L.speexhip_batch_set_gain.restype = i32
            L.speexhip_batch_set_gain.argtypes = [p, u32, C.c_float, u32]
            L.speexhip_batch_get_gain.restype = i32
            L.speexhip_batch_get_gain.argtypes = [p, u32, pf, pf, pu32]
            L.speexhip_debug_gain.restype = i32
            L.speexhip_debug_gain.argtypes = [C.c_float, C.c_float, u32, C.c_uint64, u32, pf]
        if hasattr(L, "speexhip_batch_set_buses") or "SPEEXHIP_LIB_PATH" not in os.environ:
            L.speexhip_batch_set_buses.restype = i32
            L.speexhip_batch_set_buses.argtypes = [p, u32, p]
            L.speexhip_batch_get_buses.restype = i32
            L.speexhip_batch_get_buses.argtypes = [p, pu32, p]
            L.speexhip_batch_process_bus_device.restype = i32
            L.speexhip_batch_process_bus_device.argtypes = [p, C.POINTER(Side), pu32, C.POINTER(Side), pu32, pu32, p]
            L.speexhip_batch_get_bus_meter.restype = i32
            L.speexhip_batch_get_bus_meter.argtypes = [p, u32, C.POINTER(Meter), i32]
            L.speexhip_batch_get_bus_position.restype = i32
            L.speexhip_batch_get_bus_position.argtypes = [p, C.POINTER(C.c_uint64)]
            L.speexhip_debug_bus.restype = i32
            L.speexhip_debug_bus.argtypes = [u32, u32, p, p, u32, p]
        if hasattr(L, "speexhip_mixer_init") or "SPEEXHIP_LIB_PATH" not in os.environ:
            pu64 = C.POINTER(C.c_uint64)
            L.speexhip_mixer_init.restype = p
            L.speexhip_mixer_init.argtypes = [u32, u32, u32, C.POINTER(i32)]
            L.speexhip_mixer_init_on.restype = p
            L.speexhip_mixer_init_on.argtypes = [i32, u32, u32, u32, C.POINTER(i32)]
            L.speexhip_mixer_destroy.restype = None
            L.speexhip_mixer_destroy.argtypes = [p]
            L.speexhip_mixer_set_weights.restype = i32
            L.speexhip_mixer_set_weights.argtypes = [p, p]
            L.speexhip_mixer_get_weights.restype = i32
            L.speexhip_mixer_get_weights.argtypes = [p, p]
            L.speexhip_mixer_set_dither.restype = i32
            L.speexhip_mixer_set_dither.argtypes = [p, i32, C.c_uint64, C.c_uint64]
            L.speexhip_mixer_get_dither.restype = i32
            L.speexhip_mixer_get_dither.argtypes = [p, C.POINTER(i32), pu64, pu64]
            L.speexhip_mixer_set_meter.restype = i32
            L.speexhip_mixer_set_meter.argtypes = [p, i32]
            L.speexhip_mixer_get_bus_meter.restype = i32
            L.speexhip_mixer_get_bus_meter.argtypes = [p, u32, C.POINTER(Meter), i32]
            L.speexhip_mixer_process.restype = i32
            L.speexhip_mixer_process.argtypes = [p, p, C.POINTER(Side), pu32, pu32, C.POINTER(Side), pu32, C.POINTER(i32)]
            L.speexhip_debug_mixer_counters.restype = None
            L.speexhip_debug_mixer_counters.argtypes = [pu64]
        if hasattr(L, "speexhip_mixer_set_levels") or "SPEEXHIP_LIB_PATH" not in os.environ:
            # (as above: a build without the mixer's levels)
            L.speexhip_mixer_set_levels.restype = i32
            L.speexhip_mixer_set_levels.argtypes = [p, i32]
            L.speexhip_mixer_get_levels.restype = i32
            L.speexhip_mixer_get_levels.argtypes = [p, u32, u32, p, u32]
            L.speexhip_debug_levels.restype = i32
            L.speexhip_debug_levels.argtypes = [p, u32, p]
            L.speexhip_debug_mixer_level_launches.restype = C.c_uint64
            L.speexhip_debug_mixer_level_launches.argtypes = []
        _lib = L
    return _lib


def strerror(code):
    return lib().speexhip_resampler_strerror(code).decode()


def design_filter(in_rate, out_rate, quality, want_table=True):
    """Host-only filter design; returns (info dict, table float32 array or None)."""
    info = Info()
    rc = lib().speexhip_design_filter(in_rate, out_rate, quality, C.byref(info), None, 0)
    if rc != 0:
        raise ValueError(strerror(rc))
    table = None
    if want_table:
        table = np.zeros(info.sinc_table_length, np.float32)
        rc = lib().speexhip_design_filter(in_rate, out_rate, quality, C.byref(info),
                                          table.ctypes.data_as(C.POINTER(C.c_float)), table.size)
        assert rc == 0
    return info.as_dict(), table


def plan_call(num, den, in_len, out_cap, last, frac):
    """Host-only stream bookkeeping; returns (consumed, produced, last', frac')."""
    l, f, c, p = C.c_int32(last), C.c_uint32(frac), C.c_uint32(), C.c_uint32()
    rc = lib().speexhip_plan_call(num, den, in_len, out_cap, C.byref(l), C.byref(f), C.byref(c),
                                  C.byref(p))
    if rc != 0:
        raise ValueError(strerror(rc))
    return c.value, p.value, l.value, f.value


def design_filter_frac(ratio_num, ratio_den, in_rate, out_rate, quality):
    """Host-only filter geometry for a ratio given separately from the rates; info dict."""
    info = Info()
    rc = lib().speexhip_design_filter_frac(ratio_num, ratio_den, in_rate, out_rate, quality,
                                           C.byref(info), None, 0)
    if rc != 0:
        raise ValueError(strerror(rc))
    return info.as_dict()


def plan_call_ex(num, den, in_len, out_cap, float_entry, block_in, last, frac, magic):
    """Host-only bookkeeping of one call for any entry point / state;
    returns (consumed, produced, last', frac', magic')."""
    l, f, m, c, p = C.c_int32(last), C.c_uint32(frac), C.c_uint32(magic), C.c_uint32(), C.c_uint32()
    rc = lib().speexhip_plan_call_ex(num, den, in_len, out_cap, int(float_entry), block_in, C.byref(l),
                                     C.byref(f), C.byref(m), C.byref(c), C.byref(p))
    if rc != 0:
        raise ValueError(strerror(rc))
    return c.value, p.value, l.value, f.value, m.value


def debug_dither(kind, seed, first_index, n):
    """host-only: the library's dither values d (float64, in LSB) of sample indices first_index .. first_index + n - 1"""
    d = np.zeros(max(int(n), 1), np.float64)
    rc = lib().speexhip_debug_dither(kind, seed, first_index, n, d.ctypes.data_as(C.POINTER(C.c_double)))
    if rc:
        raise ValueError(strerror(rc))
    return d[:n]


def debug_gain(from_gain, to_gain, total, first, n):
    """host-only: the library's gains g(first) .. g(first + n - 1) (float32) of the ramp (from_gain, to_gain, total)"""
    g = np.zeros(max(int(n), 1), np.float32)
    rc = lib().speexhip_debug_gain(from_gain, to_gain, total, first, n, g.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise ValueError(strerror(rc))
    return g[:n]


def debug_bus(weights, y):
    """host-only: the library's bus sums z (n_buses, n) float32 of the (already gained) stream samples y (n_streams, n)
    under the matrix weights (n_buses, n_streams): the very statement the kernel compiles"""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if w.ndim != 2 or y.ndim != 2 or w.shape[1] != y.shape[0]:
        raise ValueError("weights (n_buses, n_streams) and y (n_streams, n)")
    z = np.zeros((w.shape[0], max(y.shape[1], 1)), np.float32)[:, : y.shape[1]]
    z = np.ascontiguousarray(z)
    rc = lib().speexhip_debug_bus(w.shape[1], w.shape[0], C.c_void_p(w.ctypes.data), C.c_void_p(y.ctypes.data), y.shape[1],
                                  C.c_void_p(z.ctypes.data))
    if rc:
        raise ValueError(strerror(rc))
    return z


def debug_meter(fmt, y, d=None):
    """host-only: the library's meter over FIR values y (float32, int16 units) on their way to format fmt; d: None or the
    dither of each sample (float64, in LSB of the format; the formats of dithered_fmt only).  The totals as a dict
    (get_meter's, without 'on')."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    if d is not None:
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
        if d.size != y.size:
            raise ValueError("one dither value per sample")
    m = Meter()
    rc = lib().speexhip_debug_meter(fmt, C.c_void_p(y.ctypes.data), C.c_void_p(d.ctypes.data) if d is not None else None,
                                    y.size, C.byref(m))
    if rc:
        raise ValueError(strerror(rc))
    out = m.as_dict()
    del out["on"]
    return out


def debug_g711_decode(fmt, codes):
    """host-only: the library's decoding of G.711 bytes (FMT_ULAW / FMT_ALAW) into the internal float (int16 units)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    x = np.zeros(max(codes.size, 1), np.float32)
    rc = lib().speexhip_debug_g711_decode(fmt, C.c_void_p(codes.ctypes.data), codes.size, C.c_void_p(x.ctypes.data))
    if rc:
        raise ValueError(strerror(rc))
    return x[: codes.size]


def debug_g711_encode(fmt, y, d=None):
    """host-only: the library's G.711 bytes of FIR values y (float32, int16 units); d: None or the dither of each
    sample (float64, in int16 steps) added before the rounding"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    if d is not None:
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
        assert d.size == y.size
    codes = np.zeros(max(y.size, 1), np.uint8)
    rc = lib().speexhip_debug_g711_encode(fmt, C.c_void_p(y.ctypes.data), None if d is None else C.c_void_p(d.ctypes.data),
                                          y.size, C.c_void_p(codes.ctypes.data))
    if rc:
        raise ValueError(strerror(rc))
    return codes[: y.size]


def debug_format_decode(fmt, storage):
    """host-only: the library's decoding of storage of a half-float or big-endian format (FMT_F16N, FMT_BF16N, FMT_S16BE,
    FMT_S24BE, FMT_S32BE; an array of fmt_dtype(fmt), its bytes taken as they are) into the internal float (int16 units)"""
    storage = np.ascontiguousarray(storage, dtype=fmt_dtype(fmt)).reshape(-1)
    n = storage.nbytes // fmt_bytes(fmt)
    x = np.zeros(max(n, 1), np.float32)
    rc = lib().speexhip_debug_format_decode(fmt, C.c_void_p(storage.ctypes.data), n, C.c_void_p(x.ctypes.data))
    if rc:
        raise ValueError(strerror(rc))
    return x[:n]


def debug_format_encode(fmt, y, d=None):
    """host-only: the library's storage (flat, fmt_dtype(fmt)) of FIR values y (float32, int16 units) in a half-float or
    big-endian format; d: None or, for the big-endian formats, the dither of each sample (float64, in LSB of the format)
    added before the rounding"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    if d is not None:
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
        assert d.size == y.size
    raw = np.zeros(max(y.size, 1) * fmt_bytes(fmt), np.uint8)
    rc = lib().speexhip_debug_format_encode(fmt, C.c_void_p(y.ctypes.data), None if d is None else C.c_void_p(d.ctypes.data),
                                            y.size, C.c_void_p(raw.ctypes.data))
    if rc:
        raise ValueError(strerror(rc))
    return raw[: y.size * fmt_bytes(fmt)].view(fmt_dtype(fmt))


def debug_plan64(ratio_num, ratio_den, quality, channels):
    """the round-4 plans: fp64-accumulate kernels (fast_path 5 / 4) or phase pairs for mono (6); host-only"""
    out = (C.c_uint32 * 8)()
    rc = lib().speexhip_debug_plan64(ratio_num, ratio_den, quality, channels, out)
    if rc:
        raise ValueError(strerror(rc))
    v = list(out)
    return {"fast_path": v[0], "r_or_p": v[1], "lane_periods": v[2], "row_len": v[3], "lds_bytes": v[4],
            "pad_or_stride": v[5], "trips": v[6], "last": v[7]}


def debug_launch_shape(ratio_num, ratio_den, quality, channels, streams, frames, float_io=False):
    """host-only: the period kernel's launch for a first call of `frames` frames on each of `streams` streams"""
    out = (C.c_uint32 * 10)()
    rc = lib().speexhip_debug_launch_shape(ratio_num, ratio_den, quality, channels, streams, frames, int(float_io), out)
    if rc:
        raise ValueError(strerror(rc))
    v = list(out)
    return {"phase_pairs": bool(v[0]), "r": v[1], "int16_window": bool(v[2]), "lane_periods": v[3], "tiles": v[4],
            "splits": v[5], "wave_groups": v[6], "shares": v[7], "threads": v[8], "touch": bool(v[9])}


def device_count():
    """logical devices the library can place states on (speexhip_device_count)"""
    return lib().speexhip_device_count()


def placement(device_count_, env_device, env_devices, k, current=0):
    """host-only: the placement rule (speexhip_debug_placement); None = unset environment variable"""
    enc = lambda v: None if v is None else str(v).encode()
    return lib().speexhip_debug_placement(device_count_, enc(env_device), enc(env_devices), k, current)


def placement_live(device_count_, env_device, env_devices, k, current, live):
    """host-only: the placement rule with live state counts per device (speexhip_debug_placement_live)"""
    enc = lambda v: None if v is None else str(v).encode()
    arr = (C.c_uint32 * max(len(live), 1))(*live)
    return lib().speexhip_debug_placement_live(device_count_, enc(env_device), enc(env_devices), k, current, arr)


def process_many(states, chunks, capacities, dtype=np.int16):
    """speexhip_resampler_process_many_int / _float: chunks[i] (frames x channels, or None with capacities[i] =
    (null_frames, capacity)) through states[i], all in one call.  Returns (outputs, consumed, codes)."""
    n = len(states)
    hs, ins, outs = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    il, ol, codes = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int * n)()
    keep, bufs = [], []
    for i, (st, ch_) in enumerate(zip(states, chunks)):
        hs[i] = st._h
        if ch_ is None:
            ins[i], il[i], ol[i] = None, capacities[i][0], capacities[i][1]
        else:
            a = np.ascontiguousarray(ch_, dtype=dtype).reshape(-1, st.channels)
            keep.append(a)
            ins[i], il[i], ol[i] = a.ctypes.data, a.shape[0], capacities[i]
        b = np.zeros((max(int(ol[i]), 1), st.channels), dtype)
        bufs.append(b)
        outs[i] = b.ctypes.data
    fn = lib().speexhip_resampler_process_many_int if dtype == np.int16 else lib().speexhip_resampler_process_many_float
    rc = fn(n, hs, ins, il, outs, ol, codes)
    if rc not in (0, ERR_ALLOC_FAILED):
        raise RuntimeError(strerror(rc))
    return [bufs[i][: ol[i]].copy() for i in range(n)], list(il), list(codes)


def many_counters():
    """speexhip_debug_many_counters: process-wide counts of the many-states calls since start, as a dict -- fir_launches,
    in_passes, out_passes, own_calls (entries that took their own call)."""
    v = (C.c_uint64 * 4)()
    lib().speexhip_debug_many_counters(v)
    return dict(zip(("fir_launches", "in_passes", "out_passes", "own_calls"), (int(x) for x in v)))


def debug_mixer_counters():
    """speexhip_debug_mixer_counters: process-wide counts of the mixer calls since start, as a dict -- fir_launches,
    in_passes, bus_sum_launches, out_passes, transfers_in, transfers_out."""
    v = (C.c_uint64 * 6)()
    lib().speexhip_debug_mixer_counters(v)
    return dict(zip(("fir_launches", "in_passes", "bus_sum_launches", "out_passes", "transfers_in", "transfers_out"),
                    (int(x) for x in v)))


def debug_mixer_level_launches():
    """speexhip_debug_mixer_level_launches: launches of the mixer levels' kernels since start (apart from the six above)"""
    return int(lib().speexhip_debug_mixer_level_launches())


def debug_levels(y, into=None):
    """host-only: the library's level statement (csrc/levels.h) over float32 values y in int16 units, accumulated into the
    record `into` (a LEVEL_DTYPE array of one record; None: a fresh one).  Returns the record array."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    rec = np.zeros(1, LEVEL_DTYPE) if into is None else into
    rc = lib().speexhip_debug_levels(C.c_void_p(y.ctypes.data) if y.size else None, y.size, C.c_void_p(rec.ctypes.data))
    if rc:
        raise RuntimeError(strerror(rc))
    return rec


def audio_level(rec):
    """The RFC 6464 audio level of a level record (a LEVEL_DTYPE record, or anything with 'energy' and 'samples'): -dBov
    of the RMS, full scale = 2^15, as an integer 0 (loudest) .. 127; 127 for no energy or no samples."""
    energy, samples = int(rec["energy"]), int(rec["samples"])
    if energy == 0 or samples == 0:
        return 127
    return int(min(127, max(0, round(-10.0 * math.log10(energy / (samples * 2.0 ** 30))))))


def chunk_counters():
    """speexhip_debug_chunk_counters: process-wide counts of the formatted chunks calls since start, as a dict --
    fir_launches, in_passes, out_passes, own_calls (chunks that took a call of their own)."""
    v = (C.c_uint64 * 4)()
    lib().speexhip_debug_chunk_counters(v)
    return dict(zip(("fir_launches", "in_passes", "out_passes", "own_calls"), (int(x) for x in v)))


def release_cached_memory():
    """speexhip_release_cached_memory: hands every idle pooled buffer and cached table back to the device; bytes freed"""
    return int(lib().speexhip_release_cached_memory())


def _per_state(v, n):
    """one value for all states, or a sequence with one per state"""
    return [int(v)] * n if isinstance(v, (int, np.integer)) else [int(f) for f in v]


def many_fmt_call(states, in_fmts, in_ptrs, in_lens, out_fmts, out_ptrs, capacities):
    """speexhip_resampler_process_many_fmt itself, on addresses (None = NULL; a state may be None too): returns
    (rc, consumed, produced, codes)."""
    n = len(states)
    hs, ins, outs = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    fi, fo = (C.c_int * n)(*_per_state(in_fmts, n)), (C.c_int * n)(*_per_state(out_fmts, n))
    il, ol, codes = (C.c_uint32 * n)(*in_lens), (C.c_uint32 * n)(*capacities), (C.c_int * n)()
    for i in range(n):
        hs[i] = None if states[i] is None else states[i]._h
        ins[i], outs[i] = in_ptrs[i], out_ptrs[i]
    rc = lib().speexhip_resampler_process_many_fmt(n, hs, fi, ins, il, fo, outs, ol, codes)
    return rc, list(il), list(ol), list(codes)


def process_many_fmt(states, chunks, in_fmts, out_fmts, capacities):
    """speexhip_resampler_process_many_fmt: chunks[i] -- whole interleaved frames of in_fmts[i]'s storage type, or None
    (silence) with capacities[i] = (null_frames, capacity) -- through states[i] into out_fmts[i], all in one fused call.
    in_fmts / out_fmts: one FMT_* for all states or one per state.  Returns (outputs, consumed, codes); outputs[i] is flat,
    of out_fmts[i]'s storage type (the packed 24-bit formats: three bytes per sample)."""
    n = len(states)
    fi, fo = _per_state(in_fmts, n), _per_state(out_fmts, n)
    keep, bufs, ins, outs, il, ol = [], [], [], [], [], []
    for i, (st, ch_) in enumerate(zip(states, chunks)):
        if ch_ is None:
            ins.append(None), il.append(int(capacities[i][0])), ol.append(int(capacities[i][1]))
        else:
            a = np.ascontiguousarray(ch_, dtype=fmt_dtype(fi[i])).reshape(-1)
            frames = a.nbytes // (fmt_bytes(fi[i]) * st.channels)
            if frames * fmt_bytes(fi[i]) * st.channels != a.nbytes:
                raise ValueError("chunk %d: whole frames only" % i)
            keep.append(a)
            ins.append(a.ctypes.data), il.append(frames), ol.append(int(capacities[i]))
        b = np.zeros(max(ol[i], 1) * st.channels * fmt_bytes(fo[i]), np.uint8)
        bufs.append(b)
        outs.append(b.ctypes.data)
    rc, used, made, codes = many_fmt_call(states, fi, ins, il, fo, outs, ol)
    if rc not in (0, ERR_ALLOC_FAILED):
        raise RuntimeError(strerror(rc))
    return ([bufs[i][: made[i] * states[i].channels * fmt_bytes(fo[i])].view(fmt_dtype(fo[i])).copy() for i in range(n)],
            used, codes)


def process_many_sides(states, in_sides, in_lens, out_sides, capacities):
    """speexhip_resampler_process_many_sides: in_sides[i] / out_sides[i] = the Side structures (make_side, host buffers the
    caller keeps alive) of states[i]'s entry, in_lens[i] / capacities[i] its frames.  Returns (rc, consumed, produced,
    codes); the results lie in the callers' buffers."""
    n = len(states)
    hs = (C.c_void_p * n)()
    a, b = (Side * n)(), (Side * n)()
    for i in range(n):
        hs[i] = None if states[i] is None else states[i]._h
        C.memmove(C.byref(a[i]), C.byref(in_sides[i]), C.sizeof(Side))
        C.memmove(C.byref(b[i]), C.byref(out_sides[i]), C.sizeof(Side))
    il, ol, codes = (C.c_uint32 * n)(*in_lens), (C.c_uint32 * n)(*capacities), (C.c_int * n)()
    rc = lib().speexhip_resampler_process_many_sides(n, hs, a, il, b, ol, codes)
    return rc, list(il), list(ol), list(codes)


class PinnedBlock:
    """A pinned block of the library the caller fills (speexhip_block_acquire, round 6): `.array(dtype, shape)` is a
    numpy view of it; the host-buffer calls use such memory in place -- the kernel reads it through PCIe.  Raises
    MemoryError when no block is free.  close() (or the context manager) gives it back."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().speexhip_block_acquire(self.nbytes)
        if not self.ptr:
            raise MemoryError("speexhip_block_acquire(%d): no pinned block free" % self.nbytes)

    def array(self, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.nbytes
        buf = (C.c_char * n).from_address(self.ptr)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def close(self):
        if self.ptr:
            lib().speexhip_block_release(C.c_void_p(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def pcie_peak(nbytes, reps=6):
    """(h2d, d2h, each way with both at once) GB/s of plain pinned copies of nbytes: speexhip_debug_pcie_peak"""
    out = (C.c_double * 3)()
    rc = lib().speexhip_debug_pcie_peak(int(nbytes), int(reps), out)
    if rc:
        raise RuntimeError(strerror(rc))
    return tuple(out)


def device_clock():
    """(median GHz, slowest workgroup's GHz) the chip holds under an FIR-like load: the kind of box this is"""
    a, b = C.c_double(), C.c_double()
    rc = lib().speexhip_debug_device_clock(C.byref(a), C.byref(b))
    if rc:
        raise RuntimeError(strerror(rc))
    return a.value, b.value


def debug_plan(ratio_num, ratio_den, quality, channels):
    """host-only: which fast kernel this configuration gets and its geometry (speexhip_debug_plan)"""
    out = (C.c_uint32 * 8)()
    rc = lib().speexhip_debug_plan(ratio_num, ratio_den, quality, channels, out)
    if rc:
        raise ValueError(strerror(rc))
    v = list(out)
    return {"fast_path": v[0], "r_or_p": v[1], "lane_periods": v[2], "row_len": v[3], "lds_bytes": v[4],
            "pad": v[5], "fine_plan": bool(v[6]),
            # slide kernel: tap steps per loop iteration (out[7] means something else for period plans)
            "steps_per_iteration": v[7] if v[0] != 2 else 0,
            # period kernel: periods per tile of the int16-window plan that int16 calls take (0 = none)
            "w16_lane_periods": v[7] if v[0] == 2 else 0}


def plan_filter_change(old_taps, new_taps, magic, phase=None, old_den=1, new_den=1):
    """Host-only: (rc, shift, new_magic, last_delta, phase')."""
    sh, nm, ld = C.c_int64(), C.c_uint32(), C.c_int32()
    ph = C.c_uint32(phase or 0)
    rc = lib().speexhip_plan_filter_change(old_taps, new_taps, magic, C.byref(sh), C.byref(nm), C.byref(ld),
                                           C.byref(ph) if phase is not None else None, old_den, new_den)
    return rc, sh.value, nm.value, ld.value, ph.value


class Resampler:
    """Thin object over the C ABI state: host-buffer ``process`` and device-pointer
    ``process_device`` (same signature as oracle.Oracle.process for the shared test driver)."""

    def __init__(self, channels, in_rate, out_rate, quality=7, mode=None, ratio=None, device=None):
        err = C.c_int(0)
        if device is not None:
            self._h = lib().speexhip_resampler_init_on(device, channels, in_rate, out_rate, quality, C.byref(err))
        elif ratio is None:
            self._h = lib().speexhip_resampler_init(channels, in_rate, out_rate, quality, C.byref(err))
        else:
            self._h = lib().speexhip_resampler_init_frac(channels, ratio[0], ratio[1], in_rate, out_rate,
                                                         quality, C.byref(err))
        if not self._h:
            raise (RuntimeError if err.value == ERR_DEVICE else ValueError)(strerror(err.value))
        self.channels = channels
        if mode is not None:
            self.set_mode(mode)
        self.refresh()

    def refresh(self):
        i = self.info()
        self.num, self.den, self.taps = i["num_rate"], i["den_rate"], i["filt_len"]
        self.oversample, self.kind = i["oversample"], KERNEL_NAMES[i["kernel"]]
        self.table_len = i["sinc_table_length"]

    # ---- mid-stream control: same method names as oracle.Oracle / oracle.Reference ----
    def set_rate(self, in_rate, out_rate):
        rc = lib().speexhip_resampler_set_rate(self._h, in_rate, out_rate)
        self.refresh()
        return rc

    def set_rate_frac(self, num, den, in_rate, out_rate):
        rc = lib().speexhip_resampler_set_rate_frac(self._h, num, den, in_rate, out_rate)
        self.refresh()
        return rc

    def set_quality(self, quality):
        rc = lib().speexhip_resampler_set_quality(self._h, quality)
        self.refresh()
        return rc

    def rate(self):
        a, b = C.c_uint32(), C.c_uint32()
        lib().speexhip_resampler_get_rate(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def ratio(self):
        a, b = C.c_uint32(), C.c_uint32()
        lib().speexhip_resampler_get_ratio(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def quality(self):
        q = C.c_int()
        lib().speexhip_resampler_get_quality(self._h, C.byref(q))
        return q.value

    def input_latency(self):
        return lib().speexhip_resampler_get_input_latency(self._h)

    def output_latency(self):
        return lib().speexhip_resampler_get_output_latency(self._h)

    def skip_zeros(self):
        return lib().speexhip_resampler_skip_zeros(self._h)

    def reset_mem(self):
        return lib().speexhip_resampler_reset_mem(self._h)

    def pending(self, c=0):
        """channel c of the pending ("magic") frames"""
        return self._lines()[self.taps - 1:, c].copy()

    def _lines(self):
        n = self.taps - 1 + self.info()["magic_samples"]
        buf = np.zeros((max(n, 1), self.channels), np.float32)
        rc = lib().speexhip_resampler_get_history(self._h, buf.ctypes.data_as(C.POINTER(C.c_float)))
        if rc:
            raise RuntimeError(strerror(rc))
        return buf[:n]

    def set_mode(self, mode):
        rc = lib().speexhip_resampler_set_mode(self._h, mode)
        if rc:
            raise ValueError(strerror(rc))

    def process_take(self, frames, out_capacity, float_io=False, keep=False):
        """The host-buffer call whose result stays in a pinned block of the library (what the N-API addon wraps in
        an external Buffer).  Returns (samples, consumed): a copy with the block released, or -- keep=True -- a
        view over the block plus the block's address as a third item (release with release_block)."""
        frames = np.ascontiguousarray(frames, dtype=np.float32 if float_io else np.int16)
        n = frames.shape[0]
        il, ol = C.c_uint32(n), C.c_uint32(out_capacity)
        ctype = C.c_float if float_io else C.c_int16
        blk = C.POINTER(ctype)()
        fn = (lib().speexhip_resampler_process_interleaved_float_take if float_io
              else lib().speexhip_resampler_process_interleaved_int_take)
        rc = fn(self._h, frames.ctypes.data_as(C.c_void_p) if n else None, C.byref(il), C.byref(ol), C.byref(blk))
        if rc == ERR_NO_BLOCK:
            raise MemoryError(strerror(rc))
        if rc:
            raise RuntimeError(strerror(rc))
        if not blk:
            empty = np.zeros((0, self.channels), dtype=frames.dtype)
            return (empty, il.value, 0) if keep else (empty, il.value)
        view = np.ctypeslib.as_array(blk, shape=(ol.value * self.channels,)).reshape(ol.value, self.channels)
        if keep:
            return view, il.value, C.cast(blk, C.c_void_p).value
        out = view.copy()
        lib().speexhip_block_release(C.cast(blk, C.c_void_p))
        return out, il.value

    @staticmethod
    def release_block(addr):
        lib().speexhip_block_release(C.c_void_p(addr))

    def release_stream(self):
        """before the caller destroys the stream of this state's last device-pointer call"""
        rc = lib().speexhip_resampler_release_stream(self._h)
        if rc:
            raise RuntimeError(strerror(rc))

    def info(self):
        i = Info()
        lib().speexhip_resampler_get_info(self._h, C.byref(i))
        return i.as_dict()

    def position(self):
        i = self.info()
        return i["last_sample"], i["samp_frac_num"]

    def history(self):
        """(taps-1, channels) float32: the reference's `mem` after the last call"""
        return self._lines()[: self.taps - 1].copy()

    # ---- raw calls: same names and results as oracle._RawMixin (return code + whole buffer) ----
    SENTINEL_I16, SENTINEL_F32 = 0x5A5A, 1234.5

    def raw_call(self, kind, x, cap, null_frames=0):
        dt, cdt, fill = ((np.int16, C.c_int16, self.SENTINEL_I16) if kind == "int" else
                         (np.float32, C.c_float, self.SENTINEL_F32))
        if x is None:
            ptr, n = None, int(null_frames)
        else:
            x = np.ascontiguousarray(x, dtype=dt).reshape(-1, self.channels)
            ptr, n = x.ctypes.data_as(C.POINTER(cdt)), x.shape[0]
        out = np.full((max(int(cap), 1), self.channels), fill, dt)
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        fn = (lib().speexhip_resampler_process_interleaved_int if kind == "int"
              else lib().speexhip_resampler_process_interleaved_float)
        rc = fn(self._h, ptr, C.byref(il), out.ctypes.data_as(C.POINTER(cdt)), C.byref(ol))
        return rc, il.value, ol.value, out

    def channel_call(self, kind, c, x, cap, in_stride=1, out_stride=1, null_frames=0):
        dt, cdt, fill = ((np.int16, C.c_int16, self.SENTINEL_I16) if kind == "int" else
                         (np.float32, C.c_float, self.SENTINEL_F32))
        lib().speexhip_resampler_set_input_stride(self._h, in_stride)
        lib().speexhip_resampler_set_output_stride(self._h, out_stride)
        if x is None:
            ptr, n = None, int(null_frames)
        else:
            x = np.asarray(x, dtype=dt).reshape(-1)
            n = x.shape[0]
            buf = np.full(max((n - 1) * in_stride + 1, 1), fill, dt)
            buf[: (n - 1) * in_stride + 1: in_stride] = x
            ptr = buf.ctypes.data_as(C.POINTER(cdt))
        out = np.full(max((int(cap) - 1) * out_stride + 1, 1), fill, dt)
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        fn = lib().speexhip_resampler_process_int if kind == "int" else lib().speexhip_resampler_process_float
        rc = fn(self._h, c, ptr, C.byref(il), out.ctypes.data_as(C.POINTER(cdt)), C.byref(ol))
        return rc, il.value, ol.value, out

    def positions(self):
        res = []
        for c in range(self.channels):
            a, b, m = C.c_int32(), C.c_uint32(), C.c_uint32()
            lib().speexhip_resampler_get_channel_position(self._h, c, C.byref(a), C.byref(b), C.byref(m))
            res.append((a.value, b.value, m.value))
        return res

    def process(self, frames, out_capacity, null_frames=0):
        """frames=None: the reference's in == NULL case (null_frames frames of silence)."""
        if frames is None:
            ptr, n = None, int(null_frames)
        else:
            frames = np.ascontiguousarray(frames, dtype=np.int16)
            if frames.ndim == 1:
                frames = frames.reshape(-1, self.channels)
            ptr, n = frames.ctypes.data_as(C.POINTER(C.c_int16)), frames.shape[0]
        out = np.zeros((max(int(out_capacity), 1), self.channels), np.int16)
        il, ol = C.c_uint32(n), C.c_uint32(int(out_capacity))
        rc = lib().speexhip_resampler_process_interleaved_int(
            self._h, ptr, C.byref(il),
            out.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(ol))
        if rc:
            raise RuntimeError(strerror(rc))
        return out[: ol.value].copy(), il.value

    def process_into(self, x, out, float_io=False):
        """The C call itself on the caller's own buffers, no copy on either side: x (frames x channels) in, `out`
        (capacity x channels) written in place -- either may be a view of a PinnedBlock, which the library then uses
        where it lies (round 6).  Returns (consumed, produced)."""
        assert x.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"] and x.dtype == out.dtype
        il, ol = C.c_uint32(x.shape[0]), C.c_uint32(out.shape[0])
        if float_io:
            rc = lib().speexhip_resampler_process_interleaved_float(
                self._h, C.cast(x.ctypes.data, C.POINTER(C.c_float)), C.byref(il),
                C.cast(out.ctypes.data, C.POINTER(C.c_float)), C.byref(ol))
        else:
            rc = lib().speexhip_resampler_process_interleaved_int(
                self._h, C.cast(x.ctypes.data, C.POINTER(C.c_int16)), C.byref(il),
                C.cast(out.ctypes.data, C.POINTER(C.c_int16)), C.byref(ol))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    def process_float(self, frames, out_capacity, null_frames=0):
        """speexhip_resampler_process_interleaved_float with host buffers (float32 in / out)."""
        if frames is None:
            ptr, n = None, int(null_frames)
        else:
            frames = np.ascontiguousarray(frames, dtype=np.float32)
            if frames.ndim == 1:
                frames = frames.reshape(-1, self.channels)
            ptr, n = frames.ctypes.data_as(C.POINTER(C.c_float)), frames.shape[0]
        out = np.zeros((max(int(out_capacity), 1), self.channels), np.float32)
        il, ol = C.c_uint32(n), C.c_uint32(int(out_capacity))
        rc = lib().speexhip_resampler_process_interleaved_float(
            self._h, ptr, C.byref(il),
            out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ol))
        if rc:
            raise RuntimeError(strerror(rc))
        return out[: ol.value].copy(), il.value

    def planar_call(self, kind, planes, cap, null_frames=0, out_planes=None):
        """The host planar C call itself: planes = sequence of 1-D arrays (one per channel; None = silence of
        null_frames frames), out_planes = arrays to write (default: fresh ones of `cap` frames, sentinel-filled).
        Returns (rc, consumed, produced, out_planes)."""
        dt, fill = (np.int16, self.SENTINEL_I16) if kind == "int" else (np.float32, self.SENTINEL_F32)
        ins = None
        if planes is None:
            n = int(null_frames)
        else:
            planes = [np.asarray(q, dtype=dt) for q in planes]
            assert all(q.ndim == 1 and (q.size < 2 or q.strides[0] == q.itemsize) for q in planes)
            n = planes[0].shape[0]
            ins = (C.c_void_p * len(planes))(*[q.ctypes.data for q in planes])
        if out_planes is None:
            out_planes = [np.full(max(int(cap), 1), fill, dt) for _ in range(self.channels)]
        outs = (C.c_void_p * len(out_planes))(*[None if q is None else q.ctypes.data for q in out_planes])
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        fn = (lib().speexhip_resampler_process_planar_int if kind == "int"
              else lib().speexhip_resampler_process_planar_float)
        rc = fn(self._h, ins, C.byref(il), outs, C.byref(ol))
        return rc, il.value, ol.value, out_planes

    def process_planar(self, x, out_capacity, float_io=False, null_frames=0):
        """x: [C, F] array or a list of C 1-D arrays (None: null_frames frames of silence) -- one plane per channel,
        no transposition on the caller's side.  Returns ([C, produced] array, frames consumed)."""
        planes = None if x is None else [np.ascontiguousarray(q) for q in x]
        rc, used, made, outs = self.planar_call("float" if float_io else "int", planes, out_capacity, null_frames)
        if rc:
            raise RuntimeError(strerror(rc))
        return np.stack([q[:made] for q in outs]), used

    def process_planar_device(self, d_in_ptr, in_plane_stride, in_frames, d_out_ptr, out_plane_stride, out_capacity,
                              stream_ptr=0, float_io=False):
        """device planes: plane c at d_in_ptr + c * in_plane_stride elements; (consumed, produced)"""
        il, ol = C.c_uint32(in_frames), C.c_uint32(out_capacity)
        fn = (lib().speexhip_resampler_process_planar_float_device if float_io
              else lib().speexhip_resampler_process_planar_int_device)
        rc = fn(self._h, C.c_void_p(d_in_ptr), in_plane_stride, C.byref(il), C.c_void_p(d_out_ptr), out_plane_stride,
                C.byref(ol), C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    SENTINEL_BYTE = 0xA5

    def fmt_call(self, x, in_fmt, out_fmt, cap, null_frames=0):
        """The host formatted C call itself.  x: array of the format's storage type (FMT_DTYPE; packed S24 as uint8,
        3 bytes per sample) holding whole frames, or None = silence of null_frames frames.  Returns (rc, consumed,
        produced, out): `out` is the whole buffer of `cap` frames in the output format's storage type, flat, every
        byte pre-filled with SENTINEL_BYTE."""
        if x is None:
            ptr, n = None, int(null_frames)
        else:
            x = np.ascontiguousarray(x, dtype=fmt_dtype(in_fmt)).reshape(-1)
            n = x.nbytes // (fmt_bytes(in_fmt) * self.channels)
            assert n * fmt_bytes(in_fmt) * self.channels == x.nbytes, "whole frames only"
            ptr = C.c_void_p(x.ctypes.data)
        raw = np.full(max(int(cap), 1) * self.channels * fmt_bytes(out_fmt), self.SENTINEL_BYTE, np.uint8)
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        rc = lib().speexhip_resampler_process_interleaved_fmt(self._h, in_fmt, ptr, C.byref(il), out_fmt,
                                                              C.c_void_p(raw.ctypes.data), C.byref(ol))
        return rc, il.value, ol.value, raw.view(fmt_dtype(out_fmt))

    def process_fmt(self, x, in_fmt, out_fmt, capacity, null_frames=0):
        """Formatted call on host buffers: x in format in_fmt (FMT_*; S24 as a uint8 array of 3 * n bytes; None: silence),
        the result in out_fmt.  It is the float call on the converted input followed by the output conversion, both on the
        device.  Returns (flat array of produced * channels samples in the output format's storage type, consumed)."""
        rc, used, made, out = self.fmt_call(x, in_fmt, out_fmt, capacity, null_frames)
        if rc:
            raise RuntimeError(strerror(rc))
        per = self.channels * _per_sample(out_fmt)
        return out[: made * per].copy(), used

    def process_fmt_device(self, in_fmt, d_in_ptr, in_frames, out_fmt, d_out_ptr, out_capacity, stream_ptr=0):
        """device buffers of the named formats; (consumed, produced)"""
        il, ol = C.c_uint32(in_frames), C.c_uint32(out_capacity)
        rc = lib().speexhip_resampler_process_interleaved_fmt_device(
            self._h, in_fmt, C.c_void_p(d_in_ptr), C.byref(il), out_fmt, C.c_void_p(d_out_ptr), C.byref(ol),
            C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    def mix_call(self, x, in_fmt, out_fmt, in_mix, out_mix, cap, null_frames=0):
        """The host mixed C call itself.  in_mix: None or (channels x in_channels), out_mix: None or (out_channels x
        channels), applied to every frame before / after the float call.  x: array of in_fmt's storage type holding
        whole frames of in_channels samples, or None = silence of null_frames frames.  Returns (rc, consumed, produced,
        out): `out` is the whole buffer of `cap` frames of out_channels samples in the output format's storage type,
        flat, every byte pre-filled with SENTINEL_BYTE."""
        mi, n_in = _mix_matrix(in_mix, self.channels, True)
        mo, n_out = _mix_matrix(out_mix, self.channels, False)
        if x is None:
            ptr, n = None, int(null_frames)
        else:
            x = np.ascontiguousarray(x, dtype=fmt_dtype(in_fmt)).reshape(-1)
            n = x.nbytes // (fmt_bytes(in_fmt) * n_in)
            assert n * fmt_bytes(in_fmt) * n_in == x.nbytes, "whole frames only"
            ptr = C.c_void_p(x.ctypes.data)
        raw = np.full(max(int(cap), 1) * n_out * fmt_bytes(out_fmt), self.SENTINEL_BYTE, np.uint8)
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        rc = lib().speexhip_resampler_process_interleaved_mix(
            self._h, in_fmt, n_in, _mix_ptr(mi), ptr, C.byref(il), out_fmt, n_out, _mix_ptr(mo),
            C.c_void_p(raw.ctypes.data), C.byref(ol))
        return rc, il.value, ol.value, raw.view(fmt_dtype(out_fmt))

    def process_mix(self, x, in_fmt, out_fmt, capacity, in_mix=None, out_mix=None, null_frames=0):
        """Mixed call on host buffers: the formatted call with a channel matrix on either side -- in_mix (channels x
        in_channels) turns every input frame into a frame of the state before the FIR, out_mix (out_channels x channels)
        every frame it produced into an output frame; both on the device, folded into the conversions.  Returns (flat
        array of produced * out_channels samples in the output format's storage type, consumed)."""
        rc, used, made, out = self.mix_call(x, in_fmt, out_fmt, in_mix, out_mix, capacity, null_frames)
        if rc:
            raise RuntimeError(strerror(rc))
        n_out = self.channels if out_mix is None else len(out_mix)
        return out[: made * n_out * _per_sample(out_fmt)].copy(), used

    def process_mix_device(self, in_fmt, d_in_ptr, in_frames, out_fmt, d_out_ptr, out_capacity, in_mix=None, out_mix=None,
                           stream_ptr=0):
        """device buffers of the named formats and channel counts; (consumed, produced)"""
        mi, n_in = _mix_matrix(in_mix, self.channels, True)
        mo, n_out = _mix_matrix(out_mix, self.channels, False)
        il, ol = C.c_uint32(in_frames), C.c_uint32(out_capacity)
        rc = lib().speexhip_resampler_process_interleaved_mix_device(
            self._h, in_fmt, n_in, _mix_ptr(mi), C.c_void_p(d_in_ptr), C.byref(il), out_fmt, n_out, _mix_ptr(mo),
            C.c_void_p(d_out_ptr), C.byref(ol), C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    def sides_call(self, x, in_fmt, out_fmt, cap, in_layout=None, out_layout=None, in_mix=None, out_mix=None,
                   null_frames=0, out_plane_stride=None, separate_planes=False):
        """The host sides C call itself.  in_layout / out_layout: 'planar' | 'interleaved' (None = interleaved).  x: an
        interleaved input holds whole frames as in mix_call; a planar one is (in_channels, T) of in_fmt's storage type
        (packed S24: (in_channels, 3 * T) uint8) or a sequence of such 1-D planes; None = silence of null_frames frames.
        separate_planes: hand the planes over as separate allocations (SpeexHipSide::planes) instead of one block.
        Returns (rc, consumed, produced, out): `out` is the whole output buffer, every byte pre-filled with SENTINEL_BYTE --
        flat and `cap` frames long when interleaved, (out_channels, out_plane_stride) when planar (out_plane_stride
        defaults to cap; S24: three bytes per sample along the last axis)."""
        mi, n_in = _mix_matrix(in_mix, self.channels, True)
        mo, n_out = _mix_matrix(out_mix, self.channels, False)
        li, lo = _layout(in_layout), _layout(out_layout)
        bi, bo = fmt_bytes(in_fmt), fmt_bytes(out_fmt)
        keep = []
        a = make_side(in_fmt, n_in, li, mi)
        if x is None:
            n = int(null_frames)
        elif li == LAYOUT_PLANAR:
            planes = [np.ascontiguousarray(q, dtype=fmt_dtype(in_fmt)).reshape(-1) for q in x]
            assert len(planes) == n_in and all(q.nbytes == planes[0].nbytes for q in planes)
            n = planes[0].nbytes // bi
            if separate_planes:
                keep.append(planes)
                ptrs = (C.c_void_p * n_in)(*[q.ctypes.data for q in planes])
                a = make_side(in_fmt, n_in, li, mi, planes=ptrs)
            else:
                # (stacked as bytes: numpy would turn a big-endian storage type into the host's, values kept, bytes swapped)
                block = np.stack([q.view(np.uint8) for q in planes]) if n else np.zeros((n_in, 1), np.uint8)
                keep.append(block)
                a = make_side(in_fmt, n_in, li, mi, data=block.ctypes.data, plane_stride=n)
        else:
            xf = np.ascontiguousarray(x, dtype=fmt_dtype(in_fmt)).reshape(-1)
            n = xf.nbytes // (bi * n_in)
            assert n * bi * n_in == xf.nbytes, "whole frames only"
            keep.append(xf)
            a = make_side(in_fmt, n_in, li, mi, data=xf.ctypes.data)
        room = max(int(cap), 1)
        if lo == LAYOUT_PLANAR:
            ps = room if out_plane_stride is None else int(out_plane_stride)
            if separate_planes:
                outs = [np.full(ps * bo, self.SENTINEL_BYTE, np.uint8) for _ in range(n_out)]
                ptrs_o = (C.c_void_p * n_out)(*[q.ctypes.data for q in outs])
                b = make_side(out_fmt, n_out, lo, mo, planes=ptrs_o)
            else:
                raw = np.full((n_out, ps * bo), self.SENTINEL_BYTE, np.uint8)
                b = make_side(out_fmt, n_out, lo, mo, data=raw.ctypes.data, plane_stride=ps)
        else:
            raw = np.full(room * n_out * bo, self.SENTINEL_BYTE, np.uint8)
            b = make_side(out_fmt, n_out, lo, mo, data=raw.ctypes.data)
        il, ol = C.c_uint32(n), C.c_uint32(int(cap))
        rc = lib().speexhip_resampler_process_sides(self._h, C.byref(a), C.byref(il), C.byref(b), C.byref(ol))
        if lo == LAYOUT_PLANAR and separate_planes:
            out = np.stack(outs).view(fmt_dtype(out_fmt))
        else:
            out = raw.view(fmt_dtype(out_fmt))
        return rc, il.value, ol.value, out

    def process_sides(self, x, in_fmt, out_fmt, capacity, in_layout=None, out_layout=None, in_mix=None, out_mix=None,
                      null_frames=0):
        """Sides call on host buffers: the mixed call with a layout per side ('planar' | 'interleaved').  A planar x is
        (in_channels, T); a planar result is (out_channels, produced) (S24: three bytes per sample along the last axis),
        an interleaved one flat as in process_mix.  Returns (result, consumed)."""
        rc, used, made, out = self.sides_call(x, in_fmt, out_fmt, capacity, in_layout, out_layout, in_mix, out_mix,
                                              null_frames)
        if rc:
            raise RuntimeError(strerror(rc))
        per = _per_sample(out_fmt)
        if _layout(out_layout) == LAYOUT_PLANAR:
            return out[:, : made * per].copy(), used
        n_out = self.channels if out_mix is None else len(out_mix)
        return out[: made * n_out * per].copy(), used

    def process_sides_device(self, in_side, in_frames, out_side, out_capacity, stream_ptr=0):
        """device buffers described by two Side structures (make_side); (consumed, produced)"""
        il, ol = C.c_uint32(in_frames), C.c_uint32(out_capacity)
        rc = lib().speexhip_resampler_process_sides_device(self._h, C.byref(in_side), C.byref(il), C.byref(out_side),
                                                           C.byref(ol), C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    def set_dither(self, kind, seed=0, position=0):
        """Dither of the integer output formats of the formatted and mixed calls: kind = DITHER_NONE / _RECTANGULAR /
        _TRIANGULAR, position = index of the stream's next output frame.  Returns the C call's code (INVALID_ARG for an
        unknown kind, the state untouched)."""
        return lib().speexhip_resampler_set_dither(self._h, int(kind), int(seed), int(position))

    def get_dither(self):
        """(kind, seed, position)"""
        k, s, p_ = C.c_int(), C.c_uint64(), C.c_uint64()
        rc = lib().speexhip_resampler_get_dither(self._h, C.byref(k), C.byref(s), C.byref(p_))
        if rc:
            raise RuntimeError(strerror(rc))
        return k.value, s.value, p_.value

    def set_meter(self, on):
        """The output meter of the formatted, mixed and sides calls: clip counts and peak level of what they encode.  The
        totals are kept across the switch.  Returns the C call's code (INVALID_ARG for anything but 0 / 1 / a bool)."""
        return lib().speexhip_resampler_set_meter(self._h, int(on))

    def get_meter(self, reset=False):
        """{'on', 'samples', 'clipped_high', 'clipped_low', 'nan', 'peak'} since the last reset; peak in int16 units.
        Waits for this state's last call only."""
        m = Meter()
        rc = lib().speexhip_resampler_get_meter(self._h, C.byref(m), int(bool(reset)))
        if rc:
            raise RuntimeError(strerror(rc))
        return m.as_dict()

    def set_gain(self, gain, ramp_frames=0):
        """The output gain of the formatted, mixed and sides calls: `gain` from the next output frame on, reached over
        ramp_frames output frames from the gain that frame would have had (0: a step).  Returns the C call's code
        (INVALID_ARG for a gain that is not finite)."""
        return lib().speexhip_resampler_set_gain(self._h, float(gain), int(ramp_frames))

    def get_gain(self):
        """{'current', 'target', 'remaining'}: the next output frame's gain (numpy float32), the ramp's target, its
        frames still to come"""
        cur, tgt, rem = C.c_float(), C.c_float(), C.c_uint32()
        rc = lib().speexhip_resampler_get_gain(self._h, C.byref(cur), C.byref(tgt), C.byref(rem))
        if rc:
            raise RuntimeError(strerror(rc))
        return {"current": np.float32(cur.value), "target": np.float32(tgt.value), "remaining": rem.value}

    def peek(self, in_frames, out_capacity, float_entry=False):
        """(consumed, produced) of the next call, state untouched"""
        c, p_ = C.c_uint32(), C.c_uint32()
        rc = lib().speexhip_resampler_peek(self._h, in_frames, out_capacity, int(float_entry), C.byref(c), C.byref(p_))
        if rc:
            raise RuntimeError(strerror(rc))
        return c.value, p_.value

    def process_chunks(self, chunks, capacities, dtype=np.int16):
        """n consecutive calls as one launch (speexhip_resampler_process_chunks_int / _float).
        chunks: arrays of frames (or None with capacities[i] = (null_frames, capacity)).
        Returns (list of per-call outputs, list of frames consumed)."""
        n = len(chunks)
        keep, ptrs, lens, caps = [], (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
        for i, ch_ in enumerate(chunks):
            if ch_ is None:
                ptrs[i], lens[i], caps[i] = None, capacities[i][0], capacities[i][1]
            else:
                a = np.ascontiguousarray(ch_, dtype=dtype).reshape(-1, self.channels)
                keep.append(a)
                ptrs[i], lens[i], caps[i] = a.ctypes.data, a.shape[0], capacities[i]
        out = np.zeros((max(sum(caps), 1), self.channels), dtype)
        fn = (lib().speexhip_resampler_process_chunks_int if dtype == np.int16
              else lib().speexhip_resampler_process_chunks_float)
        rc = fn(self._h, n, ptrs, lens, C.c_void_p(out.ctypes.data), caps)
        if rc:
            raise RuntimeError(strerror(rc))
        outs, off = [], 0
        for i in range(n):
            outs.append(out[off: off + caps[i]].copy())
            off += caps[i]
        return outs, list(lens)

    def process_chunks_sides(self, in_side, in_ptrs, in_lens, out_side, capacities):
        """speexhip_resampler_process_chunks_sides itself: in_side describes every chunk's input (make_side; its data and
        planes are not read), in_ptrs the addresses of the chunks -- one per chunk, or in_side.channels per chunk (plane
        c of chunk i at i * channels + c) for a planar side of several channels; None = NULL, and in_ptrs itself may be
        None (every chunk silence).  out_side (make_side, host buffers the caller keeps alive) receives the results back
        to back.  Returns (rc, consumed, produced), one entry per chunk."""
        n = len(in_lens)
        ptrs = None
        if in_ptrs is not None:
            ptrs = (C.c_void_p * max(len(in_ptrs), 1))()
            for k, a in enumerate(in_ptrs):
                ptrs[k] = a
        il, ol = (C.c_uint32 * max(n, 1))(*in_lens), (C.c_uint32 * max(n, 1))(*capacities)
        rc = lib().speexhip_resampler_process_chunks_sides(self._h, n, C.byref(in_side), ptrs, il, C.byref(out_side), ol)
        return rc, list(il)[:n], list(ol)[:n]

    def process_chunks_fmt(self, chunks, in_fmt, out_fmt, capacities):
        """n consecutive formatted calls as one transfer each way (speexhip_resampler_process_chunks_fmt).  chunks: whole
        interleaved frames of in_fmt's storage type each (or None with capacities[i] = (null_frames, capacity)).
        Returns (list of per-call outputs, flat, of out_fmt's storage type; list of frames consumed)."""
        n = len(chunks)
        bi, bo = fmt_bytes(in_fmt) * self.channels, fmt_bytes(out_fmt) * self.channels
        keep, ptrs, lens, caps = [], (C.c_void_p * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
        for i, ch_ in enumerate(chunks):
            if ch_ is None:
                ptrs[i], lens[i], caps[i] = None, capacities[i][0], capacities[i][1]
            else:
                a = np.ascontiguousarray(ch_, dtype=fmt_dtype(in_fmt)).reshape(-1)
                if a.nbytes % bi:
                    raise ValueError("chunk %d: whole frames only" % i)
                keep.append(a)
                ptrs[i], lens[i], caps[i] = a.ctypes.data, a.nbytes // bi, capacities[i]
        out = np.zeros(max(sum(caps[:n]), 1) * bo, np.uint8)
        rc = lib().speexhip_resampler_process_chunks_fmt(self._h, n, int(in_fmt), ptrs, lens, int(out_fmt),
                                                         C.c_void_p(out.ctypes.data), caps)
        if rc not in (0, ERR_ALLOC_FAILED):
            raise RuntimeError(strerror(rc))
        outs, off = [], 0
        for i in range(n):
            outs.append(out[off * bo: (off + caps[i]) * bo].view(fmt_dtype(out_fmt)).copy())
            off += caps[i]
        return outs, list(lens)[:n]

    def process_device(self, d_in_ptr, in_frames, d_out_ptr, out_capacity, stream_ptr=0, float_io=False):
        il, ol = C.c_uint32(in_frames), C.c_uint32(out_capacity)
        fn = (lib().speexhip_resampler_process_interleaved_float_device if float_io
              else lib().speexhip_resampler_process_interleaved_int_device)
        rc = fn(
            self._h, C.c_void_p(d_in_ptr), C.byref(il), C.c_void_p(d_out_ptr), C.byref(ol),
            C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return il.value, ol.value

    def close(self):
        if getattr(self, "_h", None):
            lib().speexhip_resampler_destroy(self._h)
            self._h = None

    __del__ = close


class Batch:
    """n_streams independent streams with one shared filter; device pointers, one launch/call."""

    def __init__(self, n_streams, channels, in_rate, out_rate, quality=7, mode=None):
        err = C.c_int(0)
        self._h = lib().speexhip_batch_init(n_streams, channels, in_rate, out_rate, quality,
                                            C.byref(err))
        if not self._h:
            raise (RuntimeError if err.value == ERR_DEVICE else ValueError)(strerror(err.value))
        self.n_streams, self.channels = n_streams, channels
        if mode is not None:
            rc = lib().speexhip_batch_set_mode(self._h, mode)
            if rc:
                raise ValueError(strerror(rc))

    def info(self, stream=0):
        i = Info()
        lib().speexhip_batch_get_info(self._h, stream, C.byref(i))
        return i.as_dict()

    def set_rate_frac(self, num, den, in_rate, out_rate):
        return lib().speexhip_batch_set_rate_frac(self._h, num, den, in_rate, out_rate)

    def set_quality(self, quality):
        return lib().speexhip_batch_set_quality(self._h, quality)

    def skip_zeros(self):
        return lib().speexhip_batch_skip_zeros(self._h)

    def reset_mem(self):
        return lib().speexhip_batch_reset_mem(self._h)

    def set_dither(self, kind, seed=0, position=0):
        """Dither of every stream's integer outputs in the formatted and mixed calls (process_tensor through them): stream
        s draws from seed + s * 0x9E3779B97F4A7C15 (mod 2^64); position = every stream's next output frame.  Returns the C
        call's code."""
        return lib().speexhip_batch_set_dither(self._h, int(kind), int(seed), int(position))

    def get_dither(self, stream=0):
        """(kind, the stream's own seed, the stream's position)"""
        k, s, p_ = C.c_int(), C.c_uint64(), C.c_uint64()
        rc = lib().speexhip_batch_get_dither(self._h, stream, C.byref(k), C.byref(s), C.byref(p_))
        if rc:
            raise RuntimeError(strerror(rc))
        return k.value, s.value, p_.value

    def set_meter(self, on):
        """The output meter of every stream in the formatted, mixed and sides calls (process_tensor through them); the
        totals are kept per stream.  Returns the C call's code."""
        return lib().speexhip_batch_set_meter(self._h, int(on))

    def get_meter(self, stream, reset=False):
        """The stream's {'on', 'samples', 'clipped_high', 'clipped_low', 'nan', 'peak'}; reset clears that stream only.
        Waits for this batch's last call only."""
        m = Meter()
        rc = lib().speexhip_batch_get_meter(self._h, int(stream), C.byref(m), int(bool(reset)))
        if rc:
            raise RuntimeError(strerror(rc))
        return m.as_dict()

    def set_gain(self, gain, ramp_frames=0, stream=None):
        """The output gain of one stream (None: of every stream) in the formatted, mixed and sides calls; see
        Resampler.set_gain.  Returns the C call's code."""
        return lib().speexhip_batch_set_gain(self._h, 0xFFFFFFFF if stream is None else int(stream), float(gain), int(ramp_frames))

    def get_gain(self, stream):
        """The stream's {'current', 'target', 'remaining'}"""
        cur, tgt, rem = C.c_float(), C.c_float(), C.c_uint32()
        rc = lib().speexhip_batch_get_gain(self._h, int(stream), C.byref(cur), C.byref(tgt), C.byref(rem))
        if rc:
            raise RuntimeError(strerror(rc))
        return {"current": np.float32(cur.value), "target": np.float32(tgt.value), "remaining": rem.value}

    def set_buses(self, weights):
        """The bus matrix (n_buses, n_streams) of process_bus_device: bus j is the sum over the streams of weights[j][s]
        times the stream's gained output (mix-minus: ones - identity).  None: off.  Zeroes the bus meters and the bus
        position.  Returns the C call's code."""
        if weights is None:
            return lib().speexhip_batch_set_buses(self._h, 0, None)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim != 2 or w.shape[1] != self.n_streams:
            raise ValueError("weights must be (n_buses, %d)" % self.n_streams)
        return lib().speexhip_batch_set_buses(self._h, w.shape[0], C.c_void_p(w.ctypes.data))

    def get_buses(self):
        """the bus matrix (n_buses, n_streams) float32, or None when the buses are off"""
        n = C.c_uint32()
        rc = lib().speexhip_batch_get_buses(self._h, C.byref(n), None)
        if rc:
            raise RuntimeError(strerror(rc))
        if n.value == 0:
            return None
        w = np.zeros((n.value, self.n_streams), np.float32)
        rc = lib().speexhip_batch_get_buses(self._h, C.byref(n), C.c_void_p(w.ctypes.data))
        if rc:
            raise RuntimeError(strerror(rc))
        return w

    def get_bus_meter(self, bus, reset=False):
        """The bus's {'on', 'samples', 'clipped_high', 'clipped_low', 'nan', 'peak'}; reset clears that bus only.  Waits
        for this batch's last call only."""
        m = Meter()
        rc = lib().speexhip_batch_get_bus_meter(self._h, int(bus), C.byref(m), int(bool(reset)))
        if rc:
            raise RuntimeError(strerror(rc))
        return m.as_dict()

    def bus_position(self):
        """the buses' one dither position: the index of every bus's next output frame"""
        pos = C.c_uint64()
        rc = lib().speexhip_batch_get_bus_position(self._h, C.byref(pos))
        if rc:
            raise RuntimeError(strerror(rc))
        return pos.value

    def lines(self, stream):
        """(taps-1+pending, channels) float32 of one stream: history then pending frames"""
        i = self.info(stream)
        n = i["filt_len"] - 1 + i["magic_samples"]
        buf = np.zeros((max(n, 1), self.channels), np.float32)
        rc = lib().speexhip_batch_get_history(self._h, stream, buf.ctypes.data_as(C.POINTER(C.c_float)))
        if rc:
            raise RuntimeError(strerror(rc))
        return buf[:n]

    def process_device(self, d_in_ptr, in_stride, in_frames, d_out_ptr, out_stride, out_capacity,
                       stream_ptr=0, float_io=False):
        """in_frames / out_capacity: int (same for all streams) or sequences of n_streams.
        float_io: the buffers hold float32 samples (strides in samples either way)."""
        n = self.n_streams
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        fn = (lib().speexhip_batch_process_interleaved_float_device if float_io
              else lib().speexhip_batch_process_interleaved_int_device)
        rc = fn(
            self._h, C.c_void_p(d_in_ptr), in_stride, il, C.c_void_p(d_out_ptr), out_stride, ol,
            C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return list(il), list(ol)

    def process_planar_device(self, d_in_ptr, in_stream_stride, in_plane_stride, in_frames, d_out_ptr,
                              out_stream_stride, out_plane_stride, out_capacity, stream_ptr=0, float_io=False):
        """The same call on channel planes: plane c of stream s at d_in_ptr + s * in_stream_stride +
        c * in_plane_stride elements (a (B, C, T) tensor's strides)."""
        n = self.n_streams
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        fn = (lib().speexhip_batch_process_planar_float_device if float_io
              else lib().speexhip_batch_process_planar_int_device)
        rc = fn(self._h, C.c_void_p(d_in_ptr), in_stream_stride, in_plane_stride, il, C.c_void_p(d_out_ptr),
                out_stream_stride, out_plane_stride, ol, C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return list(il), list(ol)

    def process_fmt_device(self, in_fmt, d_in_ptr, in_stride, in_frames, out_fmt, d_out_ptr, out_stride, out_capacity,
                           stream_ptr=0):
        """Formatted call of every stream: interleaved device buffers of formats in_fmt / out_fmt (FMT_*), strides in
        samples of the respective format (a packed S24 sample is 3 bytes)."""
        n = self.n_streams
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        rc = lib().speexhip_batch_process_interleaved_fmt_device(
            self._h, in_fmt, C.c_void_p(d_in_ptr), in_stride, il, out_fmt, C.c_void_p(d_out_ptr), out_stride, ol,
            C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return list(il), list(ol)

    def process_mix_device(self, in_fmt, d_in_ptr, in_stride, in_frames, out_fmt, d_out_ptr, out_stride, out_capacity,
                           in_mix=None, out_mix=None, stream_ptr=0):
        """Mixed call of every stream: the formatted call with in_mix (channels x in_channels) before the FIR and / or
        out_mix (out_channels x channels) after it; one pair of matrices for all streams.  Strides in samples of the
        respective format, a frame of a side holding that side's channel count."""
        n = self.n_streams
        mi, n_in = _mix_matrix(in_mix, self.channels, True)
        mo, n_out = _mix_matrix(out_mix, self.channels, False)
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        rc = lib().speexhip_batch_process_interleaved_mix_device(
            self._h, in_fmt, n_in, _mix_ptr(mi), C.c_void_p(d_in_ptr), in_stride, il, out_fmt, n_out, _mix_ptr(mo),
            C.c_void_p(d_out_ptr), out_stride, ol, C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return list(il), list(ol)

    def process_sides_device(self, in_side, in_frames, out_side, out_capacity, stream_ptr=0):
        """Sides call of every stream: the mixed call with a layout per side.  in_side / out_side: Side structures
        (make_side) naming format, channel count, layout, matrix, stream 0's address and the strides in samples of the
        side's format."""
        n = self.n_streams
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        rc = lib().speexhip_batch_process_sides_device(self._h, C.byref(in_side), il, C.byref(out_side), ol,
                                                       C.c_void_p(stream_ptr))
        if rc:
            raise RuntimeError(strerror(rc))
        return list(il), list(ol)

    def bus_call(self, in_side, in_frames, out_side, out_capacity, stream_ptr=0):
        """process_bus_device without the exception: (code, consumed per stream, produced per stream, bus_frames)"""
        n = self.n_streams
        il = (C.c_uint32 * n)(*([in_frames] * n if np.isscalar(in_frames) else in_frames))
        ol = (C.c_uint32 * n)(*([out_capacity] * n if np.isscalar(out_capacity) else out_capacity))
        made = C.c_uint32(0)
        rc = lib().speexhip_batch_process_bus_device(self._h, C.byref(in_side), il, C.byref(out_side), ol, C.byref(made),
                                                     C.c_void_p(stream_ptr))
        return rc, list(il), list(ol), made.value

    def process_bus_device(self, in_side, in_frames, out_side, out_capacity, stream_ptr=0):
        """Bus call of the batch: in_side / in_frames as in process_sides_device; out_side describes the BUSES (bus j
        stream_stride samples behind bus j - 1, the state's channel count, any format and layout, no matrix), each with
        room for max(out_capacity) frames.  Returns (consumed per stream, produced per stream, bus_frames)."""
        rc, used, made, bus_frames = self.bus_call(in_side, in_frames, out_side, out_capacity, stream_ptr)
        if rc:
            raise RuntimeError(strerror(rc))
        return used, made, bus_frames

    def process_bus_tensor(self, x, weights=None, out_dtype=None, normalized=False, in_layout=None, out_layout=None,
                           out_capacity=None, in_frames=None, in_format=None, out_format=None):
        """The buses of a CUDA tensor of streams: x is (B, T, C) -- (B, C, T) with in_layout='planar' -- of uint8, int16,
        int32, float16, bfloat16 or float32 (normalized: +-1.0 full scale), as in process_tensor's formatted form.
        weights: set_buses(weights) first (None: the matrix the batch already has).  Returns (the buses, (n_buses, T', C)
        or with out_layout='planar' (n_buses, C, T'), of out_dtype (default: x's); bus_frames = T'; frames produced per
        stream).  Runs on torch's current stream."""
        import torch
        if weights is not None:
            rc = self.set_buses(weights)
            if rc:
                raise ValueError(strerror(rc))
        w = self.get_buses()
        if w is None:
            raise ValueError("no buses set")
        fmt_of = {torch.uint8: FMT_U8, torch.int16: FMT_S16, torch.int32: FMT_S32,
                  torch.float32: FMT_F32N if normalized else FMT_F32, torch.float16: FMT_F16N, torch.bfloat16: FMT_BF16N}
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if not x.is_cuda or x.dim() != 3 or x.dtype not in fmt_of or out_dtype not in fmt_of:
            raise ValueError("process_bus_tensor wants a CUDA tensor of rank 3 of uint8, int16, int32, float16, bfloat16 or float32")
        in_fmt = fmt_of[x.dtype] if in_format is None else in_format
        out_fmt = fmt_of[out_dtype] if out_format is None else out_format
        if fmt_bytes(in_fmt) != x.element_size() or fmt_bytes(out_fmt) != torch.empty(0, dtype=out_dtype).element_size():
            raise ValueError("a named format must have the size of the tensor's elements")
        planar_in, planar_out = _layout(in_layout) == LAYOUT_PLANAR, _layout(out_layout) == LAYOUT_PLANAR
        if planar_in:
            B, Cn, T = x.shape
            if T > 1 and x.stride(-1) != 1:
                raise ValueError("the last dimension of a planar tensor must be dense (stride 1)")
        else:
            B, T, Cn = x.shape
            if not x[0].is_contiguous():
                raise ValueError("the frames of a stream must be dense (T, C)")
        if B != self.n_streams or Cn != self.channels:
            raise ValueError("tensor of %d streams x %d channels for a batch of %d x %d" % (B, Cn, self.n_streams, self.channels))
        i = self.info()
        if out_capacity is None:
            out_capacity = (T * i["den_rate"] + i["num_rate"] - 1) // i["num_rate"] + 1
        cap = max(int(np.max(out_capacity)), 1)
        nb = w.shape[0]
        if planar_out:
            pitch = (cap + 127) & ~127
            out = torch.empty((nb, Cn, pitch), dtype=out_dtype, device=x.device)
            b = make_side(out_fmt, Cn, LAYOUT_PLANAR, None, out.data_ptr(), out.stride(1), out.stride(0))
        else:
            out = torch.empty((nb, cap, Cn), dtype=out_dtype, device=x.device)
            b = make_side(out_fmt, Cn, LAYOUT_INTERLEAVED, None, out.data_ptr(), 0, out.stride(0))
        a = make_side(in_fmt, Cn, _layout(in_layout), None, x.data_ptr(), x.stride(1) if planar_in else 0,
                      x.stride(0) if B > 1 else 0)
        _, made, bus_frames = self.process_bus_device(a, T if in_frames is None else in_frames, b, out_capacity,
                                                      torch.cuda.current_stream(x.device).cuda_stream)
        out = out[:, :, :bus_frames] if planar_out else out[:, :bus_frames]
        return out, bus_frames, made

    def _process_tensor_fmt(self, x, out_capacity, in_frames, out_dtype, normalized, in_mix=None, out_mix=None,
                            in_format=None, out_format=None, in_layout=None, out_layout=None):
        """process_tensor beyond int16 -> int16 and float32 -> float32: interleaved frames (..., T, C) through the
        formatted call (the mixed call when a matrix is given: x then holds in_channels per frame and the result
        out_channels).  uint8 = U8, int16 = S16, int32 = S32, float32 = F32 (normalized: +-1.0 full scale); in_format /
        out_format (FMT_*) name a side's format instead -- a uint8 tensor as FMT_ULAW or FMT_ALAW, an int16 / int32
        tensor holding the raw bytes as FMT_S16BE / FMT_S32BE.  float16 = F16N and bfloat16 = BF16N, both in +-1.0
        whatever `normalized` says: the flag speaks of float32 only."""
        import torch
        fmt_of = {torch.uint8: FMT_U8, torch.int16: FMT_S16, torch.int32: FMT_S32,
                  torch.float32: FMT_F32N if normalized else FMT_F32, torch.float16: FMT_F16N, torch.bfloat16: FMT_BF16N}

        def torch_of(fmt):  # the tensor type that holds a format's samples, one element each
            if fmt == FMT_BF16N:
                return torch.bfloat16
            return {1: {"u": torch.uint8}, 2: {"i": torch.int16, "f": torch.float16},
                    4: {"i": torch.int32, "f": torch.float32}}[fmt_bytes(fmt)][np.dtype(fmt_dtype(fmt)).kind]

        if FMT_S24 in (in_format, out_format) or FMT_S24BE in (in_format, out_format):
            raise ValueError("process_tensor does not take packed S24: a sample is not a whole element")
        if in_format is not None and x.dtype != torch_of(in_format):
            raise ValueError("in_format %d wants a %s tensor" % (in_format, torch_of(in_format)))
        if out_format is not None:
            if out_dtype is not None and out_dtype != torch_of(out_format):
                raise ValueError("out_format %d gives a %s tensor" % (out_format, torch_of(out_format)))
            out_dtype = torch_of(out_format)
        elif out_dtype is None:
            out_dtype = x.dtype
        if x.dtype not in fmt_of or out_dtype not in fmt_of:
            raise ValueError("process_tensor converts between uint8, int16, int32, float16, bfloat16 and float32 tensors")
        in_fmt = fmt_of[x.dtype] if in_format is None else in_format
        out_fmt = fmt_of[out_dtype] if out_format is None else out_format
        xb = x if x.dim() == 3 else x.unsqueeze(0)
        sides = in_layout is not None or out_layout is not None
        planar_in = _layout(in_layout) == LAYOUT_PLANAR
        if planar_in:
            B, Cn, T = xb.shape
        else:
            B, T, Cn = xb.shape
        mi, n_in = _mix_matrix(in_mix, self.channels, True)
        mo, n_out = _mix_matrix(out_mix, self.channels, False)
        if B != self.n_streams or Cn != n_in:
            raise ValueError("tensor of %d streams x %d channels for a batch of %d x %d" % (B, Cn, self.n_streams, n_in))
        if planar_in:
            if T > 1 and xb.stride(-1) != 1:
                raise ValueError("the last dimension of a planar tensor must be dense (stride 1)")
        elif not xb[0].is_contiguous():
            raise ValueError("the frames of a stream must be dense (T, C)")
        i = self.info()
        if out_capacity is None:
            out_capacity = (T * i["den_rate"] + i["num_rate"] - 1) // i["num_rate"] + 1
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if sides:
            if _layout(out_layout) == LAYOUT_PLANAR:
                # (rows of whole 128-byte lines: aligned planes take the kernels' 16-bytes-per-lane path; the result is a
                #  view of the padded buffer)
                pitch = (max(int(out_capacity), 1) + 127) & ~127
                out = torch.empty((B, n_out, pitch), dtype=out_dtype, device=x.device)
                b = make_side(out_fmt, n_out, LAYOUT_PLANAR, mo, out.data_ptr(), out.stride(1), out.stride(0))
            else:
                out = torch.empty((B, max(int(out_capacity), 1), n_out), dtype=out_dtype, device=x.device)
                b = make_side(out_fmt, n_out, LAYOUT_INTERLEAVED, mo, out.data_ptr(), 0, out.stride(0))
            # (a dimension of size 1 may carry any stride: planes and streams are then never stepped over)
            a = make_side(in_fmt, n_in, _layout(in_layout), mi, xb.data_ptr(), xb.stride(1) if planar_in else 0,
                          xb.stride(0) if B > 1 else 0)
            _, made = self.process_sides_device(a, T if in_frames is None else in_frames, b, int(out_capacity), stream)
            out = out[:, :, : max(made)] if _layout(out_layout) == LAYOUT_PLANAR else out[:, : max(made)]
            return (out if x.dim() == 3 else out[0]), made
        out = torch.empty((B, max(int(out_capacity), 1), n_out), dtype=out_dtype, device=x.device)
        if in_mix is None and out_mix is None:
            _, made = self.process_fmt_device(
                in_fmt, xb.data_ptr(), xb.stride(0) if B > 1 else 0, T if in_frames is None else in_frames,
                out_fmt, out.data_ptr(), out.stride(0), int(out_capacity), stream)
        else:
            _, made = self.process_mix_device(
                in_fmt, xb.data_ptr(), xb.stride(0) if B > 1 else 0, T if in_frames is None else in_frames,
                out_fmt, out.data_ptr(), out.stride(0), int(out_capacity), in_mix, out_mix, stream)
        out = out[:, : max(made)]
        return (out if x.dim() == 3 else out[0]), made

    def process_tensor(self, x, out_capacity=None, in_frames=None, out_dtype=None, normalized=False, in_mix=None,
                       out_mix=None, in_format=None, out_format=None, in_layout=None, out_layout=None):
        """x: a CUDA tensor (B, C, T) or (C, T), int16 or float32, whose last dimension is dense (any other strides).
        Runs on torch's current stream.  in_frames: frames per stream (default T for all); out_capacity: frames the
        result may hold per stream (default: what T frames can produce).  Returns (tensor of the same rank with
        T_out = max(produced), list of frames produced per stream).

        Other sample types -- a uint8 (offset binary), int32, float16 or bfloat16 tensor (the half types in +-1.0,
        whatever `normalized` says), out_dtype= another type than x's, or
        normalized=True (float32 in +-1.0 instead of int16 units) -- take the formatted call: without a named layout
        (below) x is then interleaved frames (B, T, C) or (T, C), dense, and so is the result; with in_layout='planar' /
        out_layout='planar' the same conversions work on (B, C, T) directly.

        in_mix (channels x in_channels) / out_mix (out_channels x channels): the mixed call, also on interleaved
        frames -- x is (B, T, in_channels) and the result (B, T', out_channels), of any of the sample types above.

        in_format / out_format (FMT_*): name a side's sample format instead of inferring it from the dtype, also on
        interleaved frames -- a uint8 tensor with in_format=FMT_ULAW is G.711 mu-law, out_format=FMT_ALAW gives a uint8
        tensor of A-law bytes; an int16 tensor with in_format=FMT_S16BE holds big-endian samples as they came off the
        wire (RTP L16), likewise int32 with FMT_S32BE.  A side that is not named goes by its dtype as above (the result's being x's unless
        out_dtype says otherwise).

        in_layout / out_layout ('planar' | 'interleaved'): the sides call, which takes either layout on either side with
        every keyword above -- no transpose on the caller's part.  When either is given (the other then defaults to
        'interleaved'), x is (B, C, T) for a planar input -- any view whose last dimension is dense -- and (B, T, C) for
        an interleaved one, and the result is (B, C', T') or (B, T', C') by out_layout.  (B, C, T) float32 in +-1.0 both
        ways: process_tensor(x, normalized=True, in_layout='planar', out_layout='planar'); a decoder's interleaved
        int16 to a model's planes: process_tensor(x, out_dtype=torch.float32, normalized=True, in_layout='interleaved',
        out_layout='planar'), or out_dtype=torch.bfloat16 for a model that runs in half precision.  With both None the function does what the paragraphs above say."""
        import torch
        if in_layout is not None or out_layout is not None:
            if not x.is_cuda or x.dim() not in (2, 3):
                raise ValueError("process_tensor wants a CUDA tensor of rank 2 or 3 for a named layout")
            return self._process_tensor_fmt(x, out_capacity, in_frames, out_dtype, normalized, in_mix, out_mix, in_format,
                                            out_format, in_layout, out_layout)
        if in_format is not None or out_format is not None:
            if not x.is_cuda or x.dim() not in (2, 3):
                raise ValueError("process_tensor wants a CUDA tensor (B, T, C) or (T, C) for a named format")
            return self._process_tensor_fmt(x, out_capacity, in_frames, out_dtype, normalized, in_mix, out_mix, in_format,
                                            out_format)
        if in_mix is not None or out_mix is not None:
            if not x.is_cuda or x.dim() not in (2, 3):
                raise ValueError("process_tensor wants a CUDA tensor (B, T, C) or (T, C) for a mixed call")
            return self._process_tensor_fmt(x, out_capacity, in_frames, out_dtype, normalized, in_mix, out_mix)
        if x.is_cuda and x.dim() in (2, 3) and (
                x.dtype in (torch.uint8, torch.int32, torch.float16, torch.bfloat16) or normalized or (out_dtype is not None and out_dtype != x.dtype)):
            return self._process_tensor_fmt(x, out_capacity, in_frames, out_dtype, normalized)
        if not x.is_cuda or x.dtype not in (torch.int16, torch.float32) or x.dim() not in (2, 3):
            raise ValueError("process_tensor wants a CUDA tensor (B, C, T) or (C, T) of int16 or float32")
        xb = x if x.dim() == 3 else x.unsqueeze(0)
        B, Cn, T = xb.shape
        if B != self.n_streams or Cn != self.channels:
            raise ValueError("tensor of %d streams x %d channels for a batch of %d x %d" % (B, Cn, self.n_streams, self.channels))
        if T > 1 and xb.stride(-1) != 1:
            raise ValueError("the last dimension of the tensor must be dense (stride 1)")
        float_io = x.dtype == torch.float32
        i = self.info()
        if out_capacity is None:
            out_capacity = (T * i["den_rate"] + i["num_rate"] - 1) // i["num_rate"] + 1
        # (rows of whole 128-byte lines: planes whose base and stride are multiples of 16 bytes take the kernels' 16-bytes-
        #  per-lane path; the result is a view of the padded buffer)
        pitch = (max(int(out_capacity), 1) + 63) & ~63
        out = torch.empty((B, Cn, pitch), dtype=x.dtype, device=x.device)
        # (a dimension of size 1 may carry any stride: planes and streams are then never stepped over)
        _, made = self.process_planar_device(
            xb.data_ptr(), xb.stride(0) if B > 1 else 0, xb.stride(1), T if in_frames is None else in_frames,
            out.data_ptr(), out.stride(0), out.stride(1), int(out_capacity), torch.cuda.current_stream(x.device).cuda_stream,
            float_io)
        out = out[:, :, : max(made)]
        return (out if x.dim() == 3 else out[0]), made

    def close(self):
        if getattr(self, "_h", None):
            lib().speexhip_batch_destroy(self._h)
            self._h = None

    __del__ = close


class Mixer:
    """speexhip_mixer_*: mix buses over many separate Resampler states in one host call per tick.  A mixer has n_legs
    slots, n_buses buses and one channel count; bus j is the weighted sum, in ascending slot order, of the slots' output
    of the call (each behind its own state's gain), encoded, dithered and metered like a stream."""

    def __init__(self, n_legs, n_buses, channels, device=None):
        err = C.c_int(0)
        if device is None:
            self._h = lib().speexhip_mixer_init(n_legs, n_buses, channels, C.byref(err))
        else:
            self._h = lib().speexhip_mixer_init_on(int(device), n_legs, n_buses, channels, C.byref(err))
        if not self._h:
            raise (RuntimeError if err.value == ERR_DEVICE else ValueError)(strerror(err.value))
        self.n_legs, self.n_buses, self.channels = n_legs, n_buses, channels

    def close(self):
        if getattr(self, "_h", None):
            lib().speexhip_mixer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, weights):
        """W (n_buses, n_legs): bus j = sum over the slots of weights[j][i] times slot i's gained output (mix-minus: ones -
        identity).  None: off.  Zeroes the bus meters and the bus position.  Returns the C call's code."""
        if weights is None:
            return lib().speexhip_mixer_set_weights(self._h, None)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.shape != (self.n_buses, self.n_legs):
            raise ValueError("weights must be (%d, %d)" % (self.n_buses, self.n_legs))
        return lib().speexhip_mixer_set_weights(self._h, C.c_void_p(w.ctypes.data))

    def get_weights(self):
        """W (n_buses, n_legs) float32, or None while the mixer is off"""
        w = np.zeros((self.n_buses, self.n_legs), np.float32)
        rc = lib().speexhip_mixer_get_weights(self._h, C.c_void_p(w.ctypes.data))
        if rc == ERR_BAD_STATE:
            return None
        if rc:
            raise RuntimeError(strerror(rc))
        return w

    def set_dither(self, kind, seed=0, position=0):
        """Dither of the buses' integer outputs: bus j draws from seed + (n_legs + j) * 0x9E3779B97F4A7C15 (mod 2^64);
        position = the buses' one position.  Returns the C call's code."""
        return lib().speexhip_mixer_set_dither(self._h, int(kind), int(seed), int(position))

    def get_dither(self):
        """(kind, the seed as given, the bus position)"""
        k, s, p_ = C.c_int(), C.c_uint64(), C.c_uint64()
        rc = lib().speexhip_mixer_get_dither(self._h, C.byref(k), C.byref(s), C.byref(p_))
        if rc:
            raise RuntimeError(strerror(rc))
        return k.value, s.value, p_.value

    def set_meter(self, on):
        return lib().speexhip_mixer_set_meter(self._h, int(on))

    def get_bus_meter(self, bus, reset=False):
        """The bus's {'on', 'samples', 'clipped_high', 'clipped_low', 'nan', 'peak'}; reset clears that bus only."""
        m = Meter()
        rc = lib().speexhip_mixer_get_bus_meter(self._h, int(bus), C.byref(m), int(bool(reset)))
        if rc:
            raise RuntimeError(strerror(rc))
        return m.as_dict()

    def bus_position(self):
        return self.get_dither()[2]

    def set_levels(self, on):
        """Per-leg levels of every tick ("Mixer levels"): off by default; a change of the switch clears the snapshot.
        Returns the C call's code."""
        return lib().speexhip_mixer_set_levels(self._h, int(on))

    def get_levels(self, first=0, count=None):
        """The last process call's records of the slots [first, first + count) as a numpy structured array with the
        fields samples, energy, nan, peak (LEVEL_DTYPE): the leg's float value BEFORE its gain.  ValueError for a range
        beyond n_legs, RuntimeError while the levels are off."""
        count = self.n_legs - first if count is None else count
        if first < 0 or count < 0:
            raise ValueError("a range of slots")
        rec = np.zeros(max(count, 1), LEVEL_DTYPE)
        rc = lib().speexhip_mixer_get_levels(self._h, int(first), int(count), C.c_void_p(rec.ctypes.data), LEVEL_DTYPE.itemsize)
        if rc == ERR_INVALID_ARG:
            raise ValueError(strerror(rc))
        if rc:
            raise RuntimeError(strerror(rc))
        return rec[:count]

    def process_sides(self, legs, in_sides, in_lens, out_side, capacities):
        """speexhip_mixer_process itself: legs[i] a Resampler or None, in_sides[i] its Side (make_side; None for an empty
        slot), out_side the buses' Side over a host buffer the caller keeps alive.  Returns (rc, consumed, produced,
        bus_frames, codes); bus_frames is None when the call did not set it."""
        n = self.n_legs
        hs = (C.c_void_p * n)()
        a = (Side * n)()
        for i in range(n):
            hs[i] = None if legs[i] is None else legs[i]._h
            if in_sides[i] is not None:
                C.memmove(C.byref(a[i]), C.byref(in_sides[i]), C.sizeof(Side))
        il, ol, codes = (C.c_uint32 * n)(*in_lens), (C.c_uint32 * n)(*capacities), (C.c_int * n)()
        frames = C.c_uint32(0xFFFFFFFF)
        rc = lib().speexhip_mixer_process(self._h, hs, a, il, ol, C.byref(out_side), C.byref(frames), codes)
        return rc, list(il), list(ol), (None if frames.value == 0xFFFFFFFF else frames.value), list(codes)

    def process(self, legs, chunks, in_formats, out_format, capacity, out_layout="interleaved"):
        """One tick.  legs[i]: a Resampler or None (an empty slot); chunks[i]: a bytes-like of whole interleaved frames of
        in_formats[i] (one FMT_* for all, or one per slot), or None -- a silent leg, with capacity[i] = (silent_frames,
        capacity).  capacity: output frames each leg may produce, one for all or one per slot.  Returns (buses, bus_frames,
        used, produced, codes): buses is (n_buses, bus_frames * channels) of out_format's storage type (the packed 24-bit
        formats: three bytes a sample), or (n_buses, channels, bus_frames) for out_layout='planar'."""
        n = self.n_legs
        fi = _per_state(in_formats, n)
        caps = [capacity] * n if isinstance(capacity, (int, np.integer)) else list(capacity)
        keep, sides, il, ol = [], [], [], []
        for i in range(n):
            if legs[i] is None:
                sides.append(None), il.append(0), ol.append(0)
                continue
            if chunks[i] is None:
                frames, cap = (int(caps[i][0]), int(caps[i][1])) if isinstance(caps[i], (tuple, list)) else (0, int(caps[i]))
                sides.append(make_side(fi[i], self.channels))
            else:
                a = np.frombuffer(chunks[i], dtype=np.uint8) if not isinstance(chunks[i], np.ndarray) else \
                    np.ascontiguousarray(chunks[i]).reshape(-1).view(np.uint8)
                frames, cap = a.nbytes // (fmt_bytes(fi[i]) * self.channels), int(caps[i])
                if frames * fmt_bytes(fi[i]) * self.channels != a.nbytes:
                    raise ValueError("chunk %d: whole frames only" % i)
                keep.append(a)
                sides.append(make_side(fi[i], self.channels, data=a.ctypes.data if a.nbytes else None))
            il.append(frames), ol.append(cap)
        most, es, layout = max(ol + [1]), fmt_bytes(out_format), _layout(out_layout)
        planar = layout == LAYOUT_PLANAR and self.channels > 1
        out = np.zeros((self.n_buses, most * self.channels * es), np.uint8)
        side = make_side(out_format, self.channels, layout=layout, data=out.ctypes.data, plane_stride=most,
                         stream_stride=most * self.channels)
        rc, used, made, bus_frames, codes = self.process_sides(legs, sides, il, side, ol)
        if bus_frames is None:
            raise RuntimeError(strerror(rc))
        dt = fmt_dtype(out_format)
        if planar:
            buses = out.reshape(self.n_buses, self.channels, most * es)[:, :, : bus_frames * es].copy().view(dt)
        else:
            buses = out[:, : bus_frames * self.channels * es].copy().view(dt)
        return buses, bus_frames, used, made, codes


class SpeexResampler:
    """Python mirror of the reference's TypeScript class (src/index.ts:21-117), over the HIP
    library: same constructor arguments, lazy init, messages, length check and -- crucially --
    the grow-only output-capacity rule (src/index.ts:80-87,95) that decides how many frames
    each processChunk call may emit (and silently drops the rest)."""

    def __init__(self, channels, inRate, outRate, quality=7):
        self.channels, self.inRate, self.outRate, self.quality = channels, inRate, outRate, quality
        self._res = None
        self._outBufferSize = -1

    def processChunk(self, chunk):
        chunk = bytes(chunk) if not isinstance(chunk, (bytes, bytearray, memoryview)) else chunk
        n = len(chunk)
        if self.channels == 0 or n % (self.channels * 2) != 0:  # JS: x % 0 is NaN !== 0
            raise ValueError("Chunk length should be a multiple of channels * 2 bytes")
        if self._res is None:
            self._res = Resampler(self.channels, self.inRate, self.outRate, self.quality)
        target = math.ceil(n * self.outRate / self.inRate)
        if self._outBufferSize < target:
            self._outBufferSize = target
        capacity = int(self._outBufferSize / self.channels / 2)
        frames = np.frombuffer(chunk, dtype=np.int16).reshape(-1, self.channels)
        out, _ = self._res.process(frames, capacity)
        return out.tobytes()
