// kernels_convert_many.hip -- the converting passes of a launch whose streams name different sample formats: the two
// passes either side of a launch group of the formatted many-states call (many.cpp, launch_group).  convert_many_in
// reads each stream's storage in the stream's own format and writes its float image; convert_many_out reads the image
// and stores the stream's format, dithered at the stream's own kind, seed and position where its state says so.
//
// Grid = (tile, stream) and a tile is 4096 samples on 256 lanes, as in kernels_convert.hip.  A stream's format and dither
// kind travel in the `reserved` word of its ConvertStream (convert_many_tag), in the kernel-argument segment, and are read
// by blockIdx.y: scalar loads, wave-uniform, so ONE scalar branch per workgroup selects the body and no lane ever runs
// another format's statements.  The bodies are stream_tile<F, ...> of kernels_convert_impl.h -- the very statements
// convert_in<F> / convert_out<F> / convert_out_dither<F> run, vector path and element path both -- so a stream's bytes are
// those kernels' bytes by construction.  Plain loads and stores, as there: the images are read by the next kernel.
//
// Arguments: the ConvertPack (1024 bytes) and, for the output pass, a DitherPack (520 bytes) whose per-stream seed and
// first index are read only by streams whose kind is not NONE; its own `kind` word is unused here.
//
// convert_many_out_meter: the output pass of a group with a metered state in it (meter.h).  A third argument (MeterPack)
// holds a cell pointer per stream; a stream whose pointer is not NULL leaves through the metered body of its format --
// stream_tile<F, true, dithered_fmt(F), true>, the statements of convert_out_meter<F> -- every other stream exactly as in
// convert_many_out, which is launched as ever when no state of the group has the meter on.
//
// convert_many_out_gain: the output pass of a group with a gained state in it (gain.h).  A fourth argument (GainPack)
// holds every stream's gain; a stream whose gain is off (channels 0) is not multiplied and leaves with the bytes of
// convert_many_out / _meter.
#include <hip/hip_runtime.h>

#include "../../include/speexhip_resampler.h"
#include "dither.h"
#include "format_device.h"
#include "kernels.h"
#include "kernels_convert_impl.h"
#include "meter.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(convert_many)

namespace {

using namespace convert_impl;

// kMeter (kOut only): the launch of a group with a metered state in it -- a stream with a cell leaves through the metered
// body of its format (meter.h: the dithered one at the stream's kind, NONE included, or the plain one of a float format)
// kGain (kOut and kMeter only): the launch of a group with a gained state in it -- every stream leaves through the gained
// body of its format (gain.h), which takes the stream's gain (or none), its kind and its cell (or none) at run time
template <bool kOut, bool kMeter, bool kGain = false>
__device__ __forceinline__ void many_tile(const ConvertPack &pack, const DitherPack *dith, const MeterPack *meter,
                                          const GainPack *gain = nullptr) {
  const ConvertStream &s = pack.s[blockIdx.y];
  MeterCell *const cell = kMeter ? meter->cell[blockIdx.y] : nullptr;
  const int fmt = static_cast<int>(s.reserved & 0xffu), kind = static_cast<int>((s.reserved >> 8) & 0xffu);
  switch (fmt) {
#define SPEEXHIP_MANY_CASE(F)                                                  \
  case F:                                                                      \
    if constexpr (kGain) {                                                     \
      stream_tile<F, true, dithered_fmt(F), true, true>(s, &dith->s[blockIdx.y], kind, cell, &gain->s[blockIdx.y]); \
    } else {                                                                   \
      if constexpr (kMeter) {                                                  \
        if (cell != nullptr) {                                                 \
          stream_tile<F, true, dithered_fmt(F), true>(s, &dith->s[blockIdx.y], kind, cell); \
          break;                                                               \
        }                                                                      \
      }                                                                        \
      if constexpr (kOut && dithered_fmt(F)) {                                 \
        if (kind != SPEEXHIP_DITHER_NONE) {                                    \
          stream_tile<F, true, true>(s, &dith->s[blockIdx.y], kind);           \
          break;                                                               \
        }                                                                      \
      }                                                                        \
      stream_tile<F, kOut, false>(s, nullptr, 0);                              \
    }                                                                          \
    break
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_U8);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S16);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S24);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S32);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_F32N);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_ULAW);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_ALAW);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_F16N);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_BF16N);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S16BE);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S24BE);
    SPEEXHIP_MANY_CASE(SPEEXHIP_FMT_S32BE);
#undef SPEEXHIP_MANY_CASE
    default: break;  // (F32 is the image's own format, anything else the launcher has refused: nothing to do)
  }
}

__global__ __launch_bounds__(kLanes) void convert_many_in(const ConvertPack pack) { many_tile<false, false>(pack, nullptr, nullptr); }
__global__ __launch_bounds__(kLanes) void convert_many_out(const ConvertPack pack, const DitherPack dith) {
  many_tile<true, false>(pack, &dith, nullptr);
}
__global__ __launch_bounds__(kLanes) void convert_many_out_meter(const ConvertPack pack, const DitherPack dith, const MeterPack meter) {
  many_tile<true, true>(pack, &dith, &meter);
}
__global__ __launch_bounds__(kLanes) void convert_many_out_gain(const ConvertPack pack, const DitherPack dith, const MeterPack meter,
                                                                const GainPack gain) {
  many_tile<true, true, true>(pack, &dith, &meter, &gain);
}

}  // namespace

hipError_t launch_convert_many(bool out, const ConvertPack &pack, const DitherPack &dith, uint32_t n, uint64_t most,
                               hipStream_t stream, const MeterPack *meter, const GainPack *gain) {
  if (n == 0 || most == 0) return hipSuccess;
  if (n > kMaxPackedStreams || ((meter != nullptr || gain != nullptr) && !out)) return hipErrorInvalidValue;
  for (uint32_t j = 0; gain != nullptr && j < n; j++)
    if (gain->s[j].channels > 0x7fffffffu) return hipErrorInvalidValue;
  for (uint32_t j = 0; j < n; j++) {
    const ConvertStream &s = pack.s[j];
    if (s.src == nullptr || s.n == 0) continue;
    const int fmt = static_cast<int>(s.reserved & 0xffu), kind = static_cast<int>((s.reserved >> 8) & 0xffu);
    if (s.reserved >> 16 != 0 || sample_bytes(fmt) == 0 || fmt == SPEEXHIP_FMT_F32 || s.step != 1 || s.dst == nullptr || s.n > most)
      return hipErrorInvalidValue;
    if (kind != SPEEXHIP_DITHER_NONE && (!out || !dithered_fmt(fmt) || !dither::known_kind(kind))) return hipErrorInvalidValue;
  }
  const dim3 grid(static_cast<uint32_t>((most + kTile - 1) / kTile), n), block(kLanes);
  const MeterPack no_cells = {};
  if (gain != nullptr)
    hipLaunchKernelGGL(convert_many_out_gain, grid, block, 0, stream, pack, dith, meter != nullptr ? *meter : no_cells, *gain);
  else if (meter != nullptr)
    hipLaunchKernelGGL(convert_many_out_meter, grid, block, 0, stream, pack, dith, *meter);
  else if (out)
    hipLaunchKernelGGL(convert_many_out, grid, block, 0, stream, pack, dith);
  else
    hipLaunchKernelGGL(convert_many_in, grid, block, 0, stream, pack);
  return hipGetLastError();
}

}  // namespace speexhip
