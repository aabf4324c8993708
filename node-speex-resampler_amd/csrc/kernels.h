// kernels.h -- host-callable launchers of the HIP kernels (product code).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/speexhip_resampler.h"
#include "device_types.h"
#include "filter_design.h"

namespace speexhip {

// ---- the sample formats (SPEEXHIP_FMT_*): what host and device both need to know of them, stated once ----------------
// bytes of one sample; 0 = no such format
constexpr uint32_t sample_bytes(int fmt) {
  switch (fmt) {
    case SPEEXHIP_FMT_U8:
    case SPEEXHIP_FMT_ULAW:
    case SPEEXHIP_FMT_ALAW: return 1;
    case SPEEXHIP_FMT_S16:
    case SPEEXHIP_FMT_S16BE:
    case SPEEXHIP_FMT_F16N:
    case SPEEXHIP_FMT_BF16N: return 2;
    case SPEEXHIP_FMT_S24:
    case SPEEXHIP_FMT_S24BE: return 3;
    case SPEEXHIP_FMT_S32:
    case SPEEXHIP_FMT_S32BE:
    case SPEEXHIP_FMT_F32:
    case SPEEXHIP_FMT_F32N: return 4;
    default: return 0;
  }
}
// the formats a state with dither on dithers on their way out: the integer ones, and the companded ones (g711.h), which
// quantise to int16 on theirs, and the big-endian ones; the float formats, the half ones among them, are written as they are
constexpr bool dithered_fmt(int fmt) {
  return fmt == SPEEXHIP_FMT_U8 || fmt == SPEEXHIP_FMT_S16 || fmt == SPEEXHIP_FMT_S24 || fmt == SPEEXHIP_FMT_S32 ||
         fmt == SPEEXHIP_FMT_ULAW || fmt == SPEEXHIP_FMT_ALAW || fmt == SPEEXHIP_FMT_S16BE || fmt == SPEEXHIP_FMT_S24BE ||
         fmt == SPEEXHIP_FMT_S32BE;
}

// Kernel attributes (the opt-in for more than 64 KiB of dynamic LDS) are per DEVICE: set them the
// first time a kernel is launched on each device of the process.  `seen` = one bit per device id;
// two threads racing on a first use both set the (idempotent) attribute before either launches.
template <typename K>
inline void opt_in_lds_on_this_device(K kern, std::atomic<uint64_t> &seen) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (seen.load(std::memory_order_acquire) & bit) return;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
  seen.fetch_or(bit, std::memory_order_release);
}

// Warm-up: each translation unit with kernels is a code object of its own, loaded onto a device by the first launch from
// it (2-4 ms of a process's first call, tools/first_call.py).  Every such unit defines an empty kernel and
// warm_unit_<name>(stream), which launches it; speexhip_warmup runs them all off the caller's path.
#define SPEEXHIP_WARM_UNIT(name)                                             \
  __global__ void warm_kernel_##name() {}                                    \
  void warm_unit_##name(hipStream_t s) {                                     \
    hipLaunchKernelGGL(warm_kernel_##name, dim3(1), dim3(64), 0, s);          \
    (void)hipGetLastError();                                                 \
  }
void warm_unit_exact(hipStream_t s);
void warm_unit_period(hipStream_t s);
void warm_unit_slide_i16(hipStream_t s);
void warm_unit_slide_f32(hipStream_t s);
void warm_unit_slide64_i16(hipStream_t s);
void warm_unit_slide64_f32(hipStream_t s);
void warm_unit_period64(hipStream_t s);
void warm_unit_period_pp(hipStream_t s);
void warm_unit_period_odd(hipStream_t s);
void warm_unit_period_frames(hipStream_t s);
void warm_unit_period64_w16(hipStream_t s);
void warm_unit_period_w16g(hipStream_t s);
void warm_unit_planar(hipStream_t s);
void warm_unit_convert(hipStream_t s);
void warm_unit_convert_many(hipStream_t s);
void warm_unit_mix(hipStream_t s);
void warm_unit_sides(hipStream_t s);

// compute units of the calling thread's current device (cached per device id)
inline uint32_t device_compute_units() {
  static std::atomic<int> cached[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int n = cached[dev & 63].load(std::memory_order_relaxed);
  if (n == 0) {
    n = 256;
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    cached[dev & 63].store(n, std::memory_order_relaxed);
  }
  return static_cast<uint32_t>(n);
}

// ---- bit-exact kernels (kernels_exact.hip) -------------------------------------------------
struct ExactGeometry {
  int ct = 1;                  // channels per lane (2 when the channel count is even)
  uint32_t channel_groups = 1;
  uint32_t outs_per_block = 256;
  uint32_t span_cap = 0;
  size_t lds_bytes = 0;
  bool staged = true;          // false: filter/window too large for LDS, read through L2
};
ExactGeometry exact_geometry(const FilterSpec &f, uint32_t channels, size_t lds_budget);
// strides (samples between two frames of a channel) of a launch that is not a plain interleaved one;
// zero = resampler_basic_zero (resample.c:561-591)
struct ExactStrides {
  uint32_t in, out, hist;
};
hipError_t launch_exact(const FilterSpec &f, const ExactGeometry &g, const float *d_table,
                        uint32_t channels, const DescPack *pack,
                        uint32_t n_streams, uint32_t max_n_out, bool float_io, hipStream_t stream,
                        const ExactStrides *strides = nullptr, bool zero = false);

// ---- primary fast kernel: period-lane mapping, taps in SGPRs (kernels_period.hip) ----------
struct PeriodPlan {         // per filter, fixed at init
  bool usable = false;
  uint32_t r = 10, ct = 1, cgroups = 0, groups = 0;
  uint32_t row_len = 0, l4 = 0, tail_frames = 0, lane_periods = 0;
  uint32_t pad = 0;          // LDS bank padding (elements after every period), 0 = none needed
  bool w16 = false;          // the LDS window holds int16 samples (2-byte elements) instead of floats: int16
                             // calls only; twice the periods per tile where the float window limits them
  bool a64 = false;          // fp64 accumulator (round 4): the tap rows are doubles, a loop trip is half as many steps,
                             // rows_floats counts doubles
  bool pp = false;           // phase pairs (round 4; mono): a lane owns ONE period and 2r phases per group -- a tile is
                             // 64 periods, not 128 (half the window), the rows are [step][2r]
  size_t rows_floats = 0, window_bytes = 0;
  bool float_ok = true;      // false (late in round 5): not even one period of the FLOAT window fits the LDS; the plan stands for
                             // its int16-window plan to hang off (int16 calls run over that), float calls take the exact kernel
  uint32_t fold = 1;         // round 6: planned on a folded view of the filter (FilterSpec::fold, period_view): the kernel's
                             // num and den are fold times the filter's
};
// Round 6: ratios with den <= 6 that the slide kernel does not cover (7:6, 11:1, 16:3, 25:1 ...) ran the exact kernel,
// ~5x slower.  They get the period kernel on a FOLDED view: *view = f with num, den and fold multiplied so that den becomes
// a multiple of 5 that is at least 10 (whole groups of five phases); returns true and fills *view (a copy of f, table
// included) when this (filter, channel count) wants it, false (view untouched) otherwise.
bool period_view(const FilterSpec &f, uint32_t channels, FilterSpec *view);
// LDS of a workgroup of the period kernel's staged-store instance (round 7, kernels_period_impl.h: StagedImage): the
// window at the front, the output image at the end -- the planners' whole budget (engine.cpp, kLdsBudget)
constexpr uint32_t kStagedLdsBytes = 150 * 1024;
PeriodPlan plan_period(const FilterSpec &f, uint32_t channels, size_t lds_budget, bool w16 = false, bool a64 = false,
                       bool pp = false);
PeriodPlan plan_period_r(const FilterSpec &f, uint32_t channels, size_t lds_budget, uint32_t r, bool w16 = false,
                         bool a64 = false, bool pp = false);
// Does this filter of up to three channels get phase-pair plans beside its other ones (wide windows: num >= 320), and
// should THIS launch run over `pp`?  `two` = the plan the launch would take otherwise (kernels_period.hip).
bool period_wants_pp_plans(const FilterSpec &f, uint32_t channels);
bool period_launch_prefers_pp(const FilterSpec &f, const PeriodPlan &two, const PeriodPlan &pp, const StreamDesc *h_descs,
                              uint32_t n_streams);
// Host only: tiles, phase-group splits, waves with a group, tap-range shares, lanes and whether the workgroups fetch the
// tap rows, as launch_period_plan would set them for this launch of `t` (speexhip_debug_launch_shape).
bool debug_period_shape(const FilterSpec &f, const PeriodPlan &t, uint32_t channels, const StreamDesc *h_descs, uint32_t n_streams,
                        bool float_io, uint32_t out[6]);
// The int16-window plan of a filter whose float plan is `t`, .usable only where it pays: at least 5/4 of the
// periods per tile (the loop converts every sample it reads: ~20 % more vector instructions per tile).
PeriodPlan plan_period_w16(const FilterSpec &f, uint32_t channels, size_t lds_budget, const PeriodPlan &t);
void build_period_rows(const FilterSpec &f, const PeriodPlan &t, std::vector<float> *rows);
// ... of an a64 plan: t.rows_floats doubles, then the per-group tables (uint32, bit-copied into the tail)
void build_period_rows64(const FilterSpec &f, const PeriodPlan &t, std::vector<double> *rows);
// `fine`: the same filter planned with r = 5 (or null); single-generation launches take it
hipError_t launch_period(const FilterSpec &f, const PeriodPlan &t, const float *d_rows, const PeriodPlan *fine,
                         const float *d_rows_fine, uint32_t channels, const StreamDesc *h_descs,
                         const DescPack *pack, uint32_t n_streams, bool float_io,
                         hipStream_t stream, bool fixed_shape = false);
// fixed_shape (SPEEXHIP_MODE_FAST_FIXED, round 5): no tap-range shares / parts -- the only launch-time choice that
// changes the ORDER in which an output's products are summed (partial sums of tap ranges meeting in LDS).  Everything
// else a launch chooses -- phases per wave, int16 or float window, phase pairs, phase-group splits, trimmed head and
// tail trips, tile size -- adds the same products in the same order (or skips exact zeros), so with this flag an
// output's bits depend on the stream alone: not on chunking, batch size, launch size or the GPU's CU count.

// Should this int16 launch run over the int16-window plan rather than `t` (the float-window plan, `has_fine`: with
// an r = 5 companion)?  Launches of few tiles want more and shorter pieces (kernels_period.hip).
bool period_launch_prefers_w16(const FilterSpec &f, const PeriodPlan &t, bool has_fine, const StreamDesc *h_descs,
                               uint32_t n_streams);

// ---- small-ratio fast kernel (kernels_slide.hip): den <= 6, num <= 4 -------------------------
struct SlidePlan {
  bool usable = false;
  bool pair_ch = true;      // packed FMA over channel pairs (even channel count) or phase pairs
  uint32_t p = 8, num = 1, np = 1, cgroups = 1, row_stride = 0, row_len = 0;
};
SlidePlan plan_slide(const FilterSpec &f, uint32_t channels);
size_t slide_lds_bytes(const SlidePlan &t, uint32_t waves);  // LDS of a workgroup of `waves` waves
void build_slide_rows(const FilterSpec &f, const SlidePlan &t, std::vector<float> *rows);
hipError_t launch_slide(const FilterSpec &f, const SlidePlan &t, const float *d_rows, uint32_t channels,
                        const StreamDesc *h_descs, const DescPack *pack,
                        uint32_t n_streams, bool float_io, hipStream_t stream, bool fixed_shape = false);

// ---- ... with an fp64 accumulator (kernels_slide64_impl.h, round 4): the reference's "double" kernels (quality 9
// and 10, resample.c:389-435, :501-558) on the same ratios.  The plan reuses SlidePlan: np = den (accumulators per
// period), cgroups = channels (one lane per channel of a lane block), pair_ch unused. ------------------------------
SlidePlan plan_slide64(const FilterSpec &f, uint32_t channels);
void build_slide64_rows(const FilterSpec &f, const SlidePlan &t, std::vector<double> *rows);
hipError_t launch_slide64(const FilterSpec &f, const SlidePlan &t, const double *d_rows, uint32_t channels,
                          const StreamDesc *h_descs, const DescPack *pack,
                          uint32_t n_streams, bool float_io, hipStream_t stream, bool fixed_shape = false);

// ---- channel planes <-> interleaved frames (kernels_planar.hip): the two passes either side of a planar call ------
struct PlanarStream {       // one stream's share of a transposing launch
  const void *planes;       // plane 0 (gather: read, scatter: written); plane c starts plane_stride elements further
  uint64_t plane_stride;    // elements between two planes (>= frames)
  void *inter;              // the interleaved image (gather: written, scatter: read); 16-byte aligned
  uint32_t frames;          // frames per channel to move; 0 (or planes == NULL) = nothing
  uint32_t reserved;
};
struct PlanarPack {         // like DescPack: up to 32 streams, in the kernel-argument segment
  PlanarStream s[kMaxPackedStreams];
};
// frames of a workgroup's tile: 16 bytes per lane and plane, 256 lanes
inline uint32_t planar_tile_frames(bool float_io) { return float_io ? 1024u : 2048u; }
// planes -> interleaved (gather) / interleaved -> planes (scatter) for streams [0, n) of `pack`; max_frames = the
// largest PlanarStream::frames among them
hipError_t launch_planar_gather(const PlanarPack &pack, uint32_t n, uint32_t channels, uint32_t max_frames, bool float_io,
                                hipStream_t stream);
hipError_t launch_planar_scatter(const PlanarPack &pack, uint32_t n, uint32_t channels, uint32_t max_frames, bool float_io,
                                 hipStream_t stream);

// ---- sample formats <-> the internal float image (kernels_convert.hip): the two passes either side of a formatted call
struct ConvertStream {      // one stream's share of a converting launch
  const void *src;          // convert_in: storage of the call's format, convert_out: the float image; NULL = nothing
  void *dst;                // convert_in: the float image, convert_out: storage
  uint64_t n;               // samples to convert
  uint32_t step;            // elements between two samples, in both buffers (1; the channel count when one channel of
                            // interleaved frames is converted: a state whose channels stand apart)
  uint32_t reserved;
};
struct ConvertPack {        // like DescPack: up to 32 streams, in the kernel-argument segment
  ConvertStream s[kMaxPackedStreams];
};

// ---- channel mix folded into the conversion (kernels_mix.hip): the pass of a mixed call's side that has a matrix ------
// mix_in: storage of the call's format, src_channels per frame -> the float image, dst_channels per frame;
// mix_out: the float image -> storage.  One frame of the destination = the matrix times the frame of the source, every
// output summed in fp64 in ascending index order and rounded once to fp32 (include/speexhip_resampler.h).
constexpr uint32_t kMixMaxChannels = 8;   // per side of a matrix: its coefficients travel in the kernel-argument segment
struct MixStream {          // one stream's share of a mixing launch
  const void *src;          // mix_in: storage, mix_out: the float image; NULL = nothing
  void *dst;                // mix_in: the float image, mix_out: storage
  uint32_t frames;          // frames to mix
  uint32_t reserved;
};
struct MixPack {            // like ConvertPack: up to 32 streams and the matrix, in the kernel-argument segment
  MixStream s[kMaxPackedStreams];
  float m[kMixMaxChannels * kMixMaxChannels];  // row-major dst_channels x src_channels
  uint32_t src_channels, dst_channels;
};

// ---- dither on the way out (dither.h): convert_out_dither<F> / mix_out_dither<F>, the output pass of a formatted or mixed
// call of a state with dither on, for the formats of dithered_fmt.  The streams' arguments are the undithered pass's; what
// the dither needs travels beside them in a second kernel argument.
struct DitherStream {       // one stream's share
  uint64_t seed;            // the stream's own seed
  uint64_t first;           // convert_out_dither: idx of the stream's sample 0 of this launch (position * channels);
                            // mix_out_dither: the stream's position, idx = (first + frame) * dst_channels + channel
};
struct DitherPack {         // like ConvertPack: up to 32 streams, in the kernel-argument segment (520 bytes)
  DitherStream s[kMaxPackedStreams];
  int32_t kind;             // SPEEXHIP_DITHER_*: one for the launch, wave-uniform
  uint32_t reserved;
};

// ---- the meter on the way out (meter.h): the metered instances of the output passes -- convert_out_meter<F>,
// convert_many_out_meter, mix_out_meter<F>, planes_out_meter<F> -- and meter_image, of a state with the meter on.  Each
// workgroup adds what its samples came to into its stream's cell; the cells' addresses travel in a last kernel argument.
struct MeterCell {          // one stream's totals, in device memory
  uint64_t hi, lo, nan;     // samples clipped at the upper rail / at the lower rail / that were NaN
  uint32_t peak_bits;       // bits of the largest |y| (int16 units) among the samples that were not NaN
  uint32_t pad;
};
struct MeterPack {          // like ConvertPack: up to 32 streams, in the kernel-argument segment (256 bytes)
  MeterCell *cell[kMaxPackedStreams];  // convert_many_out_meter: NULL = a stream that is not metered
};

// ---- the gain on the way out (gain.h): the gained instances of the output passes -- convert_out_gain<F>,
// convert_many_out_gain, mix_out_gain<F>, planes_out_gain<F> -- and gain_image, of a state with a stream's gain on.  One
// instance per format and pass: dither and meter are taken at run time (kind NONE: d = 0; a NULL cell: nothing committed).
struct GainStream {         // one stream's share: g(k) = (float)(from + k * step) for k < total, to from there on
  double step;              // (to - from) / total, formed on the host by set_gain
  uint64_t first;           // k of the stream's frame 0 of this launch
  float from, to;
  uint32_t total;
  uint32_t channels;        // 0: the stream's gain is off, nothing is multiplied; otherwise the samples of an output
                            // frame in a converting pass (frame = sample / channels), 1 in the passes that walk frames
};
struct GainPack {           // like ConvertPack: up to 32 streams, in the kernel-argument segment (1024 bytes; the largest
  GainStream s[kMaxPackedStreams];  // pass, PlanePack + DitherPack + MeterPack + GainPack, is 3096 of its 4096)
};

// ---- the launchers of a pass over streams [0, n) of `pack` -------------------------------------------------------------
// fmt = the storage side's format: any SPEEXHIP_FMT_* for a mix, any but F32 for a conversion (that IS the image's
// format).  out: image -> storage, otherwise storage -> image.  dith = NULL: the plain instances; otherwise the dithered
// ones (out only, a dithered_fmt, every ConvertStream::step 1: sample k of a stream has idx first + k).  most = the
// largest ConvertStream::n / MixStream::frames among the streams.  What a launcher refuses (and channel counts of a
// matrix outside 1..8) it refuses with hipErrorInvalidValue before it launches.
// meter = NULL: exactly the above.  Otherwise (out only, every step 1) the metered instances, for every format: the
// formats of dithered_fmt through the dithered body -- dith = NULL: kind NONE, d = 0, the undithered bytes -- and the
// float ones through the plain body; stream j is judged into meter->cell[j].
// gain = NULL: exactly the above.  Otherwise (out only, every step 1) the gained instance of the format: stream j's
// samples are multiplied by its g (gain->s[j]; channels 0: not at all) and then leave as above -- dithered when dith is
// given, judged when meter is (both at run time).
hipError_t launch_convert(int fmt, bool out, const ConvertPack &pack, const DitherPack *dith, uint32_t n, uint64_t most,
                          hipStream_t stream, const MeterPack *meter = nullptr, const GainPack *gain = nullptr);
hipError_t launch_mix(int fmt, bool out, const MixPack &pack, const DitherPack *dith, uint32_t n, uint32_t most,
                      hipStream_t stream, const MeterPack *meter = nullptr, const GainPack *gain = nullptr);
// gain_image (kernels_convert.hip): multiplies the n floats at pack.s[j].dst in place by the stream's g (frame = sample /
// gain.s[j].channels; channels 0: left alone) -- the result of a call that has no output pass.  meter != NULL: a stream
// whose cell is not NULL is judged in the same pass, product * scale as a float format (launch_meter_image's rule).
hipError_t launch_gain_image(const ConvertPack &pack, const GainPack &gain, const MeterPack *meter, float scale, uint32_t n,
                             uint64_t most, hipStream_t stream);
// meter_image (kernels_convert.hip): reads the n samples at pack.s[j].src (floats; dst and step are not read) and judges
// stored * scale as a float format into meter.cell[j] -- the result of a call that has no output pass.  Writes nothing else.
hipError_t launch_meter_image(const ConvertPack &pack, const MeterPack &meter, float scale, uint32_t n, uint64_t most,
                              hipStream_t stream);

// ---- ... with a format per stream (kernels_convert_many.hip): the passes of a launch group of the formatted many-states
// call.  Stream j's format and dither kind travel in its ConvertStream::reserved (convert_many_tag); every step is 1.  out:
// a stream whose kind is not NONE (a dithered_fmt then) leaves through the dithered body with dith.s[j].seed and .first
// (idx of its sample 0: position * channels); dith.kind is not read.  F32 streams have no pass: leave their src NULL.
constexpr uint32_t convert_many_tag(int fmt, int dither_kind) {
  return static_cast<uint32_t>(fmt) | (static_cast<uint32_t>(dither_kind) << 8);
}
// meter (out only) = the launch of a group with a metered state in it: a stream whose cell is not NULL leaves through the
// metered body of its format (meter.h), every other one exactly as without.
// gain (out only) = the launch of a group with a gained state in it: convert_many_out_gain, where every stream leaves
// through the gained body of its format -- multiplied by its own g (channels 0: not at all), dithered at its kind, judged
// into its cell when it has one.
hipError_t launch_convert_many(bool out, const ConvertPack &pack, const DitherPack &dith, uint32_t n, uint64_t most,
                               hipStream_t stream, const MeterPack *meter = nullptr, const GainPack *gain = nullptr);

// ---- channel planes of any format <-> the float image (kernels_sides.hip): the pass of a side whose layout is planar --
// planes_in: C planes of the call's format -> the interleaved float image; planes_out: the image -> planes.  Conversion,
// the channel matrix (when the side has one) and the dither happen in the same pass as the transposition.
// frames of a workgroup's tile, for every format (whole 16-byte pieces of a plane: 64 pieces of the 1-byte formats and
// packed s24, 128 of s16, 256 of the 4-byte formats)
constexpr uint32_t kSidesTileFrames = 1024;
struct PlaneStream {        // one stream's share of a launch
  const void *src;          // planes_in: plane 0 of the storage, planes_out: the float image; NULL = nothing
  void *dst;                // planes_in: the float image, planes_out: plane 0
  uint64_t plane_stride;    // samples of the format between two planes (>= frames)
  uint32_t frames;          // frames to move
  uint32_t reserved;
};
struct PlanePack {          // like MixPack: up to 32 streams and the matrix, in the kernel-argument segment
  PlaneStream s[kMaxPackedStreams];
  float m[kMixMaxChannels * kMixMaxChannels];  // row-major destination x source channels; read when mixed != 0
  uint32_t storage_channels;  // planes of a stream
  uint32_t image_channels;    // samples the pass reads or writes per frame of the image
  uint32_t image_pitch;       // floats between two frames of the image: image_channels, or more when the pass moves one
                              // channel of wider frames (a state whose channels stand apart)
  uint32_t mixed;             // 0: plane c is channel c of the image (any channel count); otherwise m applies, 1..8 a side
};
// dith as for launch_mix: DitherStream::first = the stream's position, idx = (first + frame) * storage_channels + plane
// meter and gain as for launch_mix
hipError_t launch_planes(int fmt, bool out, const PlanePack &pack, const DitherPack *dith, uint32_t n, uint32_t most,
                         hipStream_t stream, const MeterPack *meter = nullptr, const GainPack *gain = nullptr);

// ---- mix buses (kernels_bus.hip): the weighted sums of a batch's streams, between the float call and the output pass of
// a bus call (bus.h states the sum).  Stream s is frames[s] frames of `channels` floats at src[s]; bus j is bus_frames
// frames at dst + j * dst_pitch, every sample the sum over ALL n_streams streams of W[j][s] times the stream's sample
// behind its gain (gain.s[s], GainStream::channels = `channels`, or 0: not multiplied), a stream that has ended
// supplying +0.0f.  w is the device copy of W, transposed and padded: W[j][s] at w[s * 32 + j], 32 x 32 floats, zeros
// behind n_buses -- the eight weights a workgroup needs of a stream are one aligned scalar load.
struct BusPack {            // like ConvertPack: up to 32 streams, in the kernel-argument segment
  const float *src[kMaxPackedStreams];
  uint32_t frames[kMaxPackedStreams];
  float *dst;               // bus 0
  uint64_t dst_pitch;       // floats between two buses (>= bus_frames * channels)
  const float *w;           // device memory
  uint32_t n_streams, n_buses;   // 1..32 each
  uint32_t channels;
  uint32_t bus_frames;      // >= every frames[s]
};
// buses a workgroup sums in one trip: 8 x 4 fp64 accumulators beside a lane's four samples (DESIGN, "Mix buses")
constexpr uint32_t kBusGroup = 8;
hipError_t launch_bus_sum(const BusPack &pack, const GainPack &gain, hipStream_t stream);
void warm_unit_bus(hipStream_t s);

// ---- ... of a mixer's legs (kernels_bus_legs.hip): the same sum over the slots of a mixer (include/speexhip_resampler.h,
// "Mixer"), whose legs are too many for a kernel-argument pack.  The legs' records lie in DEVICE memory, one per slot in
// slot order (they ride in the call's one transfer in), and so does W: the mixer's resident copy, transposed and padded --
// W[j][s] at w[s * w_pitch + j], w_pitch = n_buses rounded up to kBusGroup (a row's pairs are 8-byte aligned), zeros behind n_buses.  Leg s is frames frames
// of `channels` floats at src (frames 0: an empty slot, a refused leg, a leg that produced nothing -- +0.0f throughout,
// summed like any other); bus j is bus_frames frames at dst + j * dst_pitch.
constexpr uint32_t kBusMaxLegs = SPEEXHIP_MIXER_MAX_LEGS, kBusMaxBuses = SPEEXHIP_MIXER_MAX_BUSES;
struct BusLeg {             // one slot's record: 64 bytes, so that a record never straddles a cache line
  const float *src;         // the leg's float image of this call (device memory)
  uint32_t frames;          // frames it produced
  uint32_t reserved;
  GainStream gain;          // first = the leg's done; channels = the mixer's, or 0: not multiplied
  uint64_t pad[2];
};
static_assert(sizeof(BusLeg) == 64, "the leg table is an array of whole lines");
struct BusLegsArgs {
  const BusLeg *legs;       // device memory, n_legs records
  const float *w;           // device memory
  float *dst;               // bus 0
  uint64_t dst_pitch;       // floats between two buses (>= bus_frames * channels)
  uint32_t w_pitch;         // floats between two legs' rows of w
  uint32_t n_legs, n_buses; // 1..1024 each
  uint32_t channels;
  uint32_t bus_frames;      // >= every frames
};
// host_legs: the same records where the host can read them (the launcher checks them before it launches)
hipError_t launch_bus_sum_legs(const BusLegsArgs &a, const BusLeg *host_legs, hipStream_t stream);
void warm_unit_bus_legs(hipStream_t s);

// ---- the levels of a mixer's legs (kernels_levels.hip; levels.h states the record): one SpeexHipLevel per slot over the
// very table bus_sum_legs reads -- src and frames, BEFORE the gain.  legs: the table in device memory, host_legs: the same
// records where the host can read them (the launcher checks them before it queues anything: a null table, a leg with
// frames > bus_frames, a leg with frames but no src).  records: n_legs records where the kernel can write them -- device
// memory, or the pinned stage of a small call; no atomic touches them.  A call in which every leg is at most one span of
// kLevelSpan samples is ONE launch that writes the records; otherwise the spans' partials go to `partials` (device
// memory, partials_room bytes >= n_legs * level_spans() records) and a second launch folds them.  bus_frames == 0:
// nothing launched.  *launches (may be null): the launches queued, added.
constexpr uint32_t kLevelSpan = 65536;
struct LevelsArgs {
  const BusLeg *legs;       // device memory, one record per workgroup row
  SpeexHipLevel *dst;       // spans == 1: the records; else the partials, slot-major, `spans` a slot
  uint32_t channels;
  uint32_t spans;           // spans of the longest leg, >= 1
};
uint64_t level_spans(const BusLeg *host_legs, uint32_t n_legs, uint32_t channels);
hipError_t launch_leg_levels(const BusLeg *legs, const BusLeg *host_legs, uint32_t n_legs, uint32_t channels, uint32_t bus_frames,
                             SpeexHipLevel *records, SpeexHipLevel *partials, size_t partials_room, hipStream_t stream,
                             uint32_t *launches);
void warm_unit_levels(hipStream_t s);

}  // namespace speexhip
