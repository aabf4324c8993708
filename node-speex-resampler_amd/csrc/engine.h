// engine.h -- host engine: owns device state for a batch of independent streams that share
// one filter, plans each call on the host and launches the HIP kernels (product code).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/speexhip_resampler.h"
#include "bus_out.h"
#include "device_types.h"
#include "engine_detail.h"
#include "filter_design.h"
#include "filter_plans.h"
#include "host_transfer.h"
#include "kernels.h"
#include "sides_route.h"
#include "stream_plan.h"

namespace speexhip {

const char *last_device_error();  // text of the most recent HIP failure on this thread
void set_last_device_error(const std::string &text);
size_t lds_budget();  // LDS the planners may give one workgroup (of the CU's 160 KiB)
// Test hook: the n-th next device allocation of a filter install fails (resample.c:785-791 path); 0 = off.
void debug_fail_device_allocs(int n);
// speexhip_debug_many_counters: process-wide counts since start, of the many-states calls old and new -- FIR launches, input
// passes, output passes, entries that took their own call.
void many_counters(uint64_t out[4]);
// speexhip_debug_chunk_counters: the same four counts over the formatted chunks call (process_sides_host_chunks); chunks
// that took a call of their own in the place of entries.
void chunk_counters(uint64_t out[4]);
// speexhip_debug_mixer_counters: of the mixer calls -- FIR launches, input passes, bus-sum launches, output passes,
// transfers in, transfers out.
void mixer_counters(uint64_t out[6]);

// Everything on the device that depends only on (filter, channel count): the reference-layout sinc
// table, the fast kernels' tap rows and the launch geometry.  Immutable once built, so states with
// the same (num, den, quality, channels) share one copy (a cache in engine.cpp keeps the most recent
// ones alive between states): a second `new SpeexResampler(2, 44100, 48000, 7)` designs nothing and
// uploads nothing.
struct DeviceTables {
  int device = 0;
  FilterPlans plans;                         // filter_plans.h: every plan of the filter, held here and nowhere else
  float *table = nullptr;                    // reference layout (exact kernel)
  void *period_rows[kPeriodVariants] = {};   // tap rows of plans.period[v]: floats, doubles for the fp64 variants; null
                                             // where the variant has none (FilterPlans::has_rows)
  float *slide_rows = nullptr;               // kernels_slide.hip
  double *slide64_rows = nullptr;            // kernels_slide64_impl.h: fp64 taps (filters of the reference's double kinds)
  size_t bytes = 0;
  DeviceTables() = default;
  DeviceTables(const DeviceTables &) = delete;
  DeviceTables &operator=(const DeviceTables &) = delete;
  ~DeviceTables();
};
// speexhip_warmup: the runtime's and the pool's one-time start-up costs on `device` (< 0: every device the placement
// rule can choose), paid now instead of by the first states.
int warmup(int device);
// Idle cache entries back to the pool (speexhip_release_cached_memory); the bytes they held.
size_t release_cached_tables();

// One side of a formatted or mixed call (process_sides_*).
struct CallSide {
  int fmt;            // SPEEXHIP_FMT_* of the caller's storage
  uint32_t channels;  // samples of a frame there: the state's count, or with a matrix any of 1..8
  const float *mix;   // host memory, row-major: input side channels() x channels, applied to every frame before the float
                      // call; output side channels x channels(), applied to every frame it produced.  NULL: no mix
  void *base;         // stream 0 (an input side is only read; NULL there: silence)
  uint64_t stride;    // samples of fmt between two streams
  // Layout (SPEEXHIP_LAYOUT_*): interleaved -- frame f, channel c at sample f * channels + c -- or planar -- at
  // c * plane_stride + f.  Layout changes where a sample lies and nothing else.  A side of one channel is the same bytes
  // either way and is served as interleaved.
  int layout;                      // (0 = interleaved: what a side built without the members below gets)
  uint64_t plane_stride;           // planar: samples of fmt between two planes (>= the frames moved)
  void *const *planes;             // planar, host calls only: plane c = planes[c] (separate allocations) instead of
                                   // base + c * plane_stride
};
// a side the formatted calls can read: with a matrix both channel counts are 1..8, without one the caller's count is the state's
inline bool side_ok(const CallSide &side, uint32_t state_channels) {
  if (sample_bytes(side.fmt) == 0) return false;
  if (side.layout != SPEEXHIP_LAYOUT_INTERLEAVED && side.layout != SPEEXHIP_LAYOUT_PLANAR) return false;
  if (side.mix == nullptr) return side.channels == state_channels;
  return state_channels <= kMixMaxChannels && side.channels >= 1 && side.channels <= kMixMaxChannels;
}
// ... whose planes a pass has to walk (a side of one channel is the same bytes in either layout)
inline bool side_planar(const CallSide &side) { return side.layout == SPEEXHIP_LAYOUT_PLANAR && side.channels != 1; }
// ... as the route of its call sees it (sides_route.h)
inline SideKind side_kind(const CallSide &side) { return SideKind{side.fmt, side.mix != nullptr, side_planar(side), side.planes != nullptr}; }

// What a mixer call (mixer.h) hands the unit machinery of the many-states calls (many.cpp, Batch::many_mixer) beside its
// legs: the sum that stands behind the legs' launches, and the buses' output stage (bus_out.h), which the unit grows the
// image of and has encode the buses.  The mixer owns all of it; the unit leaves bus_frames.
struct MixerCall {
  int device = 0;
  uint32_t n_legs = 0;
  const float *d_w = nullptr;    // the resident copy of W as bus_sum_legs reads it (kernels.h)
  uint32_t w_pitch = 0;
  CallSide out = {};             // the buses in host memory
  SidesRoute bus_route;          // of the bus side (SidesForm::Bus); pass_out false: bus_sum_legs writes the stage itself
  BusOutput *buses = nullptr;
  uint32_t bus_frames = 0;       // out: the length of the buses
  // The legs' levels ("Mixer levels"; kernels_levels.hip), when the mixer has them on: n_legs records, which the unit
  // fills from the range that travelled out -- all zeros on entry, and left so by a call of bus_frames 0 -- and the
  // mixer's device block for the partials of a call whose legs span more than one launch row, grown by the unit.
  SpeexHipLevel *levels = nullptr;   // nullptr: off -- nothing measured, nothing launched, not a byte more travels
  char **level_parts = nullptr;
  size_t *level_parts_cap = nullptr;
};
// speexhip_debug_mixer_level_launches: the launches of the levels' kernels since start (apart from mixer_counters)
uint64_t mixer_level_launches();

class Batch {
 public:
  // Returns nullptr and sets *err on failure.  device: logical ordinal (devices.h), or < 0 for the process-wide
  // placement rule (SPEEXHIP_DEVICE / SPEEXHIP_DEVICES, default = the calling thread's current HIP device).
  static Batch *create(uint32_t n_streams, uint32_t channels, uint32_t in_rate, uint32_t out_rate,
                       int quality, int *err, int device = -1);
  // speex_resampler_init_frac (resample.c:799): ratio given separately from the nominal rates.
  static Batch *create_frac(uint32_t n_streams, uint32_t channels, uint32_t ratio_num, uint32_t ratio_den,
                            uint32_t in_rate, uint32_t out_rate, int quality, int *err, int device = -1);
  ~Batch();

  // Device-resident call for all streams; asynchronous on `stream`.
  // float_io selects the sample type of in/out: int16 (process_interleaved_int) or float
  // (process_interleaved_float); strides are in samples of that type.
  int process_device(const void *d_in, uint64_t in_stride, uint32_t *in_len, void *d_out,
                     uint64_t out_stride, uint32_t *out_len, bool float_io, hipStream_t stream);
  // The same call on channel planes (planar.cpp): plane c of stream s starts at d_in + s * in_stream_stride +
  // c * in_plane_stride (elements; a plane stride >= the frame count), likewise on the output side.  It IS the
  // interleaved call on the same frames -- counters, samples and the state left behind -- between two transposing
  // kernels (kernels_planar.hip) and per-state scratch images; a mono plane goes straight to process_device.
  int process_planar_device(const void *d_in, uint64_t in_stream_stride, uint64_t in_plane_stride, uint32_t *in_len,
                            void *d_out, uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len,
                            bool float_io, hipStream_t stream);
  // ... and on host planes (one pointer per channel; in_planes == nullptr: silence) of a single-stream batch;
  // synchronous.  Each plane moves by the rule of host_transfer.h.
  int process_planar_host(const void *const *in_planes, uint32_t *in_len, void *const *out_planes, uint32_t *out_len,
                          bool float_io);
  // Formatted and mixed calls (formats.cpp): the caller names each side's sample format, and a side may carry a channel
  // matrix (CallSide).  One pipeline: storage --the input side's pass--> float image of channels() channels
  // --process_device(float)--> float image --the output side's pass--> storage, on the state's scratch images (the
  // planar calls' ones: calls on a state are ordered).  A side's pass is convert_* (kernels_convert.hip), with a matrix
  // mix_* (kernels_mix.hip), of a planar side planes_* (kernels_sides.hip), which converts, mixes and dithers while it
  // transposes.  Counters, positions and the history are the float call's.  Which calls are an existing call on the
  // caller's own bytes, which passes run, who finishes a result that no pass writes, what moves afterwards and which
  // states are refused with BAD_STATE: route_sides_call (sides_route.h), for this and every other form of the call.
  // plans_out: the plan of every channel of a state whose channels stand apart, empty otherwise.
  int process_sides_device(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len, hipStream_t stream,
                           std::vector<CallPlan> *plans_out = nullptr);
  // ... on host buffers of a single-stream batch (strides unused); synchronous.  The raw bytes of both sides move by the
  // rule of host_transfer.h, the passes run on the device.
  // With a planar side: an interleaved side still moves by that rule, a planar one plane by plane into a pitched image as
  // in process_planar_host; PTR_OVERLAP when the frames written to an output plane overlap another plane of the call.
  int process_sides_host(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len);
  // n_chunks consecutive process_sides_host calls of a single-stream batch as one transfer each way and one wait
  // (formats.cpp): chunk i is exactly process_sides_host on the state chunk i - 1 left -- its data, in_len[i] and
  // out_len[i], and an output side that begins at the frames already written -- bytes (in the modes whose bytes do not
  // depend on the launch's shape), counters, history, position and dither position.  `in` describes every chunk's input
  // (its base and planes are not read); chunk i lies at in_data[i], a planar chunk's plane c at in_data[i * channels + c];
  // in_data == nullptr or a null (first) entry: a chunk of silence.  `out` is an ordinary host output side with room for
  // the sum of the capacities: the results lie back to back in its buffer, or in every plane.  Only the frames a chunk
  // consumes travel (process_host_chunks); the passes run once over all chunks, the FIR once per run of chunks without
  // dropped input.  Which calls ARE process_host_chunks and which states take the separate calls: SidesForm::Chunks.
  int process_sides_host_chunks(uint32_t n_chunks, const CallSide &in, const void *const *in_data, uint32_t *in_len,
                                const CallSide &out, uint32_t *out_len);
  // Dither of the integer output formats of the formatted and mixed calls (dither.h; include/speexhip_resampler.h,
  // "Dither"): a property of the state, off by default.  kind = SPEEXHIP_DITHER_*; stream s draws from
  // dither::stream_seed(seed, s); position = index of the next output frame of every stream.  While the kind is not NONE
  // every formatted or mixed call advances each stream's position by the frames it produced and the formats of
  // dithered_fmt (kernels.h) leave through the dithered instances of their pass (the routes: sides_route.h).  No other
  // call reads or moves any of this, and no control call (set_rate, set_quality, reset_mem, skip_zeros) touches it.
  int set_dither(int kind, uint64_t seed, uint64_t position);
  int get_dither(uint32_t stream, int *kind, uint64_t *seed, uint64_t *position) const;  // seed: the stream's own
  // The output meter of the formatted, mixed and sides calls (meter.h; include/speexhip_resampler.h, "Metering"): a
  // property of the state, off by default.  While it is on every such call -- host, device, batch, many-states, chunks --
  // is judged on its output side, sample by sample as it is encoded, into the stream's MeterCell in device memory: by the
  // metered instances of its output pass, or, where the call has none (a float result written by the FIR itself), by
  // meter_image over the result (the routes: sides_route.h).  The int16, float, planar, per-channel,
  // chunks_int / _float, many_int / _float and take calls are never metered.  `samples` is kept here on the host: frames
  // produced x samples of an output frame, added when a call commits.  set_meter keeps the totals; no control call
  // (set_rate, set_quality, reset_mem, skip_zeros, set_dither) touches the switch or the totals.
  int set_meter(int on);
  // The totals of `stream` (m may be null): waits on the host for this state's own last call, as the control calls do --
  // never for the device -- and fetches the cells in one small copy.  reset: that stream's totals are zero from here on.
  int get_meter(uint32_t stream, SpeexHipMeter *m, bool reset);
  // The output gain of the formatted, mixed and sides calls (gain.h; include/speexhip_resampler.h, "Gain"): per stream
  // (from, to, total, done), off by default (to == 1 and no ramp in flight).  While any stream of the state has its gain
  // on, every such call -- host, device, batch, many-states, chunks -- leaves through the gained instance of its output
  // pass, which multiplies every sample of output frame f of a stream by g(done + f); a result that no pass writes (the
  // float call on the same bytes, interleaved F32 without a matrix) is multiplied in place by gain_image behind the FIR
  // launch, which judges it as well when the meter is on (the routes: sides_route.h).  A stream whose own gain is off is
  // not multiplied (selected per stream, wave-uniformly).  Every such call moves done by the frames produced, up to total.  The int16, float, planar,
  // per-channel, chunks_int / _float, many_int / _float and take calls neither apply the gain nor move done, and no
  // control call (set_rate, set_quality, reset_mem, skip_zeros, set_dither, set_meter) touches it.
  // set_gain: from = the gain the stream's next output frame would have had, to = gain, total = ramp_frames, done = 0;
  // stream = UINT32_MAX: every stream.  A gain that is not finite: INVALID_ARG, nothing changed.
  int set_gain(uint32_t stream, float gain, uint32_t ramp_frames);
  // current = g(done), target = to, remaining = total - done (any may be null)
  int get_gain(uint32_t stream, float *current, float *target, uint32_t *remaining) const;
  // Mix buses (bus.cpp, bus.h; include/speexhip_resampler.h, "Buses"): a state may carry a matrix W of n_buses x
  // n_streams() weights, off by default; while it is off nothing here is read.  set_buses copies W (host, row-major) and
  // uploads its device copy, makes the buses' meter cells, zeroes their totals and the bus position; n_buses == 0 or
  // weights == nullptr: off.  More than 32 buses, a state of more than 32 streams (the streams' image pointers travel in
  // one kernel-argument pack) or a weight that is not finite: INVALID_ARG, the state as it was.  No other control call
  // touches any of this.
  int set_buses(uint32_t n_buses, const float *weights);
  int get_buses(uint32_t *n_buses, float *weights) const;  // (either may be null)
  // The bus call: the input side's pass -> process_device(float) into the state's image -> bus_sum (kernels_bus.hip: every
  // bus the fp64 sum of all streams' samples behind their gains, a stream that has ended supplying +0.0f) into a grow-only
  // image of the buses -> the buses' output stage (bus_out.h), which encodes that image, dithered from the bus seeds at the
  // bus position and judged into the bus cells.  An interleaved F32 bus side is written by bus_sum itself (and read by
  // meter_image when the meter is on).  Counters, history and positions of every stream are the float
  // call's; the streams' gains move by what they produced, their dither positions and meter totals do not move: nothing
  // of theirs is encoded.  out_len: the streams' capacities in, their produced frames out; *bus_frames = the largest of
  // them, the length of every bus.  No buses set, or a stream whose channels stand apart: BAD_STATE; out.mix: INVALID_ARG.
  int process_bus_device(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len, uint32_t *bus_frames,
                         hipStream_t stream);
  int get_bus_meter(uint32_t bus, SpeexHipMeter *m, bool reset);  // as get_meter, of a bus's cell
  uint64_t bus_position() const { return bus_out_.position(); }  // the buses' one dither position
  // Host-buffer call for a single-stream batch; synchronous (H2D, kernels, D2H).
  int process_host(const void *in, uint32_t *in_len, void *out, uint32_t *out_len, bool float_io);
  // The same call with the result left in a pinned block of the pool that the caller then OWNS (release_block):
  // the kernel writes the block straight through PCIe, so the samples cross memory once on their way out instead
  // of twice (device or pinned buffer -> copy -> the caller's buffer).  *block = nullptr when nothing was written.
  int process_host_take(const void *in, uint32_t *in_len, uint32_t *out_len, bool float_io, void **block);
  static void release_block(void *block);
  // Host-buffer calls of n single-stream states at once (SURVEY 8b "array of states/buffers"; the reference's model
  // is many instances in one process, src/index.ts:18-45): per GPU one transfer in, one launch per <= 32 states that
  // share a filter, one transfer out; states on different GPUs run side by side (a GPU is a PCIe link of its own).
  // Samples and counters of state i are exactly those of process_host(in[i], &in_len[i], out[i], &out_len[i]);
  // codes[i] (may be null) = that call's return code; returns the first code that is not SUCCESS.
  static int process_host_many(uint32_t n, Batch *const *states, const void *const *in, uint32_t *in_len,
                               void *const *out, uint32_t *out_len, bool float_io, int *codes);
  // ... with a format per state (formats.cpp): entry i is exactly process_sides_host(in[i], &in_len[i], out[i],
  // &out_len[i]) on states[i] -- bytes (in the modes whose bytes do not depend on the launch's shape: FAST_FIXED, EXACT),
  // counters, history, position, dither position and code.  bad (may be null): bad[i]
  // != 0 = the caller's side could not be read (INVALID_ARG, nothing runs for it).  The entries that SidesForm::ManyEntry
  // calls fusable are fused -- per launch group of <= 32 states one input pass (kernels_convert_many.hip), one FIR launch
  // and one output pass, whatever formats the states name.  Every other entry takes its own process_sides_host call, in
  // the caller's order, after the fused ones.
  static int process_host_many_sides(uint32_t n, Batch *const *states, const CallSide *in, uint32_t *in_len,
                                     const CallSide *out, uint32_t *out_len, const uint8_t *bad, int *codes);
  int device() const { return device_; }
  // n_chunks consecutive host-buffer calls of a single-stream batch as one launch; outputs are
  // written back to back into `out` (room for the sum of the capacities).
  int process_host_chunks(uint32_t n_chunks, const void *const *in, uint32_t *in_len, void *out,
                          uint32_t *out_len, bool float_io);
  // One channel of a single-stream batch through host buffers with the state's input / output
  // strides: speex_resampler_process_int / _process_float (resample.c:927-1036).  Channels
  // advance independently, as in the reference (per-channel last_sample / samp_frac_num /
  // magic_samples, resample.c:135-137).
  int process_channel_host(uint32_t channel, const void *in, uint32_t *in_len, void *out, uint32_t *out_len,
                           bool float_io);
  void set_strides(uint32_t in_stride, uint32_t out_stride, bool set_in, bool set_out) {
    if (set_in) in_stride_ = in_stride;
    if (set_out) out_stride_ = out_stride;
  }
  uint32_t in_stride() const { return in_stride_; }
  uint32_t out_stride() const { return out_stride_; }
  // position of one channel (resample.c last_sample / samp_frac_num / magic_samples)
  StreamPos channel_pos(uint32_t s, uint32_t c) const { return pos_[static_cast<size_t>(s) * channels_ + c]; }
  bool zero_mode() const { return zero_mode_; }

  // Mid-stream control (reference resample.c:1084-1220).  These wait for the
  // device, re-align every stream's history on the host (resample.c:727-782) and rebuild the
  // filter tables; they apply to all streams of the batch.
  int set_rate_frac(uint32_t ratio_num, uint32_t ratio_den, uint32_t in_rate, uint32_t out_rate);
  int set_quality(int quality);
  int skip_zeros();
  int reset_mem();
  int input_latency() const { return static_cast<int>(filter_.taps / 2); }
  int output_latency() const {
    return static_cast<int>(((filter_.taps / 2) * filter_.den + (filter_.num >> 1)) / filter_.num);
  }

  // Counters of the next call for stream s, state untouched.
  CallPlan peek(uint32_t s, uint32_t in_len, uint32_t out_capacity, bool float_io) const;

  int set_mode(int mode);
  // The caller is about to destroy the stream of the state's last device-pointer call: order what is still in
  // flight on it behind an event of the state's own and forget the stream.
  int release_stream();
  void info(uint32_t stream, SpeexHipInfo *out) const;
  int history(uint32_t stream, float *dst);
  const FilterSpec &filter() const { return filter_; }
  // What speex_resampler_get_rate / get_ratio report: the filter's rates, except after a set_rate_frac that
  // returned RESAMPLER_ERR_OVERFLOW -- the reference has stored the new ones by then (resample.c:1119-1127).
  struct RateView {
    uint32_t in_rate, out_rate, num, den;
  };
  RateView rates() const {
    return shown_valid_ ? shown_ : RateView{filter_.in_rate, filter_.out_rate, filter_.num, filter_.den};
  }
  uint32_t n_streams() const { return n_streams_; }
  uint32_t channels() const { return channels_; }

 private:
  Batch() = default;
  int setup();
  int install_filter(const FilterSpec &f, const std::vector<float> &hist, uint32_t hist_frames_cap);
  int adopt_filter(const FilterSpec &next);
  int change_filter(const FilterSpec &next, int design_rc, const std::vector<uint32_t> *fracs);
  void enter_zero_mode(const FilterSpec &partly_designed);
  StreamPos &P(uint32_t s, uint32_t c) { return pos_[static_cast<size_t>(s) * channels_ + c]; }
  const StreamPos &P(uint32_t s, uint32_t c) const { return pos_[static_cast<size_t>(s) * channels_ + c]; }
  bool uniform(uint32_t s) const;  // all channels of stream s at the same position
  uint32_t max_magic(uint32_t s) const;
  int run_channel(uint32_t c, const void *d_in, uint32_t in_stride, uint32_t in_frames, void *d_out,
                  uint32_t out_stride, const CallPlan &plan, bool float_io, hipStream_t stream);
  struct SplitLayout {  // where process_split finds channel c and its samples (elements)
    uint64_t in_channel, out_channel;
    uint32_t in_sample, out_sample;
  };
  int process_split(const void *d_in, uint32_t *in_len, void *d_out, uint32_t *out_len, bool float_io,
                    hipStream_t stream, std::vector<CallPlan> *plans_out, const SplitLayout *layout = nullptr);
  int ensure_planar_scratch(size_t in_bytes, size_t out_bytes);
  // mix.cpp: one side's pass over every stream, <= kMaxPackedStreams per launch -- to_image: storage -> image, otherwise
  // image -> storage, dithered when the state and the format say so.  Stream s is lens[s] frames at side.base + s *
  // side.stride and image + s * pitch (elements).  apart (an output side without a matrix): the plans of the one
  // stream's channels, which stand apart -- channel c is plans[c].produced samples, channels() elements from one to the next.
  int side_pass(const CallSide &side, bool to_image, char *image, size_t pitch, const uint32_t *lens, hipStream_t stream,
                const CallPlan *apart = nullptr);
  bool dither_on() const { return dither_kind_ != SPEEXHIP_DITHER_NONE; }
  // the DitherPack of streams [s0, s0 + n): first = position * per_frame (per_frame = 1: the position itself)
  DitherPack dither_pack(uint32_t s0, uint32_t n, uint32_t per_frame) const;
  void dither_advance(const uint32_t *produced);  // after a formatted or mixed call with dither on
  // the cells of streams [s0, s0 + n), as a metered launch takes them
  MeterPack meter_pack(uint32_t s0, uint32_t n) const;
  void meter_count(const uint32_t *produced, uint32_t per_frame);  // after a formatted or mixed call with the meter on
  // meter_image over what a call without an output pass wrote: stream s is lens[s] frames of channels() floats at
  // result + s * stride (floats), judged as stored * scale
  int meter_result(const void *result, uint64_t stride, const uint32_t *lens, float scale, hipStream_t stream);
  // whether any stream's gain is on: the state's formatted calls then take the gained routes
  bool gain_on() const;
  // the gains of streams [s0, s0 + n), as a gained launch takes them: first = the stream's done; per_frame = the samples
  // of an output frame in a pass that walks samples, 1 in the passes that walk frames (a stream whose gain is off: 0)
  GainPack gain_pack(uint32_t s0, uint32_t n, uint32_t per_frame) const;
  void gain_advance(const uint32_t *produced);  // after a formatted or mixed call with gain on
  // What a call without an output pass wrote (meter_result's arguments), finished in place: gain_image when gain is on --
  // which judges its product too when the meter is on -- meter_image otherwise.
  int image_result(void *result, uint64_t stride, const uint32_t *lens, float scale, hipStream_t stream);
  // The route of a formatted call (sides_route.h): the state as the rule sees it; what a call that ran moves afterwards --
  // meter totals (per_frame samples a frame), gain ramps, dither positions; and the float images with the input pass
  // (formats.cpp), shared by the sides call and the bus call.
  SidesState sides_state(bool repeated = false) const;
  void sides_moved(const SidesRoute &r, const uint32_t *produced, uint32_t per_frame);
  struct SideImages {
    const void *in;      // what the float call reads: the input image, or the caller's F32 storage
    uint64_t in_stride;  // floats between two streams there
    size_t out_pitch;    // floats between two streams of the output image
    uint32_t most_out;   // the most frames any stream (or channel that stands apart) will produce
  };
  int prepare_images(const CallSide &in, const uint32_t *in_len, const uint32_t *out_len, const SidesRoute &r, bool split, bool bus,
                     hipStream_t stream, SideImages *im);
  // process_sides_host of a call with a planar side
  int planes_host_call(const CallSide &in, uint32_t *in_len, const CallSide &out, uint32_t *out_len);
  int fetch_history(std::vector<float> *host);
  int quiesce();  // waits for this batch's own enqueued work (never for the whole device)
  uint32_t block_in() const { return line_ - (filter_.taps - 1); }
  EntryRules entry_rules(bool float_io) const {
    EntryRules rules;
    rules.block_in = block_in();
    rules.float_entry = float_io;
    return rules;
  }
  // The most frames any channel of the one stream can produce from `frames` frames into room for `capacity` (integer
  // arithmetic, nothing launched): only so many need a staging buffer.
  uint32_t will_make(uint32_t frames, uint32_t capacity) const;
  // Extents: the one host rule for what a single call may ask of the 32-bit counts below it.  The
  // launchers round a frame or period count up to whole tiles in 32 bits (count + tile - 1, tiles of at most a few
  // thousand), and the slide kernels end a call's outputs at k_shift + n_out (k_shift < den) in 32 bits.  A call fits
  // when its in_len and the outputs it can make (the closed form: capacity and input both bound it) leave
  // kExtentSlack + den below 2^32; every entry point asks before it touches anything and returns
  // SPEEXHIP_ERR_OVERFLOW otherwise.  in_len / out_len: one pair of lengths for each of the first n streams.
  static constexpr uint32_t kExtentSlack = 1u << 16;
  bool lengths_fit(const uint32_t *in_len, const uint32_t *out_len, uint32_t n) const;
  // frames each of n channels of a result received: `all`, or -- channels that stand apart -- each channel's own
  static std::vector<uint32_t> made_per_channel(uint32_t n, uint32_t all, const CallPlan *apart) {
    std::vector<uint32_t> made(n, all);
    for (uint32_t c = 0; apart != nullptr && c < n; c++) made[c] = apart[c].produced;
    return made;
  }
  // host_call.cpp -- the mechanics of a single-state host-buffer call around its device call: what route_host_call
  // (host_transfer.h) decided, carried out on own_stream_ and the state's staging buffers.
  //   HostCall call(this);  call.begin(route, pieces, ...);  <the device call on call.src / call.dst>;  call.finish_...(...)
  // The calls are synchronous and their buffers go on to the next call: whichever way the function is left before a
  // finish_* has waited, `drain` waits for everything enqueued.
  struct HostPiece {    // a run of host memory and where it lies in the side's staging image
    const void *host;   // (an input piece at nullptr: zeros)
    size_t at, bytes;
  };
  struct HostCall {
    explicit HostCall(Batch *batch) : b(batch), drain(&batch->own_stream_) {}
    // Set before begin by the one entry point each concerns: where a take call's completion word lies (else the tail of
    // the pinned result buffer); the samples of a strided line (route.strided) -- line_es bytes each, line_step samples
    // apart in the caller's memory, 0 included: every frame reads the first sample.
    void *word = nullptr;
    uint32_t line_step = 0;
    size_t line_es = 0;
    // Takes the staging buffers and brings the input -- one region, the planes of an image, gathered chunks, a strided
    // line -- to where the kernels read it.  pinned_in / pinned_out: the device's view of a side used in place.
    int begin(const HostRoute &route, const HostPiece *in, uint32_t n_in, const void *pinned_in, void *pinned_out);
    const void *src = nullptr;  // what the device call reads (nullptr: silence) ...
    void *dst = nullptr;        // ... and writes
    // The result back, the wait, the hand-over: the first `bytes` of the image as they are; plane c's first made[c]
    // samples from `pitch` bytes apart; or sample by sample -- channel c's first made[c] samples of frames of n samples
    // into frames of host_step samples (channels that stand apart; n = 1: a strided line).
    int finish_whole(void *out, size_t bytes);
    int finish_planes(void *const *planes, uint32_t n, size_t pitch, size_t es, const uint32_t *made);
    int finish_samples(void *out, uint32_t n, uint32_t host_step, size_t es, const uint32_t *made);

   private:
    int wait();
    Batch *b;
    detail::DrainOnExit drain;
    HostRoute r;
  };
  int ensure_stage(size_t dev_in, size_t dev_out, size_t pin_in, size_t pin_out);
  static void pinned_sides(const void *in, size_t in_bytes, void *out, size_t out_bytes, const void **pin_in, void **pin_out);
  int run_plans(const void *d_in, uint64_t in_stride, const uint32_t *in_frames, void *d_out,
                uint64_t out_stride, const CallPlan *plans, bool float_io, hipStream_t stream);
  // The descriptor of stream s (from its channel c on: 0 for a launch of whole frames) for `plan`: the two history
  // pointers of the ping-pong as it stands and the position fields.  in_frames = frames readable at `in`.
  void fill_desc(StreamDesc &d, uint32_t s, uint32_t c, const void *in, void *out, uint32_t in_frames, const CallPlan &plan) const;
  int launch_chunk(const StreamDesc *descs, const DescPack &pack, uint32_t n, uint32_t max_out, bool float_io,
                   hipStream_t stream);
  // a large host call as pieces: input copies on a second stream, one launch per piece behind each (process_host_take)
  int take_in_pieces(const void *in, uint32_t *in_len, uint32_t *out_len, bool float_io, void *blk, uint32_t pieces);
  // One entry of a many-states call, as many_run takes it.
  struct ManyEntry {
    Batch *b = nullptr;
    int rc = SPEEXHIP_ERR_SUCCESS;      // not SUCCESS: an argument error found already; nothing runs for the entry
    const void *in = nullptr;           // the entry's interleaved host buffers, in_fmt / out_fmt samples
    void *out = nullptr;
    int in_fmt = SPEEXHIP_FMT_S16, out_fmt = SPEEXHIP_FMT_S16;
    bool sides = false;                 // an entry of process_host_many_sides: its own call is process_sides_host on
    CallSide in_side = {}, out_side = {};  // these, and the state's dither, meter and gain count
    SidesRoute route;                   // many_run's: fused or its own call, and as what (SidesForm::ManyEntry)
    bool leg = false;                   // a leg of a mixer call (SidesForm::MixerLeg): `out` is not read, nothing travels back
  };
  static int many_run(uint32_t n, ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *codes);
  // The legs of a mixer call (entries[i].leg, rc SUCCESS; i = the slot) as ONE unit on the mixer's device: staged, grouped
  // and launched as many_run's fused entries are, their results left as float images on the device; behind them the table
  // of all n slots, bus_sum_legs, the buses' output pass and the one transfer out (many.cpp).  rcs[i] of a leg that ran:
  // SUCCESS, or the zero fallback's ALLOC_FAILED.
  static int many_mixer(MixerCall &mc, uint32_t n, ManyEntry *entries, uint32_t *in_len, uint32_t *out_len, int *rcs);
  friend class Mixer;  // mixer.cpp: describes its legs as ManyEntry, asks their route and their extents
  struct ManyUnit;  // many.cpp: the fused entries of one (device, lane), planned by many_plan.h and carried out
  bool have_copy_stream();  // copy_stream_ = a pool stream other than own_stream_ (false: none -> no piecewise call)

  FilterSpec filter_;
  uint32_t n_streams_ = 0, channels_ = 0;
  int device_ = 0;
  bool counted_ = false;  // this state is in its device's live count (devices::state_born)
  int mode_ = SPEEXHIP_MODE_FAST_FIXED;  // (round 6: the default is the mode whose bytes depend on the stream alone)
  std::vector<StreamPos> pos_;    // [stream][channel] (the reference keeps them per channel, resample.c:135-137;
                                  // interleaved calls move all channels of a stream together)
  bool zero_mode_ = false;        // resampler_ptr == resampler_basic_zero (resample.c:785-791): the last
                                  // filter change failed; outputs are zeros until one succeeds
  uint32_t in_stride_ = 1, out_stride_ = 1;  // resample.c:842-843, 1170-1188 (per-channel entry points)
  RateView shown_ = {0, 0, 0, 0};  // see rates()
  bool shown_valid_ = false;
  std::vector<uint8_t> started_;  // per stream: a block has run (resample.c:886), so a filter
                                  // change must re-align the history instead of clearing it
  uint32_t line_ = 0;             // frames per channel line, grow-only (resample.c
                                  // "mem_alloc_size", :709-720): block size = line_-(taps-1)

  // Everything of the filter on the device and every plan made for it (DeviceTables: shared between states, immutable).
  // The launches read the plans and the row pointers through it; while zero_mode_ holds it is still the set of the last
  // filter that could be built, of which only the sinc table's address and the exact geometry's channel split are used.
  std::shared_ptr<const DeviceTables> tables_;
  float *d_hist_[2] = {nullptr, nullptr};  // float, like the reference's `mem`
  size_t hist_elems_ = 0;  // per stream: (taps-1 + room for pending frames)*channels
  size_t hist_bytes_ = 0;  // allocation of each history buffer (>= the copy-engine minimum, engine.cpp kCtlCopyMin)
  int hist_cur_ = 0;

  bool float_seen_ = false;  // a float call has put samples into the histories that an int16 window cannot hold
  void int16_call_done(const CallPlan *plans, uint32_t n);  // ... until int16 calls have replaced all of them (round 6)

  // Calls on one batch are chained: a call on another stream than the previous one waits for it on the device
  // (an event recorded on the previous stream at that moment), control calls and the destructor wait for the
  // previous stream on the host.  So the stream of a device-pointer call must outlive the state's next call --
  // unless the caller hands it back with release_stream(): the event is recorded then and the stream forgotten.
  // (Round 4 tried an event of the batch's own recorded behind EVERY device-pointer launch, so that nothing would
  // ever be asked of a caller's stream after its call: +3.0 us per launch on this stack -- BASELINE configs[1]
  // 11.7 -> 14.7 us per step, profiles/r04_ab_done_event.txt.  And a stale handle cannot be recognised after the
  // fact: this runtime dereferences it -- hipStreamSynchronize / hipEventRecord on a destroyed stream segfault,
  // tools/probe_stream_gone.hip.)
  hipStream_t last_stream_ = nullptr;
  bool have_last_stream_ = false;
  hipEvent_t order_ev_ = nullptr;
  bool ev_pending_ = false;          // order_ev_ stands for the batch's last work (release_stream)
  int chain_to(hipStream_t stream);  // before a launch on `stream`

  // host-buffer path (single stream)
  hipStream_t own_stream_ = nullptr;
  hipStream_t copy_stream_ = nullptr;   // input copies of a piecewise call (another of the pool's streams)
  static const int kMaxPieces = 8;
  hipEvent_t piece_ev_[kMaxPieces] = {};
  char *d_stage_in_ = nullptr, *d_stage_out_ = nullptr;
  char *h_pin_in_ = nullptr, *h_pin_out_ = nullptr;
  // planar calls (planar.cpp): the interleaved images either side of the existing launch; per state, grow-only
  char *d_planar_in_ = nullptr, *d_planar_out_ = nullptr;
  size_t planar_in_cap_ = 0, planar_out_cap_ = 0;  // bytes
  int dither_kind_ = SPEEXHIP_DITHER_NONE;  // set_dither
  uint64_t dither_seed_ = 0;
  std::vector<uint64_t> dither_pos_;        // per stream: index of its next output frame (empty until set_dither: 0)
  bool meter_on_ = false;                   // set_meter
  MeterCell *d_meter_ = nullptr;            // one cell per stream (null until the meter is first turned on)
  std::vector<uint64_t> meter_samples_;     // per stream: samples metered since the last reset
  struct Gain {                             // one stream's gain (gain.h)
    double step = 0.0;                      // (to - from) / total, formed by set_gain
    float from = 1.0f, to = 1.0f;
    uint32_t total = 0, done = 0;
  };
  std::vector<Gain> gain_;                  // per stream (empty until set_gain: off)
  // buses (bus.cpp): n_buses_ == 0 = off.  W, and behind the sum the buses' output stage: their dither, meter, cells,
  // totals, position and image (bus_out.h)
  uint32_t n_buses_ = 0;
  std::vector<float> bus_w_;                // W as the caller gave it: n_buses_ x n_streams_, row-major
  char *d_bus_ = nullptr;                   // the 32 x 32 floats of W as bus_sum reads it (BusPack::w), from the first set_buses on
  BusOutput bus_out_;
  uint32_t done_seq_ = 0;  // completion word of the small host-buffer calls (engine.cpp, process_host)
  size_t stage_in_cap_ = 0, stage_out_cap_ = 0, pin_in_cap_ = 0, pin_out_cap_ = 0;  // bytes
};

}  // namespace speexhip
