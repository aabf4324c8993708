// c_api.cpp -- the extern "C" boundary declared in include/speexhip_resampler.h.
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/speexhip_resampler.h"
#include "bus.h"
#include "devices.h"
#include "dither.h"
#include "gain.h"
#include "levels.h"
#include "meter.h"
#include "engine.h"
#include "mixer.h"
#include "filter_plans.h"
#include "g711.h"
#include "halfbe.h"
#include "pool.h"

using speexhip::Batch;

namespace {
// No C++ exception may cross the C boundary: a host allocation that fails inside a call (descriptor
// vectors, the history image of a filter change, a multi-gigabyte sinc table) becomes the
// reference's RESAMPLER_ERR_ALLOC_FAILED, anything else the device error code with its text.
template <typename F>
int guarded(F &&f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return SPEEXHIP_ERR_ALLOC_FAILED;
  } catch (const std::exception &e) {
    speexhip::set_last_device_error(std::string("internal error: ") + e.what());
    return SPEEXHIP_ERR_DEVICE;
  } catch (...) {
    speexhip::set_last_device_error("internal error: unknown exception");
    return SPEEXHIP_ERR_DEVICE;
  }
}
}  // namespace

struct SpeexHipResamplerState_ {
  Batch *batch;
};
struct SpeexHipBatch_ {
  Batch *batch;
};
struct SpeexHipMixer_ {
  speexhip::Mixer *mixer;
};

extern "C" {

int speexhip_device_count(void) { return speexhip::devices::count(); }
int speexhip_warmup(int device) {
  return guarded([&] { return speexhip::warmup(device); });
}
int speexhip_debug_placement(int device_count, const char *env_device, const char *env_devices, uint64_t k,
                             int current_device) {
  return speexhip::devices::placement_rule(device_count, env_device, env_devices, k, current_device);
}

int speexhip_debug_placement_live(int device_count, const char *env_device, const char *env_devices, uint64_t k,
                                  int current_device, const uint32_t *live) {
  return speexhip::devices::placement_rule_live(device_count, env_device, env_devices, k, current_device, live);
}
uint32_t speexhip_debug_live_states(int device) { return speexhip::devices::live_states(device); }

SpeexHipResamplerState *speexhip_resampler_init(uint32_t nb_channels, uint32_t in_rate,
                                                uint32_t out_rate, int quality, int *err) {
  return speexhip_resampler_init_on(-1, nb_channels, in_rate, out_rate, quality, err);
}

SpeexHipResamplerState *speexhip_resampler_init_on(int device, uint32_t nb_channels, uint32_t in_rate,
                                                   uint32_t out_rate, int quality, int *err) {
  Batch *b = nullptr;
  int code = SPEEXHIP_ERR_SUCCESS;
  const int rc = guarded([&] {
    b = Batch::create(1, nb_channels, in_rate, out_rate, quality, &code, device < 0 ? -1 : device);
    return code;
  });
  if (err) *err = rc;
  if (b == nullptr) return nullptr;
  SpeexHipResamplerState *st = new (std::nothrow) SpeexHipResamplerState_{b};
  if (st == nullptr) {
    delete b;
    if (err) *err = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  return st;
}

SpeexHipResamplerState *speexhip_resampler_init_frac(uint32_t nb_channels, uint32_t ratio_num,
                                                     uint32_t ratio_den, uint32_t in_rate, uint32_t out_rate,
                                                     int quality, int *err) {
  Batch *b = nullptr;
  int code = SPEEXHIP_ERR_SUCCESS;
  const int rc = guarded([&] {
    b = Batch::create_frac(1, nb_channels, ratio_num, ratio_den, in_rate, out_rate, quality, &code);
    return code;
  });
  if (err) *err = rc;
  if (b == nullptr) return nullptr;
  SpeexHipResamplerState *st = new (std::nothrow) SpeexHipResamplerState_{b};
  if (st == nullptr) {
    delete b;
    if (err) *err = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  return st;
}

int speexhip_resampler_set_rate(SpeexHipResamplerState *st, uint32_t in_rate, uint32_t out_rate) {
  return guarded([&] { return st ? st->batch->set_rate_frac(in_rate, out_rate, in_rate, out_rate) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_resampler_set_rate_frac(SpeexHipResamplerState *st, uint32_t ratio_num, uint32_t ratio_den,
                                     uint32_t in_rate, uint32_t out_rate) {
  return guarded([&] { return st ? st->batch->set_rate_frac(ratio_num, ratio_den, in_rate, out_rate) : SPEEXHIP_ERR_INVALID_ARG; });
}
void speexhip_resampler_get_ratio(SpeexHipResamplerState *st, uint32_t *ratio_num, uint32_t *ratio_den) {
  *ratio_num = st->batch->rates().num;
  *ratio_den = st->batch->rates().den;
}
int speexhip_resampler_set_quality(SpeexHipResamplerState *st, int quality) {
  return guarded([&] { return st ? st->batch->set_quality(quality) : SPEEXHIP_ERR_INVALID_ARG; });
}
void speexhip_resampler_get_quality(SpeexHipResamplerState *st, int *quality) {
  *quality = st->batch->filter().quality;
}
int speexhip_resampler_get_input_latency(SpeexHipResamplerState *st) { return st->batch->input_latency(); }
int speexhip_resampler_get_output_latency(SpeexHipResamplerState *st) { return st->batch->output_latency(); }
int speexhip_resampler_skip_zeros(SpeexHipResamplerState *st) {
  return guarded([&] { return st ? st->batch->skip_zeros() : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_resampler_reset_mem(SpeexHipResamplerState *st) {
  return guarded([&] { return st ? st->batch->reset_mem() : SPEEXHIP_ERR_INVALID_ARG; });
}

int speexhip_batch_set_rate_frac(SpeexHipBatch *b, uint32_t ratio_num, uint32_t ratio_den, uint32_t in_rate,
                                 uint32_t out_rate) {
  return guarded([&] { return b ? b->batch->set_rate_frac(ratio_num, ratio_den, in_rate, out_rate) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_set_quality(SpeexHipBatch *b, int quality) {
  return guarded([&] { return b ? b->batch->set_quality(quality) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_skip_zeros(SpeexHipBatch *b) { return guarded([&] { return b ? b->batch->skip_zeros() : SPEEXHIP_ERR_INVALID_ARG; }); }
int speexhip_batch_reset_mem(SpeexHipBatch *b) { return guarded([&] { return b ? b->batch->reset_mem() : SPEEXHIP_ERR_INVALID_ARG; }); }
int speexhip_batch_get_history(SpeexHipBatch *b, uint32_t stream, float *dst) {
  if (b == nullptr || dst == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->history(stream, dst); });
}

void speexhip_resampler_destroy(SpeexHipResamplerState *st) {
  if (st == nullptr) return;
  delete st->batch;
  delete st;
}

int speexhip_resampler_process_interleaved_int(SpeexHipResamplerState *st, const int16_t *in,
                                               uint32_t *in_len, int16_t *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || (out == nullptr && *out_len != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host(in, in_len, out, out_len, false); });
}

int speexhip_resampler_process_interleaved_int_device(SpeexHipResamplerState *st, const int16_t *d_in,
                                                      uint32_t *in_len, int16_t *d_out,
                                                      uint32_t *out_len, void *hip_stream) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_device(d_in, 0, in_len, d_out, 0, out_len, false,
                                   static_cast<hipStream_t>(hip_stream)); });
}

int speexhip_resampler_process_interleaved_int_take(SpeexHipResamplerState *st, const int16_t *in, uint32_t *in_len,
                                                    uint32_t *out_len, int16_t **out_block) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || out_block == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host_take(in, in_len, out_len, false, reinterpret_cast<void **>(out_block)); });
}

int speexhip_resampler_process_interleaved_float_take(SpeexHipResamplerState *st, const float *in, uint32_t *in_len,
                                                      uint32_t *out_len, float **out_block) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || out_block == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host_take(in, in_len, out_len, true, reinterpret_cast<void **>(out_block)); });
}

void speexhip_block_release(void *block) {
  if (block != nullptr) speexhip::Batch::release_block(block);
}

void *speexhip_block_acquire(uint64_t bytes) {
  void *p = nullptr;
  const int rc = guarded([&] {
    return speexhip::pool::block_get(&p, static_cast<size_t>(bytes)) ? SPEEXHIP_ERR_SUCCESS : SPEEXHIP_ERR_NO_BLOCK;
  });
  return rc == SPEEXHIP_ERR_SUCCESS ? p : nullptr;
}

int speexhip_resampler_process_interleaved_float(SpeexHipResamplerState *st, const float *in,
                                                 uint32_t *in_len, float *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || (out == nullptr && *out_len != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host(in, in_len, out, out_len, true); });
}

int speexhip_resampler_process_interleaved_float_device(SpeexHipResamplerState *st, const float *d_in,
                                                        uint32_t *in_len, float *d_out, uint32_t *out_len,
                                                        void *hip_stream) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_device(d_in, 0, in_len, d_out, 0, out_len, true,
                                   static_cast<hipStream_t>(hip_stream)); });
}

int speexhip_batch_process_interleaved_float_device(SpeexHipBatch *b, const float *d_in,
                                                    uint64_t in_stream_stride, uint32_t *in_len, float *d_out,
                                                    uint64_t out_stream_stride, uint32_t *out_len,
                                                    void *hip_stream) {
  if (b == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->process_device(d_in, in_stream_stride, in_len, d_out, out_stream_stride, out_len, true,
                                  static_cast<hipStream_t>(hip_stream)); });
}

int speexhip_resampler_process_chunks_int(SpeexHipResamplerState *st, uint32_t n_chunks,
                                          const int16_t *const *in, uint32_t *in_len, int16_t *out,
                                          uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host_chunks(n_chunks, reinterpret_cast<const void *const *>(in), in_len, out,
                                        out_len, false); });
}

int speexhip_resampler_process_chunks_float(SpeexHipResamplerState *st, uint32_t n_chunks,
                                            const float *const *in, uint32_t *in_len, float *out,
                                            uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_host_chunks(n_chunks, reinterpret_cast<const void *const *>(in), in_len, out,
                                        out_len, true); });
}

int speexhip_resampler_process_int(SpeexHipResamplerState *st, uint32_t channel_index, const int16_t *in,
                                   uint32_t *in_len, int16_t *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || (out == nullptr && *out_len != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_channel_host(channel_index, in, in_len, out, out_len, false); });
}

int speexhip_resampler_process_float(SpeexHipResamplerState *st, uint32_t channel_index, const float *in,
                                     uint32_t *in_len, float *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr || (out == nullptr && *out_len != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_channel_host(channel_index, in, in_len, out, out_len, true); });
}

void speexhip_resampler_set_input_stride(SpeexHipResamplerState *st, uint32_t stride) {
  st->batch->set_strides(stride, 0, true, false);
}
void speexhip_resampler_get_input_stride(SpeexHipResamplerState *st, uint32_t *stride) {
  *stride = st->batch->in_stride();
}
void speexhip_resampler_set_output_stride(SpeexHipResamplerState *st, uint32_t stride) {
  st->batch->set_strides(0, stride, false, true);
}
void speexhip_resampler_get_output_stride(SpeexHipResamplerState *st, uint32_t *stride) {
  *stride = st->batch->out_stride();
}

int speexhip_resampler_get_channel_position(SpeexHipResamplerState *st, uint32_t channel, int32_t *last_sample,
                                            uint32_t *samp_frac_num, uint32_t *magic_samples) {
  if (st == nullptr || channel >= st->batch->channels()) return SPEEXHIP_ERR_INVALID_ARG;
  const speexhip::StreamPos p = st->batch->channel_pos(0, channel);
  if (last_sample) *last_sample = p.last;
  if (samp_frac_num) *samp_frac_num = p.frac;
  if (magic_samples) *magic_samples = p.magic;
  return SPEEXHIP_ERR_SUCCESS;
}

// The three planner hooks: the plans plan_filter (filter_plans.h) gives a state of this ratio, quality and channel count,
// which are the ones build_tables uploads rows for, and for _launch_shape the choice choose_launch makes among them.
namespace {
struct HookPlans {
  speexhip::FilterSpec f, folded;
  speexhip::FilterPlans plans;
  int design(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels) {
    const int rc = speexhip::design_filter_frac(ratio_num, ratio_den, ratio_num, ratio_den, quality, &f, false);
    if (rc == SPEEXHIP_ERR_SUCCESS) (void)speexhip::plan_filter(f, channels, speexhip::lds_budget(), &plans, &folded);
    return rc;
  }
};
// out[0..5] of a period plan as _plan and _plan64 report it
void report_period(const speexhip::PeriodPlan &t, uint32_t code, uint32_t out[8]) {
  out[0] = code;
  out[1] = t.r;
  out[2] = t.lane_periods;
  out[3] = t.row_len;
  out[4] = static_cast<uint32_t>(t.window_bytes);
  out[5] = t.pad;
}
}  // namespace

int speexhip_debug_plan(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels, uint32_t out[8]) {
  if (out == nullptr || channels == 0) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    HookPlans h;
    const int rc = h.design(ratio_num, ratio_den, quality, channels);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    std::memset(out, 0, 8 * sizeof(uint32_t));
    const speexhip::PeriodPlan *p = h.plans.period;
    const speexhip::SlidePlan &sl = h.plans.slide;
    if (p[speexhip::kBase].usable) {
      report_period(p[speexhip::kBase], 2, out);
      out[6] = p[speexhip::kFine].usable;
      out[7] = p[speexhip::kW16].usable ? p[speexhip::kW16].lane_periods : 0;
    } else if (sl.usable) {
      out[0] = 3;
      out[1] = sl.p;
      out[3] = sl.row_len;
      out[4] = static_cast<uint32_t>(speexhip::slide_lds_bytes(sl, 2));
      out[7] = sl.p * sl.num;
    }
    return static_cast<int>(SPEEXHIP_ERR_SUCCESS);
  });
}
int speexhip_debug_launch_shape(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels, uint32_t streams,
                                uint32_t frames, int float_io, uint32_t out[10]) {
  if (out == nullptr || channels == 0 || streams == 0 || streams > 32) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    HookPlans h;
    const int rc = h.design(ratio_num, ratio_den, quality, channels);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    std::memset(out, 0, 10 * sizeof(uint32_t));
    // The launch of a first call of `frames` frames on every stream of a fresh state in a fast mode.  Where this models
    // less than the engine it says so, one line each ("The planner hooks"):
    const speexhip::FilterSpec &f = h.f;
    if (speexhip::is_double_kind(f)) return SPEEXHIP_ERR_SUCCESS;  // (the double kinds are not modelled: zeros)
    const speexhip::PeriodPlan &base = h.plans.period[speexhip::kBase];
    if (!base.usable) return SPEEXHIP_ERR_SUCCESS;
    if (float_io != 0 && !base.float_ok) return SPEEXHIP_ERR_SUCCESS;  // (a plan that stands for its int16 plan alone: float calls run the exact kernel; zeros)
    h.plans.period[speexhip::kFine].usable = false;  // (an r = 5 companion is not modelled: the rule sees has_fine = false and the shape is the chosen plan's alone)
    std::vector<speexhip::StreamDesc> descs(streams);
    for (auto &d : descs) {
      std::memset(&d, 0, sizeof(d));
      d.in_frames = frames;
      d.n_out = static_cast<uint32_t>(static_cast<uint64_t>(frames) * f.den / f.num);
    }
    const speexhip::LaunchChoice c =
        speexhip::choose_launch(h.plans, f, SPEEXHIP_MODE_FAST_FIXED, /*zero_mode=*/false, float_io != 0, /*float_seen=*/false,
                                /*w16_override=*/-1, descs.data(), streams);  // (no float call before, no W16 override)
    if (c.family != speexhip::KernelFamily::Period) return SPEEXHIP_ERR_SUCCESS;  // (cannot happen in the product build: a usable base plan serves every launch asked about here)
    const speexhip::PeriodPlan &t = h.plans.period[c.variant];
    out[0] = t.pp ? 1u : 0u;
    out[1] = t.r;
    out[2] = t.w16 ? 1u : 0u;
    out[3] = t.lane_periods;
    if (!speexhip::debug_period_shape(f, t, channels, descs.data(), streams, float_io != 0, out + 4)) return SPEEXHIP_ERR_BAD_STATE;
    return SPEEXHIP_ERR_SUCCESS;
  });
}
int speexhip_debug_plan64(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels, uint32_t out[8]) {
  if (out == nullptr || channels == 0) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    HookPlans h;
    const int rc = h.design(ratio_num, ratio_den, quality, channels);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    std::memset(out, 0, 8 * sizeof(uint32_t));
    const speexhip::PeriodPlan *p = h.plans.period;
    const speexhip::SlidePlan &sl = h.plans.slide64;
    if (p[speexhip::kPeriod64].usable) {
      report_period(p[speexhip::kPeriod64], 5, out);
      out[6] = p[speexhip::kPeriod64].l4;
      out[7] = p[speexhip::kPeriod64W16].usable ? p[speexhip::kPeriod64W16].lane_periods : 0;  // (round 5)
    } else if (sl.usable) {
      out[0] = 4;
      out[1] = sl.p;
      out[3] = sl.row_len;
      out[4] = static_cast<uint32_t>(speexhip::slide_lds_bytes(sl, 2) * (sl.p * h.f.den >= 4 ? 2 : 1));  // (image in doubles)
      out[5] = sl.row_stride;
      out[7] = sl.p * sl.num;
    }
    // phase-pair plans of filters of up to three channels with wide windows (reported for any quality below 9)
    if (!speexhip::is_double_kind(h.f) && p[speexhip::kPp].usable) {
      report_period(p[speexhip::kPp], 6, out);
      out[7] = p[speexhip::kPpW16].usable ? p[speexhip::kPpW16].lane_periods : 0;
    }
    return static_cast<int>(SPEEXHIP_ERR_SUCCESS);
  });
}
void speexhip_debug_fail_device_allocs(int n) { speexhip::debug_fail_device_allocs(n); }
uint64_t speexhip_release_cached_memory(void) {
  const uint64_t tables = speexhip::release_cached_tables();  // first: they return their buffers to the pool
  (void)tables;
  return speexhip::pool::release_idle();
}

void speexhip_resampler_get_rate(SpeexHipResamplerState *st, uint32_t *in_rate, uint32_t *out_rate) {
  *in_rate = st->batch->rates().in_rate;
  *out_rate = st->batch->rates().out_rate;
}

const char *speexhip_resampler_strerror(int err) {
  switch (err) {  // reference resample.c:1222-1239
    case SPEEXHIP_ERR_SUCCESS: return "Success.";
    case SPEEXHIP_ERR_ALLOC_FAILED: return "Memory allocation failed.";
    case SPEEXHIP_ERR_BAD_STATE: return "Bad resampler state.";
    case SPEEXHIP_ERR_INVALID_ARG: return "Invalid argument.";
    case SPEEXHIP_ERR_PTR_OVERLAP: return "Input and output buffers overlap.";
    case SPEEXHIP_ERR_DEVICE: return speexhip::last_device_error();
    case SPEEXHIP_ERR_NO_BLOCK: return "No pinned result block available (state untouched).";
    default: return "Unknown error. Bad error code or strange version mismatch.";
  }
}

int speexhip_resampler_peek(SpeexHipResamplerState *st, uint32_t in_len, uint32_t out_capacity, int float_entry,
                            uint32_t *consumed, uint32_t *produced) {
  if (st == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  const speexhip::CallPlan plan = st->batch->peek(0, in_len, out_capacity, float_entry != 0);
  if (consumed) *consumed = plan.consumed;
  if (produced) *produced = plan.produced;
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_resampler_set_mode(SpeexHipResamplerState *st, int mode) {
  return guarded([&] { return st ? st->batch->set_mode(mode) : SPEEXHIP_ERR_INVALID_ARG; });
}

int speexhip_resampler_release_stream(SpeexHipResamplerState *st) {
  return guarded([&] { return st ? st->batch->release_stream() : SPEEXHIP_ERR_INVALID_ARG; });
}

int speexhip_resampler_get_info(SpeexHipResamplerState *st, SpeexHipInfo *info) {
  if (st == nullptr || info == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  st->batch->info(0, info);
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_resampler_get_info2(SpeexHipResamplerState *st, SpeexHipInfo *info, uint32_t struct_size) {
  if (st == nullptr || info == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  SpeexHipInfo full;
  st->batch->info(0, &full);
  std::memcpy(info, &full, struct_size < sizeof(full) ? struct_size : sizeof(full));
  return SPEEXHIP_ERR_SUCCESS;
}

namespace {
int process_many(uint32_t n, SpeexHipResamplerState *const *st, const void *const *in, uint32_t *in_len,
                 void *const *out, uint32_t *out_len, int *codes, bool float_io) {
  if (n == 0) return SPEEXHIP_ERR_SUCCESS;
  if (st == nullptr || in == nullptr || in_len == nullptr || out == nullptr || out_len == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    std::vector<Batch *> b(n);
    for (uint32_t i = 0; i < n; i++) b[i] = st[i] != nullptr ? st[i]->batch : nullptr;
    return Batch::process_host_many(n, b.data(), in, in_len, out, out_len, float_io, codes);
  });
}
}  // namespace

int speexhip_resampler_process_many_int(uint32_t n, SpeexHipResamplerState *const *st, const int16_t *const *in,
                                        uint32_t *in_len, int16_t *const *out, uint32_t *out_len, int *codes) {
  return process_many(n, st, reinterpret_cast<const void *const *>(in), in_len, reinterpret_cast<void *const *>(out),
                      out_len, codes, false);
}
int speexhip_resampler_process_many_float(uint32_t n, SpeexHipResamplerState *const *st, const float *const *in,
                                          uint32_t *in_len, float *const *out, uint32_t *out_len, int *codes) {
  return process_many(n, st, reinterpret_cast<const void *const *>(in), in_len, reinterpret_cast<void *const *>(out),
                      out_len, codes, true);
}

int speexhip_resampler_get_history(SpeexHipResamplerState *st, float *dst) {
  if (st == nullptr || dst == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->history(0, dst); });
}

SpeexHipBatch *speexhip_batch_init(uint32_t n_streams, uint32_t nb_channels, uint32_t in_rate,
                                   uint32_t out_rate, int quality, int *err) {
  return speexhip_batch_init_on(-1, n_streams, nb_channels, in_rate, out_rate, quality, err);
}

SpeexHipBatch *speexhip_batch_init_on(int device, uint32_t n_streams, uint32_t nb_channels, uint32_t in_rate,
                                      uint32_t out_rate, int quality, int *err) {
  Batch *b = nullptr;
  int code = SPEEXHIP_ERR_SUCCESS;
  const int rc = guarded([&] {
    b = Batch::create(n_streams, nb_channels, in_rate, out_rate, quality, &code, device < 0 ? -1 : device);
    return code;
  });
  if (err) *err = rc;
  if (b == nullptr) return nullptr;
  SpeexHipBatch *h = new (std::nothrow) SpeexHipBatch_{b};
  if (h == nullptr) {
    delete b;
    if (err) *err = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  return h;
}

void speexhip_batch_destroy(SpeexHipBatch *b) {
  if (b == nullptr) return;
  delete b->batch;
  delete b;
}

int speexhip_batch_set_mode(SpeexHipBatch *b, int mode) {
  return guarded([&] { return b ? b->batch->set_mode(mode) : SPEEXHIP_ERR_INVALID_ARG; });
}

int speexhip_batch_release_stream(SpeexHipBatch *b) {
  return guarded([&] { return b ? b->batch->release_stream() : SPEEXHIP_ERR_INVALID_ARG; });
}

int speexhip_batch_get_info(SpeexHipBatch *b, uint32_t stream, SpeexHipInfo *info) {
  if (b == nullptr || info == nullptr || stream >= b->batch->n_streams()) return SPEEXHIP_ERR_INVALID_ARG;
  b->batch->info(stream, info);
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_batch_process_interleaved_int_device(SpeexHipBatch *b, const int16_t *d_in,
                                                  uint64_t in_stream_stride, uint32_t *in_len,
                                                  int16_t *d_out, uint64_t out_stream_stride,
                                                  uint32_t *out_len, void *hip_stream) {
  if (b == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->process_device(d_in, in_stream_stride, in_len, d_out, out_stream_stride, out_len, false,
                                  static_cast<hipStream_t>(hip_stream)); });
}

int speexhip_resampler_process_planar_int(SpeexHipResamplerState *st, const int16_t *const *in, uint32_t *in_len,
                                          int16_t *const *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_planar_host(reinterpret_cast<const void *const *>(in), in_len,
                                        reinterpret_cast<void *const *>(out), out_len, false); });
}
int speexhip_resampler_process_planar_float(SpeexHipResamplerState *st, const float *const *in, uint32_t *in_len,
                                            float *const *out, uint32_t *out_len) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_planar_host(reinterpret_cast<const void *const *>(in), in_len,
                                        reinterpret_cast<void *const *>(out), out_len, true); });
}
int speexhip_resampler_process_planar_int_device(SpeexHipResamplerState *st, const int16_t *d_in, uint64_t in_plane_stride,
                                                 uint32_t *in_len, int16_t *d_out, uint64_t out_plane_stride,
                                                 uint32_t *out_len, void *hip_stream) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_planar_device(d_in, 0, in_plane_stride, in_len, d_out, 0, out_plane_stride,
                                        out_len, false, static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_resampler_process_planar_float_device(SpeexHipResamplerState *st, const float *d_in, uint64_t in_plane_stride,
                                                   uint32_t *in_len, float *d_out, uint64_t out_plane_stride,
                                                   uint32_t *out_len, void *hip_stream) {
  if (st == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_planar_device(d_in, 0, in_plane_stride, in_len, d_out, 0, out_plane_stride,
                                        out_len, true, static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_batch_process_planar_int_device(SpeexHipBatch *b, const int16_t *d_in, uint64_t in_stream_stride,
                                             uint64_t in_plane_stride, uint32_t *in_len, int16_t *d_out,
                                             uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len,
                                             void *hip_stream) {
  if (b == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->process_planar_device(d_in, in_stream_stride, in_plane_stride, in_len, d_out,
                                       out_stream_stride, out_plane_stride, out_len, false,
                                       static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_batch_process_planar_float_device(SpeexHipBatch *b, const float *d_in, uint64_t in_stream_stride,
                                               uint64_t in_plane_stride, uint32_t *in_len, float *d_out,
                                               uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len,
                                               void *hip_stream) {
  if (b == nullptr || in_len == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->process_planar_device(d_in, in_stream_stride, in_plane_stride, in_len, d_out,
                                       out_stream_stride, out_plane_stride, out_len, true,
                                       static_cast<hipStream_t>(hip_stream)); });
}

uint32_t speexhip_sample_bytes(int fmt) { return speexhip::sample_bytes(fmt); }

namespace {
// the formatted and mixed calls' sides; a formatted call's sides hold the state's channel count and no matrix
speexhip::CallSide side(int fmt, uint32_t channels, const float *mix, const void *base, uint64_t stride = 0) {
  return speexhip::CallSide{fmt, channels, mix, const_cast<void *>(base), stride};
}
bool fmt_args_ok(const void *handle, const uint32_t *in_len, const uint32_t *out_len, const void *out, int in_fmt, int out_fmt) {
  return handle != nullptr && in_len != nullptr && out_len != nullptr && out != nullptr && speexhip::sample_bytes(in_fmt) != 0 &&
         speexhip::sample_bytes(out_fmt) != 0;
}
}  // namespace

int speexhip_resampler_process_interleaved_fmt(SpeexHipResamplerState *st, int in_fmt, const void *in, uint32_t *in_len,
                                               int out_fmt, void *out, uint32_t *out_len) {
  if (!fmt_args_ok(st, in_len, out_len, out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    const uint32_t ch = st->batch->channels();
    return st->batch->process_sides_host(side(in_fmt, ch, nullptr, in), in_len, side(out_fmt, ch, nullptr, out), out_len);
  });
}
int speexhip_resampler_process_interleaved_fmt_device(SpeexHipResamplerState *st, int in_fmt, const void *d_in,
                                                      uint32_t *in_len, int out_fmt, void *d_out, uint32_t *out_len,
                                                      void *hip_stream) {
  if (!fmt_args_ok(st, in_len, out_len, d_out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    const uint32_t ch = st->batch->channels();
    return st->batch->process_sides_device(side(in_fmt, ch, nullptr, d_in), in_len, side(out_fmt, ch, nullptr, d_out), out_len,
                                           static_cast<hipStream_t>(hip_stream));
  });
}
int speexhip_batch_process_interleaved_fmt_device(SpeexHipBatch *b, int in_fmt, const void *d_in, uint64_t in_stream_stride,
                                                  uint32_t *in_len, int out_fmt, void *d_out, uint64_t out_stream_stride,
                                                  uint32_t *out_len, void *hip_stream) {
  if (!fmt_args_ok(b, in_len, out_len, d_out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    const uint32_t ch = b->batch->channels();
    return b->batch->process_sides_device(side(in_fmt, ch, nullptr, d_in, in_stream_stride), in_len,
                                          side(out_fmt, ch, nullptr, d_out, out_stream_stride), out_len,
                                          static_cast<hipStream_t>(hip_stream));
  });
}

int speexhip_resampler_process_interleaved_mix(SpeexHipResamplerState *st, int in_fmt, uint32_t in_channels,
                                               const float *in_mix, const void *in, uint32_t *in_len, int out_fmt,
                                               uint32_t out_channels, const float *out_mix, void *out, uint32_t *out_len) {
  if (!fmt_args_ok(st, in_len, out_len, out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_sides_host(side(in_fmt, in_channels, in_mix, in), in_len,
                                                            side(out_fmt, out_channels, out_mix, out), out_len); });
}
int speexhip_resampler_process_interleaved_mix_device(SpeexHipResamplerState *st, int in_fmt, uint32_t in_channels,
                                                      const float *in_mix, const void *d_in, uint32_t *in_len, int out_fmt,
                                                      uint32_t out_channels, const float *out_mix, void *d_out,
                                                      uint32_t *out_len, void *hip_stream) {
  if (!fmt_args_ok(st, in_len, out_len, d_out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_sides_device(side(in_fmt, in_channels, in_mix, d_in), in_len,
                                                              side(out_fmt, out_channels, out_mix, d_out), out_len,
                                                              static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_batch_process_interleaved_mix_device(SpeexHipBatch *b, int in_fmt, uint32_t in_channels, const float *in_mix,
                                                  const void *d_in, uint64_t in_stream_stride, uint32_t *in_len, int out_fmt,
                                                  uint32_t out_channels, const float *out_mix, void *d_out,
                                                  uint64_t out_stream_stride, uint32_t *out_len, void *hip_stream) {
  if (!fmt_args_ok(b, in_len, out_len, d_out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return b->batch->process_sides_device(side(in_fmt, in_channels, in_mix, d_in, in_stream_stride), in_len,
                                                             side(out_fmt, out_channels, out_mix, d_out, out_stream_stride),
                                                             out_len, static_cast<hipStream_t>(hip_stream)); });
}

namespace {
// a caller's SpeexHipSide as the engine's CallSide; false: not a side this version can read
bool side_of(const SpeexHipSide *s, bool host, speexhip::CallSide *side) {
  if (s == nullptr || s->struct_size < sizeof(SpeexHipSide)) return false;
  if (s->layout != SPEEXHIP_LAYOUT_INTERLEAVED && s->layout != SPEEXHIP_LAYOUT_PLANAR) return false;
  *side = speexhip::CallSide{s->fmt, s->channels, s->mix, s->data, s->stream_stride};
  side->layout = s->layout;
  side->plane_stride = s->plane_stride;
  side->planes = host && s->layout == SPEEXHIP_LAYOUT_PLANAR ? s->planes : nullptr;
  for (uint32_t c = 0; side->planes != nullptr && c < s->channels; c++)
    if (side->planes[c] == nullptr) return false;
  return true;
}
}  // namespace

int speexhip_resampler_process_sides(SpeexHipResamplerState *st, const SpeexHipSide *in, uint32_t *in_len,
                                     const SpeexHipSide *out, uint32_t *out_len) {
  speexhip::CallSide a, b;
  if (st == nullptr || in_len == nullptr || out_len == nullptr || !side_of(in, true, &a) || !side_of(out, true, &b) ||
      (b.base == nullptr && b.planes == nullptr))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_sides_host(a, in_len, b, out_len); });
}
int speexhip_resampler_process_sides_device(SpeexHipResamplerState *st, const SpeexHipSide *in, uint32_t *in_len,
                                            const SpeexHipSide *out, uint32_t *out_len, void *hip_stream) {
  speexhip::CallSide a, b;
  if (st == nullptr || in_len == nullptr || out_len == nullptr || !side_of(in, false, &a) || !side_of(out, false, &b) ||
      b.base == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  a.stride = b.stride = 0;
  return guarded([&] { return st->batch->process_sides_device(a, in_len, b, out_len, static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_batch_process_sides_device(SpeexHipBatch *bt, const SpeexHipSide *in, uint32_t *in_len, const SpeexHipSide *out,
                                        uint32_t *out_len, void *hip_stream) {
  speexhip::CallSide a, b;
  if (bt == nullptr || in_len == nullptr || out_len == nullptr || !side_of(in, false, &a) || !side_of(out, false, &b) ||
      b.base == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return bt->batch->process_sides_device(a, in_len, b, out_len, static_cast<hipStream_t>(hip_stream)); });
}

// ---- chunk coalescing, formatted ------------------------------------------------------------------------------------------
int speexhip_resampler_process_chunks_sides(SpeexHipResamplerState *st, uint32_t n_chunks, const SpeexHipSide *in,
                                            const void *const *in_data, uint32_t *in_len, const SpeexHipSide *out,
                                            uint32_t *out_len) {
  speexhip::CallSide a, b;
  if (st == nullptr || in_len == nullptr || out_len == nullptr || in == nullptr || in->struct_size < sizeof(SpeexHipSide))
    return SPEEXHIP_ERR_INVALID_ARG;
  SpeexHipSide every = *in;  // (where a chunk lies is in_data's to say)
  every.data = nullptr;
  every.planes = nullptr;
  if (!side_of(&every, true, &a) || !side_of(out, true, &b) || (b.base == nullptr && b.planes == nullptr))
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return st->batch->process_sides_host_chunks(n_chunks, a, in_data, in_len, b, out_len); });
}
int speexhip_resampler_process_chunks_fmt(SpeexHipResamplerState *st, uint32_t n_chunks, int in_fmt, const void *const *in,
                                          uint32_t *in_len, int out_fmt, void *out, uint32_t *out_len) {
  if (!fmt_args_ok(st, in_len, out_len, out, in_fmt, out_fmt)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    const uint32_t ch = st->batch->channels();
    return st->batch->process_sides_host_chunks(n_chunks, side(in_fmt, ch, nullptr, nullptr), in, in_len,
                                                side(out_fmt, ch, nullptr, out), out_len);
  });
}
void speexhip_debug_chunk_counters(uint64_t out[4]) {
  if (out != nullptr) speexhip::chunk_counters(out);
}

// ---- many states, formatted ---------------------------------------------------------------------------------------------
int speexhip_resampler_process_many_sides(uint32_t n, SpeexHipResamplerState *const *st, const SpeexHipSide *in,
                                          uint32_t *in_len, const SpeexHipSide *out, uint32_t *out_len, int *codes) {
  if (n == 0) return SPEEXHIP_ERR_SUCCESS;
  if (st == nullptr || in == nullptr || in_len == nullptr || out == nullptr || out_len == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    std::vector<Batch *> b(n);
    std::vector<speexhip::CallSide> a(n), o(n);
    std::vector<uint8_t> bad(n, 0);
    for (uint32_t i = 0; i < n; i++) {
      b[i] = st[i] != nullptr ? st[i]->batch : nullptr;
      // (each entry's struct_size stands at the head of ITS side: an array of this version's structs)
      if (!side_of(&in[i], true, &a[i]) || !side_of(&out[i], true, &o[i])) bad[i] = 1;
    }
    return Batch::process_host_many_sides(n, b.data(), a.data(), in_len, o.data(), out_len, bad.data(), codes);
  });
}
int speexhip_resampler_process_many_fmt(uint32_t n, SpeexHipResamplerState *const *st, const int *in_fmt,
                                        const void *const *in, uint32_t *in_len, const int *out_fmt, void *const *out,
                                        uint32_t *out_len, int *codes) {
  if (n == 0) return SPEEXHIP_ERR_SUCCESS;
  if (st == nullptr || in_fmt == nullptr || in == nullptr || in_len == nullptr || out_fmt == nullptr || out == nullptr ||
      out_len == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    std::vector<Batch *> b(n);
    std::vector<speexhip::CallSide> a(n), o(n);
    for (uint32_t i = 0; i < n; i++) {
      b[i] = st[i] != nullptr ? st[i]->batch : nullptr;
      const uint32_t ch = b[i] != nullptr ? b[i]->channels() : 0;
      a[i] = side(in_fmt[i], ch, nullptr, in[i]);
      o[i] = side(out_fmt[i], ch, nullptr, out[i]);
    }
    return Batch::process_host_many_sides(n, b.data(), a.data(), in_len, o.data(), out_len, nullptr, codes);
  });
}
void speexhip_debug_many_counters(uint64_t out[4]) {
  if (out != nullptr) speexhip::many_counters(out);
}

int speexhip_resampler_set_dither(SpeexHipResamplerState *st, int kind, uint64_t seed, uint64_t position) {
  return guarded([&] { return st ? st->batch->set_dither(kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_resampler_get_dither(SpeexHipResamplerState *st, int *kind, uint64_t *seed, uint64_t *position) {
  return guarded([&] { return st ? st->batch->get_dither(0, kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_set_dither(SpeexHipBatch *b, int kind, uint64_t seed, uint64_t position) {
  return guarded([&] { return b ? b->batch->set_dither(kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_get_dither(SpeexHipBatch *b, uint32_t stream, int *kind, uint64_t *seed, uint64_t *position) {
  return guarded([&] { return b ? b->batch->get_dither(stream, kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_debug_dither(int kind, uint64_t seed, uint64_t first_index, uint32_t n, double *d) {
  if (!speexhip::dither::known_kind(kind) || (d == nullptr && n != 0)) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++) d[i] = speexhip::dither::noise(kind, seed, first_index + i);
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_resampler_set_meter(SpeexHipResamplerState *st, int on) {
  return guarded([&] { return st ? st->batch->set_meter(on) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_resampler_get_meter(SpeexHipResamplerState *st, SpeexHipMeter *m, int reset) {
  return guarded([&] { return st ? st->batch->get_meter(0, m, reset != 0) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_set_meter(SpeexHipBatch *b, int on) {
  return guarded([&] { return b ? b->batch->set_meter(on) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_get_meter(SpeexHipBatch *b, uint32_t stream, SpeexHipMeter *m, int reset) {
  return guarded([&] { return b ? b->batch->get_meter(stream, m, reset != 0) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_debug_meter(int fmt, const float *y, const double *d, uint32_t n, SpeexHipMeter *m) {
  namespace mt = speexhip::meter;
  if (m == nullptr || m->struct_size < sizeof(SpeexHipMeter) || speexhip::sample_bytes(fmt) == 0 || (y == nullptr && n != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  if (d != nullptr && !speexhip::dithered_fmt(fmt)) return SPEEXHIP_ERR_INVALID_ARG;  // (the float formats are not dithered)
  uint64_t hi = 0, lo = 0, nan = 0;
  uint32_t peak = 0;
  (void)speexhip::fmtdev::with_format(fmt, [&](auto format) -> hipError_t {
    for (uint32_t i = 0; i < n; i++) {
      mt::Lane one;  // (a lane's counts are 32 bits: folded sample by sample here)
      mt::judge<decltype(format)::value>(one, y[i], d != nullptr ? d[i] : 0.0);
      hi += one.hi, lo += one.lo, nan += one.nan;
      peak = one.peak > peak ? one.peak : peak;
    }
    return hipSuccess;
  });
  SpeexHipMeter now;
  std::memset(&now, 0, sizeof(now));
  now.struct_size = m->struct_size;
  now.on = m->on;
  now.samples = n;
  now.clipped_high = hi, now.clipped_low = lo, now.nan = nan;
  std::memcpy(&now.peak, &peak, sizeof(peak));
  std::memcpy(m, &now, sizeof(now));
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_resampler_set_gain(SpeexHipResamplerState *st, float gain, uint32_t ramp_frames) {
  return guarded([&] { return st ? st->batch->set_gain(0, gain, ramp_frames) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_resampler_get_gain(SpeexHipResamplerState *st, float *current, float *target, uint32_t *remaining) {
  return guarded([&] { return st ? st->batch->get_gain(0, current, target, remaining) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_set_gain(SpeexHipBatch *b, uint32_t stream, float gain, uint32_t ramp_frames) {
  return guarded([&] { return b ? b->batch->set_gain(stream, gain, ramp_frames) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_get_gain(SpeexHipBatch *b, uint32_t stream, float *current, float *target, uint32_t *remaining) {
  return guarded([&] { return b ? b->batch->get_gain(stream, current, target, remaining) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_debug_gain(float from, float to, uint32_t total, uint64_t first, uint32_t n, float *g) {
  if (g == nullptr && n != 0) return SPEEXHIP_ERR_INVALID_ARG;
  const double step = speexhip::gain::step_of(from, to, total);
  for (uint32_t i = 0; i < n; i++) g[i] = speexhip::gain::at(step, from, to, total, first + i);
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_batch_set_buses(SpeexHipBatch *b, uint32_t n_buses, const float *weights) {
  return guarded([&] { return b ? b->batch->set_buses(n_buses, weights) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_get_buses(SpeexHipBatch *b, uint32_t *n_buses, float *weights) {
  return guarded([&] { return b ? b->batch->get_buses(n_buses, weights) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_process_bus_device(SpeexHipBatch *bt, const SpeexHipSide *in, uint32_t *in_len, const SpeexHipSide *out,
                                      uint32_t *out_len, uint32_t *bus_frames, void *hip_stream) {
  speexhip::CallSide a, b;
  if (bt == nullptr || in_len == nullptr || out_len == nullptr || bus_frames == nullptr || !side_of(in, false, &a) ||
      !side_of(out, false, &b) || b.base == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] { return bt->batch->process_bus_device(a, in_len, b, out_len, bus_frames, static_cast<hipStream_t>(hip_stream)); });
}
int speexhip_batch_get_bus_meter(SpeexHipBatch *b, uint32_t bus, SpeexHipMeter *m, int reset) {
  return guarded([&] { return b ? b->batch->get_bus_meter(bus, m, reset != 0) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_batch_get_bus_position(SpeexHipBatch *b, uint64_t *position) {
  if (b == nullptr || position == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  *position = b->batch->bus_position();
  return SPEEXHIP_ERR_SUCCESS;
}
int speexhip_debug_bus(uint32_t n_streams, uint32_t n_buses, const float *weights, const float *y, uint32_t n, float *z) {
  if (n_streams == 0 || n_buses == 0 || weights == nullptr || ((y == nullptr || z == nullptr) && n != 0)) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t j = 0; j < n_buses; j++)
    for (uint32_t i = 0; i < n; i++)
      z[static_cast<size_t>(j) * n + i] = speexhip::bus::sum(weights + static_cast<size_t>(j) * n_streams, y + i, n, n_streams);
  return SPEEXHIP_ERR_SUCCESS;
}

// ---- the mixer ------------------------------------------------------------------------------------------------------------
SpeexHipMixer *speexhip_mixer_init(uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err) {
  return speexhip_mixer_init_on(-1, n_legs, n_buses, channels, err);
}
SpeexHipMixer *speexhip_mixer_init_on(int device, uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err) {
  speexhip::Mixer *m = nullptr;
  int code = SPEEXHIP_ERR_SUCCESS;
  const int rc = guarded([&] {
    m = speexhip::Mixer::create(n_legs, n_buses, channels, &code, device);
    return code;
  });
  if (err != nullptr) *err = rc;
  if (m == nullptr) return nullptr;
  SpeexHipMixer *h = new (std::nothrow) SpeexHipMixer_{m};
  if (h == nullptr) {
    delete m;
    if (err != nullptr) *err = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  return h;
}
void speexhip_mixer_destroy(SpeexHipMixer *m) {
  if (m == nullptr) return;
  (void)guarded([&] {
    delete m->mixer;
    return SPEEXHIP_ERR_SUCCESS;
  });
  delete m;
}
int speexhip_mixer_set_weights(SpeexHipMixer *m, const float *weights) {
  return guarded([&] { return m ? m->mixer->set_weights(weights) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_get_weights(SpeexHipMixer *m, float *weights) {
  return guarded([&] { return m ? m->mixer->get_weights(weights) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_set_dither(SpeexHipMixer *m, int kind, uint64_t seed, uint64_t position) {
  return guarded([&] { return m ? m->mixer->set_dither(kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_get_dither(SpeexHipMixer *m, int *kind, uint64_t *seed, uint64_t *position) {
  return guarded([&] { return m ? m->mixer->get_dither(kind, seed, position) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_set_meter(SpeexHipMixer *m, int on) {
  return guarded([&] { return m ? m->mixer->set_meter(on) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_get_bus_meter(SpeexHipMixer *m, uint32_t bus, SpeexHipMeter *meter, int reset) {
  return guarded([&] { return m ? m->mixer->get_bus_meter(bus, meter, reset != 0) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_process(SpeexHipMixer *m, SpeexHipResamplerState *const *legs, const SpeexHipSide *in, uint32_t *in_len,
                           uint32_t *out_len, const SpeexHipSide *out, uint32_t *bus_frames, int *codes) {
  speexhip::CallSide o;
  if (m == nullptr || legs == nullptr || in == nullptr || in_len == nullptr || out_len == nullptr || out == nullptr ||
      bus_frames == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  if (out->planes != nullptr || !side_of(out, false, &o)) return SPEEXHIP_ERR_INVALID_ARG;
  return guarded([&] {
    const uint32_t n = m->mixer->n_legs();
    std::vector<Batch *> b(n);
    std::vector<speexhip::CallSide> a(n);
    std::vector<uint8_t> bad(n, 0);
    for (uint32_t i = 0; i < n; i++) {
      b[i] = legs[i] != nullptr ? legs[i]->batch : nullptr;
      // (each leg's struct_size stands at the head of ITS side; stream_stride and planes are not read)
      if (b[i] != nullptr && !side_of(&in[i], false, &a[i])) bad[i] = 1;
      a[i].stride = 0;
    }
    return m->mixer->process(b.data(), a.data(), bad.data(), in_len, out_len, o, bus_frames, codes);
  });
}
void speexhip_debug_mixer_counters(uint64_t out[6]) {
  if (out != nullptr) speexhip::mixer_counters(out);
}
int speexhip_mixer_set_levels(SpeexHipMixer *m, int on) {
  return guarded([&] { return m ? m->mixer->set_levels(on) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_mixer_get_levels(SpeexHipMixer *m, uint32_t first_slot, uint32_t count, void *levels, uint32_t struct_size) {
  return guarded([&] { return m ? m->mixer->get_levels(first_slot, count, levels, struct_size) : SPEEXHIP_ERR_INVALID_ARG; });
}
int speexhip_debug_levels(const float *y, uint32_t n, SpeexHipLevel *l) {
  if (l == nullptr || (y == nullptr && n != 0)) return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++) {
    speexhip::levels::Lane one;  // (a lane's energy chain is exact up to 2^23 samples: folded sample by sample here)
    speexhip::levels::add(one, y[i]);
    speexhip::levels::fold(*l, one);
  }
  l->samples += n;
  return SPEEXHIP_ERR_SUCCESS;
}
uint64_t speexhip_debug_mixer_level_launches(void) { return speexhip::mixer_level_launches(); }

int speexhip_debug_g711_decode(int fmt, const uint8_t *codes, uint32_t n, float *x) {
  if ((fmt != SPEEXHIP_FMT_ULAW && fmt != SPEEXHIP_FMT_ALAW) || ((codes == nullptr || x == nullptr) && n != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++)
    x[i] = static_cast<float>(fmt == SPEEXHIP_FMT_ULAW ? speexhip::g711::ulaw_decode(codes[i]) : speexhip::g711::alaw_decode(codes[i]));
  return SPEEXHIP_ERR_SUCCESS;
}
int speexhip_debug_g711_encode(int fmt, const float *y, const double *d, uint32_t n, uint8_t *codes) {
  if ((fmt != SPEEXHIP_FMT_ULAW && fmt != SPEEXHIP_FMT_ALAW) || ((y == nullptr || codes == nullptr) && n != 0))
    return SPEEXHIP_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++) {
    const int32_t q = d != nullptr ? speexhip::g711::s16_of_dither(y[i], d[i]) : speexhip::g711::s16_of(y[i]);
    codes[i] = static_cast<uint8_t>(fmt == SPEEXHIP_FMT_ULAW ? speexhip::g711::ulaw_encode(q) : speexhip::g711::alaw_encode(q));
  }
  return SPEEXHIP_ERR_SUCCESS;
}

namespace {
// one sample's storage bits at byte i * bytes of a buffer of a format of halfbe.h (any address: byte by byte)
uint32_t sample_at(const uint8_t *p, uint32_t bytes) {
  uint32_t raw = 0;
  for (uint32_t k = 0; k < bytes; k++) raw |= static_cast<uint32_t>(p[k]) << (8 * k);
  return raw;
}
bool halfbe_format(int fmt) {
  return fmt == SPEEXHIP_FMT_F16N || fmt == SPEEXHIP_FMT_BF16N || fmt == SPEEXHIP_FMT_S16BE || fmt == SPEEXHIP_FMT_S24BE ||
         fmt == SPEEXHIP_FMT_S32BE;
}
}  // namespace

int speexhip_debug_format_decode(int fmt, const void *storage, uint32_t n, float *x) {
  namespace hb = speexhip::halfbe;
  if (!halfbe_format(fmt) || ((storage == nullptr || x == nullptr) && n != 0)) return SPEEXHIP_ERR_INVALID_ARG;
  const uint32_t bytes = speexhip::sample_bytes(fmt);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t raw = sample_at(static_cast<const uint8_t *>(storage) + static_cast<size_t>(i) * bytes, bytes);
    x[i] = fmt == SPEEXHIP_FMT_F16N    ? hb::f16n_decode(raw)
           : fmt == SPEEXHIP_FMT_BF16N ? hb::bf16n_decode(raw)
           : fmt == SPEEXHIP_FMT_S16BE ? hb::pcm_decode(16, hb::swap16(raw))
           : fmt == SPEEXHIP_FMT_S24BE ? hb::pcm_decode(24, hb::swap24(raw))
                                       : hb::pcm_decode(32, hb::swap32(raw));
  }
  return SPEEXHIP_ERR_SUCCESS;
}
int speexhip_debug_format_encode(int fmt, const float *y, const double *d, uint32_t n, void *storage) {
  namespace hb = speexhip::halfbe;
  if (!halfbe_format(fmt) || ((y == nullptr || storage == nullptr) && n != 0)) return SPEEXHIP_ERR_INVALID_ARG;
  if (d != nullptr && !speexhip::dithered_fmt(fmt)) return SPEEXHIP_ERR_INVALID_ARG;  // (the half formats are not dithered)
  const uint32_t bytes = speexhip::sample_bytes(fmt), bits = 8 * bytes;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t raw;
    if (fmt == SPEEXHIP_FMT_F16N) {
      raw = hb::f16n_encode(y[i]);
    } else if (fmt == SPEEXHIP_FMT_BF16N) {
      raw = hb::bf16n_encode(y[i]);
    } else {
      const uint32_t q = static_cast<uint32_t>(d != nullptr ? hb::pcm_of_dither(bits, y[i], d[i]) : hb::pcm_of(bits, y[i]));
      raw = bits == 16 ? hb::swap16(q) : bits == 24 ? hb::swap24(q) : hb::swap32(q);
    }
    uint8_t *p = static_cast<uint8_t *>(storage) + static_cast<size_t>(i) * bytes;
    for (uint32_t k = 0; k < bytes; k++) p[k] = static_cast<uint8_t>(raw >> (8 * k));
  }
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_design_filter(uint32_t in_rate, uint32_t out_rate, int quality, SpeexHipInfo *info,
                           float *table, uint32_t table_capacity) {
  if (in_rate == 0 || out_rate == 0) return SPEEXHIP_ERR_INVALID_ARG;
  return speexhip_design_filter_frac(in_rate, out_rate, in_rate, out_rate, quality, info, table, table_capacity);
}

int speexhip_design_filter_frac(uint32_t ratio_num, uint32_t ratio_den, uint32_t in_rate, uint32_t out_rate,
                                int quality, SpeexHipInfo *info, float *table, uint32_t table_capacity) {
  speexhip::FilterSpec f;
  const int rc = guarded([&] {
    return speexhip::design_filter_frac(ratio_num, ratio_den, in_rate, out_rate, quality, &f, table != nullptr);
  });
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  if (info != nullptr) {
    std::memset(info, 0, sizeof(*info));
    info->in_rate = f.in_rate;
    info->out_rate = f.out_rate;
    info->num_rate = f.num;
    info->den_rate = f.den;
    info->quality = f.quality;
    info->filt_len = f.taps;
    info->oversample = f.oversample;
    info->sinc_table_length = f.table_len;
    info->kernel = f.kind;
    info->device = -1;
  }
  if (table != nullptr) {
    const uint32_t n = f.table_len < table_capacity ? f.table_len : table_capacity;
    std::memcpy(table, f.table.data(), sizeof(float) * n);
  }
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_plan_call(uint32_t num_rate, uint32_t den_rate, uint32_t in_len, uint32_t out_cap,
                       int32_t *last_sample, uint32_t *samp_frac_num, uint32_t *consumed,
                       uint32_t *produced) {
  if (num_rate == 0 || den_rate == 0 || last_sample == nullptr || samp_frac_num == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  speexhip::StreamPos p;
  p.last = *last_sample;
  p.frac = *samp_frac_num;
  const speexhip::CallPlan plan = speexhip::plan_call(num_rate, den_rate, in_len, out_cap, p);
  *last_sample = plan.end.last;
  *samp_frac_num = plan.end.frac;
  if (consumed) *consumed = plan.consumed;
  if (produced) *produced = plan.produced;
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_plan_call_ex(uint32_t num_rate, uint32_t den_rate, uint32_t in_len, uint32_t out_cap,
                          int float_entry, uint32_t block_in, int32_t *last_sample, uint32_t *samp_frac_num,
                          uint32_t *magic_samples, uint32_t *consumed, uint32_t *produced) {
  if (num_rate == 0 || den_rate == 0 || block_in == 0 || last_sample == nullptr ||
      samp_frac_num == nullptr || magic_samples == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  speexhip::StreamPos p;
  p.last = *last_sample;
  p.frac = *samp_frac_num;
  p.magic = *magic_samples;
  speexhip::EntryRules rules;
  rules.block_in = block_in;
  rules.float_entry = float_entry != 0;
  const speexhip::CallPlan plan = speexhip::plan_call(num_rate, den_rate, in_len, out_cap, p, rules);
  *last_sample = plan.end.last;
  *samp_frac_num = plan.end.frac;
  *magic_samples = plan.end.magic;
  if (consumed) *consumed = plan.consumed;
  if (produced) *produced = plan.produced;
  return SPEEXHIP_ERR_SUCCESS;
}

int speexhip_plan_filter_change(uint32_t old_filt_len, uint32_t new_filt_len, uint32_t magic, int64_t *shift,
                                uint32_t *new_magic, int32_t *last_delta, uint32_t *phase, uint32_t old_den,
                                uint32_t new_den) {
  if (old_filt_len == 0 || new_filt_len == 0 || shift == nullptr || new_magic == nullptr ||
      last_delta == nullptr)
    return SPEEXHIP_ERR_INVALID_ARG;
  if (phase != nullptr) {
    if (old_den == 0 || new_den == 0) return SPEEXHIP_ERR_INVALID_ARG;
    if (!speexhip::scale_phase(phase, new_den, old_den)) return SPEEXHIP_ERR_OVERFLOW;
  }
  const speexhip::Realign r = speexhip::realign_history(old_filt_len, new_filt_len, magic);
  *shift = r.shift;
  *new_magic = r.new_magic;
  *last_delta = r.last_delta;
  return SPEEXHIP_ERR_SUCCESS;
}

const char *speexhip_version(void) { return "speexhip 0.7.0 gfx950"; }

}  // extern "C"
