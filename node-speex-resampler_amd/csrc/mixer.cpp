// mixer.cpp -- the mixer of mixer.h (include/speexhip_resampler.h, "Mixer"): the object, its control calls and process.
// A mixer call is the many-states call up to the float images of the legs; where that call encodes each state and sends
// it back, bus_sum_legs (kernels_bus_legs.hip) sums the slots' images -- each behind its own state's gain -- into the float
// images of the buses, and the buses' output stage (bus_out.h) encodes those.  What process does here is what bus.cpp and
// formats.cpp do for their calls: check the arguments, ask the route of every leg and of the bus side, hand the rest to
// the unit machinery (many.cpp), and move what the call moved.
#include "mixer.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "bus.h"
#include "devices.h"
#include "dither.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

// the device blocks: control-plane data, moved whole through the copy engines (engine_detail.h, kCtlCopyMin)
size_t Mixer::weights_bytes() const { return std::max(sizeof(float) * n_legs_ * w_pitch_, kCtlCopyMin); }

Mixer *Mixer::create(uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err, int device) {
  int e = SPEEXHIP_ERR_SUCCESS;
  Mixer *m = nullptr;
  if (n_legs == 0 || n_legs > kBusMaxLegs || n_buses == 0 || n_buses > kBusMaxBuses || channels == 0 || channels > kMixMaxChannels) {
    e = SPEEXHIP_ERR_INVALID_ARG;
  } else {
    const int count = devices::count();
    if (count <= 0) {
      g_last_error = "HIP device error: no GPU visible (libspeexhip has no CPU fallback)";
      e = SPEEXHIP_ERR_DEVICE;
    } else if (device >= count) {
      e = SPEEXHIP_ERR_INVALID_ARG;
    } else {
      if (device < 0) device = devices::place_next_state();
      if (device < 0) {
        g_last_error = "HIP device error: SPEEXHIP_DEVICE / SPEEXHIP_DEVICES names a device this node does not have";
        e = SPEEXHIP_ERR_DEVICE;
      }
    }
  }
  if (e == SPEEXHIP_ERR_SUCCESS) {
    m = new (std::nothrow) Mixer();
    if (m == nullptr) e = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  if (e == SPEEXHIP_ERR_SUCCESS) {
    m->n_legs_ = n_legs;
    m->n_buses_ = n_buses;
    m->channels_ = channels;
    m->device_ = device;
    m->w_pitch_ = (n_buses + kBusGroup - 1) / kBusGroup * kBusGroup;
    m->buses_.bind(device, channels, n_legs);
    e = [m, n_buses]() -> int {
      DeviceScope scope(m->device_);
      HIP_TRY(scope.error());
      HIP_TRY(pool::stream_get(m->device_, &m->stream_));
      void *w = nullptr;
      const int rc = dev_alloc(m->device_, &w, m->weights_bytes());
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
      m->d_w_ = static_cast<char *>(w);
      return m->buses_.resize(n_buses, m->stream_);
    }();
  }
  if (e != SPEEXHIP_ERR_SUCCESS) {
    delete m;
    m = nullptr;
  }
  if (err != nullptr) *err = e;
  return m;
}

Mixer::~Mixer() {
  DeviceScope scope(device_);
  // (process is synchronous and the control calls wait for their copies: nothing of the mixer's is in flight)
  buses_.release();
  pool::device_put(device_, d_level_parts_);
  pool::device_put(device_, d_w_);
  pool::stream_put(device_, stream_);
}

int Mixer::set_weights(const float *weights) {
  // (the mixer's own last call: process has waited for everything it queued before it returned)
  if (weights == nullptr) {
    on_ = false;
    w_.clear();
    return SPEEXHIP_ERR_SUCCESS;
  }
  const size_t n = static_cast<size_t>(n_buses_) * n_legs_;
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(weights[i])) return SPEEXHIP_ERR_INVALID_ARG;
  DeviceScope scope(device_);
  HIP_TRY(scope.error());
  // the transpose, rows of w_pitch_ floats, zeros behind n_buses: a group's eight weights of a leg are one aligned load
  std::vector<float> wt(static_cast<size_t>(n_legs_) * w_pitch_, 0.0f);
  for (uint32_t j = 0; j < n_buses_; j++)
    for (uint32_t s = 0; s < n_legs_; s++) wt[static_cast<size_t>(s) * w_pitch_ + j] = weights[static_cast<size_t>(j) * n_legs_ + s];
  on_ = false;  // (a copy that fails leaves the mixer off until a set_weights succeeds)
  int rc = ctl_upload(d_w_, wt.data(), wt.size() * sizeof(float), stream_);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  rc = buses_.reset(stream_);  // (the cells, the totals, the position)
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  w_.assign(weights, weights + n);
  on_ = true;
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::get_weights(float *weights) const {
  if (weights == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  if (!on_) return SPEEXHIP_ERR_BAD_STATE;
  std::memcpy(weights, w_.data(), w_.size() * sizeof(float));
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::set_dither(int kind, uint64_t seed, uint64_t position) {
  if (!dither::known_kind(kind)) return SPEEXHIP_ERR_INVALID_ARG;
  buses_.set_dither(kind, seed, position);
  return SPEEXHIP_ERR_SUCCESS;
}
int Mixer::get_dither(int *kind, uint64_t *seed, uint64_t *position) const {
  if (kind != nullptr) *kind = buses_.dither_kind();
  if (seed != nullptr) *seed = buses_.dither_seed();
  if (position != nullptr) *position = buses_.position();
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::set_meter(int on) {
  if (on != 0 && on != 1) return SPEEXHIP_ERR_INVALID_ARG;
  buses_.set_meter(on != 0);  // (the totals stay, as a state's do)
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::get_bus_meter(uint32_t bus, SpeexHipMeter *m, bool reset) {
  if (!meter_request_ok(bus, n_buses_, m, reset)) return SPEEXHIP_ERR_INVALID_ARG;
  DeviceScope scope(device_);
  HIP_TRY(scope.error());
  // (process is synchronous: nothing of the mixer's is in flight)
  return buses_.get_meter(bus, m, reset, stream_);
}

int Mixer::set_levels(int on) {
  if (on != 0 && on != 1) return SPEEXHIP_ERR_INVALID_ARG;
  if ((on != 0) == levels_on_) return SPEEXHIP_ERR_SUCCESS;  // (no change: the snapshot stays)
  levels_on_ = on != 0;
  levels_.assign(levels_on_ ? n_legs_ : 0, SpeexHipLevel{});
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::get_levels(uint32_t first, uint32_t count, void *levels, uint32_t struct_size) const {
  if (levels == nullptr || struct_size < sizeof(SpeexHipLevel) || first > n_legs_ || count > n_legs_ - first) return SPEEXHIP_ERR_INVALID_ARG;
  if (!levels_on_) return SPEEXHIP_ERR_BAD_STATE;
  for (uint32_t k = 0; k < count; k++)
    std::memcpy(static_cast<char *>(levels) + static_cast<size_t>(k) * struct_size, &levels_[first + k], sizeof(SpeexHipLevel));
  return SPEEXHIP_ERR_SUCCESS;
}

int Mixer::process(Batch *const *legs, const CallSide *in, const uint8_t *bad, uint32_t *in_len, uint32_t *out_len,
                   const CallSide &out_side, uint32_t *bus_frames, int *codes) {
  // ---- the call's own errors: nothing touched, codes not written
  if (legs == nullptr || in == nullptr || in_len == nullptr || out_len == nullptr || bus_frames == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  if (out_side.mix != nullptr || out_side.planes != nullptr || out_side.base == nullptr || !side_ok(out_side, channels_))
    return SPEEXHIP_ERR_INVALID_ARG;
  if (!on_) return SPEEXHIP_ERR_BAD_STATE;
  CallSide out = out_side;
  if (!side_planar(out)) out.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  // (the bus side's route is the Batch's bus call's: the same rule, with the mixer's switches for the state's)
  const SideKind image_kind = {SPEEXHIP_FMT_F32, false, false, false};
  SidesState bus_state = {};
  bus_state.dither = buses_.dither_kind() != SPEEXHIP_DITHER_NONE;
  bus_state.meter = buses_.meter_on();
  const SidesRoute bus_route = route_sides_call(SidesForm::Bus, image_kind, side_kind(out), bus_state);
  if (bus_route.refuse != SPEEXHIP_ERR_SUCCESS) return bus_route.refuse;

  // ---- the legs: an outcome each; a refused leg keeps its state and both its lengths and supplies +0.0f
  std::vector<Batch::ManyEntry> entries(n_legs_);
  std::vector<int> rcs(n_legs_, SPEEXHIP_ERR_SUCCESS);
  for (uint32_t i = 0; i < n_legs_; i++) {
    Batch::ManyEntry &e = entries[i];
    Batch *b = e.b = legs[i];
    if (b == nullptr) {  // an empty slot
      in_len[i] = out_len[i] = 0;
      continue;
    }
    e.leg = e.sides = true;
    bool earlier = false;
    for (uint32_t k = 0; k < i && !earlier; k++) earlier = legs[k] == b;
    if ((bad != nullptr && bad[i] != 0) || !side_ok(in[i], channels_) || in[i].channels != channels_ || b->channels_ != channels_ ||
        b->device_ != device_) {
      e.rc = SPEEXHIP_ERR_INVALID_ARG;
    } else {
      e.route = route_sides_call(SidesForm::MixerLeg, side_kind(in[i]), image_kind, b->sides_state(earlier));
      e.rc = e.route.refuse;
      if (e.rc == SPEEXHIP_ERR_SUCCESS && !b->lengths_fit(&in_len[i], &out_len[i], 1)) e.rc = SPEEXHIP_ERR_OVERFLOW;
    }
    rcs[i] = e.rc;
    e.in_side = in[i];
    e.in_fmt = in[i].fmt;
    e.out_fmt = SPEEXHIP_FMT_F32;
    e.in = in[i].base;
  }
  MixerCall mc;
  mc.device = device_;
  mc.n_legs = n_legs_;
  mc.d_w = reinterpret_cast<const float *>(d_w_);
  mc.w_pitch = w_pitch_;
  mc.out = out;
  mc.bus_route = bus_route;
  mc.buses = &buses_;
  if (levels_on_) {
    // (from here on the call touches things: the snapshot is this call's -- zeros until the unit has filled it, and so
    //  after a unit that failed and after a call of bus_frames 0)
    levels_.assign(n_legs_, SpeexHipLevel{});
    mc.levels = levels_.data();
    mc.level_parts = &d_level_parts_;
    mc.level_parts_cap = &level_parts_cap_;
  }
  int unit_rc;
  try {
    unit_rc = Batch::many_mixer(mc, n_legs_, entries.data(), in_len, out_len, rcs.data());
  } catch (const std::bad_alloc &) {
    unit_rc = SPEEXHIP_ERR_ALLOC_FAILED;
  }
  if (unit_rc != SPEEXHIP_ERR_SUCCESS) {
    // (as in the many-states calls: the unit's failure is the code of every leg it was to run)
    for (uint32_t i = 0; i < n_legs_; i++)
      if (entries[i].b != nullptr && entries[i].rc == SPEEXHIP_ERR_SUCCESS) rcs[i] = unit_rc;
    if (levels_on_) levels_.assign(n_legs_, SpeexHipLevel{});
  } else {
    // what the call moved beside its legs: the buses' totals and the one bus position
    buses_.moved(bus_route, mc.bus_frames);
    *bus_frames = mc.bus_frames;
  }
  int first = SPEEXHIP_ERR_SUCCESS;
  for (uint32_t i = 0; i < n_legs_; i++) {
    if (codes != nullptr) codes[i] = rcs[i];
    if (first == SPEEXHIP_ERR_SUCCESS && rcs[i] != SPEEXHIP_ERR_SUCCESS) first = rcs[i];
  }
  return first;
}

}  // namespace speexhip
