// mixer.h -- the mixer (include/speexhip_resampler.h, "Mixer"): mix buses over many separate single-stream states in one
// host call.  The object owns W on the device and the buses' output stage (bus_out.h: their dither kind, seed and one bus
// position, their meter switch, cells and totals, their image) -- and nothing of a leg: the caller names the state in
// every slot with every call.  process describes its legs as entries of the many-states machinery (many.cpp,
// Batch::many_mixer), which carries the call out; every decision is a pure host rule (sides_route.h: SidesForm::MixerLeg
// for a leg, SidesForm::Bus for the bus side; many_plan.h: the stage and the launch groups).
#pragma once
#include <cstdint>
#include <vector>

#include "engine.h"

namespace speexhip {

class Mixer {
 public:
  // nullptr and *err on failure.  device: a logical ordinal (devices.h), or < 0 for the placement rule -- the mixer takes
  // the device the rule gives the process's next state
  static Mixer *create(uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err, int device = -1);
  ~Mixer();
  Mixer(const Mixer &) = delete;
  Mixer &operator=(const Mixer &) = delete;

  // W: n_buses x n_legs, row-major, host; copied, uploaded as bus_sum_legs reads it (kernels.h), the cells, the totals
  // and the bus position zeroed.  nullptr: off.  A weight that is not finite: INVALID_ARG, the mixer as it was.
  int set_weights(const float *weights);
  int get_weights(float *weights) const;  // BAD_STATE while off
  int set_dither(int kind, uint64_t seed, uint64_t position);
  int get_dither(int *kind, uint64_t *seed, uint64_t *position) const;  // the seed as given; the bus position
  int set_meter(int on);
  int get_bus_meter(uint32_t bus, SpeexHipMeter *m, bool reset);
  uint64_t bus_position() const { return buses_.position(); }
  // "Mixer levels": the switch (a change clears the snapshot) and the last process call's records of the slots
  // [first, first + count), struct_size bytes apart.  BAD_STATE while off.
  int set_levels(int on);
  int get_levels(uint32_t first, uint32_t count, void *levels, uint32_t struct_size) const;
  // One tick (the header's speexhip_mixer_process): legs[i] = the state in slot i or nullptr, in[i] its input side in
  // host memory, bad[i] != 0 (bad may be null) = a side the caller could not read.  Synchronous.
  int process(Batch *const *legs, const CallSide *in, const uint8_t *bad, uint32_t *in_len, uint32_t *out_len, const CallSide &out,
              uint32_t *bus_frames, int *codes);
  uint32_t n_legs() const { return n_legs_; }
  uint32_t n_buses() const { return n_buses_; }
  uint32_t channels() const { return channels_; }
  int device() const { return device_; }

 private:
  Mixer() = default;
  size_t weights_bytes() const;
  uint32_t n_legs_ = 0, n_buses_ = 0, channels_ = 0;
  int device_ = 0;
  hipStream_t stream_ = nullptr;   // the control calls' copies
  uint32_t w_pitch_ = 0;           // floats between two legs' rows of the device copy: n_buses rounded up to kBusGroup
  bool on_ = false;                // weights are set
  std::vector<float> w_;           // W as the caller gave it
  char *d_w_ = nullptr;            // its transpose, padded (kernels.h, BusLegsArgs::w)
  BusOutput buses_;                // behind the sum (seed_base = n_legs); the cells zeroed by init and by set_weights
  bool levels_on_ = false;
  std::vector<SpeexHipLevel> levels_;  // the snapshot: n_legs records of the last call, while the levels are on
  char *d_level_parts_ = nullptr;      // the spans' partials of a call whose legs are longer than one span (kernels.h)
  size_t level_parts_cap_ = 0;         // bytes; grow-only, like the buses' image
};

}  // namespace speexhip
