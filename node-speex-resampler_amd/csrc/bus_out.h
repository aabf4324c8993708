// bus_out.h -- the output stage of a set of mix buses, and the only code that knows how buses leave the device: the float
// image of the buses is encoded into the caller's format, dithered from the bus seeds at the one bus position, judged into
// one meter cell per bus and never gained (the streams were gained before they were summed); an interleaved F32 side, which
// the summing kernel wrote itself, is only read by meter_image.  A Batch (bus.cpp: bus_sum over its own streams) and a
// Mixer (mixer.cpp: bus_sum_legs over separate states) hold one each, forward their control calls to it and ask the route
// of their bus side (sides_route.h, SidesForm::Bus), which encode and moved obey.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/speexhip_resampler.h"
#include "kernels.h"
#include "sides_route.h"

namespace speexhip {

struct CallSide;  // engine.h

namespace detail {
// The one meter read-out, of cell i of a device block of n cells (a state's streams, a set of buses).  The block is
// control-plane data: max(sizeof(MeterCell) * n, kCtlCopyMin) bytes, moved whole through the copy engines.
// meter_request_ok: what every read-out refuses with INVALID_ARG before it touches anything.  read_meter: the cell and
// samples[i] as a SpeexHipMeter into *m (may be null); reset: the cells go back whole with cell i zeroed, and samples[i]
// is zero from here on.  d_cells == nullptr (a meter that was never turned on): zeros, nothing moved.  Nothing that adds
// into the cells may be in flight.
bool meter_request_ok(uint32_t i, uint32_t n, const SpeexHipMeter *m, bool reset);
int read_meter(MeterCell *d_cells, uint32_t n, uint32_t i, bool on, uint64_t *samples, SpeexHipMeter *m, bool reset, hipStream_t stream);
// The pack of n float results as meter_image reads them (src) and gain_image multiplies them in place (dst): item j is
// lens[j] frames of `channels` floats at base + j * stride (floats).  *most: the largest sample count among them.
ConvertPack float_results_pack(const float *base, uint64_t stride, const uint32_t *lens, uint32_t n, uint32_t channels, uint64_t *most);
}  // namespace detail

class BusOutput {
 public:
  BusOutput() = default;
  BusOutput(const BusOutput &) = delete;
  BusOutput &operator=(const BusOutput &) = delete;
  // Once, before anything else.  seed_base: the index of bus 0 in the owner's seed sequence -- bus j draws from
  // dither::stream_seed(seed, seed_base + j) -- n_streams() for a batch, n_legs for a mixer.
  void bind(int device, uint32_t channels, uint32_t seed_base);
  // The owner's destructor, on the device, nothing in flight: the blocks back to the pool.
  void release();

  // n_buses buses from here on: the cells (allocated by the first call that needs them) zeroed on the device, then the
  // totals and the position zeroed.  A copy that fails: its code, everything on the host as it was.  n_buses == 0: off,
  // nothing uploaded.  reset: the same for the buses there are.
  int resize(uint32_t n_buses, hipStream_t stream);
  int reset(hipStream_t stream) { return resize(n_buses_, stream); }
  void set_dither(int kind, uint64_t seed, uint64_t position);  // (the owner has checked the kind)
  void set_meter(bool on) { meter_on_ = on; }  // (the totals stay)
  uint32_t n_buses() const { return n_buses_; }
  int dither_kind() const { return dither_kind_; }
  uint64_t dither_seed() const { return dither_seed_; }
  uint64_t position() const { return pos_; }  // index of every bus's next output frame
  bool meter_on() const { return meter_on_; }
  int get_meter(uint32_t bus, SpeexHipMeter *m, bool reset, hipStream_t stream);  // (the request checked by the owner)

  // The float image of the buses, grow-only.  The caller has waited for whatever may still read the old one.
  int grow_image(size_t bytes);
  char *image() const { return d_image_; }
  size_t image_capacity() const { return image_cap_; }  // bytes
  // The pass over the buses behind the sum, <= kMaxPackedStreams a launch: bus j is `frames` frames of channels floats at
  // image + j * pitch (floats) and leaves for side.base + j * side.stride (samples) -- planes_out for a planar side,
  // convert_out otherwise -- dithered where the kind and the format say so, judged when bus_route.counts_meter.  A side
  // that passes through no image (bus_route.pass_out false: the sum wrote side.base) is read by meter_image when the route
  // says so.  frames == 0: nothing launched.  *launches (may be null): the passes launched, added.
  int encode(const SidesRoute &bus_route, const CallSide &side, const char *image, size_t pitch, uint32_t frames, hipStream_t stream,
             uint32_t *launches);
  // What a call that ran moves: every bus's total by frames * channels, the position by frames, as the route says.
  void moved(const SidesRoute &bus_route, uint32_t frames);

 private:
  int device_ = 0;
  uint32_t n_buses_ = 0, channels_ = 0, seed_base_ = 0;
  int dither_kind_ = SPEEXHIP_DITHER_NONE;
  uint64_t dither_seed_ = 0, pos_ = 0;
  bool meter_on_ = false;
  std::vector<uint64_t> samples_;  // per bus: samples metered since the last reset
  MeterCell *d_cells_ = nullptr;   // one cell per bus
  size_t cells_cap_ = 0;           // bytes
  char *d_image_ = nullptr;
  size_t image_cap_ = 0;           // bytes
};

}  // namespace speexhip
