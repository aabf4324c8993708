// bus.cpp -- the mix buses of engine.h (include/speexhip_resampler.h, "Buses"): the state's bus matrix and the bus call.
// A bus call is the sides call up to the float images of the streams; where the sides call encodes each stream, bus_sum
// (kernels_bus.hip) sums the streams' images -- each behind its own gain -- into the float images of the buses, and the
// buses' output stage (bus_out.h) encodes those.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bus.h"
#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
// the state's device block of the buses: W as bus_sum reads it (transposed, rows of kMaxBuses floats)
constexpr size_t kWeightsFloats = static_cast<size_t>(bus::kMaxStreams) * bus::kMaxBuses;
inline size_t block_bytes() { return std::max(sizeof(float) * kWeightsFloats, kCtlCopyMin); }
}  // namespace

int Batch::set_buses(uint32_t n_buses, const float *weights) {
  if (weights == nullptr) n_buses = 0;
  if (n_buses > bus::kMaxBuses) return SPEEXHIP_ERR_INVALID_ARG;
  if (n_buses != 0 && n_streams_ > bus::kMaxStreams) return SPEEXHIP_ERR_INVALID_ARG;
  for (size_t i = 0; i < static_cast<size_t>(n_buses) * n_streams_; i++)
    if (!std::isfinite(weights[i])) return SPEEXHIP_ERR_INVALID_ARG;
  ON_DEVICE();
  int rc = quiesce();  // this state's own last call may still read the matrix and add into the cells
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // W and the zeroed cells are on the device before any host field changes: a copy that fails returns its code and
  // leaves the state's fields as they were (a block that was there keeps what the copy left)
  void *block = d_bus_;
  if (n_buses != 0) {
    if (block == nullptr) {
      rc = dev_alloc(device_, &block, block_bytes());
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    }
    std::vector<float> wt(kWeightsFloats, 0.0f);  // W transposed, zeros behind its buses
    for (uint32_t j = 0; j < n_buses; j++)
      for (uint32_t s = 0; s < n_streams_; s++) wt[s * bus::kMaxBuses + j] = weights[static_cast<size_t>(j) * n_streams_ + s];
    rc = ctl_upload(block, wt.data(), wt.size() * sizeof(float), own_stream_);
  }
  if (rc == SPEEXHIP_ERR_SUCCESS) rc = bus_out_.resize(n_buses, own_stream_);  // (the cells, the totals, the position)
  if (rc != SPEEXHIP_ERR_SUCCESS) {
    if (block != d_bus_) pool::device_put(device_, block);
    return rc;
  }
  d_bus_ = static_cast<char *>(block);
  bus_w_.assign(weights, weights + static_cast<size_t>(n_buses) * n_streams_);
  n_buses_ = n_buses;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::get_buses(uint32_t *n_buses, float *weights) const {
  if (n_buses != nullptr) *n_buses = n_buses_;
  if (weights != nullptr && !bus_w_.empty()) std::memcpy(weights, bus_w_.data(), bus_w_.size() * sizeof(float));
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::get_bus_meter(uint32_t bus, SpeexHipMeter *m, bool reset) {
  if (!meter_request_ok(bus, n_buses_, m, reset)) return SPEEXHIP_ERR_INVALID_ARG;
  ON_DEVICE();
  const int rc = quiesce();  // this state's own last call; its totals are in the cells behind it
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  return bus_out_.get_meter(bus, m, reset, own_stream_);
}

int Batch::process_bus_device(const CallSide &in_side, uint32_t *in_len, const CallSide &out_side, uint32_t *out_len,
                              uint32_t *bus_frames, hipStream_t stream) {
  if (bus_frames == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  if (n_buses_ == 0) return SPEEXHIP_ERR_BAD_STATE;
  if (out_side.mix != nullptr) return SPEEXHIP_ERR_INVALID_ARG;  // (a matrix on the sum is no part of this call)
  if (!side_ok(in_side, channels_) || !side_ok(out_side, channels_) || out_side.base == nullptr) return SPEEXHIP_ERR_INVALID_ARG;
  if (!lengths_fit(in_len, out_len, n_streams_)) return SPEEXHIP_ERR_OVERFLOW;  // (engine.h; nothing touched)
  CallSide in = in_side, out = out_side;
  if (!side_planar(in)) in.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  if (!side_planar(out)) out.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
  ON_DEVICE();
  // (channels that stand apart produce different numbers of frames: a bus has no frame to sum them in)
  const SidesRoute r = route_sides_call(SidesForm::Bus, side_kind(in), side_kind(out), sides_state());
  if (r.refuse != SPEEXHIP_ERR_SUCCESS) return r.refuse;
  // the input side as in process_sides_device; the streams' results always lie in the state's image, whatever the buses'
  // format: bus_sum reads them there.  An interleaved F32 bus side IS the buses' image.
  SideImages im;
  int rc = prepare_images(in, in_len, out_len, r, false, true, stream, &im);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  const bool pass_out = r.pass_out;
  const size_t out_pitch = im.out_pitch;
  const uint32_t most_out = im.most_out;
  const size_t image_bytes = pass_out ? out_pitch * n_buses_ * sizeof(float) : 0;
  if (image_bytes > bus_out_.image_capacity()) {
    rc = quiesce();  // (a grow waits for the state's own last call, which may still read the old image)
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    rc = bus_out_.grow_image(image_bytes);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  }
  rc = process_device(im.in, im.in_stride, in_len, d_planar_out_, out_pitch, out_len, true, stream);
  if (!ran(rc)) return rc;
  // (out_len: what the float call produced; the zero fallback's zeros are summed like any value)
  BusPack pack;
  std::memset(&pack, 0, sizeof(pack));
  for (uint32_t s = 0; s < n_streams_; s++) {
    pack.src[s] = reinterpret_cast<const float *>(d_planar_out_) + s * out_pitch;
    pack.frames[s] = out_len[s];
  }
  pack.dst = pass_out ? reinterpret_cast<float *>(bus_out_.image()) : static_cast<float *>(out.base);
  pack.dst_pitch = pass_out ? out_pitch : out.stride;
  pack.w = reinterpret_cast<const float *>(d_bus_);
  pack.n_streams = n_streams_;
  pack.n_buses = n_buses_;
  pack.channels = channels_;
  pack.bus_frames = most_out;
  if (hip_failed(launch_bus_sum(pack, gain_pack(0, n_streams_, channels_), stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  const int erc = bus_out_.encode(r, out, bus_out_.image(), out_pitch, most_out, stream, nullptr);
  if (erc != SPEEXHIP_ERR_SUCCESS) return erc;
  bus_out_.moved(r, most_out);
  if (r.moves_gain) gain_advance(out_len);
  *bus_frames = most_out;
  return rc;
}

}  // namespace speexhip
