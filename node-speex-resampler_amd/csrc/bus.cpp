// bus.cpp -- the mix buses of engine.h (include/speexhip_resampler.h, "Buses"): the state's bus matrix and the bus call.
// A bus call is the sides call up to the float images of the streams; where the sides call encodes each stream, bus_sum
// (kernels_bus.hip) sums the streams' images -- each behind its own gain -- into the float images of the buses, and the
// existing output pass (side_pass, mix.cpp) encodes those, with the buses in the place of the streams.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bus.h"
#include "dither.h"
#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

namespace {
// the state's device block of the buses: the cells, then W as bus_sum reads it (transposed, rows of kMaxBuses floats)
constexpr size_t kCellsBytes = sizeof(MeterCell) * bus::kMaxBuses;
constexpr size_t kWeightsBytes = sizeof(float) * bus::kMaxStreams * bus::kMaxBuses;
inline size_t block_bytes() { return std::max(kCellsBytes + kWeightsBytes, kCtlCopyMin); }
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
  if (n_buses != 0) {
    void *block = d_bus_;
    if (block == nullptr) {
      rc = dev_alloc(device_, &block, block_bytes());
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    }
    // one image: the cells zeroed, W transposed, zeros behind its buses
    std::vector<char> image(kCellsBytes + kWeightsBytes, 0);
    float *wt = reinterpret_cast<float *>(image.data() + kCellsBytes);
    for (uint32_t j = 0; j < n_buses; j++)
      for (uint32_t s = 0; s < n_streams_; s++) wt[s * bus::kMaxBuses + j] = weights[static_cast<size_t>(j) * n_streams_ + s];
    rc = ctl_upload(block, image.data(), image.size(), own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) {
      if (d_bus_ == nullptr) pool::device_put(device_, block);
      return rc;  // (a block that was there keeps what the copy left: the buses are off until a set_buses succeeds)
    }
    d_bus_ = static_cast<char *>(block);
    bus_w_.assign(weights, weights + static_cast<size_t>(n_buses) * n_streams_);
  } else {
    bus_w_.clear();
  }
  n_buses_ = n_buses;
  bus_samples_.assign(n_buses, 0);
  bus_pos_ = 0;
  return SPEEXHIP_ERR_SUCCESS;
}

int Batch::get_buses(uint32_t *n_buses, float *weights) const {
  if (n_buses != nullptr) *n_buses = n_buses_;
  if (weights != nullptr && !bus_w_.empty()) std::memcpy(weights, bus_w_.data(), bus_w_.size() * sizeof(float));
  return SPEEXHIP_ERR_SUCCESS;
}

DitherPack Batch::bus_dither_pack(uint32_t per_frame) const {
  DitherPack d;
  std::memset(&d, 0, sizeof(d));
  d.kind = dither_kind_;
  for (uint32_t j = 0; j < n_buses_; j++) {
    d.s[j].seed = dither::stream_seed(dither_seed_, n_streams_ + j);
    d.s[j].first = bus_pos_ * per_frame;  // (mod 2^64, like idx)
  }
  return d;
}

MeterPack Batch::bus_meter_pack() const {
  MeterPack p;
  std::memset(&p, 0, sizeof(p));
  for (uint32_t j = 0; j < n_buses_; j++) p.cell[j] = reinterpret_cast<MeterCell *>(d_bus_) + j;
  return p;
}

int Batch::get_bus_meter(uint32_t bus, SpeexHipMeter *m, bool reset) {
  if (bus >= n_buses_ || (m == nullptr && !reset)) return SPEEXHIP_ERR_INVALID_ARG;
  if (m != nullptr && m->struct_size < sizeof(SpeexHipMeter)) return SPEEXHIP_ERR_INVALID_ARG;
  ON_DEVICE();
  int rc = quiesce();  // this state's own last call; its totals are in the cells behind it
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  // (the block travels whole: a copy that ends behind the cells would take the runtime's blit kernel)
  std::vector<char> image(kCellsBytes + kWeightsBytes);
  rc = ctl_download(image.data(), d_bus_, block_bytes(), 0, image.size(), own_stream_);
  if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
  MeterCell *cells = reinterpret_cast<MeterCell *>(image.data());
  SpeexHipMeter now;
  std::memset(&now, 0, sizeof(now));
  now.on = meter_on_ ? 1u : 0u;
  now.samples = bus_samples_[bus];
  now.clipped_high = cells[bus].hi;
  now.clipped_low = cells[bus].lo;
  now.nan = cells[bus].nan;
  std::memcpy(&now.peak, &cells[bus].peak_bits, sizeof(now.peak));
  if (reset) {  // (nothing of this state is in flight: the block goes back whole, this bus's cell zeroed)
    std::memset(&cells[bus], 0, sizeof(MeterCell));
    rc = ctl_upload(d_bus_, image.data(), image.size(), own_stream_);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    bus_samples_[bus] = 0;
  }
  if (m != nullptr) {
    now.struct_size = m->struct_size;
    std::memcpy(m, &now, sizeof(now));
  }
  return SPEEXHIP_ERR_SUCCESS;
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
  rc = process_device(im.in, im.in_stride, in_len, d_planar_out_, out_pitch, out_len, true, stream);
  if (!ran(rc)) return rc;
  // (out_len: what the float call produced; the zero fallback's zeros are summed like any value)
  BusPack pack;
  std::memset(&pack, 0, sizeof(pack));
  for (uint32_t s = 0; s < n_streams_; s++) {
    pack.src[s] = reinterpret_cast<const float *>(d_planar_out_) + s * out_pitch;
    pack.frames[s] = out_len[s];
  }
  pack.dst = pass_out ? reinterpret_cast<float *>(d_bus_image_) : static_cast<float *>(out.base);
  pack.dst_pitch = pass_out ? out_pitch : out.stride;
  pack.w = reinterpret_cast<const float *>(d_bus_ + kCellsBytes);
  pack.n_streams = n_streams_;
  pack.n_buses = n_buses_;
  pack.channels = channels_;
  pack.bus_frames = most_out;
  if (hip_failed(launch_bus_sum(pack, gain_pack(0, n_streams_, channels_), stream), "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  const std::vector<uint32_t> lens(n_buses_, most_out);
  if (pass_out) {
    const int prc = side_pass(out, false, d_bus_image_, out_pitch, lens.data(), stream, nullptr, true);
    if (prc != SPEEXHIP_ERR_SUCCESS) return prc;
  } else if (r.finish != SidesRoute::Nothing) {
    // (interleaved F32: bus_sum wrote the caller's buffer, meter_image reads it once more)
    const int mrc = meter_result(out.base, out.stride, lens.data(), r.finish_scale, stream, true);
    if (mrc != SPEEXHIP_ERR_SUCCESS) return mrc;
  }
  if (r.counts_meter)
    for (uint32_t j = 0; j < n_buses_; j++) bus_samples_[j] += static_cast<uint64_t>(most_out) * channels_;
  if (r.moves_gain) gain_advance(out_len);
  if (r.moves_dither) bus_pos_ += most_out;
  *bus_frames = most_out;
  return rc;
}

}  // namespace speexhip
