// bus_out.cpp -- the output stage of a set of mix buses (bus_out.h), and the one meter read-out it shares with a state's
// streams (engine.cpp, Batch::get_meter).
#include "bus_out.h"

#include <algorithm>
#include <cstring>

#include "dither.h"
#include "engine.h"
#include "engine_detail.h"
#include "pool.h"

namespace speexhip {
using namespace detail;

bool detail::meter_request_ok(uint32_t i, uint32_t n, const SpeexHipMeter *m, bool reset) {
  if (i >= n || (m == nullptr && !reset)) return false;
  return m == nullptr || m->struct_size >= sizeof(SpeexHipMeter);
}

int detail::read_meter(MeterCell *d_cells, uint32_t n, uint32_t i, bool on, uint64_t *samples, SpeexHipMeter *m, bool reset,
                       hipStream_t stream) {
  SpeexHipMeter now;
  std::memset(&now, 0, sizeof(now));
  now.on = on ? 1u : 0u;
  if (d_cells != nullptr) {
    std::vector<MeterCell> cells(n);
    const size_t bytes = sizeof(MeterCell) * n;
    int rc = ctl_download(cells.data(), reinterpret_cast<const char *>(d_cells), std::max(bytes, kCtlCopyMin), 0, bytes, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    const MeterCell &c = cells[i];
    now.samples = samples[i];
    now.clipped_high = c.hi;
    now.clipped_low = c.lo;
    now.nan = c.nan;
    std::memcpy(&now.peak, &c.peak_bits, sizeof(now.peak));
    if (reset) {  // (nothing of the owner's is in flight: the cells go back whole, this one zeroed)
      std::memset(&cells[i], 0, sizeof(MeterCell));
      rc = ctl_upload(d_cells, cells.data(), bytes, stream);
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
      samples[i] = 0;
    }
  }
  if (m != nullptr) {
    now.struct_size = m->struct_size;
    std::memcpy(m, &now, sizeof(now));
  }
  return SPEEXHIP_ERR_SUCCESS;
}

ConvertPack detail::float_results_pack(const float *base, uint64_t stride, const uint32_t *lens, uint32_t n, uint32_t channels,
                                       uint64_t *most) {
  ConvertPack pack;
  std::memset(&pack, 0, sizeof(pack));
  *most = 0;
  for (uint32_t j = 0; j < n; j++) {
    pack.s[j].src = pack.s[j].dst = const_cast<float *>(base) + j * stride;
    pack.s[j].n = static_cast<uint64_t>(lens[j]) * channels;
    pack.s[j].step = 1;
    *most = std::max(*most, pack.s[j].n);
  }
  return pack;
}

void BusOutput::bind(int device, uint32_t channels, uint32_t seed_base) {
  device_ = device;
  channels_ = channels;
  seed_base_ = seed_base;
}

void BusOutput::release() {
  pool::device_put(device_, d_image_);
  pool::device_put(device_, d_cells_);
}

int BusOutput::resize(uint32_t n_buses, hipStream_t stream) {
  if (n_buses != 0) {
    const size_t bytes = std::max(sizeof(MeterCell) * n_buses, kCtlCopyMin);
    void *block = bytes <= cells_cap_ ? d_cells_ : nullptr;
    if (block == nullptr) {
      const int rc = dev_alloc(device_, &block, bytes);
      if (rc != SPEEXHIP_ERR_SUCCESS) return rc;
    }
    const std::vector<char> zeros(bytes, 0);
    const int rc = ctl_upload(block, zeros.data(), bytes, stream);
    if (rc != SPEEXHIP_ERR_SUCCESS) {
      if (block != d_cells_) pool::device_put(device_, block);
      return rc;  // (cells that were there keep what the copy left)
    }
    if (block != d_cells_) {
      pool::device_put(device_, d_cells_);
      d_cells_ = static_cast<MeterCell *>(block);
      cells_cap_ = bytes;
    }
  }
  n_buses_ = n_buses;
  samples_.assign(n_buses, 0);
  pos_ = 0;
  return SPEEXHIP_ERR_SUCCESS;
}

void BusOutput::set_dither(int kind, uint64_t seed, uint64_t position) {
  dither_kind_ = kind;
  dither_seed_ = seed;
  pos_ = position;
}

int BusOutput::get_meter(uint32_t bus, SpeexHipMeter *m, bool reset, hipStream_t stream) {
  return read_meter(d_cells_, n_buses_, bus, meter_on_, samples_.data(), m, reset, stream);
}

int BusOutput::grow_image(size_t bytes) { return grow_stage(device_, &d_image_, &image_cap_, bytes, false); }

int BusOutput::encode(const SidesRoute &bus_route, const CallSide &side, const char *image, size_t pitch, uint32_t frames,
                      hipStream_t stream, uint32_t *launches) {
  if (frames == 0 || (!bus_route.pass_out && bus_route.finish != SidesRoute::MeterImage)) return SPEEXHIP_ERR_SUCCESS;
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  const bool planar = side.layout == SPEEXHIP_LAYOUT_PLANAR;
  const bool dithered = dither_kind_ != SPEEXHIP_DITHER_NONE && dithered_fmt(side.fmt);
  const size_t es = sample_bytes(side.fmt);
  uint32_t lens[kMaxPackedStreams];
  std::fill(lens, lens + kChunk, frames);
  for (uint32_t first = 0; first < n_buses_; first += kChunk) {
    const uint32_t n = std::min(kChunk, n_buses_ - first);
    DitherPack dith;
    std::memset(&dith, 0, sizeof(dith));
    dith.kind = dither_kind_;
    MeterPack cells;
    std::memset(&cells, 0, sizeof(cells));
    for (uint32_t j = 0; j < n; j++) {
      dith.s[j].seed = dither::stream_seed(dither_seed_, seed_base_ + first + j);
      dith.s[j].first = pos_ * (planar ? 1 : channels_);  // (mod 2^64, like idx)
      cells.cell[j] = d_cells_ + first + j;
    }
    const DitherPack *dither = dithered ? &dith : nullptr;
    const MeterPack *meter = bus_route.counts_meter ? &cells : nullptr;
    char *storage = static_cast<char *>(side.base) + first * side.stride * es;
    const float *floats = bus_route.pass_out ? reinterpret_cast<const float *>(image) + first * pitch : nullptr;
    uint64_t most = 0;
    hipError_t e;
    if (!bus_route.pass_out) {
      // (interleaved F32: the sum wrote the caller's side, meter_image reads it once more)
      const ConvertPack pack = float_results_pack(reinterpret_cast<const float *>(storage), side.stride, lens, n, channels_, &most);
      e = launch_meter_image(pack, cells, bus_route.finish_scale, n, most, stream);
    } else if (planar) {
      PlanePack pack;
      std::memset(&pack, 0, sizeof(pack));
      pack.storage_channels = pack.image_channels = pack.image_pitch = channels_;
      for (uint32_t j = 0; j < n; j++) {
        pack.s[j].src = floats + j * pitch;
        pack.s[j].dst = storage + j * side.stride * es;
        pack.s[j].plane_stride = side.plane_stride;
        pack.s[j].frames = frames;
      }
      e = launch_planes(side.fmt, true, pack, dither, n, frames, stream, meter, nullptr);
    } else {
      ConvertPack pack = float_results_pack(floats, pitch, lens, n, channels_, &most);
      for (uint32_t j = 0; j < n; j++) pack.s[j].dst = storage + j * side.stride * es;
      e = launch_convert(side.fmt, true, pack, dither, n, most, stream, meter, nullptr);
    }
    if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
    if (launches != nullptr) (*launches)++;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

void BusOutput::moved(const SidesRoute &bus_route, uint32_t frames) {
  if (bus_route.counts_meter)
    for (uint64_t &total : samples_) total += static_cast<uint64_t>(frames) * channels_;
  if (bus_route.moves_dither) pos_ += frames;
}

}  // namespace speexhip
