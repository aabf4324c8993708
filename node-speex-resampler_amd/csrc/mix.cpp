// mix.cpp -- a side's pass of a formatted or mixed call (engine.h, process_sides_device): every stream of the batch between
// the caller's storage and the float image the FIR runs on, at most kMaxPackedStreams streams per launch.  A side with a
// matrix runs the mixing kernel (kernels_mix.hip) INSTEAD of the converting one (kernels_convert.hip), so a call launches
// the float call's kernels plus at most one pass per side.  The state's channel count C is what the FIR runs on; a frame
// of a side with a matrix holds side.channels samples in storage and C in the image.  A planar side (CallSide::layout)
// runs the plane kernel (kernels_sides.hip) instead of either, with or without a matrix: still one pass.
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "engine_detail.h"

namespace speexhip {
using namespace detail;

int Batch::side_pass(const CallSide &side, bool to_image, char *image, size_t pitch, const uint32_t *lens, hipStream_t stream,
                     const CallPlan *apart) {
  // an item of the pass: a stream of the batch, or a channel of the one stream whose channels stand apart
  const uint32_t items = apart != nullptr ? channels_ : n_streams_;
  const size_t storage_step = (apart != nullptr ? 1 : side.stride) * sample_bytes(side.fmt);
  const size_t image_step = (apart != nullptr ? 1 : pitch) * sizeof(float);
  // With dither on (set_dither) the formats of dithered_fmt leave through the dithered instances of either pass, at the
  // streams' positions: the index runs over the samples of the OUTPUT frames.
  const bool dithered = !to_image && dither_on() && dithered_fmt(side.fmt);
  // With the meter on (set_meter) every format leaves through the metered instance of its pass, stream by stream into
  // the stream's cell.  (Channels that stand apart are no stream of samples to judge: the callers have refused them.)
  const bool metered = !to_image && meter_on_;
  if (metered && apart != nullptr) return SPEEXHIP_ERR_BAD_STATE;
  // With a stream's gain on (set_gain) every format leaves through the gained instance of its pass, each stream at its own
  // g from its own frame index on; dither and meter ride along in the same instance.  (Channels that stand apart have no
  // output frame to index: the callers have refused them.)
  const bool gained = !to_image && gain_on();
  if (gained && apart != nullptr) return SPEEXHIP_ERR_BAD_STATE;
  const uint32_t kChunk = static_cast<uint32_t>(kMaxPackedStreams);
  for (uint32_t first = 0; first < items; first += kChunk) {
    const uint32_t n = std::min(kChunk, items - first);
    DitherPack dith;
    if (dithered) dith = dither_pack(first, n, side.mix != nullptr ? 1 : channels_);
    MeterPack cells;
    if (metered) cells = meter_pack(first, n);
    const MeterPack *meter = metered ? &cells : nullptr;
    GainPack gains;  // (the flat converting pass walks samples: it divides by channels(); the others walk frames)
    if (gained) gains = gain_pack(first, n, side.layout != SPEEXHIP_LAYOUT_PLANAR && side.mix == nullptr ? channels_ : 1);
    const GainPack *gain = gained ? &gains : nullptr;
    // item first + j is entry j of the launch's pack: where it reads, where it writes, its frames
    const auto place = [&](uint32_t j, const void **src, void **dst) {
      const uint32_t item = first + j;
      char *storage = static_cast<char *>(side.base) + item * storage_step, *in_image = image + item * image_step;
      *src = to_image ? storage : in_image;
      *dst = to_image ? in_image : storage;
      return apart != nullptr ? apart[item].produced : lens[item];
    };
    hipError_t e;
    if (side.layout == SPEEXHIP_LAYOUT_PLANAR) {
      // planes_* (kernels_sides.hip): conversion, matrix and dither in the pass that transposes.  A stream's planes lie
      // plane_stride samples apart; a channel that stands apart is one plane and every channels()-th float of the image
      PlanePack pack;
      std::memset(&pack, 0, sizeof(pack));
      pack.storage_channels = apart != nullptr ? 1 : side.channels;
      pack.image_channels = apart != nullptr ? 1 : channels_;
      pack.image_pitch = channels_;
      pack.mixed = side.mix != nullptr;
      if (side.mix != nullptr) std::memcpy(pack.m, side.mix, sizeof(float) * side.channels * channels_);
      const size_t planar_step = (apart != nullptr ? side.plane_stride : side.stride) * sample_bytes(side.fmt);
      uint32_t most = 0;
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t item = first + j;
        char *storage = static_cast<char *>(side.base) + item * planar_step, *in_image = image + item * image_step;
        pack.s[j].src = to_image ? storage : in_image;
        pack.s[j].dst = to_image ? in_image : storage;
        pack.s[j].plane_stride = side.plane_stride;
        pack.s[j].frames = apart != nullptr ? apart[item].produced : lens[item];
        most = std::max(most, pack.s[j].frames);
      }
      if (dithered) dith = dither_pack(first, n, 1);
      e = launch_planes(side.fmt, !to_image, pack, dithered ? &dith : nullptr, n, most, stream, meter, gain);
    } else if (side.mix != nullptr) {
      MixPack pack;
      std::memset(&pack, 0, sizeof(pack));
      pack.src_channels = to_image ? side.channels : channels_;
      pack.dst_channels = to_image ? channels_ : side.channels;
      std::memcpy(pack.m, side.mix, sizeof(float) * side.channels * channels_);
      uint32_t most = 0;
      for (uint32_t j = 0; j < n; j++) {
        pack.s[j].frames = place(j, &pack.s[j].src, &pack.s[j].dst);
        most = std::max(most, pack.s[j].frames);
      }
      e = launch_mix(side.fmt, !to_image, pack, dithered ? &dith : nullptr, n, most, stream, meter, gain);
    } else {
      ConvertPack pack;
      std::memset(&pack, 0, sizeof(pack));
      uint64_t most = 0;
      for (uint32_t j = 0; j < n; j++) {
        // (a stream's frames are channels() samples one after the other; a channel that stands apart is every channels()-th)
        const uint64_t frames = place(j, &pack.s[j].src, &pack.s[j].dst);
        pack.s[j].n = apart != nullptr ? frames : frames * channels_;
        pack.s[j].step = apart != nullptr ? channels_ : 1;
        most = std::max(most, pack.s[j].n);
      }
      e = launch_convert(side.fmt, !to_image, pack, dithered ? &dith : nullptr, n, most, stream, meter, gain);
    }
    if (hip_failed(e, "kernel launch")) return SPEEXHIP_ERR_DEVICE;
  }
  return SPEEXHIP_ERR_SUCCESS;
}

}  // namespace speexhip
