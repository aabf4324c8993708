// sides_route.h -- the route of a formatted, mixed or sides call: host only, a pure function of what the sides are and
// what the state has on, checked row by row on the CPU (tools/san_host.cpp) like route_host_call (host_transfer.h) and
// plan_many_unit (many_plan.h).  The entry points (formats.cpp, many.cpp, bus.cpp, mixer.cpp) describe their call and carry out the
// answer.  They differ in small ways that their histories chose; each difference is one commented line below and a
// sentence in DESIGN.md ("The route of a formatted call").
#pragma once
#include "../../include/speexhip_resampler.h"

namespace speexhip {

struct SideKind {
  int fmt;       // SPEEXHIP_FMT_*
  bool mix;      // the side carries a matrix
  bool planar;   // side_planar(): layout planar AND more than one channel
  bool planes;   // host calls: given as plane pointers (CallSide::planes)
};
struct SidesState {
  bool dither, meter, gain;  // set_dither's kind is not NONE / set_meter / any stream's gain is on
  bool split;                // some stream's channels stand apart (the per-channel calls moved them)
  bool zero_mode;            // the zero fallback
  bool single_stream;        // a batch of one stream
  bool repeated;             // ManyEntry: the state is named by an earlier entry of the call
};
// the entry point that asks: process_sides_device, process_sides_host, planes_host_call, process_sides_host_chunks, an
// entry of many_run, process_bus_device, a leg of a mixer call (mixer.cpp: `out` is the leg's float image, interleaved F32)
enum class SidesForm { Device, Host, PlanesHost, Chunks, ManyEntry, Bus, MixerLeg };

struct SidesRoute {
  // SPEEXHIP_ERR_SUCCESS, or the code the call returns before it touches anything.  late (Host only): the code is returned
  // behind the same-bytes shortcut and the choice of the device instead of in front of them.
  int refuse = SPEEXHIP_ERR_SUCCESS;
  bool refuse_late = false;
  // Int16Call / FloatCall: an existing call on the caller's own bytes; PlanarFloatCall: process_planar_device on them;
  // Images: the float call on float images, between the passes; OwnCalls: the separate calls of the next form down
  // (a chunk or an entry at a time), which ask again.
  enum Kind { Int16Call, FloatCall, PlanarFloatCall, Images, OwnCalls } kind = Images;
  // Int16Call / FloatCall of the host forms: the existing HOST call (process_host, process_host_chunks) on the caller's
  // buffers -- nothing is staged here
  bool direct = false;
  bool pass_in = false, pass_out = false;  // before "the input is present and not empty", which stays a run-time fact
  enum Finish { Nothing, MeterImage, GainImage } finish = Nothing;  // who finishes a result that no pass writes
  float finish_scale = 1.0f;               // what the stored value is judged at: 32768 for F32N on its own bytes
  // what moves behind the call (Bus: the bus position and the bus totals in the place of the streams')
  bool moves_dither = false, counts_meter = false, moves_gain = false;
  // ManyEntry, MixerLeg: the entry joins a launch group.  Chunks: the chunks share their launches (a direct call whose
  // state process_host_chunks serves chunk by chunk does not).
  bool fusable = false;
};

namespace sides_detail {
inline bool is_float(int fmt) { return fmt == SPEEXHIP_FMT_F32 || fmt == SPEEXHIP_FMT_F32N; }
// The calls that are an existing call on the same bytes: nothing is converted, nothing extra launched.  (F32N -> F32N: a
// power-of-two scale commutes exactly with the FIR.)  S16 -> S16 is no such call once the output side has work to do
// (`busy`: dither, meter or gain) -- it runs as the float call between its two passes.
inline bool same_bytes(const SideKind &in, const SideKind &out, bool busy) {
  if (in.mix || out.mix || in.fmt != out.fmt || in.planar || out.planar) return false;
  return in.fmt == SPEEXHIP_FMT_S16 ? !busy : is_float(in.fmt);
}
// a side passes through an image unless it has no matrix and its storage IS the image (interleaved F32)
inline bool side_passes(const SideKind &side) { return side.mix || side.fmt != SPEEXHIP_FMT_F32 || side.planar; }
inline SidesRoute refused(int code, bool late = false) {
  SidesRoute r;
  r.refuse = code;
  r.refuse_late = late;
  return r;
}
// the existing call on the same bytes, and who finishes its result
inline SidesRoute on_same_bytes(const SideKind &in, const SidesState &st, bool finish) {
  SidesRoute r;
  r.kind = in.fmt == SPEEXHIP_FMT_S16 ? SidesRoute::Int16Call : SidesRoute::FloatCall;
  if (finish) {
    r.finish = st.gain ? SidesRoute::GainImage : SidesRoute::MeterImage;  // (gain_image judges its product too)
    r.finish_scale = in.fmt == SPEEXHIP_FMT_F32N ? 32768.0f : 1.0f;
    r.counts_meter = st.meter;
    r.moves_gain = st.gain;
  }
  r.moves_dither = st.dither;  // (the float pairs, written as ever, still count their frames)
  return r;
}
// the float call between the passes
inline SidesRoute on_images(const SideKind &in, const SideKind &out, const SidesState &st) {
  SidesRoute r;
  r.kind = SidesRoute::Images;
  r.pass_in = side_passes(in);
  r.pass_out = side_passes(out);
  if (!r.pass_out && (st.meter || st.gain)) r.finish = st.gain ? SidesRoute::GainImage : SidesRoute::MeterImage;
  r.moves_dither = st.dither;
  r.counts_meter = st.meter;
  r.moves_gain = st.gain;
  return r;
}
}  // namespace sides_detail

inline SidesRoute route_sides_call(SidesForm form, const SideKind &in, const SideKind &out, const SidesState &st) {
  using namespace sides_detail;
  const bool mixed = in.mix || out.mix;
  // (what the meter asks of the routes a gained stream asks too: no shortcut past the output side)
  const bool meter = st.meter || st.gain;
  // Channels that stand apart produce different numbers of frames: neither an output frame of a matrix nor a dither
  // position nor a stream of samples to meter nor a frame index of a gain is defined.
  const bool split_undefined = st.split && (st.dither || mixed || meter);
  switch (form) {
    case SidesForm::Device: {
      // Device: a split state is served only when it is one stream
      if (split_undefined || (st.split && !st.single_stream)) return refused(SPEEXHIP_ERR_BAD_STATE);
      if (same_bytes(in, out, st.dither || meter)) return on_same_bytes(in, st, meter);
      // Device: the planar float call on the same bytes, only when not split and with neither meter nor gain on (then the
      // pairs run between planes_in and the metered or gained planes_out); it still moves the dither position
      if (in.planar && out.planar && !mixed && in.fmt == out.fmt && is_float(in.fmt) && !st.split && !meter) {
        SidesRoute r;
        r.kind = SidesRoute::PlanarFloatCall;
        r.moves_dither = st.dither;
        return r;
      }
      return on_images(in, out, st);
    }
    case SidesForm::Host: {
      if (in.planar || out.planar) return route_sides_call(SidesForm::PlanesHost, in, out, st);
      // Host: a split state with dither, meter or gain and no matrix is refused in front of the shortcut ...
      if (split_undefined && !mixed) return refused(SPEEXHIP_ERR_BAD_STATE);
      // Host: the shortcut to process_host only with meter and gain off (process_host serves a split state itself); with
      // either on the float pairs go on to the device form, which finishes its own same-bytes route
      if (same_bytes(in, out, st.dither) && !meter) {
        SidesRoute r = on_same_bytes(in, st, false);
        r.direct = true;
        return r;
      }
      // Host: ... one with a matrix behind it and behind the choice of the device
      if (st.split && mixed) return refused(SPEEXHIP_ERR_BAD_STATE, true);
      return route_sides_call(SidesForm::Device, in, out, st);
    }
    case SidesForm::PlanesHost:
      if (split_undefined) return refused(SPEEXHIP_ERR_BAD_STATE);
      return route_sides_call(SidesForm::Device, in, out, st);
    case SidesForm::Chunks: {
      if (split_undefined) return refused(SPEEXHIP_ERR_BAD_STATE);
      const bool same = same_bytes(in, out, st.dither || meter), own_calls = st.split || st.zero_mode;
      // Chunks: the rare states take the separate calls, unless process_host_chunks serves them on the same bytes
      if (own_calls && (!same || meter)) {
        SidesRoute r;
        r.kind = SidesRoute::OwnCalls;
        return r;
      }
      if (same && !meter) {  // process_host_chunks, for every state
        SidesRoute r = on_same_bytes(in, st, false);
        r.direct = true;
        r.fusable = !own_calls;
        return r;
      }
      // Chunks: no planar float call -- planar float pairs run between their passes.  On the same bytes with meter or gain
      // on: staged without passes, finished once over all chunks.
      SidesRoute r = same ? on_same_bytes(in, st, true) : on_images(in, out, st);
      r.fusable = true;
      return r;
    }
    case SidesForm::ManyEntry: {
      SidesRoute r;
      r.kind = SidesRoute::OwnCalls;
      // ManyEntry: a launch group serves sides that are interleaved (or of one channel), in one buffer each, without matrix
      if (in.planar || out.planar || mixed || in.planes || out.planes) return r;
      // ManyEntry: a metered result that no pass of the group writes -- F32, or the float call on the same bytes -- takes
      // its own call, which runs meter_image behind it; a gained one stays fused
      if (st.meter && (out.fmt == SPEEXHIP_FMT_F32 || (in.fmt == out.fmt && out.fmt == SPEEXHIP_FMT_F32N))) return r;
      // ManyEntry: the rare states keep their own call's rules
      if (st.repeated || !st.single_stream || st.split || st.zero_mode) return r;
      r = same_bytes(in, out, st.dither || meter) ? on_same_bytes(in, st, false) : on_images(in, out, st);
      // ManyEntry: a gained float result that no pass writes is multiplied by gain_image in the group; nothing is judged
      // there, so the scale stays 1
      if (st.gain && !r.pass_out && r.kind != SidesRoute::Int16Call) r.finish = SidesRoute::GainImage;
      r.counts_meter = st.meter;
      r.moves_gain = st.gain;
      r.fusable = true;
      return r;
    }
    case SidesForm::Bus: {
      // Bus: a matrix on the sum is an argument error, found with the arguments; a bus has no frame to sum channels
      // that stand apart in
      if (out.mix) return refused(SPEEXHIP_ERR_INVALID_ARG);
      if (st.split) return refused(SPEEXHIP_ERR_BAD_STATE);
      // Bus: no same-bytes and no planar float route -- the streams always land in the state's image, where bus_sum
      // reads them; pass_out is the pass over the image of the buses
      SidesRoute r = on_images(in, out, st);
      // Bus: an F32 interleaved bus side is written by bus_sum and only ever read by meter_image: the streams were
      // gained before they were summed
      r.finish = !r.pass_out && st.meter ? SidesRoute::MeterImage : SidesRoute::Nothing;
      // Bus: gain moves; the bus position and the bus totals move in the place of the streams'
      return r;
    }
    case SidesForm::MixerLeg: {
      // MixerLeg: a leg is one interleaved host buffer (or one channel) without matrix, of a single-stream state that no
      // earlier slot names -- argument errors, found with the arguments
      if (in.mix || in.planar || in.planes || !st.single_stream || st.repeated) return refused(SPEEXHIP_ERR_INVALID_ARG);
      // MixerLeg: a bus has no frame to sum channels that stand apart in
      if (st.split) return refused(SPEEXHIP_ERR_BAD_STATE);
      // MixerLeg: no same-bytes route -- the leg's result is always its float image of the call, where the bus-sum kernel
      // reads it: no output pass, nothing finished in place (the kernel gains the leg as it sums it)
      SidesRoute r;
      r.kind = SidesRoute::Images;
      r.pass_in = side_passes(in);
      // MixerLeg: gain moves; the leg's own dither position and meter totals do not -- nothing of a leg is encoded.  The
      // zero fallback joins its launch group like any leg
      r.moves_gain = st.gain;
      r.fusable = true;
      return r;
    }
  }
  return refused(SPEEXHIP_ERR_INVALID_ARG);
}

}  // namespace speexhip
