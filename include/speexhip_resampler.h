/*
 * speexhip_resampler.h -- C ABI of libspeexhip.so, the MI355X (gfx950) implementation of the
 * Speex polyphase-FIR resampler hot path.
 *
 * This is the drop-in boundary for the reference's FFI layer: the five functions the
 * reference exports from its WASM module (scripts/build_emscripten.sh:20) and calls from
 * src/index.ts:6-16, with the signatures of deps/speex/speex_resampler.h.  Symbols carry the
 * prefix `speexhip_` (the reference renames its own with RANDOM_PREFIX for the same reason,
 * deps/speex/speex_resampler.h:50-79).  Plain pointers and sizes only; no HIP/torch types.
 *
 * Numerical contract: output int16 PCM is within +-1 LSB of the reference on the same input
 * (SPEEXHIP_MODE_FAST_FIXED, the default, and SPEEXHIP_MODE_FAST) or bit-identical to it (SPEEXHIP_MODE_EXACT).  Stream
 * bookkeeping (frames consumed / produced per call, resample.c:878-902,968-1036) is always
 * identical to the reference.
 *
 * There is NO CPU fallback: without a usable gfx950 device speexhip_resampler_init() fails
 * with SPEEXHIP_ERR_DEVICE.
 */
#ifndef SPEEXHIP_RESAMPLER_H
#define SPEEXHIP_RESAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPEEXHIP_API __attribute__((visibility("default")))

/* Error codes: 0..5 are the reference's enum (deps/speex/speex_resampler.h:104-113);
 * 6 is new and reports a HIP runtime/device failure; 7 is returned by the ..._take calls only. */
enum {
  SPEEXHIP_ERR_SUCCESS = 0,
  SPEEXHIP_ERR_ALLOC_FAILED = 1,
  SPEEXHIP_ERR_BAD_STATE = 2,
  SPEEXHIP_ERR_INVALID_ARG = 3,
  SPEEXHIP_ERR_PTR_OVERLAP = 4,
  SPEEXHIP_ERR_OVERFLOW = 5,
  SPEEXHIP_ERR_DEVICE = 6,
  SPEEXHIP_ERR_NO_BLOCK = 7,   /* ..._take: no pinned result block free right now; the state is untouched */
  SPEEXHIP_ERR_MAX_ERROR
};

enum {
  SPEEXHIP_MODE_FAST = 0,      /* +-1 LSB; the filters the reference sums in fp64 (quality 9, 10) in fp64.  Launches that
                                  cannot fill the chip may split an output's sum over several waves (tap-range shares): up
                                  to 2x faster on one-stream calls of long decimators, but the last bit of a sample then
                                  depends on how the stream was cut into calls and on what shared its launch.  Opt-in
                                  since round 6 (set_mode, or SPEEXHIP_MODE=fast) */
  SPEEXHIP_MODE_EXACT = 1,     /* bit-identical arithmetic order */
  SPEEXHIP_MODE_FAST_F32 = 2,  /* FAST with one fp32 FMA chain for every filter (the fast path of rounds 1-3):
                                  narrower than the reference's accumulator at quality 9 and 10, still +-1 LSB */
  SPEEXHIP_MODE_FAST_FIXED = 3 /* THE DEFAULT (round 6).  FAST with a pinned summation order: no tap-range shares, the one
                                  launch-time choice that re-associates an output's sum.  Like the reference (whose output
                                  for 64 KiB chunks equals its output for one chunk) the bytes of a stream do
                                  not depend on how it is cut into chunks, on how many streams share a launch or on the
                                  GPU's size; +-1 LSB of the reference.  Costs nothing on launches that fill the chip
                                  (every BASELINE config); one-stream calls of long decimators run
                                  at the unshared speed (48k -> 11.025k stereo: 30 us against 14 for a 2^20-frame call) */
};

/* Which of the reference's inner kernels the (rates, quality) pair selects
 * (deps/speex/resample.c:647-648,682-698). */
enum {
  SPEEXHIP_KERNEL_DIRECT_SINGLE = 0,
  SPEEXHIP_KERNEL_DIRECT_DOUBLE = 1,
  SPEEXHIP_KERNEL_INTERPOLATE_SINGLE = 2,
  SPEEXHIP_KERNEL_INTERPOLATE_DOUBLE = 3
};

typedef struct SpeexHipResamplerState_ SpeexHipResamplerState;
typedef struct SpeexHipBatch_ SpeexHipBatch;

/* ------------------------------------------------------------------------------------------
 * The reference surface (what src/index.ts binds).
 * ---------------------------------------------------------------------------------------- */

/* Replaces speex_resampler_init (deps/speex/speex_resampler.h:127-131, resample.c:794).
 * Returns NULL and sets *err (INVALID_ARG for nb_channels==0, a zero rate, quality<0 or >10;
 * DEVICE when no gfx950 device is usable; ALLOC_FAILED). */
SPEEXHIP_API SpeexHipResamplerState *speexhip_resampler_init(uint32_t nb_channels, uint32_t in_rate,
                                                             uint32_t out_rate, int quality,
                                                             int *err);

/* Which GPU a state lives on (round 5).  The reference's model is many SpeexResampler instances in one process
 * (src/index.ts:18-45: one shared module, one state per instance); on a node with several MI355X the states of
 * one process spread over them by a process-wide rule read from the environment when a state is made:
 *   SPEEXHIP_DEVICE=k         every state on device k
 *   SPEEXHIP_DEVICES=all      every new state on the device with the fewest live states (round 6; ties in the order k mod
 *                             n, k + 1 mod n, ... for state number k: a fresh process deals its states round-robin)
 *   SPEEXHIP_DEVICES=0,2,5    ... on the (k mod 3)-th listed device
 *   neither                   the calling thread's current HIP device (the behaviour before round 5)
 * speexhip_resampler_init / _init_frac / speexhip_batch_init follow the rule; the ..._init_on forms name the device
 * (device < 0 = the rule).  A state's calls may come from any thread with any current device: every entry point
 * switches to the state's device and back.  Init fails with SPEEXHIP_ERR_DEVICE for a device the node does not have.
 * (SPEEXHIP_ALIAS_DEVICES=n, tests only: n logical devices, logical d on physical d mod the real count -- pools, table
 * caches, streams and this rule key on the logical ordinal, so a 1-GPU box walks the multi-device paths.) */
SPEEXHIP_API int speexhip_device_count(void);   /* usable logical devices; <= 0: none (no CPU fallback) */
/* The one-time costs of a process that the first states would otherwise pay -- the runtime's start (90-180 ms), the
 * pool's four shared streams per device (20 + 3 x 8 ms), the copy engines' first copy (8 ms); a state itself is 0.04 ms
 * of filter design and 0.2 ms of uploads -- paid now, on `device` or (device < 0) on every device the placement rule
 * can choose.  Blocking; call it from a thread of its own beside the application's other start-up work.  The N-API addon
 * does, at import, and SpeexResampler.initPromise resolves behind it -- where the reference compiles its WASM module
 * (src/index.ts:18-19, :31).  Optional: without it the first states pay as before.  Returns an error code. */
SPEEXHIP_API int speexhip_warmup(int device);
SPEEXHIP_API SpeexHipResamplerState *speexhip_resampler_init_on(int device, uint32_t nb_channels, uint32_t in_rate,
                                                                uint32_t out_rate, int quality, int *err);

/* Replaces speex_resampler_destroy (speex_resampler.h:157, resample.c:868). */
SPEEXHIP_API void speexhip_resampler_destroy(SpeexHipResamplerState *st);

/* Extents -- of this call and of every process call below, host or device pointers, one state or a batch.
 * A length is a uint32 count of frames and a stride a uint64 count of samples.  A single call serves
 *   *in_len <= 2^32 - 1 - 2^16 - den_rate   and as many output frames, counted as what the input can make within
 *   *out_len (an *out_len beyond that which the input cannot fill is no reason to refuse),
 * lengths from 2^31 frames included, and any sample index, byte offset or distance between streams and planes that
 * follows from them -- beyond 2^31 and 2^32 in one call.  Up to there every quantity of a call is held in a type that
 * takes it ("Extents", lists them with the test that reaches each): the planner counts in 64 bits,
 * the position a call leaves is smaller than one input block, the kernels form every address in 64 bits from 32-bit
 * frame counts, and the one place that narrows frames to int32 -- the pieces of a large ..._take call -- is entered
 * below 2^30 frames only.  Beyond, two kinds of 32-bit sums wrap -- the launchers round a count of frames or periods up
 * to whole tiles, and the slide kernels end a call's outputs at k_shift + n_out (k_shift < den_rate) -- so a call that
 * asks for more returns SPEEXHIP_ERR_OVERFLOW: the first thing every entry point does after checking its arguments,
 * with the stream's positions, history and dither position, the lengths and the output as they were (in a
 * many-states call: that entry's code).  The chunk calls, which add lengths up, refuse more than 0x7fffffff frames in
 * or out in all (OVERFLOW, before anything runs). */

/* Replaces speex_resampler_process_interleaved_int (speex_resampler.h:217-221,
 * resample.c:1061).  `in`/`out` are HOST pointers to interleaved s16 frames; *in_len /
 * *out_len are frames per channel: in = available / capacity, out = consumed / written.
 * Synchronous.  `in` may be NULL (zeros), as in the reference. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_int(SpeexHipResamplerState *st,
                                                            const int16_t *in, uint32_t *in_len,
                                                            int16_t *out, uint32_t *out_len);

/* Float I/O entry point: replaces speex_resampler_process_interleaved_float
 * (speex_resampler.h:202-206, resample.c:1038-1059 -> :927-963).  Same stream state as the
 * int16 call (int and float calls may be mixed); samples are not rounded or saturated, and a
 * 160-frame input block is not limited to 1024 outputs (resample.c:943 vs :982-991). */
SPEEXHIP_API int speexhip_resampler_process_interleaved_float(SpeexHipResamplerState *st,
                                                              const float *in, uint32_t *in_len,
                                                              float *out, uint32_t *out_len);

/* Replaces speex_resampler_get_rate (speex_resampler.h:237-239, resample.c:1089). */
SPEEXHIP_API void speexhip_resampler_get_rate(SpeexHipResamplerState *st, uint32_t *in_rate,
                                              uint32_t *out_rate);

/* ------------------------------------------------------------------------------------------
 * The rest of the reference's C API around the path: mid-stream control.
 * Not reachable from src/index.ts, but part of deps/speex/speex_resampler.h.  A change of the
 * filter length keeps the stream continuous exactly as the reference does: the history is
 * re-aligned and, when the filter gets shorter, the frames that no longer fit are kept as
 * pending input ("magic samples", resample.c:727-782, 904-922).  These calls wait for the
 * device (they touch the stream history) -- control plane, not hot path.
 * ---------------------------------------------------------------------------------------- */

/* Replaces speex_resampler_init_frac (speex_resampler.h:133-150, resample.c:799). */
SPEEXHIP_API SpeexHipResamplerState *speexhip_resampler_init_frac(uint32_t nb_channels,
                                                                  uint32_t ratio_num, uint32_t ratio_den,
                                                                  uint32_t in_rate, uint32_t out_rate,
                                                                  int quality, int *err);
/* Replace speex_resampler_set_rate / set_rate_frac / get_ratio (speex_resampler.h:223-262,
 * resample.c:1084-1151).  OVERFLOW when a phase numerator cannot be carried to the new
 * denominator: as in the reference (:1119-1134) get_rate / get_ratio then report the NEW rates and
 * a repeat of the same call returns SUCCESS without doing anything; unlike the reference, which
 * goes on with phase numerators on two denominators, processing continues consistently with the
 * OLD ratio and filter until a later filter change succeeds -- from then on get_rate / get_ratio
 * report the filter in force again. */
SPEEXHIP_API int speexhip_resampler_set_rate(SpeexHipResamplerState *st, uint32_t in_rate, uint32_t out_rate);
SPEEXHIP_API int speexhip_resampler_set_rate_frac(SpeexHipResamplerState *st, uint32_t ratio_num,
                                                  uint32_t ratio_den, uint32_t in_rate, uint32_t out_rate);
SPEEXHIP_API void speexhip_resampler_get_ratio(SpeexHipResamplerState *st, uint32_t *ratio_num,
                                               uint32_t *ratio_den);
/* Replace speex_resampler_set_quality / get_quality (speex_resampler.h:264-277, resample.c:1153-1168). */
SPEEXHIP_API int speexhip_resampler_set_quality(SpeexHipResamplerState *st, int quality);
SPEEXHIP_API void speexhip_resampler_get_quality(SpeexHipResamplerState *st, int *quality);
/* Replace speex_resampler_get_input_latency / get_output_latency (speex_resampler.h:305-315,
 * resample.c:1190-1198). */
SPEEXHIP_API int speexhip_resampler_get_input_latency(SpeexHipResamplerState *st);
SPEEXHIP_API int speexhip_resampler_get_output_latency(SpeexHipResamplerState *st);
/* Replace speex_resampler_skip_zeros / reset_mem (speex_resampler.h:317-332,
 * resample.c:1200-1220).  reset_mem restates the reference's multi-channel behaviour: its
 * single memset run covers channels*(filt_len-1) floats of a buffer whose channel lines are
 * mem_alloc_size apart, so only the first channel(s) are silenced. */
SPEEXHIP_API int speexhip_resampler_skip_zeros(SpeexHipResamplerState *st);
SPEEXHIP_API int speexhip_resampler_reset_mem(SpeexHipResamplerState *st);

/* Replace speex_resampler_process_int / _process_float (speex_resampler.h:169-191,
 * resample.c:968-1036, 927-963): ONE channel of the state, host buffers whose consecutive samples
 * are `input stride` / `output stride` apart (speex_resampler_set/get_input/output_stride,
 * speex_resampler.h:285-307, resample.c:1170-1188; both 1 after init, resample.c:842-843).  As in
 * the reference every channel keeps its own position (last_sample / samp_frac_num /
 * magic_samples, resample.c:135-137), so channels may be advanced unevenly; an interleaved call on
 * such a state then handles channel after channel with the caller's lengths and reports the
 * lengths of the last one (resample.c:1061-1082).  These run the bit-exact kernel on one channel
 * in either mode. */
SPEEXHIP_API int speexhip_resampler_process_int(SpeexHipResamplerState *st, uint32_t channel_index,
                                                const int16_t *in, uint32_t *in_len, int16_t *out,
                                                uint32_t *out_len);
SPEEXHIP_API int speexhip_resampler_process_float(SpeexHipResamplerState *st, uint32_t channel_index,
                                                  const float *in, uint32_t *in_len, float *out,
                                                  uint32_t *out_len);
SPEEXHIP_API void speexhip_resampler_set_input_stride(SpeexHipResamplerState *st, uint32_t stride);
SPEEXHIP_API void speexhip_resampler_get_input_stride(SpeexHipResamplerState *st, uint32_t *stride);
SPEEXHIP_API void speexhip_resampler_set_output_stride(SpeexHipResamplerState *st, uint32_t stride);
SPEEXHIP_API void speexhip_resampler_get_output_stride(SpeexHipResamplerState *st, uint32_t *stride);

/* When a filter change cannot build its filter -- the new filter length overflows
 * (resample.c:620-621, 641-655) or memory runs out (here: device memory) -- the reference keeps
 * its old filter length and history, keeps the NEW rates / ratio / quality, installs
 * resampler_basic_zero (resample.c:561-591, 785-791) and returns RESAMPLER_ERR_ALLOC_FAILED: from
 * then on every processing call writes zeros with the right lengths, moves the counters, and
 * returns ALLOC_FAILED too, until a later set_rate / set_quality succeeds.  Same here. */

/* Replaces speex_resampler_strerror (speex_resampler.h:338, resample.c:1222-1239); same
 * strings for codes 0..4, the reference's "Unknown error..." text for 5 and out-of-range
 * codes, and a HIP message for SPEEXHIP_ERR_DEVICE. */
SPEEXHIP_API const char *speexhip_resampler_strerror(int err);

/* ------------------------------------------------------------------------------------------
 * Extensions (not part of the reference surface).
 * ---------------------------------------------------------------------------------------- */

/* Same call with DEVICE pointers (inputs/outputs resident in HBM).  The work is enqueued on
 * `hip_stream` (a hipStream_t passed as void*; NULL = the default stream) and the call
 * returns without waiting for the GPU.  The stream position advances on the host at once
 * (it is integer arithmetic, independent of the audio), so *in_len / *out_len are final on
 * return.  d_in must stay valid until the stream has executed the call.  Calls on one state are
 * ordered: the next call -- on whatever stream -- first waits for this one on the device (an event
 * recorded on `hip_stream` at that moment), and control calls and destroy wait for `hip_stream` on
 * the host (for this state's last call only, never for the device: other states' launches keep
 * running).  `hip_stream` must therefore stay valid until the state's NEXT call of any kind --
 * or be handed back with speexhip_resampler_release_stream() before the caller destroys it (a
 * destroyed stream's handle cannot be recognised afterwards: this runtime dereferences it). */
SPEEXHIP_API int speexhip_resampler_process_interleaved_int_device(SpeexHipResamplerState *st,
                                                                   const int16_t *d_in,
                                                                   uint32_t *in_len, int16_t *d_out,
                                                                   uint32_t *out_len,
                                                                   void *hip_stream);

/* The host-buffer calls with the result left in a PINNED block owned by the caller afterwards (release it with
 * speexhip_block_release).  Same counters, same samples as speexhip_resampler_process_interleaved_int / _float with
 * *out_len as the capacity; *out_block = NULL when no frame was produced.  The kernel writes the block straight through
 * PCIe, so the samples cross memory once on their way out, not twice (device or pinned buffer, then a copy into the
 * caller's buffer).  Blocks are carved out of one pinned slab (SPEEXHIP_TAKE_MB, default 64 MiB, made by the first
 * such call), never allocated per call: while the caller holds so many blocks that none fits, the call returns
 * SPEEXHIP_ERR_NO_BLOCK WITHOUT touching the state, and the caller makes the copying call instead.  The N-API addon
 * hands the block to JavaScript as an external Buffer: src/index.ts:111-115 returns a fresh Buffer the caller owns,
 * and so does it. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_int_take(SpeexHipResamplerState *st, const int16_t *in,
                                                                 uint32_t *in_len, uint32_t *out_len,
                                                                 int16_t **out_block);
SPEEXHIP_API int speexhip_resampler_process_interleaved_float_take(SpeexHipResamplerState *st, const float *in,
                                                                   uint32_t *in_len, uint32_t *out_len,
                                                                   float **out_block);
SPEEXHIP_API void speexhip_block_release(void *block);

/* Pinned blocks for INPUT (round 6) -- the mirror of the ..._take calls.  speexhip_block_acquire(bytes) hands the caller a
 * block of the same pinned slabs to FILL (NULL: none free right now, or SPEEXHIP_TAKE_MB=0; use an ordinary buffer then);
 * speexhip_block_release gives it back, any time after the calls that read it have returned.  Every host-buffer entry
 * point -- process_interleaved_int / _float, the ..._take forms, process_chunks_*, process_many_* -- recognises such a
 * block (and, for buffers of 256 KB and more, memory the caller pinned itself with hipHostMalloc / hipHostRegister) as
 * its input or output and uses it IN PLACE: the kernel reads the chunk through PCIe while it writes the result through
 * PCIe -- both directions of the link at once, one launch, no staging copy -- where a pageable buffer goes through the
 * runtime's staged copy first.  Bytes and counters are those of the same call on pageable buffers.  In the reference this
 * is the copy of the chunk into the WASM module's heap (src/index.ts:71-92) that a caller avoids by decoding straight
 * into the block.  A block may be refilled as soon as the call that read it has returned (the host-buffer calls are
 * synchronous). */
SPEEXHIP_API void *speexhip_block_acquire(uint64_t bytes);

/* The caller is about to destroy the stream of this state's last device-pointer call (one stream per
 * request, say): what that call still has in flight is ordered behind an event of the state's own and
 * the stream is forgotten -- later calls, control calls and destroy wait for the event instead.  Costs one
 * hipEventRecord (about 3 us of stream time on this stack, which is why it is not done after every call). */
SPEEXHIP_API int speexhip_resampler_release_stream(SpeexHipResamplerState *st);

SPEEXHIP_API int speexhip_resampler_process_interleaved_float_device(SpeexHipResamplerState *st,
                                                                     const float *d_in,
                                                                     uint32_t *in_len, float *d_out,
                                                                     uint32_t *out_len,
                                                                     void *hip_stream);

/* Chunk coalescing: n_chunks CONSECUTIVE host-buffer calls on one stream as
 * ONE transfer + ONE launch.  in[i] / in_len[i] / out_len[i] are what call i of
 * speexhip_resampler_process_interleaved_int would be given (in[i] may be NULL = silence); on
 * return in_len[i] / out_len[i] hold what call i consumed / wrote, and `out` holds the calls'
 * outputs back to back (so it needs room for the sum of the capacities).  Bytes and counters
 * are exactly those of the n_chunks separate calls, including frames a capacity-bound call
 * leaves unconsumed: the host plans every call in integer arithmetic first and only the frames
 * really consumed travel to the GPU. */
SPEEXHIP_API int speexhip_resampler_process_chunks_int(SpeexHipResamplerState *st, uint32_t n_chunks,
                                                       const int16_t *const *in, uint32_t *in_len,
                                                       int16_t *out, uint32_t *out_len);
SPEEXHIP_API int speexhip_resampler_process_chunks_float(SpeexHipResamplerState *st, uint32_t n_chunks,
                                                         const float *const *in, uint32_t *in_len,
                                                         float *out, uint32_t *out_len);

/* Many states, one call (round 5; SURVEY 8b: "a batched entry (array of states/buffers) for multi-stream launches").
 * st[i] is an independent single-stream state -- what one `new SpeexResampler(...)` of the reference holds -- and
 * (in[i], in_len[i], out[i], out_len[i]) are the arguments its own speexhip_resampler_process_interleaved_int call
 * would get: HOST pointers, frames per channel, in = available / capacity, out = consumed / written.  Samples and
 * counters of every state are exactly those of the n separate calls; codes[i] (may be NULL) receives call i's return
 * code and the function returns the first one that is not SUCCESS.  What changes is the shape on the GPU: per device
 * ONE transfer in, ONE launch per <= 32 states that share (rates, quality, channels, mode), ONE transfer out -- the
 * shape BASELINE configs[4] is quoted on -- and states that live on different GPUs (SPEEXHIP_DEVICES=all) run side by
 * side, each over its own PCIe link.  States whose channels the per-channel calls moved apart, states in the zero
 * fallback and a state named twice take their own single call, in order.  Synchronous; a state must not be used
 * by another thread meanwhile. */
SPEEXHIP_API int speexhip_resampler_process_many_int(uint32_t n, SpeexHipResamplerState *const *st,
                                                     const int16_t *const *in, uint32_t *in_len,
                                                     int16_t *const *out, uint32_t *out_len, int *codes);
SPEEXHIP_API int speexhip_resampler_process_many_float(uint32_t n, SpeexHipResamplerState *const *st,
                                                       const float *const *in, uint32_t *in_len,
                                                       float *const *out, uint32_t *out_len, int *codes);

/* What the next processing call WOULD consume and produce for (in_len, out_capacity), without
 * touching the state: the counters are integer functions of the stream position alone, so a
 * binding can size its output buffer exactly before the call: the processing calls write
 * exactly `produced` frames, so a buffer of that size suffices even though *out_len is larger
 * (the N-API addon does this; do NOT pass `produced` as the capacity instead -- a tighter
 * capacity can end the block loop before trailing input is consumed).  float_entry selects the
 * float call's rules. */
SPEEXHIP_API int speexhip_resampler_peek(SpeexHipResamplerState *st, uint32_t in_len, uint32_t out_capacity,
                                         int float_entry, uint32_t *consumed, uint32_t *produced);

/* SPEEXHIP_MODE_FAST_FIXED (default; +-1 LSB, bytes a function of the stream alone), SPEEXHIP_MODE_FAST (+-1 LSB, faster on
 * small launches of long filters, bytes may depend on chunking), SPEEXHIP_MODE_EXACT (bit-identical arithmetic order,
 * slower) or SPEEXHIP_MODE_FAST_F32.  The environment variable SPEEXHIP_MODE=exact|fast|fast_f32|fast_fixed sets the
 * initial mode. */
SPEEXHIP_API int speexhip_resampler_set_mode(SpeexHipResamplerState *st, int mode);

typedef struct SpeexHipInfo {
  uint32_t in_rate, out_rate;
  uint32_t num_rate, den_rate;   /* gcd-reduced ratio, resample.c:1125-1128 */
  uint32_t nb_channels;
  int32_t quality;
  uint32_t filt_len;             /* taps per output, resample.c:616-625 */
  uint32_t oversample;           /* resample.c:615,626-635 */
  uint32_t sinc_table_length;    /* floats, resample.c:652,657 */
  int32_t kernel;                /* SPEEXHIP_KERNEL_* */
  int32_t mode;                  /* SPEEXHIP_MODE_* */
  int32_t fast_path;             /* what the fast modes run for this configuration: 2 = period-lane
                                    kernel, 3 = small-ratio sliding-window kernel, 4 / 5 = their
                                    fp64-accumulate twins (FAST mode, quality 9 and 10), 0 = falls
                                    back to the exact kernel (exotic ratios) */
  int32_t last_sample;           /* stream position, resample.c:135 */
  uint32_t samp_frac_num;        /* stream phase, resample.c:136 */
  int32_t device;                /* HIP device ordinal the state lives on */
  uint32_t magic_samples;        /* pending frames buffered after the history, resample.c:137 */
  uint32_t block_in;             /* frames per block: mem_alloc_size-(filt_len-1), resample.c:935 */
  int32_t accumulate_bits;       /* accumulator of what the current mode runs for this filter: 32 (fp32 FMA chain;
                                    exact kernels of the single kinds) or 64 (v_fma_f64 fast kernels, fast_path 4 / 5;
                                    exact kernels of the double kinds: fp64 sums of fp32 products) */
} SpeexHipInfo;

SPEEXHIP_API int speexhip_resampler_get_info(SpeexHipResamplerState *st, SpeexHipInfo *info);
/* The same with the caller's sizeof(SpeexHipInfo): at most `struct_size` bytes are written, so a caller compiled
 * against an older header (the struct grows at its end: accumulate_bits came in 0.2) is not overrun.  ABI note:
 * 0.2 -> 0.3 adds entry points and SPEEXHIP_MODE_FAST_FIXED; SpeexHipInfo and the error codes are unchanged. */
SPEEXHIP_API int speexhip_resampler_get_info2(SpeexHipResamplerState *st, SpeexHipInfo *info, uint32_t struct_size);

/* Copies the last filt_len-1 consumed frames (interleaved float, the reference's `mem`: what
 * the next call's first outputs are computed from; resample.c:898-899) followed by the
 * magic_samples pending frames to the host.  dst holds (filt_len-1+magic_samples)*ch floats. */
SPEEXHIP_API int speexhip_resampler_get_history(SpeexHipResamplerState *st, float *dst);

/* Batched streams: n_streams independent resamplers with one shared (rates, quality,
 * channels) filter, processed by ONE launch per call.  Device pointers; stream s reads
 * d_in + s*in_stream_stride and writes d_out + s*out_stream_stride (strides in int16
 * elements).  in_len[s] / out_len[s] as in the single-stream call.  Asynchronous on
 * `hip_stream`. */
SPEEXHIP_API SpeexHipBatch *speexhip_batch_init(uint32_t n_streams, uint32_t nb_channels,
                                                uint32_t in_rate, uint32_t out_rate, int quality,
                                                int *err);
SPEEXHIP_API SpeexHipBatch *speexhip_batch_init_on(int device, uint32_t n_streams, uint32_t nb_channels,
                                                   uint32_t in_rate, uint32_t out_rate, int quality, int *err);
SPEEXHIP_API void speexhip_batch_destroy(SpeexHipBatch *b);
SPEEXHIP_API int speexhip_batch_set_mode(SpeexHipBatch *b, int mode);
SPEEXHIP_API int speexhip_batch_get_info(SpeexHipBatch *b, uint32_t stream, SpeexHipInfo *info);
SPEEXHIP_API int speexhip_batch_release_stream(SpeexHipBatch *b);  /* see speexhip_resampler_release_stream */
SPEEXHIP_API int speexhip_batch_process_interleaved_int_device(
    SpeexHipBatch *b, const int16_t *d_in, uint64_t in_stream_stride, uint32_t *in_len,
    int16_t *d_out, uint64_t out_stream_stride, uint32_t *out_len, void *hip_stream);

SPEEXHIP_API int speexhip_batch_process_interleaved_float_device(
    SpeexHipBatch *b, const float *d_in, uint64_t in_stream_stride, uint32_t *in_len, float *d_out,
    uint64_t out_stream_stride, uint32_t *out_len, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Planar audio: one plane per channel instead of interleaved frames (Web Audio's getChannelData,
 * ffmpeg's s16p / fltp, a tensor shaped (channels, time)).  A planar call IS the interleaved call
 * on the same frames: the same counters, the same samples in every mode, the same state left
 * behind -- so interleaved, planar and per-channel calls may be mixed freely on one state.  It runs
 * the same kernels as the interleaved call between two transposing passes on the device.
 *
 * Lengths are frames per channel, with the in / out meaning of the interleaved calls; strides are in
 * elements (samples of the call's type).  Planes need no alignment beyond their element type; any
 * plane stride >= the frame count serves.  speexhip_resampler_peek sizes the output planes exactly
 * as it sizes an interleaved buffer.
 *
 * Host planes (synchronous): in[c] / out[c] = plane of channel c; in == NULL is silence.  Returns
 * INVALID_ARG when out, an element of out or an element of in is NULL, PTR_OVERLAP when the frames
 * the call writes to an output plane overlap another plane of the call; the state is untouched in
 * both cases.  A state whose
 * channels the per-channel calls moved apart is handled channel after channel and reports the
 * lengths of the last channel, like the interleaved call.
 *
 * ABI note: 0.4 -> 0.5 adds these six entry points; SpeexHipInfo and the error codes are unchanged. */
SPEEXHIP_API int speexhip_resampler_process_planar_int(SpeexHipResamplerState *st, const int16_t *const *in,
                                                       uint32_t *in_len, int16_t *const *out, uint32_t *out_len);
SPEEXHIP_API int speexhip_resampler_process_planar_float(SpeexHipResamplerState *st, const float *const *in,
                                                         uint32_t *in_len, float *const *out, uint32_t *out_len);
/* Device planes (asynchronous on hip_stream, ordered like the interleaved device calls): plane c
 * starts at d_in + c * in_plane_stride / d_out + c * out_plane_stride; d_in == NULL is silence. */
SPEEXHIP_API int speexhip_resampler_process_planar_int_device(SpeexHipResamplerState *st, const int16_t *d_in,
                                                              uint64_t in_plane_stride, uint32_t *in_len,
                                                              int16_t *d_out, uint64_t out_plane_stride,
                                                              uint32_t *out_len, void *hip_stream);
SPEEXHIP_API int speexhip_resampler_process_planar_float_device(SpeexHipResamplerState *st, const float *d_in,
                                                                uint64_t in_plane_stride, uint32_t *in_len,
                                                                float *d_out, uint64_t out_plane_stride,
                                                                uint32_t *out_len, void *hip_stream);
/* ... of every stream of a batch: plane c of stream s starts at d_in + s * in_stream_stride +
 * c * in_plane_stride (a tensor shaped (batch, channels, time)); in_len / out_len hold one entry per stream. */
SPEEXHIP_API int speexhip_batch_process_planar_int_device(
    SpeexHipBatch *b, const int16_t *d_in, uint64_t in_stream_stride, uint64_t in_plane_stride, uint32_t *in_len,
    int16_t *d_out, uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len, void *hip_stream);
SPEEXHIP_API int speexhip_batch_process_planar_float_device(
    SpeexHipBatch *b, const float *d_in, uint64_t in_stream_stride, uint64_t in_plane_stride, uint32_t *in_len,
    float *d_out, uint64_t out_stream_stride, uint64_t out_plane_stride, uint32_t *out_len, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Sample formats: a formatted call names the format of its input and of its output independently
 * (a decoder's s16le in, Web Audio's float32 in +-1.0 out; 24-bit WAV / FLAC; 8-bit telephony -- for
 * G.711 mu-law / A-law see "Companded formats" below).
 * The library's internal unit is the reference's: one int16 step = 1.0f, what the float entry point
 * takes and gives.  Every format has a full scale FS:
 *
 *   format  storage                     FS    to the internal float x           from a FIR value y
 *   U8      1 byte, offset binary       2^7   (u - 128) * 256                   halfup(y / 256) + 128, clamped to 0..255
 *   S16     2 bytes LE                  2^15  s                                 halfup(y), clamped
 *   S24     3 bytes LE, packed          2^23  s / 256                           halfup(y * 256), clamped to -2^23..2^23-1
 *   S32     4 bytes LE                  2^31  float(s) (nearest even) / 65536   halfup(y * 65536), clamped
 *   F32     float, int16 units          2^15  as is                             as is
 *   F32N    float, +-1.0 full scale     1     x * 32768                         y / 32768
 *
 * halfup(v) = floor(v + 0.5), evaluated exactly (ties go up, negative ones too: -2.5 -> -2).  The
 * integer formats saturate, +inf / -inf go to their rails and NaN becomes the format's zero (128 for
 * U8); the float formats never saturate.  U8 and packed S24 buffers need no alignment, the others that
 * of their element.  Further formats, stated in sections of their own below: G.711 mu-law / A-law
 * ("Companded formats"), binary16 / bfloat16 in +-1.0 and big-endian S16 / S24 / S32 ("Half-float and
 * big-endian formats").
 *
 * A formatted call IS the float call (..._process_interleaved_float*) on the converted input,
 * followed by the output conversion: the same counters (speexhip_resampler_peek with float_entry = 1
 * sizes it), the same state and history left behind, in every mode; a state whose channels the
 * per-channel calls moved apart and the zero fallback behave as in the float call (the fallback's
 * silence is the format's zero).  Both conversions run on the device, either side of the float
 * call's own launch.  Three pairs launch nothing extra: S16 -> S16 is the int16 call, bit for bit and
 * with its counter rules; F32 -> F32 is the float call; F32N -> F32N is the float call on the same
 * bytes (a power-of-two scale commutes exactly with the FIR, short of overflow and underflow).
 * Formatted, interleaved, planar and per-channel calls may be mixed on one state.
 *
 * ABI note: 0.5 -> 0.6 adds the enum and these four entry points; SpeexHipInfo and the error codes
 * are unchanged. */
enum {
  SPEEXHIP_FMT_U8 = 0,
  SPEEXHIP_FMT_S16 = 1,
  SPEEXHIP_FMT_S24 = 2,
  SPEEXHIP_FMT_S32 = 3,
  SPEEXHIP_FMT_F32 = 4,
  SPEEXHIP_FMT_F32N = 5,
  /* companded formats ("Companded formats" below) start at 16; 6..15 stay invalid */
  SPEEXHIP_FMT_ULAW = 16,
  SPEEXHIP_FMT_ALAW = 17,
  /* half-float and big-endian formats ("Half-float and big-endian formats" below); 18, 19, 22, 23 stay invalid */
  SPEEXHIP_FMT_F16N = 20,
  SPEEXHIP_FMT_BF16N = 21,
  SPEEXHIP_FMT_S16BE = 24,
  SPEEXHIP_FMT_S24BE = 25,
  SPEEXHIP_FMT_S32BE = 26
};
/* Bytes of one sample of a format (host only); 0 for an unknown format. */
SPEEXHIP_API uint32_t speexhip_sample_bytes(int fmt);
/* Host buffers, synchronous; lengths are frames per channel as in the interleaved calls, in == NULL
 * is silence.  The raw bytes of both sides travel by the rule of the other host calls (pageable,
 * speexhip_block_acquire blocks and caller-pinned buffers used in place).  An unknown format or
 * out == NULL returns INVALID_ARG with the state untouched. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_fmt(SpeexHipResamplerState *st, int in_fmt, const void *in,
                                                            uint32_t *in_len, int out_fmt, void *out,
                                                            uint32_t *out_len);
/* Device buffers, asynchronous on hip_stream, ordered like the other device calls. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_fmt_device(SpeexHipResamplerState *st, int in_fmt,
                                                                   const void *d_in, uint32_t *in_len, int out_fmt,
                                                                   void *d_out, uint32_t *out_len, void *hip_stream);
/* ... of every stream of a batch; strides are in samples of the respective format (a packed S24
 * sample is 3 bytes). */
SPEEXHIP_API int speexhip_batch_process_interleaved_fmt_device(SpeexHipBatch *b, int in_fmt, const void *d_in,
                                                               uint64_t in_stream_stride, uint32_t *in_len,
                                                               int out_fmt, void *d_out, uint64_t out_stream_stride,
                                                               uint32_t *out_len, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Channel mixing: a mixed call is a formatted call whose input and output frames may hold another
 * number of channels than the state, with a matrix on that side.  The state keeps its channel count C
 * from init: the number of channels the FIR runs on and the history holds.  Each side names
 *
 *   in_channels,  in_mix   row-major C x in_channels floats in HOST memory; NULL = no input mix,
 *                          and in_channels must then equal C
 *   out_channels, out_mix  row-major out_channels x C floats in host memory; NULL = no output mix,
 *                          and out_channels must then equal C
 *
 * so the caller places the mix by choosing C: a downmix at the input (a state of the small count: the
 * FIR does the least work), an upmix at the output, or both (6 -> 2 -> 2).  The matrices are read
 * during the call and not kept.  The call is, in order: to_internal(in_fmt) per sample as in the
 * formatted call; the input mix per frame; THE FLOAT CALL of the state on that image (its counters,
 * and the same history and position left behind, in every mode); the output mix per frame;
 * from_internal(out_fmt) per sample (half-up, saturating, NaN -> the format's zero).
 *
 * The mix of one frame x of n samples by a matrix M, exactly: output o is
 *   acc = (double)M[o][0] * (double)x[0];  acc = acc + (double)M[o][i] * (double)x[i]  for i = 1 .. n-1
 * in ascending order, then one rounding of acc to fp32 (nearest even).  Every term is included (a zero
 * coefficient is not skipped) and nothing is clamped on the float image: only the integer output
 * formats saturate, in from_internal.
 *
 * Lengths are frames, as in the other calls; speexhip_resampler_peek with float_entry = 1 sizes a
 * mixed call.  A side with a matrix supports C <= 8 and a caller-side count of 1..8; anything else,
 * an unknown format or out == NULL returns INVALID_ARG.  With both matrices NULL the call IS the
 * formatted call (S16 -> S16 being the int16 call with its counter rules); with a matrix on either
 * side the float entry's rules hold for every format pair, S16 -> S16 included.  A state whose
 * channels the per-channel calls moved apart returns BAD_STATE (its channels produce different
 * numbers of frames, so an output frame is not defined).  The zero fallback behaves as in the float
 * call: its zeros go through the output mix and the output conversion.  Every argument error leaves
 * the state, *in_len and *out_len untouched.  Both mixes run on the device, each folded into the pass
 * that converts its side: a mixed call launches no more kernels than the formatted call.  Mixed,
 * formatted, interleaved, planar and per-channel calls may be mixed on one state.
 *
 * ABI note: 0.6 -> 0.7 adds these three entry points; SpeexHipInfo, the enum and the error codes are
 * unchanged. */
/* Host buffers, synchronous, routed like speexhip_resampler_process_interleaved_fmt; an input frame
 * holds in_channels samples of in_fmt, an output frame out_channels samples of out_fmt. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_mix(SpeexHipResamplerState *st, int in_fmt, uint32_t in_channels,
                                                            const float *in_mix, const void *in, uint32_t *in_len,
                                                            int out_fmt, uint32_t out_channels, const float *out_mix,
                                                            void *out, uint32_t *out_len);
/* Device buffers, asynchronous on hip_stream, ordered like the other device calls. */
SPEEXHIP_API int speexhip_resampler_process_interleaved_mix_device(SpeexHipResamplerState *st, int in_fmt,
                                                                   uint32_t in_channels, const float *in_mix,
                                                                   const void *d_in, uint32_t *in_len, int out_fmt,
                                                                   uint32_t out_channels, const float *out_mix,
                                                                   void *d_out, uint32_t *out_len, void *hip_stream);
/* ... of every stream of a batch; strides are in samples of the respective format, a frame of a side
 * holds that side's channel count, and the one pair of matrices serves all streams. */
SPEEXHIP_API int speexhip_batch_process_interleaved_mix_device(SpeexHipBatch *b, int in_fmt, uint32_t in_channels,
                                                               const float *in_mix, const void *d_in,
                                                               uint64_t in_stream_stride, uint32_t *in_len, int out_fmt,
                                                               uint32_t out_channels, const float *out_mix, void *d_out,
                                                               uint64_t out_stream_stride, uint32_t *out_len,
                                                               void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Dither: the integer output formats (U8, S16, S24, S32) of the formatted and mixed calls are
 * quantised with a bare half-up rounding unless the state has dither on.  Requantising without
 * dither makes an error that follows the signal (harmonic distortion); with dither it is noise.  The
 * generator is counter based: the noise of an output sample is a pure function of (seed, idx), idx
 * being the sample's index in its stream, so the bytes of a stream still do not depend on how it is
 * cut into calls, on what shares its launch, or on the GPU.  Off by default; with the kind NONE
 * every call is exactly what it is without this section, shortcuts and kernels included.
 *
 *   mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32, wrapping)
 *   idx  = (position + f) * C_out + c      uint64, wrapping; f = output frame of this call, c = channel within the
 *                                          OUTPUT frame, C_out = samples per output frame (out_channels of a mixed
 *                                          call, else the state's channel count)
 *   w    = mix32( lo32(idx) ^ mix32( hi32(idx) ^ hi32(seed) ) ^ lo32(seed) )
 *   a    = w & 0xffff,  b = w >> 16
 *   d    = 0                                   SPEEXHIP_DITHER_NONE
 *   d    = (a + 0.5) / 65536 - 0.5             SPEEXHIP_DITHER_RECTANGULAR   uniform in (-0.5, 0.5) LSB
 *   d    = (a - b) / 65536                     SPEEXHIP_DITHER_TRIANGULAR    triangular in (-1, 1) LSB, variance 1/6
 *
 * d is in units of one LSB of the output format.  A FIR value y goes to an integer format of scale
 * 2^k (the table's "from a FIR value" column) as, in fp64 and evaluated as written,
 *
 *   v = (double)y * 2^k  (exact);   t = v + d  (one rounding);   q = floor(t + 0.5)  (one rounding)
 * (with a stream's gain on -- "Gain" -- y is the gained value: v = (double)y' * 2^k)
 *
 * then the U8 offset and the clamp to the format's range; NaN becomes the format's zero and +-inf go
 * to the rails, as without dither.  With d = 0 these are the undithered bytes.  (For S32 the noise
 * lies below the fp32 mantissa of y; it is allowed all the same: one rule for the four formats.)
 *
 * Dither is a property of the state and applies to the formatted and mixed calls only -- host,
 * device and batch forms.  The int16, float, planar, per-channel, chunks, many and take calls neither
 * dither nor move the position.  `position` is the index of the stream's next output frame:
 * set_dither sets it (a stream can be resumed in a new state), and while the kind is not NONE every
 * formatted or mixed call advances it by the frames it produced, whatever the output format.  Then
 *   - integer output formats are dithered (and the companded ones, at their int16 stage: "Companded
 *     formats"), the float ones (F32, F32N) written as ever;
 *   - S16 -> S16 is no longer the int16 call: it runs as the float call between the two conversions,
 *     with the float entry's counter rules (as a mixed call with a matrix does);
 *   - the zero fallback's zeros are dithered like any other value;
 *   - a state whose channels the per-channel calls moved apart returns BAD_STATE, untouched.
 * In a batch, stream s draws from seed + s * 0x9E3779B97F4A7C15 (mod 2^64) at its own position;
 * batch_set_dither sets every stream's position, batch_get_dither reports stream s's own seed.
 * An unknown kind returns INVALID_ARG and leaves the state as it was.  set_rate, set_quality,
 * reset_mem and skip_zeros touch neither kind, seed nor position.
 *
 * ABI note: 0.7 + dither adds the enum and these five entry points; SpeexHipInfo, the error codes and
 * the version string are unchanged. */
enum { SPEEXHIP_DITHER_NONE = 0, SPEEXHIP_DITHER_RECTANGULAR = 1, SPEEXHIP_DITHER_TRIANGULAR = 2 };
SPEEXHIP_API int speexhip_resampler_set_dither(SpeexHipResamplerState *st, int kind, uint64_t seed, uint64_t position);
/* Any of kind, seed, position may be NULL. */
SPEEXHIP_API int speexhip_resampler_get_dither(SpeexHipResamplerState *st, int *kind, uint64_t *seed,
                                               uint64_t *position);
SPEEXHIP_API int speexhip_batch_set_dither(SpeexHipBatch *b, int kind, uint64_t seed, uint64_t position);
SPEEXHIP_API int speexhip_batch_get_dither(SpeexHipBatch *b, uint32_t stream, int *kind, uint64_t *seed,
                                           uint64_t *position);
/* Host only, no GPU: d[i] = the d above for idx = first_index + i (wrapping), i < n -- the very
 * statement the kernels compile, for the tests to hold against their model. */
SPEEXHIP_API int speexhip_debug_dither(int kind, uint64_t seed, uint64_t first_index, uint32_t n, double *d);

/* ------------------------------------------------------------------------------------------
 * Metering: the output passes saturate -- they clamp the integer and companded formats, send +-inf
 * to the rails and turn NaN into the format's zero -- and without the meter the caller never learns
 * that they did.  A band-limiting filter overshoots on full-scale material, so a stream that did not
 * clip at one rate may clip at another; a conversion from float adds whatever gain the producer
 * applied.  With the meter on, a state counts what its formatted, mixed and sides calls had to throw
 * away and keeps the peak level, per stream.  (The remedy is in the library: "Gain" below, per
 * stream and with a ramp; a diagonal out_mix is a gain too.)  Off by default; while it is off every
 * call is exactly what it is without this section, shortcuts and kernels included.
 *
 * For one value y that an output pass is about to encode to format F, with d the dither of that sample
 * ("Dither"; 0 when dither is off):
 *
 *   nan           y != y.  Nothing else is counted for that sample.
 *   peak          |y| in int16 units: the value the format's "from a FIR value" rule takes -- behind the
 *                 output matrix, behind the gain ("Gain"), before the dither.  +inf is a legal peak.  0 when nothing was metered.
 *   clipped_high  r > hi,   clipped_low  r < lo,   in fp64 and evaluated as written:
 *                   v = (double)y * 2^k  (exact);   t = v + d  (one rounding);   r = floor(t + 0.5)  (one rounding)
 *                 that is the dither section's q before the U8 offset and the clamp; lo and hi are the format's
 *                 rails (U8: 0 and 255 behind the offset, that is -128 and 127 before it; S16: -32768 and 32767;
 *                 S24: -2^23 and 2^23 - 1; S32: -2^31 and 2^31 - 1).  The companded formats are judged at their
 *                 int16 stage -- the mu-law compressor's own limit at 32635 is no clip -- and a big-endian format
 *                 as its little-endian twin.  +-inf count as clips at their rail.
 *
 * The float formats (F32, F32N, F16N, BF16N) never count a clip: their callers read the peak, and a
 * peak above 32768.0 means beyond +-1.0.  `samples` counts every sample metered: frames produced
 * times samples of an output frame.  The totals are integers and a maximum, so like a stream's bytes
 * they depend on the stream alone: not on how it is cut into calls, on what shares its launch, or on
 * the GPU.
 *
 * The meter is a property of the state and applies to the formatted, mixed and sides calls only --
 * host, device, batch, many-states and chunks forms.  The int16, float, planar, per-channel,
 * chunks_int / _float, many_int / _float and take calls are never metered, exactly as they are never
 * dithered.  While it is on
 *   - every output format is metered on its way out; where a call has no output pass (F32 -> F32,
 *     F32N -> F32N without matrix or planar side) the result is read once more, an F32N result as
 *     stored * 32768, and its bytes stay the float call's;
 *   - S16 -> S16 is no longer the int16 call: it runs as the float call between the two conversions,
 *     with the float entry's counter rules (as with dither on);
 *   - the zero fallback's zeros are metered like any other value: they count as samples and clip nothing;
 *   - a state whose channels the per-channel calls moved apart returns BAD_STATE, untouched.
 * set_meter takes 0 or 1 (anything else: INVALID_ARG) and keeps the totals.  get_meter waits for this
 * state's own last call -- never for the device -- and reports the totals since the last reset; with
 * reset != 0 they are zero from there on (m may then be NULL), in a batch for that stream only.
 * set_rate, set_quality, reset_mem, skip_zeros and set_dither touch neither the switch nor the totals.
 *
 * ABI note: 0.7 + metering adds one struct and these five entry points; SpeexHipInfo, SpeexHipSide, the
 * enums, the error codes and the version string are unchanged. */
typedef struct SpeexHipMeter {
  uint32_t struct_size;      /* the caller's sizeof(SpeexHipMeter); at most that many bytes are written; too small for
                                the fields of this version: INVALID_ARG */
  uint32_t on;               /* out: whether the meter is on */
  uint64_t samples;          /* samples metered since the last reset */
  uint64_t clipped_high, clipped_low, nan;
  float peak;                /* int16 units; 0 when nothing was metered */
  uint32_t reserved;
} SpeexHipMeter;
SPEEXHIP_API int speexhip_resampler_set_meter(SpeexHipResamplerState *st, int on);
SPEEXHIP_API int speexhip_resampler_get_meter(SpeexHipResamplerState *st, SpeexHipMeter *m, int reset);
SPEEXHIP_API int speexhip_batch_set_meter(SpeexHipBatch *b, int on);
SPEEXHIP_API int speexhip_batch_get_meter(SpeexHipBatch *b, uint32_t stream, SpeexHipMeter *m, int reset);
/* Host only, no GPU: the very statement the kernels compile, accumulated over y[0..n) into *m (samples = n; `on` is
 * not written).  d = NULL: no dither; d != NULL for a float format: INVALID_ARG, like an unknown format or a short
 * struct_size. */
SPEEXHIP_API int speexhip_debug_meter(int fmt, const float *y, const double *d, uint32_t n, SpeexHipMeter *m);

/* ------------------------------------------------------------------------------------------
 * Gain: the volume control of a stream, applied in the output pass that already converts, mixes, dithers and meters each
 * sample as it leaves -- per stream of a batch, with a linear ramp so that a change is no click.  (A diagonal out_mix is
 * a gain too, but one for all streams of a batch, at most 8 channels wide, a step between two calls, and not fused in
 * the many-states call.)  A stream's gain state is (from, to, total, done): from and to fp32, total the output frames of
 * the ramp (0: none), done <= total the frames of it already produced.  The gain of the output frame that stands k
 * frames behind the start of the ramp -- k = done + f, f the output frame within the call, formed in 64 bits -- is
 *
 *   step = ((double)to - (double)from) / (double)total      formed ONCE, by set_gain
 *   g(k) = (float)( (double)from + (double)k * step )       for k <  total  (the product rounded once, the sum once more,
 *                                                                            never contracted; then nearest-even to fp32)
 *   g(k) = to                                               for k >= total
 *
 * and every sample of that frame becomes y' = y * g: one correctly rounded fp32 product, behind the output matrix's
 * rounding to fp32, before the meter's judgement, the dither and the format's "from a FIR value" rule.  Nothing is clamped
 * on the float image; NaN stays NaN; inf * 0 is NaN, counted as nan and encoded as the format's zero; 0 * negative is
 * -0.0f, and a float output format stores those bits.  g depends on an integer index of the stream alone, so with gain on
 * a stream's bytes still do not depend on the chunking, on what shares its launch, or on the GPU -- with one
 * qualification for the float output formats: where the product itself makes a NaN (inf * 0) its sign and payload are
 * the hardware's default NaN; a NaN that is passed on (NaN * g) keeps its payload, quieted.
 *
 * Off means to == 1.0f and (total == 0 or done == total): the default, and what a ramp that ends at 1.0 returns to.  While
 * every stream of a state is off, every call is exactly what it is without this section: the same kernels, the same
 * shortcuts, the same bytes.  A stream that is off in a batch (or an entry of a many-states call) where another is on is
 * not multiplied -- it is selected per stream, not multiplied by 1.0f -- so its bytes stay what they are without gain, NaN
 * payloads and signed zeros included; the batch's call form follows the state, though: see S16 -> S16 below.
 *
 * set_gain: the new from is the gain the stream's next output frame would have had -- g(done) of the old state, so a new
 * target in mid-ramp is continuous -- the new to is `gain`, the new total is `ramp_frames` (0: a step at the next output
 * frame), and done becomes 0.  A gain that is not finite: INVALID_ARG, the state as it was.  Negative gains (polarity) and
 * 0 (mute) are legal.  get_gain reports current = g(done), target = to, remaining = total - done; any pointer may be NULL.
 * In a batch `stream` selects the stream; set_gain takes UINT32_MAX for every stream.
 *
 * Gain applies to the formatted, mixed and sides calls only -- host, device, batch, many-states and chunks forms: the set
 * that is dithered and metered.  The int16, float, planar, per-channel, chunks_int / _float, many_int / _float and take
 * calls neither apply it nor move done; set_rate, set_quality, reset_mem, skip_zeros, set_dither and set_meter do not
 * touch it.  While any stream of a state has its gain on
 *   - every such call moves each stream's done by the frames it produced, up to total; a stream that produced nothing
 *     does not move;
 *   - S16 -> S16 is no longer the int16 call: it runs as the float call between the two conversions, with the float
 *     entry's counter rules (as with dither or the meter on);
 *   - a result that no output pass writes (F32 -> F32, F32N -> F32N without matrix or planar side; interleaved F32 out)
 *     is multiplied in place behind the FIR launch -- an F32N result as stored, which is the rule's bytes short of overflow
 *     and underflow, the remark made for F32N -> F32N above -- and judged in that same pass when the meter is on; the
 *     planar float pairs run through the plane passes;
 *   - the zero fallback's zeros are multiplied like any value (gain -1: -0.0f in F32, the format's zero elsewhere);
 *   - a state whose channels the per-channel calls moved apart returns BAD_STATE, untouched;
 *   - in a chunks call the ramp's index runs on across the chunk boundaries;
 *   - in a many-states call each entry has its own state's gain and stays fused: gain takes no entry out of a launch
 *     group.  (An entry whose F32 result the FIR writes itself is multiplied by one more kernel over the group.)
 * The meter's peak is |y'| and its clips are judged on y'; the dither's v is (double)y' * 2^k.
 *
 * ABI note: adds these five entry points; SpeexHipInfo, SpeexHipSide, SpeexHipMeter, the enums, the error codes and the
 * version string are unchanged. */
SPEEXHIP_API int speexhip_resampler_set_gain(SpeexHipResamplerState *st, float gain, uint32_t ramp_frames);
SPEEXHIP_API int speexhip_resampler_get_gain(SpeexHipResamplerState *st, float *current, float *target, uint32_t *remaining);
SPEEXHIP_API int speexhip_batch_set_gain(SpeexHipBatch *b, uint32_t stream, float gain, uint32_t ramp_frames);
SPEEXHIP_API int speexhip_batch_get_gain(SpeexHipBatch *b, uint32_t stream, float *current, float *target, uint32_t *remaining);
/* Host only, no GPU: g[i] = g(first + i) of (from, to, total), the very statement the kernels compile. */
SPEEXHIP_API int speexhip_debug_gain(float from, float to, uint32_t total, uint64_t first, uint32_t n, float *g);

/* ------------------------------------------------------------------------------------------
 * Companded formats: G.711 as telephony carries it (RTP PCMU / PCMA, 8 kHz), one byte per sample, no
 * alignment needed.  SPEEXHIP_FMT_ULAW = 16 and SPEEXHIP_FMT_ALAW = 17: companded formats start at 16,
 * the values 6..15 stay invalid.  Both are accepted wherever a format is named -- the formatted and the
 * mixed calls, host, device and batch forms -- and speexhip_sample_bytes gives 1 for them.
 *
 * Decode, storage byte b -> the internal float x, an exact integer in int16 units:
 *   mu-law  u = ~b & 0xFF,  e = (u >> 4) & 7,  m = u & 15
 *           t = (((m << 3) + 0x84) << e) - 0x84;   x = (u & 0x80) ? -t : t
 *           range +-32124; byte 0x7F is the negative zero and decodes to 0
 *   A-law   a = b ^ 0x55,  e = (a >> 4) & 7,  m = a & 15
 *           t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);   x = (a & 0x80) ? t : -t
 *           range +-32256
 *
 * Encode, FIR value y -> byte: the S16 output rule, then the G.711 compressor on that int16 -- the
 * bytes a caller gets from the S16 call followed by its own encoder.
 *   q = clamp(halfup(y), -32768, 32767) as for S16; NaN -> q = 0, +-inf -> the rails.  With dither on
 *   q comes from the dithered S16 rule above: d in int16 steps, v = y, t = v + d, floor(t + 0.5).
 *   mu-law  s = q < 0;  mag = min(|q|, 32635) + 132;  e = floor(log2(mag)) - 7  (0..7)
 *           m = (mag >> (e + 3)) & 15;   b = ~((s << 7) | (e << 4) | m) & 0xFF
 *   A-law   pos = q >= 0;  mag = (pos ? q : -q - 1) >> 3  (0..4095)
 *           e = mag < 32 ? 0 : floor(log2(mag)) - 4;   m = e == 0 ? (mag >> 1) & 15 : (mag >> e) & 15
 *           b = ((pos << 7) | (e << 4) | m) ^ 0x55
 * The format's zero (NaN, the zero fallback's silence) is 0xFF for mu-law and 0xD5 for A-law; the rails
 * are 0x80 / 0x00 for mu-law and 0xAA / 0x2A for A-law.  A-law round-trips all 256 bytes through decode
 * and encode; mu-law all but the negative zero (0x7F -> 0xFF).
 *
 * In the calls: a companded format on either side always runs as the float call between the two
 * conversions, with the float entry's counter rules (speexhip_resampler_peek with float_entry = 1
 * sizes it); no companded pair is an identity pair -- ULAW -> ULAW decodes, filters and encodes.
 * State, history and position are the float call's, so these calls mix freely with all others on one
 * state.  For dither the companded outputs count as integer formats: the noise joins at the int16
 * stage, position advances as for any formatted call, and a state whose channels the per-channel
 * calls moved apart returns BAD_STATE with dither on and goes channel by channel without it.
 *
 * ABI note: 0.7 + g711 adds two enum values and two entry points; SpeexHipInfo, the error codes and the
 * version string are unchanged. */
/* Host only, no GPU: the very statements the kernels compile, for the tests to hold against their
 * model.  x[i] = decode(codes[i]); codes[i] = encode(y[i]) with d[i] (int16 steps) added before the
 * rounding, d == NULL = no dither.  INVALID_ARG for a format that is not companded. */
SPEEXHIP_API int speexhip_debug_g711_decode(int fmt, const uint8_t *codes, uint32_t n, float *x);
SPEEXHIP_API int speexhip_debug_g711_encode(int fmt, const float *y, const double *d, uint32_t n, uint8_t *codes);

/* ------------------------------------------------------------------------------------------
 * Half-float and big-endian formats: what a model in half precision reads and writes, and linear
 * PCM in network / file byte order (RTP L16 of RFC 3551 and L24 of RFC 3190, AIFF).  All at most 4
 * bytes per sample:
 *
 *   format  value  storage                                                     FS
 *   F16N    20     IEEE binary16, little-endian, +-1.0 full scale              1
 *   BF16N   21     bfloat16 (the upper half of an fp32), little-endian, +-1.0  1
 *   S16BE   24     the S16 sample, bytes reversed                              2^15
 *   S24BE   25     the packed S24 sample, bytes reversed (3 bytes)             2^23
 *   S32BE   26     the S32 sample, bytes reversed                              2^31
 *
 * The values 6..15 stay invalid, and so do 18, 19, 22 and 23.  speexhip_sample_bytes gives 2, 2, 2, 3, 4.
 *
 * Big-endian PCM: decode is the S16 / S24 / S32 rule on the byte-reversed sample; encode is the S16 /
 * S24 / S32 rule, then the byte reversal -- half-up rounding, saturation, NaN to 0 and +-inf to the
 * rails as there.  For dither they are integer formats: the noise joins exactly as for the
 * little-endian format, and a dithered BE result is the dithered LE result with each sample's bytes
 * reversed.  S24BE needs no alignment, S16BE and S32BE that of their element.
 *
 * F16N: decode x = (float)h * 32768.0f -- both steps exact for every code, subnormals included; +-inf
 * stay +-inf and NaN stays NaN.  Encode z = y * (1.0f / 32768.0f) in fp32, then z rounded to nearest
 * even to binary16 with subnormal results kept (not flushed); |z| >= 65520 goes to +-inf.  NaN encodes
 * to the canonical 0x7E00 | sign: the bytes of a stream stay a function of the stream alone.
 *
 * BF16N: decode x = as_float(b << 16) * 32768.0f, one fp32 product, fp32 subnormal inputs honoured.
 * Encode z = y * (1.0f / 32768.0f), u = bits(z): NaN -> 0x7FC0 | (u >> 16 & 0x8000); otherwise
 * (u + 0x7FFF + ((u >> 16) & 1)) >> 16 -- round to nearest even, overflow rounds into 0x7F80 by itself.
 *
 * Both half formats are float formats: they never saturate and are never dithered (with dither on the
 * call still advances position, as for F32 / F32N), and the zero fallback's silence is +0.
 *
 * In the calls: a format of this section on either side always runs as the float call between the two
 * passes, with the float entry's counter rules (speexhip_resampler_peek with float_entry = 1 sizes
 * it); no pair among them is an identity pair -- S16BE -> S16BE decodes, filters and encodes, as the
 * companded formats do.  Everything else a formatted, mixed or sides call promises holds unchanged:
 * channels moved apart, the zero fallback, argument errors leaving state and lengths untouched,
 * struct_size.  The formats are accepted in every host, device and batch form of ..._fmt*, ..._mix*
 * and ..._sides*, interleaved or planar.
 *
 * ABI note: 0.7 + halfbe adds five enum values and two entry points; SpeexHipInfo, the error codes
 * and the version string are unchanged. */
/* Host only, no GPU: the very statements the kernels compile, for the tests to hold against their
 * model.  x[i] = decode(sample i of storage); sample i of storage = encode(y[i]), for the three
 * big-endian formats with d[i] (LSB of the format) added before the rounding, d == NULL = no dither
 * (d must be NULL for the half formats).  INVALID_ARG for a format that is not of this section. */
SPEEXHIP_API int speexhip_debug_format_decode(int fmt, const void *storage, uint32_t n, float *x);
SPEEXHIP_API int speexhip_debug_format_encode(int fmt, const float *y, const double *d, uint32_t n, void *storage);

/* ------------------------------------------------------------------------------------------
 * Layouts: a side of a call (its input or its output) is interleaved -- frame f, channel c at sample
 * f * channels + c -- or planar -- at c * plane_stride + f, one plane per channel.  The sides calls
 * name format, channel count, matrix and layout of each side independently: (B, C, T) float32 in
 * +-1.0 in and out (speech models, Web Audio's getChannelData planes), a decoder's interleaved s16le
 * or G.711 in and (C, T') float planes out, ffmpeg's s16p / s32p / u8p / fltp, a planar 5.1 downmix.
 *
 * A call with a planar side IS the mixed call (speexhip_resampler_process_interleaved_mix*) on the
 * same samples arranged as interleaved frames: the same counters, the same history and position left
 * behind in every mode, the same return codes, the same value of every sample.  The dither index is
 * unchanged -- idx = (position + f) * C_out + c with c the channel of the output frame -- so a
 * dithered planar result is the dithered interleaved result, transposed, and position advances as
 * for any formatted call.  Layout changes where a sample lies and nothing else.
 *
 * With a planar side the float entry's rules hold for every format pair, S16 -> S16 included, as with
 * a matrix; speexhip_resampler_peek with float_entry = 1 sizes the call.  A side with one channel is
 * the same bytes in either layout.  With both layouts interleaved the call IS the mixed call, its
 * S16 -> S16 rule without matrix and dither included.  Both sides planar, F32 -> F32 or F32N -> F32N,
 * no matrix: the bytes of the planar float call.  A state whose channels the per-channel calls moved
 * apart is served channel by channel when it is one stream, has no matrix and dither is off: plane c
 * receives what channel c produced and the lengths of the last channel are reported; with a matrix
 * or dither on it returns BAD_STATE.  The zero fallback goes through the passes, its silence being
 * the format's zero.  Every argument error leaves the state, *in_len and *out_len untouched.
 *
 * Lengths are frames; strides count samples of the side's format (a packed S24 sample is 3 bytes).
 * Planes need no alignment beyond their element, the 1-byte formats and S24 none; planes whose base
 * and stride are multiples of 16 bytes take the kernels' 16-bytes-per-lane path.  A planar side is
 * converted, mixed and dithered by the pass that transposes it: a sides call launches no more kernels
 * than the mixed call.  INVALID_ARG: struct_size smaller than this version's, an unknown layout or
 * format, a matrix side beyond 8 channels (or a state beyond 8 with a matrix), a channel count that
 * is not the state's without a matrix, out->data == NULL without planes, a NULL element of planes.
 * Sides, mixed, formatted, interleaved, planar and per-channel calls may be mixed on one state.
 *
 * ABI note: 0.7 + layouts adds one enum, one struct and three entry points; SpeexHipInfo, the error
 * codes and the version string are unchanged. */
enum { SPEEXHIP_LAYOUT_INTERLEAVED = 0, SPEEXHIP_LAYOUT_PLANAR = 1 };
typedef struct SpeexHipSide {
  uint32_t struct_size;   /* the caller's sizeof(SpeexHipSide); smaller than this version's: INVALID_ARG */
  int32_t fmt;            /* SPEEXHIP_FMT_* */
  uint32_t channels;      /* samples per frame on this side (the state's count unless mix != NULL) */
  int32_t layout;         /* SPEEXHIP_LAYOUT_* */
  const float *mix;       /* host memory, as in the mixed call; NULL = none */
  void *data;             /* interleaved: frame 0; planar: plane 0.  Input side: only read, NULL = silence */
  uint64_t plane_stride;  /* planar: samples of fmt between two planes (>= the frames moved); else ignored */
  uint64_t stream_stride; /* batch form: samples of fmt between two streams; else ignored */
  void *const *planes;    /* host form, planar only: plane c = planes[c] (separate allocations); NULL = data + c * plane_stride */
} SpeexHipSide;
/* Host buffers, synchronous.  An interleaved side moves like a buffer of the mixed call (pageable,
 * speexhip_block_acquire blocks and caller-pinned buffers used in place), a planar side plane by
 * plane like the host planar calls.  PTR_OVERLAP when the frames the call writes to an output plane
 * overlap another plane of the call. */
SPEEXHIP_API int speexhip_resampler_process_sides(SpeexHipResamplerState *st, const SpeexHipSide *in, uint32_t *in_len,
                                                  const SpeexHipSide *out, uint32_t *out_len);
/* Device buffers (planes is not read), asynchronous on hip_stream, ordered like the other device calls. */
SPEEXHIP_API int speexhip_resampler_process_sides_device(SpeexHipResamplerState *st, const SpeexHipSide *in,
                                                         uint32_t *in_len, const SpeexHipSide *out, uint32_t *out_len,
                                                         void *hip_stream);
/* ... of every stream of a batch: stream s of a side starts stream_stride samples after stream s - 1
 * (a tensor shaped (batch, channels, time) or (batch, time, channels)); one entry of in_len / out_len
 * per stream, the one pair of matrices serves all streams. */
SPEEXHIP_API int speexhip_batch_process_sides_device(SpeexHipBatch *b, const SpeexHipSide *in, uint32_t *in_len,
                                                     const SpeexHipSide *out, uint32_t *out_len, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Many states, formatted: speexhip_resampler_process_many_int / _float with a format per state -- a
 * gateway's few hundred RTP legs, some PCMU, some PCMA, some L16, in ONE host call per 20 ms tick
 * instead of one per leg.  in[i] / out[i] are entry i's sides (host buffers; struct_size is checked
 * per entry, stream_stride is not read), in_len[i] / out_len[i] its frames available / capacity on
 * entry and consumed / written on return.
 *
 * Entry i is exactly speexhip_resampler_process_sides(st[i], &in[i], &in_len[i], &out[i],
 * &out_len[i]): the same bytes, counters, history, position, dither position and return code, the
 * zero fallback included -- in the default mode (SPEEXHIP_MODE_FAST_FIXED) and in SPEEXHIP_MODE_EXACT,
 * whose bytes do not depend on what shares a launch.  In the opt-in modes SPEEXHIP_MODE_FAST and
 * _FAST_F32 the last bit of a sample may depend on the launch's shape, here as in every call: counters,
 * positions and codes are still the separate calls', the samples within that mode's bound.  codes[i] (may be NULL) receives entry i's code and the
 * function returns the first one that is not SUCCESS.  An entry's argument error -- a NULL state, an
 * unknown format or layout, out->data == NULL without planes, a struct_size smaller than this
 * version's, a channel count that is not the state's without a matrix -- is INVALID_ARG for that
 * entry, leaves its state and its lengths untouched, and the other entries run.
 *
 * Which entries are fused: those whose state is one uniform stream out of the zero fallback and not
 * named earlier in the call, whose sides are both interleaved (or have one channel) in one buffer each,
 * and neither of which has a matrix.  Per device they cost one transfer in, per <= 32 states that share
 * (rates, quality, channels, mode) at most one input pass, one FIR launch and one output pass --
 * whatever formats the states name, each dithered at its own state's kind, seed and position -- and
 * one transfer out.  S16 -> S16 with dither off is the int16 call (no pass), F32 -> F32 and F32N -> F32N
 * the float call on the same bytes (no pass); an F32 side needs no pass.  Every other entry -- a side
 * with a matrix, a planar side of several channels, a state whose channels the per-channel calls moved
 * apart, the zero fallback, a state named twice -- is correct through this call but NOT fused: it takes
 * its own process_sides call, in the caller's order, after the fused ones.
 *
 * ..._fmt is the thin form: every side interleaved with the state's channel count and no matrix.
 * Synchronous; a state must not be used by another thread meanwhile.
 *
 * speexhip_debug_many_counters: process-wide counts since start, over all the many-states calls (the
 * two above and _int / _float) -- out[0] FIR launches, out[1] input passes, out[2] output passes,
 * out[3] entries that took their own call.  Host only.
 *
 * ABI note: 0.7 + many formats adds these three entry points; SpeexHipInfo, SpeexHipSide, the enums,
 * the error codes and the version string are unchanged. */
SPEEXHIP_API int speexhip_resampler_process_many_sides(uint32_t n, SpeexHipResamplerState *const *st,
                                                       const SpeexHipSide *in, uint32_t *in_len,
                                                       const SpeexHipSide *out, uint32_t *out_len, int *codes);
SPEEXHIP_API int speexhip_resampler_process_many_fmt(uint32_t n, SpeexHipResamplerState *const *st,
                                                     const int *in_fmt, const void *const *in, uint32_t *in_len,
                                                     const int *out_fmt, void *const *out, uint32_t *out_len,
                                                     int *codes);
SPEEXHIP_API void speexhip_debug_many_counters(uint64_t out[4]);

/* ------------------------------------------------------------------------------------------
 * Chunk coalescing, formatted: speexhip_resampler_process_chunks_int / _float with a side per
 * direction -- a microphone's float32 stream, a G.711 RTP payload stream, a 24-bit WAV read in
 * whatever pieces the file system hands out -- n consecutive calls of one stream as one transfer in,
 * one transfer out and one wait.
 *
 * `in` describes every chunk's input: format, channels, layout, matrix (its data and planes fields
 * are not read).  Where chunk i lies is in_data's to say: an interleaved side, or a side of one
 * channel, has n_chunks entries; a planar side n_chunks * in->channels, plane c of chunk i being
 * entry i * channels + c (separate allocations).  in_data == NULL, or a NULL (first) entry of a chunk:
 * a chunk of silence; a NULL entry among a present chunk's further planes is INVALID_ARG.  `out` is an
 * ordinary host output side (data, or planes).  The chunks' results lie back to back in it -- chunk i
 * starts at the frame where chunk i - 1 ended, in the buffer or in every plane -- so it needs room for
 * the sum of the capacities.  in_len[i] / out_len[i]: chunk i's frames available / capacity on entry,
 * consumed / written on return.
 *
 * Chunk i is exactly speexhip_resampler_process_sides on the state chunk i - 1 left, with chunk i's
 * data, in_len[i] and out_len[i] and an output side that begins at the frames already written: the
 * same bytes, per-chunk counters, history, position and dither position (the dither index runs on
 * across chunk boundaries) in the default mode and in SPEEXHIP_MODE_EXACT; in SPEEXHIP_MODE_FAST and
 * _FAST_F32 the launch's shape may move a sample's last bit, as in every call.  The counter rules are
 * the int16 entry's for S16 -> S16 without matrix, planar side and dither, the float entry's
 * otherwise.  S16 -> S16, F32 -> F32 and F32N -> F32N without matrix, planar side or dither IS
 * process_chunks_int / _float.  Frames a capacity-bound chunk leaves unconsumed never travel.  A
 * state whose channels the per-channel calls moved apart runs the separate calls when it has no
 * matrix and dither is off, else BAD_STATE, untouched; a state in the zero fallback runs the separate
 * calls.  Argument errors -- an unknown format or layout, a short struct_size, the channel-count
 * rules, an output without data or planes, PTR_OVERLAP between the frames written to two output
 * planes -- leave the state and both length arrays untouched.  The return code follows
 * process_chunks_int's rule.
 *
 * On the GPU a call is one transfer in, at most one input pass, one FIR launch per run of chunks
 * without dropped input, at most one output pass, one transfer out and one wait, where the n
 * separate calls take up to 3n launches and n waits.  ..._fmt is the thin form: both sides
 * interleaved with the state's channel count and no matrix.
 *
 * speexhip_debug_chunk_counters: process-wide counts since start over these two calls -- out[0] FIR
 * launches, out[1] input passes, out[2] output passes, out[3] chunks that took a call of their own.
 * Host only.
 *
 * ABI note: 0.7 + chunk sides adds these three entry points; SpeexHipInfo, SpeexHipSide, the enums,
 * the error codes and the version string are unchanged. */
SPEEXHIP_API int speexhip_resampler_process_chunks_sides(SpeexHipResamplerState *st, uint32_t n_chunks,
                                                         const SpeexHipSide *in, const void *const *in_data,
                                                         uint32_t *in_len, const SpeexHipSide *out, uint32_t *out_len);
SPEEXHIP_API int speexhip_resampler_process_chunks_fmt(SpeexHipResamplerState *st, uint32_t n_chunks, int in_fmt,
                                                       const void *const *in, uint32_t *in_len, int out_fmt, void *out,
                                                       uint32_t *out_len);
SPEEXHIP_API void speexhip_debug_chunk_counters(uint64_t out[4]);

/* Mid-stream control for every stream of a batch (same semantics as the single-stream calls). */
SPEEXHIP_API int speexhip_batch_set_rate_frac(SpeexHipBatch *b, uint32_t ratio_num, uint32_t ratio_den,
                                              uint32_t in_rate, uint32_t out_rate);
SPEEXHIP_API int speexhip_batch_set_quality(SpeexHipBatch *b, int quality);
SPEEXHIP_API int speexhip_batch_skip_zeros(SpeexHipBatch *b);
SPEEXHIP_API int speexhip_batch_reset_mem(SpeexHipBatch *b);
SPEEXHIP_API int speexhip_batch_get_history(SpeexHipBatch *b, uint32_t stream, float *dst);

/* ------------------------------------------------------------------------------------------
 * Host-only pieces of the path, callable without a GPU (used by the CPU test-suite).
 * ---------------------------------------------------------------------------------------- */

/* Filter design (resample.c:605-702): fills *info (rates, num/den, filt_len, oversample,
 * sinc_table_length, kernel) and, when table != NULL, up to table_capacity floats of the
 * sinc table in the reference's layout.  Returns an error code. */
SPEEXHIP_API int speexhip_design_filter(uint32_t in_rate, uint32_t out_rate, int quality,
                                        SpeexHipInfo *info, float *table, uint32_t table_capacity);

/* Same with the ratio given separately from the nominal rates (init_frac / set_rate_frac). */
SPEEXHIP_API int speexhip_design_filter_frac(uint32_t ratio_num, uint32_t ratio_den, uint32_t in_rate,
                                             uint32_t out_rate, int quality, SpeexHipInfo *info,
                                             float *table, uint32_t table_capacity);

/* One call of the stream bookkeeping (resample.c:878-902 inside the block loop :988-1030) in
 * closed form: given in_len frames, out_cap frames of room and the position (*last_sample,
 * *samp_frac_num), returns frames consumed / produced and advances the position. */
SPEEXHIP_API int speexhip_plan_call(uint32_t num_rate, uint32_t den_rate, uint32_t in_len,
                                    uint32_t out_cap, int32_t *last_sample,
                                    uint32_t *samp_frac_num, uint32_t *consumed,
                                    uint32_t *produced);

/* The same for any entry point and state: float_entry selects the float call's rules
 * (resample.c:927-963: no 1024-output cap, pending frames drained once up front) instead of
 * the int16 call's (:968-1036); block_in = frames per block (160 unless a filter has been
 * shortened mid-stream); *magic_samples = pending frames, consumed ahead of the input. */
SPEEXHIP_API int speexhip_plan_call_ex(uint32_t num_rate, uint32_t den_rate, uint32_t in_len,
                                       uint32_t out_cap, int float_entry, uint32_t block_in,
                                       int32_t *last_sample, uint32_t *samp_frac_num,
                                       uint32_t *magic_samples, uint32_t *consumed, uint32_t *produced);

/* What a filter-length change does to a started stream (resample.c:727-782): afterwards the
 * stream holds new_filt_len-1+*new_magic frames, frame j being old frame j+*shift where that
 * exists (the old line has old_filt_len-1+magic frames) and silence elsewhere; last_sample
 * moves by *last_delta.  *phase (may be NULL) is carried from old_den to new_den
 * (resample.c:1130-1139); returns OVERFLOW if that is not representable. */
SPEEXHIP_API int speexhip_plan_filter_change(uint32_t old_filt_len, uint32_t new_filt_len, uint32_t magic,
                                             int64_t *shift, uint32_t *new_magic, int32_t *last_delta,
                                             uint32_t *phase, uint32_t old_den, uint32_t new_den);

/* Library build info: "speexhip <version> gfx950". */
SPEEXHIP_API const char *speexhip_version(void);

/* One channel's position (extension; the reference keeps these in its private state:
 * last_sample[c], samp_frac_num[c], magic_samples[c], resample.c:135-137). */
SPEEXHIP_API int speexhip_resampler_get_channel_position(SpeexHipResamplerState *st, uint32_t channel,
                                                         int32_t *last_sample, uint32_t *samp_frac_num,
                                                         uint32_t *magic_samples);

/* Host-only (no GPU needed, used by the CPU tests): which fast kernel a (ratio, quality, channel count)
 * gets and with what geometry.  out[0] = fast path (2 period kernel, 3 slide kernel, 0 exact kernel only),
 * period kernel: out[1] = phases per wave (10 / 5), out[2] = periods per tile, out[3] = row length (steps),
 * out[4] = LDS window bytes, out[5] = bank padding (floats per period), out[6] = 1 if a second plan with 5
 * phases per wave serves launches of one generation; slide kernel: out[1] = periods per lane, out[3] = row
 * length (steps), out[4] = LDS bytes of a two-wave workgroup, out[7] = tap steps per iteration; period kernel:
 * out[7] = periods per tile of the int16-window plan that int16 calls take instead (0 = none: the float window
 * already holds a full tile, or the layout has no such plan). */
SPEEXHIP_API int speexhip_debug_plan(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels,
                                     uint32_t out[8]);

/* ... and the round-4 plans beside it: out[0] = 5 / 4 when FAST runs the configuration through the fp64-accumulate
 * period / slide kernel (quality 9, 10: out[1] = phases per wave / periods per lane, out[2] = periods per tile,
 * out[3] = row length, out[4] = LDS bytes, out[5] = bank padding / row stride, out[6] = trips per row, out[7] = tap
 * steps per iteration of the slide kernel, or -- period kernel -- periods per tile of the int16-window plan that int16
 * calls take instead, 0 = none), 6 when the mono filter also has phase-pair plans (wide windows: same
 * fields as the period plan, out[7] = periods per tile of their int16-window plan), 0 otherwise. */
SPEEXHIP_API int speexhip_debug_plan64(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels,
                                       uint32_t out[8]);

/* Host only (tests): the shape of the period kernel's launch for a first call of `frames` frames on each of `streams`
 * (<= 32) streams -- out[0] = 1 when the launch takes the phase-pair plan, out[1] = phases per wave (r), out[2] = 1 for
 * the int16 window, out[3] = periods per tile, out[4] = tiles per stream, out[5] = phase-group splits, out[6] = waves
 * with a group, out[7] = tap-range shares (1 = none), out[8] = lanes per workgroup, out[9] = 1 when every workgroup
 * fetches the tap rows into L2 behind its window; all zero when the configuration does not run the fp32 period
 * kernel.  The rules are fitted to a 256-CU device, which is what a process without a GPU assumes. */
SPEEXHIP_API int speexhip_debug_launch_shape(uint32_t ratio_num, uint32_t ratio_den, int quality, uint32_t channels,
                                             uint32_t streams, uint32_t frames, int float_io, uint32_t out[10]);

/* Host only (tests): the placement rule above as a pure function -- the device of state number k on a node with
 * `device_count` devices, env_device / env_devices = the values of SPEEXHIP_DEVICE / SPEEXHIP_DEVICES (NULL = unset),
 * current_device = the calling thread's HIP device.  Returns the device, or -1 when the environment names a device
 * the node does not have or cannot be parsed. */
SPEEXHIP_API int speexhip_debug_placement(int device_count, const char *env_device, const char *env_devices,
                                          uint64_t k, int current_device);

/* Round 6: the placement rule with the load taken into account -- what speexhip_resampler_init really applies.  As
 * speexhip_debug_placement, except that SPEEXHIP_DEVICES=all picks the device with the fewest LIVE states (live[d] for d <
 * device_count; destroying a state frees its slot), ties going to the first such device in the order k mod n, k + 1 mod
 * n, ...: a fresh process still deals its states round-robin, a long-running server fills the holes closed connections
 * leave.  A LIST keeps the counter rule (a reproducible assignment is what the caller asked for).  Host only, pure.
 * speexhip_debug_live_states(d): states alive on logical device d right now. */
SPEEXHIP_API int speexhip_debug_placement_live(int device_count, const char *env_device, const char *env_devices,
                                               uint64_t k, int current_device, const uint32_t *live);
SPEEXHIP_API uint32_t speexhip_debug_live_states(int device);

/* Which kind of box is this?  Runs ~0.3 ms of packed fp32 FMAs with LDS reads on every CU and reports the shader
 * clock (GHz) the chip held meanwhile (median / slowest workgroup): the pool's boxes differ by 4-6 %, so bench
 * lines and the perf gate (tests/test_gpu_perf_gate.py) quote it.  Diagnostics; blocks the calling thread. */
SPEEXHIP_API int speexhip_debug_device_clock(double *ghz_median, double *ghz_min);

/* The PCIe link's own rate on this box (round 6): plain pinned copies of `bytes` host -> device (out_gbs[0]), device ->
 * host (out_gbs[1]) and both at once on two streams (out_gbs[2]: GB/s PER DIRECTION while both run), best of `reps`.
 * The roofline of the host-fed legs of bench.py (`end_to_end`, `end_to_end_streams`).  Diagnostics; blocks. */
SPEEXHIP_API int speexhip_debug_pcie_peak(uint64_t bytes, int reps, double out_gbs[3]);

/* Test hook: the n-th next device allocation made while installing a filter fails, as if the
 * device were out of memory (exercises the resampler_basic_zero fallback, and the release of what
 * an aborted install had already allocated, without exhausting HBM); 0 = off. */
SPEEXHIP_API void speexhip_debug_fail_device_allocs(int n);

/* No counterpart in the reference (its state is plain heap memory, speex_resampler_destroy
 * resample.c:858-868 frees it).  Destroying a state here returns its device buffers, pinned staging
 * buffers, stream and events to a process-wide pool, so that the next state -- callers make one per
 * file or per connection, src/test.ts:27 -- does not pay hipHostMalloc / hipHostFree again
 * (csrc/pool.h; idle memory bounded by SPEEXHIP_POOL_MB, default 1024 MiB device + 256 MiB pinned,
 * 0 = no pool).  This hands everything idle back to the driver; returns the bytes released. */
SPEEXHIP_API uint64_t speexhip_release_cached_memory(void);

/* ------------------------------------------------------------------------------------------
 * Buses: weighted sums of a batch's streams in one device call -- a conference bridge, an N-1 "mix-minus" feed per
 * participant (W = ones - identity), a stem sum -- with the output side's pass of the sides call behind the sum, so
 * that a bus is converted, dithered and metered like a stream.  A SpeexHipBatch may carry a bus matrix W: n_buses x
 * n_streams floats, row-major, host memory; the library copies it.  Off by default; while it is off every call is
 * exactly what it is without this section.
 *
 * For one bus call, with produced[s] the output frames of stream s and C the state's channels:
 *
 *   y'_s[f]     output frame f of this call of stream s, on the state's C channels: the float call's value, times
 *               g_s(done_s + f) in fp32 when that stream's gain is on, exactly as "Gain" says; a stream whose gain is off
 *               is not multiplied.  For f >= produced[s]:  y'_s[f] = +0.0f.
 *   bus_frames  = max over s of produced[s].  Every bus has this length.
 *   bus j, channel c, frame f < bus_frames:
 *               acc = (double)W[j][0] * (double)y'_0
 *               acc = acc + (double)W[j][s] * (double)y'_s        for s = 1 .. n_streams - 1, in ascending order
 *               then one rounding of acc to fp32, nearest even.
 *
 * Every term is included: a zero weight is not skipped, so 0 * inf is NaN, and nothing is clamped on the float image.
 * Each product is exact in fp64 (two 24-bit significands), so a fused multiply-add and a separate multiply and add give
 * the same bits.  The first term is the product itself, not 0 + the product: a sum of -0.0 terms is -0.0f.  Where the sum
 * makes or passes on a NaN, which payload and sign survive is the implementation's choice.  The bus image then leaves by
 * the output side's rule, like a stream's image: the format's "from a FIR value" rule, dither, meter.
 *
 * Dither: the buses take the batch's kind and seed ("Dither").  Bus j draws from seed + (n_streams + j) *
 * 0x9E3779B97F4A7C15 (mod 2^64): the stream rule continued behind the last stream.  All buses share ONE bus position,
 * because all buses have one length: idx = (bus_position + f) * C + c.  set_dither sets the bus position to its
 * `position`, set_buses sets it to 0.  With kind != NONE a bus call advances the bus position by bus_frames, whatever the
 * output format.
 *
 * Meter: with the batch's meter on ("Metering") bus j is judged into a cell of its own, by the rules of that section, and
 * samples += bus_frames * C.  speexhip_batch_get_bus_meter is speexhip_batch_get_meter of a bus's cell.
 *
 * What a bus call moves: each stream's gain `done` by produced[s], up to total.  It does NOT move the streams' own dither
 * positions or meter totals: nothing of theirs is encoded.  Counters, history and positions of every stream are the float
 * call's; a peek with float_entry = 1 (speexhip_plan_call_ex) sizes it.  There are no identity shortcuts, for S16 or
 * any other format.  The zero fallback's zeros are summed like any value.  A stream whose channels the per-channel calls
 * moved apart: BAD_STATE, the state untouched.  The OVERFLOW rule of "Extents" holds, with everything untouched.  The
 * ordering contract of the device calls holds, speexhip_batch_release_stream included.
 *
 * speexhip_batch_set_buses is a control call: it waits for the batch's own last call, as the other control calls do,
 * uploads W to device memory, makes the buses' meter cells, zeroes their totals and zeroes the bus position.  n_buses = 0
 * or weights = NULL: off.  INVALID_ARG, the state as it was: n_buses > 32; a batch of more than 32 streams (the streams'
 * image pointers travel in one kernel-argument pack of 32); a weight that is not finite.  set_rate, set_quality,
 * reset_mem, skip_zeros, set_meter and set_gain do not touch the bus state.  speexhip_batch_get_buses reports n_buses (0:
 * off) and, when weights != NULL, copies the n_buses x n_streams floats back.
 *
 * speexhip_batch_process_bus_device: `in` and in_len[s] are exactly speexhip_batch_process_sides_device's -- format,
 * matrix and layout are all allowed.  out_len[s] is stream s's capacity on entry and its produced frames on return.
 * `out` describes the BUSES: bus j starts j * stream_stride samples after bus 0; any format, interleaved or planar;
 * `channels` must be the state's C.  The caller's bus buffers hold max over s of out_len[s] frames.  *bus_frames receives
 * the length; it may not be NULL.  Every argument error leaves the state and all lengths untouched: no buses set:
 * BAD_STATE; out->mix != NULL (a matrix on the sum is deliberately no part of this call): INVALID_ARG; any other side
 * error: as in the sides call.  Asynchronous on hip_stream, ordered like the other device calls.
 *
 * A host-fed bus call and a bus over many separate states are not part of this version.
 * (Of this section, that is: both are the mixer's, in the section "Mixer" below.)
 *
 * ABI note: adds these six entry points; SpeexHipInfo, SpeexHipSide, SpeexHipMeter, the enums, the error codes and the
 * version string are unchanged. */
SPEEXHIP_API int speexhip_batch_set_buses(SpeexHipBatch *b, uint32_t n_buses, const float *weights);
SPEEXHIP_API int speexhip_batch_get_buses(SpeexHipBatch *b, uint32_t *n_buses, float *weights);
SPEEXHIP_API int speexhip_batch_process_bus_device(SpeexHipBatch *b, const SpeexHipSide *in, uint32_t *in_len,
                                                   const SpeexHipSide *out, uint32_t *out_len, uint32_t *bus_frames,
                                                   void *hip_stream);
SPEEXHIP_API int speexhip_batch_get_bus_meter(SpeexHipBatch *b, uint32_t bus, SpeexHipMeter *m, int reset);
SPEEXHIP_API int speexhip_batch_get_bus_position(SpeexHipBatch *b, uint64_t *position);
/* Host only, no GPU: the very statement the kernel compiles -- z[j * n + i] = bus j of y[s * n + i] (already gained),
 * i < n, s < n_streams. */
SPEEXHIP_API int speexhip_debug_bus(uint32_t n_streams, uint32_t n_buses, const float *weights, const float *y, uint32_t n,
                                    float *z);

/* ------------------------------------------------------------------------------------------
 * Mixer: mix buses over many SEPARATE states in one host call -- a conference bridge whose legs are G.711 at 8 kHz,
 * wideband at 16 kHz and studio feeds at 48 kHz, each an ordinary single-stream SpeexHipResamplerState with its own
 * rates, quality, mode, gain and ramp, each fed in its own sample format from host memory.  A SpeexHipMixer has n_legs
 * SLOTS, n_buses buses and one channel count C; it owns what a SpeexHipBatch owns for its buses -- W on the device, the
 * buses' dither kind, seed and ONE bus position, the buses' meter switch and cells -- and nothing of a leg: the caller
 * names the state in every slot with every call.
 *
 * The sum is the rule of "Buses", unchanged, with the slots in the place of the streams.  For one call, with produced[i]
 * the output frames of the leg in slot i:
 *
 *   y'_i[f]     output frame f OF THIS CALL of leg i, on C channels: the float call's value, times g_i(done_i + f) in
 *               fp32 when that state's gain is on ("Gain"), not multiplied when it is off.  +0.0f for f >= produced[i];
 *               +0.0f throughout for an empty slot and for a leg that was refused.
 *   bus_frames  = max over the legs that ran of produced[i].  Every bus has this length.
 *   bus j, channel c, frame f < bus_frames:
 *               (float)( (double)W[j][0] * y'_0 + (double)W[j][1] * y'_1 + ... ), summed in ascending slot order, every
 *               term included, the first term the product itself, rounded once -- "Buses" word for word.
 *
 * The bus image leaves by the output side's rule, as in the Batch's bus call: the format's encode, dither, meter.
 * Dither: bus j draws from seed + (n_legs + j) * 0x9E3779B97F4A7C15 (mod 2^64); all buses share one bus position, idx =
 * (bus_position + f) * C + c; speexhip_mixer_set_dither sets it, speexhip_mixer_set_weights zeroes it, a call with kind !=
 * NONE advances it by bus_frames, whatever the output format.  Meter: one cell per bus, samples += bus_frames * C.
 *
 * What a call moves: each leg's position, history and counters as the float call does (in_len[i] / out_len[i] are the
 * float entry's counters: speexhip_resampler_peek with float_entry = 1 sizes a leg), and each leg's gain `done` by
 * produced[i], up to total.  It does NOT move a leg's own dither position or meter totals: nothing of a leg is encoded,
 * and nothing of a leg travels back.
 *
 * What follows from "frame f of this call": the buses line the legs up by the frame of THIS CALL, as the Batch's bus
 * does.  The buses' bytes are therefore independent of how the stream of ticks is cut into calls exactly when every leg
 * produces bus_frames frames on every call.  Legs of one ratio fed equal lengths do, and so do legs of different ratios
 * fed the same whole tick -- 160 frames at 8 kHz, 320 at 16 kHz, 882 at 44.1 kHz and 960 at 48 kHz all make 960 frames at
 * 48 kHz, on the first call as on every other, whatever the filters' lengths: a state produces from its first input
 * frame on.  Legs whose input per call is not a whole number of their ratio's periods do not (44.1 kHz fed 5 ms brings 220
 * or 221 frames and makes 239 to 241), nor do legs fed different durations.  Keeping a per-leg residue to line legs up
 * by stream position is no part of this version.
 *
 * speexhip_mixer_process, one host call per tick: one transfer in (the legs' payloads and the table of the legs, gathered),
 * the legs' input passes and FIR launches grouped exactly as speexhip_resampler_process_many_sides groups them (up to 32
 * legs that share filter tables, mode and window format a launch), ONE launch of the bus-sum kernel over all slots, the
 * output pass over the buses (one per 32 buses; none for an interleaved F32 side), one transfer out of the buses.
 *   legs[i], i < n_legs   the state in slot i; NULL: an empty slot.
 *   in[i]                 that leg's input side, a HOST buffer; struct_size is checked per leg; stream_stride and planes
 *                         are not read; data == NULL: a present, silent leg.
 *   in_len[i], out_len[i] frames available and capacity on entry, frames consumed and produced on return.
 *   out                   describes the BUSES in host memory: bus j starts j * stream_stride samples after bus 0; any
 *                         format; interleaved, or planar through plane_stride; channels must be the mixer's; mix and
 *                         planes must be NULL.  Every bus buffer holds max over i of out_len[i] frames.
 *   *bus_frames           receives the length of the buses.
 *   codes                 may be NULL; codes[i] receives the outcome of slot i.  The function returns the first outcome
 *                         that is not SUCCESS.
 * A refused leg keeps its state and both its lengths untouched and counts as +0.0f in the sum; the other legs run: one bad
 * leg does not cost the tick.  Per leg:
 *   an empty slot                                         SUCCESS, both lengths set to 0
 *   a side with a short struct_size, an unknown format or layout, a matrix, a planar layout of more than one channel, or
 *   a channel count that is not the mixer's               INVALID_ARG
 *   a state of more than one stream, on another device than the mixer, or named by an earlier slot      INVALID_ARG
 *   lengths that fail "Extents"                           OVERFLOW
 *   a state whose channels the per-channel calls moved apart                                            BAD_STATE
 *   a state in the zero fallback                          runs: counters move, zeros are summed (gained), ALLOC_FAILED
 *                                                         as in every call
 * Call-level errors, returned before anything is touched, codes not written: m, legs, in, in_len, out_len, out or
 * bus_frames NULL: INVALID_ARG; an `out` side error (above, or data == NULL): INVALID_ARG; no weights set: BAD_STATE.
 *
 * The call is synchronous.  The mixer and its legs must not be used by another thread meanwhile.  A leg whose last call
 * was a device call on another stream is ordered behind it on the device, as in the many-states calls.  In the default
 * mode and in SPEEXHIP_MODE_EXACT a leg's floats do not depend on what shares its launch, so the buses' bytes are a
 * function of the legs' streams and of the cut alone; in FAST and FAST_F32 the usual last-bit caveat holds.
 *
 * speexhip_mixer_init: device by the placement rule, or named (_init_on); 0 or more than SPEEXHIP_MIXER_MAX_LEGS legs, 0 or
 * more than SPEEXHIP_MIXER_MAX_BUSES buses, 0 or more than 8 channels: NULL with INVALID_ARG.
 * speexhip_mixer_set_weights is a control call: it waits for the mixer's own last call, copies W (n_buses x n_legs floats,
 * row-major, host), uploads it, zeroes the buses' cells, totals and the bus position.  A weight that is not finite:
 * INVALID_ARG, the mixer as it was.  weights = NULL: the mixer is off (process: BAD_STATE) until weights are set again.
 * speexhip_mixer_get_weights copies W back (BAD_STATE while off).  set_dither / get_dither / set_meter /
 * get_bus_meter are the Batch's, of the buses alone; get_dither reports the mixer's seed as given and the bus position.
 *
 * speexhip_debug_mixer_counters: host only, process-wide since start -- FIR launches, input passes, bus-sum launches, output
 * passes, transfers in, transfers out of the mixer calls.  A transfer in is the call's gathered stage (copied to the
 * device, or, where the whole call fits the pinned stage, read there by the kernels), plus one for every payload large
 * enough to travel on its own; a transfer out likewise.
 *
 * Not part of this version: a device-pointer form, legs on several GPUs in one mixer, a matrix or planes on a leg's
 * input side, lining legs up by stream position, resampling a bus back to a leg's own rate (a second many-states call).
 *
 * ABI note: adds these eleven entry points and the two limits; SpeexHipInfo, SpeexHipSide, SpeexHipMeter, the enums, the
 * error codes and the version string are unchanged. */
typedef struct SpeexHipMixer_ SpeexHipMixer;
#define SPEEXHIP_MIXER_MAX_LEGS  1024
#define SPEEXHIP_MIXER_MAX_BUSES 1024
SPEEXHIP_API SpeexHipMixer *speexhip_mixer_init(uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err);
SPEEXHIP_API SpeexHipMixer *speexhip_mixer_init_on(int device, uint32_t n_legs, uint32_t n_buses, uint32_t channels, int *err);
SPEEXHIP_API void speexhip_mixer_destroy(SpeexHipMixer *m);
SPEEXHIP_API int speexhip_mixer_set_weights(SpeexHipMixer *m, const float *weights);
SPEEXHIP_API int speexhip_mixer_get_weights(SpeexHipMixer *m, float *weights);
SPEEXHIP_API int speexhip_mixer_set_dither(SpeexHipMixer *m, int kind, uint64_t seed, uint64_t position);
SPEEXHIP_API int speexhip_mixer_get_dither(SpeexHipMixer *m, int *kind, uint64_t *seed, uint64_t *position);
SPEEXHIP_API int speexhip_mixer_set_meter(SpeexHipMixer *m, int on);
SPEEXHIP_API int speexhip_mixer_get_bus_meter(SpeexHipMixer *m, uint32_t bus, SpeexHipMeter *meter, int reset);
SPEEXHIP_API int speexhip_mixer_process(SpeexHipMixer *m, SpeexHipResamplerState *const *legs, const SpeexHipSide *in,
                                        uint32_t *in_len, uint32_t *out_len, const SpeexHipSide *out, uint32_t *bus_frames,
                                        int *codes);
SPEEXHIP_API void speexhip_debug_mixer_counters(uint64_t out[6]);

/* ------------------------------------------------------------------------------------------
 * Mixer levels: how loud each leg of a tick was, measured on the device while the legs' float images are resident --
 * what active-speaker detection, "mix only the N loudest", the RFC 6464 / 6465 audio-level header extensions, a UI's
 * talking indicators and silence suppression go by.  A mixer call sends nothing of a leg back, so without this a leg's
 * level costs a second run of every leg through speexhip_resampler_process_many_fmt to F32.  Off by default; while it is
 * off a mixer call is byte for byte and launch for launch what "Mixer" describes.
 *
 * One record per slot and call, over all C channels of the leg, measured on the leg's float value y: the float call's
 * value in int16 units BEFORE the state's gain -- y_i, not y'_i of "Mixer".  Pre-gain is deliberate: the levels are for
 * deciding gains (read tick t's levels, speexhip_resampler_set_gain for tick t + 1, never touch W), and a muted leg must
 * still read as loud.
 *
 *   samples   produced[i] * C            (frames of THIS call; the +0.0f padding up to bus_frames is NOT measured)
 *   per sample y:
 *     y != y            nan += 1; nothing else for that sample
 *     otherwise         peak = max(peak, |y|)                       fp32, +inf is a legal peak
 *                       r = floor((double)y + 0.5)                  "Metering"'s S16 r with d = 0
 *                       q = r < -32768 ? -32768 : r > 32767 ? 32767 : r
 *                       energy += (uint64)(q * q)                   integer, exact; +-inf count at their rail
 *
 * energy is a sum of integers and peak a maximum: like the meter's totals they do not depend on the order of the
 * reduction, on what shares a launch, or on the GPU.  A call of more than 2^34 samples in one leg wraps energy mod 2^64.
 * An empty slot and a refused leg: all zeros.  A silent leg (data == NULL) and a leg in the zero fallback: samples
 * counted, the rest 0 -- their images are zeros.  The RFC 6464 level of a record is
 * min(127, max(0, round(-10 * log10(energy / (samples * 2^30))))), 127 when energy or samples is 0.
 *
 * speexhip_mixer_set_levels: on = 0 / 1, anything else INVALID_ARG; a CHANGE of the switch clears the snapshot.  With the
 * switch on, speexhip_mixer_process measures every slot behind the legs' last FIR launch -- one more launch for a call
 * whose every leg produced at most 65 536 samples, two otherwise -- and the records ride back behind the buses in the one
 * transfer out the call makes anyway (none, where the call is small: the kernel writes the pinned stage); no atomics.
 * speexhip_mixer_get_levels reports the LAST process call's records of the slots [first_slot, first_slot + count): record k
 * at (char *)levels + k * struct_size, its first 32 bytes written.  struct_size < 32, a range beyond n_legs, or a NULL
 * pointer: INVALID_ARG; levels off: BAD_STATE; before any call: zeros; after a call-level error (nothing touched): the
 * snapshot as it was; after a call whose unit failed: cleared; after a call with bus_frames == 0: zeros (nothing was
 * launched).  set_weights, set_dither and set_meter do not touch it.  The six speexhip_debug_mixer_counters keep their
 * meaning and their values; speexhip_debug_mixer_level_launches counts the levels' launches apart (host only,
 * process-wide since start).  speexhip_debug_levels: host only, no GPU -- the very lines the kernel compiles, over y[0 .. n),
 * ACCUMULATED into *l (samples += n; zero the record first for a fresh one).
 *
 * Not part of this version: levels in the Batch's bus call; post-gain or per-channel levels; any selection policy
 * (loudest-N, hold, hysteresis) inside the library; accumulation across calls -- the caller sums records if it wants that.
 *
 * ABI note: adds SpeexHipLevel and these four entry points; SpeexHipInfo, SpeexHipSide, SpeexHipMeter, the enums, the
 * error codes, the eleven entry points of "Mixer" and the version string are unchanged. */
typedef struct SpeexHipLevel {
  uint64_t samples, energy, nan;
  float peak;
  uint32_t reserved;
} SpeexHipLevel; /* 32 bytes */
SPEEXHIP_API int speexhip_mixer_set_levels(SpeexHipMixer *m, int on);
SPEEXHIP_API int speexhip_mixer_get_levels(SpeexHipMixer *m, uint32_t first_slot, uint32_t count, void *levels,
                                           uint32_t struct_size);
SPEEXHIP_API int speexhip_debug_levels(const float *y, uint32_t n, SpeexHipLevel *l);
SPEEXHIP_API uint64_t speexhip_debug_mixer_level_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* SPEEXHIP_RESAMPLER_H */
