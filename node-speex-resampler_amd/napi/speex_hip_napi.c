/*
 * speex_hip_napi.c -- thin raw N-API (C) addon that binds libspeexhip's C ABI
 * (include/speexhip_resampler.h) for index.js.  It REPLACES the Emscripten module
 * src/speex_wasm.js of the reference: where src/index.ts:59-102 called
 * Module._speex_resampler_init / _process_interleaved_int / _strerror on the WASM heap,
 * index.js calls init() / process() here with Buffers.  No arithmetic happens in this file.
 *
 * Beyond the reference surface it carries the SURVEY 8(f) rows: float I/O (N2), mid-stream
 * control (N3), explicit destroy (N4), chunk coalescing and an asynchronous call that keeps
 * the event loop free while the GPU works (N1).
 *
 * Built with plain gcc against /usr/include/node (N-API v3+, no node-addon-api).
 */
#include <node_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "speexhip_resampler.h"

#define NAPI_OK(call)                                            \
  do {                                                           \
    if ((call) != napi_ok) {                                     \
      napi_throw_error(env, NULL, "speexhip N-API failure: " #call); \
      return NULL;                                               \
    }                                                            \
  } while (0)

/* What a JS handle points at.  `st` becomes NULL on destroy(); the lock serialises calls that
 * reach one state from libuv pool threads (processAsync). */
typedef struct {
  SpeexHipResamplerState *st;
  pthread_mutex_t lock;
  int meter_on; /* setMeter: while on, s16 -> s16 has the float call's counters (read and written under the lock) */
} Handle;

/* whether the state's output gain is on (speexhip_resampler_set_gain): s16 -> s16 then has the float call's counters */
static int gain_is_on(SpeexHipResamplerState *st) {
  float target = 1.0f;
  uint32_t remaining = 0;
  if (speexhip_resampler_get_gain(st, NULL, &target, &remaining) != 0) return 0;
  return !(target == 1.0f && remaining == 0);
}

static void finalize_state(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  Handle *h = (Handle *)data;
  if (h->st != NULL) speexhip_resampler_destroy(h->st);
  pthread_mutex_destroy(&h->lock);
  free(h);
}

static Handle *unwrap_handle(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || p == NULL) {
    napi_throw_type_error(env, NULL, "expected a resampler handle");
    return NULL;
  }
  return (Handle *)p;
}

/* Every entry point that touches a state holds the handle's lock from before it reads anything of
 * the state until it is done with it: a processAsync job on a libuv pool thread may be running the
 * same state, and everything below -- counters (peek), filter data (setRate frees and rebuilds
 * device tables), even the st pointer (destroy) -- changes under such a job.  Returns the state
 * with the lock HELD, or NULL (exception pending, lock released). */
static SpeexHipResamplerState *lock_state(napi_env env, napi_value v, Handle **hp) {
  Handle *h = unwrap_handle(env, v);
  if (h == NULL) return NULL;
  pthread_mutex_lock(&h->lock);
  if (h->st == NULL) {
    pthread_mutex_unlock(&h->lock);
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  *hp = h;
  return h->st;
}
#define UNLOCK(h) pthread_mutex_unlock(&(h)->lock)
/* NAPI_OK for use while the lock is held */
#define NAPI_OK_LOCKED(h, call)                                     \
  do {                                                              \
    if ((call) != napi_ok) {                                        \
      UNLOCK(h);                                                    \
      napi_throw_error(env, NULL, "speexhip N-API failure: " #call); \
      return NULL;                                                  \
    }                                                               \
  } while (0)

/* init(channels, inRate, outRate, quality) -> handle; throws Error(strerror(code)) like
 * src/index.ts:63-65 */
static napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t ch = 0, in_rate = 0, out_rate = 0;
  int32_t quality = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[0], &ch));
  NAPI_OK(napi_get_value_uint32(env, argv[1], &in_rate));
  NAPI_OK(napi_get_value_uint32(env, argv[2], &out_rate));
  NAPI_OK(napi_get_value_int32(env, argv[3], &quality));
  /* optional fifth argument: the GPU (speexhip_resampler_init_on); absent / negative = the library's placement rule
   * (SPEEXHIP_DEVICE, SPEEXHIP_DEVICES=all: instance k of the process on GPU k mod the device count) */
  int32_t device = -1;
  if (argc >= 5) {
    napi_valuetype t;
    if (napi_typeof(env, argv[4], &t) == napi_ok && t == napi_number) NAPI_OK(napi_get_value_int32(env, argv[4], &device));
  }
  int err = 0;
  SpeexHipResamplerState *st = speexhip_resampler_init_on(device, ch, in_rate, out_rate, quality, &err);
  if (st == NULL) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(err));
    return NULL;
  }
  Handle *h = (Handle *)calloc(1, sizeof(Handle));
  if (h == NULL) {
    speexhip_resampler_destroy(st);
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED));
    return NULL;
  }
  h->st = st;
  pthread_mutex_init(&h->lock, NULL);
  napi_value handle;
  NAPI_OK(napi_create_external(env, h, finalize_state, NULL, &handle));
  return handle;
}

/* destroy(handle): release the device state now instead of at garbage collection (the
 * reference never calls speex_resampler_destroy: SURVEY 8f row N4). */
static napi_value Destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = unwrap_handle(env, argv[0]);
  if (h == NULL) return NULL;
  pthread_mutex_lock(&h->lock);
  if (h->st != NULL) speexhip_resampler_destroy(h->st);
  h->st = NULL;
  pthread_mutex_unlock(&h->lock);
  return NULL;
}

/* Optional Buffer argument: null / undefined -> NULL pointer (the reference's in == NULL). */
static int buffer_or_null(napi_env env, napi_value v, void **data, size_t *bytes) {
  napi_valuetype t;
  *data = NULL;
  *bytes = 0;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_null || t == napi_undefined) return 1;
  return napi_get_buffer_info(env, v, data, bytes) == napi_ok;
}

/* external Buffers over pinned blocks of the library (process_common) */
static const size_t kExternalMin = 4096;            /* below this a copy is cheaper than a finalizer */
/* (process-wide: the addon may be loaded by several environments -- the main thread and worker_threads -- and
 *  finalizers run on whichever thread owns the Buffer: every access is an atomic builtin) */
static size_t g_external_bytes = 0;
static size_t g_take_calls = 0, g_take_no_block = 0; /* stats(): results left in pinned blocks / slab full, copied instead */
static size_t g_pinned_chunks = 0;                   /* stats(): allocChunk() calls served with a pinned block */
static int g_no_external = 0; /* SPEEXHIP_NAPI_COPY=1: always copy (A/B, tests) */
static void finalize_block(napi_env env, void *data, void *hint) {
  const size_t bytes = (size_t)hint;
  int64_t adjusted = 0;
  speexhip_block_release(data);
  __atomic_fetch_sub(&g_external_bytes, bytes, __ATOMIC_RELAXED);
  (void)napi_adjust_external_memory(env, -(int64_t)bytes, &adjusted);
}

/* process / processFloat (handle, chunk: Buffer|null, inFrames, outCapacityFrames) -> Buffer
 * (fresh copy of the frames written): the src/index.ts:90-115 sequence without the WASM heap. */
static napi_value process_common(napi_env env, napi_callback_info info, size_t sample_bytes) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *in_data = NULL;
  size_t in_bytes = 0;
  if (!buffer_or_null(env, argv[1], &in_data, &in_bytes)) {
    napi_throw_type_error(env, NULL, "chunk must be a Buffer or null");
    return NULL;
  }
  uint32_t in_len = 0, out_len = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[2], &in_len));
  NAPI_OK(napi_get_value_uint32(env, argv[3], &out_len));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  const size_t frame_bytes = (size_t)si.nb_channels * sample_bytes;
  if (in_data != NULL && (size_t)in_len * frame_bytes > in_bytes) {
    UNLOCK(h);
    napi_throw_range_error(env, NULL, "input frame count exceeds the chunk");
    return NULL;
  }
  /* the counters are known before any GPU work: size the result exactly and let the library write
   * straight into it (one copy instead of three).  peek and the call see the same state: the lock
   * is held from before the peek until the call has returned. */
  uint32_t will_use = 0, will_make = 0;
  speexhip_resampler_peek(st, in_len, out_len, sample_bytes == 4, &will_use, &will_make);
  const size_t made_bytes = (size_t)will_make * frame_bytes;
  /* Round 4: results of a few KB and more stay where the kernel wrote them -- a pinned block of the library's
   * pool -- and become an EXTERNAL Buffer (a fresh, caller-owned Buffer like src/index.ts:111-115 returns; its
   * finalizer hands the block back to the pool): the samples cross memory once on their way out instead of twice.
   * Bounded: the blocks come out of one pinned slab (SPEEXHIP_TAKE_MB, 64 MiB); while JavaScript holds so many of
   * them that none fits (Buffers kept alive, or a garbage collector that has not run yet) the library says NO_BLOCK
   * without touching the state and the copying path below serves the call. */
  int take_rc = SPEEXHIP_ERR_NO_BLOCK;
  void *block = NULL;
  uint32_t take_in = in_len, take_out = out_len;
  if (made_bytes >= kExternalMin && !g_no_external)
    take_rc = sample_bytes == 2
                  ? speexhip_resampler_process_interleaved_int_take(st, (const int16_t *)in_data, &take_in, &take_out, (int16_t **)&block)
                  : speexhip_resampler_process_interleaved_float_take(st, (const float *)in_data, &take_in, &take_out, (float **)&block);
  if (take_rc == SPEEXHIP_ERR_NO_BLOCK && made_bytes >= kExternalMin && !g_no_external)
    __atomic_fetch_add(&g_take_no_block, 1, __ATOMIC_RELAXED);
  if (take_rc != SPEEXHIP_ERR_NO_BLOCK) { /* (NO_BLOCK: the state is untouched -> the copying path below) */
    int rc = take_rc;
    uint32_t cap_len = take_out;
    UNLOCK(h);
    if (rc != 0 || cap_len != will_make || block == NULL) {
      speexhip_block_release(block);
      napi_throw_error(env, NULL, speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE));
      return NULL;
    }
    napi_value ext;
    __atomic_fetch_add(&g_external_bytes, made_bytes, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_take_calls, 1, __ATOMIC_RELAXED);
    const napi_status ext_status = napi_create_external_buffer(env, made_bytes, block, finalize_block, (void *)made_bytes, &ext);
    if (ext_status != napi_ok) {
      /* The state has already advanced and the audio exists only in the block: a runtime that refuses external
       * Buffers (napi_no_external_buffers_allowed: Electron, V8 sandbox) or is out of memory for the wrapper must not
       * cost the caller its samples.  Copy them into an ordinary Buffer, hand the block back, and stop asking for
       * external Buffers for good when the runtime does not allow them. */
      __atomic_fetch_sub(&g_external_bytes, made_bytes, __ATOMIC_RELAXED);
      if ((int)ext_status == 22 /* napi_no_external_buffers_allowed (Node >= 18.?; not in this header) */) g_no_external = 1;
      napi_value copy;
      void *copied = NULL;
      const napi_status copy_status = napi_create_buffer_copy(env, made_bytes, block, &copied, &copy);
      speexhip_block_release(block);
      if (copy_status != napi_ok) {
        napi_throw_error(env, NULL, "speexhip N-API failure: napi_create_external_buffer and napi_create_buffer_copy");
        return NULL;
      }
      return copy;
    }
    int64_t adjusted = 0;
    (void)napi_adjust_external_memory(env, (int64_t)made_bytes, &adjusted); /* the collector sees what the Buffer holds */
    return ext;
  }
  napi_value out;
  void *dst = NULL;
  NAPI_OK_LOCKED(h, napi_create_buffer(env, (size_t)will_make * frame_bytes, &dst, &out));
  uint64_t nowhere = 0;
  if (dst == NULL) dst = &nowhere; /* empty Buffer: nothing will be written, but NULL means "no buffer" */
  /* out_len stays the caller's capacity (a smaller one could end the call's block loop early and
   * leave trailing input unconsumed); the library writes exactly will_make frames */
  int rc = sample_bytes == 2
               ? speexhip_resampler_process_interleaved_int(st, (const int16_t *)in_data, &in_len,
                                                            (int16_t *)dst, &out_len)
               : speexhip_resampler_process_interleaved_float(st, (const float *)in_data, &in_len,
                                                              (float *)dst, &out_len);
  UNLOCK(h);
  if (rc != 0 || out_len != will_make) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  return out;
}
static napi_value Process(napi_env env, napi_callback_info info) { return process_common(env, info, 2); }
static napi_value ProcessFloat(napi_env env, napi_callback_info info) { return process_common(env, info, 4); }

/* processPlanar(handle, planes: Int16Array[] | Float32Array[], outCapacityFrames) -> typed arrays of the same kind,
 * one per channel: speexhip_resampler_process_planar_int / _float on the arrays' own memory, the result written
 * straight into fresh typed arrays of exactly the frames the call makes (peek, as in process_common). */
static napi_value ProcessPlanar(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t n = 0, out_len = 0;
  bool is_array = false;
  if (napi_is_array(env, argv[1], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[1], &n) != napi_ok || n == 0) {
    napi_throw_type_error(env, NULL, "channels must be an array of Int16Array or of Float32Array");
    return NULL;
  }
  NAPI_OK(napi_get_value_uint32(env, argv[2], &out_len));
  const void **in = (const void **)calloc(n, sizeof(void *));
  void **out = (void **)calloc(n, sizeof(void *));
  napi_value result = NULL;
  const char *fail = NULL;
  int type_error = 0;
  napi_typedarray_type kind = napi_int16_array;
  size_t frames = 0;
  Handle *h = NULL;
  if (in == NULL || out == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  for (uint32_t c = 0; fail == NULL && c < n; c++) {
    napi_value v;
    napi_typedarray_type t;
    size_t len = 0;
    void *data = NULL;
    bool typed = false;
    if (napi_get_element(env, argv[1], c, &v) != napi_ok || napi_is_typedarray(env, v, &typed) != napi_ok || !typed ||
        napi_get_typedarray_info(env, v, &t, &len, &data, NULL, NULL) != napi_ok ||
        (t != napi_int16_array && t != napi_float32_array) || (c != 0 && t != kind)) {
      fail = "channels must be an array of Int16Array or of Float32Array";
      type_error = 1;
    } else if (c != 0 && len != frames) {
      fail = "channels must all have the same length";
    } else {
      kind = t;
      frames = len;
      in[c] = data != NULL ? data : (const void *)in; /* (an empty array: nothing is read, but NULL means "no plane") */
    }
  }
  SpeexHipResamplerState *st = NULL;
  if (fail == NULL) {
    st = lock_state(env, argv[0], &h);
    if (st == NULL) {
      free(in);
      free(out);
      return NULL;
    }
    SpeexHipInfo si;
    speexhip_resampler_get_info(st, &si);
    if (si.nb_channels != n) fail = "one typed array per channel is expected";
  }
  if (fail == NULL) {
    const int is_float = kind == napi_float32_array;
    const size_t es = is_float ? 4 : 2;
    uint32_t in_len = (uint32_t)frames, will_use = 0, will_make = 0;
    speexhip_resampler_peek(st, in_len, out_len, is_float, &will_use, &will_make);
    uint64_t nowhere = 0;
    if (napi_create_array_with_length(env, n, &result) != napi_ok) fail = "speexhip N-API failure: napi_create_array_with_length";
    for (uint32_t c = 0; fail == NULL && c < n; c++) {
      napi_value ab, ta;
      void *dst = NULL;
      if (napi_create_arraybuffer(env, (size_t)will_make * es, &dst, &ab) != napi_ok ||
          napi_create_typedarray(env, kind, will_make, ab, 0, &ta) != napi_ok || napi_set_element(env, result, c, ta) != napi_ok)
        fail = "speexhip N-API failure: creating the result arrays";
      out[c] = will_make != 0 && dst != NULL ? dst : (void *)&nowhere;
    }
    if (fail == NULL) {
      /* out_len stays the caller's capacity (process_common); the library writes exactly will_make frames */
      uint32_t cap = out_len;
      const int rc = is_float ? speexhip_resampler_process_planar_float(st, (const float *const *)in, &in_len, (float *const *)out, &cap)
                              : speexhip_resampler_process_planar_int(st, (const int16_t *const *)in, &in_len, (int16_t *const *)out, &cap);
      if (rc != 0 || cap != will_make) fail = speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE);
    }
  }
  if (h != NULL) UNLOCK(h);
  free(in);
  free(out);
  if (fail != NULL) {
    if (type_error)
      napi_throw_type_error(env, NULL, fail);
    else
      napi_throw_error(env, NULL, fail);
    return NULL;
  }
  return result;
}

/* processFormat(handle, chunk: Buffer|null, inFormat, outFormat, inFrames, outCapacityFrames) -> Buffer of the frames
 * written, in outFormat: speexhip_resampler_process_interleaved_fmt on the Buffer's own memory, the result written straight
 * into a fresh Buffer of exactly the frames the call makes (peek with the entry whose counters the pair has). */
static napi_value ProcessFormat(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *in_data = NULL;
  size_t in_bytes = 0;
  if (!buffer_or_null(env, argv[1], &in_data, &in_bytes)) {
    napi_throw_type_error(env, NULL, "chunk must be a Buffer or null");
    return NULL;
  }
  int32_t in_fmt = -1, out_fmt = -1;
  uint32_t in_len = 0, out_len = 0;
  NAPI_OK(napi_get_value_int32(env, argv[2], &in_fmt));
  NAPI_OK(napi_get_value_int32(env, argv[3], &out_fmt));
  NAPI_OK(napi_get_value_uint32(env, argv[4], &in_len));
  NAPI_OK(napi_get_value_uint32(env, argv[5], &out_len));
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0) {
    napi_throw_range_error(env, NULL, "unknown sample format");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  if (in_data != NULL && (size_t)in_len * si.nb_channels * bin > in_bytes) {
    UNLOCK(h);
    napi_throw_range_error(env, NULL, "input frame count exceeds the chunk");
    return NULL;
  }
  /* (s16 -> s16 is the int16 call, with its counters; every other pair has the float call's) */
  const int float_entry = h->meter_on || gain_is_on(st) || !(in_fmt == SPEEXHIP_FMT_S16 && out_fmt == SPEEXHIP_FMT_S16);
  uint32_t will_use = 0, will_make = 0;
  speexhip_resampler_peek(st, in_len, out_len, float_entry, &will_use, &will_make);
  napi_value out;
  void *dst = NULL;
  NAPI_OK_LOCKED(h, napi_create_buffer(env, (size_t)will_make * si.nb_channels * bout, &dst, &out));
  uint64_t nowhere = 0;
  if (dst == NULL) dst = &nowhere; /* empty Buffer: nothing will be written, but NULL means "no buffer" */
  const int rc = speexhip_resampler_process_interleaved_fmt(st, in_fmt, in_data, &in_len, out_fmt, dst, &out_len);
  UNLOCK(h);
  if (rc != 0 || out_len != will_make) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  return out;
}

/* a mixed call's matrix: null -> (NULL, 0 values), a Float32Array -> its data */
static bool mix_matrix(napi_env env, napi_value v, const float **m, size_t *n) {
  napi_valuetype t;
  *m = NULL;
  *n = 0;
  if (napi_typeof(env, v, &t) != napi_ok) return false;
  if (t == napi_null || t == napi_undefined) return true;
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type kind;
  void *data = NULL;
  if (napi_get_typedarray_info(env, v, &kind, n, &data, NULL, NULL) != napi_ok || kind != napi_float32_array) return false;
  *m = (const float *)data;
  return true;
}

/* processMix(handle, chunk: Buffer|null, inFormat, outFormat, inFrames, outCapacityFrames, inChannels,
 * inMix: Float32Array|null, outChannels, outMix: Float32Array|null) -> Buffer of the frames written, out_channels samples of
 * outFormat each: speexhip_resampler_process_interleaved_mix on the Buffer's own memory, the result written straight into a
 * fresh Buffer of exactly the frames the call makes.  The matrices are row-major (index.js flattens them). */
static napi_value ProcessMix(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *in_data = NULL;
  size_t in_bytes = 0;
  if (!buffer_or_null(env, argv[1], &in_data, &in_bytes)) {
    napi_throw_type_error(env, NULL, "chunk must be a Buffer or null");
    return NULL;
  }
  int32_t in_fmt = -1, out_fmt = -1;
  uint32_t in_len = 0, out_len = 0, in_channels = 0, out_channels = 0;
  NAPI_OK(napi_get_value_int32(env, argv[2], &in_fmt));
  NAPI_OK(napi_get_value_int32(env, argv[3], &out_fmt));
  NAPI_OK(napi_get_value_uint32(env, argv[4], &in_len));
  NAPI_OK(napi_get_value_uint32(env, argv[5], &out_len));
  NAPI_OK(napi_get_value_uint32(env, argv[6], &in_channels));
  NAPI_OK(napi_get_value_uint32(env, argv[8], &out_channels));
  const float *in_mix = NULL, *out_mix = NULL;
  size_t in_mix_n = 0, out_mix_n = 0;
  if (!mix_matrix(env, argv[7], &in_mix, &in_mix_n) || !mix_matrix(env, argv[9], &out_mix, &out_mix_n)) {
    napi_throw_type_error(env, NULL, "a mix must be a Float32Array or null");
    return NULL;
  }
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0) {
    napi_throw_range_error(env, NULL, "unknown sample format");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  if ((in_mix != NULL && in_mix_n != (size_t)si.nb_channels * in_channels) ||
      (out_mix != NULL && out_mix_n != (size_t)si.nb_channels * out_channels)) {
    UNLOCK(h);
    napi_throw_range_error(env, NULL, "mix size does not match the channel counts");
    return NULL;
  }
  if (in_data != NULL && (size_t)in_len * in_channels * bin > in_bytes) {
    UNLOCK(h);
    napi_throw_range_error(env, NULL, "input frame count exceeds the chunk");
    return NULL;
  }
  /* (without a matrix s16 -> s16 is the int16 call, with its counters; everything else has the float call's) */
  const int float_entry = h->meter_on || gain_is_on(st) || in_mix != NULL || out_mix != NULL || !(in_fmt == SPEEXHIP_FMT_S16 && out_fmt == SPEEXHIP_FMT_S16);
  uint32_t will_use = 0, will_make = 0;
  speexhip_resampler_peek(st, in_len, out_len, float_entry, &will_use, &will_make);
  napi_value out;
  void *dst = NULL;
  NAPI_OK_LOCKED(h, napi_create_buffer(env, (size_t)will_make * out_channels * bout, &dst, &out));
  uint64_t nowhere = 0;
  if (dst == NULL) dst = &nowhere; /* empty Buffer: nothing will be written, but NULL means "no buffer" */
  const int rc = speexhip_resampler_process_interleaved_mix(st, in_fmt, in_channels, in_mix, in_data, &in_len, out_fmt,
                                                            out_channels, out_mix, dst, &out_len);
  UNLOCK(h);
  if (rc != 0 || out_len != will_make) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  return out;
}

/* bytes of an element of a typed array kind; 0 for a kind the planes of a sides call do not take */
static size_t typed_element_bytes(napi_typedarray_type t) {
  switch (t) {
    case napi_uint8_array:
    case napi_int8_array: return 1;
    case napi_int16_array:
    case napi_uint16_array: return 2;
    case napi_int32_array:
    case napi_uint32_array:
    case napi_float32_array: return 4;
    default: return 0;
  }
}

/* processSides(handle, input: Buffer | null | TypedArray[], inFormat, outFormat, inFrames, outCapacityFrames, inChannels,
 * inMix: Float32Array|null, outChannels, outMix: Float32Array|null, outPlanar: boolean, outKind: the kind of a result
 * plane's typed array) -> Buffer of interleaved frames, or one typed array per output channel: speexhip_resampler_process_sides
 * on the caller's own memory -- an array of typed arrays is a planar input, plane c being element c -- the result written
 * straight into fresh memory of exactly the frames the call makes.  index.js names the formats and picks outKind. */
static napi_value ProcessSides(napi_env env, napi_callback_info info) {
  size_t argc = 12;
  napi_value argv[12];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t in_fmt = -1, out_fmt = -1, out_kind = 0;
  uint32_t in_len = 0, out_len = 0, in_channels = 0, out_channels = 0;
  bool out_planar = false, in_planar = false;
  NAPI_OK(napi_get_value_int32(env, argv[2], &in_fmt));
  NAPI_OK(napi_get_value_int32(env, argv[3], &out_fmt));
  NAPI_OK(napi_get_value_uint32(env, argv[4], &in_len));
  NAPI_OK(napi_get_value_uint32(env, argv[5], &out_len));
  NAPI_OK(napi_get_value_uint32(env, argv[6], &in_channels));
  NAPI_OK(napi_get_value_uint32(env, argv[8], &out_channels));
  NAPI_OK(napi_get_value_bool(env, argv[10], &out_planar));
  NAPI_OK(napi_get_value_int32(env, argv[11], &out_kind));
  const float *in_mix = NULL, *out_mix = NULL;
  size_t in_mix_n = 0, out_mix_n = 0;
  if (!mix_matrix(env, argv[7], &in_mix, &in_mix_n) || !mix_matrix(env, argv[9], &out_mix, &out_mix_n)) {
    napi_throw_type_error(env, NULL, "a mix must be a Float32Array or null");
    return NULL;
  }
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0 || in_channels == 0 || out_channels == 0 || in_channels > 64 || out_channels > 64) {
    napi_throw_range_error(env, NULL, "unknown sample format or channel count");
    return NULL;
  }
  /* (index.js names a result plane's kind: 0 Uint8Array, 1 Int16Array, 2 Int32Array, 3 Float32Array, 4 Uint16Array) */
  static const napi_typedarray_type kKinds[5] = {napi_uint8_array, napi_int16_array, napi_int32_array, napi_float32_array,
                                                 napi_uint16_array};
  if (out_kind < 0 || out_kind > 4) {
    napi_throw_range_error(env, NULL, "unknown kind of result plane");
    return NULL;
  }
  const napi_typedarray_type out_type = kKinds[out_kind];
  const size_t out_es = typed_element_bytes(out_type);
  if (out_planar && (out_es == 0 || bout % out_es != 0)) {
    napi_throw_range_error(env, NULL, "the result's typed array kind does not hold its format");
    return NULL;
  }
  void *in_planes[64], *out_planes[64];
  void *in_data = NULL;
  size_t in_bytes = 0;
  NAPI_OK(napi_is_array(env, argv[1], &in_planar));
  if (in_planar) {
    uint32_t n = 0;
    NAPI_OK(napi_get_array_length(env, argv[1], &n));
    if (n != in_channels) {
      napi_throw_range_error(env, NULL, "one typed array per input channel is expected");
      return NULL;
    }
    for (uint32_t c = 0; c < n; c++) {
      napi_value v;
      napi_typedarray_type t;
      size_t len = 0;
      void *data = NULL;
      bool typed = false;
      if (napi_get_element(env, argv[1], c, &v) != napi_ok || napi_is_typedarray(env, v, &typed) != napi_ok || !typed ||
          napi_get_typedarray_info(env, v, &t, &len, &data, NULL, NULL) != napi_ok || typed_element_bytes(t) == 0) {
        napi_throw_type_error(env, NULL, "a planar input must be an array of typed arrays");
        return NULL;
      }
      if ((size_t)in_len * bin > len * typed_element_bytes(t)) {
        napi_throw_range_error(env, NULL, "input frame count exceeds a plane");
        return NULL;
      }
      in_planes[c] = data != NULL ? data : (void *)in_planes; /* (an empty array: nothing is read, but NULL means "no plane") */
    }
  } else if (!buffer_or_null(env, argv[1], &in_data, &in_bytes)) {
    napi_throw_type_error(env, NULL, "input must be a Buffer, null or an array of typed arrays");
    return NULL;
  } else if (in_data != NULL && (size_t)in_len * in_channels * bin > in_bytes) {
    napi_throw_range_error(env, NULL, "input frame count exceeds the chunk");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  if ((in_mix != NULL && in_mix_n != (size_t)si.nb_channels * in_channels) ||
      (out_mix != NULL && out_mix_n != (size_t)si.nb_channels * out_channels)) {
    UNLOCK(h);
    napi_throw_range_error(env, NULL, "mix size does not match the channel counts");
    return NULL;
  }
  /* (a side of one channel is the same bytes in either layout; with a planar side, as with a matrix, every pair has the
   *  float call's counters -- otherwise s16 -> s16 is the int16 call) */
  const int planar_side = (in_planar && in_channels > 1) || (out_planar && out_channels > 1);
  const int float_entry = h->meter_on || gain_is_on(st) || planar_side || in_mix != NULL || out_mix != NULL || !(in_fmt == SPEEXHIP_FMT_S16 && out_fmt == SPEEXHIP_FMT_S16);
  uint32_t will_use = 0, will_make = 0;
  speexhip_resampler_peek(st, in_len, out_len, float_entry, &will_use, &will_make);
  napi_value result = NULL;
  uint64_t nowhere = 0;
  SpeexHipSide in_side, out_side;
  memset(&in_side, 0, sizeof(in_side));
  memset(&out_side, 0, sizeof(out_side));
  in_side.struct_size = out_side.struct_size = (uint32_t)sizeof(SpeexHipSide);
  in_side.fmt = in_fmt;
  in_side.channels = in_channels;
  in_side.mix = in_mix;
  in_side.layout = in_planar ? SPEEXHIP_LAYOUT_PLANAR : SPEEXHIP_LAYOUT_INTERLEAVED;
  in_side.data = in_data;
  in_side.planes = in_planar ? in_planes : NULL;
  out_side.fmt = out_fmt;
  out_side.channels = out_channels;
  out_side.mix = out_mix;
  out_side.layout = out_planar ? SPEEXHIP_LAYOUT_PLANAR : SPEEXHIP_LAYOUT_INTERLEAVED;
  if (out_planar) {
    NAPI_OK_LOCKED(h, napi_create_array_with_length(env, out_channels, &result));
    for (uint32_t c = 0; c < out_channels; c++) {
      napi_value ab, ta;
      void *dst = NULL;
      NAPI_OK_LOCKED(h, napi_create_arraybuffer(env, (size_t)will_make * bout, &dst, &ab));
      NAPI_OK_LOCKED(h, napi_create_typedarray(env, out_type, (size_t)will_make * bout / out_es, ab, 0, &ta));
      NAPI_OK_LOCKED(h, napi_set_element(env, result, c, ta));
      out_planes[c] = will_make != 0 && dst != NULL ? dst : (void *)&nowhere;
    }
    out_side.planes = out_planes;
  } else {
    void *dst = NULL;
    NAPI_OK_LOCKED(h, napi_create_buffer(env, (size_t)will_make * out_channels * bout, &dst, &result));
    out_side.data = dst != NULL ? dst : (void *)&nowhere; /* empty Buffer: nothing will be written, but NULL means "no buffer" */
  }
  const int rc = speexhip_resampler_process_sides(st, &in_side, &in_len, &out_side, &out_len);
  UNLOCK(h);
  if (rc != 0 || out_len != will_make) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(rc != 0 ? rc : SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  return result;
}

/* processChunks(handle, chunks: Buffer[], inFrames: number[], outCapacities: number[]) -> Buffer[]
 * n consecutive process() calls as one transfer + one launch
 * (speexhip_resampler_process_chunks_int); the i-th Buffer is what the i-th call returns. */
static napi_value ProcessChunks(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, argv[1], &n));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  const size_t frame_bytes = (size_t)si.nb_channels * 2;
  const int16_t **ptrs = (const int16_t **)calloc(n ? n : 1, sizeof(*ptrs));
  uint32_t *in_len = (uint32_t *)calloc(n ? n : 1, sizeof(uint32_t));
  uint32_t *out_len = (uint32_t *)calloc(n ? n : 1, sizeof(uint32_t));
  int16_t *tmp = NULL;
  napi_value result = NULL;
  const char *fail = NULL;
  size_t total_cap = 0;
  if (ptrs == NULL || in_len == NULL || out_len == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  for (uint32_t i = 0; fail == NULL && i < n; i++) {
    napi_value c, a, b;
    void *data = NULL;
    size_t bytes = 0;
    if (napi_get_element(env, argv[1], i, &c) != napi_ok || napi_get_element(env, argv[2], i, &a) != napi_ok ||
        napi_get_element(env, argv[3], i, &b) != napi_ok || !buffer_or_null(env, c, &data, &bytes) ||
        napi_get_value_uint32(env, a, &in_len[i]) != napi_ok ||
        napi_get_value_uint32(env, b, &out_len[i]) != napi_ok) {
      fail = "processChunks expects (handle, Buffer[], number[], number[])";
    } else if (data != NULL && (size_t)in_len[i] * frame_bytes > bytes) {
      fail = "input frame count exceeds the chunk";
    }
    ptrs[i] = (const int16_t *)data;
    total_cap += out_len[i];
  }
  if (fail == NULL) {
    tmp = (int16_t *)malloc(total_cap * frame_bytes + 2);
    if (tmp == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  }
  if (fail == NULL) {
    int rc = speexhip_resampler_process_chunks_int(st, n, ptrs, in_len, tmp, out_len);
    if (rc != 0) fail = speexhip_resampler_strerror(rc);
  }
  UNLOCK(h);
  if (fail == NULL && napi_create_array_with_length(env, n, &result) == napi_ok) {
    size_t off = 0;
    for (uint32_t i = 0; i < n; i++) {
      napi_value buf;
      void *copied = NULL;
      if (napi_create_buffer_copy(env, (size_t)out_len[i] * frame_bytes, (char *)tmp + off, &copied, &buf) != napi_ok ||
          napi_set_element(env, result, i, buf) != napi_ok) {
        fail = "speexhip N-API failure: building the result array";
        break;
      }
      off += (size_t)out_len[i] * frame_bytes;
    }
  }
  free(tmp);
  free(ptrs);
  free(in_len);
  free(out_len);
  if (fail != NULL) {
    napi_throw_error(env, NULL, fail);
    return NULL;
  }
  return result;
}

/* processChunksAsync(handle, chunks[], inFrames[], outCapacities[]) -> Promise<Buffer[]>: processChunks on a libuv pool
 * thread (the Transform's `pipeline` option: chunks that arrive while a call is in flight leave together as the next) */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref handle_ref;
  napi_ref *chunk_refs;
  Handle *h;
  uint32_t n, channels;
  const int16_t **ptrs;
  uint32_t *in_len, *out_len;
  int16_t *tmp;
  int rc;
  char errmsg[256];
} ChunksJob;

static void chunks_free(napi_env env, ChunksJob *j) {
  if (j == NULL) return;
  if (j->chunk_refs != NULL)
    for (uint32_t i = 0; i < j->n; i++)
      if (j->chunk_refs[i] != NULL) napi_delete_reference(env, j->chunk_refs[i]);
  if (j->handle_ref != NULL) napi_delete_reference(env, j->handle_ref);
  free(j->chunk_refs);
  free(j->ptrs);
  free(j->in_len);
  free(j->out_len);
  free(j->tmp);
  free(j);
}
static void chunks_execute(napi_env env, void *data) {
  (void)env;
  ChunksJob *j = (ChunksJob *)data;
  pthread_mutex_lock(&j->h->lock);
  j->rc = j->h->st == NULL ? SPEEXHIP_ERR_BAD_STATE
                           : speexhip_resampler_process_chunks_int(j->h->st, j->n, j->ptrs, j->in_len, j->tmp, j->out_len);
  if (j->rc != 0) snprintf(j->errmsg, sizeof(j->errmsg), "%s", speexhip_resampler_strerror(j->rc));
  pthread_mutex_unlock(&j->h->lock);
}
static void chunks_complete(napi_env env, napi_status status, void *data) {
  ChunksJob *j = (ChunksJob *)data;
  napi_value v, result;
  int ok = status == napi_ok && j->rc == 0 && napi_create_array_with_length(env, j->n, &result) == napi_ok;
  if (ok) {
    size_t off = 0;
    const size_t frame_bytes = (size_t)j->channels * 2;
    for (uint32_t i = 0; ok && i < j->n; i++) {
      napi_value buf;
      void *copied = NULL;
      ok = napi_create_buffer_copy(env, (size_t)j->out_len[i] * frame_bytes, (char *)j->tmp + off, &copied, &buf) == napi_ok &&
           napi_set_element(env, result, i, buf) == napi_ok;
      off += (size_t)j->out_len[i] * frame_bytes;
    }
  }
  if (ok) {
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, j->rc != 0 ? j->errmsg : "speexhip: asynchronous call failed", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    napi_reject_deferred(env, j->deferred, v);
  }
  napi_delete_async_work(env, j->work);
  chunks_free(env, j);
}
static napi_value ProcessChunksAsync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, argv[1], &n));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si); /* only the channel count is used: it never changes */
  UNLOCK(h);
  const size_t frame_bytes = (size_t)si.nb_channels * 2, m = n ? n : 1;
  ChunksJob *j = (ChunksJob *)calloc(1, sizeof(ChunksJob));
  const char *fail = NULL;
  if (j != NULL) {
    j->n = n;
    j->h = h;
    j->channels = si.nb_channels;
    j->chunk_refs = (napi_ref *)calloc(m, sizeof(napi_ref));
    j->ptrs = (const int16_t **)calloc(m, sizeof(*j->ptrs));
    j->in_len = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->out_len = (uint32_t *)calloc(m, sizeof(uint32_t));
  }
  if (j == NULL || !j->chunk_refs || !j->ptrs || !j->in_len || !j->out_len) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  size_t total_cap = 0;
  for (uint32_t i = 0; fail == NULL && i < n; i++) {
    napi_value c, a, b;
    void *data = NULL;
    size_t bytes = 0;
    if (napi_get_element(env, argv[1], i, &c) != napi_ok || napi_get_element(env, argv[2], i, &a) != napi_ok ||
        napi_get_element(env, argv[3], i, &b) != napi_ok || !buffer_or_null(env, c, &data, &bytes) ||
        napi_get_value_uint32(env, a, &j->in_len[i]) != napi_ok || napi_get_value_uint32(env, b, &j->out_len[i]) != napi_ok) {
      fail = "processChunksAsync expects (handle, Buffer[], number[], number[])";
    } else if (data != NULL && (size_t)j->in_len[i] * frame_bytes > bytes) {
      fail = "input frame count exceeds the chunk";
    } else if (data != NULL && napi_create_reference(env, c, 1, &j->chunk_refs[i]) != napi_ok) { /* keep the bytes alive */
      fail = "speexhip N-API failure: napi_create_reference";
    }
    j->ptrs[i] = (const int16_t *)data;
    total_cap += j->out_len[i];
  }
  napi_value promise = NULL, name;
  if (fail == NULL && (j->tmp = (int16_t *)malloc(total_cap * frame_bytes + 2)) == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  if (fail == NULL &&
      (napi_create_reference(env, argv[0], 1, &j->handle_ref) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
       napi_create_string_utf8(env, "speexhip.processChunksAsync", NAPI_AUTO_LENGTH, &name) != napi_ok ||
       napi_create_async_work(env, NULL, name, chunks_execute, chunks_complete, j, &j->work) != napi_ok ||
       napi_queue_async_work(env, j->work) != napi_ok))
    fail = "speexhip N-API failure: queueing processChunksAsync";
  if (fail != NULL) {
    chunks_free(env, j);
    napi_throw_error(env, NULL, fail);
    return NULL;
  }
  return promise;
}

/* processChunksFormat(handle, chunks: (Buffer|null)[], inFormat, outFormat, inFrames: number[], outCapacities: number[])
 * -> Buffer[]: n consecutive processFormat() calls as one transfer each way and one wait
 * (speexhip_resampler_process_chunks_fmt); the i-th Buffer is what the i-th call returns, in outFormat.
 * processChunksFormatAsync: the same on a libuv pool thread -> Promise<Buffer[]>.  One job serves both. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref handle_ref;
  napi_ref *chunk_refs; /* (the asynchronous form keeps the chunks' bytes alive) */
  Handle *h;
  uint32_t n;
  int32_t in_fmt, out_fmt;
  size_t out_frame_bytes;
  const void **ptrs;
  uint32_t *in_len, *out_len;
  char *tmp;
  int rc;
  char errmsg[256];
} FmtChunksJob;

static void fmt_chunks_free(napi_env env, FmtChunksJob *j) {
  if (j == NULL) return;
  if (j->chunk_refs != NULL)
    for (uint32_t i = 0; i < j->n; i++)
      if (j->chunk_refs[i] != NULL) napi_delete_reference(env, j->chunk_refs[i]);
  if (j->handle_ref != NULL) napi_delete_reference(env, j->handle_ref);
  free(j->chunk_refs);
  free(j->ptrs);
  free(j->in_len);
  free(j->out_len);
  free(j->tmp);
  free(j);
}
/* the arguments as a job; NULL with an exception pending */
static FmtChunksJob *fmt_chunks_prepare(napi_env env, napi_callback_info info, int keep_refs, napi_value *handle) {
  size_t argc = 6;
  napi_value argv[6];
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 6) {
    napi_throw_type_error(env, NULL, "processChunksFormat expects (handle, Buffer[], inFormat, outFormat, number[], number[])");
    return NULL;
  }
  uint32_t n = 0;
  int32_t in_fmt = -1, out_fmt = -1;
  if (napi_get_array_length(env, argv[1], &n) != napi_ok || napi_get_value_int32(env, argv[2], &in_fmt) != napi_ok ||
      napi_get_value_int32(env, argv[3], &out_fmt) != napi_ok) {
    napi_throw_type_error(env, NULL, "processChunksFormat expects (handle, Buffer[], inFormat, outFormat, number[], number[])");
    return NULL;
  }
  const size_t bin = speexhip_sample_bytes(in_fmt), bout = speexhip_sample_bytes(out_fmt);
  if (bin == 0 || bout == 0) {
    napi_throw_range_error(env, NULL, "unknown sample format");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si); /* only the channel count is used: it never changes */
  UNLOCK(h);
  const size_t in_frame_bytes = (size_t)si.nb_channels * bin, m = n ? n : 1;
  FmtChunksJob *j = (FmtChunksJob *)calloc(1, sizeof(FmtChunksJob));
  const char *fail = NULL;
  if (j != NULL) {
    j->n = n;
    j->h = h;
    j->in_fmt = in_fmt;
    j->out_fmt = out_fmt;
    j->out_frame_bytes = (size_t)si.nb_channels * bout;
    j->chunk_refs = (napi_ref *)calloc(m, sizeof(napi_ref));
    j->ptrs = (const void **)calloc(m, sizeof(*j->ptrs));
    j->in_len = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->out_len = (uint32_t *)calloc(m, sizeof(uint32_t));
  }
  if (j == NULL || !j->chunk_refs || !j->ptrs || !j->in_len || !j->out_len) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  size_t total_cap = 0;
  for (uint32_t i = 0; fail == NULL && i < n; i++) {
    napi_value c, a, b;
    void *data = NULL;
    size_t bytes = 0;
    if (napi_get_element(env, argv[1], i, &c) != napi_ok || napi_get_element(env, argv[4], i, &a) != napi_ok ||
        napi_get_element(env, argv[5], i, &b) != napi_ok || !buffer_or_null(env, c, &data, &bytes) ||
        napi_get_value_uint32(env, a, &j->in_len[i]) != napi_ok || napi_get_value_uint32(env, b, &j->out_len[i]) != napi_ok) {
      fail = "processChunksFormat expects (handle, Buffer[], inFormat, outFormat, number[], number[])";
    } else if (data != NULL && (size_t)j->in_len[i] * in_frame_bytes > bytes) {
      fail = "input frame count exceeds the chunk";
    } else if (keep_refs && data != NULL && napi_create_reference(env, c, 1, &j->chunk_refs[i]) != napi_ok) {
      fail = "speexhip N-API failure: napi_create_reference";
    }
    j->ptrs[i] = data;
    total_cap += j->out_len[i];
  }
  if (fail == NULL && (j->tmp = (char *)malloc(total_cap * j->out_frame_bytes + 8)) == NULL)
    fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  if (fail != NULL) {
    fmt_chunks_free(env, j);
    napi_throw_error(env, NULL, fail);
    return NULL;
  }
  *handle = argv[0];
  return j;
}
static void fmt_chunks_run(FmtChunksJob *j) {
  pthread_mutex_lock(&j->h->lock);
  j->rc = j->h->st == NULL ? SPEEXHIP_ERR_BAD_STATE
                           : speexhip_resampler_process_chunks_fmt(j->h->st, j->n, j->in_fmt, j->ptrs, j->in_len, j->out_fmt,
                                                                   j->tmp, j->out_len);
  if (j->rc != 0) snprintf(j->errmsg, sizeof(j->errmsg), "%s", speexhip_resampler_strerror(j->rc));
  pthread_mutex_unlock(&j->h->lock);
}
/* the per-chunk Buffers of a job that ran; 0: N-API failure */
static int fmt_chunks_result(napi_env env, const FmtChunksJob *j, napi_value *result) {
  if (napi_create_array_with_length(env, j->n, result) != napi_ok) return 0;
  size_t off = 0;
  for (uint32_t i = 0; i < j->n; i++) {
    napi_value buf;
    void *copied = NULL;
    const size_t bytes = (size_t)j->out_len[i] * j->out_frame_bytes;
    if (napi_create_buffer_copy(env, bytes, j->tmp + off, &copied, &buf) != napi_ok ||
        napi_set_element(env, *result, i, buf) != napi_ok)
      return 0;
    off += bytes;
  }
  return 1;
}
static napi_value ProcessChunksFormat(napi_env env, napi_callback_info info) {
  napi_value handle, result = NULL;
  FmtChunksJob *j = fmt_chunks_prepare(env, info, 0, &handle);
  if (j == NULL) return NULL;
  fmt_chunks_run(j);
  const char *fail = j->rc != 0 ? j->errmsg : fmt_chunks_result(env, j, &result) ? NULL : "speexhip N-API failure: building the result array";
  if (fail != NULL) napi_throw_error(env, NULL, fail);
  fmt_chunks_free(env, j);
  return fail != NULL ? NULL : result;
}
static void fmt_chunks_execute(napi_env env, void *data) {
  (void)env;
  fmt_chunks_run((FmtChunksJob *)data);
}
static void fmt_chunks_complete(napi_env env, napi_status status, void *data) {
  FmtChunksJob *j = (FmtChunksJob *)data;
  napi_value v, result;
  if (status == napi_ok && j->rc == 0 && fmt_chunks_result(env, j, &result)) {
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, j->rc != 0 ? j->errmsg : "speexhip: asynchronous call failed", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    napi_reject_deferred(env, j->deferred, v);
  }
  napi_delete_async_work(env, j->work);
  fmt_chunks_free(env, j);
}
static napi_value ProcessChunksFormatAsync(napi_env env, napi_callback_info info) {
  napi_value handle, promise = NULL, name;
  FmtChunksJob *j = fmt_chunks_prepare(env, info, 1, &handle);
  if (j == NULL) return NULL;
  if (napi_create_reference(env, handle, 1, &j->handle_ref) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "speexhip.processChunksFormatAsync", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, fmt_chunks_execute, fmt_chunks_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    fmt_chunks_free(env, j);
    napi_throw_error(env, NULL, "speexhip N-API failure: queueing processChunksFormatAsync");
    return NULL;
  }
  return promise;
}

/* processAsync(handle, chunk, inFrames, outCapacityFrames) -> Promise<Buffer>: the same call on
 * a libuv pool thread, so H2D + kernels + D2H do not block the event loop.  The caller
 * (index.js) chains the promises of one instance, so calls on one state stay in order. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref chunk_ref, handle_ref;
  Handle *h;
  const int16_t *in;
  int16_t *out;
  uint32_t in_len, out_len, channels;
  int rc;
  char errmsg[256];
} AsyncJob;

static void async_execute(napi_env env, void *data) {
  (void)env;
  AsyncJob *j = (AsyncJob *)data;
  pthread_mutex_lock(&j->h->lock);
  if (j->h->st == NULL) {
    j->rc = SPEEXHIP_ERR_BAD_STATE;
  } else {
    j->rc = speexhip_resampler_process_interleaved_int(j->h->st, j->in, &j->in_len, j->out, &j->out_len);
  }
  /* DEVICE errors keep their text per thread: fetch it on the thread that failed */
  if (j->rc != 0) snprintf(j->errmsg, sizeof(j->errmsg), "%s", speexhip_resampler_strerror(j->rc));
  pthread_mutex_unlock(&j->h->lock);
}

static void async_complete(napi_env env, napi_status status, void *data) {
  AsyncJob *j = (AsyncJob *)data;
  napi_value v;
  if (status == napi_ok && j->rc == 0) {
    void *copied = NULL;
    if (napi_create_buffer_copy(env, (size_t)j->out_len * j->channels * 2, j->out, &copied, &v) == napi_ok)
      napi_resolve_deferred(env, j->deferred, v);
    else
      status = napi_generic_failure;
  }
  if (status != napi_ok || j->rc != 0) {
    napi_value msg;
    napi_create_string_utf8(env, j->rc != 0 ? j->errmsg : "speexhip: asynchronous call failed", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    napi_reject_deferred(env, j->deferred, v);
  }
  if (j->chunk_ref) napi_delete_reference(env, j->chunk_ref);
  napi_delete_reference(env, j->handle_ref);
  napi_delete_async_work(env, j->work);
  free(j->out);
  free(j);
}

static napi_value ProcessAsync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *in_data = NULL;
  size_t in_bytes = 0;
  if (!buffer_or_null(env, argv[1], &in_data, &in_bytes)) {
    napi_throw_type_error(env, NULL, "chunk must be a Buffer or null");
    return NULL;
  }
  uint32_t in_len = 0, out_len = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[2], &in_len));
  NAPI_OK(napi_get_value_uint32(env, argv[3], &out_len));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si); /* only the channel count is used: it never changes */
  UNLOCK(h);
  if (in_data != NULL && (size_t)in_len * si.nb_channels * 2 > in_bytes) {
    napi_throw_range_error(env, NULL, "input frame count exceeds the chunk");
    return NULL;
  }
  AsyncJob *j = (AsyncJob *)calloc(1, sizeof(AsyncJob));
  if (j != NULL) j->out = (int16_t *)malloc((size_t)out_len * si.nb_channels * 2 + 2);
  if (j == NULL || j->out == NULL) {
    free(j);
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED));
    return NULL;
  }
  j->h = h;
  j->in = (const int16_t *)in_data;
  j->in_len = in_len;
  j->out_len = out_len;
  j->channels = si.nb_channels;
  napi_value promise, name;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  if (in_data != NULL) NAPI_OK(napi_create_reference(env, argv[1], 1, &j->chunk_ref)); /* keep the bytes alive */
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->handle_ref));
  NAPI_OK(napi_create_string_utf8(env, "speexhip.processAsync", NAPI_AUTO_LENGTH, &name));
  NAPI_OK(napi_create_async_work(env, NULL, name, async_execute, async_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* ---- mid-stream control: each throws Error(strerror(code)) on failure ---- */
static napi_value control_result(napi_env env, int rc) {
  if (rc != 0) napi_throw_error(env, NULL, speexhip_resampler_strerror(rc));
  return NULL;
}

static napi_value SetRate(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  uint32_t v[4] = {0, 0, 0, 0};
  for (size_t i = 1; i < argc && i < 5; i++) NAPI_OK_LOCKED(h, napi_get_value_uint32(env, argv[i], &v[i - 1]));
  /* (handle, inRate, outRate) or (handle, ratioNum, ratioDen, inRate, outRate) */
  const int rc = argc >= 5 ? speexhip_resampler_set_rate_frac(st, v[0], v[1], v[2], v[3])
                           : speexhip_resampler_set_rate(st, v[0], v[1]);
  UNLOCK(h);
  return control_result(env, rc);
}

static napi_value SetQuality(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  int32_t q = 0;
  NAPI_OK_LOCKED(h, napi_get_value_int32(env, argv[1], &q));
  const int rc = speexhip_resampler_set_quality(st, q);
  UNLOCK(h);
  return control_result(env, rc);
}

static napi_value SkipZeros(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  const int rc = speexhip_resampler_skip_zeros(st);
  UNLOCK(h);
  return control_result(env, rc);
}

static napi_value ResetMem(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  const int rc = speexhip_resampler_reset_mem(st);
  UNLOCK(h);
  return control_result(env, rc);
}

/* setDither(handle, kind, seedLo, seedHi, positionLo, positionHi): the 64-bit values travel as uint32 halves (index.js
 * splits and joins the BigInts) */
static napi_value SetDither(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "setDither(handle, kind, seedLo, seedHi, positionLo, positionHi)");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  int32_t kind = 0;
  uint32_t v[4] = {0, 0, 0, 0};
  NAPI_OK_LOCKED(h, napi_get_value_int32(env, argv[1], &kind));
  for (size_t i = 0; i < 4; i++) NAPI_OK_LOCKED(h, napi_get_value_uint32(env, argv[2 + i], &v[i]));
  const int rc = speexhip_resampler_set_dither(st, kind, ((uint64_t)v[1] << 32) | v[0], ((uint64_t)v[3] << 32) | v[2]);
  UNLOCK(h);
  return control_result(env, rc);
}

/* getDither(handle) -> [kind, seedLo, seedHi, positionLo, positionHi] */
static napi_value GetDither(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  int kind = 0;
  uint64_t seed = 0, position = 0;
  const int rc = speexhip_resampler_get_dither(st, &kind, &seed, &position);
  UNLOCK(h);
  if (rc != 0) return control_result(env, rc);
  const uint32_t out[5] = {(uint32_t)kind, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)position,
                           (uint32_t)(position >> 32)};
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 5, &arr));
  for (uint32_t i = 0; i < 5; i++) {
    NAPI_OK(napi_create_uint32(env, out[i], &v));
    NAPI_OK(napi_set_element(env, arr, i, v));
  }
  return arr;
}

/* setMeter(handle, on) */
static napi_value SetMeter(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "setMeter(handle, on)");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  bool on = false;
  NAPI_OK_LOCKED(h, napi_get_value_bool(env, argv[1], &on));
  const int rc = speexhip_resampler_set_meter(st, on ? 1 : 0);
  if (rc == 0) h->meter_on = on ? 1 : 0;
  UNLOCK(h);
  return control_result(env, rc);
}

/* getMeter(handle, reset) -> [on, samplesLo, samplesHi, highLo, highHi, lowLo, lowHi, nanLo, nanHi, peak]: the counts
 * travel as uint32 halves (index.js joins them into BigInts), the peak as a number */
static napi_value GetMeter(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "getMeter(handle, reset)");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  bool reset = false;
  NAPI_OK_LOCKED(h, napi_get_value_bool(env, argv[1], &reset));
  SpeexHipMeter m;
  memset(&m, 0, sizeof(m));
  m.struct_size = (uint32_t)sizeof(m);
  const int rc = speexhip_resampler_get_meter(st, &m, reset ? 1 : 0);
  UNLOCK(h);
  if (rc != 0) return control_result(env, rc);
  const uint64_t counts[4] = {m.samples, m.clipped_high, m.clipped_low, m.nan};
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 10, &arr));
  NAPI_OK(napi_create_uint32(env, m.on, &v));
  NAPI_OK(napi_set_element(env, arr, 0, v));
  for (uint32_t i = 0; i < 4; i++) {
    NAPI_OK(napi_create_uint32(env, (uint32_t)counts[i], &v));
    NAPI_OK(napi_set_element(env, arr, 1 + 2 * i, v));
    NAPI_OK(napi_create_uint32(env, (uint32_t)(counts[i] >> 32), &v));
    NAPI_OK(napi_set_element(env, arr, 2 + 2 * i, v));
  }
  NAPI_OK(napi_create_double(env, (double)m.peak, &v));
  NAPI_OK(napi_set_element(env, arr, 9, v));
  return arr;
}

/* setGain(handle, gain, rampFrames) */
static napi_value SetGain(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "setGain(handle, gain, rampFrames)");
    return NULL;
  }
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  double gain = 1.0;
  uint32_t ramp = 0;
  NAPI_OK_LOCKED(h, napi_get_value_double(env, argv[1], &gain));
  NAPI_OK_LOCKED(h, napi_get_value_uint32(env, argv[2], &ramp));
  const int rc = speexhip_resampler_set_gain(st, (float)gain, ramp);
  UNLOCK(h);
  return control_result(env, rc);
}

/* getGain(handle) -> [current, target, remaining] */
static napi_value GetGain(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  float current = 1.0f, target = 1.0f;
  uint32_t remaining = 0;
  const int rc = speexhip_resampler_get_gain(st, &current, &target, &remaining);
  UNLOCK(h);
  if (rc != 0) return control_result(env, rc);
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 3, &arr));
  NAPI_OK(napi_create_double(env, (double)current, &v));
  NAPI_OK(napi_set_element(env, arr, 0, v));
  NAPI_OK(napi_create_double(env, (double)target, &v));
  NAPI_OK(napi_set_element(env, arr, 1, v));
  NAPI_OK(napi_create_uint32(env, remaining, &v));
  NAPI_OK(napi_set_element(env, arr, 2, v));
  return arr;
}

static napi_value pair_u32(napi_env env, uint32_t a, uint32_t b) {
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 2, &arr));
  NAPI_OK(napi_create_uint32(env, a, &v));
  NAPI_OK(napi_set_element(env, arr, 0, v));
  NAPI_OK(napi_create_uint32(env, b, &v));
  NAPI_OK(napi_set_element(env, arr, 1, v));
  return arr;
}

/* getLatency(handle) -> [inputLatencyFrames, outputLatencyFrames] */
static napi_value GetLatency(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  const uint32_t in_lat = (uint32_t)speexhip_resampler_get_input_latency(st);
  const uint32_t out_lat = (uint32_t)speexhip_resampler_get_output_latency(st);
  UNLOCK(h);
  return pair_u32(env, in_lat, out_lat);
}

static napi_value SetMode(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  int32_t mode = 0;
  NAPI_OK_LOCKED(h, napi_get_value_int32(env, argv[1], &mode));
  const int rc = speexhip_resampler_set_mode(st, mode);
  UNLOCK(h);
  return control_result(env, rc);
}

static napi_value GetInfo(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  SpeexHipInfo si;
  speexhip_resampler_get_info(st, &si);
  UNLOCK(h);
  napi_value obj, v;
  NAPI_OK(napi_create_object(env, &obj));
#define PUT_U32(name)                                     \
  NAPI_OK(napi_create_uint32(env, si.name, &v));          \
  NAPI_OK(napi_set_named_property(env, obj, #name, v));
#define PUT_I32(name)                                     \
  NAPI_OK(napi_create_int32(env, si.name, &v));           \
  NAPI_OK(napi_set_named_property(env, obj, #name, v));
  PUT_U32(in_rate) PUT_U32(out_rate) PUT_U32(num_rate) PUT_U32(den_rate) PUT_U32(nb_channels)
  PUT_I32(quality) PUT_U32(filt_len) PUT_U32(oversample) PUT_U32(sinc_table_length) PUT_I32(kernel)
  PUT_I32(mode) PUT_I32(fast_path) PUT_I32(last_sample) PUT_U32(samp_frac_num) PUT_I32(device)
  PUT_U32(magic_samples) PUT_U32(block_in) PUT_I32(accumulate_bits)
  return obj;
}

/* getRate(handle) -> [inRate, outRate]  (speex_resampler_get_rate; exported but unused by
 * src/index.ts, kept for surface parity) */
static napi_value GetRate(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  Handle *h = NULL;
  SpeexHipResamplerState *st = lock_state(env, argv[0], &h);
  if (st == NULL) return NULL;
  uint32_t a = 0, b = 0;
  speexhip_resampler_get_rate(st, &a, &b);
  UNLOCK(h);
  return pair_u32(env, a, b);
}

static napi_value StrError(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t code = 0;
  NAPI_OK(napi_get_value_int32(env, argv[0], &code));
  napi_value s;
  NAPI_OK(napi_create_string_utf8(env, speexhip_resampler_strerror(code), NAPI_AUTO_LENGTH, &s));
  return s;
}

static napi_value Version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value s;
  NAPI_OK(napi_create_string_utf8(env, speexhip_version(), NAPI_AUTO_LENGTH, &s));
  return s;
}

/* releaseCachedMemory() -> bytes handed back to the driver (speexhip_release_cached_memory) */
static napi_value ReleaseCachedMemory(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value v;
  NAPI_OK(napi_create_double(env, (double)speexhip_release_cached_memory(), &v));
  return v;
}

/* ---- many states, one call (speexhip_resampler_process_many_int): SpeexResamplerBatch.processChunks and the
 * coalescer of processChunkAsync calls issued in one tick (index.js) ---- */
typedef struct {
  uint32_t n;
  Handle **h;               /* per entry */
  Handle **locked;          /* the distinct handles, sorted by address (lock order) */
  uint32_t n_locked;
  SpeexHipResamplerState **st;
  const int16_t **in;
  int16_t **out;
  uint32_t *in_len, *out_len, *will_make, *channels;
  int *codes;
  /* processManyFormat: a sample format per entry and side (SPEEXHIP_FMT_*), and whether the entry is sized by the float
   * entry's rules -- every pair but S16 -> S16 without dither; NULL in processMany, whose entries are all S16 -> S16 calls */
  int *in_fmt, *out_fmt, *float_entry;
  /* asynchronous form */
  napi_async_work work;
  napi_deferred deferred;
  napi_ref *refs;           /* handles, chunks, result Buffers: 3 per entry (chunk ref may be NULL) */
  napi_ref result_ref;      /* the result array */
  int rc;
  int ran;                  /* the library call was made: codes[] says which entries succeeded */
  char errmsg[256];
} ManyJob;

static void many_free(napi_env env, ManyJob *j) {
  if (j == NULL) return;
  if (j->refs != NULL) {
    for (uint32_t i = 0; i < 3 * j->n; i++)
      if (j->refs[i] != NULL) napi_delete_reference(env, j->refs[i]);
  }
  if (j->result_ref != NULL) napi_delete_reference(env, j->result_ref);
  free(j->h);
  free(j->locked);
  free(j->st);
  free(j->in);
  free(j->out);
  free(j->in_len);
  free(j->out_len);
  free(j->will_make);
  free(j->channels);
  free(j->codes);
  free(j->in_fmt);
  free(j->out_fmt);
  free(j->float_entry);
  free(j->refs);
  free(j);
}

static int cmp_handle(const void *a, const void *b) {
  const uintptr_t x = (uintptr_t)*(Handle *const *)a, y = (uintptr_t)*(Handle *const *)b;
  return x < y ? -1 : x > y;
}
static void many_lock(ManyJob *j) {
  for (uint32_t k = 0; k < j->n_locked; k++) pthread_mutex_lock(&j->locked[k]->lock);
}
static void many_unlock(ManyJob *j) {
  for (uint32_t k = j->n_locked; k-- > 0;) pthread_mutex_unlock(&j->locked[k]->lock);
}
/* the call itself, locks held; 0 or a code with its text in errmsg */
static void many_run(ManyJob *j) {
  for (uint32_t i = 0; i < j->n; i++) {
    j->st[i] = j->h[i]->st;
    if (j->st[i] == NULL) {
      j->rc = SPEEXHIP_ERR_BAD_STATE;
      snprintf(j->errmsg, sizeof(j->errmsg), "%s", speexhip_resampler_strerror(j->rc));
      return;
    }
  }
  /* The result Buffers were sized from the states' counters when the call was prepared (will_make).  The asynchronous
   * form released the locks in between: if a state has moved since (another call of that instance slipped in), the
   * library would now write a different number of frames -- possibly more than the Buffer holds.  Ask again, under the
   * locks, BEFORE anything is written, and refuse the step whole. */
  for (uint32_t i = 0; i < j->n; i++) {
    uint32_t will_use = 0, will_make = 0;
    speexhip_resampler_peek(j->st[i], j->in_len[i], j->out_len[i], j->float_entry != NULL ? j->float_entry[i] : 0, &will_use,
                            &will_make);
    if (will_make != j->will_make[i]) {
      j->rc = SPEEXHIP_ERR_BAD_STATE;
      snprintf(j->errmsg, sizeof(j->errmsg), "%s (a state of this step was used by another call while the step was pending)",
               speexhip_resampler_strerror(j->rc));
      return;
    }
  }
  if (j->in_fmt != NULL)
    j->rc = speexhip_resampler_process_many_fmt(j->n, j->st, j->in_fmt, (const void *const *)j->in, j->in_len, j->out_fmt,
                                                (void *const *)j->out, j->out_len, j->codes);
  else
    j->rc = speexhip_resampler_process_many_int(j->n, j->st, j->in, j->in_len, j->out, j->out_len, j->codes);
  j->ran = 1;
  for (uint32_t i = 0; i < j->n; i++)
    if (j->codes[i] == 0 && j->out_len[i] != j->will_make[i]) {
      j->codes[i] = SPEEXHIP_ERR_BAD_STATE;
      if (j->rc == 0) j->rc = SPEEXHIP_ERR_BAD_STATE;
    }
  if (j->rc != 0) snprintf(j->errmsg, sizeof(j->errmsg), "%s", speexhip_resampler_strerror(j->rc));
}

/* Parses (handles[], chunks[], inFrames[], caps[]) -- formatted: and (inFmts[], outFmts[]), SPEEXHIP_FMT_* ids per entry --
 * sizes the results from the states' counters and creates the result Buffers; returns the job with *result = the array
 * of Buffers, or NULL with an exception pending. */
static ManyJob *many_prepare(napi_env env, napi_callback_info info, napi_value *result, int keep_refs, int formatted) {
  size_t argc = 6;
  napi_value argv[6];
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < (formatted ? 6u : 4u)) {
    napi_throw_type_error(env, NULL, formatted ? "processManyFormat expects (handle[], Buffer[], number[], number[], number[], number[])"
                                               : "processMany expects (handle[], Buffer[], number[], number[])");
    return NULL;
  }
  uint32_t n = 0;
  if (napi_get_array_length(env, argv[0], &n) != napi_ok) {
    napi_throw_type_error(env, NULL, "processMany expects (handle[], Buffer[], number[], number[])");
    return NULL;
  }
  ManyJob *j = (ManyJob *)calloc(1, sizeof(ManyJob));
  const size_t m = n ? n : 1;
  if (j != NULL) {
    j->n = n;
    j->h = (Handle **)calloc(m, sizeof(Handle *));
    j->locked = (Handle **)calloc(m, sizeof(Handle *));
    j->st = (SpeexHipResamplerState **)calloc(m, sizeof(*j->st));
    j->in = (const int16_t **)calloc(m, sizeof(*j->in));
    j->out = (int16_t **)calloc(m, sizeof(*j->out));
    j->in_len = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->out_len = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->will_make = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->channels = (uint32_t *)calloc(m, sizeof(uint32_t));
    j->codes = (int *)calloc(m, sizeof(int));
    if (keep_refs) j->refs = (napi_ref *)calloc(3 * m, sizeof(napi_ref));
    if (formatted) {
      j->in_fmt = (int *)calloc(m, sizeof(int));
      j->out_fmt = (int *)calloc(m, sizeof(int));
      j->float_entry = (int *)calloc(m, sizeof(int));
    }
  }
  if (j == NULL || !j->h || !j->locked || !j->st || !j->in || !j->out || !j->in_len || !j->out_len || !j->will_make ||
      !j->channels || !j->codes || (keep_refs && !j->refs) || (formatted && (!j->in_fmt || !j->out_fmt || !j->float_entry))) {
    many_free(env, j);
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED));
    return NULL;
  }
  const char *fail = NULL;
  int type_error = 0;
  for (uint32_t i = 0; fail == NULL && i < n; i++) {
    napi_value hv, c, a, b;
    void *p = NULL, *data = NULL;
    size_t bytes = 0;
    if (napi_get_element(env, argv[0], i, &hv) != napi_ok || napi_get_value_external(env, hv, &p) != napi_ok || p == NULL ||
        napi_get_element(env, argv[1], i, &c) != napi_ok || !buffer_or_null(env, c, &data, &bytes) ||
        napi_get_element(env, argv[2], i, &a) != napi_ok || napi_get_value_uint32(env, a, &j->in_len[i]) != napi_ok ||
        napi_get_element(env, argv[3], i, &b) != napi_ok || napi_get_value_uint32(env, b, &j->out_len[i]) != napi_ok) {
      fail = "processMany expects (handle[], Buffer[], number[], number[])";
      type_error = 1;
      break;
    }
    if (formatted) {
      napi_value fa, fb;
      int32_t fi = -1, fo = -1;
      if (napi_get_element(env, argv[4], i, &fa) != napi_ok || napi_get_value_int32(env, fa, &fi) != napi_ok ||
          napi_get_element(env, argv[5], i, &fb) != napi_ok || napi_get_value_int32(env, fb, &fo) != napi_ok) {
        fail = "processManyFormat expects (handle[], Buffer[], number[], number[], number[], number[])";
        type_error = 1;
        break;
      }
      if (speexhip_sample_bytes(fi) == 0 || speexhip_sample_bytes(fo) == 0) {
        fail = "processManyFormat: unknown sample format";
        break;
      }
      j->in_fmt[i] = fi;
      j->out_fmt[i] = fo;
    }
    j->h[i] = (Handle *)p;
    j->in[i] = (const int16_t *)data;
    /* (the chunk's byte count is checked against its frames below, once the channel count is known) */
    j->channels[i] = (uint32_t)bytes;  /* borrowed until then */
    if (keep_refs) {
      if (napi_create_reference(env, hv, 1, &j->refs[3 * i]) != napi_ok ||
          (data != NULL && napi_create_reference(env, c, 1, &j->refs[3 * i + 1]) != napi_ok))
        fail = "speexhip N-API failure: napi_create_reference";
    }
  }
  if (fail == NULL) {
    memcpy(j->locked, j->h, n * sizeof(Handle *));
    qsort(j->locked, n, sizeof(Handle *), cmp_handle);
    for (uint32_t k = 0; k < n; k++) {
      if (k > 0 && j->locked[k] == j->locked[k - 1]) {
        fail = "processMany: a state may appear once per call";
        break;
      }
    }
    j->n_locked = n;
  }
  if (fail == NULL && napi_create_array_with_length(env, n, result) != napi_ok) fail = "speexhip N-API failure: napi_create_array";
  if (fail == NULL) {
    many_lock(j);
    for (uint32_t i = 0; fail == NULL && i < n; i++) {
      SpeexHipResamplerState *st = j->h[i]->st;
      if (st == NULL) {
        fail = speexhip_resampler_strerror(SPEEXHIP_ERR_BAD_STATE);
        break;
      }
      SpeexHipInfo si;
      speexhip_resampler_get_info(st, &si);
      const size_t bytes = j->channels[i];
      const size_t in_frame_bytes = (size_t)si.nb_channels * (formatted ? speexhip_sample_bytes(j->in_fmt[i]) : 2);
      const size_t frame_bytes = (size_t)si.nb_channels * (formatted ? speexhip_sample_bytes(j->out_fmt[i]) : 2);
      j->channels[i] = si.nb_channels;
      if (j->in[i] != NULL && (size_t)j->in_len[i] * in_frame_bytes > bytes) {
        fail = "input frame count exceeds the chunk";
        break;
      }
      int float_entry = 0;
      if (formatted) {
        /* (the entry's rules: S16 -> S16 is the int16 call unless the state's dither or meter is on; everything else the
         *  float call) */
        int kind = SPEEXHIP_DITHER_NONE;
        (void)speexhip_resampler_get_dither(st, &kind, NULL, NULL);
        float_entry = !(j->in_fmt[i] == SPEEXHIP_FMT_S16 && j->out_fmt[i] == SPEEXHIP_FMT_S16 && kind == SPEEXHIP_DITHER_NONE &&
                        !j->h[i]->meter_on && !gain_is_on(st));
        j->float_entry[i] = float_entry;
      }
      uint32_t will_use = 0;
      speexhip_resampler_peek(st, j->in_len[i], j->out_len[i], float_entry, &will_use, &j->will_make[i]);
      napi_value buf;
      void *dst = NULL;
      /* Round 6: like process(), results of a few KB and more are pinned blocks of the library handed to JavaScript
       * as external Buffers -- the library recognises its own blocks among the out[] pointers and lets the kernel
       * write them in place (no copy out of a staging buffer).  No block free, or a runtime without external
       * Buffers: an ordinary Buffer, as before. */
      const size_t made_bytes = (size_t)j->will_make[i] * frame_bytes;
      int have = 0;
      if (made_bytes >= kExternalMin && !g_no_external) {
        void *block = speexhip_block_acquire(made_bytes);
        if (block != NULL) {
          if (napi_create_external_buffer(env, made_bytes, block, finalize_block, (void *)made_bytes, &buf) == napi_ok) {
            int64_t adjusted = 0;
            __atomic_fetch_add(&g_external_bytes, made_bytes, __ATOMIC_RELAXED);
            __atomic_fetch_add(&g_take_calls, 1, __ATOMIC_RELAXED);
            (void)napi_adjust_external_memory(env, (int64_t)made_bytes, &adjusted);
            dst = block;
            have = 1;
          } else {
            speexhip_block_release(block);
          }
        } else {
          __atomic_fetch_add(&g_take_no_block, 1, __ATOMIC_RELAXED);
        }
      }
      if ((!have && napi_create_buffer(env, made_bytes, &dst, &buf) != napi_ok) ||
          napi_set_element(env, *result, i, buf) != napi_ok ||
          (keep_refs && napi_create_reference(env, buf, 1, &j->refs[3 * i + 2]) != napi_ok)) {
        fail = "speexhip N-API failure: building the result array";
        break;
      }
      static uint64_t nowhere = 0;
      j->out[i] = (int16_t *)(dst != NULL ? dst : (void *)&nowhere);
    }
    if (fail != NULL || keep_refs) many_unlock(j); /* (the synchronous form keeps the locks until the call is done) */
  }
  if (fail != NULL) {
    many_free(env, j);
    if (type_error)
      napi_throw_type_error(env, NULL, fail);
    else
      napi_throw_error(env, NULL, fail);
    return NULL;
  }
  return j;
}

/* processMany(handles[], chunks[], inFrames[], outCapacities[]) -> Buffer[]: entry i is what
 * process(handles[i], chunks[i], inFrames[i], outCapacities[i]) returns. */
static napi_value process_many_now(napi_env env, napi_callback_info info, int formatted);
static napi_value ProcessMany(napi_env env, napi_callback_info info) {
  return process_many_now(env, info, 0);
}
/* processManyFormat(handles[], chunks[], inFrames[], outCapacities[], inFmts[], outFmts[]) -> Buffer[]: entry i is what
 * processFormat on handles[i] returns for its formats -- one fused library call (speexhip_resampler_process_many_fmt). */
static napi_value ProcessManyFormat(napi_env env, napi_callback_info info) {
  return process_many_now(env, info, 1);
}
static napi_value process_many_now(napi_env env, napi_callback_info info, int formatted) {
  napi_value result = NULL;
  ManyJob *j = many_prepare(env, info, &result, 0, formatted);
  if (j == NULL) return NULL;
  many_run(j); /* (locks held since many_prepare) */
  many_unlock(j);
  const int rc = j->rc;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s", j->errmsg);
  many_free(env, j);
  if (rc != 0) {
    napi_throw_error(env, NULL, msg);
    return NULL;
  }
  return result;
}

static void many_execute(napi_env env, void *data) {
  (void)env;
  ManyJob *j = (ManyJob *)data;
  many_lock(j);
  many_run(j);
  many_unlock(j);
}
static void many_complete(napi_env env, napi_status status, void *data) {
  ManyJob *j = (ManyJob *)data;
  napi_value v;
  if (status == napi_ok && j->rc == 0 && napi_get_reference_value(env, j->result_ref, &v) == napi_ok) {
    napi_resolve_deferred(env, j->deferred, v);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, j->rc != 0 ? j->errmsg : "speexhip: asynchronous call failed", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    /* When the library call was made, every entry has an outcome of its own (codes[i]; the states of the entries
     * that succeeded HAVE advanced and their audio is in results[i]): the error carries both, so that a caller who
     * coalesced independent instances can settle each one by itself (index.js, flushTick) -- in the reference only the
     * offending instance fails. */
    napi_value codes, results, c;
    if (status == napi_ok && j->ran && napi_create_array_with_length(env, j->n, &codes) == napi_ok &&
        napi_get_reference_value(env, j->result_ref, &results) == napi_ok) {
      for (uint32_t i = 0; i < j->n; i++)
        if (napi_create_int32(env, j->codes[i], &c) == napi_ok) napi_set_element(env, codes, i, c);
      napi_set_named_property(env, v, "codes", codes);
      napi_set_named_property(env, v, "results", results);
    }
    napi_reject_deferred(env, j->deferred, v);
  }
  napi_delete_async_work(env, j->work);
  many_free(env, j);
}
/* processManyAsync(...) -> Promise<Buffer[]>: the same call on a libuv pool thread.  The results are sized on the
 * calling thread from the states' counters, so no state of the call may be used until the promise settles (index.js
 * keeps one call per instance in flight). */
static napi_value process_many_later(napi_env env, napi_callback_info info, int formatted);
static napi_value ProcessManyAsync(napi_env env, napi_callback_info info) { return process_many_later(env, info, 0); }
/* processManyFormatAsync(...) -> Promise<Buffer[]>: processManyFormat on a libuv pool thread, under the same rules */
static napi_value ProcessManyFormatAsync(napi_env env, napi_callback_info info) { return process_many_later(env, info, 1); }
static napi_value process_many_later(napi_env env, napi_callback_info info, int formatted) {
  napi_value result = NULL, promise, name;
  ManyJob *j = many_prepare(env, info, &result, 1, formatted);
  if (j == NULL) return NULL;
  if (napi_create_reference(env, result, 1, &j->result_ref) != napi_ok ||
      napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "speexhip.processManyAsync", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, many_execute, many_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    many_free(env, j);
    napi_throw_error(env, NULL, "speexhip N-API failure: queueing processManyAsync");
    return NULL;
  }
  return promise;
}

/* warmup() -> Promise<number>: speexhip_warmup(-1) on a libuv pool thread; resolves with its return code (never rejects:
 * a box without a GPU is reported by the first real call, like the reference's errors) */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  int rc;
} WarmJob;
static void warm_execute(napi_env env, void *data) {
  (void)env;
  ((WarmJob *)data)->rc = speexhip_warmup(-1);
}
static void warm_complete(napi_env env, napi_status status, void *data) {
  WarmJob *j = (WarmJob *)data;
  napi_value v;
  (void)status;
  napi_create_int32(env, j->rc, &v);
  napi_resolve_deferred(env, j->deferred, v);
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value Warmup(napi_env env, napi_callback_info info) {
  (void)info;
  WarmJob *j = (WarmJob *)calloc(1, sizeof(WarmJob));
  napi_value promise, name;
  if (j == NULL || napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "speexhip.warmup", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, NULL, name, warm_execute, warm_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    free(j);
    napi_throw_error(env, NULL, "speexhip N-API failure: queueing warmup");
    return NULL;
  }
  return promise;
}

/* allocChunk(bytes) -> Buffer over a pinned block of the library (speexhip_block_acquire) for the caller to FILL -- read
 * a file or a socket into it, let a decoder write it -- and pass to process() / processMany(): the library recognises its
 * own blocks and lets the kernel read the chunk in place through PCIe, where an ordinary Buffer is first copied into
 * staging memory (the reference copies every chunk into the WASM heap, src/index.ts:71-92).  The block goes back to the
 * pool when the Buffer is collected.  No block free, a runtime without external Buffers, or SPEEXHIP_NAPI_COPY=1: an
 * ordinary Buffer of that size -- same results, the usual staging. */
static napi_value AllocChunk(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], buf;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double want = 0;
  if (argc < 1 || napi_get_value_double(env, argv[0], &want) != napi_ok || !(want >= 0) || want > 4294967295.0) {
    napi_throw_range_error(env, NULL, "allocChunk expects a size in bytes");
    return NULL;
  }
  const size_t bytes = (size_t)want;
  if (bytes >= kExternalMin && !g_no_external) {
    void *block = speexhip_block_acquire(bytes);
    if (block != NULL) {
      if (napi_create_external_buffer(env, bytes, block, finalize_block, (void *)bytes, &buf) == napi_ok) {
        int64_t adjusted = 0;
        __atomic_fetch_add(&g_external_bytes, bytes, __ATOMIC_RELAXED);
        __atomic_fetch_add(&g_pinned_chunks, 1, __ATOMIC_RELAXED);
        (void)napi_adjust_external_memory(env, (int64_t)bytes, &adjusted);
        return buf;
      }
      speexhip_block_release(block);
    }
  }
  void *data = NULL;
  NAPI_OK(napi_create_buffer(env, bytes, &data, &buf));
  return buf;
}

/* deviceCount() -> GPUs the library can place states on (speexhip_device_count) */
static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value v;
  NAPI_OK(napi_create_int32(env, speexhip_device_count(), &v));
  return v;
}

/* stats() -> { externalBytes, takeCalls, takeNoBlock }: bytes of pinned result blocks JavaScript holds as external
 * Buffers, results delivered that way, and calls that found the slab full and copied instead (diagnostics) */
static napi_value Stats(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value obj, v;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_create_double(env, (double)__atomic_load_n(&g_external_bytes, __ATOMIC_RELAXED), &v));
  NAPI_OK(napi_set_named_property(env, obj, "externalBytes", v));
  NAPI_OK(napi_create_double(env, (double)__atomic_load_n(&g_take_calls, __ATOMIC_RELAXED), &v));
  NAPI_OK(napi_set_named_property(env, obj, "takeCalls", v));
  NAPI_OK(napi_create_double(env, (double)__atomic_load_n(&g_take_no_block, __ATOMIC_RELAXED), &v));
  NAPI_OK(napi_set_named_property(env, obj, "takeNoBlock", v));
  NAPI_OK(napi_create_double(env, (double)__atomic_load_n(&g_pinned_chunks, __ATOMIC_RELAXED), &v));
  NAPI_OK(napi_set_named_property(env, obj, "pinnedChunks", v));
  return obj;
}

/* ---- the mixer (speexhip_mixer_*): mix buses over many separate states in one host call ---------------------------------
 * A mixer handle is an external of its own; its calls are synchronous, on the calling thread.  The legs are ordinary
 * resampler handles: mixerProcess holds the lock of every leg for the call, taken in address order like processMany. */
typedef struct {
  SpeexHipMixer *m;
  uint32_t n_legs, n_buses, channels;
} MixerHandle;

static void finalize_mixer(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  MixerHandle *h = (MixerHandle *)data;
  if (h->m != NULL) speexhip_mixer_destroy(h->m);
  free(h);
}
static MixerHandle *unwrap_mixer(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || p == NULL) {
    napi_throw_type_error(env, NULL, "expected a mixer handle");
    return NULL;
  }
  MixerHandle *h = (MixerHandle *)p;
  if (h->m == NULL) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_BAD_STATE));
    return NULL;
  }
  return h;
}

/* mixerInit(nLegs, nBuses, channels[, device]) -> handle */
static napi_value MixerInit(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "mixerInit(nLegs, nBuses, channels[, device])");
    return NULL;
  }
  uint32_t n_legs = 0, n_buses = 0, channels = 0;
  int32_t device = -1;
  NAPI_OK(napi_get_value_uint32(env, argv[0], &n_legs));
  NAPI_OK(napi_get_value_uint32(env, argv[1], &n_buses));
  NAPI_OK(napi_get_value_uint32(env, argv[2], &channels));
  if (argc >= 4) {
    napi_valuetype t;
    if (napi_typeof(env, argv[3], &t) == napi_ok && t == napi_number) NAPI_OK(napi_get_value_int32(env, argv[3], &device));
  }
  int err = 0;
  SpeexHipMixer *m = speexhip_mixer_init_on(device, n_legs, n_buses, channels, &err);
  if (m == NULL) {
    napi_throw_error(env, NULL, speexhip_resampler_strerror(err));
    return NULL;
  }
  MixerHandle *h = (MixerHandle *)calloc(1, sizeof(MixerHandle));
  if (h == NULL) {
    speexhip_mixer_destroy(m);
    napi_throw_error(env, NULL, speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED));
    return NULL;
  }
  h->m = m;
  h->n_legs = n_legs, h->n_buses = n_buses, h->channels = channels;
  napi_value handle;
  NAPI_OK(napi_create_external(env, h, finalize_mixer, NULL, &handle));
  return handle;
}

/* mixerDestroy(handle) */
static napi_value MixerDestroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *p = NULL;
  if (argc < 1 || napi_get_value_external(env, argv[0], &p) != napi_ok || p == NULL) {
    napi_throw_type_error(env, NULL, "expected a mixer handle");
    return NULL;
  }
  MixerHandle *h = (MixerHandle *)p;
  if (h->m != NULL) speexhip_mixer_destroy(h->m);
  h->m = NULL;
  return NULL;
}

/* mixerSetWeights(handle, weights: Buffer of nBuses x nLegs float32, row-major | null) */
static napi_value MixerSetWeights(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) {
    napi_throw_type_error(env, NULL, "mixerSetWeights(handle, Buffer | null)");
    return NULL;
  }
  MixerHandle *h = unwrap_mixer(env, argv[0]);
  if (h == NULL) return NULL;
  void *data = NULL;
  size_t bytes = 0;
  if (!buffer_or_null(env, argv[1], &data, &bytes) ||
      (data != NULL && bytes != (size_t)h->n_buses * h->n_legs * sizeof(float))) {
    napi_throw_type_error(env, NULL, "mixerSetWeights expects nBuses x nLegs float32 values, or null");
    return NULL;
  }
  return control_result(env, speexhip_mixer_set_weights(h->m, (const float *)data));
}

/* mixerSetDither(handle, kind, seedLo, seedHi, positionLo, positionHi) */
static napi_value MixerSetDither(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) {
    napi_throw_type_error(env, NULL, "mixerSetDither(handle, kind, seedLo, seedHi, positionLo, positionHi)");
    return NULL;
  }
  MixerHandle *h = unwrap_mixer(env, argv[0]);
  if (h == NULL) return NULL;
  int32_t kind = 0;
  uint32_t v[4] = {0, 0, 0, 0};
  NAPI_OK(napi_get_value_int32(env, argv[1], &kind));
  for (size_t i = 0; i < 4; i++) NAPI_OK(napi_get_value_uint32(env, argv[2 + i], &v[i]));
  return control_result(env, speexhip_mixer_set_dither(h->m, kind, ((uint64_t)v[1] << 32) | v[0], ((uint64_t)v[3] << 32) | v[2]));
}

/* mixerGetDither(handle) -> [kind, seedLo, seedHi, positionLo, positionHi] */
static napi_value MixerGetDither(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  MixerHandle *h = argc >= 1 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) return NULL;
  int kind = 0;
  uint64_t seed = 0, position = 0;
  const int rc = speexhip_mixer_get_dither(h->m, &kind, &seed, &position);
  if (rc != 0) return control_result(env, rc);
  const uint32_t out[5] = {(uint32_t)kind, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)position, (uint32_t)(position >> 32)};
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 5, &arr));
  for (uint32_t i = 0; i < 5; i++) {
    NAPI_OK(napi_create_uint32(env, out[i], &v));
    NAPI_OK(napi_set_element(env, arr, i, v));
  }
  return arr;
}

/* mixerSetMeter(handle, on) */
static napi_value MixerSetMeter(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  MixerHandle *h = argc >= 2 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) return NULL;
  bool on = false;
  NAPI_OK(napi_get_value_bool(env, argv[1], &on));
  return control_result(env, speexhip_mixer_set_meter(h->m, on ? 1 : 0));
}

/* mixerGetBusMeter(handle, bus, reset) -> getMeter's array, of the bus's cell */
static napi_value MixerGetBusMeter(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  MixerHandle *h = argc >= 3 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) return NULL;
  uint32_t bus = 0;
  bool reset = false;
  NAPI_OK(napi_get_value_uint32(env, argv[1], &bus));
  NAPI_OK(napi_get_value_bool(env, argv[2], &reset));
  SpeexHipMeter m;
  memset(&m, 0, sizeof(m));
  m.struct_size = (uint32_t)sizeof(m);
  const int rc = speexhip_mixer_get_bus_meter(h->m, bus, &m, reset ? 1 : 0);
  if (rc != 0) return control_result(env, rc);
  const uint64_t counts[4] = {m.samples, m.clipped_high, m.clipped_low, m.nan};
  napi_value arr, v;
  NAPI_OK(napi_create_array_with_length(env, 10, &arr));
  NAPI_OK(napi_create_uint32(env, m.on, &v));
  NAPI_OK(napi_set_element(env, arr, 0, v));
  for (uint32_t i = 0; i < 4; i++) {
    NAPI_OK(napi_create_uint32(env, (uint32_t)counts[i], &v));
    NAPI_OK(napi_set_element(env, arr, 1 + 2 * i, v));
    NAPI_OK(napi_create_uint32(env, (uint32_t)(counts[i] >> 32), &v));
    NAPI_OK(napi_set_element(env, arr, 2 + 2 * i, v));
  }
  NAPI_OK(napi_create_double(env, (double)m.peak, &v));
  NAPI_OK(napi_set_element(env, arr, 9, v));
  return arr;
}

/* mixerSetLevels(handle, on) */
static napi_value MixerSetLevels(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  MixerHandle *h = argc >= 2 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) return NULL;
  bool on = false;
  NAPI_OK(napi_get_value_bool(env, argv[1], &on));
  return control_result(env, speexhip_mixer_set_levels(h->m, on ? 1 : 0));
}

/* mixerGetLevels(handle) -> Buffer of nLegs SpeexHipLevel records (32 bytes each, little-endian): the last call's */
static napi_value MixerGetLevels(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  MixerHandle *h = argc >= 1 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) return NULL;
  void *data = NULL;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, (size_t)h->n_legs * sizeof(SpeexHipLevel), &data, &buf));
  const int rc = speexhip_mixer_get_levels(h->m, 0, h->n_legs, data, (uint32_t)sizeof(SpeexHipLevel));
  if (rc != 0) return control_result(env, rc);
  return buf;
}

/* mixerProcess(handle, legs: (handle | null)[], chunks: (Buffer | null)[], inFrames[], caps[], inFmts[], outFmt)
 *   -> { buses: Buffer[], busFrames, consumed: number[], produced: number[], codes: number[] }
 * One speexhip_mixer_process call; the buses come interleaved in outFmt, bus j a fresh Buffer of busFrames frames.  A leg
 * whose code is not 0 was refused (its state untouched, +0.0 in the sum) -- the caller decides what that means. */
static napi_value MixerProcess(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const char *usage = "mixerProcess(handle, handle[], Buffer[], number[], number[], number[], number)";
  MixerHandle *h = argc >= 7 ? unwrap_mixer(env, argv[0]) : NULL;
  if (h == NULL) {
    if (argc < 7) napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  const uint32_t n = h->n_legs;
  int32_t out_fmt = -1;
  uint32_t len = 0;
  if (napi_get_array_length(env, argv[1], &len) != napi_ok || len != n || napi_get_value_int32(env, argv[6], &out_fmt) != napi_ok ||
      speexhip_sample_bytes(out_fmt) == 0) {
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  Handle **hs = (Handle **)calloc(n, sizeof(Handle *)), **locked = (Handle **)calloc(n, sizeof(Handle *));
  SpeexHipResamplerState **st = (SpeexHipResamplerState **)calloc(n, sizeof(*st));
  SpeexHipSide *sides = (SpeexHipSide *)calloc(n, sizeof(SpeexHipSide));
  uint32_t *in_len = (uint32_t *)calloc(n, sizeof(uint32_t)), *out_len = (uint32_t *)calloc(n, sizeof(uint32_t));
  int *codes = (int *)calloc(n, sizeof(int));
  char *image = NULL;
  napi_value result = NULL;
  const char *fail = NULL;
  int type_error = 0;
  uint32_t n_locked = 0, most = 0;
  if (!hs || !locked || !st || !sides || !in_len || !out_len || !codes) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  for (uint32_t i = 0; fail == NULL && i < n; i++) {
    napi_value hv, c, a, b, f;
    napi_valuetype t;
    void *p = NULL, *data = NULL;
    size_t bytes = 0;
    int32_t fi = -1;
    if (napi_get_element(env, argv[1], i, &hv) != napi_ok || napi_typeof(env, hv, &t) != napi_ok ||
        (t != napi_null && t != napi_undefined && (napi_get_value_external(env, hv, &p) != napi_ok || p == NULL)) ||
        napi_get_element(env, argv[2], i, &c) != napi_ok || !buffer_or_null(env, c, &data, &bytes) ||
        napi_get_element(env, argv[3], i, &a) != napi_ok || napi_get_value_uint32(env, a, &in_len[i]) != napi_ok ||
        napi_get_element(env, argv[4], i, &b) != napi_ok || napi_get_value_uint32(env, b, &out_len[i]) != napi_ok ||
        napi_get_element(env, argv[5], i, &f) != napi_ok || napi_get_value_int32(env, f, &fi) != napi_ok) {
      fail = usage;
      type_error = 1;
      break;
    }
    hs[i] = (Handle *)p;
    sides[i].struct_size = (uint32_t)sizeof(SpeexHipSide);
    sides[i].fmt = fi;
    sides[i].channels = h->channels;
    sides[i].layout = SPEEXHIP_LAYOUT_INTERLEAVED;
    sides[i].data = data;
    if (p != NULL && data != NULL && (size_t)in_len[i] * h->channels * speexhip_sample_bytes(fi) > bytes) fail = "input frame count exceeds the chunk";
    if (p != NULL) locked[n_locked++] = (Handle *)p;
    if (p != NULL && out_len[i] > most) most = out_len[i];
  }
  if (fail == NULL) {
    qsort(locked, n_locked, sizeof(Handle *), cmp_handle);
    /* (a state in two slots is locked once; the library refuses its second slot) */
    uint32_t kept = 0;
    for (uint32_t k = 0; k < n_locked; k++)
      if (kept == 0 || locked[k] != locked[kept - 1]) locked[kept++] = locked[k];
    n_locked = kept;
  }
  const size_t frame_bytes = (size_t)h->channels * speexhip_sample_bytes(out_fmt);
  const size_t bus_bytes = (size_t)(most ? most : 1) * frame_bytes;
  if (fail == NULL && (image = (char *)malloc(bus_bytes * h->n_buses)) == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_ALLOC_FAILED);
  int rc = 0;
  uint32_t bus_frames = 0;
  if (fail == NULL) {
    for (uint32_t k = 0; k < n_locked; k++) pthread_mutex_lock(&locked[k]->lock);
    for (uint32_t i = 0; fail == NULL && i < n; i++) {
      st[i] = hs[i] != NULL ? hs[i]->st : NULL;
      if (hs[i] != NULL && st[i] == NULL) fail = speexhip_resampler_strerror(SPEEXHIP_ERR_BAD_STATE);  /* a destroyed leg */
    }
    if (fail == NULL) {
      SpeexHipSide out;
      memset(&out, 0, sizeof(out));
      out.struct_size = (uint32_t)sizeof(out);
      out.fmt = out_fmt;
      out.channels = h->channels;
      out.layout = SPEEXHIP_LAYOUT_INTERLEAVED;
      out.data = image;
      out.stream_stride = (uint64_t)(most ? most : 1) * h->channels;
      bus_frames = 0xFFFFFFFFu;
      rc = speexhip_mixer_process(h->m, st, sides, in_len, out_len, &out, &bus_frames, codes);
      if (bus_frames == 0xFFFFFFFFu) fail = speexhip_resampler_strerror(rc);  /* a call-level error: nothing ran */
    }
    for (uint32_t k = n_locked; k-- > 0;) pthread_mutex_unlock(&locked[k]->lock);
  }
  if (fail == NULL) {
    napi_value buses, used, made, cs, v;
    if (napi_create_object(env, &result) != napi_ok || napi_create_array_with_length(env, h->n_buses, &buses) != napi_ok ||
        napi_create_array_with_length(env, n, &used) != napi_ok || napi_create_array_with_length(env, n, &made) != napi_ok ||
        napi_create_array_with_length(env, n, &cs) != napi_ok)
      fail = "speexhip N-API failure: building the result";
    for (uint32_t j = 0; fail == NULL && j < h->n_buses; j++) {
      void *dst = NULL;
      if (napi_create_buffer_copy(env, (size_t)bus_frames * frame_bytes, image + j * bus_bytes, &dst, &v) != napi_ok ||
          napi_set_element(env, buses, j, v) != napi_ok)
        fail = "speexhip N-API failure: building the result";
    }
    for (uint32_t i = 0; fail == NULL && i < n; i++) {
      if (napi_create_uint32(env, in_len[i], &v) != napi_ok || napi_set_element(env, used, i, v) != napi_ok ||
          napi_create_uint32(env, out_len[i], &v) != napi_ok || napi_set_element(env, made, i, v) != napi_ok ||
          napi_create_int32(env, codes[i], &v) != napi_ok || napi_set_element(env, cs, i, v) != napi_ok)
        fail = "speexhip N-API failure: building the result";
    }
    if (fail == NULL &&
        (napi_create_uint32(env, bus_frames, &v) != napi_ok || napi_set_named_property(env, result, "busFrames", v) != napi_ok ||
         napi_set_named_property(env, result, "buses", buses) != napi_ok || napi_set_named_property(env, result, "consumed", used) != napi_ok ||
         napi_set_named_property(env, result, "produced", made) != napi_ok || napi_set_named_property(env, result, "codes", cs) != napi_ok))
      fail = "speexhip N-API failure: building the result";
  }
  free(hs);
  free(locked);
  free(st);
  free(sides);
  free(in_len);
  free(out_len);
  free(codes);
  free(image);
  if (fail != NULL) {
    if (type_error)
      napi_throw_type_error(env, NULL, fail);
    else
      napi_throw_error(env, NULL, fail);
    return NULL;
  }
  return result;
}

/* NAPI_MODULE_INIT: the well-known symbol napi_register_module_v1, so that every environment of the process -- the main
 * thread and each worker_threads Worker -- can load the addon (a module that registers itself from a static constructor
 * loads once per process).  The addon keeps no per-environment state: handles are externals, the counters above are
 * atomics, the library underneath is thread-safe per state. */
NAPI_MODULE_INIT() {
  const char *copy_env = getenv("SPEEXHIP_NAPI_COPY");
  g_no_external = copy_env != NULL && copy_env[0] != '\0' && copy_env[0] != '0';
  napi_property_descriptor props[] = {
      {"init", NULL, Init, NULL, NULL, NULL, napi_default, NULL},
      {"destroy", NULL, Destroy, NULL, NULL, NULL, napi_default, NULL},
      {"process", NULL, Process, NULL, NULL, NULL, napi_default, NULL},
      {"processFloat", NULL, ProcessFloat, NULL, NULL, NULL, napi_default, NULL},
      {"processPlanar", NULL, ProcessPlanar, NULL, NULL, NULL, napi_default, NULL},
      {"processFormat", NULL, ProcessFormat, NULL, NULL, NULL, napi_default, NULL},
      {"processMix", NULL, ProcessMix, NULL, NULL, NULL, napi_default, NULL},
      {"processSides", NULL, ProcessSides, NULL, NULL, NULL, napi_default, NULL},
      {"processChunks", NULL, ProcessChunks, NULL, NULL, NULL, napi_default, NULL},
      {"processAsync", NULL, ProcessAsync, NULL, NULL, NULL, napi_default, NULL},
      {"processChunksAsync", NULL, ProcessChunksAsync, NULL, NULL, NULL, napi_default, NULL},
      {"processChunksFormat", NULL, ProcessChunksFormat, NULL, NULL, NULL, napi_default, NULL},
      {"processChunksFormatAsync", NULL, ProcessChunksFormatAsync, NULL, NULL, NULL, napi_default, NULL},
      {"setRate", NULL, SetRate, NULL, NULL, NULL, napi_default, NULL},
      {"setQuality", NULL, SetQuality, NULL, NULL, NULL, napi_default, NULL},
      {"skipZeros", NULL, SkipZeros, NULL, NULL, NULL, napi_default, NULL},
      {"resetMem", NULL, ResetMem, NULL, NULL, NULL, napi_default, NULL},
      {"setDither", NULL, SetDither, NULL, NULL, NULL, napi_default, NULL},
      {"getDither", NULL, GetDither, NULL, NULL, NULL, napi_default, NULL},
      {"setMeter", NULL, SetMeter, NULL, NULL, NULL, napi_default, NULL},
      {"getMeter", NULL, GetMeter, NULL, NULL, NULL, napi_default, NULL},
      {"setGain", NULL, SetGain, NULL, NULL, NULL, napi_default, NULL},
      {"getGain", NULL, GetGain, NULL, NULL, NULL, napi_default, NULL},
      {"getLatency", NULL, GetLatency, NULL, NULL, NULL, napi_default, NULL},
      {"setMode", NULL, SetMode, NULL, NULL, NULL, napi_default, NULL},
      {"getInfo", NULL, GetInfo, NULL, NULL, NULL, napi_default, NULL},
      {"getRate", NULL, GetRate, NULL, NULL, NULL, napi_default, NULL},
      {"strerror", NULL, StrError, NULL, NULL, NULL, napi_default, NULL},
      {"version", NULL, Version, NULL, NULL, NULL, napi_default, NULL},
      {"releaseCachedMemory", NULL, ReleaseCachedMemory, NULL, NULL, NULL, napi_default, NULL},
      {"processMany", NULL, ProcessMany, NULL, NULL, NULL, napi_default, NULL},
      {"processManyAsync", NULL, ProcessManyAsync, NULL, NULL, NULL, napi_default, NULL},
      {"processManyFormat", NULL, ProcessManyFormat, NULL, NULL, NULL, napi_default, NULL},
      {"processManyFormatAsync", NULL, ProcessManyFormatAsync, NULL, NULL, NULL, napi_default, NULL},
      {"deviceCount", NULL, DeviceCount, NULL, NULL, NULL, napi_default, NULL},
      {"warmup", NULL, Warmup, NULL, NULL, NULL, napi_default, NULL},
      {"stats", NULL, Stats, NULL, NULL, NULL, napi_default, NULL},
      {"allocChunk", NULL, AllocChunk, NULL, NULL, NULL, napi_default, NULL},
      {"mixerInit", NULL, MixerInit, NULL, NULL, NULL, napi_default, NULL},
      {"mixerDestroy", NULL, MixerDestroy, NULL, NULL, NULL, napi_default, NULL},
      {"mixerSetWeights", NULL, MixerSetWeights, NULL, NULL, NULL, napi_default, NULL},
      {"mixerSetDither", NULL, MixerSetDither, NULL, NULL, NULL, napi_default, NULL},
      {"mixerGetDither", NULL, MixerGetDither, NULL, NULL, NULL, napi_default, NULL},
      {"mixerSetMeter", NULL, MixerSetMeter, NULL, NULL, NULL, napi_default, NULL},
      {"mixerGetBusMeter", NULL, MixerGetBusMeter, NULL, NULL, NULL, napi_default, NULL},
      {"mixerSetLevels", NULL, MixerSetLevels, NULL, NULL, NULL, napi_default, NULL},
      {"mixerGetLevels", NULL, MixerGetLevels, NULL, NULL, NULL, napi_default, NULL},
      {"mixerProcess", NULL, MixerProcess, NULL, NULL, NULL, napi_default, NULL},
  };
  if (napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props) != napi_ok)
    napi_throw_error(env, NULL, "speexhip: cannot define exports");
  return exports;
}

