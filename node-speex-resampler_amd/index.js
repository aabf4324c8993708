'use strict';
// index.js -- drop-in replacement for the reference's app/index.js (compiled src/index.ts):
// same exports (default SpeexResampler, named SpeexResamplerTransform), same constructor
// arguments, same thrown messages, same lazy init, same grow-only output-capacity rule --
// but the work is done on an MI355X through the N-API addon speex_hip_napi.node ->
// libspeexhip.so (HIP kernels) instead of the Emscripten module src/speex_wasm.js.
// Hand-written CommonJS (no tsc in the build image); types live in index.d.ts.
Object.defineProperty(exports, '__esModule', { value: true });
const { Transform } = require('stream');
const path = require('path');

// Counterpart of `SpeexWasm()` (reference src/index.ts:18-19): a promise for the native
// module; `speexModule` is only set once it resolves, so calling processChunk before
// awaiting initPromise throws exactly like the reference does.
// processChunkFormat: the names of the sample formats (SPEEXHIP_FMT_* ids, bytes per sample)
const SAMPLE_FORMATS = {
  'u8': { id: 0, bytes: 1 },
  's16le': { id: 1, bytes: 2 },
  's24le': { id: 2, bytes: 3 },
  's32le': { id: 3, bytes: 4 },
  'f32le': { id: 4, bytes: 4 },
  'f32le-normalized': { id: 5, bytes: 4 },
  // companded (G.711, one byte per sample): ids start at 16
  'mulaw': { id: 16, bytes: 1 },
  'alaw': { id: 17, bytes: 1 },
  // half-float in +-1.0 (binary16, bfloat16) and big-endian PCM (RTP L16 / L24, AIFF)
  'f16le-normalized': { id: 20, bytes: 2 },
  'bf16le-normalized': { id: 21, bytes: 2 },
  's16be': { id: 24, bytes: 2 },
  's24be': { id: 25, bytes: 3 },
  's32be': { id: 26, bytes: 4 },
};
// result planes of processChunkSides: typed arrays are host-endian, so the big-endian formats come as bytes
// (Uint8Array, kind 0) and the half-float ones as their bits (Uint16Array, kind 4)
const BIG_ENDIAN_IDS = [24, 25, 26];
const HALF_FLOAT_IDS = [20, 21];
// setDither: the names of the dither kinds (SPEEXHIP_DITHER_* = the index)
const DITHER_KINDS = ['none', 'rectangular', 'triangular'];
let speexModule;
const globalModulePromise = new Promise((resolve, reject) => {
  try {
    resolve(require(path.join(__dirname, 'speex_hip_napi.node')));
  } catch (e) {
    reject(e);
  }
}).then((m) => {
  // The reference compiles its WASM module here, behind initPromise (src/index.ts:18-19).  The counterpart: the GPU
  // runtime's start, the library's shared streams and the copy engines' first copy -- 0.2-0.35 s that the first
  // instances would otherwise pay inside their first processChunk -- run on a pool thread while the application goes
  // on loading; initPromise resolves behind them.  A failure (no GPU) is not reported here: the first processChunk
  // throws Error(strerror(code)) as always.  SPEEXHIP_NO_WARMUP=1 skips it.
  const done = () => { speexModule = m; return m; };
  if (process.env.SPEEXHIP_NO_WARMUP === '1' || typeof m.warmup !== 'function') return done();
  return m.warmup().then(done, done);
});

// setGain's arguments, refused where they are given: a finite gain, a ramp of 0 .. 2^32 - 1 whole output frames
function checkGain(gain, rampFrames) {
  if (typeof gain !== 'number' || !Number.isFinite(gain)) throw new Error('gain must be a finite number');
  if (!Number.isInteger(rampFrames) || rampFrames < 0 || rampFrames > 0xFFFFFFFF) throw new Error('rampFrames must be an integer in 0 .. 2^32 - 1');
}

class SpeexResampler {
  /**
   * Same four arguments as the reference class: channel count (>= 1), input and output sample
   * rates in Hz, Speex quality 0..10 (default 7; higher = longer filter).
   */
  constructor(channels, inRate, outRate, quality = 7, options = undefined) {
    this.channels = channels;
    this.inRate = inRate;
    this.outRate = outRate;
    this.quality = quality;
    // Extension (ignored by reference-style callers): { device: k } pins this instance to GPU k.  Without it the
    // library's process-wide rule places the instance when its native state is made (first call): the calling
    // thread's current GPU, or -- SPEEXHIP_DEVICES=all -- instance number k of the process on GPU k mod the GPU count.
    this._device = options && Number.isInteger(options.device) ? options.device : -1;
    this._resamplerPtr = undefined; // native handle (the reference keeps a WASM pointer here)
    this._outBufferSize = -1;       // bytes; grow-only, drives the capacity rule below
    this._inFlight = 0;             // processChunkAsync calls not yet settled (extension)
  }

  // The reference's calls are synchronous and a state must not be used concurrently
  // (src/index.ts:50-116).  While a processChunkAsync call of this instance is running on a pool
  // thread, a synchronous call would interleave with it in an order the caller cannot know, so it
  // is refused; await the pending promise(s) first.
  _refuseWhileAsyncPending(what) {
    if (this._inFlight > 0) {
      throw new Error(what + ' called while a processChunkAsync call of this instance is pending; await it first');
    }
  }

  /**
   * One chunk of interleaved s16le PCM in, the resampled chunk out (a fresh Buffer), synchronously.
   */
  processChunk(chunk) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    this._refuseWhileAsyncPending('processChunk');
    // reference src/index.ts:55-57 (channels === 0 gives NaN !== 0 and lands here too)
    if (chunk.length % (this.channels * Uint16Array.BYTES_PER_ELEMENT) !== 0) {
      throw new Error('Chunk length should be a multiple of channels * 2 bytes');
    }
    if (!this._resamplerPtr) {
      // throws Error(strerror(code)) and leaves _resamplerPtr unset, so a bad configuration
      // fails again on every call (reference src/index.ts:59-66)
      this._resamplerPtr = speexModule.init(this.channels >>> 0, this.inRate >>> 0,
        this.outRate >>> 0, this.quality | 0, this._device);
    }
    // reference src/index.ts:80-87: the output buffer only ever grows ...
    const outBufferLengthTarget = Math.ceil(chunk.length * this.outRate / this.inRate);
    if (this._outBufferSize < outBufferLengthTarget) {
      this._outBufferSize = outBufferLengthTarget;
    }
    // ... and its size in frames (truncated like setValue(..., 'i32')) caps this call's
    // output (src/index.ts:95).  Input frames the cap leaves unconsumed are dropped, as in the
    // reference, which never reads in_len back (src/index.ts:108).
    const inFrames = chunk.length / this.channels / Uint16Array.BYTES_PER_ELEMENT;
    const outCapacity = (this._outBufferSize / this.channels / Uint16Array.BYTES_PER_ELEMENT) | 0;
    return speexModule.process(this._resamplerPtr, chunk, inFrames | 0, outCapacity);
  }

  // ------------------------------------------------------------------------------------------
  // Extensions (not in the reference's class).  Nothing above depends on them.
  // ------------------------------------------------------------------------------------------

  /** Checks + lazy init + the capacity rule of processChunk, without the call itself. */
  _prepare(chunk, bytesPerSample) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    if (chunk.length % (this.channels * bytesPerSample) !== 0) {
      throw new Error('Chunk length should be a multiple of channels * ' + bytesPerSample + ' bytes');
    }
    this._ensureNative();
    const target = Math.ceil(chunk.length * this.outRate / this.inRate);
    if (this._outBufferSize < target) {
      this._outBufferSize = target;
    }
    return [(chunk.length / this.channels / bytesPerSample) | 0,
      (this._outBufferSize / this.channels / bytesPerSample) | 0];
  }

  _ensureNative() {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    if (!this._resamplerPtr) {
      this._resamplerPtr = speexModule.init(this.channels >>> 0, this.inRate >>> 0,
        this.outRate >>> 0, this.quality | 0, this._device);
    }
    return this._resamplerPtr;
  }

  /**
   * processChunk for a list of consecutive chunks in ONE GPU launch (SURVEY 8f row N1).
   * Returns one Buffer per chunk, byte-identical to calling processChunk on each in turn
   * (the capacity rule is applied per original chunk).
   */
  processChunks(chunks) {
    this._refuseWhileAsyncPending('processChunks');
    const inFrames = [];
    const caps = [];
    for (const chunk of chunks) {
      const [f, cap] = this._prepare(chunk, Uint16Array.BYTES_PER_ELEMENT);
      inFrames.push(f);
      caps.push(cap);
    }
    return speexModule.processChunks(this._resamplerPtr, chunks, inFrames, caps);
  }

  /** processChunks off the event loop (one pool-thread call for the whole list); chained with the instance's other async calls. */
  processChunksAsync(chunks) {
    const inFrames = [], caps = [];
    try {
      for (const chunk of chunks) {
        const [f, cap] = this._prepare(chunk, Uint16Array.BYTES_PER_ELEMENT);
        inFrames.push(f);
        caps.push(cap);
      }
    } catch (e) {
      return Promise.reject(e);
    }
    const run = () => speexModule.processChunksAsync(this._resamplerPtr, chunks, inFrames, caps);
    this._inFlight++;
    const settle = () => { this._inFlight--; };
    const p = (this._pending || Promise.resolve()).then(run, run);
    this._pending = p.then(settle, settle);
    return p;
  }

  /**
   * processChunk that does not block the event loop: the transfer and the kernels run on a
   * libuv pool thread.  Calls on one instance are chained, so their order (and therefore the
   * stream) is the order of the calls.  Resolves to the same bytes processChunk returns.
   */
  processChunkAsync(chunk) {
    let args;
    try {
      args = this._prepare(chunk, Uint16Array.BYTES_PER_ELEMENT);
    } catch (e) {
      return Promise.reject(e);
    }
    // Calls of DIFFERENT instances that become ready in the same tick leave as ONE native call
    // (speexhip_resampler_process_many_int: per GPU one transfer in, one launch per <= 32 instances with the same
    // rates / quality / channels, one transfer out) -- a server's many connections are many instances
    // (reference src/index.ts:18-45), each with a small chunk per tick.  A lone call takes the single-state path.
    const run = () => new Promise((resolve, reject) => {
      tickQueue.push({ handle: this._resamplerPtr, chunk, inFrames: args[0], cap: args[1], resolve, reject });
      if (!tickScheduled) {
        tickScheduled = true;
        // (process.nextTick from inside a promise continuation runs once the continuations that are ready now have
        //  run: the calls of one tick are all in the queue by then)
        process.nextTick(flushTick);
      }
    });
    this._inFlight++;
    const settle = () => { this._inFlight--; };
    const p = (this._pending || Promise.resolve()).then(run, run);
    this._pending = p.then(settle, settle);
    return p;
  }

  /**
   * Float I/O (SURVEY 8f row N2, speex_resampler_process_interleaved_float): chunk is
   * interleaved float32 PCM; the result is float32, neither rounded nor clipped.  Same stream
   * state as processChunk; same grow-only capacity rule (in bytes of float32).
   */
  processChunkFloat(chunk) {
    this._refuseWhileAsyncPending('processChunkFloat');
    const [f, cap] = this._prepare(chunk, Float32Array.BYTES_PER_ELEMENT);
    return speexModule.processFloat(this._resamplerPtr, chunk, f, cap);
  }

  /**
   * Planar audio (Web Audio's getChannelData, a decoder's s16p / fltp): `channels` is an array of Int16Array or an
   * array of Float32Array, one per channel, all of equal length; the result is an array of the same kind, one typed
   * array per channel.  Same stream state and the same grow-only capacity rule as processChunk / processChunkFloat on
   * the interleaved frames -- and the same samples.
   */
  processChunkPlanar(channels) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    this._refuseWhileAsyncPending('processChunkPlanar');
    const first = Array.isArray(channels) ? channels[0] : undefined;
    const bytesPerSample = first instanceof Float32Array ? Float32Array.BYTES_PER_ELEMENT : Uint16Array.BYTES_PER_ELEMENT;
    const sameKind = first instanceof Float32Array || first instanceof Int16Array;
    if (!sameKind || channels.length !== this.channels ||
        channels.some((p) => p.constructor !== first.constructor || p.length !== first.length)) {
      throw new Error('Chunk length should be a multiple of channels * ' + bytesPerSample + ' bytes');
    }
    // the interleaved chunk of these frames, as far as the capacity rule is concerned
    const [, cap] = this._prepare({ length: first.length * this.channels * bytesPerSample }, bytesPerSample);
    return speexModule.processPlanar(this._resamplerPtr, channels, cap);
  }

  /**
   * Sample formats named independently for the input and the result: 'u8' | 's16le' | 's24le' (packed, 3 bytes) |
   * 's32le' | 'f32le' (float32 in int16 units, as processChunkFloat) | 'f32le-normalized' (float32 in +-1.0, Web Audio) |
   * 'mulaw' | 'alaw' (G.711 as RTP carries it, PCMU / PCMA: one byte per sample, decoded and encoded on the GPU -- 8 kHz
   * mu-law to 16 kHz float for a speech model: new SpeexResampler(1, 8000, 16000).processChunkFormat(rtpPayload, 'mulaw',
   * 'f32le-normalized'); a companded result is the 's16le' result through the G.711 compressor) |
   * 's16be' | 's24be' | 's32be' (network and file byte order: RTP L16 / L24 payloads, AIFF -- no swap16() either side of
   * the call: r.processChunkFormat(rtpL16Payload, 's16be', 'f32le-normalized')) | 'f16le-normalized' |
   * 'bf16le-normalized' (IEEE binary16 / bfloat16 in +-1.0, what a model in half precision reads; round to nearest even).
   * `chunk` is a Buffer of interleaved frames in inFormat; the result is a Buffer in outFormat.  It is processChunkFloat
   * on the converted samples followed by the output conversion (round half up, saturating), both done on the GPU:
   * a decoder's s16le goes in and Web Audio's float32 comes out with no loop over the samples in JavaScript.  Same
   * stream state and grow-only capacity rule as processChunkFloat on the same frames (processChunk for s16le -> s16le).
   */
  processChunkFormat(chunk, inFormat, outFormat) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    this._refuseWhileAsyncPending('processChunkFormat');
    const fin = SAMPLE_FORMATS[inFormat];
    const fout = SAMPLE_FORMATS[outFormat];
    if (!fin || !fout) {
      throw new Error('Unknown sample format: ' + (fin ? outFormat : inFormat));
    }
    if (chunk.length % (this.channels * fin.bytes) !== 0) {
      throw new Error('Chunk length should be a multiple of channels * ' + fin.bytes + ' bytes');
    }
    // the capacity rule of the call this one is: processChunk for s16le -> s16le, processChunkFloat on these frames otherwise
    const frames = (chunk.length / this.channels / fin.bytes) | 0;
    const asBytes = fin.id === 1 && fout.id === 1 ? Uint16Array.BYTES_PER_ELEMENT : Float32Array.BYTES_PER_ELEMENT;
    const [, cap] = this._prepare({ length: frames * this.channels * asBytes }, asBytes);
    return speexModule.processFormat(this._resamplerPtr, chunk, fin.id, fout.id, frames, cap);
  }

  // format names, frame counts and capacities of a list of chunks for the formatted chunks calls: the checks and the
  // grow-only capacity rule of processChunkFormat, chunk by chunk
  _prepareFormat(chunks, inFormat, outFormat) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    const fin = SAMPLE_FORMATS[inFormat];
    const fout = SAMPLE_FORMATS[outFormat];
    if (!fin || !fout) {
      throw new Error('Unknown sample format: ' + (fin ? outFormat : inFormat));
    }
    for (const chunk of chunks) {
      if (chunk.length % (this.channels * fin.bytes) !== 0) {
        throw new Error('Chunk length should be a multiple of channels * ' + fin.bytes + ' bytes');
      }
    }
    const asBytes = fin.id === 1 && fout.id === 1 ? Uint16Array.BYTES_PER_ELEMENT : Float32Array.BYTES_PER_ELEMENT;
    const inFrames = [], caps = [];
    for (const chunk of chunks) {
      const frames = (chunk.length / this.channels / fin.bytes) | 0;
      const [, cap] = this._prepare({ length: frames * this.channels * asBytes }, asBytes);
      inFrames.push(frames);
      caps.push(cap);
    }
    return { fin, fout, inFrames, caps };
  }

  /**
   * processChunkFormat for a list of consecutive chunks as ONE transfer each way, one conversion pass per side and
   * (normally) one resampling launch -- a microphone's float32 stream, a G.711 RTP payload stream, a 24-bit WAV as the
   * file system hands it out.  Returns one Buffer per chunk, byte-identical to calling processChunkFormat on each in
   * turn (the capacity rule is applied per original chunk; dither runs on across the chunks).
   */
  processChunksFormat(chunks, inFormat, outFormat) {
    this._refuseWhileAsyncPending('processChunksFormat');
    const a = this._prepareFormat(chunks, inFormat, outFormat);
    return speexModule.processChunksFormat(this._resamplerPtr, chunks, a.fin.id, a.fout.id, a.inFrames, a.caps);
  }

  /** processChunksFormat off the event loop (one pool-thread call for the whole list); chained with the instance's other async calls. */
  processChunksFormatAsync(chunks, inFormat, outFormat) {
    let a;
    try {
      a = this._prepareFormat(chunks, inFormat, outFormat);
    } catch (e) {
      return Promise.reject(e);
    }
    const run = () => speexModule.processChunksFormatAsync(this._resamplerPtr, chunks, a.fin.id, a.fout.id, a.inFrames, a.caps);
    this._inFlight++;
    const settle = () => { this._inFlight--; };
    const p = (this._pending || Promise.resolve()).then(run, run);
    this._pending = p.then(settle, settle);
    return p;
  }

  /**
   * processChunkFormat that does not block the event loop.  Calls on one instance are chained; calls of DIFFERENT
   * instances that become ready in the same tick leave as ONE fused native call, whatever formats they name
   * (speexhip_resampler_process_many_fmt), exactly as processChunkAsync's do.  A lone call takes the single-state path.
   * Resolves to the same bytes processChunkFormat returns.
   */
  processChunkFormatAsync(chunk, inFormat, outFormat) {
    let a;
    try {
      a = this._prepareFormat([chunk], inFormat, outFormat);
    } catch (e) {
      return Promise.reject(e);
    }
    const run = () => new Promise((resolve, reject) => {
      formatTickQueue.push({ handle: this._resamplerPtr, chunk, inFrames: a.inFrames[0], cap: a.caps[0], inFmt: a.fin.id,
        outFmt: a.fout.id, resolve, reject });
      if (!formatTickScheduled) {
        formatTickScheduled = true;
        process.nextTick(flushFormatTick);
      }
    });
    this._inFlight++;
    const settle = () => { this._inFlight--; };
    const p = (this._pending || Promise.resolve()).then(run, run);
    this._pending = p.then(settle, settle);
    return p;
  }

  /**
   * processChunkFormat with a channel mix on either side, done on the GPU in the same two passes that convert the samples.
   * This instance's `channels` is the count the resampler runs on; inMix (rows = channels, columns = the chunk's channel
   * count) turns every input frame into a frame of the resampler, outMix (rows = the result's channel count, columns =
   * channels) every frame it made into an output frame; null = no mix on that side.  48 kHz stereo s16le to 16 kHz mono
   * float for a speech model: new SpeexResampler(1, 48000, 16000).processChunkMix(chunk, 's16le', 'f32le-normalized',
   * [[0.5, 0.5]], null) -- the filter runs on one channel, not two.  Up to 8 channels on either side of a matrix.
   */
  processChunkMix(chunk, inFormat, outFormat, inMix, outMix) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    this._refuseWhileAsyncPending('processChunkMix');
    const fin = SAMPLE_FORMATS[inFormat];
    const fout = SAMPLE_FORMATS[outFormat];
    if (!fin || !fout) {
      throw new Error('Unknown sample format: ' + (fin ? outFormat : inFormat));
    }
    if (inMix == null && outMix == null) return this.processChunkFormat(chunk, inFormat, outFormat);
    // rows x columns, rectangular, 1..8 either way
    const flat = (m, rows, cols, name) => {
      if (m == null) return null;
      const ok = Array.isArray(m) && m.length >= 1 && m.length <= 8 && (rows === undefined || m.length === rows) &&
        m.every((r) => Array.isArray(r) && r.length >= 1 && r.length <= 8 && r.length === m[0].length &&
          (cols === undefined || r.length === cols) && r.every((v) => typeof v === 'number'));
      if (!ok || this.channels > 8) {
        throw new Error(name + ' should be ' + (rows === undefined ? 'rows of ' + cols : rows + ' rows of') +
          ' numbers, at most 8 x 8');
      }
      return Float32Array.from(m.flat());
    };
    const mi = flat(inMix, this.channels, undefined, 'inMix');
    const mo = flat(outMix, undefined, this.channels, 'outMix');
    const inChannels = mi ? inMix[0].length : this.channels;
    const outChannels = mo ? outMix.length : this.channels;
    if (chunk.length % (inChannels * fin.bytes) !== 0) {
      throw new Error('Chunk length should be a multiple of channels * ' + fin.bytes + ' bytes');
    }
    // the capacity rule of processChunkFloat on these frames of the resampler's channel count
    const frames = (chunk.length / inChannels / fin.bytes) | 0;
    const [, cap] = this._prepare({ length: frames * this.channels * Float32Array.BYTES_PER_ELEMENT }, Float32Array.BYTES_PER_ELEMENT);
    return speexModule.processMix(this._resamplerPtr, chunk, fin.id, fout.id, frames, cap, inChannels, mi, outChannels, mo);
  }

  /**
   * processChunkMix with a layout per side: either side may be planar (one typed array per channel) instead of interleaved.
   * `input` is a Buffer of interleaved frames, or an array of typed arrays, one per input channel, each holding the
   * plane's bytes in inSide.format (Web Audio's getChannelData planes are Float32Array in 'f32le-normalized'; a packed
   * 's24le' plane is a Uint8Array of 3 bytes per sample).  inSide: { format, mix? }; outSide: { format, planar?, channels?,
   * mix? } -- planar: true gives an array of typed arrays of the format's element type (Uint8Array for the 1-byte formats
   * and 's24le', Int16Array, Int32Array, Float32Array; typed arrays are host-endian, so planes of the big-endian formats are
   * Uint8Array, and half-float planes are Uint16Array of the bits -- a Float16Array is accepted on input where the runtime
   * defines one), otherwise a Buffer.  It is processChunkMix on the same samples
   * arranged as interleaved frames: the same values, the same stream state; with a planar side every format pair runs by
   * processChunkFloat's capacity rule.  A decoder's interleaved s16le to a model's float planes:
   * r.processChunkSides(chunk, { format: 's16le' }, { format: 'f32le-normalized', planar: true }); Web Audio planes in and
   * out: r.processChunkSides(planes, { format: 'f32le-normalized' }, { format: 'f32le-normalized', planar: true }).
   */
  processChunkSides(input, inSide, outSide) {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    this._refuseWhileAsyncPending('processChunkSides');
    const fin = SAMPLE_FORMATS[inSide && inSide.format];
    const fout = SAMPLE_FORMATS[outSide && outSide.format];
    if (!fin || !fout) {
      throw new Error('Unknown sample format: ' + (fin ? outSide && outSide.format : inSide && inSide.format));
    }
    const planarIn = Array.isArray(input);
    const planarOut = !!outSide.planar;
    const inMix = inSide.mix == null ? null : inSide.mix;
    const outMix = outSide.mix == null ? null : outSide.mix;
    if (!planarIn && !planarOut) return this.processChunkMix(input, inSide.format, outSide.format, inMix, outMix);
    const flat = (m, rows, cols, name) => {
      if (m == null) return null;
      const ok = Array.isArray(m) && m.length >= 1 && m.length <= 8 && (rows === undefined || m.length === rows) &&
        m.every((r) => Array.isArray(r) && r.length >= 1 && r.length <= 8 && r.length === m[0].length &&
          (cols === undefined || r.length === cols) && r.every((v) => typeof v === 'number'));
      if (!ok || this.channels > 8) {
        throw new Error(name + ' should be ' + (rows === undefined ? 'rows of ' + cols : rows + ' rows of') +
          ' numbers, at most 8 x 8');
      }
      return Float32Array.from(m.flat());
    };
    const mi = flat(inMix, this.channels, undefined, 'inSide.mix');
    const mo = flat(outMix, undefined, this.channels, 'outSide.mix');
    const inChannels = mi ? inMix[0].length : this.channels;
    const outChannels = mo ? outMix.length : this.channels;
    if (outSide.channels !== undefined && outSide.channels !== outChannels) {
      throw new Error('outSide.channels should be ' + outChannels);
    }
    let frames;
    if (planarIn) {
      const ok = input.length === inChannels && input.every((p) => ArrayBuffer.isView(p) && p.byteLength === input[0].byteLength);
      if (!ok || input[0].byteLength % fin.bytes !== 0) {
        throw new Error('input should be ' + inChannels + ' typed arrays of equal length, whole samples of ' + fin.bytes + ' bytes');
      }
      frames = (input[0].byteLength / fin.bytes) | 0;
    } else {
      if (input.length % (inChannels * fin.bytes) !== 0) {
        throw new Error('Chunk length should be a multiple of channels * ' + fin.bytes + ' bytes');
      }
      frames = (input.length / inChannels / fin.bytes) | 0;
    }
    // the capacity rule of processChunkFloat on these frames of the resampler's channel count
    const [, cap] = this._prepare({ length: frames * this.channels * Float32Array.BYTES_PER_ELEMENT }, Float32Array.BYTES_PER_ELEMENT);
    // kind of a result plane: Uint8Array, Int16Array, Int32Array, Float32Array, Uint16Array
    const kind = BIG_ENDIAN_IDS.includes(fout.id) ? 0 : HALF_FLOAT_IDS.includes(fout.id) ? 4
      : fout.bytes === 2 ? 1 : fout.bytes === 4 ? (fout.id === 3 ? 2 : 3) : 0;
    // (a Float16Array plane, where the runtime defines one, travels as its bits)
    if (planarIn && typeof Float16Array !== 'undefined') {
      input = input.map((p) => (p instanceof Float16Array ? new Uint16Array(p.buffer, p.byteOffset, p.length) : p));
    }
    return speexModule.processSides(this._resamplerPtr, input, fin.id, fout.id, frames, cap, inChannels, mi, outChannels, mo,
      planarOut, kind);
  }

  /** Mid-stream control (SURVEY 8f row N3; speex_resampler_set_rate / set_quality / ...). */
  setRate(inRate, outRate) {
    this._refuseWhileAsyncPending('setRate');
    if (this._resamplerPtr) speexModule.setRate(this._resamplerPtr, inRate >>> 0, outRate >>> 0);
    this.inRate = inRate;
    this.outRate = outRate;
  }

  setQuality(quality) {
    this._refuseWhileAsyncPending('setQuality');
    if (this._resamplerPtr) speexModule.setQuality(this._resamplerPtr, quality | 0);
    this.quality = quality;
  }

  /**
   * Arithmetic of this instance's kernels: 'fast_fixed' (the default since round 6: every sample within +-1 LSB of the
   * reference, fp64 sums where the reference has them -- quality 9 and 10 -- and, like the reference's, bytes that do not
   * depend on how the stream is cut into chunks, on how many streams share a launch or on the GPU), 'fast' (the same
   * tolerance; small launches of long filters may split a sum over several waves: up to 2x faster there, but the last bit
   * then depends on the chunking), 'exact' (bit-identical to the reference, slower), 'fast_f32' (one fp32 FMA chain for
   * every filter: the fast path of the first releases).  The environment variable SPEEXHIP_MODE sets the initial mode of
   * every instance.
   */
  setMode(mode) {
    this._refuseWhileAsyncPending('setMode');
    const code = { fast: 0, exact: 1, fast_f32: 2, fast_fixed: 3 }[mode];
    if (code === undefined) throw new Error("mode must be 'fast', 'exact', 'fast_f32' or 'fast_fixed'");
    speexModule.setMode(this._ensureNative(), code);
  }

  /**
   * Dither of the integer results ('u8', 's16le', 's24le', 's32le', 's16be', 's24be', 's32be', and 'mulaw' / 'alaw', where
   * the noise joins the int16 value the compressor takes; the half-float results are float results: never dithered) of processChunkFormat and processChunkMix: 'none' (the
   * default: round half up), 'rectangular' (uniform in +-0.5 LSB) or 'triangular' (TPDF, +-1 LSB: the error of a
   * requantised signal becomes noise instead of harmonics).  The noise of a sample is a pure function of (seed, its index
   * in the stream), so the bytes do not depend on how the stream is cut into chunks; `position` is the index of the next
   * output frame (resume a stream in a new instance with the seed and getDither().position of the old one).  While on,
   * 's16le' -> 's16le' runs as processChunkFloat between the two conversions.  seed and position: bigint or number.
   */
  setDither(kind, seed = 0n, position = 0n) {
    this._refuseWhileAsyncPending('setDither');
    const code = DITHER_KINDS.indexOf(kind);
    if (code < 0) throw new Error("dither must be 'none', 'rectangular' or 'triangular'");
    const s = BigInt.asUintN(64, BigInt(seed));
    const p = BigInt.asUintN(64, BigInt(position));
    speexModule.setDither(this._ensureNative(), code, Number(s & 0xffffffffn), Number(s >> 32n), Number(p & 0xffffffffn),
      Number(p >> 32n));
  }

  /** { kind, seed, position }: seed and position are bigints; position = output frames made with dither on so far */
  getDither() {
    const [code, sLo, sHi, pLo, pHi] = speexModule.getDither(this._ensureNative());
    return { kind: DITHER_KINDS[code], seed: (BigInt(sHi) << 32n) | BigInt(sLo), position: (BigInt(pHi) << 32n) | BigInt(pLo) };
  }

  /**
   * The output meter of processChunkFormat, processChunkMix and processChunkSides (and their chunk-list, many-instance and
   * asynchronous forms): while on, every sample they encode is judged on its way out -- clipped at the upper or the lower rail of
   * an integer or companded format, NaN, and the peak |value| in int16 units (above 32768: beyond +-1.0; the float results
   * count no clips, their callers read the peak).  processChunk, processChunkFloat and the planar calls are never metered.
   * The totals are kept while the meter is off.  While on, 's16le' -> 's16le' runs as processChunkFloat between the two
   * conversions.  The totals of a stream do not depend on how it is cut into chunks.
   */
  setMeter(on) {
    this._refuseWhileAsyncPending('setMeter');
    speexModule.setMeter(this._ensureNative(), !!on);
  }

  /**
   * { on, samples, clippedHigh, clippedLow, nan, peak } since the last reset; the counts are bigints.  Waits for this
   * instance's own last call only.  { reset: true } clears the totals behind the read.
   */
  getMeter(options = undefined) {
    this._refuseWhileAsyncPending('getMeter');
    const v = speexModule.getMeter(this._ensureNative(), !!(options && options.reset));
    const big = (i) => (BigInt(v[i + 1]) << 32n) | BigInt(v[i]);
    return { on: v[0] !== 0, samples: big(1), clippedHigh: big(3), clippedLow: big(5), nan: big(7), peak: v[9] };
  }

  /**
   * The output gain of processChunkFormat, processChunkMix and processChunkSides (and their chunk-list, many-instance and
   * asynchronous forms, flushFormat included): `gain` from the next output frame on, reached over rampFrames output frames
   * from the gain that frame would have had, linearly -- a change without a click; rampFrames = 0 is a step.  Each sample
   * is multiplied once, in float, before it is judged by the meter, dithered and encoded.  Negative gains (polarity) and 0
   * (mute) are legal; a gain that is not finite throws.  A new target in mid-ramp starts from where the ramp stands.
   * processChunk, processChunkFloat and the planar calls never apply it.  While the gain is not 1 (or a ramp is in flight)
   * 's16le' -> 's16le' runs as processChunkFloat between the two conversions.  A stream's bytes do not depend on how it
   * is cut into chunks.
   */
  setGain(gain, rampFrames = 0) {
    this._refuseWhileAsyncPending('setGain');
    checkGain(gain, rampFrames);
    speexModule.setGain(this._ensureNative(), gain, rampFrames);
  }

  /** { current, target, remaining }: the next output frame's gain, the ramp's target, its output frames still to come */
  getGain() {
    this._refuseWhileAsyncPending('getGain');
    const v = speexModule.getGain(this._ensureNative());
    return { current: v[0], target: v[1], remaining: v[2] };
  }

  /** Start half a filter in, so the stream does not begin with the filter's ramp-up. */
  skipZeros() {
    this._refuseWhileAsyncPending('skipZeros');
    speexModule.skipZeros(this._ensureNative());
  }

  resetMem() {
    this._refuseWhileAsyncPending('resetMem');
    speexModule.resetMem(this._ensureNative());
  }

  /** Frames of delay the filter adds, counted at the input rate / at the output rate. */
  get inputLatency() { return speexModule.getLatency(this._ensureNative())[0]; }

  get outputLatency() { return speexModule.getLatency(this._ensureNative())[1]; }

  /**
   * The tail the reference never emits (SURVEY 8f row N4): feeds inputLatency frames of silence
   * and returns what comes out -- the response to the last real input frames.
   */
  flush() {
    this._refuseWhileAsyncPending('flush');
    const ptr = this._ensureNative();
    const frames = speexModule.getLatency(ptr)[0];
    const cap = Math.ceil(frames * this.outRate / this.inRate) + 1;
    return speexModule.process(ptr, null, frames, cap);
  }

  /** flush() with the tail in outFormat: inputLatency frames of silence in, what comes out as processChunkFormat writes it. */
  flushFormat(outFormat) {
    this._refuseWhileAsyncPending('flushFormat');
    const fout = SAMPLE_FORMATS[outFormat];
    if (!fout) throw new Error('Unknown sample format: ' + outFormat);
    const ptr = this._ensureNative();
    const frames = speexModule.getLatency(ptr)[0];
    const cap = Math.ceil(frames * this.outRate / this.inRate) + 1;
    // (silence has no format: 's16le' keeps flush()'s own call for an 's16le' tail, every other tail is the float call's)
    return speexModule.processFormat(ptr, null, fout.id === 1 ? 1 : 4, fout.id, frames, cap);
  }

  /** Release the GPU state now (otherwise it goes with garbage collection). */
  destroy() {
    this._refuseWhileAsyncPending('destroy');
    if (this._resamplerPtr) speexModule.destroy(this._resamplerPtr);
    this._resamplerPtr = undefined;
    this._outBufferSize = -1;
  }

  /** GPU this instance lives on (-1 until its native state exists). */
  get device() { return this._resamplerPtr ? speexModule.getInfo(this._resamplerPtr).device : this._device; }
}
SpeexResampler.initPromise = globalModulePromise;
/** Extension: GPUs the library can place instances on (<= 0: none -- there is no CPU fallback). */
SpeexResampler.deviceCount = () => {
  if (!speexModule) {
    throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
  }
  return speexModule.deviceCount();
};

/**
 * Extension (round 6): a Buffer of `bytes` bytes over a PINNED block of the library for the caller to fill -- read a file
 * or a socket into it, let a decoder write into it -- and hand to processChunk / processChunks / SpeexResamplerBatch.
 * The library recognises its own blocks and lets the GPU read the chunk where it lies, through PCIe, while it writes the
 * result block: no staging copy (the reference copies every chunk into the WASM heap, src/index.ts:71-92).  Results are
 * the same bytes as for an ordinary Buffer.  When no block is free an ordinary Buffer comes back (same results, the usual
 * staging).  The chunk may be refilled as soon as the call that read it has returned / its promise has settled.
 */
SpeexResampler.allocChunk = (bytes) => {
  if (!speexModule) {
    throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
  }
  return speexModule.allocChunk(bytes);
};

// processChunkAsync calls that became ready in this tick (see there)
const tickQueue = [];
let tickScheduled = false;
function flushTick() {
  tickScheduled = false;
  const jobs = tickQueue.splice(0, tickQueue.length);
  if (jobs.length === 0) return;
  if (jobs.length === 1) {
    const j = jobs[0];
    speexModule.processAsync(j.handle, j.chunk, j.inFrames, j.cap).then(j.resolve, j.reject);
    return;
  }
  let promise;
  try {
    promise = speexModule.processManyAsync(jobs.map((j) => j.handle), jobs.map((j) => j.chunk),
      jobs.map((j) => j.inFrames), jobs.map((j) => j.cap));
  } catch (e) {
    for (const j of jobs) j.reject(e);
    return;
  }
  promise.then((outs) => { jobs.forEach((j, i) => j.resolve(outs[i])); },
    (e) => {
      // The instances of a tick are independent (the reference's model: one failing instance does not touch the
      // others): when the native call ran, its error carries every entry's own code and result -- entries that
      // succeeded have advanced and get their audio, only the offending ones reject.
      if (e && Array.isArray(e.codes) && Array.isArray(e.results) && e.codes.length === jobs.length) {
        const first = e.codes.find((c) => c !== 0);
        jobs.forEach((j, i) => {
          if (e.codes[i] === 0) j.resolve(e.results[i]);
          else j.reject(e.codes[i] === first ? e : new Error(speexModule.strerror(e.codes[i])));
        });
      } else {
        for (const j of jobs) j.reject(e);
      }
    });
}

// processChunkFormatAsync calls that became ready in this tick: one fused call of all of them, as flushTick above
const formatTickQueue = [];
let formatTickScheduled = false;
function flushFormatTick() {
  formatTickScheduled = false;
  const jobs = formatTickQueue.splice(0, formatTickQueue.length);
  if (jobs.length === 0) return;
  if (jobs.length === 1) {
    const j = jobs[0];
    speexModule.processChunksFormatAsync(j.handle, [j.chunk], j.inFmt, j.outFmt, [j.inFrames], [j.cap])
      .then((outs) => j.resolve(outs[0]), j.reject);
    return;
  }
  let promise;
  try {
    promise = speexModule.processManyFormatAsync(jobs.map((j) => j.handle), jobs.map((j) => j.chunk),
      jobs.map((j) => j.inFrames), jobs.map((j) => j.cap), jobs.map((j) => j.inFmt), jobs.map((j) => j.outFmt));
  } catch (e) {
    for (const j of jobs) j.reject(e);
    return;
  }
  promise.then((outs) => { jobs.forEach((j, i) => j.resolve(outs[i])); },
    (e) => {
      // (the instances of a tick are independent: entries that succeeded get their audio, only the offending ones reject)
      if (e && Array.isArray(e.codes) && Array.isArray(e.results) && e.codes.length === jobs.length) {
        const first = e.codes.find((c) => c !== 0);
        jobs.forEach((j, i) => {
          if (e.codes[i] === 0) j.resolve(e.results[i]);
          else j.reject(e.codes[i] === first ? e : new Error(speexModule.strerror(e.codes[i])));
        });
      } else {
        for (const j of jobs) j.reject(e);
      }
    });
}

/**
 * Extension: n independent streams with one (channels, rates, quality) -- n SpeexResampler instances, each with its
 * own grow-only capacity rule (reference src/index.ts:80-95 per instance) -- whose chunks of one step travel and run
 * together: per GPU one transfer in, ONE launch per <= 32 streams, one transfer out.  With SPEEXHIP_DEVICES=all (or
 * options.devices = [0, 1, ...]) the streams spread over the node's GPUs, stream k on the k-th of them modulo their
 * number, and the GPUs work side by side.  Results are byte-identical (mode 'exact') / within +-1 LSB (default) to
 * calling processChunk on n separate instances.
 */
class SpeexResamplerBatch {
  constructor(nStreams, channels, inRate, outRate, quality = 7, options = undefined) {
    if (!Number.isInteger(nStreams) || nStreams < 1) throw new Error('nStreams must be a positive integer');
    this.channels = channels;
    this.inRate = inRate;
    this.outRate = outRate;
    this.quality = quality;
    const devices = options && Array.isArray(options.devices) && options.devices.length > 0 ? options.devices : null;
    this.streams = [];
    for (let k = 0; k < nStreams; k++) {
      this.streams.push(new SpeexResampler(channels, inRate, outRate, quality,
        devices ? { device: devices[k % devices.length] } : undefined));
    }
  }

  get length() { return this.streams.length; }

  _gather(chunks) {
    if (!Array.isArray(chunks) || chunks.length !== this.streams.length) {
      throw new Error('processChunks expects one chunk (or null) per stream: ' + this.streams.length);
    }
    // every chunk is checked before any stream's state is touched (lazy init, capacity rule): a step is refused whole
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    for (let k = 0; k < chunks.length; k++) {
      if (chunks[k] === null || chunks[k] === undefined) continue;
      if (chunks[k].length % (this.channels * Uint16Array.BYTES_PER_ELEMENT) !== 0) {
        throw new Error('Chunk length should be a multiple of channels * 2 bytes');
      }
    }
    const picked = { index: [], handles: [], chunks: [], inFrames: [], caps: [] };
    for (let k = 0; k < chunks.length; k++) {
      if (chunks[k] === null || chunks[k] === undefined) continue; // this stream sits the step out
      const [f, cap] = this.streams[k]._prepare(chunks[k], Uint16Array.BYTES_PER_ELEMENT);
      picked.index.push(k);
      picked.handles.push(this.streams[k]._resamplerPtr);
      picked.chunks.push(chunks[k]);
      picked.inFrames.push(f);
      picked.caps.push(cap);
    }
    return picked;
  }

  /**
   * One chunk of interleaved s16le PCM per stream (null / undefined: the stream sits this step out) in, one fresh
   * Buffer per stream out (null for streams that sat out): entry k is what streams[k].processChunk(chunks[k]) returns.
   */
  processChunks(chunks) {
    for (const r of this.streams) r._refuseWhileAsyncPending('SpeexResamplerBatch.processChunks');
    const g = this._gather(chunks);
    const outs = g.handles.length > 0 ? speexModule.processMany(g.handles, g.chunks, g.inFrames, g.caps) : [];
    const result = new Array(this.streams.length).fill(null);
    g.index.forEach((k, i) => { result[k] = outs[i]; });
    return result;
  }

  /** processChunks off the event loop; steps are chained, so the streams advance in the order of the calls. */
  processChunksAsync(chunks) {
    let g;
    try {
      g = this._gather(chunks);
    } catch (e) {
      return Promise.reject(e);
    }
    return this._chainStep(g, () => speexModule.processManyAsync(g.handles, g.chunks, g.inFrames, g.caps));
  }

  // one asynchronous step of the gathered streams `g`: `call` makes the native call once the step's turn has come
  _chainStep(g, call) {
    const run = () => (g.handles.length > 0 ? call() : Promise.resolve([]))
      .then((outs) => {
        const result = new Array(this.streams.length).fill(null);
        g.index.forEach((k, i) => { result[k] = outs[i]; });
        return result;
      });
    // (while the step is pending the synchronous methods of its streams refuse, like after processChunkAsync: the
    //  results were sized from the streams' counters when the step was queued)
    for (const k of g.index) this.streams[k]._inFlight++;
    const settle = () => { for (const k of g.index) this.streams[k]._inFlight--; };
    // The step waits for the batch's previous step AND for what its streams have pending of their own
    // (streams[k].processChunkAsync), and later asynchronous calls of those streams wait for the step: a stream's calls
    // stay in the order they were made, whichever object they were made through (ADVICE r5 -- the native call
    // checks the same thing again under its locks and refuses the step rather than overrun a result).
    const before = [this._pending].concat(g.index.map((k) => this.streams[k]._pending)).filter(Boolean);
    const p = Promise.all(before.map((q) => q.then(() => {}, () => {}))).then(run);
    const done = p.then(settle, settle);
    this._pending = done;
    for (const k of g.index) this.streams[k]._pending = done;
    return p;
  }

  // processChunksFormat: a format name for all streams, or an array with one name per stream
  _formatsOf(format, what) {
    const names = Array.isArray(format) ? format : new Array(this.streams.length).fill(format);
    if (names.length !== this.streams.length) {
      throw new Error(what + ' expects one format name, or one per stream: ' + this.streams.length);
    }
    return names.map((name) => {
      const f = SAMPLE_FORMATS[name];
      if (!f) throw new Error('Unknown sample format: ' + name);
      return f;
    });
  }

  _gatherFormat(chunks, inFormat, outFormat) {
    if (!Array.isArray(chunks) || chunks.length !== this.streams.length) {
      throw new Error('processChunksFormat expects one chunk (or null) per stream: ' + this.streams.length);
    }
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    // formats and chunks are all checked before any stream's state is touched: a step is refused whole
    const fin = this._formatsOf(inFormat, 'processChunksFormat');
    const fout = this._formatsOf(outFormat, 'processChunksFormat');
    for (let k = 0; k < chunks.length; k++) {
      if (chunks[k] === null || chunks[k] === undefined) continue;
      if (chunks[k].length % (this.channels * fin[k].bytes) !== 0) {
        throw new Error('Chunk length should be a multiple of channels * ' + fin[k].bytes + ' bytes');
      }
    }
    const picked = { index: [], handles: [], chunks: [], inFrames: [], caps: [], inFmts: [], outFmts: [] };
    for (let k = 0; k < chunks.length; k++) {
      if (chunks[k] === null || chunks[k] === undefined) continue; // this stream sits the step out
      // the capacity rule of streams[k].processChunkFormat on these frames
      const frames = (chunks[k].length / this.channels / fin[k].bytes) | 0;
      const asBytes = fin[k].id === 1 && fout[k].id === 1 ? Uint16Array.BYTES_PER_ELEMENT : Float32Array.BYTES_PER_ELEMENT;
      const [, cap] = this.streams[k]._prepare({ length: frames * this.channels * asBytes }, asBytes);
      picked.index.push(k);
      picked.handles.push(this.streams[k]._resamplerPtr);
      picked.chunks.push(chunks[k]);
      picked.inFrames.push(frames);
      picked.caps.push(cap);
      picked.inFmts.push(fin[k].id);
      picked.outFmts.push(fout[k].id);
    }
    return picked;
  }

  /**
   * processChunks with sample formats: one chunk per stream (null / undefined: the stream sits this step out) in the
   * stream's input format, one fresh Buffer per stream out in its output format -- entry k is what
   * streams[k].processChunkFormat(chunks[k], inFormat[k], outFormat[k]) returns, all streams in ONE fused library call: a
   * gateway's PCMU, PCMA and L16 legs of a 20 ms tick as b.processChunksFormat(payloads, ['mulaw', 'alaw', 's16be', ...],
   * 'f32le-normalized').  inFormat / outFormat: one of processChunkFormat's names for all streams, or an array with one name
   * per stream.
   */
  processChunksFormat(chunks, inFormat, outFormat) {
    for (const r of this.streams) r._refuseWhileAsyncPending('SpeexResamplerBatch.processChunksFormat');
    const g = this._gatherFormat(chunks, inFormat, outFormat);
    const outs = g.handles.length > 0
      ? speexModule.processManyFormat(g.handles, g.chunks, g.inFrames, g.caps, g.inFmts, g.outFmts) : [];
    const result = new Array(this.streams.length).fill(null);
    g.index.forEach((k, i) => { result[k] = outs[i]; });
    return result;
  }

  /** processChunksFormat off the event loop, ordered with the streams' other asynchronous calls like processChunksAsync. */
  processChunksFormatAsync(chunks, inFormat, outFormat) {
    let g;
    try {
      g = this._gatherFormat(chunks, inFormat, outFormat);
    } catch (e) {
      return Promise.reject(e);
    }
    return this._chainStep(g, () => speexModule.processManyFormatAsync(g.handles, g.chunks, g.inFrames, g.caps, g.inFmts, g.outFmts));
  }

  setMode(mode) { for (const r of this.streams) r.setMode(mode); }

  /** setDither of every stream: stream k draws from seed + k * 0x9E3779B97F4A7C15 (mod 2^64), as a batch of the C API */
  setDither(kind, seed = 0n, position = 0n) {
    this.streams.forEach((r, k) => r.setDither(kind, BigInt.asUintN(64, BigInt(seed) + BigInt(k) * 0x9E3779B97F4A7C15n), position));
  }

  /** getDither of stream k (its own seed and position) */
  getDither(stream = 0) { return this.streams[stream].getDither(); }

  /** setMeter of every stream */
  setMeter(on) { for (const r of this.streams) r.setMeter(on); }

  /** getMeter of stream k: its own totals; { reset: true } clears that stream only */
  getMeter(stream = 0, options = undefined) { return this.streams[stream].getMeter(options); }

  /** setGain of stream k, or of every stream when none is named */
  setGain(gain, rampFrames = 0, stream = undefined) {
    if (stream === undefined) for (const r of this.streams) r.setGain(gain, rampFrames);
    else this.streams[stream].setGain(gain, rampFrames);
  }

  /** getGain of stream k */
  getGain(stream = 0) { return this.streams[stream].getGain(); }

  destroy() { for (const r of this.streams) r.destroy(); }
}
/**
 * Extension.  A mixer: mix buses over many separate SpeexResampler instances in ONE library call per tick -- a conference
 * bridge whose legs are G.711 at 8 kHz, wideband at 16 kHz and studio feeds at 48 kHz, every participant's mix-minus feed
 * encoded on the GPU.  nLegs slots, nBuses buses, one channel count; every leg keeps its own rates, quality, gain and ramp
 * (leg.setGain) and is fed in its own sample format.  Bus j is the sum, in ascending slot order and in float64, rounded
 * once, of rows[j][i] times slot i's output of the call; it leaves in outFormat through the format's encoder, the mixer's
 * dither and the mixer's meter.  Only the buses travel back: nothing of a leg is encoded.
 */
class SpeexResamplerMixer {
  constructor(nLegs, nBuses, channels, options = undefined) {
    for (const [v, name] of [[nLegs, 'nLegs'], [nBuses, 'nBuses'], [channels, 'channels']]) {
      if (!Number.isInteger(v) || v < 1) throw new Error(name + ' must be a positive integer');
    }
    if (nLegs > 1024 || nBuses > 1024) throw new Error('a mixer has at most 1024 legs and 1024 buses');
    this.nLegs = nLegs;
    this.nBuses = nBuses;
    this.channels = channels;
    this.legs = new Array(nLegs).fill(null);
    this._device = options && Number.isInteger(options.device) ? options.device : -1;
    this._ptr = undefined;
  }

  _native() {
    if (!speexModule) {
      throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
    }
    if (!this._ptr) this._ptr = speexModule.mixerInit(this.nLegs, this.nBuses, this.channels, this._device);
    return this._ptr;
  }

  /** the SpeexResampler in slot i (its channel count must be the mixer's), or null: an empty slot */
  setLeg(i, resampler) {
    if (!Number.isInteger(i) || i < 0 || i >= this.nLegs) throw new Error('no such slot: ' + i);
    if (resampler !== null && !(resampler instanceof SpeexResampler)) throw new Error('a leg is a SpeexResampler or null');
    if (resampler !== null && resampler.channels !== this.channels) throw new Error('a leg has the mixer\'s channel count: ' + this.channels);
    this.legs[i] = resampler;
  }

  /** rows[j][i] = the weight of slot i in bus j (nBuses rows of nLegs finite numbers; mix-minus: 1 everywhere, 0 on the
   *  diagonal); null turns the mixer off.  Zeroes the bus meters and the buses' dither position. */
  setWeights(rows) {
    if (rows === null) {
      speexModule.mixerSetWeights(this._native(), null);
      return;
    }
    if (!Array.isArray(rows) || rows.length !== this.nBuses) throw new Error('setWeights expects ' + this.nBuses + ' rows');
    const w = new Float32Array(this.nBuses * this.nLegs);
    rows.forEach((row, j) => {
      if (!row || row.length !== this.nLegs) throw new Error('setWeights expects rows of ' + this.nLegs + ' weights');
      for (let i = 0; i < this.nLegs; i++) {
        if (typeof row[i] !== 'number' || !Number.isFinite(row[i])) throw new Error('a weight must be a finite number');
        w[j * this.nLegs + i] = row[i];
      }
    });
    speexModule.mixerSetWeights(this._native(), Buffer.from(w.buffer));
  }

  /** dither of the buses' integer and companded outputs: bus j draws from seed + (nLegs + j) * 0x9E3779B97F4A7C15 (mod 2^64) */
  setDither(kind, seed = 0n, position = 0n) {
    const code = DITHER_KINDS.indexOf(kind);
    if (code < 0) throw new Error("dither must be 'none', 'rectangular' or 'triangular'");
    const s = BigInt.asUintN(64, BigInt(seed));
    const p = BigInt.asUintN(64, BigInt(position));
    speexModule.mixerSetDither(this._native(), code, Number(s & 0xffffffffn), Number(s >> 32n), Number(p & 0xffffffffn), Number(p >> 32n));
  }

  /** { kind, seed, position }: the seed as given, the buses' one position (bigints) */
  getDither() {
    const [code, sLo, sHi, pLo, pHi] = speexModule.mixerGetDither(this._native());
    return { kind: DITHER_KINDS[code], seed: (BigInt(sHi) << 32n) | BigInt(sLo), position: (BigInt(pHi) << 32n) | BigInt(pLo) };
  }

  setMeter(on) { speexModule.mixerSetMeter(this._native(), !!on); }

  /** getMeter's object, of bus j's own cell; { reset: true } clears that bus only */
  getBusMeter(j, options = undefined) {
    const v = speexModule.mixerGetBusMeter(this._native(), j >>> 0, !!(options && options.reset));
    const big = (i) => (BigInt(v[i + 1]) << 32n) | BigInt(v[i]);
    return { on: v[0] !== 0, samples: big(1), clippedHigh: big(3), clippedLow: big(5), nan: big(7), peak: v[9] };
  }

  /** per-leg levels of every tick, measured on the device (off by default; a change clears the last tick's records) */
  setLevels(on) { speexModule.mixerSetLevels(this._native(), !!on); }

  /**
   * The last tick's record of every slot, measured on the leg's output BEFORE its gain: { samples, energy, nan
   * (BigUint64Array), peak (Float32Array, int16 units), audioLevel (Uint8Array: RFC 6464, 0 loudest .. 127) }.
   */
  getLevels() {
    const raw = speexModule.mixerGetLevels(this._native());
    const n = this.nLegs;
    const view = new DataView(raw.buffer, raw.byteOffset, raw.byteLength);
    const out = { samples: new BigUint64Array(n), energy: new BigUint64Array(n), nan: new BigUint64Array(n), peak: new Float32Array(n), audioLevel: new Uint8Array(n) };
    for (let i = 0; i < n; i++) {
      out.samples[i] = view.getBigUint64(32 * i, true);
      out.energy[i] = view.getBigUint64(32 * i + 8, true);
      out.nan[i] = view.getBigUint64(32 * i + 16, true);
      out.peak[i] = view.getFloat32(32 * i + 24, true);
      const e = Number(out.energy[i]), s = Number(out.samples[i]);
      out.audioLevel[i] = e === 0 || s === 0 ? 127 : Math.min(127, Math.max(0, Math.round(-10 * Math.log10(e / (s * 2 ** 30)))));
    }
    return out;
  }

  /**
   * One tick, synchronously.  chunks[i]: the Buffer of slot i's interleaved frames in its input format (null / undefined
   * for an empty slot; an empty Buffer: the leg runs on nothing); inFormats: one of processChunkFormat's names for all
   * slots, or one per slot; outFormat: the buses' format.  Every leg advances as by processChunkFormat(chunk, inFormat,
   * 'f32le') -- the same state, the same grow-only capacity rule -- and its gain ramp by the frames it produced.
   * Returns { buses: Buffer[] (bus j: busFrames interleaved frames in outFormat), busFrames, produced: number[], codes:
   * number[] }: codes[i] !== 0 is a leg the library refused -- its state untouched, silence in the sum, the tick not lost.
   * Refuses while a leg has an asynchronous call pending, as SpeexResamplerBatch.processChunksFormat does.
   */
  process(chunks, inFormats, outFormat) {
    if (!Array.isArray(chunks) || chunks.length !== this.nLegs) throw new Error('process expects one chunk (or null) per slot: ' + this.nLegs);
    const names = Array.isArray(inFormats) ? inFormats : new Array(this.nLegs).fill(inFormats);
    if (names.length !== this.nLegs) throw new Error('process expects one format name, or one per slot: ' + this.nLegs);
    const fout = SAMPLE_FORMATS[outFormat];
    if (!fout) throw new Error('Unknown sample format: ' + outFormat);
    const ptr = this._native();
    // formats and chunks are all checked before any leg's state is touched: a tick is refused whole
    const fin = names.map((name, i) => {
      if (!this.legs[i]) return null;
      const f = SAMPLE_FORMATS[name];
      if (!f) throw new Error('Unknown sample format: ' + name);
      return f;
    });
    for (let i = 0; i < this.nLegs; i++) {
      const leg = this.legs[i];
      if (!leg) continue;
      leg._refuseWhileAsyncPending('SpeexResamplerMixer.process');
      if (chunks[i] === null || chunks[i] === undefined) throw new Error('slot ' + i + ' has a leg and no chunk');
      if (chunks[i].length % (this.channels * fin[i].bytes) !== 0) {
        throw new Error('Chunk length should be a multiple of channels * ' + fin[i].bytes + ' bytes');
      }
    }
    const handles = [], bufs = [], inFrames = [], caps = [], fmts = [];
    for (let i = 0; i < this.nLegs; i++) {
      const leg = this.legs[i];
      if (!leg) {
        handles.push(null), bufs.push(null), inFrames.push(0), caps.push(0), fmts.push(fout.id);
        continue;
      }
      // the capacity rule of leg.processChunkFloat on these frames
      const frames = (chunks[i].length / this.channels / fin[i].bytes) | 0;
      const [, cap] = leg._prepare({ length: frames * this.channels * Float32Array.BYTES_PER_ELEMENT }, Float32Array.BYTES_PER_ELEMENT);
      handles.push(leg._resamplerPtr), bufs.push(chunks[i].length ? chunks[i] : null), inFrames.push(frames), caps.push(cap), fmts.push(fin[i].id);
    }
    const r = speexModule.mixerProcess(ptr, handles, bufs, inFrames, caps, fmts, fout.id);
    return { buses: r.buses, busFrames: r.busFrames, produced: r.produced, codes: r.codes };
  }

  destroy() {
    if (this._ptr) speexModule.mixerDestroy(this._ptr);
    this._ptr = undefined;
  }
}

/**
 * Extension.  Destroyed (or collected) states leave their device buffers, pinned staging buffers and
 * filter tables in a process-wide pool for the next `new SpeexResampler` (DESIGN 3.5); this hands
 * whatever is idle there back to the driver and returns the number of bytes.
 */
SpeexResampler.releaseCachedMemory = () => {
  if (!speexModule) {
    throw new Error('You need to wait for SpeexResampler.initPromise before calling this method');
  }
  return speexModule.releaseCachedMemory();
};

const EMPTY_BUFFER = Buffer.alloc(0);

class SpeexResamplerTransform extends Transform {
  /**
   * Same arguments as SpeexResampler (reference src/index.ts:121-137).  The optional fifth
   * argument is an extension and changes nothing unless set:
   *   coalesceChunks: n  -- hold up to n aligned chunks and resample them in one GPU launch
   *                         (bytes out unchanged, they just arrive n chunks at a time)
   *   async: true        -- run each call off the event loop (processChunkAsync)
   *   flushTail: true    -- at end of stream also emit SpeexResampler.flush()
   *   pipeline: true     -- off the event loop AND batched by load: a chunk that arrives while a call is in flight is
   *                         held, and everything held leaves as ONE call when that one returns (an idle stream sends each
   *                         chunk at once; a busy one sends few, large launches).  Same bytes out.
   *   pinned: true       -- every chunk is copied ONCE into a pinned chunk of the library (SpeexResampler.allocChunk: a ring
   *                         of them, reused) and the GPU reads it there -- in the modes that hold chunks (coalesceChunks,
   *                         async, pipeline) that is the copy they make anyway, landing in pinned memory instead of an
   *                         ordinary Buffer.  Same bytes out.  (A producer that can fill chunks from allocChunk itself needs
   *                         no option: pinned chunks are recognised wherever they arrive.)
   *   inFormat, outFormat -- the stream's sample formats, processChunkFormat's names (default 's16le' each): bytes in
   *                         inFormat are written, bytes in outFormat are read, in every mode above -- a G.711 RTP payload
   *                         stream to a model's floats: { inFormat: 'mulaw', outFormat: 'f32le-normalized' }.  Without
   *                         either the Transform is the reference's and calls what it always called.
   *   meter: true         -- the output meter (SpeexResampler.setMeter) on from the first chunk; the `meter` getter reads the
   *                         totals.  The stream then runs through the formatted calls (default 's16le' each side): only
   *                         they are metered.
   *   gain: g | { gain, rampFrames }
   *                       -- the output gain (SpeexResampler.setGain) from the first chunk on; setGain(gain, rampFrames) on
   *                         the Transform changes it in mid-stream, from the next chunk's first output frame.  The stream
   *                         then runs through the formatted calls (default 's16le' each side): only they are gained.
   */
  constructor(channels, inRate, outRate, quality = 7, options = undefined) {
    super();
    this.channels = channels;
    this.inRate = inRate;
    this.outRate = outRate;
    this.quality = quality;
    this.resampler = new SpeexResampler(channels, inRate, outRate, quality);
    this._alignementBuffer = EMPTY_BUFFER;
    this._options = options || {};
    this._held = [];
    // the stream's formats, or null: the reference's s16le through the calls it has always made
    this._formats = null;
    if (this._options.inFormat !== undefined || this._options.outFormat !== undefined) {
      const names = [this._options.inFormat || 's16le', this._options.outFormat || 's16le'];
      for (const name of names) if (!SAMPLE_FORMATS[name]) throw new Error('Unknown sample format: ' + name);
      this._formats = names;
    }
    if (this._options.meter) {
      if (!this._formats) this._formats = ['s16le', 's16le'];
      this._meterPending = true;  // (switched on with the first call: the constructor works before initPromise)
    }
    if (this._options.gain !== undefined) {
      const g = typeof this._options.gain === 'number' ? { gain: this._options.gain } : (this._options.gain || {});
      checkGain(g.gain, g.rampFrames || 0);
      if (!this._formats) this._formats = ['s16le', 's16le'];
      this._gainPending = [g.gain, g.rampFrames || 0];  // (set with the first call: the constructor works before initPromise)
    }
    if (this._options.pipeline) {
      this._busy = false;       // a processChunksAsync call is in flight
      this._waiting = null;     // the end of the stream, parked until the pipeline has drained
      this._parked = null;      // a _transform callback parked while maxHeld chunks are held
      this._flush = (callback) => {
        const finish = () => {
          try {
            if (this._options.flushTail) this.push(this._tail());
            callback();
          } catch (e) {
            callback(e);
          }
        };
        if (!this._busy && this._held.length === 0) finish();
        else this._waiting = finish;
        this._pump();
      };
    } else if (this._options.coalesceChunks > 1 || this._options.flushTail) {
      // only defined when asked for: the reference has no _flush
      this._flush = (callback) => {
        try {
          this._emitHeld();
          if (this._options.flushTail) this.push(this._tail());
          callback();
        } catch (e) {
          callback(e);
        }
      };
    }
  }

  /** the stream's totals so far (SpeexResampler.getMeter) */
  get meter() {
    this._armMeter();
    return this.resampler.getMeter();
  }

  _armMeter() {
    if (this._meterPending) {
      this._meterPending = false;
      this.resampler.setMeter(true);
    }
  }

  // the gain asked for -- by the option or by setGain -- takes hold with the next call, between two calls of the stream
  _armGain() {
    if (this._gainPending && !(this.resampler._inFlight > 0)) {
      const [gain, rampFrames] = this._gainPending;
      this._gainPending = null;
      this.resampler.setGain(gain, rampFrames);
    }
  }

  // what the options and setGain asked for, in force before the stream's next call
  _arm() {
    this._armMeter();
    this._armGain();
  }

  /**
   * The stream's output gain from the next chunk's first output frame on (SpeexResampler.setGain).  A Transform that named
   * no formats and no `gain` option runs the reference's int16 calls, which are never gained: it throws.
   */
  setGain(gain, rampFrames = 0) {
    checkGain(gain, rampFrames);
    if (!this._formats) throw new Error('setGain needs a Transform of the formatted calls: name inFormat / outFormat or the gain option');
    this._gainPending = [gain, rampFrames];
  }

  /** { current, target, remaining } of the stream (a gain asked for and not yet in force is not shown) */
  getGain() { return this.resampler.getGain(); }

  // pipeline: send what is held as one asynchronous call; when it returns, push its results in order and go again
  _pump() {
    if (this._busy || this._held.length === 0) return;
    const batch = this._held;
    this._held = [];
    this._busy = true;
    if (this._parked) {  // room again: the producer may go on
      const cb = this._parked;
      this._parked = null;
      cb();
    }
    this._manyAsync(batch).then((outs) => {
      for (const out of outs) this.push(out);
      for (const h of batch) this._recycle(h);
      this._busy = false;
      if (this._held.length > 0) {
        this._pump();
      } else if (this._waiting) {
        const w = this._waiting;
        this._waiting = null;
        w();
      }
    }, (e) => {
      this._busy = false;
      this._waiting = null;
      this._parked = null;
      this.destroy(e);
    });
  }

  // The calls of every mode: the stream's formats where it names them, else the reference's s16le calls as ever.
  _one(chunk) {
    this._arm();
    return this._formats ? this.resampler.processChunkFormat(chunk, this._formats[0], this._formats[1]) : this.resampler.processChunk(chunk);
  }

  _oneAsync(chunk) {
    this._arm();
    return this._formats ? this.resampler.processChunkFormatAsync(chunk, this._formats[0], this._formats[1])
      : this.resampler.processChunkAsync(chunk);
  }

  _many(chunks) {
    this._arm();
    return this._formats ? this.resampler.processChunksFormat(chunks, this._formats[0], this._formats[1])
      : this.resampler.processChunks(chunks);
  }

  _manyAsync(chunks) {
    this._arm();
    return this._formats ? this.resampler.processChunksFormatAsync(chunks, this._formats[0], this._formats[1])
      : this.resampler.processChunksAsync(chunks);
  }

  _tail() {
    this._arm();
    return this._formats ? this.resampler.flushFormat(this._formats[1]) : this.resampler.flush();
  }

  // pinned: a copy of `chunk` in a pinned chunk of the library (a plain copy when none is to be had).  Chunks come from a
  // small free list by size class; one is free again once the call that read it has returned -- _recycle().
  _pinnedCopy(chunk) {
    if (chunk.length === 0) return chunk;
    if (!this._ring) this._ring = new Map();
    let cls = 4096;
    while (cls < chunk.length) cls *= 2;
    const free = this._ring.get(cls);
    const slab = free && free.length > 0 ? free.pop() : SpeexResampler.allocChunk(cls);
    chunk.copy(slab, 0, 0, chunk.length);
    const view = slab.slice(0, chunk.length);
    view._slab = slab;
    view._cls = cls;
    return view;
  }

  _recycle(view) {
    if (!view || !view._slab || !this._ring) return;
    let free = this._ring.get(view._cls);
    if (!free) this._ring.set(view._cls, free = []);
    if (free.length < 8) free.push(view._slab);
  }

  // the copy a held chunk needs anyway (it must not change under us while it waits for its call)
  _own(chunk) { return this._options.pinned ? this._pinnedCopy(chunk) : Buffer.from(chunk); }

  _emitHeld() {
    if (this._held.length === 0) return;
    const held = this._held;
    this._held = [];
    for (const out of this._many(held)) this.push(out);
    for (const h of held) this._recycle(h);
  }

  _transform(chunk, encoding, callback) {
    if (this._options.pipeline) {
      try {
        // (a copy: the held chunk must not change under us while it waits for its call)
        this._held.push(this._own(this._align(chunk)));
      } catch (e) {
        callback(e);
        return;
      }
      this._pump();
      // accept the next chunk at once -- unless so much is held already that the producer should wait for the GPU
      if (this._held.length < (this._options.maxHeld || 256)) callback();
      else this._parked = callback;
      return;
    }
    if (this._options.coalesceChunks > 1 || this._options.async) {
      return this._transformExtended(chunk, callback);
    }
    if (this._options.pinned) {  // the reference's one synchronous call per chunk, on a pinned copy of the chunk
      let out;
      try {
        const own = this._pinnedCopy(this._align(chunk));
        out = this._one(own);
        this._recycle(own);
      } catch (err) {
        callback(err);
        return;
      }
      callback(null, out);
      return;
    }
    return this._transformReference(chunk, encoding, callback);
  }

  /**
   * Whole frames of (carry ++ chunk); the 0 .. channels*2-1 bytes (channels x bytes(inFormat) - 1 with formats) that do not complete a frame
   * are carried to the next chunk in `_alignementBuffer` (the field name, typo included, is the
   * reference's: src/index.ts:148-154 keeps it on the instance).
   */
  _align(chunk) {
    const frameBytes = this.channels * (this._formats ? SAMPLE_FORMATS[this._formats[0]].bytes : Uint16Array.BYTES_PER_ELEMENT);
    const carry = this._alignementBuffer;
    const joined = carry.length > 0 ? Buffer.concat([carry, chunk]) : chunk;
    const whole = joined.length - (joined.length % frameBytes);
    // (a copy: the carried bytes must survive the caller reusing its chunk)
    this._alignementBuffer = whole === joined.length ? EMPTY_BUFFER : Buffer.from(joined.slice(whole));
    return whole === joined.length ? joined : joined.slice(0, whole);
  }

  _transformExtended(chunk, callback) {
    try {
      // copy: a held chunk must not change under us while it waits for its launch
      const aligned = this._own(this._align(chunk));
      if (this._options.coalesceChunks > 1) {
        this._held.push(aligned);
        if (this._held.length >= this._options.coalesceChunks) this._emitHeld();
        callback();
      } else {
        this._oneAsync(aligned).then((res) => {
          this._recycle(aligned);
          callback(null, res);
        }, callback);
      }
    } catch (e) {
      callback(e);
    }
  }

  // the reference's behaviour: one synchronous call per chunk, output pushed at once
  _transformReference(chunk, encoding, callback) {
    let out;
    try {
      out = this._one(this._align(chunk));
    } catch (err) {
      callback(err);
      return;
    }
    callback(null, out);
  }
}

exports.SpeexResamplerTransform = SpeexResamplerTransform;
exports.SpeexResamplerBatch = SpeexResamplerBatch;
exports.SpeexResamplerMixer = SpeexResamplerMixer;
exports.default = SpeexResampler;
