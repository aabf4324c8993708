/// <reference types="node" />
// Type declarations of the drop-in (hand-written).  The reference ships tsc output that types `channels`, `inRate` and
// `outRate` as `any` (app/index.d.ts:4-6, 23, 31-33, 44): so do the constructors and fields below -- a TypeScript caller
// that compiles against the reference (rates held as strings, say: they are coerced like the reference coerces them)
// compiles against the drop-in.
import { Transform, TransformCallback } from 'stream';

/**
 * Options of the streaming wrapper; all of them are extensions and default to off.  Without options the
 * Transform is the reference's, byte for byte, and it is also the FASTEST way through a pipe: measured on one
 * MI355X with the seven files of the reference's test (1.7 MB each, 64 KiB chunks, profiles/r02_node_bench.json),
 * the plain pipe takes 0.76-1.49 ms per file.  The options below buy something else than throughput.
 */
/**
 * sample formats of processChunkFormat: 's24le' is packed (3 bytes per sample), 'f32le' is float32 in int16 units (what
 * processChunkFloat takes), 'f32le-normalized' float32 with +-1.0 full scale (Web Audio), 'mulaw' / 'alaw' G.711 as RTP
 * carries it (PCMU / PCMA, one byte per sample; a companded result is the 's16le' result through the G.711 compressor),
 * 's16be' / 's24be' / 's32be' the same samples in network and file byte order (RTP L16 / L24, AIFF), 'f16le-normalized' /
 * 'bf16le-normalized' IEEE binary16 / bfloat16 with +-1.0 full scale (round to nearest even)
 */
export type SampleFormat = 'u8' | 's16le' | 's24le' | 's32le' | 'f32le' | 'f32le-normalized' | 'mulaw' | 'alaw' |
    's16be' | 's24be' | 's32be' | 'f16le-normalized' | 'bf16le-normalized';
/** dither of the integer results of processChunkFormat / processChunkMix (setDither) */
export type DitherKind = 'none' | 'rectangular' | 'triangular';
/** what getMeter reports: samples judged, samples clipped at either rail, NaN samples, the largest |value| in int16 units */
export interface MeterTotals { on: boolean, samples: bigint, clippedHigh: bigint, clippedLow: bigint, nan: bigint, peak: number }
/** what getGain reports: the next output frame's gain, the ramp's target, its output frames still to come */
export interface GainState { current: number, target: number, remaining: number }

export interface SpeexResamplerTransformOptions {
    /**
     * Hold up to n chunks and resample them in one GPU launch (same bytes out).  Trades LATENCY -- the first
     * output waits for n chunks -- for fewer launches: 20-55 % less time per file at n = 8 on five of the seven test
     * tuples (round 5: the held run stays on pinned memory), a loss on mono 24k -> 48k and stereo 24k -> 48k q10.
     */
    coalesceChunks?: number;
    /**
     * Run each call off the event loop (N-API async work).  Trades THROUGHPUT for an event loop that stays
     * free while the GPU works: a file takes 1.5-2.2x as long as through the plain pipe (two thread hand-overs
     * per 64 KiB chunk cost more than the 25-50 us call they wrap).  For servers that must not block; not a
     * way to go faster.
     */
    async?: boolean;
    /** at end of stream also emit the filter's tail */
    flushTail?: boolean;
    /**
     * Off the event loop AND batched by load: a chunk that arrives while a call is in flight is held, and everything
     * held leaves as ONE call when that one returns -- an idle stream sends each chunk at once, a busy one a few large
     * launches.  Same bytes out.  What `async` is for -- an event loop that stays free -- at about the plain pipe's
     * speed instead of 1.5-4x its time (profiles/r05_node_bench.json: 0.63-0.90 ms per 1.7 MB file, plain pipe
     * 0.47-1.08, `async` 0.83-3.6).  `maxHeld` (default 256) bounds what is held before the producer is made to wait.
     */
    pipeline?: boolean;
    maxHeld?: number;
    /**
     * Copy every chunk ONCE into a pinned chunk of the library (a small ring of `SpeexResampler.allocChunk` Buffers,
     * reused) so that the GPU reads it in place.  With `coalesceChunks`, `async` or `pipeline` this is the copy those
     * modes make anyway, landing in pinned memory; in the plain mode it replaces the library's own copy into its bounce
     * buffer.  Same bytes out.  A producer that fills chunks from `allocChunk` itself needs no option.
     */
    pinned?: boolean;
    /**
     * The stream's sample formats (default 's16le' each): bytes of inFormat are written, bytes of outFormat are read, in
     * every mode -- plain, `coalesceChunks`, `async`, `pipeline`, `pinned`, `flushTail`.  Chunks may be cut anywhere: the
     * bytes that do not complete a frame of channels x bytes(inFormat) are carried to the next chunk.  Without either
     * option the Transform is the reference's and calls what it always called.
     */
    inFormat?: SampleFormat;
    outFormat?: SampleFormat;
    /**
     * The output meter on from the first chunk (SpeexResampler.setMeter); read the totals from the Transform's `meter`.
     * The stream then runs through the formatted calls (default 's16le' each side), which alone are metered.
     */
    meter?: boolean;
    /**
     * The output gain from the first chunk on (SpeexResampler.setGain): a number, or a gain reached over rampFrames output
     * frames.  The stream then runs through the formatted calls (default 's16le' each side), which alone are gained.
     */
    gain?: number | { gain: number, rampFrames?: number };
}

/**
 * Speex resampler whose filter runs on an MI355X.  Constructor, `processChunk`, `initPromise`
 * and the instance fields are the reference's public surface; the rest are extensions.
 */
declare class SpeexResampler {
    /** resolves once the native module is loaded; `processChunk` throws before that */
    static initPromise: Promise<unknown>;

    channels: any;
    inRate: any;
    outRate: any;
    /** Speex quality, 0..10 */
    quality: number;
    /** native state handle, created by the first call */
    _resamplerPtr: unknown;
    /** grow-only byte size that caps the frames one call may return */
    _outBufferSize: number;

    /**
     * The reference's four arguments.  `options.device` (extension) pins the instance to one GPU; without it the
     * library places it when its native state is made: the process's current GPU, or -- environment
     * SPEEXHIP_DEVICES=all -- instance number k of the process on GPU k mod the GPU count (SPEEXHIP_DEVICE=k: all on k).
     */
    constructor(channels: any, inRate: any, outRate: any, quality?: number, options?: { device?: number });

    /** GPU the instance lives on (-1 until the first call made its native state) */
    readonly device: number;
    /** GPUs the library can place instances on */
    static deviceCount(): number;
    /**
     * Extension: a Buffer over a PINNED block of the native library for the caller to fill (read a file or a socket into
     * it, let a decoder write it) and pass to any processChunk* method or to SpeexResamplerBatch: the GPU reads the chunk
     * where it lies, through PCIe, while it writes the result -- no staging copy (the reference copies every chunk into
     * the WASM heap).  Same result bytes as for an ordinary Buffer; an ordinary Buffer comes back when no block is free.
     * Refill it once the call that read it has returned (or its promise has settled).
     */
    static allocChunk(bytes: number): Buffer;

    /**
     * interleaved s16le PCM in, resampled s16le PCM out: a fresh Buffer the caller owns, like the reference's.
     * Results of 4 KB and more are external Buffers over pinned memory of the native library (no copy on the way
     * out; the memory returns to the library when the Buffer is collected); an application that keeps more than
     * 64 MiB of them alive (SPEEXHIP_TAKE_MB) gets ordinary copies beyond that.  SPEEXHIP_NAPI_COPY=1: copies always.
     */
    processChunk(chunk: Buffer): Buffer;

    /** consecutive chunks in one GPU launch; result[i] equals processChunk(chunks[i]) */
    processChunks(chunks: Buffer[]): Buffer[];
    /** the same off the event loop */
    processChunksAsync(chunks: Buffer[]): Promise<Buffer[]>;
    /**
     * processChunk off the event loop; calls on one instance stay in order.  Calls of DIFFERENT instances that become
     * ready in the same tick leave as one native call: one transfer in, one GPU launch per <= 32 instances of equal
     * (channels, rates, quality) and GPU, one transfer out (a server's connections, each with a small chunk per tick).  While one is pending the
     * synchronous methods of the same instance (processChunk, processChunks, processChunkFloat, setRate,
     * setQuality, skipZeros, resetMem, flush, destroy) throw: await the promise first.
     */
    processChunkAsync(chunk: Buffer): Promise<Buffer>;
    /** interleaved float32 PCM in and out (speex_resampler_process_interleaved_float) */
    processChunkFloat(chunk: Buffer): Buffer;

    /**
     * planar PCM: one Int16Array or one Float32Array per channel (all of one kind and length) in, typed arrays of the
     * same kind out; same state, capacity rule and samples as processChunk / processChunkFloat on the interleaved frames
     */
    processChunkPlanar(channels: Int16Array[]): Int16Array[];
    processChunkPlanar(channels: Float32Array[]): Float32Array[];

    /**
     * interleaved PCM of one sample format in, another out (SampleFormat); the conversions run on the GPU: it is
     * processChunkFloat on the converted samples, then rounding half up and saturating into an integer outFormat
     */
    processChunkFormat(chunk: Buffer, inFormat: SampleFormat, outFormat: SampleFormat): Buffer;

    /**
     * consecutive chunks of inFormat as one transfer each way, one conversion pass per side and (normally) one
     * resampling launch; result[i] equals processChunkFormat(chunks[i], inFormat, outFormat), dither running on across
     * the chunks
     */
    processChunksFormat(chunks: Buffer[], inFormat: SampleFormat, outFormat: SampleFormat): Buffer[];
    /** the same off the event loop */
    processChunksFormatAsync(chunks: Buffer[], inFormat: SampleFormat, outFormat: SampleFormat): Promise<Buffer[]>;
    /**
     * processChunkFormat off the event loop; calls on one instance stay in order, and calls of DIFFERENT instances that
     * become ready in the same tick leave as one fused native call whatever formats they name, as processChunkAsync's do
     */
    processChunkFormatAsync(chunk: Buffer, inFormat: SampleFormat, outFormat: SampleFormat): Promise<Buffer>;

    /**
     * processChunkFormat with a channel mix on either side, done on the GPU in the passes that convert the samples.  The
     * instance's `channels` is the count the resampler runs on.  inMix: `channels` rows, one column per channel of the
     * chunk, applied to every input frame before the filter; outMix: one row per channel of the result, `channels`
     * columns, applied to every frame the filter made; null = no mix on that side.  Up to 8 x 8.  Stereo to mono:
     * [[0.5, 0.5]] as inMix of a mono instance; mono to stereo: [[1], [1]] as outMix.  Each output is summed in double
     * precision in ascending order and rounded once to float32.
     */
    processChunkMix(chunk: Buffer, inFormat: SampleFormat, outFormat: SampleFormat, inMix: number[][] | null,
      outMix: number[][] | null): Buffer;

    /**
     * processChunkMix with a layout per side.  `input`: a Buffer of interleaved frames, or one typed array per input
     * channel (planar) holding the plane's bytes in inSide.format.  outSide.planar: the result is one typed array per
     * channel of the format's element type (Uint8Array for the 1-byte formats, 's24le' and the big-endian formats,
     * Uint16Array of the bits for the half-float ones, for which a Float16Array is accepted on input) instead of a Buffer.  The same
     * samples and stream state as processChunkMix on the frames interleaved; with a planar side every format pair runs
     * by processChunkFloat's capacity rule.  outSide.channels, when given, must be the result's channel count.
     */
    processChunkSides(input: Buffer | ArrayBufferView[], inSide: { format: SampleFormat, mix?: number[][] | null },
        outSide: { format: SampleFormat, planar?: boolean, channels?: number, mix?: number[][] | null }):
        Buffer | Array<Uint8Array | Int16Array | Int32Array | Float32Array | Uint16Array>;

    /** mid-stream control (speex_resampler_set_rate / set_quality / skip_zeros / reset_mem) */
    setRate(inRate: number, outRate: number): void;
    setQuality(quality: number): void;
    /**
     * 'fast_fixed' (the default: +-1 LSB of the reference, fp64 sums at quality 9 / 10, and bytes that -- like the
     * reference's -- do not depend on chunking, batch size or GPU), 'fast' (+-1 LSB; up to 2x faster on one-stream calls of
     * long decimators, but the last bit of a sample may depend on how the stream was cut into chunks), 'exact'
     * (bit-identical to the reference, slower) or 'fast_f32'.  SPEEXHIP_MODE in the environment sets the initial mode.
     */
    setMode(mode: 'fast' | 'exact' | 'fast_f32' | 'fast_fixed'): void;
    /**
     * Dither of the integer results of processChunkFormat / processChunkMix ('u8', 's16le', 's24le', 's32le', 's16be', 's24be',
     * 's32be', and 'mulaw' / 'alaw', where the noise joins the int16 value the compressor takes): 'none' (default, round half up),
     * 'rectangular' (+-0.5 LSB) or 'triangular' (TPDF, +-1 LSB).  Counter based: the noise of a sample depends on (seed,
     * its index in the stream) alone, so the bytes do not depend on the chunking.  position = index of the next output
     * frame.  While on, 's16le' -> 's16le' runs as processChunkFloat between the two conversions.
     */
    setDither(kind: DitherKind, seed?: bigint | number, position?: bigint | number): void;
    /** position: output frames made by processChunkFormat / processChunkMix since setDither, plus its position */
    getDither(): { kind: DitherKind, seed: bigint, position: bigint };
    /**
     * The output meter of processChunkFormat / processChunkMix / processChunkSides and their chunk-list, many-instance and
     * asynchronous forms: clip counts and peak level of what they encode.  Totals are kept while it is off; while it is on
     * 's16le' -> 's16le' runs as processChunkFloat between the two conversions.
     */
    setMeter(on: boolean): void;
    /** totals since the last reset; peak in int16 units (above 32768: beyond +-1.0).  reset: clear them behind the read */
    getMeter(options?: { reset?: boolean }): MeterTotals;
    /**
     * The output gain of processChunkFormat / processChunkMix / processChunkSides, their chunk-list, many-instance and
     * asynchronous forms and flushFormat: `gain` from the next output frame on, reached linearly over rampFrames output
     * frames (0: a step) from the gain that frame would have had.  Negative gains and 0 are legal; a gain that is not
     * finite throws.  While the gain is on 's16le' -> 's16le' runs as processChunkFloat between the two conversions.
     */
    setGain(gain: number, rampFrames?: number): void;
    getGain(): GainState;
    skipZeros(): void;
    resetMem(): void;
    /** filter delay in frames at the input rate / at the output rate */
    readonly inputLatency: number;
    readonly outputLatency: number;

    /** the filter's tail: the response to the last inputLatency frames */
    flush(): Buffer;
    /** the tail in outFormat, as processChunkFormat writes it */
    flushFormat(outFormat: SampleFormat): Buffer;
    /** release the GPU state now instead of at garbage collection */
    destroy(): void;
    /**
     * Extension: hand the idle device / pinned memory that destroyed states left in the process-wide
     * pool (kept for the next `new SpeexResampler`) back to the driver; returns the bytes released.
     */
    static releaseCachedMemory(): number;
}

/** `stream.Transform` around a SpeexResampler; misaligned trailing bytes wait for the next chunk. */
export declare class SpeexResamplerTransform extends Transform {
    channels: any;
    inRate: any;
    outRate: any;
    quality: number;
    resampler: SpeexResampler;
    _alignementBuffer: Buffer;
    /** the stream's totals so far (option `meter`) */
    readonly meter: MeterTotals;
    /** the stream's gain from the next chunk's first output frame on; needs the formatted calls (formats or the `gain` option) */
    setGain(gain: number, rampFrames?: number): void;
    getGain(): GainState;

    constructor(channels: any, inRate: any, outRate: any, quality?: number,
                options?: SpeexResamplerTransformOptions);
    _transform(chunk: Buffer, encoding: string, callback: TransformCallback): void;
}

/**
 * Extension: n independent streams of one (channels, rates, quality), each a SpeexResampler with its own capacity
 * rule, whose chunks of one step run together -- per GPU one transfer in, one launch per <= 32 streams, one transfer
 * out; with SPEEXHIP_DEVICES=all or `options.devices` the streams spread over the node's GPUs (stream k on the k-th
 * listed GPU modulo their number).  Entry k of a result equals `streams[k].processChunk(chunks[k])`.
 */
export declare class SpeexResamplerBatch {
    channels: any;
    inRate: any;
    outRate: any;
    quality: number;
    streams: SpeexResampler[];
    readonly length: number;
    constructor(nStreams: number, channels: any, inRate: any, outRate: any, quality?: number,
                options?: { devices?: number[] });
    /** one chunk per stream (null: the stream sits the step out) -> one fresh Buffer per stream (null likewise) */
    processChunks(chunks: Array<Buffer | null>): Array<Buffer | null>;
    processChunksAsync(chunks: Array<Buffer | null>): Promise<Array<Buffer | null>>;
    /**
     * processChunks with sample formats, all streams in one fused call: entry k equals
     * `streams[k].processChunkFormat(chunks[k], inFormat[k], outFormat[k])`.  A format is one name for all streams or an
     * array with one name per stream: a gateway's PCMU / PCMA / L16 legs as `['mulaw', 'alaw', 's16be', ...]`.
     */
    processChunksFormat(chunks: Array<Buffer | null>, inFormat: SampleFormat | SampleFormat[],
                        outFormat: SampleFormat | SampleFormat[]): Array<Buffer | null>;
    processChunksFormatAsync(chunks: Array<Buffer | null>, inFormat: SampleFormat | SampleFormat[],
                             outFormat: SampleFormat | SampleFormat[]): Promise<Array<Buffer | null>>;
    setMode(mode: 'fast' | 'exact' | 'fast_f32' | 'fast_fixed'): void;
    /** setDither of every stream; stream k draws from seed + k * 0x9E3779B97F4A7C15 (mod 2^64) */
    setDither(kind: DitherKind, seed?: bigint | number, position?: bigint | number): void;
    /** getDither of stream k (default 0) */
    getDither(stream?: number): { kind: DitherKind, seed: bigint, position: bigint };
    /** setMeter of every stream */
    setMeter(on: boolean): void;
    /** getMeter of stream k (default 0); reset clears that stream only */
    getMeter(stream?: number, options?: { reset?: boolean }): MeterTotals;
    /** setGain of stream k, or of every stream when none is named */
    setGain(gain: number, rampFrames?: number, stream?: number): void;
    /** getGain of stream k (default 0) */
    getGain(stream?: number): GainState;
    destroy(): void;
}

/**
 * Mix buses over many separate SpeexResampler instances in one library call per tick: nLegs slots, nBuses buses, one
 * channel count.  Bus j is the float64 sum, in ascending slot order and rounded once, of rows[j][i] times slot i's output
 * of the call (behind that leg's own setGain), encoded in outFormat with the mixer's dither and meter.
 */
export declare class SpeexResamplerMixer {
    nLegs: number;
    nBuses: number;
    channels: number;
    legs: Array<SpeexResampler | null>;
    constructor(nLegs: number, nBuses: number, channels: number, options?: { device?: number });
    /** the instance in slot i (of the mixer's channel count), or null: an empty slot */
    setLeg(i: number, resampler: SpeexResampler | null): void;
    /** rows[j][i]: the weight of slot i in bus j; null: off.  Zeroes the bus meters and the buses' dither position */
    setWeights(rows: number[][] | null): void;
    setDither(kind: DitherKind, seed?: bigint | number, position?: bigint | number): void;
    getDither(): { kind: DitherKind, seed: bigint, position: bigint };
    setMeter(on: boolean): void;
    getBusMeter(j: number, options?: { reset?: boolean }): MeterTotals;
    /** per-leg levels of every tick, measured on the device; off by default, a change clears the last tick's records */
    setLevels(on: boolean): void;
    /** the last tick's record of every slot, measured BEFORE the leg's gain; audioLevel is the RFC 6464 value (0 .. 127) */
    getLevels(): { samples: BigUint64Array, energy: BigUint64Array, nan: BigUint64Array, peak: Float32Array, audioLevel: Uint8Array };
    /**
     * One tick, synchronously: chunks[i] in inFormats[i] (one name for all slots or one per slot; null for an empty slot).
     * codes[i] !== 0: a leg the library refused -- its state untouched, silence in the sum.
     */
    process(chunks: Array<Buffer | null>, inFormats: SampleFormat | SampleFormat[], outFormat: SampleFormat):
        { buses: Buffer[], busFrames: number, produced: number[], codes: number[] };
    destroy(): void;
}

export default SpeexResampler;
