'use strict';
// Sample formats in the streaming paths: SpeexResamplerTransform with inFormat / outFormat in every mode (plain,
// coalesceChunks, async, pipeline, pinned, each with and without flushTail), processChunksFormat(Async),
// processChunkFormatAsync and flushFormat -- all against twin SpeexResampler instances fed the same frames through
// processChunkFormat, one call per chunk: every byte must be equal.  Needs an MI355X.
const mod = require('../index.js');
const SpeexResampler = mod.default;
const { SpeexResamplerTransform } = mod;

const assert = (c, m) => { if (!c) throw new Error(m); };
const BYTES = { 'mulaw': 1, 's24le': 3, 's16le': 2, 'f32le-normalized': 4, 'alaw': 1, 's16be': 2 };

// `bytes` bytes of a stream in `format`: any bytes for the integer and companded formats, floats in +-0.5 otherwise
function payload(format, bytes, seed) {
  const buf = Buffer.alloc(bytes);
  let s = seed >>> 0;
  const next = () => { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; return s; };
  if (format === 'f32le-normalized') {
    for (let i = 0; i + 4 <= bytes; i += 4) buf.writeFloatLE((next() >>> 8) / 16777216 - 0.5, i);
  } else {
    for (let i = 0; i < bytes; i++) buf[i] = next() >>> 24;
  }
  return buf;
}

// the stream cut at byte positions that are no multiples of a frame (nor of a sample)
function cut(stream, sizes) {
  const chunks = [];
  let at = 0;
  for (let i = 0; at < stream.length; i++) {
    const n = Math.min(sizes[i % sizes.length], stream.length - at);
    chunks.push(stream.slice(at, at + n));
    at += n;
  }
  return chunks;
}

// what the Transform's alignment hands to the resampler for these chunks: whole frames, the rest carried
function aligned(chunks, frameBytes) {
  const out = [];
  let carry = Buffer.alloc(0);
  for (const c of chunks) {
    const joined = Buffer.concat([carry, c]);
    const whole = joined.length - (joined.length % frameBytes);
    out.push(joined.slice(0, whole));
    carry = joined.slice(whole);
  }
  return out;
}

function through(transform, chunks) {
  return new Promise((resolve, reject) => {
    const outs = [];
    transform.on('data', (d) => outs.push(d));
    transform.on('end', () => resolve(Buffer.concat(outs)));
    transform.on('error', reject);
    for (const c of chunks) transform.write(c);
    transform.end();
  });
}

const MODES = [
  ['plain', {}],
  ['coalesceChunks', { coalesceChunks: 4 }],
  ['async', { async: true }],
  ['pipeline', { pipeline: true }],
  ['pinned', { pinned: true }],
  ['pinned + coalesceChunks', { pinned: true, coalesceChunks: 4 }],
  ['pinned + pipeline', { pinned: true, pipeline: true }],
];
const PAIRS = [
  { inFormat: 'mulaw', outFormat: 'f32le-normalized', args: [1, 8000, 16000, 7] },
  { inFormat: 's24le', outFormat: 's16le', args: [2, 44100, 48000, 7] },
  { inFormat: 'f32le-normalized', outFormat: 's16le', args: [2, 48000, 16000, 5] },
];
const SIZES = [1001, 4099, 7, 2500, 1, 3333, 640, 5003];

async function transforms() {
  for (const pair of PAIRS) {
    const frameBytes = pair.args[0] * BYTES[pair.inFormat];
    // (the stream ends inside a frame: the incomplete frame is never resampled, as in the reference)
    const stream = payload(pair.inFormat, 6000 * frameBytes, 77);
    const chunks = cut(Buffer.concat([stream, stream.slice(0, frameBytes - 1)]), SIZES);
    assert(frameBytes === 1 || chunks.some((c) => c.length % frameBytes !== 0), 'chunks are cut inside frames');
    // the twin: processChunkFormat chunk by chunk, then flushFormat
    const twin = new SpeexResampler(...pair.args);
    const parts = aligned(chunks, frameBytes).map((c) => twin.processChunkFormat(c, pair.inFormat, pair.outFormat));
    const body = Buffer.concat(parts);
    const tail = twin.flushFormat(pair.outFormat);
    twin.destroy();
    assert(body.length > 0 && tail.length > 0, 'the twin made a body and a tail');
    for (const [name, options] of MODES) {
      for (const flushTail of [false, true]) {
        const t = new SpeexResamplerTransform(...pair.args, Object.assign({ flushTail }, options, pair));
        const got = await through(t, chunks);
        const want = flushTail ? Buffer.concat([body, tail]) : body;
        assert(Buffer.compare(got, want) === 0,
          `${pair.inFormat} -> ${pair.outFormat}, ${name}, flushTail ${flushTail}: ${got.length} vs ${want.length} bytes`);
        t.resampler.destroy();
      }
    }
  }
}

async function chunkLists() {
  for (const pair of PAIRS) {
    const frameBytes = pair.args[0] * BYTES[pair.inFormat];
    const frames = [160, 0, 1, 4097, 33, 480, 5, 160, 2048, 160];
    const chunks = frames.map((f, i) => payload(pair.inFormat, f * frameBytes, 300 + i));
    const one = new SpeexResampler(...pair.args);
    const later = new SpeexResampler(...pair.args);
    const twin = new SpeexResampler(...pair.args);
    for (const r of [one, later, twin]) r.setDither('triangular', 12345n, 0xfffffff0n);
    for (let step = 0; step < 2; step++) {
      const want = chunks.map((c) => twin.processChunkFormat(c, pair.inFormat, pair.outFormat));
      const got = one.processChunksFormat(chunks, pair.inFormat, pair.outFormat);
      const gotLater = await later.processChunksFormatAsync(chunks, pair.inFormat, pair.outFormat);
      assert(got.length === chunks.length && gotLater.length === chunks.length, 'one Buffer per chunk');
      want.forEach((w, i) => {
        assert(Buffer.compare(got[i], w) === 0, `processChunksFormat ${pair.inFormat} step ${step} chunk ${i}: ${got[i].length} vs ${w.length}`);
        assert(Buffer.compare(gotLater[i], w) === 0, `processChunksFormatAsync ${pair.inFormat} step ${step} chunk ${i}`);
      });
    }
    assert(one.getDither().position === twin.getDither().position && later.getDither().position === twin.getDither().position,
      'dither positions');
    assert(Buffer.compare(one.flushFormat(pair.outFormat), twin.flushFormat(pair.outFormat)) === 0, 'flushFormat after the lists');
    for (const r of [one, later, twin]) r.destroy();
  }
  // an s16le tail is flush()'s
  const a = new SpeexResampler(2, 44100, 48000), b = new SpeexResampler(2, 44100, 48000);
  const pcm = payload('s16le', 4000, 5);
  a.processChunk(pcm);
  b.processChunk(pcm);
  assert(Buffer.compare(a.flushFormat('s16le'), b.flush()) === 0, "flushFormat('s16le') is flush()");
  let refused = false;
  try { a.processChunksFormat([pcm], 's16le', 'nope'); } catch (e) { refused = /Unknown sample format/.test(e.message); }
  assert(refused, 'an unknown format name is refused');
  a.destroy();
  b.destroy();
}

async function sameTick() {
  const n = 8;
  const names = ['mulaw', 'alaw', 's16be', 's16le'];
  const outs = ['f32le-normalized', 's16le', 'mulaw', 's16le'];
  const live = Array.from({ length: n }, () => new SpeexResampler(1, 8000, 16000));
  const twins = Array.from({ length: n }, () => new SpeexResampler(1, 8000, 16000));
  for (let step = 0; step < 3; step++) {
    const chunks = live.map((_, k) => payload(names[k % 4], [160, 4133, 480][step] * BYTES[names[k % 4]], 50 * step + k));
    // eight instances in one tick: one fused native call
    const pending = live.map((r, k) => r.processChunkFormatAsync(chunks[k], names[k % 4], outs[k % 4]));
    let refused = false;
    try { live[0].processChunkFormat(chunks[0], names[0], outs[0]); } catch (e) { refused = /pending/.test(e.message); }
    assert(refused, 'a synchronous call while a processChunkFormatAsync call is pending is refused');
    const got = await Promise.all(pending);
    got.forEach((g, k) => {
      const want = twins[k].processChunkFormat(chunks[k], names[k % 4], outs[k % 4]);
      assert(Buffer.compare(g, want) === 0, `same tick step ${step} instance ${k} (${names[k % 4]} -> ${outs[k % 4]})`);
    });
  }
  // a lone call takes the single-state path; two calls of one instance stay in order
  const c0 = payload('mulaw', 333, 1), c1 = payload('mulaw', 160, 2);
  const [g0, g1] = await Promise.all([live[0].processChunkFormatAsync(c0, 'mulaw', 'f32le-normalized'),
    live[0].processChunkFormatAsync(c1, 'mulaw', 'f32le-normalized')]);
  assert(Buffer.compare(g0, twins[0].processChunkFormat(c0, 'mulaw', 'f32le-normalized')) === 0, 'lone call 0');
  assert(Buffer.compare(g1, twins[0].processChunkFormat(c1, 'mulaw', 'f32le-normalized')) === 0, 'lone call 1');
  for (const r of live.concat(twins)) r.destroy();
}

// without the new options the Transform is what it was: the processChunk path, byte for byte
async function unchanged() {
  const args = [2, 44100, 48000, 7];
  const stream = payload('s16le', 6000 * 4 + 3, 9);
  const chunks = cut(stream, SIZES);
  const twin = new SpeexResampler(...args);
  const body = Buffer.concat(aligned(chunks, 4).map((c) => twin.processChunk(c)));
  const tail = twin.flush();
  twin.destroy();
  for (const [name, options] of MODES) {
    for (const flushTail of [false, true]) {
      const t = new SpeexResamplerTransform(...args, Object.assign({ flushTail }, options));
      assert(t._formats === null, 'no formats named');
      const got = await through(t, chunks);
      assert(Buffer.compare(got, flushTail ? Buffer.concat([body, tail]) : body) === 0, `s16le as ever, ${name}, flushTail ${flushTail}`);
      t.resampler.destroy();
    }
  }
  const plain = new SpeexResamplerTransform(...args);
  assert(plain._flush === undefined || plain._flush === SpeexResamplerTransform.prototype._flush, 'the reference has no _flush');
  let refused = false;
  try { new SpeexResamplerTransform(...args, { inFormat: 'nope' }); } catch (e) { refused = /Unknown sample format/.test(e.message); }
  assert(refused, 'an unknown format name is refused by the constructor');
}

async function main() {
  await SpeexResampler.initPromise;
  await transforms();
  await chunkLists();
  await sameTick();
  await unchanged();
  console.log('chunk formats: ok');
}

main().catch((e) => { console.error(e.stack || e); process.exit(1); });
