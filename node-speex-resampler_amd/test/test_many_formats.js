'use strict';
// SpeexResamplerBatch.processChunksFormat / processChunksFormatAsync against twin SpeexResampler instances fed the same
// payloads through processChunkFormat, one call each: every result Buffer must be byte-identical.  Needs an MI355X.
const mod = require('../index.js');
const SpeexResampler = mod.default;
const { SpeexResamplerBatch } = mod;

const assert = (c, m) => { if (!c) throw new Error(m); };
const BYTES = { 'mulaw': 1, 'alaw': 1, 's16be': 2, 's16le': 2, 'u8': 1, 's24le': 3 };

function payload(bytes, seed) {
  const buf = Buffer.alloc(bytes);
  let s = seed >>> 0;
  for (let i = 0; i < bytes; i++) {
    s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
    buf[i] = s >>> 24;
  }
  return buf;
}

async function main() {
  await SpeexResampler.initPromise;
  const n = 12;
  const names = ['mulaw', 'alaw', 's16be', 's16le', 'u8', 's24le'];
  const inFormat = Array.from({ length: n }, (_, k) => names[k % names.length]);
  const batch = new SpeexResamplerBatch(n, 1, 8000, 16000);
  const twins = Array.from({ length: n }, () => new SpeexResampler(1, 8000, 16000));
  const frames = [160, 160, 4133, 0, 12288];
  // synchronous steps: per-stream input formats, one output format; stream 5 sits a step out
  for (let step = 0; step < frames.length; step++) {
    const chunks = inFormat.map((f, k) => (step === 1 && k === 5 ? null : payload(frames[step] * BYTES[f], 100 * step + k)));
    const outs = batch.processChunksFormat(chunks, inFormat, 'f32le-normalized');
    for (let k = 0; k < n; k++) {
      if (chunks[k] === null) { assert(outs[k] === null, 'a stream that sat out has no result'); continue; }
      const want = twins[k].processChunkFormat(chunks[k], inFormat[k], 'f32le-normalized');
      assert(Buffer.compare(outs[k], want) === 0, `sync step ${step} stream ${k} (${inFormat[k]}): ${outs[k].length} vs ${want.length} bytes`);
    }
  }
  // per-stream output formats too, s16le -> s16le (the int16 call) among them
  const outFormat = Array.from({ length: n }, (_, k) => ['s16le', 'mulaw', 'f32le-normalized', 's24le'][k % 4]);
  for (let step = 0; step < 2; step++) {
    const chunks = inFormat.map((f, k) => payload(480 * BYTES[f], 7000 + 100 * step + k));
    const outs = batch.processChunksFormat(chunks, inFormat, outFormat);
    for (let k = 0; k < n; k++) {
      const want = twins[k].processChunkFormat(chunks[k], inFormat[k], outFormat[k]);
      assert(Buffer.compare(outs[k], want) === 0, `mixed outputs step ${step} stream ${k} (${inFormat[k]} -> ${outFormat[k]})`);
    }
  }
  // the asynchronous form, interleaved with processChunkAsync calls on the same streams: a stream's calls stay in order
  const pending = [];
  const expected = [];
  for (let step = 0; step < 3; step++) {
    const chunks = inFormat.map((f, k) => payload(160 * BYTES[f], 9000 + 100 * step + k));
    pending.push(batch.processChunksFormatAsync(chunks, inFormat, 'f32le-normalized'));
    expected.push(chunks.map((c, k) => twins[k].processChunkFormat(c, inFormat[k], 'f32le-normalized')));
    const pcm = payload(160 * 2, 9500 + step);
    for (const k of [0, 7]) {
      pending.push(batch.streams[k].processChunkAsync(pcm));
      expected.push(twins[k].processChunk(pcm));
    }
  }
  const settled = await Promise.all(pending);
  settled.forEach((got, i) => {
    if (Array.isArray(got)) {
      got.forEach((b, k) => assert(Buffer.compare(b, expected[i][k]) === 0, `async step ${i} stream ${k}`));
    } else {
      assert(Buffer.compare(got, expected[i]) === 0, `processChunkAsync between the steps, call ${i}`);
    }
  });
  batch.destroy();
  for (const t of twins) t.destroy();
  console.log('many formats: ok');
}

main().catch((e) => { console.error(e.stack || e); process.exit(1); });
