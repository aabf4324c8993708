// The output meter through the JS class (setMeter / getMeter), the batch and the Transform: the totals of a formatted
// stream equal the rule of the public header applied in JavaScript to the floats a twin instance produces ('f32le'), do
// not depend on the chunking, and stay zero while the meter is off.
const path = require('path');
const mod = require(path.join(__dirname, '../index.js'));
const SpeexResampler = mod.default;
const { SpeexResamplerTransform, SpeexResamplerBatch } = mod;

function assert(cond, msg) {
  if (!cond) throw new Error('ASSERT: ' + msg);
}

// noise at 1.3 x full scale as 'f32le' (int16 units), one NaN early in the stream
function noise(frames, channels, seed) {
  const f = new Float32Array(frames * channels);
  let s = seed >>> 0;
  for (let i = 0; i < f.length; i++) {
    s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
    f[i] = (s / 4294967296 * 2.6 - 1.3) * 32767;
  }
  f[Math.floor(f.length / 8)] = NaN;
  return Buffer.from(f.buffer);
}

// the rule for 's16le': r = floor(y + 0.5) against the rails, NaN apart, peak = max |y|
function model(floats) {
  const want = { samples: BigInt(floats.length), clippedHigh: 0n, clippedLow: 0n, nan: 0n, peak: 0 };
  for (const y of floats) {
    if (Number.isNaN(y)) { want.nan++; continue; }
    want.peak = Math.max(want.peak, Math.abs(y));
    const r = Math.floor(y + 0.5);
    if (r > 32767) want.clippedHigh++;
    if (r < -32768) want.clippedLow++;
  }
  return want;
}

function same(got, want, what) {
  for (const k of ['samples', 'clippedHigh', 'clippedLow', 'nan', 'peak']) {
    assert(got[k] === want[k], `${what}: ${k} ${got[k]} != ${want[k]}`);
  }
}

function floatsOf(buf) {
  return new Float32Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length));
}

async function meterTest() {
  const ch = 2, frames = 3000;
  const pcm = noise(frames, ch, 7);
  const twin = new SpeexResampler(ch, 44100, 48000, 7);
  const want = model(floatsOf(twin.processChunkFormat(pcm, 'f32le', 'f32le')));
  assert(want.clippedHigh > 0n && want.clippedLow > 0n && want.nan > 0n, 'the input does not clip both rails');

  // one call; off by default, zero while off
  const r = new SpeexResampler(ch, 44100, 48000, 7);
  const off = r.getMeter();
  assert(off.on === false && off.samples === 0n && off.peak === 0, 'a fresh instance reports totals');
  r.setMeter(true);
  const plain = new SpeexResampler(ch, 44100, 48000, 7);
  const a = r.processChunkFormat(pcm, 'f32le', 's16le'), b = plain.processChunkFormat(pcm, 'f32le', 's16le');
  assert(a.equals(b), 'the meter changed the bytes');
  const got = r.getMeter();
  assert(got.on === true && typeof got.samples === 'bigint' && typeof got.peak === 'number', 'the shape of getMeter()');
  same(got, want, 'one call');
  same(plain.getMeter(), { samples: 0n, clippedHigh: 0n, clippedLow: 0n, nan: 0n, peak: 0 }, 'meter off');

  // ragged chunks against a twin fed the same chunks (the wrapper's capacity rule is per chunk), then a reset
  const parts = new SpeexResampler(ch, 44100, 48000, 7), twin2 = new SpeexResampler(ch, 44100, 48000, 7);
  parts.setMeter(true);
  const fb = ch * 4;
  let at = 0;
  const seen = [];
  for (const n of [1, 159, 160, 1000, 777, frames - 2097]) {
    const piece = pcm.subarray(at * fb, (at + n) * fb);
    parts.processChunkFormat(piece, 'f32le', 's16le');
    seen.push(...floatsOf(twin2.processChunkFormat(piece, 'f32le', 'f32le')));
    at += n;
  }
  same(parts.getMeter({ reset: true }), model(seen), 'six chunks');
  twin2.destroy();
  same(parts.getMeter(), { samples: 0n, clippedHigh: 0n, clippedLow: 0n, nan: 0n, peak: 0 }, 'after a reset');
  assert(parts.getMeter().on === true, 'a reset left the switch alone');

  // the batch: per stream
  const batch = new SpeexResamplerBatch(2, ch, 44100, 48000, 7);
  batch.setMeter(true);
  batch.streams[1].processChunkFormat(pcm, 'f32le', 's16le');
  same(batch.getMeter(1), want, 'batch stream 1');
  assert(batch.getMeter(0).samples === 0n && batch.getMeter().on === true, 'batch stream 0 counted');
  batch.destroy();

  // the Transform: option and getter
  const t = new SpeexResamplerTransform(ch, 44100, 48000, 7, { meter: true, inFormat: 'f32le', outFormat: 's16le' });
  const done = new Promise((res, rej) => { t.on('end', res); t.on('error', rej); });
  t.on('data', () => {});
  t.write(pcm.subarray(0, 1000 * fb));
  t.end(pcm.subarray(1000 * fb));
  await done;
  const twin3 = new SpeexResampler(ch, 44100, 48000, 7);
  const both = [...floatsOf(twin3.processChunkFormat(pcm.subarray(0, 1000 * fb), 'f32le', 'f32le')),
    ...floatsOf(twin3.processChunkFormat(pcm.subarray(1000 * fb), 'f32le', 'f32le'))];
  same(t.meter, model(both), 'the Transform');
  twin3.destroy();
  for (const x of [twin, r, plain, parts]) x.destroy();
  console.log('meter: one call, six chunks, a batch stream and a Transform give the model\'s totals');
}

(async () => {
  await SpeexResampler.initPromise;
  await meterTest();
  console.log('ALL NODE METER TESTS PASSED');
})().catch((e) => { console.error(e); process.exit(1); });
