// SpeexResamplerMixer.setLevels / getLevels: 5 legs of mixed formats and rates, two ticks, one leg muted and one halved.
// The expected record of a leg is the public header's rule ("Mixer levels") applied in JavaScript to the floats that an
// UNGAINED twin instance produces through processChunkFormat(..., 'f32le'): samples, the exact integer energy of the steps
// floor(y + 0.5) held to [-32768, 32767] (BigInt), the NaN count, the largest |y|; audioLevel is RFC 6464's value of it.
// Equality throughout.  Then: a second tick overwrites the records, the switch clears them, off throws.
const path = require('path');
const mod = require(path.join(__dirname, '../index.js'));
const SpeexResampler = mod.default;
const { SpeexResamplerMixer } = mod;

function assert(cond, msg) {
  if (!cond) throw new Error('ASSERT: ' + msg);
}

const KINDS = [[8000, 7, 'mulaw', 1, 160], [8000, 5, 'alaw', 1, 160], [16000, 7, 's16be', 2, 320], [44100, 7, 's16le', 2, 882],
  [48000, 3, 'f32le-normalized', 4, 960]];
const N = KINDS.length;

function payload(kind, seed) {
  const [, , fmt, bytes, frames] = kind;
  let s = seed >>> 0;
  const next = () => { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; return s; };
  if (fmt === 'f32le-normalized') {
    const f = new Float32Array(frames);
    for (let i = 0; i < frames; i++) f[i] = (next() / 4294967296 - 0.5) * 0.8;
    return Buffer.from(f.buffer);
  }
  const b = Buffer.alloc(frames * bytes);
  for (let i = 0; i < b.length; i++) b[i] = next() >>> 24;
  return b;
}

function floatsOf(buf) {
  return new Float32Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length));
}

// the rule, on one leg's floats
function model(y) {
  let energy = 0n, nan = 0n, peak = 0;
  for (const v of y) {
    if (Number.isNaN(v)) { nan += 1n; continue; }
    peak = Math.max(peak, Math.abs(v));
    const q = Math.min(32767, Math.max(-32768, Math.floor(v + 0.5)));   // (a float32 plus 0.5 is exact in a double)
    energy += BigInt(q * q);
  }
  const e = Number(energy);
  const level = e === 0 || y.length === 0 ? 127 : Math.min(127, Math.max(0, Math.round(-10 * Math.log10(e / (y.length * 2 ** 30)))));
  return { samples: BigInt(y.length), energy, nan, peak: Math.fround(peak), audioLevel: level };
}

function same(levels, i, want, what) {
  const got = { samples: levels.samples[i], energy: levels.energy[i], nan: levels.nan[i], peak: levels.peak[i], audioLevel: levels.audioLevel[i] };
  for (const k of Object.keys(want)) assert(got[k] === want[k], what + ', slot ' + i + ': ' + k + ' is ' + got[k] + ', model ' + want[k]);
}

SpeexResampler.initPromise.then(async () => {
  const make = () => KINDS.map(([rate, q]) => new SpeexResampler(1, rate, 48000, q));
  const legs = make(), twins = make();
  const mixer = new SpeexResamplerMixer(N, 2, 1);
  legs.forEach((r, i) => mixer.setLeg(i, r));
  mixer.setWeights([new Array(N).fill(1), new Array(N).fill(0.5)]);
  const formats = KINDS.map((k) => k[2]);
  const throws = (fn, what) => {
    let threw = false;
    try { fn(); } catch (e) { threw = true; }
    assert(threw, what + ' did not throw');
  };
  throws(() => mixer.getLevels(), 'getLevels with the levels off');
  mixer.setLevels(true);
  {
    const l = mixer.getLevels();
    assert(l.samples instanceof BigUint64Array && l.energy instanceof BigUint64Array && l.nan instanceof BigUint64Array &&
      l.peak instanceof Float32Array && l.audioLevel instanceof Uint8Array, 'the types of getLevels');
    assert(l.samples.length === N && l.samples.every((v) => v === 0n) && l.audioLevel.every((v) => v === 127), 'zeros before any tick');
  }
  legs[0].setGain(0);          // a muted leg still reads as loud
  legs[3].setGain(0.5, 100);
  let first = null;
  for (let tick = 0; tick < 2; tick++) {
    const chunks = KINDS.map((k, i) => payload(k, 3000 * tick + i));
    const ys = twins.map((t, i) => floatsOf(t.processChunkFormat(chunks[i], formats[i], 'f32le')));
    const r = mixer.process(chunks, formats, 's16le');
    assert(r.codes.every((c) => c === 0), 'tick ' + tick + ': codes ' + r.codes);
    assert(r.produced.every((p, i) => p === ys[i].length), 'tick ' + tick + ': produced ' + r.produced);
    const l = mixer.getLevels();
    ys.forEach((y, i) => same(l, i, model(y), 'tick ' + tick));
    assert(l.energy[0] > 0n && l.audioLevel[0] < 127, 'the muted leg reads as silence');
    if (tick === 0) first = l;
    else assert(l.energy.some((v, i) => v !== first.energy[i]), 'the second tick did not overwrite the records');
  }
  // an empty slot: zeros
  mixer.setLeg(1, null);
  {
    const chunks = KINDS.map((k, i) => (i === 1 ? null : payload(k, 9000 + i)));
    const ys = twins.map((t, i) => (i === 1 ? new Float32Array(0) : floatsOf(t.processChunkFormat(chunks[i], formats[i], 'f32le'))));
    mixer.process(chunks, formats, 's16le');
    const l = mixer.getLevels();
    ys.forEach((y, i) => same(l, i, model(y), 'empty slot'));
    assert(l.samples[1] === 0n && l.audioLevel[1] === 127, 'the empty slot');
  }
  // the switch clears the records
  mixer.setLevels(false);
  throws(() => mixer.getLevels(), 'getLevels behind setLevels(false)');
  mixer.setLevels(true);
  assert(mixer.getLevels().samples.every((v) => v === 0n), 'the switch did not clear the records');
  mixer.destroy();
  legs.concat(twins).forEach((r) => r.destroy());
  console.log('mixer levels ok');
}).catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
