// SpeexResamplerMixer: 5 legs of mixed formats and rates, 5 buses, mix-minus, 'f32le' out, two ticks.  The expected buses
// are the public header's rule applied in JavaScript to the floats that TWIN instances produce through
// processChunkFormat(..., 'f32le'): a sum in doubles in ascending slot order -- the first term the product itself --
// rounded once with Math.fround, +0 behind a leg's end.  Bit for bit.  Every ratio makes 960 frames of a whole 20 ms tick,
// so the second tick is ragged -- the 44.1 kHz leg brings 10 ms -- and a leg ends before the bus does.  Then: gained legs,
// the bus meter, dithered s16le buses, argument errors, the refusal while a leg has an asynchronous call pending, an empty slot.
const path = require('path');
const mod = require(path.join(__dirname, '../index.js'));
const SpeexResampler = mod.default;
const { SpeexResamplerMixer } = mod;

function assert(cond, msg) {
  if (!cond) throw new Error('ASSERT: ' + msg);
}

// the legs: [inRate, quality, format, bytes per sample, frames of a 20 ms tick]
const KINDS = [[8000, 7, 'mulaw', 1, 160], [8000, 5, 'alaw', 1, 160], [16000, 7, 's16be', 2, 320], [44100, 7, 's16le', 2, 882],
  [48000, 3, 'f32le-normalized', 4, 960]];
const N = KINDS.length;

function payload(kind, seed, half = false) {
  const [, , fmt, bytes] = kind;
  const frames = half ? kind[4] / 2 : kind[4];
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

const mixMinus = (n) => Array.from({ length: n }, (_, j) => Array.from({ length: n }, (_, i) => (i === j ? 0 : 1)));

// the rule: bus j of the legs' floats ys (null: +0 throughout), each behind gains[i] (a float, or null: not multiplied)
function model(rows, ys, gains) {
  const frames = Math.max(...ys.map((y) => (y ? y.length : 0)));
  return rows.map((row) => {
    const z = new Float32Array(frames);
    for (let f = 0; f < frames; f++) {
      let acc = 0;
      for (let i = 0; i < ys.length; i++) {
        let y = ys[i] && f < ys[i].length ? ys[i][f] : 0;
        if (gains && gains[i] !== null && ys[i] && f < ys[i].length) y = Math.fround(y * gains[i]);
        const p = row[i] * y;          // (two float32 values: exact in a double)
        acc = i === 0 ? p : acc + p;
      }
      z[f] = Math.fround(acc);
    }
    return z;
  });
}

function sameBits(buf, want, what) {
  const got = floatsOf(buf);
  assert(got.length === want.length, what + ': ' + got.length + ' samples, model ' + want.length);
  const a = new Uint32Array(got.buffer), b = new Uint32Array(want.buffer);
  for (let i = 0; i < a.length; i++) assert(a[i] === b[i], what + ': sample ' + i + ' is ' + got[i] + ', model ' + want[i]);
}

SpeexResampler.initPromise.then(async () => {
  const make = () => KINDS.map(([rate, q]) => new SpeexResampler(1, rate, 48000, q));
  const legs = make(), twins = make();
  const rows = mixMinus(N);
  const mixer = new SpeexResamplerMixer(N, N, 1);
  legs.forEach((r, i) => mixer.setLeg(i, r));
  mixer.setWeights(rows);
  mixer.setMeter(true);
  const formats = KINDS.map((k) => k[2]);
  let metered = 0n;
  for (let tick = 0; tick < 2; tick++) {
    const chunks = KINDS.map((k, i) => payload(k, 1000 * tick + i, tick === 1 && i === 3));
    const ys = twins.map((t, i) => floatsOf(t.processChunkFormat(chunks[i], formats[i], 'f32le')));
    const r = mixer.process(chunks, formats, 'f32le');
    assert(r.codes.every((c) => c === 0), 'tick ' + tick + ': codes ' + r.codes);
    assert(r.produced.every((p, i) => p === ys[i].length), 'tick ' + tick + ': produced ' + r.produced);
    assert(r.busFrames === Math.max(...r.produced) && r.buses.length === N, 'tick ' + tick + ': busFrames');
    if (tick === 0) assert(r.produced.every((p) => p === 960), 'a whole tick is not 960 frames for every leg: ' + r.produced);
    if (tick === 1) assert(new Set(r.produced).size > 1 && Math.min(...r.produced) < r.busFrames, 'no leg ends before the bus: ' + r.produced);
    const want = model(rows, ys, null);
    r.buses.forEach((b, j) => sameBits(b, want[j], 'tick ' + tick + ' bus ' + j));
    metered += BigInt(r.busFrames);
  }
  const m0 = mixer.getBusMeter(0);
  assert(m0.on === true && m0.samples === metered && m0.peak > 0, 'bus meter: ' + m0.samples + ' of ' + metered);
  assert(mixer.getBusMeter(0, { reset: true }).samples === metered && mixer.getBusMeter(0).samples === 0n, 'reset');
  assert(mixer.getBusMeter(1).samples === metered, 'reset cleared another bus');
  assert(mixer.getDither().position === 0n, 'the bus position moved without dither');

  // a muted leg and a halved one
  legs[0].setGain(0);
  legs[3].setGain(0.5);
  {
    const chunks = KINDS.map((k, i) => payload(k, 5000 + i));
    const ys = twins.map((t, i) => floatsOf(t.processChunkFormat(chunks[i], formats[i], 'f32le')));
    const r = mixer.process(chunks, formats, 'f32le');
    assert(r.codes.every((c) => c === 0), 'gained tick: codes ' + r.codes);
    const want = model(rows, ys, [0, null, null, 0.5, null]);
    r.buses.forEach((b, j) => sameBits(b, want[j], 'gained bus ' + j));
  }
  // s16le buses with dither: the position moves by busFrames
  mixer.setDither('triangular', 77n, 10n);
  {
    const chunks = KINDS.map((k, i) => payload(k, 7000 + i));
    twins.forEach((t, i) => t.processChunkFormat(chunks[i], formats[i], 'f32le'));
    const r = mixer.process(chunks, formats, 's16le');
    assert(r.buses.every((b) => b.length === r.busFrames * 2), 's16le buses: lengths');
    assert(mixer.getDither().position === 10n + BigInt(r.busFrames), 'dither position');
  }
  // argument errors refuse the tick whole, before any leg moves: the twins sit these out, and the tick behind them
  // still equals the model on the twins' floats
  const chunks = KINDS.map((k, i) => payload(k, 9000 + i));
  const throws = (fn, what) => {
    let threw = false;
    try { fn(); } catch (e) { threw = true; }
    assert(threw, what + ' did not throw');
  };
  throws(() => mixer.process(chunks.slice(1), formats, 'f32le'), 'too few chunks');
  throws(() => mixer.process(chunks, formats, 'nope'), 'an unknown output format');
  throws(() => mixer.process(chunks, ['nope'].concat(formats.slice(1)), 'f32le'), 'an unknown input format');
  throws(() => mixer.process(chunks.map((c, i) => (i === 2 ? c.subarray(1) : c)), formats, 'f32le'), 'a ragged chunk');
  throws(() => mixer.setWeights([[1, 2]]), 'a short matrix');
  throws(() => mixer.setWeights(rows.map((r, j) => r.map((v, i) => (i === 1 && j === 1 ? NaN : v)))), 'a NaN weight');
  throws(() => mixer.setLeg(0, new SpeexResampler(2, 8000, 48000)), 'a stereo leg');
  // a leg with an asynchronous call pending: refused, like SpeexResamplerBatch.processChunksFormat
  const pending = legs[4].processChunkFormatAsync(chunks[4], formats[4], 'f32le');
  throws(() => mixer.process(chunks, formats, 'f32le'), 'a tick while a leg has an async call pending');
  await pending;
  twins[4].processChunkFormat(chunks[4], formats[4], 'f32le');
  // an empty slot is silence; weights off: the library's BAD_STATE
  mixer.setLeg(1, null);
  {
    const ys = twins.map((t, i) => (i === 1 ? null : floatsOf(t.processChunkFormat(chunks[i], formats[i], 'f32le'))));
    const r = mixer.process(chunks.map((c, i) => (i === 1 ? null : c)), formats, 'f32le');
    assert(r.codes.every((c) => c === 0) && r.produced[1] === 0, 'empty slot: ' + r.codes + ' / ' + r.produced);
    const want = model(rows, ys, [0, null, null, 0.5, null]);
    r.buses.forEach((b, j) => sameBits(b, want[j], 'empty-slot bus ' + j));
  }
  mixer.setWeights(null);
  throws(() => mixer.process(chunks.map((c, i) => (i === 1 ? null : c)), formats, 'f32le'), 'a tick with the weights off');
  mixer.destroy();
  legs.concat(twins).forEach((r) => r.destroy());
  console.log('mixer ok');
}).catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
