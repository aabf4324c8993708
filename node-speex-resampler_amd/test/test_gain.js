// The output gain through the JS class (setGain / getGain), the batch and the Transform (option and mid-stream setGain): the
// bytes of a gained 's16le' stream equal the rule of the public header applied in JavaScript to the floats an ungained
// twin instance produces ('f32le') -- g(k) in doubles as written, Math.fround, one float product, floor(v + 0.5), the rails,
// NaN as zero -- whatever the chunking.
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

function floatsOf(buf) {
  return new Float32Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length));
}

// the header's state (from, to, total, done) and its rule
class Gain {
  constructor() { this.from = 1; this.to = 1; this.total = 0; this.done = 0; }
  at(k) {
    if (k >= this.total) return this.to;
    const step = (this.to - this.from) / this.total;
    return Math.fround(this.from + k * step);
  }
  set(gain, ramp) { this.from = this.at(this.done); this.to = Math.fround(gain); this.total = ramp; this.done = 0; }
  // 's16le' bytes of the twin's floats (frames of ch samples), the ramp moved on
  encode(floats, ch) {
    const out = Buffer.alloc(floats.length * 2);
    const frames = floats.length / ch;
    for (let f = 0; f < frames; f++) {
      const g = this.at(this.done + f);
      for (let c = 0; c < ch; c++) {
        const y = Math.fround(floats[f * ch + c] * g);
        const r = Number.isNaN(y) ? 0 : Math.min(32767, Math.max(-32768, Math.floor(y + 0.5)));
        out.writeInt16LE(r, (f * ch + c) * 2);
      }
    }
    this.done = Math.min(this.total, this.done + frames);
    return out;
  }
}

async function gainTest() {
  const ch = 2, frames = 3000, fb = ch * 4;
  const pcm = noise(frames, ch, 11);
  const cuts = [1, 159, 1000, frames - 1160];

  // the class: a ramp that runs across ragged chunks, a new target in mid-ramp, then back to 1 and off
  const r = new SpeexResampler(ch, 44100, 48000, 7), twin = new SpeexResampler(ch, 44100, 48000, 7);
  const fresh = r.getGain();
  assert(fresh.current === 1 && fresh.target === 1 && fresh.remaining === 0, 'a fresh instance is not at unity');
  let threw = false;
  try { r.setGain(NaN); } catch (e) { threw = true; }
  assert(threw && r.getGain().target === 1, 'a NaN gain was taken');
  const m = new Gain();
  r.setGain(0.25, 2000);
  m.set(0.25, 2000);
  let at = 0;
  cuts.forEach((n, i) => {
    if (i === 3) { r.setGain(-0.5, 300); m.set(-0.5, 300); }
    const piece = pcm.subarray(at * fb, (at + n) * fb);
    at += n;
    const got = r.processChunkFormat(piece, 'f32le', 's16le');
    const want = m.encode(floatsOf(twin.processChunkFormat(piece, 'f32le', 'f32le')), ch);
    assert(got.equals(want), `chunk ${i}: the gained bytes differ from the rule`);
    const g = r.getGain();
    assert(g.current === m.at(m.done) && g.target === m.to && g.remaining === m.total - m.done, `chunk ${i}: getGain`);
  });
  assert(m.done === m.total && r.getGain().current === Math.fround(-0.5), 'the second ramp did not end');
  // the tail is a formatted call: gained
  const tail = r.flushFormat('s16le'), tailTwin = floatsOf(twin.flushFormat('f32le'));
  assert(tail.equals(m.encode(tailTwin, ch)), 'flushFormat did not apply the gain');

  // the batch: per stream
  const batch = new SpeexResamplerBatch(3, ch, 44100, 48000, 7);
  batch.setGain(0.5, 0, 1);
  batch.setGain(2.0, 500, 2);
  assert(batch.getGain(0).target === 1 && batch.getGain(1).target === 0.5 && batch.getGain(2).remaining === 500, 'batch getGain');
  const plain = new SpeexResampler(ch, 44100, 48000, 7), twinB = new SpeexResampler(ch, 44100, 48000, 7);
  const y = floatsOf(twinB.processChunkFormat(pcm, 'f32le', 'f32le'));
  const outs = batch.streams.map((s) => s.processChunkFormat(pcm, 'f32le', 's16le'));
  assert(outs[0].equals(plain.processChunkFormat(pcm, 'f32le', 's16le')), 'the unity stream of a batch changed');
  const m1 = new Gain(), m2 = new Gain();
  m1.set(0.5, 0);
  m2.set(2.0, 500);
  assert(outs[1].equals(m1.encode(y, ch)) && outs[2].equals(m2.encode(y, ch)), 'batch streams at their own gains');
  batch.setGain(1.0);
  assert(batch.getGain(1).target === 1 && batch.getGain(2).target === 1, 'batch setGain of every stream');
  batch.destroy();

  // the Transform: the option, and setGain between two writes
  const t = new SpeexResamplerTransform(ch, 44100, 48000, 7, { gain: { gain: 0.5, rampFrames: 700 }, inFormat: 'f32le', outFormat: 's16le' });
  const got = [];
  const done = new Promise((res, rej) => { t.on('end', res); t.on('error', rej); });
  t.on('data', (d) => got.push(d));
  const first = pcm.subarray(0, 1000 * fb), second = pcm.subarray(1000 * fb);
  await new Promise((res) => t.write(first, res));
  t.setGain(-1.0, 100);
  t.end(second);
  await done;
  const twinT = new SpeexResampler(ch, 44100, 48000, 7), mt = new Gain();
  mt.set(0.5, 700);
  const wantA = mt.encode(floatsOf(twinT.processChunkFormat(first, 'f32le', 'f32le')), ch);
  mt.set(-1.0, 100);
  const wantB = mt.encode(floatsOf(twinT.processChunkFormat(second, 'f32le', 'f32le')), ch);
  assert(Buffer.concat(got).equals(Buffer.concat([wantA, wantB])), 'the Transform: option and mid-stream setGain');
  assert(t.getGain().target === -1 && t.getGain().remaining === 0, 'the Transform: getGain');
  // a Transform of the reference's int16 calls has no gain to set
  const bare = new SpeexResamplerTransform(ch, 44100, 48000, 7);
  threw = false;
  try { bare.setGain(0.5); } catch (e) { threw = true; }
  assert(threw, 'setGain on a Transform of the int16 calls');
  // a bad ramp is refused where it is given, not later as a stream error
  for (const bad of [() => t.setGain(0.5, -1), () => t.setGain(0.5, 1.5),
    () => new SpeexResamplerTransform(ch, 44100, 48000, 7, { gain: { gain: 0.5, rampFrames: -3 } })]) {
    threw = false;
    try { bad(); } catch (e) { threw = true; }
    assert(threw, 'a bad rampFrames was taken');
  }
  for (const x of [r, twin, plain, twinB, twinT]) x.destroy();
  console.log('gain: ragged chunks with a re-target, flushFormat, batch streams and a Transform give the rule\'s bytes');
}

(async () => {
  await SpeexResampler.initPromise;
  await gainTest();
  console.log('ALL NODE GAIN TESTS PASSED');
})().catch((e) => { console.error(e); process.exit(1); });
