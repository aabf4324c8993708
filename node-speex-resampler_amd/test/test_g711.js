// 'mulaw' and 'alaw' in processChunkFormat / processChunkMix against processChunkFloat of a twin instance on the decoded
// samples: byte-equal results, call after call (decoding gives exact integers, encoding is the s16le rule followed by
// the G.711 compressor, the stream state is shared).  Needs an MI355X.
const mod = require('../index.js');
const SpeexResampler = mod.default || mod;

function assert(cond, what) {
  if (!cond) {
    console.error('FAILED: ' + what);
    process.exit(1);
  }
}

function lcg(n, seed) {
  const out = new Int16Array(n);
  let s = seed >>> 0;
  for (let i = 0; i < n; i++) {
    s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
    out[i] = ((s >>> 16) & 0xffff) - 32768;
  }
  return out;
}

const halfup = (v) => Math.floor(v + 0.5);
const clamp = (v, lo, hi) => Math.min(Math.max(v, lo), hi);
const bytesOf = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const floatsOf = (buf) => new Float32Array(buf.buffer, buf.byteOffset, buf.length / 4);
const s16Of = (y) => (Number.isNaN(y) ? 0 : clamp(halfup(y), -32768, 32767));
const log2Floor = (v) => 31 - Math.clz32(v);

// the codec as the header states it
const decode = {
  'mulaw': (b) => {
    const u = ~b & 0xff, e = (u >> 4) & 7, m = u & 15;
    const t = (((m << 3) + 0x84) << e) - 0x84;
    return (u & 0x80) ? -t : t;
  },
  'alaw': (b) => {
    const a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15;
    const t = e === 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (a & 0x80) ? t : -t;
  },
};
const encode = {
  'mulaw': (q) => {
    const s = q < 0 ? 1 : 0;
    const mag = Math.min(Math.abs(q), 32635) + 132;
    const e = log2Floor(mag) - 7;
    const m = (mag >> (e + 3)) & 15;
    return ~((s << 7) | (e << 4) | m) & 0xff;
  },
  'alaw': (q) => {
    const pos = q >= 0 ? 1 : 0;
    const mag = (pos ? q : -q - 1) >> 3;
    const e = mag < 32 ? 0 : log2Floor(mag) - 4;
    const m = e === 0 ? (mag >> 1) & 15 : (mag >> e) & 15;
    return ((pos << 7) | (e << 4) | m) ^ 0x55;
  },
};

// bytes that hold all 256 codes and then full-scale noise
function codes(n, seed) {
  const pcm = lcg(n, seed);
  return Uint8Array.from(pcm, (v, i) => (i < 256 ? i : (v >> 8) & 0xff));
}

async function main() {
  await SpeexResampler.initPromise;
  // the known answers
  const q = [0, -1, 1000, -1000, 32767, -32768];
  assert(q.map(encode['mulaw']).join() === [0xff, 0x7f, 0xce, 0x4e, 0x80, 0x00].join(), 'mu-law known answers');
  assert(q.map(encode['alaw']).join() === [0xd5, 0x55, 0xfa, 0x7a, 0xaa, 0x2a].join(), 'A-law known answers');

  const sizes = [160, 16384, 1, 17, 70000, 3000];
  let seed = 711;

  // telephony in, a speech model's float out: 8 kHz mono mu-law / A-law -> 16 kHz float32 in +-1.0
  for (const law of ['mulaw', 'alaw']) {
    const fmt = new SpeexResampler(1, 8000, 16000, 7);
    const twin = new SpeexResampler(1, 8000, 16000, 7);
    for (const frames of sizes) {
      const c = codes(frames, seed++);
      const got = fmt.processChunkFormat(bytesOf(c), law, 'f32le-normalized');
      const y = floatsOf(twin.processChunkFloat(bytesOf(Float32Array.from(c, decode[law]))));
      const want = Float32Array.from(y, (v) => v / 32768);
      assert(got.equals(bytesOf(want)), law + ' -> f32le-normalized, ' + frames + ' frames');
    }
  }

  // ... and back: s16le and the other law in, companded bytes out; both rails of both laws are reached
  const rails = { 'mulaw': [0x00, 0x80], 'alaw': [0x2a, 0xaa] };
  for (const [inFormat, outFormat] of [['s16le', 'mulaw'], ['s16le', 'alaw'], ['mulaw', 'alaw'], ['alaw', 'mulaw'],
    ['mulaw', 'mulaw']]) {
    const fmt = new SpeexResampler(2, 44100, 48000, 7);
    const twin = new SpeexResampler(2, 44100, 48000, 7);
    const seen = new Set();
    for (const frames of sizes) {
      let chunk, asFloat;
      if (inFormat === 's16le') {
        const pcm = lcg(frames * 2, seed++);
        chunk = bytesOf(pcm);
        asFloat = Float32Array.from(pcm);
      } else {
        const c = codes(frames * 2, seed++);
        chunk = bytesOf(c);
        asFloat = Float32Array.from(c, decode[inFormat]);
      }
      const got = fmt.processChunkFormat(chunk, inFormat, outFormat);
      const y = floatsOf(twin.processChunkFloat(bytesOf(asFloat)));
      const want = Uint8Array.from(y, (v) => encode[outFormat](s16Of(v)));
      for (const b of want) seen.add(b);
      assert(got.equals(bytesOf(want)), inFormat + ' -> ' + outFormat + ', ' + frames + ' frames');
    }
    if (inFormat === 's16le') {
      assert(seen.has(rails[outFormat][0]) && seen.has(rails[outFormat][1]), 'full-scale noise reaches the rails of ' + outFormat);
    }
  }

  // a mixed call: 48 kHz stereo s16le -> 8 kHz mono A-law, and 8 kHz mono mu-law -> 48 kHz stereo float
  {
    const down = new SpeexResampler(1, 48000, 8000, 7);
    const twin = new SpeexResampler(1, 48000, 8000, 7);
    for (const frames of sizes) {
      const pcm = lcg(frames * 2, seed++);
      const got = down.processChunkMix(bytesOf(pcm), 's16le', 'alaw', [[0.5, 0.5]], null);
      const mono = new Float32Array(frames);
      for (let i = 0; i < frames; i++) mono[i] = Math.fround(0.5 * pcm[2 * i] + 0.5 * pcm[2 * i + 1]);
      const y = floatsOf(twin.processChunkFloat(bytesOf(mono)));
      const want = Uint8Array.from(y, (v) => encode['alaw'](s16Of(v)));
      assert(got.equals(bytesOf(want)), 'stereo s16le -> mono alaw, ' + frames + ' frames');
    }
    const up = new SpeexResampler(1, 8000, 48000, 7);
    const twinUp = new SpeexResampler(1, 8000, 48000, 7);
    for (const frames of sizes) {
      const c = codes(frames, seed++);
      const got = up.processChunkMix(bytesOf(c), 'mulaw', 'f32le', null, [[1], [1]]);
      const y = floatsOf(twinUp.processChunkFloat(bytesOf(Float32Array.from(c, decode['mulaw']))));
      const want = new Float32Array(y.length * 2);
      for (let i = 0; i < y.length; i++) want[2 * i] = want[2 * i + 1] = y[i];
      assert(got.equals(bytesOf(want)), 'mono mulaw -> stereo f32le, ' + frames + ' frames');
    }
  }

  let threw = false;
  try {
    new SpeexResampler(1, 8000, 16000, 7).processChunkFormat(Buffer.alloc(12), 'ulaw', 's16le');
  } catch (e) {
    threw = /Unknown sample format/.test(e.message);
  }
  assert(threw, 'an unknown format throws');
  console.log('ALL G711 NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
