// processChunkMix against processChunkFloat of a twin instance of the resampler's channel count on the mixed samples:
// byte-equal results, call after call (the conversions and the mix are exact statements -- every product and sum of one
// output in double precision, in ascending order, one rounding to float32 -- and the stream state is the float call's).
// Needs an MI355X.
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

// frames of n = M[0].length float32 samples -> frames of M.length samples (a JS number is a double)
function mix(M, x) {
  const n = M[0].length;
  const rows = M.map((r) => r.map(Math.fround));
  const out = new Float32Array((x.length / n) * rows.length);
  for (let f = 0; f < x.length / n; f++) {
    for (let o = 0; o < rows.length; o++) {
      let acc = rows[o][0] * x[f * n];
      for (let i = 1; i < n; i++) acc = acc + rows[o][i] * x[f * n + i];
      out[f * rows.length + o] = acc;
    }
  }
  return out;
}

async function main() {
  await SpeexResampler.initPromise;
  const sizes = [480, 16384, 1, 160, 70000, 3000];
  let seed = 21;

  // 48 kHz stereo s16le -> 16 kHz mono float in +-1.0: the filter runs on ONE channel
  const toMono = [[0.5, 0.5]];
  let res = new SpeexResampler(1, 48000, 16000, 7);
  let twin = new SpeexResampler(1, 48000, 16000, 7);
  for (const frames of sizes) {
    const pcm = lcg(frames * 2, seed++);
    const got = res.processChunkMix(bytesOf(pcm), 's16le', 'f32le-normalized', toMono, null);
    const y = floatsOf(twin.processChunkFloat(bytesOf(mix(toMono, Float32Array.from(pcm)))));
    const want = Float32Array.from(y, (v) => v / 32768);
    assert(got.equals(bytesOf(want)), 'stereo s16le -> mono f32le-normalized, ' + frames + ' frames');
  }

  // mono up to stereo after the filter, s16le -> s16le: with a matrix the float call's rules hold
  const toStereo = [[1], [1]];
  res = new SpeexResampler(1, 16000, 48000, 7);
  twin = new SpeexResampler(1, 16000, 48000, 7);
  for (const frames of sizes) {
    const pcm = lcg(frames, seed++);
    const got = res.processChunkMix(bytesOf(pcm), 's16le', 's16le', null, toStereo);
    const y = mix(toStereo, floatsOf(twin.processChunkFloat(bytesOf(Float32Array.from(pcm)))));
    const want = Int16Array.from(y, (v) => clamp(halfup(v), -32768, 32767));
    assert(got.equals(bytesOf(want)), 'mono s16le -> stereo s16le, ' + frames + ' frames');
  }

  // 5.1 -> stereo at 48k -> 44.1k, float in, s32le out: saturation on the GPU
  const c = Math.SQRT1_2;
  const fold = [[1, 0, c, 0, c, 0], [0, 1, c, 0, 0, c]];
  res = new SpeexResampler(2, 48000, 44100, 5);
  twin = new SpeexResampler(2, 48000, 44100, 5);
  let rails = 0;
  for (const frames of sizes) {
    const f = Float32Array.from(lcg(frames * 6, seed++));
    const got = res.processChunkMix(bytesOf(f), 'f32le', 's32le', fold, null);
    const y = floatsOf(twin.processChunkFloat(bytesOf(mix(fold, f))));
    const want = Int32Array.from(y, (v) => clamp(halfup(v * 65536), -2147483648, 2147483647));
    for (const v of want) if (v === 2147483647 || v === -2147483648) rails++;
    assert(got.equals(bytesOf(want)), '5.1 f32le -> stereo s32le, ' + frames + ' frames');
  }
  assert(rails > 0, 'three full-scale channels summed reach the s32 rails');

  // both sides at once (6 -> 2 -> 2), and no mix at all is processChunkFormat
  const swap = [[0, 1], [1, 0]];
  res = new SpeexResampler(2, 44100, 48000, 7);
  twin = new SpeexResampler(2, 44100, 48000, 7);
  for (const frames of [480, 5000]) {
    const f = Float32Array.from(lcg(frames * 6, seed++), (v) => v / 3.0);
    const got = res.processChunkMix(bytesOf(f), 'f32le', 'f32le', fold, swap);
    const want = mix(swap, floatsOf(twin.processChunkFloat(bytesOf(mix(fold, f)))));
    assert(got.equals(bytesOf(want)), '6 -> 2 -> 2, ' + frames + ' frames');
    const pcm = lcg(frames * 2, seed++);
    const a = res.processChunkMix(bytesOf(pcm), 's16le', 'u8', null, null);
    assert(a.equals(twin.processChunkFormat(bytesOf(pcm), 's16le', 'u8')), 'no mix, ' + frames + ' frames');
  }

  const throws = (fn, re) => {
    try {
      fn();
    } catch (e) {
      return re.test(e.message);
    }
    return false;
  };
  assert(throws(() => res.processChunkMix(Buffer.alloc(12), 's16le', 's20le', fold, null), /Unknown sample format/),
    'an unknown format throws');
  assert(throws(() => res.processChunkMix(Buffer.alloc(14), 's16le', 'u8', fold, null), /multiple of channels \* 2 bytes/),
    'a chunk that is no whole number of frames throws');
  assert(throws(() => res.processChunkMix(Buffer.alloc(12), 's16le', 'u8', [[1, 0, 0]], null), /inMix should be 2 rows/),
    'an input mix with the wrong number of rows throws');
  assert(throws(() => res.processChunkMix(Buffer.alloc(12), 's16le', 'u8', null, [[1, 0, 0]]), /outMix should be rows of 2/),
    'an output mix with the wrong number of columns throws');
  assert(throws(() => res.processChunkMix(Buffer.alloc(36), 's16le', 'u8', [new Array(9).fill(1), new Array(9).fill(1)], null),
    /at most 8 x 8/), 'nine input channels throw');
  console.log('ALL MIX NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
