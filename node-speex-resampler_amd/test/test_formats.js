// processChunkFormat against processChunk / processChunkFloat of a twin instance on the converted samples: byte-equal
// results, call after call (the conversions are exact, the stream state is shared).  Needs an MI355X.
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

async function main() {
  await SpeexResampler.initPromise;
  const channels = 2;
  const sizes = [480, 16384, 1, 160, 70000, 3000];

  // a decoder's s16le in, Web Audio's float32 out
  let fmt = new SpeexResampler(channels, 44100, 48000, 7);
  let twin = new SpeexResampler(channels, 44100, 48000, 7);
  let seed = 11;
  for (const frames of sizes) {
    const pcm = lcg(frames * channels, seed++);
    const got = fmt.processChunkFormat(bytesOf(pcm), 's16le', 'f32le-normalized');
    const y = floatsOf(twin.processChunkFloat(bytesOf(Float32Array.from(pcm))));
    const want = Float32Array.from(y, (v) => v / 32768);
    assert(got.equals(bytesOf(want)), 's16le -> f32le-normalized, ' + frames + ' frames');
  }

  // 24-bit in, 32-bit out: rounding half up and saturation on the GPU
  fmt = new SpeexResampler(channels, 44100, 48000, 7);
  twin = new SpeexResampler(channels, 44100, 48000, 7);
  let rails = 0;
  for (const frames of sizes) {
    const pcm = lcg(frames * channels, seed++);
    const packed = Buffer.alloc(pcm.length * 3);
    const asFloat = new Float32Array(pcm.length);
    for (let i = 0; i < pcm.length; i++) {
      const s24 = pcm[i] * 256 + (i % 251);  // 24 significant bits
      packed.writeIntLE(s24, 3 * i, 3);
      asFloat[i] = s24 / 256;
    }
    const got = fmt.processChunkFormat(packed, 's24le', 's32le');
    const y = floatsOf(twin.processChunkFloat(bytesOf(asFloat)));
    const want = Int32Array.from(y, (v) => clamp(halfup(v * 65536), -2147483648, 2147483647));
    for (const v of want) if (v === 2147483647 || v === -2147483648) rails++;
    assert(got.equals(bytesOf(want)), 's24le -> s32le, ' + frames + ' frames');
  }
  assert(rails > 0, 'full-scale noise reaches the s32 rails');

  // u8 out, f32le in; s16le -> s16le is processChunk
  fmt = new SpeexResampler(channels, 48000, 44100, 5);
  twin = new SpeexResampler(channels, 48000, 44100, 5);
  for (const frames of sizes) {
    const pcm = lcg(frames * channels, seed++);
    const f = Float32Array.from(pcm, (v) => v / 3.0);
    const got = fmt.processChunkFormat(bytesOf(f), 'f32le', 'u8');
    const y = floatsOf(twin.processChunkFloat(bytesOf(f)));
    const want = Uint8Array.from(y, (v) => clamp(halfup(v / 256) + 128, 0, 255));
    assert(got.equals(bytesOf(want)), 'f32le -> u8, ' + frames + ' frames');
    const same = fmt.processChunkFormat(bytesOf(pcm), 's16le', 's16le');
    assert(same.equals(twin.processChunk(bytesOf(pcm))), 's16le -> s16le, ' + frames + ' frames');
  }

  let threw = false;
  try {
    fmt.processChunkFormat(Buffer.alloc(12), 's16le', 's20le');
  } catch (e) {
    threw = /Unknown sample format/.test(e.message);
  }
  assert(threw, 'an unknown format throws');
  threw = false;
  try {
    fmt.processChunkFormat(Buffer.alloc(7), 's24le', 'u8');
  } catch (e) {
    threw = /multiple of channels \* 3 bytes/.test(e.message);
  }
  assert(threw, 'a chunk that is no whole number of frames throws');
  console.log('ALL FORMAT NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
