// processChunkSides against processChunkMix / processChunkPlanar of a twin instance on the same samples, transposed: a
// call with a planar side is the mixed call on the frames interleaved -- byte-equal results, call after call, one stream
// state.  Needs an MI355X.
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

const bytesOf = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const ELEMENT = { 1: Uint8Array, 2: Int16Array, 3: Uint8Array, 4: Float32Array };

// interleaved bytes (frames of `channels` samples of `bytes` bytes) -> one Uint8Array per channel, and back
function planesOf(buf, channels, bytes) {
  const frames = buf.length / channels / bytes;
  const planes = [];
  for (let c = 0; c < channels; c++) {
    const p = new Uint8Array(frames * bytes);
    for (let f = 0; f < frames; f++) {
      for (let b = 0; b < bytes; b++) p[f * bytes + b] = buf[(f * channels + c) * bytes + b];
    }
    planes.push(p);
  }
  return planes;
}
function framesOf(planes, bytes) {
  const channels = planes.length;
  const raw = planes.map((p) => new Uint8Array(p.buffer, p.byteOffset, p.byteLength));
  const frames = raw[0].length / bytes;
  const out = Buffer.alloc(frames * channels * bytes);
  for (let c = 0; c < channels; c++) {
    for (let f = 0; f < frames; f++) {
      for (let b = 0; b < bytes; b++) out[(f * channels + c) * bytes + b] = raw[c][f * bytes + b];
    }
  }
  return out;
}
// the planes as typed arrays of the format's element type
const typed = (planes, bytes) => planes.map((p) => new ELEMENT[bytes](p.buffer, p.byteOffset, p.byteLength / ELEMENT[bytes].BYTES_PER_ELEMENT));

async function main() {
  await SpeexResampler.initPromise;
  const sizes = [160, 1, 17, 1023, 1024, 1025, 2053, 70000, 3000];
  const identity = [[1, 0], [0, 1]];
  let seed = 4242;

  // every layout combination of a few format pairs, stereo 44.1k -> 48k
  const pairs = [['s16le', 2, 'f32le-normalized', 4], ['s16le', 2, 's16le', 2], ['f32le-normalized', 4, 's24le', 3],
    ['u8', 1, 'mulaw', 1], ['s16le', 2, 's32le', 4]];
  for (const [inFormat, bin, outFormat, bout] of pairs) {
    for (const [planarIn, planarOut] of [[true, true], [true, false], [false, true]]) {
      const r = new SpeexResampler(2, 44100, 48000, 7);
      const twin = new SpeexResampler(2, 44100, 48000, 7);
      for (const frames of sizes) {
        const what = inFormat + ' -> ' + outFormat + (planarIn ? ' planar' : ' interleaved') + ' in' +
          (planarOut ? ' planar' : ' interleaved') + ' out, ' + frames + ' frames';
        let chunk;
        if (inFormat === 'f32le-normalized') chunk = bytesOf(Float32Array.from(lcg(frames * 2, seed++), (v) => v / 32768));
        else if (inFormat === 'u8') chunk = bytesOf(Uint8Array.from(lcg(frames * 2, seed++), (v) => (v >> 8) + 128));
        else chunk = bytesOf(lcg(frames * 2, seed++));
        // (with a planar side s16le -> s16le runs by the float call's rules, as the mixed call does with a matrix)
        const want = twin.processChunkMix(chunk, inFormat, outFormat, inFormat === outFormat ? identity : null, null);
        const input = planarIn ? typed(planesOf(chunk, 2, bin), bin) : chunk;
        const got = r.processChunkSides(input, { format: inFormat }, { format: outFormat, planar: planarOut });
        if (planarOut) {
          assert(Array.isArray(got) && got.length === 2 && got.every((p) => p instanceof (outFormat === 's32le' ? Int32Array : ELEMENT[bout])),
            what + ': typed arrays of the format');
          assert(framesOf(got, bout).equals(want), what);
        } else {
          assert(Buffer.isBuffer(got) && got.equals(want), what);
        }
      }
    }
  }

  // planar float in both directions is processChunkPlanar on int16-unit floats, scaled
  {
    const r = new SpeexResampler(2, 44100, 48000, 7);
    const twin = new SpeexResampler(2, 44100, 48000, 7);
    for (const frames of sizes) {
      const pcm = lcg(frames * 2, seed++);
      const planes = [0, 1].map((c) => Float32Array.from({ length: frames }, (_, f) => pcm[2 * f + c]));
      const want = twin.processChunkPlanar(planes);
      const got = r.processChunkSides(planes, { format: 'f32le' }, { format: 'f32le', planar: true });
      for (let c = 0; c < 2; c++) assert(bytesOf(got[c]).equals(bytesOf(want[c])), 'f32le planes, ' + frames + ' frames, plane ' + c);
    }
  }

  // a planar 5.1 downmix to stereo planes, and a mono instance fed two planes
  {
    const down = [[1, 0, 0.7071, 0.5, 0.7071, 0], [0, 1, 0.7071, 0.5, 0, 0.7071]];
    const r = new SpeexResampler(2, 48000, 44100, 5);
    const twin = new SpeexResampler(2, 48000, 44100, 5);
    const m = new SpeexResampler(1, 48000, 16000, 7);
    const mTwin = new SpeexResampler(1, 48000, 16000, 7);
    for (const frames of sizes) {
      const six = bytesOf(lcg(frames * 6, seed++));
      const want = twin.processChunkMix(six, 's16le', 'f32le-normalized', down, null);
      const got = r.processChunkSides(typed(planesOf(six, 6, 2), 2), { format: 's16le', mix: down },
        { format: 'f32le-normalized', planar: true, channels: 2 });
      assert(framesOf(got, 4).equals(want), '5.1 planes -> stereo planes, ' + frames + ' frames');
      const two = bytesOf(lcg(frames * 2, seed++));
      const wantMono = mTwin.processChunkMix(two, 's16le', 'f32le-normalized', [[0.5, 0.5]], null);
      const gotMono = m.processChunkSides(typed(planesOf(two, 2, 2), 2), { format: 's16le', mix: [[0.5, 0.5]] },
        { format: 'f32le-normalized', planar: true });
      assert(gotMono.length === 1 && bytesOf(gotMono[0]).equals(wantMono), 'two planes -> mono, ' + frames + ' frames');
    }
  }

  // both sides interleaved is processChunkMix itself
  {
    const r = new SpeexResampler(2, 44100, 48000, 7);
    const twin = new SpeexResampler(2, 44100, 48000, 7);
    const chunk = bytesOf(lcg(5000 * 2, seed++));
    assert(r.processChunkSides(chunk, { format: 's16le' }, { format: 's16le' }).equals(twin.processChunkMix(chunk, 's16le', 's16le', null, null)),
      'interleaved both ways');
  }

  let threw = false;
  try {
    new SpeexResampler(2, 8000, 16000, 7).processChunkSides([new Int16Array(4)], { format: 's16le' }, { format: 's16le', planar: true });
  } catch (e) {
    threw = /typed arrays of equal length/.test(e.message);
  }
  assert(threw, 'a missing plane throws');
  console.log('ALL SIDES NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
