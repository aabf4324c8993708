// processChunkPlanar against processChunk / processChunkFloat of a twin instance on the same frames: byte-equal
// results, call after call (the capacity rule and the stream state are shared).  Needs an MI355X.
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

function planesOf(inter, channels, Kind) {
  const frames = inter.length / channels;
  const planes = [];
  for (let c = 0; c < channels; c++) {
    const p = new Kind(frames);
    for (let f = 0; f < frames; f++) p[f] = inter[f * channels + c];
    planes.push(p);
  }
  return planes;
}

function sameBytes(planes, buf, channels, Kind, what) {
  const inter = new Kind(buf.buffer, buf.byteOffset, buf.length / Kind.BYTES_PER_ELEMENT);
  assert(planes.length === channels, what + ': one array per channel');
  const frames = inter.length / channels;
  for (let c = 0; c < channels; c++) {
    assert(planes[c] instanceof Kind, what + ': kind of the result');
    assert(planes[c].length === frames, what + ': frames of channel ' + c + ' ' + planes[c].length + ' != ' + frames);
    const a = Buffer.from(planes[c].buffer, planes[c].byteOffset, planes[c].byteLength);
    const want = new Kind(frames);
    for (let f = 0; f < frames; f++) want[f] = inter[f * channels + c];
    assert(a.equals(Buffer.from(want.buffer)), what + ': bytes of channel ' + c);
  }
}

async function main() {
  await SpeexResampler.initPromise;
  const channels = 2;
  const sizes = [480, 16384, 1, 160, 70000, 3000];
  for (const Kind of [Int16Array, Float32Array]) {
    const planar = new SpeexResampler(channels, 44100, 48000, 7);
    const twin = new SpeexResampler(channels, 44100, 48000, 7);
    let seed = 7;
    for (const frames of sizes) {
      const pcm = lcg(frames * channels, seed++);
      const inter = Kind === Int16Array ? pcm : Float32Array.from(pcm, (v) => v / 3.0);
      const want = Kind === Int16Array
        ? twin.processChunk(Buffer.from(inter.buffer))
        : twin.processChunkFloat(Buffer.from(inter.buffer));
      const got = planar.processChunkPlanar(planesOf(inter, channels, Kind));
      sameBytes(got, want, channels, Kind, Kind.name + ' ' + frames + ' frames');
    }
    // the same error strings as processChunk for a bad length
    let msg = '';
    try { planar.processChunkPlanar([new Kind(4), new Kind(5)]); } catch (e) { msg = e.message; }
    assert(msg === 'Chunk length should be a multiple of channels * ' + Kind.BYTES_PER_ELEMENT + ' bytes', 'length error: ' + msg);
    msg = '';
    try { planar.processChunkPlanar([new Kind(4)]); } catch (e) { msg = e.message; }
    assert(msg === 'Chunk length should be a multiple of channels * ' + Kind.BYTES_PER_ELEMENT + ' bytes', 'count error: ' + msg);
    // a destroyed instance starts over, like processChunk
    planar.destroy();
    twin.destroy();
    const pcm = lcg(960 * channels, 99);
    const inter = Kind === Int16Array ? pcm : Float32Array.from(pcm, (v) => v / 3.0);
    const want = Kind === Int16Array ? twin.processChunk(Buffer.from(inter.buffer)) : twin.processChunkFloat(Buffer.from(inter.buffer));
    sameBytes(planar.processChunkPlanar(planesOf(inter, channels, Kind)), want, channels, Kind, Kind.name + ' after destroy');
    planar.destroy();
    twin.destroy();
  }
  console.log('ALL PLANAR NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
