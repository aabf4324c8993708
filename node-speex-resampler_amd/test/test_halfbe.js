// 's16be', 's24be', 's32be', 'f16le-normalized' and 'bf16le-normalized' in processChunkFormat / processChunkMix /
// processChunkSides against results recorded by the Python binding on the same stream cut into the same chunks: byte-equal,
// call after call.  Usage: node test_halfbe.js <directory with manifest.json, written by tests/test_gpu_halfbe.py>.
// Needs an MI355X.
const fs = require('fs');
const path = require('path');
const mod = require('../index.js');
const SpeexResampler = mod.default || mod;

function assert(cond, what) {
  if (!cond) {
    console.error('FAILED: ' + what);
    process.exit(1);
  }
}

const BYTES = { 's16le': 2, 'f32le-normalized': 4, 's16be': 2, 's24be': 3, 's32be': 4, 'f16le-normalized': 2, 'bf16le-normalized': 2 };

// interleaved bytes <-> one Uint8Array per channel
function planesOf(buf, channels, bytes) {
  const frames = buf.length / channels / bytes;
  const planes = [];
  for (let c = 0; c < channels; c++) {
    const p = new Uint8Array(frames * bytes);
    for (let f = 0; f < frames; f++) for (let k = 0; k < bytes; k++) p[f * bytes + k] = buf[(f * channels + c) * bytes + k];
    planes.push(p);
  }
  return planes;
}
function framesOf(planes, bytes) {
  const views = planes.map((p) => new Uint8Array(p.buffer, p.byteOffset, p.byteLength));
  const frames = views[0].length / bytes;
  const out = Buffer.alloc(frames * views.length * bytes);
  for (let c = 0; c < views.length; c++) {
    for (let f = 0; f < frames; f++) for (let k = 0; k < bytes; k++) out[(f * views.length + c) * bytes + k] = views[c][f * bytes + k];
  }
  return out;
}

async function main() {
  await SpeexResampler.initPromise;
  const dir = process.argv[2];
  const manifest = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json'), 'utf8'));
  assert(manifest.length > 0, 'an empty manifest');
  for (const c of manifest) {
    const input = fs.readFileSync(path.join(dir, c.input));
    const expected = fs.readFileSync(path.join(dir, c.expected));
    const bin = BYTES[c.inFormat], bout = BYTES[c.outFormat];
    const r = new SpeexResampler(c.channels, c.inRate, c.outRate, c.quality);
    if (c.dither) r.setDither(c.dither.kind, BigInt(c.dither.seed), BigInt(c.dither.position));
    const got = [];
    let at = 0;
    for (const frames of c.chunks) {
      const chunk = input.slice(at * c.inChannels * bin, (at + frames) * c.inChannels * bin);
      at += frames;
      if (c.call === 'format') {
        got.push(r.processChunkFormat(chunk, c.inFormat, c.outFormat));
      } else if (c.call === 'mix') {
        got.push(r.processChunkMix(chunk, c.inFormat, c.outFormat, c.inMix, c.outMix));
      } else {
        const inSide = { format: c.inFormat, mix: c.inMix };
        const outSide = { format: c.outFormat, mix: c.outMix, planar: c.planarOut };
        const res = r.processChunkSides(c.planarIn ? planesOf(chunk, c.inChannels, bin) : chunk, inSide, outSide);
        if (c.planarOut) {
          assert(Array.isArray(res) && res.length === c.outChannels, c.name + ': one plane per channel');
          const want = c.outFormat.endsWith('be') ? Uint8Array : (c.outFormat.startsWith('f16') || c.outFormat.startsWith('bf16')) ? Uint16Array : null;
          if (want) assert(res.every((p) => p instanceof want), c.name + ': kind of the result planes');
          got.push(framesOf(res, bout));
        } else {
          got.push(res);
        }
      }
    }
    const all = Buffer.concat(got);
    assert(all.length === expected.length, c.name + ': ' + all.length + ' bytes, expected ' + expected.length);
    assert(all.equals(expected), c.name + ': bytes differ');
    console.log('ok ' + c.name + ' (' + all.length + ' bytes)');
  }
  let threw = false;
  try {
    new SpeexResampler(1, 8000, 16000, 7).processChunkFormat(Buffer.alloc(4), 's16be', 'f16be');
  } catch (e) {
    threw = /Unknown sample format/.test(e.message);
  }
  assert(threw, 'an unknown format name throws');
  console.log('ALL HALFBE NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
