// setDither / getDither through the Node binding: node test_dither.js <in.s16le> <out.u8> <frames,frames,...>
// Stereo 44.1k -> 48k, quality 7, setDither('triangular', 5n); the input file's s16le frames go through
// processChunkFormat(chunk, 's16le', 'u8') cut as the third argument says, the results are written back to back into the
// output file and getDither() is printed as one JSON line.  tests/test_gpu_dither.py holds the bytes against the Python
// binding's for the same state.  Needs an MI355X.
const fs = require('fs');
const mod = require('../index.js');
const SpeexResampler = mod.default || mod;

function assert(cond, what) {
  if (!cond) {
    console.error('FAILED: ' + what);
    process.exit(1);
  }
}

async function main() {
  await SpeexResampler.initPromise;
  const [inPath, outPath, cuts] = process.argv.slice(2);
  const channels = 2;
  const pcm = fs.readFileSync(inPath);
  const r = new SpeexResampler(channels, 44100, 48000, 7);
  let d = r.getDither();
  assert(d.kind === 'none' && d.seed === 0n && d.position === 0n, 'a fresh instance has no dither');
  let threw = false;
  try { r.setDither('gaussian'); } catch (e) { threw = true; }
  assert(threw && r.getDither().kind === 'none', 'an unknown kind throws and changes nothing');
  r.setDither('triangular', 5n);
  d = r.getDither();
  assert(d.kind === 'triangular' && d.seed === 5n && d.position === 0n, 'setDither is read back');
  const outs = [];
  let at = 0;
  for (const frames of cuts.split(',').map(Number)) {
    const bytes = frames * channels * 2;
    outs.push(r.processChunkFormat(pcm.subarray(at, at + bytes), 's16le', 'u8'));
    at += bytes;
  }
  assert(at === pcm.length, 'the cuts cover the file');
  fs.writeFileSync(outPath, Buffer.concat(outs));
  d = r.getDither();
  // 64-bit values survive the trip whole
  const b = new mod.SpeexResamplerBatch(2, channels, 44100, 48000, 7);
  b.setDither('rectangular', 0xfffffffffffffff0n, (1n << 40n) + 3n);
  const d1 = b.getDither(1);
  assert(d1.kind === 'rectangular' && d1.position === (1n << 40n) + 3n, 'batch setDither reaches stream 1');
  assert(d1.seed === BigInt.asUintN(64, 0xfffffffffffffff0n + 0x9E3779B97F4A7C15n), 'stream 1 draws from seed + the stream step');
  assert(b.getDither().seed === 0xfffffffffffffff0n, 'stream 0 draws from the seed');
  b.destroy();
  r.destroy();
  console.log(JSON.stringify({ kind: d.kind, seed: d.seed.toString(), position: d.position.toString() }));
  console.log('ALL DITHER NODE TESTS PASSED');
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
