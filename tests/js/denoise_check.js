'use strict';
// renderer.denoise on the Cornell example through Sail.Renderer -> N-API -> libsail_hip.so, for tests/test_denoise_js.py.
// Needs an MI355X. Prints one JSON line: FNV-1a hashes of the f32 output (rgb of every texel) and of the RGBA8 output.
// argv: W H spp
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const [W, H, spp] = process.argv.slice(2).map(Number);

function fnv(bytes) {
  let h = 0x811c9dc5;
  for (let i = 0; i < bytes.length; i++) { h ^= bytes[i]; h = Math.imul(h, 0x01000193) >>> 0; }
  return h >>> 0;
}
const bytes = (a) => new Uint8Array(a.buffer, a.byteOffset, a.byteLength);

// without the AOVs the call says what it needs
const plain = new Sail.Renderer({ width: 8, height: 8, deterministic: true, accumulation: 'sum', aov: false, display: false });
let noAov = null;
try { plain.denoise(); } catch (e) { noAov = e.message; }
plain.destroy();

const scene = SCENES.C1();
const r = new Sail.Renderer({ width: W, height: H, deterministic: true, accumulation: 'sum', display: false });
r.update(scene);
const half = Math.floor(spp / 2);
r.renderSamples(scene, half);
let early = null;
try { r.denoise(); } catch (e) { early = e.message; }  // no mark yet
r.noiseMark();
r.renderSamples(scene, spp - half);
const before = r.readAccum();
const d = r.denoise();
const t = r.denoise({ iterations: 2, sigmaL: 2.5, sigmaX: 0.05, display: 'tonemapping' });
const unchanged = Buffer.from(bytes(before)).equals(Buffer.from(bytes(r.readAccum())));
r.destroy();
const rgb = new Float32Array(W * H * 3);
for (let i = 0; i < W * H; i++) for (let c = 0; c < 3; c++) rgb[3 * i + c] = d.rgba[4 * i + c];
process.stdout.write(JSON.stringify({ noAov, early, unchanged, hash: fnv(bytes(rgb)), hasU8: d.rgba8 !== undefined,
  info: d.info, hash2: fnv(bytes(t.rgba)), hashU8: fnv(bytes(t.rgba8)), info2: t.info }) + '\n');
