'use strict';
// Renderer.renderAdaptive / setActiveTiles / getActiveTiles on the Cornell example through N-API -> libsail_hip.so, for
// tests/test_adaptive_js.py. Needs an MI355X. Prints one JSON line: the view (P*MV row-major, eye), what renderAdaptive
// returned, the mask afterwards and the FNV-1a hash of the accumulator's bytes; the test makes the same call through capi.
// argv: W H bounces noise minSpp maxSpp dilate
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const [W, H, B, noise, minSpp, maxSpp, dilate] = process.argv.slice(2, 9).map(Number);

function fnv(bytes) {
  let h = 0x811c9dc5;
  for (let i = 0; i < bytes.length; i++) { h ^= bytes[i]; h = Math.imul(h, 0x01000193) >>> 0; }
  return h >>> 0;
}
const scene = SCENES.C1();
const r = new Sail.Renderer({ width: W, height: H, maxBounces: B, accumulation: 'sum', deterministic: true, display: false });
r.update(scene);
let refused = null;
try { r.setActiveTiles([1]); } catch (e) { refused = e.message; }  // a wrong count
const res = r.renderAdaptive(scene, { noise, minSpp, maxSpp, dilate: dilate !== 0 });
const mvp = [];
for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
const acc = r.readAccum();
const out = { mvp, eye: Array.from(scene.eye.elements), refused, sampleCount: scene.sampleCount,
  res: Object.assign({}, res, { tileSamples: Array.from(res.tileSamples) }),
  mask: Array.from(r.getActiveTiles()), hash: fnv(new Uint8Array(acc.buffer, acc.byteOffset, acc.byteLength)) };
// a mask by hand: every tile on, then none
r.setActiveTiles(out.mask.map(() => 1));
out.allOn = Array.from(r.getActiveTiles());
r.setActiveTiles(null);
out.cleared = Array.from(r.getActiveTiles());
const mix = new Sail.Renderer({ width: W, height: H, maxBounces: B, deterministic: true, display: false });
mix.update(scene);
try { mix.renderAdaptive(scene, { noise }); out.mixRefused = null; } catch (e) { out.mixRefused = e.message; }
mix.destroy();
r.destroy();
process.stdout.write(JSON.stringify(out) + '\n');
