'use strict';
// renderer.albedo, renderer.denoise({albedo}) and renderer.temporalFilter({albedo}) on the materials demo (C3: checkered
// room, checkered sphere) through Sail.Renderer -> N-API -> libsail_hip.so, for tests/test_albedo_js.py. Needs an MI355X.
// Prints one JSON line: the view rendered, the FNV-1a hashes of the outputs and of the maps the renderer computed by
// itself, and what the map's info says.
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

const scene = SCENES.C3();
const r = new Sail.Renderer({ width: W, height: H, deterministic: true, accumulation: 'sum', aov: true,
  temporal: { moments: true }, display: false });
r.update(scene);
let early = null;
try { r.denoise({ albedo: true }); } catch (e) { early = e.message; }  // nothing rendered: no view to make the map for
const half = Math.floor(spp / 2);
r.renderSamples(scene, half);
r.noiseMark();
r.renderSamples(scene, spp - half);
const mvp = [];
for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
r.temporalResolve();
const before = r.readAccum();
const plain = r.denoise();
const one = r.denoise({ albedo: true });                       // computes the grid-2 map by itself
const map2 = fnv(bytes(r.lib.albedoRead(r.ctx)));
const tf = r.temporalFilter({ albedo: true });                 // the map is current: used as it is
const two = r.denoise({ iterations: 2, sigmaL: 2.5, sigmaX: 0.05, display: 'gamma', albedo: { grid: 4, amin: 0.02 } });
const map4 = fnv(bytes(r.lib.albedoRead(r.ctx)));
const info = r.albedo(scene, { grid: 1 });
const unchanged = Buffer.from(bytes(before)).equals(Buffer.from(bytes(r.readAccum())));
r.updateObjects(scene);                                        // new rows drop the map: the next call makes it again
scene.sampleCount = 0;
r.renderSamples(scene, half);
r.noiseMark();
r.renderSamples(scene, spp - half);
const again = r.denoise({ albedo: true });
r.destroy();
process.stdout.write(JSON.stringify({
  mvp, eye: Array.from(scene.eye.elements), early, unchanged,
  plain: fnv(bytes(plain.rgba)), one: fnv(bytes(one.rgba)), oneInfo: one.info, map2, map4,
  tf: fnv(bytes(tf.rgba)), tfInfo: tf.info,
  two: fnv(bytes(two.rgba)), twoU8: fnv(bytes(two.rgba8)),
  map1: fnv(bytes(info.rgba)), albedo: { hitPixels: info.hitPixels, partialPixels: info.partialPixels, grid: info.grid },
  again: fnv(bytes(again.rgba)),
}) + '\n');
