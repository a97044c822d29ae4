'use strict';
// renderer.guides, renderer.denoise({guides}) and renderer.temporalFilter({guides}) on the materials demo (C3: a mirror and a
// glass sphere in a checkered room) through Sail.Renderer -> N-API -> libsail_hip.so, for tests/test_guides_js.py. Needs an
// MI355X. The renderer has no AOV maps: the guided filters need none. Prints one JSON line: the view rendered, the FNV-1a
// hashes of the outputs and of the maps the renderer computed by itself, and what the maps' info says.
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
const maps = (r) => [fnv(bytes(r.lib.guidesRead(r.ctx, 0))), fnv(bytes(r.lib.guidesRead(r.ctx, 1)))];

const scene = SCENES.C3();
const r = new Sail.Renderer({ width: W, height: H, deterministic: true, accumulation: 'sum', aov: false,
  temporal: { moments: true }, display: false });
r.update(scene);
let early = null, noAov = null;
try { r.denoise({ guides: true }); } catch (e) { early = e.message; }  // nothing rendered: no view to make the maps for
try { r.denoise(); } catch (e) { noAov = e.message; }                  // the plain call still wants the AOVs
const half = Math.floor(spp / 2);
r.renderSamples(scene, half);
r.noiseMark();
r.renderSamples(scene, spp - half);
const mvp = [];
for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
r.temporalResolve();
const before = r.readAccum();
const one = r.denoise({ guides: true });                        // computes the depth-4 maps by itself
const maps4 = maps(r);
const tf = r.temporalFilter({ guides: true });                  // the maps are current: used as they are
const both = r.denoise({ guides: true, albedo: true });
const two = r.denoise({ iterations: 2, sigmaL: 2.5, sigmaX: 0.05, display: 'gamma', guides: { depth: 1 } });
const maps1 = maps(r);
const info = r.guides(scene, { depth: 0 });
const unchanged = Buffer.from(bytes(before)).equals(Buffer.from(bytes(r.readAccum())));
r.updateObjects(scene);                                         // new rows drop the maps: the next call makes them again
scene.sampleCount = 0;
r.renderSamples(scene, half);
r.noiseMark();
r.renderSamples(scene, spp - half);
const again = r.denoise({ guides: true });
r.destroy();
process.stdout.write(JSON.stringify({
  mvp, eye: Array.from(scene.eye.elements), early, noAov, unchanged,
  one: fnv(bytes(one.rgba)), oneInfo: one.info, maps4, maps1,
  tf: fnv(bytes(tf.rgba)), tfInfo: tf.info, both: fnv(bytes(both.rgba)),
  two: fnv(bytes(two.rgba)), twoU8: fnv(bytes(two.rgba8)),
  maps0: [fnv(bytes(info.n)), fnv(bytes(info.x))],
  guides: { hitPixels: info.hitPixels, followedPixels: info.followedPixels, truncatedPixels: info.truncatedPixels,
    depth: info.depth, maxDepth: info.maxDepth },
  again: fnv(bytes(again.rgba)),
}) + '\n');
