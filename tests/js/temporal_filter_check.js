'use strict';
// Renderer({aov: true, temporal: {moments: true}}).temporalFilter on the Cornell example after an orbit by Sail.Control,
// through N-API -> libsail_hip.so, for tests/test_temporal_filter_js.py. Needs an MI355X. Prints one JSON line: the views
// rendered (P*MV row-major, eye, samples), the FNV-1a hashes of temporalFilter's outputs with the defaults and with
// options, their infos, the moment map's hash, and what temporalFilter throws without aov or without moments.
// argv: W H
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const { Control } = require('../../sail_amd/js/src/control');
const [W, H] = process.argv.slice(2, 4).map(Number);

function fnv(bytes) {
  let h = 0x811c9dc5;
  for (let i = 0; i < bytes.length; i++) { h ^= bytes[i]; h = Math.imul(h, 0x01000193) >>> 0; }
  return h >>> 0;
}
const bytesOf = (f32) => new Uint8Array(f32.buffer, f32.byteOffset, f32.byteLength);
function thrown(options) {
  const r = new Sail.Renderer(Object.assign({ width: 16, height: 16, display: false }, options));
  try { r.temporalFilter(); return null; } catch (e) { return e.message; } finally { r.destroy(); }
}

const scene = SCENES.C1();
const r = new Sail.Renderer({ width: W, height: H, aov: true, temporal: { moments: true }, deterministic: true, display: false });
r.update(scene);
Control.update(scene);
const steps = [];
function step(n) {
  for (let i = 0; i < n; i++) r.render(scene);
  const mvp = [];
  for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
  const res = r.temporalResolve();
  steps.push({ n, mvp, eye: Array.from(scene.eye.elements), k: scene.sampleCount, resolve: fnv(bytesOf(res.rgba)) });
}
step(4);
Control.mouseDown = true;   // Control's orbit: a drag that started on empty space
Control.oldX = 10; Control.oldY = 10;
Control.mousemove(15, 12);
Control.mouseup(15, 12);
step(1);
const plain = r.temporalFilter();
const other = r.temporalFilter({ iterations: 2, sigmaL: 1.5, sigmaX: 0.1, minHist: 2, display: 'gamma', gamma: 1.8 });
const out = {
  steps,
  defaults: r.lib.temporalFilterDefaults(),
  moments: fnv(bytesOf(r.lib.temporalReadMoments(r.ctx, 2))),
  plain: { rgba: fnv(bytesOf(plain.rgba)), has8: plain.rgba8 !== undefined, info: plain.info },
  other: { rgba: fnv(bytesOf(other.rgba)), rgba8: fnv(other.rgba8), info: other.info },
  noAov: thrown({ aov: false, temporal: { moments: true } }),
  noMoments: thrown({ aov: true, temporal: true }),
  noTemporal: thrown({ aov: true }),
};
r.destroy();
process.stdout.write(JSON.stringify(out) + '\n');
