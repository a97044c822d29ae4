'use strict';
// A drag of the materials demo's matte sphere with the option temporal: {objects: true}, driven by Pickup and Sail.Control,
// through N-API -> libsail_hip.so, for tests/test_temporal_motion_js.py. Needs an MI355X. Prints one JSON line: for every
// step the object rows and the motion handed to the library (null when nothing moved), the view (P*MV row-major, eye) and
// the FNV-1a hash of renderer.image(); the test replays them through capi.
// argv: W H objects (1: temporal: {objects: true}; 0: temporal: true, where a drag drops the history)
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const { Control } = require('../../sail_amd/js/src/control');
const { Vector } = require('../../sail_amd/js/src/la');
const [W, H] = process.argv.slice(2, 4).map(Number);
const objects = process.argv[4] === '1';
const ROW = 5;  // the matte sphere

function fnv(bytes) {
  let h = 0x811c9dc5;
  for (let i = 0; i < bytes.length; i++) { h ^= bytes[i]; h = Math.imul(h, 0x01000193) >>> 0; }
  return h >>> 0;
}
const scene = SCENES.C3();
scene.filter = 'color';
const r = new Sail.Renderer({ width: W, height: H, temporal: objects ? { objects: true } : true, deterministic: true, display: false });
r.update(scene);
Control.update(scene);

const steps = [];
function step(n) {
  const moved = scene.moving;
  const motion = moved ? Array.from(scene.objectMotion()) : null;   // before the render consumes it
  for (let i = 0; i < n; i++) r.render(scene);
  const mvp = [];
  for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
  // after the render the translation is applied and zeroed: serialising again changes nothing
  const rows = moved ? Array.from(scene.serializeObjects()) : null;
  steps.push({ n, moved, motion, rows, mvp, eye: Array.from(scene.eye.elements), hash: fnv(r.image()), k: scene.sampleCount });
}
step(4);
// the pixel the sphere's centre projects to, in canvas coordinates (row 0 = top)
const c = scene.objects[ROW].c.elements;
const p = scene.mat.multiply(new Vector([c[0], c[1], c[2], 1])).elements;
const x0 = ((p[0] / p[3]) * 0.5 + 0.5) * W, y0 = (1 - ((p[1] / p[3]) * 0.5 + 0.5)) * H;
const picked = Control.pick.pick(x0, y0);
const selected = scene.objects.indexOf(scene.select);
const began = picked && Control.pick.movingBegin(x0, y0);
for (const [dx, dy] of [[2, 0], [4, -1], [5, -2]]) {
  Control.mousemove(x0 + dx, y0 + dy);
  step(1);
}
Control.mouseup(x0 + 5, y0 - 2);
step(2);                 // the drag is over: the same frame goes on
r.destroy();
process.stdout.write(JSON.stringify({ steps, selected, began, histCap: r.objectHistCap }) + '\n');
