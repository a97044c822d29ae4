'use strict';
// The temporal option of Sail.Renderer on the Cornell example, orbited and zoomed by Sail.Control, through N-API ->
// libsail_hip.so, for tests/test_temporal_js.py. Needs an MI355X. Prints one JSON line: for every step the view (P*MV
// row-major, eye), how it was rendered, and the FNV-1a hash of renderer.image(); the test replays the views through capi.
// argv: W H filter temporal (0 | 1 | cap:posTol, the option's object form)
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const { Control } = require('../../sail_amd/js/src/control');
const [W, H] = process.argv.slice(2, 4).map(Number);
const filter = process.argv[4];
const targ = process.argv[5];
const temporal = targ !== '0';
const option = !temporal ? undefined : (targ === '1' ? true : { cap: Number(targ.split(':')[0]), posTol: Number(targ.split(':')[1]) });

function fnv(bytes) {
  let h = 0x811c9dc5;
  for (let i = 0; i < bytes.length; i++) { h ^= bytes[i]; h = Math.imul(h, 0x01000193) >>> 0; }
  return h >>> 0;
}
const scene = SCENES.C1();
scene.filter = filter;
const r = new Sail.Renderer({ width: W, height: H, temporal: option, deterministic: true, display: false });
r.update(scene);
Control.update(scene);

const steps = [];
function step(how, n) {
  if (how === 'render') for (let i = 0; i < n; i++) r.render(scene);
  else r.renderSamples(scene, n);
  const mvp = [];
  for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) mvp.push(scene.mat.elements[i][j]);
  steps.push({ how, n, mvp, eye: Array.from(scene.eye.elements), hash: fnv(r.image()), k: scene.sampleCount });
}
function drag(dx, dy) {  // Control's orbit: a drag that started on empty space
  Control.mouseDown = true;
  Control.oldX = 10; Control.oldY = 10;
  Control.mousemove(10 + dx, 10 + dy);
  Control.mouseup(10 + dx, 10 + dy);
}
step('render', 4);
drag(5, 2);              // 0.05 rad about the vertical axis, 0.02 rad up
step('render', 1);
step('render', 2);       // the same view, more samples: the resolve blends again from the same history
Control.wheel(true);     // zoom out
step('render', 1);
drag(-12, 0);
step('samples', 3);
let gb = null;
if (temporal) {
  const g = r.gbuffer(scene);
  gb = { id: fnv(new Uint8Array(g.id.buffer)), t: fnv(new Uint8Array(g.t.buffer)), xyz: fnv(new Uint8Array(g.xyz.buffer)) };
  const res = r.temporalResolve({ display: 'gamma', gamma: 2.2 });
  gb.resolve = fnv(new Uint8Array(res.rgba.buffer));
  gb.resolve8 = fnv(res.rgba8);
  gb.info = res.info;
}
r.destroy();
process.stdout.write(JSON.stringify({ steps, gb }) + '\n');
