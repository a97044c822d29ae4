'use strict';
// renderer.renderUntil / noiseMark / noise on the Cornell example through Sail.Renderer -> N-API -> libsail_hip.so, for
// tests/test_noise_js.py. Needs an MI355X. Prints one JSON line.
// argv: W H target minSpp maxSpp accumulation(sum|mix)
const Sail = require('../../sail_amd/js');
const { SCENES } = require('../../sail_amd/js/scenes');
const [W, H, target, minSpp, maxSpp, mode] = process.argv.slice(2);
const opts = { width: +W, height: +H, deterministic: true, accumulation: mode, display: false };
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);

const scene = SCENES.C1();
const r = new Sail.Renderer(opts);
r.update(scene);
const res = r.renderUntil(scene, { noise: +target, minSpp: +minSpp, maxSpp: +maxSpp });
const sampleCount = scene.sampleCount;
const got = r.readAccum();

// the same number of samples in one call on a second renderer
const scene2 = SCENES.C1();
const r2 = new Sail.Renderer(opts);
r2.update(scene2);
r2.renderSamples(scene2, res.k);
const same = bytes(got).equals(bytes(r2.readAccum()));

// by hand on the second renderer: mark, k more samples, estimate with the tile map, re-mark
r2.noiseMark();
let early = null;
try { r2.noise(); } catch (e) { early = e.message; }  // no sample since the mark
r2.renderSamples(scene2, res.k);
const n = r2.noise({ remark: true, tiles: true });
r.destroy();
r2.destroy();
process.stdout.write(JSON.stringify({ res, sampleCount, same, early,
  noise: { mean: n.mean, maxTile: n.maxTile, k: n.k, kMark: n.kMark, nonfinite: n.nonfinite, tilesX: n.tilesX, tilesY: n.tilesY,
    tiles: n.tileErr.length, tileMax: Math.max(...n.tileErr) } }) + '\n');
