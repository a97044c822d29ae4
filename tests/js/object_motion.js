'use strict';
// scene.objectMotion() on the materials demo, driven by Pickup's drag, for tests/test_temporal_motion_host.py. Needs no
// device: the selection is set by hand instead of picked. Prints one JSON line: the motion before the drag, after each
// Pickup.moving, and after serializeObjects(), with the dragged sphere's row before and after.
const { SCENES } = require('../../sail_amd/js/scenes');
const { Pickup } = require('../../sail_amd/js/src/control');
const { Vector } = require('../../sail_amd/js/src/la');
const ROW =Number(process.argv[2]);

const scene = SCENES.C3();
scene.serialize();                       // gives the rows their texparam ids, as Renderer.update does
const pick = new Pickup(scene);          // no renderer: a 512 x 512 canvas
scene.select = scene.objects[ROW];
const out = { n: scene.objects.length, before: Array.from(scene.objectMotion()), rows0: Array.from(scene.serializeObjects()) };
// the pixel the sphere's centre projects to
const c = scene.select.c.elements;
const p = scene.mat.multiply(new Vector([c[0], c[1], c[2], 1])).elements;
const x0 = ((p[0] / p[3]) * 0.5 + 0.5) * 512, y0 = (1 - ((p[1] / p[3]) * 0.5 + 0.5)) * 512;
out.began = pick.movingBegin(x0, y0);
out.moving = scene.moving;
pick.moving(x0 + 12, y0 - 5);
out.drag1 = Array.from(scene.objectMotion());
out.again = Array.from(scene.objectMotion());            // reading does not consume
out.rows1 = Array.from(scene.serializeObjects());
out.after = Array.from(scene.objectMotion());
process.stdout.write(JSON.stringify(out) + '\n');
