#!/usr/bin/env node
'use strict';
// Headless Sail: run a scene script the way the reference's editor does (ui/ui.js:47-52: eval the code, which
// assigns `scene`, then Renderer.update(scene)), render N samples on the GPU and write the frame to disk.
//
//   node sail_amd/js/cli.js scene.js [--width 512] [--height 512] [--spp 64] [--bounces 5] [--device -1]
//        [--noise X [--adaptive] [--min-spp 16] [--max-spp 65536]] [--denoise [--denoise-iterations 4] [--albedo [--albedo-grid 2]]
//         [--guides [--guide-depth 4]]]
//        [--filter <name>] [--filter-r 'vec2(2.0,2.0)'] [--gamma 2.2] [--deterministic]
//        [--png out.png] [--pfm out.pfm] [--exr out.exr] [--stats]
//
// --noise X (instead of --spp) renders until the frame's noise estimate is at most X: it looks at --min-spp samples and at
// every doubling, up to --max-spp. --stats then also prints the spp reached, the noise and whether it converged.
// --adaptive stops rendering each 64x64 tile once its own error is at most X (and no tile beside it is noisier) and ends
// when every tile has stopped; --stats then also prints pixel_samples (traced) and frame_pixel_samples (the frame's).
// --denoise writes the variance-guided a-trous denoiser's image instead of the frame: with --spp N it marks the frame at
// floor(N/2) samples, with --noise X it uses the mark of the look before the last. --stats then also prints denoise_ms.
// --albedo divides the frame by the albedo map of the view before the denoiser and multiplies it back afterwards, so that
// procedural textures survive; --albedo-grid N (1..4) is the map's sub-pixel grid. --stats then also prints albedo_ms.
// --guides makes the denoiser read the guide maps of the view, the normal and position of the surface behind mirror and smooth
// glass, in the AOVs' place; --guide-depth N (0..8) is how many such surfaces are followed. --stats then also prints guides_ms.
// The script sees `Sail` (the full API) and must assign `scene` (a Sail.Scene with a camera), exactly as the
// editor text does. --filter overrides scene.filter for the PNG (with --denoise it becomes the denoiser's display transform:
// color, gamma or tonemapping); without --denoise the PFM and EXR are always the unfiltered mean image.
const fs = require('fs');
const path = require('path');
const vm = require('vm');
const Sail = require('./index');
const { writePFM, writePNG, writeEXR } = require('./src/image');

function parse(argv) {
  const opt = { width: 512, height: 512, spp: 64, minSpp: 16, maxSpp: 65536, bounces: 5, device: -1, deterministic: false, stats: false };
  const rest = [];
  for (let i = 0; i < argv.length; i++) {
    const a = argv[i];
    const val = () => { if (i + 1 >= argv.length) throw new Error(`${a} needs a value`); return argv[++i]; };
    switch (a) {
      case '--width': opt.width = parseInt(val(), 10); break;
      case '--height': opt.height = parseInt(val(), 10); break;
      case '--spp': opt.spp = parseInt(val(), 10); opt.sppGiven = true; break;
      case '--noise': opt.noise = parseFloat(val()); break;
      case '--adaptive': opt.adaptive = true; break;
      case '--min-spp': opt.minSpp = parseInt(val(), 10); opt.untilGiven = a; break;
      case '--max-spp': opt.maxSpp = parseInt(val(), 10); opt.untilGiven = a; break;
      case '--denoise': opt.denoise = true; break;
      case '--denoise-iterations': opt.denoiseIterations = parseInt(val(), 10); break;
      case '--albedo': opt.albedo = true; break;
      case '--albedo-grid': opt.albedoGrid = parseInt(val(), 10); break;
      case '--guides': opt.guides = true; break;
      case '--guide-depth': opt.guideDepth = parseInt(val(), 10); break;
      case '--bounces': opt.bounces = parseInt(val(), 10); break;
      case '--device': opt.device = parseInt(val(), 10); break;
      case '--filter': opt.filter = val(); break;
      case '--filter-r': opt.filterR = val(); break;
      case '--gamma': opt.gamma = val(); break;
      case '--png': opt.png = val(); break;
      case '--pfm': opt.pfm = val(); break;
      case '--exr': opt.exr = val(); break;
      case '--deterministic': opt.deterministic = true; break;
      case '--stats': opt.stats = true; break;
      case '-h': case '--help': opt.help = true; break;
      default:
        if (a.startsWith('--')) throw new Error(`unknown option ${a}`);
        rest.push(a);
    }
  }
  if (opt.noise !== undefined && opt.sppGiven) throw new Error('--noise and --spp exclude each other');
  if (opt.noise !== undefined && Number.isNaN(opt.noise)) throw new Error('--noise needs a number');
  if (opt.noise === undefined && opt.untilGiven) throw new Error(`${opt.untilGiven} needs --noise`);
  if (opt.adaptive && opt.noise === undefined) throw new Error('--adaptive needs --noise');
  if (opt.denoiseIterations !== undefined && !opt.denoise) throw new Error('--denoise-iterations needs --denoise');
  if (opt.denoiseIterations !== undefined && !(opt.denoiseIterations >= 1 && opt.denoiseIterations <= 6))
    throw new Error('--denoise-iterations needs a number from 1 to 6');
  if (opt.albedo && !opt.denoise) throw new Error('--albedo needs --denoise');
  if (opt.albedoGrid !== undefined && !opt.albedo) throw new Error('--albedo-grid needs --albedo');
  if (opt.albedoGrid !== undefined && !(opt.albedoGrid >= 1 && opt.albedoGrid <= 4))
    throw new Error('--albedo-grid needs a number from 1 to 4');
  if (opt.guides && !opt.denoise) throw new Error('--guides needs --denoise');
  if (opt.guideDepth !== undefined && !opt.guides) throw new Error('--guide-depth needs --guides');
  if (opt.guideDepth !== undefined && !(opt.guideDepth >= 0 && opt.guideDepth <= 8))
    throw new Error('--guide-depth needs a number from 0 to 8');
  if (opt.denoise && opt.noise === undefined && !(opt.spp >= 2))
    throw new Error('--denoise needs --spp 2 or more: it compares the two halves of the samples');
  opt.script = rest[0];
  return opt;
}

function loadScene(file) {
  const code = fs.readFileSync(file, 'utf8');
  const context = { Sail, console, Math, scene: undefined };
  vm.createContext(context);
  vm.runInContext(code, context, { filename: path.basename(file) });
  if (!context.scene || !(context.scene instanceof Sail.Scene)) throw new Error(`${file} did not assign a Sail.Scene to \`scene\``);
  return context.scene;
}

function main() {
  const opt = parse(process.argv.slice(2));
  if (opt.help || !opt.script) {
    process.stdout.write(fs.readFileSync(__filename, 'utf8').split('\n').slice(2, 24).map((l) => l.replace(/^\/\/ ?/, '')).join('\n') + '\n');
    return opt.help ? 0 : 2;
  }
  const scene = loadScene(opt.script);
  if (opt.filter) scene.filter = opt.filter;
  if (opt.filterR) scene.filter.addParam('r', opt.filterR);
  if (opt.gamma) scene.filter.addParam('c', opt.gamma);
  const pointwise = ['color', 'gamma', 'tonemapping'].includes(scene.filter.name);
  if (opt.denoise && opt.png && !pointwise)
    throw new Error(`--denoise --png applies the filter to the denoised texel: it needs --filter color, gamma or tonemapping, not ${scene.filter.name}`);
  const needAov = (opt.denoise && !opt.guides) || ['wavelet', 'normal', 'position'].includes(scene.filter.name);
  const r = new Sail.Renderer({ width: opt.width, height: opt.height, device: opt.device, maxBounces: opt.bounces,
    deterministic: opt.deterministic, accumulation: 'sum', aov: needAov, display: false });
  r.update(scene);
  const t0 = process.hrtime.bigint();
  let until = null;
  if (opt.adaptive) until = r.renderAdaptive(scene, { noise: opt.noise, minSpp: opt.minSpp, maxSpp: opt.maxSpp });
  else if (opt.noise !== undefined) until = r.renderUntil(scene, { noise: opt.noise, minSpp: opt.minSpp, maxSpp: opt.maxSpp });
  else if (opt.denoise) {  // the two halves the denoiser compares
    r.renderSamples(scene, Math.floor(opt.spp / 2));
    r.noiseMark();
    r.renderSamples(scene, opt.spp - Math.floor(opt.spp / 2));
  } else r.renderSamples(scene, opt.spp);
  let mean, den = null, alb = null, gui = null;
  if (opt.denoise) {
    if (until && until.history.length < 2)
      throw new Error(`--denoise: the render stopped at its first look (${until.k} spp), which only marks the frame: no second look, so there are no two halves to compare (raise --max-spp above --min-spp)`);
    if (opt.albedo) alb = r.albedo(scene, { grid: opt.albedoGrid === undefined ? 2 : opt.albedoGrid });
    if (opt.guides) gui = r.guides(scene, { depth: opt.guideDepth === undefined ? 4 : opt.guideDepth });
    den = r.denoise({ iterations: opt.denoiseIterations, display: opt.png ? r.filter.kind : undefined, gamma: r.filter.gamma,
      albedo: opt.albedo ? { grid: alb.grid } : undefined, guides: opt.guides ? { depth: gui.depth } : undefined });
    mean = den.rgba;
  } else mean = r.readPixels();
  const ms = Number(process.hrtime.bigint() - t0) / 1e6;
  if (opt.pfm) writePFM(opt.pfm, opt.width, opt.height, mean);
  if (opt.exr) writeEXR(opt.exr, opt.width, opt.height, mean);
  if (opt.png) writePNG(opt.png, opt.width, opt.height, den ? den.rgba8 : r.image());
  if (opt.stats) {
    const st = r.stats();
    const out = { width: opt.width, height: opt.height, spp: until ? until.k : opt.spp, bounces: opt.bounces,
      ms, segments: st.segments, kernelMs: st.kernelMs, filter: scene.filter.name };
    // (a frame that never reached a second look has no estimate: its noise is infinite, null in JSON)
    if (until) Object.assign(out, { noise: until.mean, converged: until.converged });
    if (opt.adaptive) Object.assign(out, { pixel_samples: until.pixelSamples, frame_pixel_samples: until.framePixelSamples, active_tiles: until.activeTiles });
    if (den) out.denoise_ms = den.info.kernelMs;
    if (alb) Object.assign(out, { albedo_ms: alb.kernelMs, albedo_grid: alb.grid });
    if (gui) Object.assign(out, { guides_ms: gui.kernelMs, guide_depth: gui.depth });
    process.stdout.write(JSON.stringify(out) + '\n');
  }
  r.destroy();
  return 0;
}

try {
  process.exitCode = main();
} catch (e) {
  process.stderr.write(`sail: ${e.message}\n`);
  process.exitCode = 1;
}
