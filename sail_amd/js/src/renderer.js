'use strict';
// Sail.Renderer over libsail_hip.so (through the N-API addon) in place of the WebGL2 programs.
//   new Renderer(canvas | {width, height, device, devices, ...})   src/core/renderer.js:9-39
//     devices: N (GPUs 0..N-1) or an array of ordinals -> one multi-device context (sail_create_multi): the
//     frame's tiles are dealt across the GPUs and summed into GPU 0 (RCCL) before each display / readback
//   renderer.update(scene)        -> Tracer.update (tracer.js:42-90): rows + plugin set -> sail_set_scene
//   renderer.updateObjects(scene) -> Tracer.updateObjects (tracer.js:25-40) -> sail_update_objects
//   renderer.render(scene)        -> Tracer.render (tracer.js:92-101): one progressive sample with a
//                                    jittered inverse camera matrix and a time seed -> sail_render, then the
//                                    display filter (renderer.js:63) -> sail_filter, painted to the canvas
// Extensions (same API object): renderSamples(scene, spp) runs a whole deterministic sample schedule in
// one call; readPixels() / readAOV() / image() read the float frame back (the reference never reads back);
// renderUntil(scene, {noise, minSpp, maxSpp}) renders until the device-side noise estimate is at most `noise`
// (noiseMark() / noise() are its two halves: sail_noise_mark / sail_noise_estimate); denoise({...}) runs the
// variance-guided a-trous denoiser over the frame, the mark and the AOV maps (sail_denoise). Camera-motion reprojection:
// gbuffer(scene) is the id / depth / position pass of the scene's view (sail_gbuffer); temporalBegin(scene) tells the
// context that the camera is now at the scene's view and temporalResolve({display, gamma}) blends the history reprojected
// into it with the samples rendered since (sail_temporal_begin / sail_temporal_resolve). With the option
// temporal: true | {cap, posTol} (off by default) render / renderSamples / renderUntil call temporalBegin whenever they
// restart the frame, and image() shows the resolve instead of the bare frame for the pointwise display filters, so an
// orbit keeps the picture instead of dropping to one noisy sample. With temporal: {moments: true} the luminance moments are
// tracked as well and temporalFilter({...}) runs the a-trous passes over the resolved picture (sail_temporal_filter).
// With temporal: {objects: true | {histCap}} a drag keeps the history too: updateObjects hands the library each row's
// translation (sail_move_objects) and the next frame reprojects the moved object's pixels from where they were.
// albedo(scene, {grid}) is the albedo map of a view (sail_albedo); denoise({albedo: true}) and
// temporalFilter({albedo: true}) filter the picture divided by it, so that procedural textures survive
// (sail_denoise_albedo / sail_temporal_filter_albedo); the map is computed when the option is set and it is stale.
// guides(scene, {depth}) are the guide maps of a view (sail_guides): the normal and position of the surface behind mirror
// and smooth glass; denoise({guides: true}) and temporalFilter({guides: true}) read them in the AOVs' place
// (sail_use_guides) and then need no aov: true; the maps are computed when the option is set and they are stale.
const native = require('./native');
const { filterConfig } = require('./filter');

const MAXBOUNCES = 5;  // define.glsl:6
const ALBEDO_AMIN = 0.01;  // SAIL_ALBEDO_AMIN_DEFAULT: a guard, not a tuned value
const ACCUM = { sum: 0, mix: 1, compat8: 2 };
const SHAPE_ID = { cube: 1, sphere: 2, rectangle: 3, cone: 4, cylinder: 5, disk: 6, hyperboloid: 7, paraboloid: 8, cornellbox: 9 };
const MAT_ID = { matte: 1, mirror: 2, metal: 3, glass: 4 };
const TEX_ID = { checkerboard: 5, checkerboard2: 7, bilerp: 8, mixf: 9, scale: 10, uvf: 11 };
const LIGHT_ID = { area: 0, point: 1, spot: 2 };

function masksOf(cfg) {
  const m = (list, table) => list.reduce((acc, p) => acc | (1 << table[p.name]), 0) >>> 0;
  return [m(cfg.shape, SHAPE_ID), m(cfg.material, MAT_ID), m(cfg.texture, TEX_ID), m(cfg.light, LIGHT_ID)];
}
function rowMajor(mat) {
  const out = new Float64Array(16);
  for (let i = 0; i < 4; i++) for (let j = 0; j < 4; j++) out[i * 4 + j] = mat.elements[i][j];
  return out;
}

class Renderer {
  constructor(target = {}, options = {}) {
    const isCanvas = target && typeof target.getContext === 'function';
    const opts = isCanvas ? options : Object.assign({}, target, options);
    this.canvas = isCanvas ? target : null;
    this.width = opts.width || (this.canvas && this.canvas.width) || 512;    // webgl.js:24 (512 x 512)
    this.height = opts.height || (this.canvas && this.canvas.height) || 512;
    this.device = opts.device === undefined ? -1 : opts.device;
    this.devices = opts.devices === undefined ? null
      : (Array.isArray(opts.devices) ? opts.devices.slice() : Array.from({ length: opts.devices }, (_, i) => i));
    if (this.devices && this.devices.length < 1) throw new Error('Renderer: devices must name at least one GPU');
    this.maxBounces = opts.maxBounces || MAXBOUNCES;
    this.deterministic = !!opts.deterministic;  // frozen schedule (SURVEY §8(d)) instead of Math.random + clock
    // a sample split sums every device's own samples, so it accumulates sums (a running mean cannot be split)
    this.accumulation = opts.accumulation || (opts.partition === 'samples' ? 'sum' : 'mix');
    if (!(this.accumulation in ACCUM)) throw new Error(`Renderer: unknown accumulation '${this.accumulation}'`);
    if (opts.partition !== undefined && opts.partition !== 'tiles' && opts.partition !== 'samples')
      throw new Error(`Renderer: unknown partition '${opts.partition}' (tiles | samples)`);
    if (opts.partition === 'samples' && this.accumulation !== 'sum' && this.devices && this.devices.length > 1)
      throw new Error("Renderer: partition 'samples' needs accumulation 'sum' (a running mean cannot be split by samples)");
    this.aov = opts.aov !== false;
    this.display = opts.display === undefined ? !!this.canvas : !!opts.display;
    // camera-motion reprojection, off by default: true, or {cap, posTol, moments} (left out: sail_temporal_defaults' 32 and
    // 0.05, no moment tracking)
    this.temporal = opts.temporal ? Object.assign({}, opts.temporal === true ? {} : opts.temporal) : null;
    // temporal: {objects: true | {histCap}}: a drag keeps the history (sail_move_objects). histCap is the count a history
    // that crosses a move is clamped to, so that the new samples take over the changed shadows and reflections; its
    // default, 8, is a policy value, not a tuned one (0: no clamp).
    this.objectHistCap = null;
    if (this.temporal && this.temporal.objects) {
      const h = this.temporal.objects === true ? undefined : this.temporal.objects.histCap;
      this.objectHistCap = h === undefined ? 8 : h;
    }
    if (this.temporal && this.accumulation === 'compat8')
      throw new Error("Renderer: temporal needs accumulation 'sum' or 'mix' (8-bit frames carry no sample count)");
    this.lib = native.load();
    const flags = (this.aov ? 1 : 0) | 2;
    this.ctx = this.devices ? this.lib.createMulti(this.width, this.height, Int32Array.from(this.devices), flags)
      : this.lib.create(this.width, this.height, this.device, flags);
    if (opts.partition === 'samples') this.lib.setPartition(this.ctx, 0, 1, 1);
    this.lib.setAccumMode(this.ctx, ACCUM[this.accumulation]);
    // update() links the scene's program in the background (a hipRTC build takes seconds, the reference's GL link
    // milliseconds: renderer.js:45-52); until it is loaded render() uses the precompiled kernel of the scene's plugin
    // set, with identical frames. waitKernel (ms, -1 = until built) makes each launch wait for it instead [0].
    if (opts.waitKernel !== undefined) this.lib.setDebug(this.ctx, 10, opts.waitKernel);
    // temporal: {moments: true} tracks the luminance moments beside the colour history, for temporalFilter()
    if (this.temporal && this.temporal.moments) this.lib.temporalMoments(this.ctx, true);
    this.timeStart = Date.now();
    this.filter = filterConfig({ name: 'color', params: {} });
    this.pixels = null;
    this.n = 0;
    this._temporalView = false;  // a temporalBegin has made a view current since the last scene change
    // the albedo map (sail_albedo): the view last rendered or begun, and the view and grid the context's map was made for
    // (null: none, or the rows have changed since)
    this._view = null;
    this._albedoKey = null;
    // the guide maps (sail_guides): the view and depth the context's maps were made for (null as above)
    this._guidesKey = null;
  }

  update(scene) {
    // the picker (Control / Pickup) finds the renderer that holds this scene on the device
    Object.defineProperty(scene, 'renderer', { value: this, writable: true, configurable: true, enumerable: false });
    this.filter = filterConfig(scene.rendererConfig().filter);
    const s = scene.serialize();
    this.lib.setScene(this.ctx, s.objects, s.n, s.texparams, s.tn, s.lights, s.ln, masksOf(scene.tracerConfig()));
    this.n = s.n;
    scene.sampleCount = 0;
    this._temporalView = false;  // a new scene drops the temporal state
    this._albedoKey = null;      // and the albedo map
    this._guidesKey = null;      // and the guide maps
  }

  updateObjects(scene) {
    this._albedoKey = null;  // new rows drop the albedo map, whichever call brings them
    this._guidesKey = null;  // and the guide maps
    if (this.objectHistCap !== null) {
      // the motion first: serializeObjects applies and zeroes it. The current view stays; the _restart that follows begins
      // the same view again with the motion pending
      const motion = scene.objectMotion();
      this.lib.moveObjects(this.ctx, scene.serializeObjects(), this.n, motion, this.objectHistCap);
      return;
    }
    this.lib.updateObjects(this.ctx, scene.serializeObjects(), this.n);
    this._temporalView = false;  // so do moved objects: a drag drops the history
  }

  _mvp(scene) { return rowMajor(scene.mat); }
  // remember the view the frame belongs to: denoise({albedo}) and temporalFilter({albedo}) compute the map for it
  _see(scene) { this._view = { mvp: this._mvp(scene), eye: Float32Array.from(scene.eye.elements) }; }

  // the frame restarts (the reference's textureWeight 0); with the temporal option the new view takes over the history
  _restart(scene) {
    this._see(scene);
    this.lib.reset(this.ctx);
    if (this.temporal) this.temporalBegin(scene);
  }

  render(scene) {
    if (scene.moving) {
      scene.sampleCount = 0;
      this.updateObjects(scene);
    }
    if (scene.sampleCount === 0) this._restart(scene);  // textureWeight 0: the frame restarts
    const k = scene.sampleCount++;
    const mvp = this._mvp(scene);
    const eye = Float32Array.from(scene.eye.elements);
    let inv, seed;
    if (this.deterministic) {
      const sch = this.lib.schedule(mvp, this.width, this.height, k, 1);
      inv = sch.inv; seed = sch.seeds[0];
    } else {
      inv = this.lib.jitterInverse(mvp, Math.random() * 2 - 1, Math.random() * 2 - 1, this.width, this.height);
      seed = (Date.now() - this.timeStart) * 0.001;
    }
    this.lib.render(this.ctx, inv, eye, seed, this.maxBounces);
    if (this.display) this.present();
  }

  // many samples in one launch sequence, deterministic schedule k0 .. k0+spp-1
  renderSamples(scene, spp) {
    if (scene.moving) { scene.sampleCount = 0; this.updateObjects(scene); }
    if (scene.sampleCount === 0) this._restart(scene);
    const sch = this.lib.schedule(this._mvp(scene), this.width, this.height, scene.sampleCount, spp);
    this.lib.renderSchedule(this.ctx, sch.inv, sch.seeds, Float32Array.from(scene.eye.elements), this.maxBounces);
    scene.sampleCount += spp;
    if (this.display) this.present();
  }

  // Render the deterministic schedule until the frame's noise estimate is at most `noise` or maxSpp samples are in
  // (sail_render_until: looks at minSpp, then at every doubling). Moving scenes and a zero sampleCount restart the
  // frame as in renderSamples. Returns {k, mean, maxTile, converged, history: [{k, mean, maxTile}]}.
  renderUntil(scene, { noise, minSpp = 16, maxSpp = 65536 } = {}) {
    if (typeof noise !== 'number' || Number.isNaN(noise)) throw new Error('Renderer.renderUntil: noise (the target) must be a number');
    if (scene.moving) { scene.sampleCount = 0; this.updateObjects(scene); }
    if (scene.sampleCount === 0) this._restart(scene);
    let r;
    try {
      r = this.lib.renderUntil(this.ctx, this._mvp(scene), Float32Array.from(scene.eye.elements), this.maxBounces,
        noise, minSpp, maxSpp);
    } catch (e) {
      // looks rendered before the failure stay in the frame: keep the scene's count at the context's, so that the next
      // render continues the schedule instead of drawing the same sample indices again
      try { scene.sampleCount = this.lib.stats(this.ctx).samples; } catch (e2) { /* the first error is the one to report */ }
      throw e;
    }
    scene.sampleCount = r.k;
    if (this.display) this.present();
    return { k: r.k, mean: r.mean, maxTile: r.maxTile, converged: r.converged, history: r.history };
  }
  // renderUntil with adaptive sampling (sail_render_adaptive): at every look the 64x64 tiles whose own error is at most
  // `noise` are frozen (with dilate, the default, only when no tile beside them is still noisy) and the rest renders on,
  // until no tile is active or maxSpp samples are in. Options left out keep the library's defaults (minSpp 16, maxSpp
  // 1024, dilate true). Returns {k, mean, maxTile, converged, history, activeTiles, tilesX, tilesY (64x64 tiles),
  // pixelSamples (traced), framePixelSamples (what renderUntil would have traced), traceMs, tileSamples: Uint32Array (the
  // sample count each tile holds, row 0 = bottom)}. The mask stays set until the frame restarts: see getActiveTiles().
  renderAdaptive(scene, { noise, minSpp, maxSpp, dilate } = {}) {
    if (typeof noise !== 'number' || Number.isNaN(noise)) throw new Error('Renderer.renderAdaptive: noise (the target) must be a number');
    if (this.accumulation !== 'sum')
      throw new Error("Renderer.renderAdaptive needs accumulation 'sum': the tiles of its frame hold different sample counts");
    if (scene.moving) { scene.sampleCount = 0; this.updateObjects(scene); }
    if (scene.sampleCount === 0) this._restart(scene);
    let r;
    try {
      r = this.lib.renderAdaptive(this.ctx, this._mvp(scene), Float32Array.from(scene.eye.elements), this.maxBounces,
        noise, minSpp, maxSpp, dilate === undefined ? undefined : (dilate ? 1 : 0));
    } catch (e) {
      // as renderUntil: the looks rendered before the failure stay in the frame
      try { scene.sampleCount = this.lib.stats(this.ctx).samples; } catch (e2) { /* the first error is the one to report */ }
      throw e;
    }
    scene.sampleCount = this.lib.stats(this.ctx).samples;
    if (this.display) this.present();
    return { k: scene.sampleCount, mean: r.mean, maxTile: r.maxTile, converged: r.converged, history: r.history,
      activeTiles: r.activeTiles, tilesX: r.tiles64X, tilesY: r.tiles64Y, pixelSamples: r.pixelSamples,
      framePixelSamples: r.framePixelSamples, traceMs: r.traceMs, tileSamples: r.tileSamples };
  }
  // The mask over the frame's 64x64 tiles (sail_set_active_tiles): one entry per tile, row 0 = bottom, truthy = traced;
  // null or undefined removes it. Everything that restarts the frame removes it too.
  setActiveTiles(active) {
    if (active === null || active === undefined) { this.lib.setActiveTiles(this.ctx, null); return; }
    this.lib.setActiveTiles(this.ctx, Uint8Array.from(active, (v) => (v ? 1 : 0)));
  }
  getActiveTiles() { return this.lib.getActiveTiles(this.ctx); }
  // the noise estimate by hand: noiseMark() snapshots the frame, noise() compares the frame with the snapshot
  // ({mean, maxTile, k, kMark, nonfinite, tilesX, tilesY, kernelMs, tileErr?}); remark moves the mark to now
  noiseMark() { this.lib.noiseMark(this.ctx); }
  noise({ remark = false, tiles = false } = {}) { return this.lib.noise(this.ctx, !!remark, !!tiles); }

  // The variance-guided a-trous denoiser over the frame, the noise mark and the AOV maps (sail_denoise): needs a mark with
  // samples after it (noiseMark(), or a renderUntil that made a second look). Options left out keep the library's
  // defaults (4 passes, sigmaL 1, sigmaX 0.2, display 'color', gamma 2.2); display ('color' | 'gamma' | 'tonemapping')
  // asks for rgba8 as well. Returns {rgba: Float32Array (the denoised mean, row 0 = bottom), rgba8?, info: {k, kMark,
  // nonfinite, iterations, kernelMs, passMs}}. The frame itself is not changed.
  // albedo: true, or {amin, grid}: the frame is divided by the albedo map of its view before the filter and multiplied
  // by it afterwards, so that procedural textures survive (sail_denoise_albedo); the map is computed here when the
  // context has none for this view and grid.
  // guides: true, or {depth}: the filter reads the guide maps of the frame's view in the AOVs' place (sail_use_guides), so
  // that a mirror or a pane of glass is filtered by the surface it shows; the maps are computed here when the context has
  // none for this view and depth. No aov: true is needed then.
  denoise({ iterations, sigmaL, sigmaX, display, gamma, albedo, guides } = {}) {
    if (!this.aov && !guides)
      throw new Error('Renderer.denoise reads the normal and position AOVs: create the Renderer with aov: true, or pass guides');
    const kinds = { color: 0, gamma: 1, tonemapping: 2 };
    let kind;
    if (display !== undefined) {
      kind = typeof display === 'number' ? display : kinds[display];
      if (kind === undefined) throw new Error(`Renderer.denoise: unknown display '${display}' (color | gamma | tonemapping)`);
    }
    this._useGuides(guides);
    if (albedo) return this.lib.denoise(this.ctx, iterations, sigmaL, sigmaX, kind, gamma, display !== undefined, this._albedoFor(albedo));
    return this.lib.denoise(this.ctx, iterations, sigmaL, sigmaX, kind, gamma, display !== undefined);
  }

  // The guide maps of a view (sail_guides): per pixel the normal and position of the first surface that scatters, reached
  // through at most `depth` (0..8; 4 is a policy value) mirror or smooth-glass surfaces, kept by the context for
  // denoise({guides}) and temporalFilter({guides}). `scene` left out: the view last rendered. Returns {n, x: Float32Array
  // (4 per pixel: the AOVs' encodings; n.w the depth walked, x.w the object row, -1 = miss), hitPixels, followedPixels,
  // truncatedPixels, depth, maxDepth, kernelMs}.
  guides(scene, { depth = 4 } = {}) {
    if (scene) this._see(scene);
    if (!this._view) throw new Error('Renderer.guides: no view yet (pass the scene, or render first)');
    this._guidesKey = null;
    const r = this.lib.guides(this.ctx, this._view.mvp, this._view.eye, depth);
    this._guidesKey = this._viewKey(depth);
    return r;
  }
  // set the context's switch for the filter call that follows; computes the maps first when they are stale
  _useGuides(opt) {
    if (!opt) { this.lib.useGuides(this.ctx, false); return; }
    const depth = opt === true || opt.depth === undefined ? 4 : opt.depth;
    if (!this._view) throw new Error('Renderer: the guides option needs a rendered view');
    if (this._guidesKey !== this._viewKey(depth)) this.guides(null, { depth });
    this.lib.useGuides(this.ctx, true);
  }

  // The albedo map of a view (sail_albedo): the mean surface colour of the first hits of grid x grid sub-pixel rays per
  // pixel (grid 1..4; 2 is a policy value), kept by the context for the demodulated filters. `scene` left out: the view
  // last rendered. Returns {rgba: Float32Array (.w: the rays that hit; (1, 1, 1, 0) where none did), hitPixels,
  // partialPixels, grid, kernelMs}.
  albedo(scene, { grid = 2 } = {}) {
    if (scene) this._see(scene);
    if (!this._view) throw new Error('Renderer.albedo: no view yet (pass the scene, or render first)');
    this._albedoKey = null;
    const r = this.lib.albedo(this.ctx, this._view.mvp, this._view.eye, grid);
    this._albedoKey = this._viewKey(grid);
    return r;
  }
  _viewKey(grid) { return `${grid}|${Array.from(this._view.mvp).join(',')}|${Array.from(this._view.eye).join(',')}`; }
  // the amin of a demodulated call; computes the map first when it is stale
  _albedoFor(opt) {
    const o = opt === true ? {} : opt;
    const grid = o.grid === undefined ? 2 : o.grid;
    if (!this._view) throw new Error('Renderer: the albedo option needs a rendered view');
    if (this._albedoKey !== this._viewKey(grid)) this.albedo(null, { grid });
    return o.amin === undefined ? ALBEDO_AMIN : o.amin;
  }

  // The G-buffer pass of the scene's view (sail_gbuffer): {id: Int32Array (object row of each pixel's first hit, -1 = miss),
  // t: Float32Array (its distance, 1e5 on a miss), xyz: Float32Array (its world position, 3 per pixel)}, row 0 = bottom.
  gbuffer(scene) {
    return this.lib.gbuffer(this.ctx, this._mvp(scene), Float32Array.from(scene.eye.elements));
  }
  // "The camera is now at the scene's view" (sail_temporal_begin): the view that was current is committed as the history,
  // which is reprojected into the new view. Returns {k, hitPixels, historyPixels, nonfinite, kernelMs, passMs}.
  temporalBegin(scene) {
    this._see(scene);
    const t = this.temporal || {};
    this._temporalView = false;  // a begin that throws leaves no current view: image() then shows the bare frame
    const info = this.lib.temporalBegin(this.ctx, this._mvp(scene), Float32Array.from(scene.eye.elements), t.cap, t.posTol);
    this._temporalView = true;
    return info;
  }
  // Blend the reprojected history with the samples of the current view (sail_temporal_resolve). display ('color' | 'gamma'
  // | 'tonemapping', default 'color') and gamma choose the RGBA8 transform. Returns {rgba: Float32Array (colour and
  // effective sample count), rgba8, info}. The frame itself is not changed.
  temporalResolve({ display, gamma } = {}) {
    const kinds = { color: 0, gamma: 1, tonemapping: 2 };
    let kind;
    if (display !== undefined) {
      kind = typeof display === 'number' ? display : kinds[display];
      if (kind === undefined) throw new Error(`Renderer.temporalResolve: unknown display '${display}' (color | gamma | tonemapping)`);
    }
    const t = this.temporal || {};
    return this.lib.temporalResolve(this.ctx, t.cap, t.posTol, kind, gamma, true);
  }
  // The a-trous passes over the resolved picture of the current view, steered by the variance of the tracked luminance
  // moments (sail_temporal_filter): needs the option temporal: {moments: true}, aov: true, and a temporalResolve of the
  // current view. Options left out keep the library's defaults (4 passes, sigmaL 4, sigmaX 0.2, minHist 4, display
  // 'color', gamma 2.2); display asks for rgba8 as well. Returns {rgba: Float32Array (row 0 = bottom), rgba8?, info: {k,
  // temporalPixels, spatialPixels, nonfinite, iterations, kernelMs, passMs}}. Neither the frame nor the history changes.
  // albedo: true, or {amin, grid}: as in denoise (sail_temporal_filter_albedo); the history stays un-demodulated.
  // guides: true, or {depth}: as in denoise; reprojection keeps using the first hit.
  temporalFilter({ iterations, sigmaL, sigmaX, minHist, display, gamma, albedo, guides } = {}) {
    if (!this.aov && !guides)
      throw new Error('Renderer.temporalFilter reads the normal and position AOVs: create the Renderer with aov: true, or pass guides');
    if (!(this.temporal && this.temporal.moments))
      throw new Error('Renderer.temporalFilter needs the tracked moments: create the Renderer with temporal: {moments: true}');
    const kinds = { color: 0, gamma: 1, tonemapping: 2 };
    let kind;
    if (display !== undefined) {
      kind = typeof display === 'number' ? display : kinds[display];
      if (kind === undefined) throw new Error(`Renderer.temporalFilter: unknown display '${display}' (color | gamma | tonemapping)`);
    }
    this._useGuides(guides);
    if (albedo)
      return this.lib.temporalFilter(this.ctx, iterations, sigmaL, sigmaX, minHist, kind, gamma, display !== undefined, this._albedoFor(albedo));
    return this.lib.temporalFilter(this.ctx, iterations, sigmaL, sigmaX, minHist, kind, gamma, display !== undefined);
  }

  // the display pass: pixelFilter over the accumulated frame -> RGBA8 (row 0 = bottom, GL order); with the temporal option
  // and a pointwise filter (color, gamma, tonemapping) the resolve's RGBA8 of the same transform
  image() {
    const f = this.filter;
    if (f.aov && !this.aov) throw new Error('this display filter reads the AOVs: create the Renderer with aov: true');
    if (this.temporal && this._temporalView && f.kind <= 2)
      return this.lib.temporalResolve(this.ctx, this.temporal.cap, this.temporal.posTol, f.kind, f.gamma, false).rgba8;
    return this.lib.filter(this.ctx, f.kind, f.weights, f.rx, f.ry, f.gamma).rgba8;
  }

  present() {
    this.pixels = this.image();
    if (this.canvas) {
      const g = this.canvas.getContext('2d');
      if (g && typeof g.createImageData === 'function') {
        const img = g.createImageData(this.width, this.height);
        const rowBytes = this.width * 4;
        for (let y = 0; y < this.height; y++) {  // GL rows are bottom-up, canvas rows top-down
          img.data.set(this.pixels.subarray((this.height - 1 - y) * rowBytes, (this.height - y) * rowBytes), y * rowBytes);
        }
        g.putImageData(img, 0, 0);
      }
    }
    return this.pixels;
  }

  // Pickup.pick on the GPU: the trace kernel's primitive sweep for one ray -> {index (object row, -1 = miss), t}
  pick(origin, dir) {
    const rays = Float32Array.from([...origin, ...dir]);
    const r = this.lib.pick(this.ctx, rays);
    return { index: r.index[0], t: r.t[0] };
  }
  // many rays at once: Float32Array of 6 floats per ray -> {index: Int32Array, t: Float32Array}
  pickRays(rays) { return this.lib.pick(this.ctx, rays); }

  // checkpoint of a progressive render: {k: samples so far, parts: [Float32Array accumulator per device],
  // width, height}; load() into a renderer of the same size, scene, devices and accumulation continues it bit for bit
  save() {
    const ck = this.lib.saveAccum(this.ctx);
    return { k: ck.k, parts: ck.parts, width: this.width, height: this.height, accumulation: this.accumulation };
  }
  // Order: update(scene) first (it resets the accumulation), then load(ckpt, scene): the scene is required, because
  // its sampleCount must become k, or the next render() would restart the accumulation and drop the loaded samples.
  load(ckpt, scene) {
    if (!scene) throw new Error('Renderer.load(ckpt, scene): the scene is required (its sampleCount continues at ckpt.k)');
    if (ckpt.width !== this.width || ckpt.height !== this.height) throw new Error('Renderer.load: checkpoint size differs');
    if (ckpt.accumulation && ckpt.accumulation !== this.accumulation) throw new Error('Renderer.load: accumulation mode differs');
    if (ckpt.frame) this.lib.loadAccum(this.ctx, -1, ckpt.frame, ckpt.k);
    else ckpt.parts.forEach((p, i) => this.lib.loadAccum(this.ctx, i, p, ckpt.k));
    scene.sampleCount = ckpt.k;  // the next render() draws sample k (its jitter and seed)
  }

  readPixels() { return this.lib.readback(this.ctx, false).rgba; }
  readAccum() { return this.lib.readAccum(this.ctx); }
  readAOV() { const r = this.lib.readback(this.ctx, true); return { normal: r.normal, position: r.position }; }
  stats() { return this.lib.stats(this.ctx); }
  // whether the scene's run-time compiled kernel serves the next render (waiting up to timeoutMs for its build)
  kernelReady(timeoutMs = -1) { return this.lib.kernelReady(this.ctx, timeoutMs); }
  kernelInfo() { return this.lib.kernelInfo(this.ctx); }
  destroy() { if (this.ctx) { this.lib.destroy(this.ctx); this.ctx = null; } }
}

module.exports = { Renderer, masksOf, MAXBOUNCES };
