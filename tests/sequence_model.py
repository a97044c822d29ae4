"""A ledger model of a context's accumulation state and a seeded generator of API call sequences.

The ledger restates the state rules that include/sail_hip.h gives in prose, and nothing from the library's sources: every
rule below cites the header passage it restates. tests/test_sequence_model.py checks the ledger against plain oracle calls
and shows that each rule can be seen to fail (RULES); tests/test_gpu_sequences.py replays the same sequences on a
capi.Context and on the ledger side by side.

A sequence is a list of plain tuples (kind, args..., expected return code), printable as a Python literal and replayable as
is. The op kinds:

    ("schedule", n, rc)                 sail_render_schedule of the frozen schedule's samples k .. k+n-1
    ("frames", m, change, j, rc)        m calls of sail_render; change "none", or "eye" / "bounces": the calls from the j-th on
                                        use the flavour's other eye / one bounce less
    ("launch_samples", v, rc)           sail_set_launch_samples
    ("mask", bytes, rc), ("unmask", rc) sail_set_active_tiles
    ("update_objects", row, sign, rc)   the sphere `row` moved by sign * 0.25 in x, through sail_update_objects
    ("move_objects", row, sign, rc)     the same through sail_move_objects (no temporal state: exactly an update)
    ("set_scene", rc)                   sail_set_scene with the rows the context holds
    ("reset", rc), ("accum_mode", m, rc), ("partition", rank, world, mode, rc)
    ("save_load", rc)                   sail_save_accum of every part, sail_load_accum into the same context
    ("save_load_fresh", rc)             ... into a new context with the same settings, which replaces the old one
    ("mark", rc), ("estimate", remark, rc)
    ("read", rc), ("readback", rc), ("sync", rc), ("stats", rc), ("filter", rc), ("pick", rc), ("gbuffer", rc)
    ("wait_kernel", rc)                 sail_kernel_ready(-1)

Radiance comes from the CPU oracle, one 64x64 tile and one sample at a time (oracle.render's k0, crop, accum and accum_mode),
which gives the bits of one whole-frame call in all three accumulation modes: every pixel's chain of additions is its own.
`fake=True` replaces the oracle by a constant per (rows, sample, eye, bounces): every rule then runs in microseconds, which
the generator and the seed search use; no test compares fake values with anything but other fake values.
"""
import functools
import hashlib
import json
import os

import numpy as np

import oracle
from sail_amd import capi

F = np.float32
OK, E_INVALID, E_STATE = 0, -1, -4
SUM, MIX, COMPAT8 = capi.ACCUM_SUM, capi.ACCUM_MIX, capi.ACCUM_COMPAT8
TILES, SAMPLES = capi.PART_TILES, capi.PART_SAMPLES
LENGTH, MAX_SAMPLES = 24, 64
MOVE = 0.25           # an update moves a sphere row by this much in x
EYE_SHIFT = (0.5, 0.25, 0.0)   # the "other eye" of a frames op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene x context settings; `rows`: the sphere rows an update may move (columns 1..3 of a sphere row are its centre)
FLAVOURS = {
    "cornell":        dict(scene="C1", W=136, H=72, B=5, flags=0, debug={capi.DEBUG_JIT_VALUES_AFTER: 3}, devices=0, rows=(2,)),
    "cornell_aov":    dict(scene="C1", W=136, H=72, B=5, flags=capi.FLAG_AOV, debug={capi.DEBUG_JIT_VALUES_AFTER: 3}, devices=0,
                           rows=(2,)),
    "room":           dict(scene="C3", W=136, H=72, B=5, flags=0, debug={capi.DEBUG_SAMPLE_GROUPS: 0}, devices=0, rows=(2, 3, 4, 5)),
    "room_groups":    dict(scene="C3", W=136, H=72, B=5, flags=0, debug={capi.DEBUG_SAMPLE_GROUPS: 3}, devices=0, rows=(2, 3, 4, 5)),
    "precompiled_c1": dict(scene="C1", W=136, H=72, B=5, flags=0, debug={capi.DEBUG_JIT: 0}, devices=0, rows=(2,)),
    "precompiled_c3": dict(scene="C3", W=136, H=72, B=5, flags=0, debug={capi.DEBUG_JIT: 0}, devices=0, rows=(2, 3, 4, 5)),
    "cull":           dict(scene="C4", W=72, H=40, B=4, flags=0, debug={}, devices=0, rows=(1,)),
    "cull_wavefront": dict(scene="C4", W=72, H=40, B=4, flags=0, debug={capi.DEBUG_WAVEFRONT: 1}, devices=0, rows=(1,)),
    "multi":          dict(scene="C1", W=136, H=72, B=5, flags=0, debug={}, devices=3, rows=(2,)),
}

KINDS = ("schedule", "frames", "launch_samples", "mask", "unmask", "update_objects", "move_objects", "set_scene", "reset",
         "accum_mode", "partition", "save_load", "save_load_fresh", "mark", "estimate", "read", "readback", "sync", "stats",
         "filter", "pick", "gbuffer", "wait_kernel")
PURE_OBSERVERS = ("read", "sync", "stats")   # skipped when adjacency is counted: the GPU test reads after every op anyway
REFUSALS = ("mask in MIX", "sample partition in MIX", "estimate without a mark", "mark in COMPAT8")

# One switch per rule; the ledger with a switch off is a library that broke the rule. Only flushes that a result can show have
# a switch: sync, stats, pick, gbuffer, wait_kernel and launch_samples launch the queue too (the ledger does it
# unconditionally), but samples are added in the same order whenever they are launched and none of these calls returns
# anything of the frame, so no caller could tell a library that forgot them.
RULES = {
    "mask_freezes": True,            # a launch traces the active tiles and nothing else
    "mask_flushes": True,            # sail_set_active_tiles launches queued samples first
    "drop_mask_reset": True,         # each restart removes the mask ...
    "drop_mask_set_scene": True,
    "drop_mask_update_objects": True,
    "drop_mask_move_objects": True,
    "drop_mask_accum_mode": True,
    "drop_mask_partition": True,
    "drop_mask_load": True,
    "load_keeps_mark": True,         # ... and the mark, but sail_load_accum keeps the mark
    "partial_mark": True,            # sail_noise_mark under a mask writes only the active tiles
    "partial_remark": True,          # and so does the remark of sail_noise_estimate
    "flush_read": True,              # the observers whose result depends on the queue launch it first
    "flush_readback": True,
    "flush_filter": True,
    "flush_save": True,
    "flush_mark": True,
    "flush_estimate": True,
    "change_flushes": True,          # a change of eye or bounce count launches the queue before the new sample is queued
    "restart_drops_queue": True,     # a restart drops the queue instead of launching it
    "refusal_changes_nothing": True,
}
_RESTART_RULE = {"reset": "drop_mask_reset", "set_scene": "drop_mask_set_scene", "update_objects": "drop_mask_update_objects",
                 "move_objects": "drop_mask_move_objects", "accum_mode": "drop_mask_accum_mode",
                 "partition": "drop_mask_partition", "load": "drop_mask_load"}


@functools.lru_cache(maxsize=None)
def scenes():
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        return json.load(f)["scenes"]


@functools.lru_cache(maxsize=None)
def sample_args(scene, W, H, k):
    """(inverse matrix, seed) of the frozen schedule's sample k (sail_schedule)"""
    inv, seeds = capi.schedule(np.array(scenes()[scene]["mvp_rowmajor"]), W, H, k, 1)
    return inv[0], float(seeds[0])


@functools.lru_cache(maxsize=None)
def tile_rects(W, H):
    """(x0, y0, w, h) of every 64x64 tile, index t = ty * tilesX + tx, row 0 = bottom (the adaptive section's tile order)"""
    tx, ty = (W + 63) // 64, (H + 63) // 64
    return tuple((i * 64, j * 64, min(64, W - i * 64), min(64, H - j * 64)) for j in range(ty) for i in range(tx))


@functools.lru_cache(maxsize=None)
def own_tiles(W, H, rank, world):
    """the tiles of rank `rank` under a tile partition, from sail_partition_tiles (host only)"""
    tx = (W + 63) // 64
    return tuple(sorted(int(y0) // 64 * tx + int(x0) // 64 for x0, y0, _, _ in capi.partition_tiles(W, H, rank, world)))


def rank_samples(k, rank, world, mode):
    """sail_reduce_plan.samples: how many of the samples 0 .. k-1 this rank rendered"""
    if mode == TILES or world <= 1:
        return k
    return (k - 1 - rank) // world + 1 if k > rank else 0


def digest(*arrays):
    h = hashlib.blake2b(digest_size=8)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def mean_of(S, mode):
    """sail_readback's image: SUM divides each texel by its own count where that is > 0 and sets w = 1; MIX is the mean"""
    m = S.copy()
    if mode == SUM:
        cnt = S[..., 3]
        with np.errstate(all="ignore"):
            m[..., :3] = np.where((cnt > 0)[..., None], S[..., :3] / np.where(cnt > 0, cnt, F(1))[..., None], S[..., :3])
        m[..., 3] = F(1)
    return m


_RADIANCE = {}   # (scene, rows, k, tile, eye, bounces, aov) -> the tile's (radiance + count, normal map, position map)


class _Acc:
    """one accumulator: a context's own, or one device's of a multi-device context"""

    def __init__(self, W, H, aov):
        self.S = np.zeros((H, W, 4), F)
        self.N = np.zeros((H, W, 4), F) if aov else None
        self.X = np.zeros((H, W, 4), F) if aov else None
        self.samples = 0


class Ledger:
    def __init__(self, flavour, rules=None, fake=False):
        fl = FLAVOURS[flavour]
        self.flavour, self.fl, self.fake = flavour, fl, fake
        self.rules = dict(RULES, **(rules or {}))
        self.W, self.H, self.B = fl["W"], fl["H"], fl["B"]
        self.aov = bool(fl["flags"] & capi.FLAG_AOV)
        self.scene = scenes()[fl["scene"]]
        self.masks = capi.plugin_masks(self.scene["plugins"])
        self.rows = np.array(self.scene["objects"], F).reshape(self.scene["n"], 18)
        self.eye = tuple(float(F(v)) for v in self.scene["eye"])
        self.eye2 = tuple(float(F(F(a) + F(b))) for a, b in zip(self.scene["eye"], EYE_SHIFT))
        self.tiles = tile_rects(self.W, self.H)
        self.multi = fl["devices"]
        # sail_create: one accumulator, SUM, partition (0, 1, TILES); sail_create_multi: device i is rank i of N
        self.parts = [(i, self.multi) for i in range(self.multi)] if self.multi else [(0, 1)]
        self.part_mode = TILES
        self.mode = SUM
        self.acc = [_Acc(self.W, self.H, self.aov) for _ in self.parts]
        self.k = 0
        self.mask = None
        self.P, self.have_mark, self.k_mark = None, False, 0
        self.queue = []
        self._restart_aov()

    # ---- what a caller can see ---------------------------------------------------------------------------------------
    def current_scene(self):
        return dict(self.scene, objects=self.rows.reshape(-1).copy())

    def shown(self):
        """The accumulator the context shows. A multi-device context: the devices' accumulators added in rank order,
        ((r0 + r1) + r2), count channel included (sail_create_multi; for a tile partition that is the whole frame)."""
        out = self.acc[0].S.copy()
        with np.errstate(all="ignore"):
            for a in self.acc[1:]:
                out = out + a.S
        return out

    def shown_aov(self):
        """The AOV maps, or None where they are not compared (no SAIL_FLAG_AOV, or a sample partition over several ranks:
        'the shown maps are those of the rank that rendered the frame's last sample')."""
        if not self.aov or (self.part_mode == SAMPLES and self.parts[0][1] > 1):
            return None
        n, x = self.acc[0].N.copy(), self.acc[0].X.copy()
        for a in self.acc[1:]:   # a tile partition: -0 outside each device's tiles, so the sum keeps every bit
            n, x = n + a.N, x + a.X
        return n, x

    def samples(self):
        """sail_stats.samples: this rank's count; a multi-device context reports the frame's samples per pixel"""
        return self.k if self.multi else self.acc[0].samples

    def mask_bytes(self):
        """sail_get_active_tiles: the mask as bytes 0 / 1, all 1 without one"""
        return np.ones(len(self.tiles), np.uint8) if self.mask is None else np.array(self.mask, np.uint8)

    # ---- rendering ---------------------------------------------------------------------------------------------------
    def _rank_tiles(self, rank, world):
        # "which tiles a device traces: one device, the active tiles; SAIL_PART_TILES, its own tiles that are active;
        #  SAIL_PART_SAMPLES, the active tiles for its samples"
        return own_tiles(self.W, self.H, rank, world) if self.part_mode == TILES else tuple(range(len(self.tiles)))

    def _owns_sample(self, k, rank, world):
        return not (self.part_mode == SAMPLES and world > 1 and k % world != rank)

    def _advance(self):
        """the sample index and the ranks' counts move when the call is made (sail_render: 'the sample's record is built
        now, from the sample index it is given now'); a launch without an active tile of its own still advances k"""
        for a, (rank, world) in zip(self.acc, self.parts):
            if self._owns_sample(self.k, rank, world):
                a.samples += 1
        self.k += 1

    def _render(self, k, eye, bounces):
        for a, (rank, world) in zip(self.acc, self.parts):
            if not self._owns_sample(k, rank, world):
                continue
            for t in self._rank_tiles(rank, world):
                # "With a mask set, a launch traces the active tiles of the context's share and nothing else: an inactive
                #  tile's accumulator texels (their sample count in .w included) and AOV texels keep what they held."
                if self.mask is not None and self.rules["mask_freezes"] and not self.mask[t]:
                    continue
                self._trace(a, t, k, eye, bounces)

    def _trace(self, a, t, k, eye, bounces):
        x0, y0, w, h = self.tiles[t]
        ys, xs = slice(y0, y0 + h), slice(x0, x0 + w)
        if self.fake:
            v = F(0.5) + F(int(digest(self.rows, np.array([k, bounces]), np.array(eye)), 16) % 4096) / F(4096)
            e = np.array([v, v / F(2), v / F(4), 1], F)
            if self.mode == SUM:
                a.S[ys, xs] = a.S[ys, xs] + e
            else:
                m = (a.S[ys, xs] * F(k) + e) / F(k + 1)
                a.S[ys, xs] = np.round(m * F(255)) / F(255) if self.mode == COMPAT8 else m
                a.S[ys, xs, 3] = 1
            if self.aov:
                a.N[ys, xs], a.X[ys, xs] = v, -v
            return
        inv, seed = sample_args(self.fl["scene"], self.W, self.H, k)
        crop = (x0, y0, w, h)
        if self.mode == SUM:
            # the sample alone into zeros is its radiance (0 + e) with count 1; S + that is the oracle's own S += e
            key = (self.fl["scene"], self.rows.tobytes(), k, t, eye, bounces, self.aov)
            if key not in _RADIANCE:
                out = oracle.render(self.current_scene(), self.masks, self.W, self.H, inv[None], [seed], eye, bounces, k0=k,
                                    crop=crop, aov=self.aov)
                out = out if self.aov else (out, None, None)
                _RADIANCE[key] = tuple(None if o is None else o[ys, xs].copy() for o in out)
            e, n, x = _RADIANCE[key]
            with np.errstate(all="ignore"):
                a.S[ys, xs] = a.S[ys, xs] + e
        else:
            out = oracle.render(self.current_scene(), self.masks, self.W, self.H, inv[None], [seed], eye, bounces, k0=k,
                                crop=crop, accum=a.S, accum_mode=self.mode, aov=self.aov)
            n, x = (out[1][ys, xs], out[2][ys, xs]) if self.aov else (None, None)
        if self.aov:
            a.N[ys, xs], a.X[ys, xs] = n, x   # "a tile holds the maps of the last sample rendered into it"

    def flush(self):
        """launch the queue: 'every entry point that reads, filters, reduces, counts or changes the context launches the
        queue first' (sail_render). The frame is bit-identical to one launch per call, in the same order."""
        q, self.queue = self.queue, []
        for k, eye, bounces in q:
            if not self.rules["change_flushes"]:   # "a launch has one eye and one bounce count": the last queued ones
                eye, bounces = q[-1][1], q[-1][2]
            self._render(k, eye, bounces)

    # ---- restarts ----------------------------------------------------------------------------------------------------
    def _restart_aov(self):
        # sail_reset: the AOV maps restart at +0; a tile-partitioned rank's maps hold -0 outside its tiles (sail_reduce:
        # '-0 maps, the additive identity')
        for a, (rank, world) in zip(self.acc, self.parts):
            if a.N is None:
                continue
            a.N[:], a.X[:] = 0, 0
            if self.part_mode == TILES and world > 1:
                mine = set(own_tiles(self.W, self.H, rank, world))
                for t, (x0, y0, w, h) in enumerate(self.tiles):
                    if t not in mine:
                        a.N[y0:y0 + h, x0:x0 + w] = F(-0.0)
                        a.X[y0:y0 + h, x0:x0 + w] = F(-0.0)

    def _restart(self, call, keep_mark=False):
        """'everything that restarts the accumulator removes the mask: sail_reset, sail_set_scene, sail_update_objects,
        sail_move_objects, sail_set_accum_mode, sail_set_partition, sail_load_accum'; the same calls but sail_load_accum
        'drop the mark'; queued samples belong to the accumulation that is discarded (sail_reset)."""
        if self.rules["restart_drops_queue"]:
            self.queue = []
        if self.rules[_RESTART_RULE[call]]:
            self.mask = None
        if not keep_mark:
            self.have_mark = False
        for a in self.acc:
            a.S[:] = 0
            a.samples = 0
        self.k = 0
        self._restart_aov()

    def _copy_mark(self, rule="partial_mark"):
        """'sail_noise_mark and the remark of sail_noise_estimate write P only in the 16x16 tiles of active 64x64 tiles ...
        A context without a mark yet marks the whole frame.'"""
        S = self.shown()
        if self.mask is not None and self.have_mark and self.rules[rule]:
            for t, (x0, y0, w, h) in enumerate(self.tiles):
                if self.mask[t]:
                    self.P[y0:y0 + h, x0:x0 + w] = S[y0:y0 + h, x0:x0 + w]
        else:
            self.P = S
        self.have_mark, self.k_mark = True, self.k

    def _refused(self, rc, change):
        """'refused, nothing changed'"""
        if not self.rules["refusal_changes_nothing"]:
            change()
        return {"rc": rc}

    def _world(self):
        return self.parts[0][1]

    # ---- the calls ---------------------------------------------------------------------------------------------------
    def apply(self, kind, *args):
        """one op without its return code; returns {"rc": ..., and what the op lets a caller see}"""
        return getattr(self, "_op_" + kind)(*args)

    def _op_schedule(self, n):
        self.flush()
        for _ in range(n):
            k = self.k
            self._advance()
            self._render(k, self.eye, self.B)
        return {"rc": OK}

    def frame_args(self, i, change, j):
        """(eye, bounces) of call i of a frames op"""
        changed = change != "none" and i >= j
        return (self.eye2 if changed and change == "eye" else self.eye,
                self.B - 1 if changed and change == "bounces" else self.B)

    def _op_frames(self, m, change, j):
        for i in range(m):
            eye, bounces = self.frame_args(i, change, j)
            # "a change of eye or bounce count launches it before the new sample is queued"
            if self.queue and (eye, bounces) != self.queue[-1][1:] and self.rules["change_flushes"]:
                self.flush()
            self.queue.append((self.k, eye, bounces))
            self._advance()
        return {"rc": OK}

    def _op_launch_samples(self, v):
        self.flush()   # it changes the context
        return {"rc": OK}

    def _set_mask(self, m):
        if self.rules["mask_flushes"]:   # "sail_set_active_tiles launches queued samples first, then copies `active`"
            self.flush()
        self.mask = m

    def _op_mask(self, active):
        m = tuple(1 if b else 0 for b in active)
        if self.mode != SUM:   # "SAIL_E_STATE in SAIL_ACCUM_MIX and SAIL_ACCUM_COMPAT8 (no per-pixel count)"
            return self._refused(E_STATE, lambda: self._set_mask(m))
        self._set_mask(m)      # "An all-ones mask is a mask"
        return {"rc": OK}

    def _op_unmask(self):
        if self.mode != SUM:
            return self._refused(E_STATE, lambda: self._set_mask(None))
        self._set_mask(None)
        return {"rc": OK}

    def _move(self, row, sign):
        self.rows = self.rows.copy()
        self.rows[row, 1] = F(self.rows[row, 1] + F(sign * MOVE))

    def _op_update_objects(self, row, sign):
        self._move(row, sign)
        self._restart("update_objects")   # "new object rows, same n; resets accumulation"
        return {"rc": OK}

    def _op_move_objects(self, row, sign):
        self._move(row, sign)
        self._restart("move_objects")     # "restarts ... the accumulator (the noise mark goes) exactly as sail_update_objects"
        return {"rc": OK}

    def _op_set_scene(self):
        self._restart("set_scene")
        return {"rc": OK}

    def _op_reset(self):
        self._restart("reset")
        return {"rc": OK}

    def _set_mode(self, mode):
        self.mode = mode
        self._restart("accum_mode")       # "resets accumulation"

    def _op_accum_mode(self, mode):
        # a running mean cannot be split by samples (sail_set_partition)
        if mode != SUM and self.part_mode == SAMPLES and self._world() > 1:
            return self._refused(E_INVALID, lambda: self._set_mode(mode))
        self._set_mode(mode)
        return {"rc": OK}

    def _set_partition(self, rank, world, mode):
        if not self.multi:
            self.parts = [(rank, world)]
        self.part_mode = mode
        self._restart("partition")

    def _op_partition(self, rank, world, mode):
        # sail_set_partition: SAIL_E_INVALID for a sample partition over more than one rank outside SAIL_ACCUM_SUM
        if mode == SAMPLES and (self.multi or world) > 1 and self.mode != SUM:
            return self._refused(E_INVALID, lambda: self._set_partition(rank, world, mode))
        self._set_partition(rank, world, mode)
        return {"rc": OK}

    def _save(self):
        if self.rules["flush_save"]:
            self.flush()
        return {"rc": OK, "k": self.k, "parts": [a.S.copy() for a in self.acc]}

    def _load(self, ckpt):
        """sail_load_accum: 'replace accumulator `part` by `sums` and set the sample index to k'; it removes the mask and
        'keeps [the mark] (a loaded checkpoint continues a render)'; 'the AOVs restart with the next sample'."""
        self._restart("load", keep_mark=self.rules["load_keeps_mark"])
        for a, s, (rank, world) in zip(self.acc, ckpt["parts"], self.parts):
            a.S[:] = s
            a.samples = rank_samples(ckpt["k"], rank, world, self.part_mode)
        self.k = ckpt["k"]

    def _op_save_load(self):
        out = self._save()
        self._load(out)
        return out

    def _op_save_load_fresh(self):
        out = self._save()
        self._load(out)
        self.have_mark, self.mask = False, None   # a new context has no mark and no mask, whatever a load does
        return out

    def _op_mark(self):
        if self.mode == COMPAT8:   # "SAIL_ACCUM_COMPAT8 is refused (SAIL_E_STATE)"
            return self._refused(E_STATE, self._copy_mark)
        if self.rules["flush_mark"]:
            self.flush()
        self._copy_mark()
        return {"rc": OK}

    def _op_estimate(self, remark):
        if self.mode == COMPAT8:
            return {"rc": E_STATE}
        if self.rules["flush_estimate"]:
            self.flush()
        # "SAIL_E_STATE without a mark or with no sample since it"
        if not self.have_mark or self.k <= self.k_mark:
            return {"rc": E_STATE}
        out = {"rc": OK, "S": self.shown(), "P": self.P.copy(), "mix": self.mode == MIX, "k": self.k, "k_mark": self.k_mark}
        if remark:   # "remark != 0 also sets the mark to the current accumulator in the same pass"
            self._copy_mark("partial_remark")
        return out

    def _observe(self, rule):
        if rule is None or self.rules[rule]:
            self.flush()

    def _op_read(self):
        self._observe("flush_read")
        return {"rc": OK, "frame": self.shown()}

    def _op_readback(self):
        self._observe("flush_readback")
        return {"rc": OK, "mean": mean_of(self.shown(), self.mode), "aov": self.shown_aov()}

    def _op_filter(self):
        self._observe("flush_filter")
        S = self.shown()
        m = mean_of(S, self.mode)
        m[..., 3] = S[..., 3]
        return {"rc": OK, "mean": m}

    def _op_sync(self):
        self._observe(None)
        return {"rc": OK}

    def _op_stats(self):
        self._observe(None)
        return {"rc": OK, "samples": self.samples()}

    def _op_pick(self):
        self._observe(None)
        return {"rc": OK}

    def _op_gbuffer(self):
        self._observe(None)
        return {"rc": OK}

    def _op_wait_kernel(self):
        return {"rc": OK}

    def state(self):
        """what the GPU test compares after an op: the shown frame (launches the queue), k, the count, the mask"""
        self.flush()
        return {"frame": self.shown(), "k": self.k, "samples": self.samples(), "mask": self.mask_bytes(),
                "aov": self.shown_aov()}


def refusal_of(op, led_before):
    """which of REFUSALS an op with a negative return code is (None: another refusal the rules imply)"""
    kind = op[0]
    if kind in ("mask", "unmask") and led_before["mode"] == MIX:
        return REFUSALS[0]
    if kind == "partition" and led_before["mode"] == MIX:
        return REFUSALS[1]
    if kind == "estimate" and led_before["mode"] != COMPAT8 and not led_before["have_mark"]:
        return REFUSALS[2]
    if kind == "mark" and led_before["mode"] == COMPAT8:
        return REFUSALS[3]
    return None


def op_samples(op):
    return op[1] if op[0] in ("schedule", "frames") else 0


def pick_rays(eye):
    """the 4 rays of a pick op: from the eye, around +z"""
    d = np.array([(0, 0, 1), (0.2, 0.1, 1), (-0.3, 0.2, 1), (0.05, -0.35, 1)], F)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(F)
    return np.concatenate([np.tile(np.array(eye, F), (4, 1)), d], 1)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def _draw(kind, rng, led):
    fl = led.fl
    if kind == "schedule":
        return (kind, int(rng.choice([1, 2, 3, 7], p=[0.35, 0.3, 0.25, 0.1])))
    if kind == "frames":
        m = int(rng.choice([1, 2, 5], p=[0.35, 0.4, 0.25]))
        return (kind, m, str(rng.choice(["none", "eye", "bounces"], p=[0.5, 0.25, 0.25])), int(rng.integers(0, m)))
    if kind == "launch_samples":
        return (kind, int(rng.choice([0, 1, 2, 32])))
    if kind == "mask":
        n = len(led.tiles)
        how = rng.random()
        rank, world = led.parts[0]
        if how < 0.2:
            m = [1] * n                                        # an all-ones mask is a mask
        elif how < 0.4 and not led.multi and led.part_mode == TILES and world > 1:
            mine = set(own_tiles(led.W, led.H, rank, world))   # none of this rank's own tiles
            m = [0 if t in mine else 1 for t in range(n)]
        else:
            m = [int(b) for b in rng.integers(0, 2, n)]
            m[int(rng.integers(0, n))] = 1                     # at least one active tile
        return (kind, tuple(m))
    if kind in ("update_objects", "move_objects"):
        return (kind, int(rng.choice(fl["rows"])), int(rng.choice([-1, 1])))
    if kind == "accum_mode":
        return (kind, int(rng.choice([SUM, MIX, COMPAT8], p=[0.6, 0.25, 0.15] if led.mode != SUM else [0.4, 0.35, 0.25])))
    if kind == "partition":
        mode = int(rng.choice([TILES, SAMPLES]))
        if led.multi:
            return (kind, 0, 1, mode)   # all a multi-device context accepts
        world = int(rng.choice([1, 2, 3]))
        return (kind, int(rng.integers(0, world)), world, mode)
    if kind == "estimate":
        return (kind, bool(rng.random() < 0.5))
    return (kind,)


ACTIVE = tuple(k for k in KINDS if k not in PURE_OBSERVERS)
_RENDERS = ("schedule", "frames")


@functools.lru_cache(maxsize=None)
def circuit(number):
    """A closed walk over the kinds but the pure observers that takes every ordered pair (a, b), a == b included, once, and
    every pair with a render op on one side only twice (so that sequences render often): an Euler circuit of that multigraph
    (every kind has as many edges in as out), found by Hierholzer's walk with the edges shuffled by `number`."""
    rng = np.random.default_rng([0x5A11, int(number)])
    out = {a: list(ACTIVE) + ([k for k in ACTIVE if k not in _RENDERS] if a in _RENDERS else list(_RENDERS)) for a in ACTIVE}
    for a in ACTIVE:
        rng.shuffle(out[a])
    stack, walk = [ACTIVE[int(rng.integers(len(ACTIVE)))]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert walk[0] == walk[-1] and len(walk) == len(ACTIVE) ** 2 + 4 * (len(ACTIVE) - 2) + 1
    return tuple(walk[:-1])


def segments(length=LENGTH):
    """(pure observers per sequence, sequences that cover one circuit)"""
    pure = min(2, length // 10)
    stride = max(1, length - pure - 1)
    return pure, -(-len(circuit(0)) // stride)


FREE = 1000   # seeds from here on walk freely
_RESTARTS = ("update_objects", "move_objects", "set_scene", "reset", "accum_mode", "partition", "save_load_fresh")
_WEIGHT = {"schedule": 3.0, "frames": 3.0, "mask": 2.0, "mark": 2.0, "estimate": 2.0, "save_load": 1.5, "read": 0.7, "sync": 0.4,
           "stats": 0.4}


def _free_walk(rng, flavour, length):
    """Kinds drawn one by one, steered by the state: an empty accumulator is rendered into first, and while the context
    holds a mask or a mark the calls that would drop them are drawn less often, so that the rules about a mask and a mark
    together, which need six or seven calls in order, are met."""
    led = Ledger(flavour, fake=True)
    seq, total = [], 0
    while len(seq) < length:
        held = led.mask is not None or led.have_mark
        w = np.array([_WEIGHT.get(k, 1.0) * (0.25 if held and k in _RESTARTS + ("unmask",) else 1.0) for k in KINDS])
        if led.k == 0:
            w[[KINDS.index(k) for k in _RENDERS]] *= 4.0
        op = _draw(KINDS[int(rng.choice(len(KINDS), p=w / w.sum()))], rng, led)
        if total + op_samples(op) > MAX_SAMPLES:
            op = ("reset",)
        total += op_samples(op)
        seq.append(op + (led.apply(*op)["rc"],))
    return seq


def make_sequence(seed, flavour, length=LENGTH):
    """`length` ops for `flavour`, deterministic in the arguments. Seeds from FREE on: _free_walk. Below, the kinds follow circuit number seed // n from its
    (seed % n)-th stretch on, n = segments(length)[1], so the seeds c n .. c n + n - 1 of any one c put every ordered pair of
    kinds side by side; two pure observers stand at drawn places. The arguments are drawn. The samples rendered stay at
    MAX_SAMPLES by drawing a reset instead, and each op's return code comes from a ledger over constant radiance, which
    holds the same state as any other."""
    rng = np.random.default_rng([int(seed), sorted(FLAVOURS).index(flavour), int(length)])
    if int(seed) >= FREE:
        return _free_walk(rng, flavour, length)
    pure, n = segments(length)
    walk = circuit(int(seed) // n)
    start = (int(seed) % n) * max(1, length - pure - 1)
    kinds = [walk[(start + i) % len(walk)] for i in range(length - pure)]
    for _ in range(pure):
        kinds.insert(int(rng.integers(1, len(kinds) + 1)), str(rng.choice(PURE_OBSERVERS)))
    led = Ledger(flavour, fake=True)
    seq, total = [], 0
    for kind in kinds:
        op = _draw(kind, rng, led)
        if total + op_samples(op) > MAX_SAMPLES:
            op = ("reset",)
        total += op_samples(op)
        seq.append(op + (led.apply(*op)["rc"],))
    return seq


def adjacent_pairs(seq):
    """ordered pairs of kinds that stand side by side once the pure observers are skipped"""
    kinds = [op[0] for op in seq if op[0] not in PURE_OBSERVERS]
    return set(zip(kinds, kinds[1:]))


# ---- replay on the ledger alone ---------------------------------------------------------------------------------------------
def _seen(out):
    return tuple((key, digest(v) if isinstance(v, np.ndarray) else
                  (None if v is None else (tuple(digest(a) for a in v) if isinstance(v, (list, tuple)) else v)))
                 for key, v in sorted(out.items()))


def replay(flavour, seq, rules=None, fake=False, eager=False):
    """What a caller sees of `seq` on the ledger: per op its return code and what the op returns, with `eager` also the state
    after every op, and the state at the end. Returns (observations, ledger, refusals met)."""
    led = Ledger(flavour, rules=rules, fake=fake)
    seen, refusals = [], []
    for op in seq:
        before = {"mode": led.mode, "have_mark": led.have_mark}
        out = led.apply(*op[:-1])
        if rules is None:
            assert out["rc"] == op[-1], f"{op}: the ledger returns {out['rc']}"
        if out["rc"] < 0:
            refusals.append(refusal_of(op, before))
        seen.append((op[0],) + _seen(out))
        if eager:
            seen.append(_seen(led.state()))
    seen.append(_seen(led.state()))   # the mark itself is seen through an estimate only, here as on a context
    return seen, led, refusals


# ---- the committed table -----------------------------------------------------------------------------------------------------
# (flavour, seed): chosen by `PYTHONPATH=. python tests/sequence_model.py` (search_table below) so that tests/test_sequence_model.py's
# coverage conditions hold: every ordered pair of the kinds but the pure observers adjacent somewhere, every kind 5 times,
# every refusal twice, every flavour, and every rule seen to bite through what a caller sees (frames, estimates, k, return codes).
# The first 23 are the stretches of circuit 0; no smaller table puts 400 pairs side by side in sequences of 24 ops. The free
# walks add the rules that need a mask and a mark held over several calls and an estimate after them.
# the flavours of circuit 0's stretches: the cheap scene most often, every flavour at least once
_PATTERN = ("cornell", "multi", "cornell_aov", "precompiled_c1", "room", "cornell", "multi", "cornell_aov", "cull", "cornell",
            "multi", "precompiled_c1", "room_groups", "cornell_aov", "cornell", "multi", "precompiled_c3", "cornell",
            "cornell_aov", "cull_wavefront", "multi", "precompiled_c1", "cornell")
# what search_table adds to them
FREE_SEEDS = [("cornell", 1105), ("cornell", 1001), ("cornell", 1035), ("multi", 1109), ("cornell_aov", 1277), ("multi", 1000),
              ("multi", 1007)]
SEEDS = [(f, i) for i, f in enumerate(_PATTERN)] + FREE_SEEDS


def table_items(flavour, seed):
    """what a sequence adds to the table's coverage: its adjacent pairs, its refusals, the rules that bite on it (over
    constant radiance), an all-ones mask and a mask without a tile of the rank's own"""
    seq = make_sequence(seed, flavour)
    base, _, refusals = replay(flavour, seq, fake=True)
    items = [("pair",) + p for p in adjacent_pairs(seq)] + [("flavour", flavour)]
    items += [("refusal", r, i) for r in REFUSALS for i in range(refusals.count(r))]
    items += [("rule", r) for r in RULES if replay(flavour, seq, rules={r: False}, fake=True)[0] != base]
    led = Ledger(flavour, fake=True)
    for op in seq:
        if op[0] == "mask" and op[-1] == OK:
            rank, world = led.parts[0]
            if all(op[1]):
                items.append(("mask", "all ones"))
            if not led.multi and led.part_mode == TILES and world > 1 and not any(op[1][t] for t in own_tiles(led.W, led.H, rank, world)):
                items.append(("mask", "none of its own"))
        led.apply(*op[:-1])
    return items


def search_table(free=300, log=print):
    """Circuit 0's stretches with _PATTERN's flavours, then, greedily, the cheap-scene free walks that
    add the most of what is still missing (refusals twice, every rule, both special masks)."""
    n = segments()[1]
    assert len(_PATTERN) == n
    need = {("pair", a, b) for a in ACTIVE for b in ACTIVE} | {("flavour", f) for f in FLAVOURS} | {("rule", r) for r in RULES}
    need |= {("refusal", r, i) for r in REFUSALS for i in range(2)} | {("mask", "all ones"), ("mask", "none of its own")}
    have = {}

    def add(key, items):
        for it in items:
            if it[0] == "refusal":   # counted over the table
                have[it[1]] = have.get(it[1], 0) + 1
                it = ("refusal", it[1], have[it[1]] - 1)
            need.discard(it)

    table = [(f, i) for i, f in enumerate(_PATTERN)]
    first = len(table)
    for key in table:
        add(key, table_items(*key))
    log(f"circuit 0: {sorted(need)} left")
    cands = {(f, s): table_items(f, s) for f in ("cornell", "cornell_aov", "precompiled_c1", "multi")
             for s in range(FREE, FREE + free)}

    def gain(key):
        seen, g = dict(have), 0
        for it in cands[key]:
            if it[0] == "refusal":
                seen[it[1]] = seen.get(it[1], 0) + 1
                it = ("refusal", it[1], seen[it[1]] - 1)
            g += it in need
        return g

    while need:
        best = max((k for k in cands if k not in table), key=lambda k: (gain(k), -k[1]))
        if gain(best) == 0:
            raise RuntimeError(f"cannot cover {sorted(need)}")
        table.append(best)
        add(best, cands[best])
        log(f"{best}: {len(need)} left")
    return table[first:]


# literal sequences kept beside the seeded ones: name -> (flavour, sequence)
PINNED = {
    # a mask and a mark together: the tile frozen before the second mark keeps its (P, S) pair, through a checkpoint too
    "frozen-pair": ("cornell", [("schedule", 2, 0), ("mark", 0), ("frames", 2, "none", 0, 0), ("mask", (1, 0, 1, 1, 1, 0), 0),
                                ("frames", 2, "eye", 1, 0), ("estimate", True, 0), ("schedule", 1, 0), ("save_load", 0),
                                ("frames", 1, "none", 0, 0), ("estimate", False, 0)]),
    # the same through sail_noise_mark, on a multi-device context under a sample partition: the mark is the reduced frame's
    "frozen-mark": ("multi", [("partition", 0, 1, SAMPLES, 0), ("schedule", 2, 0), ("mark", 0), ("frames", 1, "none", 0, 0),
                              ("mask", (0, 1, 1, 0, 1, 1), 0), ("schedule", 2, 0), ("mark", 0), ("frames", 2, "bounces", 1, 0),
                              ("estimate", False, 0), ("unmask", 0), ("schedule", 1, 0), ("estimate", True, 0)]),
}


def tile_tree(e):
    """sail_noise_estimate's tile map from the per-pixel errors: each 16x16 tile's f32 sum by the header's tree (pixels
    outside the frame add +0), divided in double by the tile's in-frame pixels and rounded to f32"""
    H, W = e.shape
    ty, tx = (H + 15) // 16, (W + 15) // 16
    out = np.zeros((ty, tx), F)
    for j in range(ty):
        for i in range(tx):
            blk = e[j * 16:(j + 1) * 16, i * 16:(i + 1) * 16]
            v = np.zeros((16, 16), F)
            v[:blk.shape[0], :blk.shape[1]] = blk
            v = v.reshape(4, 64)          # four strips of 16 x 4 pixels
            for off in (32, 16, 8, 4, 2, 1):
                v = v[:, :off] + v[:, off:2 * off]
            s = (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])
            out[j, i] = F(np.float64(s) / np.float64(blk.size))
    return out


if __name__ == "__main__":
    import pprint
    print("FREE_SEEDS =")
    pprint.pprint(search_table(), width=120, compact=True)
