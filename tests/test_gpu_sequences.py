"""Seeded sequences of API calls replayed on a capi.Context and on the ledger of tests/sequence_model.py side by side. The
ledger restates include/sail_hip.h's rules for the queue of one-sample frames, the tile mask, the noise mark, restarts,
checkpoints and partitions over the CPU oracle's radiance; the library must show the ledger's bits. Needs a GPU.

`eager` compares after every op: the shown accumulator raw (the suite's bit_equal: one NaN is as good as another), the
sample index and every part's sums through sail_save_accum, sail_stats.samples, sail_get_active_tiles, the AOV maps of an AOV
context, and every op's return code; after a refused op that is the proof that nothing changed. Each of those reads launches
the queue, so `lazy` replays the same sequences and compares only what the sequence's own ops return, and everything at the
end: there queues stay pending across masks, partitions, checkpoints and the rest. An estimate is compared through
tests/test_gpu_noise.py's ref_error over the ledger's S and P: the pixel map raw, and the tile map raw against the sum tree
the header gives. Whichever kernel tier a launch runs, the bits are the same: no test waits for or expects a tier, and each
prints the kernel names it saw.

A failure names the flavour, the seed and the first differing op, prints the sequence up to it as a literal (replayable
through sequence_model.PINNED), the 64x64 tiles that differ, for SUM frames whether the count channel differs (a sample lost or doubled) or
only the colour (an order or a kernel), and the kernels of the launches since the last agreement."""
import re

import numpy as np
import pytest

import oracle
import sequence_model as sm
from sail_amd import capi
from test_gpu_noise import ref_error

pytestmark = pytest.mark.gpu

F = np.float32

@pytest.fixture(scope="module")
def gpu():
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    return True


def bit_equal(a, b):
    a = np.ascontiguousarray(a, dtype=F)
    b = np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


class Device:
    """the ops of a sequence as calls on a capi.Context"""

    def __init__(self, flavour):
        self.fl = sm.FLAVOURS[flavour]
        self.ctx = self.create()
        self.kernels = []   # (op index, kernel name, build and run-time kernel state) wherever they change

    def create(self):
        fl = self.fl
        return capi.Context(fl["W"], fl["H"], flags=fl["flags"], devices=[0] * fl["devices"] if fl["devices"] else None,
                            debug=fl["debug"])

    def call(self, fn, *args):
        """(return code, result): the binding raises "<call>: <code>: <text>" on a refusal"""
        try:
            return sm.OK, fn(*args)
        except capi.SailError as e:
            m = re.search(r": (-\d+): ", str(e))
            assert m, str(e)
            return int(m.group(1)), None

    def apply(self, op, led, k):
        """op on the context; `led` is the ledger after the op (its rows, mode and partition are the op's), k the sample
        index before it. Returns what the ledger's apply returns."""
        ctx, fl, kind, args = self.ctx, self.fl, op[0], op[1:-1]
        if kind == "schedule":
            inv, seeds = zip(*(sm.sample_args(fl["scene"], fl["W"], fl["H"], k + i) for i in range(args[0])))
            rc, _ = self.call(ctx.render_schedule, np.array(inv), np.array(seeds, F), led.eye, led.B)
            return {"rc": rc}
        if kind == "frames":
            for i in range(args[0]):
                inv, seed = sm.sample_args(fl["scene"], fl["W"], fl["H"], k + i)
                eye, bounces = led.frame_args(i, args[1], args[2])
                rc, _ = self.call(ctx.render, inv, eye, seed, bounces)
                if rc:
                    break
            return {"rc": rc}
        if kind == "launch_samples":
            return {"rc": self.call(ctx.set_launch_samples, args[0])[0]}
        if kind == "mask":
            return {"rc": self.call(ctx.set_active_tiles, list(args[0]))[0]}
        if kind == "unmask":
            return {"rc": self.call(ctx.set_active_tiles, None)[0]}
        if kind == "update_objects":
            return {"rc": self.call(ctx.update_objects, led.rows)[0]}
        if kind == "move_objects":
            return {"rc": self.call(ctx.move_objects, led.rows)[0]}
        if kind == "set_scene":
            return {"rc": self.call(ctx.set_scene_dict, led.current_scene())[0]}
        if kind == "reset":
            return {"rc": self.call(ctx.reset)[0]}
        if kind == "accum_mode":
            return {"rc": self.call(ctx.set_accum_mode, args[0])[0]}
        if kind == "partition":
            return {"rc": self.call(ctx.set_partition, *args)[0]}
        if kind == "save_load":
            rc, ck = self.call(ctx.save)
            assert rc == sm.OK
            return {"rc": self.call(ctx.load, ck)[0], "k": ck["k"], "parts": ck["parts"]}
        if kind == "save_load_fresh":
            rc, ck = self.call(ctx.save)
            assert rc == sm.OK
            new = self.create()
            new.set_scene_dict(led.current_scene())
            new.set_accum_mode(led.mode)
            new.set_partition(*((0, 1) if led.multi else led.parts[0]), led.part_mode)
            rc = self.call(new.load, ck)[0]
            ctx.close()
            self.ctx = new
            return {"rc": rc, "k": ck["k"], "parts": ck["parts"]}
        if kind == "mark":
            return {"rc": self.call(ctx.noise_mark)[0]}
        if kind == "estimate":
            rc, out = self.call(lambda: ctx.noise_estimate(tiles=True, pixels=True, remark=args[0]))
            return dict(out or {}, rc=rc)
        if kind == "read":
            rc, frame = self.call(ctx.read_accum)
            return {"rc": rc, "frame": frame}
        if kind == "readback":
            rc, out = self.call(lambda: ctx.readback(aov=led.aov))
            return {"rc": rc, "mean": out[0] if led.aov else out, "aov": out[1:] if led.aov else None}
        if kind == "filter":
            rc, out = self.call(ctx.filter, capi.FILTER_COLOR)
            return {"rc": rc, "out": out}
        if kind == "sync":
            return {"rc": self.call(ctx.sync)[0]}
        if kind == "stats":
            rc, st = self.call(ctx.stats)
            return {"rc": rc, "samples": int(st.samples)}
        if kind == "pick":
            rays = sm.pick_rays(led.eye)
            rc, out = self.call(ctx.pick, rays)
            return {"rc": rc, "pick": out, "rays": rays}
        if kind == "gbuffer":
            rc, out = self.call(lambda: ctx.gbuffer(np.array(led.scene["mvp_rowmajor"]), led.eye, rays=True))
            return {"rc": rc, "g": out}
        assert kind == "wait_kernel"
        return {"rc": self.call(ctx.kernel_ready, -1)[0]}

    def state(self, led):
        ctx = self.ctx
        ck = ctx.save()
        out = {"frame": ctx.read_accum(), "k": ck["k"], "parts": ck["parts"], "samples": int(ctx.stats().samples),
               "mask": ctx.get_active_tiles().reshape(-1)}
        if led.aov:
            out["aov"] = ctx.readback(aov=True)[1:]
        return out


def describe(what, got, want, led):
    """which 64x64 tiles of a frame differ and, for SUM, whether the count does"""
    bad = ~bit_equal(got, want)
    tiles = [t for t, (x0, y0, w, h) in enumerate(led.tiles) if bad[y0:y0 + h, x0:x0 + w].any()]
    text = f"{what}: {int(bad.any(-1).sum())} pixels differ, in tiles {tiles}"
    if led.mode == sm.SUM and got.shape[-1] == 4:
        if bad[..., 3].any():
            y, x = np.argwhere(bad[..., 3])[0]
            text += f"; the COUNT differs (a sample lost or doubled), first at ({x}, {y}): {got[y, x, 3]} for {want[y, x, 3]}"
        else:
            text += "; only the colour differs (an order or a kernel)"
    return text


def compare_op(op, got, want, led, sc):
    """the op's own return values against the ledger's; returns the list of differences"""
    bad = []
    if got["rc"] != op[-1] or want["rc"] != op[-1]:
        bad.append(f"return code {got['rc']}, the op expects {op[-1]}, the ledger {want['rc']}")
        return bad
    kind = op[0]
    if got["rc"] != sm.OK:
        return bad
    if kind == "read" and not bit_equal(got["frame"], want["frame"]).all():
        bad.append(describe("read_accum", got["frame"], want["frame"], led))
    if kind == "readback":
        if not bit_equal(got["mean"], want["mean"]).all():
            bad.append(describe("readback", got["mean"], want["mean"], led))
        if want["aov"] is not None:
            for name, g, w in zip(("normal", "position"), got["aov"], want["aov"]):
                if not bit_equal(g, w).all():
                    bad.append(describe(f"readback {name} map", g, w, led))
    if kind == "filter":
        ref = oracle.filter_image(want["mean"], capi.FILTER_COLOR)
        if not bit_equal(got["out"][..., :3], ref[..., :3]).all():
            bad.append(describe("filter", got["out"][..., :3], ref[..., :3], led))
    if kind == "stats" and got["samples"] != want["samples"]:
        bad.append(f"stats.samples {got['samples']} for {want['samples']}")
    if kind in ("save_load", "save_load_fresh"):
        if got["k"] != want["k"]:
            bad.append(f"saved k {got['k']} for {want['k']}")
        for i, (g, w) in enumerate(zip(got["parts"], want["parts"])):
            if not bit_equal(g, w).all():
                bad.append(describe(f"saved part {i}", g, w, led))
    if kind == "estimate":
        if (got["k"], got["k_mark"]) != (want["k"], want["k_mark"]):
            bad.append(f"estimate k, k_mark {got['k']}, {got['k_mark']} for {want['k']}, {want['k_mark']}")
        e, nonfinite = ref_error(want["S"], want["P"], mix=want["mix"], k=want["k"], h=want["k_mark"])
        if not np.array_equal(got["pixel_err"].view(np.uint32), e.view(np.uint32)):
            bad.append(describe("estimate pixel_err", got["pixel_err"][..., None], e[..., None], led))
        tree = sm.tile_tree(e)
        if not np.array_equal(got["tile_err"].view(np.uint32), tree.view(np.uint32)):
            bad.append(f"estimate tile_err differs in 16x16 tiles {np.argwhere(got['tile_err'] != tree).tolist()[:8]}")
        if got["nonfinite"] != int(nonfinite.sum()):
            bad.append(f"estimate nonfinite {got['nonfinite']} for {int(nonfinite.sum())}")
    if kind == "pick":
        idx, t = oracle.pick(sc, capi.plugin_masks(sc["plugins"])[0], got["rays"])
        if not (np.array_equal(got["pick"][0], idx) and bit_equal(got["pick"][1], t).all()):
            bad.append(f"pick {got['pick']} for {(idx, t)}")
    if kind == "gbuffer":
        g = got["g"]
        idx, t = oracle.pick(sc, capi.plugin_masks(sc["plugins"])[0], g["rays"].reshape(-1, 6))
        if not (np.array_equal(g["id"].reshape(-1), idx) and bit_equal(g["t"].reshape(-1), t).all()):
            bad.append(f"gbuffer: {int((g['id'].reshape(-1) != idx).sum())} ids differ")
    return bad


def compare_state(dev, led):
    got, want = dev.state(led), led.state()
    bad = []
    if not bit_equal(got["frame"], want["frame"]).all():
        bad.append(describe("the shown accumulator", got["frame"], want["frame"], led))
    if got["k"] != want["k"]:
        bad.append(f"sample index {got['k']} for {want['k']}")
    for i, (g, a) in enumerate(zip(got["parts"], led.acc)):
        if not bit_equal(g, a.S).all():
            bad.append(describe(f"part {i}", g, a.S, led))
    if got["samples"] != want["samples"]:
        bad.append(f"stats.samples {got['samples']} for {want['samples']}")
    if not np.array_equal(got["mask"], want["mask"]):
        bad.append(f"active tiles {got['mask'].tolist()} for {want['mask'].tolist()}")
    if want["aov"] is not None:
        for name, g, w in zip(("normal", "position"), got["aov"], want["aov"]):
            if not bit_equal(g, w).all():
                bad.append(describe(f"{name} map", g, w, led))
    return bad


def run(flavour, seq, lazy, label):
    led = sm.Ledger(flavour)
    dev = Device(flavour)
    agreed = -1   # the last op after which everything compared agreed
    names, builds = set(), set()

    def fail(i, bad):
        since = [f"op {j}: {n} ({s})" for j, n, s in dev.kernels if j > agreed]
        pytest.fail("\n".join([f"{label} ({'lazy' if lazy else 'eager'}): first difference at op {i} {seq[i] if i < len(seq) else 'the end'}",
                               f"sequence so far: {seq[:i + 1]!r}"] + bad +
                              ["kernels since the last agreement: " + ("; ".join(since) or "no launch")]), pytrace=False)

    try:
        dev.ctx.set_scene_dict(led.current_scene())
        for i, op in enumerate(seq):
            k = led.k
            want = led.apply(*op[:-1])
            got = dev.apply(op, led, k)
            info = dev.ctx.kernel_info()
            entry = (dev.ctx.kernel_name(), f"build {info['build_id']}, run-time kernel state {info['jit_state']}")
            if not dev.kernels or dev.kernels[-1][1:] != entry:
                dev.kernels.append((i,) + entry)
            names.add(info["name"])
            builds.add(info["build_id"])
            bad = compare_op(op, got, want, led, led.current_scene())
            if not bad and (not lazy or i == len(seq) - 1):
                bad = compare_state(dev, led)
                names.add(dev.ctx.kernel_info()["name"])
            if bad:
                fail(i, bad)
            if not lazy or op[0] in ("read", "readback", "filter", "estimate", "save_load", "save_load_fresh"):
                agreed = i
    finally:
        dev.ctx.close()
    print(f"kernels {label} {'lazy' if lazy else 'eager'}: {sorted(names)}, {len(builds)} builds")


@pytest.mark.parametrize("how", ["eager", "lazy"])
@pytest.mark.parametrize("flavour,seed", sm.SEEDS, ids=[f"{f}-{s}" for f, s in sm.SEEDS])
def test_a_seeded_sequence(gpu, flavour, seed, how):
    run(flavour, sm.make_sequence(seed, flavour), how == "lazy", f"{flavour} seed {seed}")


@pytest.mark.parametrize("how", ["eager", "lazy"])
@pytest.mark.parametrize("name", sorted(sm.PINNED))
def test_a_pinned_sequence(gpu, name, how):
    flavour, seq = sm.PINNED[name]
    run(flavour, seq, how == "lazy", f"{flavour} pinned {name}")
