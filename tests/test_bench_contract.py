"""bench.py's output contract on CPU: rank 0 prints exactly one JSON line on stdout, so C-level prints made
while the RCCL communicator is created (its version banner) must land on stderr."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stdout_to_stderr_covers_c_level_writes():
    code = (
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import bench\n"
        "q = bench._StdoutToStderr()\n"
        "q.__enter__()\n"
        "os.write(1, b'RCCL version : banner\\n')\n"
        "print('python-level noise')\n"
        "q.__exit__()\n"
        "print('{\"metric\": \"m\"}')\n" % ROOT
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ['{"metric": "m"}']
    assert "RCCL version" in r.stderr and "python-level noise" in r.stderr


def _bench(args, env_extra):
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=300, env=env, cwd=ROOT)


def test_gpus_must_match_world_size():
    """--gpus N under torch.distributed.run with WORLD_SIZE != N exits non-zero before touching a device"""
    r = _bench(["--gpus", "4", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "does not match WORLD_SIZE" in r.stderr
    assert r.stdout.strip() == ""


def test_gpus_beyond_visible_devices_fails():
    """--gpus N in one process needs N visible devices (the multi-device context); never a silent 1-GPU run"""
    from sail_amd import capi
    if capi.device_count() >= 64:
        pytest.skip("that many devices are visible")
    r = _bench(["--gpus", "64", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1"})
    assert r.returncode != 0 and "HIP devices are visible" in r.stderr
    assert r.stdout.strip() == ""


def test_dump_outputs_small_arrays_whole_large_ones_sampled(tmp_path):
    """--dump-outputs: float32 .npy per output; within the budget the array itself, above it the same seeded pixel
    sample in every run, so two builds' files compare element for element; all files together stay in the budget"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64_000_000
    rng = np.random.default_rng(7)
    small = rng.random((5, 7, 4), dtype=np.float32)
    big = rng.random((33, 19, 4), dtype=np.float32).astype(np.float64)  # float64 in, float32 out
    budget = 2 * 100 * 16  # 100 pixels of a float4 image each
    w1 = bench.dump_outputs(str(tmp_path / "a"), {"accum": small, "filtered": big}, budget=budget)
    w2 = bench.dump_outputs(str(tmp_path / "b"), {"accum": small, "filtered": -big}, budget=budget)
    a, f1, f2 = (np.load(tmp_path / d / n) for d, n in (("a", "accum.npy"), ("a", "filtered.npy"), ("b", "filtered.npy")))
    assert a.dtype == np.float32 and np.array_equal(a, small)
    assert w1["accum"]["sampled_pixels"] is None and w1["filtered"] == w2["filtered"]
    assert f1.dtype == np.float32 and f1.shape == (100, 4) and w1["filtered"]["sampled_pixels"] == 100
    assert np.array_equal(f2, -f1)  # the same pixels both times
    rows = {tuple(r) for r in big.reshape(-1, 4).astype(np.float32)}
    assert len({tuple(r) for r in f1}) == 100 and all(tuple(r) in rows for r in f1)  # distinct pixels of the image
    assert a.nbytes + f1.nbytes <= budget


def _gpu_bench(args):
    from sail_amd import capi
    if capi.device_count() < 1:
        pytest.skip("no HIP device")
    r = _bench(["--gpus", "1"] + args, {"WORLD_SIZE": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(tmp_path):
    """a plain run: --steps sets the timed steps, the line holds the headline figures and none of what --full adds;
    --dump-outputs writes the accumulator of the last step (every pixel counts each of its samples once)"""
    import numpy as np
    spp = 4
    rec = _gpu_bench(["--steps", "2", "--warmup", "1", "--spp", str(spp), "--dump-outputs", str(tmp_path / "out")])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "Msamples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["metric"] == "Msamples/s (paths x bounces) at 1920x1080 Cornell box"
    assert rec["ms_per_step"] > 0
    # value and ms_per_step state the same timed region: segments per step / time per step (ms_per_step is printed
    # to 0.001 ms, so they agree to half of that over the step's time)
    assert rec["value"] == pytest.approx(rec["config"]["segments_per_step"] / (rec["ms_per_step"] * 1e-3) / 1e6,
                                         rel=0.0006 / rec["ms_per_step"] + 1e-6)
    assert not {"roofline", "validation", "cpu_baseline", "filter"} & set(rec)
    assert sorted(os.listdir(tmp_path / "out")) == ["accum.npy"]
    acc = np.load(tmp_path / "out" / "accum.npy")
    assert acc.dtype == np.float32 and acc.shape == (1080, 1920, 4) and acc.nbytes <= 64_000_000
    assert np.all(acc[..., 3] == np.float32(spp)) and np.isfinite(acc).all() and acc[..., :3].max() > 0


@pytest.mark.gpu
def test_full_run_adds_validation_and_roofline():
    """--full (here without the CPU baselines, which take a minute) checks the frame against the oracle and reports
    the roofline of the timed launches beside the same headline figures"""
    rec = _gpu_bench(["--steps", "1", "--warmup", "1", "--spp", "4", "--full", "--no-cpu-baseline"])
    assert rec["steps"] == 1 and rec["ms_per_step"] > 0 and rec["unit"] == "Msamples/s"
    v = rec["validation"]
    assert v["pixels_with_wrong_count"] == 0 and v["rule"] == "bit-exact" and all(c["match"] for c in v["oracle_crops"])
    rf = rec["roofline"]
    assert rf["bound"] == "valu" and rf["achieved"] > 0 and rf["ops_per_segment_live"] > 0
    assert rf["kernel_id"].startswith(rf["kernel"] + "@")
    assert "cpu_baseline" not in rec


class _FrameCtx:
    """stands in for a context whose reduced frame is `acc` (bench.validate_frame reads it with read_accum)"""

    def __init__(self, acc):
        self.acc = acc

    def read_accum(self):
        return self.acc.copy()


def test_validate_frame_refuses_a_broken_reduce(fixtures, capsys):
    """bench.py checks the reduced frame after its timed steps: every count == spp and oracle crops in tiles of
    several ranks; a reduce that drops or double-counts one rank's tiles ends the run (exit 3) with no number"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    import oracle
    from sail_amd import capi
    sc = fixtures["scenes"]["C1"]
    W, H, B, spp, ngpu = 130, 70, 3, 2, 4
    masks = capi.plugin_masks(sc["plugins"])
    mvp = np.array(sc["mvp_rowmajor"])
    inv, seeds = capi.schedule(mvp, W, H, 0, spp)
    good = oracle.render(sc, masks, W, H, inv, seeds, sc["eye"], B)
    rep = bench.validate_frame(_FrameCtx(good), sc, masks, mvp, W, H, B, spp, inv, seeds, capi.PART_TILES, ngpu)
    assert rep["pixels_with_wrong_count"] == 0 and all(c["match"] for c in rep["oracle_crops"])
    assert {c["rank"] for c in rep["oracle_crops"]} >= {0, 3}
    for broken in ("dropped", "doubled", "wrong"):
        acc = good.copy()
        tile = acc[0:64, 64:128]  # tile 1 (rank 1 of 4)
        if broken == "dropped":
            tile[...] = 0.0
        elif broken == "doubled":
            tile[...] *= 2.0
        else:  # counts right, radiance of rank 3's tile perturbed
            acc[0:64, 0:64, 0] = np.nextafter(acc[0:64, 0:64, 0], np.float32(np.inf))
            acc[64:70, 128:130, 0] += 1e-3
        with pytest.raises(SystemExit) as e:
            bench.validate_frame(_FrameCtx(acc), sc, masks, mvp, W, H, B, spp, inv, seeds, capi.PART_TILES, ngpu)
        assert e.value.code == 3
    out = capsys.readouterr()
    assert out.out == "" and "failed validation" in out.err
