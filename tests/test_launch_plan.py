"""CPU: the shape of a trace launch (sail_plan_launch, sail_amd/csrc/sail_plan.cpp planLaunch): which kernel set and
run-time kernel, the samples in flight, the sample groups, the grid. Frames are bit-identical whatever the split, so no
parity test can see a slip here; the table states it. tests/golden/launch_plans.json holds the expected plans, worked out
from the rules as sail_plan.cpp's comments state them (its last five cases are the launches whose dispatches
profiles/plan_refactor_dispatch.txt records from the GPU).

One row of the issue's table cannot arise from the rule it describes: a launch of 11 samples at 4 in flight is never
rounded up to 12, because a group's samples are rounded only while they are fewer than the launch's (11 samples in two
groups are 6, rounded to 8; in one group they stay 11). The rule's own example is a *group* of 11: 64 samples in six
groups of 11 become groups of 12. Both are in the table."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from sail_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "sail_amd", "csrc", "sail_plan.cpp")

with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as _f:
    CASES = json.load(_f)["cases"]
with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as _f:
    SCENES = json.load(_f)["scenes"]


def plan(scene, **facts):
    if "debug" in facts:
        facts["debug"] = {int(k): v for k, v in facts["debug"].items()}
    return capi.plan_launch(SCENES[scene], **facts)


@pytest.mark.parametrize("case", CASES, ids=[c["case"] for c in CASES])
def test_plan_matches_the_table(case):
    assert plan(case["scene"], **case["facts"]) == case["plan"]


def test_table_covers_the_rows_it_must():
    by = {c["case"]: c["plan"] for c in CASES}
    full = by["C1 at 1080p on 256 CUs, value tier"]
    assert (full["ns"], full["launch_samples"], full["sample_groups"], full["threads"]) == (16, 1024, 1, 512)
    rank = by["the same as rank 3 of 8: one sample in flight, launch split"]
    assert rank["ns"] == 1 and rank["sample_groups"] > 1 and rank["staged"] == 1
    masked = by["the same under a mask leaving 4 of 510 tiles: still 16 in flight, launch split"]
    assert masked["ns"] == 16 and masked["sample_groups"] > 1
    c3 = by["C3: room form, 4 in flight, group 0 at home"]
    assert (c3["jit_mode"], c3["ns"], c3["group_home"]) == (capi.JIT_MODE_ROOM, 4, 1)
    c4 = by["C4 at 4K: pre-cull, under 64 rounds splits, whole steps of 4"]
    assert c4["cull_prims"] and c4["sample_groups"] > 1 and c4["group_spp"] % 4 == 0
    forced = by["forced 3 groups of 64 samples: 22 per group, not rounded to steps of 4"]
    assert forced["ns"] == 4 and forced["group_spp"] == 22 and forced["sample_groups"] == 3
    assert by["nspp above the stage cap: one group"]["sample_groups"] == 1
    assert by["nspp just under the stage cap"]["sample_groups"] > 1
    assert by["a launch of 1 sample: one group"]["sample_groups"] == 1
    assert by["6 groups of 64 samples at 4 in flight: groups of 11 rounded up to 12"]["group_spp"] == 12
    assert by["11 samples, 2 groups wanted: 6 rounded up to 8"]["group_spp"] == 8
    none = by["C1 with no tier loaded: the precompiled Cornell kernel, split"]
    assert none["grid"] == 510 * 16 * none["sample_groups"] and none["threads"] == 256 and none["jit_mode"] == -1
    none4 = by["C4 with no tier loaded: 1,024-thread precompiled kernel"]
    assert none4["grid"] == 510 * 16 * none4["sample_groups"] and none4["threads"] == 1024
    wf = by["wavefront switch on a pre-cull scene: one group, no stage"]
    assert (wf["wavefront"], wf["sample_groups"], wf["staged"], wf["jit_mode"]) == (1, 1, 0, -1)
    assert [c["case"] for c in CASES[-5:]] == [
        "C1 2x2 tiles unmasked", "C1 2x2 tiles under the mask [1, 0, 0, 1]", "C1 2x2 tiles, 3 groups forced",
        "C1 2x2 tiles as rank 3 of 8", "C4 2x2 tiles under the wavefront switch"]


def test_sixteen_in_flight_and_unsplit_go_together():
    """The threshold that decides the Cornell form's samples in flight (the share's residency rounds >= 12, on 256 CUs
    96 tiles) is the one that decides whether its launch is split: for every share from 1 to 510 tiles the plan holds 16
    samples in flight in one group, or 1 sample in flight in several. Under a tile mask the kernel keeps the share's 16,
    and the launch is unsplit exactly when the active tiles alone queue those rounds."""
    for tiles in range(1, 511):
        p = capi.plan_launch(SCENES["C1"], 64 * tiles, 64, 64, tier=capi.LAUNCH_TIER_TYPES)
        large = tiles * 128 / (256 * 4) >= 12
        assert (p["ns"] == 16 and p["sample_groups"] == 1) == large, tiles
        assert (p["ns"] == 1 and p["sample_groups"] > 1) == (not large), tiles
        m = capi.plan_launch(SCENES["C1"], 1920, 1080, 64, tier=capi.LAUNCH_TIER_TYPES, active_tiles=tiles)
        assert m["ns"] == 16 and (m["sample_groups"] == 1) == large, tiles


def test_bad_facts_are_refused():
    lib = capi.load()
    assert lib.sail_plan_launch(None, None) == -1
    assert "bad arguments" in lib.sail_last_error(None).decode()
    ok = dict(width=128, height=128, nspp=64)
    for bad, why in ((dict(ok, tier=capi.LAUNCH_TIER_VALUE), "no value kernel"),        # C3 has none
                     (dict(ok, tier=3), "bad launch"), (dict(ok, nspp=0), "bad launch"),
                     (dict(ok, width=0), "bad share"), (dict(ok, rank=2, world=2), "bad share"),
                     (dict(ok, compute_units=0), "bad share"), (dict(ok, rank=5, world=8), "no tile"),
                     (dict(ok, active_tiles=5), "no tile"), (dict(ok, active_tiles=0), "no tile"),
                     (dict(ok, debug={capi.DEBUG_JIT_NS: 3}), "samples in flight"),
                     (dict(ok, debug={capi.DEBUG_JIT_WAIT: 0}), "unknown option"),
                     (dict(ok, tier=capi.LAUNCH_TIER_TYPES, debug={capi.DEBUG_JIT: 0}), "no run-time kernel")):
        with pytest.raises(capi.SailError, match=why):
            capi.plan_launch(SCENES["C3"], **bad)
    f = capi.LaunchFacts(n=1, tn=1)  # a scene without rows
    assert lib.sail_plan_launch(ctypes.byref(f), ctypes.byref(capi.LaunchPlan())) == -1


def test_the_policy_file_sees_no_context_and_calls_no_hip():
    src = open(PLAN_SRC).read()
    assert "#pragma GCC poison sail_ctx" in src and "sail_ctx.h" not in src
    assert not re.search(r"hip[A-Z]\w*\(", src)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", PLAN_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
