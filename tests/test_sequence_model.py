"""The ledger of tests/sequence_model.py and its sequence generator, checked without a GPU: the generator is deterministic and
stays inside what a flavour accepts, the committed seed table covers every op kind, every adjacent pair of kinds and every
refusal, the ledger gives the oracle's own bits where the answer is known without it, and every rule of the ledger can be
seen to fail: for each switch of sequence_model.RULES some sequence of the table shows other values with the switch off, so
a library that broke that rule would fail that sequence in tests/test_gpu_sequences.py."""
import numpy as np
import pytest

import oracle
import sequence_model as sm
from sail_amd import capi

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def whole_frame(flavour, spp, mode=sm.SUM, k0=0, accum=None):
    fl = sm.FLAVOURS[flavour]
    sc = sm.scenes()[fl["scene"]]
    inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), fl["W"], fl["H"], k0, spp)
    return oracle.render(sc, capi.plugin_masks(sc["plugins"]), fl["W"], fl["H"], inv, seeds, sc["eye"], fl["B"], k0=k0,
                         accum_mode=mode, accum=accum)


@pytest.fixture(scope="module")
def table():
    """every sequence of the table with its observations on the ledger, oracle radiance, observed only where the sequence
    itself observes (so queues stay pending, as in the GPU test's lazy parametrisation) and at the end"""
    out = {}
    for flavour, seed in sm.SEEDS:
        seq = sm.make_sequence(seed, flavour)
        seen, led, refusals = sm.replay(flavour, seq)
        out[(flavour, seed)] = (seq, seen, refusals)
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    for flavour in ("cornell", "multi", "cull"):
        assert sm.make_sequence(7, flavour) == sm.make_sequence(7, flavour)
        assert sm.make_sequence(7, flavour) != sm.make_sequence(8, flavour)
    assert sm.make_sequence(7, "cornell")[:0] == [] and len(sm.make_sequence(7, "cornell", 9)) == 9
    assert eval(repr(sm.make_sequence(3, "room"))) == sm.make_sequence(3, "room"), "a sequence is a plain literal"


@pytest.mark.parametrize("flavour", sorted(sm.FLAVOURS))
def test_the_generator_stays_inside_the_flavour(flavour):
    fl = sm.FLAVOURS[flavour]
    tiles = len(sm.tile_rects(fl["W"], fl["H"]))
    seeds = [s for f, s in sm.SEEDS if f == flavour] + list(range(1000, 1040))
    for seed in seeds:
        seq = sm.make_sequence(seed, flavour)
        assert len(seq) == sm.LENGTH
        assert sum(sm.op_samples(op) for op in seq) <= sm.MAX_SAMPLES
        for op in seq:
            kind, args, rc = op[0], op[1:-1], op[-1]
            assert kind in sm.KINDS and rc in (sm.OK, sm.E_INVALID, sm.E_STATE)
            if kind == "schedule":
                assert args[0] in (1, 2, 3, 7)
            elif kind == "frames":
                assert args[0] in (1, 2, 5) and args[1] in ("none", "eye", "bounces") and 0 <= args[2] < args[0]
            elif kind == "launch_samples":
                assert args[0] in (0, 1, 2, 32)
            elif kind == "mask":
                assert len(args[0]) == tiles and any(args[0]) and set(args[0]) <= {0, 1}
            elif kind in ("update_objects", "move_objects"):
                assert args[0] in fl["rows"] and args[1] in (-1, 1)
            elif kind == "accum_mode":
                assert args[0] in (sm.SUM, sm.MIX, sm.COMPAT8)
            elif kind == "partition":
                rank, world, mode = args
                assert mode in (sm.TILES, sm.SAMPLES) and 0 <= rank < world <= 3
                if fl["devices"]:
                    assert (rank, world) == (0, 1), "all a multi-device context accepts"
            else:
                assert kind == "estimate" and args[0] in (False, True) or args == ()
        # every return code is the ledger's own (replay asserts it), and a negative one is a refusal the rules give
        sm.replay(flavour, seq, fake=True)


# ---- the committed table ---------------------------------------------------------------------------------------------------
def test_the_table_covers_kinds_pairs_refusals_and_flavours(table):
    kinds = [op[0] for seq, _, _ in table.values() for op in seq]
    for kind in sm.KINDS:
        assert kinds.count(kind) >= 5, f"{kind} appears {kinds.count(kind)} times"
    pairs = set().union(*(sm.adjacent_pairs(seq) for seq, _, _ in table.values()))
    active = [k for k in sm.KINDS if k not in sm.PURE_OBSERVERS]
    missing = [(a, b) for a in active for b in active if (a, b) not in pairs]   # every pair is legal in the single-device flavours
    assert not missing, f"{len(missing)} pairs never adjacent: {missing[:8]}"
    refusals = [r for _, _, rs in table.values() for r in rs]
    for r in sm.REFUSALS:
        assert refusals.count(r) >= 2, f"'{r}' is drawn {refusals.count(r)} times"
    assert {f for f, _ in sm.SEEDS} == set(sm.FLAVOURS)
    assert len(set(sm.SEEDS)) == len(sm.SEEDS)


def test_the_table_masks_include_all_ones_and_none_of_the_ranks_own(table):
    all_ones = foreign = 0
    for (flavour, _), (seq, _, _) in table.items():
        led = sm.Ledger(flavour, fake=True)
        for op in seq:
            if op[0] == "mask" and op[-1] == sm.OK:
                all_ones += all(op[1])
                rank, world = led.parts[0]
                if not led.multi and led.part_mode == sm.TILES and world > 1:
                    foreign += not any(op[1][t] for t in sm.own_tiles(led.W, led.H, rank, world))
            led.apply(*op[:-1])
    assert all_ones >= 1 and foreign >= 1


# ---- the ledger against plain oracle calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour,mode", [("cornell", sm.SUM), ("cornell", sm.MIX), ("cornell", sm.COMPAT8), ("room", sm.SUM),
                                          ("cull", sm.MIX)])
def test_schedules_alone_are_one_whole_frame_render(flavour, mode):
    seq = [("accum_mode", mode, 0), ("schedule", 2, 0), ("schedule", 1, 0), ("schedule", 3, 0)]
    if flavour == "cull":
        seq = seq[:3]
    _, led, _ = sm.replay(flavour, seq)
    want = whole_frame(flavour, led.k, mode)
    assert led.k == sum(sm.op_samples(op) for op in seq)
    assert np.array_equal(bits(led.shown()), bits(want)), "raw uint32"


def test_frames_with_a_pending_queue_are_the_same_frame():
    a = sm.replay("cornell", [("frames", 2, "none", 0, 0), ("frames", 1, "none", 0, 0), ("schedule", 1, 0)])[1]
    assert np.array_equal(bits(a.shown()), bits(whole_frame("cornell", 4))) and not a.queue


def test_a_tile_partition_sums_to_the_full_frame():
    parts = []
    for rank in range(3):
        _, led, _ = sm.replay("cornell", [("partition", rank, 3, sm.TILES, 0), ("schedule", 3, 0)])
        parts.append(led.shown())
        mine = set(sm.own_tiles(led.W, led.H, rank, 3))
        for t, (x0, y0, w, h) in enumerate(led.tiles):
            assert (parts[-1][y0:y0 + h, x0:x0 + w, 3] == (3 if t in mine else 0)).all()
    assert np.array_equal(bits((parts[0] + parts[1]) + parts[2]), bits(whole_frame("cornell", 3)))
    multi = sm.replay("multi", [("schedule", 3, 0)])[1]
    assert np.array_equal(bits(multi.shown()), bits(whole_frame("cornell", 3)))


def test_a_sample_partition_adds_the_ranks_in_order():
    multi = sm.replay("multi", [("partition", 0, 1, sm.SAMPLES, 0), ("schedule", 3, 0), ("frames", 2, "none", 0, 0)])[1]
    ranks = [sm.replay("cornell", [("partition", r, 3, sm.SAMPLES, 0), ("schedule", 5, 0)])[1] for r in range(3)]
    assert [r.samples() for r in ranks] == [2, 2, 1] and multi.samples() == 5
    want = (ranks[0].shown() + ranks[1].shown()) + ranks[2].shown()
    assert np.array_equal(bits(multi.shown()), bits(want))
    assert (want[..., 3] == 5).all() and np.allclose(want, whole_frame("cornell", 5), rtol=1e-5, atol=1e-5)


def test_a_frozen_tile_keeps_the_bits_of_the_frame_it_froze_at():
    t = 4
    mask = tuple(0 if i == t else 1 for i in range(6))
    _, led, _ = sm.replay("cornell", [("schedule", 3, 0), ("mask", mask, 0), ("schedule", 1, 0), ("frames", 1, "none", 0, 0)])
    three, five = whole_frame("cornell", 3), whole_frame("cornell", 5)
    got = led.shown()
    for i, (x0, y0, w, h) in enumerate(led.tiles):
        want = three if i == t else five
        assert np.array_equal(bits(got[y0:y0 + h, x0:x0 + w]), bits(want[y0:y0 + h, x0:x0 + w])), f"tile {i}"
    assert led.k == 5 and led.samples() == 5


def test_refusals_leave_the_ledger_alone():
    seq = [("schedule", 2, 0), ("estimate", False, -4), ("accum_mode", sm.MIX, 0), ("schedule", 2, 0), ("mask", (1, 0, 1, 0, 1, 0), -4),
           ("partition", 1, 2, sm.SAMPLES, -1), ("accum_mode", sm.COMPAT8, 0), ("mark", -4), ("schedule", 1, 0)]
    seen, led, refusals = sm.replay("cornell", seq)
    assert refusals == ["estimate without a mark", "mask in MIX", "sample partition in MIX", "mark in COMPAT8"]
    assert np.array_equal(bits(led.shown()), bits(whole_frame("cornell", 1, sm.COMPAT8))) and led.mask is None


def test_the_pinned_sequences_return_what_the_ledger_returns():
    for flavour, seq in sm.PINNED.values():
        sm.replay(flavour, seq, fake=True)   # asserts every return code


def test_the_tile_tree_adds_a_tiles_errors():
    """the restatement of the estimate's sum tree against float64 sums: any order of a tile's at most 256 non-negative f32
    terms lies within 255 u / (1 - 255 u), u = 2^-24, of the exact sum (the bound tests/test_gpu_noise.py derives)"""
    gamma = 255 * 2.0 ** -24 / (1 - 255 * 2.0 ** -24)
    e = np.random.default_rng(5).random((72, 136), dtype=F) * F(3)
    tree = sm.tile_tree(e)
    assert tree.shape == (5, 9)
    for j in range(5):
        for i in range(9):
            blk = e[j * 16:(j + 1) * 16, i * 16:(i + 1) * 16].astype(np.float64)
            assert abs(float(tree[j, i]) * blk.size - blk.sum()) <= gamma * blk.sum() and blk.size == (64 if (j, i) == (4, 8) else blk.size)
    one = np.zeros((16, 16), F)
    one[3, 5] = F(0.3)
    assert sm.tile_tree(one)[0, 0] == F(np.float64(F(0.3)) / 256)


# ---- every rule bites ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sorted(sm.RULES))
def test_every_rule_bites(table, rule):
    """Some sequence of the table shows other values (a compared frame, an estimate's inputs, k, a return code) when the ledger
    runs with the rule switched off. Candidates are found over constant radiance, the first is confirmed with the oracle's."""
    for (flavour, seed), (seq, seen, _) in table.items():
        off = {rule: False}
        if sm.replay(flavour, seq, rules=off, fake=True)[0] == sm.replay(flavour, seq, fake=True)[0]:
            continue
        assert sm.replay(flavour, seq, rules=off)[0] != seen, f"{flavour} {seed}: differs only over constant radiance"
        return
    pytest.fail(f"no sequence of the table notices the rule {rule} switched off")
