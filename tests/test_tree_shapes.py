"""The synthetic hierarchies of tests/_tree_shapes.py reach the paths of csrc/rules.hip they were built for (no GPU).

tests/test_rules_shapes_gpu.py runs the kernels on these shapes; what makes that worth anything is that every shape still
takes the branch it is there for.  `describe` restates the host-side selection of csrc/rules.hip, and the table below is
asserted, so a fixture that stops reaching its cell fails here and does not silently stop testing it.  The second half
checks, with the oracle alone, that the logits the GPU test uses leave no path probability so small that a relative
comparison of P would be empty.

One more caterpillar was looked for: TPS 256 with soft_forward staged and soft_tree_loss not (their LDS rows differ by
2C + 16 floats).  There is none: C = 257 is the largest caterpillar at TPS 256 (R = 2C - 2 <= 512) and both entry points
still stage it (test_no_caterpillar_at_four_waves_splits_forward_and_loss); L grows with C, so no smaller one splits them
either.  The split exists at 16 waves, caterpillar(264), which is in the table instead; at 4 waves only the tree statistics,
with their per-block counters, lose the staging row (caterpillar(257))."""
import numpy as np
import pytest

import nbdt_oracle as O
import _tree_shapes as S
from nbdt.tree import Tree

ALL_PEELS = {0, 1, 2, 3}
PER_SAMPLE = ("soft_forward", "node_outputs", "soft_backward", "soft_tree_loss", "hard_tree_loss", "hard_forward")

_cache = {}


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tree_shapes")


def _shape(name, directory):
    if name not in _cache:
        pg, pw, leaves = S.build(name, directory)
        tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
        _cache[name] = (tree, O.OracleTree(pg, pw), S.describe(tree.flat))
    return _cache[name]


# shape -> (C, R, L, tps) of the issue's table; star300 / star513: R = L = C by construction
SIZES = {"cat33": (33, 64, 560, 64), "cat34": (34, 66, 594, 256), "cat120": (120, 238, 7259, 256),
         "cat200": (200, 398, 20099, 256), "cat257": (257, 512, 33152, 256), "cat258": (258, 514, 33410, 1024),
         "cat264": (264, 526, 34979, 1024), "cat280": (280, 558, 39339, 1024),
         "star64": (64, 64, 64, 64), "star65": (65, 65, 65, 256), "star300": (300, 300, 300, 256),
         "star513": (513, 513, 513, 1024), "kary243_3": (243, 363, 1215, 256), "kary600_70": (600, 609, 1200, 1024)}


def test_every_shape_has_a_row():
    assert set(SIZES) == set(S.SHAPES)


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_and_waves_per_sample(name, shapes_dir):
    tree, otree, d = _shape(name, shapes_dir)
    assert (d["C"], d["R"], d["L"], d["tps"]) == SIZES[name]
    flat = tree.flat
    # the generators give a tree: one path per class, every class once per level, and the oracle reads the same maps
    flat.require_single_path()
    assert d["R"] == d["N"] + d["C"] - 1
    assert otree.num_classes == d["C"] and otree.num_inodes == d["N"] and otree.root == flat.root
    assert [len(c) for per in otree.child_classes for c in per] == list(np.diff(flat.slot_off))
    if S.SHAPES[name][0] == "caterpillar":
        C = d["C"]
        assert d["max_depth"] == C - 1 and d["L"] == C * (C + 1) // 2 - 1
        assert sorted(np.diff(flat.cls_off)) == sorted(list(range(1, C)) + [C - 1])
        assert d["longest_slot"] == C - 1 and d["binary_nodes"] == d["N"]
    if S.SHAPES[name][0] == "star":
        assert d["N"] == 1 and d["max_fanout"] == d["C"] and d["longest_slot"] == 1 and d["longest_path"] == 1


def test_caterpillar_33_one_wave_long_chains_and_the_trailing_gather_block(shapes_dir):
    d = _shape("cat33", shapes_dir)[2]
    assert d["tps"] == 64 and d["spb"] == 4 and d["R"] == 64                 # R exactly at the one-wave boundary
    assert d["longest_slot"] >= 16 and d["longest_path"] >= 16              # long_chain on slots and on paths
    assert (d["nr"], d["left"]) == (1, 1) and d["trailing_block"] and d["pipelined_trips"] == 0
    for entry in PER_SAMPLE:
        assert d["staged"][entry] and d["slot_peels"][entry] == ALL_PEELS
    for entry in ("soft_forward", "soft_backward", "soft_tree_loss", "hard_tree_loss"):
        assert d["path_peels"][entry] == ALL_PEELS
    assert d["longest_slot"] == 32                 # one trip of the 32-element loop; 31 .. 16 take the `rem >= 16` block
    assert S.head_launch(d, 4096) == (8, True)     # the largest LDS row of the fused head at 8 samples per block: staged


def test_caterpillar_34_is_just_over_the_one_wave_boundary(shapes_dir):
    d = _shape("cat34", shapes_dir)[2]
    assert d["C"] <= 64 and d["R"] == 66 and d["tps"] == 256 and d["joint"] == 2
    assert d["longest_path"] >= 16 and d["path_peels"]["soft_forward"] == ALL_PEELS      # chains<ChainMul, 2> -> long_chain


@pytest.mark.parametrize("name,nr,left,trailing,trips", [("cat120", 3, 5, True, 1), ("cat200", 9, 7, True, 4),
                                                         ("cat257", 16, 2, False, 8), ("cat258", 8, 1, False, 4),
                                                         ("cat264", 8, 3, False, 4), ("cat280", 9, 3, True, 4)])
def test_gather_rounds(name, nr, left, trailing, trips, shapes_dir):
    d = _shape(name, shapes_dir)[2]
    assert d["U"] == (4 if d["tps"] == 1024 else 8)
    assert (d["nr"], d["left"], d["trailing_block"], d["pipelined_trips"]) == (nr, left, trailing, trips)


def test_caterpillar_200_schedule_rows_and_the_unstaged_head(shapes_dir):
    d = _shape("cat200", shapes_dir)[2]
    assert d["chunks"] == 7 and d["rows"] > 1
    assert all(d["staged"][e] for e in PER_SAMPLE)
    assert S.head_launch(d, 64) == (4, False)      # the fused head keeps its 4 samples per block and drops the staging row


def test_caterpillar_257_and_258_straddle_the_four_wave_boundary(shapes_dir):
    d = _shape("cat257", shapes_dir)[2]
    assert d["R"] == 512 and d["tps"] == 256 and all(d["staged"][e] for e in PER_SAMPLE)
    spare = S.LDS_BYTES - 4 * (S.tree_lds_ints(d["C"], d["N"], d["R"], d["sched_len"], False) +
                               S.front_floats("soft_forward", d["C"], d["N"], d["R"]) + d["L"] + S.STAGE_PAD)
    # staged with little to spare: the wave that gets the four chunks of one-leaf slots makes the schedule 5 rows long,
    # 15 KiB of offset arrays in front of the 130 KiB staging row
    assert d["rows"] == 5 and 0 <= spare < 8 * 1024
    assert d["staged"]["tree_stats"] is False       # the statistics' counters push the staging row out: unstaged at TPS 256
    d = _shape("cat258", shapes_dir)[2]
    assert d["R"] == 514 and d["tps"] == 1024 and d["U"] == 4 and all(d["staged"][e] for e in PER_SAMPLE)
    assert S.head_launch(d, 64) is None             # too wide for the fused head


def test_no_caterpillar_at_four_waves_splits_forward_and_loss(shapes_dir):
    d = _shape("cat257", shapes_dir)[2]             # the largest at TPS 256; staging only gets easier below it
    assert S.pick_tps(258, 2 * 258 - 2) == 1024
    assert d["staged"]["soft_forward"] and d["staged"]["soft_tree_loss"]


def test_caterpillar_264_stages_some_entry_points_only(shapes_dir):
    d = _shape("cat264", shapes_dir)[2]
    assert d["tps"] == 1024
    assert d["staged"] == {"soft_forward": True, "node_outputs": True, "soft_backward": True, "soft_tree_loss": False,
                           "hard_tree_loss": True, "hard_forward": False, "tree_stats": False}


def test_caterpillar_280_is_unstaged_everywhere(shapes_dir):
    d = _shape("cat280", shapes_dir)[2]
    assert d["tps"] == 1024 and all(v is False for v in d["staged"].values())
    assert d["L"] * 4 < S.LDS_BYTES                 # smaller than the 640 / 900 cases: the offset arrays tip it over


@pytest.mark.parametrize("name,tps", [("star64", 64), ("star65", 256), ("star300", 256), ("star513", 1024)])
def test_stars_run_one_wide_softmax(name, tps, shapes_dir):
    d = _shape(name, shapes_dir)[2]
    assert d["tps"] == tps and d["binary_nodes"] == 0 and d["max_fanout"] == d["C"] >= 14
    assert d["nr"] == 0 and d["left"] == (d["C"] + tps - 1) // tps and all(d["staged"].values())
    if name == "star300":
        assert S.head_launch(d, 640) == (4, True)


def test_kary_trees_never_take_the_binary_fast_path(shapes_dir):
    d = _shape("kary243_3", shapes_dir)[2]
    assert d["N"] == 121 and d["binary_nodes"] == 0 and d["max_fanout"] == 3 and d["tps"] == 256 and d["rows"] == 2
    assert d["longest_slot"] == 81 and d["slot_peels"]["soft_forward"]
    d = _shape("kary600_70", shapes_dir)[2]
    assert d["N"] == 10 and d["binary_nodes"] == 0 and d["max_fanout"] == 70 and d["longest_slot"] == 70
    assert d["tps"] == 1024 and all(d["staged"].values())


def test_schedule_restatement_covers_every_slot_once(shapes_dir):
    for name in ("cat200", "kary243_3", "star513"):
        tree, _, d = _shape(name, shapes_dir)
        sched, rows, _ = S.slot_schedule(tree.flat.slot_off, d["tps"])
        ids = sched[0][sched[0] >= 0]
        assert sorted(ids) == list(range(d["R"])) and sched.shape == (3, rows * d["tps"])
        assert np.array_equal(sched[1][sched[0] >= 0], tree.flat.slot_off[ids])


def test_fused_head_fallbacks_cannot_be_reached():
    """launch_head tries (TPS, samples per block) = (64, 8), (64, 4), (64, 1) or (256, 4), (256, 2), (256, 1), and each try
    drops the staging row before it gives up.  The first try without staging always fits, so the others never run: a
    sample row is at most K + 3C + 2R + 16 = 4432 floats at TPS 64 (K <= 4096, C, R <= 64) and 6672 at TPS 256 (C, R <= 512),
    the offset arrays at most 3*65 + 3*64 ints and 3*513 + 3*8*256 ints (N <= R; at most 8 chunks, so at most 8 schedule
    rows), which is 35847 and 34375 floats against the 40960 of 160 KiB."""
    worst64 = (3 * 65 + 3 * 64 + 3) + 8 * (4096 + 3 * 64 + 2 * 64 + 16) + S.STAGE_PAD
    worst256 = (3 * 513 + 3 * 8 * 256 + 3) + 4 * (4096 + 3 * 512 + 2 * 512 + 16) + S.STAGE_PAD
    assert worst64 * 4 <= S.LDS_BYTES and worst256 * 4 <= S.LDS_BYTES
    for C, N, R, rows, tps in ((64, 64, 64, 1, 64), (512, 512, 512, 8, 256)):
        d = {"C": C, "N": N, "R": R, "L": 10 ** 6, "tps": tps, "sched_len": rows * tps}
        assert S.head_launch(d, 4096) == (8 if tps == 64 else 4, False)


# ------------------------------------------------------------------------------------------------------------
# the logits of the GPU test keep the comparison of P meaningful

@pytest.mark.parametrize("name", list(SIZES))
def test_no_path_probability_underflows(name, shapes_dir):
    _, otree, d = _shape(name, shapes_dir)
    z = S.logits_for(name, 6, d["C"]).numpy()
    P = O.soft_forward(otree, z)
    print(name, "min P", P.min())
    assert P.min() >= 1e-30
    np.testing.assert_allclose(P.sum(1), 1.0, atol=1e-5)


def test_plain_gaussian_logits_would_underflow_on_a_deep_caterpillar(shapes_dir):
    """Why the ramp: with 3*randn the deep products are exact zeros, and a kernel returning zeros there would pass."""
    import torch
    _, otree, d = _shape("cat200", shapes_dir)
    z = (torch.randn(6, d["C"], generator=torch.Generator().manual_seed(200)) * 3).numpy()
    assert (O.soft_forward(otree, z) == 0).any()
