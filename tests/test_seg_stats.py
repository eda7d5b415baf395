"""Segmentation evaluation, the parts that need no GPU: the metric functions on hand-written matrices, the layout and
size dispatch (a pure host function), the analyzers' state / merge / load_state on states loaded directly, and the C
entry's refusals, which come before any device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C, ops
from nbdt import segmentation as G
from nbdt.tree import Tree

import _seg_ref as S
import _tree_shapes as T

EINVAL = -1


# ------------------------------------------------------------------------------------------------ metric functions

def test_metrics_3x3_with_an_empty_class():
    """m[label, prediction] = [[3, 1, 0], [0, 2, 0], [0, 0, 0]]: 6 pixels, 5 on the diagonal.
    pixel accuracy 5/6.  Class accuracy (recall) 3/4, 2/2, NaN (class 2 has no label pixel): mean (3/4 + 1)/2 = 7/8.
    IoU: class 0: 3 / (4 + 3 - 3) = 3/4; class 1: 2 / (2 + 3 - 2) = 2/3; class 2: label pixels + predicted pixels = 0 ->
    NaN, left out of the mean: mIoU = (3/4 + 2/3) / 2 = 17/24 over 2 classes.
    Frequency-weighted IoU: (4 * 3/4 + 2 * 2/3) / 6 = 13/18."""
    m = np.array([[3, 1, 0], [0, 2, 0], [0, 0, 0]], dtype=np.int64)
    assert G.pixel_accuracy(m) == 5 / 6
    acc = G.class_accuracy(m)
    assert acc[0] == 3 / 4 and acc[1] == 1.0 and math.isnan(acc[2])
    assert G.mean_class_accuracy(m) == 7 / 8
    v = G.iou(m)
    assert v.dtype == np.float64 and v[0] == 3 / 4 and v[1] == 2 / 3 and math.isnan(v[2])
    assert G.mean_iou(m) == (3 / 4 + 2 / 3) / 2 and G.classes_with_union(m) == 2
    assert G.frequency_weighted_iou(m) == (4 * (3 / 4) + 2 * (2 / 3)) / 6
    rep = G.metrics(m, ["a", "b", "c"])
    assert rep["classes_in_mean_iou"] == 2 and rep["pixels"] == 6 and rep["mean_iou"] == G.mean_iou(m)
    assert rep["iou"] == [{"class": "a", "iou": 3 / 4}, {"class": "b", "iou": 2 / 3}, {"class": "c", "iou": None}]


def test_metrics_4x4():
    """m = [[5, 0, 1, 0], [2, 3, 0, 0], [0, 0, 4, 0], [0, 1, 0, 0]]: 16 pixels, 12 correct -> pixel accuracy 3/4.
    Label pixels (rows) 6, 5, 4, 1; predicted pixels (columns) 7, 4, 5, 0.
    Recall 5/6, 3/5, 4/4, 0/1: mean (5/6 + 3/5 + 1 + 0) / 4.
    IoU 5/(6+7-5) = 5/8, 3/(5+4-3) = 1/2, 4/(4+5-4) = 4/5, 0/(1+0-0) = 0 (a class that is only ever missed has an
    IoU of 0, not NaN): mIoU = (5/8 + 1/2 + 4/5 + 0) / 4 over 4 classes.
    Frequency-weighted: (6 * 5/8 + 5 * 1/2 + 4 * 4/5 + 1 * 0) / 16."""
    m = [[5, 0, 1, 0], [2, 3, 0, 0], [0, 0, 4, 0], [0, 1, 0, 0]]
    assert G.pixel_accuracy(m) == 3 / 4
    assert np.array_equal(G.class_accuracy(m), np.array([5 / 6, 3 / 5, 1.0, 0.0]))
    assert G.mean_class_accuracy(m) == (5 / 6 + 3 / 5 + 1.0 + 0.0) / 4
    assert np.array_equal(G.iou(m), np.array([5 / 8, 1 / 2, 4 / 5, 0.0]))
    assert G.mean_iou(m) == (5 / 8 + 1 / 2 + 4 / 5 + 0.0) / 4 and G.classes_with_union(m) == 4
    assert G.frequency_weighted_iou(m) == (6 * (5 / 8) + 5 * (1 / 2) + 4 * (4 / 5) + 0.0) / 16


def test_metrics_of_an_empty_matrix():
    """Nothing counted: every ratio is 0 / 0 = NaN, the mean runs over 0 classes, and the report stays JSON-able."""
    m = np.zeros((3, 3), dtype=np.int64)
    assert math.isnan(G.pixel_accuracy(m)) and math.isnan(G.mean_iou(m)) and math.isnan(G.frequency_weighted_iou(m))
    assert math.isnan(G.mean_class_accuracy(m)) and np.isnan(G.iou(m)).all() and G.classes_with_union(m) == 0
    rep = G.metrics(m)
    assert rep["mean_iou"] is None and rep["classes_in_mean_iou"] == 0 and rep["pixels"] == 0
    with pytest.raises(ValueError, match="square"):
        G.iou(np.zeros((3, 4)))


def test_metrics_are_integer_ratios_in_float64():
    """Counts beyond 2^24 (where fp32 would round) give the exact float64 ratio."""
    big = 3 * (1 << 40) + 1
    m = np.array([[big, 1], [0, 1]], dtype=np.int64)
    assert G.pixel_accuracy(m) == (big + 1) / (big + 2)
    assert G.iou(m)[0] == big / (big + 1)


# ------------------------------------------------------------------------------------------------ dispatch

def _strides(t):
    return tuple(t.shape), tuple(t.stride())


def test_dispatch_is_a_function_of_layout():
    """The layouts of tests/test_seg.py's dispatch cases."""
    flat = S.case("lip")[0].flat
    C = flat.num_classes
    z = torch.zeros(2, C, 5, 13)
    f = lambda t, dtype=torch.float32: ops.seg_stats_dispatch(*_strides(t), dtype, flat)  # noqa: E731
    assert f(z) == "pixel"
    assert f(z.to(memory_format=torch.channels_last)) == "rows"
    assert f(z.transpose(2, 3).contiguous().transpose(2, 3)) == "contiguous"
    assert f(torch.zeros(2, C + 3, 5, 13)[:, 1:C + 1]) == "pixel"
    assert f(torch.zeros(3, C, 1, 1)) == "pixel"
    assert f(torch.zeros(2, C, 5, 26)[:, :, :, ::2]) == "contiguous"
    assert f(z, torch.bfloat16) == "pixel" and f(z, torch.float16) == "pixel"
    with pytest.raises(_C.NBDTHipError, match="dtype"):
        f(z, torch.float64)
    with pytest.raises(_C.NBDTHipError, match="channels"):
        f(torch.zeros(2, C + 1, 5, 13))
    with pytest.raises(_C.NBDTHipError, match=r"\[N, C, H, W\]"):
        ops.seg_stats_dispatch((4, C), (C, 1), torch.float32, flat)


@pytest.mark.parametrize("tag", tuple(S.CASES))
def test_dataset_hierarchies_fit(tag):
    """rows (R + F) * 256 bytes plus the block's counters; ADE20K: 75 KB + 3 KB."""
    flat = S.case(tag)[0].flat
    assert _C.seg_stats_fits(flat) and _C.tree_stats_fits(flat)
    depth = T.max_depth(flat)
    assert _C.flat_max_depth(flat) == depth
    small = (5 * flat.num_inodes + 4 + depth + 1 + 1) & ~1
    assert _C.seg_stats_lds_bytes(flat) == (flat.num_slots + 2) * 256 + 4 * small
    if tag == "ade20k":
        assert (flat.num_slots + 2) * 256 == 75 * 1024 and 3000 < 4 * small < 3200


def _kary(tmp_path, C, k):
    pg, pw, leaves = T.kary(tmp_path, C, k)
    return Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat


def test_between_the_two_limits(tmp_path):
    """A complete binary tree over C leaves has R = 2 (C - 1), F = 2, N = C - 1: it passes the pixel form's R + F <= 640
    up to C = 320, but rows + counters <= 160 KB only up to C = 307 (at 308: 616 rows = 157 696 bytes plus 4 * 1550 bytes of
    counters = 163 896 > 163 840).  In between the statistics take the row diagnostics on a coerced copy."""
    fits, gap, edge = _kary(tmp_path, 307, 2), _kary(tmp_path, 308, 2), _kary(tmp_path, 320, 2)
    for flat, C in ((fits, 307), (gap, 308), (edge, 320)):
        assert (flat.num_classes, flat.num_inodes, flat.num_slots) == (C, C - 1, 2 * (C - 1))
        assert _C.seg_pixel_fits(flat) and _C.flat_max_depth(flat) == T.max_depth(flat) == 9
    assert _C.seg_stats_lds_bytes(fits) == 614 * 256 + 4 * 1544 == 163360 <= _C.LDS_BYTES
    assert _C.seg_stats_lds_bytes(gap) == 616 * 256 + 4 * 1550 == 163896 > _C.LDS_BYTES
    assert _C.seg_stats_fits(fits) and not _C.seg_stats_fits(gap) and not _C.seg_stats_fits(edge)
    z = torch.zeros(1, 308, 2, 3)
    assert ops.seg_stats_dispatch(*_strides(z), z.dtype, gap) == "coerced"
    assert ops.seg_stats_dispatch(*_strides(z.to(memory_format=torch.channels_last)), z.dtype, gap) == "rows"
    assert _C.seg_dispatch(*_strides(z), z.dtype, gap) == "pixel"            # prediction still takes the pixel form
    z = torch.zeros(1, 307, 2, 3)
    assert ops.seg_stats_dispatch(*_strides(z), z.dtype, fits) == "pixel"


def test_the_row_limit_restates_the_kernel_dispatch(tmp_path):
    """tree_stats_fits is the NBDT_DISPATCH_RULES_EX arithmetic of nbdt_tree_stats_accumulate; tests/_tree_shapes.py
    restates the same for its fixtures, and the two agree on shapes on both sides of the limit."""
    for name in ("cat33", "cat280", "star65", "star513", "kary243_3", "kary600_70"):
        pg, pw, leaves = T.build(name, tmp_path)
        flat = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat
        assert _C.tree_stats_fits(flat) == (T.describe(flat)["staged"]["tree_stats"] is not None), name
        assert _C.flat_max_depth(flat) == T.max_depth(flat), name


def test_beyond_both_limits(tmp_path):
    """A 15 000-way star: 30 000 pixel rows, and a sample row of C + 2R + 2N + 32 = 45 034 floats = 180 KB for the row
    diagnostics.  The error names both limits."""
    pg, pw, leaves = T.star(tmp_path, 15000)
    flat = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat
    assert not _C.seg_stats_fits(flat) and not _C.tree_stats_fits(flat)
    for z in (torch.zeros(1, 15000, 1, 2), torch.zeros(1, 15000, 1, 2).to(memory_format=torch.channels_last)):
        with pytest.raises(_C.NBDTHipError, match=r"pixel form.*640.*row diagnostics.*163840"):
            ops.seg_stats_dispatch(*_strides(z), z.dtype, flat)


# ------------------------------------------------------------------------------------------------ analyzer state

def _random_counts(analyzer, seed, C, N=0, depth=0):
    rng = np.random.default_rng(seed)
    sizes = {"totals": 4, "node_counts": 5 * N, "first_error_depth": depth + 1}
    return {f: rng.integers(0, 1 << 40, size=sizes.get(f, C * C), dtype=np.int64) for f in analyzer.fields}


def test_state_round_trip_and_merge():
    tree = S.case("lip")[0]
    C, N = tree.flat.num_classes, tree.flat.num_inodes
    depth = _C.flat_max_depth(tree.flat)
    make = lambda: G.SegmentationStatistics(tree=tree)  # noqa: E731
    a = make()
    assert a.fields == ("totals", "confusion_net", "confusion_hard", "confusion_soft", "node_counts", "first_error_depth")
    assert a.ignore_index == 255 and a.classes == tuple(tree.classes)
    parts = [_random_counts(a, seed, C, N, depth) for seed in range(4)]
    ranks = []
    for p in parts:
        r = make()
        r.load_state({"counts": p})
        state = r.state()
        assert set(state) == {"counts"} and all(v.dtype == np.int64 for v in state["counts"].values())
        assert all(np.array_equal(state["counts"][f], p[f]) for f in a.fields)                 # round trip
        ranks.append(state)
    idle = make().state()
    assert idle == {"counts": {}}                                                               # saw no batch
    merged = a.merge(ranks + [idle])
    total = {f: sum(p[f] for p in parts) for f in a.fields}
    assert all(np.array_equal(merged["counts"][f], total[f]) for f in a.fields)
    assert all(np.array_equal(a.merge([idle] + ranks)["counts"][f], total[f]) for f in a.fields)
    whole = make()
    whole.load_state({"counts": total})
    a.load_state(merged)
    assert all(np.array_equal(a.state()["counts"][f], whole.state()["counts"][f]) for f in a.fields)
    assert np.array_equal(a.confusion("hard"), total["confusion_hard"].reshape(C, C))
    nobody = make()
    nobody.load_state(nobody.merge([idle, idle]))
    with pytest.raises(RuntimeError, match="no batch"):
        nobody.counts()
    assert a.reduce() is a                                                   # no process group: a no-op


def test_report_follows_the_host_functions(capsys):
    tree = S.case("lip")[0]
    C, N = tree.flat.num_classes, tree.flat.num_inodes
    a = G.SegmentationStatistics(tree=tree, worst=3)
    rng = np.random.default_rng(7)
    counts = {f: rng.integers(0, 50, size=n, dtype=np.int64) for f, n in (
        ("totals", 4), ("confusion_net", C * C), ("confusion_hard", C * C), ("confusion_soft", C * C),
        ("node_counts", 5 * N), ("first_error_depth", _C.flat_max_depth(tree.flat) + 1))}
    counts["confusion_soft"].reshape(C, C)[3, :] = 0
    counts["confusion_soft"].reshape(C, C)[:, 3] = 0                        # class 3: empty union under the soft rules
    a.load_counts(counts)
    rep = a.report()
    for kind in ("net", "hard", "soft"):
        m = counts["confusion_" + kind].reshape(C, C)
        r = rep["rules"][kind]
        assert r["mean_iou"] == G.mean_iou(m) and r["pixel_accuracy"] == G.pixel_accuracy(m)
        assert r["mean_class_accuracy"] == G.mean_class_accuracy(m)
        assert r["frequency_weighted_iou"] == G.frequency_weighted_iou(m)
        assert [e["class"] for e in r["iou"]] == list(tree.classes)
    assert rep["rules"]["soft"]["classes_in_mean_iou"] == C - 1 and rep["rules"]["soft"]["iou"][3]["iou"] is None
    assert rep["rules"]["net"]["classes_in_mean_iou"] == C
    assert len(rep["worst_nodes"]) == 3 and "entropy_mean" not in rep["worst_nodes"][0]
    assert rep["first_error_depth"] == counts["first_error_depth"].tolist() and rep["totals"] == counts["totals"].tolist()
    import json
    json.dumps(rep, allow_nan=False)
    a.start_epoch(0)
    a.phase = "test"
    a.end_test(0)
    out = capsys.readouterr().out
    assert "mIoU" in out and f"over {C - 1} classes" in out and "first wrong turn by depth" in out


def test_backbone_only_needs_no_tree():
    a = G.SegmentationStatistics(classes=("road", "car", "sky"), rules=("net",), ignore_index=0)
    assert a.tree is None and a.fields == ("totals", "confusion_net") and a.ignore_index == 0 and not a.with_nodes
    a.load_counts({"totals": [6, 5, 5, 5], "confusion_net": [3, 1, 0, 0, 2, 0, 0, 0, 0]})
    rep = a.report()
    assert rep["rules"]["net"]["mean_iou"] == (3 / 4 + 2 / 3) / 2 and "worst_nodes" not in rep
    with pytest.raises(ValueError, match="hard rules"):
        a.node_table()
    with pytest.raises(ValueError, match="rules must be chosen"):
        G.SegmentationStatistics(classes=("a",), rules=("net", "fuzzy"))
    with pytest.raises(ValueError, match="classes"):
        G.SegmentationStatistics(rules=("net",))


def test_thin_analyzers_track_the_best_miou(capsys):
    tree = S.case("lip")[0]
    C = tree.flat.num_classes
    for cls, name, kind in ((G.HardSegEmbeddedDecisionRules, "SegNBDT-Hard", "hard"),
                            (G.SoftSegEmbeddedDecisionRules, "SegNBDT-Soft", "soft")):
        a = cls(tree=tree)
        assert a.name == name and a.fields == ("confusion_" + kind,) and a.best_accuracy == 0.0
        assert a.accepts_path_graph and a.accepts_path_wnids and cls.accepts_tree(tree) is tree
        assert a.accuracy() == 0.0
        best = 0.0
        for epoch, diag in enumerate((4, 9, 2)):
            m = np.ones((C, C), dtype=np.int64) + diag * np.eye(C, dtype=np.int64)
            a.start_test(epoch)
            a.load_counts({"confusion_" + kind: m})
            assert a.accuracy() == 100.0 * G.mean_iou(m) and a.pixel_accuracy() == 100.0 * G.pixel_accuracy(m)
            a.end_test(epoch)
            best = max(best, round(100.0 * G.mean_iou(m), 2))
            assert a.best_accuracy == best
        assert f"[{name}] mIoU" in capsys.readouterr().out
    assert G.names == ("SegmentationStatistics", "HardSegEmbeddedDecisionRules", "SoftSegEmbeddedDecisionRules")
    import nbdt
    assert nbdt.segmentation is G and "segmentation" in nbdt.__all__


def test_batches_are_checked_before_any_device_work():
    a = G.SegmentationStatistics(classes=("a", "b"), rules=("net",))
    with pytest.raises(ValueError, match="resize the logits to the label size first"):
        a.update_batch(torch.zeros(1, 2, 4, 4), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        a.update_batch(torch.zeros(4, 2), torch.zeros(4, dtype=torch.long))
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        a.update_batch(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


# ------------------------------------------------------------------------------------------------ ABI

def test_header_binding_and_version():
    with open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")) as f:
        header = f.read()
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert _C.SIGNATURES["nbdt_seg_stats_accumulate"] == (
        ctypes.c_int, [P, P, ctypes.c_int, I64, I64, I64, I64, P, I64, P, P, P, P, P])
    assert _C.SIGNATURES["nbdt_seg_stats_fits"] == (ctypes.c_int, [P])
    for name in ("nbdt_seg_stats_accumulate", "nbdt_seg_stats_fits", "nbdt_set_seg_stats_max_blocks",
                 "nbdt_get_seg_stats_max_blocks"):
        assert re.search(r"\b" + name + r"\(", header) and name in _C.SIGNATURES and name in _C.exported_symbols()
    assert _C.lib().nbdt_version() >= 132
    assert "nbdt_seg_stats_accumulate also pixels" in header              # its line of the "Size limits" list
    assert ops.SEG_STATS_FIELDS == ("totals", "confusion_net", "confusion_hard", "confusion_soft", "node_counts",
                                    "first_error_depth")


def test_refusals_come_before_any_device_call():
    """What the entry refuses without looking at the hierarchy is checked first, so a NULL handle and pointers that lead
    nowhere show it on a box without a GPU: a call that got past these checks would stop at "null tree handle".  The
    refusal of a hierarchy beyond nbdt_seg_stats_fits needs a handle (nbdt_tree_create needs a device): the arithmetic
    is tested above on the host, the entry's own refusal in tests/test_seg_stats_gpu.py."""
    lib = _C.lib()
    dummy = 4096                            # never dereferenced: every call below is refused first

    def call(stats, y, N=1, HW=64, pred=None):
        rc = lib.nbdt_seg_stats_accumulate(None, dummy, 0, N, HW, 20 * HW, HW, y, 255,
                                           ctypes.byref(stats) if stats is not None else None, pred, None, None, None)
        return rc, lib.nbdt_last_error().decode()

    def block(**fields):
        b = _C.TreeStats()
        for k in fields:
            setattr(b, k, dummy)
        return b

    rc, why = call(block(totals=1, node_entropy=1), dummy)
    assert rc == EINVAL and "node_entropy is not part of the segmentation statistics" in why
    for field in ops.SEG_STATS_FIELDS:
        rc, why = call(block(**{field: 1}), None)
        assert rc == EINVAL and "need the labels" in why, field
    rc, why = call(None, dummy)
    assert rc == EINVAL and "nothing requested" in why
    rc, why = call(block(), None)
    assert rc == EINVAL and "nothing requested" in why
    rc, why = call(block(totals=1), dummy, N=1 << 15, HW=1 << 16)                     # 2^31 pixels
    assert rc == EINVAL and "N * HW must stay below 2^31" in why
    rc, why = call(block(totals=1), dummy, N=(1 << 15) - 1, HW=1 << 16)               # just below: goes on to the handle
    assert rc == EINVAL and "null tree handle" in why
    rc, why = call(None, None, pred=dummy)                                            # predictions alone need no labels
    assert rc == EINVAL and "null tree handle" in why
    assert lib.nbdt_seg_stats_fits(None) == 0
    assert lib.nbdt_set_seg_stats_max_blocks(-1) == EINVAL and "block cap" in lib.nbdt_last_error().decode()
    assert lib.nbdt_get_seg_stats_max_blocks() == 0
