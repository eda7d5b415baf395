"""Segmentation evaluation on the GPU: nbdt_seg_stats_accumulate (csrc/seg_stats.h) against the reference's recorded
outputs, against the row diagnostics on the coerced tensor, on inputs that take both ends of the key aggregation, under
every way of cutting a pass into calls, and through the analyzers.  Everything compared is an integer: every
comparison is array_equal."""
import ctypes

import numpy as np
import pytest
import torch

from nbdt import _C, ops
from nbdt import segmentation as G
from nbdt.tree import Tree

import _seg_ref as S
import _tree_shapes as T

pytestmark = pytest.mark.gpu

TAGS = tuple(S.CASES)
DEV = "cuda:0"
FIELDS = ops.SEG_STATS_FIELDS


def coerce(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def zeros(handle, fields=FIELDS):
    sizes = ops.tree_stats_sizes(handle)
    return {f: torch.zeros(sizes[f], dtype=torch.int64, device=DEV) for f in fields}


def seg_stats(handle, z, y, ignore=S.IGNORE, fields=FIELDS, want_pred=False, block=None):
    block = zeros(handle, fields) if block is None else block
    pred = ops.seg_stats_accumulate(handle, z, y, ignore, block, want_pred=want_pred)
    return {f: t.cpu().numpy() for f, t in block.items()}, pred


def row_stats(handle, z, y, ignore=S.IGNORE):
    """The parent commit's path: nbdt_tree_stats_accumulate on coerce(z), ignored labels set to -1."""
    block = zeros(handle)
    labels = y.reshape(-1).clone()
    labels[labels == ignore] = -1
    ops.tree_stats_accumulate(handle, coerce(z), labels, block)
    assert _C.last_rules_path() in ("lds", "lds-unstaged")
    return {f: t.cpu().numpy() for f, t in block.items()}


def confusion(y, pred, C, ignore=S.IGNORE):
    """np.bincount over the valid pixels of (label, prediction)."""
    y, pred = np.asarray(y).reshape(-1), np.asarray(pred).reshape(-1)
    keep = (y != ignore) & (y >= 0) & (y < C)
    return np.bincount(y[keep] * C + pred[keep], minlength=C * C).astype(np.int64)


def totals_of(y, preds, C, ignore=S.IGNORE):
    y = np.asarray(y).reshape(-1)
    keep = (y != ignore) & (y >= 0) & (y < C)
    return np.array([keep.sum()] + [(np.asarray(p).reshape(-1)[keep] == y[keep]).sum() for p in preds], dtype=np.int64)


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f]), f"{what}: {f}"


# ------------------------------------------------------------------------------------ 1. against the goldens

@pytest.mark.parametrize("tag", TAGS)
def test_against_the_reference(tag):
    tree, _, g = S.case(tag)
    C = tree.flat.num_classes
    assert g["y"].size == 130 and (g["y"] != S.IGNORE).sum() == 40            # the matrices are not trivial
    handle = tree.device_handle(0)
    z = torch.from_numpy(g["z"]).to(DEV)
    y, y_none = torch.from_numpy(g["y"]).to(DEV), torch.from_numpy(g["y_none"]).to(DEV)
    net, hard, soft = g["z"].argmax(1), g["hard"], g["soft"].argmax(1)

    got, pred = seg_stats(handle, z, y, want_pred=True)
    assert _C.last_rules_path() == "pixel"
    assert np.array_equal(got["confusion_net"], confusion(g["y"], net, C))
    assert np.array_equal(got["confusion_hard"], confusion(g["y"], hard, C))
    assert np.array_equal(got["confusion_soft"], confusion(g["y"], soft, C))
    assert np.array_equal(got["totals"], totals_of(g["y"], (net, hard, soft), C)) and got["totals"][0] == 40
    assert np.array_equal(pred[0].cpu().numpy(), net)
    assert np.array_equal(pred[1].cpu().numpy(), hard) and np.array_equal(pred[2].cpu().numpy(), soft)   # ignored too
    assert got["first_error_depth"].sum() == 40 and got["first_error_depth"][-1] == got["totals"][2]

    none, pred = seg_stats(handle, z, y_none, want_pred=True)
    assert all(not v.any() for v in none.values())
    assert np.array_equal(pred[1].cpu().numpy(), hard)
    none, _ = seg_stats(handle, z, y_none)                                   # the whole launch has nothing to count
    assert all(not v.any() for v in none.values())


# ------------------------------------------------------------------------------------ 2. against the row diagnostics

def _shapes(C, seed):
    """The four inputs of tests/test_seg_gpu.py: one pixel per image; a wave and a one-pixel tail; several chunks
    without a tail; a channel-sliced view."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (2.0 * torch.randn(*s, generator=g)).to(DEV)  # noqa: E731
    return {"one_pixel": r(3, C, 1, 1), "tail": r(2, C, 5, 13), "blocks": r(1, C, 16, 24),
            "sliced": r(2, C + 2, 5, 13)[:, 1:C + 1]}


def _targets(z, C, seed, ignore=S.IGNORE):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (z.shape[0], z.shape[2], z.shape[3]), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.3] = ignore
    return y.to(DEV)


def _tree(name, tmp_path):
    if name in TAGS:
        return S.case(name)[0]
    pg, pw, leaves = {"star": lambda: T.star(tmp_path, 37), "caterpillar": lambda: T.caterpillar(tmp_path, 24),
                      "kary3": lambda: T.kary(tmp_path, 50, 3)}[name]()
    return Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)


@pytest.mark.parametrize("name", TAGS + ("star", "caterpillar", "kary3"))
def test_against_the_row_diagnostics(name, tmp_path):
    tree = _tree(name, tmp_path)
    assert _C.seg_stats_fits(tree.flat)
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    seed = 100 + 7 * len(name)
    shapes = _shapes(C, seed)
    for shape, z in shapes.items():
        y = _targets(z, C, seed + 1)
        assert ops.seg_stats_dispatch(tuple(z.shape), tuple(z.stride()), z.dtype, tree.flat) == "pixel", shape
        got, _ = seg_stats(handle, z, y)
        assert _C.last_rules_path() == "pixel", shape
        ref = row_stats(handle, z, y)
        same(got, ref, f"{name} {shape}")
        assert got["totals"][0] == int((y != S.IGNORE).sum()) and (shape != "blocks" or got["node_counts"].any())

    # a persistent grid smaller than the chunks: 6 chunks of 64 pixels on 4 blocks, then on 1
    z = shapes["blocks"]
    y = _targets(z, C, seed + 1)
    ref = row_stats(handle, z, y)
    try:
        for cap in (4, 1):
            assert _C.lib().nbdt_set_seg_stats_max_blocks(cap) == 0
            same(seg_stats(handle, z, y)[0], ref, f"{name} {cap} blocks")
    finally:
        _C.lib().nbdt_set_seg_stats_max_blocks(0)

    z = shapes["tail"]
    # ignore_index = 0, a label inside [0, C)
    y0 = _targets(z, C, seed + 2, ignore=0)
    got, _ = seg_stats(handle, z, y0, ignore=0)
    same(got, row_stats(handle, z, y0, ignore=0), f"{name} ignore_index 0")
    assert not got["confusion_net"].reshape(C, C)[0].any() and got["totals"][0] == int((y0 != 0).sum())

    # a stray label C + 3 that is not the ignore index counts nowhere
    ys = _targets(z, C, seed + 3)
    ys.view(-1)[5], ys.view(-1)[70] = C + 3, C + 3
    got, _ = seg_stats(handle, z, ys)
    same(got, row_stats(handle, z, ys), f"{name} stray label")
    assert got["totals"][0] == int(((ys != S.IGNORE) & (ys < C)).sum())

    # bf16 logits: both sides are fed the same bf16 tensor
    zb = z.to(torch.bfloat16)
    y = _targets(z, C, seed + 4)
    same(seg_stats(handle, zb, y)[0], row_stats(handle, zb, y), f"{name} bf16")

    # channels_last memory takes the row diagnostics without a copy and still agrees
    zl = z.to(memory_format=torch.channels_last)
    assert ops.seg_stats_dispatch(tuple(zl.shape), tuple(zl.stride()), zl.dtype, tree.flat) == "rows"
    ref, _ = seg_stats(handle, z, y)
    got, _ = seg_stats(handle, zl, y)
    assert _C.last_rules_path() in ("lds", "lds-unstaged")
    same(got, ref, f"{name} channels_last")


# ------------------------------------------------------------------------------------ 3. the aggregation paths

def test_one_key_per_wave():
    """Logits and labels constant over the images: every wave holds one (label, prediction) pair, and the single
    non-zero entry of every matrix is the pixel count."""
    tree = S.case("lip")[0]
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    column = 2.0 * torch.randn(C, generator=torch.Generator().manual_seed(3))
    z = column.view(1, C, 1, 1).expand(2, C, 8, 24).contiguous().to(DEV)          # 3 chunks per image
    y = torch.full((2, 8, 24), 11, dtype=torch.int64, device=DEV)
    got, pred = seg_stats(handle, z, y, want_pred=True)
    pixels = 2 * 8 * 24
    for kind, p in zip(("net", "hard", "soft"), pred):
        m = got["confusion_" + kind]
        assert int(p.min()) == int(p.max())
        assert np.count_nonzero(m) == 1 and m[11 * C + int(p[0, 0, 0])] == pixels, kind
    assert got["totals"][0] == pixels and got["first_error_depth"].sum() == pixels
    same(got, row_stats(handle, z, y), "constant")


def test_sixty_four_keys_per_wave():
    """Lane l of every wave has label l mod C and a large logit on class (7 l) mod C, C = 150: the 64 lanes hold 64
    distinct (label, prediction) pairs for the backbone's matrix.  The hard and the soft predictions are the existing
    kernels' (nbdt_seg_hard_forward, argmax of nbdt_seg_soft_forward)."""
    tree = S.case("ade20k")[0]
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    assert C == 150
    N, H, W = 2, 3, 64                                                            # W = 64: a wave is one image row
    lane = torch.arange(W)
    z = 0.5 * torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(4))
    z[:, (lane * 7) % C, :, lane] += 20.0
    y = (lane % C).view(1, 1, W).expand(N, H, W).contiguous()
    z, y = z.to(DEV), y.to(DEV)
    net = z.argmax(1).cpu().numpy()
    assert np.array_equal(net[0, 0], ((lane * 7) % C).numpy()) and len(set(zip(range(W), net[0, 0]))) == 64
    hard = _C.seg_hard_forward(handle, z, want_onehot=False)[0].cpu().numpy()
    soft = _C.seg_soft_forward(handle, z).argmax(1).cpu().numpy()
    got, pred = seg_stats(handle, z, y, want_pred=True)
    yn = y.cpu().numpy()
    assert np.array_equal(got["confusion_net"], confusion(yn, net, C))
    assert np.array_equal(got["confusion_hard"], confusion(yn, hard, C))
    assert np.array_equal(got["confusion_soft"], confusion(yn, soft, C))
    assert np.array_equal(got["totals"], totals_of(yn, (net, hard, soft), C))
    assert np.count_nonzero(got["confusion_net"]) == 64 and (got["confusion_net"][got["confusion_net"] > 0] == N * H).all()
    assert np.array_equal(pred[1].cpu().numpy(), hard) and np.array_equal(pred[2].cpu().numpy(), soft)


# ------------------------------------------------------------------------------------ 4. split invariance

def test_split_invariance():
    tree = S.case("pascal")[0]
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    z = (2.0 * torch.randn(4, C, 5, 13, generator=torch.Generator().manual_seed(5))).to(DEV)
    y = _targets(z, C, 6)
    whole, _ = seg_stats(handle, z, y)
    block = zeros(handle)
    for i in range(4):
        seg_stats(handle, z[i:i + 1], y[i:i + 1], block=block)
    same({f: t.cpu().numpy() for f, t in block.items()}, whole, "image by image")
    block = zeros(handle)
    for lo in (2, 0):
        seg_stats(handle, z[lo:lo + 2], y[lo:lo + 2], block=block)
    same({f: t.cpu().numpy() for f, t in block.items()}, whole, "two halves, the second first")
    same(seg_stats(handle, z, y)[0], whole, "again")


# ------------------------------------------------------------------------------------ 5. the analyzers

def test_analyzers(capsys):
    tree = S.case("lip")[0]
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    gen = torch.Generator().manual_seed(8)
    batches = []
    for n in (2, 3):
        z = (2.0 * torch.randn(n, C, 9, 11, generator=gen)).to(DEV)
        batches.append((z, _targets(z, C, 9 + n)))
    m = {k: np.zeros(C * C, dtype=np.int64) for k in ("net", "hard", "soft")}
    for z, y in batches:
        yn = y.cpu().numpy()
        m["net"] += confusion(yn, z.argmax(1).cpu().numpy(), C)
        m["hard"] += confusion(yn, _C.seg_hard_forward(handle, z, want_onehot=False)[0].cpu().numpy(), C)
        m["soft"] += confusion(yn, _C.seg_soft_forward(handle, z).argmax(1).cpu().numpy(), C)
    m = {k: v.reshape(C, C) for k, v in m.items()}

    stats = G.SegmentationStatistics(tree=tree)
    hard = G.HardSegEmbeddedDecisionRules(tree=tree)
    soft = G.SoftSegEmbeddedDecisionRules(tree=tree)
    for a in (stats, hard, soft):
        a.start_test(0)
        for z, y in batches:
            assert a.update_batch(z, y) is None
        a.end_test(0)
    rep = stats.report()
    for kind in ("net", "hard", "soft"):
        assert np.array_equal(stats.confusion(kind), m[kind])
        assert rep["rules"][kind]["mean_iou"] == G.mean_iou(m[kind])
        assert rep["rules"][kind]["pixel_accuracy"] == G.pixel_accuracy(m[kind])
    assert rep["totals"][0] == int(m["net"].sum()) and sum(rep["first_error_depth"]) == rep["totals"][0]
    assert rep["worst_nodes"] and rep["worst_nodes"][0]["visited_on_path"] > 0
    assert hard.best_accuracy == round(100.0 * G.mean_iou(m["hard"]), 2) and np.array_equal(hard.m, m["hard"])
    assert soft.accuracy() == 100.0 * G.mean_iou(m["soft"])
    assert "[SegNBDT-Hard] mIoU" in capsys.readouterr().out
    z, y = batches[0]
    with pytest.raises(ValueError, match="resize the logits to the label size first"):
        stats.update_batch(z, torch.zeros(2, 18, 22, dtype=torch.int64, device=DEV))

    # the backbone alone: no hierarchy, the star trick of nbdt.diagnostics
    net = G.SegmentationStatistics(classes=tree.classes, rules=("net",))
    net.start_test(0)
    for z, y in batches:
        net.update_batch(z, y)
    assert np.array_equal(net.confusion("net"), m["net"]) and net.totals()[:2] == rep["totals"][:2]


# ------------------------------------------------------------------------------------ 6. beyond the limit

def test_a_hierarchy_between_the_limits_is_refused_by_the_entry_and_routed_by_the_binding(tmp_path):
    """A complete binary tree over 308 classes fits the pixel form but not rows + counters (tests/test_seg_stats.py):
    the C entry refuses it before any launch, ops.seg_stats_accumulate takes the row diagnostics."""
    pg, pw, leaves = T.kary(tmp_path, 308, 2)
    tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
    handle = tree.device_handle(0)
    lib = _C.lib()
    assert lib.nbdt_seg_pixel_fits(handle.h) == 1 and lib.nbdt_seg_stats_fits(handle.h) == 0
    z = (2.0 * torch.randn(1, 308, 5, 13, generator=torch.Generator().manual_seed(10))).to(DEV)
    y = _targets(z, 308, 11)
    block = zeros(handle, ("totals",))
    stats = _C.TreeStats()
    stats.totals = block["totals"].data_ptr()
    rc = lib.nbdt_seg_stats_accumulate(handle.h, _C.ptr(z), 0, 1, 65, 308 * 65, 65, _C.ptr(y), S.IGNORE,
                                       ctypes.byref(stats), None, None, None, None)
    assert rc == -1 and "beyond the segmentation statistics" in lib.nbdt_last_error().decode()
    assert not block["totals"].any()
    got, _ = seg_stats(handle, z, y)
    assert _C.last_rules_path() in ("lds", "lds-unstaged")
    same(got, row_stats(handle, z, y), "coerced")
