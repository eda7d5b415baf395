"""The segmentation classes restated for the tests: the functions of oracle/nbdt_oracle.py (fp32 numpy, the arithmetic
contract of the rules layer) applied to the coerced tensor, which is what the reference's SegNBDT / SoftSegTreeSupLoss do
(nbdt/model.py:376-399, nbdt/loss.py:318-327), plus the masked mean of nn.CrossEntropyLoss(ignore_index=...).

The label-smoothed loss comes from tests/_soft_target_ref.py (float64, pinned to the reference by test_soft_targets.py):
the oracle has no smoothing.  tests/test_seg.py pins everything here to tests/golden/seg_*.npz, recorded from the
unmodified reference by tests/golden/make_seg_golden.py."""
import functools
import os

import numpy as np

import nbdt_oracle as O
import _soft_target_ref as R
from nbdt.tree import Tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IGNORE, TSW = 255, 10.0
CASES = {        # tag -> (dataset, hierarchy, C, N, R, L)
    "lip": ("LookIntoPerson", "induced-HRNet-w48-cls20", 20, 19, 38, 126),
    "pascal": ("PascalContext", "induced-HRNet-w48-cls59", 59, 58, 116, 397),
    "ade20k": ("ADE20K", "induced-HRNet-w48", 150, 149, 298, 1320),
}


def paths(tag):
    dataset, hierarchy = CASES[tag][:2]
    d = os.path.join(GOLDEN, "seg_hierarchies")
    return os.path.join(d, f"{dataset}-graph-{hierarchy}.json"), os.path.join(d, f"{dataset}-wnids.txt")


@functools.lru_cache(maxsize=None)
def case(tag):
    """(nbdt.tree.Tree, OracleTree, golden arrays) of one dataset; loaded once per test session."""
    pg, pw = paths(tag)
    return Tree(CASES[tag][0], path_graph=pg, path_wnids=pw), O.OracleTree(pg, pw), dict(np.load(
        os.path.join(GOLDEN, f"seg_{tag}.npz")))


def coerce(x):
    """[N, C, H, W] -> [N*H*W, C] (reference nbdt/utils.py coerce_tensor)."""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1))).reshape(-1, x.shape[1])


def uncoerce(rows, shape):
    N, _, H, W = shape
    return np.ascontiguousarray(np.transpose(rows.reshape(N, H, W, rows.shape[1]), (0, 3, 1, 2)))


def soft(otree, z):
    """SoftSegNBDT: path probabilities [N, C, H, W] fp32."""
    return uncoerce(O.soft_forward(otree, coerce(z)), z.shape)


def hard(otree, z):
    """HardSegNBDT as labels [N, H, W] int64."""
    return O.hard_forward(otree, coerce(z)).reshape(z.shape[0], z.shape[2], z.shape[3])


def loss(otree, flat, z, y, ignore=IGNORE, tsw=TSW, eps=0.0):
    """SoftSegTreeSupLoss(CrossEntropyLoss(ignore_index, label_smoothing=eps), tree_supervision_weight=tsw):
    (loss, dL/dz [N, C, H, W]) -- the row loss on the valid pixels alone, whose mean is the masked mean."""
    rows, yy = coerce(z), y.reshape(-1)
    keep = np.nonzero(yy != ignore)[0]
    dz = np.zeros(rows.shape, dtype=np.float64)
    if keep.size == 0:
        return float("nan"), uncoerce(dz, z.shape)
    if eps == 0.0:
        value, d = O.soft_tree_sup_loss(otree, rows[keep], yy[keep], 1.0, tsw)
    else:
        value, d = R.soft_loss(flat, rows[keep], yy[keep], eps, 1.0, tsw)
    dz[keep] = d
    return float(value), uncoerce(dz, z.shape)
