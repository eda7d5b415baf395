"""Hierarchies too large for the LDS form of the tree-rule kernels (csrc/rules.hip), and a restatement of the automatic
choice between that form and the global-row form (csrc/rules_global.h).

The shapes come from the generators of tests/_tree_shapes.py; tests/test_large_hierarchy.py asserts without a GPU that
each lies where the LDS form refuses, tests/test_large_hierarchy_gpu.py runs them.

``takes_global`` is copied from ``rules_take_global`` in csrc/rules.hip BY HAND: the global-row form is taken exactly
where the unstaged LDS row of the entry point does not fit, i.e. where ``_tree_shapes.describe`` records ``None``."""
import numpy as np
import torch

import _soft_target_ref as R
import _tree_shapes as S

B = 6
# name -> (generator, arguments)
LARGE = {
    "kary2560_2": ("kary", (2560, 2)),       # the smallest binary tree every entry point refuses
    "star6000": ("star", (6000,)),           # one 6,000-way node: no per-node loop may assume a wave or a block pass
    "kary5000_17": ("kary", (5000, 17)),     # odd fan-out, ragged last groups
    "kary8192_2": ("kary", (8192, 2)),       # iNaturalist-sized
    "kary21841_2": ("kary", (21841, 2)),     # ImageNet-21k-sized: root children of ~11k leaves
}
# the entry points with a global-row form (tree_stats has none)
ENTRY_POINTS = tuple(e for e in S.ENTRY_POINTS if e != "tree_stats")


def build(name, directory):
    gen, args = LARGE[name]
    return S.GENERATORS[gen](directory, *args)


def logits_for(C, batch=B, seed=None):
    """3 * randn, seeded by the shape: the trees here are shallow (depth <= 15), so no path probability gets near the
    1e-30 floor of _assert_P (smallest: 6.6e-17 on the 21,841-class tree)."""
    gen = torch.Generator().manual_seed(C + 1000 * batch if seed is None else seed)
    return (torch.randn(batch, C, generator=gen) * 3).numpy()


def labels_for(C, batch=B):
    y = torch.randint(0, C, (batch,), generator=torch.Generator().manual_seed(7 * C + batch)).numpy()
    y[0] = C - 1
    if batch > 1:
        y[1] = 0
    return y


def takes_global(flat, entry, sched_len):
    """rules_take_global in automatic mode: the unstaged row of `entry` does not fit kLdsBytes."""
    C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
    tps = S.pick_tps(C, R)
    spb = S.block_of(tps) // tps
    tl = S.tree_lds_ints(C, N, R, sched_len, entry == "hard_forward")
    return (tl + spb * S.front_floats(entry, C, N, R) + S.STAGE_PAD) * 4 > S.LDS_BYTES


def expected_path(flat, entry, described):
    """What _C.last_rules_path() reports after a launch of `entry` in automatic mode."""
    if takes_global(flat, entry, described["sched_len"]):
        return "global"
    return "lds" if described["staged"][entry] else "lds-unstaged"


def row_floats(flat):
    """global_row_floats: floats of one block's row in the workspace."""
    C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
    return (C + 2 * R + max(2 * C, 2 * N) + 3) & ~3


def wide_nodes(flat, fan=64):
    """Inner nodes the global-row kernels fold with the whole block (kWideFan)."""
    return np.nonzero(np.diff(flat.node_off) > fan)[0]


# _soft_target_ref restated on a sparse membership matrix.  Its dense float64 [R, C] matrix (and a normalised copy, both
# kept alive under autograd) is 15 GB at 21,841 classes; the matrix has one entry per (slot, leaf), 320k there.  Same
# float64 formulas, operation for operation; tests/test_large_hierarchy.py pins both functions to _soft_target_ref's own
# soft_loss / hard_loss at 1e-12 on kary(243, 3), kary(600, 70) and kary(2560, 2).

def _membership(flat):
    """_soft_target_ref._membership as a sparse [R, C] float64 tensor, and the leaf count of every slot."""
    R_, C = flat.num_slots, flat.num_classes
    counts = np.diff(flat.slot_off).astype(np.int64)
    rows = torch.from_numpy(np.repeat(np.arange(R_, dtype=np.int64), counts))
    cols = torch.from_numpy(flat.slot_cls.astype(np.int64))
    M = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones(len(cols), dtype=torch.float64), (R_, C)).coalesce()
    return M, torch.from_numpy(counts).double()


def _node_logits(z, M, counts):
    return torch.sparse.mm(M, z.T).T / counts            # [B, R]: mean of the child's leaves


def _soft_rules(flat, z, M, counts):
    """_soft_target_ref.soft_rules: per-node log-softmax of the child means, summed along every class's path."""
    S_ = _node_logits(z, M, counts)
    node = torch.from_numpy(np.repeat(np.arange(flat.num_inodes, dtype=np.int64), np.diff(flat.node_off)))
    idx = node.expand(S_.shape[0], -1)
    m = torch.full((S_.shape[0], flat.num_inodes), -np.inf, dtype=torch.float64).scatter_reduce(1, idx, S_.detach(), "amax")
    lse = m + torch.log(torch.zeros_like(m).scatter_add(1, idx, torch.exp(S_ - m[:, node])))
    logp = S_ - lse[:, node]
    return torch.exp(torch.sparse.mm(M.t(), logp.T).T)


def ref_soft_losses(flat, z, targets, w_xent, w_tree):
    """_soft_target_ref.soft_loss for several (target, eps) pairs on one path product: [(loss, dloss/dz), ...]."""
    zt = torch.as_tensor(np.array(z), dtype=torch.float64).requires_grad_(True)
    P = _soft_rules(flat, zt, *_membership(flat))
    out = []
    for target, eps in targets:
        target = torch.as_tensor(np.array(target))
        t = torch.nn.functional.one_hot(target, zt.shape[1]).double() if target.dim() == 1 else target.double()
        t = R.smooth(t, eps)
        T = t.sum(1)
        rows = w_xent * (T * torch.logsumexp(zt, 1) - (t * zt).sum(1)) + w_tree * (T * torch.logsumexp(P, 1) - (t * P).sum(1))
        (dz,) = torch.autograd.grad(rows.mean(), zt, retain_graph=True)
        out.append((rows.mean().item(), dz.numpy()))
    return out


def ref_hard_loss(flat, z, y, eps, w_xent, w_node):
    """_soft_target_ref.hard_loss: the nodes on a label's path are the owners of its slots (class -> slots, ascending), a
    node counted once, for its first child that holds the label."""
    zt = torch.as_tensor(np.array(z), dtype=torch.float64).requires_grad_(True)
    S_ = _node_logits(zt, *_membership(flat))
    C = zt.shape[1]
    rows = []
    for b, yb in enumerate(int(v) for v in np.asarray(y)):
        row = w_xent * (torch.logsumexp(zt[b], 0) - (1.0 - eps) * zt[b, yb] - eps / C * zt[b].sum())
        slots = flat.cls_slot[flat.cls_off[yb]:flat.cls_off[yb + 1]]
        owners = np.searchsorted(flat.node_off, slots, side="right") - 1
        first = {}
        for s, n in zip(slots, owners):
            first.setdefault(int(n), int(s))
        for n in sorted(first):
            lo, hi = int(flat.node_off[n]), int(flat.node_off[n + 1])
            s_n = S_[b, lo:hi]
            row = row + w_node * (torch.logsumexp(s_n, 0) - (1.0 - eps) * S_[b, first[n]] - eps / (hi - lo) * s_n.sum())
        rows.append(row)
    loss = torch.stack(rows).mean()
    loss.backward()
    return loss.item(), zt.grad.numpy()
