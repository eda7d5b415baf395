"""Numpy restatement of the superclass evaluation, in this project's conventions: fp32 throughout, sequential sums in the
listed order, torch's maximum (NaN largest, the first of equal values wins).

What it restates: the reference's ``Superclass.build_mapping`` / ``forward`` / ``_update_batch`` and
``SuperclassNBDT.forward`` (nbdt/analysis.py:482-559), ``get_node_logits`` over an ad-hoc grouping (nbdt/model.py:84-99)
and ``ResampleLabelsDataset.build_index_mapping`` (nbdt/data/custom.py:90-105).  Test infrastructure only: the product
never imports it.  Every value it returns is the EXACT expectation of include/nbdt_hip.h's "superclass evaluation"
section -- nothing here needs a tolerance.
"""
import random

import numpy as np

MASKED, GROUP_MEAN = 0, 1
F32 = np.float32


def bf16_round(a):
    """fp32 array rounded to bf16 (nearest even) and widened back: the values a bf16 tensor of `a` holds."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def build_mapping(dataset_wnids, superclass_wnids, hypernyms):
    """(mapping list, {value: [old indices]}): the first listed superclass among a class's hypernyms-or-self, else -1."""
    mapping, new_to_old = [], {}
    for old, wnid in enumerate(dataset_wnids):
        own = set(hypernyms[wnid]) | {wnid}
        value = -1
        for new, sup in enumerate(superclass_wnids):
            if sup in own:
                value = new
                break
        mapping.append(value)
        new_to_old.setdefault(value, []).append(old)
    return mapping, new_to_old


def group_logits(z, groups):
    """[B, G] fp32: per group the sequential fp32 sum of its members in the listed order, from 0.0f, then one division by
    the member count (0 / 0 = NaN for an empty group)."""
    z = np.asarray(z, dtype=F32)
    out = np.empty((z.shape[0], len(groups)), dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g, members in enumerate(groups):
            acc = np.zeros(z.shape[0], dtype=F32)
            for c in members:
                acc = (acc + z[:, c]).astype(F32)
            out[:, g] = acc / F32(len(members))
    return out


def group_logits_backward(gs, groups, num_classes):
    """[B, C] fp32: per class the sequential sum, over the groups holding it in ascending group index and from 0.0f, of
    gs[:, g] / n_g (one fp32 division per term)."""
    gs = np.asarray(gs, dtype=F32)
    gz = np.zeros((gs.shape[0], num_classes), dtype=F32)
    for g, members in enumerate(groups):           # ascending g: every class meets its groups in ascending order
        term = (gs[:, g] / F32(len(members))).astype(F32) if members else None
        for c in members:
            gz[:, c] = (gz[:, c] + term).astype(F32)
    return gz


def first_max(row):
    """torch's argmax: the first NaN if there is one, else the first of the largest values."""
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def predictions(z, mode, map_pred, groups):
    z = np.asarray(z, dtype=F32)
    if mode == MASKED:
        masked = z.copy()
        masked[:, np.asarray(map_pred) < 0] = F32(-100.0)
        return np.array([map_pred[first_max(r)] for r in masked], dtype=np.int64)
    return np.array([first_max(r) for r in group_logits(z, groups)], dtype=np.int64)


def accumulate(z, y, map_target, map_pred, groups, mode, totals=None, confusion=None):
    """(totals [2], confusion [G, G], pred [B]) after adding one batch to the given counters (zeros when None)."""
    G = len(groups)
    totals = np.zeros(2, dtype=np.int64) if totals is None else np.array(totals, dtype=np.int64)
    confusion = np.zeros((G, G), dtype=np.int64) if confusion is None else np.array(confusion, dtype=np.int64).reshape(G, G)
    pred = predictions(z, mode, map_pred, groups)
    for b, label in enumerate(np.asarray(y).tolist()):
        t = map_target[label] if 0 <= label < len(map_target) else -1
        if t < 0:
            continue
        totals[0] += 1
        totals[1] += int(pred[b] == t)
        if pred[b] >= 0:
            confusion[t, pred[b]] += 1
    return totals, confusion, pred


def label_subset(labels, p, seed=0):
    """The reference's build_index_mapping with the module-level generator it uses: random.seed(seed), one
    random.random() per sample in dataset order, kept when below p[label]."""
    state = random.getstate()
    try:
        random.seed(seed)
        return [i for i, label in enumerate(labels) if random.random() < p[label]]
    finally:
        random.setstate(state)
