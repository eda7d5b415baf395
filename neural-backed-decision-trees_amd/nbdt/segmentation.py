"""Evaluation of segmentation NBDTs: confusion matrices, pixel accuracy, mIoU and the per-node statistics of a test
pass over ``[N, C, H, W]`` logits and ``[N, H, W]`` label maps with an ``ignore_index``.

The analyzers speak the hook protocol of ``nbdt.analysis.Noop`` and are fed by ONE launch per evaluation batch,
``nbdt_seg_stats_accumulate`` (csrc/seg_stats.h): the per-pixel twin of the launch behind ``nbdt.diagnostics``.  It forms
the child logits once, takes the backbone's argmax, the hard walk and the argmax of the soft path product from them and
adds into int64 counters on the device; no probability tensor is written and ``update_batch`` never waits for the GPU.
The first host transfer is in ``end_test`` or an explicit accessor.

The reference has no counterpart: its ``ConfusionMatrix`` skips every prediction that is not 1-D (nbdt/analysis.py:150).
The metric functions at the top work on any int64 confusion matrix ``m[label, prediction]`` and need no device.

Not here: bilinear upsampling of the logits to the label size (resize them first), segmentation backbones and datasets,
colour-map dumps, per-node entropy sums.
"""
import json
import math

import numpy as np
import torch

from nbdt import _C, ops
from nbdt.diagnostics import KINDS, _Fused, _jsonable, node_rows, worst_nodes
from nbdt.tree import Tree

__all__ = names = ("SegmentationStatistics", "HardSegEmbeddedDecisionRules", "SoftSegEmbeddedDecisionRules")


# ------------------------------------------------------------------------------------------------------------
# metrics of a confusion matrix m[label, prediction]: integer ratios formed in float64, no device needed

def _square(m):
    a = np.asarray(m)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"a confusion matrix is square [classes, classes], got shape {a.shape}")
    return a.astype(np.int64)


def _over(num, den):
    """num / den in float64, NaN where den is 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den != 0)


def pixel_accuracy(m):
    """Correct pixels over counted pixels; NaN for an empty matrix."""
    a = _square(m)
    return float(_over(np.trace(a), a.sum()))


def class_accuracy(m):
    """Per class: correct pixels over the pixels labelled with it (recall); NaN for a class without label pixels."""
    a = _square(m)
    return _over(np.diagonal(a), a.sum(axis=1))


def mean_class_accuracy(m):
    """Mean of class_accuracy over the classes that have label pixels; NaN when there is none."""
    acc = class_accuracy(m)
    seen = ~np.isnan(acc)
    return float(acc[seen].mean()) if seen.any() else math.nan


def iou(m):
    """Per class: intersection over union = m[c, c] / (label pixels + predicted pixels - m[c, c]); NaN where label
    pixels + predicted pixels = 0."""
    a = _square(m)
    hit = np.diagonal(a)
    return _over(hit, a.sum(axis=1) + a.sum(axis=0) - hit)


def classes_with_union(m):
    """How many classes mean_iou averages over: those with a label pixel or a predicted pixel."""
    return int((~np.isnan(iou(m))).sum())


def mean_iou(m):
    """Mean of iou over the classes with a non-empty union; NaN when there is none."""
    v = iou(m)
    seen = ~np.isnan(v)
    return float(v[seen].mean()) if seen.any() else math.nan


def frequency_weighted_iou(m):
    """Sum over the classes with label pixels of (label pixels / counted pixels) * iou; NaN for an empty matrix."""
    a = _square(m)
    total = int(a.sum())
    if total == 0:
        return math.nan
    label = a.sum(axis=1)
    v = iou(a)
    return float((label[label > 0] * v[label > 0]).sum() / total)


def metrics(m, classes=None):
    """All of the above for one matrix, as the JSON-able dict the analyzers report."""
    a = _square(m)
    names_ = list(classes) if classes else [str(c) for c in range(a.shape[0])]
    return _jsonable({
        "pixels": int(a.sum()), "pixel_accuracy": pixel_accuracy(a), "mean_class_accuracy": mean_class_accuracy(a),
        "mean_iou": mean_iou(a), "classes_in_mean_iou": classes_with_union(a),
        "frequency_weighted_iou": frequency_weighted_iou(a),
        "iou": [{"class": name, "iou": float(v)} for name, v in zip(names_, iou(a))]})


# ------------------------------------------------------------------------------------------------------------
# device side

def _check_batch(outputs, targets):
    if outputs.dim() != 4:
        raise ValueError(f"segmentation analyzers take [N, C, H, W] logits, got shape {tuple(outputs.shape)}")
    if targets.dim() != 3 or targets.shape[0] != outputs.shape[0]:
        raise ValueError(f"segmentation targets are label maps [N, H, W]; got {tuple(targets.shape)} for logits "
                         f"{tuple(outputs.shape)}")
    if tuple(targets.shape[1:]) != tuple(outputs.shape[2:]):
        raise ValueError(f"targets are {tuple(targets.shape[1:])} but the logits are {tuple(outputs.shape[2:])}: resize "
                         f"the logits to the label size first (e.g. F.interpolate(outputs, size=targets.shape[1:], "
                         f"mode='bilinear')); the launch does not upsample")


class _SegFused(_Fused):
    """One block of int64 counters per test pass, filled by one nbdt_seg_stats_accumulate launch per batch.  State,
    merge and reduce are those of the fused diagnostics: the counters as numpy int64, summed exactly."""

    accepts_tree = lambda tree, **kwargs: tree                                        # noqa: E731
    accepts_dataset = lambda trainset, **kwargs: trainset.__class__.__name__          # noqa: E731
    accepts_path_graph = True
    accepts_path_wnids = True

    def __init__(self, classes, tree, ignore_index):
        super().__init__(classes, tree=tree)
        self.ignore_index = int(ignore_index)

    def update_batch(self, outputs, targets, images=None):
        """Enqueues one launch and returns None: nothing here waits for the GPU."""
        _check_batch(outputs, targets)
        _C.require_gpu(outputs, type(self).__name__)
        dev = outputs.device
        handle = self._handle(dev)
        if self._block is not None and any(t.device != dev for t in self._block.values()):
            self._block = None
        if self._block is None:
            sizes = ops.tree_stats_sizes(handle)
            self._block = {f: torch.zeros(sizes[f], dtype=torch.int64, device=dev) for f in self.fields}
        self._host = None
        with torch.no_grad():
            ops.seg_stats_accumulate(handle, outputs.detach(), targets, self.ignore_index, self._block)
        return None

    def confusion(self, kind):
        """[label, prediction] pixel counts of the pass for the backbone ("net"), the hard or the soft rules."""
        c = self.counts()
        if "confusion_" + kind not in c:
            raise ValueError(f"{type(self).__name__} counts {[f for f in self.fields if f.startswith('confusion_')]}, "
                             f"not the {kind!r} rules")
        return c["confusion_" + kind].reshape(self.num_classes, self.num_classes)

    def _counted(self):
        return self._block is not None or self._host is not None


class SegmentationStatistics(_SegFused):
    """Pixel accuracy, mean class accuracy, mIoU, frequency-weighted IoU and per-class IoU of the backbone, the hard and
    the soft rules over a test pass, plus -- with the hard rules -- which inner node makes the pixel errors
    (``worst_nodes``) and at what depth a pixel's walk first leaves its label's path.  ``rules=("net",)`` needs no
    hierarchy, only ``classes``."""

    name = "SegmentationStatistics"

    def __init__(self, dataset=None, path_graph=None, path_wnids=None, classes=(), tree=None, hierarchy=None,
                 ignore_index=255, rules=KINDS, worst=5, min_support=1):
        rules = tuple(rules)
        if not rules or any(r not in KINDS for r in rules):
            raise ValueError(f"rules must be chosen from {KINDS}, got {rules!r}")
        if tree is None and rules != ("net",):
            tree = Tree(dataset, path_graph=path_graph, path_wnids=path_wnids, classes=list(classes) or None,
                        hierarchy=hierarchy)
        if tree is None and not classes:
            raise ValueError("the backbone's statistics need `classes` (or a tree)")
        super().__init__(tree.classes if tree is not None else classes, tree, ignore_index)
        self.rules = rules
        self.with_nodes = tree is not None and "hard" in rules
        self.fields = ("totals",) + tuple("confusion_" + r for r in rules) + (
            ("node_counts", "first_error_depth") if self.with_nodes else ())
        self.worst, self.min_support = int(worst), int(min_support)

    def totals(self):
        """[valid pixels, backbone hits, hard hits, soft hits]"""
        return [int(v) for v in self.counts()["totals"]]

    def node_table(self):
        if not self.with_nodes:
            raise ValueError("the per-node counters belong to the hard rules: build with a tree and 'hard' in rules")
        c = self.counts()
        rows = node_rows(self.tree, c["node_counts"], np.zeros(2 * len(self.tree.inodes), dtype=np.int64),
                         int(c["totals"][0]))
        for r in rows:                       # the entropy sums are not part of the segmentation statistics
            del r["entropy_mean"], r["entropy_std"]
        return rows

    def first_error_histogram(self):
        """List over depths d (root 0) of the pixels whose hard walk first leaves the label's path at d; the last entry
        counts the pixels that never leave it."""
        return [int(v) for v in self.counts()["first_error_depth"]]

    def report(self):
        out = {"ignore_index": self.ignore_index, "totals": self.totals(),
               "rules": {r: metrics(self.confusion(r), self.classes) for r in self.rules}}
        if self.with_nodes:
            rows = self.node_table()
            out["worst_nodes"] = worst_nodes(rows, self.worst, self.min_support)
            out["first_error_depth"] = self.first_error_histogram()
            out["counts"] = {"node_counts": self.counts()["node_counts"].tolist()}
        return _jsonable(out)

    def to_json(self, path):
        with open(path, "w") as f:
            json.dump(self.report(), f, indent=1, allow_nan=False)

    def end_test(self, epoch):
        super().end_test(epoch)
        if not (self.verbose and self._counted()):
            return
        print(f"[{self.name}] {self.totals()[0]} valid pixels (ignore_index {self.ignore_index})")
        for r in self.rules:
            m = self.confusion(r)
            print(f"[{self.name}] {r:>4}: pixel acc {100 * pixel_accuracy(m):.2f}% | class acc "
                  f"{100 * mean_class_accuracy(m):.2f}% | mIoU {100 * mean_iou(m):.2f}% over {classes_with_union(m)} "
                  f"classes | fwIoU {100 * frequency_weighted_iou(m):.2f}%")
            for name, v in zip(self.classes, iou(m)):
                print(f"[{self.name}]       {name}: IoU {100 * v:.2f}%")
        if self.with_nodes:
            print(f"[{self.name}] first wrong turn by depth: {self.first_error_histogram()[:-1]}")
            for r in worst_nodes(self.node_table(), self.worst, self.min_support):
                print(f"[{self.name}]   {r['wnid']} ({r['name']}) depth {r['depth']}: "
                      f"{100.0 * r['accuracy_given_arrival']:.2f}% of {r['visited_on_path']} arrivals")


class _SegDecisionRules(_SegFused):
    """mIoU and pixel accuracy of ONE rule over a test pass, with the surface of nbdt.analysis.DecisionRules:
    ``accuracy()`` is the mIoU in percent and ``best_accuracy`` its best value over the epochs."""

    kind = "hard"

    def __init__(self, dataset=None, path_graph=None, path_wnids=None, classes=(), tree=None, hierarchy=None,
                 ignore_index=255):
        tree = tree or Tree(dataset, path_graph=path_graph, path_wnids=path_wnids, classes=list(classes) or None,
                            hierarchy=hierarchy)
        super().__init__(tree.classes, tree, ignore_index)
        self.fields = ("confusion_" + self.kind,)
        self.best_accuracy = 0.0

    @property
    def m(self):
        return self.confusion(self.kind)

    def accuracy(self):
        """mIoU in percent (0 before any pixel is counted)."""
        v = mean_iou(self.m) if self._counted() else math.nan
        return 0.0 if math.isnan(v) else 100.0 * v

    def pixel_accuracy(self):
        v = pixel_accuracy(self.m) if self._counted() else math.nan
        return 0.0 if math.isnan(v) else 100.0 * v

    def report(self):
        return _jsonable({"kind": self.kind, **metrics(self.m, self.classes)})

    def end_test(self, epoch):
        super().end_test(epoch)
        acc = round(self.accuracy(), 2)
        self.best_accuracy = max(self.best_accuracy, acc)
        if self.verbose:
            print(f"[{self.name}] mIoU {acc}%, pixel accuracy {round(self.pixel_accuracy(), 2)}%; best mIoU so far "
                  f"{self.best_accuracy}%")


class HardSegEmbeddedDecisionRules(_SegDecisionRules):
    """Greedy root-to-leaf walk per pixel."""

    name = "SegNBDT-Hard"
    kind = "hard"


class SoftSegEmbeddedDecisionRules(_SegDecisionRules):
    """Argmax of the path-probability product per pixel."""

    name = "SegNBDT-Soft"
    kind = "soft"
