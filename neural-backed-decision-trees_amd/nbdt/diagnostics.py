"""Tree diagnostics: which inner node makes the mistakes, at what depth a sample leaves its label's path, which classes
get confused after the walk, how uncertain every node is.

The analyzers of the reference's ``nbdt/analysis.py`` that ``nbdt.analysis`` leaves out -- ``ConfusionMatrix`` (:133-180),
``Entropy`` / ``NBDTEntropyMaxMin`` (:324-389), ``TopDifference`` (:421-427) -- plus ``TreeStatistics``, the per-node
statistics the reference does not have.  All of them speak the hook protocol of ``nbdt.analysis.Noop`` and are fed by the
fused launch ``nbdt_tree_stats_accumulate`` (csrc/rules.hip), which adds into int64 counters on the device: an analyzer
on its own does one launch per evaluation batch, and the members of a ``Chain`` that are on one hierarchy share ONE
launch and one block of counters.  ``update_batch`` only enqueues work, the first host transfer is in ``end_test`` or
an explicit accessor.

Not here: image dumps (``highest`` / ``lowest`` return tensors; writing JPEGs is presentation), ``TopEntropy``,
``NBDTEntropyBottom`` (scores only the last sample of a batch in the reference), ``IgnoredSamples``.  ``Superclass`` and
``SuperclassNBDT`` (zero-shot evaluation on superclasses) are in ``nbdt.superclass``.
"""
import json
import math
from types import SimpleNamespace

import numpy as np
import torch

from nbdt import _C, ops
from nbdt.analysis import Noop, merge_sum
from nbdt.tree import Tree

__all__ = names = ("TreeStatistics", "ConfusionMatrix", "Entropy", "TopDifference", "NBDTEntropyMaxMin")

COUNTERS = ("on_path", "on_path_right", "visited", "visited_on_path", "visited_on_path_right")
KINDS = ("net", "hard", "soft")
_SCORE_COLUMN = {"Entropy": 0, "TopDifference": 1, "NBDTEntropyMaxMin": 2}
SUMS_DTYPE = torch.float64     # Entropy's running sum and sum of squares (the only floating accumulators here)


# ------------------------------------------------------------------------------------------------------------
# report arithmetic on host arrays (no device needed)

def _ratio(a, b):
    return float(a) / float(b) if b else math.nan


def node_rows(tree, node_counts, node_entropy, valid):
    """One dict per inner node (``tree.inodes`` order) from the int64 blocks ``node_counts`` [N, 5] and ``node_entropy``
    [N, 2] (fixed point, units of 2^-32) of a pass over ``valid`` labelled samples."""
    counts = np.asarray(node_counts, dtype=np.int64).reshape(-1, 5)
    sums = np.asarray(node_entropy, dtype=np.int64).reshape(-1, 2)
    depth = inode_depths(tree)
    rows = []
    for i, node in enumerate(tree.inodes):
        c = dict(zip(COUNTERS, (int(v) for v in counts[i])))
        mean = _ratio(int(sums[i, 0]) / ops.ENTROPY_ONE, valid)
        square = _ratio(int(sums[i, 1]) / ops.ENTROPY_ONE, valid)
        rows.append({
            "index": i, "wnid": node.wnid, "name": node.name, "depth": depth[i], "children": node.num_children, **c,
            # of the samples the walk brought here while still on the label's path, the share sent on correctly
            "accuracy_given_arrival": _ratio(c["visited_on_path_right"], c["visited_on_path"]),
            # of all samples whose label lies under the node, the share its own decision would send on correctly
            "accuracy_all": _ratio(c["on_path_right"], c["on_path"]),
            "entropy_mean": mean,
            "entropy_std": math.sqrt(max(square - mean * mean, 0.0)) if valid else math.nan,
        })
    return rows


def inode_depths(tree):
    """Depth of every inner node (root 0; the shortest way down where a node has several parents), -1 if unreachable."""
    index = {n.wnid: i for i, n in enumerate(tree.inodes)}
    depth = [-1] * len(index)
    frontier, d = [tree.root.wnid], 0
    while frontier:
        nxt = []
        for w in frontier:
            if depth[index[w]] >= 0:
                continue
            depth[index[w]] = d
            nxt.extend(c for c in tree.wnid_to_node[w].succ if c in index)
        frontier, d = nxt, d + 1
    return depth


def accuracies(totals):
    """Percent correct of the backbone, the hard rules and the soft rules over the valid samples."""
    t = [int(v) for v in totals]
    return {kind: _ratio(100.0 * t[1 + i], t[0]) for i, kind in enumerate(KINDS)}


def worst_nodes(rows, k=5, min_support=1):
    """The k nodes with the lowest accuracy given a correct arrival, among those with at least ``min_support`` such
    arrivals (ties: the node that saw more samples first, then inode order)."""
    seen = [r for r in rows if r["visited_on_path"] >= max(int(min_support), 1)]
    seen.sort(key=lambda r: (r["accuracy_given_arrival"], -r["visited_on_path"], r["index"]))
    return seen[:k]


def normalize(matrix, axis):
    """reference ConfusionMatrix.normalize (:170-174): rows (axis 1, recall) or columns (axis 0, precision) sum to 1;
    a class that never occurs gives nan."""
    m = np.asarray(matrix, dtype=np.float64)
    total = m.sum(axis=axis)
    total = total[:, None] if axis == 1 else total[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return m / total


def _jsonable(v):
    if isinstance(v, float) and not math.isfinite(v):
        return None
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.generic):
        return _jsonable(v.item())
    return v


# ------------------------------------------------------------------------------------------------------------
# device side

def _star_flat(num_classes):
    """The trivial hierarchy (a root with one leaf child per class) as the flat CSR form: what an analyzer that only
    looks at the backbone's logits hands to the kernel when it was given no tree."""
    C = int(num_classes)
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))  # noqa: E731
    ramp = np.arange(C + 1)
    return SimpleNamespace(num_classes=C, num_inodes=1, num_slots=C, root=0, node_off=i32([0, C]), slot_off=i32(ramp),
                           slot_cls=i32(ramp[:C]), cls_off=i32(ramp), cls_slot=i32(ramp[:C]),
                           slot_next=i32(-ramp[:C] - 1), inode_wnids=["root"], multi_path_node=None)


def _launch(members, outputs, targets, images=None):
    """Feeds one batch to every analyzer of ``members`` with as few launches as their hierarchies allow: the members
    that share a tree (analyzers without one ride along: what they ask for does not depend on the hierarchy) get ONE
    nbdt_tree_stats_accumulate launch into one block of counters -- a field two of them want is one tensor -- and one
    scores tensor; a member on another tree, or whose counters are not the group's, launches on its own."""
    _C.require_gpu(outputs, type(members[0]).__name__)
    dev = outputs.device
    tree = next((m.tree for m in members if m.tree is not None), None)
    group = [m for m in members if m.tree is None or m.tree is tree]
    for m in members:
        if m not in group:
            _launch([m], outputs, targets, images)
    shared = {}
    for m in group:
        if m._block is not None and any(t.device != dev for t in m._block.values()):
            m._block = None
        for f, t in (m._block or {}).items():
            if shared.setdefault(f, t) is not t:            # counted apart so far: keep them apart
                for lone in group:
                    _launch([lone], outputs, targets, images)
                return
    handle = tree.device_handle(dev.index) if tree is not None else group[0]._handle(dev)
    sizes = ops.tree_stats_sizes(handle)
    for m in group:           # members of a group are started together (Chain.start_test): a field is one tensor
        for f in m.fields:
            if f not in shared:
                shared[f] = torch.zeros(sizes[f], dtype=torch.int64, device=dev)
        if m.fields:
            m._block = {f: shared[f] for f in m.fields}
        m._host = None
    scores = None
    if any(m.wants_scores for m in group):
        scores = torch.empty((outputs.shape[0], 3), dtype=torch.float32, device=dev)
    with torch.no_grad():
        ops.tree_stats_accumulate(handle, outputs, targets if shared else None, shared, scores)
        for m in group:
            if m.wants_scores:
                m._absorb(scores, images)


class _Fused(Noop):
    """Shared plumbing: the hierarchy handle per device and one zeroed block of counters per test pass."""

    fields = ()            # nbdt_tree_stats fields this analyzer asks the kernel for
    wants_scores = False   # ... and whether it wants the per-sample scores

    def __init__(self, classes=(), tree=None):
        self.tree = tree
        super().__init__(classes if classes else (tree.classes if tree is not None else ()))
        self._handles = {}
        self._block = None
        self._host = None

    def _handle(self, device):
        if self.tree is not None:
            return self.tree.device_handle(device.index)
        h = self._handles.get(device.index)
        if h is None:
            h = self._handles[device.index] = _C.TreeHandle(_star_flat(self.num_classes), device.index)
        return h

    def start_test(self, epoch):
        self.epoch = epoch           # an eval-only driver has no enclosing start_epoch (as nbdt.analysis.DecisionRules)
        super().start_test(epoch)
        self._block = None
        self._host = None

    def update_batch(self, outputs, targets, images=None):
        """Enqueues one launch and returns None: nothing here waits for the GPU."""
        _launch([self], outputs, targets, images)
        return None

    def load_counts(self, counts):
        """Adopt a block of counters that is already on the host (a dict of integer arrays by nbdt_tree_stats field
        name), e.g. one read back from ``to_json`` or summed over several processes."""
        self._host = {k: np.asarray(v, dtype=np.int64).ravel().copy() for k, v in counts.items()}
        return self

    def counts(self):
        """The pass's counters as int64 numpy arrays by field name (the host transfer happens here, once)."""
        if self._host is None:
            if self._block is None:
                raise RuntimeError(f"{type(self).__name__}: no batch has been counted since start_test")
            self._host = {k: v.cpu().numpy() for k, v in self._block.items()}
        return self._host

    # distributed evaluation (nbdt.analysis.Noop.reduce): the counters are integers, so the merge is an exact sum
    def state(self, counts=True):
        """counts=False leaves the counters out (``"counts": None``): a Chain sends a block its members share once."""
        if not counts:
            return {"counts": None}
        have = self.fields and (self._host is not None or self._block is not None)
        return {"counts": {k: v.copy() for k, v in self.counts().items()} if have else {}}

    def load_state(self, state):
        if state.get("counts"):
            self.load_counts(state["counts"])


class TreeStatistics(_Fused):
    """Per-node accuracy and entropy, the depth of the first wrong turn and the three confusion matrices of a test
    pass.  ``confusions=False`` leaves the C x C matrices out (3 x 8 MB of counters at 1000 classes)."""

    accepts_tree = lambda tree, **kwargs: tree                                        # noqa: E731
    accepts_dataset = lambda trainset, **kwargs: trainset.__class__.__name__          # noqa: E731
    accepts_path_graph = True
    accepts_path_wnids = True
    name = "TreeStatistics"

    def __init__(self, tree=None, dataset=None, path_graph=None, path_wnids=None, hierarchy=None, classes=None,
                 confusions=True, worst=5, min_support=1):
        tree = tree or Tree(dataset, path_graph=path_graph, path_wnids=path_wnids, classes=classes, hierarchy=hierarchy)
        super().__init__(tree.classes, tree=tree)
        self.fields = ("totals", "node_counts", "node_entropy", "first_error_depth") + (
            ("confusion_net", "confusion_hard", "confusion_soft") if confusions else ())
        self.worst, self.min_support = int(worst), int(min_support)

    def totals(self):
        return [int(v) for v in self.counts()["totals"]]

    def node_table(self):
        c = self.counts()
        return node_rows(self.tree, c["node_counts"], c["node_entropy"], int(c["totals"][0]))

    def first_error_histogram(self):
        """List over depths d (root 0) of the samples whose hard walk first leaves the label's path at d; the last
        entry counts the samples that never leave it (the hard rules' hits)."""
        return [int(v) for v in self.counts()["first_error_depth"]]

    def confusion(self, kind="hard"):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        c = self.counts()
        if "confusion_" + kind not in c:
            raise RuntimeError("TreeStatistics was built with confusions=False")
        return c["confusion_" + kind].reshape(self.num_classes, self.num_classes)

    def summary(self, k=None, min_support=None):
        rows = self.node_table()
        t = self.totals()
        return {"samples": t[0], "accuracy": accuracies(t),
                "worst_nodes": worst_nodes(rows, self.worst if k is None else k,
                                           self.min_support if min_support is None else min_support)}

    def report(self):
        c = self.counts()
        out = {"totals": self.totals(), "accuracy": accuracies(c["totals"]),
               "first_error_depth": self.first_error_histogram(), "nodes": self.node_table(),
               "counts": {k: c[k].tolist() for k in ("node_counts", "node_entropy")}}
        return _jsonable(out)

    def to_json(self, path):
        with open(path, "w") as f:
            json.dump(self.report(), f, indent=1, allow_nan=False)

    def end_test(self, epoch):
        super().end_test(epoch)
        if self.verbose and self._block is not None:
            s = self.summary()
            acc = s["accuracy"]
            print(f"[{self.name}] {s['samples']} samples | backbone {acc['net']:.2f}% | hard rules {acc['hard']:.2f}% | "
                  f"soft rules {acc['soft']:.2f}%")
            print(f"[{self.name}] first wrong turn by depth: {self.first_error_histogram()[:-1]}")
            for r in s["worst_nodes"]:
                print(f"[{self.name}]   {r['wnid']} ({r['name']}) depth {r['depth']}: "
                      f"{100.0 * r['accuracy_given_arrival']:.2f}% of {r['visited_on_path']} arrivals, "
                      f"entropy {r['entropy_mean']:.3f} +- {r['entropy_std']:.3f}")


class ConfusionMatrix(_Fused):
    """reference nbdt/analysis.py:133-180.  ``ConfusionMatrix(classes)`` counts the backbone's predictions; with a
    ``tree`` it counts the hard rules' (``kind="hard"``, the default then) or the soft rules' predictions."""

    name = "ConfusionMatrix"

    def __init__(self, classes=(), tree=None, kind=None):
        super().__init__(classes, tree=tree)
        self.kind = kind or ("hard" if tree is not None else "net")
        if self.kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {self.kind!r}")
        if self.kind != "net" and tree is None:
            raise ValueError(f"the {self.kind} rules' confusion matrix needs a tree")
        self.fields = ("confusion_" + self.kind,)
        self.k = self.num_classes

    def start_train(self, epoch):
        super().start_train(epoch)
        raise NotImplementedError()

    @property
    def m(self):
        """[label, prediction] counts of the pass."""
        return self.counts()[self.fields[0]].reshape(self.k, self.k)

    normalize = staticmethod(normalize)

    def recall(self):
        return normalize(self.m, 1)

    def precision(self):
        return normalize(self.m, 0)

    def report(self):
        return _jsonable({"kind": self.kind, "matrix": self.m.tolist()})

    def end_test(self, epoch):
        super().end_test(epoch)
        if self.verbose and self._block is not None:
            recall = self.recall()
            for row, cls in zip(recall, self.classes):
                print(row, cls)
            print(recall.diagonal(), "(diagonal)")


def merge_topk(candidates, k, largest):
    """The k best of several lists of ranked samples: ``candidates`` is a sequence of ``{"score": [n], "index": [n],
    "images": [n, ...] or None}`` (None entries are skipped); returns one such dict, best first.  The order is total: by
    score (the largest or the smallest first), then by the smaller sample index.  So as long as every list holds the k
    best of what its rank saw, under this order, the result does not depend on how the samples were split into lists."""
    candidates = [c for c in candidates if c is not None and len(c["score"])]
    if not candidates:
        return None
    score = torch.cat([torch.as_tensor(c["score"]).reshape(-1) for c in candidates])
    index = torch.cat([torch.as_tensor(c["index"]).reshape(-1).long() for c in candidates])
    with_images = [c.get("images") is not None for c in candidates]
    if any(with_images) and not all(with_images):
        raise ValueError("some ranked samples come with images and some without")
    images = torch.cat([torch.as_tensor(c["images"]) for c in candidates]) if all(with_images) else None
    pick = _rank_order(score, index, largest)[:int(k)]
    return {"score": score[pick], "index": index[pick], "images": images[pick] if images is not None else None}


def _rank_order(score, index, largest):
    """The permutation that puts (score, index) into ranking order: two stable sorts, the minor key first."""
    by_index = torch.sort(index, stable=True).indices
    by_score = torch.sort(score[by_index], stable=True, descending=largest).indices
    return by_index[by_score]


class _Ranking(_Fused):
    """Keeps the ``save_k`` highest and lowest scorers of a pass on the device: their score, their ordinal within the
    pass and, when ``update_batch`` is given images, the image.  Equal scores rank by ordinal, the earlier sample first.
    In a distributed evaluation the ordinal is the sample's index in the whole split (``set_sample_offset``)."""

    def __init__(self, classes=(), tree=None, save_k=20):
        super().__init__(classes, tree=tree)
        self.save_k = int(save_k)
        self.column = _SCORE_COLUMN[type(self).__name__]
        self._reset()

    def _reset(self):
        self._seen = 0
        self._next = 0                              # ordinal of the next sample (set_sample_offset moves it)
        self._top = {True: None, False: None}      # largest?: (scores, ordinals, images or None)

    def set_sample_offset(self, offset):
        self._next = int(offset)

    def start_test(self, epoch):
        super().start_test(epoch)
        self._reset()

    wants_scores = True

    def _absorb(self, scores, images):
        B = scores.shape[0]
        if self._seen and (images is None) != (self._top[True][2] is None):
            raise ValueError(f"{type(self).__name__}: give images with every batch of a pass, or with none")
        self._observe(scores)
        ordinals = torch.arange(self._next, self._next + B, device=scores.device)
        for largest in (True, False):
            self._top[largest] = self._retain(self._top[largest], scores[:, self.column], ordinals, images, largest)
        self._seen += B
        self._next += B

    def _observe(self, scores):
        pass

    def _retain(self, kept, score, ordinal, images, largest):
        if kept is not None:
            score, ordinal = torch.cat((kept[0], score)), torch.cat((kept[1], ordinal))
            images = torch.cat((kept[2], images)) if images is not None else None
        pick = _rank_order(score, ordinal, largest)[:self.save_k]
        return score[pick], ordinal[pick], (images[pick] if images is not None else None)

    def state(self, counts=True):
        out = {**super().state(counts), "seen": self._seen}
        for key, kept in (("highest", self._top[True]), ("lowest", self._top[False])):
            out[key] = None if kept is None else {"score": kept[0].cpu(), "index": kept[1].cpu(),
                                                  "images": kept[2].cpu() if kept[2] is not None else None}
        return out

    def merge(self, states):
        out = {"counts": merge_sum([s.get("counts") for s in states]), "seen": sum(int(s["seen"]) for s in states)}
        for key, largest in (("highest", True), ("lowest", False)):
            out[key] = merge_topk([s[key] for s in states], self.save_k, largest)
        return out

    def load_state(self, state):
        super().load_state(state)
        self._seen = int(state["seen"])
        for key, largest in (("highest", True), ("lowest", False)):
            kept, had = state[key], self._top[largest]
            if kept is not None:
                dev = had[0].device if had is not None else kept["score"].device
                kept = (kept["score"].to(dev), kept["index"].to(dev),
                        kept["images"].to(dev) if kept["images"] is not None else None)
            self._top[largest] = kept

    def highest(self):
        """(scores, ordinals within the pass, images or None), the highest score first."""
        return self._top[True]

    def lowest(self):
        """(scores, ordinals within the pass, images or None), the lowest score first."""
        return self._top[False]

    def report(self):
        out = {"samples": self._seen}
        for key, kept in (("highest", self.highest()), ("lowest", self.lowest())):
            if kept is not None:
                out[key] = {"score": kept[0].tolist(), "ordinal": kept[1].tolist()}
        return _jsonable(out)

    def end_test(self, epoch):
        Noop.end_test(self, epoch)
        if self.verbose and self._seen:
            print(f"[{self.name}] max {float(self.highest()[0][0]):.2e}, min {float(self.lowest()[0][0]):.2e} "
                  f"over {self._seen} samples")


class TopDifference(_Ranking):
    """reference :421-427: ranks samples by the top-1 minus top-2 softmax probability of the backbone."""

    name = "TopDifference"


class Entropy(_Ranking):
    """reference :324-361: ranks samples by the entropy of the backbone's softmax and keeps its statistics.

    ``avg`` is the mean entropy of the pass.  ``std`` has the reference's meaning: the running sum of squared
    deviations from the mean, NOT divided by the count (the reference updates it Welford-style per sample, :351-355);
    it is computed here from the sum and the sum of squares, both accumulated in fp64 on the device."""

    name = "Entropy"

    def _reset(self):
        super()._reset()
        self._sums = None

    def _observe(self, scores):
        h = scores[:, 0].to(SUMS_DTYPE)
        s = torch.stack((h.sum(), (h * h).sum()))
        self._sums = s if self._sums is None else self._sums + s

    def state(self, counts=True):
        return {**super().state(counts), "sums": None if self._sums is None else self._sums.cpu()}

    def merge(self, states):
        return {**super().merge(states), "sums": merge_sum([s["sums"] for s in states])}      # summed in rank order

    def load_state(self, state):
        dev = self._sums.device if self._sums is not None else "cpu"
        super().load_state(state)
        self._sums = None if state["sums"] is None else state["sums"].to(dev)

    @property
    def avg(self):
        return float(self._sums[0]) / self._seen if self._seen else 0.0

    @property
    def std(self):
        if not self._seen:
            return 0.0
        s, q = (float(v) for v in self._sums)
        return max(q - s * s / self._seen, 0.0)

    def report(self):
        return {**super().report(), "avg": self.avg, "std": self.std}

    def end_test(self, epoch):
        Noop.end_test(self, epoch)
        if self.verbose and self._seen:
            print(f"[{self.name}] avg {self.avg:.2e}, std {self.std:.2e}, max {float(self.highest()[0][0]):.2e}, "
                  f"min {float(self.lowest()[0][0]):.2e}")


class NBDTEntropyMaxMin(Entropy):
    """reference :364-389: ranks samples by the largest minus the smallest node entropy along the hard rules' path
    (the path's opening root entry, at entropy 0, included); ``avg`` / ``std`` stay the backbone's, as there."""

    accepts_tree = lambda tree, **kwargs: tree                                        # noqa: E731
    accepts_dataset = lambda trainset, **kwargs: trainset.__class__.__name__          # noqa: E731
    accepts_path_graph = True
    accepts_path_wnids = True
    name = "NBDTEntropyMaxMin"

    def __init__(self, classes=(), tree=None, dataset=None, path_graph=None, path_wnids=None, hierarchy=None,
                 save_k=20):
        tree = tree or Tree(dataset, path_graph=path_graph, path_wnids=path_wnids, hierarchy=hierarchy,
                            classes=list(classes) or None)
        super().__init__(tree.classes, tree=tree, save_k=save_k)


class Chain(Noop):
    """Fans every hook out to its members, in order: lets a driver run diagnostics beside its ``--analysis`` analyzer.
    What the chain itself does not define (``accuracy``, ``best_accuracy``, ...) is the first member's."""

    def __init__(self, *analyzers):
        if not analyzers:
            raise ValueError("Chain needs at least one analyzer")
        self.analyzers = tuple(analyzers)
        super().__init__(analyzers[0].classes)

    def __getattr__(self, item):
        if item == "analyzers":
            raise AttributeError(item)
        return getattr(self.analyzers[0], item)

    @property
    def name(self):
        return self.analyzers[0].name

    @property
    def verbose(self):
        return self.analyzers[0].verbose

    @verbose.setter
    def verbose(self, value):
        for a in self.analyzers:
            a.verbose = value

    def _fan(self, hook, *args):
        """Every member gets the hook, even when an earlier one raises; the first error is raised afterwards."""
        error = None
        for a in self.analyzers:
            try:
                getattr(a, hook)(*args)
            except Exception as e:        # noqa: BLE001
                error = error or e
        if error is not None:
            raise error

    def start_epoch(self, epoch):
        self._fan("start_epoch", epoch)

    def end_epoch(self, epoch):
        self._fan("end_epoch", epoch)

    def start_train(self, epoch):
        self._fan("start_train", epoch)

    def end_train(self, epoch):
        self._fan("end_train", epoch)

    def start_test(self, epoch):
        self._fan("start_test", epoch)

    def end_test(self, epoch):
        self._fan("end_test", epoch)

    def set_sample_offset(self, offset):
        self._fan("set_sample_offset", offset)

    # distributed evaluation: the members' states, with a block of counters that fused members share sent (and summed,
    # and read back from the device) once rather than once per member
    def _sharing(self):
        """(field -> tensor of the block the fused members share, the members that are entirely in it)."""
        block, inside = {}, []
        for a in self.analyzers:
            own = a._block if isinstance(a, _Fused) and a._host is None else None
            if own and all(block.get(f, t) is t for f, t in own.items()):
                block.update(own)
                inside.append(a)
        return block, inside

    def state(self):
        block, inside = self._sharing()
        return {"shared": {f: t.cpu().numpy() for f, t in block.items()},
                "members": [a.state(counts=False) if a in inside else a.state() for a in self.analyzers]}

    def merge(self, states):
        return {"shared": merge_sum([s["shared"] for s in states]) or {},
                "members": [a.merge([s["members"][i] for s in states]) for i, a in enumerate(self.analyzers)]}

    def load_state(self, state):
        for a, member in zip(self.analyzers, state["members"]):
            a.load_state(member)
            if isinstance(a, _Fused) and a.fields and not member.get("counts") \
                    and all(f in state["shared"] for f in a.fields):       # its counters travelled in the shared block
                a.load_counts({f: state["shared"][f] for f in a.fields})

    def update_batch(self, outputs, targets, images=None):
        """Returns the first member's statistic (what the driver's own analyzer would have returned).  The members of
        this module share their launch (see ``_launch``): one per batch when they are on one hierarchy."""
        fused = [a for a in self.analyzers if isinstance(a, _Fused) and type(a).update_batch is _Fused.update_batch]
        results = [a.update_batch(outputs, targets, images) if a not in fused else None for a in self.analyzers]
        if fused:
            _launch(fused, outputs, targets, images)
        return results[0]
