"""Zero-shot evaluation on superclasses: does a classifier trained on one label set put the images of ANOTHER label set
on the right side of a coarse split ("Animal vs. Vehicle")?

``Superclass`` and ``SuperclassNBDT`` of the reference's ``nbdt/analysis.py`` (:430-559).  Every class of the training
label set and of the test label set is mapped to the first listed superclass among its WordNet hypernyms, or to -1.
``Superclass`` masks the unmapped training classes with -100, takes the backbone's argmax and looks up its superclass;
``SuperclassNBDT`` averages the logits of each superclass's training classes (``get_node_logits`` over an ad-hoc
grouping) and takes the argmax of those means.  A test sample whose own class maps nowhere is not counted.

Both speak the whole protocol of ``nbdt.analysis.DecisionRules``.  What is behind it is one launch per evaluation batch,
``nbdt_superclass_accumulate`` (csrc/superclass.hip), which adds into int64 counters on the device: the reference's
``outputs[targets >= 0]`` compaction, its ``-100`` write into a copy of the logits and its ``.item()`` per batch would
each make the host wait.  ``update_batch`` only enqueues work; the first host transfer is in ``end_test`` or an accessor.

The hypernyms of a class come from, in this order: an explicit table (a dict or a JSON file ``{class wnid: [hypernym
wnids]}``), nltk's WordNet when it is installed with its corpus, or the shipped ``hierarchies/<dataset>/graph-wordnet.json``
(``graph_hypernyms``).  The last one is LOSSY and warns: the graph keeps one parent per contracted chain, so a class that
reaches a superclass only through a second WordNet parent loses it (CIFAR10's automobile and truck reach "vehicle" that
way and map to -1).
"""
import json
import os
import warnings
from collections import defaultdict

import numpy as np
import torch

from nbdt import _C
from nbdt.analysis import DecisionRules, Noop, merge_sum
from nbdt.model import SoftEmbeddedDecisionRules as _SoftRules
from nbdt.tree import get_wnids
from nbdt.utils import dataset_to_default_path_wnids, hierarchy_to_path_graph

__all__ = names = ("Superclass", "SuperclassNBDT")


def add_arguments(parser):
    parser.add_argument("--superclass-wnids", nargs="*", default=[],
                        help="--analysis Superclass | SuperclassNBDT: the superclasses, as WordNet ids (e.g. n00015388 "
                             "n04524313: animal, vehicle); the first one listed among a class's hypernyms wins")
    parser.add_argument("--superclass-file", metavar="JSON",
                        help="{class wnid: [hypernym wnids]} for every class of --dataset and --dataset-test: the hypernym "
                             "table the superclass mapping is built from, instead of nltk's WordNet or the shipped graph")


# ------------------------------------------------------------------------------------------------------------
# hypernym sources

def load_hypernyms(hypernyms):
    """A dict {class wnid: [hypernym wnids]} as given, or read from the JSON file whose path was given."""
    if isinstance(hypernyms, (str, os.PathLike)):
        with open(hypernyms) as f:
            hypernyms = json.load(f)
    if not isinstance(hypernyms, dict):
        raise TypeError(f"hypernyms must be a dict {{class wnid: [hypernym wnids]}} or a path to a JSON file of one, got "
                        f"{type(hypernyms).__name__}")
    return hypernyms


def wordnet_hypernyms(wnids):
    """{wnid: hypernym wnids, the class itself first} from nltk's WordNet (the reference's all_hypernyms: breadth first
    over every parent), or None when nltk or its corpus is not installed."""
    try:
        from nltk.corpus import wordnet as wn
        wn.ensure_loaded()
    except Exception:      # ImportError without nltk, LookupError without the corpus
        return None
    table = {}
    for wnid in wnids:
        frontier, found = [wn.synset_from_pos_and_offset(wnid[0], int(wnid[1:]))], []
        while frontier:
            current = frontier.pop(0)
            found.append(f"{current.pos()}{current.offset():08d}")
            frontier.extend(current.hypernyms())
        table[wnid] = found
    return table


def graph_hypernyms(wnids, path_graph):
    """{wnid: hypernym wnids} read off a shipped WordNet hierarchy file: the ancestors-or-self of the leaf in the graph,
    plus the keys of every such node's ``contraction`` attribute (the single-child chains the graph's builder folded into
    the node).  LOSSY: only the parents the graph kept are followed."""
    with open(path_graph) as f:
        g = json.load(f)
    contracted = {n["id"]: list(n.get("contraction", {})) for n in g["nodes"]}
    parents = defaultdict(list)
    for e in g.get("links", g.get("edges", [])):
        parents[e["target"]].append(e["source"])
    table = {}
    for wnid in wnids:
        if wnid not in contracted:
            raise KeyError(f"{wnid} is not a node of {path_graph}")
        frontier, found, seen = [wnid], [], set()
        while frontier:
            current = frontier.pop(0)
            if current in seen:
                continue
            seen.add(current)
            found.append(current)
            found.extend(contracted.get(current, ()))
            frontier.extend(parents[current])
        table[wnid] = found
    return table


def dataset_of_wnids(dataset_wnids):
    """The shipped dataset whose wnid list this is, or None."""
    from nbdt.utils import DATASETS
    for dataset in DATASETS:
        path = dataset_to_default_path_wnids(dataset)
        if os.path.exists(path) and get_wnids(path) == list(dataset_wnids):
            return dataset
    return None


# ------------------------------------------------------------------------------------------------------------
# the analyzers

class Superclass(DecisionRules):
    """Accuracy of the backbone's own prediction on the superclass problem (reference nbdt/analysis.py:430-535).

    superclass_wnids: the G superclasses; dataset_test: the dataset whose labels the evaluation batches carry (None: the
    training dataset); hypernyms: an explicit hypernym table, see ``build_mapping``; metric: accepted and ignored, as in the
    reference.  ``accuracy()`` / ``correct`` / ``total`` count the samples whose own class maps to a superclass;
    ``confusion()`` is [G, G], entry [target superclass, predicted superclass] (a prediction of -1 -- every mapped logit
    below -100 -- is in ``total`` and in no cell)."""

    accepts_dataset = lambda trainset, **kwargs: trainset.__class__.__name__               # noqa: E731
    accepts_dataset_test = lambda testset, **kwargs: testset.__class__.__name__            # noqa: E731
    accepts_superclass_wnids = True
    name = "Superclass"
    mode = _C.NBDT_SUPER_MASKED

    def __init__(self, *args, superclass_wnids, dataset_test=None, Rules=_SoftRules, metric=None, hypernyms=None,
                 sync_every_batch=False, **kwargs):
        super().__init__(*args, Rules=_SoftRules, metric="top1", sync_every_batch=sync_every_batch, **kwargs)
        self.superclass_wnids = list(superclass_wnids)
        if not self.superclass_wnids:
            raise ValueError(f"{type(self).__name__} needs at least one superclass wnid")
        self.num_superclasses = len(self.superclass_wnids)
        wnids_train = self.rules.tree.wnids_leaves
        if dataset_test is None or dataset_test == self.rules.tree.dataset:
            self.dataset_test, self.wnids_test = self.rules.tree.dataset, list(wnids_train)
        else:        # the reference builds a second rules object only to read its tree's wnids_leaves
            self.dataset_test, self.wnids_test = dataset_test, get_wnids(dataset_to_default_path_wnids(dataset_test))
        self.mapping_target, self.new_to_old_classes_target = self.build_mapping(
            self.wnids_test, self.superclass_wnids, hypernyms)
        self.mapping_pred, self.new_to_old_classes_pred = self.build_mapping(
            wnids_train, self.superclass_wnids, hypernyms)
        self.groups = [list(self.new_to_old_classes_pred[g]) if g in self.new_to_old_classes_pred else []
                       for g in range(self.num_superclasses)]
        self.mapped_classes = [i for i, v in enumerate(self.mapping_target.tolist()) if v >= 0]
        self._device = None
        self._totals = self._confusion = self._map_target = self._map_pred = self._handle = None

    # ---- the mapping (host; no device needed)
    @staticmethod
    def build_mapping(dataset_wnids, superclass_wnids, hypernyms=None):
        """(mapping, new_to_old_classes): mapping[i] is the index of the first listed superclass among the hypernyms of class
        i -- the class itself counts as one of them -- or -1 (an int64 tensor); new_to_old_classes[v] lists the classes with
        mapping v in ascending order, key -1 included (a defaultdict, as in the reference :482-498).

        The hypernym sets come from ``hypernyms`` (a dict {class wnid: [hypernym wnids]} or the path of a JSON file holding
        one; every class must have an entry), else from nltk's WordNet when it and its corpus are installed, else from the
        shipped ``graph-wordnet.json`` of the dataset these wnids belong to -- lossy, with a UserWarning."""
        dataset_wnids = list(dataset_wnids)
        if hypernyms is not None:
            table = load_hypernyms(hypernyms)
            missing = [w for w in dataset_wnids if w not in table]
            if missing:
                raise KeyError(f"the hypernym table has no entry for {len(missing)} classes, e.g. {missing[:3]}")
        else:
            table = wordnet_hypernyms(dataset_wnids)
        if table is None:
            dataset = dataset_of_wnids(dataset_wnids)
            path = hierarchy_to_path_graph(dataset, "wordnet") if dataset else None
            if not path or not os.path.exists(path):
                raise RuntimeError("no hypernym source for this label set: nltk's WordNet is not installed and no shipped "
                                   "graph-wordnet.json belongs to these wnids; pass hypernyms= (a table or a JSON file)")
            warnings.warn(f"superclass mapping from {os.path.relpath(path, os.path.dirname(__file__))}: nltk's WordNet is "
                          "not installed, and this fallback is LOSSY -- the graph keeps one parent per contracted chain, so "
                          "a class that reaches a superclass only through another WordNet parent maps to -1.  Pass "
                          "hypernyms= (a table or a JSON file) for an exact mapping.", UserWarning, stacklevel=2)
            table = graph_hypernyms(dataset_wnids, path)
        new_to_old_classes = defaultdict(list)
        mapping = []
        for old_index, wnid in enumerate(dataset_wnids):
            own = set(table[wnid]) | {wnid}
            value = next((new for new, sup in enumerate(superclass_wnids) if sup in own), -1)
            mapping.append(value)
            new_to_old_classes[value].append(old_index)
        return torch.tensor(mapping, dtype=torch.int64), new_to_old_classes

    # ---- device side
    def to(self, device):
        """Put the two mappings, the grouping handle and zeroed counters on `device` now (four small host-to-device copies)
        instead of in the first update_batch there, so that not even the first batch waits for the host."""
        self._on(torch.device(device))
        return self

    def _on(self, device):
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if self._device != device:
            G = self.num_superclasses
            self._device = device
            self._map_target = self.mapping_target.to(device=device, dtype=torch.int32)
            self._map_pred = self.mapping_pred.to(device=device, dtype=torch.int32)
            self._handle = _C.groups_handle(self.groups, len(self.mapping_pred), device.index)
            self._totals = torch.zeros(2, dtype=torch.int64, device=device)
            self._confusion = torch.zeros(G * G, dtype=torch.int64, device=device)

    def forward(self, outputs, targets):
        """(predicted superclass [B] int64, target superclass [B] int64) on the device, -1 where unmapped; counts nothing
        (its counters go to a scratch block).  The reference compacts both to the mapped samples; select with
        ``targets >= 0`` where that is wanted."""
        _C.require_gpu(outputs, self.name)
        device = outputs.device
        self._on(device)
        y = targets.to(device=device, dtype=torch.int64).contiguous()
        scratch = torch.zeros(2, dtype=torch.int64, device=device)
        pred = _C.superclass_accumulate(self._handle, outputs, y, self._map_target, self._map_pred, self.mode, scratch,
                                        None, want_pred=True)
        valid = (y >= 0) & (y < self._map_target.numel())
        mapped = torch.where(valid, self._map_target[y.clamp(0, self._map_target.numel() - 1)].long(),
                             torch.full_like(y, -1))
        return pred, mapped

    def _update_batch(self, outputs, targets):
        _C.require_gpu(outputs, self.name)
        self._on(outputs.device)
        y = targets.to(device=outputs.device, dtype=torch.int64).contiguous()
        with torch.no_grad():
            _C.superclass_accumulate(self._handle, outputs, y, self._map_target, self._map_pred, self.mode, self._totals,
                                     self._confusion)
        return f"{self.name}: {round(self.accuracy(), 2)}%" if self.sync_every_batch else None

    def start_test(self, epoch):
        super().start_test(epoch)
        if self._totals is not None:
            self._totals.zero_()
            self._confusion.zero_()

    # ---- accessors (host transfer)
    def _host_totals(self):
        return [0, 0] if self._totals is None else [int(v) for v in self._totals.tolist()]

    @property
    def total(self):
        return self._host_totals()[0]

    @property
    def correct(self):
        return self._host_totals()[1]

    def accuracy(self):
        """Percent of the counted samples (own class mapped) whose predicted superclass is their class's."""
        total, correct = self._host_totals()
        return 100.0 * correct / max(total, 1)

    def confusion(self):
        """[G, G] int64 numpy array: entry [target superclass, predicted superclass]."""
        G = self.num_superclasses
        if self._confusion is None:
            return np.zeros((G, G), dtype=np.int64)
        return self._confusion.cpu().numpy().reshape(G, G).copy()

    # ---- distributed evaluation
    def state(self):
        return {"totals": np.asarray(self._host_totals(), dtype=np.int64), "confusion": self.confusion()}

    def merge(self, states):
        G = self.num_superclasses
        return merge_sum(states) or {"totals": np.zeros(2, dtype=np.int64), "confusion": np.zeros((G, G), dtype=np.int64)}

    def load_state(self, state):
        device = self._device if self._device is not None else torch.device("cpu")
        self._totals = torch.as_tensor(np.asarray(state["totals"], dtype=np.int64).reshape(2)).to(device)
        self._confusion = torch.as_tensor(np.asarray(state["confusion"], dtype=np.int64).reshape(-1)).to(device)

    def end_test(self, epoch):
        Noop.end_test(self, epoch)
        acc = round(self.accuracy(), 2)
        self.best_accuracy = max(self.best_accuracy, acc)
        if self.verbose:
            total, correct = self._host_totals()
            print(f"[{self.name}] Accuracy: {acc}% ({correct} of {total} samples of {len(self.mapped_classes)} mapped "
                  f"{self.dataset_test} classes); best so far {self.best_accuracy}%")


class SuperclassNBDT(Superclass):
    """Accuracy of the mean logit per superclass -- a one-node decision tree over the training classes -- on the
    superclass problem (reference nbdt/analysis.py:538-559)."""

    name = "Superclass-NBDT"
    mode = _C.NBDT_SUPER_GROUP_MEAN

    def __init__(self, *args, Rules=None, **kwargs):
        super().__init__(*args, Rules=_SoftRules, **kwargs)
        empty = [w for w, g in zip(self.superclass_wnids, self.groups) if not g]
        if empty:
            raise ValueError(f"no class of {self.rules.tree.dataset} lies under superclass {empty[0]}"
                             + (f" (nor under {', '.join(empty[1:])})" if empty[1:] else "")
                             + ": its mean logit would be NaN and win every argmax")
