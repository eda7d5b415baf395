"""Induced hierarchies: agglomerative clustering of the classifier's weight rows -> graph JSON.

Restates the induced-hierarchy part of the reference's ``nbdt/graph.py``:
``MODEL_FC_KEYS`` / ``get_centers_from_*`` (:386-399, :466-511), ``build_induced_graph`` (:402-464),
``generate_graph_fname`` / ``get_graph_path_from_args`` (:194-281) and ``write_graph``
(nbdt/thirdparty/nx.py:63-66, networkx node-link JSON).  The clustering (ward linkage on a [C, F] matrix) runs
where ``linkage_children``'s backend says: sklearn on the host, as the reference does it, or csrc/linkage.hip on the
GPU (fp64 pairwise distances + the nearest-neighbour chain; only the labelling of the n - 1 merges is host work).
Either way it produces the on-disk format ``nbdt.tree.Tree`` and the HIP kernels consume, so new backbones / class
sets are not limited to the shipped JSON files.

Differences from the reference, both forced by the target image:
* scikit-learn >= 1.4 renamed ``AgglomerativeClustering(affinity=)`` to ``metric=``; the reference's call
  (:437-439) raises ``TypeError`` there.  Same algorithm, new keyword.
* WordNet (nltk) is not installed, so inner nodes get the reference's own fallback identity -- a
  ``FakeSynset`` id ``f<number of nodes so far, 8 digits>`` with label ``(generated)``
  (nbdt/graph.py:610-615, nbdt/thirdparty/wn.py:74-94) -- instead of a common WordNet hypernym.  Node
  names are cosmetic; the tree structure and child order (what the rules layer computes with) are equal.
"""
import json
import os
from pathlib import Path

import numpy as np
import torch

from nbdt.utils import fwd

MODEL_FC_KEYS = (
    "fc.weight", "linear.weight", "module.linear.weight", "module.net.linear.weight", "output.weight",
    "module.output.weight", "output.fc.weight", "module.output.fc.weight", "classifier.weight",
    "model.last_layer.3.weight",
)


class Graph:
    """Minimal ordered digraph with the two things the file format needs: node and edge insertion order."""

    def __init__(self):
        self.nodes = {}      # id -> {"label": ...}
        self.edges = []      # (source, target)

    def add_node(self, wnid, **attrs):
        self.nodes.setdefault(wnid, {}).update(attrs)

    def add_edge(self, source, target):
        self.add_node(source)
        self.add_node(target)
        self.edges.append((source, target))

    def succ(self, wnid):
        return [t for s, t in self.edges if s == wnid]

    def roots(self):
        targets = {t for _, t in self.edges}
        return [n for n in self.nodes if n not in targets]

    def node_link_data(self):
        nodes = [dict(attrs, id=wnid) for wnid, attrs in self.nodes.items()]
        links = [{"source": s, "target": t} for s, t in self.edges]
        return {"directed": True, "multigraph": False, "graph": {}, "nodes": nodes, "links": links}


def write_graph(G, path):
    path = str(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"          # readers never see a partial file
    with open(tmp, "w") as f:
        json.dump(G.node_link_data(), f)
    os.replace(tmp, path)


def get_centers_from_state_dict(state_dict):
    for key in MODEL_FC_KEYS:
        if key in state_dict:
            return state_dict[key].squeeze().detach()
    return None


def get_centers_from_checkpoint(checkpoint):
    data = torch.load(checkpoint, map_location=torch.device("cpu"))
    state_dict = data
    for key in ("net", "state_dict"):
        if isinstance(data, dict) and key in data:
            state_dict = data[key]
            break
    fc = get_centers_from_state_dict(state_dict)
    assert fc is not None, f"Could not find FC weights in checkpoint {checkpoint} with keys: {list(state_dict)[:8]}"
    return fc


LINKAGES = ("ward", "complete", "single", "average")
AFFINITIES = ("euclidean", "l2", "manhattan", "l1", "cityblock", "cosine")
BACKENDS = (None, "sklearn", "device")


def _linkage_sklearn(centers, linkage, affinity):
    """The reference's call (nbdt/graph.py:437-439).  n_clusters only cuts the finished tree into flat labels, which
    nothing here reads: children_ is the whole tree whatever its value; compute_distances adds the heights."""
    from sklearn.cluster import AgglomerativeClustering

    centers = centers.detach().float().cpu().numpy()
    clustering = AgglomerativeClustering(linkage=linkage, n_clusters=2, metric=affinity,
                                         compute_distances=True).fit(centers)
    return np.asarray(clustering.children_, dtype=np.int64), np.asarray(clustering.distances_, dtype=np.float64)


def label_merges(merges, heights, n):
    """Raw chain merges -> scipy's / sklearn's ``children_``: stable sort by height, then a union-find in which merge
    ``i`` creates cluster ``n + i``; each row is (min, max) of the two roots.  Child order is decision order in the
    written graph."""
    order = np.argsort(heights, kind="stable")
    parent = np.arange(2 * n - 1)

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    children = np.empty((n - 1, 2), dtype=np.int64)
    for i, (a, b) in enumerate(merges[order].tolist()):
        ra, rb = find(a), find(b)
        children[i] = (min(ra, rb), max(ra, rb))
        parent[ra] = parent[rb] = n + i
    return children, heights[order]


def linkage_workspace_bytes(n):
    """Bytes of device memory nbdt_linkage needs for `n` rows (the fp64 distance matrix and two index arrays)."""
    import ctypes
    from nbdt import _C
    nbytes = ctypes.c_int64()
    _C.check(_C.lib().nbdt_linkage_workspace_bytes(int(n), ctypes.byref(nbytes)))
    return nbytes.value


def _linkage_device(centers, linkage, affinity):
    """csrc/linkage.hip: pairwise distances and the nearest-neighbour chain on the device, labelling on the host."""
    from nbdt import _C

    if not torch.cuda.is_available():
        raise _C.NBDTHipError('linkage_children(backend="device") needs a HIP device (no CPU fallback)')
    x = centers.detach()
    if not x.is_cuda:
        x = x.cuda()
    x = x.float().contiguous()
    n, d = x.shape
    if not bool(torch.isfinite(x).all()):
        raise ValueError("the classifier matrix holds non-finite values")
    if _C.NBDT_METRIC[affinity] == _C.NBDT_METRIC["cosine"] and bool((x == 0).all(dim=1).any()):
        raise ValueError("Cosine affinity cannot be used when X contains zero vectors")      # sklearn's refusal
    nbytes = linkage_workspace_bytes(n)
    refusal = (f"inducing a hierarchy over n = {n} classes on the device needs a workspace of {nbytes} bytes "
               f"(the fp64 [n, n] distance matrix), more than {x.device} can allocate")
    with torch.cuda.device(x.device):
        free, _ = torch.cuda.mem_get_info()
        cached = torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        if nbytes > free + cached:
            raise RuntimeError(f"{refusal}: {free + cached} bytes are free")
        try:
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        except torch.cuda.OutOfMemoryError as e:
            raise RuntimeError(refusal) from e
        merges = torch.empty((n - 1, 2), dtype=torch.int32, device=x.device)
        heights = torch.empty(n - 1, dtype=torch.float64, device=x.device)
        sizes = torch.empty(n - 1, dtype=torch.int32, device=x.device)
        _C.check(_C.lib().nbdt_linkage(_C.ptr(x), n, d, _C.NBDT_LINKAGE[linkage], _C.NBDT_METRIC[affinity],
                                       _C.ptr(workspace), nbytes, _C.ptr(merges), _C.ptr(heights), _C.ptr(sizes),
                                       _C.stream_of(x)))
        merges, heights, sizes = merges.cpu().numpy(), heights.cpu().numpy(), sizes.cpu().numpy()     # the one read-back
    if sizes.min() < 2 or not np.isfinite(heights).all():
        raise RuntimeError("nbdt_linkage did not finish: the distances are not finite")
    return label_merges(merges.astype(np.int64), heights, n)


def linkage_children(centers, linkage="ward", affinity="euclidean", backend=None):
    """Agglomerative clustering of the rows of `centers` ([n, d] tensor, CPU or GPU) -> (children [n-1, 2] int64,
    heights [n-1] float64) in scipy's / sklearn's ``children_`` convention.

    backend "sklearn": sklearn.cluster.AgglomerativeClustering on the host (what build_induced_graph always did).
    backend "device":  csrc/linkage.hip; a GPU tensor stays where it is, the workspace comes from torch.
    backend None:      sklearn when it imports, the device when it does not and a GPU is present."""
    if backend not in BACKENDS:
        raise ValueError(f"unknown backend {backend!r} (one of {BACKENDS})")
    if linkage not in LINKAGES:
        raise ValueError(f"unknown linkage {linkage!r} (one of {LINKAGES})")
    if affinity not in AFFINITIES:
        raise ValueError(f"unknown affinity {affinity!r} (one of {AFFINITIES})")
    if linkage == "ward" and affinity not in ("euclidean", "l2"):
        raise ValueError(f"ward can only work with euclidean distances, got {affinity!r}")
    centers = torch.as_tensor(centers)
    if centers.dim() != 2 or centers.size(0) < 2 or centers.size(1) < 1:
        raise ValueError(f"need a [n, d] matrix with n >= 2 and d >= 1, got shape {tuple(centers.shape)}")
    if backend is None:
        try:
            import sklearn.cluster  # noqa: F401
            backend = "sklearn"
        except ImportError:
            if not torch.cuda.is_available():
                raise
            backend = "device"
    if backend == "sklearn":
        return _linkage_sklearn(centers, linkage, affinity)
    return _linkage_device(centers, linkage, affinity)


def build_induced_graph(wnids, checkpoint=None, model=None, linkage="ward", affinity="euclidean",
                        branching_factor=2, dataset="CIFAR10", state_dict=None, backend=None):
    """reference nbdt/graph.py:402-464.  `model`: an nn.Module (its state_dict is used); the reference's
    form "architecture name -> download the pretrained model" needs network access and raises here.
    `backend`: where the clustering runs (linkage_children)."""
    num_classes = len(wnids)
    assert checkpoint or model is not None or state_dict, \
        "Need to specify either `checkpoint` or `method` or `state_dict`."
    if state_dict:
        centers = get_centers_from_state_dict(state_dict)
    elif checkpoint:
        centers = get_centers_from_checkpoint(checkpoint)
    else:
        if isinstance(model, str):
            raise NotImplementedError(
                f"inducing from the pretrained `{model}` downloads a checkpoint; pass `checkpoint=` or a module")
        centers = get_centers_from_state_dict(model.state_dict())
    assert centers is not None, "Could not find FC weights (looked for: %s)" % ", ".join(MODEL_FC_KEYS)
    assert num_classes == centers.size(0), (
        f"The model FC supports {centers.size(0)} classes. However, the dataset {dataset} features "
        f"{num_classes} classes. Try passing the `--dataset` with the right number of classes.")
    if centers.dim() != 2:
        centers = centers.reshape(centers.size(0), -1)
    children, _ = linkage_children(centers, linkage=linkage, affinity=affinity, backend=backend)

    G = Graph()
    for wnid in wnids:                       # leaves first, in class order
        G.add_node(wnid)
    index_to_wnid = {}
    for index, pair in enumerate(map(tuple, children.tolist())):
        child_wnids = [wnids[c] if c < num_classes else index_to_wnid[c - num_classes] for c in pair]
        parent_wnid = "f{:08d}".format(len(G.nodes))     # FakeSynset.create_from_offset(len(G.nodes))
        G.add_node(parent_wnid, label="(generated)")
        index_to_wnid[index] = parent_wnid
        for child_wnid in child_wnids:
            G.add_edge(parent_wnid, child_wnid)
    assert len(G.roots()) == 1, G.roots()
    return G


def _checkpoint_tag(checkpoint):
    """`ckpt-<dataset>-<rest>[-induced]` -> `<rest>`; any other file name -> its stem."""
    stem = Path(checkpoint).stem
    parts = stem.split("-")
    if parts[0] == "ckpt" and len(parts) >= 3:
        return "-".join(parts[2:]).replace("-induced", "")
    return stem


def generate_graph_fname(method, seed=0, branching_factor=2, extra=0, no_prune=False, fname="", path="",
                         multi_path=False, induced_linkage="ward", induced_affinity="euclidean", checkpoint=None,
                         arch=None, **kwargs):
    """File stem of a hierarchy JSON.  The naming scheme is an on-disk contract with the reference
    (nbdt/graph.py:194-245): `graph-<method>` followed by one `-<tag><value>` suffix per non-default option,
    in a fixed order, so hierarchies written by either implementation are found by the other."""
    if path:
        return Path(path).stem
    if fname:
        return fname
    induced = method == "induced"
    if induced:
        assert checkpoint or arch, "Induced hierarchy needs either `arch` or `checkpoint`"
    suffixes = [
        (method == "random" and seed != 0, f"seed{seed}"),
        (induced and induced_linkage not in ("ward", None), f"linkage{induced_linkage}"),
        (induced and induced_affinity not in ("euclidean", None), f"affinity{induced_affinity}"),
        (induced, _checkpoint_tag(checkpoint) if checkpoint else arch),
        (method in ("random", "induced") and branching_factor != 2, f"branch{branching_factor}"),
        (extra > 0, f"extra{extra}"),
        (bool(no_prune), "noprune"),
        (bool(multi_path), "multi"),
    ]
    return "-".join([f"graph-{method}"] + [str(tag) for on, tag in suffixes if on])


def get_directory(dataset, root=None):
    return os.path.join(root or fwd(), "hierarchies", dataset)


def get_graph_path_from_args(dataset, method, path="", **kwargs):
    """reference nbdt/graph.py:248-281."""
    if path:
        return path
    return os.path.join(get_directory(dataset), generate_graph_fname(method=method, **kwargs) + ".json")
