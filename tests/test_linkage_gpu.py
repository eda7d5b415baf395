"""csrc/linkage.hip on the MI355X: nbdt.graph.linkage_children(backend="device") against the numpy oracle
(tests/_linkage_ref.py, pinned to scipy by tests/test_linkage.py), against a scipy recording for the case too long for
the oracle, against the reference's recorded hierarchies, and through generate_hierarchy / Tree.update_from_model /
SoftTreeLoss.set_epoch.

Exact comparisons (children equal, heights to HEIGHT_RTOL) are made only on inputs whose oracle heights have a smallest
relative gap of at least MIN_GAP between consecutive merges: a condition on the inputs, asserted before comparing.
HEIGHT_RTOL is 100 times MEASURED_DEVIATION, the largest relative deviation between device and oracle heights over all
exact cases as measured on an MI355X; it has to stay at or below 1e-10, two orders under MIN_GAP.
Inputs with ties are compared as dendrograms (valid, heights as a multiset, run-to-run identical bits), not by children.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from nbdt import _C
from nbdt import graph as G
from nbdt.hierarchy import generate_hierarchy
from nbdt.tree import Tree, get_wnids
from nbdt.utils import dataset_to_default_path_wnids

import _linkage_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_GAP = 1e-8
MEASURED_DEVIATION = 7.556e-16   # at 3000 x 16 against scipy; every case against the numpy oracle: 0
HEIGHT_RTOL = 100 * MEASURED_DEVIATION
assert MEASURED_DEVIATION <= 1e-10

WARD_SHAPES = [(2, 5), (3, 5), (5, 5),                  # a single merge; the chain empties and restarts
               (63, 9), (64, 9), (65, 9),               # one wave, +-1
               (1023, 8), (1025, 8),                    # one block's lanes +-1: the strided loops' second trip
               (40, 1), (40, 3), (40, 70), (40, 2048)]  # distance-tile remainders; the longest accumulation
OTHER_LINKAGES = [(n, d, m, "euclidean") for (n, d) in ((65, 7), (300, 33)) for m in ("complete", "single", "average")]
OTHER_METRICS = [(300, 33, m, a) for m in ("complete", "single", "average") for a in ("manhattan", "cosine")]
FIXTURES = [("cifar10", "CIFAR10"), ("cifar100", "CIFAR100"), ("tiny200", "TinyImagenet200")]


def random_centers(n, d, seed=1):
    return np.random.default_rng(1000 * n + d + seed).standard_normal((n, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle(n, d, method, metric):
    return R.linkage_ref(random_centers(n, d), method, metric)


def device_linkage(X, method="ward", metric="euclidean"):
    return G.linkage_children(torch.from_numpy(X).to(DEV), linkage=method, affinity=metric, backend="device")


def assert_heights(got, want, what):
    dev = float(np.max(np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)))
    print(f"linkage-deviation {what}: {dev:.3e}")
    assert dev <= HEIGHT_RTOL, (what, dev)


def assert_exact(X, method, metric, want_children, want_heights, what):
    assert R.smallest_relative_gap(want_heights) >= MIN_GAP, "the input does not qualify for an exact comparison"
    children, heights = device_linkage(X, method, metric)
    assert children.dtype == np.int64 and heights.dtype == np.float64
    assert children.shape == want_children.shape
    assert np.array_equal(children, want_children), what
    assert_heights(heights, want_heights, what)


@pytest.mark.parametrize("n,d", WARD_SHAPES)
def test_ward_equals_the_oracle(n, d):
    assert_exact(random_centers(n, d), "ward", "euclidean", *oracle(n, d, "ward", "euclidean"), f"ward {n}x{d}")


@pytest.mark.parametrize("n,d,method,metric", OTHER_LINKAGES + OTHER_METRICS)
def test_other_linkages_and_metrics_equal_the_oracle(n, d, method, metric):
    assert_exact(random_centers(n, d), method, metric, *oracle(n, d, method, metric), f"{method} {metric} {n}x{d}")


def test_a_matrix_far_beyond_any_cache_tile_equals_scipy(golden_dir):
    """3000 x 16: rows longer than two trips of the block, 72 MB of distances.  The recording is scipy's
    (tests/golden/make_linkage_golden.py)."""
    g = np.load(os.path.join(golden_dir, "linkage_3000x16.npz"))
    X = np.random.default_rng(int(g["seed"])).standard_normal((int(g["n"]), int(g["d"]))).astype(np.float32)
    assert_exact(X, "ward", "euclidean", g["children"].astype(np.int64), g["heights"], "ward 3000x16 (scipy)")


@pytest.mark.parametrize("tag,dataset", FIXTURES)
def test_induced_graph_equals_the_reference_on_the_device(tag, dataset, golden_dir):
    """tests/test_hierarchy.py::test_induced_graph_equals_the_reference with backend="device"."""
    g = np.load(os.path.join(golden_dir, f"induced_{tag}.npz"))
    wnids = get_wnids(dataset_to_default_path_wnids(dataset))
    W = torch.from_numpy(g["W"]).to(DEV)
    graph = G.build_induced_graph(wnids, state_dict={"linear.weight": W}, dataset=dataset, backend="device")
    data = graph.node_link_data()
    assert [n["id"] for n in data["nodes"]] == list(g["node_ids"])
    assert [n.get("label", "") for n in data["nodes"]] == list(g["node_labels"])
    assert [l["source"] for l in data["links"]] == list(g["link_source"])
    assert [l["target"] for l in data["links"]] == list(g["link_target"])
    want_children, want_heights = R.linkage_ref(g["W"])
    assert_exact(g["W"], "ward", "euclidean", want_children, want_heights, f"fixture {tag}")


def test_cpu_tensors_and_other_layouts_are_taken(golden_dir):
    """A CPU tensor is moved, a non-contiguous or fp64 one is made fp32 contiguous: same result as the plain call."""
    X = random_centers(65, 9)
    want = device_linkage(X)
    for x in (torch.from_numpy(X), torch.from_numpy(X).to(DEV).double(),
              torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).t()):
        children, heights = G.linkage_children(x, backend="device")
        assert np.array_equal(children, want[0]) and np.array_equal(heights, want[1])


class Net(nn.Module):
    def __init__(self, W):
        super().__init__()
        self.linear = nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            self.linear.weight.copy_(torch.from_numpy(W))


def test_generate_hierarchy_and_tree_update_from_a_gpu_module(tmp_path, golden_dir):
    W = np.load(os.path.join(golden_dir, "induced_cifar100.npz"))["W"]
    net = Net(W).to(DEV)
    path = generate_hierarchy("CIFAR100", "induced", arch="ResNet18", model=net, path=str(tmp_path / "graph-dev.json"),
                              induced_backend="device")
    host = generate_hierarchy("CIFAR100", "induced", arch="ResNet18", model=net, path=str(tmp_path / "graph-host.json"),
                              induced_backend="sklearn")
    with open(path) as f, open(host) as h:
        assert json.load(f) == json.load(h)                        # the tree the sklearn backend gives
    tree = Tree("CIFAR100", path_graph=path)
    assert len(tree.inodes) == 99 and all(len(n.children) == 2 for n in tree.inodes)
    # rules built on it run: the soft rules' class probabilities sum to one, the hard rules return classes
    z = torch.randn(16, 100, device=DEV)
    handle = tree.device_handle(0)
    P = _C.soft_forward(handle, z)
    assert torch.allclose(P.sum(1), torch.ones(16, device=DEV), atol=1e-5)
    pred = _C.hard_forward(handle, z, want_onehot=False)[0]
    assert pred.shape == (16,) and int(pred.min()) >= 0 and int(pred.max()) < 100
    # in place, from the same module
    old = Tree("CIFAR100", hierarchy="induced-ResNet18")
    shape = lambda t: [(n.wnid, [c.wnid for c in n.children]) for n in t.inodes]
    before = shape(old)
    old.update_from_model(net, "ResNet18", "CIFAR100", path_graph=str(tmp_path / "graph-epoch0.json"), backend="device")
    assert shape(old) == shape(tree) != before


def test_soft_tree_loss_reinduces_on_the_device(tmp_path, golden_dir):
    from nbdt.loss import SoftTreeLoss
    W = np.load(os.path.join(golden_dir, "induced_cifar10.npz"))["W"]
    net = Net(W).to(DEV)
    kwargs = dict(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18", net=net,
                  arch="ResNet18", tree_start_epochs=2, tree_update_every_epochs=2, tree_update_end_epochs=5)
    crit = SoftTreeLoss(checkpoint_path=str(tmp_path / "ckpt-dev.pth"), tree_update_backend="device", **kwargs)
    host = SoftTreeLoss(checkpoint_path=str(tmp_path / "ckpt-host.pth"), tree_update_backend="sklearn", **kwargs)
    shape = lambda t: [(n.wnid, [c.wnid for c in n.children]) for n in t.inodes]
    before = shape(crit.tree)
    crit.set_epoch(2, 10)
    host.set_epoch(2, 10)
    assert os.path.exists(tmp_path / "ckpt-dev" / "graph-epoch2.json")
    assert shape(crit.tree) == shape(host.tree) != before
    z = torch.randn(32, 10, device=DEV)
    y = torch.randint(0, 10, (32,), device=DEV)
    loss, gz = crit.loss_and_grad(z, y)                            # one step on the swapped tree
    want, gz_host = host.loss_and_grad(z, y)
    assert torch.isfinite(loss) and abs(loss.item() - want.item()) <= 1e-6 * abs(want.item())
    assert torch.allclose(gz, gz_host, rtol=0, atol=1e-7)


def _tie_inputs():
    grid = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(64, 2).astype(np.float32)
    twins = random_centers(20, 5)
    twins[7] = twins[3]
    same = np.tile(random_centers(1, 4), (16, 1))
    return {"grid": grid, "twins": twins, "same": same}


@pytest.mark.parametrize("method", R.LINKAGES)
@pytest.mark.parametrize("name", ["grid", "twins", "same"])
def test_ties_give_a_valid_reproducible_dendrogram(name, method):
    X = _tie_inputs()[name]
    n = X.shape[0]
    children, heights = device_linkage(X, method)
    R.check_dendrogram(children, n)
    assert np.all(np.diff(heights) >= 0)
    _, want_heights = R.linkage_ref(X, method)
    assert_heights(np.sort(heights), np.sort(want_heights), f"ties {name} {method}")
    again_children, again_heights = device_linkage(X, method)
    assert np.array_equal(children, again_children) and heights.tobytes() == again_heights.tobytes()


def test_abi_refusals_launch_nothing_and_leave_the_outputs():
    lib = _C.lib()
    n, d = 8, 3
    x = torch.from_numpy(random_centers(n, d)).to(DEV)
    nbytes = G.linkage_workspace_bytes(n)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    merges = torch.full((n - 1, 2), -7, dtype=torch.int32, device=DEV)
    heights = torch.full((n - 1,), -7.0, dtype=torch.float64, device=DEV)
    sizes = torch.full((n - 1,), -7, dtype=torch.int32, device=DEV)
    stream = _C.stream_of(x)

    def call(centers=x, n=n, d=d, method=0, metric=0, workspace=ws, workspace_bytes=nbytes, m=merges, h=heights, s=sizes):
        return lib.nbdt_linkage(_C.ptr(centers), n, d, method, metric, _C.ptr(workspace), workspace_bytes, _C.ptr(m),
                                _C.ptr(h), _C.ptr(s), stream)

    refused = [dict(n=1), dict(n=0), dict(d=0), dict(method=_C.NBDT_LINKAGE["ward"], metric=_C.NBDT_METRIC["cosine"]),
               dict(method=_C.NBDT_LINKAGE["ward"], metric=_C.NBDT_METRIC["manhattan"]), dict(method=4), dict(metric=-1),
               dict(workspace_bytes=nbytes - 1), dict(centers=None), dict(workspace=None), dict(m=None), dict(h=None),
               dict(s=None)]
    for kwargs in refused:
        assert call(**kwargs) == -1, kwargs
        assert lib.nbdt_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((merges == -7).all()) and bool((heights == -7.0).all())
    assert bool((sizes == -7).all())
    nb = ctypes.c_int64(-5)
    assert lib.nbdt_linkage_workspace_bytes(1, ctypes.byref(nb)) == -1 and nb.value == -5
    assert call() == 0                                             # the same buffers, accepted
    torch.cuda.synchronize()
    assert int(sizes.max()) == n and float(heights.min()) > 0


def test_an_input_whose_workspace_cannot_be_allocated_is_refused():
    """200,000 classes need a 320 GB distance matrix: a RuntimeError that names n and the bytes, nothing allocated."""
    n = 200_000
    x = torch.zeros(n, 1, device=DEV)
    x[:, 0] = torch.arange(n, device=DEV)
    with pytest.raises(RuntimeError, match=rf"n = {n} .* {G.linkage_workspace_bytes(n)} bytes"):
        G.linkage_children(x, backend="device")


def test_main_induces_the_hierarchy_from_the_resumed_checkpoint(tmp_path, monkeypatch):
    """main.py --induce-hierarchy: the graph is written from the checkpoint's classifier before the tree is built (to
    --path-graph here, so that the package's own hierarchies stay as shipped), equals the sklearn backend's, and the
    evaluation that follows runs on it."""
    import importlib.util
    import nbdt_path
    spec = importlib.util.spec_from_file_location("nbdt_main_induce", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    common = "--arch ResNet10 --dataset CIFAR10 --batch-size 64 --synthetic 128 --lr 0.05".split()
    M.main(common + ["--epochs", "1"])
    ck = "checkpoint/ckpt-CIFAR10-ResNet10-lr0.05.pth"
    assert os.path.exists(ck)
    path_graph = str(tmp_path / "graph-induced-ResNet10.json")
    acc, nbdt_acc = M.main(common + ["--loss", "SoftTreeSupLoss", "--analysis", "SoftEmbeddedDecisionRules", "--eval",
                                     "--resume", "--path-resume", ck, "--induce-hierarchy", "--path-graph", path_graph])
    assert 0.0 <= nbdt_acc <= 100.0
    wnids = get_wnids(dataset_to_default_path_wnids("CIFAR10"))
    want = G.build_induced_graph(wnids, checkpoint=ck, dataset="CIFAR10", backend="sklearn").node_link_data()
    with open(path_graph) as f:
        assert json.load(f) == want
