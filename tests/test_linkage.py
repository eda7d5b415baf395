"""Host side of device-induced hierarchies (no GPU): the numpy oracle the GPU tests compare csrc/linkage.hip with
(tests/_linkage_ref.py) is pinned to scipy.cluster.hierarchy.linkage -- children exactly, heights to 1e-12 -- and
nbdt.graph.linkage_children refuses bad arguments, keeps the sklearn backend's results and labels raw merges the way
scipy does."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import graph as G

import _linkage_ref as R

SHAPES = [(2, 3), (3, 1), (5, 1), (65, 7), (300, 33)]
PAIRS = [(m, a) for m in R.LINKAGES for a in R.METRICS if m != "ward" or a == "euclidean"]
SCIPY_METRIC = {"euclidean": "euclidean", "manhattan": "cityblock", "cosine": "cosine"}
FIXTURES = ("cifar10", "cifar100", "tiny200")


def random_centers(n, d, seed=1):
    """Seeded Gaussian fp32 rows.  With d = 1 every cosine distance is exactly 0 or 2, so the n = 5 case is all ties and
    its children are a matter of tie order: scipy's single linkage (a minimum spanning tree, not a chain) orders them
    differently for some seeds.  Seed 1 is one for which no case depends on that."""
    return np.random.default_rng(1000 * n + d + seed).standard_normal((n, d)).astype(np.float32)


def _assert_equals_scipy(X, method, metric):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    Z = hierarchy.linkage(X.astype(np.float64), method=method, metric=SCIPY_METRIC[metric])
    children, heights = R.linkage_ref(X, method, metric)
    assert children.dtype == np.int64 and np.array_equal(children, Z[:, :2].astype(np.int64))
    np.testing.assert_allclose(heights, Z[:, 2], rtol=1e-12, atol=1e-300)
    R.check_dendrogram(children, X.shape[0])


@pytest.mark.parametrize("method,metric", PAIRS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_oracle_equals_scipy_on_random_inputs(n, d, method, metric):
    _assert_equals_scipy(random_centers(n, d), method, metric)


@pytest.mark.parametrize("method,metric", PAIRS)
@pytest.mark.parametrize("tag", FIXTURES)
def test_oracle_equals_scipy_on_the_reference_fixtures(tag, method, metric, golden_dir):
    _assert_equals_scipy(np.load(os.path.join(golden_dir, f"induced_{tag}.npz"))["W"], method, metric)


def test_label_merges_is_the_oracles_labelling():
    """nbdt.graph.label_merges (product) and _linkage_ref.label (oracle) are written separately and agree, ties in
    the heights included (stable sort)."""
    X = random_centers(65, 7)
    merges, heights, _ = R.nn_chain(R.pairwise(X), "ward")
    for h in (heights, np.round(heights, 1)):
        want_c, want_h = R.label(merges, h, 65)
        got_c, got_h = G.label_merges(merges, h, 65)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_h, want_h)


def test_linkage_children_refuses_bad_arguments():
    x = torch.from_numpy(random_centers(8, 3))
    for backend in (None, "sklearn", "device"):
        with pytest.raises(ValueError, match="ward"):
            G.linkage_children(x, linkage="ward", affinity="cosine", backend=backend)
        with pytest.raises(ValueError, match="n >= 2"):
            G.linkage_children(x[:1], backend=backend)
        with pytest.raises(ValueError, match="unknown linkage"):
            G.linkage_children(x, linkage="centroid", backend=backend)
        with pytest.raises(ValueError, match="unknown affinity"):
            G.linkage_children(x, affinity="chebyshev", backend=backend)
    with pytest.raises(ValueError, match="unknown backend"):
        G.linkage_children(x, backend="scipy")


def test_device_backend_has_no_cpu_fallback():
    x = torch.from_numpy(random_centers(8, 3))
    if torch.cuda.is_available():           # (tests/test_linkage_gpu.py is where the device backend is checked)
        assert G.linkage_children(x, backend="device")[0].shape == (7, 2)
        return
    with pytest.raises(_C.NBDTHipError, match="needs a HIP device"):
        G.linkage_children(x, backend="device")


def test_abi_refusals_need_no_gpu():
    """nbdt_linkage validates every argument before its first device call: each refusal is NBDT_EINVAL on a box
    without a GPU too, and nbdt_linkage_workspace_bytes is host arithmetic."""
    import ctypes
    lib = _C.lib()
    assert lib.nbdt_version() >= 128
    nbytes = ctypes.c_int64(-1)
    assert lib.nbdt_linkage_workspace_bytes(1000, ctypes.byref(nbytes)) == 0
    assert 8 * 1000 * 1000 + 8 * 1000 <= nbytes.value <= 8 * 1000 * 1000 + 8 * 1000 + 256
    assert lib.nbdt_linkage_workspace_bytes(21841, ctypes.byref(nbytes)) == 0 and nbytes.value > 8 * 21841 ** 2 > 2 ** 31
    assert lib.nbdt_linkage_workspace_bytes(1, ctypes.byref(nbytes)) == -1
    assert lib.nbdt_linkage_workspace_bytes(1000, None) == -1
    assert G.linkage_workspace_bytes(65) == 8 * 65 * 65 + 768
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused on the host
    big = 1 << 40
    assert lib.nbdt_linkage(None, 8, 3, 0, 0, p, big, p, p, p, None) == -1
    assert b"null pointer" in lib.nbdt_last_error()
    assert lib.nbdt_linkage(p, 8, 3, 0, 0, None, big, p, p, p, None) == -1
    assert lib.nbdt_linkage(p, 8, 3, 0, 0, p, big, None, p, p, None) == -1
    assert lib.nbdt_linkage(p, 1, 3, 0, 0, p, big, p, p, p, None) == -1
    assert lib.nbdt_linkage(p, 8, 0, 0, 0, p, big, p, p, p, None) == -1
    assert lib.nbdt_linkage(p, 8, 3, 4, 0, p, big, p, p, p, None) == -1
    assert lib.nbdt_linkage(p, 8, 3, 1, 3, p, big, p, p, p, None) == -1
    assert lib.nbdt_linkage(p, 8, 3, _C.NBDT_LINKAGE["ward"], _C.NBDT_METRIC["cosine"], p, big, p, p, p, None) == -1
    assert b"ward" in lib.nbdt_last_error()
    assert lib.nbdt_linkage(p, 8, 3, 0, 0, p, 8 * 8 * 8, p, p, p, None) == -1
    assert b"workspace too small" in lib.nbdt_last_error()


@pytest.mark.parametrize("linkage,affinity", [("ward", "euclidean"), ("average", "cosine"), ("complete", "l1")])
def test_sklearn_backend_returns_sklearns_children(linkage, affinity):
    cluster = pytest.importorskip("sklearn.cluster")
    X = random_centers(65, 7)
    want = cluster.AgglomerativeClustering(linkage=linkage, n_clusters=2, metric=affinity).fit(X).children_
    for backend in ("sklearn", None):           # None: sklearn imports here, so callers get what they always got
        children, heights = G.linkage_children(torch.from_numpy(X), linkage=linkage, affinity=affinity, backend=backend)
        assert children.dtype == np.int64 and heights.dtype == np.float64
        assert np.array_equal(children, want) and heights.shape == (64,) and np.all(np.diff(heights) >= 0)


def test_induce_hierarchy_flag_parses():
    spec = importlib.util.spec_from_file_location("nbdt_main_linkage", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    a = M.parse_args("--arch ResNet18 --loss SoftTreeSupLoss --induce-hierarchy --resume --path-resume x.pth".split())
    assert a.induce_hierarchy and a.induced_linkage == "ward" and a.path_resume == "x.pth"
    assert not M.parse_args([]).induce_hierarchy                  # existing command lines: nothing changes
    with pytest.raises(SystemExit):                               # a classifier to cluster is required
        M.parse_args(["--induce-hierarchy"])
    with pytest.raises(SystemExit):
        M.parse_args("--induce-hierarchy --resume --path-resume x.pth --hierarchy wordnet".split())
