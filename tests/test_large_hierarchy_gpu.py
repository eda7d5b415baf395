"""The global-row form of the tree-rule kernels (csrc/rules_global.h): hierarchies too large for LDS in automatic mode,
and, forced with ops.set_rules_path("global"), everything the LDS form runs -- against oracle/nbdt_oracle.py,
tests/_soft_target_ref.py and the LDS form's own bits.

Tolerances are the ones stated at the top of tests/test_rules_shapes_gpu.py (its helpers are imported, not restated).
tests/test_large_hierarchy.py asserts without a GPU that the large shapes lie where the LDS form refuses.

The float64 reference of the smoothed / dense losses (_soft_target_ref) builds a dense [R, C] membership matrix, 7.6 GB
at 21,841 classes.  _large_tree_cases.ref_soft_losses / ref_hard_loss are the same formulas on a sparse matrix (and one
path product per shape for the three soft targets); tests/test_large_hierarchy.py pins them to _soft_target_ref."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _large_tree_cases as L
import _tree_shapes as S
import nbdt_oracle as O
from conftest import GOLDEN_CASES
from test_diagnostics import soft_gap_rows
from test_rules_shapes_gpu import W_XENT, TSW, _assert_P, _check, _decisions, _np, dense_targets, inputs

pytestmark = pytest.mark.gpu

from nbdt import _C, analysis, diagnostics, engine as E, ops  # noqa: E402
from nbdt.loss import HardTreeSupLoss, SoftTreeSupLoss  # noqa: E402
from nbdt.model import HardNBDT, SoftNBDT  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
B = L.B
LARGE = list(L.LARGE)
_large = {}


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("large_hierarchy_gpu")


class _Fixture:
    """A hierarchy with seeded inputs and the oracle's node outputs and P: computed once, shared, never written to."""

    def __init__(self, name, tree, otree, z, y):
        self.name, self.tree, self.otree, self.flat = name, tree, otree, tree.flat
        self.C, self.N = self.flat.num_classes, self.flat.num_inodes
        self.single_path = self.flat.multi_path_node is None
        self.handle = tree.device_handle(0)
        self.z, self.y = np.ascontiguousarray(z, dtype=np.float32), np.ascontiguousarray(y, dtype=np.int64)
        self.outs = O.node_outputs(otree, self.z)
        self.P = O.soft_forward(otree, self.z, self.outs) if self.single_path else None
        for a in (self.z, self.y):
            a.setflags(write=False)
        self.zd, self.yd = torch.from_numpy(self.z.copy()).to(DEV), torch.from_numpy(self.y.copy()).to(DEV)
        self._soft_refs = None

    def soft_refs(self):
        """_soft_target_ref's (loss, dz) for class indices at smoothing 0 and 0.1 and for dense rows at smoothing 0."""
        if self._soft_refs is None:
            t = dense_targets(self.z.shape[0], self.C)
            self.t = t
            self._soft_refs = L.ref_soft_losses(self.flat, self.z, [(self.y, 0.0), (self.y, 0.1), (t.numpy(), 0.0)],
                                               W_XENT, TSW)
        return self._soft_refs


def _large_case(name, directory):
    if name not in _large:
        pg, pw, leaves = L.build(name, directory)
        tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
        C = len(leaves)
        _large[name] = _Fixture(name, tree, O.OracleTree(pg, pw), L.logits_for(C), L.labels_for(C))
    return _large[name]


# ------------------------------------------------------------------------------------------------------------
# the comparisons against the oracle, shared by the automatic and the forced tests; `path` is what every launch must take

def _took(path):
    assert _C.last_rules_path() == path, (_C.last_rules_path(), path)


def check_node_outputs(c, path):
    logits, probs, preds, ent = _np(*_C.node_outputs(c.handle, c.zd))
    _took(path)
    assert np.array_equal(logits, np.concatenate([o["logits"] for o in c.outs], 1))      # the ordered-sum contract
    assert np.array_equal(preds, np.stack([o["preds"] for o in c.outs], 1))
    np.testing.assert_allclose(probs, np.concatenate([o["probs"] for o in c.outs], 1), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(ent, np.stack([o["entropy"] for o in c.outs], 1), rtol=1e-4, atol=1e-6)
    only = _C.node_logits(c.handle, c.zd).cpu().numpy()                                   # the logits-only launch
    _took(path)
    assert np.array_equal(only, logits)
    return logits, preds


def check_soft_forward(c, path):
    P = _C.soft_forward(c.handle, c.zd).cpu().numpy()
    _took(path)
    _assert_P(P, c.P, c.flat, c.name)
    safe = soft_gap_rows(c.P)
    assert np.array_equal(P.argmax(1)[safe], c.P.argmax(1)[safe])
    return P


def check_hard_forward(c, path):
    want, steps = O.hard_forward(c.otree, c.z, c.outs, with_decisions=True)
    pred, onehot, dec = _C.hard_forward(c.handle, c.zd, want_onehot=True, want_decisions=True)
    _took(path)
    pred = pred.cpu().numpy()
    assert np.array_equal(pred, want)
    assert torch.equal(onehot.argmax(1).cpu(), torch.from_numpy(want)) and onehot.sum().item() == len(want)
    assert set(onehot.unique().tolist()) <= {0.0, 1.0}
    dec = _np(*dec)
    _decisions(c, steps, *dec, c.name)
    assert np.array_equal(_C.hard_forward(c.handle, c.zd, want_onehot=False)[0].cpu().numpy(), want)
    _took(path)
    return pred, dec[0], dec[1]


def check_soft_backward(c, path):
    gP = torch.randn(c.z.shape[0], c.C, generator=torch.Generator().manual_seed(c.C + 1))
    gz = _C.soft_backward(c.handle, c.zd, gP.to(DEV)).cpu().numpy()
    _took(path)
    want = O.rules_backward(c.otree, c.z, gP.numpy(), outs=c.outs, P=c.P)
    print(f"{c.name}: rules backward max abs err {np.abs(gz - want).max():.2e}")
    np.testing.assert_allclose(gz, want, atol=2e-6, rtol=1e-5)


def check_hard_loss(c, path):
    for wx, tsw in ((1.0, 1.0), (0.5, 10.0)):
        loss, gz = _C.hard_tree_loss(c.handle, c.zd, c.yd, wx, tsw * tsw * 2.0 / c.N)
        _took(path)
        lo, dzo = O.hard_tree_sup_loss(c.otree, c.z, c.y, wx, tsw)
        print(f"{c.name} hard ({wx}, {tsw}): loss rel {abs(loss.item() - lo) / abs(lo):.2e}, "
              f"dz abs {np.abs(gz.cpu().numpy() - dzo).max():.2e}")
        assert abs(loss.item() - lo) <= 1e-5 * abs(lo)
        np.testing.assert_allclose(gz.cpu().numpy(), dzo, atol=1e-6, rtol=1e-5)
    w_node = TSW * TSW * 2.0 / c.N
    loss, gz = _C.hard_tree_loss(c.handle, c.zd, c.yd, W_XENT, w_node, smoothing=0.1)
    _took(path)
    _check("hard", loss.item(), gz.cpu().numpy(), *L.ref_hard_loss(c.flat, c.z, c.y, 0.1, W_XENT, w_node),
           f"{c.name} smoothed hard")


def check_soft_loss(c, path):
    for wx, wt in ((1.0, 1.0), (0.5, 10.0)):
        loss, gz = _C.soft_tree_loss(c.handle, c.zd, c.yd, wx, wt)
        _took(path)
        lo, dzo = O.soft_tree_sup_loss(c.otree, c.z, c.y, wx, wt)
        print(f"{c.name} soft ({wx}, {wt}): loss rel {abs(loss.item() - lo) / abs(lo):.2e}, "
              f"dz abs {np.abs(gz.cpu().numpy() - dzo).max():.2e}")
        assert abs(loss.item() - lo) <= 1e-5 * abs(lo)
        np.testing.assert_allclose(gz.cpu().numpy(), dzo, atol=1e-6, rtol=0)
        assert np.abs(gz.cpu().numpy().sum(1)).max() < 1e-6 * max(1.0, wx + wt)


def check_soft_targets(c, path):
    """As test_soft_targets_gpu._check: class indices, smoothing 0.1, dense rows, against _soft_target_ref."""
    plain, smoothed, dense = c.soft_refs()
    loss, gz = _C.soft_tree_loss(c.handle, c.zd, c.yd, W_XENT, TSW)
    _took(path)
    _check("soft", loss.item(), gz.cpu().numpy(), *plain, f"{c.name} class indices")
    loss, gz = _C.soft_tree_loss(c.handle, c.zd, c.yd, W_XENT, TSW, smoothing=0.1)
    _took(path)
    _check("soft", loss.item(), gz.cpu().numpy(), *smoothed, f"{c.name} smoothed soft")
    loss, gz = _C.soft_tree_loss_dense(c.handle, c.zd, c.t.to(DEV), W_XENT, TSW)
    _took(path)
    _check("soft", loss.item(), gz.cpu().numpy(), *dense, f"{c.name} dense")


# ------------------------------------------------------------------------------------------------------------
# 1. large shapes, automatic mode: each of these fails with "hierarchy too large for LDS" without the global-row form

@pytest.mark.parametrize("name", LARGE)
def test_large_node_outputs(name, shapes_dir):
    assert ops.rules_path() == "auto"
    check_node_outputs(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_soft_forward(name, shapes_dir):
    check_soft_forward(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_hard_forward_and_decisions(name, shapes_dir):
    check_hard_forward(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_soft_backward(name, shapes_dir):
    check_soft_backward(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_hard_tree_loss(name, shapes_dir):
    check_hard_loss(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_soft_tree_loss(name, shapes_dir):
    check_soft_loss(_large_case(name, shapes_dir), "global")


@pytest.mark.parametrize("name", LARGE)
def test_large_soft_tree_loss_smoothed_and_dense(name, shapes_dir):
    check_soft_targets(_large_case(name, shapes_dir), "global")


def test_large_node_logits_backward(shapes_dir):
    """nbdt_node_logits_backward has no LDS limit: its VJP on a large shape is the transpose of the mean."""
    c = _large_case("kary5000_17", shapes_dir)
    gs = torch.randn(B, c.flat.num_slots, generator=torch.Generator().manual_seed(5))
    gz = _C.node_logits_backward(c.handle, gs.to(DEV)).cpu().numpy()
    f = c.flat
    want = np.zeros((B, c.C))
    for s in range(f.num_slots):
        cls = f.slot_cls[f.slot_off[s]:f.slot_off[s + 1]]
        want[:, cls] += gs.numpy()[:, s:s + 1].astype(np.float64) / len(cls)
    np.testing.assert_allclose(gz, want, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------
# 2. forced mode on everything the LDS form runs

def _lds_then_global(c):
    """The bit-exact outputs under both forms, and every oracle comparison under the forced one."""
    d = S.describe(c.flat)
    assert ops.rules_path() == "auto"
    lds = {"logits": _C.node_outputs(c.handle, c.zd)[0], "preds": _C.node_outputs(c.handle, c.zd)[2]}
    assert _C.last_rules_path() == L.expected_path(c.flat, "node_outputs", d) != "global"
    pred, _, dec = _C.hard_forward(c.handle, c.zd, want_onehot=False, want_decisions=True)
    assert _C.last_rules_path() == L.expected_path(c.flat, "hard_forward", d) != "global"
    lds.update(pred=pred, nodes=dec[0], children=dec[1])
    ops.set_rules_path("global")
    try:
        logits, preds = check_node_outputs(c, "global")
        pred, nodes, children = check_hard_forward(c, "global")
        check_hard_loss(c, "global")
        if c.single_path:               # the soft rules refuse a class under two children of one node
            check_soft_forward(c, "global")
            check_soft_backward(c, "global")
            check_soft_loss(c, "global")
            check_soft_targets(c, "global")
    finally:
        ops.set_rules_path("auto")
    for key, got in (("logits", logits), ("preds", preds), ("pred", pred), ("nodes", nodes), ("children", children)):
        want = lds[key].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32)), (c.name, key)


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_forced_global_rows_on_the_synthetic_shapes(name, shapes_dir):
    pg, pw, leaves = S.build(name, shapes_dir)
    tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
    _lds_then_global(_Fixture(name, tree, O.OracleTree(pg, pw), *inputs(name, B, len(leaves))))


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_forced_global_rows_on_the_shipped_hierarchies(tag, golden_dir, pkg_dir):
    ds, h = GOLDEN_CASES[tag]
    g = np.load(os.path.join(golden_dir, f"rules_{tag}.npz"))
    c = _Fixture(tag, Tree(ds, hierarchy=h), O.OracleTree(*O.default_paths(ds, h, pkg_dir)), g["z"], g["y"])
    _lds_then_global(c)           # a multi-parent WordNet graph (c.single_path false): the hard and node entry points


# ------------------------------------------------------------------------------------------------------------
# 3. / 4. batch independence and run-to-run, bit for bit

def _loss_rows(c, kind, z, y, grad_scale, smoothing=0.0):
    """(row losses [B], gz) of a fused loss through the C ABI: the row buffer is what _C's wrappers drop."""
    n = z.shape[0]
    row = torch.empty((n,), dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    gz = torch.empty((n, c.C), dtype=torch.float32, device=DEV)
    lib, p = _C.lib(), _C.ptr
    if kind == "soft":
        _C.check(lib.nbdt_soft_tree_loss_ex(c.handle.h, p(z), _C.ztype_of(z), n, c.C, p(y), None, 0, float(smoothing), 1.0, 1.0,
                                            float(grad_scale), p(row), p(loss), p(gz), _C.stream_of(z)))
    else:
        _C.check(lib.nbdt_hard_tree_loss_ex(c.handle.h, p(z), _C.ztype_of(z), n, c.C, p(y), float(smoothing), 1.0, 2.0 / c.N,
                                            float(grad_scale), p(row), p(loss), p(gz), _C.stream_of(z)))
    _took("global")
    return row, gz


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_rows_do_not_depend_on_the_batch(shapes_dir):
    """B = 1, 6, 300 on kary(2560, 2) with grad_scale = B (scale = 1 in every launch).  300 samples are more than one
    pass of the CU-bounded grid, so the blocks stride."""
    c = _large_case("kary2560_2", shapes_dir)
    big = 300
    z = torch.from_numpy(L.logits_for(c.C, big)).to(DEV)
    y = torch.from_numpy(L.labels_for(c.C, big)).to(DEV)

    def launch(n):
        zz, yy = z[:n].contiguous(), y[:n].contiguous()
        out = [*_loss_rows(c, "soft", zz, yy, n), *_loss_rows(c, "soft", zz, yy, n, 0.1), *_loss_rows(c, "hard", zz, yy, n),
               _C.soft_forward(c.handle, zz), _C.hard_forward(c.handle, zz, want_onehot=False)[0],
               _C.node_outputs(c.handle, zz)[2]]
        _took("global")
        return out

    full = launch(big)
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all()
    Po = O.soft_forward(c.otree, z[:8].cpu().numpy())
    _assert_P(full[6][:8].cpu().numpy(), Po, c.flat, "B=300, first rows")
    for n in (1, 6):
        for i, (a, b) in enumerate(zip(launch(n), full)):
            assert torch.equal(_bits(a), _bits(b[:n])), f"B={n}: output {i}"


def test_two_launches_leave_the_same_bits(shapes_dir):
    c = _large_case("kary8192_2", shapes_dir)
    t = dense_targets(B, c.C).to(DEV)
    w_node = TSW * TSW * 2.0 / c.N

    def launch():
        out = [*_C.soft_tree_loss(c.handle, c.zd, c.yd, W_XENT, TSW), *_C.soft_tree_loss(c.handle, c.zd, c.yd, W_XENT, TSW, smoothing=0.1),
               *_C.soft_tree_loss_dense(c.handle, c.zd, t, W_XENT, TSW), *_C.hard_tree_loss(c.handle, c.zd, c.yd, W_XENT, w_node),
               *_C.hard_tree_loss(c.handle, c.zd, c.yd, W_XENT, w_node, smoothing=0.1)]
        _took("global")
        return out

    for i, (a, b) in enumerate(zip(launch(), launch())):
        assert torch.equal(_bits(a), _bits(b)), f"output {i}"


# ------------------------------------------------------------------------------------------------------------
# 5. inputs

def _rounded(c, zl):
    """A fixture on the logits a half-precision or strided tensor really holds."""
    return _Fixture(c.name, c.tree, c.otree, zl.float().cpu().numpy(), c.y)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_precision_logits(dtype, shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    zl = c.zd.to(dtype)
    assert not torch.equal(zl.float(), c.zd)
    r = _rounded(c, zl)
    r.zd = zl                                     # the launches read the 16-bit tensor, the oracle its up-cast values
    check_node_outputs(r, "global")
    check_soft_forward(r, "global")
    check_hard_forward(r, "global")
    check_soft_loss(r, "global")
    check_hard_loss(r, "global")
    check_soft_backward(r, "global")


def test_row_stride_above_the_class_count(shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    wide = torch.full((B, c.C + 7), 1e6, device=DEV)      # what lies behind a row would be seen at once
    wide[:, :c.C] = c.zd
    view = wide[:, :c.C]
    assert view.stride(0) == c.C + 7 and not view.is_contiguous()
    r = _rounded(c, c.zd)
    r.zd = view
    check_node_outputs(r, "global")
    check_soft_forward(r, "global")
    check_hard_forward(r, "global")
    check_soft_loss(r, "global")
    check_hard_loss(r, "global")
    check_soft_backward(r, "global")


def test_bad_labels_give_nan_and_empty_batches_are_accepted(shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    for bad in (-1, c.C):
        y = c.yd.clone()
        y[2] = bad
        for loss, gz in (_C.soft_tree_loss(c.handle, c.zd, y, 1.0, 1.0), _C.soft_tree_loss(c.handle, c.zd, y, 1.0, 1.0, smoothing=0.1),
                         _C.hard_tree_loss(c.handle, c.zd, y, 1.0, 1.0), _C.hard_tree_loss(c.handle, c.zd, y, 1.0, 1.0, smoothing=0.1)):
            _took("global")
            assert torch.isnan(loss).item(), bad
    empty = torch.empty((0, c.C), device=DEV)
    assert _C.soft_forward(c.handle, empty).shape == (0, c.C)
    pred, onehot, _ = _C.hard_forward(c.handle, empty)
    assert pred.shape == (0,) and onehot.shape == (0, c.C)
    assert _C.node_outputs(c.handle, empty)[0].shape == (0, c.flat.num_slots)


# ------------------------------------------------------------------------------------------------------------
# 6. / 7. the public layer on kary(2560, 2), and what still refuses

class _Stub(nn.Module):
    """A backbone that returns fixed logits."""

    def __init__(self, z):
        super().__init__()
        self.z = z

    def forward(self, x):
        return self.z[:x.shape[0]]


def _paths(shapes_dir):
    pg, pw, leaves = L.build("kary2560_2", shapes_dir)
    return dict(path_graph=pg, path_wnids=pw, classes=leaves)


def test_nbdt_modules(shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    kw = _paths(shapes_dir)
    x = torch.zeros(B, 3, device=DEV)
    soft = SoftNBDT(None, _Stub(c.zd), **kw)
    P = soft(x)
    _took("global")
    _assert_P(P.detach().cpu().numpy(), c.P, c.flat, "SoftNBDT")
    Ps, sdec = soft.forward_with_decisions(x)
    assert len(sdec) == B and torch.equal(Ps, P)
    hard = HardNBDT(None, _Stub(c.zd), **kw)
    want, steps = O.hard_forward(c.otree, c.z, c.outs, with_decisions=True)
    H, hdec = hard.forward_with_decisions(x)
    _took("global")
    assert np.array_equal(H.argmax(1).cpu().numpy(), want) and torch.equal(hard(x), H)
    for dec, walk, p in zip(hdec, steps, want):
        assert dec[0]["name"] == "root" and len(dec) == len(walk) + 1
        assert dec[-1]["node"].wnid == hard.rules.tree.wnids_leaves[p]
    # autograd through the soft rules
    zz = c.zd.clone().requires_grad_(True)
    gP = torch.randn(B, c.C, generator=torch.Generator().manual_seed(c.C + 1))
    soft.rules(zz).backward(gP.to(DEV))
    _took("global")
    np.testing.assert_allclose(zz.grad.cpu().numpy(), O.rules_backward(c.otree, c.z, gP.numpy(), outs=c.outs, P=c.P),
                               atol=2e-6, rtol=1e-5)


def test_losses_forward_backward_equal_loss_and_grad(shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    for Loss, ref in ((SoftTreeSupLoss, O.soft_tree_sup_loss), (HardTreeSupLoss, O.hard_tree_sup_loss)):
        crit = Loss(dataset=None, criterion=nn.CrossEntropyLoss(), tree=c.tree, tree_supervision_weight=2.0)
        zz = c.zd.clone().requires_grad_(True)
        loss = crit(zz, c.yd)
        loss.backward()
        _took("global")
        l2, g2 = crit.loss_and_grad(c.zd, c.yd)
        _took("global")
        assert loss.item() == l2.item() and torch.equal(zz.grad, g2)
        lo, dzo = ref(c.otree, c.z, c.y, 1.0, 2.0)
        assert abs(loss.item() - lo) <= 1e-5 * abs(lo)
        np.testing.assert_allclose(zz.grad.cpu().numpy(), dzo, atol=1e-6, rtol=1e-5)
    crit = SoftTreeSupLoss(dataset=None, criterion=nn.CrossEntropyLoss(), tree=c.tree, tree_supervision_weight=TSW,
                           xent_weight=W_XENT)
    _, _, dense = c.soft_refs()
    loss, gz = crit.soft_target_loss_and_grad(c.zd, c.t.to(DEV))
    _took("global")
    _check("soft", loss.item(), gz.cpu().numpy(), *dense, "soft_target_loss_and_grad")
    assert crit.can_fuse_head(c.C) is False


def test_analysis_top5_counts(shapes_dir):
    """Half of the labels are the oracle's most probable class (in any top 5), half its least probable one (in none)."""
    c = _large_case("kary2560_2", shapes_dir)
    y = c.P.argmax(1)
    y[B // 2:] = c.P.argmin(1)[B // 2:]
    for Rules, metric, want in ((analysis.SoftEmbeddedDecisionRules, "top5", B // 2),
                                (analysis.SoftEmbeddedDecisionRules, "top1", B // 2),
                                (analysis.HardEmbeddedDecisionRules, "top1",
                                 int((O.hard_forward(c.otree, c.z, c.outs) == y).sum()))):
        a = Rules(tree=c.tree, metric=metric)
        a.start_test(0)
        a.update_batch(c.zd, torch.from_numpy(y).to(DEV))
        _took("global")
        assert (a.correct, a.total) == (want, B), (Rules.__name__, metric)


def test_train_step_takes_the_unfused_head(shapes_dir):
    """A 2,560-class classifier: linear_fwd -> loss_and_grad -> linear_bwd, the loss on the global-row kernels."""
    c = _large_case("kary2560_2", shapes_dir)
    crit = SoftTreeSupLoss(dataset=None, criterion=nn.CrossEntropyLoss(), tree=c.tree)
    assert not crit.can_fuse_head(c.C)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, c.C, (4,), generator=g).to(DEV)
    ops.set_deterministic(True)          # the forward below and the step's own are then the same bits
    try:
        eng = E.ResNetEngine(num_blocks=(1, 1, 1, 1), num_classes=c.C, device=DEV, seed=5)
        z = eng.forward(x, training=True).float().cpu().numpy()
        loss = E.train_step(eng, crit, x, y, 0.0, 0.0, 0.0, zero_grad=False).item()
    finally:
        ops.set_deterministic(False)
    _took("global")
    assert z.shape == (4, c.C)
    lo, _ = O.soft_tree_sup_loss(c.otree, z, y.cpu().numpy())
    print(f"train_step loss {loss:.6f}, oracle {lo:.6f}")
    assert abs(loss - lo) <= 1e-5 * abs(lo)
    grad = eng.store.grad
    assert torch.isfinite(grad).all() and grad.abs().max().item() > 0


def test_diagnostics_and_fused_head_still_refuse(shapes_dir):
    c = _large_case("kary2560_2", shapes_dir)
    stats = diagnostics.TreeStatistics(tree=c.tree, confusions=False)
    stats.start_test(0)
    with pytest.raises((ValueError, _C.NBDTHipError), match="too large for LDS"):
        stats.update_batch(c.zd, c.yd)
    crit = SoftTreeSupLoss(dataset=None, criterion=nn.CrossEntropyLoss(), tree=c.tree)
    assert crit.can_fuse_head(2560) is False
    pooled, W = torch.randn(B, 64, device=DEV), torch.randn(c.C, 64, device=DEV)
    with pytest.raises(_C.NBDTHipError, match="512 classes"):
        _C.head_soft_tree_loss(c.handle, pooled, W, None, c.yd, 1.0, 1.0)
