"""The tree-rule kernels of csrc/rules.hip on synthetic hierarchies that reach the paths the shipped hierarchies never
select, against oracle/nbdt_oracle.py (and tests/_soft_target_ref.py for smoothed / dense targets).

tests/_tree_shapes.py builds the shapes and tests/test_tree_shapes.py asserts, without a GPU, which path each one takes
(waves per sample, Gather rounds, long_chain peels, staged or not, fan-out) and that the logits used here leave no path
probability below 1e-30.

Tolerances.  Integers and the node logits are exact (the ordered-sum contract).  Everything else is the project's:
node probabilities rtol 2e-5 / atol 1e-6, entropies rtol 1e-4 / atol 1e-6, decision probabilities 1e-6 and entropies 1e-5
absolute, loss 1e-5 relative, soft dL/dz 1e-6 absolute, hard dL/dz atol 1e-6 + rtol 1e-5 (test_full_size_vs_oracle), rules
backward atol 2e-6 + rtol 1e-5, smoothed / dense targets as test_soft_targets_gpu._check.  The path probabilities P get a
purely relative check on every entry (atol = 0; the project's atol of 1e-6 would hide every entry of a 200-factor
product): rtol = max(2e-5, 3.2e-7 * path length of the class), the per-factor figure of test_deep_hierarchy_without_lds_stage
(2e-4 over 639 factors) which agrees with the 2e-5 of SURVEY 8c at 64 factors.

Batch independence is asserted bit for bit by launching every batch size with grad_scale = B, so that the kernel's
scale = grad_scale / B is exactly 1 in each launch and the rows of two launches are the same fp32 operations (rescaling
the gradients of one launch afterwards, as test_soft_targets_gpu.test_goldens does at a tolerance, cannot be bit-exact)."""
import numpy as np
import pytest
import torch

import _soft_target_ref as R
import _tree_shapes as S
import nbdt_oracle as O
from test_diagnostics import restate, soft_gap_rows
from test_diagnostics_gpu import _check_against

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
B = 6                                    # ragged at one wave per sample, where 4 samples share a block
ALL = list(S.SHAPES)
THREE = ["cat33", "kary243_3", "kary600_70"]           # one per waves-per-sample choice (64, 256, 1024 lanes)
W_XENT, TSW = 0.5, 10.0                  # the weights of the soft-target tests

_cases = {}


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rules_shapes")


class _Case:
    """One shape: the two trees, the kernel handle, seeded inputs, and the oracle's node outputs and P (computed once,
    shared by the tests below, never written to)."""

    def __init__(self, name, directory):
        pg, pw, leaves = S.build(name, directory)
        self.name = name
        self.tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
        self.otree = O.OracleTree(pg, pw)
        self.flat = self.tree.flat
        self.C, self.N = self.flat.num_classes, self.flat.num_inodes
        self.handle = self.tree.device_handle(0)
        self.z, self.y = inputs(name, B, self.C)
        self.outs = O.node_outputs(self.otree, self.z)
        self.P = O.soft_forward(self.otree, self.z, self.outs)
        for a in (self.z, self.y, self.P):
            a.setflags(write=False)
        self.zd, self.yd = torch.from_numpy(self.z.copy()).to(DEV), torch.from_numpy(self.y.copy()).to(DEV)


def inputs(name, batch, C):
    z = S.logits_for(name, batch, C).numpy()
    y = torch.randint(0, C, (batch,), generator=torch.Generator().manual_seed(7 * C + batch)).numpy()
    y[0] = C - 1                         # the deepest class of a caterpillar
    if batch > 1:
        y[1] = 0
    return z, y


def _case(name, directory):
    if name not in _cases:
        _cases[name] = _Case(name, directory)
    return _cases[name]


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _assert_P(P, Po, flat, what):
    rtol = np.maximum(2e-5, 3.2e-7 * np.diff(flat.cls_off))[None, :]
    assert Po.min() >= 1e-30
    err = np.abs(P.astype(np.float64) - Po) / Po
    print(f"{what}: P max rel err {err.max():.2e}, worst share of the allowance {(err / rtol).max():.2f}")
    assert (err <= rtol).all(), what
    np.testing.assert_allclose(P.sum(1), 1.0, atol=2e-5)


def _decisions(c, steps, pn, pc, pp, pe, what):
    """Rows of the decision buffers against the oracle's walks, over the full depth."""
    D = pn.shape[1]
    assert D == c.handle.max_depth
    for b, walk in enumerate(steps):
        n = len(walk)
        assert n <= D
        assert np.array_equal(pn[b, :n], [s[0] for s in walk]), what
        assert np.array_equal(pc[b, :n], [s[1] for s in walk]), what
        assert (pn[b, n:] == -1).all() and (pc[b, n:] == -1).all(), what
        np.testing.assert_allclose(pp[b, :n], [s[2] for s in walk], atol=1e-6, rtol=0, err_msg=what)
        np.testing.assert_allclose(pe[b, :n], [s[3] for s in walk], atol=1e-5, rtol=0, err_msg=what)
        assert (pp[b, n:] == 0).all() and (pe[b, n:] == 0).all(), what


# ------------------------------------------------------------------------------------------------------------
# every shape against the oracle

@pytest.mark.parametrize("name", ALL)
def test_node_outputs(name, shapes_dir):
    c = _case(name, shapes_dir)
    logits, probs, preds, ent = _np(*_C.node_outputs(c.handle, c.zd))
    assert np.array_equal(logits, np.concatenate([o["logits"] for o in c.outs], 1))      # the ordered-sum contract
    assert np.array_equal(preds, np.stack([o["preds"] for o in c.outs], 1))
    np.testing.assert_allclose(probs, np.concatenate([o["probs"] for o in c.outs], 1), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(ent, np.stack([o["entropy"] for o in c.outs], 1), rtol=1e-4, atol=1e-6)
    assert np.array_equal(_C.node_logits(c.handle, c.zd).cpu().numpy(), logits)           # the logits-only launch


@pytest.mark.parametrize("name", ALL)
def test_soft_forward(name, shapes_dir):
    c = _case(name, shapes_dir)
    P = _C.soft_forward(c.handle, c.zd).cpu().numpy()
    _assert_P(P, c.P, c.flat, name)
    safe = soft_gap_rows(c.P)                                     # rows whose top-2 gap the tolerance cannot flip
    assert np.array_equal(P.argmax(1)[safe], c.P.argmax(1)[safe])


@pytest.mark.parametrize("name", ALL)
def test_hard_forward_and_decisions(name, shapes_dir):
    c = _case(name, shapes_dir)
    want, steps = O.hard_forward(c.otree, c.z, c.outs, with_decisions=True)
    pred, onehot, dec = _C.hard_forward(c.handle, c.zd, want_onehot=True, want_decisions=True)
    pred = pred.cpu().numpy()
    assert np.array_equal(pred, want)
    assert np.array_equal(onehot.cpu().numpy(), np.eye(c.C, dtype=np.float32)[want])
    _decisions(c, steps, *_np(*dec), name)
    assert np.array_equal(_C.hard_forward(c.handle, c.zd, want_onehot=False)[0].cpu().numpy(), want)
    # a walk that goes all the way down: the deepest leaf wins every node
    zdeep = np.zeros((2, c.C), dtype=np.float32)
    zdeep[:, c.C - 1] = 30.0
    zdeep[1, 0] = 31.0 if c.flat.num_inodes == 1 else -5.0
    wd, sd = O.hard_forward(c.otree, zdeep, with_decisions=True)
    pd, _, dd = _C.hard_forward(c.handle, torch.from_numpy(zdeep).to(DEV), want_onehot=False, want_decisions=True)
    assert np.array_equal(pd.cpu().numpy(), wd)
    _decisions(c, sd, *_np(*dd), name + " deepest")
    if S.SHAPES[name][0] == "caterpillar":
        assert len(sd[0]) == c.C - 1 == c.handle.max_depth


@pytest.mark.parametrize("name", ALL)
def test_soft_and_hard_tree_loss(name, shapes_dir):
    c = _case(name, shapes_dir)
    for wx, wt in ((1.0, 1.0), (0.5, 10.0)):
        loss, gz = _C.soft_tree_loss(c.handle, c.zd, c.yd, wx, wt)
        lo, dzo = O.soft_tree_sup_loss(c.otree, c.z, c.y, wx, wt)
        print(f"{name} soft ({wx}, {wt}): loss rel {abs(loss.item() - lo) / abs(lo):.2e}, "
              f"dz abs {np.abs(gz.cpu().numpy() - dzo).max():.2e}")
        assert abs(loss.item() - lo) <= 1e-5 * abs(lo)
        np.testing.assert_allclose(gz.cpu().numpy(), dzo, atol=1e-6, rtol=0)
        assert np.abs(gz.cpu().numpy().sum(1)).max() < 1e-6 * max(1.0, wx + wt)     # rows of a softmax-CE gradient sum to ~0
    for wx, tsw in ((1.0, 1.0), (0.5, 10.0)):
        loss, gz = _C.hard_tree_loss(c.handle, c.zd, c.yd, wx, tsw * tsw * 2.0 / c.N)
        lo, dzo = O.hard_tree_sup_loss(c.otree, c.z, c.y, wx, tsw)
        print(f"{name} hard ({wx}, {tsw}): loss rel {abs(loss.item() - lo) / abs(lo):.2e}, "
              f"dz abs {np.abs(gz.cpu().numpy() - dzo).max():.2e}")
        assert abs(loss.item() - lo) <= 1e-5 * abs(lo)
        np.testing.assert_allclose(gz.cpu().numpy(), dzo, atol=1e-6, rtol=1e-5)


def _check(kind, loss, gz, ref_loss, ref_dz, what):          # test_soft_targets_gpu._check
    print(f"{what}: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e}, dz abs {np.abs(gz - ref_dz).max():.2e}")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), what
    if kind == "hard":
        np.testing.assert_allclose(gz, ref_dz, atol=2e-6, rtol=1e-5, err_msg=what)
    else:
        np.testing.assert_allclose(gz, ref_dz, atol=1e-6, rtol=0, err_msg=what)


def dense_targets(batch, C):
    """Probability rows the way MixUp leaves them: two classes share the mass, the rest is zero."""
    g = torch.Generator().manual_seed(3 * C + batch)
    a, b = torch.randint(0, C, (batch,), generator=g), torch.randint(0, C, (batch,), generator=g)
    lam = torch.rand(batch, generator=g)
    t = torch.zeros(batch, C)
    t[torch.arange(batch), a] += lam
    t[torch.arange(batch), b] += 1 - lam
    return t


@pytest.mark.parametrize("name", ALL)
def test_smoothed_and_dense_targets(name, shapes_dir):
    c = _case(name, shapes_dir)
    w_node = TSW * TSW * 2.0 / c.N
    loss, gz = _C.soft_tree_loss(c.handle, c.zd, c.yd, W_XENT, TSW, smoothing=0.1)
    _check("soft", loss.item(), gz.cpu().numpy(), *R.soft_loss(c.flat, c.z, c.y, 0.1, W_XENT, TSW), f"{name} smoothed soft")
    loss, gz = _C.hard_tree_loss(c.handle, c.zd, c.yd, W_XENT, w_node, smoothing=0.1)
    _check("hard", loss.item(), gz.cpu().numpy(), *R.hard_loss(c.flat, c.z, c.y, 0.1, W_XENT, w_node), f"{name} smoothed hard")
    t = dense_targets(B, c.C)
    for eps in (0.0, 0.1):
        loss, gz = _C.soft_tree_loss_dense(c.handle, c.zd, t.to(DEV), W_XENT, TSW, smoothing=eps)
        _check("soft", loss.item(), gz.cpu().numpy(), *R.soft_loss(c.flat, c.z, t.numpy(), eps, W_XENT, TSW),
               f"{name} dense eps={eps}")


@pytest.mark.parametrize("name", ALL)
def test_soft_backward(name, shapes_dir):
    c = _case(name, shapes_dir)
    gP = torch.randn(B, c.C, generator=torch.Generator().manual_seed(c.C + 1))
    gz = _C.soft_backward(c.handle, c.zd, gP.to(DEV)).cpu().numpy()
    want = O.rules_backward(c.otree, c.z, gP.numpy(), outs=c.outs, P=c.P)
    print(f"{name}: rules backward max abs err {np.abs(gz - want).max():.2e}")
    np.testing.assert_allclose(gz, want, atol=2e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------
# one shape per waves-per-sample choice: dtypes, row stride, batch independence, tree statistics

def _every_entry_point(c, z, y, t, gP):
    """Every output of every per-sample entry point on logits z (any dtype / row stride), as a flat list of tensors."""
    w_node = TSW * TSW * 2.0 / c.N
    out = list(_C.node_outputs(c.handle, z))
    out.append(_C.soft_forward(c.handle, z))
    pred, onehot, dec = _C.hard_forward(c.handle, z, want_onehot=True, want_decisions=True)
    out += [pred, onehot, *dec]
    out.append(_C.soft_backward(c.handle, z, gP))
    out += _C.soft_tree_loss(c.handle, z, y, W_XENT, TSW)
    out += _C.soft_tree_loss(c.handle, z, y, W_XENT, TSW, smoothing=0.1)
    out += _C.soft_tree_loss_dense(c.handle, z, t, W_XENT, TSW)
    out += _C.hard_tree_loss(c.handle, z, y, W_XENT, w_node)
    out += _C.hard_tree_loss(c.handle, z, y, W_XENT, w_node, smoothing=0.1)
    return out


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: output {i}"
        if a.dim() == 0:
            assert a.item() == b.item(), f"{what}: output {i}"


def _side_inputs(c):
    gP = torch.randn(B, c.C, generator=torch.Generator().manual_seed(c.C + 2)).to(DEV)
    return dense_targets(B, c.C).to(DEV), gP


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", THREE)
def test_half_precision_logits_are_the_fp32_launch_on_the_up_cast_values(name, dtype, shapes_dir):
    c = _case(name, shapes_dir)
    t, gP = _side_inputs(c)
    zl = c.zd.to(dtype)
    assert not torch.equal(zl.float(), c.zd)                      # the rounding is visible, so the load is exercised
    _same_bits(_every_entry_point(c, zl, c.yd, t, gP), _every_entry_point(c, zl.float(), c.yd, t, gP), f"{name} {dtype}")


@pytest.mark.parametrize("name", THREE)
def test_row_stride_above_the_class_count(name, shapes_dir):
    c = _case(name, shapes_dir)
    t, gP = _side_inputs(c)
    wide = torch.full((B, c.C + 7), 1e6, device=DEV)              # what lies behind a row would be seen at once
    wide[:, :c.C] = c.zd
    view = wide[:, :c.C]
    assert view.stride(0) == c.C + 7 and not view.is_contiguous()
    _same_bits(_every_entry_point(c, view, c.yd, t, gP), _every_entry_point(c, view.contiguous(), c.yd, t, gP), name)


@pytest.mark.parametrize("name", THREE)
def test_rows_do_not_depend_on_the_batch(name, shapes_dir):
    c = _case(name, shapes_dir)
    w_node = 2.0 / c.N
    z, y = inputs(name, 7, c.C)
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    gP = torch.randn(7, c.C, generator=torch.Generator().manual_seed(c.C + 3)).to(DEV)

    def launch(n):
        loss, gz = _C.hard_tree_loss(c.handle, zd[:n], yd[:n], 1.0, w_node, grad_scale=float(n))     # scale = n / n = 1
        _, _, dec = _C.hard_forward(c.handle, zd[:n], want_onehot=False, want_decisions=True)
        rows = [gz, *_C.node_outputs(c.handle, zd[:n]), *dec, _C.soft_backward(c.handle, zd[:n], gP[:n])]
        return loss.item(), rows

    _, full = launch(7)
    for n in (1, 5, 7):
        loss, rows = launch(n)
        lo, dzo = O.hard_tree_sup_loss(c.otree, z[:n], y[:n])
        assert abs(loss - lo) <= 1e-5 * abs(lo), (name, n)
        np.testing.assert_allclose(rows[0].cpu().numpy() / n, dzo, atol=1e-6, rtol=1e-5)
        for i, (a, b) in enumerate(zip(rows, full)):
            assert torch.equal(a, b[:n]), f"{name} B={n}: output {i}"


def _struct(otree):
    """The maps tests/test_diagnostics.restate reads, from an OracleTree (golden_structure builds them from a golden file)."""
    cls = {w: i for i, w in enumerate(otree.wnids_leaves)}
    nxt = [[otree.inode_index[w] if w in otree.inode_index else -cls[w] - 1 for w in ch] for ch in otree.children]
    return {"wnids": otree.inode_wnids, "root": otree.root, "sets": [[set(k) for k in per] for per in otree.child_classes],
            "next": nxt, "C": otree.num_classes}


STATS_B = 70


def stats_inputs(name, C):
    """Seed chosen on the CPU so that the oracle's own P has no row with a top-2 gap below 1e-4 on any of the three
    shapes (seeds 1-11 counted: 1, 3, 4, 7 and 9 have none)."""
    z = S.logits_for(name, STATS_B, C, seed=3).numpy()
    y = torch.randint(0, C, (STATS_B,), generator=torch.Generator().manual_seed(111)).numpy()
    y[::9] = z.argmax(1)[::9]                    # some backbone hits, so that every counter moves
    return z, y


@pytest.mark.parametrize("name", THREE)
def test_tree_statistics(name, shapes_dir):
    """tests/test_diagnostics_gpu.test_larger_batch_equals_the_oracle's route on a synthetic hierarchy."""
    c = _case(name, shapes_dir)
    struct = _struct(c.otree)
    z, y = stats_inputs(name, c.C)
    outs = O.node_outputs(c.otree, z)
    preds = np.stack([o["preds"] for o in outs], 1)
    ent = np.stack([o["entropy"] for o in outs], 1)
    hard, P = O.hard_forward(c.otree, z, outs), O.soft_forward(c.otree, z, outs)
    skipped = int((~soft_gap_rows(P)).sum())
    assert skipped <= STATS_B // 1000

    def want_of(rows):
        return restate(struct, z[rows], y[rows], preds[rows], ent[rows], hard[rows], P[rows])
    got = _check_against(c.handle, want_of, z, y, ent, P, skipped)
    assert got["totals"][0] == STATS_B and got["totals"][1] >= STATS_B // 9


# ------------------------------------------------------------------------------------------------------------
# the fused head: unstaged at 4 waves, the largest staged row at one wave, a 300-wide node

@pytest.fixture
def deterministic_mode(request):
    ops.set_deterministic(request.param)
    yield request.param
    ops.set_deterministic(False)


@pytest.mark.parametrize("batch,deterministic_mode", [(5, False), (9, False), (9, True)], indirect=["deterministic_mode"])
@pytest.mark.parametrize("name,K", [("cat200", 64), ("cat33", 4096), ("star300", 640)])
def test_fused_head_equals_linear_then_loss_then_linear_backward(name, K, batch, deterministic_mode, shapes_dir):
    """As tests/test_rules_gpu.py::test_fused_head_equals_linear_then_loss_then_linear_backward compares them.  The bias of
    a caterpillar carries the ramp of _tree_shapes.logits_for, so the deep path products stay normal numbers."""
    c = _case(name, shapes_dir)
    handle, C = c.handle, c.C
    staged = S.head_launch(S.describe(c.flat), K)
    assert staged == {"cat200": (4, False), "cat33": (8, True), "star300": (4, True)}[name]
    g = torch.Generator().manual_seed(batch + K)
    pooled = torch.rand(batch, K, generator=g).mul_(2.0).to(DEV)
    W = torch.randn(C, K, generator=g).mul_(K ** -0.5).to(DEV)
    bias = torch.randn(C, generator=g).mul_(0.1)
    if S.SHAPES[name][0] == "caterpillar":
        bias += S.RAMP * torch.arange(C, dtype=torch.float32) / C
    bias = bias.to(DEV)
    y = torch.randint(0, C, (batch,), generator=g).to(DEV)
    for wx, wt in ((1.0, 1.0), (0.5, 10.0)):
        gW, gb = torch.zeros_like(W), torch.zeros_like(bias)
        loss, gp, z = _C.head_soft_tree_loss(handle, pooled, W, bias, y, wx, wt, gW=gW, gb=gb, want_logits=True)
        z_ref = torch.empty(batch, C, device=DEV)
        ops.linear_fwd(pooled, W, bias, z_ref)
        loss_ref, gz_ref = _C.soft_tree_loss(handle, z_ref, y, wx, wt)
        gp_ref, gW_ref, gb_ref = torch.empty_like(pooled), torch.zeros_like(W), torch.zeros_like(bias)
        ops.linear_bwd(pooled, W, gz_ref, gp_ref, gW_ref, gb_ref)
        scale = z_ref.abs().max().item()
        if C < 64:
            assert torch.equal(z, z_ref)
            assert torch.equal(gp, gp_ref)
            assert loss.item() == loss_ref.item()
        else:
            assert (z - z_ref).abs().max().item() < 1e-5 * scale
            assert (gp - gp_ref).abs().max().item() < 1e-5 * gp_ref.abs().max().item() + 1e-9
            assert abs(loss.item() - loss_ref.item()) < 1e-5 * abs(loss_ref.item())
        assert (gW - gW_ref).abs().max().item() < 2e-5 * gW_ref.abs().max().item() + 1e-9
        assert (gb - gb_ref).abs().max().item() < 2e-5 * gb_ref.abs().max().item() + 1e-9
        zn = z.cpu().numpy()
        lo, dzo = O.soft_tree_sup_loss(c.otree, zn, y.cpu().numpy(), wx, wt)
        assert abs(loss.item() - lo) < 1e-5 * abs(lo)
        gp_oracle = torch.from_numpy(dzo).to(DEV) @ W
        assert (gp - gp_oracle).abs().max().item() < 1e-5 * gp_oracle.abs().max().item() + 1e-8
        pred = _C.hard_forward(handle, z, want_onehot=False)[0].cpu().numpy()
        assert np.array_equal(pred, O.hard_forward(c.otree, zn))
        assert O.soft_forward(c.otree, zn).min() >= 1e-30
    gW2 = gW.clone()
    loss2, gp2, z2 = _C.head_soft_tree_loss(handle, pooled, W, bias, y, 0.5, 10.0, gW=gW2, want_gpooled=False)
    assert gp2 is None and z2 is None and loss2.item() == loss.item()
    assert (gW2 - 2 * gW).abs().max().item() < 1e-5 * gW.abs().max().item() + 1e-9
