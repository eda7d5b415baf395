"""Label smoothing and probability targets in the fused tree losses on the MI355X (nbdt_soft_tree_loss_ex,
nbdt_hard_tree_loss_ex), against the reference's goldens (tests/golden/soft_targets_*.npz), the float64 restatement
(tests/_soft_target_ref.py) and the existing class-index kernel.  Tolerances are test_rules_gpu.py::test_golden_inputs':
loss 1e-5 relative, soft dL/dz 1e-6 absolute, hard dL/dz atol 2e-6 + rtol 1e-5."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN_CASES
from test_soft_targets import TAGS, TSW, W_XENT, golden_case, reference_loss

pytestmark = pytest.mark.gpu

from nbdt import _C  # noqa: E402
from nbdt import engine as E  # noqa: E402
from nbdt.loss import HardTreeSupLoss, SoftTreeLoss, SoftTreeSupLoss  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"


def _launch(handle, z, kind, target, eps, n_inodes, grad_scale=1.0):
    """One case through the ctypes layer: (loss float, dL/dz numpy)."""
    t = torch.as_tensor(target).to(DEV)
    if kind == "hard":
        loss, gz = _C.hard_tree_loss(handle, z, t, W_XENT, TSW * TSW * 2.0 / n_inodes, grad_scale, smoothing=eps)
    elif t.is_floating_point():
        loss, gz = _C.soft_tree_loss_dense(handle, z, t, W_XENT, TSW, grad_scale, smoothing=eps)
    else:
        loss, gz = _C.soft_tree_loss(handle, z, t, W_XENT, TSW, grad_scale, smoothing=eps)
    return loss.item(), gz.cpu().numpy()


def _check(kind, loss, gz, ref_loss, ref_dz, what):
    print(f"{what}: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e}, dz abs {np.abs(gz - ref_dz).max():.2e}")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), what
    if kind == "hard":
        np.testing.assert_allclose(gz, ref_dz, atol=2e-6, rtol=1e-5, err_msg=what)
    else:
        np.testing.assert_allclose(gz, ref_dz, atol=1e-6, rtol=0, err_msg=what)


@pytest.mark.parametrize("tag", TAGS)
def test_goldens(tag, golden_dir):
    """Cases a-d through _C.* and through the nn.Module's forward + backward, then the first 7 rows (a ragged last block)
    and the first row alone: dL/dz is the recorded rows times 8/B, the loss is the restatement's."""
    tree, z_np, _, g, cases = golden_case(tag, golden_dir)
    handle = tree.device_handle(0)
    N = len(tree.inodes)
    ds = GOLDEN_CASES[tag][0]
    z = torch.from_numpy(z_np).to(DEV)
    for name, (kind, target, eps) in cases.items():
        loss, gz = _launch(handle, z, kind, target, eps, N)
        _check(kind, loss, gz, float(g["loss_" + name]), g["dz_" + name], f"{tag} {name} _C")

        cls = HardTreeSupLoss if kind == "hard" else SoftTreeSupLoss
        crit = cls(dataset=ds, criterion=nn.CrossEntropyLoss(label_smoothing=eps), tree=tree,
                   tree_supervision_weight=TSW, xent_weight=W_XENT)
        zz = z.clone().requires_grad_(True)
        lm = crit(zz, torch.as_tensor(target).to(DEV))
        lm.backward()
        _check(kind, lm.item(), zz.grad.cpu().numpy(), float(g["loss_" + name]), g["dz_" + name], f"{tag} {name} module")
        lf, gf = crit.loss_and_grad(z, torch.as_tensor(target).to(DEV)) if np.asarray(target).ndim == 1 else \
            crit.soft_target_loss_and_grad(z, torch.as_tensor(target).to(DEV))
        assert lf.item() == loss and np.array_equal(gf.cpu().numpy(), gz)          # the same launch

        for B in (7, 1):
            loss_b, gz_b = _launch(handle, z[:B], kind, target[:B], eps, N)
            ref_loss, _ = reference_loss(tree.flat, z_np[:B], kind, target[:B], eps)
            _check(kind, loss_b, gz_b, ref_loss, g["dz_" + name][:B] * (8.0 / B), f"{tag} {name} B={B}")


@pytest.mark.parametrize("case", "ac")
def test_bf16_logits_are_the_fp32_launch_on_the_rounded_values(case, golden_dir):
    tree, z_np, _, _, cases = golden_case("cifar100_wordnet", golden_dir)
    handle = tree.device_handle(0)
    kind, target, eps = cases[case]
    zb = torch.from_numpy(z_np).to(DEV).bfloat16()
    lb, gb = _launch(handle, zb, kind, target, eps, len(tree.inodes))
    lf, gf = _launch(handle, zb.float(), kind, target, eps, len(tree.inodes))
    assert lb == lf and np.array_equal(gb, gf)
    assert torch.equal(torch.from_numpy(gb), torch.from_numpy(gf))


@pytest.mark.parametrize("tag", TAGS)
def test_one_hot_rows_give_the_index_launch(tag, golden_dir):
    """Dense one-hot rows without smoothing: T = 1 and every sum has one non-zero term, so the arithmetic allows the
    bits of the class-index kernel; asserted at its tolerances, the bit comparison is printed."""
    tree, z_np, y_np, _, _ = golden_case(tag, golden_dir)
    handle = tree.device_handle(0)
    z, y = torch.from_numpy(z_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    li, gi = _C.soft_tree_loss(handle, z, y, W_XENT, TSW)
    onehot = torch.nn.functional.one_hot(y, z.shape[1]).float()
    ld, gd = _C.soft_tree_loss_dense(handle, z, onehot, W_XENT, TSW)
    print(f"{tag}: one-hot dense vs index: loss bit-identical {li.item() == ld.item()}, "
          f"dL/dz bit-identical {torch.equal(gi, gd)}, max abs {(gi - gd).abs().max().item():.2e}")
    assert abs(li.item() - ld.item()) <= 1e-5 * abs(li.item())
    np.testing.assert_allclose(gd.cpu().numpy(), gi.cpu().numpy(), atol=1e-6, rtol=0)
    # a padded row stride (a column slice of a wider buffer) is the same launch
    wide = torch.zeros(z.shape[0], z.shape[1] + 3, device=DEV)
    wide[:, :z.shape[1]] = onehot
    lw, gw = _C.soft_tree_loss_dense(handle, z, wide[:, :z.shape[1]], W_XENT, TSW)
    assert lw.item() == ld.item() and torch.equal(gw, gd)


def test_mixed_targets_are_linear_in_the_target_row(golden_dir):
    """Case b at B = 130 on the 1000-class hierarchy (several blocks, a ragged last one): the loss and its gradient are
    linear in the target row, so they equal 0.3*L(y) + 0.7*L(roll(y)) from two class-index launches."""
    tree = Tree(*[GOLDEN_CASES["imagenet_eff"][0]], hierarchy=GOLDEN_CASES["imagenet_eff"][1])
    handle = tree.device_handle(0)
    g = torch.Generator().manual_seed(130)
    z = (torch.randn(130, 1000, generator=g) * 3).to(DEV)
    y = torch.randint(0, 1000, (130,), generator=g).to(DEV)
    onehot = torch.nn.functional.one_hot(y, 1000).float()
    t_mix = 0.3 * onehot + 0.7 * onehot.roll(1, 0)
    lm, gm = _C.soft_tree_loss_dense(handle, z, t_mix, W_XENT, TSW)
    l1, g1 = _C.soft_tree_loss(handle, z, y, W_XENT, TSW)
    l2, g2 = _C.soft_tree_loss(handle, z, y.roll(1, 0), W_XENT, TSW)
    want = 0.3 * l1.double().item() + 0.7 * l2.double().item()
    assert abs(lm.item() - want) <= 1e-5 * abs(want)
    np.testing.assert_allclose(gm.cpu().numpy(), (0.3 * g1.double() + 0.7 * g2.double()).cpu().numpy(), atol=1e-6, rtol=0)


def test_refusals(golden_dir):
    tree, z_np, y_np, _, _ = golden_case("cifar10_wrn", golden_dir)
    handle = tree.device_handle(0)
    z, y = torch.from_numpy(z_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    onehot = torch.nn.functional.one_hot(y, 10).float()
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(label_smoothing=0.1), tree=tree)
    with pytest.raises(_C.NBDTHipError, match="class-index"):
        crit.loss_and_grad(z, onehot)
    with pytest.raises(_C.NBDTHipError, match="class-index"):
        _C.hard_tree_loss(handle, z, onehot, 1.0, 1.0, smoothing=0.1)
    # exactly one of y / tprob
    lib = _C.lib()
    row, loss, gz = torch.empty(8, device=DEV), torch.empty((), device=DEV), torch.empty(8, 10, device=DEV)
    args = lambda yy, tt: (handle.h, _C.ptr(z), _C.NBDT_F32, 8, 10, _C.ptr(yy), _C.ptr(tt), 10, 0.0, 1.0, 1.0, 1.0,
                           _C.ptr(row), _C.ptr(loss), _C.ptr(gz), _C.stream_of(z))
    for yy, tt in ((y, onehot), (None, None)):
        assert lib.nbdt_soft_tree_loss_ex(*args(yy, tt)) == -1
        assert b"exactly one" in lib.nbdt_last_error()
    bad = list(args(None, onehot))
    bad[7] = 9                                                      # row stride below C
    assert lib.nbdt_soft_tree_loss_ex(*bad) == -1 and b"stride" in lib.nbdt_last_error()
    bad = list(args(y, None))
    bad[8] = 1.0                                                    # smoothing outside [0, 1)
    assert lib.nbdt_soft_tree_loss_ex(*bad) == -1 and b"smoothing" in lib.nbdt_last_error()
    # wrong shape / dtype / device / layout of the probability targets
    for t in (onehot[:, :9], onehot[:7], onehot.double(), onehot.half(), y, onehot.cpu(), onehot.t().contiguous().t(),
              onehot.flatten()):
        with pytest.raises(_C.NBDTHipError, match="probability targets"):
            _C.soft_tree_loss_dense(handle, z, t, 1.0, 1.0)
    # a criterion the kernels do not implement
    for cls in (SoftTreeSupLoss, HardTreeSupLoss, SoftTreeLoss):
        weird = cls(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(reduction="sum"), tree=tree)
        with pytest.raises(_C.NBDTHipError, match="reduction"):
            weird.loss_and_grad(z, y)
    # an out-of-range class index is still a loud NaN, smoothed or not, and forms no address
    y_bad = y.clone()
    y_bad[2] = 10
    for eps in (0.0, 0.1):
        assert torch.isnan(_C.soft_tree_loss(handle, z, y_bad, 1.0, 1.0, smoothing=eps)[0])
        assert torch.isnan(_C.hard_tree_loss(handle, z, y_bad, 1.0, 1.0, smoothing=eps)[0])
    y_bad[2] = -1
    assert torch.isnan(_C.soft_tree_loss(handle, z, y_bad, 1.0, 1.0, smoothing=0.1)[0])


def test_soft_tree_loss_before_the_tree_starts(golden_dir):
    """SoftTreeLoss before tree_start_epochs: both weights on the cross-entropy term, for probability targets too."""
    tree, z_np, y_np, g, cases = golden_case("cifar10_wrn", golden_dir)
    z = torch.from_numpy(z_np).to(DEV)
    t = torch.from_numpy(g["t_dir"]).to(DEV)
    crit = SoftTreeLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(label_smoothing=0.1), tree=tree,
                        tree_supervision_weight=TSW, xent_weight=W_XENT, tree_start_epochs=5)
    crit.set_epoch(0, 10)
    loss, gz = crit.soft_target_loss_and_grad(z, t)
    want = (W_XENT + TSW) * nn.CrossEntropyLoss(label_smoothing=0.1)(z.double().cpu(), t.double().cpu()).item()
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    ref_loss, ref_dz = reference_loss(tree.flat, z_np, "soft", g["t_dir"], 0.1)
    assert abs(loss.item() - ref_loss) > 1e-3 * abs(ref_loss)            # not the tree loss


@pytest.fixture
def deterministic_mode():
    from nbdt import ops
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


@pytest.mark.parametrize("targets", ["dense", "smoothed-index"])
def test_train_step(targets, deterministic_mode):
    """ResNet18, B = 8, 32 x 32: a step on probability targets (criterion with can_fuse_head true: the fused head must be
    skipped, not fed float targets) and a step on class indices under a smoothed criterion return the loss of the
    unfused loss launch on the twin engine's logits and leave finite, changed parameters."""
    eps = 0.0 if targets == "dense" else 0.1
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(label_smoothing=eps),
                           hierarchy="induced-ResNet18")
    assert crit.can_fuse_head(10) == (targets == "dense")
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, 10, (8,), generator=g).to(DEV)
    if targets == "dense":
        onehot = torch.nn.functional.one_hot(y, 10).float()
        t = 0.6 * onehot + 0.4 * onehot.roll(1, 0)
    else:
        t = y
    eng, twin = (E.ResNetEngine(num_classes=10, device=DEV, seed=4) for _ in range(2))
    before = eng.store.flat.clone()
    assert torch.equal(before, twin.store.flat)
    loss = E.train_step(eng, crit, x, t, lr=0.05)
    z = twin.forward(x, training=True)
    want = (crit.soft_target_loss_and_grad(z, t) if targets == "dense" else crit.loss_and_grad(z, t))[0]
    torch.cuda.synchronize()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    after = eng.store.flat
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    with pytest.raises(ValueError, match="class-index"):
        E.GraphedStep(eng, crit, x, t.float() if targets != "dense" else t, lr=0.05)
