"""Label smoothing and probability targets, the parts that need no GPU: the float64 restatement the GPU tests lean on
agrees with the reference's goldens (tests/golden/soft_targets_*.npz, recorded by make_soft_target_golden.py), the
fusable-criterion helper, the header's new symbols and the host-side argument checks of their entries."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_path
from conftest import GOLDEN_CASES
from nbdt import _C
from nbdt import loss as L
from nbdt.tree import Tree

import _soft_target_ref as R

TAGS = ("cifar10_wrn", "cifar100_wordnet", "tiny_r18", "imagenet_eff")
W_XENT, TSW = 0.5, 10.0          # the weights the goldens were recorded with


def golden_case(tag, golden_dir):
    """(FlatTree, z [8,C], y [8], golden arrays, the four cases as name -> (kind, target, eps))."""
    ds, h = GOLDEN_CASES[tag]
    g = np.load(os.path.join(golden_dir, f"soft_targets_{tag}.npz"))
    src = np.load(os.path.join(golden_dir, f"rules_{tag}.npz"))
    z, y = src["z"][:8], src["y"][:8]
    onehot = np.eye(z.shape[1], dtype=np.float32)[y]
    t_mix = np.float32(0.3) * onehot + np.float32(0.7) * np.roll(onehot, 1, 0)
    cases = {"a": ("soft", y, 0.1), "b": ("soft", t_mix, 0.0), "c": ("soft", g["t_dir"], 0.1), "d": ("hard", y, 0.1)}
    return Tree(ds, hierarchy=h), z, y, g, cases


def reference_loss(flat, z, kind, target, eps):
    if kind == "soft":
        return R.soft_loss(flat, z, target, eps, W_XENT, TSW)
    return R.hard_loss(flat, z, target, eps, W_XENT, TSW * TSW * 2.0 / flat.num_inodes)


@pytest.mark.parametrize("case", "abcd")
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_agrees_with_the_reference(tag, case, golden_dir):
    """The float64 restatement against the reference's float64 result (the goldens are recorded and stored in float64:
    dL/dz reaches 2.7, where fp32 cannot carry 1e-7): loss 1e-6 relative, dL/dz 1e-7 absolute."""
    tree, z, _, g, cases = golden_case(tag, golden_dir)
    kind, target, eps = cases[case]
    assert abs(float(g["eps"]) - 0.1) < 1e-7
    assert g["dz_" + case].dtype == np.float64 and g["loss_" + case].dtype == np.float64
    loss, dz = reference_loss(tree.flat, z, kind, target, eps)
    ref_loss, ref_dz = float(g["loss_" + case]), g["dz_" + case]
    print(f"{tag} {case}: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e}, dz abs {np.abs(dz - ref_dz).max():.2e}")
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss)
    np.testing.assert_allclose(dz, ref_dz, atol=1e-7, rtol=0)


def test_goldens_are_small_and_row_three_is_not_normalised(golden_dir):
    limit = os.path.getsize(os.path.join(golden_dir, "rules_imagenet_eff.npz"))
    for tag in TAGS:
        path = os.path.join(golden_dir, f"soft_targets_{tag}.npz")
        assert os.path.getsize(path) < limit
        sums = np.load(path)["t_dir"].sum(1)
        assert abs(sums[3] - 0.5) < 1e-5 and np.allclose(np.delete(sums, 3), 1.0, atol=1e-5)


class _MyCE(nn.CrossEntropyLoss):
    pass


@pytest.mark.parametrize("criterion,expect", [
    (nn.CrossEntropyLoss(), 0.0),
    (nn.CrossEntropyLoss(label_smoothing=0.1), 0.1),
    (nn.CrossEntropyLoss(label_smoothing=0.999), 0.999),
    (nn.CrossEntropyLoss(label_smoothing=1.0), None),
    (nn.CrossEntropyLoss(weight=torch.ones(10)), None),
    (nn.CrossEntropyLoss(reduction="sum"), None),
    (nn.CrossEntropyLoss(reduction="none", label_smoothing=0.1), None),
    (nn.CrossEntropyLoss(ignore_index=3), None),
    (_MyCE(), None),
    (nn.NLLLoss(), None),
    (nn.MSELoss(), None),
])
def test_fusable_smoothing(criterion, expect):
    got = L._fusable_smoothing(criterion)
    assert got is None if expect is None else got == pytest.approx(expect, abs=0)
    # the fused classifier head keeps its own, narrower test
    assert L._is_plain_cross_entropy(criterion) == (expect == 0.0)
    if expect is None:
        with pytest.raises(_C.NBDTHipError, match="fused tree loss cannot apply"):
            L._require_fusable(criterion, "loss_and_grad")


def test_loss_and_grad_refuses_a_criterion_it_cannot_apply():
    """Until now loss_and_grad computed plain cross entropy whatever was wrapped; the refusal comes before any device
    work, so it shows without a GPU."""
    tree = Tree("CIFAR10", hierarchy="induced-wrn28_10_cifar10")
    z, y = torch.zeros(2, 10), torch.zeros(2, dtype=torch.long)
    for cls in (L.SoftTreeSupLoss, L.HardTreeSupLoss, L.SoftTreeLoss):
        crit = cls(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(weight=torch.ones(10)), tree=tree)
        with pytest.raises(_C.NBDTHipError, match="class weights"):
            crit.loss_and_grad(z, y)
        if cls is not L.HardTreeSupLoss:
            with pytest.raises(_C.NBDTHipError, match="class weights"):
                crit.soft_target_loss_and_grad(z, torch.zeros(2, 10))
    assert not hasattr(L.HardTreeSupLoss, "soft_target_loss_and_grad")


def test_header_declares_the_new_symbols():
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("nbdt_soft_tree_loss_ex", "nbdt_hard_tree_loss_ex", "nbdt_mix_batch"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _C.SIGNATURES
    assert _C.lib().nbdt_version() >= 116
    # the existing entries keep their signatures
    assert len(_C.SIGNATURES["nbdt_soft_tree_loss"][1]) == 13 and len(_C.SIGNATURES["nbdt_hard_tree_loss"][1]) == 13


def test_loss_entries_check_their_arguments_before_any_hip_call():
    lib = _C.lib()
    assert lib.nbdt_soft_tree_loss_ex(None, None, 0, 4, 10, None, None, 0, 0.0, 1.0, 1.0, 1.0, None, None, None, None) == -1
    assert b"null tree handle" in lib.nbdt_last_error()
    assert lib.nbdt_hard_tree_loss_ex(None, None, 0, 4, 10, None, 0.0, 1.0, 1.0, 1.0, None, None, None, None) == -1
    assert b"null tree handle" in lib.nbdt_last_error()


spec = importlib.util.spec_from_file_location("nbdt_main_soft", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)


def test_main_flags():
    args = M.parse_args([])
    assert (args.label_smoothing, args.mixup_alpha, args.cutmix_alpha) == (0.0, 0.0, 0.0)
    args = M.parse_args(["--label-smoothing", "0.1", "--mixup-alpha", "0.2", "--cutmix-alpha", "1.0", "--loss",
                         "SoftTreeSupLoss"])
    assert (args.label_smoothing, args.mixup_alpha, args.cutmix_alpha) == (0.1, 0.2, 1.0)
    assert M.parse_args(["--mixup-alpha", "0.2"]).loss == ["CrossEntropyLoss"]          # plain cross entropy mixes too
    assert M.parse_args(["--cutmix-alpha", "1", "--loss", "SoftTreeLoss"]).cutmix_alpha == 1.0
    assert M.parse_args(["--label-smoothing", "0.1", "--loss", "HardTreeSupLoss"]).label_smoothing == 0.1
    with pytest.raises(SystemExit, match="HardTreeSupLoss"):
        M.parse_args(["--mixup-alpha", "0.2", "--loss", "HardTreeSupLoss"])
    with pytest.raises(SystemExit, match="HardTreeSupLoss"):
        M.main(["--mixup-alpha", "0.2", "--loss", "HardTreeSupLoss"])      # before the device is touched
    with pytest.raises(SystemExit):
        M.parse_args(["--label-smoothing", "1.0"])


def test_main_builds_the_smoothed_criterion():
    args = M.parse_args(["--label-smoothing", "0.1", "--loss", "SoftTreeSupLoss", "--hierarchy", "induced-ResNet18"])
    tree = Tree("CIFAR10", hierarchy="induced-ResNet18")
    crit = M.build_criterion(args, tree)
    assert isinstance(crit, L.SoftTreeSupLoss) and crit.criterion.label_smoothing == 0.1
    assert not crit.can_fuse_head(10)            # a smoothed criterion keeps the unfused head
    plain = M.build_criterion(M.parse_args(["--label-smoothing", "0.2"]), tree)
    assert type(plain) is nn.CrossEntropyLoss and plain.label_smoothing == 0.2
    assert M._PlainCE(tree, 0.2).inner.criterion.label_smoothing == 0.2
