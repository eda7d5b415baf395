"""Segmentation NBDTs, the parts that need no GPU: the restatement the GPU tests lean on reproduces the reference's
goldens (tests/golden/seg_*.npz), the layout dispatch is a pure host function, and the constructors, flags and names
behave like the reference's."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_path
from nbdt import _C
from nbdt import loss as L
from nbdt import model as M
from nbdt.tree import Tree
from nbdt.utils import DATASETS, DATASET_TO_NUM_CLASSES

import _seg_ref as S
import _tree_shapes as T

TAGS = tuple(S.CASES)


@pytest.mark.parametrize("tag", TAGS)
def test_hierarchy_sizes(tag):
    """The sizes the pixel kernels were laid out for: all three are binary and fit the pixel form."""
    tree, otree, g = S.case(tag)
    flat = tree.flat
    assert (flat.num_classes, flat.num_inodes, flat.num_slots, len(flat.slot_cls)) == S.CASES[tag][2:]
    assert int((flat.node_off[1:] - flat.node_off[:-1]).max()) == 2
    assert _C.seg_pixel_fits(flat)
    assert g["z"].shape == (2, flat.num_classes, 5, 13) and g["z"].dtype == np.float32
    assert (g["y"][0, :2] == 255).all() and (g["y"][1] != 255).sum() == 1 and (g["y_none"] == 255).all()


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(tag):
    """Integers exact; floats within the bounds tests/test_oracle_golden.py uses for the row case: P rtol 2e-5 / atol
    1e-6, loss 1e-5 relative, dL/dz 1e-6 absolute."""
    tree, otree, g = S.case(tag)
    z = g["z"]
    P = S.soft(otree, z)
    assert np.array_equal(S.hard(otree, z), g["hard"])
    assert np.array_equal(P.argmax(1), g["soft"].argmax(1))
    np.testing.assert_allclose(P, g["soft"], rtol=2e-5, atol=1e-6)
    for key, eps in (("a", 0.0), ("b", float(g["eps"]))):
        loss, dz = S.loss(otree, tree.flat, z, g["y"], eps=eps)
        ref_loss, ref_dz = float(g["loss_" + key]), g["dz_" + key]
        print(f"{tag} {key}: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e}, dz abs {np.abs(dz - ref_dz).max():.2e}")
        assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
        np.testing.assert_allclose(dz, ref_dz, atol=1e-6, rtol=0)
        assert (dz[0, :, :2] == 0).all() and np.count_nonzero(np.abs(dz[1]).sum(0)) == 1
    loss, dz = S.loss(otree, tree.flat, z, g["y_none"])
    assert np.isnan(loss) and np.isnan(g["loss_none"])          # torch's mean over no pixel
    assert not dz.any() and not g["dz_none"].any()


def test_goldens_are_small():
    total = 0
    for name in os.listdir(os.path.join(S.GOLDEN, "seg_hierarchies")):
        total += os.path.getsize(os.path.join(S.GOLDEN, "seg_hierarchies", name))
    assert total < 64 * 1024
    for tag in TAGS:
        assert os.path.getsize(os.path.join(S.GOLDEN, f"seg_{tag}.npz")) < 512 * 1024


# ------------------------------------------------------------------------------------------------ dispatch

def _strides(t):
    return tuple(t.shape), tuple(t.stride())


def test_dispatch_is_a_function_of_layout():
    flat = S.case("lip")[0].flat
    C = flat.num_classes
    z = torch.zeros(2, C, 5, 13)
    f = lambda t, dtype=torch.float32: M.seg_dispatch(*_strides(t), dtype, flat)
    assert f(z) == "pixel"
    assert f(z.to(memory_format=torch.channels_last)) == "rows"
    assert f(z.transpose(2, 3).contiguous().transpose(2, 3)) == "contiguous"          # W is not the fastest axis
    assert f(torch.zeros(2, C + 3, 5, 13)[:, 1:C + 1]) == "pixel"                    # channel stride of the wider tensor
    assert f(torch.zeros(3, C, 1, 1)) == "pixel"
    assert f(torch.zeros(2, C, 5, 26)[:, :, :, ::2]) == "contiguous"
    assert f(z, torch.bfloat16) == "pixel" and f(z, torch.float16) == "pixel"
    with pytest.raises(_C.NBDTHipError, match="dtype"):
        f(z, torch.float64)
    with pytest.raises(_C.NBDTHipError, match="channels"):
        f(torch.zeros(2, C + 1, 5, 13))
    with pytest.raises(_C.NBDTHipError, match=r"\[N, C, H, W\]"):
        M.seg_dispatch((4, C), (C, 1), torch.float32, flat)


def test_dispatch_beyond_the_pixel_form(tmp_path):
    """R + F <= 640 (include/nbdt_hip.h): a 400-way star has R = F = 400 and takes the row kernels on a coerced copy;
    channels_last memory needs no copy even then."""
    pg, pw, leaves = T.star(tmp_path, 400)
    flat = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat
    assert flat.num_slots == 400 and not _C.seg_pixel_fits(flat)
    z = torch.zeros(1, 400, 2, 3)
    assert M.seg_dispatch(*_strides(z), z.dtype, flat) == "coerced"
    assert M.seg_dispatch(*_strides(z.to(memory_format=torch.channels_last)), z.dtype, flat) == "rows"
    pg, pw, leaves = T.star(tmp_path, 320)
    assert _C.seg_pixel_fits(Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat)      # 320 + 320 = 640
    pg, pw, leaves = T.star(tmp_path, 321)
    assert not _C.seg_pixel_fits(Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat)


# ------------------------------------------------------------------------------------------------ surface

def _kw(tag="lip"):
    pg, pw = S.paths(tag)
    return dict(dataset=S.CASES[tag][0], path_graph=pg, path_wnids=pw)


def test_names_and_datasets():
    assert "SoftSegTreeSupLoss" in L.names and "SoftSegTreeSupLoss" in L.__all__
    assert issubclass(L.SoftSegTreeSupLoss, L.SoftTreeSupLoss)
    assert issubclass(M.HardSegNBDT, M.SegNBDT) and issubclass(M.SoftSegNBDT, M.SegNBDT) and issubclass(M.SegNBDT, M.NBDT)
    for name, classes in (("LookIntoPerson", 20), ("PascalContext", 59), ("ADE20K", 150), ("Cityscapes", 19)):
        assert name in DATASETS and DATASET_TO_NUM_CLASSES[name] == classes


def test_missing_default_files_say_what_to_pass():
    with pytest.raises(FileNotFoundError, match="ships no graph or wnid files.*path_graph="):
        Tree("Cityscapes")
    pg, _ = S.paths("lip")
    with pytest.raises(FileNotFoundError, match="path_wnids="):
        Tree("Cityscapes", path_graph=pg)


def test_constructors_follow_the_reference():
    net = nn.Conv2d(3, 20, 1)
    for cls, rules in ((M.HardSegNBDT, M.HardEmbeddedDecisionRules), (M.SoftSegNBDT, M.SoftEmbeddedDecisionRules)):
        net.train()
        m = cls(model=net, **_kw())
        assert type(m.rules) is rules and not m.training and not net.training            # eval-on-init
        assert set(m.state_dict()) == set(net.state_dict())                              # proxied to the backbone
        m.load_state_dict({"net": {"module." + k: v for k, v in net.state_dict().items()}})
        with pytest.raises(AssertionError, match=r"Input must be of shape \(N,C,H,W\) for segmentation"):
            m(torch.zeros(4, 3))
        with pytest.raises(AssertionError, match=r"Input must be of shape \(N,C,H,W\) for segmentation"):
            m.predict(torch.zeros(4, 3))
        with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
            m(torch.zeros(1, 3, 2, 2))


def test_loss_guards_and_weights():
    crit = L.SoftSegTreeSupLoss(criterion=nn.CrossEntropyLoss(ignore_index=255), tree_supervision_weight=10,
                                xent_weight=0.25, xent_weight_end=0.5, tree_supervision_weight_end=3.0, **_kw())
    assert crit.weights() == (1.0, 10.0)
    crit.set_epoch(5, 10)
    assert crit.weights() == (1.0, 10.0)            # reference nbdt/loss.py:318-327 never reads the schedules
    crit.xent_weight = 7.0
    assert crit.weights() == (1.0, 10.0)
    flagged = torch.zeros(1, 20, 2, 2)
    flagged._nbdt_output_flag = True               # what a SegNBDT hands out
    with pytest.raises(AssertionError, match="NBDT wrapper"):
        crit(flagged, torch.zeros(1, 2, 2, dtype=torch.long))
    with pytest.raises(AssertionError, match=r"\(N,C,H,W\)"):
        crit(torch.zeros(4, 20), torch.zeros(4, dtype=torch.long))
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        crit(torch.zeros(1, 20, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))


def test_fusable_criteria():
    assert L._seg_fusable(nn.CrossEntropyLoss()) == (-100, 0.0)
    assert L._seg_fusable(nn.CrossEntropyLoss(ignore_index=255, label_smoothing=0.1)) == (255, 0.1)
    assert L._seg_fusable(nn.CrossEntropyLoss(weight=torch.ones(20))) is None
    assert L._seg_fusable(nn.CrossEntropyLoss(reduction="sum")) is None

    class Ohem(nn.CrossEntropyLoss):
        pass

    assert L._seg_fusable(Ohem()) is None


def test_header_and_binding_agree():
    with open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")) as f:
        header = f.read()
    for name in ("nbdt_seg_soft_forward", "nbdt_seg_soft_backward", "nbdt_seg_soft_tree_loss", "nbdt_seg_hard_forward",
                 "nbdt_seg_pixel_fits", "nbdt_seg_loss_workspace_floats"):
        assert re.search(r"\b" + name + r"\(", header) and name in _C.SIGNATURES
    assert "R + F <= 640" in header and _C.SEG_PIXEL_MAX_ROWS == 640
