"""Segmentation NBDTs on the GPU: the pixel kernels (csrc/rules_pixel.h) against the reference's goldens and against
the row kernels on the coerced tensor.  Bounds are the ones tests/test_rules_gpu.py / test_soft_targets_gpu.py apply to
the row kernels against their goldens: P rtol 2e-5 / atol 1e-6, loss 1e-5 relative, dL/dz 1e-6 absolute."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from nbdt import _C
from nbdt import loss as L
from nbdt import model as M
from nbdt.tree import Tree

import _seg_ref as S
import _tree_shapes as T

pytestmark = pytest.mark.gpu

TAGS = tuple(S.CASES)
DEV = "cuda:0"


def coerce(x):
    """[N, C, H, W] -> contiguous [N*H*W, C] rows: the reference's coerce_tensor, the input of the row kernels."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def uncoerce(rows, shape):
    N, _, H, W = shape
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def close_P(P, ref):
    np.testing.assert_allclose(P.detach().cpu().numpy(), ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref,
                               rtol=2e-5, atol=1e-6)


def close_dz(gz, ref):
    np.testing.assert_allclose(gz.detach().cpu().numpy(), ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref,
                               atol=1e-6, rtol=0)


# ------------------------------------------------------------------------------------ 1. against the goldens

@pytest.mark.parametrize("tag", TAGS)
def test_against_the_reference(tag):
    tree, _, g = S.case(tag)
    handle = tree.device_handle(0)
    z = torch.from_numpy(g["z"]).to(DEV)
    y, y_none = torch.from_numpy(g["y"]).to(DEV), torch.from_numpy(g["y_none"]).to(DEV)

    pred, onehot = _C.seg_hard_forward(handle, z)
    assert _C.last_rules_path() == "pixel"
    assert np.array_equal(pred.cpu().numpy(), g["hard"])
    assert np.array_equal(onehot.argmax(1).cpu().numpy(), g["hard"]) and float(onehot.sum()) == pred.numel()
    P = _C.seg_soft_forward(handle, z)
    assert np.array_equal(P.argmax(1).cpu().numpy(), g["soft"].argmax(1))
    close_P(P, g["soft"])

    for key, eps in (("a", 0.0), ("b", float(g["eps"]))):
        loss, gz = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, S.TSW, smoothing=eps)
        ref_loss, ref_dz = float(g["loss_" + key]), g["dz_" + key]
        print(f"{tag} {key}: loss rel {abs(loss.item() - ref_loss) / abs(ref_loss):.2e}, "
              f"dz abs {np.abs(gz.cpu().numpy() - ref_dz).max():.2e}")
        assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
        close_dz(gz, ref_dz)
        assert not gz[y.unsqueeze(1).expand_as(gz) == S.IGNORE].any()          # exactly 0 at ignored pixels

    loss, gz = _C.seg_soft_tree_loss(handle, z, y_none, S.IGNORE, 1.0, S.TSW)
    assert torch.isnan(loss) and np.isnan(g["loss_none"])
    assert not gz.any() and not g["dz_none"].any()


# ------------------------------------------------------------------------------------ 2. against the row kernels

def _shapes(C, seed):
    """The issue's four inputs: one pixel per image; a wave and a one-pixel tail; several blocks without a tail; a
    channel-sliced view, whose channel stride is that of the wider tensor."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (2.0 * torch.randn(*s, generator=g)).to(DEV)
    return {"one_pixel": r(3, C, 1, 1), "tail": r(2, C, 5, 13), "blocks": r(1, C, 16, 24),
            "sliced": r(2, C + 2, 5, 13)[:, 1:C + 1]}


def _targets(z, C, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (z.shape[0], z.shape[2], z.shape[3]), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.3] = S.IGNORE
    y.view(-1)[0] = 0                                                   # at least one valid pixel
    return y.to(DEV)


def check_against_rows(tree, seed):
    """Pixel kernels == row kernels on coerce_tensor(z): integers bit-equal, P and gz within the golden bounds."""
    handle = tree.device_handle(0)
    C = tree.flat.num_classes
    for name, z in _shapes(C, seed).items():
        rows = coerce(z)
        assert (_C.seg_dispatch(tuple(z.shape), tuple(z.stride()), z.dtype, tree.flat) == "pixel"), name
        pred, onehot = _C.seg_hard_forward(handle, z)
        assert _C.last_rules_path() == "pixel", name
        pred_rows, onehot_rows, _ = _C.hard_forward(handle, rows)
        assert _C.last_rules_path() != "pixel"
        assert torch.equal(pred.view(-1), pred_rows), name
        assert torch.equal(onehot, uncoerce(onehot_rows, z.shape)), name
        assert torch.equal(_C.seg_hard_forward(handle, z, want_onehot=False)[0], pred), name

        P = _C.seg_soft_forward(handle, z)
        assert _C.last_rules_path() == "pixel", name
        P_rows = uncoerce(_C.soft_forward(handle, rows), z.shape)
        assert torch.equal(P.argmax(1), P_rows.argmax(1)), name
        close_P(P, P_rows)

        gP = torch.randn(z.shape, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
        gz = _C.seg_soft_backward(handle, z, gP)
        assert _C.last_rules_path() == "pixel", name
        np.testing.assert_allclose(gz.cpu().numpy(), uncoerce(_C.soft_backward(handle, rows, coerce(gP)), z.shape)
                                   .cpu().numpy(), atol=2e-6, rtol=1e-5, err_msg=name)      # test_rules_gpu.py: dz_rules

        y = _targets(z, C, seed + 2)
        keep = (y.view(-1) != S.IGNORE).nonzero().squeeze(1)
        for eps in (0.0, 0.1):
            loss, gz = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, 2.0, smoothing=eps)
            assert _C.last_rules_path() == "pixel", name
            loss_rows, g_rows = _C.soft_tree_loss(handle, rows[keep], y.view(-1)[keep], 1.0, 2.0, smoothing=eps)
            full = torch.zeros_like(rows)
            full[keep] = g_rows
            assert abs(loss.item() - loss_rows.item()) <= 1e-5 * abs(loss_rows.item()), name
            close_dz(gz, uncoerce(full, z.shape))
            assert not gz[y.unsqueeze(1).expand_as(gz) == S.IGNORE].any(), name


@pytest.mark.parametrize("tag", TAGS)
def test_against_the_row_kernels(tag):
    check_against_rows(S.case(tag)[0], seed=60 + TAGS.index(tag))


@pytest.mark.parametrize("shape", ["star", "caterpillar", "kary3"])
def test_against_the_row_kernels_on_synthetic_hierarchies(shape, tmp_path):
    """One wide node (the generic softmax and F = R rows of T), a deep chain, and fan-out 3 (neither binary path)."""
    pg, pw, leaves = {"star": lambda: T.star(tmp_path, 37), "caterpillar": lambda: T.caterpillar(tmp_path, 24),
                      "kary3": lambda: T.kary(tmp_path, 50, 3)}[shape]()
    tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
    assert _C.seg_pixel_fits(tree.flat)
    check_against_rows(tree, seed=70)


# ------------------------------------------------------------------------------------ 3. precision and layout

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_inputs(dtype):
    """A 16-bit input is widened exactly in the loaders: the same bits as the fp32 kernel on the widened values."""
    tree, _, g = S.case("pascal")
    handle = tree.device_handle(0)
    z = torch.from_numpy(g["z"]).to(DEV).to(dtype)
    y = torch.from_numpy(g["y"]).to(DEV)
    wide = z.float()
    assert torch.equal(_C.seg_hard_forward(handle, z)[0], _C.seg_hard_forward(handle, wide)[0])
    assert torch.equal(_C.seg_soft_forward(handle, z), _C.seg_soft_forward(handle, wide))
    gP = torch.randn(z.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(_C.seg_soft_backward(handle, z, gP), _C.seg_soft_backward(handle, wide, gP))
    a, b = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, S.TSW), _C.seg_soft_tree_loss(handle, wide, y, S.IGNORE, 1.0, S.TSW)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert _C.last_rules_path() == "pixel"


def test_channels_last_takes_the_row_kernels_without_a_copy():
    tree, _, g = S.case("lip")
    handle = tree.device_handle(0)
    z = torch.from_numpy(g["z"]).to(DEV)
    y = torch.from_numpy(g["y"]).to(DEV)
    zl = z.to(memory_format=torch.channels_last)
    assert _C.seg_dispatch(tuple(zl.shape), tuple(zl.stride()), zl.dtype, tree.flat) == "rows"
    pred = _C.seg_hard_forward(handle, zl)[0]
    assert _C.last_rules_path() in ("lds", "lds-unstaged")
    assert torch.equal(pred, _C.seg_hard_forward(handle, z)[0])
    P = _C.seg_soft_forward(handle, zl)
    assert _C.last_rules_path() in ("lds", "lds-unstaged") and P.shape == z.shape
    close_P(P, _C.seg_soft_forward(handle, z))
    loss_l, gz_l = _C.seg_soft_tree_loss(handle, zl, y, S.IGNORE, 1.0, S.TSW)
    assert _C.last_rules_path() in ("lds", "lds-unstaged")
    loss, gz = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, S.TSW)
    assert abs(loss_l.item() - loss.item()) <= 1e-5 * abs(loss.item())
    close_dz(gz_l, gz)
    # a transposed view goes through one .contiguous() and then the pixel kernels: the same bits as the dense tensor
    zt = z.transpose(2, 3).contiguous().transpose(2, 3)
    assert torch.equal(_C.seg_soft_forward(handle, zt), _C.seg_soft_forward(handle, z)) and _C.last_rules_path() == "pixel"


def test_fused_loss_is_reproducible():
    tree, _, _ = S.case("lip")
    handle = tree.device_handle(0)
    z = _shapes(20, 80)["blocks"]
    y = _targets(z, 20, 81)
    a = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, S.TSW, smoothing=0.1)
    b = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, S.TSW, smoothing=0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    bad = y.clone()
    bad[0, 3, 3] = 20                                       # outside [0, C) and not the ignore index: loud
    assert torch.isnan(_C.seg_soft_tree_loss(handle, z, bad, S.IGNORE, 1.0, S.TSW)[0])


# ------------------------------------------------------------------------------------ 4. autograd

class NotFusable(nn.CrossEntropyLoss):
    """The same criterion under another type: the loss module composes it with the autograd-enabled pixel rules."""


def test_autograd_through_a_backbone():
    tree, _, _ = S.case("lip")
    torch.manual_seed(5)
    net = nn.Conv2d(8, 20, 1).to(DEV)
    x = torch.randn(2, 8, 9, 11, device=DEV)
    y = _targets(torch.empty(2, 20, 9, 11), 20, 6)
    fused = L.SoftSegTreeSupLoss(dataset="LookIntoPerson", criterion=nn.CrossEntropyLoss(ignore_index=S.IGNORE),
                                 tree=tree, tree_supervision_weight=S.TSW)
    composed = L.SoftSegTreeSupLoss(dataset="LookIntoPerson", criterion=NotFusable(ignore_index=S.IGNORE), tree=tree,
                                    tree_supervision_weight=S.TSW)
    grads = []
    for crit in (fused, composed):
        net.zero_grad()
        z = net(x)
        z.retain_grad()
        loss = crit(z, y)
        loss.backward()
        grads.append((loss.item(), z.grad.clone(), net.weight.grad.clone(), net.bias.grad.clone()))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * abs(grads[1][0])
    close_dz(grads[0][1], grads[1][1])                      # dL/dz: the bound of test 1
    # dL/dW[c, k] = sum over pixels of dL/dz[p, c] * x[p, k]: two dL/dz within 1e-6 of each other per element give
    # weight gradients within 1e-6 * sum_p |x[p, k]| (plus the rounding of the sums themselves, rtol), the bias 1e-6 * pixels
    bound = 1e-6 * x.abs().sum(dim=(0, 2, 3)).cpu().numpy()
    dw = (grads[0][2] - grads[1][2]).abs().view(20, 8).cpu().numpy()
    assert (dw <= bound[None, :] + 1e-5 * grads[1][2].abs().view(20, 8).cpu().numpy()).all(), dw.max()
    np.testing.assert_allclose(grads[0][3].cpu().numpy(), grads[1][3].cpu().numpy(), atol=1e-6 * 2 * 9 * 11, rtol=1e-5)

    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    first = last = None
    for _ in range(5):
        opt.zero_grad()
        loss = fused(net(x), y)
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
        last = loss.item()
    assert last < first

    soft = M.SoftSegNBDT(dataset="LookIntoPerson", model=net, path_graph=S.paths("lip")[0], path_wnids=S.paths("lip")[1])
    hard = M.HardSegNBDT(dataset="LookIntoPerson", model=net, path_graph=S.paths("lip")[0], path_wnids=S.paths("lip")[1])
    with torch.no_grad():
        out, labels = soft(x), hard.predict(x)
        assert out.shape == (2, 20, 9, 11) and out._nbdt_output_flag and labels.shape == (2, 9, 11)
        assert torch.equal(hard(x).argmax(1), labels) and torch.equal(soft.predict(x), out.argmax(1))
    with pytest.raises(AssertionError, match="NBDT wrapper"):
        fused(out, y)


# ------------------------------------------------------------------------------------ 5. fallback

def test_beyond_the_pixel_form(tmp_path):
    """A 400-way star (R + F = 800 > 640) takes the row kernels on a coerced copy and still gives their results."""
    pg, pw, leaves = T.star(tmp_path, 400)
    tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
    handle = tree.device_handle(0)
    z = _shapes(400, 90)["tail"]
    rows = coerce(z)
    pred = _C.seg_hard_forward(handle, z)[0]
    assert _C.last_rules_path() not in ("pixel", "")
    assert torch.equal(pred.view(-1), _C.hard_forward(handle, rows)[0])
    P = _C.seg_soft_forward(handle, z)
    assert _C.last_rules_path() != "pixel"
    assert torch.equal(P, uncoerce(_C.soft_forward(handle, rows), z.shape))
    y = _targets(z, 400, 91)
    keep = (y.view(-1) != S.IGNORE).nonzero().squeeze(1)
    loss, gz = _C.seg_soft_tree_loss(handle, z, y, S.IGNORE, 1.0, 2.0)
    assert _C.last_rules_path() != "pixel"
    loss_rows, g_rows = _C.soft_tree_loss(handle, rows[keep], y.view(-1)[keep], 1.0, 2.0)
    full = torch.zeros_like(rows)
    full[keep] = g_rows
    assert torch.equal(loss, loss_rows) and torch.equal(gz, uncoerce(full, z.shape))
    with pytest.raises(_C.NBDTHipError, match="beyond the pixel form"):
        _C.check(_C.lib().nbdt_seg_soft_forward(handle.h, _C.ptr(z), 0, 2, 65, 400 * 65, 65, _C.ptr(P.contiguous()), None))
