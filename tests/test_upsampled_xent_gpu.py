"""Cross-entropy on bilinearly upsampled logits on the GPU (csrc/upsampled_xent.hip) and SoftSegTreeSupLoss on top of it.

Yardstick: torch's composition F.cross_entropy(F.interpolate(...)) in float64 on the CPU with autograd.  Bounds: the
project's own from tests/test_seg_gpu.py -- loss 1e-5 relative, gradient 1e-6 absolute.  The fp32 CPU composition stays
within them on every case here (tests/test_upsampled_xent.py::test_fp32_composition_is_within_the_bounds).

Shapes (h, w) -> (H, W): (1, 1) -> (3, 5) every tap clamped; (3, 4) -> (12, 16) integer scale, exactly three waves;
(5, 7) -> (17, 23) non-integer scale, 391 pixels, a tail; (2, 3) -> (2, 9) one axis only.  N = 2 on a channel-sliced
view, 30 % ignored labels with pixel 0 valid, in the odd pairs a whole image ignored.  C = 5 stays inside one load block
of the forward (8 classes) and one and a half class chunks of the backward (4), C = 40 is several full ones, C = 19 (the
non-integer pair only) full blocks and a tail."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from nbdt import _C
from nbdt import loss as L
from nbdt.tree import Tree

import _seg_ref as S
import _tree_shapes as T
import _upsampled_ref as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES, KINDS = U.CASES, U.KINDS


def run(x, y, ac, weight=None, smoothing=0.0, **kw):
    return _C.upsampled_xent(U.on_device(x, DEV), y.to(DEV), ac, U.IGNORE, None if weight is None else weight.to(DEV),
                             smoothing, **kw)


def check(tag, loss, gx, ref_loss, ref_dx):
    rel = abs(loss.item() - ref_loss) / abs(ref_loss)
    worst = np.abs(gx.cpu().numpy().astype(np.float64) - ref_dx).max()
    print(f"{tag}: loss rel {rel:.2e}, gx abs {worst:.2e}")
    assert rel <= 1e-5, tag
    assert worst <= 1e-6, tag


# ------------------------------------------------------------------------------------ 1. the stand-alone criterion

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair, C, ac", CASES)
def test_criterion_against_float64(pair, C, ac, kind):
    x, y, weight, eps, ref_loss, ref_dx = U.standalone_case(pair, C, ac, kind)
    xd = U.on_device(x, DEV)
    assert not xd.is_contiguous() and _C._dense_planes(tuple(xd.shape), tuple(xd.stride()))     # the sliced view, as it is
    loss, gx = _C.upsampled_xent(xd, y.to(DEV), ac, U.IGNORE, None if weight is None else weight.to(DEV), eps)
    check(f"{U.PAIRS[pair]} C={C} ac={ac} {kind}", loss, gx, ref_loss, ref_dx)
    assert gx.shape == x.shape and gx.dtype == torch.float32
    # grad_scale scales the gradient and nothing else
    loss2, gx2 = _C.upsampled_xent(xd, y.to(DEV), ac, U.IGNORE, None if weight is None else weight.to(DEV), eps,
                                   grad_scale=0.5)
    assert torch.equal(loss2, loss)
    np.testing.assert_allclose(gx2.cpu().numpy(), 0.5 * gx.cpu().numpy(), rtol=2e-7, atol=0)


@pytest.mark.parametrize("ac", [False, True])
def test_module_autograd_and_layouts(ac):
    """The nn.Module through autograd on a backbone's output; a layout without dense planes takes one .contiguous()."""
    x, y, _, _, ref_loss, ref_dx = U.standalone_case(2, 5, ac, "plain")
    crit = L.UpsampledCrossEntropyLoss(ignore_index=U.IGNORE, align_corners=ac)
    xd = x.to(DEV).contiguous().requires_grad_(True)
    assert crit.route(xd, y.to(DEV)) == "fused"
    loss = crit(xd * 1.0, y.to(DEV))
    (3.0 * loss).backward()
    check(f"module ac={ac}", loss.detach(), xd.grad / 3.0, ref_loss, ref_dx)
    direct = run(x, y, ac)
    for view in (x.to(DEV).to(memory_format=torch.channels_last), x.to(DEV).transpose(2, 3).contiguous().transpose(2, 3)):
        loss_v, gx_v = _C.upsampled_xent(view, y.to(DEV), ac, U.IGNORE)
        assert torch.equal(loss_v, direct[0]) and torch.equal(gx_v, direct[1])
    # targets at the logits' size and no weights: torch's criterion
    same = U.targets(2, 5, 5, 7, 9).to(DEV)
    assert crit.route(xd, same) == "plain"
    assert torch.equal(crit(xd, same), F.cross_entropy(xd, same, ignore_index=U.IGNORE))
    # the same size with class weights is the kernel's (H == h, W == w: every tap is the pixel itself)
    weight = U.class_weights(5, 10)
    wcrit = L.UpsampledCrossEntropyLoss(weight=weight, ignore_index=U.IGNORE, align_corners=ac).to(DEV)
    assert wcrit.route(xd, same) == "fused"
    ref = U.composition(x, same, ac, weight)
    loss_w, gx_w = _C.upsampled_xent(xd.detach(), same, ac, U.IGNORE, weight.to(DEV))
    check(f"same size, weights, ac={ac}", loss_w, gx_w, *ref)
    assert abs(wcrit(xd, same).item() - ref[0]) <= 1e-5 * abs(ref[0])
    # what the kernel refuses composes: class weights together with smoothing
    both = L.UpsampledCrossEntropyLoss(weight=weight, ignore_index=U.IGNORE, label_smoothing=0.1, align_corners=ac).to(DEV)
    assert both.route(xd, y.to(DEV)) == "composed"
    ref_both = U.composition(x, y, ac, weight, 0.1)
    assert abs(both(xd, y.to(DEV)).item() - ref_both[0]) <= 1e-5 * abs(ref_both[0])


def test_no_valid_pixel_and_stray_labels():
    x, y, _, _, _, _ = U.standalone_case(2, 5, False, "plain")
    none = torch.full_like(y, U.IGNORE)
    for weight in (None, U.class_weights(5, 1)):
        loss, gx = run(x, none, False, weight)
        assert torch.isnan(loss) and not gx.any()
    bad = y.clone()
    bad[0, 3, 3] = 5 + 3                                     # outside [0, C) and not the ignore index: loud
    for weight in (None, U.class_weights(5, 1)):
        assert torch.isnan(run(x, bad, False, weight)[0])
    bad[0, 3, 3] = -1
    assert torch.isnan(run(x, bad, False)[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_inputs(dtype):
    """A 16-bit input is widened exactly in the loaders: the same bits as the fp32 kernel on the widened values."""
    for pair, C in ((1, 5), (2, 40)):
        x, y, _, _, _, _ = U.standalone_case(pair, C, False, "plain")
        narrow = x.to(DEV).to(dtype)
        a, b = run(narrow, y, False, smoothing=0.1), run(narrow.float(), y, False, smoothing=0.1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_two_calls_give_the_same_bits():
    for kind in KINDS:
        x, y, weight, eps, _, _ = U.standalone_case(2, 40, False, kind)
        a, b = run(x, y, False, weight, eps), run(x, y, False, weight, eps)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kind
    x, y, _, _, ref_loss, ref_dx = U.standalone_case(2, 5, False, "plain")
    crit = L.UpsampledCrossEntropyLoss(ignore_index=U.IGNORE)
    torch.use_deterministic_algorithms(True)
    try:                                                     # torch's bilinear backward raises here; the kernels run
        grads = []
        for _ in range(2):
            xd = x.to(DEV).contiguous().requires_grad_(True)
            loss = crit(xd, y.to(DEV))
            loss.backward()
            grads.append((loss.detach(), xd.grad))
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    check("deterministic mode", grads[0][0], grads[0][1], ref_loss, ref_dx)


@pytest.mark.parametrize("pair, ac", [(p, ac) for p in range(4) for ac in (False, True)])
def test_backward_is_the_adjoint_of_the_forward_taps(pair, ac):
    """<A x, g> = <x, A^T g> with A from nbdt_upsample_taps, and the kernel's gx against A^T applied to a float64 f:
    the gather's weights are the forward's taps, clamped borders included."""
    (h, w), (H, W) = U.PAIRS[pair]
    Ay, Ax = U.matrix(h, H, ac, _C.upsample_taps), U.matrix(w, W, ac, _C.upsample_taps)
    rng = np.random.default_rng(pair)
    xs, g = rng.standard_normal((h, w)), rng.standard_normal((H, W))
    lhs, rhs = ((Ay @ xs @ Ax.T) * g).sum(), (xs * (Ay.T @ g @ Ax)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    for kind in KINDS:
        x, y, weight, eps, _, _ = U.standalone_case(pair, 5, ac, kind)
        ref_loss, ref_dx = U.gather_form(x, y, ac, _C.upsample_taps, weight, eps)
        loss, gx = run(x, y, ac, weight, eps)
        check(f"adjoint {U.PAIRS[pair]} ac={ac} {kind}", loss, gx, ref_loss, ref_dx)


# ------------------------------------------------------------------------------------ 2. SoftSegTreeSupLoss

class Composed(L.UpsampledCrossEntropyLoss):
    """The same criterion under another type, and torch's composition throughout: SoftSegTreeSupLoss applies it through
    autograd to the logits and to the output of the autograd-enabled pixel rules (F.interpolate, F.cross_entropy)."""

    def forward(self, score, target):
        return self.composed(score, target)


def _lip():
    return S.case("lip")[0], S.case("lip")[1], 20


def _kary(tmp_path):
    pg, pw, leaves = T.kary(tmp_path, 40, 3)
    return Tree(None, path_graph=pg, path_wnids=pw, classes=leaves), None, 40


def _losses(tree, **kw):
    make = lambda crit: L.SoftSegTreeSupLoss(dataset=None, criterion=crit, tree=tree, tree_supervision_weight=S.TSW)  # noqa: E731
    return make(L.UpsampledCrossEntropyLoss(ignore_index=S.IGNORE, **kw)), make(Composed(ignore_index=S.IGNORE, **kw))


@pytest.mark.parametrize("which", ["lip", "kary40_3"])
def test_tree_loss_against_the_composed_criterion(which, tmp_path):
    """Through a 1 x 1 convolution, as tests/test_seg_gpu.py::test_autograd_through_a_backbone: the fused pair against the
    same loss with a subclassed criterion (torch's interpolate and cross-entropy on the autograd-enabled pixel rules)."""
    tree, _, C = _lip() if which == "lip" else _kary(tmp_path)
    torch.manual_seed(5)
    net = nn.Conv2d(8, C, 1).to(DEV)
    x = torch.randn(2, 8, 9, 11, device=DEV)
    y = U.targets(2, C, 36, 44, 6).to(DEV)
    fused, composed = _losses(tree)
    assert L.seg_criterion_route(fused.criterion, (2, C, 9, 11), torch.float32, (2, 36, 44), torch.int64) == ("upsampled",)
    grads = []
    for crit in (fused, composed):
        net.zero_grad()
        z = net(x)
        z.retain_grad()
        loss = crit(z, y)
        loss.backward()
        grads.append((loss.item(), z.grad.clone(), net.weight.grad.clone(), net.bias.grad.clone()))
    dz = (grads[0][1] - grads[1][1]).abs().max().item()
    print(f"{which}: loss rel {abs(grads[0][0] - grads[1][0]) / abs(grads[1][0]):.2e}, dL/dz abs {dz:.2e}")
    assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * abs(grads[1][0])
    assert dz <= 1e-6
    # the derived bounds of test_autograd_through_a_backbone: two dL/dz within 1e-6 per element give weight gradients
    # within 1e-6 * sum_p |x[p, k]| (plus the rounding of the sums themselves, rtol), the bias 1e-6 * pixels
    bound = 1e-6 * x.abs().sum(dim=(0, 2, 3)).cpu().numpy()
    dw = (grads[0][2] - grads[1][2]).abs().view(C, 8).cpu().numpy()
    assert (dw <= bound[None, :] + 1e-5 * grads[1][2].abs().view(C, 8).cpu().numpy()).all(), dw.max()
    np.testing.assert_allclose(grads[0][3].cpu().numpy(), grads[1][3].cpu().numpy(), atol=1e-6 * 2 * 9 * 11, rtol=1e-5)
    # loss_and_grad is the same computation without autograd
    z = net(x).detach()
    loss, gz = fused.loss_and_grad(z, y, grad_scale=2.0)
    assert abs(loss.item() - grads[1][0]) <= 1e-5 * abs(grads[1][0])
    assert (gz / 2.0 - grads[1][1]).abs().max().item() <= 1e-6

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


@pytest.mark.parametrize("ac", [False, True])
def test_tree_loss_against_float64(ac):
    """loss = CE(up(z), y) + w * CE(up(P), y) in float64 on the CPU, P from the oracle's rules (_seg_ref.soft) and the
    rules' backward from the oracle too (nbdt_oracle.rules_backward on dL/dP)."""
    import nbdt_oracle as O
    tree, otree, C = _lip()
    z = U.logits(2, C, 9, 11, 21)
    y = U.targets(2, C, 36, 44, 22, ignored_image=1)
    P = torch.from_numpy(S.soft(otree, z.numpy()))
    loss_z, dz = U.composition(z, y, ac, ignore=S.IGNORE)
    loss_p, dP = U.composition(P, y, ac, ignore=S.IGNORE)
    back = O.rules_backward(otree, S.coerce(z.numpy()), S.coerce((S.TSW * dP).astype(np.float32)))
    ref_loss, ref_dz = loss_z + S.TSW * loss_p, dz + S.uncoerce(back, z.shape).astype(np.float64)
    fused, _ = _losses(tree, align_corners=ac)
    loss, gz = fused.loss_and_grad(z.to(DEV), y.to(DEV))
    check(f"tree loss ac={ac}", loss, gz, ref_loss, ref_dz)
    assert not gz[1].any()                                   # the image without a valid pixel gets nothing
    only = y.clone()
    only[0] = S.IGNORE
    assert not fused.loss_and_grad(z.to(DEV), only.to(DEV))[1].any()


def test_targets_at_the_logits_size_take_the_existing_call():
    tree, _, C = _lip()
    z = U.logits(2, C, 9, 11, 31).to(DEV)
    y = U.targets(2, C, 9, 11, 32).to(DEV)
    fused, _ = _losses(tree)
    plain = L.SoftSegTreeSupLoss(dataset=None, criterion=nn.CrossEntropyLoss(ignore_index=S.IGNORE), tree=tree,
                                 tree_supervision_weight=S.TSW)
    a, b = fused.loss_and_grad(z, y), plain.loss_and_grad(z, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    la, lb = fused(za, y), plain(zb, y)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(za.grad, zb.grad)
    assert _C.last_rules_path() == "pixel"


def test_beyond_the_pixel_form(tmp_path):
    """A 400-way star (R + F = 800 > 640): the rules take the row kernels on a coerced copy, the cross-entropies do not
    care, and the result matches the composed path."""
    pg, pw, leaves = T.star(tmp_path, 400)
    tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
    assert not _C.seg_pixel_fits(tree.flat)
    z = U.logits(2, 400, 5, 13, 41).to(DEV)
    y = U.targets(2, 400, 10, 39, 42).to(DEV)
    fused, composed = _losses(tree)
    loss, gz = fused.loss_and_grad(z, y)
    assert _C.last_rules_path() not in ("pixel", "")
    zc = z.clone().requires_grad_(True)
    ref = composed(zc, y)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert (gz - zc.grad).abs().max().item() <= 1e-6
    # channels_last logits keep their route through the rules as well
    loss_l, gz_l = fused.loss_and_grad(z.to(memory_format=torch.channels_last), y)
    assert abs(loss_l.item() - ref.item()) <= 1e-5 * abs(ref.item()) and (gz_l - zc.grad).abs().max().item() <= 1e-6


def test_no_full_resolution_tensor():
    """A condition, not a measurement: forward + backward of the fused loss allocate less than ONE [N, C, H, W] fp32
    tensor at their peak; the composed path needs several."""
    tree, _, C = _lip()
    N, h, w, H, W = 2, 64, 64, 256, 256
    full = N * C * H * W * 4
    z = U.logits(N, C, h, w, 51).to(DEV)
    y = U.targets(N, C, H, W, 52).to(DEV)
    peaks = []
    for crit in _losses(tree):
        zz = z.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = crit(zz, y)
        loss.backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        del loss, zz
    print(f"peak bytes: fused {peaks[0]}, composed {peaks[1]}, one full-resolution tensor {full}")
    assert peaks[0] < full
    assert peaks[1] > 3 * full
