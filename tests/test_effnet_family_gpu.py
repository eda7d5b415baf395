"""EfficientNet-B1..B7 / b0b..b7b on the GPU: the strided depthwise and stem convolutions at any extent and with a
low-side padding (per-op parity against F.conv2d on the CPU, borders, bounds, the old entry points' bits), whole training
steps against the fp32 restatement of tests/_effnet_family_ref.py, the largest variant, the driver.

Tolerances are those tests/test_effnet_gpu.py applies to the same entry points at even extents (bf16 outputs: 2^-7
relative + 1e-3; weight gradients: 2e-3 of their scale; fused statistics: mean 1e-3, rstd 2e-3 relative), those of
tests/test_reference_fp32_gpu.py for fp32 storage (outputs 1e-4 of their scale, gradients 1e-3 relative L2) and those of
tests/test_baseline_configs_gpu.py's EfficientNet-B0 case for bf16 storage of a whole step, re-based on what bf16 storage
alone costs at the small shapes used here (BF16_BOUNDS)."""
import importlib.util
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nbdt_oracle as O
import nbdt_path

pytestmark = pytest.mark.gpu

from nbdt import models, ops  # noqa: E402
from nbdt.engine import train_step  # noqa: E402
from nbdt.engine_effnet import EfficientNetEngine, efficientnet_config  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

from _effnet_family_ref import EfficientNetRef  # noqa: E402

DEV = "cuda:0"
SENTINEL = 1024.0        # (exact in bf16)
SYM = [(9, 9), (15, 13), (7, 5), (17, 33)]
SAME = [(8, 8), (16, 12), (10, 6), (15, 13)]
CASES = [(False, hw) for hw in SYM] + [(True, hw) for hw in SAME]
# bf16 storage of a whole step: (logit error / logit scale, gradient-cosine floor).  test_baseline_configs_gpu.py asks 6 % and
# 0.93 of EfficientNet-B0 at 32 x 224 x 224, where it measured 3.1 % and 0.98.  At 4 images and 3 x 3 final maps a BatchNorm
# channel averages 36 values and those bounds do not hold for ANY bf16 storage: the fp32 restatement against itself with
# bf16-rounded stored tensors and 1x1 weights (_effnet_family_ref.emulate_bf16, same weights and batch as below, CPU)
# measures 7.98 % / 0.8537 for b1 at 72 and 11.11 % / 0.9190 for b2b at 80.  The bounds are those plus the existing file's
# margins (+ 2.9 points, - 0.05).  The engine itself measured, over two runs (the order of its fp32 atomics differs from
# run to run), 6.9 % / 0.852 .. 0.878 and 6.4 .. 8.0 % / 0.939 .. 0.945.
BF16_BOUNDS = {"b1": (0.0798 + 0.029, 0.8537 - 0.05), "b2": (0.1111 + 0.029, 0.9190 - 0.05)}


def _bf(x):
    return x.to(torch.bfloat16).float()


def _guarded(B, H, W, C, dtype, fill):
    """A zeroed padded [B][H+2][W+2][C] tensor in the middle of one allocation whose cells in front of and behind it hold
    `fill`: NaN around an input poisons any read beyond the tensor, a sentinel behind an output shows any write there."""
    n, guard = B * (H + 2) * (W + 2) * C, 2 * (W + 2) * C + 64
    flat = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    t = flat[guard:guard + n].view(B, H + 2, W + 2, C)
    t.zero_()
    return t, flat, guard


def _guards_intact(flat, guard, fill):
    lo, hi = flat[:guard].float(), flat[-guard:].float()
    return bool((lo == fill).all() and (hi == fill).all())


def _fill(t, x_nchw):
    ops.interior(t).copy_(x_nchw.permute(0, 2, 3, 1).to(DEV))
    return t


def _nchw(t):
    return ops.interior(t).float().permute(0, 3, 1, 2).cpu()


def _border_is_zero(t):
    return all(v.abs().max().item() == 0 for v in (t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1]))


def _close_bf16(got, want, what, rel=2 ** -7, abs_=1e-3):
    err = (got - want).abs()
    assert (err <= rel * want.abs() + abs_).all(), f"{what}: max err {err.max().item():.4g} at |ref| {want.abs().max().item():.4g}"


def _close_fp32(got, want, what):
    assert (got - want).abs().max().item() < 1e-4 * want.abs().max().item(), what


def _rel_l2(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _pads(h, w, k, same):
    return ops.conv_padding(h, k, 2, same), ops.conv_padding(w, k, 2, same)


def _conv_ref(x, w, k, same, groups):
    (pt, pb), (pl, pr) = _pads(x.shape[2], x.shape[3], k, same)
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, None, 2, 0, 1, groups)


@pytest.fixture(scope="module")
def dw_reference():
    """(same, H, W, C, k) -> bf16-rounded operands and the fp32 CPU results, computed once per case and never changed."""
    cache = {}

    def get(same, H, W, C, k):
        key = (same, H, W, C, k)
        if key not in cache:
            g = torch.Generator().manual_seed(hash(key) % 100000)
            B = 3
            x = _bf(torch.randn(B, C, H, W, generator=g))
            w = torch.randn(C, 1, k, k, generator=g) * 0.3
            Ho, Wo = ops.conv_out_size(H, 2), ops.conv_out_size(W, 2)
            gy = _bf(torch.randn(B, C, Ho, Wo, generator=g))
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            y = _conv_ref(xr, wr, k, same, C)
            assert tuple(y.shape[2:]) == (Ho, Wo)
            y.backward(gy)
            cache[key] = dict(x=x, w=w, gy=gy, y=y.detach(), gx=xr.grad, gw=wr.grad.view(C, k * k).t().contiguous(),
                              Ho=Ho, Wo=Wo)
        return cache[key]

    return get


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("same,hw", CASES, ids=[f"{'same' if s else 'sym'}-{h}x{w}" for s, (h, w) in CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32ref"])
def test_strided_depthwise_at_any_extent_and_padding(dw_reference, dtype, same, hw, C, k):
    """Forward (plain and with the next BatchNorm's statistics fused), data gradient and weight gradient at stride 2 against
    F.conv2d (F.pad for the asymmetric cases) on the same bf16-rounded operands; the one-pixel border of every written
    tensor stays zero, a sentinel in front of and behind it is untouched, and NaN around the inputs reaches no output."""
    (H, W), B = hw, 3
    r = dw_reference(same, H, W, C, k)
    Ho, Wo = r["Ho"], r["Wo"]
    pad = (_pads(H, W, k, same)[0][0], _pads(H, W, k, same)[1][0])
    bf = dtype == torch.bfloat16
    close = _close_bf16 if bf else _close_fp32
    wt = r["w"].view(C, k * k).t().contiguous().to(DEV)
    xp = _fill(_guarded(B, H, W, C, dtype, float("nan"))[0], r["x"])
    gyp = _fill(_guarded(B, Ho, Wo, C, dtype, float("nan"))[0], r["gy"])

    yp, yflat, yg = _guarded(B, Ho, Wo, C, dtype, SENTINEL)
    ops.dwconv_fwd(xp, wt, yp, k, 2, pad=pad)
    assert torch.isfinite(yp.float()).all()
    close(_nchw(yp), r["y"], "forward")
    assert _border_is_zero(yp) and _guards_intact(yflat, yg, SENTINEL)

    gxp, gflat, gg = _guarded(B, H, W, C, dtype, SENTINEL)
    ops.dwconv_bwd_data(gyp, wt, gxp, k, 2, pad=pad)
    assert torch.isfinite(gxp.float()).all()
    close(_nchw(gxp), r["gx"], "data gradient")
    assert _border_is_zero(gxp) and _guards_intact(gflat, gg, SENTINEL)

    dw = torch.zeros(k * k, C, device=DEV)
    ops.dwconv_bwd_weight(xp, gyp, dw, k, 2, pad=pad)
    ops.dwconv_bwd_weight(xp, gyp, dw, k, 2, pad=pad)           # accumulates (+=)
    want = 2 * r["gw"]
    print(f"weight gradient: max err {(dw.cpu() - want).abs().max().item():.3g} of {want.abs().max().item():.3g}; "
          f"rel-L2 {_rel_l2(dw, want):.3g}")
    if bf:
        assert (dw.cpu() - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-4
    else:
        assert _rel_l2(dw, want) < 1e-3

    if bf:      # fused batch statistics of the output (the fp32 twin leaves none: bn_stats re-reads the tensor there)
        scratch = torch.zeros(ops.BN_SLOTS * 2 * 2048, device=DEV)
        mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        yp2, y2flat, y2g = _guarded(B, Ho, Wo, C, dtype, SENTINEL)
        ops.dwconv_fwd(xp, wt, yp2, k, 2, bn_scratch=scratch, pad=pad)
        ops.bn_stats(yp2, scratch, mean, rstd, slots_filled=True)
        assert torch.equal(yp2, yp) and scratch.abs().max().item() == 0 and _guards_intact(y2flat, y2g, SENTINEL)
        yq = _nchw(yp)
        want_mean = yq.mean((0, 2, 3))
        want_rstd = 1.0 / torch.sqrt(yq.var((0, 2, 3), unbiased=False) + 1e-5)
        assert (mean.cpu() - want_mean).abs().max().item() < 1e-3 * (1 + want_mean.abs().max().item())
        assert ((rstd.cpu() - want_rstd).abs() / want_rstd).max().item() < 2e-3


@pytest.mark.parametrize("same,hw", [(True, (16, 20)), (False, (17, 19))], ids=["same-16x20", "sym-17x19"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32ref"])
def test_strided_stem_at_any_extent_and_padding(dtype, same, hw):
    (H, W), B, cout, cpad = hw, 3, 40, 64
    g = torch.Generator().manual_seed(H * 100 + W)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.2
    Ho, Wo = ops.conv_out_size(H, 2), ops.conv_out_size(W, 2)
    gy = _bf(torch.randn(B, cout, Ho, Wo, generator=g))
    wr = w.clone().requires_grad_(True)
    ref = _conv_ref(img, wr, 3, same, 1)
    ref.backward(gy)
    pad = (_pads(H, W, 3, same)[0][0], _pads(H, W, 3, same)[1][0])
    bf = dtype == torch.bfloat16
    nan = float("nan")
    iflat = torch.full((img.numel() + 2048,), nan, device=DEV)        # NaN in front of and behind the image
    imgd = iflat[1024:1024 + img.numel()].view_as(img)
    imgd.copy_(img)
    wk = w.permute(0, 2, 3, 1).contiguous().to(DEV)                   # [co][r][s][ci]
    out, oflat, og = _guarded(B, Ho, Wo, cpad, dtype, SENTINEL)
    ops.stem_conv(imgd, wk, out, cout, stride=2, pad=pad)
    got = _nchw(out)
    assert torch.isfinite(got).all() and got[:, cout:].abs().max().item() == 0
    (_close_bf16 if bf else _close_fp32)(got[:, :cout], ref.detach(), "stem forward")
    assert _border_is_zero(out) and _guards_intact(oflat, og, SENTINEL)
    gyp = _guarded(B, Ho, Wo, cpad, dtype, nan)[0]
    ops.interior(gyp)[..., :cout].copy_(gy.permute(0, 2, 3, 1).to(DEV))
    dw = torch.zeros(cout, 3, 3, 3, device=DEV)
    ops.stem_wgrad(imgd, gyp, dw, cout, stride=2, pad=pad)
    want = wr.grad.permute(0, 2, 3, 1)
    assert torch.isfinite(dw).all()
    if bf:
        assert (dw.cpu() - want).abs().max().item() < 2e-3 * want.abs().max().item()
    else:
        assert _rel_l2(dw, want) < 1e-3


@pytest.mark.parametrize("k,C,H,W", [(3, 96, 12, 16), (5, 64, 16, 8), (3, 32, 10, 6), (5, 1152, 4, 4)])
def test_symmetric_padding_on_even_extents_is_the_old_entry_points_bit_for_bit(k, C, H, W):
    """pad_lo = k / 2 through the new entry points = the entry points without a padding argument: forward (with and without
    statistics), both stride-2 data-gradient forms (W % 4 == 0 and not), the weight gradient in deterministic mode; stem too."""
    g = torch.Generator().manual_seed(k + C + H)
    B = 3
    x = _fill(ops.padded(B, H, W, C, DEV), _bf(torch.randn(B, C, H, W, generator=g)))
    gy = _fill(ops.padded(B, H // 2, W // 2, C, DEV), _bf(torch.randn(B, C, H // 2, W // 2, generator=g)))
    wt = (torch.randn(k * k, C, generator=g) * 0.3).to(DEV)
    pad = (k // 2, k // 2)
    outs = []
    for p in (None, pad):
        y, gx = ops.padded(B, H // 2, W // 2, C, DEV), ops.padded(B, H, W, C, DEV)
        ys = ops.padded(B, H // 2, W // 2, C, DEV)
        scratch = torch.zeros(ops.BN_SLOTS * 2 * 2048, device=DEV)
        ops.dwconv_fwd(x, wt, y, k, 2, pad=p)
        ops.set_deterministic(True)
        try:
            ops.dwconv_fwd(x, wt, ys, k, 2, bn_scratch=scratch, pad=p)
            dw = torch.zeros(k * k, C, device=DEV)
            ops.dwconv_bwd_weight(x, gy, dw, k, 2, pad=p)
        finally:
            ops.set_deterministic(False)
        ops.dwconv_bwd_data(gy, wt, gx, k, 2, pad=p)
        outs.append((y, ys, scratch.clone(), gx, dw))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    if k == 3:
        img = torch.randn(B, 3, H, W, generator=g).to(DEV)
        wk = (torch.randn(32, 3, 3, 3, generator=g) * 0.2).to(DEV)
        gys = _fill(ops.padded(B, H // 2, W // 2, 32, DEV), _bf(torch.randn(B, 32, H // 2, W // 2, generator=g)))
        res = []
        for p in (None, (1, 1)):
            out, dws = ops.padded(B, H // 2, W // 2, 32, DEV), torch.zeros(32, 3, 3, 3, device=DEV)
            ops.stem_conv(img, wk, out, 32, stride=2, pad=p)
            ops.stem_wgrad(img, gys, dws, 32, stride=2, pad=p)
            res.append((out, dws))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------- whole steps

def _oracle_step(ref, otree, x, y):
    ref.train()
    z = ref(x)
    loss, dz = O.soft_tree_sup_loss(otree, z.detach().numpy(), y.numpy(), 1.0, 1.0)
    z.backward(torch.from_numpy(dz))
    return z.detach(), float(loss), {n: p.grad.clone() for n, p in ref.named_parameters()}


def _engine_step(eng, crit, x, y):
    eng.zero_grad()
    z = eng.forward(x.to(DEV), training=True)
    loss, gz = crit.loss_and_grad(z, y.to(DEV))
    eng.backward(gz)
    torch.cuda.synchronize()
    return z.float().cpu(), loss.item(), {k: v.float().cpu().clone() for k, v in eng.named_params("grad").items()}


@pytest.mark.parametrize("version,tf_mode,size", [("b1", False, 72), ("b2", True, 80)], ids=["b1-72", "b2b-80"])
def test_whole_step_against_the_fp32_restatement(version, tf_mode, size, pkg_dir):
    """One training step of efficientnet_b1 at 72 (72 -> 36 -> 18 -> 9 -> 5 -> 3: odd extents, a stage-1 unit with a skip)
    and of efficientnet_b2b at 80 (SAME padding on even extents, then 5 -> 3; widths 88 / 120 / 208 / 352 and a 2112-wide
    expansion: two channel ranges per launch): in fp32 storage within test_reference_fp32_gpu.py's EfficientNet-B0 bounds of
    the restatement with identical weights, in bf16 storage within BF16_BOUNDS (test_baseline_configs_gpu.py's, re-based)."""
    classes, B = 10, 4
    config = efficientnet_config(version, tf_mode)
    otree = O.OracleTree(*O.default_paths("CIFAR10", "induced-ResNet18", pkg_dir))
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    torch.manual_seed(7)
    ref = EfficientNetRef(config, num_classes=classes, dropout_rate=0.0)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    eng = EfficientNetEngine.from_config(config, num_classes=classes, dropout_rate=0.0, device=DEV)
    assert set(eng.state_dict()) == set(init)
    assert all(tuple(v.shape) == tuple(init[k].shape) for k, v in eng.state_dict().items())
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, 3, size, size, generator=g)
    y = torch.randint(0, classes, (B,), generator=g)
    z_ref, loss_ref, g_ref = _oracle_step(ref, otree, x, y)
    scale = z_ref.abs().max().item()
    gmax = max(v.abs().max().item() for v in g_ref.values())
    zero = {n for n in g_ref if g_ref[n].norm().item() < 1e-6 * gmax}     # a BatchNorm shift feeding conv -> BatchNorm

    eng.set_reference_fp32(True)
    eng.load_state_dict(init)
    z, loss, grads = _engine_step(eng, crit, x, y)
    errs = sorted((_rel_l2(grads[n], g_ref[n]), n) for n in g_ref if n not in zero)
    print(f"[{version}{'b' if tf_mode else ''} fp32] logits {(z - z_ref).abs().max().item():.3g} of {scale:.3g}; loss {loss:.6f} vs "
          f"{loss_ref:.6f}; gradient rel-L2 worst {errs[-1][0]:.2e} ({errs[-1][1]}), median {errs[len(errs) // 2][0]:.2e}")
    assert (z - z_ref).abs().max().item() < 1e-4 * scale
    assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref)
    assert set(grads) == set(g_ref)
    for n in zero:
        assert grads[n].norm().item() < 1e-4 * gmax, n
    assert errs[-1][0] < 1e-3, errs[-1]

    eng.set_reference_fp32(False)
    eng.load_state_dict(init)
    z, loss, grads = _engine_step(eng, crit, x, y)
    rows = [(n, _cos(grads[n], g_ref[n]), grads[n].norm().item() / (g_ref[n].norm().item() + 1e-30)) for n in g_ref
            if g_ref[n].norm().item() >= 1e-6]
    worst = min(rows, key=lambda r: r[1])
    print(f"[{version}{'b' if tf_mode else ''} bf16] logits {(z - z_ref).abs().max().item():.3g} of {scale:.3g}; loss {loss:.5f} vs "
          f"{loss_ref:.5f}; worst cosine {worst[1]:.4f} ({worst[0]}); norm ratios {min(r[2] for r in rows):.3f}.."
          f"{max(r[2] for r in rows):.3f}")
    logit_bound, cos_floor = BF16_BOUNDS[version]
    assert (z - z_ref).abs().max().item() < logit_bound * scale
    assert abs(loss - loss_ref) < 2e-2 * abs(loss_ref)
    bad = [(n, round(c, 4), round(ratio, 4)) for n, c, ratio in rows if not c > cos_floor]
    assert not bad, bad


def test_fused_evaluation_of_a_tf_padded_variant_equals_the_unfused_one():
    eng = models.efficientnet_b1b(num_classes=10, device=DEV, seed=1).engine
    assert eng.tf_mode and eng.bn_eps == 1e-3 and all(b.eps == 1e-3 for b in eng.bns)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, 3, 72, 72, generator=g).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    for _ in range(3):                                    # make the running statistics non-trivial
        train_step(eng, crit, x, y, 0.02)
    eng.fuse_eval = True
    zf = eng.forward(x, training=False).clone()
    eng.fuse_eval = False
    zu = eng.forward(x, training=False).clone()
    scale = zu.abs().max().item()
    assert torch.isfinite(zu).all()
    assert (zf - zu).abs().max().item() < 3e-2 * scale, ((zf - zu).abs().max().item(), scale)
    assert (zf.argmax(1) == zu.argmax(1)).float().mean().item() >= 0.9


def test_largest_variant_trains_with_stochastic_depth():
    """efficientnet_b7: 55 units, 3840-channel expansions (two channel ranges), four stage-1 units; the drawn table has a
    row per unit, a step is finite and the loss falls over three steps at a small learning rate."""
    net = models.efficientnet_b7(num_classes=10, device=DEV, seed=2, stochastic_depth_prob=0.2, dropout_rate=0.0)
    eng = net.engine
    assert len(eng.units) == 55 and sum(v.numel() for v in eng.named_params("flat").values()) == 66347960 - 2560 * 990 - 990
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 96, 96, generator=g).to(DEV)
    y = torch.randint(0, 10, (2,), generator=g).to(DEV)
    losses = [float(train_step(eng, crit, x, y, 0.01)) for _ in range(3)]
    print("b7 losses", losses)
    assert tuple(eng._sd_rows.shape) == (55, 2) and eng.sd_counter == 3
    assert all(torch.isfinite(v).all() for v in eng.named_params("flat").values())
    assert all(l == l and abs(l) < 1e4 for l in losses) and losses[-1] < losses[0]


def test_any_side_from_32_up_is_accepted_and_smaller_refused():
    eng = models.efficientnet_b0b(num_classes=10, device=DEV).engine
    for side in (32, 47):
        z = eng.forward(torch.randn(2, 3, side, side, device=DEV), training=False)
        assert tuple(z.shape) == (2, 10) and torch.isfinite(z).all()
    with pytest.raises(ValueError, match="at least 32"):
        eng.forward(torch.randn(2, 3, 31, 40, device=DEV), training=False)
    assert eng.algorithmic_bytes(2, 47) > eng.algorithmic_bytes(2, 46) > 0


# ---------------------------------------------------------------------------------------- driver

spec = importlib.util.spec_from_file_location("nbdt_main_family", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)


def test_driver_trains_a_scaled_variant_and_finds_the_shipped_imagenet_hierarchy(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    acc, _ = M.main("--arch efficientnet_b1 --dataset CIFAR10 --batch-size 32 --synthetic 64 --image-size 48 --lr 0.02 "
                    "--epochs 1 --stochastic-depth 0.1".split())
    assert 0.0 <= acc <= 100.0
    # no --hierarchy: the default induced-<arch> is the file the package ships for Imagenet1000
    acc, nbdt_acc = M.main("--arch efficientnet_b7b --dataset Imagenet1000 --batch-size 8 --synthetic 16 --image-size 64 "
                           "--eval --analysis SoftEmbeddedDecisionRules".split())
    assert 0.0 <= acc <= 100.0 and 0.0 <= nbdt_acc <= 100.0
