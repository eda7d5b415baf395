"""Per-op parity of the conv, data-gradient and weight-gradient kernels at the shapes ResNetEngine and BottleneckEngine
launch (tests/_resnet_conv_cases.py: 64 .. 2048 channels on 32x32 .. 4x4 grids), each on the kernel the engine's launch at
128 images takes -- the name is asserted on every launch.

  * test_case_table_covers_what_the_engines_launch: no launch of a training step of either engine is outside the table;
  * integer inputs (exactly representable results, tests/test_conv_resnet_cases.py): every output bit for bit the int64
    convolution, whatever the summation order, K split or atomics -- a dropped K slice, a wrong tap or a lost partial sum
    cannot hide in a tolerance;
  * bf16-rounded real inputs against float64 with the bounds of tests/test_backbone_gpu.py: the rounding of the epilogues."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_conv_cases as C  # noqa: E402
from _resnet_conv_cases import RESNET_CASES  # noqa: E402
from test_backbone_gpu import _check_border_zero, _close_bf16, _rand_act, _rand_weight  # noqa: E402

from nbdt import engine as E  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

DEV = "cuda:0"
SENTINEL = 1.5          # exactly representable in bf16
IDS = [C.case_id(c) for c in RESNET_CASES]
PW_CASES = [c for c in RESNET_CASES if C.pointwise(c)]
KSPLIT_CASE = (16, 4, 4, 512, 512, 3, 1)
cases = pytest.mark.parametrize("case", RESNET_CASES, ids=IDS)


def _padded_from(t, halo=0.0):
    """Padded bf16 device buffer with interior t ([B,H,W,C] on the host, values that are bf16s) and `halo` in the ring."""
    B, H, W, Cc = t.shape
    p = torch.full((B, H + 2, W + 2, Cc), halo, dtype=torch.bfloat16, device=DEV)
    ops.interior(p).copy_(t.to(torch.bfloat16).to(DEV))
    return p


def _sentinel_out(B, H, W, Cc):
    return torch.full((B, H + 2, W + 2, Cc), SENTINEL, dtype=torch.bfloat16, device=DEV)


def _halo_untouched(p, value=SENTINEL):
    ring = torch.ones(p.shape[:3], dtype=torch.bool, device=p.device)
    ring[:, 1:-1, 1:-1] = False
    return torch.equal(p[ring], torch.full_like(p[ring], value))


class _Weights:
    """Device copies of one [cout][taps][cin] fp32 master: bf16, the data-gradient transpose, and (dense 3x3) the DMA-ordered
    tiles of both -- what _Engine.finalize builds; descs() hands engine.Conv's descriptors with the tiles attached."""

    def __init__(self, case, master):
        _, _, _, cin, cout, k, _ = case
        self.case = case
        self.wb = torch.empty(cout, k * k, cin, dtype=torch.bfloat16, device=DEV)
        self.wd = torch.empty(cin, k * k, cout, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(master.float().contiguous().to(DEV), cout, k * k, cin, self.wb, self.wd)
        self.wt = ops.weight_tiles(self.wb) if C.dense3x3(case) else None
        self.wdt = ops.weight_tiles(self.wd) if C.dense3x3(case) else None

    def descs(self):
        tiles = (self.wt.data_ptr(), self.wdt.data_ptr()) if self.wt is not None else (0, 0)
        return C.descs(self.case, tiles=tiles)


def _equal_int(got, ref):
    """A device tensor of floats equals an int64 reference, element for element."""
    return torch.equal(got.double().cpu(), ref.double())


def _folded(part, rows, cout):
    return part.view(rows, 2, cout).double().sum(0).cpu()


# ------------------------------------------------------------------------------------------------------------------------
# 1. the case table against the engines

def test_case_table_covers_what_the_engines_launch():
    """One training step of ResNetEngine and of BottleneckEngine (one block per stage) at 2 images with every conv entry
    point wrapped: each descriptor's (cin, cout, ntaps, strided, gh, gw) is a launch of a RESNET_CASES entry."""
    conv_keys, wgrad_keys = C.table_keys()
    seen_conv, seen_wgrad = [], []
    names = ("conv_igemm", "conv_pw", "conv_igemm_bnbwd", "conv_igemm_multi", "conv_wgrad")
    real = {n: getattr(ops, n) for n in names}

    def spy(name):
        def f(desc, *a, **k):
            if name == "conv_wgrad":
                seen_wgrad.append(C.wgrad_key(desc))
            else:
                seen_conv.extend(C.conv_key(d) for d in (desc if name == "conv_igemm_multi" else [desc]))
            return real[name](desc, *a, **k)
        return f

    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(2, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (2,), generator=g).to(DEV)
    per_engine = []
    for n in names:
        setattr(ops, n, spy(n))
    try:
        for make in (lambda: E.ResNetEngine(10, device=DEV), lambda: E.BottleneckEngine(10, num_blocks=(1, 1, 1, 1), device=DEV)):
            eng = make()
            eng.zero_grad()
            z = eng.forward(x, training=True)
            _, gz = crit.loss_and_grad(z, y)
            eng.backward(gz)
            torch.cuda.synchronize()
            per_engine.append((len(seen_conv), len(seen_wgrad)))
    finally:
        for n in names:
            setattr(ops, n, real[n])
    assert all(n_conv > 0 and n_wgrad > 0 for n_conv, n_wgrad in per_engine) and per_engine[1] > per_engine[0]
    assert not set(seen_conv) - conv_keys, sorted(set(seen_conv) - conv_keys)
    assert not set(seen_wgrad) - wgrad_keys, sorted(set(seen_wgrad) - wgrad_keys)
    # ... and the step reaches the table's widest and longest launches
    assert (512, 512, 9, False, 4, 4) in seen_conv and (512, 2048, 1, False, 4, 4) in seen_conv
    assert (1024, 2048, 1, True, 4, 4) in seen_wgrad and (512, 512, 9, False, 4, 4) in seen_wgrad


# ------------------------------------------------------------------------------------------------------------------------
# 2. integer inputs: bit for bit

_INT_DEV = {}


def _int_dev(case):
    """Device copies of the integer inputs of a case (built once, never written)."""
    if case not in _INT_DEV:
        c = C.integer_case(case)
        _INT_DEV[case] = dict(c, xp=_padded_from(c["x"]), gp=_padded_from(c["gy"]), rp=_padded_from(c["res"]),
                              wts=_Weights(case, c["w"]))
    return _INT_DEV[case]


@cases
def test_integer_forward_residual_and_statistics_are_exact(case):
    B, H, W, cin, cout, k, stride = case
    Ho, Wo = H // stride, W // stride
    c = _int_dev(case)
    wts, xp = c["wts"], c["xp"]
    name = C.kernel_names(case)[0]
    fwd = wts.descs()[0]
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, xp, wts.wb, out)
    assert ops.last_igemm_kernel() == name
    assert _equal_int(ops.interior(out), c["fwd"])
    _check_border_zero(out)
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, xp, wts.wb, out, residual=c["rp"])
    assert ops.last_igemm_kernel() == name
    assert _equal_int(ops.interior(out), c["fwd"] + c["res"])
    _check_border_zero(out)
    # statistics epilogue: one [2][cout] row of partial sums per 256 output pixels, all integers
    rows = (B * Ho * Wo + 255) // 256
    sums = torch.stack([c["fwd"].sum((0, 1, 2)), (c["fwd"] ** 2).sum((0, 1, 2))]).double()
    out, part = ops.padded(B, Ho, Wo, cout, DEV), torch.full((rows * 2 * cout,), float("nan"), device=DEV)
    ops.conv_igemm(fwd, xp, wts.wb, out, bn_scratch=part)
    assert ops.last_igemm_kernel() == name
    assert _equal_int(ops.interior(out), c["fwd"])
    assert torch.equal(_folded(part, rows, cout), sums)
    _check_border_zero(out)
    if not C.pointwise(case):
        return
    # the pointwise GEMM kernel (BottleneckEngine.pointwise): the halo of the input is never read, that of the output
    # never written; statistics launches from Conv.PW_STATS_MIN_CIN input channels on
    xn = _padded_from(c["x"], float("nan"))
    out = _sentinel_out(B, Ho, Wo, cout)
    ops.conv_pw(fwd, xn, wts.wb, out)
    assert ops.last_igemm_kernel() == "conv_pw_kernel"
    assert _equal_int(ops.interior(out), c["fwd"]) and _halo_untouched(out)
    if cin >= E.Conv.PW_STATS_MIN_CIN:
        out, part = _sentinel_out(B, Ho, Wo, cout), torch.full((rows * 2 * cout,), float("nan"), device=DEV)
        ops.conv_pw(fwd, xn, wts.wb, out, bn_scratch=part)
        assert ops.last_igemm_kernel() == "conv_pw_kernel"
        assert _equal_int(ops.interior(out), c["fwd"]) and _halo_untouched(out)
        assert torch.equal(_folded(part, rows, cout), sums)


def test_pointwise_statistics_cases_exist():
    assert sorted(c[3] for c in PW_CASES if c[3] >= E.Conv.PW_STATS_MIN_CIN) == [1024, 1024, 2048]


@cases
def test_integer_data_gradient_plain_and_accumulating_is_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = _int_dev(case)
    wts, gp = c["wts"], c["gp"]
    _, name, _ = C.kernel_names(case)
    one = "conv_igemm_dma_kernel" if name == "conv_igemm_dma_multi_kernel" else name      # a descriptor on its own
    _, plain, acc, _ = wts.descs()
    assert (plain is None) == (k == 1 and stride == 2) and len(acc) == (4 if (k, stride) == (3, 2) else 1)
    for descs, base in ((plain, None), (acc, c["base"])):
        if descs is None:       # a strided 1x1 data gradient writes every other pixel: accumulating only
            continue
        ref = c["dgrad"] if base is None else c["dgrad"] + base
        fresh = lambda: ops.padded(B, H, W, cin, DEV) if base is None else _padded_from(base)      # noqa: E731
        gx = fresh()
        for d in descs:
            ops.conv_igemm(d, gp, wts.wd, gx)
            assert ops.last_igemm_kernel() == one
        assert _equal_int(ops.interior(gx), ref), ("conv_igemm", base is not None)
        _check_border_zero(gx)
        if len(descs) == 4:     # the four parity classes in one grid, as engine.Conv.backward_data issues them
            gx = fresh()
            ops.conv_igemm_multi(descs, gp, wts.wd, gx)
            assert ops.last_igemm_kernel() == name
            assert _equal_int(ops.interior(gx), ref), ("conv_igemm_multi", base is not None)
            _check_border_zero(gx)
        if C.pointwise(case):
            gn = _padded_from(c["gy"], float("nan"))
            gx = _sentinel_out(B, H, W, cin)
            if base is not None:
                ops.interior(gx).copy_(base.to(torch.bfloat16).to(DEV))
            ops.conv_pw(descs[0], gn, wts.wd, gx)
            assert ops.last_igemm_kernel() == "conv_pw_kernel"
            assert _equal_int(ops.interior(gx), ref) and _halo_untouched(gx), ("conv_pw", base is not None)


@cases
def test_integer_weight_gradient_is_exact_in_both_modes(case):
    B, H, W, cin, cout, k, stride = case
    c = _int_dev(case)
    name = C.kernel_names(case)[2]
    wg = c["wts"].descs()[3]
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros(cout, k * k, cin, dtype=torch.float32, device=DEV)
            ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
            assert ops.last_wgrad_kernel() == name
            once = dw.clone()
            ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
            assert ops.last_wgrad_kernel() == name
        finally:
            ops.set_deterministic(False)
        assert _equal_int(once, c["dw"]), det
        assert _equal_int(dw, 2 * c["dw"]), det


# ------------------------------------------------------------------------------------------------------------------------
# 3. bf16-rounded real inputs against float64

_REAL = {}


def _real(case):
    """Random inputs with the scaling of tests/test_backbone_gpu.py (activations N(0, 1), weights N(0, 1 / fan-in), all
    rounded to bf16) and the float64 convolutions of those values; built once per case."""
    if case not in _REAL:
        B, H, W, cin, cout, k, stride = case
        Ho, Wo = H // stride, W // stride
        xf, xp = _rand_act(B, H, W, cin, seed=1)
        w_oihw, w_int = _rand_weight(cout, cin, k, seed=2)
        rf, rp = _rand_act(B, Ho, Wo, cout, seed=3)
        gf, gp = _rand_act(B, Ho, Wo, cout, seed=4)
        bf, _ = _rand_act(B, H, W, cin, seed=5)
        fwd, dgrad, dw = C.conv_refs(xf, w_oihw, gf, stride)
        _REAL[case] = dict(xp=xp, rp=rp, gp=gp, rf=rf.double(), bf=bf, fwd=fwd, dgrad=dgrad, dw=dw,
                           wts=_Weights(case, w_int))
    return _REAL[case]


@cases
def test_real_forward_and_folded_batchnorm_epilogue(case):
    """Forward, forward + residual, and nbdt_conv_igemm_affine -- act(conv * scale + shift [+ residual]): the residual is
    added BEFORE the activation (conv_common.h) -- without / with ReLU and residual, against float64."""
    B, H, W, cin, cout, k, stride = case
    Ho, Wo = H // stride, W // stride
    c = _real(case)
    wts, xp = c["wts"], c["xp"]
    name = C.kernel_names(case)[0]
    fwd = wts.descs()[0]
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, xp, wts.wb, out)
    assert ops.last_igemm_kernel() == name
    _close_bf16(ops.interior(out), c["fwd"], "forward")
    _check_border_zero(out)
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, xp, wts.wb, out, residual=c["rp"])
    assert ops.last_igemm_kernel() == name
    _close_bf16(ops.interior(out), c["fwd"] + c["rf"], "forward + residual")
    if C.pointwise(case):
        out = _sentinel_out(B, Ho, Wo, cout)
        ops.conv_pw(fwd, xp, wts.wb, out)
        assert ops.last_igemm_kernel() == "conv_pw_kernel"
        _close_bf16(ops.interior(out), c["fwd"], "pointwise forward")
        assert _halo_untouched(out)
    g = torch.Generator().manual_seed(cin + cout)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    affine = c["fwd"] * scale.double() + shift.double()
    for act in (0, 1):
        for res in (False, True):
            ref = affine + c["rf"] if res else affine
            ref = torch.relu(ref) if act == 1 else ref
            out = ops.padded(B, Ho, Wo, cout, DEV)
            ops.conv_igemm_affine(fwd, xp, wts.wb, out, scale.to(DEV), shift.to(DEV), act, c["rp"] if res else None)
            assert ops.last_igemm_kernel() == name
            _close_bf16(ops.interior(out), ref, f"affine epilogue, act {act}, residual {res}")
            _check_border_zero(out)


@cases
def test_real_data_gradient_plain_and_accumulating(case):
    B, H, W, cin, cout, k, stride = case
    c = _real(case)
    wts, gp = c["wts"], c["gp"]
    _, name, _ = C.kernel_names(case)
    _, plain, acc, _ = wts.descs()
    for descs, base in ((plain, None), (acc, c["bf"])):
        if descs is None:
            continue
        ref = c["dgrad"] if base is None else c["dgrad"] + base.double()
        gx = ops.padded(B, H, W, cin, DEV) if base is None else _padded_from(base)
        if len(descs) == 4:
            ops.conv_igemm_multi(descs, gp, wts.wd, gx)
        else:
            ops.conv_igemm(descs[0], gp, wts.wd, gx)
        assert ops.last_igemm_kernel() == name
        _close_bf16(ops.interior(gx), ref, f"data gradient, accumulate {base is not None}")
        _check_border_zero(gx)
        if C.pointwise(case):
            gx = _sentinel_out(B, H, W, cin)
            if base is not None:
                ops.interior(gx).copy_(base.to(torch.bfloat16).to(DEV))
            ops.conv_pw(descs[0], gp, wts.wd, gx)
            assert ops.last_igemm_kernel() == "conv_pw_kernel"
            _close_bf16(ops.interior(gx), ref, f"pointwise data gradient, accumulate {base is not None}")
            assert _halo_untouched(gx)


@cases
def test_real_weight_gradient(case):
    B, H, W, cin, cout, k, stride = case
    c = _real(case)
    dw = torch.zeros(cout, k * k, cin, dtype=torch.float32, device=DEV)
    ops.conv_wgrad(c["wts"].descs()[3], c["xp"], c["gp"], dw)
    assert ops.last_wgrad_kernel() == C.kernel_names(case)[2]
    ref = c["dw"].numpy()
    np.testing.assert_allclose(dw.cpu().double().numpy(), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())


def test_automatic_k_split_is_reproducible_and_one_ulp_from_the_unsplit_launch():
    """512 -> 512 at 4x4: conv_ksplit_rule splits the 144 K steps of the one half tile four ways, forward (wide_tile = 1)
    and data gradient (wide_tile = 0).  Three launches leave the same bits, whichever block of a tile comes last; the
    same descriptor with ksplit = 1 (another summation order) is within one bf16 ulp -- the bound
    test_pingpong_kernel_forced_on_small_shapes holds the forced split to."""
    case = KSPLIT_CASE
    assert case in RESNET_CASES
    B, H, W, cin, cout, k, stride = case
    c = _real(case)
    wts = c["wts"]
    for what, src, wgt, ref in (("forward", c["xp"], wts.wb, c["fwd"]), ("data gradient", c["gp"], wts.wd, c["dgrad"])):
        def desc():
            fwd, plain, _, _ = wts.descs()
            return fwd if what == "forward" else plain[0]
        d = desc()
        assert d.ksplit == 0 and d.wide_tile == (1 if what == "forward" else 0)
        assert ops.conv_plan(d) == (C.HALF, 4)
        outs = []
        for _ in range(3):
            o = ops.padded(B, H, W, d.cout, DEV)
            ops.conv_igemm(d, src, wgt, o)
            assert ops.last_igemm_kernel() == "conv3x3_pp_kernel/half/ksplit", what
            outs.append(o)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), what
        _close_bf16(ops.interior(outs[0]), ref, what)
        d1 = desc()
        d1.ksplit = 1
        unsplit = ops.padded(B, H, W, d.cout, DEV)
        ops.conv_igemm(d1, src, wgt, unsplit)
        assert ops.last_igemm_kernel() == "conv3x3_pp_kernel/half", what
        a, b = ops.interior(outs[0]).float(), ops.interior(unsplit).float()
        assert ((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 1e-4).all(), what
