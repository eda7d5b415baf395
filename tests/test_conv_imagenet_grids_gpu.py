"""The existing conv, data-gradient and weight-gradient launches on the grids an ImageNet-style ResNet has at 224 x 224
input -- 56, 28, 14 and 7 pixels wide, where the halo-tile and K-split kernels do not apply (their tiles need a width that
divides 256 or 512 pixels) and the generic kernels run -- with batches that leave every pixel count ragged against the
256-pixel tile (3136, 1568, 588, 245).  No new kernel runs here: this guards the ground the ImageNet engines stand on.
Integer inputs and int64 references of tests/_resnet_conv_cases.py, descriptors as engine.Conv plans them (force=False),
every output bit for bit as in tests/test_conv_resnet_shapes_gpu.py.  The kernel each launch took is printed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_conv_cases as C  # noqa: E402

from nbdt import ops  # noqa: E402

DEV = "cuda:0"
IMAGENET_CASES = [
    # dense and strided 3x3, the strided 1x1 shortcut (BasicBlock trunks)
    (1, 56, 56, 64, 64, 3, 1), (2, 28, 28, 128, 128, 3, 1), (3, 14, 14, 256, 256, 3, 1), (5, 7, 7, 512, 512, 3, 1),
    (1, 56, 56, 64, 128, 3, 2), (3, 14, 14, 256, 512, 3, 2), (1, 56, 56, 64, 128, 1, 2),
    # Bottleneck 1x1 convs
    (1, 56, 56, 64, 256, 1, 1), (5, 7, 7, 2048, 512, 1, 1), (3, 14, 14, 512, 1024, 1, 2),
]
cases = pytest.mark.parametrize("case", IMAGENET_CASES, ids=[C.case_id(c) for c in IMAGENET_CASES])


def test_every_pixel_count_is_ragged_against_the_tile():
    counts = {B * (H // s) * (W // s) for B, H, W, _, _, _, s in IMAGENET_CASES} | {B * H * W for B, H, W, *_ in IMAGENET_CASES}
    assert counts == {3136, 1568, 588, 245, 784, 147} and all(n % 256 for n in counts)


def _padded_from(t):
    B, H, W, Cc = t.shape
    p = ops.padded(B, H, W, Cc, DEV)
    ops.interior(p).copy_(t.to(torch.bfloat16).to(DEV))
    return p


def _ring_zero(p):
    ring = torch.ones(p.shape[:3], dtype=torch.bool, device=p.device)
    ring[:, 1:-1, 1:-1] = False
    return not p[ring].float().abs().max().item()


def _equal_int(got, ref):
    return torch.equal(got.double().cpu(), ref.double())


_DEV = {}


def _dev(case):
    """Device copies of a case's integer inputs and weights, and engine.Conv's descriptors (built once, never written)."""
    if case not in _DEV:
        _, _, _, cin, cout, k, _ = case
        c = C.integer_case(case)
        wb = torch.empty(cout, k * k, cin, dtype=torch.bfloat16, device=DEV)
        wd = torch.empty(cin, k * k, cout, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(c["w"].float().contiguous().to(DEV), cout, k * k, cin, wb, wd)
        tiles = (0, 0)
        keep = None
        if C.dense3x3(case):
            keep = (ops.weight_tiles(wb), ops.weight_tiles(wd))
            tiles = (keep[0].data_ptr(), keep[1].data_ptr())
        _DEV[case] = dict(c, xp=_padded_from(c["x"]), gp=_padded_from(c["gy"]), rp=_padded_from(c["res"]), wb=wb, wd=wd,
                          keep=keep, descs=C.descs(case, tiles=tiles, force=False))
    return _DEV[case]


@cases
def test_integer_forward_residual_and_statistics_are_exact(case):
    B, H, W, cin, cout, k, stride = case
    Ho, Wo = H // stride, W // stride
    c = _dev(case)
    fwd = c["descs"][0]
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, c["xp"], c["wb"], out)
    print(f"[{C.case_id(case)}] forward: {ops.last_igemm_kernel()}")
    assert _equal_int(ops.interior(out), c["fwd"]) and _ring_zero(out)
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(fwd, c["xp"], c["wb"], out, residual=c["rp"])
    assert _equal_int(ops.interior(out), c["fwd"] + c["res"]) and _ring_zero(out)
    rows = (B * Ho * Wo + 255) // 256
    sums = torch.stack([c["fwd"].sum((0, 1, 2)), (c["fwd"] ** 2).sum((0, 1, 2))]).double()
    out, part = ops.padded(B, Ho, Wo, cout, DEV), torch.full((rows * 2 * cout,), float("nan"), device=DEV)
    ops.conv_igemm(fwd, c["xp"], c["wb"], out, bn_scratch=part)
    assert _equal_int(ops.interior(out), c["fwd"]) and _ring_zero(out)
    assert torch.equal(part.view(rows, 2, cout).double().sum(0).cpu(), sums)
    if C.pointwise(case):           # BottleneckEngine's routing of stride-1 1x1 launches
        out = ops.padded(B, Ho, Wo, cout, DEV)
        ops.conv_pw(fwd, c["xp"], c["wb"], out)
        assert ops.last_igemm_kernel() == "conv_pw_kernel"
        assert _equal_int(ops.interior(out), c["fwd"]) and _ring_zero(out)


@cases
def test_integer_data_gradient_plain_and_accumulating_is_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = _dev(case)
    _, plain, acc, _ = c["descs"]
    for descs, base in ((plain, None), (acc, c["base"])):
        if descs is None:       # a strided 1x1 data gradient writes every other pixel: accumulating only
            continue
        ref = c["dgrad"] if base is None else c["dgrad"] + base
        gx = ops.padded(B, H, W, cin, DEV) if base is None else _padded_from(base)
        if len(descs) > 1:      # the four parity classes in one grid, as engine.Conv.backward_data issues them
            ops.conv_igemm_multi(descs, c["gp"], c["wd"], gx)
        else:
            ops.conv_igemm(descs[0], c["gp"], c["wd"], gx)
        print(f"[{C.case_id(case)}] data gradient (accumulate {base is not None}): {ops.last_igemm_kernel()}")
        assert _equal_int(ops.interior(gx), ref) and _ring_zero(gx), base is not None
        if C.pointwise(case):
            gx = ops.padded(B, H, W, cin, DEV) if base is None else _padded_from(base)
            ops.conv_pw(descs[0], c["gp"], c["wd"], gx)
            assert ops.last_igemm_kernel() == "conv_pw_kernel"
            assert _equal_int(ops.interior(gx), ref) and _ring_zero(gx), ("conv_pw", base is not None)


@cases
def test_integer_weight_gradient_is_exact_in_both_modes(case):
    B, H, W, cin, cout, k, stride = case
    c = _dev(case)
    wg = c["descs"][3]
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros(cout, k * k, cin, dtype=torch.float32, device=DEV)
            ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
            once = dw.clone()
            ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
        finally:
            ops.set_deterministic(False)
        print(f"[{C.case_id(case)}] weight gradient (deterministic {det}): {ops.last_wgrad_kernel()}")
        assert _equal_int(once, c["dw"]), det
        assert _equal_int(dw, 2 * c["dw"]), det
