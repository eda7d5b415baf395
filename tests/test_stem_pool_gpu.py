"""The two new ops of the ImageNet-style stem (csrc/stem_pool.hip) on the MI355X, exactly:

  * nbdt_stem_patches against F.unfold: every border and corner tap, the zero channels, the untouched ring, both storages;
  * nbdt_maxpool3x3s2_fwd / _bwd against F.max_pool2d and its autograd on small integers (frequent ties, all-negative and
    constant tensors): values, window positions, gradient, ring, reproducibility;
  * the stem as a whole -- patches + the existing 1x1 launches (ops.conv_igemm, ops.conv_wgrad) -- against F.conv2d with a
    7x7 / 2 / 3 kernel on integers, bit for bit."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402

DEV = "cuda:0"
SENTINEL = 1.5          # exactly representable in bf16


def _ring(p):
    ring = torch.ones(p.shape[:3], dtype=torch.bool, device=p.device)
    ring[:, 1:-1, 1:-1] = False
    return p[ring]


def _ring_is(p, value=SENTINEL):
    r = _ring(p)
    return torch.equal(r, torch.full_like(r, value))


def _ref_patches(x, k, stride):
    """[B, Ho, Wo, 3*k*k] in (r, s, ci) channel order from F.unfold's (ci, r, s)."""
    B, _, H, W = x.shape
    Ho, Wo = H // stride, W // stride
    u = F.unfold(x, k, padding=k // 2, stride=stride)                     # [B, 3*k*k, Ho*Wo]
    return u.view(B, 3, k, k, Ho, Wo).permute(0, 4, 5, 2, 3, 1).reshape(B, Ho, Wo, k * k * 3).contiguous()


@pytest.mark.parametrize("B,H,W,k,stride,cpad", [(3, 16, 24, 7, 2, 160), (2, 32, 32, 7, 2, 160), (2, 8, 12, 3, 1, 32),
                                                (1, 10, 6, 5, 2, 96)])
def test_patches_equal_unfold(B, H, W, k, stride, cpad):
    g = torch.Generator().manual_seed(H * W + k)
    x = torch.randn(B, 3, H, W, generator=g)
    ref = _ref_patches(x, k, stride)
    n, Ho, Wo = 3 * k * k, H // stride, W // stride
    for dtype in (torch.bfloat16, torch.float32):
        out = torch.full((B, Ho + 2, Wo + 2, cpad), SENTINEL, dtype=dtype, device=DEV)
        ops.stem_patches(x.to(DEV), out, k, stride)
        got = ops.interior(out).cpu()
        assert torch.equal(got[..., :n], ref.to(dtype)), dtype
        assert torch.equal(got[..., n:], torch.zeros(B, Ho, Wo, cpad - n, dtype=dtype)), dtype
        assert _ring_is(out), dtype


def test_patches_refuse_what_they_do_not_cover():
    from nbdt._C import NBDTHipError
    x = torch.zeros(1, 3, 15, 16, device=DEV)
    with pytest.raises(NBDTHipError, match="divisible"):
        ops.stem_patches(x, ops.padded(1, 7, 8, 160, DEV), 7, 2)
    with pytest.raises(NBDTHipError, match="cpad"):
        ops.stem_patches(torch.zeros(1, 3, 16, 16, device=DEV), ops.padded(1, 8, 8, 128, DEV), 7, 2)


POOL_SHAPES = [(3, 8, 12, 32), (2, 16, 16, 64), (1, 6, 6, 8)]


def _pool_inputs(B, H, W, C, kind):
    g = torch.Generator().manual_seed(B * H + W + C)
    if kind == "negative":
        return -torch.randint(1, 4, (B, H, W, C), generator=g).float()
    if kind == "constant":
        return torch.full((B, H, W, C), 2.0)
    return torch.randint(-3, 4, (B, H, W, C), generator=g).float()


def _padded_from(t, dtype, halo=0.0):
    B, H, W, C = t.shape
    p = torch.full((B, H + 2, W + 2, C), halo, dtype=dtype, device=DEV)
    ops.interior(p).copy_(t.to(dtype).to(DEV))
    return p


def _ref_pool(x_nhwc):
    """(values [B,Ho,Wo,C], window positions 3*dy+dx, autograd function) of the CPU op."""
    x = x_nhwc.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    W = x.shape[3]
    iy, ix = flat // W, flat % W
    Ho, Wo = y.shape[2], y.shape[3]
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, Wo)
    pos = 3 * (iy - (2 * oy - 1)) + (ix - (2 * ox - 1))
    return x, y, pos.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("kind", ["ties", "negative", "constant"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_maxpool_forward_and_backward_equal_torch(shape, kind, dtype):
    B, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    xi = _pool_inputs(B, H, W, C, kind)
    x_ref, y_ref, pos_ref = _ref_pool(xi)
    # the ring holds +100: a kernel that read it instead of deciding by bounds would return it
    xp = _padded_from(xi, dtype, halo=100.0)
    y = torch.full((B, Ho + 2, Wo + 2, C), SENTINEL, dtype=dtype, device=DEV)
    idx = torch.full((B, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xp, y, idx)
    want = y_ref.detach().permute(0, 2, 3, 1)
    assert torch.equal(ops.interior(y).float().cpu(), want)
    assert _ring_is(y)
    assert torch.equal(idx.cpu().long(), pos_ref)
    if kind == "negative":
        assert ops.interior(y).float().max().item() < 0
    # inference: no index buffer, the same values
    y2 = torch.full_like(y, SENTINEL)
    ops.maxpool_fwd(xp, y2, None)
    assert torch.equal(y2, y)
    # backward
    g = torch.Generator().manual_seed(7)
    gy = torch.randint(-2, 3, (B, Ho, Wo, C), generator=g).float()
    y_ref.backward(gy.permute(0, 3, 1, 2))
    gx_ref = x_ref.grad.permute(0, 2, 3, 1)
    gyp = _padded_from(gy, dtype, halo=100.0)
    runs = []
    for _ in range(2):
        gx = torch.full((B, H + 2, W + 2, C), float("nan"), dtype=dtype, device=DEV)
        ops.maxpool_bwd(gyp, idx, gx)
        runs.append(gx)
    got = ops.interior(runs[0]).float().cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, gx_ref)
    assert torch.isnan(_ring(runs[0]).float()).all()                      # the ring was not written
    assert torch.equal(ops.interior(runs[0]), ops.interior(runs[1]))      # no atomics: the same bits


def test_maxpool_propagates_nan():
    x = torch.zeros(1, 4, 4, 8)
    x[0, 1, 1, 3] = float("nan")
    y = ops.padded(1, 2, 2, 8, DEV)
    idx = torch.zeros(1, 2, 2, 8, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(_padded_from(x, torch.bfloat16), y, idx)
    ref, flat = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    got = ops.interior(y).float().cpu().permute(0, 3, 1, 2)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.isnan(got).sum().item() == 4
    assert torch.equal(got.nan_to_num(7.0), ref.nan_to_num(7.0))


def test_stem_composite_is_the_7x7_convolution_bit_for_bit():
    """patches + the existing 1x1 forward and weight-gradient launches == Conv2d(3, 64, 7, 2, 3) and its weight gradient on
    integers (image in [-2, 2], weights in {-1, 0, 1}): every partial sum is an integer far below 2^24, so fp32
    accumulation is exact whatever its order, and the one rounding left is the epilogue's fp32 -> bf16 (|sum| can reach
    294, above the 256 up to which every integer is a bf16), which the float64 reference takes with .to(bfloat16)."""
    B, H, W = 2, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-2, 3, (B, 3, H, W), generator=g).float()
    w = torch.randint(-1, 2, (64, 3, 7, 7), generator=g).float()
    Ho, Wo = H // 2, W // 2
    patches = ops.padded(B, Ho, Wo, 160, DEV)
    ops.stem_patches(x.to(DEV), patches, 7, 2)
    master = torch.zeros(64, 1, 160)
    master[:, 0, :147] = w.permute(0, 2, 3, 1).reshape(64, 147)         # (r, s, ci)
    wb = master.to(torch.bfloat16).to(DEV)
    fwd = ops.conv_fwd_desc(B, Ho, Wo, 160, 64, 1, 1)
    out = ops.padded(B, Ho, Wo, 64, DEV)
    ops.conv_igemm(fwd, patches, wb, out)
    ref = F.conv2d(x.double(), w.double(), None, 2, 3).permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(ops.interior(out).cpu(), ref)
    assert ops.interior(out).float().abs().max().item() > 16            # (not a vacuous comparison)
    # weight gradient: integer gy in [-2, 2]; |dw| <= 2 * 2 * B * Ho * Wo = 8192 < 2^24, exact in fp32
    gy = torch.randint(-2, 3, (B, Ho, Wo, 64), generator=g).float()
    gyp = ops.padded(B, Ho, Wo, 64, DEV)
    ops.interior(gyp).copy_(gy.to(torch.bfloat16).to(DEV))
    dw = torch.zeros(64, 1, 160, device=DEV)
    ops.conv_wgrad(ops.conv_wgrad_desc(B, Ho, Wo, 160, 64, 1, 1), patches, gyp, dw)
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), gy.permute(0, 3, 1, 2).double(), 2, 3)
    got = dw.cpu()[:, 0, :147].view(64, 7, 7, 3).permute(0, 3, 1, 2).double()
    assert torch.equal(got, dw_ref)
    assert torch.equal(dw.cpu()[:, 0, 147:], torch.zeros(64, 13))
