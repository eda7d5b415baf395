"""nbdt_conv_pw (csrc/conv_pw.hip): stride-1 1x1 convolutions as a GEMM, forward and data gradient, against
F.conv2d / F.conv_transpose2d on the same bf16-rounded inputs, with the bound the other conv kernels are held to
(tests/test_backbone_gpu.py: err <= 2^-7 |ref| + 2e-2).

Cout tile of a launch (pw_cout_tile in conv_pw.hip): the widest of 5 / 4 / 3 / 2 / 1 x 32 channels that divides cout and
still gives 256 blocks, else the narrowest (statistics launches: not below 64 channels when 64 divides cout).  So every
small shape below runs the NARROW form -- 2048 -> 512 at 4x4 does from batch 1 up to batch 1023 (M = 16368: 64 pixel tiles
x 4 cout tiles of 128 = 256 blocks first at batch 1024) -- and the wide form is reached here through a shape with few
channels and many pixels (test_tile_width_follows_the_grid: the same switch at 255 / 256 pixel tiles)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402
from nbdt._C import NBDTHipError  # noqa: E402

DEV = "cuda:0"
SENTINEL = 1.5          # exactly representable in bf16

SHAPES = [
    # B, H, W, cin, cout
    (2, 8, 8, 64, 256),      # less than one 256-pixel tile
    (5, 8, 8, 256, 64),      # M = 320: one full tile and a ragged one
    (3, 6, 6, 96, 96),       # odd pixel count; N not a multiple of 64
    (1, 4, 4, 2048, 512),    # long K, M = 16; the few-tile regime (narrow cout tiles from batch 1)
    (17, 4, 4, 2048, 512),   # the same with two pixel tiles, the second ragged (M = 272)
    (2, 8, 8, 32, 160),      # the 160-channel cout tile (NT = 5): two trips of the statistics pass, its own LDS scratch
    (3, 6, 6, 64, 32),       # a single 32-channel cout tile (NT = 1), statistics included
]


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _padded_from(x_nhwc, halo):
    """Padded device buffer whose interior is x (bf16) and whose halo ring holds `halo`."""
    B, H, W, C = x_nhwc.shape
    p = torch.full((B, H + 2, W + 2, C), halo, dtype=torch.bfloat16, device=DEV)
    ops.interior(p).copy_(x_nhwc.to(torch.bfloat16).to(DEV))
    return p


def _halo_untouched(p, value):
    ring = torch.ones(p.shape[:3], dtype=torch.bool, device=p.device)
    ring[:, 1:-1, 1:-1] = False
    return torch.equal(p[ring], torch.full_like(p[ring], value))


_CASES = {}


def _case(B, H, W, cin, cout):
    """Inputs and CPU references of one shape, computed once and shared (never modified)."""
    key = (B, H, W, cin, cout)
    if key not in _CASES:
        g = torch.Generator().manual_seed(cin * 7 + cout * 3 + B)
        x = _bf16(torch.randn(B, H, W, cin, generator=g))
        gy = _bf16(torch.randn(B, H, W, cout, generator=g))
        w = _bf16(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        base_y = _bf16(torch.randn(B, H, W, cout, generator=g))
        base_x = _bf16(torch.randn(B, H, W, cin, generator=g))
        w4 = w[:, :, None, None]
        fwd = F.conv2d(x.permute(0, 3, 1, 2), w4).permute(0, 2, 3, 1).contiguous()
        dgrad = F.conv_transpose2d(gy.permute(0, 3, 1, 2), w4).permute(0, 2, 3, 1).contiguous()
        wb = torch.empty(cout, 1, cin, dtype=torch.bfloat16, device=DEV)
        wd = torch.empty(cin, 1, cout, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(w.view(cout, 1, cin).to(DEV), cout, 1, cin, wb, wd)
        _CASES[key] = dict(x=x, gy=gy, base_y=base_y, base_x=base_x, fwd=fwd, dgrad=dgrad, wb=wb, wd=wd)
    return _CASES[key]


def _within(got, ref):
    err = (got - ref).abs()
    assert (err <= 2 ** -7 * ref.abs() + 2e-2).all(), err.max().item()


@pytest.mark.parametrize("direction", ["forward", "dgrad"])
@pytest.mark.parametrize("B,H,W,cin,cout", SHAPES)
def test_matches_conv2d_plain_and_accumulating(B, H, W, cin, cout, direction):
    c = _case(B, H, W, cin, cout)
    if direction == "forward":
        desc = lambda acc: _acc(ops.conv_fwd_desc(B, H, W, cin, cout, 1, 1), acc)       # noqa: E731
        src, wgt, ref, base, C = c["x"], c["wb"], c["fwd"], c["base_y"], cout
    else:
        desc = lambda acc: ops.conv_dgrad_descs(B, H, W, cin, cout, 1, 1, accumulate=acc)[0]      # noqa: E731
        src, wgt, ref, base, C = c["gy"], c["wd"], c["dgrad"], c["base_x"], cin
    inp = _padded_from(src, float("nan"))            # the halo of `in` is never read
    # plain
    out = torch.full((B, H + 2, W + 2, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.conv_pw(desc(False), inp, wgt, out)
    assert ops.last_igemm_kernel() == "conv_pw_kernel"
    got = ops.interior(out).float().cpu()
    assert torch.isfinite(got).all()
    _within(got, ref)
    assert _halo_untouched(out, SENTINEL)            # the halo ring of `out` keeps its bytes
    # accumulate: out pre-filled with random bf16; fp32 add, one rounding
    out = _padded_from(base, SENTINEL)
    ops.conv_pw(desc(True), inp, wgt, out)
    got = ops.interior(out).float().cpu()
    assert torch.isfinite(got).all()
    _within(got, _bf16(base + ref))
    assert _halo_untouched(out, SENTINEL)


def _acc(d, acc):
    d.accumulate = 1 if acc else 0
    return d


@pytest.mark.parametrize("B,H,W,cin,cout", SHAPES)
def test_statistics_epilogue(B, H, W, cin, cout):
    c = _case(B, H, W, cin, cout)
    d = ops.conv_fwd_desc(B, H, W, cin, cout, 1, 1)
    inp = _padded_from(c["x"], float("nan"))
    rows = (B * H * W + 255) // 256
    outs, parts = [], []
    for _ in range(2):
        out = ops.padded(B, H, W, cout, DEV)
        part = torch.full(((rows + 1) * 2 * cout,), float("nan"), device=DEV)      # one row more than the launch owns
        ops.conv_pw(d, inp, c["wb"], out, bn_scratch=part)
        outs.append(out)
        parts.append(part)
    out, part = outs[0], parts[0]
    plain = ops.padded(B, H, W, cout, DEV)
    ops.conv_pw(d, inp, c["wb"], plain)
    assert torch.equal(out, plain)
    # run-to-run identical bits, statistics included (deterministic mode is off)
    assert not ops.is_deterministic()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(parts[0][:rows * 2 * cout], parts[1][:rows * 2 * cout])
    # rows past ceil(M / 256) are not written
    assert torch.isnan(part[rows * 2 * cout:]).all()
    # folding the partial rows == sums of the returned bf16 tensor
    folded = part[:rows * 2 * cout].view(rows, 2, cout).double().sum(0).cpu()
    v = ops.interior(out).double().cpu().reshape(-1, cout)
    np.testing.assert_allclose(folded[0].numpy(), v.sum(0).numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(folded[1].numpy(), (v * v).sum(0).numpy(), rtol=1e-4)
    # bn_finalize on the partials == bn_stats on the same tensor
    mean_f, rstd_f, mean_r, rstd_r = (torch.empty(cout, device=DEV) for _ in range(4))
    ops.bn_finalize(out, part, mean_f, rstd_f)
    ops.bn_stats(out, torch.zeros(ops.BN_SLOTS * 2 * cout, device=DEV), mean_r, rstd_r)
    np.testing.assert_allclose(mean_f.cpu().numpy(), mean_r.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rstd_f.cpu().numpy(), rstd_r.cpu().numpy(), rtol=1e-4)
    with pytest.raises(NBDTHipError, match="plain outputs"):
        ops.conv_pw(_acc(ops.conv_fwd_desc(B, H, W, cin, cout, 1, 1), True), inp, c["wb"], out, bn_scratch=part)


@pytest.mark.parametrize("B,H,W,cin,cout", SHAPES)
def test_routing_and_agreement_with_the_first_generation_kernel(B, H, W, cin, cout):
    c = _case(B, H, W, cin, cout)
    inp = _padded_from(c["x"], 0.0)
    d = ops.conv_fwd_desc(B, H, W, cin, cout, 1, 1)
    a, b = ops.padded(B, H, W, cout, DEV), ops.padded(B, H, W, cout, DEV)
    ops.conv_pw(d, inp, c["wb"], a)
    assert ops.last_igemm_kernel() == "conv_pw_kernel"
    assert ops.last_igemm_kernel_full().startswith("conv_pw_kernel<")
    ops.conv_igemm(d, inp, c["wb"], b)
    assert ops.last_igemm_kernel() == "conv_igemm_dma_kernel"
    af, bf = a.float(), b.float()
    assert ((af - bf).abs() <= 2.0 ** -7 * torch.maximum(af.abs(), bf.abs())).all()      # 1 bf16 ulp
    # ... and the statistics launches leave the same bits, partial sums included: the pointwise kernel adds them in
    # nbdt_conv_igemm_stats' order
    rows = (B * H * W + 255) // 256
    pa, pb = (torch.full((rows * 2 * cout,), float("nan"), device=DEV) for _ in range(2))
    ops.conv_pw(d, inp, c["wb"], a, bn_scratch=pa)
    ops.conv_igemm(d, inp, c["wb"], b, bn_scratch=pb)
    assert torch.equal(a, b)
    if cout % 64 == 0 or cout % 96 == 0 or cout % 160 == 0:
        assert torch.equal(pa, pb)
    else:       # (a single 32-channel cout tile of nbdt_conv_igemm_stats adds with LDS atomics: no fixed order to reproduce)
        np.testing.assert_allclose(pa.cpu().numpy(), pb.cpu().numpy(), rtol=1e-4, atol=1e-4)


def test_tile_width_follows_the_grid():
    """32 -> 128 channels: 255 pixel tiles run 64-channel cout tiles (narrow form: 510 blocks instead of 255), 256 pixel
    tiles run the 128-channel tile.  Both against F.conv2d, with statistics."""
    cin, cout, H, W = 32, 128, 16, 16
    for B, nt in ((255, 2), (256, 4)):
        g = torch.Generator().manual_seed(B)
        x = _bf16(torch.randn(B, H, W, cin, generator=g))
        w = _bf16(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        ref = F.conv2d(x.permute(0, 3, 1, 2), w[:, :, None, None]).permute(0, 2, 3, 1)
        inp = _padded_from(x, float("nan"))
        out = torch.full((B, H + 2, W + 2, cout), SENTINEL, dtype=torch.bfloat16, device=DEV)
        rows = B * H * W // 256
        part = torch.full((rows * 2 * cout,), float("nan"), device=DEV)
        ops.conv_pw(ops.conv_fwd_desc(B, H, W, cin, cout, 1, 1), inp, w.view(cout, 1, cin).to(torch.bfloat16).to(DEV), out,
                    bn_scratch=part)
        assert ops.last_igemm_kernel_full() == f"conv_pw_kernel<{nt}, false, 1>"
        got = ops.interior(out).float().cpu()
        _within(got, ref)
        assert _halo_untouched(out, SENTINEL)
        folded = part.view(rows, 2, cout).double().sum(0).cpu()
        v = got.double().reshape(-1, cout)
        np.testing.assert_allclose(folded[0].numpy(), v.sum(0).numpy(), rtol=1e-4, atol=1e-4)


def test_refuses_what_it_does_not_run():
    B, H, W = 2, 8, 8
    x = ops.padded(B, H, W, 64, DEV)
    w = torch.zeros(64, 9, 64, dtype=torch.bfloat16, device=DEV)
    out = ops.padded(B, H, W, 64, DEV)
    with pytest.raises(NBDTHipError, match="one tap"):
        ops.conv_pw(ops.conv_fwd_desc(B, H, W, 64, 64, 3, 1), x, w, out)
    with pytest.raises(NBDTHipError, match="stride-1"):
        ops.conv_pw(ops.conv_fwd_desc(B, H, W, 64, 64, 1, 2), x, w, ops.padded(B, H // 2, W // 2, 64, DEV))
