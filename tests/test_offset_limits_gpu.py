"""Tensors one image below the 32-bit offset limits (tests/_offset_limit_cases.py), computed for real: the guards of the
entry points allow them, so the kernels must get every element right -- a kernel whose true limit is lower than its
guard (a signed BYTE offset under a guard in elements, a 64-bit path that narrows somewhere) fails here.

  * Inputs are periodic: image b is image b % 3 of three images of bf16 values, so the expected output is the float64
    reference of three images, tiled; every element of the big output is compared ON THE DEVICE, in chunks, with the
    tolerance of the op's own test (tests/test_backbone_gpu.py::_close_bf16, tests/test_effnet_gpu.py::_close_bf16 --
    restated for device tensors below, and checked against the originals on the first and the last images).
  * Outputs are prefilled with NaN (interior) and zero (border): a row that was never stored fails the comparison (which
    counts `not (err <= tol)`, so a NaN is an error), the border must still be zero.
  * Reductions (statistics partials, BatchNorm sums, weight gradients) are compared with float64 sums: of the verified
    output itself, or in closed form from the three images and the counts of b % 3.
  * Every big tensor lives in ONE arena: 4 GiB in front (where an element offset wrapped at 2^31 lands: 2^32 bytes back)
    and 64 MiB behind, filled with a sentinel that must be intact after the call.

  * Three 4 GiB tensors and the margins are 16.06 GiB, so the forms with three activation-sized operands (and dropout)
    write their output over one input.  include/nbdt_hip.h does not promise that this is allowed, and the kernels declare
    the pointers __restrict__: it works because each lane loads and stores at one and the same offset.  A kernel that
    came to fetch ahead across lanes, or through LDS, would break these cases while staying correct for its callers --
    the cases would then need separate tensors (and a larger budget), not the kernel a fix.

The only skip: less free device memory than the arena and the comparison's temporaries need."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _offset_limit_cases as L  # noqa: E402
from test_backbone_gpu import _check_border_zero, _close_bf16, _rand_act, _rand_weight  # noqa: E402
from test_effnet_gpu import _close_bf16 as _close_bf16_mb  # noqa: E402

from nbdt import ops  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A           # (as bf16: 1.5e16 -- a read from a margin cannot pass for data either)
CHUNK = 384                             # images per comparison chunk (a multiple of 3)
WORK = 6 * L.GIB                        # temporaries of a chunked comparison / fill, generously
NAN = float("nan")

_ARENA = {}


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_device_error():
    """A device error (an illegal address, say) leaves the context unusable: end the session instead of launching the
    remaining cases on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"device error, no further launches: {e}", returncode=3)


class Arena:
    """[4 GiB sentinel][tensor 0][tensor 1]...[64 MiB sentinel] carved from one allocation that the module keeps."""

    def __init__(self, cid):
        case = L.gpu_case(cid)
        need = max(L.footprint(c) for c in L.GPU_CASES)
        if "buf" not in _ARENA:
            free, total = torch.cuda.mem_get_info(0)
            if free < need + WORK:
                pytest.skip(f"device memory: {free} bytes free of {total}, the arena needs {need} and the comparison {WORK}")
            _ARENA["buf"] = torch.empty(need, dtype=torch.uint8, device=DEV)
        buf = _ARENA["buf"]
        assert buf.data_ptr() % 256 == 0
        self.front = buf[:L.FRONT_MARGIN].view(torch.int64)
        off = L.FRONT_MARGIN
        self.raw = {}
        for name, n, size in case[2]:
            self.raw[name] = buf[off:off + n * size]
            off += -(-n * size // 256) * 256
        self.back = buf[off:off + L.BACK_MARGIN].view(torch.int64)
        assert off + L.BACK_MARGIN == L.footprint(case) <= buf.numel()
        self.front.fill_(SENTINEL)
        self.back.fill_(SENTINEL)

    def tensor(self, name, shape, dtype=torch.bfloat16):
        t = self.raw[name].view(dtype)
        assert t.numel() == int(np.prod(shape)), (name, t.numel(), shape)
        return t.view(*shape)

    def assert_margins_clean(self):
        dirty = int((self.front != SENTINEL).sum().item()), int((self.back != SENTINEL).sum().item())
        assert dirty == (0, 0), f"sentinel words overwritten (front, back): {dirty}"


def _counts(B):
    return [len(range(i, B, 3)) for i in range(3)]


def _tile_into(view, src3):
    """view[b] = src3[b % 3] (device tensors of one dtype)."""
    B = view.shape[0]
    rep = src3.repeat((CHUNK // 3,) + (1,) * (src3.dim() - 1))
    for b0 in range(0, B, CHUNK):
        n = min(CHUNK, B - b0)
        view[b0:b0 + n] = rep[:n]


def _assert_tiled_equal(got, want3, what):
    """got[b] == want3[b % 3] in every element, border included (value equality, as torch.equal; a NaN is an error)."""
    rep = want3.repeat((CHUNK // 3,) + (1,) * (want3.dim() - 1))
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for b0 in range(0, got.shape[0], CHUNK):
        n = min(CHUNK, got.shape[0] - b0)
        bad += (~(got[b0:b0 + n] == rep[:n])).sum()
    assert int(bad.item()) == 0, f"{what}: {int(bad.item())} of {got.numel()} elements differ or were never stored"


def _poison_interior(p):
    """Padded NHWC output: NaN where the kernel must store, zero in the border it must leave alone."""
    p.fill_(NAN)
    p[:, 0] = 0
    p[:, -1] = 0
    p[:, :, 0] = 0
    p[:, :, -1] = 0


def _border_zero(p):
    """test_backbone_gpu._check_border_zero without a float copy of the whole tensor."""
    for s in (p[:, 0], p[:, -1], p[:, :, 0], p[:, :, -1]):
        assert s.float().abs().max().item() == 0
    _check_border_zero(p[:3])
    _check_border_zero(p[-3:])


def _tol_backbone(ref3, B):
    """test_backbone_gpu._close_bf16's bound for the tiled reference: 2^-7 |ref| + 2e-2 mean|ref| + 1e-6, the mean over the
    whole batch (image i appears counts[i] times)."""
    r = ref3.float()
    cnt = torch.tensor(_counts(B), dtype=torch.float64)
    mean_abs = float((r.abs().double().flatten(1).sum(1) * cnt).sum() / (B * r[0].numel()))
    return 2.0 ** -7 * r.abs() + 2e-2 * mean_abs + 1e-6


def _tol_mbconv(ref3, B, rel=2 ** -7, abs_=1e-3):
    """test_effnet_gpu._close_bf16's bound: rel |want| + abs_."""
    return rel * ref3.float().abs() + abs_


def _assert_tiled(got, ref3, tol3, what, helper=_close_bf16):
    """Every interior element of the padded device tensor `got` [B, H+2, W+2, C] against ref3[b % 3] ([3, H, W, C], host
    float64) within tol3 ([3, H, W, C], host float32) -- and no NaN left.  `helper`: the op's own comparison, applied to
    the first and the last three images as it stands."""
    B = got.shape[0]
    r3, t3 = ref3.float().to(DEV), tol3.to(DEV)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    worst = torch.zeros((), device=DEV)
    for b0 in range(0, B, CHUNK):
        n = min(CHUNK, B - b0)
        g = ops.interior(got[b0:b0 + n]).float()
        full = n - n % 3
        parts = [(g[:full].view(full // 3, 3, *g.shape[1:]), r3[None], t3[None])] if full else []
        if n % 3:
            parts.append((g[full:], r3[:n % 3], t3[:n % 3]))
        for gg, rr, tt in parts:
            err = (gg - rr).abs()
            bad += (~(err <= tt)).sum()
            worst = torch.maximum(worst, torch.nan_to_num(err, nan=float("inf")).max())
    assert int(bad.item()) == 0, f"{what}: {int(bad.item())} of {got.numel()} elements off or never stored, max err {worst.item():.4g}"
    last = [(B - 3 + j) % 3 for j in range(3)]
    if helper is _close_bf16:
        helper(ops.interior(got[:3]), ref3, what + " (first images)")
        helper(ops.interior(got[-3:]), ref3[last], what + " (last images)")
    else:
        helper(ops.interior(got[:3]).float().cpu(), ref3.float(), what + " (first images)")
        helper(ops.interior(got[-3:]).float().cpu(), ref3[last].float(), what + " (last images)")


def _sums64(got):
    """Per-channel float64 sum and sum of squares over the interior of a padded device tensor, in chunks."""
    C = got.shape[-1]
    s1, s2 = torch.zeros(C, dtype=torch.float64, device=DEV), torch.zeros(C, dtype=torch.float64, device=DEV)
    for b0 in range(0, got.shape[0], CHUNK):
        g = ops.interior(got[b0:b0 + CHUNK]).double().reshape(-1, C)
        s1 += g.sum(0)
        s2 += (g * g).sum(0)
    return s1.cpu(), s2.cpu()


# ------------------------------------------------------------------------------------------------------------------------
# convolutions

class _Conv:
    """Three images, weights and float64 references of Conv2d(cin, cout, k, padding=k//2) on `side` x `side` images."""

    def __init__(self, side, cin, cout, k, seed):
        self.side, self.cin, self.cout, self.k = side, cin, cout, k
        self.x3, self.x3p = _rand_act(3, side, side, cin, seed=seed)
        w_oihw, w_int = _rand_weight(cout, cin, k, seed=seed + 1)
        self.wb = torch.empty(cout, k * k, cin, dtype=torch.bfloat16, device=DEV)
        self.wd = torch.empty(cin, k * k, cout, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(w_int.to(DEV), cout, k * k, cin, self.wb, self.wd)
        self.w64 = w_oihw.double()
        self.fwd3 = F.conv2d(self.x3.double().permute(0, 3, 1, 2), self.w64, padding=k // 2).permute(0, 2, 3, 1).contiguous()

    def grads(self, g3, counts):
        """(data gradient of the three images [3, H, W, cin], weight gradient of the whole periodic batch
        [cout][taps][cin]) for output gradients g3 [3, H, W, cout]: float64 autograd, the weight gradient in closed form --
        image i counts[i] times."""
        xt = self.x3.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        wt = self.w64.clone().requires_grad_(True)
        y = F.conv2d(xt, wt, padding=self.k // 2)
        gt = g3.double().permute(0, 3, 1, 2)
        (gx,) = torch.autograd.grad(y, xt, gt, retain_graph=True)
        (gw,) = torch.autograd.grad(y, wt, gt * torch.tensor(counts, dtype=torch.float64).view(3, 1, 1, 1))
        return gx.permute(0, 2, 3, 1).contiguous(), gw.permute(0, 2, 3, 1).reshape(self.cout, self.k * self.k, self.cin)


def _forward_case(cid, kernel, tiled, with_residual_and_stats):
    _, rid, _ = L.gpu_case(cid)
    B, side, _, cin, cout, k, stride = L.row(rid)[4]
    c = _Conv(side, cin, cout, k, seed=100 + cin + k)
    a = Arena(cid)
    P = side + 2
    xin = a.tensor("in", (B, P, P, cin))
    out = a.tensor("out", (B, P, P, cout))
    _tile_into(xin, c.x3p)
    d = ops.conv_fwd_desc(B, side, side, cin, cout, k, stride)
    wt = ops.weight_tiles(c.wb) if tiled else None
    if tiled:
        d.w_tiled = wt.data_ptr()
    _poison_interior(out)
    ops.conv_igemm(d, xin, c.wb, out)
    assert ops.last_igemm_kernel() == kernel
    _assert_tiled(out, c.fwd3, _tol_backbone(c.fwd3, B), f"{cid}: forward")
    _border_zero(out)
    a.assert_margins_clean()
    if not with_residual_and_stats:
        return
    r3, r3p = _rand_act(3, side, side, cout, seed=7)
    res = a.tensor("res", (B, P, P, cout))
    _tile_into(res, r3p)
    ref = c.fwd3 + r3.double()
    _poison_interior(out)
    ops.conv_igemm(d, xin, c.wb, out, residual=res)
    assert ops.last_igemm_kernel() == kernel
    _assert_tiled(out, ref, _tol_backbone(ref, B), f"{cid}: forward + residual")
    _border_zero(out)
    # fused statistics: one [2][cout] row of partial sums per 256 output pixels, against float64 sums of the (verified)
    # output itself -- mean and E[x^2] with the bounds test_backbone_gpu holds bn_finalize to (rtol 1e-4, atol 1e-5)
    n = B * side * side
    rows = (n + 255) // 256
    part = torch.full((rows * 2 * cout,), NAN, device=DEV)
    _poison_interior(out)
    ops.conv_igemm(d, xin, c.wb, out, residual=res, bn_scratch=part)
    assert ops.last_igemm_kernel() == kernel
    _assert_tiled(out, ref, _tol_backbone(ref, B), f"{cid}: forward + residual + statistics")
    _border_zero(out)
    folded = part.view(rows, 2, cout).double().sum(0).cpu()
    s1, s2 = _sums64(out)
    np.testing.assert_allclose((folded[0] / n).numpy(), (s1 / n).numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose((folded[1] / n).numpy(), (s2 / n).numpy(), rtol=1e-4, atol=1e-5)
    a.assert_margins_clean()


def test_dense_3x3_forward_on_the_halo_kernel_plain_residual_statistics():
    """7256 images of 32x32x256 out: the output ends 172 032 elements below 2^31 and crosses byte 2^31 half way."""
    _forward_case("conv_fwd_halo_residual_stats", "conv3x3_pp_kernel", True, True)


def test_dense_3x3_forward_on_the_halo_kernel_with_4_gib_of_input():
    """The halo kernels' 32-bit byte lane offsets: 4 294 623 232 bytes of input."""
    _forward_case("conv_fwd_halo_input", "conv3x3_pp_kernel", True, False)


def test_dense_3x3_forward_on_the_dma_kernel_plain_residual_statistics():
    """8191 images of 30x30 (no halo tile fits a 30-wide row): conv_igemm_dma's int element offsets up to 2^31 - 2^18."""
    _forward_case("conv_fwd_dma_3x3", "conv_igemm_dma_kernel", False, True)


def test_1x1_forward_on_the_dma_kernel():
    _forward_case("conv_fwd_dma_1x1", "conv_igemm_dma_kernel", False, False)


def test_dense_3x3_forward_on_the_dma_kernel_with_the_input_at_the_limit():
    _forward_case("conv_fwd_dma_input", "conv_igemm_dma_kernel", False, False)


def test_pointwise_kernel_forward():
    cid = "conv_pw_fwd"
    B, side, _, cin, cout, k, stride = L.row(L.gpu_case(cid)[1])[4]
    c = _Conv(side, cin, cout, 1, seed=31)
    a = Arena(cid)
    P = side + 2
    xin, out = a.tensor("in", (B, P, P, cin)), a.tensor("out", (B, P, P, cout))
    _tile_into(xin, c.x3p)
    _poison_interior(out)
    ops.conv_pw(ops.conv_fwd_desc(B, side, side, cin, cout, 1, 1), xin, c.wb, out)
    assert ops.last_igemm_kernel() == "conv_pw_kernel"
    _assert_tiled(out, c.fwd3, _tol_backbone(c.fwd3, B), "pointwise forward")
    _border_zero(out)
    a.assert_margins_clean()


def test_accumulating_data_gradient_reads_its_own_output_as_the_residual():
    cid = "conv_dgrad_accumulate"
    B, side, _, cin, cout, k, stride = L.row(L.gpu_case(cid)[1])[4]
    c = _Conv(side, cin, cout, k, seed=41)
    g3, g3p = _rand_act(3, side, side, cout, seed=42)
    b3, b3p = _rand_act(3, side, side, cin, seed=43)
    gx3, _ = c.grads(g3, _counts(B))
    a = Arena(cid)
    P = side + 2
    gy, gx = a.tensor("gy", (B, P, P, cout)), a.tensor("gx", (B, P, P, cin))
    _tile_into(gy, g3p)
    _tile_into(gx, b3p)           # (a row the launch skipped keeps its base value: off by the whole gradient)
    (d,) = ops.conv_dgrad_descs(B, side, side, cin, cout, k, stride, accumulate=True)
    ops.conv_igemm(d, gy, c.wd, gx)
    assert ops.last_igemm_kernel() == "conv_igemm_dma_kernel"
    ref = gx3 + b3.double()
    _assert_tiled(gx, ref, _tol_backbone(ref, B), "accumulating data gradient")
    _border_zero(gx)
    a.assert_margins_clean()


@pytest.mark.parametrize("cid,k,dma", [("wgrad_x_3x3_taps", 3, False), ("wgrad_x_3x3", 3, True), ("wgrad_gy_1x1", 1, True)])
def test_weight_gradient(cid, k, dma):
    """x (an all-nine-taps kernel on 32-wide images; conv_wgrad_dma_kernel on 30-wide ones) or gy (1x1) one image below
    2^31 elements; the reference is the float64 weight gradient of the three images in closed form (image i counts[i]
    times), compared as test_backbone_gpu does."""
    B, side, _, cin, cout, _, stride = L.row(L.gpu_case(cid)[1])[4]
    c = _Conv(side, cin, cout, k, seed=51 + k)
    g3, g3p = _rand_act(3, side, side, cout, seed=52)
    _, gw = c.grads(g3, _counts(B))
    a = Arena(cid)
    P = side + 2
    x, gy = a.tensor("x", (B, P, P, cin)), a.tensor("gy", (B, P, P, cout))
    _tile_into(x, c.x3p)
    _tile_into(gy, g3p)
    dw = torch.zeros(cout, k * k, cin, dtype=torch.float32, device=DEV)
    ops.conv_wgrad(ops.conv_wgrad_desc(B, side, side, cin, cout, k, stride), x, gy, dw)
    print(f"{cid}: {ops.last_wgrad_kernel()}")
    assert ops.last_wgrad_kernel() == ("conv_wgrad_dma_kernel" if dma else "conv_wgrad_ks_kernel")
    ref = gw.numpy()
    np.testing.assert_allclose(dw.cpu().double().numpy(), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())
    a.assert_margins_clean()


# ------------------------------------------------------------------------------------------------------------------------
# BatchNorm (csrc/bn.hip) and the MBConv streaming kernels (csrc/effnet.hip) on [8191, 30, 30, 256]

class _Bn:
    """Three images x3 (N(0.5, 2), bf16) and the float64 batch statistics of the periodic batch in closed form."""

    def __init__(self, B, side, C, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.side, self.C = B, side, C
        x = (torch.randn(3, side, side, C, generator=g) * 2 + 0.5).to(torch.bfloat16)
        self.x3 = x.float()
        self.x3p = ops.padded(3, side, side, C, DEV)
        ops.interior(self.x3p).copy_(x.to(DEV))
        self.cnt = torch.tensor(_counts(B), dtype=torch.float64)
        self.n = B * side * side
        xd = self.x3.double()
        self.mean = (xd.sum((1, 2)) * self.cnt[:, None]).sum(0) / self.n
        self.var = ((xd * xd).sum((1, 2)) * self.cnt[:, None]).sum(0) / self.n - self.mean ** 2
        self.rstd = (self.var + 1e-5).rsqrt()
        self.gamma = torch.rand(C, generator=g) + 0.5
        self.beta = torch.randn(C, generator=g) * 0.3
        self.dev = [t.float().to(DEV) for t in (self.mean, self.rstd, self.gamma, self.beta)]

    def bn(self):
        return (self.x3.double() - self.mean) * self.rstd * self.gamma.double() + self.beta.double()


def _bn_case(cid, seed):
    B, side, _, C = L.row(L.gpu_case(cid)[1])[4]
    return _Bn(B, side, C, seed), Arena(cid), (B, side + 2, side + 2, C)


def test_batchnorm_statistics_and_apply():
    f, a, shape = _bn_case("bn_stats_apply", 61)
    x, y = a.tensor("x", shape), a.tensor("y", shape)
    _tile_into(x, f.x3p)
    scratch = torch.zeros(ops.BN_SLOTS * 2 * f.C, device=DEV)
    mean, rstd = torch.empty(f.C, device=DEV), torch.empty(f.C, device=DEV)
    ops.bn_stats(x, scratch, mean, rstd)
    np.testing.assert_allclose(mean.cpu().numpy(), f.mean.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rstd.cpu().numpy(), f.rstd.numpy(), rtol=1e-4)
    assert scratch.abs().max().item() == 0
    _poison_interior(y)
    ops.bn_apply(x, f.dev[0], f.dev[1], f.dev[2], f.dev[3], y, relu=True)
    ref = torch.relu(f.bn())
    _assert_tiled(y, ref, _tol_backbone(ref, f.B), "bn apply")
    _border_zero(y)
    a.assert_margins_clean()


def test_batchnorm_backward_sums():
    """nbdt_bn_bwd_reduce with the ReLU mask recomputed from x: dbeta = sum g', dgamma = sum g' * xhat over 7.4 M pixels per
    channel, in closed form from the three images; the bounds test_batchnorm_forward_backward holds them to.  (The
    elementwise pass needs gy, x and gx -- 12 GiB -- and does not fit the 16 GiB a case may take with its margins.)"""
    f, a, shape = _bn_case("bn_bwd_reduce", 62)
    g3, g3p = _rand_act(3, f.side, f.side, f.C, seed=63)
    x, gy = a.tensor("x", shape), a.tensor("gy", shape)
    _tile_into(x, f.x3p)
    _tile_into(gy, g3p)
    scratch = torch.zeros(ops.BN_SLOTS * 2 * f.C, device=DEV)
    dsum, dgamma, dbeta = torch.empty(2 * f.C, device=DEV), torch.zeros(f.C, device=DEV), torch.zeros(f.C, device=DEV)
    from nbdt._C import check, lib, ptr
    check(lib().nbdt_bn_bwd_reduce(ptr(gy), None, ptr(x), ptr(f.dev[0]), ptr(f.dev[1]), ptr(f.dev[2]), ptr(f.dev[3]), 1,
                                   f.B, f.side, f.side, f.C, ptr(scratch), ptr(dsum), ptr(dgamma), ptr(dbeta),
                                   ops.stream_ptr(DEV)))
    # the kernel forms the mask in fp32 from the fp32 copies of mean / rstd: use the same values here
    m, r, ga, be = (t.double().cpu() for t in f.dev)
    xhat = (f.x3.double() - m) * r
    gm = g3.double() * ((xhat * ga + be) > 0)
    w = f.cnt.view(3, 1, 1, 1)
    db_ref, dg_ref = (gm * w).sum((0, 1, 2)), (gm * xhat * w).sum((0, 1, 2))
    np.testing.assert_allclose(dbeta.cpu().numpy(), db_ref.numpy(), rtol=2e-2, atol=2e-2 * db_ref.abs().mean().item())
    np.testing.assert_allclose(dgamma.cpu().numpy(), dg_ref.numpy(), rtol=2e-2, atol=2e-2 * dg_ref.abs().mean().item())
    assert scratch.abs().max().item() == 0
    # the elementwise pass, gx written over gy: every lane of bn_bwd_apply_kernel loads its 16 bytes of gy and x at an
    # offset and stores gx at the same offset, so the two may be one tensor -- gy, x and a separate gx (3 x 4 GiB) with the
    # 4 GiB + 64 MiB margins would be 16.06 GiB.  A row that was never stored keeps gy.
    check(lib().nbdt_bn_bwd_apply(ptr(gy), None, ptr(x), ptr(f.dev[0]), ptr(f.dev[1]), ptr(f.dev[2]), ptr(f.dev[3]),
                                  ptr(dsum), None, 1, f.B, f.side, f.side, f.C, ptr(gy), None, ops.stream_ptr(DEV)))
    gx3 = ga * r * (gm - db_ref / f.n - xhat * dg_ref / f.n)
    _assert_tiled(gy, gx3, _tol_backbone(gx3, f.B), "bn backward, elementwise pass in place")
    _border_zero(gy)
    a.assert_margins_clean()


def _swish(v):
    return v * torch.sigmoid(v)


def test_mbconv_apply_gated_apply_and_pool():
    f, a, shape = _bn_case("bn_act_apply_pool", 71)
    x, y = a.tensor("x", shape), a.tensor("y", shape)
    _tile_into(x, f.x3p)
    act3 = _swish(f.bn())
    _poison_interior(y)
    ops.bn_act_apply(x, *f.dev, y, act=ops.ACT_SWISH)
    _assert_tiled(y, act3, _tol_mbconv(act3, f.B), "bn_act_apply", helper=_close_bf16_mb)
    _border_zero(y)
    # gated: gate[b] = gate3[b % 3]
    gate3 = torch.rand(3, f.C, generator=torch.Generator().manual_seed(72))
    gate = gate3.repeat(f.B // 3 + 1, 1)[:f.B].contiguous().to(DEV)
    ref = act3 * gate3.double()[:, None, None, :]
    _poison_interior(y)
    ops.bn_act_apply(x, *f.dev, y, act=ops.ACT_SWISH, gate=gate)
    _assert_tiled(y, ref, _tol_mbconv(ref, f.B), "bn_act_apply, gated", helper=_close_bf16_mb)
    _border_zero(y)
    # with a residual, y written over it (mb_apply_kernel: a lane loads x and the residual at an offset and stores y at
    # the same one; three separate 4 GiB tensors and the margins would be 16.06 GiB)
    r3, r3p = _rand_act(3, f.side, f.side, f.C, seed=73)
    _tile_into(y, r3p)
    ref = act3 + r3.double()
    ops.bn_act_apply(x, *f.dev, y, act=ops.ACT_SWISH, residual=y)
    _assert_tiled(y, ref, _tol_mbconv(ref, f.B), "bn_act_apply, residual in place", helper=_close_bf16_mb)
    _border_zero(y)
    # pooled mean per (image, channel): 2e-3 absolute, as test_bn_act_apply_pool_and_backward_forms
    out = torch.full((f.B, f.C), 7.0, device=DEV)
    ops.bn_act_pool(x, *f.dev, out, act=ops.ACT_SWISH)
    want = act3.mean((1, 2)).float().to(DEV)
    full = f.B - f.B % 3
    err = (out[:full].view(-1, 3, f.C) - want[None]).abs().max().item()
    err = max(err, (out[full:] - want[:f.B % 3]).abs().max().item())
    assert err < 2e-3, err
    a.assert_margins_clean()


def test_mbconv_backward_pooled_form():
    """nbdt_bn_act_bwd with a pooled upstream gradient (x and gx are the two big tensors; the forms with a gradient tensor
    need three): gx against float64 autograd through the closed-form batch statistics, dgamma / dbeta in closed form."""
    f, a, shape = _bn_case("bn_act_bwd_pooled", 81)
    x, gx = a.tensor("x", shape), a.tensor("gx", shape)
    _tile_into(x, f.x3p)
    gpool3 = torch.randn(3, f.C, generator=torch.Generator().manual_seed(82))
    gpool = gpool3.repeat(f.B // 3 + 1, 1)[:f.B].contiguous().to(DEV)
    # float64 reference: the periodic batch's statistics are count-weighted sums over the three images
    xr = f.x3.double().clone().requires_grad_(True)
    gr, br = f.gamma.double().clone().requires_grad_(True), f.beta.double().clone().requires_grad_(True)
    w = f.cnt.view(3, 1, 1, 1)
    mean = (xr * w).sum((0, 1, 2)) / f.n
    var = (xr * xr * w).sum((0, 1, 2)) / f.n - mean ** 2
    act = _swish((xr - mean) * (var + 1e-5).rsqrt() * gr + br)
    # L = sum_b <gpool[b], mean_pixels act[b]>; image i stands for cnt[i] images, and d/dx3[i] is then cnt[i] x the
    # gradient of ONE of its copies
    loss = (act.mean((1, 2)) * gpool3.double() * f.cnt[:, None]).sum()
    gx3, dg_ref, db_ref = torch.autograd.grad(loss, (xr, gr, br))
    gx3 = gx3 / w
    scratch = torch.zeros(ops.BN_SLOTS * 2 * 2048, device=DEV)
    dsum, dgamma, dbeta = torch.empty(2 * f.C, device=DEV), torch.zeros(f.C, device=DEV), torch.zeros(f.C, device=DEV)
    _poison_interior(gx)
    ops.bn_act_bwd(None, x, *f.dev, scratch, dsum, dgamma, dbeta, gx, act=ops.ACT_SWISH, gpool=gpool)
    # the bounds of test_bn_act_apply_pool_and_backward_forms
    scale = gx3.abs().max().item()
    tol = torch.full_like(gx3, 2e-2 * scale + 1e-3).float()
    _assert_tiled(gx, gx3, tol, "bn_act_bwd, pooled form",
                  helper=lambda got, want, what: _close_bf16_mb(got, want, what, rel=0.0, abs_=2e-2 * scale + 1e-3))
    _border_zero(gx)
    assert (dgamma.cpu() - dg_ref).abs().max().item() < 5e-3 * dg_ref.abs().max().item() + 1e-3
    assert (dbeta.cpu() - db_ref).abs().max().item() < 5e-3 * db_ref.abs().max().item() + 1e-3
    assert scratch.abs().max().item() == 0
    a.assert_margins_clean()
    # the form with a gradient tensor, gx written over gu (the sums are a launch of their own that ends before
    # mb_bwd_apply_kernel, whose lanes load gu and x at an offset and store gx at the same one; gu, x and a separate gx
    # with the margins would be 16.06 GiB)
    g3, g3p = _rand_act(3, f.side, f.side, f.C, seed=83)
    _tile_into(gx, g3p)
    xr = f.x3.double().clone().requires_grad_(True)
    gr, br = f.gamma.double().clone().requires_grad_(True), f.beta.double().clone().requires_grad_(True)
    mean = (xr * w).sum((0, 1, 2)) / f.n
    var = (xr * xr * w).sum((0, 1, 2)) / f.n - mean ** 2
    act = _swish((xr - mean) * (var + 1e-5).rsqrt() * gr + br)
    gx3, dg_ref, db_ref = torch.autograd.grad((act * g3.double() * w).sum(), (xr, gr, br))
    gx3 = gx3 / w
    dgamma.zero_()
    dbeta.zero_()
    ops.bn_act_bwd(gx, x, *f.dev, scratch, dsum, dgamma, dbeta, gx, act=ops.ACT_SWISH)
    scale = gx3.abs().max().item()
    tol = torch.full_like(gx3, 2e-2 * scale + 1e-3).float()
    _assert_tiled(gx, gx3, tol, "bn_act_bwd, gradient tensor in place",
                  helper=lambda got, want, what: _close_bf16_mb(got, want, what, rel=0.0, abs_=2e-2 * scale + 1e-3))
    _border_zero(gx)
    assert (dgamma.cpu() - dg_ref).abs().max().item() < 5e-3 * dg_ref.abs().max().item() + 1e-3
    assert (dbeta.cpu() - db_ref).abs().max().item() < 5e-3 * db_ref.abs().max().item() + 1e-3
    assert scratch.abs().max().item() == 0
    a.assert_margins_clean()


@pytest.mark.parametrize("k,stride", [(3, 1), (5, 1), (3, 2), (5, 2)])
def test_depthwise_forward_data_gradient_weight_gradient(k, stride):
    """x / gx at [8191, 30, 30, 256]; the references and bounds of test_depthwise_conv_forward_and_gradients in float64."""
    cid = "dwconv"
    B, side, _, C = L.row(L.gpu_case(cid)[1])[4]
    so = side // stride
    gen = torch.Generator().manual_seed(90 + 10 * k + stride)
    x3 = torch.randn(3, C, side, side, generator=gen).to(torch.bfloat16).float()
    g3 = torch.randn(3, C, so, so, generator=gen).to(torch.bfloat16).float()
    w = torch.randn(C, 1, k, k, generator=gen) * 0.3
    cnt = torch.tensor(_counts(B), dtype=torch.float64).view(3, 1, 1, 1)
    xr, wr = x3.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride, k // 2, 1, C)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, g3.double(), retain_graph=True)
    (dw_ref,) = torch.autograd.grad(y_ref, wr, g3.double() * cnt)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()       # noqa: E731
    wt = w.view(C, k * k).t().contiguous().to(DEV)

    def padded3(t_nchw):
        p = ops.padded(3, t_nchw.shape[2], t_nchw.shape[3], C, DEV)
        ops.interior(p).copy_(nhwc(t_nchw).to(DEV))
        return p

    a = Arena(cid)
    n_small = B * (so + 2) * (so + 2) * C
    big = lambda name: a.tensor(name, (B, side + 2, side + 2, C))      # noqa: E731
    small = lambda name: a.raw[name].view(torch.bfloat16)[:n_small].view(B, so + 2, so + 2, C)      # noqa: E731
    # forward: x (at the limit) -> y
    x, y = big("x"), small("y")
    _tile_into(x, padded3(x3))
    _poison_interior(y)
    ops.dwconv_fwd(x, wt, y, k, stride)
    ref = nhwc(y_ref)
    _assert_tiled(y, ref, _tol_mbconv(ref, B), f"dw fwd k{k} s{stride}", helper=_close_bf16_mb)
    _border_zero(y)
    # weight gradient: x, gy (y's place) -> dw, twice (+=)
    _tile_into(y, padded3(g3))
    dw = torch.zeros(k * k, C, device=DEV)
    ops.dwconv_bwd_weight(x, y, dw, k, stride)
    ops.dwconv_bwd_weight(x, y, dw, k, stride)
    want = 2 * dw_ref.reshape(C, k * k).t()
    assert (dw.cpu() - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-4
    # data gradient: gy -> gx (x's place, at the limit)
    _poison_interior(x)
    ops.dwconv_bwd_data(y, wt, x, k, stride)
    ref = nhwc(gx_ref)
    _assert_tiled(x, ref, _tol_mbconv(ref, B), f"dw bwd_data k{k} s{stride}", helper=_close_bf16_mb)
    _border_zero(x)
    a.assert_margins_clean()


# ------------------------------------------------------------------------------------------------------------------------
# the slice-list convolution and the space-to-depth copy one image below their output guards

def test_strided_forward_over_space_to_depth_one_image_below_the_output_guard():
    """nbdt_conv_seg: 7256 images of 64x64x32 as the space-to-depth copy [7256, 34, 34, 128] -> 32x32x256 outputs, 172 032
    elements below 2^31; reference and bound of tests/test_conv_seg_gpu.py in float64."""
    from test_conv_seg_gpu import _s2d
    cid = "conv_seg_fwd"
    B, Hi, Wi, cin, cout = L.row("conv_seg_out")[4]
    Ho, Wo = Hi // 2, Wi // 2
    x3, x3p = _rand_act(3, Hi, Wi, cin, seed=11)
    w_oihw, w_int = _rand_weight(cout, cin, 3, seed=12)
    wb = torch.empty(cout, 9, cin, dtype=torch.bfloat16, device=DEV)
    wd = torch.empty(cin, 9, cout, dtype=torch.bfloat16, device=DEV)
    ops.weight_prep(w_int.to(DEV), cout, 9, cin, wb, wd)
    ref3 = F.conv2d(x3.double().permute(0, 3, 1, 2), w_oihw.double(), stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    plan = ops.seg_fwd_s2(B, Hi, Wi, cin, cout)
    a = Arena(cid)
    xin, out = a.tensor("in", (B, Ho + 2, Wo + 2, 4 * cin)), a.tensor("out", (B, Ho + 2, Wo + 2, cout))
    _tile_into(xin, _s2d(x3p, 3, Hi, Wi, cin))
    _poison_interior(out)
    plan([xin], plan.tile_weights([wb]), out)
    _assert_tiled(out, ref3, _tol_backbone(ref3, B), "slice-list strided forward")
    _border_zero(out)
    a.assert_margins_clean()


def test_space_to_depth_copy_one_image_below_its_output_guard():
    """nbdt_bn_apply_s2d on [7256, 30, 30, 256]: the copy [7256, 17, 17, 1024] ends 172 032 elements below 2^31.  As
    tests/test_conv_seg_gpu.py: bit for bit nbdt_bn_apply rearranged (here of the three images, which in turn meet the
    float64 reference)."""
    from test_conv_seg_gpu import _s2d
    B, side, _, C = L.row("bn_s2d_out_30")[4]
    f, a = _Bn(B, side, C, 65), Arena("bn_s2d")
    x, y = a.tensor("x", (B, side + 2, side + 2, C)), a.tensor("y", (B, side // 2 + 2, side // 2 + 2, 4 * C))
    _tile_into(x, f.x3p)
    y3 = ops.padded(3, side, side, C, DEV)
    ops.bn_apply(f.x3p, *f.dev, y3, relu=True)
    _close_bf16(ops.interior(y3), torch.relu(f.bn()), "bn apply of the three images")
    _poison_interior(y)
    ops.bn_apply_s2d(x, *f.dev, y, relu=True)
    _assert_tiled_equal(y, _s2d(y3, 3, side, side, C), "space-to-depth copy")
    a.assert_margins_clean()


# ------------------------------------------------------------------------------------------------------------------------
# the 64-bit paths: tensors past 2^31 elements / 2^32 bytes

def test_grouped_conv_forward_data_gradient_weight_gradient_past_2_31_elements():
    """csrc/conv_group.hip on bf16 [8200, 30, 30, 256], 8 channels per group: 2 149 580 800 padded elements each way (the
    guard is on padded pixels).  References of tests/_conv_group_cases.py in float64, bounds of tests/test_conv_group_gpu.py
    (|a - b| <= 2^-7 |ref| + 1e-4 -- its max(|a|, |b|) is not smaller; weight gradient rtol 2e-3, atol 2e-3 mean|ref|)."""
    import _conv_group_cases as G
    from test_conv_group_gpu import _close as _close_group
    B, side, C, cg = L.GROUP_B, L.S, L.WIDE, 8
    gen = torch.Generator().manual_seed(77)
    bf = lambda t: t.to(torch.bfloat16).float()      # noqa: E731
    x3, g3 = bf(torch.randn(3, C, side, side, generator=gen)), bf(torch.randn(3, C, side, side, generator=gen))
    w = bf(torch.randn(C, cg, 3, 3, generator=gen) / (9 * cg) ** 0.5)
    cnt = torch.tensor(_counts(B), dtype=torch.float64).view(3, 1, 1, 1)
    fwd, gx, _ = G.refs(x3, w, g3, 1, C // cg, torch.float64)
    dw_ref = G.refs(x3, w, g3.double() * cnt, 1, C // cg, torch.float64)[2].numpy()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()       # noqa: E731
    master = G.master_of(w).float().to(DEV)
    wf = torch.empty(C // 32, 32, 9, 32, dtype=torch.bfloat16, device=DEV)
    wd = torch.empty_like(wf)
    ops.conv_group_weight_prep(master, C, cg, wf, wd)

    def padded3(t):
        p = ops.padded(3, side, side, C, DEV)
        ops.interior(p).copy_(nhwc(t).to(DEV))
        return p

    tol = lambda r: 2.0 ** -7 * r.float().abs() + 1e-4      # noqa: E731
    a = Arena("conv_group")
    shape = (B, side + 2, side + 2, C)
    x, y = a.tensor("x", shape), a.tensor("y", shape)
    _tile_into(x, padded3(x3))
    _poison_interior(y)
    ops.conv_group_fwd(x, wf, y, cg, 1)
    _assert_tiled(y, nhwc(fwd), tol(nhwc(fwd)), "grouped forward", helper=_close_group)
    _border_zero(y)
    _tile_into(y, padded3(g3))
    dw = torch.zeros(C, 9, cg, device=DEV)
    ops.conv_group_wgrad(x, y, dw, cg, 1)
    np.testing.assert_allclose(dw.cpu().double().numpy(), dw_ref, rtol=2e-3, atol=2e-3 * np.abs(dw_ref).mean())
    _poison_interior(x)
    ops.conv_group_dgrad(y, wd, x, cg, 1)
    _assert_tiled(x, nhwc(gx), tol(nhwc(gx)), "grouped data gradient", helper=_close_group)
    _border_zero(x)
    a.assert_margins_clean()


def test_dropout_past_2_31_elements():
    """nbdt_dropout_fwd / _bwd on fp32 [1 680 000, 1280] = 2 150 400 000 elements, y written over x (a thread reads x[i] and
    writes y[i]; x, y and the mask apart would be 19.4 GB before the margins).  The checks of test_dropout_and_strided_stem:
    y = x * mask / 0.8 within 1e-6, the kept share within 0.01 of 0.8 -- and every mask byte written (0 or 1)."""
    n = L.DROPOUT_N
    rows, step = n // 1280, 3 * 32768
    a = Arena("dropout")
    x, mask = a.tensor("x", (rows, 1280), torch.float32), a.tensor("mask", (rows, 1280), torch.uint8)
    x3 = torch.randn(3, 1280, generator=torch.Generator().manual_seed(9)).to(DEV)
    rep = x3.repeat(step // 3, 1)

    def fill():
        for b0 in range(0, rows, step):
            x[b0:b0 + step] = rep[:min(step, rows - b0)]

    def check(what):
        err, kept, top = torch.zeros((), device=DEV), torch.zeros((), dtype=torch.int64, device=DEV), 0
        for b0 in range(0, rows, step):
            m = mask[b0:b0 + step]
            err = torch.maximum(err, torch.nan_to_num((x[b0:b0 + step] - rep[:m.shape[0]] * m.float() / 0.8).abs(),
                                                      nan=float("inf")).max())
            kept += m.sum(dtype=torch.int64)
            top = max(top, int(m.max().item()))
        assert top == 1, f"{what}: a mask byte holds {top}"
        assert err.item() < 1e-6, (what, err.item())
        assert abs(kept.item() / n - 0.8) < 0.01, (what, kept.item() / n)

    fill()
    mask.fill_(7)
    ops.dropout_fwd(x, 0.2, 123, mask, x)
    check("dropout forward")
    fill()
    ops.dropout_bwd(x, 0.2, mask, x)
    check("dropout backward")
    a.assert_margins_clean()


def test_pixel_tree_rules_on_logits_past_2_31_elements():
    """bf16 NCHW logits [3496, 150, 64, 64] (2 147 942 400 elements; image 3495 straddles element 2^31) on the ADE20K
    hierarchy, against tests/_seg_ref.py's restatement of the three distinct images.

    nbdt_seg_hard_forward on the whole tensor: bit for bit the labels of the row kernels on the three images (as
    tests/test_seg_gpu.py), and the restatement's labels wherever no decision on the restatement's path is a tie (bf16
    logits tie, and the two sides need not break a tie alike: a pixel counts as tied where the two largest child logits
    of a node on its path are within 1e-4 -- the fp32 means of up to 150 logits differ by their summation order).

    The soft forward, the soft backward and the fused loss with its gradient run on the view z[7::32]: 110 images whose
    image stride is 32 x 150 x 64 x 64 elements, the last of them image 3495, so the 64-bit input strides carry offsets up
    to the end of the tensor while each fp32 output is 270 MB (the whole tensor's would be 8.6 GB: 17.2 GB with z and
    the margins).  Outputs are prefilled with NaN.  Bounds of tests/test_seg_gpu.py: P rtol 2e-5 / atol 1e-6; backward
    rtol 1e-5 / atol 2e-6; loss 1e-5 relative; dL/dz 1e-6 absolute -- a bound made for the goldens' 40 valid pixels
    (|dL/dz| up to 0.03), so the loss runs with grad_scale = valid pixels / 40, which gives every pixel the gradient it
    would have in a batch of 40 (at grad_scale 1 no gradient here exceeds 1e-5 and the bound would pass anything).
    Labels are periodic like the logits, 30 % of them ignore_index, and the last image's upper half is ignore_index
    throughout; the loss and the count of valid pixels follow in closed form from the four distinct (image, labels)
    pairs."""
    import _seg_ref as S
    from nbdt import _C
    from test_seg_gpu import close_P, close_dz, coerce
    O = S.O
    tree, otree, _ = S.case("ade20k")
    handle = tree.device_handle(0)
    N, C, side = L.SEG_N, L.SEG_C, L.SEG_SIDE
    gen = torch.Generator().manual_seed(21)
    z3 = (2.0 * torch.randn(3, C, side, side, generator=gen)).to(torch.bfloat16)
    z3n = z3.float().numpy()
    a = Arena("seg_rules")
    z = a.tensor("z", (N, C, side, side))
    _tile_into(z, z3.to(DEV))

    # ---- hard forward, the whole tensor
    pred, _ = _C.seg_hard_forward(handle, z, want_onehot=False)
    assert _C.last_rules_path() == "pixel"
    pred3 = _C.hard_forward(handle, coerce(z3.to(DEV).float()))[0].view(3, side, side)
    assert torch.equal(pred, pred3[torch.arange(N, device=DEV) % 3])
    rows3 = S.coerce(z3n)
    outs = O.node_outputs(otree, rows3)
    ref_pred, decisions = O.hard_forward(otree, rows3, outs, with_decisions=True)
    gap = []
    for o in outs:
        top = np.sort(o["logits"], axis=1)
        gap.append(top[:, -1] - top[:, -2])
    gap = np.stack(gap)
    tied = np.array([any(gap[n, b] <= 1e-4 for n, *_ in steps) for b, steps in enumerate(decisions)])
    print(f"hard forward: {tied.mean():.4f} of the pixels tied")
    assert tied.mean() < 0.05
    assert np.array_equal(pred3.cpu().numpy().reshape(-1)[~tied], ref_pred[~tied])

    # ---- the strided view
    zs = z[L.SEG_FIRST::L.SEG_EVERY]
    idx = torch.arange(L.SEG_FIRST, N, L.SEG_EVERY)
    n = len(idx)
    assert idx[-1] == N - 1 and _C.seg_dispatch(tuple(zs.shape), tuple(zs.stride()), zs.dtype, tree.flat) == "pixel"
    nn_, HW, zi, zc = _C._seg_geom(zs)
    assert (nn_, HW, zi, zc) == (n, side * side, L.SEG_EVERY * C * side * side, side * side)
    kind = (idx % 3).to(DEV)
    head = (handle.h, _C.ptr(zs), _C.ztype_of(zs), n, HW, zi, zc)
    st = _C.stream_of(zs)
    out = torch.full((n, C, side, side), NAN, device=DEV)

    def within(want, atol, rtol, what):
        bad = ~((out - want).abs() <= atol + rtol * want.abs())
        assert not bad.any(), f"{what}: {int(bad.sum())} of {out.numel()} elements off or never stored"

    # soft forward
    _C.check(_C.lib().nbdt_seg_soft_forward(*head, _C.ptr(out), st))
    assert _C.last_rules_path() == "pixel"
    P3 = O.soft_forward(otree, rows3, outs)
    want = torch.from_numpy(S.uncoerce(P3, z3n.shape)).to(DEV)[kind]
    within(want, 1e-6, 2e-5, "path probabilities")
    close_P(out[-1], want[-1])

    # soft backward
    gP3 = torch.randn(3, C, side, side, generator=gen)
    gz3 = O.rules_backward(otree, rows3, S.coerce(gP3.numpy()), outs=outs, P=P3)
    gP = gP3.to(DEV)[kind].contiguous()
    out.fill_(NAN)
    _C.check(_C.lib().nbdt_seg_soft_backward(*head, _C.ptr(gP), _C.ptr(out), st))
    assert _C.last_rules_path() == "pixel"
    want = torch.from_numpy(S.uncoerce(gz3, z3n.shape)).to(DEV)[kind]
    within(want, 2e-6, 1e-5, "soft backward")
    np.testing.assert_allclose(out[-1].cpu().numpy(), want[-1].cpu().numpy(), atol=2e-6, rtol=1e-5)
    del gP

    # fused loss and gradient: pairs 0, 1, 2 = (image i, labels i), pair 3 = the last image with its upper half ignored
    y3 = torch.randint(0, C, (3, side, side), generator=gen)
    y3[torch.rand(3, side, side, generator=gen) < 0.3] = S.IGNORE
    last = int(idx[-1]) % 3
    y_last = y3[last].clone()
    y_last[:side // 2] = S.IGNORE
    y4 = torch.cat([y3, y_last[None]])
    kind4 = kind.clone()
    kind4[-1] = 3
    y = y4.to(DEV)[kind4].contiguous()
    GOLDEN_VALID = 40
    sums, valid, grads = [], [], []
    for q in range(4):
        zq = z3n[[q if q < 3 else last]]
        value, dz = S.loss(otree, tree.flat, zq, y4[q:q + 1].numpy(), tsw=S.TSW)
        nq = int((y4[q] != S.IGNORE).sum())
        sums.append(float(value) * nq)
        valid.append(nq)
        grads.append(torch.from_numpy(dz[0] * (nq / GOLDEN_VALID)).float())         # per pixel, as in a batch of 40
    times = [int((kind4 == q).sum()) for q in range(4)]
    n_valid = sum(t * v for t, v in zip(times, valid))
    ref_loss = sum(t * s_ for t, s_ in zip(times, sums)) / n_valid
    assert times[3] == 1 and valid[3] < valid[last] and n_valid == int((y != S.IGNORE).sum())
    ws = torch.empty((int(_C.lib().nbdt_seg_loss_workspace_floats(n, HW)),), device=DEV)
    loss = torch.full((), NAN, device=DEV)
    out.fill_(NAN)
    _C.check(_C.lib().nbdt_seg_soft_tree_loss(*head, _C.ptr(y), S.IGNORE, 0.0, 1.0, S.TSW, n_valid / GOLDEN_VALID,
                                              _C.ptr(ws), _C.ptr(loss), _C.ptr(out), st))
    assert _C.last_rules_path() == "pixel"
    print(f"fused loss {loss.item():.6f} against {ref_loss:.6f}, {n_valid} valid pixels")
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    want = torch.stack(grads).to(DEV)[kind4]
    within(want, 1e-6, 0.0, "dL/dz of the fused loss")
    close_dz(out[-1], want[-1])
    assert not out[y.unsqueeze(1).expand_as(out) == S.IGNORE].any()          # exactly 0 at ignored pixels
    a.assert_margins_clean()


def test_mix_batch_past_4_gib():
    """MixUp and CutMix of fp32 [87400, 3, 64, 64] (4 295 884 800 bytes in, as many out), bit for bit the torch expression
    of tests/test_mix_gpu.py on the three distinct images: out[b] pairs image b % 3 with image (b - 1) % 3, and out[0]
    with image B - 1."""
    from test_mix_gpu import f32, target_reference
    B, S, C = L.MIX_B, L.MIX_SIDE, 10
    a = Arena("mix_batch")
    x, out = a.tensor("x", (B, 3, S, S), torch.float32), a.tensor("out", (B, 3, S, S), torch.float32)
    x3 = torch.randn(3, 3, S, S, generator=torch.Generator().manual_seed(5))
    _tile_into(x, x3.to(DEV))
    y = torch.arange(B) % C
    tgt = torch.full((B, C), NAN, device=DEV)
    for lam, box in ((0.3, (0, 0, 0, 0)), (1.0, (5, 41, 10, 63))):
        partner = x3.roll(1, 0)                      # image (i - 1) % 3
        if box == (0, 0, 0, 0):
            mix = lambda u, v: u.mul(f32(lam)).add(v.mul(f32(1.0 - lam)))      # noqa: E731
            lam_t = lam
        else:
            def mix(u, v):
                w = u.clone()
                w[..., box[0]:box[1], box[2]:box[3]] = v[..., box[0]:box[1], box[2]:box[3]]
                return w
            lam_t = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(S * S)
        want3 = mix(x3, partner).to(DEV)
        want0 = mix(x3[0], x3[(B - 1) % 3]).to(DEV)
        out.fill_(NAN)
        ops.mix_batch(x, y.to(DEV), out, tgt, lam=lam, box=box, lam_t=lam_t)
        assert torch.equal(out[0], want0)
        assert torch.equal(out[1:3], want3[1:3])
        full = (B - 3) - (B - 3) % 3
        for b0 in range(3, 3 + full, 3 * 1024):
            b1 = min(b0 + 3 * 1024, 3 + full)
            assert torch.equal(out[b0:b1].view(-1, 3, 3, S, S), want3[None].expand((b1 - b0) // 3, 3, 3, S, S)), (lam, b0)
        assert torch.equal(out[3 + full:], want3[:B - 3 - full])
        assert torch.equal(tgt.cpu(), target_reference(y, C, lam_t))
        a.assert_margins_clean()


def _dataset_rows(idx):
    """Rows `idx` of the resident dataset as the host sees them: byte `pos` of image i is (131 i + 7 pos) & 255."""
    n = 3 * L.DATA_SIDE * L.DATA_SIDE
    i = torch.as_tensor(idx, dtype=torch.int64).view(-1, 1)
    return ((131 * i + 7 * torch.arange(n).view(1, -1)) & 255).to(torch.uint8).view(-1, 3, L.DATA_SIDE, L.DATA_SIDE)


def test_batches_from_a_dataset_past_4_gib():
    """A uint8 dataset of 350 000 images of 3x64x64 (4 300 800 000 bytes) generated on the device; a batch of 64 indices
    holds row 0, the rows around bytes 2^31 and 2^32 and the last one.  nbdt_augment_batch, nbdt_policy_batch (no policy,
    no erase: the same transform on the LDS-staged kernel) and nbdt_resized_crop_batch with given draws, whole and as a
    shard with index_base = 1000, bit for bit the CPU restatements of tests/test_data_gpu.py and tests/test_resample_gpu.py;
    an index below the shard gives a zero image and label -1."""
    from nbdt import data as D
    from test_data_gpu import TINY, restate
    from test_resample_gpu import MEAN, STD, normalise
    N, S = L.DATA_N, L.DATA_SIDE
    n = 3 * S * S
    a = Arena("resident_dataset")
    src = a.tensor("src", (N, 3, S, S), torch.uint8)
    pos7 = 7 * torch.arange(n, device=DEV).view(1, -1)
    flat = src.view(N, n)
    for i0 in range(0, N, 8192):
        i = torch.arange(i0, min(i0 + 8192, N), device=DEV).view(-1, 1)
        flat[i0:i0 + i.shape[0]] = ((131 * i + pos7) & 255).to(torch.uint8)
    labels = ((torch.arange(N) * 7) % 200).to(DEV)
    r31, r32 = (1 << 31) // n, (1 << 32) // n                # the rows that hold bytes 2^31 and 2^32
    assert r31 * n < (1 << 31) < (r31 + 1) * n and r32 * n < (1 << 32) < (r32 + 1) * n < N * n
    special = [0, 1, 2, r31 - 1, r31, r31 + 1, r32 - 1, r32, r32 + 1, N - 2, N - 1]
    g = torch.Generator().manual_seed(3)
    index = torch.tensor(special + torch.randint(0, N, (64 - len(special),), generator=g).tolist())
    B = len(index)
    rows, rows_y = _dataset_rows(index), (index * 7) % 200
    pad = TINY["pad"]
    params = torch.stack([torch.randint(0, 2 * pad + 1, (B,), generator=g), torch.randint(0, 2 * pad + 1, (B,), generator=g),
                          torch.randint(0, 2, (B,), generator=g)], 1).to(torch.int8)
    want, want_y = restate(rows, rows_y, torch.arange(B), params, TINY["mean"], TINY["std"], pad)
    hw = torch.randint(8, S + 1, (B, 2), generator=g)
    tl = (torch.rand(B, 2, generator=g) * (S + 1 - hw)).long()
    boxes = torch.cat([tl, hw, torch.randint(0, 2, (B, 1), generator=g)], 1).to(torch.int32)
    want_rc = normalise(np.stack([D.resample_reference(rows[j].numpy(), tuple(boxes[j, :4].tolist()), (32, 32)) for j in range(B)]),
                        flip=boxes[:, 4])
    base = 1000
    in_shard = (index >= base)
    assert int((~in_shard).sum()) >= 3           # rows 0, 1, 2 (and whatever else the draw put below the shard)
    idx_d, par_d, box_d = index.to(DEV), params.to(DEV), boxes.to(DEV)
    for index_base in (None, base):
        s_src, s_lab = (src, labels) if index_base is None else (src[base:], labels[base:])
        keep = torch.ones(B, dtype=torch.bool) if index_base is None else in_shard
        exp_y = torch.where(keep, want_y, torch.full_like(want_y, -1))
        for what in ("augment", "policy", "resized_crop"):
            side = 32 if what == "resized_crop" else S
            img = torch.full((B, 3, side, side), NAN, device=DEV)
            tgt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
            if what == "augment":
                ops.augment_batch(s_src, s_lab, idx_d, img, tgt, pad, True, mean=TINY["mean"], std=TINY["std"],
                                  params_in=par_d, index_base=index_base)
            elif what == "policy":
                ops.policy_batch(s_src, s_lab, idx_d, img, tgt, pad, True, TINY["mean"], TINY["std"], params_in=par_d,
                                 index_base=index_base)
            else:
                ops.resized_crop_batch(s_src, s_lab, idx_d, img, tgt, (32, 32), (0, 0), True, MEAN, STD, params_in=box_d,
                                       index_base=index_base)
            exp = (want_rc if what == "resized_crop" else want) * keep.view(-1, 1, 1, 1)
            got = img.cpu()
            assert torch.equal(got[keep], exp[keep]) and not got[~keep].any(), (what, index_base)
            assert torch.equal(tgt.cpu(), exp_y), (what, index_base)
    a.assert_margins_clean()


def test_the_comparison_notices_one_element_and_one_sentinel_word():
    """The checks of this module on a fabricated output: one NaN (a store that never happened) or one wrong element at the
    far end of a 2^31 - 2^18 element tensor fails _assert_tiled, one byte in either margin fails the arena."""
    a = Arena("bn_stats_apply")
    B, side, _, C = L.row("bn_tensor")[4]
    y = a.tensor("y", (B, side + 2, side + 2, C))
    ref3 = torch.randn(3, side, side, C, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).double()
    p3 = ops.padded(3, side, side, C, DEV)
    ops.interior(p3).copy_(ref3.to(DEV))
    _tile_into(y, p3)
    tol = _tol_backbone(ref3, B)
    _assert_tiled(y, ref3, tol, "fabricated")
    _border_zero(y)
    a.assert_margins_clean()
    for value in (NAN, 1e3):
        keep = y[B - 2, side, side, C - 1].clone()
        y[B - 2, side, side, C - 1] = value
        with pytest.raises(AssertionError, match="1 of"):
            _assert_tiled(y, ref3, tol, "fabricated")
        y[B - 2, side, side, C - 1] = keep
    y[B - 1, side + 1, 5, 7] = 1.0
    with pytest.raises(AssertionError):
        _border_zero(y)
    for margin in (a.front, a.back):
        margin.view(torch.uint8)[-1] ^= 1
        with pytest.raises(AssertionError, match="sentinel"):
            a.assert_margins_clean()
        margin.view(torch.uint8)[-1] ^= 1
    a.assert_margins_clean()
