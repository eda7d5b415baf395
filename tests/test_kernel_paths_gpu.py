"""Per-op parity for kernel paths the rest of the suite never selects: the nontemporal (NT) BatchNorm passes, the SE
parameter gradient on its own, the order of nbdt_bn_act_se_bwd_apply's argument checks, the batched weight-copy
launches, the pooled head's elementwise backward on its own, the stride-2 1x1 forward over the space-to-depth copy, and
EfficientNet-B0's depthwise / SE kernels at the batch sizes the benchmark runs.

Every check compares a HIP entry point with an independent reference: fp32 / fp64 PyTorch on the same bf16-rounded
inputs, or -- where two forms of a kernel must agree exactly -- the other form, bit for bit."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt._C import NBDTHipError, lib, ptr  # noqa: E402

DEV = "cuda:0"
PLAIN = 2 ** 62          # a threshold no tensor reaches: plain loads


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _act(B, H, W, C, g, scale=1.0, shift=0.0):
    p = ops.padded(B, H, W, C, DEV)
    ops.interior(p).copy_(torch.randn(B, H, W, C, generator=g, device=DEV) * scale + shift)
    return p


def _bn_params(C, g):
    mean = torch.randn(C, generator=g, device=DEV) * 0.1
    rstd = torch.rand(C, generator=g, device=DEV) + 0.5
    gamma = torch.randn(C, generator=g, device=DEV)
    beta = torch.randn(C, generator=g, device=DEV) * 0.3
    return mean, rstd, gamma, beta


def _close_bf16(got, ref, what, rel=2.0 ** -7, abs_mean=2e-2):
    got, ref = got.float(), ref.float()
    tol = rel * ref.abs() + abs_mean * ref.abs().mean() + 1e-6
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {(got - ref).abs().max().item():.4g}"


def _with_threshold(nbytes, fn):
    """fn() with the NT threshold at nbytes; the threshold is restored whatever happens."""
    old = ops.stream_nt_min_bytes()
    ops.set_stream_nt_min_bytes(nbytes)
    try:
        return fn()
    finally:
        ops.set_stream_nt_min_bytes(old)


def _nt_and_plain(fn):
    """fn() once with nontemporal loads forced, once with plain loads forced; the readback proves which one ran."""
    outs = []
    for thr, want in ((0, True), (PLAIN, False)):
        outs.append(_with_threshold(thr, fn))
        assert ops.last_stream_nt() is want, thr
    return outs


# ------------------------------------------------------------------------------------------------------------------------
# A. nontemporal BatchNorm passes

NT_SHAPES = [   # B, H, W, C: every C class of the launchers' layouts, odd B, last block not full
    (5, 4, 4, 8), (3, 32, 32, 32), (7, 8, 8, 160), (3, 6, 10, 640), (5, 4, 4, 2048), (9, 13, 7, 160),
]


@pytest.mark.parametrize("B,H,W,C", NT_SHAPES)
def test_nontemporal_batchnorm_passes_are_bit_equal_to_plain_loads(B, H, W, C):
    """nbdt_bn_apply, nbdt_bn_bwd_apply_cus, nbdt_bn_bwd_reduce_cus and nbdt_bn_bwd_cus take a <..., NT=true>
    instantiation for tensors >= the threshold.  Threshold 0 (NT) and 2^62 (plain) on identical inputs: y / gx, dsum,
    dgamma, dbeta bit-equal, for every variant (relu / residual / gx_add).  The reductions run in deterministic mode (the
    slot order of their atomics is otherwise not reproducible); the elementwise passes in the default mode."""
    g = _gen(B * 1000 + C)
    x, gy, add, res = _act(B, H, W, C, g, 2.0, 0.3), _act(B, H, W, C, g), _act(B, H, W, C, g), _act(B, H, W, C, g)
    mean, rstd, gamma, beta = _bn_params(C, g)
    part = torch.randn(((B * H * W + 255) // 256) * 2 * C, generator=g, device=DEV)

    for relu in (True, False):
        for r in (None, res):
            def apply():
                y = ops.padded(B, H, W, C, DEV)
                ops.bn_apply(x, mean, rstd, gamma, beta, y, relu=relu, residual=r)
                return y
            a, b = _nt_and_plain(apply)
            assert a.float().abs().max().item() > 0
            assert torch.equal(a, b), ("bn_apply", relu, r is not None)

    for gx_add in (None, add):
        def fused():       # nbdt_bn_bwd_fold + nbdt_bn_bwd_apply_cus
            dsum, dg, db = torch.empty(2 * C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV)
            gx = ops.padded(B, H, W, C, DEV)
            ops.bn_bwd_fused(gy, x, mean, rstd, gamma, beta, part, dsum, dg, db, gx, gx_add=gx_add, cus=48)
            return dsum, dg, db, gx
        a, b = _nt_and_plain(fused)
        assert a[3].float().abs().max().item() > 0
        for u, v in zip(a, b):
            assert torch.equal(u, v), ("bn_bwd_apply_cus", gx_add is not None)

    scratch = torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV)
    pair = (torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV), torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV))
    ops.set_deterministic(True)
    try:
        for gx_add in (None, add):
            for sc in (scratch, pair):        # reduce_cus + apply_cus, or nbdt_bn_bwd_cus
                for cus in (7, 256):
                    def whole():
                        dsum, dg, db = torch.empty(2 * C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV)
                        gx = ops.padded(B, H, W, C, DEV)
                        ops.bn_bwd_cus(gy, x, mean, rstd, gamma, beta, sc, dsum, dg, db, gx, cus, gx_add=gx_add)
                        if sc is pair:
                            pair[0].zero_()          # (the buffer this call summed into: clean for the next call)
                        return dsum, dg, db, gx
                    a, b = _nt_and_plain(whole)
                    assert a[0].abs().max().item() > 0 and a[3].float().abs().max().item() > 0
                    for u, v in zip(a, b):
                        assert torch.equal(u, v), ("bn_bwd_cus" if sc is pair else "bn_bwd_reduce_cus", gx_add is not None, cus)
    finally:
        ops.set_deterministic(False)


def _bn_bwd_ref(gy, x, mean, rstd, gamma, beta, B, H, W, C):
    """fp64 BatchNorm + ReLU backward (mask recomputed from x, as the CU-subset passes do) on padded bf16 tensors.
    Returns dsum [2C], gx, and per channel the |terms| of elements whose mask fp32 rounding may flip (the tolerance)."""
    xi = ops.interior(x).double()
    gi = ops.interior(gy).double()
    sc, sh = (gamma * rstd), (beta - mean * (gamma * rstd))
    pre = xi * sc.double() + sh.double()
    near = pre.abs() <= 1e-6 * (sh.double().abs() + (xi * sc.double()).abs()) + 1e-30
    gg = torch.where(pre > 0, gi, torch.zeros_like(gi))
    xhat = (xi - mean.double()) * rstd.double()
    s0, s1 = gg.sum((0, 1, 2)), (gg * xhat).sum((0, 1, 2))
    n = B * H * W
    gx = sc.double() * (gg - s0 / n - xhat * s1 / n)
    amb = (gi.abs() * near).sum((0, 1, 2)), (gi.abs() * xhat.abs() * near).sum((0, 1, 2))
    absum = gg.abs().sum((0, 1, 2)), (gg * xhat).abs().sum((0, 1, 2))
    return torch.cat([s0, s1]), gx, torch.cat(amb), torch.cat(absum), near


def test_nontemporal_threshold_default_and_its_exact_boundary():
    """Default threshold 96 MiB.  384 x 30 x 30 x 128 bf16 images padded to 32 x 32 are exactly 96 MiB (NT); 383 of them
    are one image less (plain).  nbdt_bn_apply: the first 383 images of both runs bit-equal.  nbdt_bn_bwd_cus and
    nbdt_bn_bwd_reduce_cus + _apply_cus (sums over 384 vs 383 images, so no bit-equality): each run against fp64."""
    assert ops.stream_nt_min_bytes() == 96 << 20
    B, H, W, C = 384, 30, 30, 128
    assert B * (H + 2) * (W + 2) * C * 2 == 96 << 20
    g = _gen(96)
    x, gy = _act(B, H, W, C, g, 2.0, 0.3), _act(B, H, W, C, g)
    mean, rstd, gamma, beta = _bn_params(C, g)

    ys = []
    for b, want in ((B, True), (B - 1, False)):
        y = ops.padded(b, H, W, C, DEV)
        ops.bn_apply(x[:b], mean, rstd, gamma, beta, y, relu=True)
        assert ops.last_stream_nt() is want, b
        ys.append(y)
    assert ys[0].float().abs().max().item() > 0
    assert torch.equal(ys[0][:B - 1], ys[1])
    del ys

    scratch = torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV)
    pair = (torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV), torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV))
    for b, want in ((B, True), (B - 1, False)):
        ref, gx_ref, amb, absum, near = _bn_bwd_ref(gy[:b], x[:b], mean, rstd, gamma, beta, b, H, W, C)
        tol = 2e-5 * absum + amb + 1e-4
        for sc in (scratch, pair):
            dsum, dg, db = torch.empty(2 * C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV)
            gx = ops.padded(b, H, W, C, DEV)
            ops.bn_bwd_cus(gy[:b], x[:b], mean, rstd, gamma, beta, sc, dsum, dg, db, gx, 256)
            assert ops.last_stream_nt() is want, b
            if sc is pair:
                pair[0].zero_()
            assert ((dsum.double() - ref).abs() <= tol).all(), (b, (dsum.double() - ref).abs().max().item())
            assert ((db.double() - 1 - ref[:C]).abs() <= tol[:C] + 1e-6 * absum[:C]).all(), b
            assert ((dg.double() - 1 - ref[C:]).abs() <= tol[C:] + 1e-6 * absum[C:]).all(), b
            got = ops.interior(gx).double()
            err = (got - gx_ref).abs()
            ok = (err <= 2.0 ** -7 * gx_ref.abs() + 1e-3 * gx_ref.abs().mean()) | near
            assert ok.all(), (b, int((~ok).sum()))
            del gx, got, err, ok


# ------------------------------------------------------------------------------------------------------------------------
# B. SE parameter gradients; argument checks before the first launch

SE_SIZES = [(32, 32, 8), (160, 144, 6), (1152, 1152, 48)]     # C, Cr (real channels), S


def _se_case(B, C, Cr, S, seed):
    """fp64 autograd of the SE MLP pre2 = w2 @ swish(w1 @ pooled[:Cr] + b1) + b2 for an upstream gradient dpre2.
    Returns the kernel inputs (fp32, device) and the four fp64 parameter gradients."""
    g = torch.Generator().manual_seed(seed)
    pooled = torch.zeros(B, C, dtype=torch.float64)
    pooled[:, :Cr] = torch.randn(B, Cr, generator=g, dtype=torch.float64)
    w1 = (torch.randn(S, Cr, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    b1 = (torch.randn(S, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    w2 = (torch.randn(Cr, S, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    b2 = (torch.randn(Cr, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    dpre2 = torch.randn(B, Cr, generator=g, dtype=torch.float64)
    pre1 = pooled[:, :Cr] @ w1.t() + b1
    pre1.retain_grad()
    pre2 = (pre1 * torch.sigmoid(pre1)) @ w2.t() + b2
    pre2.backward(dpre2)
    d = lambda v: v.detach().float().to(DEV).contiguous()
    inputs = (d(dpre2), d(pre1.grad), d(pre1), d(pooled))
    return inputs, [v.grad for v in (w1, b1, w2, b2)], (w1, b1, w2, b2)


@pytest.mark.parametrize("C,Cr,S", SE_SIZES)
@pytest.mark.parametrize("B", [5, 16, 17, 128])
def test_se_parameter_gradient_over_batch_chunks(B, C, Cr, S):
    """nbdt_se_param_grad folds the batch in chunks of 16 images with atomics (one chunk in deterministic mode): one
    chunk, exactly one, a ragged last chunk, eight.  Against fp64 autograd, in both modes, twice (the second call adds);
    and equal to the parameter outputs of the fused nbdt_se_gate_bwd on the data gradients that call computes."""
    (dpre2, dpre1, pre1, pooled), want, _ = _se_case(B, C, Cr, S, seed=B * 7 + S)
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            grads = [torch.zeros(S, Cr, device=DEV), torch.zeros(S, device=DEV), torch.zeros(Cr, S, device=DEV),
                     torch.zeros(Cr, device=DEV)]
            ops.se_param_grad(dpre2, dpre1, pre1, pooled, *grads, Cr)
            once = [v.clone() for v in grads]
            ops.se_param_grad(dpre2, dpre1, pre1, pooled, *grads, Cr)
        finally:
            ops.set_deterministic(False)
        for name, a, two, w in zip(("dw1", "db1", "dw2", "db2"), once, grads, want):
            scale = w.abs().max().item()
            err = (a.double().cpu() - w).abs().max().item()
            assert err <= 2e-5 * scale + 1e-6, (name, det, err, scale)
            assert (two.double().cpu() - 2 * w).abs().max().item() <= 4e-5 * scale + 2e-6, (name, det)

    # the fused form: the same sums as se_gate_bwd's own parameter outputs (deterministic: bit for bit)
    g = torch.Generator().manual_seed(B + C)
    w1, b1 = torch.randn(S, Cr, generator=g) * 0.3, torch.randn(S, generator=g) * 0.1
    w2, b2 = torch.randn(Cr, S, generator=g) * 0.3, torch.randn(Cr, generator=g) * 0.1
    w1, b1, w2, b2 = (v.to(DEV) for v in (w1, b1, w2, b2))
    dgate = torch.randn(B, C, generator=g).to(DEV)
    p1, gate = torch.empty(B, S, device=DEV), torch.empty(B, C, device=DEV)
    ops.se_gate_fwd(pooled, w1, b1, w2, b2, p1, gate, Cr)
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            fused = [torch.zeros(S, Cr, device=DEV), torch.zeros(S, device=DEV), torch.zeros(Cr, S, device=DEV),
                     torch.zeros(Cr, device=DEV)]
            e2, e1, gpool = torch.empty(B, Cr, device=DEV), torch.empty(B, S, device=DEV), torch.empty(B, C, device=DEV)
            ops.se_gate_bwd(dgate, gate, p1, pooled, w1, w2, e2, e1, gpool, *fused, Cr)
            sep = [torch.zeros_like(v) for v in fused]
            ops.se_param_grad(e2, e1, p1, pooled, *sep, Cr)
        finally:
            ops.set_deterministic(False)
        for a, b in zip(fused, sep):
            if det:
                assert torch.equal(a, b)
            else:
                assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())


def test_refused_se_backward_apply_leaves_its_buffers_untouched():
    """nbdt_bn_act_se_bwd_apply's first kernel consumes and zeroes `sums` and adds into dgamma / dbeta.  A call refused
    for a null gx, a null x or an unknown activation must refuse before that kernel: sums, dsum, dgamma, dbeta
    byte-identical afterwards, and a valid retry then matches autograd (not twice the parameter gradients)."""
    B, C, H, W = 4, 32, 8, 8
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.3).to(torch.bfloat16).float()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    gate, gpool = torch.rand(B, C, generator=g), torch.randn(B, C, generator=g)
    gu = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16).float()
    xp, gup = ops.padded(B, H, W, C, DEV), ops.padded(B, H, W, C, DEV)
    ops.interior(xp).copy_(x.permute(0, 2, 3, 1).to(DEV))
    ops.interior(gup).copy_(gu.permute(0, 2, 3, 1).to(DEV))
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.bn_stats(xp, torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV), mean, rstd)
    gd, bd, gate_d, gpool_d = gamma.to(DEV), beta.to(DEV), gate.to(DEV), gpool.to(DEV)
    sums = torch.zeros((5, B, C), device=DEV)
    ops.bn_act_se_sums(gup, xp, mean, rstd, gd, bd, sums)
    dsum = torch.full((2 * C,), 3.0, device=DEV)
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gx = ops.padded(B, H, W, C, DEV)
    before = [t.clone() for t in (sums, dsum, dgamma, dbeta)]
    assert sums.abs().max().item() > 0

    def unchanged(what):
        for t, b in zip((sums, dsum, dgamma, dbeta), before):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32)), what

    with pytest.raises(NBDTHipError, match="null argument"):
        ops.bn_act_se_bwd_apply(gup, gate_d, gpool_d, sums, xp, mean, rstd, gd, bd, dsum, dgamma, dbeta, None)
    unchanged("null gx")
    with pytest.raises(NBDTHipError, match="null argument"):
        _C.check(lib().nbdt_bn_act_se_bwd_apply(ptr(gup), ptr(gate_d), ptr(gpool_d), ptr(sums), None, ptr(mean),
                                                ptr(rstd), ptr(gd), ptr(bd), ops.ACT_SWISH, B, H, W, C, ptr(dsum),
                                                ptr(dgamma), ptr(dbeta), ptr(gx), ops.stream_ptr(xp.device)))
    unchanged("null x")
    with pytest.raises(NBDTHipError, match="unknown activation"):
        ops.bn_act_se_bwd_apply(gup, gate_d, gpool_d, sums, xp, mean, rstd, gd, bd, dsum, dgamma, dbeta, gx, act=7)
    unchanged("act 7")

    ops.bn_act_se_bwd_apply(gup, gate_d, gpool_d, sums, xp, mean, rstd, gd, bd, dsum, dgamma, dbeta, gx)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.batch_norm(xr, None, None, gr, br, True, 0.0, 1e-5)
    a = a * torch.sigmoid(a)
    (a * gate[:, :, None, None]).backward(gu, retain_graph=True)
    a.mean((2, 3)).backward(gpool)
    got_gx = ops.interior(gx).float().permute(0, 3, 1, 2).cpu()
    assert (got_gx - xr.grad).abs().max().item() < 2e-2 * xr.grad.abs().max().item() + 1e-3
    assert (dgamma.cpu() - gr.grad).abs().max().item() < 5e-3 * gr.grad.abs().max().item() + 1e-3
    assert (dbeta.cpu() - br.grad).abs().max().item() < 5e-3 * br.grad.abs().max().item() + 1e-3
    assert sums.abs().max().item() == 0


# ------------------------------------------------------------------------------------------------------------------------
# D. wrappers no other test calls

def test_batched_dgrad_weight_copies_equal_per_layer_weight_prep():
    """nbdt_weight_prep_batched over a table of four layers (3x3 and 1x1, couts that are and are not multiples of 64 /
    160) writes exactly what nbdt_weight_prep writes layer by layer."""
    layers = [(160, 9, 160), (96, 1, 64), (320, 9, 32), (32, 1, 96)]          # cout, taps, cin
    g = torch.Generator().manual_seed(1)
    ws = [torch.randn(co * t * ci, generator=g) for co, t, ci in layers]
    flat = torch.cat([torch.zeros(8)] + ws).to(DEV)      # (layers at nonzero offsets)
    rows, src, dst, tiles = [], 8, 0, 0
    for (co, t, ci), w in zip(layers, ws):
        rows.append([src, dst, co, t, ci, tiles])
        src += w.numel()
        dst += w.numel()
        tiles += t * ((co + 63) // 64) * (ci // 32)
    wd_flat = torch.full((dst,), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.weight_prep_batched(flat, torch.tensor(rows, dtype=torch.int64, device=DEV), len(layers), tiles, wd_flat)
    for (co, t, ci), w, r in zip(layers, ws, rows):
        wd = torch.empty(ci, t, co, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(w.to(DEV), co, t, ci, None, wd)
        assert torch.equal(wd_flat[r[1]:r[1] + w.numel()], wd.reshape(-1)), (co, t, ci)
        ref = w.view(co, t, ci).to(torch.bfloat16).flip(1).permute(2, 1, 0).reshape(-1)
        assert torch.equal(wd.reshape(-1).cpu(), ref)


def test_batched_weight_tiles_equal_concatenated_single_matrix_tiles():
    """nbdt_weight_tile_batched with n = 4 matrices (cout tiles nt = 5, 2, 1, 4) equals weight_tiles of each matrix."""
    mats = [(160, 64), (64, 32), (96, 160), (128, 96)]       # rows, k
    g = torch.Generator().manual_seed(2)
    ws = [torch.randn(r, 9, k, generator=g).to(torch.bfloat16).to(DEV) for r, k in mats]
    src = torch.cat([torch.zeros(16, dtype=torch.bfloat16, device=DEV)] + [w.reshape(-1) for w in ws])
    rows, s, d, tiles = [], 16, 0, 0
    for (r, k), w in zip(mats, ws):
        r32 = r // 32
        nt = 5 if r32 % 5 == 0 else 4 if r32 % 4 == 0 else 2 if r32 % 2 == 0 else 1
        rows.append([s, d, r, k, tiles])
        s += w.numel()
        d += w.numel()
        tiles += (r // (32 * nt)) * (k // 32) * 9
    dst = torch.full((d,), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.weight_tile_batched(src, torch.tensor(rows, dtype=torch.int64, device=DEV), len(mats), tiles, dst)
    assert torch.equal(dst, torch.cat([ops.weight_tiles(w) for w in ws]))


@pytest.mark.parametrize("B,H,W,C", [(5, 8, 8, 160), (3, 4, 4, 640), (7, 5, 3, 32)])
def test_pooled_head_backward_elementwise_pass_alone(B, H, W, C):
    """nbdt_pool_bn_bwd_apply with the caller's sums against autograd of avgpool(relu(bn(x))): with the real batch sums
    (nonzero dsum), and in ResNet's identity form (mean 0, rstd 1, gamma 1, beta 0, dsum 0 = relu + average pool)."""
    g = torch.Generator().manual_seed(B * C)
    x = (torch.randn(B, H, W, C, generator=g) * 2 + 0.3).to(torch.bfloat16).float()
    gpool = torch.randn(B, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    xp = ops.padded(B, H, W, C, DEV)
    ops.interior(xp).copy_(x.to(DEV))
    x64 = x.double().permute(0, 3, 1, 2)
    mean = x64.mean((0, 2, 3))
    rstd = (x64.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()

    xr, gr, br = x64.clone().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = F.batch_norm(xr, None, None, gr, br, True, 0.0, 1e-5)
    F.relu(pre).mean((2, 3)).backward(gpool.double())
    # the batch sums the reduce pass would give: sum g', sum g' * xhat with g' = relu mask * gpool / HW
    gg = (pre.detach() > 0).double() * gpool.double()[:, :, None, None] / (H * W)
    xhat = (x64 - mean[None, :, None, None]) * rstd[None, :, None, None]
    dsum = torch.cat([gg.sum((0, 2, 3)), (gg * xhat).sum((0, 2, 3))]).float().to(DEV)
    gx = ops.padded(B, H, W, C, DEV)
    ops.pool_bn_bwd_apply(gpool.to(DEV), xp, mean.float().to(DEV), rstd.float().to(DEV), gamma.to(DEV), beta.to(DEV),
                          dsum, gx)
    near = (pre.detach().abs() < 1e-4).permute(0, 2, 3, 1)
    ref = xr.grad.permute(0, 2, 3, 1)
    got = ops.interior(gx).double().cpu()
    ok = ((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-3 * ref.abs().mean()) | near
    assert ok.all(), f"{int((~ok).sum())} off"
    assert dsum.abs().max().item() > 0

    # identity form: the average pool's gradient through relu, to its bf16 store (one rounding of gpool / HW)
    xr2 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    F.relu(xr2).mean((2, 3)).backward(gpool.double())
    gx2 = ops.padded(B, H, W, C, DEV)
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ops.pool_bn_bwd_apply(gpool.to(DEV), xp, zeros, ones, ones, zeros, torch.zeros(2 * C, device=DEV), gx2)
    want = xr2.grad.permute(0, 2, 3, 1)
    got2 = ops.interior(gx2).double().cpu()
    assert ((got2 - want).abs() <= 2.0 ** -8 * want.abs()).all()
    assert torch.equal(got2 == 0, want == 0)


@pytest.mark.parametrize("B,Hi,Wi,cin,cout", [(2, 32, 32, 32, 160), (2, 32, 32, 160, 320), (2, 16, 16, 320, 640),
                                               (3, 10, 14, 64, 96)])
def test_stride2_1x1_forward_over_space_to_depth(B, Hi, Wi, cin, cout):
    """conv_igemm with conv_fwd_desc_s2d_1x1 over the space-to-depth copy (all four phases filled: only phase (0, 0)
    may be read) against F.conv2d(stride=2) of a 1x1: WRN-28-10's shortcut shapes scaled down, and a ragged M of 105."""
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, Hi, Wi, cin, generator=g).to(torch.bfloat16).float()
    w = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(torch.bfloat16).float()
    xs = ops.s2d_buffer(B, Hi, Wi, cin, DEV)
    xsi = ops.interior(xs)
    for p in (0, 1):
        for q in (0, 1):
            xsi[..., (2 * p + q) * cin:(2 * p + q + 1) * cin] = x[:, p::2, q::2, :].to(DEV)
    wb = w.view(cout, 1, cin).to(torch.bfloat16).to(DEV)
    Ho, Wo = Hi // 2, Wi // 2
    out = ops.padded(B, Ho, Wo, cout, DEV)
    ops.conv_igemm(ops.conv_fwd_desc_s2d_1x1(B, Hi, Wi, cin, cout), xs, wb, out)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=2).permute(0, 2, 3, 1)
    _close_bf16(ops.interior(out).cpu(), ref, "s2d 1x1 stride-2 forward")
    t = out.float()
    assert t[:, 0].abs().max() == 0 and t[:, -1].abs().max() == 0 and t[:, :, 0].abs().max() == 0


# ------------------------------------------------------------------------------------------------------------------------
# F. EfficientNet-B0 layers at the benchmarked batch

B0_LAYERS = [   # B, H, W (input), C, k, stride
    (128, 112, 112, 96, 3, 2), (128, 56, 56, 144, 3, 2), (128, 28, 28, 240, 5, 1), (128, 7, 7, 1152, 5, 1),
    (512, 28, 28, 240, 5, 1),
]


def _chunks(B, n=32):
    return [(i, min(i + n, B)) for i in range(0, B, n)]


@pytest.mark.parametrize("B,H,W,C,k,stride", B0_LAYERS)
def test_depthwise_kernels_at_the_benchmarked_batch(B, H, W, C, k, stride):
    """nbdt_dwconv_fwd / _bwd_data / _bwd_weight (default and deterministic) at EfficientNet-B0 layer shapes and 128 /
    512 images, where the XCD-contiguous block order over (slices, B) and the weight gradient's batch chunks are those
    of the benchmark: against fp32 torch in image chunks, weight-gradient chunks summed in fp64."""
    g = _gen(B + C + k)
    Ho, Wo = H // stride, W // stride
    xp, gyp = _act(B, H, W, C, g), _act(B, Ho, Wo, C, g)
    w = torch.randn(C, 1, k, k, generator=g, device=DEV) * 0.3
    wt = w.view(C, k * k).t().contiguous()
    y = ops.padded(B, Ho, Wo, C, DEV)
    ops.dwconv_fwd(xp, wt, y, k, stride)
    gx = ops.padded(B, H, W, C, DEV)
    ops.dwconv_bwd_data(gyp, wt, gx, k, stride)
    dws = {}
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dws[det] = torch.zeros(k * k, C, device=DEV)
            ops.dwconv_bwd_weight(xp, gyp, dws[det], k, stride)
        finally:
            ops.set_deterministic(False)
    dw_ref = torch.zeros(C, 1, k, k, dtype=torch.float64, device=DEV)
    for b0, b1 in _chunks(B):
        xc = ops.interior(xp[b0:b1]).float().permute(0, 3, 1, 2)
        gc = ops.interior(gyp[b0:b1]).float().permute(0, 3, 1, 2)
        yr = F.conv2d(xc, w, None, stride, k // 2, 1, C)
        _close_bf16(ops.interior(y[b0:b1]).permute(0, 3, 1, 2), yr, f"dw fwd images {b0}..{b1}", abs_mean=1e-3)
        gr = torch.nn.grad.conv2d_input(xc.shape, w, gc, stride, k // 2, 1, C)
        _close_bf16(ops.interior(gx[b0:b1]).permute(0, 3, 1, 2), gr, f"dw bwd_data images {b0}..{b1}", abs_mean=1e-3)
        dw_ref += torch.nn.grad.conv2d_weight(xc, w.shape, gc, stride, k // 2, 1, C).double()
        del xc, gc, yr, gr
    want = dw_ref.view(C, k * k).t()
    scale = want.abs().max().item()
    for det, dw in dws.items():
        err = (dw.double() - want).abs().max().item()
        assert err <= 1e-4 * scale, (det, err, scale)
    for t in (y, gx):
        assert t[:, 0].abs().max().item() == 0 and t[:, :, -1].abs().max().item() == 0


SE_LAYERS = [(128, 56, 56, 96), (128, 28, 28, 144), (128, 28, 28, 240), (128, 7, 7, 1152), (512, 28, 28, 240)]


@pytest.mark.parametrize("B,H,W,C", SE_LAYERS)
def test_se_sums_at_the_benchmarked_batch(B, H, W, C):
    """nbdt_bn_act_se_sums (dL/dgate and the BatchNorm sums of the SE-scaled activation, one block per (slice, image))
    + nbdt_bn_act_se_bwd_apply at 128 / 512 images against fp32 autograd through swish(bn(x)) * gate and the pooled
    branch."""
    g = _gen(B * 3 + C)
    xp, gup = _act(B, H, W, C, g, 2.0, 0.3), _act(B, H, W, C, g)
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.2
    gate = torch.rand(B, C, generator=g, device=DEV)
    gpool = torch.randn(B, C, generator=g, device=DEV)
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.bn_stats(xp, torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV), mean, rstd)
    sums = torch.zeros((5, B, C), device=DEV)
    ops.bn_act_se_sums(gup, xp, mean, rstd, gamma, beta, sums)
    dgate = sums[0].clone()
    dsum, dgamma, dbeta = torch.empty(2 * C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gx = ops.padded(B, H, W, C, DEV)
    ops.bn_act_se_bwd_apply(gup, gate, gpool, sums, xp, mean, rstd, gamma, beta, dsum, dgamma, dbeta, gx)
    assert sums.abs().max().item() == 0

    x = ops.interior(xp).float().permute(0, 3, 1, 2)
    gu = ops.interior(gup).float().permute(0, 3, 1, 2)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.batch_norm(xr, None, None, gr, br, True, 0.0, 1e-5)
    a = a * torch.sigmoid(a)
    want_dgate = (a.detach().double() * gu.double()).sum((2, 3))
    (a * gate[:, :, None, None]).backward(gu, retain_graph=True)
    a.mean((2, 3)).backward(gpool)
    assert (dgate.double() - want_dgate).abs().max().item() < 2e-3 * max(1.0, want_dgate.abs().max().item())
    scale = xr.grad.abs().max().item()
    assert (ops.interior(gx).float().permute(0, 3, 1, 2) - xr.grad).abs().max().item() < 2e-2 * scale + 1e-3
    assert (dgamma - gr.grad).abs().max().item() < 5e-3 * gr.grad.abs().max().item() + 1e-3
    assert (dbeta - br.grad).abs().max().item() < 5e-3 * br.grad.abs().max().item() + 1e-3
