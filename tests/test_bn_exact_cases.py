"""The fixtures of tests/test_bn_exact_gpu.py, checked on the host: the values are the exactly representable ones the
method needs, every per-channel sum meets the 2^24 condition, the float64 references are F.batch_norm's, and an fp32
restatement of the kernels' expressions -- sums taken in shuffled orders -- reproduces the references as closely as the
GPU tests demand of the kernels: bit for bit where they ask for bits, inside the half-ulp bound elsewhere."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_exact_cases as E  # noqa: E402

IDS = [E.shape_id(s) for s in E.SHAPES]
BWD_FORMS = [dict(relu=True, mask_res=True), dict(relu=True, mask_res=False), dict(relu=False, mask_res=False)]

# the restatement runs at 16 channels and every pixel count of the GPU tests' grids, plus one that is neither a power of
# two nor a multiple of anything (36913 images of one pixel)
RESTATE_GRIDS = E.POW2_GRIDS + E.RESNET_GRIDS + ((2, 8, 16), (36913, 1, 1))


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_fixture_values_and_exactness_conditions(shape):
    """Every GPU fixture (they are built on the host, from the same seeds): value ranges, bf16 representability, the 2^24
    condition of every sum, and -- inside ref_bwd -- the coverage guards (the ReLU mask of every channel takes both
    values, at most a quarter of the channels have a zero sum) and, at power-of-two n, fp32 exactness of gx."""
    f = E.make(*shape)
    E.assert_values(f)
    E.assert_sums_exact(f)
    for form in BWD_FORMS:
        for with_add in (False, True):
            r = E.ref_bwd(f, with_add=with_add, **form)
            assert r["gx"].abs().max().item() > 0
    if f["gpooled"] is not None:
        E.ref_bwd(f, pooled=True)
    for relu in (True, False):
        for with_res in (True, False):
            assert E.ref_apply(f, relu, with_res).abs().max().item() < 32
    st = E.ref_stats(f)
    assert (st["sum"] == 0).double().mean().item() <= 0.25
    if f["n"] >= 64:        # statistics input: mean near 2 in even channels, near 0 in odd ones
        assert st["mean"][0::2].min().item() > 1.5 and st["mean"][1::2].abs().max().item() < 1.5


def test_largest_cases_meet_the_condition_by_their_ranges():
    """The grid-cap cases are built on the device; their condition follows from the value ranges alone."""
    for B, H, W, C in E.CAP_CASES:
        n = B * H * W
        assert (E.X_MAX + 1) ** 2 * n < E.EXACT                  # sum x^2 (x_stats reaches 4)
        assert E.G_MAX * (E.X_MAX + 1) * n + 16 < E.EXACT        # sum |g'| |x - mean| + the start value
        assert B * (H + 2) * (W + 2) * C < 2 ** 31
    assert 32 * 458752 < E.EXACT


def test_reference_statistics_are_batch_norms():
    """ref_stats against F.batch_norm in float64 (training mode, the same momentum and eps)."""
    f = E.make(3, 5, 7, 16)
    r = E.ref_stats(f)
    eps, mom = float(torch.tensor(E.EPS, dtype=torch.float32)), E.MOMENTUM
    x = f["x_stats"].double().permute(0, 3, 1, 2)
    rm, rv = f["running_mean"].double().clone(), f["running_var"].double().clone()
    y = F.batch_norm(x, rm, rv, None, None, True, mom, eps)
    torch.testing.assert_close(rm, r["running_mean"], rtol=1e-13, atol=0)
    torch.testing.assert_close(rv, r["running_var"], rtol=1e-13, atol=0)
    mine = (x - r["mean"][None, :, None, None]) * r["rstd"][None, :, None, None]
    torch.testing.assert_close(y, mine, rtol=1e-12, atol=1e-13)


def test_reference_backward_is_autograds():
    """ref_bwd against autograd through F.batch_norm (float64) on statistics-consistent parameters: the fixture's own
    mean / rstd are inputs, not statistics of x, so this takes x's real statistics and compares the same formula."""
    f = E.make(2, 4, 4, 8)
    st = E.ref_stats(f, "x", running=False)
    f["mean"], f["rstd"] = st["mean"], st["rstd"]
    x = f["x"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    res = f["residual"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    eps = float(torch.tensor(E.EPS, dtype=torch.float32))
    y = F.relu(F.batch_norm(x, None, None, f["gamma"].double(), f["beta"].double(), True, 0.1, eps) + res)
    y.backward(f["gy"].double().permute(0, 3, 1, 2))
    n, dims = f["n"], (0, 1, 2)
    sc = f["gamma"].double() * f["rstd"]
    xh = (f["x"].double() - f["mean"]) * f["rstd"]
    pre = xh * f["gamma"].double() + f["beta"].double() + f["residual"].double()
    g = torch.where(pre > 0, f["gy"].double(), torch.zeros(()).double())
    gx = sc * (g - g.sum(dims) / n - xh * (g * xh).sum(dims) / n)
    torch.testing.assert_close(x.grad.permute(0, 2, 3, 1), gx, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(res.grad.permute(0, 2, 3, 1), g, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------------------------------
# the fp32 restatement of the kernels' expressions

def _sum_shuffled(t, gen):
    """Per-channel fp32 sum of t [n][C] in a random order: shuffled rows, then a pairwise tree of fp32 adds."""
    t = t[torch.randperm(t.shape[0], generator=gen)]
    while t.shape[0] > 1:
        if t.shape[0] & 1:
            t = torch.cat((t, t.new_zeros(1, t.shape[1])))
        t = t[0::2] + t[1::2]
    return t[0]


def _sum_strided(t, gen):
    """Another order: `lanes` sequential accumulators over strided rows (a grid-stride loop), then folded in sequence."""
    lanes = int(torch.randint(2, 40, (1,), generator=gen))
    t = t[torch.randperm(t.shape[0], generator=gen)]
    pad = (-t.shape[0]) % lanes
    t = torch.cat((t, t.new_zeros(pad, t.shape[1]))) if pad else t
    t = t.view(-1, lanes, t.shape[1])
    acc = torch.zeros_like(t[0])
    for row in t:
        acc = acc + row
    out = torch.zeros_like(acc[0])
    for lane in acc:
        out = out + lane
    return out


def _restate_bwd(f, sums, gen, relu=True, mask_res=False, with_add=False, pooled=False):
    """bn_bwd_reduce_kernel + bn_bwd_apply_kernel in fp32 tensor ops (every operation rounds to fp32, no fused
    multiply-add): sc = gamma*rstd, sh = beta - mean*sc, k = dsum*(1/n), v = sc*(g' - k0 - xhat*k1) + add."""
    n, C, hw = f["n"], f["C"], f["H"] * f["W"]
    one = torch.ones((), dtype=torch.float32)
    x = f["x"]
    sc = f["gamma"] * f["rstd"]
    sh = f["beta"] - f["mean"] * sc
    if pooled:
        g = (f["gpooled"] * (one / float(hw)))[:, None, None, :].expand(x.shape)
    else:
        g = f["gy"]
    if relu:
        pre = x * sc + sh
        if mask_res:        # the y-mask reads the stored bf16 forward output
            pre = torch.relu(pre + f["residual"]).bfloat16().float()
        g = torch.where(pre > 0, g, torch.zeros((), dtype=torch.float32))
    xh = (x - f["mean"]) * f["rstd"]
    s0, s1 = sums(g.reshape(n, C), gen), sums((g * xh).reshape(n, C), gen)
    inv_n = one / float(n)
    k0, k1 = s0 * inv_n, s1 * inv_n
    v = sc * (g - k0 - xh * k1)
    if with_add:
        v = v + f["gx_add"]
    assert v.dtype == torch.float32 and s0.dtype == torch.float32
    return s0, s1, v.bfloat16(), g.bfloat16()


def _restate_stats(f, sums, gen, eps=E.EPS, momentum=E.MOMENTUM):
    """bn_stats_kernel + bn_finalize_kernel in fp32 tensor ops."""
    n, C = f["n"], f["C"]
    x = f["x_stats"].reshape(n, C)
    s, q = sums(x, gen), sums(x * x, gen)
    nf = torch.tensor(float(n), dtype=torch.float32)
    mean = s / nf
    var = torch.clamp_min(q / nf - mean * mean, 0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    mom = torch.tensor(momentum, dtype=torch.float32)
    unbiased = var * nf / (nf - 1) if n > 1 else var
    rm = (1 - mom) * f["running_mean"] + mom * mean
    rv = (1 - mom) * f["running_var"] + mom * unbiased
    assert rstd.dtype == torch.float32 and rv.dtype == torch.float32
    return s, q, mean, rstd, rm, rv


@pytest.mark.parametrize("grid", RESTATE_GRIDS, ids=lambda g: "b%d_%dx%d" % g)
def test_fp32_restatement_reproduces_the_references(grid):
    """What the GPU tests assert of the kernels holds for a plain fp32 evaluation of the kernels' expressions with the sums
    taken in two shuffled orders: sums bit-equal to the float64 reference at every n; y, g_resid and pooled bit-equal;
    gx bit-equal when n is a power of two and inside 2^-8*|ref| + 2^-21*M, every element, otherwise; mean * n the
    integer sum; rstd / running_var inside ref_stats' bound, running_mean within 3 ulp."""
    f = E.make(*grid, 16)
    n = f["n"]
    E.assert_sums_exact(f)
    gen = torch.Generator().manual_seed(n)
    forms = [dict(with_add=a, **form) for form in BWD_FORMS for a in (False, True)]
    if f["gpooled"] is not None:
        forms.append(dict(pooled=True))
    for sums in (_sum_shuffled, _sum_strided):
        for form in forms:
            r = E.ref_bwd(f, **form)
            s0, s1, gx, g_resid = _restate_bwd(f, sums, gen, **form)
            assert torch.equal(s0.double(), r["s0"]) and torch.equal(s1.double(), r["s1"]), form
            assert torch.equal(g_resid, E.bf16_of(r["g_resid"])), form
            E.check_elementwise(gx, r, str(form))
        s, q, mean, rstd, rm, rv = _restate_stats(f, sums, gen)
        st = E.ref_stats(f)
        assert torch.equal(s.double(), st["sum"]) and torch.equal(q.double(), st["sumsq"])
        E.check_stats(mean, rstd, st, "restatement", n, rm, rv)
    # forward: exact at every n
    sc = f["gamma"] * f["rstd"]
    sh = f["beta"] - f["mean"] * sc
    for relu in (True, False):
        for with_res in (True, False):
            y = f["x"] * sc + sh
            y = y + f["residual"] if with_res else y
            y = torch.relu(y) if relu else y
            assert torch.equal(y.bfloat16(), E.bf16_of(E.ref_apply(f, relu, with_res)))
    if E.is_pow2(f["H"] * f["W"]):
        pooled = torch.relu(f["x"] * sc + sh).sum((1, 2)) * (torch.ones(()) / float(f["H"] * f["W"]))
        assert torch.equal(pooled.double(), E.ref_pool(f))


def test_one_pixel_statistics_follow_the_kernels_contract():
    """n = 1: var = 0, rstd = 1/sqrt(eps), the running variance moves toward the BIASED value (0)."""
    f = E.make(*E.ONE_PIXEL, 64)
    st = E.ref_stats(f)
    assert st["var"].abs().max().item() == 0
    assert torch.equal(st["running_var"], (1 - E.MOMENTUM) * f["running_var"].double())
    s, q, mean, rstd, rm, rv = _restate_stats(f, _sum_shuffled, torch.Generator().manual_seed(1))
    E.check_stats(mean, rstd, st, "n = 1", 1, rm, rv)


def test_a_dropped_pixel_or_swapped_sums_fail_the_checks():
    """The faults the method is for, injected into the restatement: one pixel left out of a sum, one counted twice, k0 and
    k1 swapped.  Each must fail the comparison the GPU tests make."""
    f = E.make(3, 56, 56, 16)
    n, C = f["n"], f["C"]
    r = E.ref_bwd(f)
    gen = torch.Generator().manual_seed(0)

    def dropped(t, g):
        t = t.clone()
        t[1234] = 0
        return _sum_shuffled(t, g)

    def doubled(t, g):
        return _sum_shuffled(torch.cat((t, t[1234:1235])), g)

    for faulty in (dropped, doubled):
        s0, s1, _, _ = _restate_bwd(f, faulty, gen)
        assert not torch.equal(s0.double(), r["s0"]) and not torch.equal(s1.double(), r["s1"])
    s0, s1, gx, _ = _restate_bwd(f, _sum_shuffled, gen)
    sc = f["gamma"] * f["rstd"]
    xh = (f["x"] - f["mean"]) * f["rstd"]
    g = r["g_resid"].float()
    v = sc * (g - s1 / n - xh * (s0 / n))           # k0 <-> k1
    with pytest.raises(AssertionError):
        E.check_elementwise(v.bfloat16(), r, "swapped")
    E.check_elementwise(gx, r, "control")
