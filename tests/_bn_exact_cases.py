"""Exactly representable BatchNorm fixtures and their float64 references (tests/test_bn_exact_cases.py on the host,
tests/test_bn_exact_gpu.py on the GPU).

The streaming kernels of csrc/bn.hip are HBM-bound passes whose faults are small: a pixel dropped at a grid-stride tail, a
channel chunk folded into the wrong row, k0 and k1 swapped.  Random fp32 data hides them behind summation-order and
ReLU-mask slack.  These fixtures remove the slack instead of bounding it:

  x                     integers in [-3, 3]      (statistics tests: [0, 4] in even channels, [-3, 3] in odd ones)
  gy, gx_add, residual  integers in [-4, 4]
  gpooled               H*W x an integer in [-4, 4], only when H*W is a power of two (gpooled / (H*W) is then exact)
  mean, beta            integers in {-1, 0, 1}
  rstd, |gamma|         in {0.5, 1, 2}, gamma of both signs

All of them are bf16 values, sc = gamma*rstd and sh = beta - mean*sc are dyadic, y = x*sc + sh (+ residual) is a multiple
of 1/4 below 32 (a bf16), xhat = (x - mean)*rstd is rstd x an integer of at most 4.  So

  * the ReLU mask (pre-activation > 0) is unambiguous: no value sits within a rounding of zero;
  * every per-channel sum (x, x^2, g', g'*xhat) is a power of two times an integer, and as long as the sum of the
    MAGNITUDES of its terms, in that unit, stays below 2^24 every partial sum in every order is an fp32 value: atomics,
    ordered folds and a float64 reference give the same bits (assert_sums_exact);
  * with a power-of-two pixel count, 1/n is exact too and so is the whole input gradient in fp32 (ref_bwd asserts it
    for each fixture): the bf16 result is THE rounding of the float64 reference;
  * otherwise 1/n, k = dsum*(1/n), xhat*k1, the two subtractions, the scale and the add round: every element stays
    within 2^-8*|ref| (half a bf16 ulp) + 2^-21*M, M = |sc|*(|g'| + |k0| + |xhat*k1|) + |add| the magnitude of the
    terms (eight fp32 roundings of the largest one).

A dropped or doubled pixel changes an integer sum by at least one unit, and the comparison fails."""
import torch

X_MAX, G_MAX = 3, 4
EXACT = 2 ** 24                     # integers below it are fp32 values
EPS, MOMENTUM = 1e-5, 0.125         # (a dyadic momentum: the running-statistics update adds two roundings, not five)

WIDTHS = (8, 16, 24, 64, 128, 160, 256, 320, 512, 640, 1024, 2048)
WIDTH_GRID = (2, 8, 16)                                                   # n = 256
PIXEL_WIDTHS = (64, 160)                                                  # C/8 = 8 divides 256, C/8 = 20 does not
POW2_GRIDS = ((1, 4, 4), (4, 16, 16), (8, 32, 32), (16, 64, 64))
RESNET_GRIDS = ((2, 7, 7), (6, 14, 14), (5, 28, 28), (3, 56, 56), (2, 112, 112))
ONE_PIXEL = (1, 1, 1)                                                     # statistics and apply only
CAP_CASES = ((9, 64, 64, 2048), (7, 256, 256, 160))                       # more pixels than 2048 blocks x py x 16
FOLD_ROWS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4097)
FOLD_WIDTHS = (24, 320)

SHAPES = [WIDTH_GRID + (c,) for c in WIDTHS] + [g + (c,) for c in PIXEL_WIDTHS for g in POW2_GRIDS + RESNET_GRIDS]


def shape_id(s):
    return "b%d_%dx%d_c%d" % tuple(s)


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def seed_of(B, H, W, C):
    return ((B * 131 + H) * 131 + W) * 4099 + C


# ------------------------------------------------------------------------------------------------------------------------
# fixtures

def make(B, H, W, C, seed=None, device="cpu"):
    """The fixture of one shape: float32 tensors holding the values of the module docstring ([B, H, W, C] unpadded,
    [C] per channel).  Two pixels of every channel are planted (x = +3 and -3, residual 0 there) so that the ReLU mask
    of every channel has both values whatever the parameters drew; beta is 0 where |sc| <= 1/2 (there |sh| = |beta - mean*sc|
    could reach 3*|sc| and leave the mask constant; elsewhere |sh| <= 1 + |sc| < 3*|sc|)."""
    seed = seed_of(B, H, W, C) if seed is None else seed
    gen = torch.Generator(device=device).manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=gen, device=device, dtype=torch.float32)

    def dyadic(*shape):
        return torch.exp2(ints(-1, 1, *shape))

    n = B * H * W
    f = dict(B=B, H=H, W=W, C=C, n=n, seed=seed)
    f["x"] = ints(-X_MAX, X_MAX, B, H, W, C)
    f["gy"] = ints(-G_MAX, G_MAX, B, H, W, C)
    f["gx_add"] = ints(-G_MAX, G_MAX, B, H, W, C)
    f["residual"] = ints(-G_MAX, G_MAX, B, H, W, C)
    f["gpooled"] = ints(-G_MAX, G_MAX, B, C) * float(H * W) if is_pow2(H * W) else None
    f["mean"] = ints(-1, 1, C)
    f["rstd"] = dyadic(C)
    f["gamma"] = dyadic(C) * (ints(0, 1, C) * 2 - 1)
    f["gamma"][0].abs_()                            # both signs, whatever the draw
    f["gamma"][1] = -f["gamma"][1].abs()
    f["beta"] = ints(-1, 1, C)
    f["beta"][(f["gamma"] * f["rstd"]).abs() <= 0.5] = 0.0
    # statistics input: mean near 2 in even channels (E[x^2] = 3 var: the cancellation in E[x^2] - mean^2), near 0 in odd
    xs = ints(-X_MAX, X_MAX, B, H, W, C)
    xs[..., 0::2] = ints(0, 4, B, H, W, (C + 1) // 2)
    f["x_stats"] = xs
    f["running_mean"] = ints(1, 3, C)               # (no cancellation against momentum * mean, |mean| <= 4)
    f["running_var"] = dyadic(C)
    f["dgamma0"] = ints(1, 8, C) * (ints(0, 1, C) * 2 - 1)        # non-zero integer start values of the accumulated sums
    f["dbeta0"] = ints(1, 8, C) * (ints(0, 1, C) * 2 - 1)
    if n >= 2:
        flat_x, flat_r = f["x"].view(n, C), f["residual"].view(n, C)
        flat_x[0], flat_x[n - 1] = X_MAX, -X_MAX
        flat_r[0], flat_r[n - 1] = 0, 0
    return f


def affine(f):
    """float64 sc = gamma*rstd and sh = beta - mean*sc (both exact)."""
    sc = f["gamma"].double() * f["rstd"].double()
    return sc, f["beta"].double() - f["mean"].double() * sc


def assert_values(f):
    """The value ranges of the module docstring, and that every tensor is a bf16 tensor."""
    def within(t, lo, hi):
        return torch.equal(t, t.round()) and t.min().item() >= lo and t.max().item() <= hi
    assert within(f["x"], -X_MAX, X_MAX) and within(f["x_stats"], -X_MAX, 4)
    for k in ("gy", "gx_add", "residual"):
        assert within(f[k], -G_MAX, G_MAX), k
    assert within(f["mean"], -1, 1) and within(f["beta"], -1, 1)
    for k in ("rstd", "gamma"):
        assert set(f[k].abs().unique().tolist()) <= {0.5, 1.0, 2.0}, k
    assert f["gamma"].min().item() < 0 < f["gamma"].max().item()
    if f["gpooled"] is not None:
        assert within(f["gpooled"] / (f["H"] * f["W"]), -G_MAX, G_MAX)
    for k, t in f.items():
        if torch.is_tensor(t):
            assert torch.equal(t.bfloat16().float(), t), k


def assert_sums_exact(f):
    """The fp32-exactness condition: for every per-channel sum a launch forms, the sum of |term| in the sum's unit (1, or
    rstd for g'*xhat) is below 2^24 -- with the non-zero start value of dgamma / dbeta included.  Taken over the UNMASKED
    gradient, which bounds every mask."""
    dims = (0, 1, 2)
    n, hw = f["n"], f["H"] * f["W"]
    worst = {}
    for key in ("x", "x_stats"):
        x = f[key].double()
        worst["sum " + key] = x.abs().sum(dims)
        worst["sum %s^2" % key] = (x * x).sum(dims)
    dev = (f["x"].double() - f["mean"].double()).abs()           # |xhat| / rstd
    grads = [f["gy"].double().abs()]
    if f["gpooled"] is not None:
        grads.append((f["gpooled"].double() / hw).abs()[:, None, None, :].expand(f["B"], f["H"], f["W"], f["C"]))
    for i, g in enumerate(grads):
        worst["sum g' (%d)" % i] = g.sum(dims) + f["dbeta0"].double().abs()
        worst["sum g'*xhat (%d)" % i] = (g * dev).sum(dims) + f["dgamma0"].double().abs() / f["rstd"].double()
    for what, w in worst.items():
        assert w.max().item() < EXACT, (what, w.max().item())
    assert (X_MAX + 1) ** 2 * n < EXACT and G_MAX * (X_MAX + 1) * n + 16 < EXACT      # (the ranges alone guarantee it)


def _f32_exact(t):
    return torch.equal(t.float().double(), t)


# ------------------------------------------------------------------------------------------------------------------------
# float64 references, from the definitions

def ref_stats(f, x_key="x_stats", running=True, eps=EPS, momentum=MOMENTUM):
    """Train-mode F.batch_norm statistics of f[x_key]: integer sums, mean, biased variance, rstd, and the running
    statistics after one update (unbiased variance; n = 1, where torch refuses, follows bn_finalize_kernel's contract:
    var = 0 and the running variance takes the biased value).  eps and momentum are the fp32 values the launch
    receives.  `rel_tol`: the bound on the relative error of rstd and running_var, 4 * 2^-24 * E[x^2] / (var + eps) --
    the roundings of sq/n, mean*mean (with mean's own) and the subtraction are at most 2^-24 * (E[x^2] + 3 mean^2 + var)
    <= 4 * 2^-24 * E[x^2] of absolute error in var."""
    x = f[x_key].double()
    return stats_from_sums(x.sum((0, 1, 2)), (x * x).sum((0, 1, 2)), f["n"], f["running_mean"] if running else None,
                           f["running_var"] if running else None, eps, momentum)


def stats_from_sums(s, q, n, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM):
    """ref_stats from the integer sums s = sum x and q = sum x^2 (float64) of n values per channel.  The biased variance
    is (q*n - s^2) / n^2: the numerator is an integer below 2^53, exact in float64."""
    eps, momentum = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))
    assert (q * n).max().item() < 2.0 ** 52
    mean = s / n
    var = (q * n - s * s) / (float(n) * n)
    r = dict(sum=s, sumsq=q, mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps))
    r["rel_tol"] = 4 * 2.0 ** -24 * (q / n) / (var + eps)
    if running_mean is not None:
        unbiased = var * n / (n - 1) if n > 1 else var
        r["running_mean"] = (1 - momentum) * running_mean.double() + momentum * mean
        r["running_var"] = (1 - momentum) * running_var.double() + momentum * unbiased
    return r


def ref_apply(f, relu, with_res):
    """y = [relu](x*sc + sh [+ residual]): exact, and a bf16 tensor."""
    sc, sh = affine(f)
    y = f["x"].double() * sc + sh
    if with_res:
        y = y + f["residual"].double()
    y = torch.relu(y) if relu else y
    assert torch.equal(y.bfloat16().double(), y)
    return y


def s2d(y):
    """[B, H, W, C] -> the space-to-depth interior [B, H/2, W/2, 4C]: pixel (h, w) -> channels ((h&1)*2 + (w&1))*C + c."""
    B, H, W, C = y.shape
    return y.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)


def ref_pool(f):
    """pooled[b][c] = mean over the image of relu(x*sc + sh)."""
    return ref_apply(f, True, False).sum((1, 2)) / (f["H"] * f["W"])


def ref_bwd(f, relu=True, mask_res=False, with_add=False, pooled=False):
    """The textbook backward gx = gamma*rstd*(g' - sum g'/n - xhat * sum g'*xhat/n) [+ gx_add], g' = gy masked by
    (forward pre-activation > 0) when relu -- the pre-activation including the residual when mask_res (the y-mask of a
    residual unit); pooled: gy = gpooled[b][c] / (H*W).  Returns the sums s0 = sum g', s1 = sum g'*xhat, gx, g_resid = g',
    and M, the magnitude of gx's terms.  With a power-of-two n it asserts that every intermediate of the fp32
    evaluation is an fp32 value, i.e. that bit-equality may be asked for."""
    n, dims = f["n"], (0, 1, 2)
    sc, sh = affine(f)
    x = f["x"].double()
    if pooled:
        g = (f["gpooled"].double() / (f["H"] * f["W"]))[:, None, None, :].expand(x.shape)
    else:
        g = f["gy"].double()
    if relu:
        pre = x * sc + sh
        if mask_res:
            pre = pre + f["residual"].double()
        g = torch.where(pre > 0, g, torch.zeros_like(g))
        if n >= 2:      # coverage guard: the mask takes both values in every channel
            on = (pre > 0).double().mean(dims)
            assert on.min().item() > 0 and on.max().item() < 1
    xh = (x - f["mean"].double()) * f["rstd"].double()
    s0, s1 = g.sum(dims), (g * xh).sum(dims)
    for s in (s0, s1):      # coverage guard: not a comparison of zeros
        assert (s == 0).double().mean().item() <= 0.25
    k0, k1 = s0 / n, s1 / n
    inner = g - k0 - xh * k1
    gx = sc * inner
    add = f["gx_add"].double() if with_add else torch.zeros_like(gx)
    M = sc.abs() * (g.abs() + k0.abs() + (xh * k1).abs()) + add.abs()
    if is_pow2(n):
        for t in (k0, k1, xh * k1, g - k0, inner, gx, gx + add):
            assert _f32_exact(t)
    return dict(n=n, s0=s0, s1=s1, gx=gx + add, g_resid=g, M=M)


def tile_partials(f, r):
    """[rows][2][C] fp32: the sums of g' and g'*xhat of reference r = ref_bwd(...) over 256-pixel tiles, the rows a data
    gradient's epilogue leaves for nbdt_bn_bwd_fold."""
    n, C = f["n"], f["C"]
    rows = (n + 255) // 256
    g = r["g_resid"].reshape(n, C)
    xh = ((f["x"].double() - f["mean"].double()) * f["rstd"].double()).reshape(n, C)
    pad = rows * 256 - n
    both = torch.stack((g, g * xh), 1)                                      # [n][2][C]
    both = torch.cat((both, both.new_zeros(pad, 2, C))) if pad else both
    return both.view(rows, 256, 2, C).sum(1).float().contiguous()


def fold_rows(rows, C, seed, device="cpu"):
    """Hand-made integer partial rows [rows][2][C] (float32) for the fold kernels: row r holds what 256 pixels of values in
    [-3, 3] could give, a sum in [-256, 256] and a sum of squares in [1024, 2304] (so var > 0); 4097 * 2304 < 2^24."""
    gen = torch.Generator(device=device).manual_seed(seed)
    s = torch.randint(-256, 257, (rows, 1, C), generator=gen, device=device, dtype=torch.float32)
    q = torch.randint(1024, 2305, (rows, 1, C), generator=gen, device=device, dtype=torch.float32)
    assert rows * 2304 < EXACT
    return torch.cat((s, q), 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# comparisons

def ulp32(ref):
    """Spacing of the fp32 numbers at |ref| (float64 tensor)."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.exp2(e.double() - 24)


def bf16_of(ref):
    """The float64 reference rounded to bf16 (through fp32: callers ask for it only where the reference is an fp32 value)."""
    assert _f32_exact(ref)
    return ref.float().bfloat16()


def half_ulp_bound(ref, M):
    return 2.0 ** -8 * ref.abs() + 2.0 ** -21 * M


def check_elementwise(got, r, what):
    """got (any float dtype, unpadded) against reference r = ref_bwd(...): bit-equal to the bf16 rounding of the reference
    when n is a power of two, otherwise every element inside half_ulp_bound."""
    ref, n = r["gx"], r["n"]
    if is_pow2(n):
        assert torch.equal(got.bfloat16(), bf16_of(ref)), what
    else:
        err, bound = (got.double() - ref).abs(), half_ulp_bound(ref, r["M"])
        worst = (err / bound.clamp_min(2.0 ** -200)).max().item()
        assert bool((err <= bound).all()), "%s: %d elements outside the bound, worst %.3f of it" % (
            what, int((err > bound).sum()), worst)


def check_stats(got_mean, got_rstd, r, what, n, got_rm=None, got_rv=None):
    """mean: round(mean * n) is the integer sum; rstd and running_var within r['rel_tol']; running_mean within 3 ulp."""
    assert torch.equal(torch.round(got_mean.double() * n), r["sum"]), what + ": mean"
    tol = r["rel_tol"] if n > 1 else torch.full_like(r["rel_tol"], 2.0 ** -22)    # (n = 1: var is exactly 0; eps + rsqrt)
    assert bool(((got_rstd.double() - r["rstd"]).abs() <= tol * r["rstd"]).all()), what + ": rstd"
    if got_rm is not None:
        assert bool(((got_rm.double() - r["running_mean"]).abs() <= 3 * ulp32(r["running_mean"])).all()), what + ": running_mean"
        assert bool(((got_rv.double() - r["running_var"]).abs() <= tol * r["running_var"]).all()), what + ": running_var"


def to(f, device):
    """The fixture with its tensors on `device`."""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in f.items()}
