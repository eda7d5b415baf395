"""Bit-exact parity of the BatchNorm launches of csrc/bn.hip on exactly representable fixtures (tests/_bn_exact_cases.py;
its conditions are checked on the host by tests/test_bn_exact_cases.py).

What is asserted follows from the fixtures, not from a measurement:
  * per-channel sums (dsum, and dgamma / dbeta accumulated onto non-zero integers): the float64 reference, bit for bit;
  * mean: round(mean * n) is the integer sum of x; rstd and running_var within 4 * 2^-24 * E[x^2] / (var + eps), relative
    (the reference's own bound per channel); running_mean within 3 ulp;
  * y, the space-to-depth y, g_resid: the float64 reference, bit for bit, at every n;
  * gx: the bf16 rounding of the float64 reference, bit for bit, when n is a power of two; otherwise EVERY element within
    2^-8 * |ref| + 2^-21 * M (half a bf16 ulp + eight fp32 roundings of the terms' magnitude M);
  * pooled (fp32): the reference's bits when H*W is a power of two, else within 2^-22 relative (1/(H*W) and the product
    round once each);
  * borders of padded outputs stay zero, the slot scratch is left zeroed (the pair form: the OTHER buffer);
  * default and deterministic mode give the same bits: exact sums do not depend on their order."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_exact_cases as E  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt._C import check, lib, ptr  # noqa: E402

DEV = "cuda:0"
PLAIN = 2 ** 62          # a nontemporal threshold no tensor reaches
IDS = [E.shape_id(s) for s in E.SHAPES]
ONE_PIXEL = [E.ONE_PIXEL + (c,) for c in E.PIXEL_WIDTHS]
POOL_SHAPES = [s for s in E.SHAPES if E.is_pow2(s[1] * s[2])]
FP32_SHAPES = [(4, 16, 16, 64), (2, 7, 7, 160), (2, 8, 16, 2048)]


def _pad(t, dtype=torch.bfloat16):
    B, H, W, C = t.shape
    p = ops.padded(B, H, W, C, DEV, dtype)
    ops.interior(p).copy_(t)
    return p


def _border_zero(p):
    return not (p[:, 0].any() or p[:, -1].any() or p[:, :, 0].any() or p[:, :, -1].any())


_CACHE = {}


def _fixture(shape, device="cpu"):
    """The fixture of `shape` on the GPU with padded bf16 copies of its activations, built once per shape (the host
    builds it, from the seed the host test checked; device=DEV for the two cases too large for that)."""
    if shape not in _CACHE:
        _CACHE.clear()
        f = E.to(E.make(*shape, device=device), DEV)
        f["pad"] = {k: _pad(f[k]) for k in ("x", "gy", "gx_add", "residual", "x_stats")}
        f["refs"] = {}
        _CACHE[shape] = f
    return _CACHE[shape]


def _ref_bwd(f, **form):
    key = tuple(sorted(form.items()))
    if key not in f["refs"]:
        f["refs"][key] = E.ref_bwd(f, **form)
    return f["refs"][key]


def _both_modes(run):
    """run() in default and in deterministic mode (restored whatever happens): the same bits from both."""
    old, outs = ops.is_deterministic(), []
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            outs.append(run())
    finally:
        ops.set_deterministic(old)
    assert len(outs[0]) == len(outs[1])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), "output %d differs between default and deterministic mode" % i
    return outs[0]


def _scratch(C):
    return torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV)


def _sum_outputs(f):
    return torch.full((2 * f["C"],), float("nan"), device=DEV), f["dgamma0"].clone(), f["dbeta0"].clone()


def _check_sums(f, r, dsum, dgamma, dbeta, what):
    C = f["C"]
    assert torch.equal(dsum[:C].double(), r["s0"]), what + ": sum g'"
    assert torch.equal(dsum[C:].double(), r["s1"]), what + ": sum g'*xhat"
    assert torch.equal(dbeta.double(), f["dbeta0"].double() + r["s0"]), what + ": dbeta"
    assert torch.equal(dgamma.double(), f["dgamma0"].double() + r["s1"]), what + ": dgamma"


def _check_gx(gx, r, what):
    assert _border_zero(gx), what + ": border"
    E.check_elementwise(ops.interior(gx), r, what)


# ------------------------------------------------------------------------------------------------------------------------
# forward

def _run_stats(f, x_key="x_stats"):
    C, n = f["C"], f["n"]
    scratch = _scratch(C)
    outs = []
    for running in (True, False):
        st = E.ref_stats(f, x_key, running)

        def run():
            mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            rm, rv = (f["running_mean"].clone(), f["running_var"].clone()) if running else (None, None)
            ops.bn_stats(f["pad"][x_key], scratch, mean, rstd, rm, rv, momentum=E.MOMENTUM)
            assert not scratch.any(), "slots not left zeroed"
            E.check_stats(mean, rstd, st, "bn_stats running=%s" % running, n, rm, rv)
            return (mean, rstd, rm, rv) if running else (mean, rstd)
        outs.append(_both_modes(run))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _run_apply(f, forms=((True, False), (True, True), (False, False), (False, True))):
    p = f["pad"]
    for relu, with_res in forms:
        ref = E.bf16_of(E.ref_apply(f, relu, with_res))

        def run():
            y = ops.padded(f["B"], f["H"], f["W"], f["C"], DEV)
            ops.bn_apply(p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], y, relu=relu,
                         residual=p["residual"] if with_res else None)
            assert _border_zero(y)
            assert torch.equal(ops.interior(y), ref), "bn_apply relu=%s residual=%s" % (relu, with_res)
            return (y,)
        _both_modes(run)


@pytest.mark.parametrize("shape", E.SHAPES + ONE_PIXEL, ids=IDS + [E.shape_id(s) for s in ONE_PIXEL])
def test_stats_with_and_without_running_statistics(shape):
    """bn_stats_kernel + bn_finalize_kernel on x of mean ~2 (even channels) and ~0 (odd); n = 1: var = 0, the running
    variance takes the biased value."""
    _run_stats(_fixture(shape))


@pytest.mark.parametrize("shape", E.SHAPES + ONE_PIXEL, ids=IDS + [E.shape_id(s) for s in ONE_PIXEL])
def test_apply_every_form(shape):
    """bn_apply_kernel: relu x residual; bn_apply_s2d_kernel (even H and W): with and without relu."""
    f = _fixture(shape)
    _run_apply(f)
    B, H, W, C = shape
    if H % 2 or W % 2:
        return
    for relu in (True, False):
        ref = E.s2d(E.bf16_of(E.ref_apply(f, relu, False)))

        def run():
            y = ops.s2d_buffer(B, H, W, C, DEV)
            ops.bn_apply_s2d(f["pad"]["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], y, relu=relu)
            assert _border_zero(y)
            assert torch.equal(ops.interior(y), ref), "bn_apply_s2d relu=%s" % relu
            return (y,)
        _both_modes(run)


# ------------------------------------------------------------------------------------------------------------------------
# backward

def _run_bwd(f, mask, with_add, with_gres):
    """ops.bn_bwd.  mask: 'y' (the stored output of the residual forward), 'x' (y=None: recomputed) or None (no relu)."""
    B, H, W, C = f["B"], f["H"], f["W"], f["C"]
    p = f["pad"]
    r = _ref_bwd(f, relu=mask is not None, mask_res=mask == "y", with_add=with_add)
    y = _pad(E.bf16_of(E.ref_apply(f, True, True))) if mask == "y" else None
    g_ref = E.bf16_of(r["g_resid"])
    scratch = _scratch(C)
    what = "bn_bwd mask=%s add=%s g_resid=%s" % (mask, with_add, with_gres)

    def run():
        dsum, dgamma, dbeta = _sum_outputs(f)
        gx = ops.padded(B, H, W, C, DEV)
        gres = ops.padded(B, H, W, C, DEV) if with_gres else None
        ops.bn_bwd(p["gy"], y, p["x"], f["mean"], f["rstd"], f["gamma"], scratch, dsum, dgamma, dbeta, gx,
                   relu=mask is not None, gx_add=p["gx_add"] if with_add else None, g_resid=gres, beta=f["beta"])
        assert not scratch.any(), what + ": slots not left zeroed"
        _check_sums(f, r, dsum, dgamma, dbeta, what)
        _check_gx(gx, r, what)
        if with_gres:
            assert _border_zero(gres) and torch.equal(ops.interior(gres), g_ref), what + ": g_resid"
        return (dsum, dgamma, dbeta, gx) + ((gres,) if with_gres else ())
    _both_modes(run)


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_backward_every_form(shape):
    """bn_bwd_reduce_kernel + bn_bwd_finalize_kernel + bn_bwd_apply_kernel: y-mask / x-mask / no relu, each with and
    without gx_add and g_resid."""
    f = _fixture(shape)
    for mask in ("y", "x", None):
        for with_add in (False, True):
            for with_gres in (False, True):
                _run_bwd(f, mask, with_add, with_gres)


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_backward_from_tile_partials(shape):
    """ops.bn_bwd_fused: bn_bwd_fold_partials_kernel over the 256-pixel tile rows a data gradient leaves, then
    bn_bwd_apply_kernel (cus = 0) or bn_bwd_apply_cus_kernel (cus = 7)."""
    f = _fixture(shape)
    B, H, W, C = shape
    p = f["pad"]
    for with_add in (False, True):
        r = _ref_bwd(f, relu=True, mask_res=False, with_add=with_add)
        part = E.tile_partials(f, r)
        keep = part.clone()
        for cus in (0, 7):
            what = "bn_bwd_fused add=%s cus=%d" % (with_add, cus)

            def run():
                dsum, dgamma, dbeta = _sum_outputs(f)
                gx = ops.padded(B, H, W, C, DEV)
                ops.bn_bwd_fused(p["gy"], p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], part, dsum, dgamma, dbeta,
                                 gx, gx_add=p["gx_add"] if with_add else None, cus=cus)
                _check_sums(f, r, dsum, dgamma, dbeta, what)
                _check_gx(gx, r, what)
                return dsum, dgamma, dbeta, gx
            _both_modes(run)
        assert torch.equal(part, keep)


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_backward_on_a_cu_subset(shape):
    """ops.bn_bwd_cus on 1, 7 and 64 CUs: a single scratch (bn_bwd_reduce_cus_kernel, bn_bwd_finalize_kernel,
    bn_bwd_apply_cus_kernel) and a slot pair (the fold in the elementwise pass's prologue; the other buffer, dirty
    from the call before, is the one left zeroed)."""
    f = _fixture(shape)
    B, H, W, C = shape
    p = f["pad"]
    scratch, pair = _scratch(C), (_scratch(C), _scratch(C))
    for with_add in (False, True):
        r = _ref_bwd(f, relu=True, mask_res=False, with_add=with_add)
        for paired in (False, True):
            for cus in (1, 7, 64):
                what = "bn_bwd_cus %s add=%s cus=%d" % ("pair" if paired else "single", with_add, cus)

                def run():
                    dsum, dgamma, dbeta = _sum_outputs(f)
                    gx = ops.padded(B, H, W, C, DEV)
                    if paired:
                        pair[0].zero_()
                        pair[1].fill_(3.0)          # (what the call before left there)
                    ops.bn_bwd_cus(p["gy"], p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], pair if paired else scratch,
                                   dsum, dgamma, dbeta, gx, cus, gx_add=p["gx_add"] if with_add else None)
                    if paired:
                        assert not pair[1].any(), what + ": the other slot buffer not left zeroed"
                        assert pair[0].any()
                    else:
                        assert not scratch.any(), what + ": slots not left zeroed"
                    _check_sums(f, r, dsum, dgamma, dbeta, what)
                    _check_gx(gx, r, what)
                    return dsum, dgamma, dbeta, gx
                _both_modes(run)


# ------------------------------------------------------------------------------------------------------------------------
# pooled head

def _check_pooled(f, pooled, what):
    ref = E.ref_pool(f)
    if E.is_pow2(f["H"] * f["W"]):
        assert torch.equal(pooled.double(), ref), what
    else:
        assert bool(((pooled.double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all()), what


@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_relu_pool(shape):
    """bn_relu_pool_kernel: the sum of relu(bn(x)) over an image is exact (multiples of 1/4 below 2^24 / 4)."""
    f = _fixture(shape)
    B, H, W, C = shape

    def run():
        pooled = torch.full((B, C), float("nan"), device=DEV)
        ops.bn_relu_pool(f["pad"]["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], pooled)
        _check_pooled(f, pooled, "bn_relu_pool")
        return (pooled,)
    _both_modes(run)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=[E.shape_id(s) for s in POOL_SHAPES])
def test_pooled_head_backward(shape):
    """pool_bn_bwd (bn_bwd_reduce_kernel<POOL> + bn_bwd_apply_kernel<POOL>) and pool_bn_bwd_apply alone with the caller's
    sums: the reference's, and zeros (a plain average pool: gx = sc * g')."""
    f = _fixture(shape)
    B, H, W, C = shape
    p = f["pad"]
    r = _ref_bwd(f, pooled=True)
    scratch = _scratch(C)
    args = (f["gpooled"], p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"])

    def run():
        dsum, dgamma, dbeta = _sum_outputs(f)
        gx = ops.padded(B, H, W, C, DEV)
        ops.pool_bn_bwd(*args, scratch, dsum, dgamma, dbeta, gx)
        assert not scratch.any()
        _check_sums(f, r, dsum, dgamma, dbeta, "pool_bn_bwd")
        _check_gx(gx, r, "pool_bn_bwd")
        gx2 = ops.padded(B, H, W, C, DEV)
        ops.pool_bn_bwd_apply(*args, torch.cat((r["s0"], r["s1"])).float(), gx2)
        _check_gx(gx2, r, "pool_bn_bwd_apply")
        gx3 = ops.padded(B, H, W, C, DEV)
        ops.pool_bn_bwd_apply(*args, torch.zeros(2 * C, device=DEV), gx3)
        sc, _ = E.affine(f)
        assert _border_zero(gx3) and torch.equal(ops.interior(gx3), E.bf16_of(sc * r["g_resid"]))
        return dsum, dgamma, dbeta, gx, gx2, gx3
    _both_modes(run)


# ------------------------------------------------------------------------------------------------------------------------
# the 2048-block cap of grid_for

def _cap_fixture(case):
    B, H, W, C = case
    py = max(1, 256 // (C // 8))
    assert B * H * W > 2048 * py * 16, "the block cap does not bind in the reductions"
    return _fixture(case, device=DEV)


@pytest.mark.parametrize("case", E.CAP_CASES, ids=[E.shape_id(s) for s in E.CAP_CASES])
def test_grid_cap_forward(case):
    """More pixels than 2048 blocks x py rows x 16 (reductions) or x 8 (elementwise): every block strides.  Statistics
    with running statistics, and relu(bn(x) + residual).  Fixture and references are built on the device."""
    f = _cap_fixture(case)
    C, n = f["C"], f["n"]
    st = E.ref_stats(f)
    scratch = _scratch(C)

    def run():
        mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rm, rv = f["running_mean"].clone(), f["running_var"].clone()
        ops.bn_stats(f["pad"]["x_stats"], scratch, mean, rstd, rm, rv, momentum=E.MOMENTUM)
        assert not scratch.any()
        E.check_stats(mean, rstd, st, "bn_stats", n, rm, rv)
        return mean, rstd, rm, rv
    _both_modes(run)
    _run_apply(f, forms=((True, True),))


@pytest.mark.parametrize("case", E.CAP_CASES, ids=[E.shape_id(s) for s in E.CAP_CASES])
def test_grid_cap_backward(case):
    """The same cases through bn_bwd with the mask recomputed from x and a gx_add."""
    _run_bwd(_cap_fixture(case), "x", True, False)
    _CACHE.clear()


# ------------------------------------------------------------------------------------------------------------------------
# fold tables

@pytest.mark.parametrize("C", E.FOLD_WIDTHS)
@pytest.mark.parametrize("rows", E.FOLD_ROWS)
def test_fold_tables(rows, C):
    """bn_fold_partials_kernel<32> / <8> (1024 rows and up) behind ops.bn_finalize and bn_bwd_fold_partials_kernel behind
    nbdt_bn_bwd_fold on integer partial rows, either side of every unrolled loop and of the kernel switch.  B x 16 x 16
    makes ceil(B*H*W / 256) = B rows; only the partials are read, the activation tensor gives the shape."""
    part = E.fold_rows(rows, C, 1000 * rows + C, DEV)
    keep = part.clone()
    n = rows * 256
    s, q = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    g = torch.Generator(device=DEV).manual_seed(rows + C)
    rm0 = torch.randint(1, 4, (C,), generator=g, device=DEV, dtype=torch.float32)
    rv0 = torch.exp2(torch.randint(-1, 2, (C,), generator=g, device=DEV, dtype=torch.float32))
    start = torch.randint(1, 9, (2, C), generator=g, device=DEV, dtype=torch.float32)
    shape_only = torch.zeros(1, device=DEV).expand(rows, 18, 18, C)
    for running in (True, False):
        st = E.stats_from_sums(s, q, n, rm0 if running else None, rv0 if running else None)

        def run():
            mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
            ops.bn_finalize(shape_only, part, mean, rstd, rm, rv, momentum=E.MOMENTUM)
            E.check_stats(mean, rstd, st, "bn_finalize rows=%d" % rows, n, rm, rv)
            return (mean, rstd, rm, rv) if running else (mean, rstd)
        _both_modes(run)

    def run_bwd():
        dsum = torch.full((2 * C,), float("nan"), device=DEV)
        dgamma, dbeta = start[0].clone(), start[1].clone()
        check(lib().nbdt_bn_bwd_fold(rows, 16, 16, C, ptr(part), ptr(dsum), ptr(dgamma), ptr(dbeta), ops.stream_ptr(DEV)))
        assert torch.equal(dsum[:C].double(), s) and torch.equal(dsum[C:].double(), q)
        assert torch.equal(dbeta.double(), start[1].double() + s) and torch.equal(dgamma.double(), start[0].double() + q)
        return dsum, dgamma, dbeta
    _both_modes(run_bwd)
    assert torch.equal(part, keep)


# ------------------------------------------------------------------------------------------------------------------------
# nontemporal loads, fp32 storage

def test_nontemporal_loads_give_the_same_bits():
    """One apply and one backward case with every tensor over the nontemporal threshold (0) and with none (2^62): each
    run is checked against the reference, and the two give the same bits."""
    f = _fixture((5, 28, 28, 160))
    B, H, W, C = f["B"], f["H"], f["W"], f["C"]
    p = f["pad"]
    r = _ref_bwd(f, relu=True, mask_res=False, with_add=True)
    y_ref = E.bf16_of(E.ref_apply(f, True, True))
    pair = (_scratch(C), _scratch(C))
    old, outs = ops.stream_nt_min_bytes(), []
    try:
        for thr, want in ((0, True), (PLAIN, False)):
            ops.set_stream_nt_min_bytes(thr)

            def run():
                y = ops.padded(B, H, W, C, DEV)
                ops.bn_apply(p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], y, relu=True, residual=p["residual"])
                assert ops.last_stream_nt() is want
                assert _border_zero(y) and torch.equal(ops.interior(y), y_ref)
                dsum, dgamma, dbeta = _sum_outputs(f)
                gx = ops.padded(B, H, W, C, DEV)
                pair[0].zero_()
                ops.bn_bwd_cus(p["gy"], p["x"], f["mean"], f["rstd"], f["gamma"], f["beta"], pair, dsum, dgamma, dbeta, gx,
                               7, gx_add=p["gx_add"])
                assert ops.last_stream_nt() is want
                _check_sums(f, r, dsum, dgamma, dbeta, "bn_bwd_cus nt=%s" % want)
                _check_gx(gx, r, "bn_bwd_cus nt=%s" % want)
                return y, dsum, dgamma, dbeta, gx
            outs.append(_both_modes(run))
    finally:
        ops.set_stream_nt_min_bytes(old)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", FP32_SHAPES, ids=[E.shape_id(s) for s in FP32_SHAPES])
def test_fp32_storage_gives_the_same_values(shape):
    """The nbdt_ref_bn_* entries (fp32 padded tensors select them) on the same fixture: its values are fp32 values too, so
    sums, y, g_resid and pooled are the reference's bits; gx is the reference's bits at a power-of-two n (its bf16
    rounding is then the bf16 path's output) and within 2^-21 * M otherwise (no bf16 rounding of the output)."""
    f = _fixture(shape)
    B, H, W, C = shape
    n = f["n"]
    p32 = {k: _pad(f[k], torch.float32) for k in ("x", "gy", "gx_add", "residual", "x_stats")}
    params = (f["mean"], f["rstd"], f["gamma"], f["beta"])

    def check_gx(gx, r, what):
        assert _border_zero(gx), what
        got = ops.interior(gx).double()
        if E.is_pow2(n):
            assert torch.equal(got, r["gx"]), what
        else:
            assert bool(((got - r["gx"]).abs() <= 2.0 ** -21 * r["M"]).all()), what

    st = E.ref_stats(f)
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = f["running_mean"].clone(), f["running_var"].clone()
    ops.bn_stats(p32["x_stats"], None, mean, rstd, rm, rv, momentum=E.MOMENTUM)
    E.check_stats(mean, rstd, st, "fp32 bn_stats", n, rm, rv)
    for relu, with_res in ((True, False), (True, True), (False, False), (False, True)):
        y = ops.padded(B, H, W, C, DEV, torch.float32)
        ops.bn_apply(p32["x"], *params, y, relu=relu, residual=p32["residual"] if with_res else None)
        assert _border_zero(y) and torch.equal(ops.interior(y).double(), E.ref_apply(f, relu, with_res))
    if H % 2 == 0 and W % 2 == 0:
        y = ops.s2d_buffer(B, H, W, C, DEV, torch.float32)
        ops.bn_apply_s2d(p32["x"], *params, y, relu=True)
        assert _border_zero(y) and torch.equal(ops.interior(y).double(), E.s2d(E.ref_apply(f, True, False)))
    pooled = torch.full((B, C), float("nan"), device=DEV)
    ops.bn_relu_pool(p32["x"], *params, pooled)
    _check_pooled(f, pooled, "fp32 bn_relu_pool")

    y32 = _pad(E.ref_apply(f, True, True).float(), torch.float32)
    for mask, yy in (("y", y32), ("x", None), (None, None)):
        r = _ref_bwd(f, relu=mask is not None, mask_res=mask == "y", with_add=True)
        dsum, dgamma, dbeta = _sum_outputs(f)
        gx, gres = ops.padded(B, H, W, C, DEV, torch.float32), ops.padded(B, H, W, C, DEV, torch.float32)
        ops.bn_bwd(p32["gy"], yy, p32["x"], f["mean"], f["rstd"], f["gamma"], None, dsum, dgamma, dbeta, gx,
                   relu=mask is not None, gx_add=p32["gx_add"], g_resid=gres, beta=f["beta"])
        _check_sums(f, r, dsum, dgamma, dbeta, "fp32 bn_bwd mask=%s" % mask)
        check_gx(gx, r, "fp32 bn_bwd mask=%s" % mask)
        assert _border_zero(gres) and torch.equal(ops.interior(gres).double(), r["g_resid"])
    r = _ref_bwd(f, relu=True, mask_res=False, with_add=False)
    dsum, dgamma, dbeta = _sum_outputs(f)
    gx = ops.padded(B, H, W, C, DEV, torch.float32)
    ops.bn_bwd_cus(p32["gy"], p32["x"], *params, None, dsum, dgamma, dbeta, gx, 7)
    _check_sums(f, r, dsum, dgamma, dbeta, "fp32 bn_bwd_cus")
    check_gx(gx, r, "fp32 bn_bwd_cus")
    if f["gpooled"] is not None:
        r = _ref_bwd(f, pooled=True)
        dsum, dgamma, dbeta = _sum_outputs(f)
        gx = ops.padded(B, H, W, C, DEV, torch.float32)
        ops.pool_bn_bwd(f["gpooled"], p32["x"], *params, None, dsum, dgamma, dbeta, gx)
        _check_sums(f, r, dsum, dgamma, dbeta, "fp32 pool_bn_bwd")
        check_gx(gx, r, "fp32 pool_bn_bwd")
        gx = ops.padded(B, H, W, C, DEV, torch.float32)
        ops.pool_bn_bwd_apply(f["gpooled"], p32["x"], *params, torch.cat((r["s0"], r["s1"])).float(), gx)
        check_gx(gx, r, "fp32 pool_bn_bwd_apply")
    # the bf16 path on the same fixture gives these values: every check above and _run_bwd share one reference
    _run_bwd(f, "y", True, True)
