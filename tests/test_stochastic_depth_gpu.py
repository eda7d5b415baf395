"""Stochastic depth on the MI355X: the row-scaled residual add and BatchNorm backward (nbdt_bn_act_apply_rows /
nbdt_bn_act_bwd_rows and their fp32 twins) against plain PyTorch on the same inputs, the draw kernel against its numpy
restatement bit for bit, the whole EfficientNet-B0 step in fp32 storage against the fp32 oracle given the SAME masks, the
engine's behaviour in the bf16 product path, and the driver's flag.

Tolerances are those of the tests these extend (tests/test_effnet_gpu.py test_bn_act_apply_pool_and_backward_forms,
tests/test_reference_fp32_gpu.py): the new term is one multiply by a per-image constant, no new reduction.  Everything
the issue calls exact is compared with torch.equal / on the bits."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nbdt_oracle as O
import nbdt_path
import torch_models as TM

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt.engine import GraphedStep, train_step  # noqa: E402
from nbdt.engine_effnet import EfficientNetEngine  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

DEV = "cuda:0"
SHAPES = [(5, 32, 8, 8), (3, 96, 5, 7), (4, 320, 2, 2), (2, 192, 14, 14)]
ROWS = [0.0, 1.25, 1.0, 0.0, 2.5]          # arbitrary factors: a wrong image index or a scale applied twice shows
RESIDUAL_KEYS = ["s2u2", "s3u2", "s4u2", "s4u3", "s4u5", "s4u6", "s5u2", "s5u3", "s5u4"]
TOL = 1e-3                                   # tests/test_reference_fp32_gpu.py: relative L2 per parameter gradient


def _padded_from(x_nchw, dtype=torch.bfloat16):
    B, C, H, W = x_nchw.shape
    t = ops.padded(B, H, W, C, DEV, dtype=dtype)
    ops.interior(t).copy_(x_nchw.permute(0, 2, 3, 1).to(DEV))
    return t


def _nchw(t):
    return ops.interior(t).float().permute(0, 3, 1, 2).cpu()


def _bf(x):
    return x.to(torch.bfloat16).float()


def _close_bf16(got, want, what, rel=2 ** -7, abs_=1e-3):
    err = (got - want).abs()
    tol = rel * want.abs() + abs_
    assert (err <= tol).all(), f"{what}: max err {err.max().item():.4g} at |ref| {want.abs().max().item():.4g}"


def _bits(t):
    t = ops.interior(t).contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _case(B, C, H, W):
    g = torch.Generator().manual_seed(1000 * B + C + H)
    d = dict(x=_bf(torch.randn(B, C, H, W, generator=g) * 2 + 0.3), gamma=torch.rand(C, generator=g) + 0.5,
             beta=torch.randn(C, generator=g) * 0.2, res=_bf(torch.randn(B, C, H, W, generator=g)),
             gu=_bf(torch.randn(B, C, H, W, generator=g)), add=_bf(torch.randn(B, C, H, W, generator=g)),
             rows=torch.tensor(ROWS[:B]))
    return d


def _device_side(d, dtype):
    """The padded device tensors of a case and the batch statistics the library computes for them."""
    C = d["x"].shape[1]
    xp = _padded_from(d["x"], dtype)
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    scratch = torch.zeros(ops.BN_SLOTS * 2 * 2048, device=DEV)
    ops.bn_stats(xp, scratch, mean, rstd)
    return xp, mean, rstd, d["gamma"].to(DEV), d["beta"].to(DEV), scratch


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_forward_scales_the_branch_per_image(B, C, H, W):
    d = _case(B, C, H, W)
    rows = d["rows"]
    want = F.batch_norm(d["x"], None, None, d["gamma"], d["beta"], True, 0.0, 1e-5) * rows[:, None, None, None] + d["res"]
    for dtype in (torch.bfloat16, torch.float32):
        xp, mean, rstd, gd, bd, _ = _device_side(d, dtype)
        resp = _padded_from(d["res"], dtype)
        yp = ops.padded(B, H, W, C, DEV, dtype=dtype)
        ops.bn_act_apply(xp, mean, rstd, gd, bd, yp, act=ops.ACT_NONE, residual=resp, row_scale=rows.to(DEV))
        if dtype == torch.bfloat16:
            _close_bf16(_nchw(yp), want, "apply rows+res", abs_=4e-3)
        else:       # the twin stores fp32: summation-order noise of the statistics only
            assert (_nchw(yp) - want).abs().max().item() < 1e-4 * want.abs().max().item()
        # a factor of exactly 0 passes the residual's bits through
        for b in range(B):
            if rows[b] == 0:
                assert torch.equal(_bits(yp)[b], _bits(resp)[b]), (dtype, b)
        assert sum(1 for r in ROWS[:B] if r == 0) >= 1
        # factors of 1 give the bits of the call without row_scale
        y1, y0 = ops.padded(B, H, W, C, DEV, dtype=dtype), ops.padded(B, H, W, C, DEV, dtype=dtype)
        ops.bn_act_apply(xp, mean, rstd, gd, bd, y1, act=ops.ACT_NONE, residual=resp, row_scale=torch.ones(B, device=DEV))
        ops.bn_act_apply(xp, mean, rstd, gd, bd, y0, act=ops.ACT_NONE, residual=resp)
        assert torch.equal(_bits(y1), _bits(y0)), dtype


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_backward_scales_the_branch_gradient_per_image(B, C, H, W):
    d = _case(B, C, H, W)
    rows = d["rows"]
    xp, mean, rstd, gd, bd, scratch = _device_side(d, torch.bfloat16)
    gup, addp, rows_d = _padded_from(d["gu"]), _padded_from(d["add"]), rows.to(DEV)

    def run(row_scale, gx_add):
        dsum, dgamma, dbeta = torch.empty(2 * C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        gx = ops.padded(B, H, W, C, DEV)
        ops.bn_act_bwd(gup, xp, mean, rstd, gd, bd, scratch, dsum, dgamma, dbeta, gx, act=ops.ACT_NONE, gx_add=gx_add,
                       row_scale=row_scale)
        assert scratch.abs().max().item() == 0, "scratch must be left zeroed"
        return dsum, dgamma, dbeta, gx

    for with_add in (False, True):
        xr = d["x"].clone().requires_grad_(True)
        gr, br = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
        out = F.batch_norm(xr, None, None, gr, br, True, 0.0, 1e-5) * rows[:, None, None, None] + d["res"]
        out.backward(d["gu"])
        _, dgamma, dbeta, gx = run(rows_d, addp if with_add else None)
        want_gx = xr.grad + (d["add"] if with_add else 0)
        scale = want_gx.abs().max().item()
        assert (_nchw(gx) - want_gx).abs().max().item() < 2e-2 * scale + 1e-3, with_add
        assert (dgamma.cpu() - gr.grad).abs().max().item() < 5e-3 * gr.grad.abs().max().item() + 1e-3, with_add
        assert (dbeta.cpu() - br.grad).abs().max().item() < 5e-3 * br.grad.abs().max().item() + 1e-3, with_add
        # every image dropped: exact zeros into the sums, and gx is gx_add (or zero)
        dsum, dgamma, dbeta, gx = run(torch.zeros(B, device=DEV), addp if with_add else None)
        assert (dsum == 0).all() and (dgamma == 0).all() and (dbeta == 0).all()
        assert torch.equal(ops.interior(gx), ops.interior(addp) if with_add else torch.zeros_like(ops.interior(gx)))
        # factors of 1: the bits of the call without row_scale.  (These shapes have at most 32 blocks, one per slot of the
        # scratch, so the sums do not depend on the order of the atomics; deterministic mode below fixes it by contract.)
        for a, b in zip(run(torch.ones(B, device=DEV), addp if with_add else None), run(None, addp if with_add else None)):
            assert torch.equal(a, b)
        ops.set_deterministic(True)
        try:
            ones = run(torch.ones(B, device=DEV), addp if with_add else None)
            none = run(None, addp if with_add else None)
            first = run(rows_d, addp if with_add else None)
            again = run(rows_d, addp if with_add else None)
        finally:
            ops.set_deterministic(False)
        for a, b in zip(ones, none):
            assert torch.equal(a, b)
        for a, b in zip(first, again):          # dsum, dgamma, dbeta, gx: identical bits call after call
            assert torch.equal(a, b)
        want_d = xr.grad + (d["add"] if with_add else 0)
        assert (_nchw(first[3]) - want_d).abs().max().item() < 2e-2 * scale + 1e-3       # and still right
        assert (first[1].cpu() - gr.grad).abs().max().item() < 5e-3 * gr.grad.abs().max().item() + 1e-3
    # the fp32 twin: same meaning
    xf, mean, rstd, gd, bd, _ = _device_side(d, torch.float32)
    guf = _padded_from(d["gu"], torch.float32)
    dsum, dgamma, dbeta = torch.empty(2 * C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gx = ops.padded(B, H, W, C, DEV, dtype=torch.float32)
    ops.bn_act_bwd(guf, xf, mean, rstd, gd, bd, None, dsum, dgamma, dbeta, gx, act=ops.ACT_NONE, row_scale=rows_d)
    xr = d["x"].clone().requires_grad_(True)
    gr = d["gamma"].clone().requires_grad_(True)
    (F.batch_norm(xr, None, None, gr, d["beta"], True, 0.0, 1e-5) * rows[:, None, None, None]).backward(d["gu"])
    assert (_nchw(gx) - xr.grad).abs().max().item() < 1e-3 * xr.grad.abs().max().item()
    assert (dgamma.cpu() - gr.grad).abs().max().item() < 1e-3 * gr.grad.abs().max().item()


def test_row_scale_is_refused_outside_the_residual_and_plain_forms():
    B, C, H, W = 3, 32, 4, 4
    d = _case(B, C, H, W)
    rows = torch.ones(B, device=DEV)
    gate, gpool = torch.rand(B, C, device=DEV), torch.randn(B, C, device=DEV)
    launches = []
    for dtype in (torch.bfloat16, torch.float32):
        xp, mean, rstd, gd, bd, scratch = _device_side(d, dtype)
        resp, gup = _padded_from(d["res"], dtype), _padded_from(d["gu"], dtype)
        yp = ops.padded(B, H, W, C, DEV, dtype=dtype)
        dsum, dgamma, dbeta = torch.full((2 * C,), 7.0, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        for kw in (dict(residual=resp, gate=gate), dict(residual=None), dict(residual=None, gate=gate)):
            with pytest.raises(_C.NBDTHipError, match="row_scale"):
                ops.bn_act_apply(xp, mean, rstd, gd, bd, yp, act=ops.ACT_NONE, row_scale=rows, **kw)
        for gu, kw in ((gup, dict(gate=gate, gpool=gpool)), (gup, dict(gpool=gpool)), (None, dict(gpool=gpool)),
                       (None, dict())):
            with pytest.raises(_C.NBDTHipError, match="error -1"):       # NBDT_EINVAL, raised by check
                ops.bn_act_bwd(gu, xp, mean, rstd, gd, bd, scratch, dsum, dgamma, dbeta, yp, act=ops.ACT_NONE,
                               row_scale=rows, **kw)
        torch.cuda.synchronize()
        launches.append((yp.abs().max().item(), (dsum == 7.0).all().item(), dgamma.abs().max().item()))
    assert launches == [(0.0, True, 0.0)] * 2, "a refused call must not launch"
    with pytest.raises(_C.NBDTHipError):        # a wrong-length table never reaches the library
        ops.bn_act_apply(xp, mean, rstd, gd, bd, yp, act=ops.ACT_NONE, residual=resp, row_scale=torch.ones(B + 1, device=DEV))


@pytest.mark.parametrize("P", [0.2, 0.5])
def test_draw_kernel_equals_its_numpy_restatement(P):
    flags = [i in (2, 4, 6, 7, 9, 10, 12, 13, 14) for i in range(16)]
    prob, scale = ops.stochastic_depth_probs(P, 16, flags)
    for B in (1, 7, 512):
        table = torch.full((16, B), -1.0, device=DEV)
        for counter in (0, 1, 2 ** 31):
            for stream in (0, 7):
                ops.stochastic_depth_draw(table, prob, scale, 11, stream, counter)
                want = torch.from_numpy(ops.draw_stochastic_depth(11, stream, counter, prob, scale, B))
                assert torch.equal(table.cpu(), want), (B, counter, stream)
    with pytest.raises(_C.NBDTHipError):
        ops.stochastic_depth_draw(table, np.full(16, 1.0, np.float32), scale, 0, 0, 0)


def _search_seed(prob, scale, B, ok, counters=(0,), stream=0):
    """The first engine seed whose tables (host restatement) satisfy `ok` for every counter."""
    for seed in range(1, 2000):
        tables = [ops.draw_stochastic_depth(seed, stream, c, prob, scale, B) for c in counters]
        if all(ok(t) for t in tables):
            return seed, tables
    raise AssertionError("no seed found")


@pytest.mark.parametrize("schedule", ["two-streams", "one-stream"])
def test_whole_step_in_fp32_storage_equals_the_fp32_oracle_with_the_same_masks(schedule, pkg_dir):
    """The engine's forward() / backward() with P = 0.5 in fp32 storage against oracle.torch_models.EfficientNetB0 whose
    residual units' last conv block (BatchNorm output, nothing rounded in between) is multiplied by the same [B, 1, 1, 1]
    factors through forward hooks.  Bounds: those of test_efficientnet_b0_whole_step_in_fp32_storage_equals_the_fp32_oracle."""
    classes, size, B = 10, 64, 8
    res_idx = [2, 4, 6, 7, 9, 10, 12, 13, 14]
    prob, scale = ops.stochastic_depth_probs(0.5, 16, [i in res_idx for i in range(16)])

    def ok(t):      # every residual unit keeps an image, at least 5 of the 9 drop one
        return all((t[i] != 0).any() for i in res_idx) and sum(bool((t[i] == 0).any()) for i in res_idx) >= 5

    seed, tables = _search_seed(prob, scale, B, ok, counters=(0, 1))
    assert all(ok(t) for t in tables)
    otree = O.OracleTree(*O.default_paths("CIFAR10", "induced-ResNet18", pkg_dir))
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    torch.manual_seed(5)
    init = {k: v.clone() for k, v in TM.EfficientNetB0(num_classes=classes, dropout_rate=0.0).state_dict().items()}
    eng = EfficientNetEngine(num_classes=classes, dropout_rate=0.0, device=DEV, seed=seed, stochastic_depth_prob=0.5)
    assert [u["key"] for u in eng.units if u["residual"]] == RESIDUAL_KEYS
    assert [u["index"] for u in eng.units if u["residual"]] == res_idx
    if schedule == "one-stream":
        eng.set_overlap(False)
    eng.set_reference_fp32(True)
    for step, in_seed in enumerate((31, 32)):
        assert eng.sd_counter == step and eng.sd_seed == seed and eng.sd_stream == 0
        table = torch.from_numpy(tables[step])
        ref = TM.EfficientNetB0(num_classes=classes, dropout_rate=0.0)
        ref.load_state_dict(init)
        eng.load_state_dict(init)
        for u in eng.units:
            if u["residual"]:
                block = getattr(getattr(ref.features, f"stage{u['stage']}"), "unit" + u["key"].split("u")[1]).conv3
                assert not block.round_out and not block.act
                block.register_forward_hook(lambda m, i, out, r=table[u["index"]]: out * r[:, None, None, None])
        g = torch.Generator().manual_seed(in_seed)
        x = torch.randn(B, 3, size, size, generator=g)
        y = torch.randint(0, classes, (B,), generator=g)
        ref.train()
        z_ref = ref(x)
        loss_ref, dz = O.soft_tree_sup_loss(otree, z_ref.detach().numpy(), y.numpy(), 1.0, 1.0)
        z_ref.backward(torch.from_numpy(dz))
        z_ref, loss_ref = z_ref.detach(), float(loss_ref)
        g_ref = {n: p.grad.clone() for n, p in ref.named_parameters()}
        eng.zero_grad()
        z = eng.forward(x.to(DEV), training=True)
        loss, gz = crit.loss_and_grad(z, y.to(DEV))
        eng.backward(gz)
        torch.cuda.synchronize()
        assert torch.equal(eng._sd_rows.cpu(), table), "the engine drew another table than the host restatement"
        grads = {k: v.clone() for k, v in eng.named_params("grad").items()}
        zscale = z_ref.abs().max().item()
        zerr = (z.float().cpu() - z_ref).abs().max().item()
        print(f"[{schedule} / inputs {in_seed}] logits err {zerr:.3e} of scale {zscale:.3e}; loss {loss.item():.6f} vs {loss_ref:.6f}")
        assert zerr < 1e-4 * zscale
        assert abs(loss.item() - loss_ref) < 1e-5 * abs(loss_ref), (loss.item(), loss_ref)
        assert set(grads) == set(g_ref)
        gmax = max(v.abs().max().item() for v in g_ref.values())
        errs = []
        for n in g_ref:     # (a BatchNorm shift that feeds conv -> BatchNorm has a mathematically zero gradient)
            if g_ref[n].norm().item() < 1e-6 * gmax:
                assert grads[n].float().cpu().norm().item() < 1e-4 * gmax, n
                continue
            a, b = grads[n].float().cpu().flatten(), g_ref[n].float().flatten()
            errs.append((((a - b).norm() / (b.norm() + 1e-30)).item(), n))
        errs.sort()
        print(f"[{schedule} / inputs {in_seed}] parameter-gradient rel-L2 over {len(errs)} tensors: worst {errs[-1][0]:.2e} "
              f"({errs[-1][1]}), median {errs[len(errs) // 2][0]:.2e}")
        assert errs[-1][0] < TOL, errs[-1]
        sd, sd_ref = eng.state_dict(), ref.state_dict()
        for k in sd_ref:
            if k.endswith("running_var") or k.endswith("running_mean"):
                a, b = sd[k].float().cpu(), sd_ref[k].float().cpu()
                assert (a - b).norm().item() < 1e-4 * b.norm().item() + 1e-6, k


# ------------------------------------------------------------------------------------------------ engine, bf16 product path

@pytest.fixture(scope="module")
def crit10():
    return SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(9)
    return torch.randn(8, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV)


def _engine(P, seed=3, **kw):
    return EfficientNetEngine(num_classes=10, dropout_rate=0.0, device=DEV, seed=seed, stochastic_depth_prob=P, **kw)


def _step(eng, crit, x, y):
    eng.zero_grad()
    z = eng.forward(x, training=True)
    loss, gz = crit.loss_and_grad(z, y)
    eng.backward(gz)
    torch.cuda.synchronize()
    return loss.item()


def test_evaluation_ignores_stochastic_depth(batch):
    x, _ = batch
    off, on = _engine(0.0), _engine(0.2)
    on.load_state_dict(off.state_dict())
    for fuse in (True, False):
        off.fuse_eval = on.fuse_eval = fuse
        assert torch.equal(on.forward(x, training=False), off.forward(x, training=False)), fuse
        assert on._sd_rows is None and on.sd_counter == 0
    on.set_stochastic_depth(0.0)
    assert on.stochastic_depth_prob == 0.0
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            on.set_stochastic_depth(bad)


def test_launch_sequence_gains_one_draw_and_nine_row_scales(batch, crit10, monkeypatch):
    x, y = batch
    seen = {}
    real = {n: getattr(ops, n) for n in ("bn_act_apply", "bn_act_bwd", "stochastic_depth_draw")}

    def spy(name):
        def f(*a, **k):
            seen[name] = seen.get(name, 0) + 1
            if k.get("row_scale") is not None:
                seen[name + ".rows"] = seen.get(name + ".rows", 0) + 1
                assert tuple(k["row_scale"].shape) == (x.shape[0],)
            else:
                assert "row_scale" not in k, "with P = 0 the call must be exactly today's"
            return real[name](*a, **k)
        return f

    for n in real:
        monkeypatch.setattr(ops, n, spy(n))
    counts = {}
    for P in (0.0, 0.2):
        eng = _engine(P)
        seen.clear()
        _step(eng, crit10, x, y)
        counts[P] = dict(seen)
        if P == 0.0:
            assert eng._sd_rows is None and not any(k[0] == "sd_rows" for k in eng._bufs)
    assert "stochastic_depth_draw" not in counts[0.0] and "bn_act_apply.rows" not in counts[0.0]
    assert "bn_act_bwd.rows" not in counts[0.0]
    assert counts[0.2]["stochastic_depth_draw"] == 1
    assert counts[0.2]["bn_act_apply.rows"] == 9 and counts[0.2]["bn_act_bwd.rows"] == 9
    # nothing else changed: the same number of applies and backwards, one launch more per step
    assert counts[0.2]["bn_act_apply"] == counts[0.0]["bn_act_apply"]
    assert counts[0.2]["bn_act_bwd"] == counts[0.0]["bn_act_bwd"]


def test_masks_follow_seed_stream_and_counter_and_steps_are_reproducible(batch, crit10):
    x, y = batch
    a, b, c = _engine(0.2, seed=5), _engine(0.2, seed=5), _engine(0.2, seed=5)
    c.set_stochastic_depth(0.2, stream=1)
    tables = []
    for step in range(3):
        for e in (a, b, c):
            e.forward(x, training=True)
        ta, tb, tc = a._sd_rows.clone(), b._sd_rows.clone(), c._sd_rows.clone()
        assert torch.equal(ta, tb) and not torch.equal(ta, tc), step
        want = ops.draw_stochastic_depth(5, 0, step, a._sd_prob, a._sd_scale, x.shape[0])
        assert torch.equal(ta.cpu(), torch.from_numpy(want))
        tables.append(ta)
    assert a.sd_counter == 3 and not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])
    ops.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            a.sd_counter = 7                    # the same draw for both passes
            _step(a, crit10, x, y)
            grads.append(a.store.grad.clone())
        assert torch.equal(grads[0], grads[1])
    finally:
        ops.set_deterministic(False)


def test_a_dropped_image_passes_its_unit_unchanged(batch, crit10):
    x, y = batch
    B = x.shape[0]
    flags = [i in (2, 4, 6, 7, 9, 10, 12, 13, 14) for i in range(16)]
    prob, scale = ops.stochastic_depth_probs(0.2, 16, flags)
    seed, (table,) = _search_seed(prob, scale, B, lambda t: (t[2] == 0).any() and (t[2] != 0).any())
    eng = _engine(0.2, seed=seed)
    eng.debug_keep = True
    _step(eng, crit10, x, y)
    assert torch.equal(eng._sd_rows.cpu(), torch.from_numpy(table))
    u = eng.units[2]
    assert u["key"] == "s2u2" and u["residual"]
    h, w = u["hw_in"]
    x_in = u["x_in"]
    key = ("s2u2.out", B, h, w, x_in.shape[3])
    assert key in eng._bufs
    out = eng._bufs[key]
    dropped = [b for b in range(B) if table[2, b] == 0]
    kept = [b for b in range(B) if table[2, b] != 0]
    assert dropped and kept
    for b in dropped:
        assert torch.equal(_bits(out)[b], _bits(x_in)[b]), b
    for b in kept:
        assert not torch.equal(_bits(out)[b], _bits(x_in)[b]), b
    # backward: the branch of a dropped image got a zero upstream gradient, so gp[b] holds only the batch-statistics
    # terms -- and the skip gradient passed through: g_in is g_out (accumulated in place)
    assert u["dbg"]["g_in"] is u["dbg"]["g_out"]


def test_training_with_stochastic_depth_reduces_the_loss(batch, crit10):
    x, y = batch
    eng = _engine(0.2, seed=1)
    losses = [train_step(eng, crit10, x, y, lr=0.05).item() for _ in range(6)]
    assert all(math.isfinite(l) for l in losses), losses
    assert losses[-1] < losses[0], losses
    assert eng.sd_counter == 6


def test_graphed_step_refuses_stochastic_depth(batch, crit10):
    x, y = batch
    with pytest.raises(ValueError, match="stochastic depth"):
        GraphedStep(_engine(0.2), crit10, x, y, lr=0.05)


# ------------------------------------------------------------------------------------------------ driver

def test_driver_trains_with_the_flag_and_evaluation_ignores_it(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    draws = []
    real = ops.stochastic_depth_draw
    monkeypatch.setattr(ops, "stochastic_depth_draw", lambda *a, **k: (draws.append(a[4]), real(*a, **k))[1])
    common = ("--arch efficientnet_b0 --dataset CIFAR10 --batch-size 64 --synthetic 512 --image-size 64 --lr 0.05 "
              "--loss SoftTreeSupLoss --hierarchy induced-ResNet18").split()
    acc, _ = M.main(common + ["--epochs", "1", "--stochastic-depth", "0.2"])
    assert len(draws) == 8 and set(draws) == {0}            # one draw per training step, stream = rank 0; none in evaluation
    ck = "checkpoint/ckpt-CIFAR10-efficientnet_b0-lr0.05-induced-ResNet18-SoftTreeSupLoss.pth"
    assert os.path.exists(ck)
    state = torch.load(ck, map_location="cpu")
    assert state["acc"] == acc
    acc_plain, _ = M.main(common + ["--resume", "--eval"])
    acc_flag, _ = M.main(common + ["--resume", "--eval", "--stochastic-depth", "0.2"])
    assert len(draws) == 8
    assert acc_plain == acc_flag == acc          # the evaluation after training (P = 0.2 set) is the flagless one's
