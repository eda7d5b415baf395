"""nbdt_lars_step on the MI355X: an exactly representable fixture bit for bit, a ragged segment table against the float64
reference (tests/_lars_ref.py), degenerate norms, agreement with the SGD kernel, run-to-run reproducibility, the engines'
lars_step (per-parameter reference, refreshed derived weights), two data-parallel ranks and the driver's flags."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_path

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402
from nbdt.engine import LarsConfig, ResNetEngine, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

import _lars_ref as R  # noqa: E402
from test_lars import check_segment_table  # noqa: E402

DEV = "cuda:0"
RTOL, ATOL, RATIO_RTOL = 1e-5, 1e-6, 1e-5      # p / buf: the bounds of test_sgd_matches_torch_optim; ratios: see test 2


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bad = err > ATOL + RTOL * want.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} off, max err {err.max().item():.3e}"


def _inside(n, segments):
    m = torch.zeros(n, dtype=torch.bool)
    for o, l, _, _ in segments:
        m[o:o + l] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. exact fixture
def _exact_expected(L, sign, steps, wd, trust, eps, momentum, lr, gs):
    """float32 evaluation of the formula, one rounding per operation, after checking that every sum of squares (and
    every partial sum of it, whatever the order) is exactly representable."""
    f = np.float32
    p, g, buf = (f(2.0) * sign).astype(f), (f(1.0) * sign).astype(f), np.zeros(L, f)
    ratios = []
    for _ in range(steps):
        norms = []
        for v in (p, (f(gs) * g).astype(f)):
            c = float(v[0]) ** 2
            assert np.all(np.abs(v.astype(np.float64)) == abs(float(v[0]))) and float(f(v[0]) * f(v[0])) == c
            k = np.arange(1, L + 1, dtype=np.float64) * c                    # every partial sum is k * c for some k <= L
            assert np.all(k.astype(f).astype(np.float64) == k) and k[-1] < 2 ** 24
            norms.append(np.sqrt(f(k[-1])))
        wn, gn = norms
        r = f(f(f(trust) * wn) / f(f(gn + f(f(wd) * wn)) + f(eps)))
        ratios.append(r)
        u = (r * ((f(gs) * g).astype(f) + (f(wd) * p).astype(f)).astype(f)).astype(f)
        buf = ((f(momentum) * buf).astype(f) + u).astype(f)
        p = (p - (f(lr) * buf).astype(f)).astype(f)
    return p, buf, ratios


@pytest.mark.parametrize("flip", [False, True])
def test_exact_fixture_bit_for_bit(flip):
    hp = dict(wd=0.5, trust=0.25, eps=0.0, momentum=0.5, lr=0.5, gs=1.0)
    lengths, segments, off = [16, 64, 4096], [], 0
    for L in lengths:
        segments.append((off, L, hp["wd"], 1))
        off += L
    n = off
    want_p, want_b, want_r = np.zeros(n, np.float32), np.zeros(n, np.float32), []
    p0, g0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for (o, L, _, _) in segments:
        sign = np.where(np.arange(L) % 2 == 1, -1.0, 1.0).astype(np.float32) if flip else np.ones(L, np.float32)
        p0[o:o + L], g0[o:o + L] = 2.0 * sign, 1.0 * sign
        want_p[o:o + L], want_b[o:o + L], r = _exact_expected(L, sign, 2, **hp)
        want_r.append(r)
        assert float(r[0]) == 0.25               # first step: wn = 2 sqrt(L), gn = sqrt(L), the denominator a power of two
    p, g = torch.from_numpy(p0).to(DEV), torch.from_numpy(g0).to(DEV)
    buf, mirror = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    plan = ops.LarsPlan(n, segments, device=DEV)
    assert torch.equal(plan.ratios(), torch.ones(3))
    for step in range(2):
        plan.step(p, g, buf, hp["lr"], hp["momentum"], hp["trust"], hp["eps"], hp["gs"], mirror, zero_grad=False)
        got = plan.ratios().numpy()
        assert got.tobytes() == np.array([r[step] for r in want_r], np.float32).tobytes(), (step, got)
    assert torch.equal(g.cpu(), torch.from_numpy(g0))                         # zero_grad = 0: untouched
    assert p.cpu().numpy().tobytes() == want_p.tobytes() and buf.cpu().numpy().tobytes() == want_b.tobytes()
    assert torch.equal(mirror, p.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ 2. ragged table
_RAGGED_HP = dict(lr=0.02, momentum=0.9, trust=0.5, eps=1e-8, gs=0.5)
_ragged_cache = {}


def _ragged():
    """The ragged case and its float64 reference, computed once: (n, segments, p0, buf0, grads, reference after three steps
    (p, buf, ratios of the last step))."""
    if not _ragged_cache:
        n, segments, p0, b0, grads = R.ragged_case(ops.LARS_ITEM)
        hp = _RAGGED_HP
        ref = R.LarsRef(p0, b0, segments, hp["momentum"])
        for g in grads:
            before = ref.param.clone()
            ratios = ref.step(g, hp["lr"], hp["trust"], hp["eps"], hp["gs"])
            assert (ref.param - before).abs().max().item() < 0.1        # the scale the tolerances below are stated for
        _ragged_cache["case"] = (n, segments, p0, b0, grads, (ref.param.clone(), ref.buf.clone(), ratios))
    return _ragged_cache["case"]


def _run_ragged():
    n, segments, p0, b0, grads, _ = _ragged()
    hp = _RAGGED_HP
    p, buf, g = p0.to(DEV), b0.to(DEV), torch.empty(n, device=DEV)
    mirror = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    plan = ops.LarsPlan(n, segments, device=DEV)
    for gk in grads:
        g.copy_(gk)
        plan.step(p, g, buf, hp["lr"], hp["momentum"], hp["trust"], hp["eps"], hp["gs"], mirror, zero_grad=True)
    return p, buf, g, mirror, plan.ratios()


def test_ragged_table_matches_the_fp64_reference():
    """Ratios to 1e-5 relative: a pairwise fp32 sum of n <= 2^22 non-negative terms is off by at most about
    (log2 n + 2) 2^-24 = 1.5e-6, the square root halves it, the quotient adds two roundings -- a 6x margin."""
    n, segments, p0, b0, grads, (ref_p, ref_b, ref_r) = _ragged()
    assert max(l for _, l, _, _ in segments) > 3 * 4 * ops.LARS_ITEM and [l for _, l, _, _ in segments][:6] == [1, 3, 4, 5, 8, 1000]
    p, buf, g, mirror, ratios = _run_ragged()
    inside = _inside(n, segments)
    assert 0 < int((~inside).sum()) and all(4 <= b[0] - (a[0] + a[1]) <= 12 for a, b in zip(segments, segments[1:]))
    for (o, l, _, adapt), got, want in zip(segments, ratios.tolist(), ref_r):
        assert abs(got - want) <= RATIO_RTOL * abs(want), (o, l, got, want)
        assert adapt or got == 1.0
    pc, bc = p.cpu(), buf.cpu()
    _close(pc[inside], ref_p[inside], "p")
    _close(bc[inside], ref_b[inside], "buf")
    seven = torch.full((int((~inside).sum()),), 7.0)
    assert torch.equal(pc[~inside], seven) and torch.equal(bc[~inside], seven)          # sentinels: bit-unchanged
    assert torch.equal(mirror.cpu()[~inside], seven.to(torch.bfloat16))
    assert torch.equal(mirror.cpu()[inside], pc.to(torch.bfloat16)[inside])
    assert int(torch.count_nonzero(g)) == 0                                             # zero_grad: all of g[0, n)


def test_ragged_update_is_the_fp32_formula_bit_for_bit():
    """The element update alone, exactly: with the kernel's own ratios (plan.ratios(), so the order of the norm sums does
    not enter) u = r (gs g + wd p), buf = mu buf + u, p = p - lr buf evaluated in numpy float32 -- one rounding per
    operation, which is what -ffp-contract=off makes of csrc/lars.hip -- gives the bytes of p, buf and the mirror inside
    every segment of the ragged table (float4 bodies, length % 4 tails, items of every length), after each of three steps."""
    n, segments, p0, b0, grads, _ = _ragged()
    hp, f = _RAGGED_HP, np.float32
    lr, mu, gs = f(hp["lr"]), f(hp["momentum"]), f(hp["gs"])
    inside = _inside(n, segments)
    want_p, want_b = p0.numpy().copy(), b0.numpy().copy()
    p, buf, g = p0.to(DEV), b0.to(DEV), torch.empty(n, device=DEV)
    mirror = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    plan = ops.LarsPlan(n, segments, device=DEV)
    for step, gk in enumerate(grads):
        g.copy_(gk)
        plan.step(p, g, buf, hp["lr"], hp["momentum"], hp["trust"], hp["eps"], hp["gs"], mirror, zero_grad=True)
        ratios, gn = plan.ratios().numpy(), gk.numpy()
        assert ratios.dtype == gn.dtype == want_p.dtype == np.float32
        for (o, l, wd, _), r in zip(segments, ratios):
            sl = slice(o, o + l)
            u = r * (gs * gn[sl] + f(wd) * want_p[sl])
            want_b[sl] = mu * want_b[sl] + u
            want_p[sl] = want_p[sl] - lr * want_b[sl]
        assert want_p.dtype == want_b.dtype == np.float32
        got_p, got_b = p.cpu(), buf.cpu()
        m = inside.numpy()
        assert got_p.numpy()[m].tobytes() == want_p[m].tobytes(), f"p, step {step}"
        assert got_b.numpy()[m].tobytes() == want_b[m].tobytes(), f"buf, step {step}"
        assert torch.equal(mirror.cpu()[inside], torch.from_numpy(want_p).to(torch.bfloat16)[inside]), f"mirror, step {step}"


# ------------------------------------------------------------------------------------------------ 3. degenerate norms
def test_degenerate_norms_take_ratio_one():
    gen = torch.Generator().manual_seed(5)
    n, L = 2 * 1032, 1027
    segments = [(0, L, 0.1, 1), (1032, L, 0.1, 1)]
    p0, g0 = torch.zeros(n), torch.zeros(n)
    p0[:L] = torch.randn(L, generator=gen)              # segment 0: g == 0 -> moves by decay alone
    g0[1032:1032 + L] = torch.randn(L, generator=gen)   # segment 1: p == 0 -> a plain SGD step
    p, g, buf = p0.to(DEV), g0.to(DEV), torch.zeros(n, device=DEV)
    plan = ops.LarsPlan(n, segments, device=DEV)
    lr, mom = 0.05, 0.9
    plan.step(p, g, buf, lr, mom, 0.25, 0.0, 1.0, None, zero_grad=False)
    assert plan.ratios().tolist() == [1.0, 1.0]
    ref = R.LarsRef(p0, torch.zeros(n), segments, mom)
    assert ref.step(g0, lr, 0.25, 0.0, 1.0) == [1.0, 1.0]
    pc, bc = p.cpu(), buf.cpu()
    assert torch.isfinite(pc).all() and torch.isfinite(bc).all()
    _close(pc, ref.param, "p")
    _close(bc, ref.buf, "buf")
    _close(pc[:L], p0[:L].double() * (1 - lr * 0.1), "decay alone")
    _close(pc[1032:1032 + L], -lr * g0[1032:1032 + L].double(), "plain SGD step")


# ------------------------------------------------------------------------------------------------ 4. against the SGD kernel
def test_one_unadapted_segment_agrees_with_the_sgd_kernel():
    gen = torch.Generator().manual_seed(6)
    n = 100003 // 4 * 4
    p0, g0, b0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen)
    out = {}
    plan = ops.LarsPlan(n, [(0, n, 5e-4, 0)], device=DEV)
    for tag in ("sgd", "lars"):
        p, g, buf = p0.to(DEV), g0.to(DEV), b0.to(DEV)
        mirror = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        for _ in range(2):
            if tag == "sgd":
                ops.sgd_step(p, g, buf, 0.05, 0.9, 5e-4, 0.5, mirror, zero_grad=False)
            else:
                plan.step(p, g, buf, 0.05, 0.9, 1e-3, 1e-8, 0.5, mirror, zero_grad=False)
        assert torch.equal(mirror, p.to(torch.bfloat16))
        out[tag] = (p.cpu(), buf.cpu())
    _close(out["lars"][0], out["sgd"][0], "p")
    _close(out["lars"][1], out["sgd"][1], "buf")


# ------------------------------------------------------------------------------------------------ 5. reproducible
def test_ragged_step_is_bit_reproducible_in_both_modes():
    runs = []
    was = ops.is_deterministic()
    try:
        for det in (False, False, True, True):
            ops.set_deterministic(det)
            p, buf, _, _, ratios = _run_ragged()
            runs.append((p.cpu(), buf.cpu(), ratios))
    finally:
        ops.set_deterministic(was)
    for p, buf, ratios in runs[1:]:
        assert torch.equal(p, runs[0][0]) and torch.equal(buf, runs[0][1]) and torch.equal(ratios, runs[0][2])


# ------------------------------------------------------------------------------------------------ 6. engines
def _batch(B, size, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(DEV), torch.randint(0, classes, (B,), generator=g).to(DEV)


def _assert_refreshed(eng, fresh, x):
    """Every derived weight layout was rebuilt from the updated parameters: the next eval forward equals, bit for bit, the
    forward of a fresh engine that loaded this engine's state dict.  (Deterministic mode while the two forwards run, so
    that no reduction order stands between two launches of the same kernels on the same bits.)"""
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        z = eng.forward(x, training=False).clone()
        fresh.load_state_dict(eng.state_dict())
        z2 = fresh.forward(x, training=False).clone()
    finally:
        ops.set_deterministic(was)
    assert torch.isfinite(z).all() and torch.equal(z, z2), f"max diff {(z - z2).abs().max().item():.3e}"


def test_wrn_engine_lars_step_matches_the_reference_per_parameter():
    eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=2)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    x, y = _batch(32, 32, 10, 7)
    lr, mom, wd, trust, eps = 0.5, 0.9, 5e-4, 0.05, 1e-8
    store = eng.store
    segments = check_segment_table(store, wd)
    names = store.segment_names()
    # train_step(..., zero_grad=False)'s pieces by hand: the gradient is read before the optimizer pass
    eng.zero_grad()
    z = eng.forward(x, training=True)
    loss, gz = crit.loss_and_grad(z, y)
    eng.backward(gz)
    eng.join_side_stream()
    torch.cuda.synchronize()
    p0, g0, b0 = store.flat.cpu(), store.grad.cpu(), store.mom.cpu()
    eng.lars_step(lr, mom, wd, trust, eps, zero_grad=False)
    torch.cuda.synchronize()
    assert math.isfinite(loss.item()) and not eng._grad_is_zero and torch.equal(store.grad.cpu(), g0)
    ref = R.LarsRef(p0, b0, segments, mom)
    ref_r = ref.step(g0, lr, trust, eps, 1.0)
    p1, b1 = store.flat.cpu(), store.mom.cpu()
    ratios = eng.last_trust_ratios()
    assert list(ratios) == names and set(eng.named_params("flat")) <= set(names)
    moved = 0
    for name, (o, l, _, adapt), want in zip(names, segments, ref_r):
        _close(p1[o:o + l], ref.param[o:o + l], name)
        _close(b1[o:o + l], ref.buf[o:o + l], name + " (momentum)")
        if len(store.entries[name][1]) <= 1:            # 1-D: a plain SGD step, no decay, ratio exactly 1
            assert ratios[name] == 1.0 and adapt == 0, name
            _close(p1[o:o + l], p0[o:o + l].double() - lr * g0[o:o + l].double(), name + " (no decay)")
        else:
            assert ratios[name] != 1.0 and abs(ratios[name] - want) <= RATIO_RTOL * abs(want), (name, ratios[name], want)
            moved += int(not torch.equal(p1[o:o + l], p0[o:o + l]))
    assert moved == sum(len(store.entries[nm][1]) > 1 for nm in names)
    assert torch.equal(store.bf16.cpu(), store.flat.cpu().to(torch.bfloat16))
    inside = _inside(store.flat.numel(), segments)
    assert torch.equal(p1[~inside], p0[~inside]) and torch.equal(b1[~inside], b0[~inside])
    _assert_refreshed(eng, WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=99), x)
    # zero_grad=True leaves the gradient buffer zeroed and the engine knows it
    train_step(eng, crit, x, y, lr=0.1, lars=LarsConfig(trust))
    assert eng._grad_is_zero and int(torch.count_nonzero(store.grad)) == 0


@pytest.mark.parametrize("arch", ["ResNet18", "efficientnet_b0"])
def test_lars_step_refreshes_derived_weights(arch):
    if arch == "ResNet18":
        make = lambda seed: ResNetEngine(num_classes=10, num_blocks=(2, 2, 2, 2), device=DEV, seed=seed)  # noqa: E731
        crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
        x, y = _batch(32, 32, 10, 8)
    else:
        from nbdt.engine_effnet import EfficientNetEngine
        make = lambda seed: EfficientNetEngine(num_classes=1000, dropout_rate=0.0, device=DEV, seed=seed)  # noqa: E731
        crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")
        x, y = _batch(32, 64, 1000, 9)
    eng = make(1)
    check_segment_table(eng.store, 5e-4)
    before = eng.store.flat.clone()
    for _ in range(2):
        loss = train_step(eng, crit, x, y, lr=0.2, lars=LarsConfig(0.02))
    assert math.isfinite(loss.item()) and eng._grad_is_zero and not torch.equal(before, eng.store.flat)
    r = eng.last_trust_ratios()
    assert all(math.isfinite(v) and v > 0 for v in r.values())
    assert all(v == 1.0 for k, v in r.items() if len(eng.store.entries[k][1]) <= 1)
    _assert_refreshed(eng, make(77), x)


# ------------------------------------------------------------------------------------------------ 7. two ranks
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _lars_dp_worker(rank, world, port, out_dir, backend, devices):
    import nbdt_path as npth
    npth.add()
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(devices[rank]),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist
    from nbdt import dist as nd
    from nbdt.engine import LarsConfig as Cfg, WRNEngine as Eng, train_step as step
    from nbdt.loss import SoftTreeSupLoss as Loss
    dev = torch.device("cuda", devices[rank])
    torch.cuda.set_device(dev)
    nd.init_from_env(backend=backend)
    eng = Eng(num_classes=10, blocks=10, width_factor=2, device=dev, seed=5)
    crit = Loss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    g = torch.Generator().manual_seed(9)
    gx, gy = torch.randn(32, 3, 32, 32, generator=g), torch.randint(0, 10, (32,), generator=g)
    x, y = nd.shard_batch(gx, rank, world).to(dev), nd.shard_batch(gy, rank, world).to(dev)
    comm = nd.GradComm()
    assert comm.world_size == world
    losses = [step(eng, crit, x, y, lr=0.2, comm=comm, lars=Cfg(0.02)).item() for _ in range(3)]
    torch.cuda.synchronize()
    ratios = eng.last_trust_ratios()
    torch.save({"flat": eng.store.flat.cpu(), "mom": eng.store.mom.cpu(), "ratios": ratios, "losses": losses},
               os.path.join(out_dir, f"lars{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_stay_bit_identical_under_lars(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    multi = torch.cuda.device_count() >= 2
    backend, devices = ("nccl", [0, 1]) if multi else ("gloo", [0, 0])
    mp.spawn(_lars_dp_worker, args=(world, _free_port(), str(tmp_path), backend, devices), nprocs=world, join=True)
    a, b = (torch.load(tmp_path / f"lars{r}.pt") for r in range(world))
    assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["mom"], b["mom"])
    assert a["ratios"] == b["ratios"] and any(v != 1.0 for v in a["ratios"].values())
    assert all(math.isfinite(l) for l in a["losses"] + b["losses"])


# ------------------------------------------------------------------------------------------------ 8. driver
def test_driver_lars_warmup_cosine_and_the_default_path(tmp_path, monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nbdt_main_lars", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    base = "--arch ResNet18 --synthetic 512 --epochs 2 --batch-size 128".split()
    M.main(base + "--optimizer lars --warmup-epochs 1 --lr-schedule cosine".split())          # returns: exit status 0
    out = capsys.readouterr().out
    assert "Checkpoints will be saved to: ./checkpoint/ckpt-CIFAR10-ResNet18-lars.pth" in out
    spe = [int(m) for m in re.findall(r"\((\d+) steps of", out)]
    assert spe == [4, 4]
    logged = re.findall(r"Epoch: (\d+) / LR: ([0-9.]+) -> ([0-9.]+)", out)
    assert [int(e) for e, _, _ in logged] == [0, 1]
    for e, first, last in logged:
        e = int(e)
        want = [M.lr_at(0.1, e * 4 + i, 4, 2, "cosine", 1.0) for i in (0, 3)]
        assert [first, last] == ["%.6f" % w for w in want], (e, first, last, want)
    losses = [float(v) for v in re.findall(r"^Loss: ([-0-9.a-z]+) \(", out, flags=re.M)]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out
    M.main(base)
    out = capsys.readouterr().out
    assert re.findall(r"Epoch: (\d+) / LR: ([0-9.]+)\n", out) == [(str(e), "%.04f" % M.multistep_lr(0.1, e, 2)) for e in (0, 1)]
    assert "->" not in out and "Checkpoints will be saved to: ./checkpoint/ckpt-CIFAR10-ResNet18.pth" in out
