"""nbdt_adamw_step / nbdt_rmsprop_step on the MI355X: bit for bit against the fp32 restatement (tests/_adaptive_ref.py) on a
ragged segment table, untouched gaps and the zero_grad contract, independence of the item boundaries, the engines'
adamw_step / rmsprop_step (per-parameter restatement, refreshed derived weights, EMA, the refusals), two data-parallel
ranks, and the driver's flags."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_path

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt.engine import AdamWConfig, LarsConfig, RMSpropConfig, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

import _adaptive_ref as A  # noqa: E402
from test_adaptive import GS, HP, kind_of  # noqa: E402

DEV = "cuda:0"
ITEM = ops.ARENA_OPT_ITEM


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu().view(torch.int16)


def _same_bits(got, want, what):
    got = got.detach().cpu()
    want = torch.as_tensor(want)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {int(bad.nonzero()[0])}: "
                           f"{got[bad][0].item()!r} != {want[bad][0].item()!r}")


def _inside(n, rows):
    m = torch.zeros(n, dtype=torch.bool)
    for r in rows:
        m[r[0]:r[0] + r[1]] = True
    return m


def _step(plan, name, p, g, s1, s2, t, mirror, zero_grad):
    hp = HP[name]
    if name == "adamw":
        plan.adamw(p, g, s1, s2, hp["lr"], hp["betas"], hp["eps"], t, GS, mirror, zero_grad=zero_grad)
    else:
        plan.rmsprop(p, g, s2, s1, hp["lr"], hp["alpha"], hp["eps"], hp["momentum"], name == "rmsprop_tf", GS, mirror,
                     zero_grad=zero_grad)


# ------------------------------------------------------------------------------------------------ 1, 2. ragged table
_case = {}


def _ragged(name):
    """The ragged case of optimizer `name`, its restatement after three steps and the device's run, computed once:
    (n, rows, inside, p0, s1_0, s2_0, grads, restatement, (p, g, s1, s2, mirror) from the device)."""
    if name not in _case:
        if "table" not in _case:
            _case["table"] = A.ragged_table(ITEM)
        n, rows, p0, b0, grads = _case["table"]
        s1_0, s2_0 = A.start_state(kind_of(name), n, rows, b0)
        ref = A.Fp32Ref(p0, s1_0, s2_0, rows)
        hp = HP[name]
        for t, gk in enumerate(grads, 1):
            if name == "adamw":
                ref.adamw(gk, hp["lr"], hp["betas"], hp["eps"], t, GS)
            else:
                ref.rmsprop(gk, hp["lr"], hp["alpha"], hp["eps"], hp["momentum"], name == "rmsprop_tf", GS)
        p, s1, s2, g = p0.to(DEV), s1_0.to(DEV), s2_0.to(DEV), torch.empty(n, device=DEV)
        mirror = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
        plan = ops.ArenaOptPlan(n, rows, device=DEV)
        assert _C.lib().nbdt_arena_opt_n(plan.handle) == n
        for t, gk in enumerate(grads, 1):
            g.copy_(gk)
            _step(plan, name, p, g, s1, s2, t, mirror, zero_grad=True)
        torch.cuda.synchronize()
        _case[name] = (n, rows, _inside(n, rows), p0, s1_0, s2_0, grads, ref, tuple(x.cpu() for x in (p, g, s1, s2, mirror)))
    return _case[name]


@pytest.mark.parametrize("name", list(HP))
def test_ragged_table_is_the_fp32_restatement_bit_for_bit(name):
    """Every operation of the update is a single IEEE fp32 operation and nothing crosses an element: random data must give
    the restatement's bits in p and both state arenas, after three steps, whole arena (the gaps included)."""
    n, rows, inside, p0, s1_0, s2_0, grads, ref, (p, g, s1, s2, mirror) = _ragged(name)
    assert [r[1] for r in rows] == [1, 3, 4, 5, 8, 1000, 2 * ITEM + 5]
    assert all(4 <= b[0] - (a[0] + a[1]) <= 11 for a, b in zip(rows, rows[1:])) and 4 <= n - (rows[-1][0] + rows[-1][1]) <= 11
    assert len({r[2] for r in rows}) == len(rows) and len(grads) == 3
    _same_bits(p, ref.p, name + " p")
    _same_bits(s1, ref.s1, name + " first state")
    _same_bits(s2, ref.s2, name + " second state")
    assert torch.isfinite(p).all() and not torch.equal(p[inside], p0[inside])
    assert torch.equal(mirror[inside], A.mirror(p)[inside])
    if name == "rmsprop_mu0":
        _same_bits(s1, s1_0, "the unused momentum buffer")


@pytest.mark.parametrize("name", list(HP))
def test_gaps_keep_their_sentinels_and_zero_grad_is_honoured(name):
    n, rows, inside, p0, s1_0, s2_0, grads, _, (p, g, s1, s2, mirror) = _ragged(name)
    k = int((~inside).sum())
    assert k > 0
    seven = torch.full((k,), 7.0)
    for t, what in ((p, "p"), (s1, "first state"), (s2, "second state")):
        _same_bits(t[~inside], seven, what + " in the gaps")
    _same_bits(mirror[~inside], seven.to(torch.bfloat16), "mirror in the gaps")
    assert int(torch.count_nonzero(g)) == 0 and not torch.signbit(g).any()        # zero_grad: all of g[0, n), +0.0
    # without zero_grad: g bit-unchanged, the same p
    pd, s1d, s2d, gd = p0.to(DEV), s1_0.to(DEV), s2_0.to(DEV), grads[0].to(DEV)
    plan = ops.ArenaOptPlan(n, rows, device=DEV)
    _step(plan, name, pd, gd, s1d, s2d, 1, None, zero_grad=False)
    _same_bits(gd, grads[0], "g without zero_grad")
    one = A.Fp32Ref(p0, s1_0, s2_0, rows)
    hp = HP[name]
    if name == "adamw":
        one.adamw(grads[0], hp["lr"], hp["betas"], hp["eps"], 1, GS)
    else:
        one.rmsprop(grads[0], hp["lr"], hp["alpha"], hp["eps"], hp["momentum"], name == "rmsprop_tf", GS)
    _same_bits(pd, one.p, "p after one step without a mirror")


def test_python_layer_refuses_wrong_lengths_and_the_library_bad_pointers():
    n, rows = _ragged("adamw")[:2]
    plan = ops.ArenaOptPlan(n, rows, device=DEV)
    good = [torch.zeros(n, device=DEV) for _ in range(4)]
    short = torch.zeros(n - 4, device=DEV)
    for i in range(4):                                      # n not matching the plan
        args = list(good)
        args[i] = short
        with pytest.raises(_C.NBDTHipError, match=f"{n} elements"):
            plan.adamw(*args, 1e-3, (0.9, 0.999), 1e-8, 1)
        with pytest.raises(_C.NBDTHipError, match=f"{n} elements"):
            plan.rmsprop(*args, 1e-3, 0.99, 1e-8, 0.9)
    with pytest.raises(_C.NBDTHipError, match="mirror"):
        plan.adamw(*good, 1e-3, (0.9, 0.999), 1e-8, 1, p_bf16=torch.zeros(n - 4, dtype=torch.bfloat16, device=DEV))
    lib = _C.lib()
    P, G, S1, S2 = (t.data_ptr() for t in good)
    for p, g, s1, s2, what in [(None, G, S1, S2, b"null"), (P, None, S1, S2, b"null"), (P, G, None, S2, b"null"),
                               (P, G, S1, None, b"null"), (P + 4, G, S1, S2, b"aligned"), (P, G, S1 + 8, S2, b"aligned"),
                               (P, G, S1, S2 + 4, b"aligned"), (P, G, P, S2, b"distinct")]:
        assert lib.nbdt_adamw_step(plan.handle, p, g, s1, s2, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None, 0, None) == -1
        assert what in lib.nbdt_last_error(), (what, lib.nbdt_last_error())
        assert lib.nbdt_rmsprop_step(plan.handle, p, g, s2, s1, 1e-3, 0.99, 1e-8, 0.9, 0, 1.0, None, 0, None) == -1
        assert what in lib.nbdt_last_error(), (what, lib.nbdt_last_error())
    mirror = torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV)
    assert lib.nbdt_adamw_step(plan.handle, P, G, S1, S2, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, mirror.data_ptr() + 2, 0, None) == -1
    # torch's form without momentum takes no buffer at all
    assert lib.nbdt_rmsprop_step(plan.handle, P, G, S2, None, 1e-3, 0.99, 1e-8, 0.0, 0, 1.0, None, 0, None) == 0
    assert lib.nbdt_rmsprop_step(plan.handle, P, G, S2, None, 1e-3, 0.99, 1e-8, 0.0, 1, 1.0, None, 0, None) == -1
    torch.cuda.synchronize()
    assert all(int(torch.count_nonzero(t)) == 0 for t in good)             # nothing was launched by a refused call


# ------------------------------------------------------------------------------------------------ 3. item boundaries
def test_adamw_does_not_depend_on_where_the_items_are_cut():
    """Decay 0, one segment over the whole arena against the same arena cut into many rows of ragged lengths (so the
    items and the lanes that take an element fall elsewhere): the same bits, in both modes of the switch."""
    gen = torch.Generator().manual_seed(11)
    n = 3 * ITEM + 12
    cuts = [0, 4, 12, ITEM // 4 + 12, ITEM + ITEM // 4 + 16, 2 * ITEM + ITEM // 2, 3 * ITEM, n]
    tables = {"one": [(0, n, 0.0)], "many": [(a, b - a, 0.0) for a, b in zip(cuts, cuts[1:])]}
    assert all(a % 4 == 0 and a < b for a, b in zip(cuts, cuts[1:])) and sum(r[1] for r in tables["many"]) == n
    assert max(r[1] for r in tables["many"]) > ITEM > min(r[1] for r in tables["many"])
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) for _ in range(2)]
    out = {}
    was = ops.is_deterministic()
    try:
        for tag, rows, det in (("one", tables["one"], False), ("many", tables["many"], False), ("det", tables["many"], True)):
            ops.set_deterministic(det)
            p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
            mirror = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
            plan = ops.ArenaOptPlan(n, rows, device=DEV)
            for t, gk in enumerate(grads, 1):
                plan.adamw(p, gk.to(DEV), m, v, 0.01, (0.9, 0.999), 1e-8, t, 1.0, mirror, zero_grad=True)
            out[tag] = (p.cpu(), m.cpu(), v.cpu(), mirror.cpu())
    finally:
        ops.set_deterministic(was)
    for tag in ("many", "det"):
        for a, b, what in zip(out["one"], out[tag], ("p", "m", "v", "mirror")):
            _same_bits(b, a, f"{what} ({tag} rows against one row)")
    assert not torch.equal(out["one"][0], p0)


# ------------------------------------------------------------------------------------------------ 4. engines
def _batch(B, size, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(DEV), torch.randint(0, classes, (B,), generator=g).to(DEV)


def _gradient(eng, crit, x, y):
    """train_step(..., zero_grad=False)'s pieces before the optimizer pass; returns host copies of (flat, grad, mom)."""
    eng.zero_grad()
    z = eng.forward(x, training=True)
    loss, gz = crit.loss_and_grad(z, y)
    eng.backward(gz)
    eng.join_side_stream()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    s = eng.store
    return s.flat.cpu(), s.grad.cpu(), s.mom.cpu()


def _check_engine_step(eng, rows, names, p0, g0, ref):
    """store.flat / mom / sq are the restatement's bits per parameter, the gaps untouched, the mirror bf16(flat)."""
    s = eng.store
    p1, m1, q1 = s.flat.cpu(), s.mom.cpu(), s.sq.cpu()
    moved = 0
    for name, (o, l, _) in zip(names, rows):
        _same_bits(p1[o:o + l], ref.p[o:o + l], name)
        _same_bits(m1[o:o + l], ref.s1[o:o + l], name + " (first state)")
        _same_bits(q1[o:o + l], ref.s2[o:o + l], name + " (second state)")
        moved += int(not torch.equal(p1[o:o + l], p0[o:o + l]))
    assert moved == len(names)
    inside = _inside(p0.numel(), rows)
    assert torch.equal(p1[~inside], p0[~inside]) and int(torch.count_nonzero(m1[~inside])) == 0
    assert int(torch.count_nonzero(q1[~inside])) == 0
    assert torch.equal(s.bf16.cpu(), p1.to(torch.bfloat16))
    assert torch.equal(s.grad.cpu(), g0) and not eng._grad_is_zero          # zero_grad=False: the gradient is still there


def test_wrn_engine_adamw_step_matches_the_restatement_per_parameter():
    eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=2)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    x, y = _batch(32, 32, 10, 7)
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-2
    store = eng.store
    assert store.sq is None and eng.opt_steps == 0
    rows = [r[:3] for r in store.segments(wd)]
    names = store.segment_names()
    assert any(w == 0.0 for _, _, w in rows) and any(w == wd for _, _, w in rows)      # 1-D entries are not decayed
    p0, g0, m0 = _gradient(eng, crit, x, y)
    assert int(torch.count_nonzero(m0)) == 0
    z0 = eng.forward(x, training=False).clone()
    eng.ema_enable(0.99)
    eng.adamw_step(lr, betas, eps, wd, zero_grad=False)
    torch.cuda.synchronize()
    assert eng.opt_steps == 1 and store.sq is not None
    ref = A.Fp32Ref(p0, m0, torch.zeros_like(p0), rows)
    ref.adamw(g0, lr, betas, eps, 1)
    _check_engine_step(eng, rows, names, p0, g0, ref)
    # derived weights were rebuilt: the next forward sees the new parameters
    z1 = eng.forward(x, training=False).clone()
    assert torch.isfinite(z1).all() and not torch.equal(z0, z1)
    # the average follows the stepped weights; no step while it is swapped in
    eng.ema_update()
    torch.cuda.synchronize()
    assert eng.ema_updates == 1 and torch.isfinite(store.ema).all() and not torch.equal(store.ema.cpu(), p0)
    eng.ema_swap()
    with pytest.raises(RuntimeError, match="swapped in"):
        eng.adamw_step(lr, betas, eps, wd)
    with pytest.raises(RuntimeError, match="swapped in"):
        eng.rmsprop_step(lr)
    eng.ema_swap()
    assert eng.opt_steps == 1                                              # the refused calls did not count
    # the state belongs to AdamW until it is reset
    with pytest.raises(RuntimeError, match="reset_optimizer_state"):
        eng.rmsprop_step(lr)
    with pytest.raises(RuntimeError, match="reset_optimizer_state"):
        eng.rmsprop_step(lr, tf=True)
    eng.reset_optimizer_state()
    assert eng.opt_steps == 0 and int(torch.count_nonzero(store.mom)) == 0 and int(torch.count_nonzero(store.sq)) == 0
    p1 = store.flat.cpu()
    eng.rmsprop_step(lr, 0.99, 1e-3, 0.9, wd, zero_grad=True)
    torch.cuda.synchronize()
    ref2 = A.Fp32Ref(p1, torch.zeros_like(p1), torch.zeros_like(p1), rows)
    ref2.rmsprop(g0, lr, 0.99, 1e-3, 0.9)
    _same_bits(store.flat, ref2.p, "rmsprop after the reset")
    assert eng.opt_steps == 1 and eng._grad_is_zero and int(torch.count_nonzero(store.grad)) == 0
    # train_step drives both through optim=, and refuses two optimizers at once
    with pytest.raises(RuntimeError, match="reset_optimizer_state"):
        train_step(eng, crit, x, y, lr=lr, optim=AdamWConfig())
    loss = train_step(eng, crit, x, y, lr=lr, optim=RMSpropConfig(0.99, 1e-3))
    assert math.isfinite(loss.item()) and eng.opt_steps == 2 and eng._grad_is_zero
    with pytest.raises(ValueError, match="lars= and optim="):
        train_step(eng, crit, x, y, lr=lr, lars=LarsConfig(), optim=AdamWConfig())
    with pytest.raises(TypeError, match="AdamWConfig"):
        train_step(eng, crit, x, y, lr=lr, optim="adamw")


def test_efficientnet_engine_rmsprop_tf_step_matches_the_restatement_per_parameter():
    from nbdt.engine_effnet import EfficientNetEngine
    eng = EfficientNetEngine(num_classes=1000, dropout_rate=0.0, device=DEV, seed=1)
    crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")
    x, y = _batch(32, 64, 1000, 9)
    lr, alpha, eps, mu, wd = 0.016, 0.9, 1e-3, 0.9, 1e-5                  # the published recipe's coefficients
    store = eng.store
    rows = [r[:3] for r in store.segments(wd)]
    names = store.segment_names()
    p0, g0, m0 = _gradient(eng, crit, x, y)
    z0 = eng.forward(x, training=False).clone()
    eng.ema_enable(0.9999)
    eng.rmsprop_step(lr, alpha, eps, mu, wd, tf=True, zero_grad=False)
    torch.cuda.synchronize()
    inside = _inside(p0.numel(), rows)
    ref = A.Fp32Ref(p0, m0, inside.float(), rows)                          # the mean square starts at 1 inside the segments
    ref.rmsprop(g0, lr, alpha, eps, mu, tf=True)
    s = eng.store
    p1, m1, q1 = s.flat.cpu(), s.mom.cpu(), s.sq.cpu()
    for name, (o, l, _) in zip(names, rows):
        _same_bits(p1[o:o + l], ref.p[o:o + l], name)
        _same_bits(m1[o:o + l], ref.s1[o:o + l], name + " (buffer)")
        _same_bits(q1[o:o + l], ref.s2[o:o + l], name + " (mean square)")
    assert torch.equal(p1[~inside], p0[~inside]) and int(torch.count_nonzero(q1[~inside])) == 0
    assert torch.equal(s.bf16.cpu(), p1.to(torch.bfloat16)) and not torch.equal(p1, p0)
    z1 = eng.forward(x, training=False).clone()
    assert torch.isfinite(z1).all() and not torch.equal(z0, z1)
    eng.ema_update()
    assert eng.ema_updates == 1 and torch.isfinite(store.ema).all()
    eng.ema_swap()
    with pytest.raises(RuntimeError, match="swapped in"):
        eng.rmsprop_step(lr, alpha, eps, mu, wd, tf=True)
    eng.ema_swap()
    with pytest.raises(RuntimeError, match="reset_optimizer_state"):
        eng.rmsprop_step(lr, alpha, eps, mu, wd, tf=False)                  # torch's form starts its mean square at 0
    with pytest.raises(RuntimeError, match="reset_optimizer_state"):
        eng.adamw_step(lr)
    loss = train_step(eng, crit, x, y, lr=lr, weight_decay=wd, optim=RMSpropConfig(alpha, eps, True))
    assert math.isfinite(loss.item()) and eng.opt_steps == 2 and eng._grad_is_zero


# ------------------------------------------------------------------------------------------------ 5. two ranks
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _adaptive_dp_worker(rank, world, port, out_dir, backend, devices):
    import nbdt_path as npth
    npth.add()
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(devices[rank]),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist
    from nbdt import dist as nd
    from nbdt.engine import AdamWConfig as Adam, RMSpropConfig as Rms, WRNEngine as Eng, train_step as step
    from nbdt.loss import SoftTreeSupLoss as Loss
    dev = torch.device("cuda", devices[rank])
    torch.cuda.set_device(dev)
    nd.init_from_env(backend=backend)
    crit = Loss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    g = torch.Generator().manual_seed(9)
    gx, gy = torch.randn(32, 3, 32, 32, generator=g), torch.randint(0, 10, (32,), generator=g)
    x, y = nd.shard_batch(gx, rank, world).to(dev), nd.shard_batch(gy, rank, world).to(dev)
    comm = nd.GradComm()
    assert comm.world_size == world
    out = {}
    for tag, cfg, lr in (("adamw", Adam(), 1e-3), ("rmsprop_tf", Rms(0.9, 1e-3, True), 0.01)):
        eng = Eng(num_classes=10, blocks=10, width_factor=2, device=dev, seed=5)
        losses = [step(eng, crit, x, y, lr=lr, comm=comm, optim=cfg).item() for _ in range(3)]
        torch.cuda.synchronize()
        out[tag] = {"flat": eng.store.flat.cpu(), "mom": eng.store.mom.cpu(), "sq": eng.store.sq.cpu(), "losses": losses,
                    "t": eng.opt_steps}
    torch.save(out, os.path.join(out_dir, f"adaptive{rank}.pt"))
    dist.destroy_process_group()


def run_two_ranks(out_dir, backend, devices):
    """A fresh child process per rank; returns what each rank saved."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_adaptive_dp_worker, args=(world, _free_port(), str(out_dir), backend, devices), nprocs=world, join=True)
    return [torch.load(os.path.join(str(out_dir), f"adaptive{r}.pt")) for r in range(world)]


def check_two_ranks(a, b):
    for tag in ("adamw", "rmsprop_tf"):
        for key in ("flat", "mom", "sq"):
            assert torch.equal(a[tag][key], b[tag][key]), (tag, key)
        assert a[tag]["t"] == b[tag]["t"] == 3
        assert all(math.isfinite(l) for l in a[tag]["losses"] + b[tag]["losses"])
        assert int(torch.count_nonzero(a[tag]["mom"])) > 0 and int(torch.count_nonzero(a[tag]["sq"])) > 0


def test_two_ranks_stay_bit_identical_under_adamw_and_rmsprop(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    check_two_ranks(*run_two_ranks(tmp_path, "nccl", [0, 1]))


# ------------------------------------------------------------------------------------------------ 6. driver
def test_driver_runs_each_new_optimizer(tmp_path, monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nbdt_main_adaptive", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    base = "--arch ResNet18 --synthetic 512 --epochs 2 --batch-size 128".split()

    def losses_of(out):
        v = [float(s) for s in re.findall(r"^Loss: ([-0-9.a-z]+) \(", out, flags=re.M)]
        assert len(v) == 2 and all(math.isfinite(s) for s in v), out
        assert [int(m) for m in re.findall(r"\((\d+) steps of", out)] == [4, 4]

    M.main(base + "--optimizer adamw --lr 0.001 --weight-decay 0.01".split())          # returns: exit status 0
    out = capsys.readouterr().out
    assert "Checkpoints will be saved to: ./checkpoint/ckpt-CIFAR10-ResNet18-lr0.001-adamw.pth" in out
    losses_of(out)
    assert re.findall(r"Epoch: (\d+) / LR: ([0-9.]+)\n", out) == [(str(e), "%.04f" % M.multistep_lr(0.001, e, 2)) for e in (0, 1)]
    M.main(base + ("--optimizer rmsprop --rmsprop-tf --lr 0.01 --weight-decay 1e-5 --lr-schedule exp --lr-decay-rate 0.5 "
                   "--lr-decay-epochs 0.5 --warmup-epochs 1 --ema-decay 0.9999").split())
    out = capsys.readouterr().out
    assert "Checkpoints will be saved to: ./checkpoint/ckpt-CIFAR10-ResNet18-lr0.01-rmsprop-ema.pth" in out
    losses_of(out)
    logged = re.findall(r"Epoch: (\d+) / LR: ([0-9.]+) -> ([0-9.]+)", out)
    assert [int(e) for e, _, _ in logged] == [0, 1]
    for e, first, last in logged:                     # warm-up over epoch 0, then 0.5 x every 2 steps: 0.01 0.01 0.005 0.005
        want = [M.lr_at(0.01, int(e) * 4 + i, 4, 2, "exp", 1.0, 0.5, 0.5) for i in (0, 3)]
        assert [first, last] == ["%.6f" % w for w in want], (e, first, last, want)
    assert logged[1][1:] == ("0.010000", "0.005000")
    assert "EMA Accuracy" in out
