"""The weight EMA on the MI355X, every comparison bit for bit against tests/_ema_ref.py: the update and swap kernels and
their _multi forms, the engines' ema_enable / ema_update / ema_swap / ema_weights / state dicts, and the driver's flags.
All under ops.set_deterministic(True), restored afterwards."""
import math
import os
import re

import pytest
import torch
import torch.nn as nn

import nbdt_path

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402
from nbdt.engine import ResNetEngine, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

import _ema_ref as R  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _deterministic():
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


def _update_data(n, seed):
    """p and e (CPU, fp32) in five strides: unrelated normals; equal values; neighbours one ulp apart; normal values just
    above the smallest normal whose differences are denormal; denormal values."""
    g = torch.Generator().manual_seed(seed)
    p, e = torch.randn(n, generator=g), torch.randn(n, generator=g)
    k = torch.arange(n) % 5
    e[k == 1] = p[k == 1]
    e[k == 2] = torch.nextafter(p[k == 2], torch.full_like(p[k == 2], math.inf))
    tiny = 2.0 ** -126
    p[k == 3] = tiny * (1.0 + torch.rand(int((k == 3).sum()), generator=g))
    e[k == 3] = tiny * (1.0 + torch.rand(int((k == 3).sum()), generator=g))
    p[k == 4] = 2.0 ** -140 * torch.randn(int((k == 4).sum()), generator=g)
    e[k == 4] = 2.0 ** -140 * torch.randn(int((k == 4).sum()), generator=g)
    if n > 8:
        d = (p - e)[k == 3]
        assert ((d != 0) & (d.abs() < tiny)).any() and (p[k == 4].abs() < tiny).all() and (p[k == 4] != 0).any()
    return p, e


def _ties_data(n, seed):
    """fp32 values for the bf16 mirror: random ones, and exact ties (low half 0x8000) above even and odd bf16 mantissas."""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(0x0080, 0x7f00, (n,), generator=g, dtype=torch.int32)          # finite, normal bf16 patterns
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 31
    low = torch.randint(0, 0x10000, (n,), generator=g, dtype=torch.int32)
    k = torch.arange(n) % 4
    low[k == 0] = 0x8000                        # ties
    low[k == 1] = 0x7fff                        # just below / just above one
    low[k == 2] = 0x8001
    v = ((hi << 16) | low | sign).view(torch.float32)
    assert torch.isfinite(v).all()
    odd = ((hi >> 0) & 1 == 1) & (k == 0)
    assert n < 8 or (odd.any() and ((k == 0) & ~odd).any())
    return v


# ------------------------------------------------------------------------------------------------ 1. update
@pytest.mark.parametrize("n", [4, 1028, 262148])
def test_update_bit_for_bit(n):
    p0, e0 = _update_data(n, 11 + n)
    p = p0.to(DEV)
    for omd in (0.0, 2.0 ** -13, R.omd32(0.9), R.omd32(0.1), 1.0):      # 0, 2^-13, float32(0.1), float32(0.9), 1
        e = e0.to(DEV)
        ops.ema_update(p, e, omd)
        want = R.update_(e0.clone(), p0, omd)
        _same(e, want, f"n = {n}, one_minus_decay = {omd!r}")
        _same(p, p0, "p is only read")
        if omd == 0.0:
            assert torch.equal(e.cpu(), e0), "one_minus_decay = 0 adds a zero: the same values (-0 + 0 is +0)"
    # several updates in a row stay on the restatement's bits (a moving target)
    e, want = e0.to(DEV), e0.clone()
    for t in range(3):
        q0 = p0 + 0.01 * t
        ops.ema_update(q0.to(DEV), e, R.omd32(R.decay_at(t)))
        R.update_(want, q0, R.omd32(R.decay_at(t)))
    _same(e, want, "three updates up the ramp")


# ------------------------------------------------------------------------------------------------ 2. swap
@pytest.mark.parametrize("n", [4, 1028, 262148])
def test_swap_exchanges_and_mirrors(n):
    p0, e0 = _ties_data(n, 5 + n), _ties_data(n, 7 + n)
    p, e = p0.to(DEV), e0.to(DEV)
    sentinel = torch.full((n,), -7.0, dtype=torch.bfloat16)
    m = sentinel.to(DEV)
    ops.ema_swap(p, e, m)
    _same(p, e0, "p holds the shadow's values")
    _same(e, p0, "the shadow holds p's values")
    _same(m, R.mirror(e0), "the mirror of the new p, ties to even")
    ops.ema_swap(p, e, m)
    _same(p, p0, "two swaps: p")
    _same(e, e0, "two swaps: the shadow")
    _same(m, R.mirror(p0), "two swaps: the mirror")
    m = sentinel.to(DEV)
    ops.ema_swap(p, e)                                                    # no mirror: nothing else is written
    _same(p, e0, "swap without a mirror")
    _same(m, sentinel, "a mirror that was not passed")


# ------------------------------------------------------------------------------------------------ 3. _multi
@pytest.mark.parametrize("lengths", [[2048], [32, 96, 2048, 96, 32, 2048, 32]])
def test_multi_tables_bit_for_bit(lengths):
    total = sum(lengths)
    p0, e0 = _update_data(total + 64, 3 + len(lengths))
    # the live tensors are separate allocations with a bystander between them; the shadows are views of one flat tensor
    live, off = [], 0
    for L in lengths:
        live.append(p0[off:off + L].to(DEV))
        off += L
    bystander0 = p0[off:off + 32].clone()
    bystander = bystander0.to(DEV)
    flat0 = torch.cat([e0[:total], e0[total:total + 32]])                 # 32 more elements that are in no row
    flat = flat0.to(DEV)
    views, off = [], 0
    for L in lengths:
        views.append(flat[off:off + L])
        off += L
    table = ops.EmaTable(list(zip(live, views)), DEV)
    assert table.n_rows == len(lengths)
    want = flat0.clone()
    for omd in (R.omd32(0.9), 2.0 ** -13, 1.0, 0.0):
        table.update(omd)
        R.update_(want[:total], p0[:total], omd)
        _same(flat, want, f"update, one_minus_decay = {omd!r}")
    _same(torch.cat(live), p0[:total], "the live tensors are only read")
    table.swap()
    _same(torch.cat(live), want[:total], "swap: the live tensors hold the averages")
    _same(flat[:total], p0[:total], "swap: the shadows hold the live values")
    _same(flat[total:], flat0[total:], "the shadow's tail, in no row")
    _same(bystander, bystander0, "a neighbouring tensor, in no row")
    table.swap()
    _same(torch.cat(live), p0[:total], "two swaps")
    _same(flat, want, "two swaps: the shadows")


# ------------------------------------------------------------------------------------------------ 4. engine
def _batch(B, size, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(DEV), torch.randint(0, classes, (B,), generator=g).to(DEV)


def _cpu(sd):
    return {k: v.detach().cpu().clone() for k, v in sd.items()}


def _same_dict(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        if want[k].is_floating_point():
            _same(got[k], want[k], f"{what}: {k}")
        else:
            assert int(got[k]) == int(want[k]), f"{what}: {k}"


def _live_bits(eng):
    return ([eng.store.flat.cpu(), eng.store.bf16.cpu()] + [b.running_mean.cpu() for b in eng.bns]
            + [b.running_var.cpu() for b in eng.bns], [b.num_batches_tracked for b in eng.bns])


def test_wrn_engine_average_swap_and_state_dicts():
    from nbdt.models._hip_module import HipBackbone
    make = lambda seed: WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=seed)  # noqa: E731
    eng, twin = make(3), make(3)
    net = HipBackbone(eng)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    x, y = _batch(32, 32, 10, 7)
    with pytest.raises(RuntimeError, match="ema_enable"):
        eng.ema_update()
    eng.ema_enable(decay=0.9999, warmup=True)
    assert eng.ema_updates == 0 and not eng.ema_swapped
    want = _cpu(eng.state_dict())
    _same_dict(eng.ema_state_dict(), want, "the average starts as the weights")
    for t in range(3):
        la = train_step(eng, crit, x, y, lr=0.05)
        eng.ema_update()
        lb = train_step(twin, crit, x, y, lr=0.05)
        assert math.isfinite(la.item()) and _bits(la).item() == _bits(lb).item()
        R.fold_(want, eng.state_dict(), R.omd32(R.decay_at(t, 0.9999, True)))
    assert eng.ema_updates == 3
    live = _cpu(eng.state_dict())
    _same_dict(eng.ema_state_dict(), want, "three updates folded by the restatement")
    assert any(not torch.equal(want[k], live[k]) for k in want if k.endswith(".running_mean"))
    assert any(not torch.equal(want[k], live[k]) for k in want if k.endswith(".weight"))
    before, nbt_before = _live_bits(eng)

    with eng.ema_weights() as inside:
        assert inside is eng and eng.ema_swapped
        z = eng.forward(x, training=False).clone()
        fresh = make(99)
        fresh.load_state_dict(want)
        z2 = fresh.forward(x, training=False).clone()
        assert torch.isfinite(z).all()
        _same(z, z2, "eval logits of the swapped-in average vs an engine that loaded it")
        _same_dict(_cpu(net.state_dict()), want, "the facade shows the averaged values")
        _same_dict(eng.ema_state_dict(), want, "ema_state_dict while swapped")
        _same_dict(eng.state_dict(), want, "state_dict while swapped")
        _same(eng.store.bf16, R.mirror(eng.store.flat.cpu()), "the mirror of the swapped-in arena")
        for call in (lambda: eng.sgd_step(0.1), lambda: eng.lars_step(0.1), eng.ema_update):
            with pytest.raises(RuntimeError, match="swapped in"):
                call()
    assert not eng.ema_swapped and eng.ema_updates == 3
    after, nbt_after = _live_bits(eng)
    assert nbt_after == nbt_before
    for a, b in zip(after, before):
        _same(a, b, "flat / bf16 / running statistics after the context")
    _same_dict(eng.ema_state_dict(), want, "the average after the context")
    z_live = eng.forward(x, training=False).clone()
    assert not torch.equal(z_live, z)

    with pytest.raises(ZeroDivisionError):           # swapped back on exceptions too
        with eng.ema_weights():
            1 / 0
    assert not eng.ema_swapped
    for a, b in zip(_live_bits(eng)[0], before):
        _same(a, b, "after a context that raised")

    # the twin never swapped: the next step's loss has the same bits
    la, lb = train_step(eng, crit, x, y, lr=0.05), train_step(twin, crit, x, y, lr=0.05)
    assert math.isfinite(la.item()) and _bits(la).item() == _bits(lb).item()
    _same(eng.store.flat, twin.store.flat, "weights after the next step")

    # load_ema_state_dict on either side; ema_enable again starts over
    eng.load_ema_state_dict(live)
    _same_dict(eng.ema_state_dict(), live, "load_ema_state_dict, average in the shadow")
    eng.ema_swap()
    eng.load_ema_state_dict(want)
    _same_dict(eng.ema_state_dict(), want, "load_ema_state_dict, average in the arena")
    with pytest.raises(RuntimeError, match="swap back"):
        eng.ema_enable()
    eng.ema_swap()
    _same_dict(eng.ema_state_dict(), want, "swapped back")
    _same(eng.store.flat, twin.store.flat, "the live weights came back")
    eng.ema_enable(0.5, warmup=False)
    assert eng.ema_updates == 0
    _same_dict(eng.ema_state_dict(), _cpu(eng.state_dict()), "ema_enable again re-initialises")


# ------------------------------------------------------------------------------------------------ 5. other engines
@pytest.mark.parametrize("arch", ["ResNet18", "efficientnet_b0"])
def test_other_engines_swap_round_trip(arch):
    if arch == "ResNet18":
        eng = ResNetEngine(num_classes=10, num_blocks=(2, 2, 2, 2), device=DEV, seed=1)
        crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
        x, y = _batch(32, 32, 10, 8)
    else:
        from nbdt.engine_effnet import EfficientNetEngine
        eng = EfficientNetEngine(num_classes=1000, dropout_rate=0.0, device=DEV, seed=1)
        crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")
        x, y = _batch(32, 64, 1000, 9)
    eng.ema_enable(0.99, warmup=False)
    start = _cpu(eng.state_dict())
    loss = train_step(eng, crit, x, y, lr=0.2)
    eng.ema_update()
    assert math.isfinite(loss.item()) and eng.ema_updates == 1
    live = _cpu(eng.state_dict())
    avg = _cpu(eng.ema_state_dict())
    _same_dict(avg, R.fold_(start, live, R.omd32(0.99)), "one update without warm-up")
    assert sorted(avg) == sorted(live)
    assert any(not torch.equal(avg[k], live[k]) for k in live if live[k].is_floating_point())
    eng.ema_swap()
    assert eng.ema_swapped
    _same_dict(_cpu(eng.state_dict()), avg, "swapped: the arena holds the average")
    z = eng.forward(x, training=False)
    assert torch.isfinite(z).all()
    eng.ema_swap()
    assert not eng.ema_swapped
    _same_dict(_cpu(eng.state_dict()), live, "the swap round trip is the identity")
    _same_dict(_cpu(eng.ema_state_dict()), avg, "... on the average too")
    _same(eng.store.bf16, R.mirror(eng.store.flat.cpu()), "the mirror after the round trip")


# ------------------------------------------------------------------------------------------------ 6. driver
def test_driver_trains_saves_and_evaluates_the_average(tmp_path, monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nbdt_main_ema", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    base = "--arch ResNet18 --synthetic 256 --epochs 1 --batch-size 128 --deterministic".split()
    acc, _ = M.main(base + "--ema-decay 0.99".split())
    out = capsys.readouterr().out
    path = "./checkpoint/ckpt-CIFAR10-ResNet18-ema.pth"
    assert f"Checkpoints will be saved to: {path}" in out
    logged = re.findall(r"^EMA Accuracy: ([0-9.]+) \| EMA Loss: ([-0-9.a-z]+) \| (\d+) updates$", out, flags=re.M)
    assert len(logged) == 1 and logged[0][2] == "2" and math.isfinite(float(logged[0][1])), out
    assert re.findall(r"^Accuracy: ([0-9.]+) \| Best Accuracy: 0.0$", out, flags=re.M) == [repr(acc)]
    ckpt = torch.load(path, map_location="cpu")
    assert {"net", "acc", "epoch", "net_ema", "acc_ema", "ema_updates"} <= set(ckpt)
    assert ckpt["ema_updates"] == 2 and ckpt["acc"] == acc and repr(ckpt["acc_ema"]) == logged[0][0]
    assert sorted(ckpt["net_ema"]) == sorted(ckpt["net"])
    assert any(not torch.equal(ckpt["net_ema"][k], ckpt["net"][k]) for k in ckpt["net"])
    # the averaged weights alone, from the checkpoint: the same accuracy, exactly
    acc2, _ = M.main(base + "--eval --resume --use-ema".split())
    out = capsys.readouterr().out
    assert acc2 == ckpt["acc_ema"], (acc2, ckpt["acc_ema"])
    assert "EMA Accuracy" not in out
    # ... the live ones without --use-ema (the -ema name comes from --ema-decay; the restored average is evaluated too)
    acc3, _ = M.main(base + "--eval --resume --ema-decay 0.99".split())
    out = capsys.readouterr().out
    assert acc3 == acc and "Averaged weights restored after 2 updates" in out
    assert re.findall(r"^EMA Accuracy: ([0-9.]+) ", out, flags=re.M) == [repr(ckpt["acc_ema"])]
    # a checkpoint without an average is refused with a clear message
    torch.save({"net": ckpt["net"], "acc": acc, "epoch": 0}, path)
    with pytest.raises(SystemExit, match="holds no averaged weights"):
        M.main(base + "--eval --resume --use-ema".split())
