"""Global-norm clipping (csrc/clip.hip) and gradient accumulation (train_step micro_batches=) on the GPU: the kernels
against the numpy restatement of include/nbdt_hip.h (tests/_clip_ref.py) -- bit for bit where every sum is exact, to the
one fp32 ulp of the cast elsewhere --, then the engines, two ranks and the driver."""
import ctypes
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
from nbdt import engine as E  # noqa: E402
from nbdt.engine import AdamWConfig, ClipConfig, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

import _clip_ref as C  # noqa: E402

DEV = "cuda:0"
SENTINEL = 7.25
PAD = 20                      # sentinels behind the arena: a multiple of 4, so a 16-byte store past n would hit them


def _arena(values):
    """(the whole buffer, its first n elements as the arena): sentinels from n on."""
    n = values.numel()
    buf = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:n] = values.to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:n]


def _integers(n, seed):
    g = torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(seed)).float()
    g[0] = 3.0                # never the zero vector
    return g


def _record_bits(rec):
    return (int(C.bits(rec["norm"])), int(C.bits(rec["coef"])), rec["clipped"], rec["steps"], rec["nonfinite"],
            rec["total_clipped"])


def _check_sentinels(buf, n):
    assert torch.equal(buf[n:].cpu(), torch.full((PAD,), SENTINEL)), "written beyond n"


@pytest.fixture
def deterministic():
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ 1. exact fixtures
@pytest.mark.parametrize("n", [4, 8, 252, 256, 260, 4100, 65540, 1_000_004])
def test_exact_fixtures_are_the_restatement_bit_for_bit(n):
    """Integers in [-8, 8]: every square, every partial sum and S itself (<= 64 n < 2^53) are exact in fp64 in any order,
    so norm, coef, the record and the clipped gradient must be the restatement's bits.  Three steps on one plan, each on
    the integers again: one that clips, one under a bound that does not, one that clips with a negative grad_scale; the
    counters carry over."""
    g0 = _integers(n, n)
    buf, g = _arena(g0)
    plan = ops.ClipPlan(n, DEV)
    assert _record_bits(plan.to_host()) == _record_bits(C.new_record())
    ref = C.new_record()
    for grad_scale, max_norm in ((1.0, 1.0), (0.5, 1.0e6), (-0.25, 0.375)):
        g.copy_(g0)
        want, ref = C.clip(g0.numpy(), grad_scale, max_norm, ref)
        plan.norm(g, grad_scale, max_norm)
        plan.apply(g)
        got = plan.to_host()
        assert _record_bits(got) == _record_bits(ref), (got, ref)
        assert np.array_equal(C.bits(g.cpu().numpy()), C.bits(want))
        _check_sentinels(buf, n)
    assert (ref["clipped"], ref["steps"], ref["total_clipped"], ref["nonfinite"]) == (1, 3, 2, 0)
    view = plan.record()
    assert view.is_cuda and view.dtype == torch.int32 and view.numel() == 8
    words = view.cpu().numpy()
    assert (int(words[:1].view(np.uint32)[0]), int(words[1:2].view(np.uint32)[0])) == _record_bits(ref)[:2]
    assert tuple(int(w) for w in words[2:6]) == _record_bits(ref)[2:]


def test_the_c_entry_takes_a_length_that_is_no_multiple_of_four():
    """n = 4099: three elements in the scalar tail, read for the norm, scaled by apply, and nothing behind them touched."""
    lib = _C.lib()
    n = 4099
    g0 = _integers(n, 99)
    g0[-3:] = torch.tensor([8.0, -8.0, 8.0])                              # the tail carries weight in the norm
    buf, g = _arena(torch.cat([g0, torch.full((1,), SENTINEL)]))          # (keep PAD sentinels + 1 behind n)
    handle = ctypes.c_void_p()
    with torch.cuda.device(DEV):
        _C.check(lib.nbdt_clip_create(n, ctypes.byref(handle)))
        try:
            st = ops.stream_ptr(torch.device(DEV))
            _C.check(lib.nbdt_clip_norm(handle, _C.ptr(g), 1.0, 2.0, st))
            _C.check(lib.nbdt_clip_apply(handle, _C.ptr(g), st))
            out = ops.ClipRecord()
            _C.check(lib.nbdt_clip_record_to_host(handle, ctypes.byref(out), st))
        finally:
            lib.nbdt_clip_destroy(handle)
    want, ref = C.clip(g0.numpy(), 1.0, 2.0)
    assert ref["clipped"] == 1
    assert C.norm_of(g0.numpy()[:4096]) != ref["norm"]                    # the tail shows in the norm
    assert (int(C.bits(out.norm)), int(C.bits(out.coef)), out.clipped, out.steps) == _record_bits(ref)[:4]
    assert np.array_equal(C.bits(buf[:n].cpu().numpy()), C.bits(want))
    assert torch.equal(buf[n:].cpu(), torch.full((PAD + 1,), SENTINEL))


# ------------------------------------------------------------------------------------------------ 2. random data
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_data_norm_within_one_ulp_and_the_rest_exact(seed):
    """The kernel's S and numpy's differ by summation order only: relative error <= n 2^-53 each, ~1e-10 for a million
    elements, far below 2^-24 -- so (float)S lands on the same float or, when S sits next to a rounding boundary, on its
    neighbour; sqrtf is correctly rounded and monotone, the multiply by |grad_scale| too: at most 1 ulp in norm.  From
    the kernel's own norm on, everything is exact fp32 arithmetic: coef and g * coef must be the restatement's bits."""
    n = 1_000_004
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.01
    buf, g = _arena(g0)
    plan = ops.ClipPlan(n, DEV)
    grad_scale, max_norm = 0.5, 1.0
    plan.norm(g, grad_scale, max_norm)
    plan.apply(g)
    got = plan.to_host()
    want_norm = C.norm_of(g0.numpy(), grad_scale)
    d = C.ulp_distance(got["norm"], want_norm)
    print(f"seed {seed}: norm {got['norm']!r} vs restatement {float(want_norm)!r}: {d} ulp")
    assert d <= 1 and float(want_norm) > 2.0                             # ~ 0.5 x 0.01 x 1000 = 5: it clips
    ref = C.new_record()
    coef = C.fold(np.float32(got["norm"]), max_norm, ref)
    assert _record_bits(got) == _record_bits(ref) and ref["clipped"] == 1
    assert np.array_equal(C.bits(g.cpu().numpy()), C.bits(C.apply(g0.numpy(), coef)))
    _check_sentinels(buf, n)


# ------------------------------------------------------------------------------------------------ 3. not clipped
def test_a_norm_below_the_bound_leaves_every_bit():
    n = 65540
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    buf, g = _arena(g0)
    plan = ops.ClipPlan(n, DEV)
    for step in (1, 2, 3):
        plan.norm(g, 1.0, 1.0e4)
        plan.apply(g)
        got = plan.to_host()
        assert got["coef"] == 1.0 and got["clipped"] == 0 and got["steps"] == step and got["total_clipped"] == 0
        assert C.ulp_distance(got["norm"], C.norm_of(g0.numpy())) <= 1 and got["norm"] < 1.0e4
    assert np.array_equal(C.bits(g.cpu().numpy()), C.bits(g0.numpy()))
    _check_sentinels(buf, n)


# ------------------------------------------------------------------------------------------------ 4. non-finite input
@pytest.mark.parametrize("where,bad", [(12345, float("inf")), (-1, float("nan"))])
def test_non_finite_gradients_are_counted_and_left_alone(where, bad):
    n = 65540
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(6))
    g0[where] = bad
    buf, g = _arena(g0)
    plan = ops.ClipPlan(n, DEV)
    plan.norm(g, 1.0, 1.0)
    plan.apply(g)
    got = plan.to_host()
    assert not math.isfinite(got["norm"]) and got["coef"] == 1.0
    assert (got["clipped"], got["steps"], got["nonfinite"], got["total_clipped"]) == (0, 1, 1, 0)
    assert np.array_equal(C.bits(g.cpu().numpy()), C.bits(g0.numpy()))
    g[where] = 1.0                                                         # the next, finite step clips and counts on
    plan.norm(g, 1.0, 1.0)
    got = plan.to_host()
    assert math.isfinite(got["norm"]) and (got["clipped"], got["steps"], got["nonfinite"], got["total_clipped"]) == (1, 2, 1, 1)
    _check_sentinels(buf, n)


# ------------------------------------------------------------------------------------------------ 5. determinism, refusals
def test_the_record_does_not_depend_on_deterministic_mode_and_the_python_layer_refuses():
    n = 1_000_004
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    _, g = _arena(g0)
    was = ops.is_deterministic()
    seen = []
    try:
        for on in (True, False, True):
            ops.set_deterministic(on)
            plan = ops.ClipPlan(n, DEV)
            for _ in range(2):
                plan.norm(g, 1.0, 1.0e6)                                   # (never clips: g stays the input)
            seen.append(_record_bits(plan.to_host()))
    finally:
        ops.set_deterministic(was)
    assert seen[0] == seen[1] == seen[2] and seen[0][3] == 2
    plan = ops.ClipPlan(64, DEV)
    ok = torch.zeros(64, device=DEV)
    for bad, what in [(torch.zeros(68, device=DEV), "64 elements"), (torch.zeros(60, device=DEV), "64 elements"),
                      (torch.zeros(64, device=DEV, dtype=torch.float64), "fp32"),
                      (torch.zeros(64, device=DEV, dtype=torch.bfloat16), "fp32"),
                      (torch.zeros(128, device=DEV)[::2], "contiguous"), (torch.zeros(64), "no CPU fallback")]:
        with pytest.raises(_C.NBDTHipError, match=what):
            plan.norm(bad, 1.0, 1.0)
        with pytest.raises(_C.NBDTHipError, match=what):
            plan.apply(bad)
    for gs, m, what in [(1.0, 0.0, "max_norm"), (1.0, float("nan"), "max_norm"), (float("inf"), 1.0, "grad_scale")]:
        with pytest.raises(_C.NBDTHipError, match=what):
            plan.norm(ok, gs, m)
    assert plan.to_host()["steps"] == 0                                   # nothing above was launched


# ------------------------------------------------------------------------------------------------ 6.-8. engines
def _batch(B, size, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g).to(DEV), torch.randint(0, classes, (B,), generator=g).to(DEV)


def _wrn(seed=3):
    return WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=seed)


def _cifar_crit():
    return SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")


def _by_hand(eng, crit, x, y):
    """zero_grad + forward + loss + backward exactly as train_step issues them for one chunk; the gradient stays."""
    eng.zero_grad()
    loss = E._loss_backward(eng, crit, x, y, None, True)
    eng.join_side_stream()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    return loss


def test_wrn_step_with_clipping_equals_the_step_driven_by_hand(deterministic):
    crit = _cifar_crit()
    x, y = _batch(16, 32, 10, 11)
    lr = 0.05
    a, b = _wrn(), _wrn()
    assert torch.equal(a.store.flat, b.store.flat)
    # a first, unclipped step's report gives the bound: half of the gradient norm
    probe = _wrn()
    train_step(probe, crit, x, y, lr, zero_grad=False, clip=ClipConfig(1.0e6))
    first = probe.clip_stats()
    assert first["clipped"] == 0 and first["coef"] == 1.0 and first["steps"] == 1 and first["norm"] > 0.0
    # ... which is the norm over the LOGICAL gradients: the arena's padding and gaps hold +0
    logical = np.concatenate([v.detach().float().cpu().numpy().ravel() for v in probe.named_params("grad").values()])
    assert logical.size < probe.store.grad.numel()
    d = C.ulp_distance(first["norm"], C.norm_of(logical))
    print(f"norm {first['norm']!r}, restatement over {logical.size} logical elements {float(C.norm_of(logical))!r}: {d} ulp")
    assert d <= 1
    m = 0.5 * first["norm"]
    loss_a = train_step(a, crit, x, y, lr, zero_grad=False, clip=ClipConfig(m))
    stats = a.clip_stats()
    assert stats["clipped"] == 1 and stats["norm"] == first["norm"]       # same seed, deterministic mode: the same bits
    ref = C.new_record()
    coef_ref = C.fold(np.float32(stats["norm"]), m, ref)
    assert float(coef_ref) == stats["coef"] and 0.49 < stats["coef"] < 0.51
    loss_b = _by_hand(b, crit, x, y)
    b.store.grad.mul_(float(coef_ref))
    b.sgd_step(lr, zero_grad=False)
    torch.cuda.synchronize()
    assert loss_a.item() == loss_b.item()
    pa, pb = a.named_params("flat"), b.named_params("flat")
    for name in pa:
        assert torch.equal(pa[name], pb[name]), name
    assert torch.equal(a.store.flat, b.store.flat) and torch.equal(a.store.grad, b.store.grad)
    assert torch.equal(a.store.mom, b.store.mom) and not torch.equal(a.store.flat, probe.store.flat)


def _accumulation_case(make, crit, x, y, reference_fp32):
    """micro_batches=2 on engine B against two single-chunk passes on the identically seeded engine A."""
    lr, K = 0.05, 2
    a, b = make(), make()
    for e in (a, b):
        if reference_fp32:
            e.set_reference_fp32(True)
    xs, ys = x.chunk(K), y.chunk(K)
    parts = []
    for xc, yc in zip(xs, ys):                                            # the same weights: no optimizer step between
        _by_hand(a, crit, xc, yc)
        parts.append({k: v.detach().double().cpu() for k, v in a.named_params("grad").items()})
    loss = train_step(b, crit, x, y, lr, zero_grad=False, micro_batches=K)
    b.join_side_stream()
    torch.cuda.synchronize()
    acc = {k: v.detach().double().cpu() for k, v in b.named_params("grad").items()}
    worst = 0.0
    for name, got in acc.items():
        want = parts[0][name] + parts[1][name]
        scale = want.abs().max().item()
        err = (got - want).abs().max().item()
        if scale > 0.0:
            worst = max(worst, err / scale)
        assert err <= 1e-6 * scale, (name, err, scale)
    print(f"accumulated gradient vs g1 + g2 in float64: worst max|diff| / max|g1 + g2| over {len(acc)} tensors {worst:.3e}")
    assert math.isfinite(loss.item())
    # each chunk normalised with its own statistics and moved the running ones once: two updates, A's two passes' bits
    for bn_a, bn_b in zip(a.bns, b.bns):
        assert bn_b.num_batches_tracked == 2 == bn_a.num_batches_tracked
        assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)
    # the applied update is sgd_step(grad_scale = 1 / K) on that gradient
    a.store.grad.copy_(b.store.grad)
    a.sgd_step(lr, grad_scale=1.0 / K, zero_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(a.store.flat, b.store.flat) and torch.equal(a.store.mom, b.store.mom)
    assert torch.equal(b.store.bf16.cpu(), b.store.flat.cpu().to(torch.bfloat16))
    return worst


@pytest.mark.parametrize("reference_fp32", [True, False], ids=["fp32-reference", "bf16"])
def test_wrn_accumulates_two_micro_batches(deterministic, reference_fp32):
    x, y = _batch(16, 32, 10, 12)
    _accumulation_case(_wrn, _cifar_crit(), x, y, reference_fp32)


@pytest.mark.parametrize("reference_fp32", [True, False], ids=["fp32-reference", "bf16"])
def test_efficientnet_accumulates_two_micro_batches(deterministic, reference_fp32):
    """Its backward re-zeroes the squeeze-and-excitation sum buffers per call and adds (+=) into every parameter gradient."""
    from nbdt.engine_effnet import EfficientNetEngine
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    x, y = _batch(16, 32, 10, 13)
    _accumulation_case(lambda: EfficientNetEngine(num_classes=10, dropout_rate=0.0, device=DEV, seed=4), crit, x, y,
                       reference_fp32)


# ------------------------------------------------------------------------------------------------ 9. two ranks
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _clip_dp_worker(rank, world, port, out_dir, backend, devices):
    import nbdt_path as npth
    npth.add()
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(devices[rank]),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist
    from nbdt import dist as nd
    from nbdt.engine import AdamWConfig as Adam, ClipConfig as Clip, WRNEngine as Eng, train_step as step
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
    eng = Eng(num_classes=10, blocks=10, width_factor=2, device=dev, seed=5)
    losses, ranges = [], []
    for _ in range(3):
        losses.append(step(eng, crit, x, y, lr=1e-3, comm=comm, micro_batches=2, clip=Clip(0.5), optim=Adam()).item())
        ranges.append([tuple(r) for r in comm.last_ranges])
    torch.cuda.synchronize()
    out = {"flat": eng.store.flat.cpu(), "mom": eng.store.mom.cpu(), "sq": eng.store.sq.cpu(), "losses": losses,
           "clip": eng.clip_stats(), "ranges": ranges, "buckets": [tuple(b) for b in eng.grad_buckets()],
           "t": eng.opt_steps}
    torch.save(out, os.path.join(out_dir, f"clip{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_stay_bit_identical_with_accumulation_and_clipping(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_clip_dp_worker, args=(world, _free_port(), str(tmp_path), "nccl", [0, 1]), nprocs=world, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), f"clip{r}.pt")) for r in range(world))
    for key in ("flat", "mom", "sq"):
        assert torch.equal(a[key], b[key]), key
    assert _record_bits(a["clip"]) == _record_bits(b["clip"]) and a["clip"]["steps"] == 3
    assert a["t"] == b["t"] == 3 and all(math.isfinite(l) for l in a["losses"] + b["losses"])
    for r in (a, b):                              # one set of buckets per optimizer step, although two backward passes ran
        nonempty = [x for x in r["buckets"] if x[1] > x[0]]
        for step_ranges in r["ranges"]:
            assert sorted(step_ranges) == sorted(nonempty), (step_ranges, nonempty)


# ------------------------------------------------------------------------------------------------ 10. driver
def test_driver_accumulates_and_clips(tmp_path, monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nbdt_main_clip", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    M.main("--arch ResNet18 --synthetic 512 --epochs 2 --batch-size 128 --accum-steps 2 --clip-grad-norm 1.0".split())
    out = capsys.readouterr().out
    assert "Checkpoints will be saved to: ./checkpoint/ckpt-CIFAR10-ResNet18-acc2-clip1.0.pth" in out
    v = [float(s) for s in re.findall(r"^Loss: ([-0-9.a-z]+) \(", out, flags=re.M)]
    assert len(v) == 2 and all(math.isfinite(s) for s in v), out
    assert [int(m) for m in re.findall(r"\((\d+) steps of 1 x 128 images", out)] == [4, 4]
    clip = re.findall(r"^Clip: last norm ([-0-9.a-z+]+), clipped (\d+) of (\d+) steps \(max norm 1\), (\d+) non-finite", out,
                      flags=re.M)
    assert len(clip) == 2, out
    assert [int(c[2]) for c in clip] == [4, 8] and all(math.isfinite(float(c[0])) for c in clip)
    assert all(int(c[3]) == 0 for c in clip) and int(clip[1][1]) <= 8
    with pytest.raises(SystemExit, match="--accum-steps"):
        M.main("--arch ResNet18 --synthetic 512 --epochs 1 --batch-size 128 --accum-steps 3".split())
