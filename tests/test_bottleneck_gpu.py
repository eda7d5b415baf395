"""BottleneckEngine (ResNet50 / 101 / 152 of the reference's nbdt/models/resnet.py:77-112, 193-223) on the MI355X against
the fp32 restatement tests/_bottleneck_ref.py, which tests/test_bottleneck.py pins to the reference's own ResNet50.

  * fp32 reference mode: the engine's own forward() / backward() on fp32 storage equals the oracle to the tolerances
    tests/test_reference_fp32_gpu.py holds ResNet18 to -- the orchestration (launch order, two streams, rotating
    buffers, accumulate-after-plain shortcut gradient) is right;
  * bf16 product path: the pointwise GEMM kernel (engine.pointwise = True) is no further from the oracle than the
    first-generation kernel on the same launches (pointwise = False: storage precision alone);
  * determinism, training, eval, state dict, the main.py driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_oracle as O
import nbdt_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bottleneck_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt import engine as E  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
DATASET, HIERARCHY = "CIFAR10", "induced-ResNet18"
# tests/test_reference_fp32_gpu.py: relative L2 per parameter gradient; a ReLU tie moves one to TOL_TIE, so every batch
# meets TOL_TIE and at least one of the SEEDS batches meets TOL
TOL, TOL_TIE, SEEDS = 1e-3, 2e-2, (21, 22, 23, 24)
SMALL = (1, 1, 1, 1)


def _rel_l2(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _crit():
    return SoftTreeSupLoss(dataset=DATASET, criterion=nn.CrossEntropyLoss(), hierarchy=HIERARCHY)


def _oracle_step(ref, otree, x, y):
    ref.train()
    ref.zero_grad()
    z = ref(x)
    loss, dz = O.soft_tree_sup_loss(otree, z.detach().numpy(), y.numpy())
    z.backward(torch.from_numpy(dz))
    return z.detach(), float(loss), {n: p.grad.clone() for n, p in ref.named_parameters()}


def _engine_step(eng, crit, x, y):
    eng.zero_grad()
    z = eng.forward(x.to(DEV), training=True)
    loss, gz = crit.loss_and_grad(z, y.to(DEV))
    eng.backward(gz)
    torch.cuda.synchronize()
    return z.float().cpu(), loss.item(), {k: v.clone() for k, v in eng.named_params("grad").items()}


def _batch(seed, B=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B,), generator=g)


@pytest.fixture(scope="module")
def otree(pkg_dir):
    return O.OracleTree(*O.default_paths(DATASET, HIERARCHY, pkg_dir))


@pytest.fixture(scope="module")
def resnet50(otree):
    """The full ResNet50 at 8 images: engine, oracle with the same weights, one batch and the oracle's step on it."""
    torch.manual_seed(0)
    ref = R.ResNet50(10)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    eng = E.BottleneckEngine(num_classes=10, device=DEV, seed=0)
    eng.load_state_dict(init)
    x, y = _batch(31)
    z_ref, loss_ref, g_ref = _oracle_step(ref, otree, x, y)
    return dict(eng=eng, init=init, x=x, y=y, z_ref=z_ref, loss_ref=loss_ref, g_ref=g_ref)


def test_fp32_reference_mode_equals_the_oracle(otree):
    crit = _crit()
    torch.manual_seed(3)
    init = {k: v.clone() for k, v in R.BottleneckResNet(SMALL, 10).state_dict().items()}
    eng = E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=0)
    assert eng.pointwise and eng._side is not None and eng._overlap and eng.res_share is None
    eng.set_reference_fp32(True)
    assert eng.act_dtype == torch.float32
    worst_by_seed = []
    for seed in SEEDS:
        ref = R.BottleneckResNet(SMALL, 10)
        ref.load_state_dict(init)
        eng.load_state_dict(init)
        x, y = _batch(seed)
        z_ref, loss_ref, g_ref = _oracle_step(ref, otree, x, y)
        z, loss, grads = _engine_step(eng, crit, x, y)
        scale = z_ref.abs().max().item()
        assert (z - z_ref).abs().max().item() < 1e-4 * scale
        assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref), (loss, loss_ref)
        assert set(grads) == set(g_ref)
        errs = sorted((_rel_l2(grads[n], g_ref[n]), n) for n in g_ref)
        print(f"[bottleneck {SMALL} fp32 / inputs {seed}] loss {loss:.6f} vs {loss_ref:.6f}; parameter-gradient rel-L2: "
              f"worst {errs[-1][0]:.2e} ({errs[-1][1]}), median {errs[len(errs) // 2][0]:.2e}")
        assert errs[-1][0] < TOL_TIE, errs[-1]
        sd, sd_ref = eng.state_dict(), ref.state_dict()
        for k in sd_ref:
            if k.endswith("running_var") or k.endswith("running_mean"):
                assert _rel_l2(sd[k], sd_ref[k]) < 1e-4, k
        worst_by_seed.append((errs[-1][0], seed))
    assert min(worst_by_seed)[0] < TOL, worst_by_seed


def _leg(r, pointwise, otree):
    eng = r["eng"]
    eng.pointwise = pointwise
    eng.load_state_dict(r["init"])
    kernels = set()
    real_pw, real_ig = ops.conv_pw, ops.conv_igemm

    def spy_pw(*a, **k):
        real_pw(*a, **k)
        kernels.add(ops.last_igemm_kernel())

    def spy_ig(*a, **k):
        real_ig(*a, **k)
        kernels.add(ops.last_igemm_kernel())

    ops.conv_pw, ops.conv_igemm = spy_pw, spy_ig
    try:
        z, loss, grads = _engine_step(eng, _crit(), r["x"], r["y"])
    finally:
        ops.conv_pw, ops.conv_igemm = real_pw, real_ig
        eng.pointwise = True
    assert ("conv_pw_kernel" in kernels) == pointwise, kernels
    g_ref = r["g_ref"]
    gmax = max(v.norm().item() for v in g_ref.values())
    live = [n for n in g_ref if g_ref[n].norm().item() > 1e-6 * gmax]      # (the cosine of a zero vector says nothing)
    cos = min((_cos(grads[n], g_ref[n]), n) for n in live)
    cos_big = min((_cos(grads[n], g_ref[n]), n) for n in live if g_ref[n].numel() >= 4096)      # (reported, not asserted)
    tree = Tree(DATASET, hierarchy=HIERARCHY)
    hard = _C.hard_forward(tree.device_handle(0), z.to(DEV), want_onehot=False)[0].cpu().numpy()
    return dict(loss=loss, logit_err=(z - r["z_ref"]).abs().max().item() / r["z_ref"].abs().max().item(), cos=cos,
                cos_big=cos_big,
                hard_ok=bool(np.array_equal(hard, O.hard_forward(otree, z.numpy()))))


def test_resnet50_bf16_step_pointwise_kernel_vs_first_generation_kernel(resnet50, otree):
    """One training step of the full ResNet50 (53 convolutions, 8 images, random initialisation) in bf16 storage against
    the fp32 oracle, with the stride-1 1x1 convolutions on nbdt_conv_pw (`pointwise`) and on nbdt_conv_igemm (the parent's
    kernels: storage precision alone).  Nobody had measured a 50-layer net here, so the bar is relative: the pointwise leg
    stays within 1.25 x the other leg's logit error (relative to the logit scale) and within 0.02 of its worst
    per-parameter gradient cosine -- the margin is the atomics-order noise of the BatchNorm sums
    (tests/test_baseline_configs_gpu.py explains why one step at random initialisation moves by about that much).

    Measured on an MI355X (the same figures on every run; neither leg moved from run to run):
        conv_igemm leg: logit error 0.2579 of the logit scale, worst cosine 0.0661 (layer2.1.bn2.bias),
                        worst over the tensors of >= 4096 elements 0.2396 (layer2.1.conv1.weight)
        conv_pw leg:    logit error 0.2579 of the logit scale, worst cosine 0.0661 (layer2.1.bn2.bias),
                        worst over the tensors of >= 4096 elements 0.2396 (layer2.1.conv1.weight)
    The two legs are the same to the last digit because the pointwise kernel leaves the same bits as nbdt_conv_igemm,
    statistics partial sums included (tests/test_conv_pw_gpu.py asserts torch.equal of both).  That is by design, and
    this figure is why: after 50 layers of bf16 storage at 8 images the gradients of the 64-channel BatchNorm shifts keep
    no direction against the fp32 oracle on EITHER kernel (cosine 0.07; the large tensors are at 0.24), and a first
    version of the kernel whose partial sums differed from nbdt_conv_igemm_stats' in the last bit (4e-7 relative: 8 waves
    x 32 pixels instead of 4 x 64) moved the worst cosine to -0.036 and the logit error to 0.2941 -- a step of this net
    at random initialisation amplifies one ulp of a BatchNorm mean to an uncorrelated small gradient.  Absolute
    agreement with the oracle is what test_fp32_reference_mode_equals_the_oracle holds (3e-6 in fp32 storage)."""
    a = _leg(resnet50, False, otree)
    b = _leg(resnet50, True, otree)
    for tag, m in (("conv_igemm", a), ("conv_pw", b)):
        print(f"[ResNet50 bf16 / {tag}] loss {m['loss']:.5f} (oracle {resnet50['loss_ref']:.5f}); logit error "
              f"{m['logit_err']:.4f} of scale; worst gradient cosine {m['cos'][0]:.4f} ({m['cos'][1]}); worst over the "
              f"tensors of >= 4096 elements {m['cos_big'][0]:.4f} ({m['cos_big'][1]})")
    assert np.isfinite(a["loss"]) and np.isfinite(b["loss"])
    assert a["hard_ok"] and b["hard_ok"]          # HardNBDT decisions: HIP kernel == the oracle's rules on the SAME logits
    assert b["logit_err"] <= 1.25 * a["logit_err"], (a["logit_err"], b["logit_err"])
    assert b["cos"][0] >= a["cos"][0] - 0.02, (a["cos"], b["cos"])


def test_which_kernel_each_pointwise_launch_takes():
    """Conv's routing, launch by launch, over one training step: a stride-1 1x1 launch goes to nbdt_conv_pw unless it is
    a statistics launch (the training forward) with fewer than Conv.PW_STATS_MIN_CIN = 1024 input channels, which stays
    on nbdt_conv_igemm; nothing else reaches nbdt_conv_pw.  With pointwise off nothing does."""
    eng = E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=0)
    assert E.Conv.PW_STATS_MIN_CIN == 1024
    seen = []
    real_pw, real_ig = ops.conv_pw, ops.conv_igemm

    def spy(real):
        def f(desc, inp, w, out, *a, **k):
            real(desc, inp, w, out, *a, **k)
            stats = k.get("bn_scratch") is not None or any(isinstance(t, torch.Tensor) and t.dtype == torch.float32 for t in a)
            dense1x1 = desc.ntaps == 1 and desc.in_ws == desc.cin and desc.out_ws == desc.cout
            seen.append((ops.last_igemm_kernel(), desc.cin, desc.cout, stats, bool(desc.accumulate), dense1x1))
        return f

    ops.conv_pw, ops.conv_igemm = spy(real_pw), spy(real_ig)
    try:
        x, y = _batch(9)
        _engine_step(eng, _crit(), x, y)
        on = list(seen)
        del seen[:]
        eng.pointwise = False
        _engine_step(eng, _crit(), x, y)
        off = list(seen)
    finally:
        ops.conv_pw, ops.conv_igemm = real_pw, real_ig
    assert all(k != "conv_pw_kernel" for k, *_ in off)
    for kernel, cin, cout, stats, acc, dense1x1 in on:
        want_pw = dense1x1 and not (stats and cin < 1024)
        assert (kernel == "conv_pw_kernel") == want_pw, (kernel, cin, cout, stats, acc, dense1x1)
    fwd = {(cin, k) for k, cin, _, stats, _, d in on if d and stats}
    assert (1024, "conv_pw_kernel") in fwd and (512, "conv_igemm_dma_kernel") in fwd and (64, "conv_igemm_dma_kernel") in fwd
    dgrad = [(k, acc) for k, _, _, stats, acc, d in on if d and not stats]
    assert len(dgrad) == 9 and all(k == "conv_pw_kernel" for k, _ in dgrad)      # conv1 + conv3 of 4 blocks, layer1.0's shortcut
    assert sum(acc for _, acc in dgrad) == 1                                     # ... the shortcut's, accumulating


def test_two_stream_step_equals_one_stream_step_bit_for_bit(resnet50):
    """Deterministic mode: the step is a pure function of weights and inputs, so the two-stream schedule (weight gradients
    on the second stream, gradient buffers alternating between consecutive blocks) must reproduce the one-stream
    schedule's loss and every gradient exactly -- a weight gradient that read a buffer the next block had already
    overwritten would not."""
    eng, crit = resnet50["eng"], _crit()
    ops.set_deterministic(True)
    try:
        out = []
        for overlap in (True, False):
            eng.set_overlap(overlap)
            eng.load_state_dict(resnet50["init"])
            out.append(_engine_step(eng, crit, resnet50["x"], resnet50["y"]))
    finally:
        ops.set_deterministic(False)
        eng.set_overlap(True)
    (z2, l2, g2), (z1, l1, g1) = out
    assert l2 == l1 and torch.equal(z2, z1)
    for n in g1:
        assert torch.equal(g2[n], g1[n]), n


def test_three_train_steps_lower_the_loss():
    eng = E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=0)
    crit = _crit()
    x, y = _batch(5)
    x, y = x.to(DEV), y.to(DEV)
    losses = [E.train_step(eng, crit, x, y, lr=0.05).item() for _ in range(3)]
    final = crit.loss_and_grad(eng.forward(x, training=True), y)[0].item()
    print(f"[bottleneck {SMALL}] losses {losses} -> {final:.4f}")
    assert all(np.isfinite(losses)) and final < losses[0]


def test_eval_logits_and_state_dict_round_trip():
    torch.manual_seed(0)
    ref = R.BottleneckResNet(SMALL, 10)
    eng = E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=1)
    eng.load_state_dict(ref.state_dict())
    x, _ = _batch(7, B=32)
    ref.train()
    with torch.no_grad():
        ref(x)                                   # move the running statistics off their initial values, both sides
    eng.forward(x.to(DEV), training=True)
    ref.eval()
    assert eng.fuse_eval
    calls = []
    real = ops.conv_igemm_affine
    ops.conv_igemm_affine = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        z = eng.forward(x.to(DEV), training=False).float().cpu()
    finally:
        ops.conv_igemm_affine = real
    assert len(calls) == 4 * 4                   # conv1, conv2, shortcut, conv3 + residual: one launch each
    with torch.no_grad():
        z_ref = ref(x)
    # the ResNet18 eval bar of tests/test_models_gpu.py
    assert (z.argmax(1) == z_ref.argmax(1)).float().mean().item() >= 0.9
    assert (z - z_ref).abs().max().item() < 3e-2 * z_ref.abs().max().item()
    # engine -> restatement (strict) -> a fresh engine
    sd = {k: v.cpu() for k, v in eng.state_dict().items()}
    ref2 = R.BottleneckResNet(SMALL, 10)
    ref2.load_state_dict(sd, strict=True)
    eng2 = E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=2)
    eng2.load_state_dict(ref2.state_dict())
    sd2 = eng2.state_dict()
    assert set(sd2) == set(sd)
    for k in sd:
        assert torch.equal(sd2[k].cpu(), sd[k]), k
    assert torch.equal(eng2.forward(x.to(DEV), training=False), eng.forward(x.to(DEV), training=False))


def test_main_driver_trains_resnet50(tmp_path):
    main = os.path.join(nbdt_path.PKG_DIR, "main.py")
    out = subprocess.run([sys.executable, main] + "--arch ResNet50 --dataset CIFAR10 --synthetic 64 --batch-size 32 --epochs 1 "
                         "--hierarchy induced-ResNet18 --loss SoftTreeSupLoss".split(), cwd=tmp_path, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
