"""ImageNetResNetEngine / ImageNetBottleneckEngine (torchvision's resnet18 ... resnet152: 7x7 / 2 stem as a patch gather +
the 1x1 convolution, MaxPool2d(3, 2, 1) as its own op, ``fc``) on the MI355X against the fp32 restatement
tests/_imagenet_resnet_ref.py, with the yardsticks of tests/test_bottleneck_gpu.py:

  * fp32 reference mode equals the restatement at 128 x 128 (stages of 32 / 16 / 8 / 4 pixels: the CIFAR trunks' grids) and
    at 224 x 224 (56 / 28 / 14 / 7: the generic kernels) to the tolerances of tests/test_reference_fp32_gpu.py;
  * the bf16 product path at both sizes; determinism; training; the eval path; state dict; wrappers; the main.py driver."""
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
import _imagenet_resnet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from nbdt import _C, models, ops  # noqa: E402
from nbdt import engine as E  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402
from nbdt.model import HardNBDT, SoftNBDT  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
DATASET, HIERARCHY = "CIFAR10", "induced-ResNet18"
# tests/test_reference_fp32_gpu.py: relative L2 per parameter gradient; a ReLU tie moves one to TOL_TIE, so every batch
# meets TOL_TIE and at least one of the SEEDS batches meets TOL
TOL, TOL_TIE, SEEDS = 1e-3, 2e-2, (21, 22, 23, 24)
SMALL = (1, 1, 1, 1)
KINDS = {"basic": ("resnet18", E.ImageNetResNetEngine), "bottleneck": ("resnet50", E.ImageNetBottleneckEngine)}


def _rel_l2(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _crit():
    return SoftTreeSupLoss(dataset=DATASET, criterion=nn.CrossEntropyLoss(), hierarchy=HIERARCHY)


def _ref(kind, num_blocks=SMALL, classes=10):
    return R.make(KINDS[kind][0], classes, num_blocks=num_blocks)


def _eng(kind, num_blocks=SMALL, classes=10, seed=0, **kw):
    return KINDS[kind][1](num_classes=classes, num_blocks=num_blocks, device=DEV, seed=seed, **kw)


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


def _batch(seed, B, size):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, size, size, generator=g), torch.randint(0, 10, (B,), generator=g)


@pytest.fixture(scope="module")
def otree(pkg_dir):
    return O.OracleTree(*O.default_paths(DATASET, HIERARCHY, pkg_dir))


@pytest.mark.parametrize("B,size", [(4, 128), (2, 224)])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fp32_reference_mode_equals_the_restatement(kind, B, size, otree):
    crit = _crit()
    torch.manual_seed(3)
    init = {k: v.clone() for k, v in _ref(kind).state_dict().items()}
    eng = _eng(kind)
    assert eng._side is not None and eng._overlap and eng.res_share is None
    assert eng.classifier_names == ("fc.weight", "fc.bias")
    eng.set_reference_fp32(True)
    assert eng.act_dtype == torch.float32
    worst_by_seed = []
    for seed in SEEDS:
        ref = _ref(kind)
        ref.load_state_dict(init)
        eng.load_state_dict(init)
        x, y = _batch(seed, B, size)
        z_ref, loss_ref, g_ref = _oracle_step(ref, otree, x, y)
        z, loss, grads = _engine_step(eng, crit, x, y)
        scale = z_ref.abs().max().item()
        assert (z - z_ref).abs().max().item() < 1e-4 * scale
        assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref), (loss, loss_ref)
        assert set(grads) == set(g_ref)
        errs = sorted((_rel_l2(grads[n], g_ref[n]), n) for n in g_ref)
        print(f"[{kind} {SMALL} fp32 {size}x{size} / inputs {seed}] loss {loss:.6f} vs {loss_ref:.6f}; parameter-gradient "
              f"rel-L2: worst {errs[-1][0]:.2e} ({errs[-1][1]}), median {errs[len(errs) // 2][0]:.2e}")
        assert errs[-1][0] < TOL_TIE, errs[-1]
        sd, sd_ref = eng.state_dict(), ref.state_dict()
        for k in sd_ref:
            if k.endswith("running_var") or k.endswith("running_mean"):
                assert _rel_l2(sd[k], sd_ref[k]) < 1e-4, k
        worst_by_seed.append((errs[-1][0], seed))
    assert min(worst_by_seed)[0] < TOL, worst_by_seed


def test_loaded_conv1_weight_gives_the_restatements_stem_output():
    """A [64,3,7,7] conv1.weight loaded through the (r, s, ci) view of the [64][1][160] master: the engine's stem (patches ->
    1x1 conv -> bn1 -> ReLU, fp32 storage) is the restatement's conv1 -> bn1 -> ReLU, and the pooled tensor its max-pool."""
    torch.manual_seed(5)
    ref = _ref("basic")
    eng = _eng("basic", seed=9)
    eng.load_state_dict(ref.state_dict())
    assert torch.equal(eng.state_dict()["conv1.weight"].cpu(), ref.state_dict()["conv1.weight"])
    master = eng.store.p("conv1.weight").cpu()
    assert tuple(master.shape) == (64, 1, 160) and master[:, 0, 147:].abs().sum().item() == 0
    assert torch.equal(master[:, 0, :147].view(64, 7, 7, 3), ref.conv1.weight.detach().permute(0, 2, 3, 1))
    eng.set_reference_fp32(True)
    x, _ = _batch(2, 2, 64)
    eng.forward(x.to(DEV), training=True)
    ref.train()
    with torch.no_grad():
        a_ref = ref.stem(x)
        p_ref = torch.nn.functional.max_pool2d(a_ref, 3, 2, 1)
    a = ops.interior(eng.buf("a0", 2, 32, 32, 64)).cpu().permute(0, 3, 1, 2)
    p = ops.interior(eng.buf("p0", 2, 16, 16, 64)).cpu().permute(0, 3, 1, 2)
    scale = a_ref.abs().max().item()
    assert (a - a_ref).abs().max().item() < 1e-4 * scale and (p - p_ref).abs().max().item() < 1e-4 * scale


@pytest.mark.parametrize("size", [128, 224])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bf16_product_path(kind, size, otree):
    """One training step and the eval-mode logits of the (1,1,1,1) nets in bf16 storage, 8 images.  Asserted: finite loss;
    HardNBDT decisions of the HIP rules kernel on the engine's own logits equal the oracle's rules on the same logits;
    eval-mode logits (after one shared training-mode forward) meet the eval bar of tests/test_models_gpu.py against the
    restatement: argmax agreement >= 0.9, max error < 3e-2 of the logit scale.

    Measured on an MI355X (train-mode logit error against the restatement's step; eval argmax agreement, eval logit error):
        basic      128 x 128: train 0.0066 of the logit scale; eval 1.000, 0.0023
        basic      224 x 224: train 0.0042;                    eval 1.000, 0.0019
        bottleneck 128 x 128: train 0.0172;                    eval 1.000, 0.0038
        bottleneck 224 x 224: train 0.0134;                    eval 1.000, 0.0018
    The 224 figures are no worse than the 128 ones: the generic kernels the ragged grids fall back to round as the others."""
    torch.manual_seed(4)
    ref = _ref(kind)
    eng = _eng(kind, seed=1)
    eng.load_state_dict(ref.state_dict())
    x, y = _batch(31, 8, size)
    z_ref, loss_ref, _ = _oracle_step(ref, otree, x, y)             # the shared training-mode forward (running statistics)
    z, loss, _ = _engine_step(eng, _crit(), x, y)
    assert np.isfinite(loss)
    tree = Tree(DATASET, hierarchy=HIERARCHY)
    hard = _C.hard_forward(tree.device_handle(0), z.to(DEV), want_onehot=False)[0].cpu().numpy()
    assert np.array_equal(hard, O.hard_forward(otree, z.numpy()))
    ref.eval()
    with torch.no_grad():
        ze_ref = ref(x)
    ze = eng.forward(x.to(DEV), training=False).float().cpu()
    agree = (ze.argmax(1) == ze_ref.argmax(1)).float().mean().item()
    err = (ze - ze_ref).abs().max().item() / ze_ref.abs().max().item()
    print(f"[{kind} {SMALL} bf16 {size}x{size}] train loss {loss:.5f} (restatement {loss_ref:.5f}), train logit error "
          f"{(z - z_ref).abs().max().item() / z_ref.abs().max().item():.4f} of scale; eval argmax agreement {agree:.3f}, "
          f"eval logit error {err:.4f} of scale")
    assert agree >= 0.9
    assert err < 3e-2


def test_two_stream_step_equals_one_stream_step_bit_for_bit():
    """Deterministic mode, resnet18 depth at 128 x 128: the two-stream schedule (weight gradients, conv1's over the patch
    tensor included, on the second stream) reproduces the one-stream schedule's loss, logits and every gradient exactly, and
    two identical steps are bit-identical."""
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in _ref("basic", (2, 2, 2, 2)).state_dict().items()}
    eng, crit = _eng("basic", (2, 2, 2, 2)), _crit()
    x, y = _batch(6, 4, 128)
    ops.set_deterministic(True)
    try:
        out = []
        for overlap in (True, True, False):
            eng.set_overlap(overlap)
            eng.load_state_dict(init)
            out.append(_engine_step(eng, crit, x, y))
    finally:
        ops.set_deterministic(False)
        eng.set_overlap(True)
    (z2, l2, g2), (z2b, l2b, g2b), (z1, l1, g1) = out
    assert l2 == l1 == l2b and torch.equal(z2, z1) and torch.equal(z2, z2b)
    for n in g1:
        assert torch.equal(g2[n], g1[n]), n
        assert torch.equal(g2[n], g2b[n]), n
    assert g1["conv1.weight"].abs().sum().item() > 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_three_train_steps_lower_the_loss(kind):
    eng = _eng(kind, zero_init_residual=(kind == "bottleneck"))
    if kind == "bottleneck":
        assert eng.state_dict()["layer2.0.bn3.weight"].abs().sum().item() == 0
        assert eng.state_dict()["layer2.0.bn2.weight"].min().item() == 1
    crit = _crit()
    x, y = _batch(5, 8, 128)
    x, y = x.to(DEV), y.to(DEV)
    losses = [E.train_step(eng, crit, x, y, lr=0.05).item() for _ in range(3)]
    final = crit.loss_and_grad(eng.forward(x, training=True), y)[0].item()
    print(f"[{kind} {SMALL}] losses {losses} -> {final:.4f}")
    assert all(np.isfinite(losses)) and final < losses[0]


def test_input_sides_must_be_multiples_of_32():
    eng = _eng("basic")
    with pytest.raises(ValueError, match="multiples of 32"):
        eng.forward(torch.zeros(1, 3, 112, 120, device=DEV), training=False)


def test_eval_path_and_state_dict_round_trip():
    torch.manual_seed(0)
    ref = _ref("bottleneck")
    eng = _eng("bottleneck", seed=1)
    eng.load_state_dict(ref.state_dict())
    x, _ = _batch(7, 8, 128)
    ref.train()
    with torch.no_grad():
        ref(x)                                   # move the running statistics off their initial values, both sides
    eng.forward(x.to(DEV), training=True)
    assert eng.fuse_eval
    calls, pool = [], []
    real, real_pool = ops.conv_igemm_affine, ops.maxpool_fwd
    ops.conv_igemm_affine = lambda *a, **k: (calls.append(a[0].cin), real(*a, **k))[1]
    ops.maxpool_fwd = lambda x_, y_, idx=None: (pool.append(idx), real_pool(x_, y_, idx))[1]
    try:
        z = eng.forward(x.to(DEV), training=False).float().cpu()
    finally:
        ops.conv_igemm_affine, ops.maxpool_fwd = real, real_pool
    assert len(calls) == 1 + 4 * 4 and calls[0] == 160     # the stem over 160 patch channels, then 4 launches per block
    assert pool == [None]                                  # inference keeps no window positions
    ref.eval()
    with torch.no_grad():
        z_ref = ref(x)
    assert (z - z_ref).abs().max().item() < 3e-2 * z_ref.abs().max().item()
    # engine -> restatement (strict) -> a fresh engine
    sd = {k: v.cpu() for k, v in eng.state_dict().items()}
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and tuple(sd["layer2.0.downsample.0.weight"].shape) == (512, 256, 1, 1)
    ref2 = _ref("bottleneck")
    ref2.load_state_dict(sd, strict=True)
    eng2 = _eng("bottleneck", seed=2)
    eng2.load_state_dict(ref2.state_dict())
    sd2 = eng2.state_dict()
    assert set(sd2) == set(sd)
    for k in sd:
        assert torch.equal(sd2[k].cpu(), sd[k]), k
    assert torch.equal(eng2.forward(x.to(DEV), training=False), eng.forward(x.to(DEV), training=False))


def test_initialisation_follows_torchvision():
    eng = _eng("basic", (2, 2, 2, 2), seed=3)
    sd = eng.state_dict()
    ref = R.make("resnet18", 10)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    # kaiming_normal_(fan_out, relu): std = sqrt(2 / (cout * k * k))
    for name, fan_out in (("conv1.weight", 64 * 49), ("layer3.1.conv2.weight", 256 * 9), ("layer4.0.downsample.0.weight", 512)):
        w = sd[name].float()
        assert abs(w.std().item() / (2.0 / fan_out) ** 0.5 - 1) < 0.05 and abs(w.mean().item()) < 0.1 * w.std().item(), name
    assert sd["fc.weight"].abs().max().item() <= 1 / 512 ** 0.5 and sd["fc.bias"].abs().max().item() <= 1 / 512 ** 0.5
    assert sd["layer1.0.bn2.weight"].min().item() == 1 and sd["bn1.bias"].abs().sum().item() == 0


def test_nbdt_wrappers_around_resnet18():
    model = models.resnet18(num_classes=10)
    x = torch.randn(2, 3, 64, 64).to(DEV)
    soft = SoftNBDT(dataset=DATASET, model=model, hierarchy=HIERARCHY)
    hard = HardNBDT(dataset=DATASET, model=model, hierarchy=HIERARCHY)
    with torch.no_grad():
        P, H = soft(x), hard(x)
    assert torch.isfinite(P).all() and torch.isfinite(H).all()
    assert getattr(P, "_nbdt_output_flag", False) and getattr(H, "_nbdt_output_flag", False)
    assert P.shape == (2, 10) and H.shape == (2, 10)


@pytest.mark.parametrize("argv", [
    "--arch resnet18 --dataset CIFAR10 --image-size 128 --synthetic 32 --batch-size 16 --epochs 1 "
    "--hierarchy induced-ResNet18 --loss SoftTreeSupLoss",
    "--arch resnet50 --dataset Imagenet1000 --image-size 128 --synthetic 16 --batch-size 8 --epochs 1 "
    "--hierarchy induced-efficientnet_b7b --loss SoftTreeSupLoss --weight-decay 1e-4"], ids=["resnet18", "resnet50-1000"])
def test_main_driver_trains(argv, tmp_path):
    main = os.path.join(nbdt_path.PKG_DIR, "main.py")
    out = subprocess.run([sys.executable, main] + argv.split(), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
