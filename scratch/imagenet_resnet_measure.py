"""Measurements of the ImageNet-style ResNets for DESIGN.md ("ImageNet-style ResNets"), on one MI355X:

  1. which kernel every conv / data-gradient / weight-gradient launch of a training step takes, per grid, at 224 x 224 and
     at 256 x 256 (ops.last_igemm_kernel / last_wgrad_kernel around every launch);
  2. images/s of engine.train_step with SoftTreeSupLoss (1000 classes) for resnet18 and resnet50 at 128 images, both sizes:
     median of 20 steps after 5 warm-up steps, each step ended by a device synchronise;
  3. the stem's five launches alone at 128 images (patch gather, 1x1 conv + statistics, its weight gradient, pool forward,
     pool backward): median of 20 event-bracketed launches, next to their byte bounds and as a share of the resnet18 step.

usage: python scratch/imagenet_resnet_measure.py OUT.txt"""
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nbdt_path  # noqa: E402

nbdt_path.add()
from nbdt import engine as E  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

DEV = "cuda:0"
B = 128
NETS = {"resnet18": (E.ImageNetResNetEngine, (2, 2, 2, 2)), "resnet50": (E.ImageNetBottleneckEngine, (3, 4, 6, 3))}
HBM_TBPS = 6.3     # what a streaming copy reaches on an MI355X (8.0 is the specification)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def say(line=""):
    print(line, file=out, flush=True)
    if out is not sys.stdout:
        print(line, flush=True)


def kernels_of_a_step(eng, crit, x, y):
    """{(role, gh x gw, cin -> cout, taps): kernel name} over one training step."""
    seen = {}
    names = ("conv_igemm", "conv_pw", "conv_igemm_bnbwd", "conv_igemm_multi", "conv_igemm_affine", "conv_wgrad")
    real = {n: getattr(ops, n) for n in names}

    def spy(name):
        def f(desc, *a, **k):
            r = real[name](desc, *a, **k)
            d = desc[0] if name == "conv_igemm_multi" else desc
            if name == "conv_wgrad":
                role, kern = "wgrad", ops.last_wgrad_kernel()
            else:
                at = 3 if name == "conv_pw" else 4          # bn_scratch's position after desc
                stats = k.get("bn_scratch") is not None or (name != "conv_igemm_bnbwd" and len(a) > at and a[at] is not None)
                role = "fwd" if stats else "dgrad"
                kern = ops.last_igemm_kernel()
            key = (role, f"{d.gh}x{d.gw}", f"{d.cin}->{d.cout}", d.ntaps)
            seen.setdefault(key, set()).add(kern)
            return r
        return f

    for n in names:
        setattr(ops, n, spy(n))
    try:
        E.train_step(eng, crit, x, y, lr=0.01)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(ops, n, real[n])
    return seen


def step_ms(eng, crit, x, y, warmup=5, steps=20):
    for _ in range(warmup):
        E.train_step(eng, crit, x, y, lr=0.01)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        E.train_step(eng, crit, x, y, lr=0.01)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def launch_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(1e3 * s.elapsed_time(e))
    return statistics.median(ts)


def stem_launches(size):
    """name -> (median us, bytes moved) of the stem's launches at B images of size x size."""
    h = size // 2
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, size, size, generator=g).to(DEV)
    patches = ops.padded(B, h, h, 160, DEV)
    t0, a0, ga = (ops.padded(B, h, h, 64, DEV) for _ in range(3))
    p0, gp = ops.padded(B, h // 2, h // 2, 64, DEV), ops.padded(B, h // 2, h // 2, 64, DEV)
    idx = torch.empty(B, h // 2, h // 2, 64, dtype=torch.uint8, device=DEV)
    w = (torch.randn(64, 1, 160, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    dw = torch.zeros(64, 1, 160, device=DEV)
    part = torch.empty(((B * h * h + 255) // 256) * 2 * 64, device=DEV)
    fwd, wg = ops.conv_fwd_desc(B, h, h, 160, 64, 1, 1), ops.conv_wgrad_desc(B, h, h, 160, 64, 1, 1)
    ops.stem_patches(img, patches, 7, 2)
    ops.interior(a0).copy_(torch.randn(B, h, h, 64, generator=g).to(torch.bfloat16))
    ops.interior(t0).copy_(ops.interior(a0))
    ops.interior(gp).copy_(torch.randn(B, h // 2, h // 2, 64, generator=g).to(torch.bfloat16))
    ops.maxpool_fwd(a0, p0, idx)
    npix, act = B * h * h, B * h * h * 64 * 2
    return {
        "stem_patches": (launch_us(lambda: ops.stem_patches(img, patches, 7, 2)), img.numel() * 4 + npix * 160 * 2),
        "conv1 1x1 forward + statistics": (launch_us(lambda: ops.conv_igemm(fwd, patches, w, t0, bn_scratch=part)),
                                           npix * 160 * 2 + act),
        "conv1 weight gradient": (launch_us(lambda: ops.conv_wgrad(wg, patches, t0, dw)), npix * 160 * 2 + act),
        "maxpool forward (+ positions)": (launch_us(lambda: ops.maxpool_fwd(a0, p0, idx)), act + act // 4 + idx.numel()),
        "maxpool backward": (launch_us(lambda: ops.maxpool_bwd(gp, idx, ga)), act // 4 + idx.numel() + act),
    }, (ops.last_igemm_kernel(), ops.last_wgrad_kernel())


def main():
    assert torch.cuda.is_available()
    crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    steps = {}
    for name, (cls, blocks) in NETS.items():
        eng = cls(num_classes=1000, num_blocks=blocks, device=DEV, seed=0)
        for size in (224, 256):
            x = torch.randn(B, 3, size, size, generator=g).to(DEV)
            seen = kernels_of_a_step(eng, crit, x, y)
            say(f"== {name}, {B} x 3 x {size} x {size}: kernel of every launch of a training step (role, grid, channels, taps)")
            for key in sorted(seen, key=lambda k: (-int(k[1].split("x")[0]), k[0], k[2], k[3])):
                say(f"   {key[0]:5s} {key[1]:>9s} {key[2]:>11s} taps {key[3]}: {', '.join(sorted(seen[key]))}")
            med, lo, hi = step_ms(eng, crit, x, y)
            steps[(name, size)] = med
            say(f"== {name}, {B} x 3 x {size} x {size}: train_step median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, 20 steps) "
                f"= {B / med * 1e3:.0f} images/s")
            say()
        del eng
        torch.cuda.empty_cache()
    for size in (224, 256):
        table, (k_fwd, k_wg) = stem_launches(size)
        say(f"== stem launches alone, {B} x 3 x {size} x {size} (conv1: {k_fwd}; its weight gradient: {k_wg})")
        total = 0.0
        for what, (us, nbytes) in table.items():
            bound = nbytes / (HBM_TBPS * 1e12) * 1e6
            total += us
            say(f"   {what:32s} {us:8.1f} us   {nbytes / 1e6:8.1f} MB   byte bound at {HBM_TBPS:.1f} TB/s {bound:6.1f} us "
                f"({bound / us:5.1%} of it)   {us / (steps[('resnet18', size)] * 1e3):5.1%} of the resnet18 step, "
                f"{us / (steps[('resnet50', size)] * 1e3):5.1%} of the resnet50 step")
        say(f"   sum {total:.1f} us")
        say()


main()
