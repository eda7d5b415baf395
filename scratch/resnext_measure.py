"""Measurements of the grouped 3x3 convolution and of the ResNeXt / wide ResNet steps for DESIGN.md ("ResNeXt and wide
ResNets"), on one MI355X, 128 images:

  1. per launch, resnext50_32x4d's conv2 shapes at 224 x 224 and 256 x 256 input (the stride-1 conv of every stage and the
     strided one that opens stages 2 - 4), forward / data gradient / weight gradient:
       (a) the grouped kernels (csrc/conv_group.hip),
       (b) the dense block-diagonal launch of the same width on the dense entries as engine.Conv launches them
           (nbdt_conv_igemm with DMA-ordered tiles where it takes them, nbdt_conv_igemm_multi for the strided data
           gradient, nbdt_conv_wgrad),
       (c) the byte floor (input + output bytes) / 6.3 TB/s.
     (a) and (b) alternate on one device: REPS rounds of one event-bracketed run of INNER launches each, median and min - max
     of the per-launch time over the rounds.  Random bf16 data; (a) and (b) are compared bit for bit on integer data by
     tests/test_conv_group_gpu.py, not here.
  2. whole step: engine.train_step with SoftTreeSupLoss (1000 classes) for resnet50, resnext50_32x4d and wide_resnet50_2,
     median of 20 steps after 5 warm-up steps, each ended by a device synchronise; and, in a one-stream step
     (set_overlap(False)), the time between events around every grouped launch as a share of that step.

usage: python scratch/resnext_measure.py OUT.txt"""
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
REPS, INNER = 15, 10
HBM_TBPS = 6.3     # what a streaming copy reaches on an MI355X (8.0 is the specification)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def say(line=""):
    print(line, file=out, flush=True)
    if out is not sys.stdout:
        print(line, flush=True)


def bracket_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(INNER):
        fn()
    e.record()
    e.synchronize()
    return 1e3 * s.elapsed_time(e) / INNER


def alternate(fa, fb):
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(bracket_us(fa))
        tb.append(bracket_us(fb))
    return ta, tb


def fmt(ts):
    return f"{statistics.median(ts):7.1f} ({min(ts):6.1f} - {max(ts):6.1f})"


def conv2_shapes(size):
    """(stage, width, cg, input side, stride) of resnext50_32x4d's conv2 launches."""
    s = size // 4
    return [("layer1", 128, 4, s, 1), ("layer2.0", 256, 8, s, 2), ("layer2", 256, 8, s // 2, 1), ("layer3.0", 512, 16, s // 2, 2),
            ("layer3", 512, 16, s // 4, 1), ("layer4.0", 1024, 32, s // 4, 2), ("layer4", 1024, 32, s // 8, 1)]


def per_launch(size):
    g = torch.Generator().manual_seed(size)
    say(f"== per launch, {B} images, {size} x {size} input: us per launch, median (min - max) of {REPS} rounds of {INNER} launches")
    say(f"   {'conv2 of':9s} {'width/cg':>8s} {'grid':>9s} s  {'op':6s} {'(a) grouped kernel':>26s} {'(b) dense block-diagonal':>26s} "
        f"{'(c) floor':>9s} {'(a)/(b)':>8s} {'(a)/(c)':>8s}   kernel of (b)")
    for stage, width, cg, H, s in conv2_shapes(size):
        Ho = H // s
        x, gin = ops.padded(B, H, H, width, DEV), ops.padded(B, H, H, width, DEV)
        gy, y = ops.padded(B, Ho, Ho, width, DEV), ops.padded(B, Ho, Ho, width, DEV)
        ops.interior(x).copy_(torch.randn(B, H, H, width, generator=g).to(torch.bfloat16))
        ops.interior(gy).copy_(torch.randn(B, Ho, Ho, width, generator=g).to(torch.bfloat16))
        master = (torch.randn(width, 9, cg, generator=g) / (9 * cg) ** 0.5).to(DEV)
        wf = torch.empty(width * 9 * 32, dtype=torch.bfloat16, device=DEV)
        wd = torch.empty_like(wf)
        ops.conv_group_weight_prep(master, width, cg, wf, wd)
        dense = torch.zeros(width, 9, width, device=DEV)
        for c0 in range(0, width, cg):
            dense[c0:c0 + cg, :, c0:c0 + cg] = master[c0:c0 + cg]
        conv = E.Conv(E.ParamStore(DEV), "w", width, width, 3, s, torch.Generator().manual_seed(0))      # engine.Conv's plan
        wb = torch.empty(width, 9, width, dtype=torch.bfloat16, device=DEV)
        wdd = torch.empty(width, 9, width, dtype=torch.bfloat16, device=DEV)
        ops.weight_prep(dense, width, 9, width, wb, wdd)
        if s == 1:
            conv.wt_fwd, conv.wt_dgrad = ops.weight_tiles(wb), ops.weight_tiles(wdd)
        fwd, dgrad, _, wgd = conv.plan(B, H, H)
        dw, dwd = torch.zeros(width, 9, cg, device=DEV), torch.zeros(width, 9, width, device=DEV)
        act_in, act_out = B * H * H * width * 2, B * Ho * Ho * width * 2

        def dense_dgrad():
            if len(dgrad) > 1:
                ops.conv_igemm_multi(dgrad, gy, wdd, gin)
            else:
                ops.conv_igemm(dgrad[0], gy, wdd, gin)

        rows = [("fwd", lambda: ops.conv_group_fwd(x, wf, y, cg, s), lambda: ops.conv_igemm(fwd, x, wb, y), ops.last_igemm_kernel),
                ("dgrad", lambda: ops.conv_group_dgrad(gy, wd, gin, cg, s), dense_dgrad, ops.last_igemm_kernel),
                ("wgrad", lambda: ops.conv_group_wgrad(x, gy, dw, cg, s), lambda: ops.conv_wgrad(wgd, x, gy, dwd),
                 ops.last_wgrad_kernel)]
        for op, fa, fb, kern in rows:
            ta, tb = alternate(fa, fb)
            floor = (act_in + act_out) / (HBM_TBPS * 1e12) * 1e6
            ma, mb = statistics.median(ta), statistics.median(tb)
            say(f"   {stage:9s} {width:5d}/{cg:<2d} {Ho:4d}x{Ho:<4d} {s}  {op:6s} {fmt(ta):>26s} {fmt(tb):>26s} {floor:9.1f} "
                f"{ma / mb:8.2f} {ma / floor:8.2f}   {kern()}")
        del x, gin, gy, y, dense, wb, wdd, dwd
    say()


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


def grouped_share(eng, crit, x, y):
    """One-stream steps with events around every grouped launch: (sum of the bracketed times, step time) in ms, median of 5."""
    names = ("conv_group_fwd", "conv_group_dgrad", "conv_group_wgrad")
    real = {n: getattr(ops, n) for n in names}
    evs = []

    def spy(name):
        def f(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = real[name](*a, **k)
            e.record()
            evs.append((s, e))
            return r
        return f

    eng.set_overlap(False)
    res = []
    try:
        for n in names:
            setattr(ops, n, spy(n))
        for i in range(7):
            evs.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.train_step(eng, crit, x, y, lr=0.01)
            torch.cuda.synchronize()
            step = 1e3 * (time.perf_counter() - t0)
            if i >= 2:
                res.append((sum(s.elapsed_time(e) for s, e in evs), step, len(evs)))
    finally:
        for n in names:
            setattr(ops, n, real[n])
        eng.set_overlap(True)
    res.sort()
    return res[len(res) // 2]


def whole_steps():
    crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    nets = {"resnet50": {}, "resnext50_32x4d": dict(groups=32, width_per_group=4), "wide_resnet50_2": dict(width_per_group=128)}
    for name, kw in nets.items():
        eng = E.ImageNetBottleneckEngine(num_classes=1000, num_blocks=(3, 4, 6, 3), device=DEV, seed=0, **kw)
        for size in (224, 256):
            x = torch.randn(B, 3, size, size, generator=g).to(DEV)
            med, lo, hi = step_ms(eng, crit, x, y)
            say(f"== {name}, {B} x 3 x {size} x {size}: train_step median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, 20 steps) "
                f"= {B / med * 1e3:.0f} images/s")
            if eng.gconvs:
                inside, step, n = grouped_share(eng, crit, x, y)
                say(f"   one-stream step {step:.2f} ms, of which {inside:.2f} ms ({inside / step:.1%}) between the events around its "
                    f"{n} grouped launches (16 forward, 16 data gradient, 16 weight gradient with its fold)")
        del eng
        torch.cuda.empty_cache()
        say()


assert torch.cuda.is_available()
which = sys.argv[2] if len(sys.argv) > 2 else "all"
if which in ("all", "launch"):
    per_launch(224)
    per_launch(256)
if which in ("all", "step"):
    whole_steps()
