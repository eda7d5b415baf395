#!/usr/bin/env python3
"""nbdt_tree_stats_accumulate (every output requested) against the three launches it subsumes -- nbdt_node_outputs,
nbdt_hard_forward with decision buffers, nbdt_soft_forward -- at the BASELINE.json rules shapes: median of per-launch
device-event times, the two alternating in one process.  `--once` runs each launch once per shape (for a kernel trace)."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nbdt_path
nbdt_path.add()
import torch
from nbdt import _C, ops
from nbdt.tree import Tree

SHAPES = [(512, "CIFAR10", "induced-wrn28_10_cifar10"), (1024, "CIFAR100", "induced-wrn28_10_cifar100"),
          (1024, "TinyImagenet200", "induced-ResNet18"), (256, "Imagenet1000", "induced-efficientnet_b7b")]
once = "--once" in sys.argv
dev = torch.device("cuda", 0)


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


for B, ds, h in SHAPES:
    tree = Tree(ds, hierarchy=h)
    handle = tree.device_handle(0)
    C = len(tree.classes)
    g = torch.Generator().manual_seed(B + C)
    z = (torch.randn(B, C, generator=g) * 3).to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    block = {f: torch.zeros(n, dtype=torch.int64, device=dev) for f, n in ops.tree_stats_sizes(handle).items()}
    scores = torch.empty(B, 3, device=dev)
    fused = lambda: ops.tree_stats_accumulate(handle, z, y, block, scores)
    parts = [lambda: _C.node_outputs(handle, z), lambda: _C.hard_forward(handle, z, want_onehot=False, want_decisions=True),
             lambda: _C.soft_forward(handle, z)]
    if once:
        for fn in [fused] + parts:
            fn()
        torch.cuda.synchronize()
        continue
    for fn in [fused] + parts:
        timed(fn, 10)
    t_fused, t_parts = [], [[], [], []]
    for _ in range(5):                      # alternate, 5 x 20 launches each
        t_fused += timed(fused, 20)
        for i, fn in enumerate(parts):
            t_parts[i] += timed(fn, 20)
    med = statistics.median
    three = [med(t) for t in t_parts]
    print(f"B={B} {ds}: fused {med(t_fused):.1f} us | node_outputs {three[0]:.1f} + hard_forward(decisions) {three[1]:.1f} "
          f"+ soft_forward {three[2]:.1f} = {sum(three):.1f} us | fused/sum {med(t_fused) / sum(three):.2f}", flush=True)
