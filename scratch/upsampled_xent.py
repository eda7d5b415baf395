"""SoftSegTreeSupLoss forward + backward with an UpsampledCrossEntropyLoss criterion: the fused path (csrc/upsampled_xent.hip
for both cross-entropies, the rules on the low-resolution grid) against the composed torch path (the same criterion under a
subclass: F.interpolate and F.cross_entropy through autograd on the autograd-enabled pixel rules), which is what a user
with a 1/4-resolution backbone had before.

  python scratch/upsampled_xent.py [OUT.txt] [SHAPES]      (needs an MI355X; profiles/upsampled_xent.txt is its output)

Shapes: 8 x 19 x 128 x 256 -> 512 x 1024 (Cityscapes-like, on a synthetic 19-class binary hierarchy) and
8 x 150 x 128 x 128 -> 512 x 512 (ADE20K, tests/golden/seg_hierarchies), fp32 and bf16 logits, 10 % ignored labels.
SHAPES = "city", "ade" or "city,ade" (default).  Per call: a host clock around `iters` forward + backward passes that end
in a device synchronise, after a warm-up; windows of the two paths alternate, the median of 5 and [min, max] are printed.
Peak bytes: torch.cuda.max_memory_allocated() across one forward + backward, minus what was allocated before it.  The
stand-alone kernel pair (nbdt_upsampled_xent on the logits alone) is timed too, with the terms it evaluates per second.
The two paths are compared on the timed tensors before they are timed."""
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbdt_path  # noqa: E402

nbdt_path.add()
import _tree_shapes as S  # noqa: E402
from nbdt import _C  # noqa: E402
from nbdt import loss as L  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
IGNORE, TSW = 255, 10.0


class Composed(L.UpsampledCrossEntropyLoss):
    """Another type, and torch's composition throughout: SoftSegTreeSupLoss applies it through autograd."""

    def forward(self, score, target):
        return self.composed(score, target)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def time_pair(a, b):
    """Median, min, max of 5 alternating windows of each, in us per call."""
    iters = []
    for fn in (a, b):
        for _ in range(2):
            fn()
        once = window(fn, 1)
        iters.append(max(5, min(500, int(0.25e6 / max(once, 1.0)))))
    wa, wb = [], []
    for _ in range(5):
        wa.append(window(a, iters[0]))
        wb.append(window(b, iters[1]))
    wa.sort()
    wb.sort()
    return (wa[2], wa[0], wa[-1], iters[0]), (wb[2], wb[0], wb[-1], iters[1])


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - before
    del out
    return top


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    which = (sys.argv[2] if len(sys.argv) > 2 else "city,ade").split(",")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "needs an MI355X"
    tmp = tempfile.mkdtemp()
    pg, pw, leaves = S.kary(tmp, 19, 2)
    gold = os.path.join(ROOT, "tests", "golden", "seg_hierarchies")
    shapes = {"city": ("kary19_2 (Cityscapes-like)", Tree(None, path_graph=pg, path_wnids=pw, classes=leaves),
                       (8, 19, 128, 256), (512, 1024)),
              "ade": ("ADE20K induced-HRNet-w48",
                      Tree("ADE20K", path_graph=os.path.join(gold, "ADE20K-graph-induced-HRNet-w48.json"),
                           path_wnids=os.path.join(gold, "ADE20K-wnids.txt")), (8, 150, 128, 128), (512, 512))}
    props = torch.cuda.get_device_properties(0)
    say(f"SoftSegTreeSupLoss(UpsampledCrossEntropyLoss(ignore_index={IGNORE}), tree_supervision_weight={TSW:g}) forward + "
        f"backward, fused against composed, {props.name} ({props.multi_processor_count} CUs)")
    say("us = median of 5 alternating windows [min, max] x calls per window; peak = bytes allocated above the inputs")
    for key in which:
        name, tree, shape, (H, W) = shapes[key]
        N, C, h, w = shape
        full = N * C * H * W * 4
        say()
        say(f"{name}: {' x '.join(map(str, shape))} -> {H} x {W}; one [N, C, H, W] fp32 tensor is {full / 1e6:.1f} MB")
        g = torch.Generator().manual_seed(7)
        z32 = 3.0 * torch.randn(shape, generator=g)
        y = torch.randint(0, C, (N, H, W), generator=g)
        y[torch.rand(y.shape, generator=g) < 0.1] = IGNORE
        y = y.to(DEV)
        make = lambda crit: L.SoftSegTreeSupLoss(dataset=None, criterion=crit, tree=tree, tree_supervision_weight=TSW)  # noqa: E731
        fused, composed = make(L.UpsampledCrossEntropyLoss(ignore_index=IGNORE)), make(Composed(ignore_index=IGNORE))
        for dtype in (torch.float32, torch.bfloat16):
            z = z32.to(DEV).to(dtype)

            def step(crit):
                zz = z.detach().requires_grad_(True)
                loss = crit(zz, y)
                loss.backward()
                return loss.detach(), zz.grad

            a, b = step(fused), step(composed)
            same = (f"loss {a[0].item():.6f} / {b[0].item():.6f}, max |dz diff| "
                    f"{(a[1].float() - b[1].float()).abs().max().item():.2e}")
            del a, b
            pf, pc = peak(lambda: step(fused)), peak(lambda: step(composed))
            tf, tc = time_pair(lambda: step(fused), lambda: step(composed))
            for label, (med, lo, hi, iters), pk in (("fused", tf, pf), ("composed", tc, pc)):
                say(f"  {str(dtype)[6:]:8s} loss fwd+bwd {label:8s} {med:10.1f} us [{lo:.1f}, {hi:.1f}] x{iters:<4d} "
                    f"peak {pk / 1e6:9.1f} MB = {pk / full:5.2f} full-resolution tensors")
            say(f"  {'':8s} fused is {tc[0] / tf[0]:.2f}x the composed path (windows do"
                f"{'' if tf[2] < tc[1] else ' NOT'} separate); {same}")
            # the kernel pair alone, on the logits: forward lerps 2 * C per pixel, backward about (H/h) * (W/w) * 4 terms
            # per low-resolution element (each a lerp and an exponential)
            alone = lambda: _C.upsampled_xent(z, y, False, IGNORE)  # noqa: E731
            rules = lambda: _C.seg_soft_backward(tree.device_handle(0), z, _C.seg_soft_forward(tree.device_handle(0), z))  # noqa: E731
            ta, tr = time_pair(alone, rules)
            terms = N * C * (2 * H * W + h * w * 4 * (H // h) * (W // w))
            say(f"  {str(dtype)[6:]:8s} nbdt_upsampled_xent alone {ta[0]:10.1f} us [{ta[1]:.1f}, {ta[2]:.1f}] x{ta[3]:<4d} "
                f"{terms / ta[0] / 1e3:7.1f} G terms/s;  rules forward + backward on the low-resolution grid "
                f"{tr[0]:10.1f} us [{tr[1]:.1f}, {tr[2]:.1f}]")
            del z
        del y
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
