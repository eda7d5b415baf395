"""The gradient-clipping launches alone at the WRN-28-10 arena size (36.5 M fp32 elements), and the WRN-28-10 training step
with and without clip=, in one process.  Launches: each the median (and minimum) of 20 event-bracketed calls after 3 warm-up
calls, three interleaved rounds, as achieved TB/s on their bytes -- 4 per element for the norm pair (one read), 8 for an
apply that clips (one read, one write), none for one that does not -- next to ops.sgd_step (26 bytes per element) in the
same process.  The 146 MB arena fits the 256 MiB Infinity Cache, so "cold" calls follow a 1 GiB read (outside the bracket; a read, so that
no dirty lines are left to be written back inside it) and read from HBM, as the step's do; "back to back" calls and a second arena a quarter the size read from the cache: what is
left there is launch + arithmetic, which says whether the fp64 work or the bytes bound the norm pass.  Step: train_step at
512 x 32 x 32 with clip=None, with a bound that never clips and with one that always does, medians of 20 after 3
warm-up steps, alternating.  profiles/clip_launches.txt."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.engine import ClipConfig, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
eng = WRNEngine(num_classes=10, blocks=28, width_factor=10, device="cuda:0", seed=0)
s = eng.store
n = s.flat.numel()
g = s.grad
g.normal_(0.0, 1e-3, generator=torch.Generator(device="cuda:0").manual_seed(1))      # norm ~ 6: any bound below clips
plan = ops.ClipPlan(n, "cuda:0")
small_n = n // 4 // 4 * 4
small = g[:small_n]
small_plan = ops.ClipPlan(small_n, "cuda:0")


scrub = torch.zeros(1 << 28, dtype=torch.float32, device="cuda:0")      # 1 GiB: four times the Infinity Cache


def timed(fn, reps=20, warm=3, cold=False):
    """cold: a 1 GiB read before every call, outside the bracket, so the call's reads come from HBM and not from what
    the previous call left in the cache (the 146 MB arena fits the 256 MiB Infinity Cache)."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if cold:
            scrub.sum()
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def fmt(name, t, bytes_per_el=None, elements=None):
    out = f"{name} median {t[0]:.1f} us min {t[1]:.1f} us"
    if bytes_per_el:
        out += f" ({bytes_per_el * (elements or n) / t[0] / 1e6:.2f} TB/s on {bytes_per_el} B per element)"
    return out


def apply_clipping():
    plan.apply(g)


print(f"{tag}: WRN-28-10 arena n = {n} fp32 elements ({4 * n / 1e6:.1f} MB); second arena {small_n} elements "
      f"({4 * small_n / 1e6:.1f} MB)")
for r in range(3):
    row = [fmt("norm pair, cold", timed(lambda: plan.norm(g, 1.0, 1.0e9), cold=True), 4),
           fmt("norm pair, back to back", timed(lambda: plan.norm(g, 1.0, 1.0e9)), 4)]
    plan.norm(g, 1.0, 1.0e9)                       # the record now says coef == 1
    row.append(fmt("apply, coef == 1", timed(apply_clipping)))
    g.normal_(0.0, 1e-3)
    plan.norm(g, 1.0, 1.0e-30)                     # coef ~ 1e-30 / 6: every apply scales, and g stays finite (it underflows to 0)
    row.append(fmt("apply, coef < 1, cold", timed(apply_clipping, cold=True), 8))
    g.normal_(0.0, 1e-3)
    row.append(fmt("norm pair, quarter arena (cache-resident)", timed(lambda: small_plan.norm(small, 1.0, 1.0e9)), 4, small_n))
    row.append(fmt("sgd launch, cold", timed(lambda: ops.sgd_step(s.flat, s.grad, s.mom, 1e-6, 0.9, 5e-4, 1.0, s.bf16,
                                                                   zero_grad=False), cold=True), 26))
    print(f"{tag} round {r}: " + "\n    ".join(row))
print(f"{tag} record: {plan.to_host()}")

crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
gen = torch.Generator().manual_seed(0)
x = torch.randn(512, 3, 32, 32, generator=gen).to("cuda:0")
y = torch.randint(0, 10, (512,), generator=gen).to("cuda:0")
eng.store.mom.zero_()
eng.zero_grad()
for r in range(3):
    off = timed(lambda: train_step(eng, crit, x, y, lr=1e-3))
    loose = timed(lambda: train_step(eng, crit, x, y, lr=1e-3, clip=ClipConfig(1.0e9)))
    tight = timed(lambda: train_step(eng, crit, x, y, lr=1e-3, clip=ClipConfig(1.0e-3)))
    print(f"{tag} step round {r}: clip=None median {off[0] / 1e3:.3f} ms min {off[1] / 1e3:.3f} ms    "
          f"never clipping median {loose[0] / 1e3:.3f} ms min {loose[1] / 1e3:.3f} ms    "
          f"always clipping median {tight[0] / 1e3:.3f} ms min {tight[1] / 1e3:.3f} ms")
print(f"{tag} record after the steps: {eng.clip_stats()}")
