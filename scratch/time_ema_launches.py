"""The weight-EMA launches alone at the WRN-28-10 arena size (36.5 M fp32 elements), and the WRN-28-10 training step with
and without engine.ema_update(), in one process.  Launches: each the median (and minimum) of 20 event-bracketed calls after
3 warm-up calls, three interleaved rounds, next to their byte bounds at the 6.3 TB/s a streaming copy reaches -- 12 bytes per
element for the update (two reads, one write), 18 for the swap with the mirror (two reads, two writes, the bf16 write), 16
without it -- and next to ops.sgd_step (26 bytes per element) on the same box.  Step: train_step at 512 x 32 x 32, the
median of 20 event-bracketed steps after 3 warm-up steps, alternating off / on.  profiles/ema_launches.txt."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.engine import WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
COPY_TBPS = 6.3
eng = WRNEngine(num_classes=10, blocks=28, width_factor=10, device="cuda:0", seed=0)
eng.ema_enable(0.9999)
s = eng.store
n = s.flat.numel()
table = eng._ema_table


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def fmt(name, t, bytes_per_el=None):
    out = f"{name} median {t[0]:.1f} us min {t[1]:.1f} us"
    if bytes_per_el:
        bound = bytes_per_el * n / (COPY_TBPS * 1e6)
        out += f" (bound {bound:.1f} us, {bytes_per_el * n / t[0] / 1e6:.2f} TB/s)"
    return out


print(f"{tag}: WRN-28-10 arena n = {n} fp32 elements ({4 * n / 1e6:.1f} MB); {table.n_rows} running-statistics rows, "
      f"{eng._ema_stats.numel()} elements")
for r in range(3):
    row = [fmt("update", timed(lambda: ops.ema_update(s.flat, s.ema, 1e-4)), 12),
           fmt("swap + mirror", timed(lambda: ops.ema_swap(s.flat, s.ema, s.bf16)), 18),   # (20 + 3 calls: an odd count ...)
           fmt("swap", timed(lambda: ops.ema_swap(s.flat, s.ema)), 16),                    # (... and 23 more: back where it was)
           fmt("update_multi", timed(lambda: table.update(1e-4))),
           fmt("swap_multi", timed(lambda: (table.swap(), table.swap()))),
           fmt("sgd launch", timed(lambda: ops.sgd_step(s.flat, s.grad, s.mom, 1e-6, 0.9, 5e-4, 1.0, s.bf16, zero_grad=True)), 26)]
    print(f"{tag} round {r}: " + "\n    ".join(row))
print(f"{tag} engine calls: " + "  ".join([
    fmt("ema_update()", timed(eng.ema_update)),
    fmt("ema_swap() x 2 (with the derived-weight refresh)", timed(lambda: (eng.ema_swap(), eng.ema_swap())))]))
assert not eng.ema_swapped

crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
g = torch.Generator().manual_seed(0)
x = torch.randn(512, 3, 32, 32, generator=g).to("cuda:0")
y = torch.randint(0, 10, (512,), generator=g).to("cuda:0")


def step_off():
    train_step(eng, crit, x, y, lr=1e-3)


def step_on():
    train_step(eng, crit, x, y, lr=1e-3)
    eng.ema_update()


for r in range(3):
    off, on = timed(step_off), timed(step_on)
    print(f"{tag} step round {r}: without ema_update median {off[0] / 1e3:.3f} ms min {off[1] / 1e3:.3f} ms    "
          f"with median {on[0] / 1e3:.3f} ms min {on[1] / 1e3:.3f} ms")
