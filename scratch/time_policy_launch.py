"""The policy launch (nbdt_policy_batch: TrivialAugmentWide + random erasing) next to nbdt_augment_batch at 512 CIFAR-shaped
and 512 TinyImagenet-shaped uint8 images, and the WRN-28-10 training step fed by either, in one process.  Launches: each
the median (and minimum) of 20 event-bracketed calls after 3 warm-up calls and the time per call of 50 calls issued back to
back, three interleaved rounds; then one round per
operation (every image of the batch given that operation at bin 15), which shows what the slowest block of a mixed batch
costs.  Step: DeviceDataset.batch + train_step at 512 x 32 x 32, the median of 20 event-bracketed steps after 3, alternating
policy off / on (--no-step: the launches only).  profiles/policy_launch.txt."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from nbdt import data as D  # noqa: E402
from nbdt.engine import WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
with_step = "--no-step" not in sys.argv
B = 512


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


def streamed(fn, calls=50):
    """us per call of `calls` calls issued back to back between one pair of events: what the device (or, when it is slower,
    the host side of the call) sustains, without the idle-queue launch latency every single bracketed call pays."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def fmt(name, fn):
    t = timed(fn)
    return f"{name} median {t[0]:.1f} us min {t[1]:.1f} us; back to back {streamed(fn):.1f} us per call"


g = torch.Generator().manual_seed(0)
sets = {}
for name, n, side in (("CIFAR10", 50000, 32), ("TinyImagenet200", 20000, 64)):
    st = D.DATASET_STATS[name]
    x = torch.randint(0, 256, (n, 3, side, side), dtype=torch.uint8, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    kw = dict(device="cuda:0")
    sets[name] = (D.DeviceDataset(x, y, st["mean"], st["std"], st["pad"], **kw),
                  D.DeviceDataset(x, y, st["mean"], st["std"], st["pad"], policy="ta_wide", erase_prob=0.1, **kw),
                  torch.randint(0, n, (B,), generator=g).to("cuda:0"))

for name, (plain, policy, index) in sets.items():
    side = plain.shape[2]
    moved = 3 * side * side * 5
    identity = torch.zeros(B, 7, dtype=torch.int32, device="cuda:0")
    print(f"{tag}: {name}, {B} images of 3 x {side} x {side}: {moved} bytes per image (1 in, 4 out), {B * moved / 1e6:.1f} MB per launch")
    for r in range(3):
        row = [fmt("nbdt_augment_batch", lambda: plain.batch(index, epoch=r)),
               fmt("nbdt_policy_batch (ta_wide, erase 0.1)", lambda: policy.batch(index, epoch=r)),
               fmt("nbdt_policy_batch (Identity, no erase)", lambda: plain.batch(index, epoch=r, policy_params=identity))]
        print(f"{tag} {name} round {r}: " + "\n    ".join(row))
    per_op = []
    for op, op_name in enumerate(D.POLICY_OPS):
        pp = torch.tensor([[op, 15, 0, 0, 0, 0, 0]] * B, dtype=torch.int32, device="cuda:0")
        per_op.append(f"{op_name} {streamed(lambda: plain.batch(index, policy_params=pp)):.1f}")
    print(f"{tag} {name} every image the same op, back to back, us per call: " + ", ".join(per_op))

if not with_step:
    sys.exit(0)

eng = WRNEngine(num_classes=10, blocks=28, width_factor=10, device="cuda:0", seed=0)
crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
plain, policy, index = sets["CIFAR10"]


def step_with(ds):
    def step():
        img, tgt = ds.batch(index)
        train_step(eng, crit, img, tgt, lr=1e-3)
    return step


for r in range(3):
    off, on = timed(step_with(plain)), timed(step_with(policy))
    print(f"{tag} WRN-28-10 batch + step round {r}: policy off median {off[0] / 1e3:.3f} ms min {off[1] / 1e3:.3f} ms    "
          f"policy on median {on[0] / 1e3:.3f} ms min {on[1] / 1e3:.3f} ms")
