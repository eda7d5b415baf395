"""The policy-chain launch (nbdt_policy_chain_batch: RandAugment N = 2, N = 4, AutoAugment's CIFAR-10 policy, each with
random erasing 0.1) next to nbdt_policy_batch (ta_wide + erase 0.1) at 512 CIFAR-shaped and 512 TinyImagenet-shaped uint8
images, and the WRN-28-10 training step fed by a plain or a RandAugment dataset, in one process.  Launches: each the median
(and minimum) of 20 event-bracketed calls after 3 warm-up calls and the time per call of 50 calls issued back to back, three
interleaved rounds; then every image given the same chain of 1..4 Equalize (the dearest op) or Brightness slots, which shows
what one more applied op costs.  Step: DeviceDataset.batch + train_step at 512 x 32 x 32, the median of 20 event-bracketed
steps after 3, alternating policy off / on.  A tree without the chain entry (the parent commit) times what it has.
profiles/policy_chain_launch.txt."""
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
chains = hasattr(D, "chain_table")
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


SETTINGS = [("nbdt_policy_batch (ta_wide, erase 0.1)", dict(policy="ta_wide"))]
if chains:
    SETTINGS += [("nbdt_policy_chain_batch (ra N=2 M=9, erase 0.1)", dict(policy="ra", policy_ops=2, policy_magnitude=9)),
                 ("nbdt_policy_chain_batch (ra N=4 M=9, erase 0.1)", dict(policy="ra", policy_ops=4, policy_magnitude=9)),
                 ("nbdt_policy_chain_batch (cifar10, erase 0.1)", dict(policy="cifar10"))]

g = torch.Generator().manual_seed(0)
sets = {}
for name, n, side in (("CIFAR10", 50000, 32), ("TinyImagenet200", 20000, 64)):
    st = D.DATASET_STATS[name]
    x = torch.randint(0, 256, (n, 3, side, side), dtype=torch.uint8, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    kw = dict(device="cuda:0")
    sets[name] = (D.DeviceDataset(x, y, st["mean"], st["std"], st["pad"], **kw),
                  [(label, D.DeviceDataset(x, y, st["mean"], st["std"], st["pad"], erase_prob=0.1, **s, **kw))
                   for label, s in SETTINGS],
                  torch.randint(0, n, (B,), generator=g).to("cuda:0"))

for name, (plain, policies, index) in sets.items():
    side = plain.shape[2]
    moved = 3 * side * side * 5
    print(f"{tag}: {name}, {B} images of 3 x {side} x {side}: {moved} bytes per image (1 in, 4 out), {B * moved / 1e6:.1f} MB per launch")
    for r in range(3):
        row = [fmt("nbdt_augment_batch", lambda: plain.batch(index, epoch=r))]
        row += [fmt(label, lambda ds=ds: ds.batch(index, epoch=r)) for label, ds in policies]
        print(f"{tag} {name} round {r}: " + "\n    ".join(row))
    if chains:
        ra = policies[1][1]
        none = torch.zeros(B, 4, dtype=torch.int32, device="cuda:0")
        for op_name in ("Brightness", "Equalize"):
            per_len = []
            for length in range(0, 5):
                c = torch.zeros(B, 4, 3, dtype=torch.int32)
                c[:, :length, 0] = D.CHAIN_OPS.index(op_name)
                c[:, :length, 1] = 15
                c = c.to("cuda:0")
                per_len.append(f"{length}: {streamed(lambda: ra.batch(index, chain_params=c, erase_params=none)):.1f}")
            print(f"{tag} {name} every image a chain of k x {op_name}, no erase, back to back, us per call: " + ", ".join(per_len))

if with_step:
    eng = WRNEngine(num_classes=10, blocks=28, width_factor=10, device="cuda:0", seed=0)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    plain, policies, index = sets["CIFAR10"]
    label, on_ds = policies[1] if chains else policies[0]

    def step_with(ds):
        def step():
            img, tgt = ds.batch(index)
            train_step(eng, crit, img, tgt, lr=1e-3)
        return step

    for r in range(3):
        off, on = timed(step_with(plain)), timed(step_with(on_ds))
        print(f"{tag} WRN-28-10 batch + step round {r}: policy off median {off[0] / 1e3:.3f} ms min {off[1] / 1e3:.3f} ms    "
              f"{label} median {on[0] / 1e3:.3f} ms min {on[1] / 1e3:.3f} ms")
