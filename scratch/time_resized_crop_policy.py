"""nbdt_resized_crop_policy_batch (both launches: RandAugment N = 2, M = 9 with random erasing 0.1) next to the plain
nbdt_resized_crop_batch on the same inputs in one process: 512 images, 256 x 256 uint8 source -> 224.  Each the median (and
minimum) of 20 event-bracketed calls after 3 warm-up calls and the time per call of 30 calls issued back to back, three
interleaved rounds; then every image given the same chain of 0..4 Brightness (a point operation), Rotate (a gather) or
Equalize (statistics) slots, which shows what one more pass costs; then the EfficientNet-B0 + SoftTreeSupLoss training step
at 224 and 512 images, the median of 10 steps after 3.  profiles/resized_crop_policy_launch.txt.

    python scratch/time_resized_crop_policy.py TAG [--no-step] [LIB=PATH ...]

LIB=PATH: further builds of libnbdt_hip.so (another block size of resized_crop_policy_kernel, byte loads for the point
operations) timed on the same inputs in the same rounds, for an A/B; each is named by its file."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from nbdt import _C  # noqa: E402
from nbdt import data as D  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
with_step = "--no-step" not in sys.argv
B, N, SRC, S = 512, 2048, 256, 224


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _C.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


LIBS = [("default", _C.lib())] + [(os.path.basename(a[4:]), load(a[4:])) for a in sys.argv[2:] if a.startswith("LIB=")]


def using(lib, fn):
    def call():
        _C._lib = lib
        return fn()
    return call


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


def streamed(fn, calls=30):
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


st = D.RESIZED_CROP_STATS["Imagenet1000"]
g = torch.Generator().manual_seed(0)
x = torch.randint(0, 256, (N, 3, SRC, SRC), dtype=torch.uint8, generator=g)
y = torch.randint(0, 1000, (N,), generator=g)
kw = dict(size=S, device="cuda:0")
plain = D.ResizedCropDataset(x, y, st["mean"], st["std"], **kw)
ra = D.ResizedCropDataset(x, y, st["mean"], st["std"], policy="ra", policy_ops=2, policy_magnitude=9, erase_prob=0.1, **kw)
index = torch.randint(0, N, (B,), generator=g).to("cuda:0")
tile = 3 * S * S
print(f"{tag}: {B} images, {SRC} x {SRC} -> {S}: a tile is {tile} bytes; the byte-output resample writes 1 tile per image, "
      f"every byte pass reads 1 and writes 1, the output pass reads 1 and writes 4 (fp32): {B * tile / 1e6:.1f} MB per tile "
      "and batch")
for r in range(3):
    row = [fmt("nbdt_resized_crop_batch", using(LIBS[0][1], lambda: plain.batch(index, epoch=r)))]
    row += [fmt(f"nbdt_resized_crop_policy_batch (ra N=2 M=9, erase 0.1) [{name}]", using(lib, lambda: ra.batch(index, epoch=r)))
            for name, lib in LIBS]
    print(f"{tag} round {r}: " + "\n    ".join(row))
none = torch.zeros(B, 4, dtype=torch.int32, device="cuda:0")
for op_name in ("Brightness", "Rotate", "Equalize"):
    for name, lib in LIBS:
        per_len = []
        for length in range(0, 5):
            c = torch.zeros(B, 4, 3, dtype=torch.int32)
            c[:, :length, 0] = D.CHAIN_OPS.index(op_name)
            c[:, :length, 1] = 15
            c = c.to("cuda:0")
            per_len.append(f"{length}: {streamed(using(lib, lambda: ra.batch(index, chain_params=c, erase_params=none))):.1f}")
        print(f"{tag} [{name}] every image a chain of k x {op_name}, no erase, back to back, us per call: " + ", ".join(per_len))
_C._lib = LIBS[0][1]

if with_step:
    from nbdt.engine import train_step
    from nbdt.engine_effnet import EfficientNetEngine
    from nbdt.loss import SoftTreeSupLoss
    eng = EfficientNetEngine(num_classes=1000, device="cuda:0")
    crit = SoftTreeSupLoss(dataset="Imagenet1000", criterion=nn.CrossEntropyLoss(), hierarchy="induced-efficientnet_b7b")

    def step_with(ds):
        def step():
            img, tgt = ds.batch(index)
            train_step(eng, crit, img, tgt, lr=1e-3)
        return step

    for r in range(2):
        off, on = timed(step_with(plain), reps=10), timed(step_with(ra), reps=10)
        print(f"{tag} EfficientNet-B0 batch + step at {B} x {S} x {S} round {r}: policy off median {off[0] / 1e3:.3f} ms min "
              f"{off[1] / 1e3:.3f} ms    ra N=2 M=9, erase 0.1 median {on[0] / 1e3:.3f} ms min {on[1] / 1e3:.3f} ms")
