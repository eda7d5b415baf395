"""SHA-256 digests of what the device datasets return, for comparing two commits bit for bit (run this file at both and
diff the output; profiles/data_path_refactor_digests.txt).  Random input bytes, fixed seeds and epochs.  DeviceDataset: 61
images of 9 x 7 with pad 2 and 211 images of 32 x 32 with pad 4, batches of 1, 37 and 64, policy None with erase_prob 0.5,
"ta_wide", "ra" with 4 ops and "cifar10" (erase_prob 0.25), each with drawn parameters and with device-resident *_params
(out-of-range values among them: the kernel clamps), unsharded and as shard (1, 3), every return_* flag on.
ResizedCropDataset: 32 images of 40 x 56 to size 22 and 24, "ta_wide", "ra" and "imagenet" with erase_prob 0.5, training
(drawn and device-resident parameters) and evaluation batches."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from nbdt import data as D  # noqa: E402

DEV = "cuda:0"
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
SEED, EPOCH = 7, 3


def show(tag, out, names):
    torch.cuda.synchronize()
    for name, t in zip(names, out):
        raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        print(f"{tag}.{name} {hashlib.sha256(raw).hexdigest()}")


def wild(rng, shape, lo, hi):
    """int32 rows on the device, mostly inside [lo, hi) and some far outside."""
    v = rng.integers(lo, hi, shape)
    v = np.where(rng.random(shape) < 0.1, rng.integers(-2 ** 31, 2 ** 31, shape), v)
    return torch.from_numpy(v.astype(np.int32)).to(DEV)


rng = np.random.default_rng(20)
for n, H, W, pad in ((61, 9, 7, 2), (211, 32, 32, 4)):
    x = torch.from_numpy(rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8))
    y = torch.from_numpy(rng.integers(0, 10, n))
    for shard in (None, (1, 3)):
        lo, hi = (0, n) if shard is None else D.shard_range(n, *shard)
        for pname, kw in (("none_erase", dict(erase_prob=0.5)), ("ta_wide", dict(policy="ta_wide", erase_prob=0.25)),
                          ("ra4", dict(policy="ra", policy_ops=4, erase_prob=0.25)),
                          ("cifar10", dict(policy="cifar10", erase_prob=0.25))):
            ds = D.DeviceDataset(x, y, MEAN, STD, pad, device=DEV, shard=shard, **kw)
            for B in (1, 37, 64):
                index = torch.from_numpy(rng.integers(lo, hi, B))
                crop = torch.from_numpy(rng.integers(-3, 2 * pad + 3, (B, 3)).astype(np.int8)).to(DEV)
                tag = f"dd.{H}x{W}.{'whole' if shard is None else 'shard1of3'}.{pname}.B{B}"
                if ds.chain:
                    names = ("img", "targets", "params", "chain", "erase")
                    flags = dict(return_params=True, return_chain_params=True, return_erase_params=True)
                    given = dict(params=crop, chain_params=wild(rng, (B, 4, 3), 0, 15), erase_params=wild(rng, (B, 4), 0, H))
                else:
                    names = ("img", "targets", "params", "policy")
                    flags = dict(return_params=True, return_policy_params=True)
                    given = dict(params=crop, policy_params=wild(rng, (B, 7), 0, 14))
                show(tag + ".drawn", ds.batch(index, epoch=EPOCH, seed=SEED, **flags), names)
                show(tag + ".given", ds.batch(index.to(DEV), epoch=EPOCH, seed=SEED, **given, **flags), names)
                show(tag + ".eval", ds.batch(index, train=False, **flags), names)

x = torch.from_numpy(rng.integers(0, 256, (32, 3, 40, 56), dtype=np.uint8))
y = torch.from_numpy(rng.integers(0, 10, 32))
for size in (22, 24):
    for pname, kw in (("ta_wide", dict(policy="ta_wide")), ("ra", dict(policy="ra")), ("imagenet", dict(policy="imagenet"))):
        ds = D.ResizedCropDataset(x, y, MEAN, STD, size=size, device=DEV, erase_prob=0.5, **kw)
        index = torch.from_numpy(rng.integers(0, 32, 19))
        names = ("img", "targets", "params", "chain", "erase")
        flags = dict(return_params=True, return_chain_params=True, return_erase_params=True)
        box = torch.tensor([[3, 5, 30, 40, 1]] * 19, dtype=torch.int32, device=DEV)
        given = dict(params=box, chain_params=wild(rng, (19, 4, 3), 0, 15), erase_params=wild(rng, (19, 4), 0, size))
        tag = f"rc.size{size}.{pname}"
        show(tag + ".train.drawn", ds.batch(index, epoch=EPOCH, seed=SEED, **flags), names)
        show(tag + ".train.given", ds.batch(index.to(DEV), epoch=EPOCH, seed=SEED, **given, **flags), names)
        show(tag + ".eval", ds.batch(index, train=False, **flags), names)
