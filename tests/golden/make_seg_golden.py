#!/usr/bin/env python3
"""Golden vectors for the segmentation classes, from the UNMODIFIED reference on the CPU.

    PYTHONHASHSEED=0 python tests/golden/make_seg_golden.py <path to the reference checkout>

The recipe of make_soft_target_golden.py: the reference's import-time dependencies that the rules / loss path never
touches are inert stub modules, nothing of the reference is copied into this script, it only calls the reference and
records inputs and outputs.  The hash seed must be given on the command line.

The three segmentation hierarchies the reference can load as it stands (it has no wnids/Cityscapes.txt) are copied, as
data, to tests/golden/seg_hierarchies/ (graph JSON and wnid list per dataset), and seg_<tag>.npz records per dataset
  z          [2, C, 5, 13] fp32, seeded: H*W = 65 is one full wave of pixels and a one-pixel tail per image
  y          [2, 5, 13] int64: the first two rows of image 0 are 255, image 1 is 255 except one pixel
  y_none     all 255
  soft       SoftSegNBDT(model = identity)(z)                       float64 [2, C, 5, 13]
  hard       HardSegNBDT(model = identity)(z).argmax(1)             int64 [2, 5, 13]
  loss_a, dz_a   SoftSegTreeSupLoss(CrossEntropyLoss(ignore_index=255), tree_supervision_weight=10)(z, y) and dL/dz
  loss_b, dz_b   the same with label_smoothing=0.1
  loss_none, dz_none   criterion a on y_none: whatever the reference returns when no pixel is valid
The reference runs in float64 (default dtype float64, the fp32 logits widened exactly); losses and gradients are stored
as float64.
"""
import importlib.machinery
import os
import shutil
import sys
import types
import warnings

if os.environ.get("PYTHONHASHSEED") != "0":
    sys.exit("run as: PYTHONHASHSEED=0 python tests/golden/make_seg_golden.py <reference checkout>")
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nbdt")):
    sys.exit("usage: PYTHONHASHSEED=0 python tests/golden/make_seg_golden.py <reference checkout>")

REF = os.path.abspath(sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))


class _Stub(types.ModuleType):
    """Inert module: any attribute is a dummy class."""

    def __init__(self, name):
        super().__init__(name)
        self.__path__ = []
        self.__all__ = []
        self.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return type(item, (), {})


for name in ["torchvision", "torchvision.datasets", "torchvision.transforms", "torchvision.models",
             "pytorchcv", "pytorchcv.models", "pytorchcv.models.wrn_cifar", "pytorchcv.models.efficientnet",
             "nltk", "nltk.corpus"]:
    sys.modules[name] = _Stub(name)

sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from nbdt.loss import SoftSegTreeSupLoss  # noqa: E402
from nbdt.model import HardSegNBDT, SoftSegNBDT  # noqa: E402

torch.set_num_threads(8)
torch.set_default_dtype(torch.float64)

IGNORE = 255
EPS = 0.1
TSW = 10.0
CASES = [
    # (tag, dataset, hierarchy, classes, seed)
    ("lip", "LookIntoPerson", "induced-HRNet-w48-cls20", 20, 50),
    ("pascal", "PascalContext", "induced-HRNet-w48-cls59", 59, 51),
    ("ade20k", "ADE20K", "induced-HRNet-w48", 150, 52),
]


def loss_and_grad(crit, z, y):
    zz = z.clone().requires_grad_(True)
    loss = crit(zz, y)
    if loss.requires_grad:
        loss.backward()
    grad = zz.grad if zz.grad is not None else torch.zeros_like(zz)
    return np.float64(loss.item()), grad.numpy().astype(np.float64)


def run_case(tag, dataset, hierarchy, C, seed):
    dst = os.path.join(HERE, "seg_hierarchies")
    os.makedirs(dst, exist_ok=True)
    graph = os.path.join(REF, "nbdt", "hierarchies", dataset, f"graph-{hierarchy}.json")
    wnids = os.path.join(REF, "nbdt", "wnids", f"{dataset}.txt")
    shutil.copyfile(graph, os.path.join(dst, f"{dataset}-graph-{hierarchy}.json"))
    shutil.copyfile(wnids, os.path.join(dst, f"{dataset}-wnids.txt"))

    g = torch.Generator().manual_seed(seed)
    z32 = 3.0 * torch.randn(2, C, 5, 13, generator=g, dtype=torch.float32)
    y = torch.randint(0, C, (2, 5, 13), generator=g)
    y[0, :2] = IGNORE
    keep = int(y[1, 3, 7])
    y[1] = IGNORE
    y[1, 3, 7] = keep
    y_none = torch.full_like(y, IGNORE)
    z = z32.double()

    kw = dict(dataset=dataset, hierarchy=hierarchy)
    with torch.no_grad():
        soft = SoftSegNBDT(model=nn.Identity(), **kw)(z)
        hard = HardSegNBDT(model=nn.Identity(), **kw)(z)
    assert soft.shape == z.shape and hard.shape == z.shape
    crit = lambda eps: SoftSegTreeSupLoss(criterion=nn.CrossEntropyLoss(ignore_index=IGNORE, label_smoothing=eps),
                                          tree_supervision_weight=TSW, **kw)
    out = {"z": z32.numpy(), "y": y.numpy(), "y_none": y_none.numpy(), "eps": np.float32(EPS),
           "soft": soft.numpy().astype(np.float64), "hard": hard.argmax(1).numpy().astype(np.int64)}
    out["loss_a"], out["dz_a"] = loss_and_grad(crit(0.0), z, y)
    out["loss_b"], out["dz_b"] = loss_and_grad(crit(EPS), z, y)
    out["loss_none"], out["dz_none"] = loss_and_grad(crit(0.0), z, y_none)

    path = os.path.join(HERE, f"seg_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: C={C} a={out['loss_a']:.6f} b={out['loss_b']:.6f} none={out['loss_none']} "
          f"|dz_none|max={np.abs(out['dz_none']).max()} -> {os.path.basename(path)} "
          f"({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    for case in CASES:
        run_case(*case)
