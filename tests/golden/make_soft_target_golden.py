#!/usr/bin/env python3
"""Golden vectors for label smoothing and probability targets, from the UNMODIFIED reference on the CPU.

    PYTHONHASHSEED=0 python tests/golden/make_soft_target_golden.py <path to the reference checkout>

The recipe of make_golden.py: the reference's import-time dependencies that the rules / loss path never touches are inert
stub modules, nothing of the reference is copied, the script only calls it and records inputs and outputs.  The hash seed
must be given on the command line (the script refuses to run otherwise; it does not restart itself).

soft_targets_<tag>.npz, on the first 8 rows of z, y of rules_<tag>.npz, with xent_weight = 0.5 and
tree_supervision_weight = 10 (the `_w` configuration of make_golden.py), loss and autograd dL/dz of
  a  SoftTreeSupLoss(CrossEntropyLoss(label_smoothing=0.1))(z, y)
  b  SoftTreeSupLoss(CrossEntropyLoss())(z, t_mix),   t_mix = 0.3*onehot(y) + 0.7*roll(onehot(y), 1)   (a MixUp batch)
  c  SoftTreeSupLoss(CrossEntropyLoss(label_smoothing=0.1))(z, t_dir),  t_dir = softmax(2*randn) under a fixed seed with
     row 3 halved, so that the row sum is not 1 (torch does not normalise it); t_dir is stored
  d  HardTreeSupLoss(CrossEntropyLoss(label_smoothing=0.1))(z, y)

The reference runs in float64 here (torch's default dtype is set to float64 and the fp32 logits of rules_<tag>.npz are
widened exactly), and loss and dL/dz are stored as float64.  These fixtures are pinned to 1e-7 absolute on dL/dz, which
reaches 2.7 on the cifar10 hard case: one fp32 ulp there is 2.4e-7, so an fp32 run of the reference (1.7e-7 away from its
own float64 run on that case), or merely fp32 storage (up to 1.2e-7), cannot carry that bound.  The inputs stay fp32: z, y
and the stored t_dir are exactly what the kernels are given.
"""
import importlib.machinery
import os
import sys
import types
import warnings

if os.environ.get("PYTHONHASHSEED") != "0":
    sys.exit("run as: PYTHONHASHSEED=0 python tests/golden/make_soft_target_golden.py <reference checkout>")
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nbdt")):
    sys.exit("usage: PYTHONHASHSEED=0 python tests/golden/make_soft_target_golden.py <reference checkout>")

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
import torch.nn.functional as F  # noqa: E402

from nbdt.loss import HardTreeSupLoss, SoftTreeSupLoss  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

torch.set_num_threads(8)
torch.set_default_dtype(torch.float64)      # the reference's own constants and buffers follow the default dtype

ROWS = 8
EPS = 0.1
WEIGHTS = dict(tree_supervision_weight=10.0, xent_weight=0.5)
CASES = [
    # (tag, dataset, hierarchy, seed of t_dir)
    ("cifar10_wrn", "CIFAR10", "induced-wrn28_10_cifar10", 40),
    ("cifar100_wordnet", "CIFAR100", "wordnet", 41),
    ("tiny_r18", "TinyImagenet200", "induced-ResNet18", 42),
    ("imagenet_eff", "Imagenet1000", "induced-efficientnet_b7b", 43),
]


def loss_and_grad(crit, z, target):
    zz = z.clone().requires_grad_(True)
    loss = crit(zz, target)
    loss.backward()
    assert loss.dtype == torch.float64 and zz.grad.dtype == torch.float64
    return np.float64(loss.item()), zz.grad.numpy()


def run_case(tag, dataset, hierarchy, seed):
    src = np.load(os.path.join(HERE, f"rules_{tag}.npz"))
    z = torch.from_numpy(src["z"][:ROWS].copy()).double()
    y = torch.from_numpy(src["y"][:ROWS].copy())
    tree = Tree(dataset, hierarchy=hierarchy)
    C = len(tree.classes)
    assert z.shape == (ROWS, C)

    onehot = F.one_hot(y, C).float()                      # the target rows are fp32 values, as the kernels get them ...
    t_mix = (0.3 * onehot + 0.7 * onehot.roll(1, 0)).double()
    g = torch.Generator().manual_seed(seed)
    t_dir = torch.softmax(2.0 * torch.randn(ROWS, C, generator=g, dtype=torch.float32), dim=1)
    t_dir[3] *= 0.5
    t_dir32 = t_dir.clone()
    t_dir = t_dir.double()                                # ... widened exactly for the float64 run

    soft = lambda eps: SoftTreeSupLoss(dataset=dataset, criterion=nn.CrossEntropyLoss(label_smoothing=eps), tree=tree,
                                       **WEIGHTS)
    hard = HardTreeSupLoss(dataset=dataset, criterion=nn.CrossEntropyLoss(label_smoothing=EPS), tree=tree, **WEIGHTS)
    out = {"eps": np.float32(EPS), "t_dir": t_dir32.numpy()}
    out["loss_a"], out["dz_a"] = loss_and_grad(soft(EPS), z, y)
    out["loss_b"], out["dz_b"] = loss_and_grad(soft(0.0), z, t_mix)
    out["loss_c"], out["dz_c"] = loss_and_grad(soft(EPS), z, t_dir)
    out["loss_d"], out["dz_d"] = loss_and_grad(hard, z, y)

    path = os.path.join(HERE, f"soft_targets_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: C={C} a={out['loss_a']:.6f} b={out['loss_b']:.6f} c={out['loss_c']:.6f} d={out['loss_d']:.6f} -> "
          f"{os.path.basename(path)} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    for case in CASES:
        run_case(*case)
