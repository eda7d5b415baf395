#!/usr/bin/env python3
"""Golden vector for the Bottleneck ResNets: the `run_backbone` recipe of make_golden.py on the UNMODIFIED reference's
ResNet50 (nbdt/models/resnet.py:193-201), imported under the same stubs.

    PYTHONHASHSEED=0 python tests/golden/make_bottleneck_golden.py <path of the reference checkout>

Seed 23 -> construct -> one train-mode batch of 4 x 3x32x32 on CIFAR10 with the reference's SoftTreeSupLoss on
induced-ResNet18.  Nothing of the reference is copied; the weights are re-creatable from the seed, so the fixture
(tests/golden/backbone_resnet50_cifar10.npz) holds digests only: the state-dict key list, per-tensor parameter sums,
x, y, logits, loss, per-parameter gradient norms and two BatchNorm running statistics after the forward."""
import importlib.machinery
import os
import sys
import types
import warnings

if os.environ.get("PYTHONHASHSEED") != "0":     # (before anything touches a device: this process has opened none)
    import subprocess
    sys.exit(subprocess.call([sys.executable] + sys.argv, env=dict(os.environ, PYTHONHASHSEED="0")))

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 23


class _Stub(types.ModuleType):
    """Inert module: any attribute is a dummy class (the reference imports these packages and never calls them here)."""

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

from nbdt.loss import SoftTreeSupLoss  # noqa: E402
from nbdt.models.resnet import ResNet50  # noqa: E402

torch.set_num_threads(8)


def main():
    torch.manual_seed(SEED)
    net = ResNet50(num_classes=10)
    net.train()
    g = torch.Generator().manual_seed(SEED + 1000)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    keys = list(net.state_dict().keys())
    sums0 = np.array([float(v.double().sum()) for v in net.state_dict().values()])
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-ResNet18")
    z = net(x)
    loss = crit(z, y)
    loss.backward()
    names = [n for n, _ in net.named_parameters()]
    gnorm = np.array([float(p.grad.double().norm()) for _, p in net.named_parameters()])
    sd = net.state_dict()
    path = os.path.join(HERE, "backbone_resnet50_cifar10.npz")
    np.savez_compressed(path, keys=np.array(keys), param_sums=sums0, x=x.numpy(), y=y.numpy(), logits=z.detach().numpy(),
                        loss=np.float64(loss.item()), grad_names=np.array(names), grad_norms=gnorm,
                        bn1_running_mean=sd["bn1.running_mean"].numpy(),
                        last_running_var=sd["layer4.2.bn3.running_var"].numpy(), seed=np.int64(SEED))
    print(f"backbone resnet50 cifar10: loss {loss.item():.6f}, {len(keys)} state-dict entries -> "
          f"{os.path.basename(path)} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
