"""Backbones of the NBDT hot path, MI355X-native (same factory names as the reference's
``nbdt.models``: resnet.py :171-223, wideresnet.py :1-5, 28-40, __init__.py :3 efficientnet_b0 .. efficientnet_b7b, and torchvision's
lower-case resnet18 ... resnet152, resnext50_32x4d, resnext101_64x4d and wide_resnet50_2 / 101_2 that its star import of
torchvision.models brings in).  Each factory returns an
``nn.Module`` facade (see _hip_module.py) over the HIP execution engine."""
from .efficientnet import (EFFICIENTNET_NAMES, efficientnet_b0, efficientnet_b0b, efficientnet_b1, efficientnet_b1b,
                           efficientnet_b2, efficientnet_b2b, efficientnet_b3, efficientnet_b3b, efficientnet_b4,
                           efficientnet_b4b, efficientnet_b5, efficientnet_b5b, efficientnet_b6, efficientnet_b6b,
                           efficientnet_b7, efficientnet_b7b)
from .resnet import (ResNet10, ResNet18, ResNet34, ResNet50, ResNet101, ResNet152, resnet18, resnet34, resnet50, resnet101,
                     resnet152, resnext50_32x4d, resnext101_64x4d, wide_resnet50_2, wide_resnet101_2)
from .wideresnet import wrn28_10, wrn28_10_cifar10, wrn28_10_cifar100

__all__ = ("ResNet10", "ResNet18", "ResNet34", "ResNet50", "ResNet101", "ResNet152", "wrn28_10", "wrn28_10_cifar10",
           "wrn28_10_cifar100", "efficientnet_b0", "resnet18", "resnet34", "resnet50", "resnet101", "resnet152",
           "resnext50_32x4d", "resnext101_64x4d", "wide_resnet50_2", "wide_resnet101_2") + tuple(
               n for n in EFFICIENTNET_NAMES if n != "efficientnet_b0")


def get_model_choices():
    return list(__all__)
