"""CIFAR ResNets -- reference nbdt/models/resnet.py: BasicBlock variants (:42-74, 115-149, 161-199) on ResNetEngine,
Bottleneck variants (:77-112, 193-223) on BottleneckEngine -- and the ImageNet-style ResNets the reference takes from
torchvision.models (nbdt/models/__init__.py: resnet18 ... resnet152, resnext50_32x4d, resnext101_64x4d, wide_resnet50_2,
wide_resnet101_2, lower-case) on the ImageNet* engines."""
from nbdt.engine import BottleneckEngine, ImageNetBottleneckEngine, ImageNetResNetEngine, ResNetEngine
from nbdt.models._hip_module import HipBackbone


def _resnet(num_blocks, num_classes=10, pretrained=False, progress=True, dataset="CIFAR10", device="cuda", seed=0,
            engine=ResNetEngine):
    if pretrained:
        raise NotImplementedError("pretrained checkpoints need network access; use load_state_dict")
    return HipBackbone(engine(num_classes=num_classes, num_blocks=num_blocks, device=device, seed=seed))


def ResNet10(**kwargs):
    return _resnet((1, 1, 1, 1), **kwargs)


def ResNet18(**kwargs):
    return _resnet((2, 2, 2, 2), **kwargs)


def ResNet34(**kwargs):
    return _resnet((3, 4, 6, 3), **kwargs)


def ResNet50(**kwargs):
    return _resnet((3, 4, 6, 3), engine=BottleneckEngine, **kwargs)


def ResNet101(**kwargs):
    return _resnet((3, 4, 23, 3), engine=BottleneckEngine, **kwargs)


def ResNet152(**kwargs):
    return _resnet((3, 8, 36, 3), engine=BottleneckEngine, **kwargs)


def _tv_resnet(engine, num_blocks, pretrained=False, progress=True, num_classes=1000, zero_init_residual=False,
               dataset="Imagenet1000", device="cuda", seed=0, **block_kw):
    if pretrained:
        raise NotImplementedError("pretrained checkpoints need network access; use load_state_dict")
    return HipBackbone(engine(num_classes=num_classes, num_blocks=num_blocks, zero_init_residual=zero_init_residual,
                              device=device, seed=seed, **block_kw))


def resnet18(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetResNetEngine, (2, 2, 2, 2), pretrained, **kwargs)


def resnet34(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetResNetEngine, (3, 4, 6, 3), pretrained, **kwargs)


def resnet50(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 6, 3), pretrained, **kwargs)


def resnet101(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 23, 3), pretrained, **kwargs)


def resnet152(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 8, 36, 3), pretrained, **kwargs)


# torchvision.models.resnet's other half: the Bottleneck with groups / width_per_group (torchvision fixes the two per
# factory and takes the remaining keywords; resnext101_32x8d -- 64 channels per group in layer4 -- is not offered)
def resnext50_32x4d(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 6, 3), pretrained, groups=32, width_per_group=4, **kwargs)


def resnext101_64x4d(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 23, 3), pretrained, groups=64, width_per_group=4, **kwargs)


def wide_resnet50_2(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 6, 3), pretrained, width_per_group=128, **kwargs)


def wide_resnet101_2(pretrained=False, **kwargs):
    return _tv_resnet(ImageNetBottleneckEngine, (3, 4, 23, 3), pretrained, width_per_group=128, **kwargs)
