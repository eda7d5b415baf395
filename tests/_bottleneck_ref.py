"""fp32 PyTorch restatement of the reference's CIFAR Bottleneck ResNets (nbdt/models/resnet.py:77-112 Bottleneck,
:115-149 ResNet, :193-223 ResNet50 / 101 / 152), the oracle of BottleneckEngine: a 3x3 stem, four stages of
1x1 -> 3x3 (stride s) -> 1x1 (x 4) blocks with a projection shortcut wherever the shape changes, global average pool,
``linear``.  Modules are created in the reference's order (conv1, bn1, conv2, bn2, conv3, bn3, shortcut), so that a seed
gives the reference's parameters under the reference's state-dict names; tests/test_bottleneck.py pins that to
tests/golden/backbone_resnet50_cifar10.npz, which tests/golden/make_bottleneck_golden.py recorded from the reference."""
import torch.nn as nn
import torch.nn.functional as F

EXPANSION = 4
STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))     # (planes, stride of the stage's first block)


def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


class _Bottleneck(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        cout = EXPANSION * planes
        self.conv1, self.bn1 = _conv(cin, planes, 1), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = _conv(planes, cout, 1), nn.BatchNorm2d(cout)
        project = stride != 1 or cin != cout
        self.shortcut = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout)) if project else nn.Sequential()

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return F.relu(y + self.shortcut(x))


class BottleneckResNet(nn.Module):
    def __init__(self, num_blocks, num_classes=10):
        super().__init__()
        self.conv1, self.bn1 = _conv(3, 64, 3), nn.BatchNorm2d(64)
        cin = 64
        for i, ((planes, stride), n) in enumerate(zip(STAGES, num_blocks)):
            blocks = []
            for j in range(n):
                blocks.append(_Bottleneck(cin, planes, stride if j == 0 else 1))
                cin = EXPANSION * planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.linear = nn.Linear(cin, num_classes)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        for i in range(len(STAGES)):
            y = getattr(self, f"layer{i + 1}")(y)
        return self.linear(y.mean((2, 3)))


def ResNet50(num_classes=10):
    return BottleneckResNet((3, 4, 6, 3), num_classes)


def ResNet101(num_classes=10):
    return BottleneckResNet((3, 4, 23, 3), num_classes)


def ResNet152(num_classes=10):
    return BottleneckResNet((3, 8, 36, 3), num_classes)
