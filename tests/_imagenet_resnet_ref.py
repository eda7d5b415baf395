"""fp32 PyTorch restatement of torchvision.models.resnet (the ImageNet-style ResNets the reference's ImageNet recipe trains:
its nbdt/models/__init__.py star-imports torchvision.models), the oracle of ImageNetResNetEngine / ImageNetBottleneckEngine.
Written from torchvision's published structure -- torchvision is not a dependency of this repository:

  conv1 7x7 / 2 / pad 3 (no bias) -> bn1 -> ReLU -> MaxPool2d(3, 2, 1) -> layer1..4 -> global average pool -> fc

BasicBlock: conv1 3x3 (stride s) -> bn1 -> ReLU -> conv2 3x3 -> bn2, + identity, ReLU.  Bottleneck (v1.5, the stride on the
3x3 conv): conv1 1x1 -> conv2 3x3 (stride s) -> conv3 1x1 (x 4).  ``downsample`` = Sequential(conv 1x1 / s, BatchNorm) where
the shape changes.  Initialisation as torchvision's: kaiming_normal_(fan_out, relu) for convs, 1 / 0 for BatchNorm, and
zero_init_residual zeroes each block's last BatchNorm weight.  tests/test_imagenet_resnet.py pins the parameter counts and
shapes to torchvision's published ones."""
import torch.nn as nn
import torch.nn.functional as F

STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))     # (planes, stride of the stage's first block)


def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


def _downsample(cin, cout, stride):
    return nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout)) if stride != 1 or cin != cout else None


class BasicBlock(nn.Module):
    expansion = 1
    last_bn = "bn2"

    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv(cin, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3), nn.BatchNorm2d(planes)
        self.downsample = _downsample(cin, planes, stride)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class Bottleneck(nn.Module):
    expansion = 4
    last_bn = "bn3"

    def __init__(self, cin, planes, stride):
        super().__init__()
        cout = self.expansion * planes
        self.conv1, self.bn1 = _conv(cin, planes, 1), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = _conv(planes, cout, 1), nn.BatchNorm2d(cout)
        self.downsample = _downsample(cin, cout, stride)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    def __init__(self, block, num_blocks, num_classes=1000, zero_init_residual=False):
        super().__init__()
        self.conv1, self.bn1 = _conv(3, 64, 7, 2), nn.BatchNorm2d(64)
        cin = 64
        for i, ((planes, stride), n) in enumerate(zip(STAGES, num_blocks)):
            blocks = []
            for j in range(n):
                blocks.append(block(cin, planes, stride if j == 0 else 1))
                cin = block.expansion * planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.fc = nn.Linear(cin, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, (BasicBlock, Bottleneck)):
                    nn.init.zeros_(getattr(m, m.last_bn).weight)

    def stem(self, x):
        """conv1 -> bn1 -> ReLU (before the pool)."""
        return F.relu(self.bn1(self.conv1(x)))

    def forward(self, x):
        y = F.max_pool2d(self.stem(x), 3, 2, 1)
        for i in range(len(STAGES)):
            y = getattr(self, f"layer{i + 1}")(y)
        return self.fc(y.mean((2, 3)))


DEPTHS = {"resnet18": (BasicBlock, (2, 2, 2, 2)), "resnet34": (BasicBlock, (3, 4, 6, 3)),
          "resnet50": (Bottleneck, (3, 4, 6, 3)), "resnet101": (Bottleneck, (3, 4, 23, 3)),
          "resnet152": (Bottleneck, (3, 8, 36, 3))}


def make(name, num_classes=1000, num_blocks=None, **kwargs):
    block, depth = DEPTHS[name]
    return ResNet(block, num_blocks or depth, num_classes, **kwargs)
