"""fp32 PyTorch restatement of the other half of torchvision.models.resnet: the Bottleneck with ``groups`` and
``width_per_group`` (resnext50_32x4d, resnext101_64x4d, wide_resnet50_2, wide_resnet101_2), the oracle of
ImageNetBottleneckEngine(groups=..., width_per_group=...).  Written from torchvision's published structure -- torchvision is
not a dependency of this repository -- on top of tests/_imagenet_resnet_ref.py (stem, stages, head, initialisation):

  width = int(planes * width_per_group / 64) * groups
  conv1 1x1 cin -> width, conv2 3x3 width -> width (stride s, groups), conv3 1x1 width -> 4 planes

conv2 is F.conv2d(..., groups=groups) through nn.Conv2d, so its weight is [width, width / groups, 3, 3] and
kaiming_normal_(mode="fan_out") gives it std sqrt(2 / (width * 9)): torch takes fan_out from the tensor's shape."""
import os
import sys

import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _imagenet_resnet_ref as R  # noqa: E402


class Bottleneck(nn.Module):
    expansion = 4
    last_bn = "bn3"

    def __init__(self, cin, planes, stride, groups=1, width_per_group=64):
        super().__init__()
        width = int(planes * width_per_group / 64) * groups
        cout = self.expansion * planes
        self.conv1, self.bn1 = R._conv(cin, width, 1), nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3, self.bn3 = R._conv(width, cout, 1), nn.BatchNorm2d(cout)
        self.downsample = R._downsample(cin, cout, stride)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    def __init__(self, num_blocks, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64):
        super().__init__()
        self.conv1, self.bn1 = R._conv(3, 64, 7, 2), nn.BatchNorm2d(64)
        cin = 64
        for i, ((planes, stride), n) in enumerate(zip(R.STAGES, num_blocks)):
            blocks = []
            for j in range(n):
                blocks.append(Bottleneck(cin, planes, stride if j == 0 else 1, groups, width_per_group))
                cin = Bottleneck.expansion * planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.fc = nn.Linear(cin, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)

    def forward(self, x):
        y = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        for i in range(len(R.STAGES)):
            y = getattr(self, f"layer{i + 1}")(y)
        return self.fc(y.mean((2, 3)))


# name -> (depth, groups, width_per_group): torchvision's factories
ARCHS = {"resnext50_32x4d": ((3, 4, 6, 3), 32, 4), "resnext101_64x4d": ((3, 4, 23, 3), 64, 4),
         "wide_resnet50_2": ((3, 4, 6, 3), 1, 128), "wide_resnet101_2": ((3, 4, 23, 3), 1, 128)}
# torchvision's model cards
PARAMS = {"resnext50_32x4d": 25028904, "resnext101_64x4d": 83455272, "wide_resnet50_2": 68883240,
          "wide_resnet101_2": 126886696}


def make(name, num_classes=1000, num_blocks=None, **kwargs):
    depth, groups, wpg = ARCHS[name]
    return ResNet(num_blocks or depth, num_classes, groups=groups, width_per_group=wpg, **kwargs)
