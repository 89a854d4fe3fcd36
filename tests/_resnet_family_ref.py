"""Plain ``torch.nn`` reference of the timm ResNet family with ``num_classes=0`` (TEST INFRASTRUCTURE ONLY): the
default-stem ResNet of timm ``resnet.py`` parametrised by (block, layers, groups, base_width), with timm's key names.

  BasicBlock  conv3x3(stride) bn relu conv3x3 bn (+downsample) relu
  Bottleneck  width = floor(planes * base_width / 64) * groups:
              conv1x1(inplanes -> width) bn relu conv3x3(width -> width, stride, groups) bn relu
              conv1x1(width -> 4 planes) bn (+downsample) relu
  downsample: Conv2d 1x1 stride s (no bias) + BN when the stride is not 1 or the channels change.

The blocks carry ``act1 / act2 / act3`` ReLU modules like oracle/resnet.py's, so a test can swap them for fixed masks
(teacher forcing).  Weights come from ``oracle.weights.fill_module``.
"""
from __future__ import annotations

import torch.nn as nn

# name -> (block, layers, groups, base_width, parameters with num_classes=0, num_features)
FAMILY = {
    "resnet34": ("basic", (3, 4, 6, 3), 1, 64, 21_284_672, 512),
    "resnet101": ("bottleneck", (3, 4, 23, 3), 1, 64, 42_500_160, 2048),
    "resnet152": ("bottleneck", (3, 8, 36, 3), 1, 64, 58_143_808, 2048),
    "resnet50_a2": ("bottleneck", (3, 4, 6, 3), 1, 64, 23_508_032, 2048),
    "resnet50_b": ("bottleneck", (3, 4, 6, 3), 1, 64, 23_508_032, 2048),
    "resnet50_c": ("bottleneck", (3, 4, 6, 3), 1, 64, 23_508_032, 2048),
    "wide_resnet50": ("bottleneck", (3, 4, 6, 3), 1, 128, 66_834_240, 2048),
    "wide_resnet101": ("bottleneck", (3, 4, 23, 3), 1, 128, 124_837_696, 2048),
    "resnext50": ("bottleneck", (3, 4, 6, 3), 32, 4, 22_979_904, 2048),
}


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        assert groups == 1 and base_width == 64
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.act1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.act2 = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        x = self.act1(self.bn1(self.conv1(x)))
        x = self.bn2(self.conv2(x))
        return self.act2(x + sc)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = (planes * base_width // 64) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.act1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.act2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.act3 = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        x = self.act1(self.bn1(self.conv1(x)))
        x = self.act2(self.bn2(self.conv2(x)))
        x = self.bn3(self.conv3(x))
        return self.act3(x + sc)


class ResNet(nn.Module):
    def __init__(self, kind, layers, groups=1, base_width=64):
        super().__init__()
        block = BasicBlock if kind == "basic" else Bottleneck
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.act1 = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            blocks = []
            for j in range(n):
                s = stride if j == 0 else 1
                ds = None
                if j == 0 and (s != 1 or inplanes != planes * block.expansion):
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, stride=s, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(inplanes, planes, s, ds, groups, base_width))
                inplanes = planes * block.expansion
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.num_features = inplanes

    def forward(self, x):
        x = self.maxpool(self.act1(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return x.mean((2, 3))


def create(name: str) -> ResNet:
    kind, layers, groups, base_width, _, _ = FAMILY[name]
    return ResNet(kind, layers, groups, base_width)
