"""Plain ``torch.nn`` restatement of timm's ResNet-RS and ResNet-50-D with ``num_classes=0`` (TEST INFRASTRUCTURE
ONLY), written from the architecture description (timm ``resnet.py``), with timm's key names.

  stem       deep: conv1 = Sequential(conv3x3 s2 3->32, BN, ReLU, conv3x3 32->32, BN, ReLU, conv3x3 32->64), bn1, act1
  stem pool  resnetrs*: maxpool = Sequential(conv3x3 s2 64->64, BN, ReLU);  resnet50_d: MaxPool2d(3, 2, 1)
  Bottleneck conv1x1 bn relu conv3x3(stride) bn relu conv1x1 bn [se] (+shortcut) relu
  se         x * sigmoid(fc2(relu(fc1(mean_hw x)))), fc1 = Conv2d(C, C/4, 1, bias), fc2 = Conv2d(C/4, C, 1, bias)
  shortcut   first block of each layer: Sequential(pool, conv1x1 stride 1, BN), pool = Identity (stride 1) or
             AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)

The blocks carry ``act1 / act2 / act3`` ReLU modules so a test can swap them for fixed masks (teacher forcing).
Weights come from ``oracle.weights.fill_module``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

# name -> (layers, squeeze-excitation, conv stem pool, parameters with num_classes=0, num_features); the ResNet-RS counts
# are timm's published totals minus the 2,049,000 of the 1000-class head, resnet50_d's is timm's 25,576,264 minus the same
CFGS = {
    "resnetrs50": ((3, 4, 6, 3), True, True, 33_642_912, 2048),
    "resnetrs101": ((3, 4, 23, 3), True, True, 61_569_696, 2048),
    "resnetrs152": ((3, 8, 36, 3), True, True, 84_572_576, 2048),
    "resnet50_d": ((3, 4, 6, 3), False, False, 23_527_264, 2048),
}


class SE(nn.Module):
    def __init__(self, channels, rd_channels):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, rd_channels, 1, bias=True)
        self.fc2 = nn.Conv2d(rd_channels, channels, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.fc2(torch.relu(self.fc1(s))))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, se=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.act1 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.act2 = nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.se = SE(planes * 4, planes) if se else None
        self.act3 = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        x = self.act1(self.bn1(self.conv1(x)))
        x = self.act2(self.bn2(self.conv2(x)))
        x = self.bn3(self.conv3(x))
        if self.se is not None:
            x = self.se(x)
        return self.act3(x + sc)


class ResNet(nn.Module):
    def __init__(self, layers, se=True, conv_pool=True):
        super().__init__()
        self.conv1 = nn.Sequential(
            nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(32, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(32, 64, 3, padding=1, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        self.act1 = nn.ReLU(inplace=True)
        if conv_pool:
            self.maxpool = nn.Sequential(nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(64),
                                         nn.ReLU(inplace=True))
        else:
            self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            blocks = []
            for j in range(n):
                s = stride if j == 0 else 1
                ds = None
                if j == 0:
                    pool = nn.Identity() if s == 1 else nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)
                    ds = nn.Sequential(pool, nn.Conv2d(inplanes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4))
                blocks.append(Bottleneck(inplanes, planes, s, ds, se))
                inplanes = planes * 4
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.num_features = inplanes

    def forward(self, x):
        x = self.maxpool(self.act1(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return x.mean((2, 3))


def create(name: str, layers=None) -> ResNet:
    """``layers``: a shallower copy of the same configuration (the GPU tests run (1, 1, 1, 1))."""
    full, se, conv_pool, _, _ = CFGS[name]
    return ResNet(layers or full, se, conv_pool)
