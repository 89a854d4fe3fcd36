"""Plain ``torch.nn`` restatement of timm's ``efficientnetv2_s / m / l`` (non-``tf_``, non-``rw``) with
``num_classes=0`` (TEST INFRASTRUCTURE ONLY), written from the architecture description, with timm's key names.

  stem        conv_stem 3x3 s2 (no bias), bn1, SiLU
  cn          ConvBnAct: conv 3x3, bn1, SiLU, then + x (the skip is added AFTER the activation)
  er          EdgeResidual: conv_exp 3x3 (stride) to in * e, bn1, SiLU, conv_pwl 1x1, bn2, + x
  ir          InvertedResidual: conv_pw 1x1 to in * e, bn1, SiLU, conv_dw depthwise 3x3 (stride), bn2, SiLU,
              se: x * sigmoid(conv_expand(silu(conv_reduce(mean_hw x)))) with rd = in / 4, conv_pwl 1x1, bn3, + x
  head        conv_head 1x1 to 1280, bn2, SiLU, global average pool
  skip        when stride == 1 and in == out; BatchNorm eps 1e-5, momentum 0.1; symmetric padding k // 2

Weights come from ``oracle.weights.fill_module`` or ``init_goog`` (timm ``_init_weight_goog``).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

# name -> (stem, stages (type, repeats, stride, expansion, out), parameters with num_classes=0, blocks)
CFGS = {
    "efficientnetv2_s": (24, (("cn", 2, 1, 1, 24), ("er", 4, 2, 4, 48), ("er", 4, 2, 4, 64), ("ir", 6, 2, 4, 128),
                              ("ir", 9, 1, 6, 160), ("ir", 15, 2, 6, 256)), 20_177_488, 40),
    "efficientnetv2_m": (24, (("cn", 3, 1, 1, 24), ("er", 5, 2, 4, 48), ("er", 5, 2, 4, 80), ("ir", 7, 2, 4, 160),
                              ("ir", 14, 1, 6, 176), ("ir", 18, 2, 6, 304), ("ir", 5, 1, 6, 512)), 52_858_356, 57),
    "efficientnetv2_l": (32, (("cn", 4, 1, 1, 32), ("er", 7, 2, 4, 64), ("er", 7, 2, 4, 96), ("ir", 10, 2, 4, 192),
                              ("ir", 19, 1, 6, 224), ("ir", 25, 2, 6, 384), ("ir", 7, 1, 6, 640)), 117_234_272, 79),
}


def shallow(name: str, repeats) -> tuple:
    """the stage table of ``name`` with other repeat counts (same widths, strides and expansions)"""
    return tuple((k, r, s, e, c) for (k, _, s, e, c), r in zip(CFGS[name][1], repeats))


class ConvBnAct(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.skip = stride == 1 and cin == cout

    def forward(self, x):
        y = F.silu(self.bn1(self.conv(x)))
        return y + x if self.skip else y


class EdgeResidual(nn.Module):
    def __init__(self, cin, cout, stride, e):
        super().__init__()
        self.conv_exp = nn.Conv2d(cin, cin * e, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cin * e)
        self.conv_pwl = nn.Conv2d(cin * e, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.skip = stride == 1 and cin == cout

    def forward(self, x):
        y = self.bn2(self.conv_pwl(F.silu(self.bn1(self.conv_exp(x)))))
        return y + x if self.skip else y


class SE(nn.Module):
    def __init__(self, channels, rd):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, rd, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd, channels, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.conv_expand(F.silu(self.conv_reduce(s))))


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, e):
        super().__init__()
        mid = cin * e
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, 3, stride=stride, padding=1, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = SE(mid, cin // 4)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.skip = stride == 1 and cin == cout

    def forward(self, x):
        y = F.silu(self.bn1(self.conv_pw(x)))
        y = self.se(F.silu(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.skip else y


class EfficientNetV2(nn.Module):
    def __init__(self, stem, stages):
        super().__init__()
        self.conv_stem = nn.Conv2d(3, stem, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem)
        cin, mods = stem, []
        for kind, repeats, stride, e, cout in stages:
            blocks = []
            for i in range(repeats):
                s = stride if i == 0 else 1
                blocks.append(ConvBnAct(cin, cout, s) if kind == "cn" else EdgeResidual(cin, cout, s, e) if kind == "er"
                              else InvertedResidual(cin, cout, s, e))
                cin = cout
            mods.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*mods)
        self.conv_head = nn.Conv2d(cin, 1280, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(1280)
        self.num_features = 1280

    def block_list(self):
        return [b for stage in self.blocks for b in stage]

    def forward(self, x):
        x = F.silu(self.bn1(self.conv_stem(x)))
        x = self.blocks(x)
        return F.silu(self.bn2(self.conv_head(x))).mean((2, 3))


def init_goog(m: nn.Module) -> nn.Module:
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            fan_out = mod.kernel_size[0] * mod.kernel_size[1] * mod.out_channels // mod.groups
            nn.init.normal_(mod.weight, 0.0, (2.0 / fan_out) ** 0.5)
            if mod.bias is not None:
                nn.init.zeros_(mod.bias)
        elif isinstance(mod, nn.BatchNorm2d):
            nn.init.ones_(mod.weight)
            nn.init.zeros_(mod.bias)
    return m


def create(name: str, stages=None) -> EfficientNetV2:
    stem, full, _, _ = CFGS[name]
    return EfficientNetV2(stem, full if stages is None else stages)
