"""Plain ``torch.nn`` restatement of timm's ``efficientnet_b0`` .. ``efficientnet_b4`` (non-``tf_``) with
``num_classes=0`` (TEST INFRASTRUCTURE ONLY), written from the architecture description, with timm's key names.

  stem        conv_stem 3x3 s2 (no bias), bn1, SiLU
  ds          DepthwiseSeparable: conv_dw depthwise k x k (stride), bn1, SiLU, se (rd = in / 4), conv_pw 1x1, bn2, + x
  ir          InvertedResidual: conv_pw 1x1 to in * e, bn1, SiLU, conv_dw depthwise k x k (stride), bn2, SiLU,
              se: x * sigmoid(conv_expand(silu(conv_reduce(mean_hw x)))) with rd = in / 4, conv_pwl 1x1, bn3, + x
  head        conv_head 1x1 to num_features, bn2, SiLU, global average pool
  skip        when stride == 1 and in == out; BatchNorm eps 1e-5, momentum 0.1; symmetric padding k // 2
  scaling     widths round_channels(c w, 8, round_limit 0.9), repeats ceil(r d); the tables below are written out
"""
from __future__ import annotations

import torch.nn as nn
import torch.nn.functional as F

from _effnetv2_ref import SE, init_goog  # noqa: F401  (init_goog: timm _init_weight_goog, re-exported)

_T = ("ds", "ir", "ir", "ir", "ir", "ir", "ir")
_K = (3, 3, 5, 3, 5, 5, 3)
_S = (1, 2, 2, 2, 1, 2, 1)
_E = (1, 6, 6, 6, 6, 6, 6)


def _stages(widths, repeats):
    return tuple(zip(_T, repeats, _K, _S, _E, widths))


# name -> (stem, stages (type, repeats, kernel, stride, expansion, out), num_features, parameters with num_classes=0)
CFGS = {
    "efficientnet_b0": (32, _stages((16, 24, 40, 80, 112, 192, 320), (1, 2, 2, 3, 3, 4, 1)), 1280, 4_007_548),
    "efficientnet_b1": (32, _stages((16, 24, 40, 80, 112, 192, 320), (2, 3, 3, 4, 4, 5, 2)), 1280, 6_513_184),
    "efficientnet_b2": (32, _stages((16, 24, 48, 88, 120, 208, 352), (2, 3, 3, 4, 4, 5, 2)), 1408, 7_700_994),
    "efficientnet_b3": (40, _stages((24, 32, 48, 96, 136, 232, 384), (2, 3, 3, 5, 5, 6, 2)), 1536, 10_696_232),
    "efficientnet_b4": (48, _stages((24, 32, 56, 112, 160, 272, 448), (2, 4, 4, 6, 6, 8, 2)), 1792, 17_548_616),
}


def shallow(name: str, repeats) -> tuple:
    """the stage table of ``name`` with other repeat counts (same types, kernels, widths, strides and expansions)"""
    return tuple((t, r, k, s, e, c) for (t, _, k, s, e, c), r in zip(CFGS[name][1], repeats))


class DepthwiseSeparable(nn.Module):
    def __init__(self, cin, cout, stride, k):
        super().__init__()
        self.conv_dw = nn.Conv2d(cin, cin, k, stride=stride, padding=k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.se = SE(cin, int(cin / 4 + 0.5))
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.skip = stride == 1 and cin == cout

    def forward(self, x):
        y = self.se(F.silu(self.bn1(self.conv_dw(x))))
        y = self.bn2(self.conv_pw(y))
        return y + x if self.skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, e, k):
        super().__init__()
        mid = cin * e
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride=stride, padding=k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = SE(mid, int(cin / 4 + 0.5))
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.skip = stride == 1 and cin == cout

    def forward(self, x):
        y = F.silu(self.bn1(self.conv_pw(x)))
        y = self.se(F.silu(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.skip else y


class EfficientNet(nn.Module):
    def __init__(self, stem, stages, num_features):
        super().__init__()
        self.conv_stem = nn.Conv2d(3, stem, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem)
        cin, mods = stem, []
        for kind, repeats, k, stride, e, cout in stages:
            blocks = []
            for i in range(repeats):
                s = stride if i == 0 else 1
                blocks.append(DepthwiseSeparable(cin, cout, s, k) if kind == "ds" else InvertedResidual(cin, cout, s, e, k))
                cin = cout
            mods.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*mods)
        self.conv_head = nn.Conv2d(cin, num_features, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(num_features)
        self.num_features = num_features

    def block_list(self):
        return [b for stage in self.blocks for b in stage]

    def forward(self, x):
        x = F.silu(self.bn1(self.conv_stem(x)))
        x = self.blocks(x)
        return F.silu(self.bn2(self.conv_head(x))).mean((2, 3))


def create(name: str, stages=None) -> EfficientNet:
    stem, full, nf, _ = CFGS[name]
    return EfficientNet(stem, full if stages is None else stages, nf)
