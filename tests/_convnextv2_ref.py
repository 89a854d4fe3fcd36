"""fp32 CPU restatement of timm 1.0.22 ConvNeXt V2 (Linear-MLP variants, num_classes=0) for the V2 tests: the V1
oracle's stem, stages and head (oracle/convnext.py) with V2 blocks -- no layer-scale ``gamma``, and Global Response
Normalization (``mlp.grn.{weight,bias}``) between GELU and fc2.  timm-keyed, so one generated state dict feeds this
module, the HIP backbone and (after a key remap) HF transformers' ConvNextV2Model."""

from __future__ import annotations

import torch
import torch.nn as nn

from oracle import convnext as oc

CFGS = {"convnextv2_base": oc.CFGS["convnext_base"], "convnextv2_large": oc.CFGS["convnext_large"]}


class GRN(nn.Module):
    """timm GlobalResponseNorm, channels-last: x + bias + weight * x * (G / (mean_c G + eps)), G = ||x||_2 over (H, W)."""

    def __init__(self, dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):  # [B, H, W, n]
        g = x.norm(p=2, dim=(1, 2), keepdim=True)
        n = g / (g.mean(dim=-1, keepdim=True) + self.eps)
        return x + torch.addcmul(self.bias, self.weight, x * n)


class GrnMlp(nn.Module):
    def __init__(self, dim: int, hidden: int) -> None:
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.grn = GRN(hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.grn(self.act(self.fc1(x))))


class Block(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = GrnMlp(dim, 4 * dim)

    def forward(self, x):
        y = self.mlp(self.norm(self.conv_dw(x).permute(0, 2, 3, 1)))
        return y.permute(0, 3, 1, 2) + x


def create(name: str) -> oc.ConvNeXt:
    depths, dims = CFGS[name.split(".")[0]]
    model = oc.ConvNeXt(depths, dims)
    for st, d, c in zip(model.stages, depths, dims):
        st.blocks = nn.Sequential(*[Block(c) for _ in range(d)])
    return model
