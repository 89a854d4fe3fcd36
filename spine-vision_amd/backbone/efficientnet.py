"""EfficientNetV2-S / M / L backbone on the gfx950 kernel library -- drop-in for
``timm.create_model("efficientnetv2_{s,m,l}", num_classes=0)`` (timm ``efficientnet.py`` ``_gen_efficientnetv2_*``, the
non-``tf_``, non-``rw`` variants: symmetric padding k // 2, BatchNorm eps 1e-5, SiLU, drop-path 0) -- and, on the same
block routines, EfficientNet-B0 .. B4 (``EfficientNetHip`` at the end of the file: ``efficientnet_b{0..4}``, the
``DepthwiseSeparable`` first stage, 5x5 depthwise convolutions on csrc/dwconv5.hip, every stored channel stride a
multiple of 32 and every squeeze-and-excitation hidden width a multiple of 4, zero-padded as described below).

* Same module tree / ``state_dict`` keys as timm: ``conv_stem``, ``bn1``, ``blocks.{stage}.{i}.*``, ``conv_head``,
  ``bn2``; ConvBnAct (``conv``, ``bn1``), EdgeResidual (``conv_exp``, ``bn1``, ``conv_pwl``, ``bn2``) and InvertedResidual
  (``conv_pw``, ``bn1``, ``conv_dw``, ``bn2``, ``se.conv_reduce``, ``se.conv_expand``, ``conv_pwl``, ``bn3``).
  Sub-modules are parameter / buffer containers; their own ``forward`` is never called.  ``num_features`` = 1280,
  ``forward([B,3,H,W] f32 | [B,H,W,3] uint8) -> [B,1280]``, any input size.
* Every 1x1 convolution is a row-major GEMM over the NHWC rows (``sv_gemm``); the depthwise 3x3, BatchNorm + SiLU and
  the squeeze-and-excitation that gates the expanded activation run on csrc/mbconv.hip (``K.dwconv3_*``,
  ``K.bn_silu_*``, ``K.mbse_*``); the dense 3x3 convolutions (stem, ConvBnAct, ``conv_exp``) go through the ``sv_conv_*``
  entry points the ResNets use, unchanged.  Those need power-of-two channel counts, so the tensors they touch are stored
  with their channel stride padded to a power of two (>= 32): padded weight rows / columns are zero, padded BatchNorm
  gamma / beta are zero, so the padded channels are exactly zero through BatchNorm and SiLU; parameters, buffers and
  ``state_dict`` hold the real channels only and the gradients of padded rows are discarded.
* Backward is an explicit kernel sequence writing the parameter gradients into ``p.grad`` and calling
  ``grad_ready_hook`` after each block; the GEMM / conv weight gradients run on a side stream.
* ``precision="bf16"``: bf16 MFMA, bf16 activations and gradient stream, f32 statistics and master weights;
  ``precision="fp32"``: f32 everywhere (parity mode).
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Callable

import torch
import torch.nn as nn

from .. import kernels as K
from .. import native as nv
from ._explicit import ExplicitBackward

# SV_EFFNET_EPI_STATS=0: the BatchNorm statistics of the 1x1 convolutions from their own pass instead of the GEMM
# epilogue (SV_EPI_STORE_STATS; bf16, K % 32 == 0 and N % 32 == 0) (A/B runs)
_EPI_STATS = os.environ.get("SV_EFFNET_EPI_STATS", "1") != "0"

# name -> (stem width, ((type, repeats, stride of the first block, expansion, out channels), ...))
EFFNETV2_CFGS = {
    "efficientnetv2_s": (24, (("cn", 2, 1, 1, 24), ("er", 4, 2, 4, 48), ("er", 4, 2, 4, 64), ("ir", 6, 2, 4, 128),
                              ("ir", 9, 1, 6, 160), ("ir", 15, 2, 6, 256))),
    "efficientnetv2_m": (24, (("cn", 3, 1, 1, 24), ("er", 5, 2, 4, 48), ("er", 5, 2, 4, 80), ("ir", 7, 2, 4, 160),
                              ("ir", 14, 1, 6, 176), ("ir", 18, 2, 6, 304), ("ir", 5, 1, 6, 512))),
    "efficientnetv2_l": (32, (("cn", 4, 1, 1, 32), ("er", 7, 2, 4, 64), ("er", 7, 2, 4, 96), ("ir", 10, 2, 4, 192),
                              ("ir", 19, 1, 6, 224), ("ir", 25, 2, 6, 384), ("ir", 7, 1, 6, 640))),
}
HEAD_WIDTH = 1280
BN_EPS = 1e-5


def _round_channels(v: float) -> int:
    """timm round_channels(v, 8, round_limit=0.9)"""
    n = max(8, int(v + 4) // 8 * 8)
    return n + 8 if n < 0.9 * v else n


# EfficientNet-B0's stages: (type, repeats, kernel, stride of the first block, expansion, out channels), type ``ds``
# (DepthwiseSeparable) or ``ir``; B1..B4 scale the widths by w (round_channels) and the repeats by d (ceil)
_B0_STAGES = (("ds", 1, 3, 1, 1, 16), ("ir", 2, 3, 2, 6, 24), ("ir", 2, 5, 2, 6, 40), ("ir", 3, 3, 2, 6, 80),
              ("ir", 3, 5, 1, 6, 112), ("ir", 4, 5, 2, 6, 192), ("ir", 1, 3, 1, 6, 320))


def _scaled(w: float, d: float) -> tuple:
    stages = tuple((t, math.ceil(r * d), k, s, e, _round_channels(c * w)) for t, r, k, s, e, c in _B0_STAGES)
    return _round_channels(32 * w), stages, _round_channels(HEAD_WIDTH * w)


# name -> (stem width, stages, num_features)
EFFNET_CFGS = {f"efficientnet_b{i}": _scaled(w, d)
               for i, (w, d) in enumerate(((1.0, 1.0), (1.0, 1.1), (1.1, 1.2), (1.2, 1.4), (1.4, 1.8)))}


def _r32(c: int) -> int:
    """the stored channel stride of an EfficientNet-B activation: the streaming kernels take multiples of 32"""
    return -(-c // 32) * 32


def _pow2(c: int) -> int:
    """the stored channel stride of a tensor a dense 3x3 convolution touches"""
    p = 32
    while p < c:
        p *= 2
    return p


class ConvBnAct(nn.Module):
    kind = "cn"

    def __init__(self, cin: int, cout: int, stride: int) -> None:
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride, self.has_skip = stride, stride == 1 and cin == cout


class EdgeResidual(nn.Module):
    kind = "er"

    def __init__(self, cin: int, cout: int, stride: int, expand: int) -> None:
        super().__init__()
        mid = cin * expand
        self.conv_exp = nn.Conv2d(cin, mid, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride, self.has_skip = stride, stride == 1 and cin == cout


class SqueezeExcite(nn.Module):
    def __init__(self, channels: int, rd_channels: int) -> None:
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, rd_channels, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd_channels, channels, 1, bias=True)

    def params(self) -> list:
        return [self.conv_reduce.weight, self.conv_reduce.bias, self.conv_expand.weight, self.conv_expand.bias]


class InvertedResidual(nn.Module):
    kind = "ir"

    def __init__(self, cin: int, cout: int, stride: int, expand: int, k: int = 3) -> None:
        super().__init__()
        mid = cin * expand
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride=stride, padding=k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid, eps=BN_EPS)
        # timm: se_ratio 0.25 of the block's INPUT channels (se_from_exp=False), not of the expanded width
        self.se = SqueezeExcite(mid, cin // 4)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride, self.has_skip = stride, stride == 1 and cin == cout


class DepthwiseSeparable(nn.Module):
    """EfficientNet-B's first stage: the InvertedResidual without its expansion (depthwise 3x3 on the block input)"""
    kind = "ds"

    def __init__(self, cin: int, cout: int, stride: int, k: int = 3) -> None:
        super().__init__()
        self.conv_dw = nn.Conv2d(cin, cin, k, stride=stride, padding=k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin, eps=BN_EPS)
        self.se = SqueezeExcite(cin, cin // 4)
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride, self.has_skip = stride, stride == 1 and cin == cout


def _mb_parts(blk) -> tuple:
    """(expand conv, its BatchNorm, the depthwise BatchNorm, project conv, its BatchNorm) of an ir | ds block"""
    if blk.kind == "ir":
        return blk.conv_pw, blk.bn1, blk.bn2, blk.conv_pwl, blk.bn3
    return None, None, blk.bn1, blk.conv_pw, blk.bn2


class _EffNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, model):  # noqa: D401 - autograd signature
        feat, tape = model._forward_impl(x, save=True)
        ctx.model = model
        ctx.tape = tape
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        ctx.model._backward_impl(ctx.tape, dfeat)
        ctx.tape = None
        return None, None, None


@dataclass
class _Tape:
    stem: tuple = ()
    blocks: list = field(default_factory=list)  # (x_in, saved, out) per block
    head: tuple = ()
    out_shape: tuple = ()
    batch_stats: bool = True


@dataclass
class _Bn:
    """One BatchNorm as the kernels read it over the stored channels: direct views, or -- a padded tensor -- the
    model's zero-padded copies (``pad`` [4][Cs]: gamma, beta, running_mean, running_var)."""
    mod: nn.BatchNorm2d
    gamma: torch.Tensor
    beta: torch.Tensor
    rm: torch.Tensor
    rv: torch.Tensor
    padded: bool
    mean: torch.Tensor | None = None
    rstd: torch.Tensor | None = None

    @property
    def ref(self) -> tuple:
        return (self.mean, self.rstd, self.gamma, self.beta)


class EfficientNetV2Hip(ExplicitBackward, nn.Module):
    def __init__(self, stem: int = 24, stages=EFFNETV2_CFGS["efficientnetv2_s"][1], precision: str = "bf16") -> None:
        """``stages``: (type, repeats, stride of the first block, expansion, out channels) per stage, type ``cn``
        (ConvBnAct), ``er`` (EdgeResidual) or ``ir`` (InvertedResidual with squeeze-and-excitation)."""
        super().__init__()
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        self.precision = precision
        self.conv_stem = nn.Conv2d(3, stem, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem, eps=BN_EPS)
        cin, stage_mods = stem, []
        for kind, repeats, stride, expand, cout in stages:
            if kind not in ("cn", "er", "ir"):
                raise ValueError(f"unknown block type {kind!r}")
            if kind == "ir" and ((cin * expand) % 32 or cin % 16 or cout % 8):
                raise ValueError(f"InvertedResidual {cin} -> {cout} (x{expand}): the depthwise width must be a multiple "
                                 "of 32 and the squeeze width a multiple of 4")
            blocks = []
            for i in range(repeats):
                s = stride if i == 0 else 1
                blocks.append(ConvBnAct(cin, cout, s) if kind == "cn" else
                              EdgeResidual(cin, cout, s, expand) if kind == "er" else
                              InvertedResidual(cin, cout, s, expand))
                cin = cout
            stage_mods.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stage_mods)
        self._finish_init(cin, HEAD_WIDTH)

    def _finish_init(self, cin: int, num_features: int) -> None:
        """the head and the run-time state, after ``conv_stem``, ``bn1`` and ``blocks``"""
        self.conv_head = nn.Conv2d(cin, num_features, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(num_features, eps=BN_EPS)
        self.num_features = num_features
        self.grad_ready_hook: Callable[[list], None] | None = None
        self._shadow: dict[int, torch.Tensor] | None = None
        self.overlap_wgrad = os.environ.get("SV_SIDE_STREAM", "1") != "0"
        self.side_grid_cap: int | None = None  # None: 3/4 of the device's CUs (as ResNetHip)
        self._side: dict = {}
        self._pads: dict = {}  # zero-padded copies of the weights / BatchNorm vectors of padded tensors
        # the step cannot be captured yet: the padded copies are allocated on first use and the forward has no
        # captured-graph form (DESIGN.md "EfficientNetV2", not built)
        self.graph_safe = False
        self.comm_reserve_cus = 0
        self.comm_cu_mask = False
        self._init_weights()

    # timm _init_weight_goog: conv N(0, sqrt(2 / fan_out)), fan_out = k k out / groups; bias 0; BatchNorm 1 / 0
    def _init_weights(self) -> None:
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0.0, (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def set_weight_shadow(self, shadow: dict[int, torch.Tensor] | None) -> None:
        """Install bf16 views kept fresh by the flat optimizer (id(param) -> bf16 tensor): the unpadded 1x1 convolutions
        read them directly."""
        self._shadow = shadow

    def _apply(self, fn, *args, **kwargs):
        self._pads.clear()  # device / dtype moves: the padded copies are rebuilt on first use
        return super()._apply(fn, *args, **kwargs)

    @property
    def compute_bf16(self) -> bool:
        return self.precision == "bf16"

    @property
    def act_dtype(self) -> torch.dtype:
        return torch.bfloat16 if self.compute_bf16 else torch.float32

    @property
    def grad_dtype(self) -> torch.dtype:
        """dtype of the backward's gradient stream (block output / input gradients)."""
        return self.act_dtype

    def block_list(self) -> list:
        return [blk for stage in self.blocks for blk in stage]

    def _cs(self, c: int, dense: bool) -> int:
        """stored channel stride of a c-channel tensor: padded to a power of two where a dense 3x3 touches it"""
        return _pow2(c) if dense else c

    def _out_cs(self, blk) -> int:
        """stored stride of a block's output: ConvBnAct / EdgeResidual outputs feed (or may feed) a dense 3x3"""
        cout = (blk.conv if blk.kind == "cn" else blk.conv_pwl).out_channels
        return self._cs(cout, blk.kind != "ir")

    def _mid_cs(self, c: int) -> int:
        """stored stride of an InvertedResidual's expanded tensors (the constructor admits multiples of 32 only)"""
        return c

    def _rd_cs(self, rd: int) -> int:
        """stored width of a squeeze-and-excitation's hidden vector (the constructor admits multiples of 4 only)"""
        return rd

    # -- operands ----------------------------------------------------------------------------------
    def _zeros(self, key, shape: tuple, dtype, device, fill_rows=None) -> torch.Tensor:
        buf = self._pads.get(key)
        if buf is None or buf.device != device:
            buf = self._pads[key] = torch.zeros(shape, device=device, dtype=dtype)
            if fill_rows is not None:
                buf[fill_rows] = 1.0
        return buf

    def _lin_w(self, conv: nn.Conv2d, Ns: int, Ks: int, cache: dict) -> torch.Tensor:
        """A 1x1 convolution's weight [Ns][Ks] as the GEMM reads it (activation dtype): the f32 parameter, its bf16
        shadow or cast, or -- padded operands -- a zero-padded copy."""
        w = conv.weight
        N, Kc = w.shape[:2]
        k = id(w)
        if k in cache:
            return cache[k]
        if (Ns, Ks) == (N, Kc):
            if not self.compute_bf16:
                out = w.detach().view(N, Kc)
            elif self._shadow is not None and k in self._shadow:
                out = self._shadow[k].view(N, Kc)
            else:
                out = K.cast_bf16(w.detach().contiguous()).view(N, Kc)
        else:
            out = self._zeros(("lin", k), (Ns, Ks), self.act_dtype, w.device)
            out[:N, :Kc].copy_(w.detach().view(N, Kc))
        cache[k] = out
        return out

    def _dense_w(self, conv: nn.Conv2d, Cout_s: int, Cin_s: int) -> torch.Tensor:
        """A dense 3x3 weight over the stored channels, f32 [Cout_s][Cin_s][3][3] (padded rows / columns zero)."""
        w = conv.weight
        Cout, Cin = w.shape[:2]
        if (Cout_s, Cin_s) == (Cout, Cin):
            return w.detach()
        buf = self._zeros(("dense", id(w)), (Cout_s, Cin_s, 3, 3), torch.float32, w.device)
        buf[:Cout, :Cin].copy_(w.detach())
        return buf

    def _dw_w(self, conv: nn.Conv2d, Cs: int) -> torch.Tensor:
        """A depthwise weight over the stored channels, f32 [Cs][1][k][k] (padded rows zero)."""
        w = conv.weight
        C = w.shape[0]
        if Cs == C:
            return w.detach()
        buf = self._zeros(("dw", id(w)), (Cs, *w.shape[1:]), torch.float32, w.device)
        buf[:C].copy_(w.detach())
        return buf

    def _se_w(self, se: SqueezeExcite, Cs: int, rds: int) -> tuple:
        """(w1 [rds][Cs], b1 [rds], w2 [Cs][rds], b2 [Cs]) of a squeeze-and-excitation over the stored widths: the
        parameters, or zero-padded copies (a padded hidden unit is silu(0) = 0; a padded channel's gate scales a zero)."""
        ps = se.params()
        rd, C = ps[0].shape[:2]
        if (rds, Cs) == (rd, C):
            return tuple(ps)
        out = []
        for i, (p, shape) in enumerate(zip(ps, ((rds, Cs, 1, 1), (rds,), (Cs, rds, 1, 1), (Cs,)))):
            buf = self._zeros(("se", id(p)), shape, torch.float32, p.device)
            buf[tuple(slice(0, n) for n in p.shape)].copy_(p.detach())
            out.append(buf)
        return tuple(out)

    def _se_grads(self, se: SqueezeExcite, Cs: int, rds: int) -> tuple:
        """(dw1, db1, dw2, db2) accumulators over the stored widths, and the fold into p.grad for a padded one (the
        gradients of padded rows / columns are dropped)."""
        ps = se.params()
        rd, C = ps[0].shape[:2]
        if (rds, Cs) == (rd, C):
            return (*map(self._grad, ps), lambda: None)
        scr = [torch.zeros(shape, device=ps[0].device, dtype=torch.float32)
               for shape in ((rds, Cs, 1, 1), (rds,), (Cs, rds, 1, 1), (Cs,))]

        def fold():
            for p, t in zip(ps, scr):
                self._grad(p).add_(t[tuple(slice(0, n) for n in p.shape)])
        return (*scr, fold)

    def _dw_wgrad(self, conv: nn.Conv2d, dy4d, x4d):
        """weight-gradient job of a depthwise convolution: into p.grad, or -- padded channels -- through a scratch"""
        g = self._grad(conv.weight)
        C, k, st = conv.weight.shape[0], conv.kernel_size[0], conv.stride[0]
        wgrad = K.dwconv5_bwd_weight if k == 5 else K.dwconv3_bwd_weight

        def job(pol):
            if dy4d.shape[-1] == C:
                wgrad(dy4d, x4d, st, dw=g, accumulate=True)
            else:
                tmp = torch.empty(dy4d.shape[-1], 1, k, k, device=g.device, dtype=torch.float32)
                wgrad(dy4d, x4d, st, dw=tmp, accumulate=False)
                g.add_(tmp[:C])
        return job

    def _bn_ref(self, bn: nn.BatchNorm2d, Cs: int) -> _Bn:
        C = bn.num_features
        if Cs == C:
            return _Bn(bn, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, False)
        pad = self._zeros(("bn", id(bn)), (4, Cs), torch.float32, bn.weight.device, fill_rows=3)
        for i, t in enumerate((bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            pad[i, :C].copy_(t.detach())
        return _Bn(bn, pad[0], pad[1], pad[2], pad[3], True)

    def _stats(self, b: _Bn, y2d: torch.Tensor, part: torch.Tensor | None = None) -> _Bn:
        """Fill (mean, rstd): batch statistics (+ running update) in train mode -- from the producer's partials, from
        sv_bn_stats, or (above its 1024 channels) from csrc/mbconv.hip's statistics pass -- else the running ones."""
        bn = b.mod
        if not self.training:
            b.mean, b.rstd = K.bn_eval_params(b.rm, b.rv, bn.eps)
            return b
        kw = dict(eps=bn.eps, momentum=0.1 if bn.momentum is None else bn.momentum, running_mean=b.rm,
                  running_var=b.rv, num_batches_tracked=bn.num_batches_tracked)
        if part is not None:
            b.mean, b.rstd = K.bn_stats_from_partials(part, y2d.shape[0], **kw)
        elif K._bn_c_ok(y2d.shape[1]):
            b.mean, b.rstd = K.bn_stats(y2d, **kw)
        else:
            b.mean, b.rstd = K.mb_bn_stats(y2d, **kw)
        if b.padded:
            C = bn.num_features
            bn.running_mean.copy_(b.rm[:C])
            bn.running_var.copy_(b.rv[:C])
        return b

    def _bn_grads(self, b: _Bn) -> tuple:
        """(dgamma, dbeta) accumulators over the stored channels, and the fold into p.grad for padded ones."""
        bn = b.mod
        if not b.padded:
            return self._grad(bn.weight), self._grad(bn.bias), lambda: None
        scr = torch.zeros(2, b.gamma.numel(), device=b.gamma.device, dtype=torch.float32)
        C = bn.num_features

        def fold():
            self._grad(bn.weight).add_(scr[0, :C])
            self._grad(bn.bias).add_(scr[1, :C])
        return scr[0], scr[1], fold

    def _conv3(self, x4d, conv: nn.Conv2d, Cout_s: int, Cin=None):
        """dense 3x3 conv over the stored channels -> (y, packed weight, shape, BatchNorm partials or None)"""
        B, H, W, Cs = x4d.shape
        s = K.conv_shape(B, H, W, Cs, Cout_s, 3, conv.stride[0], 1, Cin)
        wp = K.conv_weight_pack(self._dense_w(conv, Cout_s, Cin if Cin is not None else Cs), Cs, self.act_dtype)
        if self.training and self.compute_bf16:
            y, part = K.conv_fwd_bn_stats(x4d, wp, s, self.act_dtype)
            return y, wp, s, part
        return K.conv_fwd(x4d, wp, s, self.act_dtype), wp, s, None

    def _lin(self, x2d, w2d):
        """1x1 conv as a GEMM -> (y [M][N], BatchNorm partials or None)"""
        M, Kc = x2d.shape
        N = w2d.shape[0]
        y = torch.empty(M, N, device=x2d.device, dtype=self.act_dtype)
        if self.training and self.compute_bf16 and _EPI_STATS and Kc % 32 == 0 and N % 32 == 0:
            part = torch.empty((M + 63) // 64, 2, N, device=x2d.device, dtype=torch.float32)
            K.linear_fwd(x2d, w2d, out=y, out2=part, epilogue=nv.SV_EPI_STORE_STATS)
            return y, part
        K.linear_fwd(x2d, w2d, out=y, compute_bf16=self.compute_bf16)
        return y, None

    # -- forward -----------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the MI355X kernel library only (got a CPU tensor)")
        x = x.contiguous() if x.dtype == torch.uint8 else x.float().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad:
            anchor = torch.zeros((), device=x.device, requires_grad=True)
            return _EffNetFn.apply(x, anchor, self)
        feat, _ = self._forward_impl(x, save=False)
        return feat

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)

    @torch.no_grad()
    def _forward_impl(self, img: torch.Tensor, save: bool):
        act = self.act_dtype
        cs0 = 8 if self.compute_bf16 else 4
        x0 = (K.image_u8_hwc_to_nhwc(img, cs0, act) if img.dtype == torch.uint8 else K.image_to_nhwc(img, cs0, act))
        cache: dict = {}
        tape = _Tape(batch_stats=self.training) if save else None
        # stem: conv 3x3 / 2 -> BatchNorm + SiLU
        stem_s = _pow2(self.conv_stem.out_channels)
        y, wp, s, part = self._conv3(x0, self.conv_stem, stem_s, Cin=3)
        b = self._stats(self._bn_ref(self.bn1, stem_s), y.view(-1, stem_s), part)
        x = K.bn_silu_fwd(y.view(-1, stem_s), b.ref, out_dtype=act).view(y.shape)
        if save:
            tape.stem = (x0, y, b, s)
        for blk in self.block_list():
            out, saved = self._block_forward(blk, x, cache)
            if save:
                tape.blocks.append((x, saved, out))
            x = out
        # head: conv 1x1 -> BatchNorm + SiLU -> global average pool
        B, H, W, Cs = x.shape
        nf = self.num_features
        wh = self._lin_w(self.conv_head, nf, Cs, cache)
        yh, part = self._lin(x.view(-1, Cs), wh)
        bh = self._stats(self._bn_ref(self.bn2, nf), yh, part)
        a = K.bn_silu_fwd(yh, bh.ref, out_dtype=act).view(B, H, W, nf)
        feat = K.avgpool_fwd(a)
        if save:
            tape.head = (x, yh, bh, wh)
            tape.out_shape = tuple(a.shape)
        return feat, tape

    def _block_forward(self, blk, x, cache: dict):
        """-> (block output [B,OH,OW,out stride], what the backward needs)"""
        act = self.act_dtype
        B, H, W, Cs = x.shape
        out_s = self._out_cs(blk)
        res = x.view(-1, Cs) if blk.has_skip else None
        if blk.kind == "cn":
            y, wp, s, part = self._conv3(x, blk.conv, out_s)
            b1 = self._stats(self._bn_ref(blk.bn1, out_s), y.view(-1, out_s), part)
            out = K.bn_silu_fwd(y.view(-1, out_s), b1.ref, res=res, out_dtype=act).view(y.shape)  # skip AFTER the SiLU
            return out, (y, b1, wp, s)
        if blk.kind == "er":
            mid_s = _pow2(blk.conv_exp.out_channels)
            y1, wp, s, part = self._conv3(x, blk.conv_exp, mid_s)
            b1 = self._stats(self._bn_ref(blk.bn1, mid_s), y1.view(-1, mid_s), part)
            a1 = K.bn_silu_fwd(y1.view(-1, mid_s), b1.ref, out_dtype=act)
            w2 = self._lin_w(blk.conv_pwl, out_s, mid_s, cache)
            y2, part2 = self._lin(a1, w2)
            b2 = self._stats(self._bn_ref(blk.bn2, out_s), y2, part2)
            out = K.bn_act(y2, b2.mean, b2.rstd, b2.gamma, b2.beta, res=res, relu=False, out_dtype=act)
            return out.view(B, y1.shape[1], y1.shape[2], out_s), (y1, b1, wp, s, a1, y2, b2, w2)
        # ir | ds: (1x1 expand -> BatchNorm + SiLU ->) depthwise -> BatchNorm + SiLU -> SE -> 1x1 project -> BatchNorm
        conv_e, bn_e, bn_d, conv_p, bn_p = _mb_parts(blk)
        if conv_e is None:
            mid, y1, b1, w1, a1 = Cs, None, None, None, x
        else:
            mid = self._mid_cs(conv_e.out_channels)
            w1 = self._lin_w(conv_e, mid, Cs, cache)
            y1, part1 = self._lin(x.view(-1, Cs), w1)
            b1 = self._stats(self._bn_ref(bn_e, mid), y1, part1)
            a1 = K.bn_silu_fwd(y1, b1.ref, out_dtype=act).view(B, H, W, mid)
        dw_fwd = K.dwconv5_fwd if blk.conv_dw.kernel_size[0] == 5 else K.dwconv3_fwd
        y2 = dw_fwd(a1, self._dw_w(blk.conv_dw, mid), blk.stride, out_dtype=act)
        _, OH, OW, _ = y2.shape
        b2 = self._stats(self._bn_ref(bn_d, mid), y2.view(-1, mid))
        # s = silu(bn(y2)) is never stored: the squeeze, the scale and both backward passes recompute it from y2
        sew = self._se_w(blk.se, mid, self._rd_cs(blk.se.conv_reduce.out_channels))
        state = K.mbse_excite(K.mbse_squeeze(y2, b2.ref), OH * OW, *sew)
        a2 = K.mbse_scale(y2, b2.ref, state[3], out_dtype=act)
        w3 = self._lin_w(conv_p, out_s, mid, cache)
        y3, part3 = self._lin(a2.view(-1, mid), w3)
        b3 = self._stats(self._bn_ref(bn_p, out_s), y3, part3)
        out = K.bn_act(y3, b3.mean, b3.rstd, b3.gamma, b3.beta, res=res, relu=False, out_dtype=act)
        return out.view(B, OH, OW, out_s), (y1, b1, w1, a1, y2, b2, state, a2, y3, b3, w3)

    # -- backward ----------------------------------------------------------------------------------
    def _flush(self, jobs: list, params: list, side, keep: list, deferred: list | None) -> None:
        """Run a block's weight-gradient jobs (callables taking the GEMM policy) and report its parameters ready: on the
        side stream after one hand-off (the jobs stay referenced in ``keep`` until the streams join), else here."""
        if side is None:
            for job in jobs:
                job(None)
            if deferred is not None:
                deferred.extend(params)
            else:
                self._ready(params)
            return
        side.wait_event(torch.cuda.current_stream().record_event())
        ncu = torch.cuda.get_device_properties(side.device).multi_processor_count
        if self.side_grid_cap is None:
            self.side_grid_cap = ncu * 3 // 4
        cap = self.side_grid_cap
        if self.comm_reserve_cus > 0:
            cap = min(cap, max(1, ncu - self.comm_reserve_cus))
        spol = nv.policy(grid_cap=cap)
        with torch.cuda.stream(side):
            for job in jobs:
                job(spol)
            self._ready(params)
        keep.append(jobs)

    def _lin_wgrad(self, conv: nn.Conv2d, dy2d, x2d):
        """weight-gradient job of a 1x1 convolution: straight into p.grad, or -- padded operands -- through a padded
        scratch whose real block is added"""
        g = self._grad(conv.weight)
        N, Kc = conv.weight.shape[:2]
        bf = self.compute_bf16

        def job(pol):
            if (dy2d.shape[1], x2d.shape[1]) == (N, Kc):
                K.linear_wgrad(dy2d, x2d, out=g.view(N, Kc), accumulate=True, compute_bf16=bf, policy=pol)
            else:
                tmp = K.linear_wgrad(dy2d, x2d, compute_bf16=bf, policy=pol)
                g.view(N, Kc).add_(tmp.view(dy2d.shape[1], x2d.shape[1])[:N, :Kc])
        return job

    def _conv_wgrad(self, conv: nn.Conv2d, dy4d, x4d, s):
        g = self._grad(conv.weight)
        Cout, Cin = conv.weight.shape[:2]

        def job(pol):
            if (s.Cout, s.Cin) == (Cout, Cin):
                K.conv_bwd_weight(dy4d, x4d, s, dw=g, accumulate=True, policy=pol)
            else:
                tmp = torch.zeros(s.Cout, s.Cin, 3, 3, device=g.device, dtype=torch.float32)
                K.conv_bwd_weight(dy4d, x4d, s, dw=tmp, accumulate=True, policy=pol)
                g.add_(tmp[:Cout, :Cin])
        return job

    def _lin_dgrad(self, dy2d, w2d, dtype):
        dx = torch.empty(dy2d.shape[0], w2d.shape[1], device=dy2d.device, dtype=dtype)
        K.linear_dgrad(dy2d, w2d, out=dx, compute_bf16=self.compute_bf16)
        return dx

    @torch.no_grad()
    def _block_backward(self, blk, saved_block, d: torch.Tensor, side=None, keep=None, deferred=None,
                        batch_stats: bool = True) -> torch.Tensor:
        """Backward of one block given d = dL/d(block output) (``grad_dtype``, NHWC over the stored channels,
        contiguous; left unchanged); accumulates the block's parameter gradients and returns dL/d(block input)."""
        assert d.is_contiguous() and d.dtype == self.grad_dtype
        act = self.act_dtype
        x_in, saved, out = saved_block
        keep = [] if keep is None else keep
        B, H, W, Cs = x_in.shape
        jobs, folds = [], []
        if blk.kind == "cn":
            y, b1, wp, s = saved
            C = y.shape[-1]
            dg, db, fold = self._bn_grads(b1)
            dy = K.bn_silu_bwd(d.view(-1, C), y.view(-1, C), b1.ref, dgamma=dg, dbeta=db, dx_dtype=act,
                               batch_stats=batch_stats)
            fold()
            jobs.append(self._conv_wgrad(blk.conv, dy.view(y.shape), x_in, s))
            dx = K.conv_bwd_data(dy.view(y.shape), wp, s, dx_dtype=self.grad_dtype)
            params = [blk.conv.weight, blk.bn1.weight, blk.bn1.bias]
        elif blk.kind == "er":
            y1, b1, wp, s, a1, y2, b2, w2 = saved
            Cm, Co = y1.shape[-1], y2.shape[-1]
            dg, db, fold = self._bn_grads(b2)
            dy2 = K.bn_bwd(d.view(-1, Co), y2, b2.mean, b2.rstd, b2.gamma, dgamma=dg, dbeta=db, dx_dtype=act,
                           batch_stats=batch_stats)
            fold()
            jobs.append(self._lin_wgrad(blk.conv_pwl, dy2, a1))
            da1 = self._lin_dgrad(dy2, w2, act)
            dg, db, fold = self._bn_grads(b1)
            dy1 = K.bn_silu_bwd(da1, y1.view(-1, Cm), b1.ref, dgamma=dg, dbeta=db, dx_dtype=act, batch_stats=batch_stats)
            fold()
            jobs.append(self._conv_wgrad(blk.conv_exp, dy1.view(y1.shape), x_in, s))
            dx = K.conv_bwd_data(dy1.view(y1.shape), wp, s, dx_dtype=self.grad_dtype)
            params = [blk.conv_pwl.weight, blk.bn2.weight, blk.bn2.bias, blk.conv_exp.weight, blk.bn1.weight, blk.bn1.bias]
        else:
            y1, b1, w1, a1, y2, b2, state, a2, y3, b3, w3 = saved
            conv_e, bn_e, bn_d, conv_p, bn_p = _mb_parts(blk)
            se = blk.se
            Cm, Co = y2.shape[-1], y3.shape[-1]
            rds = self._rd_cs(se.conv_reduce.out_channels)
            dg, db, fold = self._bn_grads(b3)
            dy3 = K.bn_bwd(d.view(-1, Co), y3, b3.mean, b3.rstd, b3.gamma, dgamma=dg, dbeta=db, dx_dtype=act,
                           batch_stats=batch_stats)
            fold()
            jobs.append(self._lin_wgrad(conv_p, dy3, a2.view(-1, Cm)))
            da2 = self._lin_dgrad(dy3, w3, act).view(y2.shape)
            # pass A: per-image sum_hw da s; the gate's backward; pass B: dpre and the depthwise BatchNorm's partials
            part = K.mbse_bwd_stats(da2, y2, b2.ref)
            sew = self._se_w(se, Cm, rds)
            dw1, db1, dw2, db2, fold = self._se_grads(se, Cm, rds)
            dpool = K.mbse_bwd_gate(part, state, sew[0], sew[2], dw1=dw1, db1=db1, dw2=dw2, db2=db2)
            fold()
            dpre, bpart = K.mbse_bwd_apply(da2, y2, b2.ref, state[3], dpool, out_dtype=act)
            dg, db, fold = self._bn_grads(b2)
            dy2 = K.bn_bwd_from_partials(dpre.view(-1, Cm), y2.view(-1, Cm), b2.mean, b2.rstd, b2.gamma, bpart,
                                         dgamma=dg, dbeta=db, dx_dtype=act, batch_stats=batch_stats).view(y2.shape)
            fold()
            jobs.append(self._dw_wgrad(blk.conv_dw, dy2, a1))
            dw_bwd = K.dwconv5_bwd_data if blk.conv_dw.kernel_size[0] == 5 else K.dwconv3_bwd_data
            da1 = dw_bwd(dy2, self._dw_w(blk.conv_dw, Cm), H, W, blk.stride, dx_dtype=act)
            params = [conv_p.weight, bn_p.weight, bn_p.bias, *se.params(), bn_d.weight, bn_d.bias, blk.conv_dw.weight]
            if conv_e is None:
                dx = da1
            else:
                dg, db, fold = self._bn_grads(b1)
                dy1 = K.bn_silu_bwd(da1.view(-1, Cm), y1, b1.ref, dgamma=dg, dbeta=db, dx_dtype=act,
                                    batch_stats=batch_stats)
                fold()
                jobs.append(self._lin_wgrad(conv_e, dy1, x_in.view(-1, Cs)))
                dx = self._lin_dgrad(dy1, w1, self.grad_dtype).view(x_in.shape)
                params += [bn_e.weight, bn_e.bias, conv_e.weight]
        if blk.has_skip:
            K.mb_add(dx, d)
        self._flush(jobs, params, side, keep, deferred)
        return dx

    @torch.no_grad()
    def _backward_impl(self, tape: _Tape, dfeat: torch.Tensor) -> None:
        act = self.act_dtype
        main = torch.cuda.current_stream()
        side = self._side_stream(main.device) if (self.overlap_wgrad and self.compute_bf16) else None
        keep: list = []
        deferred: list | None = [] if side is not None else None
        bs = tape.batch_stats
        # head
        x, yh, bh, wh = tape.head
        d = K.avgpool_bwd(dfeat, tape.out_shape, dx_dtype=self.grad_dtype)
        dy = K.bn_silu_bwd(d.view(-1, self.num_features), yh, bh.ref, dgamma=self._grad(self.bn2.weight),
                           dbeta=self._grad(self.bn2.bias), dx_dtype=act, batch_stats=bs)
        d = self._lin_dgrad(dy, wh, self.grad_dtype).view(x.shape)
        self._flush([self._lin_wgrad(self.conv_head, dy, x.view(-1, x.shape[-1]))],
                    [self.conv_head.weight, self.bn2.weight, self.bn2.bias], side, keep, deferred)
        blocks = self.block_list()
        for blk, saved_block in zip(reversed(blocks), reversed(tape.blocks)):
            d = self._block_backward(blk, saved_block, d, side, keep, deferred, batch_stats=bs)
        # stem (weight gradient only)
        x0, y, b, s = tape.stem
        C = y.shape[-1]
        dg, db, fold = self._bn_grads(b)
        dy = K.bn_silu_bwd(d.view(-1, C), y.view(-1, C), b.ref, dgamma=dg, dbeta=db, dx_dtype=act, batch_stats=bs)
        fold()
        self._flush([self._conv_wgrad(self.conv_stem, dy.view(y.shape), x0, s)],
                    [self.conv_stem.weight, self.bn1.weight, self.bn1.bias], None, keep, deferred)
        if side is not None:
            main.wait_stream(side)
            self._ready(deferred)
        keep.clear()


def create_efficientnetv2(name: str, precision: str = "bf16") -> EfficientNetV2Hip:
    key = name.split(".")[0]
    if key not in EFFNETV2_CFGS:
        raise ValueError(f"unsupported EfficientNetV2 variant {name!r}")
    stem, stages = EFFNETV2_CFGS[key]
    return EfficientNetV2Hip(stem, stages, precision=precision)


class EfficientNetHip(EfficientNetV2Hip):
    """EfficientNet-B0..B4 -- drop-in for ``timm.create_model("efficientnet_b{0..4}", num_classes=0)`` (the non-``tf_``
    variants) on the block routines of EfficientNetV2Hip, with what the B series adds: the ``ds`` block, 5x5 depthwise
    convolutions (csrc/dwconv5.hip), and widths the streaming kernels refuse (16, 24, 40, 88, 144, 240, ...; SE widths
    6, 10, 22, ...).  Every stored activation has its channel stride rounded up to a multiple of 32 (a power of two where
    the dense 3x3 stem writes it) and every SE hidden vector to a multiple of 4, with the zero-padding rules of the
    module docstring: padded channels are exactly zero in every forward tensor and every gradient."""

    def __init__(self, stem: int = 32, stages=EFFNET_CFGS["efficientnet_b0"][1], num_features: int = HEAD_WIDTH,
                 precision: str = "bf16") -> None:
        """``stages``: (type, repeats, kernel, stride of the first block, expansion, out channels) per stage, type ``ds``
        (DepthwiseSeparable) or ``ir`` (InvertedResidual), kernel 3 | 5."""
        nn.Module.__init__(self)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        self.precision = precision
        self.conv_stem = nn.Conv2d(3, stem, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem, eps=BN_EPS)
        cin, stage_mods = stem, []
        for kind, repeats, k, stride, expand, cout in stages:
            if kind not in ("ds", "ir") or k not in (3, 5):
                raise ValueError(f"unknown block type / kernel {kind!r} / {k}")
            if cin % 8 or cout % 8 or _r32(cin * expand) > K.MB_MAX_C:
                raise ValueError(f"{kind} {cin} -> {cout} (x{expand}): widths must be multiples of 8 and the depthwise "
                                 f"width at most {K.MB_MAX_C}")
            blocks = []
            for i in range(repeats):
                s = stride if i == 0 else 1
                blocks.append(DepthwiseSeparable(cin, cout, s, k) if kind == "ds" else
                              InvertedResidual(cin, cout, s, expand, k))
                cin = cout
            stage_mods.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stage_mods)
        self._finish_init(cin, num_features)

    def _out_cs(self, blk) -> int:
        return _r32((blk.conv_pw if blk.kind == "ds" else blk.conv_pwl).out_channels)

    def _mid_cs(self, c: int) -> int:
        return _r32(c)

    def _rd_cs(self, rd: int) -> int:
        return -(-rd // 4) * 4

    def stored_strides(self) -> list:
        """(stem output, then per block (input, expanded, output)) stored channel strides"""
        cs = _pow2(self.conv_stem.out_channels)
        out = [cs]
        for blk in self.block_list():
            mid = cs if blk.kind == "ds" else self._mid_cs(blk.conv_dw.out_channels)
            out.append((cs, mid, self._out_cs(blk)))
            cs = self._out_cs(blk)
        return out


def create_efficientnet(name: str, precision: str = "bf16") -> EfficientNetHip:
    key = name.split(".")[0]
    if key not in EFFNET_CFGS:
        raise ValueError(f"unsupported EfficientNet variant {name!r}")
    stem, stages, num_features = EFFNET_CFGS[key]
    return EfficientNetHip(stem, stages, num_features, precision=precision)
