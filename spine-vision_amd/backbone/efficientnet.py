"""EfficientNetV2-S / M / L backbone on the gfx950 kernel library -- drop-in for
``timm.create_model("efficientnetv2_{s,m,l}", num_classes=0)`` (timm ``efficientnet.py`` ``_gen_efficientnetv2_*``, the
non-``tf_``, non-``rw`` variants: symmetric padding k // 2, BatchNorm eps 1e-5, SiLU, drop-path 0).

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

    def __init__(self, cin: int, cout: int, stride: int, expand: int) -> None:
        super().__init__()
        mid = cin * expand
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.conv_dw = nn.Conv2d(mid, mid, 3, stride=stride, padding=1, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid, eps=BN_EPS)
        # timm: se_ratio 0.25 of the block's INPUT channels (se_from_exp=False), not of the expanded width
        self.se = SqueezeExcite(mid, cin // 4)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride, self.has_skip = stride, stride == 1 and cin == cout


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
        self.conv_head = nn.Conv2d(cin, HEAD_WIDTH, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(HEAD_WIDTH, eps=BN_EPS)
        self.num_features = HEAD_WIDTH
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
            raise RuntimeError("EfficientNetV2Hip runs on the MI355X kernel library only (got a CPU tensor)")
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
        wh = self._lin_w(self.conv_head, HEAD_WIDTH, Cs, cache)
        yh, part = self._lin(x.view(-1, Cs), wh)
        bh = self._stats(self._bn_ref(self.bn2, HEAD_WIDTH), yh, part)
        a = K.bn_silu_fwd(yh, bh.ref, out_dtype=act).view(B, H, W, HEAD_WIDTH)
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
        mid = blk.conv_pw.out_channels
        w1 = self._lin_w(blk.conv_pw, mid, Cs, cache)
        y1, part1 = self._lin(x.view(-1, Cs), w1)
        b1 = self._stats(self._bn_ref(blk.bn1, mid), y1, part1)
        a1 = K.bn_silu_fwd(y1, b1.ref, out_dtype=act).view(B, H, W, mid)
        wdw = blk.conv_dw.weight.detach()
        y2 = K.dwconv3_fwd(a1, wdw, blk.stride, out_dtype=act)
        _, OH, OW, _ = y2.shape
        b2 = self._stats(self._bn_ref(blk.bn2, mid), y2.view(-1, mid))
        # s = silu(bn2(y2)) is never stored: the squeeze, the scale and both backward passes recompute it from y2
        se = blk.se
        state = K.mbse_excite(K.mbse_squeeze(y2, b2.ref), OH * OW, se.conv_reduce.weight, se.conv_reduce.bias,
                              se.conv_expand.weight, se.conv_expand.bias)
        a2 = K.mbse_scale(y2, b2.ref, state[3], out_dtype=act)
        w3 = self._lin_w(blk.conv_pwl, out_s, mid, cache)
        y3, part3 = self._lin(a2.view(-1, mid), w3)
        b3 = self._stats(self._bn_ref(blk.bn3, out_s), y3, part3)
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
            g = self._grad
            se = blk.se
            Cm, Co = y2.shape[-1], y3.shape[-1]
            _, OH, OW, _ = y2.shape
            dg, db, fold = self._bn_grads(b3)
            dy3 = K.bn_bwd(d.view(-1, Co), y3, b3.mean, b3.rstd, b3.gamma, dgamma=dg, dbeta=db, dx_dtype=act,
                           batch_stats=batch_stats)
            fold()
            jobs.append(self._lin_wgrad(blk.conv_pwl, dy3, a2.view(-1, Cm)))
            da2 = self._lin_dgrad(dy3, w3, act).view(y2.shape)
            # pass A: per-image sum_hw da s; the gate's backward; pass B: dpre and bn2's backward partials
            part = K.mbse_bwd_stats(da2, y2, b2.ref)
            dpool = K.mbse_bwd_gate(part, state, se.conv_reduce.weight, se.conv_expand.weight,
                                    dw1=g(se.conv_reduce.weight), db1=g(se.conv_reduce.bias),
                                    dw2=g(se.conv_expand.weight), db2=g(se.conv_expand.bias))
            dpre, bpart = K.mbse_bwd_apply(da2, y2, b2.ref, state[3], dpool, out_dtype=act)
            dy2 = K.bn_bwd_from_partials(dpre.view(-1, Cm), y2.view(-1, Cm), b2.mean, b2.rstd, b2.gamma, bpart,
                                         dgamma=g(blk.bn2.weight), dbeta=g(blk.bn2.bias), dx_dtype=act,
                                         batch_stats=batch_stats).view(y2.shape)
            wdw, gdw, st = blk.conv_dw.weight.detach(), g(blk.conv_dw.weight), blk.stride
            jobs.append(lambda pol: K.dwconv3_bwd_weight(dy2, a1, st, dw=gdw, accumulate=True))
            da1 = K.dwconv3_bwd_data(dy2, wdw, H, W, st, dx_dtype=act)
            dy1 = K.bn_silu_bwd(da1.view(-1, Cm), y1, b1.ref, dgamma=g(blk.bn1.weight), dbeta=g(blk.bn1.bias),
                                dx_dtype=act, batch_stats=batch_stats)
            jobs.append(self._lin_wgrad(blk.conv_pw, dy1, x_in.view(-1, Cs)))
            dx = self._lin_dgrad(dy1, w1, self.grad_dtype).view(x_in.shape)
            params = [blk.conv_pwl.weight, blk.bn3.weight, blk.bn3.bias, *se.params(), blk.bn2.weight, blk.bn2.bias,
                      blk.conv_dw.weight, blk.bn1.weight, blk.bn1.bias, blk.conv_pw.weight]
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
        dy = K.bn_silu_bwd(d.view(-1, HEAD_WIDTH), yh, bh.ref, dgamma=self._grad(self.bn2.weight),
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
