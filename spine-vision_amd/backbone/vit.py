"""ViT and DeiT-III backbones on the gfx950 kernel library -- drop-in for
``timm.create_model("vit_{tiny,small,base,large}_patch16_224...", num_classes=0)`` and
``timm.create_model("deit3_{small,base}_patch16_224...", num_classes=0)`` as called at
spine_vision/training/models/backbone.py:166-170.

timm is not a dependency of this package, so the architecture is restated here (timm 1.0.22
``timm/models/vision_transformer.py`` as published; tests/_vit_ref.py is the plain ``torch.nn`` form the tests compare
against): ``VisionTransformer`` with patch 16, ``qkv_bias=True``, MLP ratio 4, erf GELU, LayerNorm eps 1e-6,
``global_pool='token'``, no dropout / drop-path, head dimension 64; DeiT-III adds LayerScale (``ls1`` / ``ls2``,
init 1e-6) and ``no_embed_class`` (the position embedding covers the patches only and is added before the class
token is prepended).  These timm models are strict about the image size: an input that is not ``img_size`` x
``img_size`` raises ``ValueError``.  ``img_size`` is any multiple of 16 up to 2048 tokens (224: 197 tokens, 256: 257,
384: 577, 512: 1025; default: env ``SV_VIT_IMG_SIZE``, else 224); a state_dict saved at another square size loads
with its ``pos_embed`` resampled (``resample_abs_pos_embed``).

* Same module tree and ``state_dict`` keys as timm (``cls_token``, ``pos_embed``, ``patch_embed.proj``,
  ``blocks.i.{norm1,attn.qkv,attn.proj,ls1,norm2,mlp.fc1,mlp.fc2,ls2}``, ``norm``), ``num_features``,
  ``forward([B,3,H,W] f32 | uint8 [B,H,W,3] | uint8 [B,H,W]) -> [B, C]`` (the class-token row of the final norm).
  The sub-modules are parameter containers only; their own ``forward`` is never called.
* Forward and backward are explicit kernel sequences over a token matrix [B * Np, C] (DESIGN.md "ViT / DeiT-III"):
  ``sv_patchify16`` -> patch GEMM -> ``sv_vit_tokens``; per block LayerNorm -> qkv GEMM (+bias) -> ``sv_attn_fwd``
  (up to 256 tokens; above, or with ``SV_ATTN=stream``, ``sv_attn_stream_fwd``: DESIGN.md "ViT / DeiT-III at 256-512
  px") -> proj GEMM (+bias, *gamma, +residual) -> LayerNorm -> fc1 GEMM (+bias, GELU and GELU') -> fc2 GEMM (+bias,
  *gamma, +residual); the final LayerNorm over the class rows only.  ViT has no layer scale: its two residual epilogues get a
  buffer of ones that is not in the state_dict (as ConvNeXt V2's fc2).
* Row layout: every image owns Np = N rounded up to a multiple of 8 rows (N = 197 tokens -> 200), so every GEMM and
  LayerNorm row count stays a multiple of 8, the ground those kernels were built and tested on.  Pad rows are zero
  where they enter the first block, are masked out as keys (``sv_attn_*`` never read them and write zeros), carry
  finite values forward that nothing reads, and have exactly zero gradient everywhere in the backward (their output
  gradient is zero and every backward kernel maps a zero row to a zero row), so they add nothing to any weight,
  bias or LayerNorm gradient.
* ``precision="bf16"``: bf16 MFMA, bf16 saved GEMM operands, f32 residual / gradient streams, f32 master weights.
  ``precision="fp32"``: every tensor f32 and f32 MFMA (parity mode) -- except attention, which in f32 runs as torch
  ops (``kernels.attn_fwd`` / ``attn_bwd``, the ``SV_ATTN=torch`` arm): the one part of the fp32 parity mode that does
  not run on this library.
* The weight gradients (qkv / proj / fc1 / fc2 wgrad GEMMs and their folds) run on a side stream beside the
  data-gradient chain in bf16 mode (``SV_SIDE_STREAM=0``: the same kernels on one stream, the same bits);
  ``grad_ready_hook`` is called after each block.
"""

from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass, field
from typing import Callable

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernels as K
from .. import native as nv
from ._explicit import ExplicitBackward
from .convnext import _comm_cap

# name -> (C, depth, heads, LayerScale init or None, no_embed_class); the reference maps deit_tiny to deit3_small
VIT_CFGS = {
    "vit_tiny": (192, 12, 3, None, False),
    "vit_small": (384, 12, 6, None, False),
    "vit_base": (768, 12, 12, None, False),
    "vit_large": (1024, 24, 16, None, False),
    "deit_tiny": (384, 12, 6, 1e-6, True),
    "deit_small": (384, 12, 6, 1e-6, True),
    "deit_base": (768, 12, 12, 1e-6, True),
}
PATCH = 16
HEAD_DIM = 64
_log = logging.getLogger(__name__)
_RESAMPLE_LOGGED = False


class _PatchEmbed(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=PATCH, stride=PATCH)


class _Attention(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)


class _LayerScale(nn.Module):
    def __init__(self, dim: int, init: float) -> None:
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))


class ViTBlock(nn.Module):
    """Parameter container for timm ``Block`` (``qkv_bias=True``, ``init_values`` = LayerScale init or None)."""

    def __init__(self, dim: int, ls_init: float | None) -> None:
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim)
        self.ls1 = _LayerScale(dim, ls_init) if ls_init is not None else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim)
        self.ls2 = _LayerScale(dim, ls_init) if ls_init is not None else nn.Identity()


@dataclass
class _Tape:
    """Activations saved by the training forward for the explicit backward."""

    B: int
    patches: torch.Tensor = None
    blocks: list = field(default_factory=list)  # per block: the tuple _block_forward saves
    head: tuple = ()  # (class rows of the last block's output, mean, rstd)
    wcache: dict = field(default_factory=dict)  # bf16 weight casts shared by forward and backward (no shadow)


class _ViTFn(torch.autograd.Function):
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


class _Wgrads:
    """Where the weight-gradient jobs of the backward run: on the side stream behind a main -> side event each (the
    closures keep their operands alive until the streams join), or inline when there is none.  A job takes the GEMM
    policy of the stream it runs on; ``ready``: the parameters to report once it has been issued, on its stream."""

    def __init__(self, model, main, side, pol) -> None:
        self.model, self.main, self.side, self.pol = model, main, side, pol
        self.spol = nv.policy(grid_cap=pol.grid_cap, wg_per_cu=pol.wg_per_cu, priority=1)
        self.keep: list = []

    def submit(self, job, ready=None) -> None:
        if self.side is None:
            job(self.pol)
            if ready:
                self.model._ready(ready)
            return
        self.side.wait_event(self.main.record_event())
        self.keep.append(job)
        with torch.cuda.stream(self.side):
            job(self.spol)
            if ready:
                self.model._ready(ready)

    def join(self) -> None:
        if self.side is not None:
            self.main.wait_stream(self.side)  # clip / AdamW / the next step see every side-stream gradient
        self.keep.clear()  # safe: later main-stream allocations are ordered after the join


class ViTHip(ExplicitBackward, nn.Module):
    def __init__(self, dim: int = 768, depth: int = 12, heads: int = 12, ls_init: float | None = None,
                 no_embed_class: bool = False, img_size: int | tuple[int, int] = 224, precision: str = "bf16") -> None:
        super().__init__()
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if dim != heads * HEAD_DIM:
            raise ValueError(f"head dimension must be {HEAD_DIM}: dim {dim} with {heads} heads")
        if isinstance(img_size, (tuple, list)):
            if len(img_size) != 2 or img_size[0] != img_size[1]:
                raise ValueError(f"img_size must be square, got {tuple(img_size)}")
            img_size = img_size[0]
        img_size = int(img_size)
        if img_size % PATCH or img_size <= 0:
            raise ValueError(f"img_size must be a positive multiple of {PATCH}, got {img_size}")
        self.dim, self.depth, self.heads = dim, depth, heads
        self.no_embed_class = bool(no_embed_class)
        self.img_size = img_size
        self.num_patches = (img_size // PATCH) ** 2
        self.num_tokens = self.num_patches + 1
        if self.num_tokens > K.ATTN_STREAM_MAX_N:
            raise ValueError(f"img_size {img_size}: {self.num_tokens} tokens, the attention kernels hold at most "
                             f"{K.ATTN_STREAM_MAX_N}")
        # up to 256 tokens (224 px) the one-pass kernels of csrc/attn.hip, above that the streaming pair of
        # csrc/attn_stream.hip; SV_ATTN=stream (or this attribute) forces the streaming pair at any size (A/B runs)
        self.attn_stream = os.environ.get("SV_ATTN", "") == "stream"
        self.rows_per_img = -(-self.num_tokens // 8) * 8  # Np: tokens padded to a multiple of 8 rows
        self.precision = precision
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + (0 if no_embed_class else 1), dim))
        self.patch_embed = _PatchEmbed(dim)
        self.blocks = nn.Sequential(*[ViTBlock(dim, ls_init) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.has_ls = ls_init is not None
        if not self.has_ls:
            # the bias + residual epilogue (SV_EPI_BIAS_GAMMA_RES) with a layer scale of exactly one; not persistent:
            # it stays out of the state_dict
            self.register_buffer("ls_ones", torch.ones(dim), persistent=False)
        self.num_features = self.embed_dim = self.head_hidden_size = dim
        self.grad_ready_hook: Callable[[list], None] | None = None
        self._shadow: dict[int, torch.Tensor] | None = None  # id(param) -> bf16 shadow view
        # weight-gradient kernels on a side stream beside the data-gradient chain (SV_SIDE_STREAM=0: off)
        self.overlap_wgrad = os.environ.get("SV_SIDE_STREAM", "1") != "0"
        self.side_wg_per_cu = 1  # the data-gradient GEMMs keep one workgroup per CU free for the side stream
        self._side: dict = {}
        # the backward only records and waits for events, but a captured step of this backbone has not been run:
        # StepEngine(cuda_graph=True) refuses it rather than assume
        self.graph_safe = False
        self.comm_reserve_cus = 0  # data-parallel runs: CUs the backward's GEMM grids leave to RCCL (see ConvNeXtHip)
        self.comm_cu_mask = False
        self.wgrad_target = int(os.environ.get("SV_VIT_WGRAD_WGS", "256"))
        self._register_load_state_dict_pre_hook(self._resample_pos_embed_hook)
        self._init_weights()

    # -- timm init: trunc_normal(.02) for pos_embed and the Linears, zero Linear biases, normal(1e-6) class token; the
    # patch conv keeps nn.Conv2d's default init
    def _init_weights(self) -> None:
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def _resample_pos_embed_hook(self, state_dict, prefix, *args) -> None:
        """Weights trained at another (square) image size: ``pos_embed`` is resampled to this model's grid, as timm's
        checkpoint filter does.  Anything else that does not fit stays the error load_state_dict reports."""
        key = prefix + "pos_embed"
        pe = state_dict.get(key)
        if not isinstance(pe, torch.Tensor) or pe.dim() != 3 or pe.shape[0] != 1 or pe.shape[2] != self.dim \
                or pe.shape[1] == self.pos_embed.shape[1]:
            return
        npt = 0 if self.no_embed_class else 1
        g = math.isqrt(max(pe.shape[1] - npt, 0))
        if g == 0 or g * g != pe.shape[1] - npt:
            return  # not a square grid: the shape mismatch is reported by load_state_dict
        new = self.img_size // PATCH
        state_dict[key] = resample_abs_pos_embed(pe, (new, new), npt)
        global _RESAMPLE_LOGGED
        if not _RESAMPLE_LOGGED:
            _RESAMPLE_LOGGED = True
            _log.info("resampled %s from a %dx%d to a %dx%d grid (bicubic, antialias)", key, g, g, new, new)

    def _use_stream(self) -> bool:
        return self.attn_stream or self.num_tokens > K.ATTN_MAX_N

    # -- precision / weight shadows --------------------------------------------------------------
    @property
    def compute_bf16(self) -> bool:
        return self.precision == "bf16"

    @property
    def act_dtype(self) -> torch.dtype:
        return torch.bfloat16 if self.compute_bf16 else torch.float32

    def set_weight_shadow(self, shadow: dict[int, torch.Tensor] | None) -> None:
        """Install bf16 views kept fresh by the flat optimizer (id(param) -> bf16 tensor)."""
        self._shadow = shadow

    def gemm_weight_params(self) -> list[nn.Parameter]:
        ps = [self.patch_embed.proj.weight]
        for blk in self.blocks:
            ps += [blk.attn.qkv.weight, blk.attn.proj.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight]
        return ps

    def _w(self, p: torch.Tensor, cache: dict) -> torch.Tensor:
        """Weight as the GEMM reads it: f32 param (fp32 mode) or its bf16 shadow."""
        if not self.compute_bf16:
            return p.detach()
        if self._shadow is not None and id(p) in self._shadow:
            return self._shadow[id(p)]
        k = id(p)
        if k not in cache:
            cache[k] = K.cast_bf16(p.detach().contiguous())
        return cache[k]

    def _gamma(self, ls) -> torch.Tensor:
        return ls.gamma if self.has_ls else self.ls_ones

    @staticmethod
    def _block_params(blk) -> list:
        return [p for p in blk.parameters()]

    # -- forward -----------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[-2], x.shape[-1])
        if H != self.img_size or W != self.img_size:
            raise ValueError(
                f"ViT / DeiT-III backbones take {self.img_size}x{self.img_size} images only (got {H}x{W}): set "
                f"ClassificationConfig.output_size / LocalizationConfig.image_size to ({self.img_size}, {self.img_size})")
        if not x.is_cuda:
            raise RuntimeError("ViTHip runs on the MI355X kernel library only (got a CPU tensor)")
        x = x.contiguous() if x.dtype == torch.uint8 else x.float().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad:
            anchor = torch.zeros((), device=x.device, requires_grad=True)
            return _ViTFn.apply(x, anchor, self)
        feat, _ = self._forward_impl(x, save=False)
        return feat

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)

    def _block_forward(self, blk, x, B: int, cache: dict, save: bool):
        """One block over the token matrix x [B * Np, C] f32 -> (the new x, what the backward needs or None)."""
        bf, act = self.compute_bf16, self.act_dtype
        M, C = x.shape
        N, Np = self.num_tokens, self.rows_per_img
        y1, m1, r1 = K.layernorm_fwd(x, blk.norm1.weight, blk.norm1.bias, out_dtype=act)
        qkv = torch.empty(M, 3 * C, device=x.device, dtype=act)
        K.linear_fwd(y1, self._w(blk.attn.qkv.weight, cache), out=qkv, bias=blk.attn.qkv.bias, compute_bf16=bf)
        attn_fwd = K.attn_stream_fwd if self._use_stream() else K.attn_fwd
        o, lse = attn_fwd(qkv, B, N, self.heads, img_rows=Np)
        x1 = torch.empty(M, C, device=x.device, dtype=torch.float32)
        K.linear_fwd(o, self._w(blk.attn.proj.weight, cache), out=x1, bias=blk.attn.proj.bias, gamma=self._gamma(blk.ls1),
                     residual=x, epilogue=nv.SV_EPI_BIAS_GAMMA_RES, compute_bf16=bf)
        y2, m2, r2 = K.layernorm_fwd(x1, blk.norm2.weight, blk.norm2.bias, out_dtype=act)
        a = torch.empty(M, 4 * C, device=x.device, dtype=act)
        gh = None
        w1 = self._w(blk.mlp.fc1.weight, cache)
        if save:  # a = GELU(h) (fc2 operand) and gh = GELU'(h) (for the backward) from one erf
            gh = torch.empty(M, 4 * C, device=x.device, dtype=act)
            K.linear_fwd(y2, w1, out=gh, out2=a, bias=blk.mlp.fc1.bias, epilogue=nv.SV_EPI_BIAS_GELU_DUAL, compute_bf16=bf)
        else:
            K.linear_fwd(y2, w1, out=a, bias=blk.mlp.fc1.bias, epilogue=nv.SV_EPI_BIAS_GELU, compute_bf16=bf)
        x2 = torch.empty(M, C, device=x.device, dtype=torch.float32)
        K.linear_fwd(a, self._w(blk.mlp.fc2.weight, cache), out=x2, bias=blk.mlp.fc2.bias, gamma=self._gamma(blk.ls2),
                     residual=x1, epilogue=nv.SV_EPI_BIAS_GAMMA_RES, compute_bf16=bf)
        return x2, ((x, y1, m1, r1, qkv, o, lse, x1, y2, m2, r2, gh, a) if save else None)

    @torch.no_grad()
    def _forward_impl(self, img: torch.Tensor, save: bool):
        bf, act = self.compute_bf16, self.act_dtype
        B = img.shape[0]
        C, P, Np = self.dim, self.num_patches, self.rows_per_img
        tape = _Tape(B=B) if save else None
        cache: dict = tape.wcache if save else {}
        proj = self.patch_embed.proj
        # the patch rows inside the padded token layout (row 0 of an image: the class token's, zero here; rows > P: pad)
        patches = K.patchify16(img, out_dtype=act, rows_per_img=Np, row0=1)
        pe = torch.empty(B * Np, C, device=img.device, dtype=torch.float32)
        K.linear_fwd(patches, self._w(proj.weight, cache).view(C, 3 * PATCH * PATCH), out=pe, bias=proj.bias,
                     compute_bf16=bf)
        x = K.vit_tokens(pe, self.cls_token.detach().view(-1), self.pos_embed.detach().view(-1, C), B, P, Np,
                         pos_has_cls=not self.no_embed_class)
        if save:
            tape.patches = patches
        for blk in self.blocks:
            x, saved = self._block_forward(blk, x, B, cache, save)
            if save:
                tape.blocks.append(saved)
        # global_pool='token': the final norm only needs the class rows
        xc = x.view(B, Np, C)[:, 0].contiguous()
        feat, h_mean, h_rstd = K.layernorm_fwd(xc, self.norm.weight, self.norm.bias, out_dtype=torch.float32)
        if save:
            tape.head = (xc, h_mean, h_rstd)
        return feat, tape

    # -- backward ----------------------------------------------------------------------------------
    def _res_branch_backward(self, lin, ls, operand, dsrc, out, wg: _Wgrads, cache, aux=None):
        """The data gradient of out = x + gamma (.) (operand W^T + b) w.r.t. ``operand`` into ``out`` (times ``aux``
        when given: GELU'), and the W / b / gamma gradients as a job for ``wg``."""
        bf, g = self.compute_bf16, self._grad
        epi = nv.SV_EPI_MUL_AUX if aux is not None else nv.SV_EPI_STORE

        def wgrad(policy):
            if self.has_ls:  # dW = gamma (.) d^T a, dgamma = rowdot(W, d^T a) + b (.) colsum(d), db = gamma (.) colsum(d)
                K.layerscale_wgrad(dsrc, operand, lin.weight.detach(), ls.gamma.detach(), lin.bias.detach(),
                                   dw2=g(lin.weight), dgamma=g(ls.gamma), db2=g(lin.bias), compute_bf16=bf,
                                   policy=policy, wgrad_target=self.wgrad_target)
            else:
                K.linear_wgrad(dsrc, operand, out=g(lin.weight), accumulate=True, bias_out=g(lin.bias), compute_bf16=bf,
                               policy=policy, wgrad_target=self.wgrad_target)

        wg.submit(wgrad)
        if not self.has_ls:
            K.linear_dgrad(dsrc, self._w(lin.weight, cache), out=out, epilogue=epi, aux=aux, compute_bf16=bf,
                           policy=wg.pol)
        elif bf:  # gamma folded into a bf16 copy of W
            wgm = K.scale_rows_bf16(lin.weight.detach(), ls.gamma.detach())
            K.linear_dgrad(dsrc, wgm, out=out, epilogue=epi, aux=aux, compute_bf16=True, policy=wg.pol)
        else:
            K.linear_dgrad(dsrc, lin.weight.detach(), out=out, epilogue=epi, a_scale_k=ls.gamma, aux=aux,
                           compute_bf16=False, policy=wg.pol)

    def _block_backward(self, blk, saved, d, B: int, wg: _Wgrads, cache: dict, ready: bool = True):
        """Backward of one block given the f32 gradient stream ``d`` [B * Np, C] (updated in place and returned).  The
        data-gradient chain runs on the main stream: fc2 dgrad (x GELU'), fc1 dgrad, LayerNorm backward, proj dgrad,
        attention backward, qkv dgrad, LayerNorm backward; the four weight-gradient GEMMs are jobs for ``wg``."""
        bf, act, g = self.compute_bf16, self.act_dtype, self._grad
        x, y1, m1, r1, qkv, o, lse, x1, y2, m2, r2, gh, a = saved
        M, C = x.shape
        N, Np = self.num_tokens, self.rows_per_img
        fc1, aq = blk.mlp.fc1, blk.attn.qkv
        # ---- MLP branch
        dsrc = K.cast_bf16(d) if bf else d
        dh = torch.empty(M, 4 * C, device=d.device, dtype=act)
        self._res_branch_backward(blk.mlp.fc2, blk.ls2, a, dsrc, dh, wg, cache, aux=gh)
        wg.submit(lambda policy: K.linear_wgrad(dh, y2, out=g(fc1.weight), accumulate=True, bias_out=g(fc1.bias),
                                                compute_bf16=bf, policy=policy, wgrad_target=self.wgrad_target))
        dy2 = torch.empty(M, C, device=d.device, dtype=torch.float32)
        K.linear_dgrad(dh, self._w(fc1.weight, cache), out=dy2, compute_bf16=bf, policy=wg.pol)
        K.layernorm_bwd(dy2, x1, m2, r2, blk.norm2.weight, dw=g(blk.norm2.weight), db=g(blk.norm2.bias), dx=d,
                        accumulate_dx=True)
        # ---- attention branch
        dsrc = K.cast_bf16(d) if bf else d
        do = torch.empty(M, C, device=d.device, dtype=act)
        self._res_branch_backward(blk.attn.proj, blk.ls1, o, dsrc, do, wg, cache)
        attn_bwd = K.attn_stream_bwd if self._use_stream() else K.attn_bwd
        dqkv = attn_bwd(qkv, o, lse, do, B, N, self.heads, img_rows=Np)
        dy1 = torch.empty(M, C, device=d.device, dtype=torch.float32)
        K.linear_dgrad(dqkv, self._w(aq.weight, cache), out=dy1, compute_bf16=bf, policy=wg.pol)
        K.layernorm_bwd(dy1, x, m1, r1, blk.norm1.weight, dw=g(blk.norm1.weight), db=g(blk.norm1.bias), dx=d,
                        accumulate_dx=True)
        # every gradient of the block is final on the reporting stream after this job (it is ordered behind the
        # LayerNorm folds above through the main -> side event)
        wg.submit(lambda policy: K.linear_wgrad(dqkv, y1, out=g(aq.weight), accumulate=True, bias_out=g(aq.bias),
                                                compute_bf16=bf, policy=policy, wgrad_target=self.wgrad_target),
                  ready=self._block_params(blk) if ready else None)
        return d

    def _wgrads(self) -> _Wgrads:
        main = torch.cuda.current_stream()
        # fp32 (parity mode): one stream -- the weight gradients read the f32 gradient stream itself, which the
        # LayerNorm backwards update in place
        side = self._side_stream(main.device) if self.overlap_wgrad and self.compute_bf16 else None
        pol = nv.policy(grid_cap=_comm_cap(main.device, self.comm_reserve_cus),
                        wg_per_cu=self.side_wg_per_cu if side is not None else 0)
        return _Wgrads(self, main, side, pol)

    @torch.no_grad()
    def _backward_impl(self, tape: _Tape, dfeat: torch.Tensor) -> None:
        bf, g = self.compute_bf16, self._grad
        cache: dict = tape.wcache
        B, C, N, Np = tape.B, self.dim, self.num_tokens, self.rows_per_img
        wg = self._wgrads()
        xc, h_mean, h_rstd = tape.head
        dxc = K.layernorm_bwd(dfeat.float().contiguous(), xc, h_mean, h_rstd, self.norm.weight, dw=g(self.norm.weight),
                              db=g(self.norm.bias))
        # d: the f32 gradient stream over the token matrix; only the class rows have a gradient to start with
        d = torch.zeros(B * Np, C, device=dxc.device, dtype=torch.float32)
        d.view(B, Np, C)[:, 0] = dxc
        self._ready([self.norm.weight, self.norm.bias])
        for i in range(len(self.blocks) - 1, -1, -1):
            saved, tape.blocks[i] = tape.blocks[i], None
            d = self._block_backward(self.blocks[i], saved, d, B, wg, cache)
        # the class-token and position-embedding gradients: sums over the batch of the block-0 input gradient
        d3 = d.view(B, Np, C)
        g(self.cls_token).add_(d3[:, 0].sum(0).view(1, 1, C))
        g(self.pos_embed).add_(d3[:, (1 if self.no_embed_class else 0):N].sum(0, keepdim=True))
        # the patch embedding has no data gradient; its weight gradient is one wgrad GEMM over the token rows (the
        # class and pad rows of `patches` are zero), its bias gradient the sum of the patch rows' gradient
        proj = self.patch_embed.proj
        K.linear_wgrad(K.cast_bf16(d) if bf else d, tape.patches, out=g(proj.weight).view(C, 3 * PATCH * PATCH),
                       accumulate=True, compute_bf16=bf, policy=wg.pol, wgrad_target=self.wgrad_target)
        g(proj.bias).add_(d3[:, 1:N].sum((0, 1)))
        wg.join()
        self._ready([self.cls_token, self.pos_embed, proj.weight, proj.bias])


def resample_abs_pos_embed(posemb: torch.Tensor, new_grid, num_prefix_tokens: int = 1) -> torch.Tensor:
    """A [1, prefix + g * g, C] absolute position embedding on another grid (timm 1.0.22 ``resample_abs_pos_embed``
    as published): the prefix tokens are copied, the grid part is interpolated in float as a [1, C, g, g] image
    (bicubic, antialias, align_corners=False) and cast back."""
    new_h, new_w = (new_grid, new_grid) if isinstance(new_grid, int) else new_grid
    prefix, grid = posemb[:, :num_prefix_tokens], posemb[:, num_prefix_tokens:]
    g = math.isqrt(grid.shape[1])
    if g * g != grid.shape[1]:
        raise ValueError(f"position embedding of {grid.shape[1]} grid tokens is not square")
    if (g, g) == (new_h, new_w):
        return posemb
    C = posemb.shape[-1]
    img = grid.reshape(1, g, g, C).permute(0, 3, 1, 2).float()
    img = F.interpolate(img, size=(new_h, new_w), mode="bicubic", antialias=True, align_corners=False)
    grid = img.permute(0, 2, 3, 1).reshape(1, new_h * new_w, C).to(posemb.dtype)
    return torch.cat([prefix, grid], dim=1) if num_prefix_tokens else grid


def default_img_size() -> int:
    """The image size of a ViT / DeiT-III built without one: env SV_VIT_IMG_SIZE, else 224."""
    return int(os.environ.get("SV_VIT_IMG_SIZE", "224"))


def create_vit(name: str, precision: str = "bf16", img_size=None) -> ViTHip:
    key = name.split(".")[0]
    if img_size is None:
        img_size = default_img_size()
    if key not in VIT_CFGS:
        raise ValueError(f"unsupported ViT / DeiT-III variant {name!r}")
    dim, depth, heads, ls_init, no_embed_class = VIT_CFGS[key]
    return ViTHip(dim, depth, heads, ls_init=ls_init, no_embed_class=no_embed_class, img_size=img_size,
                  precision=precision)
