"""Swin Transformer backbones on the gfx950 kernel library -- drop-in for
``timm.create_model("swin_{tiny,small,base}_patch4_window7_224...", num_classes=0)`` as called at
spine_vision/training/models/backbone.py:166-170.

timm is not a dependency of this package, so the architecture is restated here (timm 1.0.x
``timm/models/swin_transformer.py`` as published; tests/_swin_ref.py is the plain ``torch.nn`` form the tests compare
against): ``SwinTransformer`` with patch 4, window 7, MLP ratio 4, erf GELU, LayerNorm eps 1e-5, head dimension 32,
``qkv_bias=True``, a learned relative-position bias per block, shifted windows in the odd blocks of a stage,
``PatchMerging`` between the stages, ``drop_path_rate=0.1`` (timm's default for this class, which the reference does
not override) and the mean over the tokens of the final norm.  The image size is strict: one square ``img_size``, a
multiple of 224 (window 7) or of 256 (window 8, timm's ``create_model(..., img_size=S, window_size=8)``); an input
of another size raises ``ValueError``.  A relative-position table saved at another window size is refused (resampling
it is not built).

* Same module tree and ``state_dict`` keys as timm (``patch_embed.{proj,norm}``, ``layers.s.downsample.{norm,
  reduction}``, ``layers.s.blocks.j.{norm1,attn.relative_position_bias_table,attn.qkv,attn.proj,norm2,mlp.fc1,
  mlp.fc2}``, ``norm``); ``relative_position_index`` / ``attn_mask`` entries of old checkpoints are dropped on load.
  The sub-modules are parameter containers only; their own ``forward`` is never called.
* Forward and backward are explicit kernel sequences over the f32 residual stream of a stage, [rows_s, C_s] in image
  raster order (DESIGN.md "Swin"): the ConvNeXt stem kernels (4x4 / stride-4 conv + LayerNorm) are ``patch_embed``;
  per block LayerNorm -> qkv GEMM (+bias) -> ``sv_winattn_fwd`` (roll, window partition, bias, mask and their
  inverses as addressing) -> proj GEMM (+bias, +residual) -> LayerNorm -> fc1 GEMM (+bias, GELU and GELU') -> fc2
  GEMM (+bias, +residual); between stages ``sv_patch_merge`` -> LayerNorm(4C) -> the bias-free reduction GEMM; the
  final LayerNorm over all rows and the average pool.
* Row layout: rows_s = B * H_s * W_s rounded up to a multiple of 8 (B * 196 and B * 49 are not for every B).  The
  tail rows are zero where they enter a stage, are never read by the window attention (which writes zeros there),
  and have exactly zero gradient everywhere in the backward.
* Stochastic depth: in train mode block k of the sum(depths) blocks drops each sample's residual branch with
  probability linspace(0, drop_path_rate, sum(depths))[k] and scales the kept ones by 1 / (1 - p); the two branches
  of a block draw independently (``torch.rand`` on the device), one draw covers a branch's forward and backward.  A
  branch with p = 0 keeps the fused bias + residual GEMM epilogue; one with p > 0 stores the GEMM's result to a
  scratch and runs ``sv_rowscale_add``, its backward enters through ``sv_rowscale_cast_bf16``.
  ``drop_path_scales`` (a callable ``(block, branch, B) -> f32 [B]`` of 0 or 1 / (1 - p) entries) replaces the draw.
* ``precision="bf16"``: bf16 MFMA, bf16 saved GEMM operands, f32 residual / gradient streams, f32 master weights.
  ``precision="fp32"``: every GEMM and LayerNorm in f32 on this library (parity mode); the window attention then runs
  as torch ops on gathered windows (``kernels.winattn_*``, the ``SV_WINATTN=torch`` arm) and the stochastic-depth
  gradient scaling as a torch multiply.
* The weight gradients run on a side stream beside the data-gradient chain in bf16 mode (``SV_SIDE_STREAM=0``: the
  same kernels on one stream, the same bits); ``grad_ready_hook`` is called after each block.
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
from .convnext import _comm_cap
from .vit import _Wgrads

# name -> (C, depths, heads per stage)
SWIN_CFGS = {
    "swin_tiny": (96, (2, 2, 6, 2), (3, 6, 12, 24)),
    "swin_small": (96, (2, 2, 18, 2), (3, 6, 12, 24)),
    "swin_base": (128, (2, 2, 18, 2), (4, 8, 16, 32)),
}
PATCH = 4
HEAD_DIM = 32
EPS = 1e-5  # nn.LayerNorm's default, which timm's Swin keeps


def window_for(img_size: int) -> int:
    """Window side of an image size: 7 for the multiples of 224, 8 for the multiples of 256."""
    if img_size > 0 and img_size % 224 == 0:
        return 7
    if img_size > 0 and img_size % 256 == 0:
        return 8
    raise ValueError(
        f"Swin backbones take square images whose side is a multiple of 224 (window 7) or 256 (window 8), got "
        f"{img_size}: set ClassificationConfig.output_size / LocalizationConfig.image_size accordingly")


class _PatchEmbed(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=PATCH, stride=PATCH)
        self.norm = nn.LayerNorm(dim, eps=EPS)


class _WindowAttention(nn.Module):
    def __init__(self, dim: int, heads: int, window: int) -> None:
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)


class SwinBlock(nn.Module):
    """Parameter container for timm ``SwinTransformerBlock``; ``window`` / ``shift`` as timm resolves them (a grid no
    larger than the window: the window is the grid and nothing shifts)."""

    def __init__(self, dim: int, grid: int, heads: int, window: int, shift: int, drop_path: float, index: int) -> None:
        super().__init__()
        if grid <= window:
            window, shift = grid, 0
        self.grid, self.heads, self.window, self.shift = grid, heads, window, shift
        self.drop_path, self.index = float(drop_path), index
        self.norm1 = nn.LayerNorm(dim, eps=EPS)
        self.attn = _WindowAttention(dim, heads, window)
        self.norm2 = nn.LayerNorm(dim, eps=EPS)
        self.mlp = _Mlp(dim)


class _PatchMerging(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim, eps=EPS)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)


class SwinStage(nn.Module):
    def __init__(self, dim: int, grid: int, depth: int, heads: int, window: int, downsample: bool, dprs: list,
                 first: int) -> None:
        super().__init__()
        self.dim, self.grid = dim, grid
        self.downsample = _PatchMerging(dim // 2) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[SwinBlock(dim, grid, heads, window, 0 if j % 2 == 0 else window // 2, dprs[j],
                                                first + j) for j in range(depth)])


@dataclass
class _Tape:
    """Activations saved by the training forward for the explicit backward."""

    B: int
    img: torch.Tensor = None
    stem: tuple = ()
    stages: list = field(default_factory=list)  # per stage: (merge tuple or None, [per block: saved tuple])
    head: tuple = ()
    wcache: dict = field(default_factory=dict)  # bf16 weight casts shared by forward and backward (no shadow)


class _SwinFn(torch.autograd.Function):
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


def _rows8(n: int) -> int:
    return -(-n // 8) * 8


class SwinHip(ExplicitBackward, nn.Module):
    def __init__(self, dim: int = 96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), img_size: int | tuple[int, int] = 224,
                 drop_path_rate: float = 0.1, precision: str = "bf16") -> None:
        super().__init__()
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if isinstance(img_size, (tuple, list)):
            if len(img_size) != 2 or img_size[0] != img_size[1]:
                raise ValueError(f"img_size must be square, got {tuple(img_size)}: set ClassificationConfig.output_size "
                                 f"/ LocalizationConfig.image_size to a square size")
            img_size = img_size[0]
        img_size = int(img_size)
        window = window_for(img_size)
        if len(depths) != len(heads):
            raise ValueError("depths and heads must have one entry per stage")
        for s, h in enumerate(heads):
            if dim * 2 ** s != h * HEAD_DIM:
                raise ValueError(f"head dimension must be {HEAD_DIM}: stage {s} has width {dim * 2 ** s}, {h} heads")
            grid = img_size // PATCH // 2 ** s
            if grid > window and grid % window:
                raise ValueError(f"img_size {img_size}: the {grid}x{grid} grid of stage {s} is no multiple of the "
                                 f"window {window} (timm's padding path is not built)")
        self.dim, self.depths, self.heads = dim, tuple(depths), tuple(heads)
        self.img_size, self.window = img_size, window
        self.drop_path_rate = float(drop_path_rate)
        self.precision = precision
        self.patch_embed = _PatchEmbed(dim)
        dpr = torch.linspace(0, self.drop_path_rate, sum(depths)).tolist()
        stages, first = [], 0
        for s, depth in enumerate(depths):
            stages.append(SwinStage(dim * 2 ** s, img_size // PATCH // 2 ** s, depth, heads[s], window, s > 0,
                                    dpr[first:first + depth], first))
            first += depth
        self.layers = nn.Sequential(*stages)
        self.num_features = self.embed_dim = self.head_hidden_size = dim * 2 ** (len(depths) - 1)
        self.norm = nn.LayerNorm(self.num_features, eps=EPS)
        # the bias + residual epilogue (SV_EPI_BIAS_GAMMA_RES) with a layer scale of exactly one, per stage width; not
        # persistent: they stay out of the state_dict
        for s in range(len(depths)):
            self.register_buffer(f"ls_ones{s}", torch.ones(dim * 2 ** s), persistent=False)
        # test hook: callable(block index, branch 0 | 1, B) -> f32 [B] of 0 or 1 / (1 - p) on the device
        self.drop_path_scales: Callable | None = None
        self.grad_ready_hook: Callable[[list], None] | None = None
        self._shadow: dict[int, torch.Tensor] | None = None  # id(param) -> bf16 shadow view
        self.overlap_wgrad = os.environ.get("SV_SIDE_STREAM", "1") != "0"
        self.side_wg_per_cu = 1  # the data-gradient GEMMs keep one workgroup per CU free for the side stream
        self._side: dict = {}
        # a captured step of this backbone has not been run: StepEngine(cuda_graph=True) refuses it
        self.graph_safe = False
        self.comm_reserve_cus = 0
        self.comm_cu_mask = False
        self.wgrad_target = int(os.environ.get("SV_VIT_WGRAD_WGS", "256"))
        self._register_load_state_dict_pre_hook(self._load_hook)
        self._init_weights()

    # -- timm init: trunc_normal(.02) for the Linears and the bias tables, zero Linear biases; the patch conv keeps
    # nn.Conv2d's default init
    def _init_weights(self) -> None:
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, _WindowAttention):
                nn.init.trunc_normal_(m.relative_position_bias_table, std=0.02)

    def _load_hook(self, state_dict, prefix, *args) -> None:
        """Old checkpoints carry the (now non-persistent) ``relative_position_index`` / ``attn_mask`` buffers: dropped.
        A bias table of another window size is refused here with the reason (load_state_dict would only report a
        shape)."""
        for key in [k for k in state_dict if k.startswith(prefix)
                    and k.endswith(("relative_position_index", "attn_mask"))]:
            del state_dict[key]
        own = {prefix + n: p for n, p in self.named_parameters() if n.endswith("relative_position_bias_table")}
        for key, p in own.items():
            t = state_dict.get(key)
            if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] != p.shape[0]:
                raise ValueError(
                    f"{key}: a relative-position table of {t.shape[0]} entries does not fit this model's "
                    f"{p.shape[0]} (window {self.window} at img_size {self.img_size}); resampling a table to another "
                    f"window size is not built -- build the model at the checkpoint's window (224: 7, 256: 8)")

    def all_blocks(self) -> list:
        return [blk for st in self.layers for blk in st.blocks]

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
        ps = []
        for st in self.layers:
            if isinstance(st.downsample, _PatchMerging):
                ps.append(st.downsample.reduction.weight)
            for blk in st.blocks:
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

    # -- stochastic depth ----------------------------------------------------------------------------
    def _scales(self, blk: SwinBlock, branch: int, B: int, device) -> torch.Tensor | None:
        """The per-sample scale vector of one residual branch (None: the branch is never dropped)."""
        if not self.training or blk.drop_path <= 0.0:
            return None
        if self.drop_path_scales is not None:
            s = self.drop_path_scales(blk.index, branch, B)
            return None if s is None else s.to(device=device, dtype=torch.float32).contiguous()
        keep = 1.0 - blk.drop_path
        return (torch.rand(B, device=device) < keep).to(torch.float32) / keep

    # -- forward -----------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[-2], x.shape[-1])
        if H != self.img_size or W != self.img_size:
            raise ValueError(
                f"Swin backbones take {self.img_size}x{self.img_size} images only (got {H}x{W}): set "
                f"ClassificationConfig.output_size / LocalizationConfig.image_size to ({self.img_size}, {self.img_size})")
        if not x.is_cuda:
            raise RuntimeError("SwinHip runs on the MI355X kernel library only (got a CPU tensor)")
        if x.dtype == torch.uint8:
            # decoded grayscale batch [B,H,W]: the reference transform runs inside the stem gather (bf16) or as the
            # standalone normalise kernel (fp32 parity mode), as for ConvNeXt
            x = x.contiguous() if self.compute_bf16 else K.normalize_u8_gray(x.contiguous())
        else:
            x = x.float().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad:
            anchor = torch.zeros((), device=x.device, requires_grad=True)
            return _SwinFn.apply(x, anchor, self)
        feat, _ = self._forward_impl(x, save=False)
        return feat

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)

    def _res_branch_forward(self, lin, operand, x, ones, scales, hw: int, cache: dict):
        """x + (operand W^T + b), or x + s (.) (operand W^T + b) per sample when the branch can drop."""
        bf = self.compute_bf16
        out = torch.empty_like(x)
        if scales is None:
            K.linear_fwd(operand, self._w(lin.weight, cache), out=out, bias=lin.bias, gamma=ones, residual=x,
                         epilogue=nv.SV_EPI_BIAS_GAMMA_RES, compute_bf16=bf)
            return out
        t = torch.empty_like(x)
        K.linear_fwd(operand, self._w(lin.weight, cache), out=t, bias=lin.bias, compute_bf16=bf)
        return K.rowscale_add(x, t, scales, hw, out=out)

    def _block_forward(self, blk: SwinBlock, x, B: int, ones, cache: dict, save: bool):
        """One block over the stage's stream x [rows, C] f32 -> (the new x, what the backward needs or None)."""
        bf, act = self.compute_bf16, self.act_dtype
        M, C = x.shape
        g, w = blk.grid, blk.window
        s1, s2 = self._scales(blk, 0, B, x.device), self._scales(blk, 1, B, x.device)
        y1, m1, r1 = K.layernorm_fwd(x, blk.norm1.weight, blk.norm1.bias, out_dtype=act, eps=EPS)
        qkv = torch.empty(M, 3 * C, device=x.device, dtype=act)
        K.linear_fwd(y1, self._w(blk.attn.qkv.weight, cache), out=qkv, bias=blk.attn.qkv.bias, compute_bf16=bf)
        bias = K.swin_bias_expand(blk.attn.relative_position_bias_table.detach(), w)
        o, lse = K.winattn_fwd(qkv, bias, B, g, g, w, blk.shift, blk.heads)
        x1 = self._res_branch_forward(blk.attn.proj, o, x, ones, s1, g * g, cache)
        y2, m2, r2 = K.layernorm_fwd(x1, blk.norm2.weight, blk.norm2.bias, out_dtype=act, eps=EPS)
        a = torch.empty(M, 4 * C, device=x.device, dtype=act)
        gh = None
        w1 = self._w(blk.mlp.fc1.weight, cache)
        if save:  # a = GELU(h) (fc2 operand) and gh = GELU'(h) (for the backward) from one erf
            gh = torch.empty(M, 4 * C, device=x.device, dtype=act)
            K.linear_fwd(y2, w1, out=gh, out2=a, bias=blk.mlp.fc1.bias, epilogue=nv.SV_EPI_BIAS_GELU_DUAL, compute_bf16=bf)
        else:
            K.linear_fwd(y2, w1, out=a, bias=blk.mlp.fc1.bias, epilogue=nv.SV_EPI_BIAS_GELU, compute_bf16=bf)
        x2 = self._res_branch_forward(blk.mlp.fc2, a, x1, ones, s2, g * g, cache)
        return x2, ((x, y1, m1, r1, qkv, bias, o, lse, x1, y2, m2, r2, gh, a, s1, s2) if save else None)

    @torch.no_grad()
    def _forward_impl(self, img: torch.Tensor, save: bool):
        bf, act = self.compute_bf16, self.act_dtype
        B = img.shape[0]
        tape = _Tape(B=B, img=img) if save else None
        cache: dict = tape.wcache if save else {}
        conv, ln = self.patch_embed.proj, self.patch_embed.norm
        C0 = self.dim
        if bf:  # the ConvNeXt stem: 4x4 patch rows (bf16, K padded to 64) x packed weight on MFMA, then LayerNorm
            patches = K.stem_patchify(img)
            z0 = torch.empty(patches.shape[0], C0, device=img.device, dtype=act)
            K.linear_fwd(patches, K.stem_weight_pack(conv.weight.detach()), out=z0, bias=conv.bias, compute_bf16=True)
            x, s_mean, s_rstd = K.layernorm_fwd(z0, ln.weight, ln.bias, out_dtype=torch.float32, eps=EPS)
            if save:
                tape.stem = (patches, z0, s_mean, s_rstd)
        else:
            x4, s_mean, s_rstd = K.stem_fwd(img, conv.weight, conv.bias, ln.weight, ln.bias, eps=EPS)
            x = x4.view(-1, C0)
            if save:
                tape.stem = (s_mean, s_rstd)
        g = self.img_size // PATCH
        if x.shape[0] % 8:  # B * g * g is a multiple of 8 at every accepted size; kept for completeness
            x = torch.cat([x, x.new_zeros(_rows8(x.shape[0]) - x.shape[0], C0)])
        for s, st in enumerate(self.layers):
            merge_saved = None
            if s > 0:
                ds = st.downsample
                n = B * (g // 2) ** 2
                rows = _rows8(n)
                xm = K.patch_merge(x, B, g, g, rows_out=rows)
                ym, mm, rm = K.layernorm_fwd(xm, ds.norm.weight, ds.norm.bias, out_dtype=act, eps=EPS)
                x = torch.empty(rows, st.dim, device=img.device, dtype=torch.float32)
                K.linear_fwd(ym, self._w(ds.reduction.weight, cache), out=x, compute_bf16=bf)
                if rows > n:
                    x[n:].zero_()  # the tail rows enter the stage as zeros
                merge_saved = (xm, ym, mm, rm, g)
                g //= 2
            ones = getattr(self, f"ls_ones{s}")
            saved_blocks = []
            for blk in st.blocks:
                x, saved = self._block_forward(blk, x, B, ones, cache, save)
                saved_blocks.append(saved)
            if save:
                tape.stages.append((merge_saved, saved_blocks))
        C = self.num_features
        yn, h_mean, h_rstd = K.layernorm_fwd(x, self.norm.weight, self.norm.bias, out_dtype=torch.float32, eps=EPS)
        feat = K.avgpool_fwd(yn[:B * g * g].view(B, g, g, C))
        if save:
            tape.head = (x, h_mean, h_rstd, g)
        return feat, tape

    # -- backward ----------------------------------------------------------------------------------
    def _branch_dsrc(self, d, scales, hw: int):
        """The gradient entering a residual branch: the stream ``d``, scaled per sample where the branch can drop, in
        the GEMM operand's dtype."""
        if scales is None:
            return K.cast_bf16(d) if self.compute_bf16 else d
        if self.compute_bf16:
            return K.rowscale_cast_bf16(d, scales, hw)
        rows = torch.zeros(d.shape[0], device=d.device, dtype=torch.float32)
        rows[:scales.shape[0] * hw] = scales.repeat_interleave(hw)
        return d * rows.unsqueeze(1)

    def _res_branch_backward(self, lin, operand, dsrc, out, wg: _Wgrads, cache, aux=None):
        """The data gradient of x + (operand W^T + b) w.r.t. ``operand`` into ``out`` (times ``aux`` when given:
        GELU'), and the W / b gradients as a job for ``wg``."""
        bf, g = self.compute_bf16, self._grad
        wg.submit(lambda policy: K.linear_wgrad(dsrc, operand, out=g(lin.weight), accumulate=True, bias_out=g(lin.bias),
                                                compute_bf16=bf, policy=policy, wgrad_target=self.wgrad_target))
        K.linear_dgrad(dsrc, self._w(lin.weight, cache), out=out,
                       epilogue=nv.SV_EPI_MUL_AUX if aux is not None else nv.SV_EPI_STORE, aux=aux, compute_bf16=bf,
                       policy=wg.pol)

    def _block_backward(self, blk: SwinBlock, saved, d, B: int, wg: _Wgrads, cache: dict):
        """Backward of one block given the f32 gradient stream ``d`` [rows, C] (updated in place and returned): fc2
        dgrad (x GELU'), fc1 dgrad, LayerNorm backward, proj dgrad, window-attention backward, the bias-table gradient,
        qkv dgrad, LayerNorm backward on the main stream; the four weight-gradient GEMMs are jobs for ``wg``."""
        bf, act, g = self.compute_bf16, self.act_dtype, self._grad
        x, y1, m1, r1, qkv, bias, o, lse, x1, y2, m2, r2, gh, a, s1, s2 = saved
        M, C = x.shape
        gr, w = blk.grid, blk.window
        fc1, aq = blk.mlp.fc1, blk.attn.qkv
        # ---- MLP branch
        dsrc = self._branch_dsrc(d, s2, gr * gr)
        dh = torch.empty(M, 4 * C, device=d.device, dtype=act)
        self._res_branch_backward(blk.mlp.fc2, a, dsrc, dh, wg, cache, aux=gh)
        wg.submit(lambda policy: K.linear_wgrad(dh, y2, out=g(fc1.weight), accumulate=True, bias_out=g(fc1.bias),
                                                compute_bf16=bf, policy=policy, wgrad_target=self.wgrad_target))
        dy2 = torch.empty(M, C, device=d.device, dtype=torch.float32)
        K.linear_dgrad(dh, self._w(fc1.weight, cache), out=dy2, compute_bf16=bf, policy=wg.pol)
        K.layernorm_bwd(dy2, x1, m2, r2, blk.norm2.weight, dw=g(blk.norm2.weight), db=g(blk.norm2.bias), dx=d,
                        accumulate_dx=True)
        # ---- attention branch
        dsrc = self._branch_dsrc(d, s1, gr * gr)
        do = torch.empty(M, C, device=d.device, dtype=act)
        self._res_branch_backward(blk.attn.proj, o, dsrc, do, wg, cache)
        dqkv, part = K.winattn_bwd(qkv, o, lse, do, bias, B, gr, gr, w, blk.shift, blk.heads)
        K.swin_bias_grad(part, g(blk.attn.relative_position_bias_table), w, accumulate=True)
        dy1 = torch.empty(M, C, device=d.device, dtype=torch.float32)
        K.linear_dgrad(dqkv, self._w(aq.weight, cache), out=dy1, compute_bf16=bf, policy=wg.pol)
        K.layernorm_bwd(dy1, x, m1, r1, blk.norm1.weight, dw=g(blk.norm1.weight), db=g(blk.norm1.bias), dx=d,
                        accumulate_dx=True)
        # every gradient of the block is final on the reporting stream after this job (it is ordered behind the
        # LayerNorm and bias-table folds above through the main -> side event)
        wg.submit(lambda policy: K.linear_wgrad(dqkv, y1, out=g(aq.weight), accumulate=True, bias_out=g(aq.bias),
                                                compute_bf16=bf, policy=policy, wgrad_target=self.wgrad_target),
                  ready=[p for p in blk.parameters()])
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
        B, C = tape.B, self.num_features
        wg = self._wgrads()
        x_last, h_mean, h_rstd, gr = tape.head
        n = B * gr * gr
        dyn = torch.empty(x_last.shape, device=x_last.device, dtype=torch.float32)
        K.avgpool_bwd(dfeat, (B, gr, gr, C), out=dyn[:n].view(B, gr, gr, C))
        if dyn.shape[0] > n:
            dyn[n:].zero_()
        d = K.layernorm_bwd(dyn, x_last, h_mean, h_rstd, self.norm.weight, dw=g(self.norm.weight), db=g(self.norm.bias))
        self._ready([self.norm.weight, self.norm.bias])
        for s in range(len(self.layers) - 1, -1, -1):
            st = self.layers[s]
            merge_saved, saved_blocks = tape.stages[s]
            for j in range(len(st.blocks) - 1, -1, -1):
                saved, saved_blocks[j] = saved_blocks[j], None
                d = self._block_backward(st.blocks[j], saved, d, B, wg, cache)
            if merge_saved is not None:
                ds = st.downsample
                xm, ym, mm, rm, g_prev = merge_saved
                dsrc = K.cast_bf16(d) if bf else d
                wg.submit(lambda policy, dsrc=dsrc, ym=ym, ds=ds: K.linear_wgrad(
                    dsrc, ym, out=g(ds.reduction.weight), accumulate=True, compute_bf16=bf, policy=policy,
                    wgrad_target=self.wgrad_target))
                dym = torch.empty(xm.shape, device=d.device, dtype=torch.float32)
                K.linear_dgrad(dsrc, self._w(ds.reduction.weight, cache), out=dym, compute_bf16=bf, policy=wg.pol)
                dxm = K.layernorm_bwd(dym, xm, mm, rm, ds.norm.weight, dw=g(ds.norm.weight), db=g(ds.norm.bias))
                d = K.patch_merge_bwd(dxm, B, g_prev, g_prev, rows_in=_rows8(B * g_prev * g_prev))
                wg.submit(lambda policy: None, ready=[p for p in ds.parameters()])
        conv, ln = self.patch_embed.proj, self.patch_embed.norm
        C0 = self.dim
        n0 = B * (self.img_size // PATCH) ** 2
        d = d[:n0]
        if bf:
            patches, z0, s_mean, s_rstd = tape.stem
            dz0 = K.layernorm_bwd(d, z0, s_mean, s_rstd, ln.weight, dw=g(ln.weight), db=g(ln.bias),
                                  out_dtype=torch.bfloat16)
            K.linear_wgrad(dz0, patches, out=g(conv.weight).view(C0, 48), accumulate=True, bias_out=g(conv.bias),
                           compute_bf16=True, cols=48, policy=wg.pol)
        else:
            s_mean, s_rstd = tape.stem
            K.stem_bwd(tape.img, conv.weight, conv.bias, ln.weight, s_mean, s_rstd, d, dw=g(conv.weight),
                       db=g(conv.bias), dlnw=g(ln.weight), dlnb=g(ln.bias))
        wg.join()
        self._ready([conv.weight, conv.bias, ln.weight, ln.bias])


def default_img_size() -> int:
    """The image size of a Swin backbone built without one: env SV_SWIN_IMG_SIZE, else 224."""
    return int(os.environ.get("SV_SWIN_IMG_SIZE", "224"))


def create_swin(name: str, precision: str = "bf16", img_size=None, drop_path_rate: float = 0.1,
                depths=None) -> SwinHip:
    """``depths``: other block counts per stage than the variant's (reduced models of the tests)."""
    key = name.split(".")[0]
    if img_size is None:
        img_size = default_img_size()
    if key not in SWIN_CFGS:
        raise ValueError(f"unsupported Swin variant {name!r}")
    dim, d, heads = SWIN_CFGS[key]
    return SwinHip(dim, depths or d, heads, img_size=img_size, drop_path_rate=drop_path_rate, precision=precision)
