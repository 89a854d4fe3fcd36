"""Plain ``torch.nn`` restatement of timm's ``VisionTransformer`` as the reference builds it for ``vit_*`` and ``deit_*``
(``timm.create_model(..., num_classes=0)``): patch 16, ``qkv_bias=True``, MLP ratio 4, erf GELU, LayerNorm eps 1e-6,
``global_pool='token'``, no dropout / drop-path, head dimension 64; DeiT-III: LayerScale (init 1e-6) and
``no_embed_class`` (position embedding over the patches only, added before the class token is prepended).  Test
infrastructure only (timm is not installed): the module tree gives timm's state_dict keys and shapes, and ``forward``
is autograd-differentiable on the CPU in fp32 or float64.

``block_restated`` is the float64 restatement of one block as the HIP module's bf16 mode runs it: float64 arithmetic,
rounded to bf16 exactly where the module stores bf16 (the rule of tests/test_attn_gpu.py applied to the block)."""
import math

import torch
import torch.nn as nn

# name -> (C, depth, heads, LayerScale init or None, no_embed_class, parameters with num_classes=0)
CFGS = {
    "vit_tiny": (192, 12, 3, None, False, 5_524_416),
    "vit_small": (384, 12, 6, None, False, 21_665_664),
    "vit_base": (768, 12, 12, None, False, 85_798_656),
    "vit_large": (1024, 24, 16, None, False, 303_301_632),
    "deit_tiny": (384, 12, 6, 1e-6, True, 21_674_496),  # the reference maps deit_tiny to deit3_small
    "deit_small": (384, 12, 6, 1e-6, True, 21_674_496),
    "deit_base": (768, 12, 12, 1e-6, True, 85_816_320),
}
FEATURE_DIMS = {n: c[0] for n, c in CFGS.items()}


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=16, stride=16)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)  # [B, P, C], row-major patch order


class Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        p = torch.softmax(q @ k.transpose(-1, -2) * (C // self.heads) ** -0.5, dim=-1)
        return self.proj((p @ v).transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class LayerScale(nn.Module):
    def __init__(self, dim, init):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Block(nn.Module):
    def __init__(self, dim, heads, ls_init):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, heads)
        self.ls1 = LayerScale(dim, ls_init) if ls_init is not None else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim)
        self.ls2 = LayerScale(dim, ls_init) if ls_init is not None else nn.Identity()

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class VisionTransformer(nn.Module):
    def __init__(self, dim, depth, heads, ls_init=None, no_embed_class=False, img_size=224):
        super().__init__()
        P = (img_size // 16) ** 2
        self.img_size, self.no_embed_class = img_size, no_embed_class
        self.num_features = dim
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, P + (0 if no_embed_class else 1), dim))
        self.patch_embed = PatchEmbed(dim)
        self.blocks = nn.Sequential(*[Block(dim, heads, ls_init) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def tokens(self, x):
        if x.shape[-2] != self.img_size or x.shape[-1] != self.img_size:
            raise ValueError(f"input {tuple(x.shape[-2:])} is not {self.img_size}x{self.img_size}")
        x = self.patch_embed(x)
        cls = self.cls_token.expand(x.shape[0], -1, -1)
        if self.no_embed_class:
            return torch.cat([cls, x + self.pos_embed], dim=1)
        return torch.cat([cls, x], dim=1) + self.pos_embed

    def forward(self, x):
        return self.norm(self.blocks(self.tokens(x)))[:, 0]


def create(name, img_size=224):
    dim, depth, heads, ls_init, no_embed_class, _ = CFGS[name]
    return VisionTransformer(dim, depth, heads, ls_init, no_embed_class, img_size)


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _ln64(x, w, b, eps=1e-6):
    mu = x.mean(-1, keepdim=True)
    rs = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - mu) * rs
    return xh * w + b, xh, rs


def _ln64_bwd(dy, xh, rs, w):
    """-> dx, dw, db of y = xh * w + b"""
    gy = dy * w
    dx = rs * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    C = dy.shape[-1]
    return dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)


def block_restated(blk, x, d, *, rows_per_img, slab_split=None):
    """One block's forward from ``x`` and backward from the output gradient ``d`` (both [B, N, C]) in float64, rounded
    to bf16 where ViTHip (precision="bf16") stores bf16: the four GEMM weights (for DeiT-III's proj / fc2 data
    gradients: bf16(W * gamma[:, None])), y1, qkv, attention's P, o, dS, dq / dk / dv (tests/test_attn_gpu.py), y2,
    a = GELU(h), gh = GELU'(h), the bf16 casts of the gradient stream, dh, do, and each split-K slab of a weight
    gradient where the module takes bf16 slabs.  Everything the module keeps in f32 (the residual and gradient streams,
    LayerNorm, the weight-gradient sums, the layer-scale finish on the f32 master weight) stays float64.

    ``blk``: a ``Block`` (f32 masters); ``slab_split(n, k)``: the number of bf16 slab slices of the weight gradient
    [n, k] over the B * rows_per_img padded rows (1: f32 slabs).  -> dict(out, dx, grads by parameter name)."""
    p = {n: t.detach().double() for n, t in blk.named_parameters()}
    B, N, C = x.shape
    heads, hd = blk.attn.heads, C // blk.attn.heads
    scale = hd ** -0.5
    has_ls = "ls1.gamma" in p
    ones = torch.ones(C, dtype=torch.float64)
    g1, g2 = (p["ls1.gamma"], p["ls2.gamma"]) if has_ls else (ones, ones)
    x, d = x.double(), d.double()
    wq, wp, w1, w2 = (_bf(p[n + ".weight"]) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"))

    def heads_of(t):  # [B, N, C] -> [B, heads, N, hd]
        return t.reshape(B, N, heads, hd).permute(0, 2, 1, 3)

    def merge(t):
        return t.permute(0, 2, 1, 3).reshape(B, N, C)

    def wgrad(dy, a):  # dy^T a over the padded token rows, bf16 slabs where the module takes them
        n, k = dy.shape[-1], a.shape[-1]
        split = 1 if slab_split is None else slab_split(n, k)
        if split == 1:
            return dy.reshape(-1, n).T @ a.reshape(-1, k)
        M = B * rows_per_img
        dyp, ap = torch.zeros(B, rows_per_img, n, dtype=torch.float64), torch.zeros(B, rows_per_img, k, dtype=torch.float64)
        dyp[:, :N], ap[:, :N] = dy, a
        dyp, ap = dyp.view(M, n), ap.view(M, k)
        rows = M // split
        return sum(_bf(dyp[s * rows:(s + 1) * rows].T @ ap[s * rows:(s + 1) * rows]) for s in range(split))

    def branch_grads(lin, ls, G, cs, grads):  # ViTHip._res_branch_backward's weight-gradient job
        if has_ls:
            gam = p[ls + ".gamma"]
            grads[lin + ".weight"] = gam[:, None] * G
            grads[ls + ".gamma"] = (p[lin + ".weight"] * G).sum(1) + p[lin + ".bias"] * cs
            grads[lin + ".bias"] = gam * cs
        else:
            grads[lin + ".weight"], grads[lin + ".bias"] = G, cs

    # ---- forward
    y1f, xh1, rs1 = _ln64(x, p["norm1.weight"], p["norm1.bias"])
    y1 = _bf(y1f)
    qkv = _bf(y1 @ wq.T + p["attn.qkv.bias"]).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    pr = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    oh = _bf(_bf(pr) @ v)
    o = merge(oh)
    x1 = x + g1 * (o @ wp.T + p["attn.proj.bias"])
    y2f, xh2, rs2 = _ln64(x1, p["norm2.weight"], p["norm2.bias"])
    y2 = _bf(y2f)
    h = y2 @ w1.T + p["mlp.fc1.bias"]
    Phi = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
    a, gh = _bf(h * Phi), _bf(Phi + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi))
    out = x1 + g2 * (a @ w2.T + p["mlp.fc2.bias"])
    # ---- backward
    grads = {}
    dsrc = _bf(d)
    w2d = _bf(p["mlp.fc2.weight"] * g2[:, None]) if has_ls else w2
    dh = _bf((dsrc @ w2d) * gh)
    branch_grads("mlp.fc2", "ls2", wgrad(dsrc, a), dsrc.reshape(-1, C).sum(0), grads)
    grads["mlp.fc1.weight"], grads["mlp.fc1.bias"] = wgrad(dh, y2), dh.reshape(-1, 4 * C).sum(0)
    ddx, grads["norm2.weight"], grads["norm2.bias"] = _ln64_bwd(dh @ w1, xh2, rs2, p["norm2.weight"])
    d = d + ddx
    dsrc = _bf(d)
    wpd = _bf(p["attn.proj.weight"] * g1[:, None]) if has_ls else wp
    do = _bf(dsrc @ wpd)
    branch_grads("attn.proj", "ls1", wgrad(dsrc, o), dsrc.reshape(-1, C).sum(0), grads)
    doh = heads_of(do)
    dp = doh @ v.transpose(-1, -2)
    ds = _bf(pr * (dp - (doh * oh).sum(-1, keepdim=True)) * scale)
    dq, dk, dv = _bf(ds @ k), _bf(ds.transpose(-1, -2) @ q), _bf(_bf(pr).transpose(-1, -2) @ doh)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * C)
    grads["attn.qkv.weight"], grads["attn.qkv.bias"] = wgrad(dqkv, y1), dqkv.reshape(-1, 3 * C).sum(0)
    ddx, grads["norm1.weight"], grads["norm1.bias"] = _ln64_bwd(dqkv @ wq, xh1, rs1, p["norm1.weight"])
    return dict(out=out, dx=d + ddx, grads=grads)
