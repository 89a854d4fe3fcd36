"""Plain ``torch.nn`` restatement of timm's ``VisionTransformer`` as the reference builds it for ``vit_*`` and ``deit_*``
(``timm.create_model(..., num_classes=0)``): patch 16, ``qkv_bias=True``, MLP ratio 4, erf GELU, LayerNorm eps 1e-6,
``global_pool='token'``, no dropout / drop-path, head dimension 64; DeiT-III: LayerScale (init 1e-6) and
``no_embed_class`` (position embedding over the patches only, added before the class token is prepended).  Test
infrastructure only (timm is not installed): the module tree gives timm's state_dict keys and shapes, and ``forward``
is autograd-differentiable on the CPU in fp32 or float64."""
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
