"""Plain ``torch.nn`` restatement of timm's ``SwinTransformer`` as the reference builds it for ``swin_*``
(``timm.create_model("swin_{tiny,small,base}_patch4_window7_224", num_classes=0)``): patch 4, window 7 (8 at the
256-multiples, timm's ``img_size=S, window_size=8``), MLP ratio 4, erf GELU, LayerNorm eps 1e-5, head dimension 32,
``drop_path_rate=0.1`` (linearly increasing over the blocks), final norm then the mean over the tokens.  Test
infrastructure only (timm is not installed): the module tree gives timm's state_dict keys and shapes, ``forward`` is
autograd-differentiable on the CPU in fp32 or float64, and it is written as timm writes it (``torch.roll``,
``window_partition``, an ``attn_mask`` built from slices) -- not from the index formula the HIP kernels use;
``token_rows`` / ``token_regions`` state that formula so that a CPU test can compare the two.

``drop_path_scales``: None (no stochastic depth), or ``callable(block_index, branch, B) -> [B]`` tensor of 0 or
1 / (1 - p) (the hook the HIP module has too).

``winattn_f64`` is float64 windowed attention over raster rows with autograd; ``winattn_restated`` the same rounding to
bf16 exactly where the kernels do (the rule of tests/test_attn_gpu.py).  The last section states each window-attention
call alone in float64 with a per-element error bound, and in float32 with faults that can be switched on
(tests/test_swin_calls_gpu.py, tests/test_swin_calls_cpu.py)."""
import functools

import torch
import torch.nn as nn

# name -> (C, depths, heads, parameters with num_classes=0)
CFGS = {
    "swin_tiny": (96, (2, 2, 6, 2), (3, 6, 12, 24), 27_519_354),
    "swin_small": (96, (2, 2, 18, 2), (3, 6, 12, 24), 48_837_258),
    "swin_base": (128, (2, 2, 18, 2), (4, 8, 16, 32), 86_743_224),
}
FEATURE_DIMS = {n: 8 * c[0] for n, c in CFGS.items()}
MASKED = -100.0


def window_for(img_size):
    if img_size % 224 == 0:
        return 7
    if img_size % 256 == 0:
        return 8
    raise ValueError(f"img_size {img_size}")


def window_partition(x, w):  # [B, H, W, C] -> [B * nW, w, w, C]
    B, H, W, C = x.shape
    x = x.view(B, H // w, w, W // w, w, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, w, w, C)


def window_reverse(win, w, H, W):  # [B * nW, w, w, C] -> [B, H, W, C]
    C = win.shape[-1]
    x = win.view(-1, H // w, W // w, w, w, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, H, W, C)


def relative_position_index(w):
    coords = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")).flatten(1)  # [2, w*w]
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    return rel.sum(-1)  # [w*w, w*w]


def attn_mask(H, W, w, shift):
    """timm's mask of a shifted block: [nW, w*w, w*w], 0 or -100; None when shift = 0."""
    if shift == 0:
        return None
    img = torch.zeros(1, H, W, 1)
    cnt = 0
    for hs in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
        for ws in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
            img[:, hs, ws, :] = cnt
            cnt += 1
    mw = window_partition(img, w).view(-1, w * w)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, MASKED).masked_fill(m == 0, 0.0)


def token_rows(B, H, W, w, shift):
    """The index formula of the kernels: raster row of token (i, j) of window (wy, wx), [B * nW, w*w]."""
    rows = torch.empty(B, H // w, W // w, w, w, dtype=torch.long)
    for wy in range(H // w):
        for wx in range(W // w):
            for i in range(w):
                for j in range(w):
                    y, x = (wy * w + i + shift) % H, (wx * w + j + shift) % W
                    rows[:, wy, wx, i, j] = torch.arange(B) * H * W + y * W + x
    return rows.view(-1, w * w)


def token_regions(H, W, w, shift):
    """The region label (0..8) of every token by its ROLLED coordinate, [nW, w*w]."""
    def reg(v, L):
        return 0 if v < L - w else (1 if v < L - shift else 2)
    lab = torch.zeros(H // w, W // w, w, w, dtype=torch.long)
    for wy in range(H // w):
        for wx in range(W // w):
            for i in range(w):
                for j in range(w):
                    lab[wy, wx, i, j] = reg(wy * w + i, H) * 3 + reg(wx * w + j, W) if shift else 0
    return lab.view(-1, w * w)


class WindowAttention(nn.Module):
    def __init__(self, dim, heads, w):
        super().__init__()
        self.heads, self.w = heads, w
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * w - 1) ** 2, heads))
        self.register_buffer("relative_position_index", relative_position_index(w), persistent=False)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def bias(self):
        N = self.w * self.w
        b = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        return b.permute(2, 0, 1).contiguous()  # [heads, N, N]

    def forward(self, x, mask):  # x [B * nW, N, C]
        Bw, N, C = x.shape
        qkv = self.qkv(x).reshape(Bw, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = (q * (C // self.heads) ** -0.5) @ k.transpose(-1, -2) + self.bias().unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            a = a.view(-1, nW, self.heads, N, N) + mask.to(a.dtype).unsqueeze(1).unsqueeze(0)
            a = a.view(-1, self.heads, N, N)
        a = torch.softmax(a, dim=-1)
        return self.proj((a @ v).transpose(1, 2).reshape(Bw, N, C))


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, grid, heads, w, shift, drop_path):
        super().__init__()
        if grid <= w:  # the window is the grid, no shift
            w, shift = grid, 0
        self.grid, self.w, self.shift, self.drop_path = grid, w, shift, drop_path
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, heads, w)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim)
        m = attn_mask(grid, grid, w, shift)
        self.register_buffer("attn_mask", m, persistent=False)
        self.index = 0  # position among all blocks, set by the model
        self.scales = None

    def _dp(self, t, branch):
        if self.scales is None or not self.training:
            return t
        s = self.scales(self.index, branch, t.shape[0]).to(t.dtype)
        return t * s.view(-1, 1, 1, 1)

    def _attn(self, x):
        B, H, W, C = x.shape
        s = self.shift
        sx = torch.roll(x, shifts=(-s, -s), dims=(1, 2)) if s else x
        win = window_partition(sx, self.w).view(-1, self.w * self.w, C)
        win = self.attn(win, self.attn_mask).view(-1, self.w, self.w, C)
        sx = window_reverse(win, self.w, H, W)
        return torch.roll(sx, shifts=(s, s), dims=(1, 2)) if s else sx

    def forward(self, x):  # [B, H, W, C]
        x = x + self._dp(self._attn(self.norm1(x)), 0)
        return x + self._dp(self.mlp(self.norm2(x)), 1)


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        B, H, W, C = x.shape
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3)
        return self.reduction(self.norm(x))


class Stage(nn.Module):
    def __init__(self, dim, grid, depth, heads, w, downsample, dprs):
        super().__init__()
        self.downsample = PatchMerging(dim // 2) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[Block(dim, grid, heads, w, 0 if j % 2 == 0 else w // 2, dprs[j])
                                      for j in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=4, stride=4)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        return self.norm(self.proj(x).permute(0, 2, 3, 1))  # NHWC


class SwinTransformer(nn.Module):
    def __init__(self, dim, depths, heads, img_size=224, drop_path_rate=0.1):
        super().__init__()
        w = window_for(img_size)
        self.img_size, self.window = img_size, w
        self.num_features = dim * 2 ** (len(depths) - 1)
        self.patch_embed = PatchEmbed(dim)
        dpr = torch.linspace(0, drop_path_rate, sum(depths)).tolist()
        stages, k = [], 0
        for s, depth in enumerate(depths):
            stages.append(Stage(dim * 2 ** s, img_size // 4 // 2 ** s, depth, heads[s], w, s > 0, dpr[k:k + depth]))
            k += depth
        self.layers = nn.Sequential(*stages)
        self.norm = nn.LayerNorm(self.num_features)
        for i, blk in enumerate(self.all_blocks()):
            blk.index = i
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def all_blocks(self):
        return [blk for st in self.layers for blk in st.blocks]

    def set_drop_path_scales(self, fn):
        for blk in self.all_blocks():
            blk.scales = fn

    def forward(self, x):
        if x.shape[-2] != self.img_size or x.shape[-1] != self.img_size:
            raise ValueError(f"input {tuple(x.shape[-2:])} is not {self.img_size}x{self.img_size}")
        x = self.norm(self.layers(self.patch_embed(x)))
        return x.mean(dim=(1, 2))


def create(name, img_size=224, drop_path_rate=0.1, depths=None):
    dim, d, heads, _ = CFGS[name]
    return SwinTransformer(dim, depths or d, heads, img_size, drop_path_rate)


# ---- windowed attention over raster rows: float64 reference and the restatement that rounds where the kernels do
def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def dense_bias(table, w):
    """[(2w-1)^2, heads] -> [heads, N, N] through timm's index."""
    N = w * w
    return table[relative_position_index(w).view(-1)].view(N, N, -1).permute(2, 0, 1)


def _gather(qkv, B, H, W, w, shift, heads):
    C = heads * 32
    x = qkv[:B * H * W].view(B, H, W, 3 * C)
    x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift else x
    x = window_partition(x, w).view(-1, w * w, 3, heads, 32).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]  # [B * nW, heads, N, 32]


def _scatter(t, B, H, W, w, shift):  # [B * nW, heads, N, 32] -> raster [B * H * W, heads * 32]
    Bw, heads, N, _ = t.shape
    x = t.permute(0, 2, 1, 3).reshape(Bw, w, w, heads * 32)
    x = window_reverse(x, w, H, W)
    x = torch.roll(x, shifts=(shift, shift), dims=(1, 2)) if shift else x
    return x.reshape(B * H * W, heads * 32)


def _scores(q, k, table, B, H, W, w, shift, scale):
    N = w * w
    s = q @ k.transpose(-1, -2) * scale + dense_bias(table, w).unsqueeze(0)
    m = attn_mask(H, W, w, shift)
    if m is not None:
        s = (s.view(B, -1, s.shape[1], N, N) + m.double().view(1, -1, 1, N, N)).view(-1, s.shape[1], N, N)
    return s


def winattn_f64(qkv, table, dout, B, H, W, w, shift, heads, scale=32 ** -0.5):
    """float64 attention and autograd on the given (bf16-representable) operands -> out, lse, dqkv, dtable."""
    qkv = qkv[:B * H * W].double().clone().requires_grad_(True)
    table = table.double().clone().requires_grad_(True)
    q, k, v = _gather(qkv, B, H, W, w, shift, heads)
    s = _scores(q, k, table, B, H, W, w, shift, scale)
    out = _scatter(torch.softmax(s, -1) @ v, B, H, W, w, shift)
    out.backward(dout[:B * H * W].double())
    return out.detach(), torch.logsumexp(s, -1).detach(), qkv.grad, table.grad


def winattn_restated(qkv, table, dout, B, H, W, w, shift, heads, scale=32 ** -0.5):
    """The same in float64 arithmetic, rounded to bf16 where the kernels round: in the forward exp(score - rowmax)
    before P v (the kernel divides by the row sum afterwards, on the accumulator), out; in the backward P recomputed
    from lse before P^T dout, dS, dq / dk / dv; D = rowsum(dout . bf16(out)); the bias gradient from the unrounded
    P (dP - D)."""
    qkv, table, dout = qkv[:B * H * W].double(), table.double(), dout[:B * H * W].double()
    q, k, v = _gather(qkv, B, H, W, w, shift, heads)
    do = _gather(dout.repeat(1, 3), B, H, W, w, shift, heads)[0]
    s = _scores(q, k, table, B, H, W, w, shift, scale)
    pu = torch.exp(s - s.max(-1, keepdim=True).values)
    l = pu.sum(-1, keepdim=True)
    p = pu / l
    o = _bf((_bf(pu) @ v) / l)
    t = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    ds = _bf(t * scale)
    dq, dk, dv = _bf(ds @ k), _bf(ds.transpose(-1, -2) @ q), _bf(_bf(p).transpose(-1, -2) @ do)
    dqkv = torch.cat([_scatter(g, B, H, W, w, shift) for g in (dq, dk, dv)], dim=1)
    dtable = torch.zeros_like(table).index_add_(0, relative_position_index(w).view(-1),
                                                t.sum(0).permute(1, 2, 0).reshape(w ** 4, heads))
    return _scatter(o, B, H, W, w, shift), torch.logsumexp(s, -1), dqkv, dtable


# ---- one block as SwinHip's bf16 mode runs it, in float64
def _ln64(x, w, b, eps=1e-5):
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


def block_restated(blk, x, d, *, rows, slab_split=None, s1=None, s2=None, rounded=True):
    """One block's forward from ``x`` and backward from the output gradient ``d`` (both [B, H, W, C]) in float64.
    ``rounded``: round to bf16 where SwinHip (precision="bf16") stores bf16 -- the four GEMM weights, y1, qkv, the
    window attention's roundings (``winattn_restated``), y2, a = GELU(h), gh = GELU'(h), the bf16 casts of the
    (per-sample scaled) gradient stream, dh, do, and each split-K slab of a weight gradient where the module takes
    bf16 slabs; everything the module keeps in f32 stays float64.  ``rounded=False``: plain float64 with the same
    stochastic-depth scales.  ``s1`` / ``s2``: the per-sample scales [B] of the two branches (None: 1).
    ``rows``: the row count of the module's (padded) stream; ``slab_split(n, k)``: the number of bf16 slab slices of
    the weight gradient [n, k] (1: f32 slabs).  -> dict(out, dx, grads by parameter name)."""
    import math

    bf = _bf if rounded else (lambda t: t)
    p = {n: t.detach().double() for n, t in blk.named_parameters()}
    B, H, W, C = x.shape
    heads, w, shift = blk.attn.heads, blk.w, blk.shift
    n = B * H * W
    x, d = x.double().reshape(n, C), d.double().reshape(n, C)
    one = torch.ones(B, dtype=torch.float64)
    r1 = (one if s1 is None else s1.double()).repeat_interleave(H * W).unsqueeze(1)
    r2 = (one if s2 is None else s2.double()).repeat_interleave(H * W).unsqueeze(1)
    wq, wp, w1, w2 = (bf(p[k + ".weight"]) for k in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"))
    table = p["attn.relative_position_bias_table"].float().double()

    def wgrad(dy, a):  # dy^T a over the padded rows, bf16 slabs where the module takes them
        nn_, k = dy.shape[-1], a.shape[-1]
        split = 1 if slab_split is None or not rounded else slab_split(nn_, k)
        if split == 1:
            return dy.T @ a
        dyp, ap = torch.zeros(rows, nn_, dtype=torch.float64), torch.zeros(rows, k, dtype=torch.float64)
        dyp[:n], ap[:n] = dy, a
        per = rows // split
        return sum(_bf(dyp[s * per:(s + 1) * per].T @ ap[s * per:(s + 1) * per]) for s in range(split))

    def attention(qkv, do):
        if rounded:
            return winattn_restated(qkv, table, do, B, H, W, w, shift, heads)
        return winattn_f64(qkv, table, do, B, H, W, w, shift, heads)

    # ---- forward
    y1f, xh1, rs1 = _ln64(x, p["norm1.weight"], p["norm1.bias"])
    y1 = bf(y1f)
    qkv = bf(y1 @ wq.T + p["attn.qkv.bias"])
    o = attention(qkv, torch.zeros(n, C, dtype=torch.float64))[0]
    x1 = x + r1 * (o @ wp.T + p["attn.proj.bias"])
    y2f, xh2, rs2 = _ln64(x1, p["norm2.weight"], p["norm2.bias"])
    y2 = bf(y2f)
    h = y2 @ w1.T + p["mlp.fc1.bias"]
    Phi = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
    a, gh = bf(h * Phi), bf(Phi + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi))
    out = x1 + r2 * (a @ w2.T + p["mlp.fc2.bias"])
    # ---- backward
    g = {}
    dsrc = bf(r2 * d)
    dh = bf((dsrc @ w2) * gh)
    g["mlp.fc2.weight"], g["mlp.fc2.bias"] = wgrad(dsrc, a), dsrc.sum(0)
    g["mlp.fc1.weight"], g["mlp.fc1.bias"] = wgrad(dh, y2), dh.sum(0)
    ddx, g["norm2.weight"], g["norm2.bias"] = _ln64_bwd(dh @ w1, xh2, rs2, p["norm2.weight"])
    d = d + ddx
    dsrc = bf(r1 * d)
    do = bf(dsrc @ wp)
    g["attn.proj.weight"], g["attn.proj.bias"] = wgrad(dsrc, o), dsrc.sum(0)
    _, _, dqkv, g["attn.relative_position_bias_table"] = attention(qkv, do)
    g["attn.qkv.weight"], g["attn.qkv.bias"] = wgrad(dqkv, y1), dqkv.sum(0)
    ddx, g["norm1.weight"], g["norm1.bias"] = _ln64_bwd(dqkv @ wq, xh1, rs1, p["norm1.weight"])
    return dict(out=out.reshape(B, H, W, C), dx=(d + ddx).reshape(B, H, W, C), grads=g)


# ---- the window-attention calls one at a time: float64 references, per-element bounds and a float32 restatement
# (tests/test_swin_calls_gpu.py derives every term of the bounds in its docstring; tests/test_swin_calls_cpu.py checks
# the bounds against the restatement and against faults put into it)
U32 = 2.0 ** -24  # unit roundoff of f32 (round to nearest)
U16 = 2.0 ** -8  # unit roundoff of bf16
TINY = 2.0 ** -126  # smallest normal f32 / bf16: what a flushed denormal loses
EXP2_REL = 2.0 ** -21  # relative error granted to the hardware exp2 (documented at 1 ulp = 2^-23; four times that)
LSE_ABS = 1e-3  # the project's bound on lse (the fast log's accuracy cannot be read from the code)
WAVE_TARGET = 1024
FAULTS = ("dropped_key", "mask_unrolled", "bias_transposed", "shift_sign", "skip_round2", "db_reset", "lse_by_part",
          "no_max", "d_unrounded")


def f32_scale(scale):
    """the scale as the entry points receive it (a C float)"""
    return float(torch.tensor(scale, dtype=torch.float32))


def win_nparts(B, H, W, w, heads):
    """csrc/swin.hip's win_nparts restated: the waves of one head"""
    return max(1, min(max(1, WAVE_TARGET // heads), B * (H // w) * (W // w)))


def walk_depths(total, nparts):
    """how many windows the waves part = 0 .. nparts-1 walk: the set of depths"""
    return {len(range(p, total, nparts)) for p in range(nparts)}


def calls_inputs(geom, variant="uniform"):
    """qkv, dout (bf16-exact float64) and the f32-exact table of tests/test_winattn_gpu.py's recipe: q, k in
    [-1.5, 1.5], v and dout in [-1, 1], table in [-2, 2] (16 for ``table16``), q[..., 0] = 24 and k[..., 0] = +-24 for
    ``shift_up`` / ``shift_down``; independent draws per row, so every window and head has its own data."""
    B, H, W, w, shift, heads = geom
    g = torch.Generator().manual_seed(15485863 + 104729 * B + 7919 * H + 131 * W + 17 * w + 5 * shift + heads)
    C, n = heads * 32, B * H * W
    qkv = torch.rand(n, 3 * C, generator=g, dtype=torch.float64) * 2 - 1
    qkv.view(n, 3, C)[:, :2] *= 1.5
    if variant.startswith("shift"):
        qk = qkv.view(n, 3, heads, 32)
        qk[:, 0, :, 0] = 24.0
        qk[:, 1, :, 0] = 24.0 if variant == "shift_up" else -24.0
    qkv = _bf(qkv)
    dout = _bf(torch.rand(n, C, generator=g, dtype=torch.float64) * 2 - 1)
    amp = 16.0 if variant == "table16" else 2.0
    table = ((torch.rand((2 * w - 1) ** 2, heads, generator=g, dtype=torch.float64) * 2 - 1) * amp).float().double()
    return qkv, dout, table


def _gather1(x, B, H, W, w, shift, heads):  # raster [rows, heads * 32] -> [B * nW, heads, N, 32]
    x = x[:B * H * W].view(B, H, W, heads * 32)
    x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift else x
    return window_partition(x, w).view(-1, w * w, heads, 32).permute(0, 2, 1, 3)


def score_bound(absdot, scaled, *, head_dim, biased=None, masked=None):
    """|error| of a score: a head_dim-term f32 MFMA sum of exact bf16 products (``absdot`` = scale sum_d |q_d||k_d|),
    one rounding of the product with the scale or of the fma with the bias (``biased`` = scale q.k + bias; None: no
    bias term), one of the addition of the mask (``masked``; None: no mask added)."""
    e = head_dim * U32 * absdot + U32 * (scaled if biased is None else biased).abs()
    return e if masked is None else e + U32 * masked.abs()


def _scores_dense(q, k, bias, geom, scale):
    """float64 scores [B * nW, heads, N, N] from the dense bias, and their error bound"""
    B, H, W, w, shift, heads = geom
    N = w * w
    scaled = (q @ k.transpose(-1, -2)) * scale
    absdot = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    s0 = scaled + bias.unsqueeze(0)
    m = attn_mask(H, W, w, shift)
    if m is None:
        return s0, score_bound(absdot, scaled, head_dim=q.shape[-1], biased=s0)
    s = (s0.view(B, -1, heads, N, N) + m.double().view(1, -1, 1, N, N)).view(-1, heads, N, N)
    return s, score_bound(absdot, scaled, head_dim=q.shape[-1], biased=s0, masked=s)


def stored_bf16(ref, err):
    """the bound of a value computed within ``err`` and then stored as bf16"""
    return err + U16 * (ref.abs() + err) + TINY


def softmax_out_bound(p, v, out, ds, arg, nkeys):
    """|error| of out = (sum_k bf16(e_k) v_k) / l before its store, e_k = exp2((s_k - m) log2 e), l = sum_k e_k in f32.
    ``arg`` = s - m.  The max m is common to the row and cancels in e / l."""
    pv = p @ v.abs()
    dmax = (ds + 3 * U32 * arg.abs()).max(-1, keepdim=True).values + EXP2_REL  # relative error of an e_k, row maximum
    return (U16 + 2 * dmax + 2 * nkeys * U32) * pv + 3 * U32 * out.abs()


def winattn_fwd_ref(qkv, bias, geom, scale):
    """float64 of sv_winattn_fwd on its operands -> dict(out, out_bound [B*H*W, C] raster; lse [B * nW, heads, N])"""
    B, H, W, w, shift, heads = geom
    q, k, v = _gather(qkv.double(), B, H, W, w, shift, heads)
    s, ds = _scores_dense(q, k, bias.double(), geom, scale)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = p @ v
    err = softmax_out_bound(p, v, out, ds, s - s.max(-1, keepdim=True).values, w * w)
    return dict(out=_scatter(out, B, H, W, w, shift), out_bound=_scatter(stored_bf16(out, err), B, H, W, w, shift),
                lse=lse)


def winattn_bwd_ref(qkv, out, lse, dout, bias, geom, scale, nparts):
    """float64 of sv_winattn_bwd on its operands (``out`` bf16 and ``lse`` f32 are operands: D = rowsum(dout . out),
    P = exp(score - lse)) -> dict(dqkv, dqkv_bound raster; part, part_bound [nparts, heads, N, N], part p the sum
    of T over the windows p, p + nparts, ...; tsum / tabs [heads, N, N], the sums of T and of |T| over all windows)."""
    B, H, W, w, shift, heads = geom
    N, hd = w * w, 32
    q, k, v = _gather(qkv.double(), B, H, W, w, shift, heads)
    do, o = (_gather1(t.double(), B, H, W, w, shift, heads) for t in (dout, out))
    s, ds = _scores_dense(q, k, bias.double(), geom, scale)
    arg = s - lse.double().unsqueeze(-1)
    p = torch.exp(arg)
    ep = p * (ds + 3 * U32 * arg.abs() + EXP2_REL) + TINY  # score, the argument's subtraction and product, exp2
    del s, ds, arg
    g = do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)  # dP - D
    eg = hd * U32 * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * o.abs()).sum(-1, keepdim=True))
    t = p * g
    et = ep * g.abs() + p * eg + 2 * U32 * t.abs() + TINY  # P's error, dP's and D's sums, the subtraction, the product
    del g, eg
    dS = t * scale
    edS = (scale * et + U32 * dS.abs()) * (1 + U16) + U16 * dS.abs() + TINY  # the product with scale, then bf16
    epb = ep * (1 + U16) + U16 * p  # P as a bf16 MFMA operand
    del ep
    acc = N * U32  # f32 accumulation over the N tokens of the window
    dq, edq = dS @ k, edS @ k.abs() + acc * (dS.abs() @ k.abs())
    dk, edk = dS.transpose(-1, -2) @ q, edS.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs())
    dv, edv = p.transpose(-1, -2) @ do, epb.transpose(-1, -2) @ do.abs() + acc * (p.transpose(-1, -2) @ do.abs())
    del dS, edS, epb, p
    dqkv = torch.cat([_scatter(x, B, H, W, w, shift) for x in (dq, dk, dv)], dim=1)
    bound = torch.cat([_scatter(stored_bf16(x, e), B, H, W, w, shift) for x, e in ((dq, edq), (dk, edk), (dv, edv))], dim=1)
    total = t.shape[0]
    part = torch.zeros(nparts, heads, N, N, dtype=torch.float64)
    pe, pa = torch.zeros_like(part), torch.zeros_like(part)
    depth = torch.zeros(nparts, 1, 1, 1, dtype=torch.float64)
    for first in range(0, total, nparts):  # round r of the walk: windows r * nparts + p
        m = min(nparts, total - first)
        part[:m] += t[first:first + m]
        pe[:m] += et[first:first + m]
        pa[:m] += t[first:first + m].abs()
        depth[:m] += 1
    return dict(dqkv=dqkv, dqkv_bound=bound, part=part, part_bound=pe + depth * U32 * pa,  # one f32 addition per window
                tsum=t.sum(0), tabs=t.abs().sum(0))


def _to_table(x, w):  # [heads, N, N] -> [(2w-1)^2, heads]: every table entry's sum over its (i, j) pairs
    heads = x.shape[0]
    return torch.zeros((2 * w - 1) ** 2, heads, dtype=x.dtype).index_add_(
        0, relative_position_index(w).view(-1), x.permute(1, 2, 0).reshape(w ** 4, heads))


def bias_grad_ref(part, prior, w, accumulate):
    """float64 of sv_swin_bias_grad on its operands -> (dtable, bound): nparts additions per lane, up to w*w in lane
    order, then the prior"""
    nparts = part.shape[0]
    t = _to_table(part.double().sum(0), w)
    ref = t + prior.double() if accumulate else t
    bound = (nparts + w * w) * U32 * _to_table(part.double().abs().sum(0), w)
    return ref, bound + (U32 * ref.abs() if accumulate else 0.0) + TINY


def dtable_chain_ref(b, prior, w, nparts):
    """dtable = prior + sum over all windows and pairs of T, from winattn_bwd_ref's dict: the bounds of the partials
    (the terms' own and one addition per window of the walk), then nparts additions per lane, w*w in lane order and
    the prior"""
    ref = _to_table(b["tsum"], w) + prior.double()
    return ref, _to_table(b["part_bound"].sum(0) + (nparts + w * w) * U32 * b["tabs"], w) + U32 * ref.abs() + TINY


def ratio(got, ref, bound):
    """|got - ref| / bound per element, inf where got is not finite"""
    r = (got.double() - ref).abs() / bound
    return torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))


# the float32 restatement: the kernels' index formula, the kernels' rounding points, torch's summation orders
def walk_index(B, H, W, w, shift, *, sign=1, unrolled_labels=False):
    """(rows [B * nW, N], labels [B * nW, N]) by the kernels' formula; ``sign`` = -1 and ``unrolled_labels`` are
    the faults 'shift sign flipped' and 'mask regions from the unrolled coordinate'"""
    nwy, nwx, N = H // w, W // w, w * w
    yr = (torch.arange(nwy).view(-1, 1, 1, 1) * w + torch.arange(w).view(1, 1, -1, 1)).expand(nwy, nwx, w, w)
    xr = (torch.arange(nwx).view(1, -1, 1, 1) * w + torch.arange(w).view(1, 1, 1, -1)).expand(nwy, nwx, w, w)
    y, x = (yr + sign * shift) % H, (xr + sign * shift) % W
    rows = ((y * W + x).reshape(1, -1, N) + (torch.arange(B) * H * W).view(B, 1, 1)).reshape(-1, N)

    def reg(v, L):
        return (v >= L - w).long() + (v >= L - shift).long()

    ly, lx = (y, x) if unrolled_labels else (yr, xr)
    lab = (reg(ly, H) * 3 + reg(lx, W)).reshape(1, -1, N).expand(B, -1, -1).reshape(-1, N)
    return rows, (lab if shift else torch.zeros_like(lab))


def _restated_scores(qkv, bias, geom, scale, fault):
    B, H, W, w, shift, heads = geom
    N = w * w
    rows, lab = walk_index(B, H, W, w, shift, sign=-1 if fault == "shift_sign" else 1,
                           unrolled_labels=fault == "mask_unrolled")
    x = qkv.float()[rows].view(-1, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    b = bias.float()
    b = b.transpose(-1, -2) if fault == "bias_transposed" else b
    s = (q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32) + b.unsqueeze(0)
    masked = (lab[:, :, None] != lab[:, None, :]).unsqueeze(1)
    return rows, q, k, v, torch.where(masked, s + MASKED, s)


def _done(total, nparts, fault):
    return min(total, nparts) if fault == "skip_round2" else total


def winattn_fwd_restated32(qkv, bias, geom, scale, nparts, fault=None):
    """-> (out [B*H*W, C] of bf16 values, lse [B * nW, heads, N] of f32 values), NaN where nothing was written"""
    B, H, W, w, shift, heads = geom
    N, C = w * w, heads * 32
    rows, q, k, v, s = _restated_scores(qkv, bias, geom, scale, fault)
    m = torch.zeros_like(s[..., :1]) if fault == "no_max" else s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    if fault == "dropped_key":
        e[..., N - 1] = 0
    l = e.sum(-1, keepdim=True)
    o = ((e.bfloat16().float() @ v) * (1.0 / l)).bfloat16().float()
    lse = (m + torch.log(l)).squeeze(-1)
    total = rows.shape[0]
    done = _done(total, nparts, fault)
    out = torch.full((B * H * W, C), float("nan"))
    out[rows[:done].reshape(-1)] = o[:done].permute(0, 2, 1, 3).reshape(-1, C)
    lse_out = torch.full_like(lse, float("nan"))
    if fault == "lse_by_part":
        for first in range(0, total, nparts):
            mm = min(nparts, total - first)
            lse_out[:mm] = lse[first:first + mm]
    else:
        lse_out[:done] = lse[:done]
    return out.double(), lse_out.double()


def winattn_bwd_restated32(qkv, out, lse, dout, bias, geom, scale, nparts, fault=None, out_unrounded=None):
    """-> (dqkv [B*H*W, 3C] of bf16 values, part [nparts, heads, N, N] of f32 values)"""
    B, H, W, w, shift, heads = geom
    N, C = w * w, heads * 32
    rows, q, k, v, s = _restated_scores(qkv, bias, geom, scale, fault)
    total = rows.shape[0]

    def win(x):
        return x.float()[rows].view(-1, N, heads, 32).permute(0, 2, 1, 3)

    do, o = win(dout), win(out_unrounded if fault == "d_unrounded" else out)
    ls = lse.float()
    ls = ls[torch.arange(total) % nparts] if fault == "lse_by_part" else ls
    p = torch.exp(s - ls.unsqueeze(-1))
    if fault == "dropped_key":
        p[..., N - 1] = 0
    t = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dS = (t * torch.tensor(scale, dtype=torch.float32)).bfloat16().float()
    g = torch.stack([(dS @ k), (dS.transpose(-1, -2) @ q), (p.bfloat16().float().transpose(-1, -2) @ do)])
    g = g.bfloat16().float()  # [3, B * nW, heads, N, 32]
    done = _done(total, nparts, fault)
    dqkv = torch.full((B * H * W, 3 * C), float("nan"))
    dqkv[rows[:done].reshape(-1)] = g[:, :done].permute(1, 3, 0, 2, 4).reshape(-1, 3 * C)
    part = torch.zeros(nparts, heads, N, N)
    for first in range(0, done, nparts):
        mm = min(nparts, total - first)
        if fault == "db_reset":
            part[:mm] = t[first:first + mm]
        else:
            part[:mm] += t[first:first + mm]
    return dqkv.double(), part.double()


def bias_grad_restated32(part, prior, w, accumulate):
    t = _to_table(part.float().sum(0), w)
    return (t + prior.float() if accumulate else t).double()


@functools.lru_cache(maxsize=None)
def calls_case(geom, variant="uniform", scale=32 ** -0.5):
    """Operands, float64 references and bounds of the three calls, the backward's on CPU-made operands (the float64
    forward rounded to bf16 / f32) and a non-zero prior of dtable; computed once per case, shared by the tests of
    both files, never modified."""
    B, H, W, w, shift, heads = geom
    scale = f32_scale(scale)
    qkv, dout, table = calls_inputs(geom, variant)
    bias = dense_bias(table, w).contiguous()
    nparts = win_nparts(B, H, W, w, heads)
    f = winattn_fwd_ref(qkv, bias, geom, scale)
    out, lse = _bf(f["out"]), f["lse"].float().double()
    g = torch.Generator().manual_seed(heads)
    prior = (torch.rand(table.shape, generator=g) * 2 - 1).double()
    b = winattn_bwd_ref(qkv, out, lse, dout, bias, geom, scale, nparts)
    return dict(qkv=qkv, dout=dout, table=table, bias=bias, nparts=nparts, scale=scale, fwd=f, out=out, lse=lse,
                prior=prior, bwd=b, dtable=dtable_chain_ref(b, prior, w, nparts))
