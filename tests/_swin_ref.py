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
bf16 exactly where the kernels do (the rule of tests/test_attn_gpu.py)."""
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
