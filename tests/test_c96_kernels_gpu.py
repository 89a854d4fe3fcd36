"""Per-kernel parity of the C = 96 forms (ConvNeXt-tiny / small's stage-1 width) on the MI355X: each case is its
sibling in test_kernels_gpu.py at the new width, with that test's bounds -- relative L2 1e-5 against torch fp32 (f32
operands), the bf16 bounds of the bf16-I/O siblings.  The depthwise cases add the channel counts at which the masked
half group sits alone (C = 32) or behind two full groups (C = 160), and a guard test around the tensors' ends."""

import pytest
import torch
import torch.nn.functional as F

from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bf(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows", [1, 15, 333, 9001])
def test_layernorm_fwd_bwd_c96(dev, rows):
    """4 lanes x 24 channels, 16 rows per wave: fewer rows than a wave holds (1, 15), rows that fill no whole wave
    (333, 9001), several row groups per wave in the backward (9001)."""
    C = 96
    g = torch.Generator().manual_seed(C + rows)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    y, mean, rstd = K.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), out_dtype=torch.float32)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), wr, br, 1e-6)
    yr.backward(dy)
    assert rel(y, yr) < 1e-5
    assert rel(mean, x.mean(1)) < 1e-5
    dw = torch.zeros(C, device=dev)
    db = torch.zeros(C, device=dev)
    dx = K.layernorm_bwd(dy.to(dev), x.to(dev), mean, rstd, w.to(dev), dw=dw, db=db)
    assert rel(dx, xr.grad) < 1e-5
    assert rel(dw, wr.grad) < 1e-5
    assert rel(db, br.grad) < 1e-5


@pytest.mark.parametrize("rows", [15, 333])
@pytest.mark.parametrize("dy_f32", [False, True])
def test_layernorm_bwd_bf16_io_c96(dev, rows, dy_f32):
    C = 96
    g = torch.Generator().manual_seed(C + rows + 1)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(torch.bfloat16)
    w = torch.rand(C, generator=g) + 0.5
    dy = torch.randn(rows, C, generator=g)
    if not dy_f32:  # (f32, bf16, bf16) is the stem's combination: f32 gradient stream, bf16 saved input
        dy = dy.to(torch.bfloat16)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), wr, None, 1e-6)
    yr.backward(dy.double())
    xd = x.to(dev)
    yb, mean, rstd = K.layernorm_fwd(xd, w.to(dev), torch.zeros(C, device=dev), out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16
    assert rel(yb, yr) < 8e-3  # output rounded to bf16
    y32, mean2, rstd2 = K.layernorm_fwd(xd, w.to(dev), torch.zeros(C, device=dev), out_dtype=torch.float32)
    assert rel(y32, yr) < 1e-5 and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    dw = torch.zeros(C, device=dev)
    db = torch.zeros(C, device=dev)
    dx = K.layernorm_bwd(dy.to(dev), xd, mean, rstd, w.to(dev), dw=dw, db=db, out_dtype=torch.bfloat16)
    assert dx.dtype == torch.bfloat16
    assert rel(dx, xr.grad) < 8e-3  # output rounded to bf16
    assert rel(dw, wr.grad) < 1e-5
    assert rel(db, dy.double().sum(0)) < 1e-5


# ------------------------------------------------------------------------------ depthwise conv
DW_SHAPES = [(2, 16, 16, 96), (1, 13, 11, 96), (2, 2, 2, 96), (1, 37, 45, 96), (3, 4, 4, 32), (1, 9, 5, 160)]


@pytest.mark.parametrize("shape", DW_SHAPES)
def test_dwconv7_fwd_bwd_c96(dev, shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B * H * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, 1, 7, 7, generator=g) * 0.1
    bias = torch.randn(C, generator=g) * 0.1
    lnw = torch.rand(C, generator=g) + 0.5
    lnb = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, H, W, C, generator=g)
    z, y, mean, rstd = K.dwconv7_ln_fwd(x.to(dev), w.to(dev), bias.to(dev), lnw.to(dev), lnb.to(dev),
                                        act_dtype=torch.float32)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    zr = F.conv2d(xr, wr, br, padding=3, groups=C)
    zr_nhwc = zr.permute(0, 2, 3, 1)
    yr = F.layer_norm(zr_nhwc, (C,), lnw, lnb, 1e-6)
    assert rel(z, zr_nhwc) < 1e-5
    assert rel(y.view(B, H, W, C), yr) < 1e-5
    zr_nhwc.backward(dy)
    ref_dx = xr.grad.permute(0, 2, 3, 1)
    # accumulate on (from zero and from a base) and off, each with the bf16 copy
    for accumulate in (True, False):
        base = torch.randn(B, H, W, C, generator=g)
        dx = base.clone().to(dev)
        dxb = torch.empty(B, H, W, C, device=dev, dtype=torch.bfloat16)
        K.dwconv7_bwd_data(dy.to(dev), w.to(dev), dx, accumulate=accumulate, dx_bf16=dxb)
        assert torch.equal(dxb.cpu(), dx.cpu().to(torch.bfloat16))
        assert rel(dx.cpu() - (base if accumulate else 0), ref_dx) < 1e-5
    dw = torch.zeros(C, 49, device=dev)
    db = torch.zeros(C, device=dev)
    K.dwconv7_bwd_weight(dy.to(dev), x.to(dev), dw=dw, db=db)
    assert rel(dw, wr.grad.view(C, 49)) < 1e-5
    assert rel(db, br.grad) < 1e-5
    dw2 = torch.zeros(C, 49, device=dev)
    db2 = torch.zeros(C, device=dev)
    K.dwconv7_bwd_weight(dy.to(dev), x.to(dev), dw=dw2, db=db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)  # fixed-order partial folds: run to run the same bits


@pytest.mark.parametrize("shape", DW_SHAPES)
def test_dwconv7_bf16_io_c96(dev, shape, monkeypatch):
    """The VALU kernels over bf16 tensors: bf16 x -> bf16 z, and a bf16 dz through backward-data / -weight."""
    monkeypatch.setattr(K, "DW_MFMA", False)
    monkeypatch.setattr(K, "DW_MFMA_WGRAD", False)
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B * H * W + C + 7)
    x = torch.randn(B, H, W, C, generator=g)
    xb = x.to(torch.bfloat16)
    w = torch.randn(C, 1, 7, 7, generator=g) * 0.1
    bias = torch.randn(C, generator=g) * 0.1
    dz = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    z, _, _, _ = K.dwconv7_ln_fwd(xb.to(dev), w.to(dev), bias.to(dev), torch.ones(C, device=dev),
                                  torch.zeros(C, device=dev), act_dtype=torch.bfloat16)
    zq = F.conv2d(xb.permute(0, 3, 1, 2).double(), w.double(), bias.double(), padding=3, groups=C)
    assert z.dtype == torch.bfloat16
    assert rel(z.view(B, H, W, C), zq.permute(0, 2, 3, 1)) < 8e-3  # output rounded to bf16
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    zr = F.conv2d(xr, wr, None, padding=3, groups=C)
    zr.permute(0, 2, 3, 1).backward(dz.double())
    base = torch.randn(B, H, W, C, generator=g)
    dx = base.clone().to(dev)
    K.dwconv7_bwd_data(dz.to(dev), w.to(dev), dx, accumulate=True)
    assert rel(dx - base.to(dev), xr.grad.permute(0, 2, 3, 1)) < 1e-5
    dw = torch.zeros(C, 49, device=dev)
    db = torch.zeros(C, device=dev)
    K.dwconv7_bwd_weight(dz.to(dev), x.to(dev), dw=dw, db=db)
    assert rel(dw, wr.grad.view(C, 49)) < 1e-5
    assert rel(db, dz.double().sum((0, 1, 2))) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 5, 6, 96), (1, 3, 3, 32), (1, 4, 5, 160)])
def test_dwconv7_half_group_stays_inside_its_tensors(dev, shape, dtype, monkeypatch):
    """x / dz and every output are slices of ONE allocation, each followed at once by a NaN block: a half-group
    lane that read past channel C would carry NaN into an output, one that wrote past it would break the poison."""
    monkeypatch.setattr(K, "DW_MFMA", False)
    monkeypatch.setattr(K, "DW_MFMA_WGRAD", False)
    B, H, W, C = shape
    n, pad = B * H * W * C, 256
    g = torch.Generator().manual_seed(n)

    def guarded(count, dt, fill=None):
        """-> (arena, [views]) with a NaN block after every view; sizes keep every view 16-byte aligned."""
        arena = torch.full((count * (n + pad),), float("nan"), device=dev, dtype=dt)
        views = []
        for k in range(count):
            v = arena[k * (n + pad):k * (n + pad) + n].view(B, H, W, C)
            v.copy_(torch.randn(B, H, W, C, generator=g).to(dt) if fill is None else torch.full((B, H, W, C), fill).to(dt))
            views.append(v)
        return arena, views

    def poison_intact(arena):
        a = arena.view(-1, n + pad)[:, n:]
        return bool(torch.isnan(a.float()).all())

    w = (torch.randn(C, 1, 7, 7, generator=g) * 0.1).to(dev)
    bias = (torch.randn(C, generator=g) * 0.1).to(dev)
    lnw, lnb = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    in_arena, (x, dz) = guarded(2, dtype)
    z, y, mean, rstd = K.dwconv7_ln_fwd(x, w, bias, lnw, lnb, act_dtype=dtype)
    xr = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.cpu(), bias.cpu(), padding=3, groups=C).permute(0, 2, 3, 1)
    assert torch.isfinite(z.float()).all() and torch.isfinite(y.float()).all()
    assert rel(z, xr) < (1e-5 if dtype == torch.float32 else 8e-3)
    f_arena, (dx,) = guarded(1, torch.float32, fill=0.5)
    b_arena, (dxb,) = guarded(1, torch.bfloat16, fill=0.0)
    K.dwconv7_bwd_data(dz, w, dx, accumulate=True, dx_bf16=dxb)
    assert torch.isfinite(dx).all() and torch.isfinite(dxb.float()).all()
    assert poison_intact(f_arena) and poison_intact(b_arena) and poison_intact(in_arena)
    dw = torch.zeros(C, 49, device=dev)
    db = torch.zeros(C, device=dev)
    K.dwconv7_bwd_weight(dz, x, dw=dw, db=db)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert rel(db, dz.double().sum((0, 1, 2))) < 1e-5
    assert poison_intact(in_arena)


# ------------------------------------------------------------------------ stem / downsample
@pytest.mark.parametrize("C,B,H,W", [(96, 2, 8, 6), (96, 2, 128, 128), (96, 1, 6, 2)])
def test_downsample_c96(dev, C, B, H, W):
    """Two patches per wave (one per 32-lane half): a small shape, more patches than the launch has waves, and an
    odd patch count (3: the last wave's second half has no patch)."""
    g = torch.Generator().manual_seed(C + 1)
    x = torch.randn(B, H, W, C, generator=g)
    lnw = torch.rand(C, generator=g) + 0.5
    lnb = torch.randn(C, generator=g) * 0.1
    wc = torch.randn(2 * C, C, 2, 2, generator=g) * 0.05
    bc = torch.randn(2 * C, generator=g) * 0.1
    patches, mean, rstd = K.downsample_fwd(x.to(dev), lnw.to(dev), lnb.to(dev), act_dtype=torch.float32)
    out = torch.empty(B * (H // 2) * (W // 2), 2 * C, device=dev)
    K.linear_fwd(patches, wc.reshape(2 * C, 4 * C).to(dev), out=out, bias=bc.to(dev), compute_bf16=False)
    xr = x.clone().requires_grad_(True)
    lwr, lbr = lnw.clone().requires_grad_(True), lnb.clone().requires_grad_(True)
    n = F.layer_norm(xr, (C,), lwr, lbr, 1e-6).permute(0, 3, 1, 2)
    o = F.conv2d(n, wc, bc, stride=2).permute(0, 2, 3, 1)
    assert rel(out.view(o.shape), o) < 1e-5
    dpatch = torch.randn(patches.shape, generator=g)
    Ho, Wo = H // 2, W // 2
    pr = n.reshape(B, C, Ho, 2, Wo, 2).permute(0, 2, 4, 1, 3, 5).reshape(B * Ho * Wo, 4 * C)
    assert rel(patches, pr) < 1e-5
    pb, _, _ = K.downsample_fwd(x.to(dev), lnw.to(dev), lnb.to(dev), act_dtype=torch.bfloat16)
    assert torch.equal(pb, patches.to(torch.bfloat16))  # the bf16 patches are the f32 ones rounded
    pr.backward(dpatch)
    dlnw = torch.zeros(C, device=dev)
    dlnb = torch.zeros(C, device=dev)
    dx, dxb = K.downsample_bwd(dpatch.to(dev), x.to(dev), mean, rstd, lnw.to(dev), dlnw=dlnw, dlnb=dlnb,
                               with_bf16=True)
    assert torch.equal(dxb.cpu(), dx.cpu().to(torch.bfloat16))
    assert rel(dx, xr.grad) < 1e-5
    assert rel(dlnw, lwr.grad) < 1e-5
    assert rel(dlnb, lbr.grad) < 1e-5


@pytest.mark.parametrize("B,H,W", [(2, 32, 24), (1, 12, 4)])
def test_stem_c96(dev, B, H, W):
    """Two pixels per wave; 1 x 12 x 4 has 3 pixels (the second half of the last wave has none)."""
    C = 96
    g = torch.Generator().manual_seed(C + H)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(C, 3, 4, 4, generator=g) * 0.2
    b = torch.randn(C, generator=g) * 0.1
    lnw = torch.rand(C, generator=g) + 0.5
    lnb = torch.randn(C, generator=g) * 0.1
    y, mean, rstd = K.stem_fwd(img.to(dev), w.to(dev), b.to(dev), lnw.to(dev), lnb.to(dev))
    wr, br, lwr, lbr = (t.clone().requires_grad_(True) for t in (w, b, lnw, lnb))
    zr = F.conv2d(img, wr, br, stride=4).permute(0, 2, 3, 1)
    yr = F.layer_norm(zr, (C,), lwr, lbr, 1e-6)
    assert rel(y, yr) < 1e-5
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy)
    grads = [torch.zeros_like(t, device=dev) for t in (w, b, lnw, lnb)]
    K.stem_bwd(img.to(dev), w.to(dev), b.to(dev), lnw.to(dev), mean, rstd, dy.to(dev),
               dw=grads[0], db=grads[1], dlnw=grads[2], dlnb=grads[3])
    for got, ref in zip(grads, (wr.grad, br.grad, lwr.grad, lbr.grad)):
        assert rel(got, ref) < 1e-5


# ---------------------------------------------------------------------------------------- GEMMs
@pytest.mark.parametrize("M", [512, 1000])
@pytest.mark.parametrize("compute_bf16", [False, True])
def test_mlp_gemms_c96(dev, M, compute_bf16):
    """Stage 1 of ConvNeXt-tiny: fc1 (N = 384, K = 96) with the dual GELU epilogue, fc2 (N = 96, K = 384) with bias,
    layer scale and residual, and the two data gradients (x stored GELU' / plain store); test_gemm_epilogues' bounds."""
    Cc = 96
    g = torch.Generator().manual_seed(M)
    y = torch.randn(M, Cc, generator=g)
    w1 = torch.randn(4 * Cc, Cc, generator=g) * 0.1
    b1 = torch.randn(4 * Cc, generator=g) * 0.1
    w2 = torch.randn(Cc, 4 * Cc, generator=g) * 0.05
    b2 = torch.randn(Cc, generator=g) * 0.1
    gam = torch.rand(Cc, generator=g) * 0.25 + 0.05
    x = torch.randn(M, Cc, generator=g)
    act = torch.bfloat16 if compute_bf16 else torch.float32
    q = bf if compute_bf16 else (lambda t: t)
    tol = 1e-2 if compute_bf16 else 1e-5
    gh = torch.empty(M, 4 * Cc, device=dev, dtype=act)
    a = torch.empty_like(gh)
    K.linear_fwd(y.to(act).to(dev), w1.to(act).to(dev), out=gh, out2=a, bias=b1.to(dev),
                 epilogue=nv.SV_EPI_BIAS_GELU_DUAL, compute_bf16=compute_bf16)
    h_ref = q(y) @ q(w1).t() + b1
    hr = h_ref.clone().requires_grad_(True)
    F.gelu(hr).sum().backward()
    assert rel(a, F.gelu(h_ref)) < tol
    assert rel(gh, hr.grad) < tol
    out = torch.empty(M, Cc, device=dev)
    K.linear_fwd(a, w2.to(act).to(dev), out=out, bias=b2.to(dev), gamma=gam.to(dev), residual=x.to(dev),
                 epilogue=nv.SV_EPI_BIAS_GAMMA_RES, compute_bf16=compute_bf16)
    a_used = a.float().cpu()
    assert rel(out, x + gam * (a_used @ q(w2).t() + b2)) < tol
    # fc2 data gradient x GELU' (SV_EPI_MUL_AUX), then the fc1 data gradient (plain store)
    d = torch.randn(M, Cc, generator=g)
    dh = torch.empty(M, 4 * Cc, device=dev, dtype=act)
    K.linear_dgrad(d.to(dev), w2.to(act).to(dev), out=dh, epilogue=nv.SV_EPI_MUL_AUX, a_scale_k=gam.to(dev),
                   aux=gh, compute_bf16=compute_bf16)
    assert rel(dh, (q(d * gam) @ q(w2)) * gh.float().cpu()) < tol
    dyo = torch.empty(M, Cc, device=dev, dtype=act)
    K.linear_dgrad(dh, w1.to(act).to(dev), out=dyo, compute_bf16=compute_bf16)
    assert rel(dyo, dh.float().cpu() @ q(w1)) < tol


@pytest.mark.parametrize("M", [512, 8192])
@pytest.mark.parametrize("N,Kd", [(384, 96), (96, 384)])
@pytest.mark.parametrize("compute_bf16", [False, True])
@pytest.mark.parametrize("slabs", ["f32", "bf16"])
def test_wgrad_split_and_bias_c96(dev, M, N, Kd, compute_bf16, slabs, monkeypatch):
    monkeypatch.setattr(K, "_WGRAD_BF16_SLABS", slabs == "bf16")
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, N, generator=g)
    x = torch.randn(M, Kd, generator=g)
    out = torch.ones(N, Kd, device=dev)
    bias = torch.ones(N, device=dev)
    dt = torch.bfloat16 if compute_bf16 else torch.float32
    q = bf if compute_bf16 else (lambda t: t.double())
    K.linear_wgrad(dy.to(dt).to(dev), x.to(dt).to(dev), out=out, accumulate=True, bias_out=bias,
                   compute_bf16=compute_bf16)
    tol = (4e-3 if slabs == "bf16" else 2e-3) if compute_bf16 else 1e-5
    assert rel(out, q(dy).t() @ q(x) + 1) < tol
    assert rel(bias, q(dy).sum(0) + 1) < (2e-3 if compute_bf16 else 1e-5)


@pytest.mark.parametrize("M,compute_bf16", [(4096, True), (2048, False)])
@pytest.mark.parametrize("slabs", ["f32", "bf16"])
def test_layerscale_wgrad_fused_c96(dev, M, compute_bf16, slabs, monkeypatch):
    monkeypatch.setattr(K, "_WGRAD_BF16_SLABS", slabs == "bf16")
    C = 96
    g = torch.Generator().manual_seed(M + C)
    d = torch.randn(M, C, generator=g)
    a = torch.randn(M, 4 * C, generator=g)
    w2 = torch.randn(C, 4 * C, generator=g) * 0.05
    gam = torch.rand(C, generator=g) + 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    base = [torch.randn(C, 4 * C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)]
    dt_ = torch.bfloat16 if compute_bf16 else torch.float32
    dq, aq = d.to(dt_), a.to(dt_)
    G = dq.double().t() @ aq.double()
    cs = dq.double().sum(0)
    ref_w = base[0].double() + gam.double()[:, None] * G
    ref_g = base[1].double() + (w2.double() * G).sum(1) + b2.double() * cs
    ref_b = base[2].double() + gam.double() * cs
    dw2, dgam, db2 = (t.clone().to(dev) for t in base)
    K.layerscale_wgrad(dq.to(dev), aq.to(dev), w2.to(dev), gam.to(dev), b2.to(dev), dw2=dw2, dgamma=dgam, db2=db2,
                       compute_bf16=compute_bf16)
    tol = (4e-3 if slabs == "bf16" else 1e-4) if compute_bf16 else 1e-5
    assert rel(dw2, ref_w) < tol
    assert rel(dgam, ref_g) < tol
    assert rel(db2, ref_b) < (1e-4 if compute_bf16 else 1e-5)
