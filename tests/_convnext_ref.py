"""Float64 CPU references, operands, bounds and the host-side launch geometry for tests/test_convnext_calls_gpu.py (the
ConvNeXt path's own kernels: csrc/dwconv.hip, csrc/dwmfma.hip, csrc/norm.hip and the partial folds of csrc/optim.hip).
Test infrastructure only: no kernel is called from here.

Operands are drawn on the CPU in float64 and rounded to the dtype the call takes, so the float64 reference and the kernel
see the same numbers.  Every bound follows DESIGN.md's "Bound per element, derived": an f32 sum differs from float64 by
at most n 2^-24 S, S the same operation over absolute values and n the longest chain of dependent f32 roundings a term
passes through in the kernel's documented order (``*_depth`` below, restated from the sources); elementwise forms carry
one 2^-24 per operation.  Nothing here is fitted to a kernel's output.  The only empirical term is ``rsqrt_rel()``: 4 x
the largest relative error of torch's float32 CPU rsqrt against float64 (rsqrtf is not correctly rounded).

LayerNorm after a producer in the same call (depthwise + LayerNorm, pool + LayerNorm, stem conv + LayerNorm): the
LayerNorm reads what the producer stored, which differs from the float64 value by at most e (the producer's bound; for
a bf16 store, one bf16 step where the float64 value lies within the producer's bound of a rounding boundary and 0
elsewhere).  The first-order effect of e on mean, rstd and y is added to the LayerNorm's own bound with every term taken
in absolute value (``ln_fwd_ref(..., e=)``)."""
import functools
import math

import torch
import torch.nn.functional as F

from _conv_ref import BF, F32, F64, U8, U23, U24, cdiv, store_bound  # noqa: F401  (re-exported for the test file)

EPS = 1e-6
DTN = {"bf16": BF, "f32": F32}


# ----------------------------------------------------------------------------------------- host geometry, restated
# csrc/dwconv.hip
DW_TH, DW_TW, DW_WGS = 16, 4, 1024


def dw_geo(B, H, W, C):
    """-> (tilesW, tilesH, ntiles) of the VALU strips (16 rows x 4 columns)"""
    tw, th = cdiv(W, DW_TW), cdiv(H, DW_TH)
    return tw, th, B * tw * th


def dw_ncg(C):
    return cdiv(C, 64)


def dw_blocks(B, H, W, C):
    return cdiv(dw_geo(B, H, W, C)[2] * dw_ncg(C), 4)


def dw_wgrad_nparts(B, H, W, C, wgs=DW_WGS):
    """sv_dwconv7_bwd_weight_nparts (``wgs``: SV_DW_WGRAD_WGS, floor 64)"""
    return min(cdiv(dw_geo(B, H, W, C)[2], 4), max(1, max(wgs, 64) // dw_ncg(C)))


def dw_wgrad_tiles_per_wave(B, H, W, C, wgs=DW_WGS):
    return cdiv(dw_geo(B, H, W, C)[2], 4 * dw_wgrad_nparts(B, H, W, C, wgs))


def dw_arm(B, H, W, C):
    tw, th, nt = dw_geo(B, H, W, C)
    return f"strips{tw}x{th}x{B} groups{dw_ncg(C)}{' half' if C % 64 else ''}"


def dw_ln_fusable(C, x_dt, act_dt):
    return C in (128, 256, 512) and x_dt == F32


# csrc/dwmfma.hip
def dwm_geo(B, H, W, C):
    """-> (tile width, ntiles) of the matrix-core tiles (16 rows x 16 or 32 columns)"""
    tw = 32 if W > 16 else 16
    return tw, B * cdiv(W, tw) * cdiv(H, 16)


def dwm_cg(mode, C):
    """cg_choice: mode 0 forward, 1 / 2 backward-data"""
    return 32 if mode != 0 and C <= 256 else 16


def dwm_wgrad_nparts(B, H, W, C):
    return max(1, min(512 // max(C // 16, 1), dwm_geo(B, H, W, C)[1]))


def dwm_arm(mode, B, H, W, C):
    tw, nt = dwm_geo(B, H, W, C)
    return f"mfma tile16x{tw} tiles{nt} CG{dwm_cg(mode, C)}"


DWM_K_FWD = 7 * 32  # 7 v_mfma_f32_16x16x32_bf16 per output (one per kernel row), K = 32 each, the zero taps included


def dwm_wgrad_k(W):
    """K extent of one tile in the weight gradient: NCH = TH * (IC / 8) / 4 chunks of 32, IC = (TW + 6 + 7) / 8 * 8"""
    tw = 32 if W > 16 else 16
    ic = (tw + 13) // 8 * 8
    return 16 * ic // 8 // 4 * 32


# csrc/norm.hip
def ln_vec_kind(C):
    """-> (LPR, NV) of the vectorised LayerNorm or None (the per-lane-channel kernels)"""
    if C % 8:
        return None
    u = C // 8
    if u in (16, 32, 64):
        return u, 1
    if u in (4, 12, 20):
        return 4, u // 4
    if u == 128:
        return 64, 2
    if u == 256:
        return 64, 4
    if u % 3 == 0 and u // 3 in (8, 16, 32, 64):
        return u // 3, 3
    return None


def ln_grid(rows):
    return max(1, min(cdiv(rows, 4), 1024))


def ln_vec_bwd_grid(rows, C):
    rpw = 64 // ln_vec_kind(C)[0]
    return max(1, min(cdiv(cdiv(rows, rpw), 32), 2048))


def ln_bwd_nparts(rows, C):
    return ln_vec_bwd_grid(rows, C) if ln_vec_kind(C) else ln_grid(rows)


def ln_arm(rows, C):
    k = ln_vec_kind(C)
    if k is None:
        return f"scalar CPL{C // 64} grid{ln_grid(rows)}"
    rpw = 64 // k[0]
    return f"vec LPR{k[0]} NV{k[1]} fwd{cdiv(cdiv(rows, rpw), 4)} bwd{ln_vec_bwd_grid(rows, C)}"


def ln_row_depth(C):
    """additions a channel passes through in a row's statistics: the lane's serial sum, then the butterfly"""
    k = ln_vec_kind(C)
    return 8 * k[1] + int(math.log2(k[0])) if k else C // 64 + 6


def stem_grid(B, H, W, C):
    return max(1, min(cdiv(B * (H // 4) * (W // 4), 4 * (2 if C % 64 else 1)), 2048))


def stem_bwd_nparts(B, H, W, C):
    return min(stem_grid(B, H, W, C), 256)


def ds_grid(B, H, W, C):
    return max(1, min(cdiv(B * (H // 2) * (W // 2), 4 * (2 if C % 64 else 1)), 1024))


def g32_row_depth(C):
    return C // 32 + 5 if C % 64 else C // 64 + 6


# csrc/optim.hip
def pair_cols(P, na, nb):
    """sv_reduce_partials_pair's column block (after the wide slab, which none of these calls reaches: n < 65536)"""
    cols = 256 if P <= 4 else 128 if P <= 8 else 64
    while cols > 4 and cdiv(na, cols) + cdiv(nb, cols) < 512:
        cols >>= 1
    return cols


def fold_depth(P, na, nb=0, multi=False):
    """additions a partial passes through in reduce_pair_kernel<C4> (PG = 256 / C4 row groups of ceil(P / PG) rows, PG
    / F of them per thread of the second stage, F <= 16 in the last) or reduce_multi_kernel's deep body (C4 = 16), and
    the addition into the prior"""
    assert max(na, nb) < 65536 or P > 64, "the wide body is not restated here"
    c4 = 16 if multi else pair_cols(P, na, nb) // 4
    pg = 256 // c4
    f = min(pg, 16)
    return cdiv(P, pg) + pg // f + f + 1


# -------------------------------------------------------------------------------------------------------- operands
def _rt(t, dt):
    return t.to(dt).to(F64)


def f32r(t):
    return t.float().double()


def _gen(*key):
    s = 0
    for i, v in enumerate(key):
        s = (s * 1000003 + sum(map(ord, str(v))) * (i + 1)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _signed(g, shape, lo, hi):
    mag = torch.rand(shape, generator=g, dtype=F64) * (hi - lo) + lo
    return mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()


@functools.lru_cache(maxsize=None)
def prior(shape, tag):
    return _rt(torch.rand(shape, generator=_gen("prior", shape, tag), dtype=F64) * 4 - 2, F32)


@functools.lru_cache(maxsize=None)
def rsqrt_rel():
    """4 x the largest relative error of torch's float32 CPU rsqrt against float64 on the same arguments"""
    v = torch.logspace(-7, 4, 200001, dtype=F64).float()
    rel = float(((v.rsqrt().double() - v.double().rsqrt()) * v.double().sqrt()).abs().max())
    return 4 * rel


# ---------------------------------------------------------------------------------------------------- depthwise
@functools.lru_cache(maxsize=None)
def dw_operands(shape, x_dt, dz_dt, mfma=False):
    """x, dz [B,H,W,C]: |.| uniform in [0.5, 1.5], random sign; w [C,49] |.| in [0.1, 0.3], random sign (f32; for the
    matrix-core arms ``wq`` / ``xq`` are the bf16 roundings the kernel takes); bias in [-0.1, 0.1]"""
    B, H, W, C = shape
    g = _gen("dw", shape, x_dt, dz_dt)
    o = dict(x=_rt(_signed(g, shape, 0.5, 1.5), DTN[x_dt]), dz=_rt(_signed(g, shape, 0.5, 1.5), DTN[dz_dt]),
             w=_rt(_signed(g, (C, 49), 0.1, 0.3), F32), b=_rt(torch.rand(C, generator=g, dtype=F64) * 0.2 - 0.1, F32))
    o["lnw"] = _rt(torch.rand(C, generator=g, dtype=F64) + 0.5, F32)
    o["lnb"] = _rt(_signed(g, (C,), 0.2, 0.4), F32)
    o["wq"], o["xq"] = (_rt(o["w"], BF), _rt(o["x"], BF)) if mfma else (o["w"], o["x"])
    return o


def dw_conv(x, w, flip=False, skip=None):
    """sum_tap w[c][tap] x[p + tap - 3] (NHWC, zero padding); ``flip``: w[48 - tap]; ``skip``: a tap left out"""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    out = torch.zeros_like(x)
    for kh in range(7):
        for kw in range(7):
            t = kh * 7 + kw
            if t != skip:
                out += w[:, 48 - t if flip else t] * xp[:, kh:kh + H, kw:kw + W]
    return out


def dw_wgrad(dz, x):
    """dW[c][tap] = sum_p dz[p] x[p + tap - 3] -> [C,49]"""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    return torch.stack([(dz * xp[:, kh:kh + H, kw:kw + W]).sum((0, 1, 2)) for kh in range(7) for kw in range(7)], 1)


def bf16_step(t):
    """the spacing of bf16 numbers around t (float64)"""
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - 7)


def stored(z, e, dt):
    """what a store of z (known within e) to ``dt`` can hold: (the rounding of z, the bound of its distance from
    whatever the kernel stored).  f32: e.  bf16: one step where z lies within e of a rounding boundary, else 0."""
    if dt == F32:
        return z, e
    zs = _rt(z, BF)
    step = bf16_step(z)
    near = (step / 2 - (z - zs).abs()) <= e
    return zs, torch.where(near, step, torch.zeros_like(z))


@functools.lru_cache(maxsize=None)
def dw_fwd_ref(shape, x_dt, act_dt, mfma):
    """-> refs z / y / mean / rstd -> (ref, bound before the store), and the sensitivity share of a dropped centre tap"""
    B, H, W, C = shape
    o = dw_operands(shape, x_dt, "f32", mfma)
    z = dw_conv(o["xq"], o["wq"]) + o["b"]
    S = dw_conv(o["xq"].abs(), o["wq"].abs()) + o["b"].abs()
    n = DWM_K_FWD + 1 if mfma else 49
    ez = n * U24 * S
    adt = DTN[act_dt]
    zs, e = stored(z, ez, adt)
    refs = dict(z=(z, ez))
    refs.update(ln_fwd_ref_of(zs.view(-1, C), o["lnw"], o["lnb"], e.view(-1, C)))
    drop = (o["wq"][:, 24] * o["xq"]).abs()
    sens = dict(z=_share(drop, ez + store_bound(z, adt)))
    return refs, sens


@functools.lru_cache(maxsize=None)
def dw_bwd_data_ref(shape, dz_dt, mfma, accumulate):
    B, H, W, C = shape
    o = dw_operands(shape, "f32", dz_dt, mfma)
    t = dw_conv(o["dz"], o["wq"], flip=True)
    S = dw_conv(o["dz"].abs(), o["wq"].abs(), flip=True)
    b = (DWM_K_FWD if mfma else 49) * U24 * S
    p = prior(shape, "dx") if accumulate else None
    ref = t + p if accumulate else t
    b = b + (store_bound(ref, F32, p, t) if accumulate else store_bound(ref, F32))
    drop = (o["wq"][:, 24] * o["dz"]).abs()
    return dict(dx=(ref, b)), dict(dx=_share(drop, b)), p


def dw_wgrad_depth(shape, mfma, wgs=DW_WGS, multi=False):
    """-> (dw chain, db chain).  VALU: a wave's tiles x 16 rows x 4 columns of fmas, the 4 waves added in turn, the
    fold.  Matrix cores: a workgroup's tiles x the tile's K extent (the MFMA's accumulation length per tap, zero
    columns included), the fold; the bias: a thread's items per tile (16 TW C8 / 256, C8 = 2), 128 threads in order."""
    B, H, W, C = shape
    if mfma:
        P = dwm_wgrad_nparts(*shape)
        tiles = cdiv(dwm_geo(*shape)[1], P)
        fold = fold_depth(P, C * 49, C, multi)
        return tiles * dwm_wgrad_k(W) + fold, tiles * (16 * dwm_geo(*shape)[0] * 2 // 256) + 128 + fold
    P = dw_wgrad_nparts(B, H, W, C, wgs)
    n = dw_wgrad_tiles_per_wave(B, H, W, C, wgs) * 64 + 4 + fold_depth(P, C * 49, C, multi)
    return n, n


@functools.lru_cache(maxsize=None)
def dw_bwd_weight_ref(shape, dz_dt, x_dt, mfma, wgs=DW_WGS, multi=False):
    """dw / db with the priors added -> refs, sensitivity (one pixel dropped: the RMS over the pixels of its
    contribution to a tap, per channel and tap), priors"""
    B, H, W, C = shape
    o = dw_operands(shape, x_dt, dz_dt, mfma)
    x, dz = o["xq"], o["dz"]
    tw, tb = dw_wgrad(dz, x), dz.sum((0, 1, 2))
    Sw, Sb = dw_wgrad(dz.abs(), x.abs()), dz.abs().sum((0, 1, 2))
    nw, nb = dw_wgrad_depth(shape, mfma, wgs, multi)
    pw, pb = prior((C, 49), "dw"), prior((C,), "db")
    refs = dict(dw=(tw + pw, nw * U24 * Sw + store_bound(None, F32, pw, tw)),
                db=(tb + pb, nb * U24 * Sb + store_bound(None, F32, pb, tb)))
    n_pix = B * H * W
    rms_w = (dw_wgrad(dz * dz, x * x) / n_pix).sqrt()
    rms_b = (dz * dz).mean((0, 1, 2)).sqrt()
    live = Sw > 0  # a tap that no pixel of so small an image reaches has nothing to drop
    sens = dict(dw=_share(rms_w[live], refs["dw"][1][live]), db=_share(rms_b, refs["db"][1]))
    return refs, sens, dict(dw=pw, db=pb)


# ---------------------------------------------------------------------------------------------------- LayerNorm
RATIOS = (0.0, 1.0, 4.0, 64.0)


@functools.lru_cache(maxsize=None)
def ln_rows(rows, C, dt, tag=""):
    """[rows, C]: |mean| / std 0, 1, 4, 64 cycling by row; row 1 (if any) exactly constant, row 2 zero but for one
    channel"""
    g = _gen("ln", rows, C, dt, tag)
    std = torch.rand(rows, 1, generator=g, dtype=F64) + 0.5
    ratio = torch.tensor(RATIOS, dtype=F64)[torch.arange(rows) % 4].view(rows, 1)
    sign = torch.where(torch.arange(rows) % 8 < 4, 1.0, -1.0).double().view(rows, 1)
    x = torch.randn(rows, C, generator=g, dtype=F64) * std + sign * ratio * std
    if rows > 1:
        x[1] = 0.75
    if rows > 2:
        x[2] = 0.0
        x[2, C // 3] = 2.5
    return _rt(x, DTN[dt])


@functools.lru_cache(maxsize=None)
def ln_params(C, tag=""):
    g = _gen("lnp", C, tag)
    return _rt(torch.rand(C, generator=g, dtype=F64) + 0.5, F32), _rt(_signed(g, (C,), 0.2, 0.4), F32)


def row_stats(x):
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, var, (var + EPS).rsqrt()


def ln_fwd_ref_of(x, w, b, e=None, D=None):
    """LayerNorm over the rows of x (float64 values the kernel reads within ``e``): y / mean / rstd -> (ref, bound
    before the store).  mean: D 2^-24 mean |x| for the sum, the rounding of 1 / C and of the product.  var: the kernel
    centres on ITS mean, sum (x - mu')^2 = sum (x - mu)^2 + C (mu - mu')^2 exactly, so the mean's error enters squared;
    each term rounds three times (difference, square), the sum D + 1 times, 1 / C and the product once each.  rstd:
    the derivative of rsqrt, the rounding of var + eps, rsqrtf's own error.  y = (x - mu) rs w + b: one rounding per
    operation."""
    rows, C = x.shape
    D = ln_row_depth(C) if D is None else D
    mean, var, rstd = row_stats(x)
    d = x - mean[:, None]
    dmu = D * U24 * x.abs().mean(1) + 2 * U24 * mean.abs()
    dvar = dmu ** 2 + (D + 6) * U24 * (var + dmu ** 2)
    if e is not None:  # first order in the producer's error, absolute values throughout
        dmu = dmu + e.mean(1)
        dvar = dvar + 2 * (d.abs() * e).mean(1) + (e * e).mean(1)
    drs = rstd * ((dvar + U24 * (var + EPS)) / (2 * (var + EPS)) + rsqrt_rel())
    dd = dmu[:, None] + U24 * d.abs() + (e if e is not None else 0)
    t = d * rstd[:, None] * w
    y = t + b
    dy = w.abs() * (rstd[:, None] * dd + d.abs() * drs[:, None]) + 2 * U24 * t.abs() + U24 * y.abs()
    return dict(y=(y, dy), mean=(mean, dmu), rstd=(rstd, drs))


@functools.lru_cache(maxsize=None)
def ln_fwd_ref(rows, C, x_dt):
    x = ln_rows(rows, C, x_dt)
    w, b = ln_params(C)
    refs = ln_fwd_ref_of(x, w, b)
    # one channel dropped from a row's statistics: the RMS over the channels of the change of mean and of rstd
    mean, var, rstd = row_stats(x)
    d = x - mean[:, None]
    ch_mean = (x.pow(2).mean(1)).sqrt() / C
    ch_rstd = rstd * ((d * d - var[:, None]).pow(2).mean(1)).sqrt() / C / (2 * (var + EPS))
    live = var > 0  # the constant row: every channel equals the mean, dropping one changes nothing
    sens = dict(mean=_share(ch_mean[live], refs["mean"][1][live]), rstd=_share(ch_rstd[live], refs["rstd"][1][live]))
    return refs, sens


def ln_bwd_core(d, x, mean, rstd, w, D, exh=None):
    """dx = rs (g - mean(g) - xhat mean(g xhat)), g = d w, with mean / rstd the f32 roundings of the float64 statistics
    -> (dx, bound, xhat, dxhat).  dxhat = 2^-24 (|mu| rs + 3 |xhat|): the mean's rounding; rstd's, the difference's and
    the product's (+ ``exh``, the error of a recomputed x times rstd).  One rounding per operation after that; the two
    row sums carry D 2^-24 of their absolute sums."""
    C = x.shape[1]
    rs = rstd[:, None]
    xh = (x - mean[:, None]) * rs
    dxh = U24 * (mean.abs()[:, None] * rs + 3 * xh.abs()) + (exh if exh is not None else 0)
    g = d * w
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ds1 = (D + 1) * U24 * g.abs().mean(1, keepdim=True) + 2 * U24 * s1.abs()
    ds2 = (D + 2) * U24 * (g * xh).abs().mean(1, keepdim=True) + (g.abs() * dxh).mean(1, keepdim=True) + 2 * U24 * s2.abs()
    inner = g - s1 - xh * s2
    dx = rs * inner
    b = rs * (U24 * g.abs() + ds1 + dxh * s2.abs() + xh.abs() * ds2 + U24 * (xh * s2).abs()
              + U24 * ((g - s1).abs() + inner.abs())) + 2 * U24 * dx.abs()
    return dx, b, xh, dxh


def red_bounds(d, xh, dxh, n):
    """the per-channel sums over rows: dw = sum d xhat within n 2^-24 sum |d xhat| + sum |d| dxhat + 2^-24 sum |d xhat|
    (the product's rounding), db = sum d within n 2^-24 sum |d|"""
    a = (d * xh).abs().sum(0)
    return (d * xh).sum(0), (n + 1) * U24 * a + (d.abs() * dxh).sum(0), d.sum(0), n * U24 * d.abs().sum(0)


def ln_bwd_depth(rows, C, multi=False):
    """a row's term: the wave's serial rows, the fold of the wave's row slots (shuffles), the 4 waves, the fold"""
    P = ln_bwd_nparts(rows, C)
    k = ln_vec_kind(C)
    if k:
        rpw = 64 // k[0]
        return cdiv(cdiv(rows, rpw), 4 * P) + int(math.log2(rpw)) + 4 + fold_depth(P, C, C, multi)
    return cdiv(rows, 4 * P) + 4 + fold_depth(P, C, C, multi)


@functools.lru_cache(maxsize=None)
def ln_bwd_ref(rows, C, dy_dt, x_dt, multi=False):
    """-> operands (dy, x, mean, rstd as call inputs, w), refs dx / dw / db (priors added), sens, priors"""
    x = ln_rows(rows, C, x_dt)
    g = _gen("lnbwd", rows, C, dy_dt)
    dy = _rt(_signed(g, (rows, C), 0.5, 1.5), DTN[dy_dt])
    w, _ = ln_params(C)
    mean, var, rstd = row_stats(x)
    dx, bdx, xh, dxh = ln_bwd_core(dy, x, mean, rstd, w, ln_row_depth(C))
    n = ln_bwd_depth(rows, C, multi)
    tw, bw, tb, bb = red_bounds(dy, xh, dxh, n)
    pw, pb = prior((C,), "lnw"), prior((C,), "lnb")
    refs = dict(dx=(dx, bdx), dw=(tw + pw, bw + store_bound(None, F32, pw, tw)),
                db=(tb + pb, bb + store_bound(None, F32, pb, tb)))
    sens = dict(dw=_share(_rms0(dy * xh), refs["dw"][1]), db=_share(_rms0(dy), refs["db"][1]))
    return dict(dy=dy, x=x, mean=mean, rstd=rstd, w=w), refs, sens, dict(dw=pw, db=pb)


def _rms0(t):
    return t.pow(2).mean(0).sqrt()


def _share(change, bound):
    """share of the elements whose float64 change exceeds 4 x bound"""
    return float((change > 4 * bound).double().mean())


# --------------------------------------------------------------------------------------------------- downsample
@functools.lru_cache(maxsize=None)
def ds_ref(shape):
    """LayerNorm2d per pixel + the 2x2 / 2 gather, forward and backward.  patches [(b,i,j)][4 c + 2 kh + kw]."""
    B, H, W, C = shape
    x = ln_rows(B * H * W, C, "f32", "ds")
    w, b = ln_params(C, "ds")
    D = g32_row_depth(C)
    fwd = ln_fwd_ref_of(x, w, b, D=D)

    def gather(t):
        return t.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B * (H // 2) * (W // 2), 4 * C)

    def scatter(t):
        return t.view(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)

    fwd["patches"] = (gather(fwd["y"][0]), gather(fwd["y"][1]))
    del fwd["y"]
    g = _gen("dsbwd", shape)
    dp = _rt(_signed(g, (B * (H // 2) * (W // 2), 4 * C), 0.5, 1.5), F32)
    d = scatter(dp)
    mean, var, rstd = row_stats(x)
    dx, bdx, xh, dxh = ln_bwd_core(d, x, mean, rstd, w, D)
    P = ds_grid(*shape)
    npatch = B * (H // 2) * (W // 2)
    per_wave = cdiv(npatch, 4 * P * (2 if C % 64 else 1))
    n = 4 * per_wave + (8 if C % 64 else 4) + fold_depth(P, C, C)
    tw, bw, tb, bb = red_bounds(d, xh, dxh, n)
    pw, pb = prior((C,), "dslnw"), prior((C,), "dslnb")
    bwd = dict(dx=(dx, bdx), dlnw=(tw + pw, bw + store_bound(None, F32, pw, tw)),
               dlnb=(tb + pb, bb + store_bound(None, F32, pb, tb)))
    sens = dict(dlnw=_share(_rms0(d * xh), bwd["dlnw"][1]), dlnb=_share(_rms0(d), bwd["dlnb"][1]))
    return dict(x=x, w=w, b=b, dp=dp, mean=mean, rstd=rstd), fwd, bwd, sens, dict(dlnw=pw, dlnb=pb)


def ds_arm(shape):
    B, H, W, C = shape
    npatch = B * (H // 2) * (W // 2)
    P = ds_grid(*shape)
    per = 4 * P * (2 if C % 64 else 1)
    return f"{'g32' if C % 64 else 'CPL' + str(C // 64)} grid{P} passes{cdiv(npatch, per)}{' capped' if P == 1024 else ''}"


# -------------------------------------------------------------------------------------------------- pool + LN
def pool_depth(HW):
    """pool_sum_kernel: a wave's rows go to 8 accumulators in turn (ceil(ceil(HW / 4) / 8) additions, the tail loop's
    rows all to the first: at most 7 more), the 8 are joined, the 4 waves added, the division by HW"""
    return cdiv(cdiv(HW, 4), 8) + 7 + 8 + 4


@functools.lru_cache(maxsize=None)
def pool_ref(B, HW, C):
    g = _gen("pool", B, HW, C)
    x = _rt(torch.randn(B, HW, C, generator=g, dtype=F64) + ln_rows(B, C, "f32", "poolmean").view(B, 1, C), F32)
    w, b = ln_params(C, "pool")
    pooled = x.mean(1)
    e = pool_depth(HW) * U24 * x.abs().mean(1) + 2 * U24 * pooled.abs()
    D = cdiv(C, 256) + 6 + 4  # pool_norm_kernel: a thread's channels, the wave butterfly, the 4 waves
    fwd = ln_fwd_ref_of(pooled, w, b, e, D=D)
    fwd["feat"] = fwd.pop("y")
    fwd["pooled"] = (pooled, e)
    sens = dict(pooled=_share(_rms1(x) / HW, e + store_bound(pooled, F32)))
    # backward, judged alone: pooled as an input is the f32 rounding of the float64 one
    pin = f32r(pooled)
    mean, var, rstd = row_stats(pin)
    dfeat = _rt(_signed(g, (B, C), 0.5, 1.5), F32)
    dp, bdp, xh, dxh = ln_bwd_core(dfeat, pin, mean, rstd, w, D)
    dx = (dp / HW).view(B, 1, C).expand(B, HW, C)
    bdx = ((bdp + 2 * U24 * dp.abs()) / HW).view(B, 1, C).expand(B, HW, C)
    tw, bw, tb, bb = red_bounds(dfeat, xh, dxh, fold_depth(B, C, C))
    pw, pb = prior((C,), "poollnw"), prior((C,), "poollnb")
    bwd = dict(dx=(dx, bdx), dlnw=(tw + pw, bw + store_bound(None, F32, pw, tw)),
               dlnb=(tb + pb, bb + store_bound(None, F32, pb, tb)))
    sens.update(dlnw=_share(_rms0(dfeat * xh), bwd["dlnw"][1]), dlnb=_share(_rms0(dfeat), bwd["dlnb"][1]))
    return dict(x=x, w=w, b=b, pooled=pin, mean=mean, rstd=rstd, dfeat=dfeat), fwd, bwd, sens, dict(dlnw=pw, dlnb=pb)


def _rms1(t):
    return t.pow(2).mean(1).sqrt()


def pool_arm(HW):
    """rows per wave (wave 0 first), rounds of the 8-deep loop of wave 0, its tail rows"""
    per = [len(range(w, HW, 4)) for w in range(4)]
    rounds = len([p for p in range(0, HW, 32) if p + 28 < HW])
    return f"rows{'/'.join(map(str, per))} deep{rounds} tail{per[0] - 8 * rounds}"


# -------------------------------------------------------------------------------------------------------- stem
@functools.lru_cache(maxsize=None)
def stem_ref(B, H, W, C):
    """Conv2d(3, C, 4, 4) + LayerNorm2d forward (y, mean, rstd) and backward (dw [C,48], db, dlnw, dlnb)"""
    g = _gen("stem", B, H, W, C)
    img = _rt(torch.randn(B, 3, H, W, generator=g, dtype=F64), F32)
    w = _rt(_signed(g, (C, 48), 0.05, 0.25), F32)
    b = _rt(torch.rand(C, generator=g, dtype=F64) * 0.2 - 0.1, F32)
    lnw, lnb = ln_params(C, "stem")
    Ho, Wo = H // 4, W // 4
    npix = B * Ho * Wo
    p = img.view(B, 3, Ho, 4, Wo, 4).permute(0, 2, 4, 1, 3, 5).reshape(npix, 48)  # k = ci 16 + kh 4 + kw
    z = p @ w.t() + b
    ez = 48 * U24 * (p.abs() @ w.abs().t() + b.abs())
    D = g32_row_depth(C)
    fwd = ln_fwd_ref_of(z, lnw, lnb, ez, D=D)
    sens = dict(y=_share(_rms1(p).view(-1, 1) * w.abs().pow(2).mean(1).sqrt() * lnw.abs() * row_stats(z)[2].view(-1, 1),
                         fwd["y"][1] + store_bound(fwd["y"][0], F32)))
    # backward: mean / rstd of z as inputs; z is recomputed (within ez), so xhat carries ez rstd
    mean, var, rstd = row_stats(z)
    dy = _rt(_signed(g, (npix, C), 0.5, 1.5), F32)
    dz, bdz, xh, dxh = ln_bwd_core(dy, z, mean, rstd, lnw, D, exh=ez * rstd[:, None])
    P = stem_bwd_nparts(B, H, W, C)
    n = cdiv(npix, 4 * P * (2 if C % 64 else 1)) + 4 + fold_depth(P, C * 48, C)
    n2 = cdiv(npix, 4 * P * (2 if C % 64 else 1)) + 4 + fold_depth(P, C, C)
    tlw, blw, tlb, blb = red_bounds(dy, xh, dxh, n2)
    tdw = dz.t() @ p
    bdw = (n + 1) * U24 * (dz.abs().t() @ p.abs()) + bdz.t() @ p.abs()
    tdb = dz.sum(0)
    bdb = n * U24 * dz.abs().sum(0) + bdz.sum(0)
    pr = dict(dw=prior((C, 48), "stemw"), db=prior((C,), "stemb"), dlnw=prior((C,), "stemlw"), dlnb=prior((C,), "stemlb"))
    bwd = {k: (t + pr[k], bb + store_bound(None, F32, pr[k], t))
           for k, t, bb in (("dw", tdw, bdw), ("db", tdb, bdb), ("dlnw", tlw, blw), ("dlnb", tlb, blb))}
    sens.update(dw=_share(((dz * dz).t() @ (p * p) / npix).sqrt(), bwd["dw"][1]), db=_share(_rms0(dz), bwd["db"][1]),
                dlnw=_share(_rms0(dy * xh), bwd["dlnw"][1]), dlnb=_share(_rms0(dy), bwd["dlnb"][1]))
    return dict(img=img, w=w, b=b, lnw=lnw, lnb=lnb, mean=mean, rstd=rstd, dy=dy), fwd, bwd, sens, pr


def stem_arm(B, H, W, C):
    npix = B * (H // 4) * (W // 4)
    P = stem_bwd_nparts(B, H, W, C)
    per = 4 * (2 if C % 64 else 1)
    return f"{'g32' if C % 64 else 'CPL' + str(C // 64)} fwd{stem_grid(B, H, W, C)} bwd{P} passes{cdiv(npix, per * P)}"
