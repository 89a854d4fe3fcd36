"""Float64 CPU references, operands, bounds and the host-side launch geometry for tests/test_bn_calls_gpu.py (the
BatchNorm and pooling calls of csrc/bn.hip).  Test infrastructure only: no kernel is called from here.

A case is ``(rows, C, mode)``; operands are drawn on the CPU in float64 and rounded to the dtype the call takes (bf16
or f32), so the float64 reference and the kernel see the same numbers.  Every reference is the plain float64 formula, the
backward through ``torch.autograd`` of that same expression.  Every bound is derived from the order in which the kernels
sum (below) and from the roundings of the elementwise forms ``bn_pre`` / ``bn_dx``; none is fitted to a kernel's output.

Summation order (csrc/bn.hip).  A statistics pass splits the rows into P = nparts_for(rows, C) parts of rpp = ceil(rows /
P) rows; in a part, each of rp row-groups sums its rows serially (``ceil(rpp / rp)`` additions), ``reduce_write`` adds the
rp groups in order (rp - 1), the fold reads each chunk of up to 1024 partials as 128 streams of 4 accumulators (ceil(ceil(q
/ 128) / 4) additions, 2 to join them), adds the 128 stream sums in order (128) and the chunks in order (S - 1).  A term
passes through at most ``depth`` = the sum of those counts additions, each rounding by at most 2^-24 of a partial sum that
is itself at most sum |t|: |error| <= depth 2^-24 sum |t|."""
import functools

import torch
import torch.nn.functional as F

from _conv_ref import BF, F32, F64, U8, U23, U24, cdiv, store_bound  # noqa: F401  (re-exported for the test file)

EPS, MOM = 1e-5, 0.1
K_THREADS, FOLD_Q, FOLD_MAX_S, FOLD_MAX_C, GRID_CAP = 256, 1024, 16, 2048, 8192


# ----------------------------------------------------------------------------------------- host geometry, restated
def vec_for(C):
    return 8 if C % 8 == 0 and (C // 8 <= K_THREADS or (C // 8) % K_THREADS == 0) else 4


def red_geo(C):
    """-> (vec, tpr, rp, cslices) of a per-channel reduction's workgroup (csrc/bn.hip red_geo)"""
    vec = vec_for(C)
    cg = C // vec
    tpr = min(cg, K_THREADS)
    return vec, tpr, K_THREADS // tpr, cg // tpr


def nparts_for(rows, C):
    vec, tpr, rp, cslices = red_geo(C)
    return max(1, min(rows // (8 * rp), 1024 // cslices))


def grid_for(n):
    return max(1, min(cdiv(n, K_THREADS), GRID_CAP))


def fixc_ok(grid, V, C):
    return (grid * K_THREADS * V) % C == 0


def fold_chunks(P):
    return cdiv(P, FOLD_Q)


def fin_split(P, C):
    """workgroups per channel group of a separate fold launch (csrc/bn.hip fin_split, with the workspace kernels.py
    always hands it)"""
    S = fold_chunks(P)
    return S if 1 < S <= FOLD_MAX_S and C <= FOLD_MAX_C else 1


def stats_arm(rows, C):
    """the arm of a statistics pass: channels per thread, threads per row, row-groups, slices, parts, rows per part"""
    vec, tpr, rp, cs = red_geo(C)
    P = nparts_for(rows, C)
    return f"V{vec} tpr{tpr} rp{rp} slices{cs} P{P} rpp{cdiv(rows, P)}"


def apply_arm(rows, C):
    """the arm of an elementwise pass: channels per thread, hoisted parameters or not, grid capped or not"""
    vec = vec_for(C)
    grid = grid_for(rows * C // vec)
    capped = cdiv(rows * C // vec, K_THREADS) > GRID_CAP
    return f"V{vec} {'fixc' if fixc_ok(grid, vec, C) else 'anyc'} {'capped' if capped else 'grid'}"


def fold_arm(P, C):
    S = fold_chunks(P)
    return f"chunks{S} {'split' if fin_split(P, C) > 1 else 'one-workgroup'}"


def channel_arm(C):
    """what a production BatchNorm's kernels depend on besides the row count"""
    vec, tpr, rp, cs = red_geo(C)
    return f"V{vec} tpr{tpr} rp{rp} slices{cs} {'fixc-always' if (K_THREADS * vec) % C == 0 else 'fixc-by-grid'}"


def fold_depth(P):
    S = fold_chunks(P)
    return cdiv(cdiv(min(P, FOLD_Q), 128), 4) + 2 + 128 + (S - 1)


def depth(rows, C):
    """additions a term of a statistics pass goes through (see the module docstring)"""
    vec, tpr, rp, cs = red_geo(C)
    P = nparts_for(rows, C)
    return cdiv(cdiv(rows, P), rp) + (rp - 1) + fold_depth(P)


def last_rows(rows, C):
    """the rows that are some thread's last of its part: the last min(rp, length) rows of every part"""
    vec, tpr, rp, cs = red_geo(C)
    P = nparts_for(rows, C)
    rpp = cdiv(rows, P)
    idx = []
    for p in range(P):
        r0, r1 = p * rpp, min((p + 1) * rpp, rows)
        idx += list(range(max(r0, r1 - rp), r1))
    return torch.tensor(idx)


# -------------------------------------------------------------------------------------------------------- operands
def _rt(t, dt):
    return t.to(dt).to(F64)


def _gen_stable(*key):
    s = 0
    for i, v in enumerate(key):
        s = (s * 1000003 + sum(map(ord, str(v))) * (i + 1)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ratios(C):
    """|mean| / std per channel: 0, 1 and 4 in turn"""
    return torch.tensor([0.0, 1.0, 4.0], dtype=F64)[torch.arange(C) % 3]


def draw_y(rows, C, dt, tag):
    g = _gen_stable("y", rows, C, tag)
    std = torch.rand(C, generator=g, dtype=F64) + 0.5
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    return _rt(torch.randn(rows, C, generator=g, dtype=F64) * std + sign * ratios(C) * std, dt)


@functools.lru_cache(maxsize=None)
def operands(rows, C, mode):
    """y, res, y2 [rows, C] in the activation dtype of ``mode`` (bf16 / fp32); gamma in [0.5, 1.5], beta around +-0.3,
    a second BatchNorm's gamma2 / beta2; running statistics rm0 / rv0; dout32 / dout16 with a non-zero channel mean"""
    dt = BF if mode == "bf16" else F32
    g = _gen_stable("ops", rows, C, mode)
    o = dict(y=draw_y(rows, C, dt, mode), y2=draw_y(rows, C, dt, mode + "2"))
    o["res"] = _rt(torch.randn(rows, C, generator=g, dtype=F64), dt)
    for s in ("", "2"):
        o["gamma" + s] = _rt(torch.rand(C, generator=g, dtype=F64) + 0.5, F32)
        sgn = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
        o["beta" + s] = _rt(sgn * (0.3 + 0.05 * torch.randn(C, generator=g, dtype=F64)), F32)
    o["rm0"] = _rt(torch.randn(C, generator=g, dtype=F64) * 0.2, F32)
    o["rv0"] = _rt(torch.rand(C, generator=g, dtype=F64) + 0.5, F32)
    d = torch.randn(rows, C, generator=g, dtype=F64) + (torch.rand(C, generator=g, dtype=F64) + 0.5)
    o["dout32"], o["dout16"] = _rt(d, F32), _rt(d, BF)
    return o


def batch_stats(y):
    """float64 (mean, biased variance, rstd)"""
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return mean, var, (var + EPS).rsqrt()


def f32r(t):
    return t.float().double()


# ---------------------------------------------------------------------------------------------- statistics bounds
def finish_bounds(s1, s2, k, n, d1, d2):
    """bn_finish_channel: m1 = s1 / n, var = fma(-m1, m1, s2 / n), mean = k + m1, rstd = 1 / sqrtf(var + eps) (sqrtf and the
    division correctly rounded).  s1 / s2: the exact (shifted by k) sums, d1 / d2 the bounds of the f32 sums' errors.
    -> (dmean, dvar, drstd); dvar = d2 / n + 2^-24 s2 / n + 2 |m1| dm1 + ..: proportional to s2 / n, so the rstd bound
    dvar / (2 (var + eps)) carries the cancellation factor (s2 / n) / var = 1 + (m1 / std)^2 explicitly"""
    m1 = s1 / n
    var = (s2 / n - m1 ** 2).clamp_min(0)
    dm1 = d1 / n + U24 * m1.abs()
    dmean = dm1 + U24 * (k + m1).abs()
    dvar = d2 / n + U24 * s2 / n + 2 * m1.abs() * dm1 + dm1 ** 2 + U24 * var
    rstd = (var + EPS).rsqrt()
    drstd = rstd * ((dvar + U24 * (var + EPS)) / (2 * (var + EPS)) + 2 * U24)
    return dmean, dvar, drstd


def running_bounds(mean, var, n, dmean, dvar, rm0, rv0):
    """-> ((rm ref, bound), (rv ref, bound)): torch's update, unbiased variance; the kernel's fmaf(mom, stat, (1 - mom)
    r0) with momentum and 1 - momentum rounded to f32"""
    ub = var * n / (n - 1) if n > 1 else var
    dub = (dvar * n / (n - 1) if n > 1 else dvar) + 2 * U24 * ub
    out = []
    for stat, dstat, r0 in ((mean, dmean, rm0), (ub, dub, rv0)):
        ref = (1 - MOM) * r0 + MOM * stat
        out.append((ref, MOM * dstat + 3 * U24 * (MOM * stat.abs() + (1 - MOM) * r0.abs()) + U24 * ref.abs()))
    return out


def shifted_sums(y, rows, C):
    """the shifted statistics pass on y: (k, s1, s2, d1, d2) - each term y - k rounds once (2^-24 |y - k|), its square
    carries twice that, the fmaf adds nothing"""
    k = y[0]
    d = y - k
    s1, s2, a1 = d.sum(0), (d * d).sum(0), d.abs().sum(0)
    D = depth(rows, C)
    return k, s1, s2, (D + 1) * U24 * a1, (D + 2) * U24 * s2


@functools.lru_cache(maxsize=None)
def stats_ref(rows, C, mode):
    """bn_stats on operands(rows, C, mode)['y']: name -> (float64 reference, bound), and the sensitivity shares"""
    o = operands(rows, C, mode)
    y = o["y"]
    mean, var, rstd = batch_stats(y)
    k, s1, s2, d1, d2 = shifted_sums(y, rows, C)
    dmean, dvar, drstd = finish_bounds(s1, s2, k, rows, d1, d2)
    (rm, drm), (rv, drv) = running_bounds(mean, var, rows, dmean, dvar, o["rm0"], o["rv0"])
    refs = dict(mean=(mean, dmean), rstd=(rstd, drstd), rm=(rm, drm), rv=(rv, drv))
    d = (y - k)[last_rows(rows, C)]
    sens = dict(mean=_share(_rms(d) / rows, dmean),
                rstd=_share(rstd * _rms(d * d - 2 * (s1 / rows) * d) / rows / (2 * (var + EPS)), drstd))
    return refs, sens


def _rms(t):
    return t.pow(2).mean(0).sqrt()


def _share(change, bound):
    """share of the channels whose float64 change exceeds 4 x bound"""
    return float((change > 4 * bound).double().mean())


# -------------------------------------------------------------------------- unshifted statistics from given partials
def group_bounds(n_groups):
    """row ranges of P groups of 2 and 3 rows in turn"""
    sizes = torch.tensor([2 + (i % 2) for i in range(n_groups)])
    ends = sizes.cumsum(0)
    return ends - sizes, ends


@functools.lru_cache(maxsize=None)
def partials_case(P, C):
    """unshifted partials [P][2][C] (f32 values) of a known bf16 y split into P groups of 2 - 3 rows, the float64
    statistics of y, their bounds and the sensitivity shares.  The reference is y's own float64 statistics: the partials'
    f32 rounding (2^-24 each) and the fold (fold_depth(P) 2^-24 sum |partial|) are both in the bound."""
    starts, ends = group_bounds(P)
    rows = int(ends[-1])
    o = operands(rows, C, "bf16")
    y = draw_y(rows, C, BF, f"part{P}")
    cs1 = torch.cat([torch.zeros(1, C, dtype=F64), y.cumsum(0)])
    cs2 = torch.cat([torch.zeros(1, C, dtype=F64), (y * y).cumsum(0)])
    part = torch.stack([f32r(cs1[ends] - cs1[starts]), f32r(cs2[ends] - cs2[starts])], 1)
    mean, var, rstd = batch_stats(y)
    D = fold_depth(P) + 1
    s1, s2 = y.sum(0), (y * y).sum(0)
    d1, d2 = D * U24 * part[:, 0].abs().sum(0), D * U24 * part[:, 1].sum(0)
    dmean, dvar, drstd = finish_bounds(s1, s2, torch.zeros(C, dtype=F64), rows, d1, d2)
    (rm, drm), (rv, drv) = running_bounds(mean, var, rows, dmean, dvar, o["rm0"], o["rv0"])
    refs = dict(mean=(mean, dmean), rstd=(rstd, drstd), rm=(rm, drm), rv=(rv, drv))
    # a dropped unit: one partial; from 16384 partials on, one stream of one chunk (its 8 partials).  The bound grows as
    # fold_depth 2^-24 sum |partial| ~ 150 x 2^-24 x P partials while one partial is a 1 / P share, so a single one of
    # 16384 (150 x 2^-24 x 16384 = 0.15, times 4) cannot stand out of a worst-case bound; what the fold can drop there is a
    # stream, a chunk or the tail, all of 8 partials or more
    unit = part
    if P >= 16384:
        n_c = P // FOLD_Q
        unit = part[:n_c * FOLD_Q].view(n_c, FOLD_Q // 128, 128, 2, C).sum(1).view(-1, 2, C)
    sens = dict(mean=_share(_rms(unit[:, 0]) / rows, dmean),
                rstd=_share(rstd * _rms(unit[:, 1] - 2 * mean * unit[:, 0]) / rows / (2 * (var + EPS)), drstd))
    return dict(part=part, rows=rows, rm0=o["rm0"], rv0=o["rv0"], refs=refs, sens=sens, var=var, mean=mean)


def finish_of(part, rows, rm0, rv0):
    """the finish judged alone on partials a kernel produced (the conv epilogue's): the float64 statistics of exactly
    those f32 partials, bounded by the fold alone"""
    P = part.shape[0]
    p = part.double()
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    D = fold_depth(P)
    mean = s1 / rows
    var = (s2 / rows - mean ** 2).clamp_min(0)
    dmean, dvar, drstd = finish_bounds(s1, s2, torch.zeros_like(s1), rows, D * U24 * p[:, 0].abs().sum(0),
                                       D * U24 * p[:, 1].abs().sum(0))
    (rm, drm), (rv, drv) = running_bounds(mean, var, rows, dmean, dvar, rm0, rv0)
    return dict(mean=(mean, dmean), rstd=((var + EPS).rsqrt(), drstd), rm=(rm, drm), rv=(rv, drv))


# ------------------------------------------------------------------------------------------------------ forward
def pre_bound(gamma, rstd, y, mean, beta):
    """(pre, bound): bn_pre = fmaf(gamma rstd, y - mean, beta) with mean / rstd the f32 roundings of the float64
    statistics: 2^-24 (|A mean| + 3 |A (y - mean)| + |pre|), A = gamma rstd (the mean's rounding; rstd's, the product
    A's and the difference's; the fmaf's)"""
    A = gamma * rstd
    t = A * (y - mean)
    pre = t + beta
    return pre, U24 * ((A * mean).abs() + 3 * t.abs() + pre.abs())


@functools.lru_cache(maxsize=None)
def act_ref(rows, C, mode, res_kind, relu):
    """act(BN(y) + r): r absent (""), the residual ("res") or a second BatchNorm of y2 ("res_bn") -> (ref, bound before
    the store); the statistics are the batch's own float64 ones"""
    o = operands(rows, C, mode)
    mean, var, rstd = batch_stats(o["y"])
    ref, b = pre_bound(o["gamma"], rstd, o["y"], mean, o["beta"])
    if res_kind == "res":
        ref = ref + o["res"]
        b = b + U24 * ref.abs()
    elif res_kind == "res_bn":
        m2, v2, r2 = batch_stats(o["y2"])
        p2, b2 = pre_bound(o["gamma2"], r2, o["y2"], m2, o["beta2"])
        ref = ref + p2
        b = b + b2 + U24 * ref.abs()
    return (ref.clamp_min(0) if relu else ref), b


def tau(gamma, rstd, y, mean, beta):
    """the margin below which f32 cannot decide the sign of the pre-activation: twice pre_bound"""
    return 2 * pre_bound(gamma, rstd, y, mean, beta)[1]


# ------------------------------------------------------------------------------------------------------ backward
def _bn_expr(y, gamma, beta, train, mean, rstd):
    if train:
        mean = y.mean(0)
        rstd = (((y - mean) ** 2).mean(0) + EPS).rsqrt()
    return gamma * (y - mean) * rstd + beta


def sum_bounds(g, xhat, mu_rs, D):
    """the backward sums of one BatchNorm over the masked gradient g: sg = sum g within D 2^-24 sum |g|; sgx = sum g
    xhat within D 2^-24 sum |g xhat| + sum |g| dxhat, dxhat = 2^-24 (3 |xhat| + |mean| rstd) (the roundings of mean,
    rstd, the difference and the product; the fmaf adds none)"""
    dxh = U24 * (3 * xhat.abs() + mu_rs)
    return D * U24 * g.abs().sum(0), D * U24 * (g * xhat).abs().sum(0) + (g.abs() * dxh).sum(0), dxh


def dx_bound(A, g, xhat, dxh, sg, sgx, dsg, dsgx, n, dx):
    """bn_dx = (gamma rstd) fma(-(xhat sgx), 1/n, fma(-sg, 1/n, g)) against A (g - sg / n - xhat sgx / n): the sums'
    errors, xhat's, 1/n's rounding and one rounding per operation"""
    a1 = g - sg / n
    t3 = xhat * sgx / n
    inner = a1 - t3
    return A * (dsg / n + (dxh * sgx.abs() + xhat.abs() * dsgx) / n
                + U24 * (2 * (sg / n).abs() + a1.abs() + 3 * t3.abs() + inner.abs())) + 3 * U24 * dx.abs()


@functools.lru_cache(maxsize=None)
def bwd_ref(rows, C, mode, form, dout_dt, train, D=None):
    """One BatchNorm backward.  form: "plain" (no mask), "act" (mask = act > 0, act the rounded forward output with the
    residual), "relu" (the BatchNorm's own ReLU, mask recomputed), "dual" (act mask, two BatchNorms).
    -> dict: dout (ties zeroed for "relu"), act, g, refs name -> (ref, bound before store / prior), tie share, sens.
    ``D``: the sums' depth when the partials are not the statistics pass's own."""
    o = operands(rows, C, mode)
    adt = BF if mode == "bf16" else F32
    y, gamma, beta = o["y"], o["gamma"], o["beta"]
    mean, var, rstd = batch_stats(y)
    dout = o["dout16" if dout_dt == BF else "dout32"].clone()
    D = depth(rows, C) if D is None else D
    r = dict(ties=0.0, act=None)
    yv = y.clone().requires_grad_(True)
    gv, bv = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    pre = _bn_expr(yv, gv, bv, train, mean, rstd)
    if form == "relu":
        tie = pre.detach().abs() < tau(gamma, rstd, y, mean, beta)
        dout[tie] = 0.0
        r["ties"] = float(tie.double().mean())
        out, g = pre.clamp_min(0), dout * (pre.detach() > 0)
    elif form == "plain":
        out, g = pre, dout
    else:
        act = _rt((pre.detach() + o["res"]).clamp_min(0), adt)
        r["act"] = act
        out, g = pre, dout * (act > 0)
    ins = [yv, gv, bv]
    if form == "dual":
        m2, v2, r2 = batch_stats(o["y2"])
        y2v = o["y2"].clone().requires_grad_(True)
        g2v, b2v = o["gamma2"].clone().requires_grad_(True), o["beta2"].clone().requires_grad_(True)
        out = out + _bn_expr(y2v, g2v, b2v, train, m2, r2)
        ins += [y2v, g2v, b2v]
    grads = torch.autograd.grad(out, ins, dout if form == "relu" else g)
    r["dout"], r["g"] = dout, g
    refs, sens = {}, {}
    last = last_rows(rows, C)
    bns = {"": (y, gamma, mean, rstd, grads[:3])}
    if form == "dual":
        bns["2"] = (o["y2"], o["gamma2"], m2, r2, grads[3:])
    for s, (yy, gam, mu, rs, gr) in bns.items():
        xhat = (yy - mu) * rs
        sg, sgx = g.sum(0), (g * xhat).sum(0)
        dsg, dsgx, dxh = sum_bounds(g, xhat, mu.abs() * rs, D)
        refs["dgamma" + s], refs["dbeta" + s] = (gr[1], dsgx), (gr[2], dsg)
        A = gam * rs
        if train:
            refs["dx" + s] = (gr[0], dx_bound(A, g, xhat, dxh, sg, sgx, dsg, dsgx, rows, gr[0]))
        else:
            refs["dx" + s] = (gr[0], 3 * U24 * gr[0].abs())  # (gamma rstd) g: rstd's rounding and two products
        gl, xl = g[last], xhat[last]
        live = (gl != 0).any(0)  # a channel whose candidate rows are all masked has nothing to drop (5 rows: 2^-5)
        sens["dbeta" + s] = _share(_rms(gl)[live], dsg[live])
        sens["dgamma" + s] = _share(_rms(gl * xl)[live], dsgx[live])
        if train:  # dx through its sums: some element of the channel moves by more than 4 x its bound
            move = A * (_rms(gl) ** 2 + xhat ** 2 * _rms(gl * xl) ** 2).sqrt() / rows
            hit = (move / (refs["dx" + s][1] + store_bound(gr[0], BF))).max(0).values > 4
            sens["dx" + s] = float(hit[live].double().mean())
    r["refs"], r["sens"] = refs, sens
    return r


# ------------------------------------------------------------------------------------------------------ pooling
def pool_out(n):
    return (n - 1) // 2 + 1


def _taps(x):
    """NHWC [B,H,W,C] -> [B,OH,OW,C,9] the 3x3 / 2 windows in scan order, -inf outside"""
    B, H, W, C = x.shape
    OH, OW = pool_out(H), pool_out(W)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    cols = [xp[:, :, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] for kh in range(3) for kw in range(3)]
    return torch.stack(cols, -1).permute(0, 2, 3, 1, 4)


def maxpool_ref(x):
    """-> (values [B,OH,OW,C], the first tap in scan order holding the maximum, uint8 3 kh + kw, taps)"""
    t = _taps(x)
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    w = (t == y.unsqueeze(-1)).long() * torch.arange(9, 0, -1)
    return y, w.argmax(-1).to(torch.uint8), t


def maxpool_bwd_ref(d, idx, H, W):
    """float64 scatter of d [B,OH,OW,C] to the input pixel idx names, NHWC [B,H,W,C]"""
    B, OH, OW, C = d.shape
    dx = torch.zeros(B, H + 2, W + 2, C, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            dx[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] += d * (idx == 3 * kh + kw)
    return dx[:, 1:H + 1, 1:W + 1].contiguous()


def pool_target(idx, H, W):
    """flat input pixel index [B,OH,OW,C] (b, iy, ix) each pooled element's gradient lands on"""
    B, OH, OW, C = idx.shape
    kh, kw = idx.long() // 3, idx.long() % 3
    oy = torch.arange(OH).view(1, OH, 1, 1)
    ox = torch.arange(OW).view(1, 1, OW, 1)
    b = torch.arange(B).view(B, 1, 1, 1)
    return (b * H + 2 * oy - 1 + kh) * W + 2 * ox - 1 + kw


@functools.lru_cache(maxsize=None)
def pool_input(B, H, W, C, mode):
    """a post-ReLU activation: five in six exact zeros, so about a fifth of the windows hold nothing else and tie"""
    g = _gen_stable("pool", B, H, W, C, mode)
    return _rt((torch.randn(B, H, W, C, generator=g, dtype=F64) - 1).clamp_min(0), BF if mode == "bf16" else F32)


@functools.lru_cache(maxsize=None)
def pooled_ref(B, H, W, C, mode, dpool_dt, train):
    """bn_relu_bwd_pooled: the stem's BatchNorm + ReLU + max pool.  The activation a = relu(BN(y)) rounded to the
    activation dtype feeds the reference max pool, whose idx is the call's input; the pooled gradients that land on an
    element whose sign f32 cannot decide are set to exactly 0."""
    rows = B * H * W
    o = operands(rows, C, mode)
    adt = BF if mode == "bf16" else F32
    y, gamma, beta = o["y"], o["gamma"], o["beta"]
    mean, var, rstd = batch_stats(y)
    pre = pre_bound(gamma, rstd, y, mean, beta)[0]
    a = _rt(pre.clamp_min(0), adt).view(B, H, W, C)
    _, idx, _ = maxpool_ref(a)
    OH, OW = idx.shape[1:3]
    g = _gen_stable("dpool", B, H, W, C, mode)
    dpool = _rt(torch.randn(B, OH, OW, C, generator=g, dtype=F64) + 0.75, dpool_dt)
    tie = (pre.abs() < tau(gamma, rstd, y, mean, beta)).view(rows, C)
    tgt = pool_target(idx, H, W)
    hit = tie.gather(0, tgt.view(-1, C)).view(B, OH, OW, C)
    dpool[hit] = 0.0
    da = maxpool_bwd_ref(dpool, idx, H, W).view(rows, C)
    yv = y.clone().requires_grad_(True)
    gv, bv = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = _bn_expr(yv, gv, bv, train, mean, rstd).clamp_min(0)
    dx, dgam, dbet = torch.autograd.grad(out, [yv, gv, bv], da)
    gm = da * (pre > 0).view(rows, C)
    xhat = (y - mean) * rstd
    D = depth(rows, C) + 3  # up to four windows are added into one element before it enters the sums
    dsg, dsgx, dxh = sum_bounds(gm, xhat, mean.abs() * rstd, D)
    dsg, dsgx = dsg + 3 * U24 * gm.abs().sum(0), dsgx + 3 * U24 * (gm * xhat).abs().sum(0)
    if train:
        bdx = dx_bound(gamma * rstd, gm, xhat, dxh, gm.sum(0), (gm * xhat).sum(0), dsg, dsgx, rows, dx) \
            + gamma * rstd * 3 * U24 * gm.abs()
    else:
        bdx = 6 * U24 * dx.abs()  # the eval form's 3, and the gather's up to 3 additions
    last = last_rows(rows, C)
    sens = dict(dbeta=_share(_rms(gm[last]), dsg), dgamma=_share(_rms((gm * xhat)[last]), dsgx))
    return dict(dpool=dpool, idx=idx, refs=dict(dx=(dx, bdx), dgamma=(dgam, dsgx), dbeta=(dbet, dsg)),
                ties=float(hit.double().mean()), sens=sens)


@functools.lru_cache(maxsize=None)
def prior(C, tag):
    g = _gen_stable("prior", C, tag)
    return _rt(torch.rand(C, generator=g, dtype=F64) * 4 - 2, F32)


# --------------------------------------------------------------------------------------- production BatchNorms
# resnet18/34/50/101/152, wide_resnet50_2 and resnext50_32x4d under backbone/resnet.py's names
MODELS = ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152", "wide_resnet50", "resnext50")


def production_channels(create):
    """the channel counts of every BatchNorm2d of the ResNet family (``create``: backbone.resnet.create_resnet); the
    modules are built without storage"""
    with torch.device("meta"):
        return sorted({m.num_features for name in MODELS for m in create(name).modules()
                       if isinstance(m, torch.nn.BatchNorm2d)})
