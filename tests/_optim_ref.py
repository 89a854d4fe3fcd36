"""Float64 references, inputs, per-element bounds and the launchers' arm rules (restated from csrc/optim.hip) for
tests/test_optim_calls_gpu.py and tests/test_optim_calls_cpu.py.  Test infrastructure only; nothing here imports the
kernel library.

u = 2^-24 (one f32 rounding, round to nearest even).  hipcc's default keeps f32 division and sqrtf correctly rounded, so
each counts as one rounding.  Every bound is first order in u and stated from the kernels' operation sequence; a
contraction to FMA removes roundings and only tightens it.

AdamW (adamw_kernel; the same statements in its float4 loop and its scalar tail).  The reference is the decoupled update
in float64 from the f32 scalars that cross the C ABI (lr, beta1, beta2, eps, weight_decay rounded to f32; bc1 = f32(1 -
b1^step), bc2s = sqrtf(f32(1 - b2^step)) as kernels.adamw_hyper states them, restated in ``hyper_row``; sc = the f32 clip
coefficient read back, 1 when there is none):
    gk = g sc                       one rounding (none when sc = 1)
    m' = b1 m + (1 - b1) gk         1 - b1 is exact (Sterbenz: 0.5 <= b1 <= 2 x 0.5); b1 m passes its product and the sum
                                    (2u), (1 - b1) gk the rounding of gk, its product and the sum (3u):
                                    Em = 3u (|b1 m| + |(1 - b1) g sc|)
    v' = b2 v + ((1 - b2) gk) gk    the second term carries gk twice (2u), two products and the sum (5u), the first 2u;
                                    both are non-negative: Ev = 5u v'
    decay = 1 - lr wd               lr wd rounds (u lr wd), the difference rounds (u decay): |error| <= u
    pk = p decay                    u |p| from decay, u |p| from the product
    r = sqrtf(v') / bc2s + eps      the kernel's v' is within 5u: 2.5u after the root, + root, quotient, sum = 5.5u
    upd = (lr / bc1) (m' / r)       Em / r from m', 5.5u from r, the quotient, lr / bc1 and the product: 8.5u
    p' = pk - upd                   u |p'| <= u (|p| + |upd|)
                                    Ep = u (3 |p| + 9.5 |upd|) + (lr / bc1) Em / r
(1 - lr wd in float64: at lr = 1e-4, wd = 1e-5 the kernel's decay rounds to 1.0f, as torch's does in float32; that is
inside the u |p| the bound allows for decay.)

Sums.  out (+)= alpha sum_p part[p]: |error| <= (d + 2) u (|alpha| sum_p |part| + |prior|), d the roundings of the
longest chain of additions in the body that runs (an addition to a zero accumulator is exact, so d <= P - 1 whatever
the order), + 1 for alpha, + 1 for the prior.  Per body, from the source:
    reduce_partials_kernel (the wide arm of _pair and _multi, _bf16, sv_reduce_partials per group): one accumulator per
        column over the group's rows in order: d = rows - 1                                         -> ``wide_depth``
    reduce_pair_kernel<C4> (cols = 4 C4; the deep body of _multi is <16>): PG = 256 / C4 row groups; a thread adds
        rows pg, pg + PG, ... (ceil(P / PG) - 1 roundings; the 4-deep unroll adds in the same order), F = min(PG, 16)
        threads add PG / F groups each from zero (PG / F - 1), one thread adds the F sums (F - 1)   -> ``pair_depth``
    colsum_kernel: one accumulator per column over the block's rpb = ceil(rows / 512) rows: d = rpb - 1; colsum_into
        folds the partials through reduce_pair_kernel<1> (cols = 4 at every C <= 2048), the depths add.
bf16 slabs widen exactly (a shift), so the operands are exact and the same bound holds.

Squared norm.  All terms are non-negative, so the bounds are relative.  sqnorm_kernel: a float4's squares pass their
product (the "+ 1") and 3 additions, the thread's accumulator takes one addition per lap (L = ceil(n4 / (grid 256))) and
one for a tail element, block_sum is 6 shuffle additions + 4; clip_coef_kernel: ceil(P / 256) per thread, block_sum again.
    d = 3 + L + 1 + 10 + ceil(P / 256) + 10                                                        -> ``sq_depth``
    sum within (d + 1) u, norm = sqrtf(sum) within ((d + 1) / 2 + 1) u, coef = max_norm / (norm + 1e-6f) 2u more (the
    sum of two positive terms and the quotient; max_norm and 1e-6f are the f32 values the kernel holds).
A one-hot gradient adds zeros only: the square, the root: 1.5u, held to the 2u the issue sets."""
import functools
import math

import numpy as np
import torch

from _conv_ref import F32, F64, U24, cdiv

U = U24
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
# (lr, weight_decay, step): FlatAdamW's defaults; the oracle's (1 - lr wd rounds to 1.0f); a late step; no decay
HYPERS = [(1e-3, 1e-2, 3), (1e-4, 1e-5, 1), (3.7e-5, 0.05, 10000), (1e-3, 0.0, 2)]
KTHREADS = 256
ADAMW_LAP = 2048 * KTHREADS * 4  # stream_grid(n, 4) caps at 2048 workgroups of 256 threads x 4 elements
SQ_LAP = 1024 * KTHREADS * 4  # kSqBlocks
CAST_LAP = 2048 * KTHREADS
SMALL = [1, 3, 4, 5, 1023, 1024, 1027]
ADAMW_BIG = 2 * ADAMW_LAP + 1024 + 3  # two full laps, a partial third, a scalar tail
SQ_BIG = 2 * SQ_LAP + 1024 + 3
CAST_BIG = 2 * CAST_LAP + 77
SCALES = [None, 0.37117, 1.0]  # no coefficient; a device coefficient below 1; a coefficient of exactly 1
GENERIC, FIRST, GZERO, PAD, EPSD, CANCEL = range(6)
CLASS_NAMES = ["generic", "first_step", "g_zero", "padding", "eps_dominated", "cancelling"]
_CLASS_OF = torch.tensor([GENERIC, PAD, GENERIC, CANCEL, GZERO, GENERIC, EPSD, FIRST])


def f32v(x):
    return float(np.float32(x))


def hyper_row(lr, step):
    """[lr, 1 - b1^step, sqrt(1 - b2^step)] as sv_adamw_flat derives them: the betas as f32, the power in double, the
    difference rounded to f32, the root taken in f32 (kernels.adamw_hyper, restated)"""
    b1, b2 = f32v(BETA1), f32v(BETA2)
    return [f32v(lr), float(np.float32(1.0 - b1 ** step)), float(np.sqrt(np.float32(1.0 - b2 ** step), dtype=np.float32))]


def classes(n):
    """element i's class: (5 i) mod 8 through _CLASS_OF, so that n = 3, 4, 5 already mix classes and every float4 does"""
    return _CLASS_OF[(5 * torch.arange(n)) % 8]


@functools.lru_cache(maxsize=4)
def adamw_inputs(n, sc=1.0, seed=0):
    """(p, g, m, v) f32 CPU tensors and the class of each element.  ``sc`` is the f32 gradient scale the case will run
    under: the eps-dominated class has |g sc| ~ 1e-9, v ~ 1e-18, and the cancelling class b1 m = -(1 - b1) g sc
    (1 + 1e-3 N(0, 1))."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * n + int(sc * 4096))
    cls = classes(n)
    p = torch.randn(n, generator=gen, dtype=F64)
    g = torch.randn(n, generator=gen, dtype=F64) * 3
    m = torch.randn(n, generator=gen, dtype=F64) * 0.1
    v = torch.rand(n, generator=gen, dtype=F64) * 0.1
    r1, r2, r3 = (torch.rand(n, generator=gen, dtype=F64) + 0.5 for _ in range(3))
    s1, s2 = (torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double() for _ in range(2))
    noise = torch.randn(n, generator=gen, dtype=F64)
    b1 = f32v(BETA1)
    first, gz, pad, ed, cn = (cls == c for c in (FIRST, GZERO, PAD, EPSD, CANCEL))
    m[first], v[first] = 0.0, 0.0
    g[gz] = 0.0
    for t in (p, g, m, v):
        t[pad] = 0.0
    g[ed], m[ed], v[ed] = (s1 * 1e-9 * r1 / sc)[ed], (s2 * 1e-9 * r2)[ed], (1e-18 * r3)[ed]
    g32 = g.float().double()
    m[cn] = (-(1.0 - b1) / b1 * g32 * sc * (1.0 + 1e-3 * noise))[cn]
    return p.float(), g.float(), m.float(), v.float(), cls


def adamw_ref(p, g, m, v, lr, wd, step, sc=1.0, fault=None):
    """-> ({p, m, v}: float64 reference, {p, m, v}: bound per element); ``fault`` perturbs the reference only (the
    bounds are always the correct update's)"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    b1, b2, eps, wd_ = f32v(BETA1), f32v(BETA2), f32v(EPS), f32v(wd)
    lr_, bc1, bc2s = hyper_row(lr, step)
    ss = lr_ / bc1

    def update(scale, eps_, wd__, ss_, bc2s_):
        gs = g * scale
        m1 = b1 * m + (1.0 - b1) * gs
        v1 = b2 * v + (1.0 - b2) * gs * gs
        r = v1.sqrt() / bc2s_ + eps_
        upd = ss_ * m1 / r
        return p * (1.0 - lr_ * wd__) - upd, m1, v1, r, upd, gs

    p1, m1, v1, r, upd, gs = update(sc, eps, wd_, ss, bc2s)
    Em = 3 * U * ((b1 * m).abs() + ((1.0 - b1) * gs).abs())
    bound = dict(p=U * (3 * p.abs() + 9.5 * upd.abs()) + ss * Em / r, m=Em, v=5 * U * v1)
    if fault is not None:
        lr2, bc1_2, bc2s_2 = hyper_row(lr, step + 1)
        args = dict(no_eps=(sc, 0.0, wd_, ss, bc2s), half_wd=(sc, eps, 0.5 * wd_, ss, bc2s),
                    no_scale=(1.0, eps, wd_, ss, bc2s), step_plus_1=(sc, eps, wd_, lr2 / bc1_2, bc2s_2))[fault]
        p1, m1, v1 = update(*args)[:3]
    return dict(p=p1, m=m1, v=v1), bound


def adamw_f32(p, g, m, v, lr, wd, step, sc=1.0):
    """the kernel's statements in float32 on the CPU (no FMA contraction)"""
    f = np.float32
    lr_, bc1, bc2s = (f(x) for x in hyper_row(lr, step))
    b1, b2 = f(BETA1), f(BETA2)
    ss, decay = lr_ / bc1, f(1.0) - lr_ * f(wd)
    gk = g * float(f(sc))
    pk = p * float(decay)
    m1 = float(b1) * m + float(f(1.0) - b1) * gk
    v1 = float(b2) * v + float(f(1.0) - b2) * gk * gk
    den = v1.sqrt() / float(bc2s) + float(f(EPS))
    return dict(p=pk - float(ss) * (m1 / den), m=m1, v=v1)


def ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ sums
def signed(shape, gen, lo=0.25):
    """float64 values with magnitudes uniform on [lo, 1], one in four negative: signed, with a mean, and no term near
    zero, so that a dropped row moves every column by at least ``lo``"""
    mag = lo + (1.0 - lo) * torch.rand(*shape, generator=gen, dtype=F64)
    return torch.where(torch.rand(*shape, generator=gen) < 0.25, -mag, mag)


def fold_inputs(P, n, seed, dtype=F32):
    """(part [P, n] of ``dtype``, prior [n] f32) on the CPU"""
    gen = torch.Generator().manual_seed(104729 * seed + 31 * P + n)
    return signed((P, n), gen).to(dtype), (signed((n,), gen, 0.5) * 3).float()


def fold_ref(part, alpha, prior, d, drop=None):
    """-> (float64 alpha sum_p part[p] (+ prior), bound); ``drop`` leaves one row out of the reference (never the bound)"""
    part = part.double()
    S = part.abs().sum(0)
    s = part.sum(0) - (part[drop] if drop is not None else 0.0)
    a = f32v(alpha)
    pr = prior.double() if prior is not None else torch.zeros_like(s)
    return a * s + pr, (d + 2) * U * (abs(a) * S + pr.abs())


def takes_wide(P, n, out_aligned=True):
    """sv_reduce_partials_pair / _multi: the wide arm (reduce_partials_kernel's body)"""
    return P <= 64 and n >= 65536 and n % 4 == 0 and out_aligned


def pair_cols(P, n_a, n_b=0):
    """sv_reduce_partials_pair: the column width of reduce_pair_kernel<cols / 4> -- the widest that still gives 512
    workgroups, starting at 256 (P <= 4), 128 (P <= 8) or 64"""
    cols = 256 if P <= 4 else (128 if P <= 8 else 64)
    while cols > 4 and cdiv(n_a, cols) + cdiv(n_b, cols) < 512:
        cols >>= 1
    return cols


def wide_depth(P):
    return max(P - 1, 0)


def pair_depth(P, cols):
    PG = KTHREADS // (cols // 4)
    F = min(PG, 16)
    return max(min(P - 1, (cdiv(P, PG) - 1) + (PG // F - 1) + (F - 1)), 0)


def pair_f32(part, cols):
    """reduce_pair_kernel<cols / 4>'s order of additions in float32 on the CPU: [P, n] -> [n]"""
    P, n = part.shape
    PG = KTHREADS // (cols // 4)
    F = min(PG, 16)
    T = cdiv(P, PG)
    x = torch.cat([part, torch.zeros(T * PG - P, n)]).view(T, PG, n)
    acc = torch.zeros(PG, n)
    for t in range(T):
        acc = acc + x[t]
    acc = acc.view(PG // F, F, n)
    s = torch.zeros(F, n)
    for k in range(PG // F):
        s = s + acc[k]
    t = s[0]
    for k in range(1, F):
        t = t + s[k]
    return t


def wide_f32(part):
    """reduce_partials_kernel's order (rows in order) in float32 on the CPU; bf16 rows widen first"""
    acc = torch.zeros(part.shape[1])
    for p in range(part.shape[0]):
        acc = acc + part[p].float()
    return acc


def finish_f32(s, alpha, prior):
    s = s * float(np.float32(alpha))
    return s + prior if prior is not None else s


def colsum_geometry(rows):
    """(rows per workgroup, partial rows) of sv_colsum"""
    rpb = max(cdiv(rows, 512), 1)
    return rpb, cdiv(rows, rpb)


def colsum_parts(x, rows):
    """[rows, C] float64 -> (the partials [nparts, C], their sums of absolute values)"""
    rpb, nparts = colsum_geometry(rows)
    C = x.shape[1]
    xp = torch.cat([x, torch.zeros(nparts * rpb - rows, C, dtype=F64)]).view(nparts, rpb, C)
    return xp.sum(1), xp.abs().sum(1)


# ------------------------------------------------------------------------------------------------ squared norm
def sq_geometry(n):
    """(workgroups = partials, laps of the float4 loop) of sv_sqnorm_partial"""
    grid = min(max(cdiv(n // 4, KTHREADS), 1), 1024)
    return grid, cdiv(n // 4, grid * KTHREADS)


def sq_depth(n):
    grid, laps = sq_geometry(n)
    return 3 + laps + 1 + 10 + cdiv(grid, KTHREADS) + 10


def clip_ref(g, max_norm, drop_block=None):
    """-> (norm, coef, relative bound of the norm, of the coefficient) in float64 from the f32 gradient;
    ``drop_block`` leaves one workgroup's partial out of the reference"""
    n = g.numel()
    sq = g.double() ** 2
    total = float(sq.sum())
    if drop_block is not None:
        grid, laps = sq_geometry(n)
        n4 = n // 4
        idx = torch.arange(n4)
        own = ((idx % (grid * KTHREADS)) // KTHREADS) == drop_block
        total -= float(sq[: n4 * 4].view(n4, 4)[own].sum())
        if drop_block == 0:
            total -= float(sq[n4 * 4:].sum())
    norm = math.sqrt(max(total, 0.0))
    coef = min(1.0, f32v(max_norm) / (norm + f32v(1e-6)))
    bn = ((sq_depth(n) + 1) / 2 + 1) * U
    return norm, coef, bn, bn + 2 * U


def clip_f32(g, max_norm):
    """sqnorm_kernel + clip_coef_kernel in float32 on the CPU: the float4's squares in order, a thread's laps in order,
    the tail element, then float32 sums over the block and over the partials"""
    f = np.float32
    n = g.numel()
    grid, laps = sq_geometry(n)
    n4 = n // 4
    q = g * g
    q4 = q[: n4 * 4].view(n4, 4)
    s4 = ((q4[:, 0] + q4[:, 1]) + q4[:, 2]) + q4[:, 3]
    x = torch.cat([s4, torch.zeros(laps * grid * KTHREADS - n4)]).view(laps, grid * KTHREADS)
    acc = torch.zeros(grid * KTHREADS)
    for lap in range(laps):
        acc = acc + x[lap]
    tail = q[n4 * 4:]
    acc[: tail.numel()] = acc[: tail.numel()] + tail
    part = acc.view(grid, KTHREADS).sum(1)
    pp = torch.cat([part, torch.zeros(cdiv(grid, KTHREADS) * KTHREADS - grid)]).view(-1, KTHREADS)
    a2 = torch.zeros(KTHREADS)
    for k in range(pp.shape[0]):
        a2 = a2 + pp[k]
    norm = np.sqrt(f(a2.sum().item()), dtype=f)
    coef = f(max_norm) / (norm + f(1e-6))
    return float(norm), float(min(coef, f(1.0)))


def clip_gradient(n, seed=0):
    gen = torch.Generator().manual_seed(15485863 * seed + n)
    return (torch.randn(n, generator=gen, dtype=F64) * 3).float()


def one_hot_positions(n):
    """position 0, n - 1, the first tail element, the first element of the second lap and the last of the first"""
    return sorted({i for i in (0, n - 1, 4 * (n // 4), SQ_LAP, SQ_LAP - 1) if 0 <= i < n})


# ------------------------------------------------------------------------------------------------ cast
def cast_specials():
    """f32 values at the edges of the bf16 conversion"""
    e = lambda k: 2.0 ** k  # noqa: E731
    fmax = float(np.finfo(np.float32).max)
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan,
            1.0 + e(-8), 1.0 + 3 * e(-8), -(1.0 + e(-8)), -(1.0 + 3 * e(-8)),  # exact ties: to even, down and up
            1.0 + e(-8) + e(-23), 1.0 + e(-8) - e(-23) / 2,  # one f32 step to either side of a tie
            fmax, -fmax, 3.3895313892515355e38,  # the largest finite f32 (rounds to inf); the largest finite bf16
            e(-126), e(-127), e(-130), e(-133), -e(-133),  # the smallest normal; bf16 subnormals
            e(-134), 3 * e(-134), -3 * e(-134), e(-134) + e(-149), e(-140), e(-149), -e(-149)]  # f32 subnormals, ties
    return torch.tensor(vals, dtype=F64).float()


def cast_input(n, seed=0):
    """random f32 values over many binades with the specials at both ends and around the lap boundaries"""
    gen = torch.Generator().manual_seed(32452843 * seed + n)
    x = (torch.randn(n, generator=gen, dtype=F64) * torch.exp2(torch.randint(-30, 30, (n,), generator=gen).double())).float()
    sp = cast_specials()
    k = sp.numel()
    for at in (0, CAST_LAP - k // 2, 2 * CAST_LAP - k // 2, n - k):
        if 0 <= at and at + k <= n:
            x[at: at + k] = sp
    return x
