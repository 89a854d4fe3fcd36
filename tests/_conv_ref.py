"""Float64 CPU references, operands, bounds and the host-side arm arithmetic for tests/test_resnet_calls_gpu.py.  Test
infrastructure only.

A shape is ``(B, H, W, Cs, Cout, k, stride, pad)`` (+ ``Cin`` for the stem, whose stored channels Cs exceed its real
ones).  Operands are drawn on the CPU in float64 and rounded to the compute dtype (bf16, or f32 for the parity mode), so
the float64 reference and the kernel see the same numbers.  Every reference is ``F.conv2d`` / ``conv_transpose2d`` /
conv2d's autograd in float64 on the CPU; ``S`` is the same operation over the operands' absolute values."""
import functools
import math

import torch
import torch.nn.functional as F

U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _round(t, mode):
    return t.to(BF if mode == "bf16" else F32).to(F64)


def _seed(shape, mode, tag):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(shape)) + 104729 * len(tag) + sum(map(ord, tag + mode))


@functools.lru_cache(maxsize=None)
def operands(shape, mode="bf16"):
    """x [B,H,W,Cs] (every stored channel non-zero: the padded ones must not reach any output), w [Cout,Cin,k,k],
    dy [B,OH,OW,Cout], all float64 holding values of the compute dtype; NHWC like the kernels' tensors."""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    g = torch.Generator().manual_seed(_seed(shape, mode, "ops"))
    OH, OW = out_hw(H, W, k, stride, pad)
    x = _round(torch.rand(B, H, W, Cs, generator=g, dtype=F64) * 2 - 1, mode)
    w = _round(torch.randn(Cout, Cin, k, k, generator=g, dtype=F64) * (k * k * Cin) ** -0.5, mode)
    dy = _round(torch.rand(B, OH, OW, Cout, generator=g, dtype=F64) * 2 - 1, mode)
    return x, w, dy


def packed(w, Cs):
    """torch weight [Cout,Cin,k,k] -> the packed layout [Cout][k*k][Cs], stored channels >= Cin zero"""
    Cout, Cin, k, _ = w.shape
    wp = torch.zeros(Cout, k * k, Cs, dtype=w.dtype)
    wp[:, :, :Cin] = w.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin)
    return wp


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_ref(shape, mode="bf16"):
    """(y, S) [B,OH,OW,Cout] float64"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    x, w, _ = operands(shape, mode)
    xc = _nchw(x[..., :Cin])
    return (_nhwc(F.conv2d(xc, w, stride=stride, padding=pad)),
            _nhwc(F.conv2d(xc.abs(), w.abs(), stride=stride, padding=pad)))


@functools.lru_cache(maxsize=None)
def dgrad_ref(shape, mode="bf16"):
    """(dx, S) [B,H,W,Cs] float64: the transposed convolution of dy, with the output padding that restores H x W"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    assert Cin == Cs
    _, w, dy = operands(shape, mode)
    OH, OW = out_hw(H, W, k, stride, pad)
    op = (H - ((OH - 1) * stride - 2 * pad + k), W - ((OW - 1) * stride - 2 * pad + k))
    d = _nchw(dy)
    return (_nhwc(F.conv_transpose2d(d, w, stride=stride, padding=pad, output_padding=op)),
            _nhwc(F.conv_transpose2d(d.abs(), w.abs(), stride=stride, padding=pad, output_padding=op)))


def _wgrad(x, dy, shape):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    wz = torch.zeros(Cout, Cin, k, k, dtype=F64, requires_grad=True)
    y = F.conv2d(_nchw(x[..., :Cin]), wz, stride=stride, padding=pad)
    return torch.autograd.grad(y, wz, _nchw(dy))[0]


@functools.lru_cache(maxsize=None)
def wgrad_ref(shape, mode="bf16"):
    """(dw, S) [Cout,Cin,k,k] float64 from conv2d's autograd"""
    x, _, dy = operands(shape, mode)
    return _wgrad(x, dy, shape), _wgrad(x.abs(), dy.abs(), shape)


@functools.lru_cache(maxsize=None)
def prior(shape, which, dtype_name):
    """a non-zero prior for an accumulating output, values of ``dtype_name`` ("bf16" / "f32") in float64"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    g = torch.Generator().manual_seed(_seed(shape, dtype_name, "prior" + which))
    dims = (B, H, W, Cs) if which == "dx" else (Cout, Cin, k, k)
    t = torch.rand(*dims, generator=g, dtype=F64) * 4 - 2
    return t.to(BF if dtype_name == "bf16" else F32).to(F64)


@functools.lru_cache(maxsize=None)
def bn_operands(shape):
    """the BatchNorm + ReLU that produced the conv's input, for conv_bwd_data_bn: its input y [B,H,W,Cs] (bf16 values),
    mean / rstd / gamma / beta [Cs] (f32 values), all float64.  Drawn so that the mask's argument
    beta + gamma rstd (y - mean) is spread over about +-3 with both signs well populated."""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    g = torch.Generator().manual_seed(_seed(shape, "bf16", "bn"))
    y = (torch.randn(B, H, W, Cs, generator=g, dtype=F64) * 1.5 + 0.25).to(BF).to(F64)
    mean = (torch.randn(Cs, generator=g, dtype=F64) * 0.3 + 0.25).float().double()
    rstd = (torch.rand(Cs, generator=g, dtype=F64) * 0.5 + 0.5).float().double()
    gamma = ((torch.rand(Cs, generator=g, dtype=F64) + 0.5) * torch.where(torch.rand(Cs, generator=g) < 0.25, -1.0, 1.0)
             ).float().double()
    beta = (torch.randn(Cs, generator=g, dtype=F64) * 0.4).float().double()
    return y, mean, rstd, gamma, beta


def bn_mask(shape):
    """(mask [B,H,W,Cs] bool, unsure [B,H,W,Cs] bool, xhat float64): ``unsure`` marks the elements whose argument
    beta + gamma rstd (y - mean) lies within f32 rounding of zero (the kernel evaluates fmaf(f32(gamma rstd), y - mean,
    beta): three roundings, each at most 2^-24 of the larger of the two addends), whose mask float64 cannot decide."""
    y, mean, rstd, gamma, beta = bn_operands(shape)
    t = gamma * rstd * (y - mean)
    arg = beta + t
    unsure = arg.abs() <= 4 * U24 * (beta.abs() + t.abs())
    return arg > 0, unsure, (y - mean) * rstd


def group_sums(v, rows_per_group=64):
    """[M, C] float64 -> [ceil(M/64), C]: sums over runs of 64 rows (the last one short)"""
    M, C = v.shape
    P = cdiv(M, rows_per_group)
    pad = torch.zeros(P * rows_per_group - M, C, dtype=v.dtype)
    return torch.cat([v, pad]).view(P, rows_per_group, C).sum(1)


def class_rows(t, cls):
    """NHWC [B,H,W,C] (even H, W) -> the rows [B*H/2*W/2, C] of output parity class cls = 2 py + px, in the order
    (b, gy, gx) of the one-launch stride-2 data gradient"""
    py, px = cls >> 1, cls & 1
    return t[:, py::2, px::2, :].reshape(-1, t.shape[-1])


# ------------------------------------------------------------------------------------------- host schedule, restated
def is_pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def wgrad_transposed(shape):
    """csrc/conv.hip wgrad_transposed: the transposed product (mode 4) when it wastes fewer MFMA rows than mode 3"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    tc = k * k * Cs
    e3 = Cout / (256.0 * cdiv(Cout, 256)) * tc / (128.0 * cdiv(tc, 128))
    e4 = tc / (256.0 * cdiv(tc, 256)) * Cout / (128.0 * cdiv(Cout, 128))
    return e4 > 1.1 * e3


def wgrad_split3(shape):
    """csrc/conv.hip wgrad_split3: slices of the gathered weight gradients (modes 3 / 4)"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    OH, OW = out_hw(H, W, k, stride, pad)
    K, tc = B * OH * OW, k * k * Cs
    maxs = max(K // 512, 1)
    if wgrad_transposed(shape):
        tiles = cdiv(tc, 256) * cdiv(Cout, 128)
        lo, hi = cdiv(256 * 3 // 4, tiles), cdiv(256, tiles)
        split = min(max(K // 2048, lo), hi, maxs)
    else:
        split = min(cdiv(512, cdiv(Cout, 256) * cdiv(tc, 128)), maxs)
    return max(1, min(split, 256))


def wgrad_split(shape):
    """csrc/conv.hip wgrad_split: slices of the register-staged weight gradient (128 x 128 tiles)"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    OH, OW = out_hw(H, W, k, stride, pad)
    K = B * OH * OW
    split = min(cdiv(768, cdiv(Cout, 128) * cdiv(k * k * Cs, 128)), max(K // 256, 1), 256)
    return max(split, 1)


def wgrad_work_floats(shape):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    return max(wgrad_split(shape), wgrad_split3(shape)) * Cout * k * k * Cs


def wgrad_arm(shape, mode="bf16"):
    """-> (arm, slices, kper, output tiles): which of sv_conv_bwd_weight's three kernels runs, restated from its
    conditions (the pointwise arm, linear_wgrad, is decided by kernels._pointwise before)"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    OH, OW = out_hw(H, W, k, stride, pad)
    npix, tc = B * OH * OW, k * k * Cs
    if mode == "bf16" and Cs >= 8 and is_pow2(Cs) and npix % 32 == 0 and Cout % 8 == 0:
        sp = wgrad_split3(shape)
        kper = cdiv(cdiv(npix, sp), 32) * 32
        if wgrad_transposed(shape):
            return "mode4", sp, kper, cdiv(tc, 256) * cdiv(Cout, 128)
        return "mode3", sp, kper, cdiv(Cout, 256) * cdiv(tc, 128)
    sp = wgrad_split(shape)
    return "staged", sp, cdiv(cdiv(npix, sp), 32) * 32, cdiv(Cout, 128) * cdiv(tc, 128)


def split_kper(K, split):
    """gemm3.hip launch(): the k range of one slice"""
    return cdiv(cdiv(K, split), 32) * 32


# --------------------------------------------------------------------------------------------------------- bounds
def acc_bound(S, n, mode="bf16", split=1, kper=None):
    """the accumulation term: n 2^-24 S for an f32 sum of n exact bf16 products in any order; (kper + split) 2^-24 S
    for split-K (the slab sums and the fold bounded separately); (n + 1) 2^-24 S in fp32 mode, whose products round"""
    if mode != "bf16":
        return (n + 1) * U24 * S if split == 1 else (kper + 1 + split) * U24 * S
    return n * U24 * S if split == 1 else (kper + split) * U24 * S


def store_bound(ref, dtype, prior_=None, term=None):
    """2^-8 |ref| for a bf16 store, 2^-23 |ref| for an f32 one; accumulating forms: the f32 term on the addends,
    2^-23 (|prior| + |term|), plus the bf16 store of the sum where dx is bf16"""
    if prior_ is None:
        return (U8 if dtype == BF else U23) * ref.abs()
    b = U23 * (prior_.abs() + term.abs())
    return b + U8 * ref.abs() if dtype == BF else b


def kstep_rms(a, b):
    """the RMS contribution of one 32-deep k-step to an output element: sqrt(32) rms(a) rms(b)"""
    return math.sqrt(32.0) * float(a.pow(2).mean().sqrt()) * float(b.pow(2).mean().sqrt())


def sensitive_share(bound, a, b):
    """share of the elements whose 2 x bound lies below one k-step's RMS contribution"""
    return float((2.0 * bound < kstep_rms(a, b)).double().mean())
