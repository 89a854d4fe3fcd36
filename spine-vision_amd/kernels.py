"""Typed host-side launch helpers over the C ABI (``include/sv_kernels.h``).

Every helper takes/returns torch device tensors, validates shapes on the host *before* launching
(the kernels assume the grid/shape contract checked here), allocates outputs and workspaces from
PyTorch's caching allocator and enqueues on the current stream.  There is no fallback path: a
missing library or a CPU tensor raises.
"""

from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import native as nv
from .native import SV_BF16, SV_F32, call, dt, ptr, value

EPS_LN = 1e-6


class GemmProbe:
    """Times every launch of one GEMM class with HIP events on the launching stream (bench.py's live
    roofline measurement).  key = (a_kmajor, b_kmajor, compute_bf16) or, to single out one epilogue
    kind, (a_kmajor, b_kmajor, compute_bf16, epilogue).  ``bytes`` counts the ALGORITHMIC HBM bytes
    of the launch: operands read once (A, B, the epilogue operand) and the REQUIRED outputs written
    once -- for a split-K weight gradient that is the N x K f32 gradient, not the self-chosen slabs."""

    def __init__(self, key: tuple, name: str = "") -> None:
        self.key = key
        self.name = name
        self.events: list[tuple[torch.cuda.Event, torch.cuda.Event]] = []
        self.flops = 0.0
        self.bytes = 0.0
        self.launches = 0
        # per launch: the fraction of the chip's CUs its grid is sized for (256x256 tiles x split-K slices, capped
        # by the policy's grid cap), so a class that runs on part of the chip by design can be read against the
        # peak of the CUs it was given (bench.py: frac_of_granted_cus)
        self.shares: list[float] = []

    def matches(self, a_kmajor: bool, b_kmajor: bool, bf: bool, epilogue: int) -> bool:
        k = (bool(a_kmajor), bool(b_kmajor), bool(bf))
        return self.key[:3] == k and (len(self.key) < 4 or self.key[3] == epilogue)

    def elapsed_ms(self) -> float:
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


PROBES: list[GemmProbe] = []


class OpProbe:
    """Times every launch of one HBM-bound kernel (depthwise conv fwd / bwd-data / wgrad, LayerNorm
    backward, AdamW) with HIP events on the launching stream; ``bytes`` are the kernel's ALGORITHMIC HBM
    bytes (every operand read once, every required output written once; partial sums it chooses to
    write for a later fold are not counted)."""

    def __init__(self, name: str) -> None:
        self.name = name
        self.events: list = []
        self.flops = 0.0
        self.bytes = 0.0
        self.fma = 0.0  # f32 VALU FMAs (the depthwise convolutions: 49 per output element)
        self.launches = 0

    def elapsed_ms(self) -> float:
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


OP_PROBES: dict[str, OpProbe] = {}  # name -> probe; bench.py fills it for the timed step it probes


# SV_DIAG_SKIP=fold,...: skip every launch of those probe classes (an upper bound on what removing them could buy;
# the step's results are wrong -- never for training or tests)
_DIAG_SKIP = {x for x in os.environ.get("SV_DIAG_SKIP", "").split(",") if x}


def _fin(name: str, *args) -> None:
    """call() of a BatchNorm fold / activation launch; SV_DIAG_SKIP=bn_fin / bn_act skips those (diagnostic only)"""
    if _DIAG_SKIP and not name.endswith("_fold") and ("bn_act" if name == "sv_bn_act_fwd" else "bn_fin") in _DIAG_SKIP:
        return
    call(name, *args)


def _timed_call(op: str, nbytes: float, *args, fma: float = 0.0, flops: float = 0.0) -> None:
    """call(*args), bracketed by HIP events on the current stream when ``op`` is being probed; ``fma``: the
    launch's algorithmic f32 VALU FMAs (its roof when they outlast its bytes)."""
    if _DIAG_SKIP and op in _DIAG_SKIP:  # diagnostic timing only: the launch is skipped, its results are garbage
        return
    pr = OP_PROBES.get(op)
    if pr is None:
        call(*args)
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    call(*args)
    ev1.record()
    pr.events.append((ev0, ev1))
    pr.bytes += nbytes
    pr.fma += fma
    pr.flops += flops
    pr.launches += 1


_CUS: dict = {}


def _device_cus(device) -> int:
    n = _CUS.get(device)
    if n is None:
        n = _CUS[device] = torch.cuda.get_device_properties(device).multi_processor_count
    return n


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _cdt(compute_bf16: bool) -> int:
    return SV_BF16 if compute_bf16 else SV_F32


# ----------------------------------------------------------------------------------------------
# GEMM
def gemm(
    A: torch.Tensor,
    B: torch.Tensor,
    *,
    M: int,
    N: int,
    K: int,
    a_kmajor: bool,
    b_kmajor: bool,
    lda: int,
    ldb: int,
    epilogue: int = nv.SV_EPI_STORE,
    C: torch.Tensor | None = None,
    C2: torch.Tensor | None = None,
    ldc: int | None = None,
    bias: torch.Tensor | None = None,
    gamma: torch.Tensor | None = None,
    aux: torch.Tensor | None = None,
    ld_aux: int | None = None,
    a_scale_k: torch.Tensor | None = None,
    split_k: int = 1,
    compute_bf16: bool = True,
    bn: "nv.BnRef | None" = None,
    policy: "nv.GemmPolicy | None" = None,
    fold: tuple | None = None,
) -> torch.Tensor:
    """C = epilogue(A(m,k) . B(k,n)); see sv_gemm in include/sv_kernels.h for the layouts.  ``policy``: the
    launch policy of this call (nv.policy(...): kernel family, grid cap, residency, priority); None = defaults."""
    _check(C is not None, "gemm: output tensor C is required")
    need_a = (M - 1) * lda + K if a_kmajor else (K - 1) * lda + M
    need_b = (N - 1) * ldb + K if b_kmajor else (K - 1) * ldb + N
    _check(A.numel() >= need_a, f"gemm: A too small ({A.numel()} < {need_a})")
    _check(B.numel() >= need_b, f"gemm: B too small ({B.numel()} < {need_b})")
    if epilogue == nv.SV_EPI_SLAB:
        _check(C.dtype in (torch.float32, torch.bfloat16) and C.numel() >= split_k * M * N, "gemm: slab too small")
    else:
        ldc = N if ldc is None else ldc
        _check(C.numel() >= (M - 1) * ldc + N, "gemm: C too small")
    if bias is not None:
        _check(bias.numel() >= N and bias.dtype == torch.float32, "gemm: bad bias")
    d = nv.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.a_dtype, d.a_kmajor, d.lda = ptr(A), dt(A), int(a_kmajor), lda
    d.B, d.b_dtype, d.b_kmajor, d.ldb = ptr(B), dt(B), int(b_kmajor), ldb
    d.a_scale_k = ptr(a_scale_k)
    d.epilogue = epilogue
    d.C, d.c_dtype, d.ldc = ptr(C), dt(C), ldc if ldc is not None else N
    if C2 is not None:
        d.C2, d.c2_dtype = ptr(C2), dt(C2)
    d.bias = ptr(bias)
    d.gamma = ptr(gamma)
    if aux is not None:
        d.aux, d.aux_dtype, d.ld_aux = ptr(aux), dt(aux), ld_aux if ld_aux is not None else N
    d.split_k = split_k
    d.compute = _cdt(compute_bf16)
    if bn is not None:
        d.bn = ctypes.pointer(bn)
    if policy is not None:
        d.policy = policy
    if fold is not None:  # (out, accumulate, counters): the split-K fold inside the GEMM (SV_EPI_SLAB)
        fo, facc, fcnt = fold
        d.fold_out, d.fold_ld, d.fold_accumulate, d.fold_counters = ptr(fo), N, int(bool(facc)), ptr(fcnt)
    probes = [p_ for p_ in PROBES if p_.matches(a_kmajor, b_kmajor, compute_bf16, epilogue)]
    if probes:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("sv_gemm", ctypes.byref(d))
        ev1.record()
        nbytes = M * K * A.element_size() + N * K * B.element_size()
        if epilogue == nv.SV_EPI_SLAB:
            nbytes += M * N * 4  # the weight gradient itself (the split-K slabs are a design choice)
            if C2 is not None:
                nbytes += M * 4  # its bias gradient (column sums)
        elif epilogue == nv.SV_EPI_BIAS_GELU_DUAL:
            nbytes += M * N * C2.element_size()  # GELU(h) is required; the GELU'(h) store is a design choice
        elif epilogue == nv.SV_EPI_LN_BWD:
            nbytes += M * N * C.element_size() + M * 8 + C2.numel() * 4  # dz; mean / rstd; the weight / bias partials
        else:
            nbytes += M * N * C.element_size()
            if C2 is not None:
                nbytes += M * N * C2.element_size()
        if aux is not None:
            nbytes += M * N * aux.element_size()
        cus = _device_cus(C.device)
        cap = policy.grid_cap if policy is not None and policy.grid_cap > 0 else cus
        share = min(-(-M // 256) * -(-N // 256) * max(split_k, 1), cap, cus) / cus
        for p_ in probes:
            p_.events.append((ev0, ev1))
            p_.shares.append(share)
            p_.flops += 2.0 * M * N * K
            p_.bytes += nbytes
            p_.launches += 1
    else:
        call("sv_gemm", ctypes.byref(d))
    return C


# the LayerNorm backward in the fc1 data gradient's epilogue (SV_EPI_LN_BWD, round 6): dy never reaches HBM.  v9 only,
# N % 256 == 0 (ConvNeXt C = 512 / 1024), every 256x256 tile resident at once (else the two-pass form runs).
# SV_FUSED_LN_BWD=0 keeps the two passes (A/B runs)
FUSED_LN_BWD = os.environ.get("SV_FUSED_LN_BWD", "1") != "0"
_LN_XCH: dict = {}


def linear_dgrad_ln(dh2d, w, z2d, mean, rstd, lnw, *, dw, db, policy=None):
    """dz = LayerNorm backward of dy = bf16(dh2d @ w) over (z2d, mean, rstd, lnw) in ONE launch (sv_gemm,
    SV_EPI_LN_BWD); -> (dz bf16 [M, C], finish) as layernorm_bwd(..., defer_reduce=True) returns, or None where the
    shape or the chip's free CUs do not take the fused form (the caller then runs linear_dgrad + layernorm_bwd)."""
    if not FUSED_LN_BWD:
        return None
    M, K = dh2d.shape
    C = w.shape[1]
    if C % 256 or C > 1024 or dh2d.dtype != torch.bfloat16 or z2d.dtype != torch.bfloat16:
        return None
    _check(tuple(z2d.shape) == (M, C) and z2d.is_contiguous() and mean.numel() == M and rstd.numel() == M
           and lnw.numel() == C, "linear_dgrad_ln: z [M, C], mean / rstd [M], lnw [C]")
    tilesM, tilesN = -(-M // 256), C // 256
    if tilesM * tilesN > _device_cus(dh2d.device):
        return None
    dz = torch.empty(M, C, device=dh2d.device, dtype=torch.bfloat16)
    P = -(-M // 128)
    part = torch.empty(2, P, C, device=dh2d.device, dtype=torch.float32)
    key = (dh2d.device, nv._stream())
    xch = _LN_XCH.get(key)
    if xch is None or xch.numel() < tilesM * tilesN * 512:
        xch = _LN_XCH[key] = torch.empty(max(tilesM * tilesN * 512, 1 << 18), device=dh2d.device, dtype=torch.float32)
    bn = nv.BnRef(ptr(mean), ptr(rstd), ptr(lnw), None)
    try:
        linear_dgrad(dh2d, w, out=dz, epilogue=nv.SV_EPI_LN_BWD, out2=part, aux=z2d, ld_aux=C, bn=bn, policy=policy,
                     fold=(xch, False, _fold_counters(dh2d.device, tilesM)))
    except RuntimeError as err:
        if "(status 2)" in str(err):  # SV_ERR_UNSUPPORTED: not every tile resident at once (CU mask, grid cap)
            return None
        raise
    return dz, _ln_partials_finish(part, P, dw, db)


# The three operand layouts of the host paths; nothing else in this file names a layout (the conv paths and
# linear_dgrad_ln pass their split / second output / BatchNorm / fold operands through these).
def linear_fwd(x2d, w, *, out, bias=None, epilogue=nv.SV_EPI_STORE, out2=None, gamma=None, residual=None,
               compute_bf16=True, policy=None, split_k=1):
    """out[M,N] = epilogue(x2d[M,K] @ w[N,K]^T)  (torch Linear weight layout)."""
    M, K = x2d.shape
    N = w.shape[0]
    return gemm(x2d, w, M=M, N=N, K=K, a_kmajor=True, b_kmajor=True, lda=K, ldb=K, epilogue=epilogue, C=out,
                C2=out2, bias=bias, gamma=gamma, aux=residual, split_k=split_k, compute_bf16=compute_bf16,
                policy=policy)


def linear_dgrad(dy2d, w, *, out, epilogue=nv.SV_EPI_STORE, a_scale_k=None, aux=None, compute_bf16=True, policy=None,
                 split_k=1, out2=None, bn=None, gamma=None, ld_aux=None, fold=None):
    """out[M,K] = epilogue((dy2d[M,N] * a_scale_k[N]) @ w[N,K])."""
    M, N = dy2d.shape
    K = w.shape[1]
    return gemm(dy2d, w, M=M, N=K, K=N, a_kmajor=True, b_kmajor=False, lda=N, ldb=K, epilogue=epilogue, C=out,
                C2=out2, gamma=gamma, a_scale_k=a_scale_k, aux=aux, ld_aux=ld_aux, split_k=split_k,
                compute_bf16=compute_bf16, bn=bn, policy=policy, fold=fold)


def _wgrad_slabs(dy2d, x2d, K, split, *, bf16_slabs=False, cs=None, fold=None, compute_bf16=True, policy=None):
    """The split-K slabs of G[N,K] = dy2d[M,N]^T x2d[M,:K] (SV_EPI_SLAB), f32 or -- ``bf16_slabs`` -- bf16;
    ``cs``: receives the column sums of dy2d per slice; ``fold`` = (out, accumulate): the in-kernel fold's target."""
    M, N = dy2d.shape
    slab = torch.empty(split * N * K, device=dy2d.device, dtype=torch.bfloat16 if bf16_slabs else torch.float32)
    if fold is not None:
        fold = (*fold, _fold_counters(dy2d.device, -(-N // 256) * -(-K // 256)))
    gemm(dy2d, x2d, M=N, N=K, K=M, a_kmajor=False, b_kmajor=False, lda=N, ldb=x2d.shape[1], epilogue=nv.SV_EPI_SLAB,
         C=slab, C2=cs, split_k=split, compute_bf16=compute_bf16, policy=policy, fold=fold)
    return slab


# channel counts the fused MLP forward kernel (csrc/mlp.hip) is built for: ConvNeXt-base S1 / S2, ConvNeXt-large S1
MLP_FUSED_C = (128, 192, 256, 512)


def mlp_fwd(y, w1, b1, w2, b2, gamma, x, *, out, gelu_grad=None, gelu_out=None):
    """Fused ConvNeXt MLP forward (sv_mlp_fwd): out = gamma (.) (GELU(y w1^T + b1) w2^T + b2) + x in one kernel,
    the 4C-wide hidden activation kept on chip; ``gelu_grad`` / ``gelu_out`` ([M, 4C] bf16, both or neither) receive
    GELU'(h) / GELU(h) for the backward (training).  Bit for bit the two-GEMM path (linear_fwd GELU dual, then the
    gamma-residual epilogue)."""
    M, C = y.shape
    H = 4 * C
    _check(C in MLP_FUSED_C, f"mlp_fwd: C = {C} not supported {MLP_FUSED_C}")
    _check(y.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16,
           "mlp_fwd: y / w1 / w2 must be bf16")
    _check(tuple(w1.shape) == (H, C) and tuple(w2.shape) == (C, H), "mlp_fwd: weight shapes")
    for t_, n_ in ((b1, H), (b2, C), (gamma, C)):
        _check(t_.dtype == torch.float32 and t_.numel() == n_ and t_.is_contiguous(), "mlp_fwd: bias / gamma")
    _check(x.dtype == torch.float32 and out.dtype == torch.float32 and x.numel() == M * C and out.numel() == M * C,
           "mlp_fwd: x / out must be f32 [M, C]")
    _check(out.data_ptr() != x.data_ptr(), "mlp_fwd: out must not alias x")
    _check((gelu_grad is None) == (gelu_out is None), "mlp_fwd: gelu_grad and gelu_out go together")
    ts = [y, w1, b1, w2, b2, gamma, x, out]
    if gelu_grad is not None:
        for t_ in (gelu_grad, gelu_out):
            _check(t_.dtype == torch.bfloat16 and t_.numel() == M * H, "mlp_fwd: GELU outputs must be bf16 [M, 4C]")
        ts += [gelu_grad, gelu_out]
    _check(all(t_.is_contiguous() and t_.data_ptr() % 16 == 0 for t_ in ts), "mlp_fwd: contiguous 16-B aligned tensors")
    _check(M * H * 2 < 2**31, "mlp_fwd: hidden tensor must be < 2 GiB")
    # algorithmic: y, x read; out written; both weights once; the GELU pair written in training
    nb = M * C * (2 + 4 + 4) + 2 * H * C * 2 + (2 * M * H * 2 if gelu_grad is not None else 0)
    _timed_call("mlp_fused", nb, "sv_mlp_fwd", ptr(y), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(gamma), ptr(x), ptr(out),
                ptr(gelu_grad), ptr(gelu_out), M, C, flops=4.0 * M * C * H)
    return out


def transpose_scale_bf16(W: torch.Tensor, scale: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """bf16(W * scale[:, None])^T for a 2-D f32 weight [R, C] -> [C, R] bf16 (the operand images of mlp_bwd)."""
    R_, C_ = W.shape
    _check(W.dtype == torch.float32 and W.is_contiguous(), "transpose_scale_bf16: need contiguous f32")
    _check(scale is None or (scale.numel() == R_ and scale.dtype == torch.float32), "transpose_scale_bf16: bad scale")
    if out is None:
        out = torch.empty(C_, R_, device=W.device, dtype=torch.bfloat16)
    _check(tuple(out.shape) == (C_, R_) and out.dtype == torch.bfloat16 and out.is_contiguous(),
           "transpose_scale_bf16: bad out")
    call("sv_transpose_scale_bf16", ptr(W), ptr(scale), ptr(out), R_, C_)
    return out


MLP_BWD_FUSED_C = (128,)


def mlp_bwd(d, w2t, gelu_grad, w1t, z, mean, rstd, lnw, *, dh, dz):
    """Fused backward of fc2 (x GELU') -> fc1 -> LayerNorm of a ConvNeXt block at C = 128 (sv_mlp_bwd): dh (bf16
    [M, 4C], bit for bit linear_dgrad(d, W2 gamma, x GELU')), dz (bf16 [M, C], the LayerNorm backward of bf16(dh W1)).
    Returns the LayerNorm weight / bias partial sums (ln_part [2][P][C] f32) and P, to fold into dw / db."""
    M, C = d.shape
    H = 4 * C
    _check(C in MLP_BWD_FUSED_C, f"mlp_bwd: C = {C} not supported {MLP_BWD_FUSED_C}")
    for t_, shp in ((d, (M, C)), (w2t, (H, C)), (gelu_grad, (M, H)), (w1t, (C, H)), (z, (M, C)), (dh, (M, H)),
                    (dz, (M, C))):
        _check(t_.dtype == torch.bfloat16 and t_.numel() == shp[0] * shp[1] and t_.is_contiguous(),
               f"mlp_bwd: bf16 [{shp[0]}, {shp[1]}] operand expected")
    for t_, n_ in ((mean, M), (rstd, M), (lnw, C)):
        _check(t_.dtype == torch.float32 and t_.numel() == n_ and t_.is_contiguous(), "mlp_bwd: f32 vector")
    P = value("sv_mlp_bwd_nparts", M, C)
    part = torch.empty(2, P, C, device=d.device, dtype=torch.float32)
    ts = [d, w2t, gelu_grad, w1t, z, mean, rstd, lnw, dh, dz, part]
    _check(all(t_.data_ptr() % 16 == 0 for t_ in ts), "mlp_bwd: 16-B aligned tensors")
    _check(M * H * 2 < 2**31, "mlp_bwd: hidden tensor must be < 2 GiB")
    # algorithmic: d, GELU'(h), z read; dh, dz written; both weights, mean / rstd once
    nb = M * (C * 2 + H * 2 + C * 2 + H * 2 + C * 2 + 8) + 2 * H * C * 2
    _timed_call("mlp_bwd_fused", nb, "sv_mlp_bwd", ptr(d), ptr(w2t), ptr(gelu_grad), ptr(w1t), ptr(z), ptr(mean),
                ptr(rstd), ptr(lnw), ptr(dh), ptr(dz), ptr(part), M, C, flops=4.0 * M * C * H)
    return part, P


_WGRAD_TARGET = 512  # workgroups per split-K wgrad launch (2 per CU)
# persistent 256x256 wgrads: tiles x split ~ this many workgroups (SV_WGRAD9_WGS for A/B runs).  Half the chip
# (128): the side-stream weight gradients share it with the main stream's data gradients anyway, and half the
# split depth halves the f32 slabs written and folded -- round 4 on the final kernels: 1072.6-1075.6 vs
# 1065.7-1067.9 img/s interleaved, fold 4.0 -> 2.5 ms/step (profiles/round4/r7f_fold_ab.txt; round 3 had
# measured 128 and 256 equal)
_WGRAD9_TARGET = int(os.environ.get("SV_WGRAD9_WGS", "128"))
# ...but the whole chip for long weight gradients: ConvNeXt-large bs64's (309 GFLOP each) on half the chip made the
# side stream the long pole (590 vs 598 img/s at 256, profiles/round4/r9c_large_wgrad_target.txt)
_WGRAD9_LONG_GFLOP = float(os.environ.get("SV_WGRAD9_LONG_GFLOP", "150"))


def _wgrad_split(tiles: int, K: int) -> int:
    """K slices so that tiles*split ~ 512 workgroups (2 per CU), each slice >= 16 k-steps."""
    split = max(1, -(-_WGRAD_TARGET // max(tiles, 1)))
    return max(1, min(split, K // 512 if K >= 512 else 1))


def _wgrad_split_for(N: int, K: int, M: int, target: int | None = None) -> int:
    """Split-K factor of a weight gradient G[N,K] = dY[M,N]^T X[M,K].  Outputs of at least 128 x 256 run
    on the persistent 256x256 kernel (gemm9.hip; a 128-row output half-fills its tiles and still beats
    the 256x128 kernel): one tile per CU (tiles * split ~ 256 CUs) with every K slice a whole number of
    64-deep K-tiles; smaller ones on the 256x128 kernel (~512 workgroups)."""
    if min(N, K) >= 128 and max(N, K) >= 256:
        tiles9 = -(-N // 256) * -(-K // 256)
        target = (target or _WGRAD9_TARGET) if 2.0 * M * N * K <= _WGRAD9_LONG_GFLOP * 1e9 else 256
        # the slice count whose grid is nearest the target, among those that cut M into whole 64-row K-tiles and
        # keep one workgroup per CU (rounding down alone left ConvNeXt-large's S3 wgrads, 36 tiles, at split 2:
        # 72 workgroups, 47 % longer launches, the large bs64 step 16 % slower, profiles/round4/r9b_configs/)
        ok = [s_ for s_ in range(1, max(2, 2 * target // tiles9 + 1)) if M % (s_ * 64) == 0 and tiles9 * s_ <= 256]
        if ok:
            return min(ok, key=lambda s_: (abs(tiles9 * s_ - target), s_))
    return _wgrad_split(-(-N // 128) * -(-K // 128), M)


# In-kernel split-K fold of the weight gradients (gemm9.hip, sv_gemm_desc.fold_out), where the separate fold would
# take sv_reduce_partials' sequential wide body (bitwise the same result).  The kernel spreads each tile's fold over
# the tile's own slices when the grid allows it (every slice resident: one unit per workgroup, at most half the
# CUs), else the last workgroup to finish a slice sums the tile.  Opt-in (SV_INKERNEL_FOLD=1), both forms measured
# slower in the step: the last-arriver form 1009-1051 vs 1066-1068 img/s (r7f_fold_ab.txt: one CU streams the
# tile), the spread form 1037-1039 vs 1056-1057 (r8j_spread_fold_ab.txt: the fold passes drop 2.4 -> 1.7 ms/step
# but each wgrad launch grows 170 -> 195 us in-step, its slices waiting on one another beside the main stream)
_INKERNEL_FOLD = os.environ.get("SV_INKERNEL_FOLD", "0") != "0"
_FOLD_MAX_SPLIT = int(os.environ.get("SV_FOLD_MAX_SPLIT", "64"))
_FOLD_COUNTERS: dict = {}


def _fold_counters(device, tiles: int) -> torch.Tensor:
    """Zeroed int32 counters (arrivals, departures) per tile for in-kernel folds on the current stream (the kernel
    leaves them zero)."""
    key = (device, nv._stream())
    t = _FOLD_COUNTERS.get(key)
    if t is None or t.numel() < 2 * tiles:
        t = _FOLD_COUNTERS[key] = torch.zeros(max(2 * tiles, 4096), device=device, dtype=torch.int32)
    return t


# bf16 split-K slabs for the v9 weight gradients: each slice's f32 partial rounded to bf16 once (the reference's
# autocast rounds the whole weight gradient to bf16 once), summed in f32 in slice order by the fold -- half the slab
# bytes written and read.  ConvNeXt-base bs32 +1.5 % (1091-1098 vs 1077-1079 img/s interleaved), its B=32 parity
# against the fp32 oracle unchanged (worst gradient 7.89e-3 vs 7.9e-3; profiles/round4/r9zh_bf16_slabs_ab.txt).
# SV_WGRAD_BF16_SLABS=0: f32 slabs.  Only the default / v9 kernel family (policy.impl 0 or 9) takes them.
_WGRAD_BF16_SLABS = os.environ.get("SV_WGRAD_BF16_SLABS", "1") != "0"


def _bf16_slabs(N: int, K: int, M: int, split: int, compute_bf16: bool, policy=None) -> bool:
    """the v9 weight-gradient shapes (whole 64-row K-tiles per slice: _wgrad_split_for's v9 branch)"""
    return (_WGRAD_BF16_SLABS and compute_bf16 and split > 1 and min(N, K) >= 128 and max(N, K) >= 256
            and K % 8 == 0 and M % (split * 64) == 0 and (policy is None or policy.impl in (0, 9)))


def _fold_ok(split: int, n: int, out: torch.Tensor, compute_bf16: bool) -> bool:
    return (_INKERNEL_FOLD and compute_bf16 and 1 < split <= _FOLD_MAX_SPLIT and n >= 65536 and n % 4 == 0
            and out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() % 16 == 0)


def linear_wgrad(dy2d, x2d, *, out=None, accumulate=False, bias_out=None, bias_accumulate=True,
                 compute_bf16=True, cols=None, defer: list | None = None, policy=None,
                 wgrad_target: int | None = None) -> torch.Tensor:
    """G[N,K] = dy2d[M,N]^T @ x2d[M,K] in f32 (split-K over M into slabs, then one reduce pass that
    writes -- or, with ``accumulate``, adds -- into ``out``).  With ``bias_out`` the column sums of
    dy2d (the bias gradient) come out of the same GEMM (SV_EPI_SLAB colsum).  ``cols``: use only the
    first ``cols`` columns of x2d (the stem's 48 of its 64-wide padded patch rows).  ``defer`` (a list, with
    ``out`` given): append the slab folds to it for one ``reduce_multi`` launch instead of reducing here."""
    M, N = dy2d.shape
    K = x2d.shape[1] if cols is None else cols
    split = _wgrad_split_for(N, K, M, wgrad_target)
    cs = torch.empty(split * N, device=dy2d.device, dtype=torch.float32) if bias_out is not None else None
    # the form: bf16 slabs, else the in-kernel fold, else f32 slabs
    bf16 = (out is not None and _bf16_slabs(N, K, M, split, compute_bf16, policy) and out.is_contiguous()
            and out.numel() == N * K)
    infold = not bf16 and out is not None and _fold_ok(split, N * K, out, compute_bf16)
    if infold:
        _check(out.numel() == N * K, "linear_wgrad: bad out")
    slab = _wgrad_slabs(dy2d, x2d, K, split, bf16_slabs=bf16, cs=cs, fold=(out, accumulate) if infold else None,
                        compute_bf16=compute_bf16, policy=policy)
    if bf16:
        _timed_call("fold", 2.0 * split * N * K + 4.0 * N * K * (1 + int(bool(accumulate))), "sv_reduce_partials_bf16",
                    ptr(slab), split, N * K, ptr(out), 1.0, int(bool(accumulate)))
    if bf16 or infold:
        _colsum_finish(cs, split, bias_out, bias_accumulate, defer)
        return out
    if out is None:
        if split == 1 and not accumulate:
            _colsum_finish(cs, split, bias_out, bias_accumulate, None)
            return slab.view(N, K)
        out = torch.empty(N, K, device=dy2d.device, dtype=torch.float32)
        accumulate = False
    _check(out.numel() == N * K and out.is_contiguous(), "linear_wgrad: bad out")
    if defer is not None:
        defer.append((slab, out, split, accumulate))
        _colsum_finish(cs, split, bias_out, bias_accumulate, defer)
    elif cs is not None and bias_accumulate == accumulate:
        reduce_pair(slab, out, cs, bias_out, split, accumulate=accumulate)
    else:
        _colsum_finish(cs, split, bias_out, bias_accumulate, None)
        reduce_into(slab, split, out, accumulate)
    return out


def _colsum_finish(cs, split, bias_out, accumulate, defer) -> None:
    """The bias gradient from the wgrad GEMM's column-sum partials (none: nothing): folded here, or by the caller's
    ``defer`` list."""
    if cs is None:
        return
    if defer is not None:
        defer.append((cs, bias_out, split, accumulate))
    else:
        reduce_into(cs, split, bias_out, accumulate=accumulate)


def layerscale_wgrad(dsrc2d, a2d, w2, gamma, b2, *, dw2, dgamma, db2, compute_bf16=True, policy=None,
                     wgrad_target: int | None = None):
    """fc2 weight / bias / layer-scale gradients of out = x + gamma * (a W2^T + b2) from d_out:
    dW2 += gamma (.) d^T a, dgamma += rowdot(W2, d^T a) + b2 (.) colsum(d), db2 += gamma (.) colsum(d).
    The wgrad GEMM writes split-K slabs (+ colsum partials); ONE fused pass (a workgroup per row)
    reduces them and applies the layer-scale finish (sv_layerscale_wgrad_reduce) -- G = d^T a is
    never materialised."""
    M, C = dsrc2d.shape
    K4 = a2d.shape[1]
    split = _wgrad_split_for(C, K4, M, wgrad_target)
    cs = torch.empty(split * C, device=dsrc2d.device, dtype=torch.float32)
    bf16 = _bf16_slabs(C, K4, M, split, compute_bf16, policy)
    # G = d^T a folded inside the wgrad GEMM (opt-in); the finish then reads one G instead of `split` slabs
    G = None if bf16 else torch.empty(C * K4, device=dsrc2d.device, dtype=torch.float32)
    infold = not bf16 and _fold_ok(split, C * K4, G, compute_bf16)
    slab = _wgrad_slabs(dsrc2d, a2d, K4, split, bf16_slabs=bf16, cs=cs, fold=(G, False) if infold else None,
                        compute_bf16=compute_bf16, policy=policy)
    rest = (ptr(cs), split, ptr(w2), ptr(gamma), ptr(b2), ptr(dw2), ptr(dgamma), ptr(db2))
    if bf16:
        _timed_call("fold", 2.0 * split * C * K4 + 8.0 * C * K4 + 4.0 * (split + 4) * C,
                    "sv_layerscale_wgrad_reduce_bf16", ptr(slab), *rest, C, K4)
    elif infold:
        _timed_call("fold", 4.0 * (3 * C * K4 + (split + 4) * C), "sv_layerscale_wgrad_fold_finish", ptr(G), *rest,
                    C, K4)
    else:
        _timed_call("fold", 4.0 * ((split + 2) * C * K4 + (split + 4) * C), "sv_layerscale_wgrad_reduce", ptr(slab),
                    *rest, None, C, K4)


# ----------------------------------------------------------------------------------------------
# reductions
def reduce_into(part: torch.Tensor, nparts: int, out: torch.Tensor, accumulate: bool = True, alpha: float = 1.0):
    """out (+)= alpha * sum of nparts partial rows -- one launch for any depth (sv_reduce_partials_pair)."""
    reduce_pair(part, out, None, None, nparts, accumulate=accumulate, alpha=alpha)


def reduce_pair(part_a: torch.Tensor, out_a: torch.Tensor, part_b: torch.Tensor | None, out_b: torch.Tensor | None,
                nparts: int, accumulate: bool = True, alpha: float = 1.0):
    """Two independent partial reductions with the same depth in ONE launch (weight + bias gradients)."""
    na = out_a.numel()
    _check(part_a.numel() >= nparts * na, "reduce_pair: partial buffer a too small")
    _check(out_a.dtype == torch.float32 and out_a.is_contiguous(), "reduce_pair: out must be contiguous f32")
    nb = 0
    if out_b is not None:
        nb = out_b.numel()
        _check(part_b is not None and part_b.numel() >= nparts * nb, "reduce_pair: partial buffer b too small")
        _check(out_b.dtype == torch.float32 and out_b.is_contiguous(), "reduce_pair: out must be contiguous f32")
    moved = 4.0 * (na + nb) * (nparts + 1 + int(bool(accumulate)))  # slabs read, out written (+ read)
    _timed_call("fold", moved, "sv_reduce_partials_pair", ptr(part_a), na, ptr(out_a), ptr(part_b), nb, ptr(out_b),
                nparts, float(alpha), int(accumulate))


def reduce_multi(segs: list, alpha: float = 1.0) -> None:
    """Independent partial reductions out (+)= alpha * sum_p part[p] in one launch per SV_MAX_RED_SEGS
    segments (sv_reduce_partials_multi).  segs: (part, out, P, accumulate) tuples, f32 contiguous."""
    for i in range(0, len(segs), nv.SV_MAX_RED_SEGS):
        chunk = segs[i:i + nv.SV_MAX_RED_SEGS]
        arr = (nv.RedSeg * len(chunk))()
        moved = 0.0
        for j, (part, out, P, acc) in enumerate(chunk):
            n = out.numel()
            _check(out.dtype == torch.float32 and out.is_contiguous() and part.numel() >= P * n,
                   "reduce_multi: bad segment")
            arr[j] = nv.RedSeg(ptr(part), ptr(out), n, int(P), int(bool(acc)))
            moved += 4.0 * n * (P + 1 + int(bool(acc)))
        _timed_call("fold", moved, "sv_reduce_partials_multi", arr, len(chunk), float(alpha))


def _ln_partials_finish(part: torch.Tensor, P: int, dw: torch.Tensor, db: torch.Tensor):
    """finish(record, defer) of a LayerNorm backward's weight / bias partials ``part`` [2][P * C]: folds them into
    dw / db on whatever stream is current when it is called (layernorm_bwd(defer_reduce=True), linear_dgrad_ln)."""
    def finish(record: bool = True, defer: list | None = None):
        if record:  # the caller may instead keep the partials alive until the streams have joined
            part.record_stream(torch.cuda.current_stream())
        if defer is not None:  # folded by the caller's reduce_multi launch
            defer += [(part[0], dw, P, True), (part[1], db, P, True)]
            return
        reduce_pair(part[0], dw, part[1], db, P)
    return finish


def colsum_into(x2d: torch.Tensor, out: torch.Tensor, accumulate: bool = True):
    rows, C = x2d.shape
    P = value("sv_colsum_nparts", rows, C)
    part = torch.empty(P * C, device=x2d.device, dtype=torch.float32)
    call("sv_colsum", ptr(x2d), dt(x2d), rows, C, ptr(part))
    reduce_into(part, P, out, accumulate)


def colsum(x2d: torch.Tensor) -> torch.Tensor:
    out = torch.empty(x2d.shape[1], device=x2d.device, dtype=torch.float32)
    colsum_into(x2d, out, accumulate=False)
    return out


# ----------------------------------------------------------------------------------------------
# LayerNorm
def layernorm_fwd(x2d, w, b, *, out_dtype, eps=EPS_LN):
    rows, C = x2d.shape
    y = torch.empty(rows, C, device=x2d.device, dtype=out_dtype)
    mean = torch.empty(rows, device=x2d.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("sv_layernorm_fwd", ptr(x2d), dt(x2d), ptr(w), ptr(b), ptr(y), dt(y), ptr(mean), ptr(rstd), rows, C, eps)
    return y, mean, rstd


def layernorm_bwd(dy2d, x2d, mean, rstd, w, *, dw, db, dx=None, accumulate_dx=False, out_dtype=torch.float32,
                  defer_reduce=False):
    """dx (+)= LayerNorm backward; dw/db (+)= the weight/bias gradient through per-block partials.
    ``defer_reduce``: return ``(dx, finish)`` instead, ``finish()`` folding the partials into dw/db on
    whatever stream is current when it is called (the ConvNeXt backward runs it on the weight-gradient
    side stream, off the data-gradient chain)."""
    rows, C = x2d.shape
    _check(tuple(dy2d.shape) == (rows, C) and dy2d.is_contiguous(), "layernorm_bwd: dy must be contiguous [rows,C]")
    if dx is None:
        dx = torch.empty(rows, C, device=x2d.device, dtype=out_dtype)
    P = value("sv_layernorm_bwd_nparts", rows, C)
    pw = torch.empty(2, P * C, device=x2d.device, dtype=torch.float32)
    # algorithmic: dy, x read; dx written (read too when accumulating); mean / rstd read
    nb = rows * C * (dy2d.element_size() + x2d.element_size() + dx.element_size() * (2 if accumulate_dx else 1)) + rows * 8
    _timed_call("ln_bwd", nb, "sv_layernorm_bwd", ptr(dy2d), dt(dy2d), ptr(x2d), dt(x2d), ptr(mean), ptr(rstd), ptr(w),
                ptr(dx), dt(dx), int(accumulate_dx), ptr(pw[0]), ptr(pw[1]), rows, C)
    if defer_reduce:
        return dx, _ln_partials_finish(pw, P, dw, db)
    if dw is not None and db is not None:
        reduce_pair(pw[0], dw, pw[1], db, P)
    elif dw is not None:
        reduce_into(pw[0], P, dw)
    elif db is not None:
        reduce_into(pw[1], P, db)
    return dx


# ----------------------------------------------------------------------------------------------
# Multi-head self-attention (ViT / DeiT-III, csrc/attn.hip; above 256 tokens csrc/attn_stream.hip)
# SV_ATTN=torch: the same maths as torch ops on views of the same buffers (A/B and parity arm, in the style of
# SV_GCONV=dense): matmul -> f32 softmax -> bf16 -> matmul, and an explicit backward from the same formulas (no
# autograd).  The two products that feed f32 maths (q k^T and dout v^T) take f32 copies of the bf16 operands, so they
# are summed in f32 like the kernel's accumulators; the three that consume the bf16 P / dS are bf16 matmuls.  f32 operands (precision="fp32") always take this arm, in f32 throughout: attention is the one part of
# the fp32 parity mode that does not run on this library.
ATTN_TORCH = os.environ.get("SV_ATTN", "") == "torch"
ATTN_HEAD_DIM = 64
ATTN_MAX_N = 256  # sv_attn_fwd / sv_attn_bwd: every key of a head in one pass
ATTN_STREAM_MAX_N = 2048  # sv_attn_stream_fwd / sv_attn_stream_bwd


def _attn_geometry(who: str, qkv, B: int, N: int, heads: int, img_rows) -> tuple[int, int]:
    rows = N if img_rows is None else int(img_rows)
    C = heads * ATTN_HEAD_DIM
    _check(B > 0 and heads > 0 and 1 <= N <= rows, f"{who}: need B, heads > 0 and 1 <= N <= img_rows")
    _check(qkv.dim() == 2 and tuple(qkv.shape) == (B * rows, 3 * C) and qkv.is_contiguous()
           and qkv.dtype in (torch.bfloat16, torch.float32),
           f"{who}: qkv must be contiguous bf16 / f32 [{B * rows}, {3 * C}], got {tuple(qkv.shape)} {qkv.dtype}")
    return rows, C


def _attn_views(t2d, B: int, rows: int, N: int, heads: int, parts: int):
    """[B * rows, parts * heads * 64] -> `parts` views [B, heads, N, 64] (no copy)."""
    v = t2d.view(B, rows, parts, heads, ATTN_HEAD_DIM)[:, :N].permute(2, 0, 3, 1, 4)
    return tuple(v[i] for i in range(parts))


def _attn_torch_arm(qkv) -> bool:
    return ATTN_TORCH or qkv.dtype == torch.float32


def attn_fwd(qkv, B: int, N: int, heads: int, *, img_rows: int | None = None, scale: float | None = None,
             out: torch.Tensor | None = None, lse: torch.Tensor | None = None, torch_arm: bool | None = None,
             _who: str = "attn_fwd", _max_n: int = ATTN_MAX_N):
    """(out [B * img_rows, heads * 64], lse f32 [B, heads, N]) = softmax(q k^T * scale) v per (image, head) of
    qkv [B * img_rows, 3 * heads * 64] (columns (q|k|v, head, d); an image's first N rows are its tokens, the other
    rows padding: not read, zero in ``out``).  bf16 operands run sv_attn_fwd unless ``torch_arm`` (default: the
    SV_ATTN=torch switch); f32 operands always run the torch arm in f32."""
    rows, C = _attn_geometry(_who, qkv, B, N, heads, img_rows)
    scale = ATTN_HEAD_DIM ** -0.5 if scale is None else float(scale)
    if out is None:
        out = torch.empty(B * rows, C, device=qkv.device, dtype=qkv.dtype)
    if lse is None:
        lse = torch.empty(B, heads, N, device=qkv.device, dtype=torch.float32)
    _check(tuple(out.shape) == (B * rows, C) and out.is_contiguous() and out.dtype == qkv.dtype, f"{_who}: bad out")
    _check(tuple(lse.shape) == (B, heads, N) and lse.is_contiguous() and lse.dtype == torch.float32, f"{_who}: bad lse")
    if _attn_torch_arm(qkv) if torch_arm is None else (torch_arm or qkv.dtype == torch.float32):
        q, k, v = _attn_views(qkv, B, rows, N, heads, 3)
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
        torch.logsumexp(s, dim=-1, out=lse)
        p = torch.exp(s - lse.unsqueeze(-1)).to(qkv.dtype)
        o = out.view(B, rows, heads, ATTN_HEAD_DIM)
        o[:, :N] = torch.matmul(p, v).permute(0, 2, 1, 3)
        if rows > N:
            o[:, N:] = 0
        return out, lse
    _check(N <= _max_n, f"{_who}: N = {N} tokens (at most {_max_n})")
    call("sv_" + _who, ptr(qkv), ptr(out), ptr(lse), B, N, rows, heads, ATTN_HEAD_DIM, scale)
    return out, lse


def attn_stream_fwd(qkv, B: int, N: int, heads: int, *, img_rows: int | None = None, scale: float | None = None,
                    out: torch.Tensor | None = None, lse: torch.Tensor | None = None, torch_arm: bool | None = None):
    """``attn_fwd`` for N up to ATTN_STREAM_MAX_N: bf16 operands run sv_attn_stream_fwd (K and V streamed through LDS
    in tiles, online softmax); the torch arm is attn_fwd's, which takes any N."""
    return attn_fwd(qkv, B, N, heads, img_rows=img_rows, scale=scale, out=out, lse=lse, torch_arm=torch_arm,
                    _who="attn_stream_fwd", _max_n=ATTN_STREAM_MAX_N)


def attn_bwd(qkv, out, lse, dout, B: int, N: int, heads: int, *, img_rows: int | None = None,
             scale: float | None = None, dqkv: torch.Tensor | None = None, torch_arm: bool | None = None,
             _who: str = "attn_bwd", _max_n: int = ATTN_MAX_N):
    """dqkv [B * img_rows, 3 * heads * 64] from dout [B * img_rows, heads * 64]: P recomputed from ``lse``,
    D = rowsum(dout . out), dv = P^T dout, dS = P (dout v^T - D) scale, dq = dS k, dk = dS^T q (pad rows zero)."""
    rows, C = _attn_geometry(_who, qkv, B, N, heads, img_rows)
    scale = ATTN_HEAD_DIM ** -0.5 if scale is None else float(scale)
    for name, t_ in (("out", out), ("dout", dout)):
        _check(tuple(t_.shape) == (B * rows, C) and t_.is_contiguous() and t_.dtype == qkv.dtype, f"{_who}: bad {name}")
    _check(tuple(lse.shape) == (B, heads, N) and lse.is_contiguous() and lse.dtype == torch.float32, f"{_who}: bad lse")
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    _check(dqkv.shape == qkv.shape and dqkv.is_contiguous() and dqkv.dtype == qkv.dtype, f"{_who}: bad dqkv")
    if _attn_torch_arm(qkv) if torch_arm is None else (torch_arm or qkv.dtype == torch.float32):
        q, k, v = _attn_views(qkv, B, rows, N, heads, 3)
        (o,), (do,) = _attn_views(out, B, rows, N, heads, 1), _attn_views(dout, B, rows, N, heads, 1)
        p = torch.exp(torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale - lse.unsqueeze(-1))
        dp = torch.matmul(do.float(), v.float().transpose(-1, -2))
        dsum = (do.float() * o.float()).sum(-1, keepdim=True)
        ds = (p * (dp - dsum) * scale).to(qkv.dtype)
        g = dqkv.view(B, rows, 3, heads, ATTN_HEAD_DIM)
        g[:, :N, 0] = torch.matmul(ds, k).permute(0, 2, 1, 3)
        g[:, :N, 1] = torch.matmul(ds.transpose(-1, -2), q).permute(0, 2, 1, 3)
        g[:, :N, 2] = torch.matmul(p.to(qkv.dtype).transpose(-1, -2), do).permute(0, 2, 1, 3)
        if rows > N:
            g[:, N:] = 0
        return dqkv
    _check(N <= _max_n, f"{_who}: N = {N} tokens (at most {_max_n})")
    if _who == "attn_bwd":
        call("sv_attn_bwd", ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), B, N, rows, heads, ATTN_HEAD_DIM, scale)
    else:  # the streaming pair: D = rowsum(dout . out) goes through a workspace the library does not allocate
        dws = torch.empty(B, heads, N, device=qkv.device, dtype=torch.float32)
        call("sv_attn_stream_bwd", ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), ptr(dws), B, N, rows, heads,
             ATTN_HEAD_DIM, scale)
    return dqkv


def attn_stream_bwd(qkv, out, lse, dout, B: int, N: int, heads: int, *, img_rows: int | None = None,
                    scale: float | None = None, dqkv: torch.Tensor | None = None, torch_arm: bool | None = None):
    """``attn_bwd`` for N up to ATTN_STREAM_MAX_N on sv_attn_stream_bwd (a D pre-pass, a dk / dv kernel and a dq
    kernel, no atomics); the torch arm is attn_bwd's."""
    return attn_bwd(qkv, out, lse, dout, B, N, heads, img_rows=img_rows, scale=scale, dqkv=dqkv, torch_arm=torch_arm,
                    _who="attn_stream_bwd", _max_n=ATTN_STREAM_MAX_N)


def patchify16(img, *, out_dtype, rows_per_img: int | None = None, row0: int = 0, out: torch.Tensor | None = None,
               mean=None, std=None) -> torch.Tensor:
    """The 16x16 patch rows of a batch as the patch-embedding GEMM's A operand (sv_patchify16): [B * rows_per_img, 768],
    k = (c, ky, kx) -- ``patch_embed.proj.weight.view(C, 768)`` is the B operand as stored; image b's patch p is row
    b * rows_per_img + row0 + p (default: the plain [B * P, 768] matrix).  ``img``: f32 [B,3,H,W] (normalised), uint8
    [B,H,W,3] (classification: ToTensor + Normalize in flight) or uint8 [B,H,W] (localization: also gray -> RGB).
    With ``rows_per_img`` larger than the patch count the other rows are zeros (a fresh buffer) or kept (``out``)."""
    if img.dtype == torch.uint8:
        _check(img.is_contiguous() and (img.dim() == 3 or (img.dim() == 4 and img.shape[-1] == 3)),
               "patchify16: uint8 input must be contiguous [B,H,W] or [B,H,W,3]")
        B, H, W = img.shape[:3]
        kind = nv.SV_IMG_U8_GRAY if img.dim() == 3 else nv.SV_IMG_U8_HWC
    else:
        _check(img.dim() == 4 and img.shape[1] == 3 and img.dtype == torch.float32 and img.is_contiguous(),
               "patchify16: expects contiguous f32 [B,3,H,W]")
        B, _, H, W = img.shape
        kind = nv.SV_IMG_F32_NCHW
    _check(H % 16 == 0 and W % 16 == 0 and H > 0 and W > 0, "patchify16: H, W must be multiples of 16")
    P = (H // 16) * (W // 16)
    rows = P if rows_per_img is None else int(rows_per_img)
    _check(row0 >= 0 and rows >= row0 + P, "patchify16: rows_per_img must hold row0 + the patch rows")
    if out is None:
        alloc = torch.empty if rows == P else torch.zeros
        out = alloc(B * rows, 768, device=img.device, dtype=out_dtype)
    _check(tuple(out.shape) == (B * rows, 768) and out.is_contiguous() and out.dtype == out_dtype, "patchify16: bad out")
    call("sv_patchify16", ptr(img), kind, _host3(IMAGENET_MEAN if mean is None else mean),
         _host3(IMAGENET_STD if std is None else std), ptr(out), dt(out), B, H, W, rows, row0)
    return out


def vit_tokens(pe: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int, P: int, rows_per_img: int,
               pos_has_cls: bool, out: torch.Tensor | None = None) -> torch.Tensor:
    """The token matrix [B * rows_per_img, C] f32 (sv_vit_tokens): per image row 0 the class token (+ pos[0] for ViT),
    rows 1..P the patch embeddings ``pe`` (same row layout) + their position embedding, the rest zero.  ``out``: the
    buffer to write (default: a fresh one)."""
    C = pe.shape[1]
    _check(tuple(pe.shape) == (B * rows_per_img, C) and pe.dtype == torch.float32 and pe.is_contiguous(),
           "vit_tokens: pe must be contiguous f32 [B * rows_per_img, C]")
    _check(cls.numel() == C and pos.numel() == (P + int(bool(pos_has_cls))) * C and cls.dtype == pos.dtype == torch.float32
           and cls.is_contiguous() and pos.is_contiguous(), "vit_tokens: bad cls / pos")
    x = torch.empty_like(pe) if out is None else out
    _check(x.shape == pe.shape and x.dtype == torch.float32 and x.is_contiguous(), "vit_tokens: bad out")
    call("sv_vit_tokens", ptr(pe), ptr(cls), ptr(pos), ptr(x), B, P, rows_per_img, C, int(bool(pos_has_cls)))
    return x


# ----------------------------------------------------------------------------------------------
# Swin: shifted-window attention with a relative-position bias, patch merging, stochastic depth (csrc/swin.hip)
# SV_WINATTN=torch: the same maths as torch ops on gathered windows (A/B and parity arm, as SV_ATTN=torch): the rows
# of every window gathered through an index, matmul -> f32 softmax -> bf16 -> matmul, an explicit backward from the
# same formulas and a scatter back.  f32 operands (precision="fp32") always take this arm, in f32 throughout.
WINATTN_TORCH = os.environ.get("SV_WINATTN", "") == "torch"
WIN_HEAD_DIM = 32
WIN_MAX = 8
WIN_MASKED = -100.0
_WIN_CACHE: dict = {}


def window_rows(B: int, H: int, W: int, w: int, shift: int, device) -> tuple[torch.Tensor, torch.Tensor | None]:
    """(rows int64 [B * nW * w*w], mask f32 [nW, w*w, w*w] or None): the raster row of token (i, j) of window
    (wy, wx) -- pixel ((wy w + i + shift) mod H, (wx w + j + shift) mod W) -- and timm's shifted-window mask (0 / -100
    by the region of the rolled coordinate; None when shift = 0).  Cached per geometry."""
    key = (B, H, W, w, shift, str(device))
    if key not in _WIN_CACHE:
        yr = torch.arange(H).view(H // w, 1, w, 1).expand(H // w, W // w, w, w)
        xr = torch.arange(W).view(1, W // w, 1, w).expand(H // w, W // w, w, w)
        rows = (((yr + shift) % H) * W + (xr + shift) % W).reshape(1, -1) + (torch.arange(B) * H * W).view(B, 1)
        mask = None
        if shift:
            def reg(v, L):
                return (v >= L - w).long() + (v >= L - shift).long()
            lab = (reg(yr, H) * 3 + reg(xr, W)).reshape(-1, w * w)
            mask = (lab[:, :, None] != lab[:, None, :]).float() * WIN_MASKED
            mask = mask.to(device)
        _WIN_CACHE[key] = (rows.reshape(-1).to(device), mask)
    return _WIN_CACHE[key]


def _win_geometry(who: str, qkv, B, H, W, w, shift, heads) -> tuple[int, int]:
    C = heads * WIN_HEAD_DIM
    _check(B > 0 and heads > 0 and 1 <= w <= WIN_MAX and 0 <= shift < w and H > 0 and W > 0 and H % w == 0
           and W % w == 0, f"{who}: need B, heads > 0, 1 <= w <= {WIN_MAX}, 0 <= shift < w and H, W multiples of w")
    _check(qkv.dim() == 2 and qkv.shape[0] >= B * H * W and qkv.shape[1] == 3 * C and qkv.is_contiguous()
           and qkv.dtype in (torch.bfloat16, torch.float32),
           f"{who}: qkv must be contiguous bf16 / f32 [>= {B * H * W}, {3 * C}], got {tuple(qkv.shape)} {qkv.dtype}")
    return qkv.shape[0], C


def _win_torch_arm(qkv, torch_arm) -> bool:
    return qkv.dtype == torch.float32 or (WINATTN_TORCH if torch_arm is None else bool(torch_arm))


def _win_scores(qkv, bias, B, H, W, w, shift, heads, scale):
    idx, mask = window_rows(B, H, W, w, shift, qkv.device)
    N = w * w
    x = qkv[idx].view(-1, N, 3, heads, WIN_HEAD_DIM).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale + bias.unsqueeze(0)
    if mask is not None:
        s = (s.view(B, -1, heads, N, N) + mask.view(1, -1, 1, N, N)).view(-1, heads, N, N)
    return idx, q, k, v, s


def swin_bias_expand(table: torch.Tensor, w: int) -> torch.Tensor:
    """timm's relative_position_bias_table [(2w-1)^2, heads] f32 -> the dense bias [heads, w*w, w*w] the window
    attention reads (sv_swin_bias_expand)."""
    heads = table.shape[1]
    _check(table.dim() == 2 and table.shape[0] == (2 * w - 1) ** 2 and table.dtype == torch.float32
           and table.is_contiguous(), f"swin_bias_expand: table must be contiguous f32 [{(2 * w - 1) ** 2}, heads]")
    dense = torch.empty(heads, w * w, w * w, device=table.device, dtype=torch.float32)
    call("sv_swin_bias_expand", ptr(table), ptr(dense), w, heads)
    return dense


def swin_bias_grad(part: torch.Tensor, dtable: torch.Tensor, w: int, accumulate: bool = True) -> torch.Tensor:
    """dtable [(2w-1)^2, heads] (+)= the partials [nparts, heads, w*w, w*w] of winattn_bwd folded in part order, then
    over each table entry's (i, j) pairs (sv_swin_bias_grad)."""
    nparts, heads = part.shape[0], part.shape[1]
    _check(part.dim() == 4 and tuple(part.shape[2:]) == (w * w, w * w) and part.dtype == torch.float32
           and part.is_contiguous(), "swin_bias_grad: part must be contiguous f32 [nparts, heads, w*w, w*w]")
    _check(tuple(dtable.shape) == ((2 * w - 1) ** 2, heads) and dtable.dtype == torch.float32 and dtable.is_contiguous(),
           "swin_bias_grad: bad dtable")
    call("sv_swin_bias_grad", ptr(part), ptr(dtable), nparts, w, heads, int(bool(accumulate)))
    return dtable


def winattn_fwd(qkv, bias, B: int, H: int, W: int, w: int, shift: int, heads: int, *, scale: float | None = None,
                torch_arm: bool | None = None):
    """(out [rows, heads * 32], lse f32 [B * nW, heads, w*w]) = softmax(scale q k^T + bias + mask) v per (window,
    head) of qkv [rows, 3 * heads * 32] (rows >= B*H*W in raster order; the rows beyond are not read and zero in
    ``out``).  bf16 operands run sv_winattn_fwd unless ``torch_arm`` (default: SV_WINATTN=torch); f32 operands always
    run the torch arm."""
    rows, C = _win_geometry("winattn_fwd", qkv, B, H, W, w, shift, heads)
    N = w * w
    scale = WIN_HEAD_DIM ** -0.5 if scale is None else float(scale)
    _check(tuple(bias.shape) == (heads, N, N) and bias.dtype == torch.float32 and bias.is_contiguous(),
           "winattn_fwd: bias must be contiguous f32 [heads, w*w, w*w]")
    nwin = B * (H // w) * (W // w)
    if _win_torch_arm(qkv, torch_arm):
        idx, q, k, v, s = _win_scores(qkv, bias, B, H, W, w, shift, heads, scale)
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.unsqueeze(-1)).to(qkv.dtype)
        out = torch.zeros(rows, C, device=qkv.device, dtype=qkv.dtype)
        out[idx] = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(-1, C)
        return out, lse
    out = torch.empty(rows, C, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(nwin, heads, N, device=qkv.device, dtype=torch.float32)
    call("sv_winattn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(bias), B, H, W, w, shift, heads, WIN_HEAD_DIM, scale, rows)
    return out, lse


def winattn_bwd(qkv, out, lse, dout, bias, B: int, H: int, W: int, w: int, shift: int, heads: int, *,
                scale: float | None = None, torch_arm: bool | None = None):
    """(dqkv, dbias_part [nparts, heads, w*w, w*w]) from dout: P recomputed from ``lse``, D = rowsum(dout . out),
    T = P (dout v^T - D), dv = P^T dout, dS = scale T, dq = dS k, dk = dS^T q; the bias gradient sum_windows T comes as
    per-wave partials for ``swin_bias_grad`` (one part on the torch arm)."""
    rows, C = _win_geometry("winattn_bwd", qkv, B, H, W, w, shift, heads)
    N = w * w
    scale = WIN_HEAD_DIM ** -0.5 if scale is None else float(scale)
    nwin = B * (H // w) * (W // w)
    for name, t_ in (("out", out), ("dout", dout)):
        _check(tuple(t_.shape) == (rows, C) and t_.is_contiguous() and t_.dtype == qkv.dtype, f"winattn_bwd: bad {name}")
    _check(tuple(lse.shape) == (nwin, heads, N) and lse.is_contiguous() and lse.dtype == torch.float32,
           "winattn_bwd: bad lse")
    _check(tuple(bias.shape) == (heads, N, N) and bias.dtype == torch.float32 and bias.is_contiguous(),
           "winattn_bwd: bad bias")
    if _win_torch_arm(qkv, torch_arm):
        idx, q, k, v, s = _win_scores(qkv, bias, B, H, W, w, shift, heads, scale)
        o = out[idx].view(-1, N, heads, WIN_HEAD_DIM).permute(0, 2, 1, 3)
        do = dout[idx].view(-1, N, heads, WIN_HEAD_DIM).permute(0, 2, 1, 3)
        p = torch.exp(s - lse.unsqueeze(-1))
        dp = torch.matmul(do.float(), v.float().transpose(-1, -2))
        t = p * (dp - (do.float() * o.float()).sum(-1, keepdim=True))
        ds = (t * scale).to(qkv.dtype)
        g = torch.stack([torch.matmul(ds, k), torch.matmul(ds.transpose(-1, -2), q),
                         torch.matmul(p.to(qkv.dtype).transpose(-1, -2), do)])  # [3, nwin, heads, N, 32]
        dqkv = torch.zeros_like(qkv)
        dqkv[idx] = g.permute(1, 3, 0, 2, 4).reshape(-1, 3 * C)
        return dqkv, t.sum(0, keepdim=True).contiguous()
    nparts = value("sv_winattn_bwd_nparts", B, H, W, w, heads)
    dqkv = torch.empty_like(qkv)
    part = torch.empty(nparts, heads, N, N, device=qkv.device, dtype=torch.float32)
    call("sv_winattn_bwd", ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(bias), ptr(dqkv), ptr(part), B, H, W, w, shift,
         heads, WIN_HEAD_DIM, scale, rows)
    return dqkv, part


def patch_merge(x2d: torch.Tensor, B: int, H: int, W: int, *, rows_out: int | None = None) -> torch.Tensor:
    """timm PatchMerging's gather (sv_patch_merge): [>= B*H*W, C] -> [rows_out >= B*(H/2)*(W/2), 4C], channel blocks
    (h0,w0), (h1,w0), (h0,w1), (h1,w1); rows beyond the merged ones are zeros."""
    C = x2d.shape[1]
    n = B * (H // 2) * (W // 2)
    rows_out = n if rows_out is None else int(rows_out)
    _check(x2d.dim() == 2 and x2d.shape[0] >= B * H * W and x2d.is_contiguous() and H % 2 == 0 and W % 2 == 0
           and rows_out >= n, "patch_merge: need contiguous [>= B*H*W, C], even H, W and rows_out >= B*H*W/4")
    y = torch.empty(rows_out, 4 * C, device=x2d.device, dtype=x2d.dtype)
    call("sv_patch_merge", ptr(x2d), ptr(y), dt(x2d), B, H, W, C, rows_out)
    return y


def patch_merge_bwd(dy2d: torch.Tensor, B: int, H: int, W: int, *, rows_in: int | None = None) -> torch.Tensor:
    """The inverse permutation of ``patch_merge`` (H, W: the unmerged grid): [>= B*H*W/4, 4C] -> [rows_in, C]."""
    C = dy2d.shape[1] // 4
    rows_in = B * H * W if rows_in is None else int(rows_in)
    _check(dy2d.dim() == 2 and dy2d.shape[1] == 4 * C and dy2d.shape[0] >= B * (H // 2) * (W // 2)
           and dy2d.is_contiguous() and H % 2 == 0 and W % 2 == 0 and rows_in >= B * H * W, "patch_merge_bwd: bad dy")
    dx = torch.empty(rows_in, C, device=dy2d.device, dtype=dy2d.dtype)
    call("sv_patch_merge_bwd", ptr(dy2d), ptr(dx), dt(dy2d), B, H, W, C, rows_in)
    return dx


def _rowscale_check(who: str, x, s, rows_per_img: int) -> None:
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] % 4 == 0
           and s.dim() == 1 and s.dtype == torch.float32 and s.is_contiguous() and rows_per_img > 0,
           f"{who}: need contiguous f32 [rows, C % 4 == 0] and an f32 scale vector [B]")


def rowscale_add(x: torch.Tensor, t: torch.Tensor, s: torch.Tensor, rows_per_img: int,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """x + s[row // rows_per_img] * t per row (sv_rowscale_add; stochastic depth's residual add).  Rows of a dropped
    sample (s = 0) and rows beyond the B images copy x."""
    _rowscale_check("rowscale_add", x, s, rows_per_img)
    _check(t.shape == x.shape and t.dtype == torch.float32 and t.is_contiguous(), "rowscale_add: bad t")
    out = torch.empty_like(x) if out is None else out
    call("sv_rowscale_add", ptr(x), ptr(t), ptr(s), ptr(out), x.shape[0], rows_per_img, s.shape[0], x.shape[1])
    return out


def rowscale_cast_bf16(d: torch.Tensor, s: torch.Tensor, rows_per_img: int) -> torch.Tensor:
    """bf16(s[row // rows_per_img] * d) per row (sv_rowscale_cast_bf16; the gradient entering a dropped branch)."""
    _rowscale_check("rowscale_cast_bf16", d, s, rows_per_img)
    out = torch.empty(d.shape, device=d.device, dtype=torch.bfloat16)
    call("sv_rowscale_cast_bf16", ptr(d), ptr(s), ptr(out), d.shape[0], rows_per_img, s.shape[0], d.shape[1])
    return out


# ----------------------------------------------------------------------------------------------
# Global Response Normalization (ConvNeXt V2, csrc/grn.hip)
EPS_GRN = 1e-6


def _grn_act(who: str, B: int, *ts) -> tuple[int, int]:
    """Checks of the [B*HW, n] activations of one GRN launch (same shape and dtype); returns (HW, n)."""
    t0 = ts[0]
    _check(t0.dim() == 2 and B > 0 and t0.shape[0] % B == 0 and t0.shape[0] > 0,
           f"{who}: activations must be [B*HW, n] with B={B} dividing the rows")
    _check(t0.shape[1] % 8 == 0, f"{who}: n={t0.shape[1]} must be a multiple of 8")
    _check(t0.dtype in (torch.float32, torch.bfloat16), f"{who}: activations must be f32 or bf16")
    for t in ts:
        _check(t.is_cuda and t.shape == t0.shape and t.dtype == t0.dtype and t.is_contiguous()
               and t.data_ptr() % 16 == 0,
               f"{who}: activations must be contiguous, 16-byte aligned device tensors of one shape and dtype")
    return t0.shape[0] // B, t0.shape[1]


def _grn_f32(who: str, numel: int, *ts) -> None:
    for t in ts:
        _check(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel
               and t.data_ptr() % 16 == 0, f"{who}: expected contiguous 16-byte aligned f32 tensors of {numel} elements")


def grn_nparts(HW: int, n: int) -> int:
    return value("sv_grn_nparts", HW, n)


def grn_stats(a2d: torch.Tensor, B: int) -> torch.Tensor:
    """Per-chunk sums of a^2: f32 partials [B, P, n], P = grn_nparts(HW, n)."""
    HW, n = _grn_act("grn_stats", B, a2d)
    part = torch.empty(B, grn_nparts(HW, n), n, device=a2d.device, dtype=torch.float32)
    _timed_call("grn_stats", float(a2d.numel() * a2d.element_size()), "sv_grn_stats", ptr(a2d), dt(a2d),
                ptr(part), B, HW, n)
    return part


def grn_finish(part: torch.Tensor, gamma: torch.Tensor, *, eps: float = EPS_GRN) -> tuple:
    """Folds the partials of grn_stats; returns (G, N, scale = 1 + gamma N) as [B, n] and D as [B], all f32."""
    _check(part.dim() == 3, "grn_finish: partials must be [B, P, n]")
    B, P, n = part.shape
    _grn_f32("grn_finish", B * P * n, part)
    _grn_f32("grn_finish", n, gamma)
    G, N, scale = (torch.empty(B, n, device=part.device, dtype=torch.float32) for _ in range(3))
    D = torch.empty(B, device=part.device, dtype=torch.float32)
    call("sv_grn_finish", ptr(part), P, ptr(gamma), ptr(G), ptr(N), ptr(scale), ptr(D), B, n, float(eps))
    return G, N, scale, D


def grn_apply(a2d: torch.Tensor, scale: torch.Tensor, beta: torch.Tensor, *, out: torch.Tensor | None = None):
    """u = a * scale[b, c] + beta[c] in a's dtype; ``out`` may be ``a2d`` itself (the eval forward keeps no a)."""
    B = scale.shape[0]
    if out is None:
        out = torch.empty_like(a2d)
    HW, n = _grn_act("grn_apply", B, a2d, out)
    _grn_f32("grn_apply", B * n, scale)
    _grn_f32("grn_apply", n, beta)
    _timed_call("grn_apply", 2.0 * a2d.numel() * a2d.element_size(), "sv_grn_apply", ptr(a2d), dt(a2d), ptr(scale),
                ptr(beta), ptr(out), B, HW, n)
    return out


def grn_fwd(a2d: torch.Tensor, B: int, gamma: torch.Tensor, beta: torch.Tensor, *, inplace: bool = False) -> tuple:
    """The three forward passes; returns (u, (G, N, scale, D))."""
    st = grn_finish(grn_stats(a2d, B), gamma)
    return grn_apply(a2d, st[2], beta, out=a2d if inplace else None), st


def grn_bwd_stats(du2d: torch.Tensor, a2d: torch.Tensor, B: int) -> tuple:
    """Per-chunk sums of du * a and of du: two f32 partial buffers [B, P, n]."""
    HW, n = _grn_act("grn_bwd_stats", B, du2d, a2d)
    P = grn_nparts(HW, n)
    sp = torch.empty(B, P, n, device=a2d.device, dtype=torch.float32)
    dp = torch.empty_like(sp)
    _timed_call("grn_bwd_stats", 2.0 * a2d.numel() * a2d.element_size(), "sv_grn_bwd_stats",
                ptr(du2d), ptr(a2d), dt(a2d), ptr(sp), ptr(dp), B, HW, n)
    return sp, dp


def grn_bwd_finish(sp: torch.Tensor, dp: torch.Tensor, gamma, G, N, D, *, dgamma, dbeta, accumulate: bool = True):
    """Folds the partials of grn_bwd_stats (their chunk 0 then holds the per-image totals S and sum du); returns
    k = dG / G [B, n] and writes / adds dgamma and dbeta."""
    _check(sp.dim() == 3 and dp.shape == sp.shape, "grn_bwd_finish: partials must be two [B, P, n] buffers")
    B, P, n = sp.shape
    _grn_f32("grn_bwd_finish", B * P * n, sp, dp)
    _grn_f32("grn_bwd_finish", B * n, G, N)
    _grn_f32("grn_bwd_finish", n, gamma, dgamma, dbeta)
    _check(D.is_cuda and D.dtype == torch.float32 and D.numel() == B and D.is_contiguous(), "grn_bwd_finish: bad D")
    k = torch.empty(B, n, device=sp.device, dtype=torch.float32)
    call("sv_grn_bwd_finish", ptr(sp), ptr(dp), P, ptr(gamma), ptr(G), ptr(N), ptr(D), ptr(k), ptr(dgamma),
         ptr(dbeta), int(bool(accumulate)), B, n)
    return k


def grn_bwd_apply(du2d, a2d, gh2d, scale, k, *, out: torch.Tensor | None = None):
    """dh = (du * scale[b, c] + a * k[b, c]) * gh in the activations' dtype; ``out`` may be ``du2d`` itself."""
    B = scale.shape[0]
    if out is None:
        out = torch.empty_like(du2d)
    HW, n = _grn_act("grn_bwd_apply", B, du2d, a2d, gh2d, out)
    _grn_f32("grn_bwd_apply", B * n, scale, k)
    _timed_call("grn_bwd_apply", 4.0 * a2d.numel() * a2d.element_size(), "sv_grn_bwd_apply", ptr(du2d), ptr(a2d),
                ptr(gh2d), dt(a2d), ptr(scale), ptr(k), ptr(out), B, HW, n)
    return out


def grn_bwd(du2d, a2d, gh2d, B: int, gamma, stats: tuple, *, dgamma, dbeta):
    """The three backward passes, in place over du: returns dh (= du2d's storage)."""
    G, N, scale, D = stats
    sp, dp = grn_bwd_stats(du2d, a2d, B)
    k = grn_bwd_finish(sp, dp, gamma, G, N, D, dgamma=dgamma, dbeta=dbeta)
    return grn_bwd_apply(du2d, a2d, gh2d, scale, k, out=du2d)


# ----------------------------------------------------------------------------------------------
# depthwise 7x7 + LN
# The depthwise conv on the matrix cores (csrc/dwmfma.hip, round 6): per channel a banded-Toeplitz GEMM along the image
# row on v_mfma_f32_16x16x32_bf16, with bf16 operands (the precision torch.autocast gives conv_dw).  Default: the bf16
# training forward (z kept) and the bf16-dz backward-data run on it (+1.3-1.4 % training step over the f32 VALU kernels,
# profiles/round6/r13g_*), and the tape-free eval forward (MFMA + LayerNorm beat the VALU one pass: S3 35.3 vs 44.5 us,
# r13l); SV_DW_MFMA=0 keeps the VALU kernels (dwconv.hip), which the f32 parity mode always uses.
DW_MFMA = os.environ.get("SV_DW_MFMA", "1") != "0"
# the weight gradient on the matrix cores (sv_dwconv7_bwd_weight_mfma): opt-in -- correct, but 20 % slower than the VALU
# ring kernel standalone and in the step (r13l: S3 39.0 vs 31.9 us; dw_wgrad 3.4-3.8 vs 2.9 ms/step)
DW_MFMA_WGRAD = DW_MFMA and os.environ.get("SV_DW_MFMA_WGRAD", "0") != "0"


def dwconv7_fwd_mfma(x4d, wdw, bdw):
    """z (bf16) = bf16(bdw + sum_tap bf16(w) bf16(x)) (sv_dwconv7_fwd_mfma)."""
    B, H, W, C = x4d.shape
    _check(C % 32 == 0 and x4d.is_contiguous() and x4d.dtype in (torch.float32, torch.bfloat16),
           "dwconv7_fwd_mfma: contiguous f32 / bf16 [B,H,W,C], C % 32 == 0")
    _check(wdw.dtype == torch.float32 and wdw.is_contiguous() and wdw.numel() == 49 * C and bdw.numel() == C,
           "dwconv7_fwd_mfma: f32 weight [C,1,7,7], bias [C]")
    z = torch.empty(B, H, W, C, device=x4d.device, dtype=torch.bfloat16)
    n = B * H * W * C
    _timed_call("dw_fwd", n * (x4d.element_size() + 2), "sv_dwconv7_fwd_mfma", ptr(x4d), dt(x4d), ptr(wdw), ptr(bdw),
                ptr(z), B, H, W, C, flops=98.0 * n)
    return z


def dwconv7_ln_fwd(x4d, wdw, bdw, lnw, lnb, *, act_dtype, eps=EPS_LN, save_z=True):
    """-> z (the conv output, saved for the LayerNorm backward; None when ``save_z`` is False and the one-pass form
    runs), y = LN(z), mean, rstd.  C = 128 / 256 / 512 over an f32 input run as ONE kernel (sv_dwconv7_ln_fused_ok),
    bitwise the two-launch result."""
    B, H, W, C = x4d.shape
    _check(C % 32 == 0, "dwconv7: C must be a multiple of 32")
    if DW_MFMA and act_dtype == torch.bfloat16:
        z = dwconv7_fwd_mfma(x4d, wdw, bdw)
        y, mean, rstd = layernorm_fwd(z.view(-1, C), lnw, lnb, out_dtype=act_dtype, eps=eps)
        return (z if save_z else None), y, mean, rstd
    act_code = SV_BF16 if act_dtype == torch.bfloat16 else SV_F32
    if not save_z and value("sv_dwconv7_ln_fused_ok", B, H, W, C, dt(x4d), act_code, act_code):
        z = None
    else:
        z = torch.empty(B, H, W, C, device=x4d.device, dtype=act_dtype)
    y = torch.empty(B * H * W, C, device=x4d.device, dtype=act_dtype)
    mean = torch.empty(B * H * W, device=x4d.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    n = B * H * W * C
    # algorithmic: x read once; z (saved for the LN backward) and y (the fc1 operand) written; mean / rstd
    nb = n * (x4d.element_size() + (z.element_size() if z is not None else 0) + y.element_size()) + B * H * W * 8
    _timed_call("dw_fwd", nb, "sv_dwconv7_ln_fwd", ptr(x4d), dt(x4d), ptr(wdw), ptr(bdw), ptr(lnw), ptr(lnb), eps, ptr(z),
                dt(y) if z is None else dt(z), ptr(y), dt(y), ptr(mean), ptr(rstd), B, H, W, C, fma=49.0 * n)
    return z, y, mean, rstd


def dwconv7_bwd_data(dz4d, wdw, dx4d, accumulate=True, dx_bf16=None):
    B, H, W, C = dz4d.shape
    _check(dx4d.shape == dz4d.shape and dx4d.dtype == torch.float32, "dwconv7_bwd_data: shape")
    if dx_bf16 is not None:
        _check(dx_bf16.numel() == dx4d.numel() and dx_bf16.dtype == torch.bfloat16, "dwconv7_bwd_data: bf16 copy")
    n = B * H * W * C
    # algorithmic: dz read; the f32 gradient stream dx written (and read when accumulating); its bf16 copy
    nb = n * (dz4d.element_size() + 4 * (2 if accumulate else 1) + (2 if dx_bf16 is not None else 0))
    if DW_MFMA and dz4d.dtype == torch.bfloat16 and C % 32 == 0:
        _timed_call("dw_bwd_data", nb, "sv_dwconv7_bwd_data_mfma", ptr(dz4d), ptr(wdw), ptr(dx4d), ptr(dx_bf16),
                    int(accumulate), B, H, W, C, flops=98.0 * n)
        return
    _timed_call("dw_bwd_data", nb, "sv_dwconv7_bwd_data", ptr(dz4d), dt(dz4d), ptr(wdw), ptr(dx4d), ptr(dx_bf16),
                int(accumulate), B, H, W, C, fma=49.0 * n)


def dwconv7_bwd_weight(dz4d, x4d, *, dw, db, defer: list | None = None):
    B, H, W, C = dz4d.shape
    mfma = DW_MFMA_WGRAD and dz4d.dtype == torch.bfloat16 and C % 16 == 0
    P = value("sv_dwconv7_bwd_weight_mfma_nparts" if mfma else "sv_dwconv7_bwd_weight_nparts", B, H, W, C)
    pw = torch.empty(P * C * 49, device=dz4d.device, dtype=torch.float32)
    pb = torch.empty(P * C, device=dz4d.device, dtype=torch.float32)
    # algorithmic: dz and x read once, the [C,49] + [C] gradient written (the partials are a design choice)
    nb = B * H * W * C * (dz4d.element_size() + x4d.element_size()) + C * 50 * 4
    if mfma:
        _timed_call("dw_wgrad", nb, "sv_dwconv7_bwd_weight_mfma", ptr(dz4d), ptr(x4d), dt(x4d), ptr(pw), ptr(pb),
                    B, H, W, C, flops=98.0 * B * H * W * C)
    else:
        _timed_call("dw_wgrad", nb, "sv_dwconv7_bwd_weight", ptr(dz4d), dt(dz4d), ptr(x4d), dt(x4d), ptr(pw), ptr(pb),
                    B, H, W, C, fma=49.0 * B * H * W * C)
    if defer is not None:
        defer += [(pw, dw, P, True), (pb, db, P, True)]
        return
    reduce_pair(pw, dw, pb, db, P)


# ----------------------------------------------------------------------------------------------
# stem / downsample / pool
def stem_fwd(img, w, b, lnw, lnb, *, eps=EPS_LN):
    B, Cin, H, W = img.shape
    _check(Cin == 3 and H % 4 == 0 and W % 4 == 0, "stem: expects [B,3,H,W] with H,W % 4 == 0")
    _check(img.dtype == torch.float32 and img.is_contiguous(), "stem: image must be contiguous f32 NCHW")
    C = w.shape[0]
    y = torch.empty(B, H // 4, W // 4, C, device=img.device, dtype=torch.float32)
    mean = torch.empty(B * (H // 4) * (W // 4), device=img.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("sv_stem_patchify_ln_fwd", ptr(img), ptr(w), ptr(b), ptr(lnw), ptr(lnb), eps, ptr(y), dt(y), ptr(mean),
         ptr(rstd), B, H, W, C)
    return y, mean, rstd


def stem_bwd(img, w, b, lnw, mean, rstd, dy, *, dw, db, dlnw, dlnb):
    B, _, H, W = img.shape
    C = w.shape[0]
    P = value("sv_stem_patchify_ln_bwd_nparts", B, H, W, C)
    pw = torch.empty(P * C * 48, device=img.device, dtype=torch.float32)
    pv = torch.empty(3, P * C, device=img.device, dtype=torch.float32)
    call("sv_stem_patchify_ln_bwd", ptr(img), ptr(w), ptr(b), ptr(lnw), ptr(mean), ptr(rstd), ptr(dy), ptr(pw),
         ptr(pv[0]), ptr(pv[1]), ptr(pv[2]), B, H, W, C)
    reduce_pair(pw, dw, pv[0], db, P)
    reduce_pair(pv[1], dlnw, pv[2], dlnb, P)


IMAGENET_MEAN = (0.485, 0.456, 0.406)  # torchvision Normalize constants of the reference transform
IMAGENET_STD = (0.229, 0.224, 0.225)


def _host3(v) -> ctypes.Array:
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def stem_patchify(img, *, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """Stem patch rows for the MFMA stem conv: bf16 [B*(H/4)*(W/4), 64] (k = ci*16 + kh*4 + kw, 48..63
    zero).  img: the normalised f32 batch [B,3,H,W] or a uint8 grayscale batch [B,H,W] (the reference
    transform ToTensor + gray->RGB + Normalize(mean, std) is then applied in the gather)."""
    if img.dtype == torch.uint8:
        _check(img.dim() == 3 and img.is_contiguous(), "stem_patchify: uint8 input must be contiguous [B,H,W]")
        B, H, W = img.shape
        kind = nv.SV_IMG_U8_GRAY
    else:
        _check(img.dim() == 4 and img.shape[1] == 3 and img.dtype == torch.float32 and img.is_contiguous(),
               "stem_patchify: expects contiguous f32 [B,3,H,W]")
        B, _, H, W = img.shape
        kind = nv.SV_IMG_F32_NCHW
    _check(H % 4 == 0 and W % 4 == 0, "stem_patchify: H, W must be multiples of 4")
    patches = torch.empty(B * (H // 4) * (W // 4), 64, device=img.device, dtype=torch.bfloat16)
    call("sv_stem_patchify", ptr(img), kind, _host3(mean), _host3(std), ptr(patches), B, H, W)
    return patches


def stem_weight_pack(w) -> torch.Tensor:
    """timm stem.0.weight [C,3,4,4] f32 -> bf16 [C,64] (k 48..63 zero), the B operand of the stem GEMM."""
    C = w.shape[0]
    _check(w.numel() == C * 48 and w.dtype == torch.float32 and w.is_contiguous(), "stem_weight_pack: bad weight")
    out = torch.empty(C, 64, device=w.device, dtype=torch.bfloat16)
    call("sv_stem_weight_pack", ptr(w), ptr(out), C)
    return out


def normalize_u8_gray(img_u8, *, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None) -> torch.Tensor:
    """Device form of the reference transform tail (localization.py:196-233, 254): uint8 grayscale
    [B,H,W] -> convert("RGB") -> ToTensor (/255) -> Normalize(mean, std) -> f32 [B,3,H,W]."""
    _check(img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.is_contiguous(),
           "normalize_u8_gray: expects contiguous uint8 [B,H,W]")
    B, H, W = img_u8.shape
    _check((H * W) % 4 == 0, "normalize_u8_gray: H*W must be a multiple of 4")
    if out is None:
        out = torch.empty(B, 3, H, W, device=img_u8.device, dtype=torch.float32)
    _check(out.shape == (B, 3, H, W) and out.dtype == torch.float32 and out.is_contiguous(),
           "normalize_u8_gray: bad out")
    call("sv_normalize_u8_gray", ptr(img_u8), _host3(mean), _host3(std), ptr(out), B, H, W)
    return out


def augment_u8(img_u8: torch.Tensor, params: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Train-time flip / affine / colour jitter of decoded uint8 images on the device (row f1):
    ``img_u8`` [B,H,W] (grayscale) or [B,H,W,3] (RGB), ``params`` float64 [B,10] from
    ``training.datasets.augment.sample_params`` (torchvision's draws).  Bitwise equal to the PIL
    operations torchvision applies on the host (sv_augment_u8)."""
    _check(img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() in (3, 4),
           "augment_u8: expects contiguous uint8 [B,H,W] or [B,H,W,3]")
    B, H, W = img_u8.shape[:3]
    C = 1 if img_u8.dim() == 3 else img_u8.shape[3]
    _check(C in (1, 3), "augment_u8: 1 or 3 channels")
    params = params.to(device=img_u8.device, dtype=torch.float64).contiguous()
    _check(tuple(params.shape) == (B, 10), "augment_u8: params must be [B,10]")
    if out is None:
        out = torch.empty_like(img_u8)
    _check(out.shape == img_u8.shape and out.dtype == torch.uint8 and out.is_contiguous()
           and out.data_ptr() != img_u8.data_ptr(), "augment_u8: bad out")
    rows = torch.empty(B * H, device=img_u8.device, dtype=torch.int32)
    call("sv_augment_u8", ptr(img_u8), ptr(out), B, H, W, C, ptr(params), ptr(rows))
    return out


def resize_u8(src: torch.Tensor, desc: torch.Tensor, coef: torch.Tensor, B: int, H: int, W: int, C: int,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """PIL Image.resize((W, H), BILINEAR) of a ragged uint8 batch on the device (row f1, sv_resize_u8):
    ``src`` flat uint8, ``desc`` int64 [B,8] and ``coef`` int32 tables from
    ``training.datasets.resize.ragged_batch``.  Returns uint8 [B,H,W] (C = 1) or [B,H,W,3]."""
    _check(src.dtype == torch.uint8 and src.is_contiguous(), "resize_u8: src must be contiguous uint8")
    _check(desc.dtype == torch.int64 and tuple(desc.shape) == (B, 8) and desc.is_contiguous(), "resize_u8: desc [B,8]")
    _check(coef.dtype == torch.int32 and coef.is_contiguous(), "resize_u8: coef must be int32")
    _check(C in (1, 3), "resize_u8: C must be 1 or 3")
    shape = (B, H, W) if C == 1 else (B, H, W, 3)
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=torch.uint8)
    _check(tuple(out.shape) == shape and out.dtype == torch.uint8 and out.is_contiguous(), "resize_u8: bad out")
    call("sv_resize_u8", ptr(src), ptr(desc), ptr(coef), B, H, W, C, ptr(out))
    return out


def device_images(batch: dict, device) -> torch.Tensor:
    """The decoded uint8 image batch of a device_transform loader on ``device``, resized (ragged batch:
    "resize" = ragged_batch(...)) and augmented ("augment") there -- the reference's Resize -> [flip /
    affine / jitter] on the GPU; ToTensor -> Normalize then run inside the backbone's stem gather."""
    rz = batch.get("resize")
    if rz is not None:
        H, W, C = (int(v) for v in rz["out_hw"])
        img = resize_u8(rz["src"].to(device, non_blocking=True), rz["desc"].to(device, non_blocking=True),
                        rz["coef"].to(device, non_blocking=True), rz["desc"].shape[0], H, W, C)
    else:
        img = batch["image"].to(device, non_blocking=True)
    if "augment" in batch:
        img = augment_u8(img, batch["augment"].to(device, non_blocking=True))
    return img


def downsample_fwd(x4d, lnw, lnb, *, act_dtype, eps=EPS_LN):
    B, H, W, C = x4d.shape
    _check(H % 2 == 0 and W % 2 == 0, "downsample: H, W must be even")
    patches = torch.empty(B * (H // 2) * (W // 2), 4 * C, device=x4d.device, dtype=act_dtype)
    mean = torch.empty(B * H * W, device=x4d.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("sv_downsample_ln_patch2_fwd", ptr(x4d), ptr(lnw), ptr(lnb), eps, ptr(patches), dt(patches), ptr(mean),
         ptr(rstd), B, H, W, C)
    return patches, mean, rstd


def downsample_bwd(dpatches, x4d, mean, rstd, lnw, *, dlnw, dlnb, with_bf16=False):
    """-> dx (f32 [B,H,W,C]) and, with ``with_bf16``, its bf16 GEMM-operand copy (else None)."""
    B, H, W, C = x4d.shape
    dx = torch.empty(B, H, W, C, device=x4d.device, dtype=torch.float32)
    dxb = torch.empty(B, H, W, C, device=x4d.device, dtype=torch.bfloat16) if with_bf16 else None
    P = value("sv_downsample_ln_patch2_bwd_nparts", B, H, W, C)
    pv = torch.empty(2, P * C, device=x4d.device, dtype=torch.float32)
    call("sv_downsample_ln_patch2_bwd", ptr(dpatches), ptr(x4d), ptr(mean), ptr(rstd), ptr(lnw), ptr(dx), ptr(dxb),
         ptr(pv[0]), ptr(pv[1]), B, H, W, C)
    reduce_pair(pv[0], dlnw, pv[1], dlnb, P)
    return dx, dxb


def pool_ln_fwd(x4d, lnw, lnb, *, eps=EPS_LN):
    B, H, W, C = x4d.shape
    pooled = torch.empty(B, C, device=x4d.device, dtype=torch.float32)
    feat = torch.empty_like(pooled)
    mean = torch.empty(B, device=x4d.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("sv_pool_ln_fwd", ptr(x4d), ptr(lnw), ptr(lnb), eps, ptr(pooled), ptr(feat), ptr(mean), ptr(rstd), B,
         H * W, C)
    return feat, pooled, mean, rstd


def pool_ln_bwd(dfeat, pooled, mean, rstd, lnw, shape, *, dlnw, dlnb, with_bf16=False):
    """-> dx (f32 [B,H,W,C]) and, with ``with_bf16``, its bf16 GEMM-operand copy (else None)."""
    B, H, W, C = shape
    dx = torch.empty(B, H, W, C, device=dfeat.device, dtype=torch.float32)
    dxb = torch.empty(B, H, W, C, device=dfeat.device, dtype=torch.bfloat16) if with_bf16 else None
    pv = torch.empty(2, B * C, device=dfeat.device, dtype=torch.float32)
    call("sv_pool_ln_bwd", ptr(dfeat.contiguous()), ptr(pooled), ptr(mean), ptr(rstd), ptr(lnw), ptr(dx), ptr(dxb),
         ptr(pv[0]), ptr(pv[1]), B, H * W, C)
    reduce_pair(pv[0], dlnw, pv[1], dlnb, B)
    return dx, dxb


# ----------------------------------------------------------------------------------------------
# optimizer pieces
def scale_rows_bf16(W: torch.Tensor, scale: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16(W * scale[:, None]) for a 2-D f32 weight (fc2 weight with the layer scale folded in)."""
    rows, cols = W.shape
    _check(W.dtype == torch.float32 and W.is_contiguous() and scale.numel() == rows, "scale_rows_bf16: bad args")
    if out is None:
        out = torch.empty(rows, cols, device=W.device, dtype=torch.bfloat16)
    _check(out.shape == (rows, cols) and out.dtype == torch.bfloat16 and out.is_contiguous(), "scale_rows_bf16: bad out")
    call("sv_scale_rows_bf16", ptr(W), ptr(scale), ptr(out), rows, cols)
    return out


def cast_bf16(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    _check(x.dtype == torch.float32 and x.is_contiguous(), "cast_bf16: need contiguous f32")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    call("sv_cast_f32_bf16", ptr(x), ptr(out), x.numel())
    return out


def grad_clip_coef(g_flat: torch.Tensor, max_norm: float) -> torch.Tensor:
    """Device tensor [norm, coef] with coef = min(1, max_norm/(norm+1e-6)) -- no host sync."""
    n = g_flat.numel()
    P = value("sv_sqnorm_nparts", n)
    part = torch.empty(P, device=g_flat.device, dtype=torch.float32)
    call("sv_sqnorm_partial", ptr(g_flat), n, ptr(part))
    out = torch.empty(2, device=g_flat.device, dtype=torch.float32)
    call("sv_clip_coef", ptr(part), P, float(max_norm), ptr(out))
    return out


def adamw_hyper(lr: float, beta1: float, beta2: float, step: int) -> list[float]:
    """[lr, 1 - b1^step, sqrt(1 - b2^step)] as f32 values, rounded exactly as sv_adamw_flat derives
    them on the host (double power, f32 rounding, f32 sqrt) -- the device operand of adamw_flat(hyper=)."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))  # the C ABI takes the betas as f32
    bc1 = np.float32(1.0 - b1 ** step)
    bc2 = np.float32(1.0 - b2 ** step)
    return [float(np.float32(lr)), float(bc1), float(np.sqrt(bc2, dtype=np.float32))]


def adamw_flat(p, g, m, v, p_bf16, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=None, hyper=None):
    """``hyper``: optional f32 device tensor [3] (adamw_hyper) replacing lr/step -- graph replay."""
    n = p.numel()
    _check(g.numel() == n and m.numel() == n and v.numel() == n, "adamw_flat: size mismatch")
    if hyper is not None:
        _check(hyper.dtype == torch.float32 and hyper.is_cuda and hyper.numel() >= 3, "adamw_flat: hyper")
        call("sv_adamw_flat_dev", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), n, float(beta1), float(beta2),
             float(eps), float(weight_decay), ptr(hyper), ptr(grad_scale))
        return
    # algorithmic: p, g, m, v read; p, m, v written; the bf16 shadow written (30 B / parameter)
    nb = n * (28 + (2 if p_bf16 is not None else 0))
    _timed_call("adamw", nb, "sv_adamw_flat", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), n, float(lr), float(beta1),
                float(beta2), float(eps), float(weight_decay), int(step), ptr(grad_scale))


# ----------------------------------------------------------------------------------------------
# ResNet-18/50: implicit-GEMM convolution, BatchNorm (train-mode batch statistics), pooling
EPS_BN = 1e-5


def _is_pow2(v: int) -> bool:
    return v > 0 and (v & (v - 1)) == 0


def conv_out_hw(H: int, W: int, k: int, stride: int, pad: int) -> tuple[int, int]:
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_shape(B, H, W, Cs, Cout, k, stride, pad, Cin=None) -> nv.ConvShape:
    s = nv.ConvShape()
    s.B, s.H, s.W, s.Cs, s.Cout = B, H, W, Cs, Cout
    s.KH = s.KW = k
    s.stride, s.pad = stride, pad
    s.Cin = Cs if Cin is None else Cin
    _check(_is_pow2(Cs) and Cs >= 4 and Cout % 8 == 0 and 0 < s.Cin <= Cs and stride in (1, 2),
           f"conv: unsupported shape Cs={Cs} Cout={Cout} Cin={s.Cin} stride={stride}")
    return s


def conv_weight_pack(w: torch.Tensor, Cs: int, dtype: torch.dtype) -> torch.Tensor:
    """torch weight [Cout][Cin][k][k] f32 -> packed [Cout][k*k][Cs] (`dtype`), channels >= Cin zero."""
    Cout, Cin, KH, KW = w.shape
    _check(w.dtype == torch.float32 and w.is_contiguous() and KH == KW, "conv_weight_pack: need contiguous f32 [Co,Ci,k,k]")
    s = conv_shape(1, KH, KW, Cs, Cout, KH, 1, 0, Cin)
    wp = torch.empty(Cout, KH * KW, Cs, device=w.device, dtype=dtype)
    call("sv_conv_weight_pack", ptr(w), ptr(wp), dt(wp), ctypes.byref(s))
    return wp


def conv_weight_pack_multi(items: list, dtype: torch.dtype) -> list:
    """conv_weight_pack for several weights in one launch per SV_MAX_PACK_SEGS (sv_conv_weight_pack_multi).
    items: (w f32 [Cout][Cin][k][k], Cs) pairs -> the packed [Cout][k*k][Cs] tensors, in order."""
    out = []
    for i in range(0, len(items), nv.SV_MAX_PACK_SEGS):
        chunk = items[i:i + nv.SV_MAX_PACK_SEGS]
        segs = (nv.PackSeg * len(chunk))()
        for j, (w, Cs) in enumerate(chunk):
            Cout, Cin, KH, KW = w.shape
            _check(w.dtype == torch.float32 and w.is_contiguous() and KH == KW and Cs >= Cin,
                   "conv_weight_pack_multi: need contiguous f32 [Co,Ci,k,k] and Cs >= Ci")
            wp = torch.empty(Cout, KH * KW, Cs, device=w.device, dtype=dtype)
            segs[j] = nv.PackSeg(ptr(w), ptr(wp), Cout, Cin, KH * KW, Cs)
            out.append(wp)
        call("sv_conv_weight_pack_multi", segs, len(chunk), SV_BF16 if dtype == torch.bfloat16 else SV_F32)
    return out


def _conv_check_x(x: torch.Tensor, s: nv.ConvShape, dtype: torch.dtype, who: str) -> None:
    _check(x.is_contiguous() and tuple(x.shape) == (s.B, s.H, s.W, s.Cs) and x.dtype == dtype,
           f"{who}: x must be contiguous {dtype} [B,H,W,Cs]={(s.B, s.H, s.W, s.Cs)}, got {tuple(x.shape)} {x.dtype}")


def _pointwise(s: nv.ConvShape, dtype: torch.dtype) -> bool:
    """1x1 / stride 1 / no padding over unpadded channels in bf16: in NHWC the conv IS a GEMM over
    [B*H*W, C] rows, so it runs on the LDS-DMA MFMA GEMM (sv_gemm v3) instead of the implicit-GEMM
    conv kernel (ResNet-50 bottleneck conv1 / conv3: ~half of its conv FLOPs)."""
    return (s.KH == 1 and s.KW == 1 and s.stride == 1 and s.pad == 0 and s.Cs == s.Cin and dtype == torch.bfloat16
            and s.Cs % 32 == 0 and s.Cout % 32 == 0)


# gathered forward convolutions split K only from this many 32-deep k-steps (round 4, profiles/round4/
# r8e_conv_split_sweep.txt: layer2's 3x3 forward, K = 1152, 128 tiles, runs in 30 us unsplit against 35 + a 7 us
# finish at split 2; layer3 / 4, K = 2304 / 4608, are fastest at split 4 / 8 as before)
_CONV_FWD_MIN_KSTEPS = int(os.environ.get("SV_CONV_FWD_MIN_KSTEPS", "64"))


def _conv_split(M: int, N: int, K: int, min_ksteps: int = 32) -> int:
    """split-K depth of a bf16 conv GEMM whose grid of 256x128 tiles would not give every CU a workgroup
    (ResNet layer3/4 at 256 px: 32-128 tiles, each a long latency-bound chain of 32-deep k-steps):
    about one workgroup per CU, >= 16 k-steps per slice, <= 32 MiB of f32 slabs (written by the GEMM,
    read back by sv_gemm_slab_finish), at most 16 slices.  1 = no split (also below ``min_ksteps`` k-steps, where
    the slab round trip costs more than the chain it shortens)."""
    tiles = -(-M // 256) * -(-N // 128)
    ksteps = K // 32
    if tiles >= 192 or ksteps < min_ksteps:
        return 1
    return max(1, min(-(-256 // tiles), ksteps // 16, (32 << 20) // (M * N * 4), 16))


def _gathered(s: nv.ConvShape, dtype: torch.dtype) -> bool:
    """the bf16 gathered-operand GEMM path of sv_conv_fwd (csrc/conv.hip conv_fwd_impl)"""
    return dtype == torch.bfloat16 and s.Cs >= 32 and _is_pow2(s.Cs) and (s.KH * s.KW * s.Cs) % 32 == 0


def _stem8(s: nv.ConvShape, dtype: torch.dtype) -> bool:
    """the bf16 8-channel gathered path of sv_conv_fwd (conv.hip mode 6: the ResNet stem over its zero-padded
    RGB operand, one tap per 16-B chunk)"""
    return (_STEM_GATHER and dtype == torch.bfloat16 and s.Cs == 8 and s.KH == s.KW and s.KH <= 7
            and s.Cout % 8 == 0)


# SV_STEM_GATHER=0: the stem forward on the register-staged conv kernel plus a BatchNorm statistics pass (A/B runs)
_STEM_GATHER = os.environ.get("SV_STEM_GATHER", "1") != "0"


def _slab_finish(work: torch.Tensor, split: int, M: int, N: int, C: torch.Tensor, *, accumulate: bool = False,
                 stats: torch.Tensor | None = None) -> None:
    _timed_call("fold", 4.0 * M * N * (split + 1 + int(bool(accumulate))), "sv_gemm_slab_finish", ptr(work), split, M,
                N, ptr(C), dt(C), N, int(accumulate), ptr(stats))


def _pointwise_fwd(x, wp, s, y, M, stats=None, policy=None, work=None):
    """1x1 conv forward as a GEMM over [M, Cs] rows; split-K + slab finish when the grid is small."""
    split = _conv_split(M, s.Cout, s.Cs)
    x2d, w2d = x.view(M, s.Cs), wp.view(s.Cout, s.Cs)
    if split > 1:
        work = (torch.empty(split * M * s.Cout, device=x.device, dtype=torch.float32) if work is None
                else _conv_work(work, split * M * s.Cout, x.device, "conv_fwd")[:split * M * s.Cout])
        linear_fwd(x2d, w2d, out=work, epilogue=nv.SV_EPI_SLAB, split_k=split, policy=policy)
        _slab_finish(work, split, M, s.Cout, y, stats=stats)
    elif stats is not None:
        linear_fwd(x2d, w2d, out=y.view(M, s.Cout), out2=stats, epilogue=nv.SV_EPI_STORE_STATS, policy=policy)
    else:
        linear_fwd(x2d, w2d, out=y.view(M, s.Cout), policy=policy)


def _conv_buf(t, shape: tuple, dtype: torch.dtype, device, who: str) -> torch.Tensor:
    """the caller's ``out=`` / ``part=`` buffer, checked (callers allocate a fresh one when none is given)"""
    _check(t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.device == device,
           f"{who} must be contiguous {dtype} {tuple(shape)}, got {tuple(t.shape)} {t.dtype}")
    return t


def _conv_work(work, n: int, device, who: str) -> torch.Tensor:
    """the caller's f32 ``work=`` space of at least n floats, checked (callers allocate a fresh one when none is given)"""
    _check(work.is_contiguous() and work.dtype == torch.float32 and work.numel() >= n and work.device == device,
           f"{who}: work must be contiguous f32 with at least {n} elements")
    return work


def conv_fwd(x: torch.Tensor, wp: torch.Tensor, s: nv.ConvShape, out_dtype: torch.dtype,
             policy: "nv.GemmPolicy | None" = None, *, out: torch.Tensor | None = None,
             work: torch.Tensor | None = None, split: int | None = None) -> torch.Tensor:
    """``out`` / ``work``: the output and the split-K slab space (default: fresh allocations); ``split``: the slice
    count of the gathered split-K form (default: the host schedule ``_conv_split``)."""
    _conv_check_x(x, s, wp.dtype, "conv_fwd")
    _check(tuple(wp.shape) == (s.Cout, s.KH * s.KW, s.Cs), "conv_fwd: packed weight shape")
    OH, OW = conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)
    y = (torch.empty(s.B, OH, OW, s.Cout, device=x.device, dtype=out_dtype) if out is None
         else _conv_buf(out, (s.B, OH, OW, s.Cout), out_dtype, x.device, "conv_fwd: out"))
    if _pointwise(s, wp.dtype):
        _check(split is None, "conv_fwd: split applies to the gathered path")
        _pointwise_fwd(x, wp, s, y, s.B * s.H * s.W, policy=policy, work=work)
        return y
    M, K = s.B * OH * OW, s.KH * s.KW * s.Cs
    if split is None:
        split = _conv_split(M, s.Cout, K, _CONV_FWD_MIN_KSTEPS) if _gathered(s, wp.dtype) else 1
    else:
        _check(_gathered(s, wp.dtype) and 1 <= split <= K // 32, "conv_fwd: split needs the gathered path")
    if split > 1:
        work = (torch.empty(split * M * s.Cout, device=x.device, dtype=torch.float32) if work is None
                else _conv_work(work, split * M * s.Cout, x.device, "conv_fwd"))
        call("sv_conv_fwd_split", ptr(x), ptr(wp), ptr(y), dt(y), dt(wp), ctypes.byref(s), None, ptr(work), split,
             nv.pol_ref(policy))
        return y
    call("sv_conv_fwd", ptr(x), ptr(wp), ptr(y), dt(y), dt(wp), ctypes.byref(s), nv.pol_ref(policy))
    return y


_ONES: dict = {}


def _ones(n: int, device: torch.device) -> torch.Tensor:
    """Cached f32 ones[n] per device (the gamma of an in-place accumulate epilogue): no fill launch per call."""
    key = (n, device)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(n, device=device, dtype=torch.float32)
    return t


def conv_fwd_bn_stats(x: torch.Tensor, wp: torch.Tensor, s: nv.ConvShape, out_dtype: torch.dtype,
                      policy: "nv.GemmPolicy | None" = None, *, out: torch.Tensor | None = None,
                      part: torch.Tensor | None = None, work: torch.Tensor | None = None, split: int | None = None):
    """conv_fwd plus the train-mode BatchNorm statistics of y straight from the GEMM epilogue
    (SV_EPI_STORE_STATS: no separate read pass over y) -> (y, partials [ceil(M/64)][2][Cout] f32), or
    (y, None) when the conv runs on a path without that epilogue (then use bn_stats(y)).
    ``out`` / ``part`` / ``work`` / ``split``: as conv_fwd's (``part``: the partials buffer)."""
    if wp.dtype != torch.bfloat16 or out_dtype != torch.bfloat16 or s.Cout % 8:
        return conv_fwd(x, wp, s, out_dtype, policy, out=out, work=work, split=split), None
    OH, OW = conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)
    M = s.B * OH * OW
    if _pointwise(s, wp.dtype):
        if s.Cs % 32:
            return conv_fwd(x, wp, s, out_dtype, policy, out=out, work=work, split=split), None
        _check(split is None, "conv_fwd: split applies to the gathered path")
        _conv_check_x(x, s, wp.dtype, "conv_fwd")
        y = (torch.empty(s.B, OH, OW, s.Cout, device=x.device, dtype=out_dtype) if out is None
             else _conv_buf(out, (s.B, OH, OW, s.Cout), out_dtype, x.device, "conv_fwd: out"))
        part = (torch.empty((M + 63) // 64, 2, s.Cout, device=x.device, dtype=torch.float32) if part is None
                else _conv_buf(part, ((M + 63) // 64, 2, s.Cout), torch.float32, x.device, "conv_fwd_bn_stats: part"))
        _pointwise_fwd(x, wp, s, y, M, stats=part, policy=policy, work=work)
        return y, part
    if not (_gathered(s, wp.dtype) or _stem8(s, wp.dtype)):
        return conv_fwd(x, wp, s, out_dtype, policy, out=out, work=work, split=split), None
    _conv_check_x(x, s, wp.dtype, "conv_fwd")
    _check(tuple(wp.shape) == (s.Cout, s.KH * s.KW, s.Cs), "conv_fwd: packed weight shape")
    y = (torch.empty(s.B, OH, OW, s.Cout, device=x.device, dtype=out_dtype) if out is None
         else _conv_buf(out, (s.B, OH, OW, s.Cout), out_dtype, x.device, "conv_fwd: out"))
    part = (torch.empty((M + 63) // 64, 2, s.Cout, device=x.device, dtype=torch.float32) if part is None
            else _conv_buf(part, ((M + 63) // 64, 2, s.Cout), torch.float32, x.device, "conv_fwd_bn_stats: part"))
    if split is None:
        split = 1 if _stem8(s, wp.dtype) else _conv_split(M, s.Cout, s.KH * s.KW * s.Cs, _CONV_FWD_MIN_KSTEPS)
    else:
        _check(_gathered(s, wp.dtype) and 1 <= split <= s.KH * s.KW * s.Cs // 32,
               "conv_fwd: split needs the gathered path")
    if split > 1:
        work = (torch.empty(split * M * s.Cout, device=x.device, dtype=torch.float32) if work is None
                else _conv_work(work, split * M * s.Cout, x.device, "conv_fwd"))
        call("sv_conv_fwd_split", ptr(x), ptr(wp), ptr(y), dt(y), dt(wp), ctypes.byref(s), ptr(part), ptr(work), split,
             nv.pol_ref(policy))
    else:
        call("sv_conv_fwd_stats", ptr(x), ptr(wp), ptr(y), dt(y), dt(wp), ctypes.byref(s), ptr(part), nv.pol_ref(policy))
    return y, part


def bn_stats_from_partials(part: torch.Tensor, rows: int, *, eps: float = EPS_BN, momentum: float = 0.1,
                           running_mean=None, running_var=None, num_batches_tracked=None, out: tuple | None = None):
    """(mean, rstd) from conv_fwd_bn_stats' unshifted partials; running stats updated like bn_stats.
    ``out``: the caller's (mean, rstd) f32 [C] buffers (default: fresh allocations)."""
    P, two, C = part.shape
    _check(two == 2 and part.dtype == torch.float32 and part.is_contiguous(), "bn_stats_from_partials: bad partials")
    if out is None:
        mean = torch.empty(C, device=part.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
    else:
        mean, rstd = _bn_stat_out(out, C, part.device, "bn_stats_from_partials")
    _fin("sv_bn_stats_finish", None, SV_F32, ptr(part), P, rows, C, float(eps), float(momentum), ptr(mean),
         ptr(rstd), ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), *_fin_ws(part.device))
    return mean, rstd


def conv_bwd_data(dy: torch.Tensor, wp: torch.Tensor, s: nv.ConvShape, *, dx: torch.Tensor | None = None,
                  accumulate: bool = False, dx_dtype: torch.dtype = torch.float32,
                  policy: "nv.GemmPolicy | None" = None, work: torch.Tensor | None = None) -> torch.Tensor:
    """``work``: the slab space of the split-K and the stride-2 scatter forms (default: a fresh allocation)"""
    OH, OW = conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)
    _check(dy.is_contiguous() and tuple(dy.shape) == (s.B, OH, OW, s.Cout) and dy.dtype == wp.dtype,
           "conv_bwd_data: dy must be contiguous [B,OH,OW,Cout] in the compute dtype")
    _check(_is_pow2(s.Cout), "conv_bwd_data: Cout must be a power of two")
    if dx is None:
        _check(not accumulate, "conv_bwd_data: accumulate needs dx")
        dx = torch.empty(s.B, s.H, s.W, s.Cs, device=dy.device, dtype=dx_dtype)
    _check(dx.is_contiguous() and tuple(dx.shape) == (s.B, s.H, s.W, s.Cs), "conv_bwd_data: dx shape")
    if _pointwise(s, wp.dtype) and (not accumulate or dx.dtype == torch.float32):
        M = s.B * s.H * s.W
        split = _conv_split(M, s.Cs, s.Cout)
        dy2d, w2d = dy.view(M, s.Cout), wp.view(s.Cout, s.Cs)
        if split > 1:
            work = (torch.empty(split * M * s.Cs, device=dy.device, dtype=torch.float32) if work is None
                    else _conv_work(work, split * M * s.Cs, dy.device, "conv_bwd_data")[:split * M * s.Cs])
            linear_dgrad(dy2d, w2d, out=work, epilogue=nv.SV_EPI_SLAB, split_k=split, policy=policy)
            _slab_finish(work, split, M, s.Cs, dx, accumulate=accumulate)
        elif accumulate:  # dx += dy W: the layer-scale/residual epilogue with gamma = 1, residual = dx (in place)
            linear_dgrad(dy2d, w2d, out=dx.view(M, s.Cs), epilogue=nv.SV_EPI_BIAS_GAMMA_RES,
                         gamma=_ones(s.Cs, dy.device), aux=dx.view(M, s.Cs), policy=policy)
        else:
            linear_dgrad(dy2d, w2d, out=dx.view(M, s.Cs), policy=policy)
        return dx
    T = s.KH * s.KW
    # (a bf16 dx accumulates here too -- the ResNet gradient stream: the sum in f32, stored bf16 -- rather than in
    # the pointwise path above, whose residual epilogue reads an f32 operand)
    if (wp.dtype == torch.bfloat16 and s.stride == 1 and s.Cout >= 32 and s.Cs % 8 == 0 and (T * s.Cout) % 32 == 0):
        M = s.B * s.H * s.W
        split = _conv_split(M, s.Cs, T * s.Cout)
        if split > 1:
            work = (torch.empty(split * M * s.Cs, device=dy.device, dtype=torch.float32) if work is None
                    else _conv_work(work, split * M * s.Cs, dy.device, "conv_bwd_data"))
            call("sv_conv_bwd_data_split", ptr(dy), ptr(wp), ptr(dx), dt(dx), int(accumulate), dt(wp),
                 ctypes.byref(s), ptr(work), split, nv.pol_ref(policy))
            return dx
    if wp.dtype == torch.bfloat16 and s.stride == 2 and s.Cout >= 32 and s.Cs % 8 == 0:
        # stride 2: one gathered GEMM per output parity class into compact f32 slabs + one scatter pass
        # (csrc/conv.hip dgrad_s2_scatter_kernel); the workspace holds every class's slabs.  Even H, W
        # without a split: the one-launch form stores each class's rows straight into dx (no workspace)
        M = s.B * s.H * s.W
        split = _s2_split(s, M, T)
        if split == 1 and _s2_direct(s):
            call("sv_conv_bwd_data", ptr(dy), ptr(wp), ptr(dx), dt(dx), int(accumulate), dt(wp), ctypes.byref(s),
                 nv.pol_ref(policy))
            return dx
        work = (torch.empty(split * M * s.Cs, device=dy.device, dtype=torch.float32) if work is None
                else _conv_work(work, split * M * s.Cs, dy.device, "conv_bwd_data"))
        call("sv_conv_bwd_data_split", ptr(dy), ptr(wp), ptr(dx), dt(dx), int(accumulate), dt(wp),
             ctypes.byref(s), ptr(work), split, nv.pol_ref(policy))
        return dx
    call("sv_conv_bwd_data", ptr(dy), ptr(wp), ptr(dx), dt(dx), int(accumulate), dt(wp), ctypes.byref(s),
         nv.pol_ref(policy))
    return dx


# stride-2 data gradients stored straight into dx by the parity-class GEMM's epilogue (csrc/gemm3.hip mode 5
# with remapped rows); 0 = the compact f32 slabs + scatter pass (A/B and the bitwise cross-check)
_S2_DIRECT = os.environ.get("SV_S2_DIRECT", "1") != "0"
# no split-K for the stride-2 dgrads that the one-launch form takes: the four classes already give the grid
# 4x the tiles, and the split's slabs cost more than the longer chains (+0.6 %, r9j); SV_S2_NOSPLIT=0 restores it
_S2_NOSPLIT = os.environ.get("SV_S2_NOSPLIT", "1") != "0"


def _s2_direct(s: nv.ConvShape) -> bool:
    return _S2_DIRECT and s.stride == 2 and s.H % 2 == 0 and s.W % 2 == 0


def _s2_split(s: nv.ConvShape, M: int, T: int) -> int:
    """split-K depth of a stride-2 dgrad's per-class GEMMs (M = B*H*W dx pixels, T taps)"""
    if _S2_NOSPLIT and _s2_direct(s):
        return 1
    return _conv_split(M // 4, s.Cs, max(32, (T * s.Cout) // 4))


def _al16(*ts) -> bool:
    return all(t.data_ptr() % 16 == 0 for t in ts)


def conv_bwd_data_bn(dy: torch.Tensor, wp: torch.Tensor, s: nv.ConvShape, y: torch.Tensor, mean: torch.Tensor,
                     rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, unsplit: bool = True,
                     policy: "nv.GemmPolicy | None" = None, out: torch.Tensor | None = None,
                     part: torch.Tensor | None = None, work: torch.Tensor | None = None):
    """conv_bwd_data (bf16 dx, no accumulate) fused with the backward statistics of the BatchNorm + ReLU that
    produced the conv's input: y [B,H,W,Cs] is that BatchNorm's input (bf16), mean / rstd its batch statistics,
    gamma / beta its affine parameters.  -> (dx, part), part = f32 [ceil(B*H*W/64)][2][Cs] partial sums of g
    and g*xhat (g = dx * relu mask) for bn_bwd(part=...), summed by the GEMM epilogue (SV_EPI_STORE_BN_BWD)
    or, for split-K shapes, by the finish that reads the slabs anyway (sv_gemm_slab_finish_bn_bwd): no
    statistics pass over dx and y.  ``unsplit=False`` fuses the split-K shapes only.  Stride 2 (even H, W,
    no split): the one-launch parity-class GEMM with the same epilogue, 4 * ceil(B*H*W/256) partial rows
    (one run per class).  None when the shape is not on these paths (odd stride-2 grids, split stride-2
    shapes, fp32, unaligned parameters): use conv_bwd_data + bn_bwd.  ``out`` / ``part`` / ``work``: dx, the partials
    and the split-K slab space (default: fresh allocations)."""
    if wp.dtype != torch.bfloat16 or y.dtype != torch.bfloat16 or s.Cs % 8 or s.stride not in (1, 2):
        return None
    M = s.B * s.H * s.W
    T = s.KH * s.KW
    pw = _pointwise(s, wp.dtype)
    s2 = s.stride == 2
    if s2:  # the one-launch parity-class GEMM without a split; partials [4][ceil(M/4/64)][2][Cs]
        if not (_s2_direct(s) and T > 1 and _is_pow2(s.Cout) and s.Cout >= 32
                and _s2_split(s, M, T) == 1):
            return None
        split = 1
    elif pw:
        split = _conv_split(M, s.Cs, s.Cout)
    elif _is_pow2(s.Cout) and s.Cout >= 32 and (T * s.Cout) % 32 == 0:
        split = _conv_split(M, s.Cs, T * s.Cout)
    else:
        return None
    if split < 2 and not unsplit:
        return None
    OH, OW = conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)
    _check(dy.is_contiguous() and tuple(dy.shape) == (s.B, OH, OW, s.Cout) and dy.dtype == wp.dtype,
           "conv_bwd_data_bn: dy must be contiguous [B,OH,OW,Cout] bf16")
    _check(y.is_contiguous() and y.numel() == M * s.Cs, "conv_bwd_data_bn: y shape")
    prm = [p_.detach() for p_ in (mean, rstd, gamma, beta)]
    if not _al16(y, *prm) or any(p_.dtype != torch.float32 or not p_.is_contiguous() for p_ in prm):
        return None
    ref = nv.BnRef(ptr(prm[0]), ptr(prm[1]), ptr(prm[2]), ptr(prm[3]))
    dx = (torch.empty(s.B, s.H, s.W, s.Cs, device=dy.device, dtype=torch.bfloat16) if out is None
          else _conv_buf(out, (s.B, s.H, s.W, s.Cs), torch.bfloat16, dy.device, "conv_bwd_data_bn: out"))
    prows = 4 * ((M // 4 + 63) // 64) if s2 else (M + 63) // 64
    part = (torch.empty(prows, 2, s.Cs, device=dy.device, dtype=torch.float32) if part is None
            else _conv_buf(part, (prows, 2, s.Cs), torch.float32, dy.device, "conv_bwd_data_bn: part"))
    if split == 1:
        work = None
    elif work is None:
        work = torch.empty(split * M * s.Cs, device=dy.device, dtype=torch.float32)
    else:
        work = _conv_work(work, split * M * s.Cs, dy.device, "conv_bwd_data_bn")[:split * M * s.Cs]
    if pw and split > 1:
        linear_dgrad(dy.view(M, s.Cout), wp.view(s.Cout, s.Cs), out=work, epilogue=nv.SV_EPI_SLAB, split_k=split,
                     policy=policy)
        call("sv_gemm_slab_finish_bn_bwd", ptr(work), split, M, s.Cs, ptr(dx), ptr(y), ctypes.byref(ref), ptr(part))
    elif pw:
        linear_dgrad(dy.view(M, s.Cout), wp.view(s.Cout, s.Cs), out=dx.view(M, s.Cs), out2=part,
                     epilogue=nv.SV_EPI_STORE_BN_BWD, aux=y.view(M, s.Cs), bn=ref, policy=policy)
    else:
        call("sv_conv_bwd_data_bn", ptr(dy), ptr(wp), ptr(dx), dt(wp), ctypes.byref(s), ptr(y), ctypes.byref(ref),
             ptr(part), ptr(work), split, nv.pol_ref(policy))
    return dx, part


def conv_bwd_weight(dy: torch.Tensor, x: torch.Tensor, s: nv.ConvShape, *, dw: torch.Tensor,
                    accumulate: bool = True, policy: "nv.GemmPolicy | None" = None,
                    work: torch.Tensor | None = None) -> torch.Tensor:
    """``work``: the split-K slab space, sv_conv_bwd_weight_work_floats(s) floats (default: a fresh allocation)"""
    OH, OW = conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)
    _conv_check_x(x, s, dy.dtype, "conv_bwd_weight")
    _check(dy.is_contiguous() and tuple(dy.shape) == (s.B, OH, OW, s.Cout), "conv_bwd_weight: dy shape")
    _check(dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == (s.Cout, s.Cin, s.KH, s.KW),
           "conv_bwd_weight: dw must be f32 [Cout,Cin,k,k]")
    if _pointwise(s, dy.dtype):
        M = s.B * s.H * s.W
        linear_wgrad(dy.view(M, s.Cout), x.view(M, s.Cs), out=dw.view(s.Cout, s.Cs), accumulate=accumulate,
                     compute_bf16=True, policy=policy)
        return dw
    nwork = value("sv_conv_bwd_weight_work_floats", ctypes.byref(s))
    work = (torch.empty(nwork, device=dy.device, dtype=torch.float32) if work is None
            else _conv_work(work, nwork, dy.device, "conv_bwd_weight"))
    call("sv_conv_bwd_weight", ptr(dy), ptr(x), ptr(work), ptr(dw), int(accumulate), dt(dy), ctypes.byref(s),
         nv.pol_ref(policy))
    return dw


# ---- grouped 3x3 convolution (ResNeXt conv2; csrc/gconv.hip) ---------------------------------------------------
# SV_GCONV=dense: the bf16 model runs its grouped convs as the dense embedding through the conv_* wrappers above
# (the A/B arm; the fp32 model always does, it is the parity path)
GCONV_DENSE = os.environ.get("SV_GCONV", "") == "dense"


def gconv_shape(B, H, W, C, groups, k=3, stride=1, pad=1) -> nv.GConvShape:
    """sv_gconv_shape of a grouped k x k conv with C_in = C_out = C; raises for a shape csrc/gconv.hip does not take."""
    _check(groups > 0 and C % groups == 0 and C % 32 == 0 and C // groups in (4, 8, 16, 32) and k == 3 and pad == 1
           and stride in (1, 2) and B > 0 and H > 0 and W > 0,
           f"gconv: unsupported shape C={C} groups={groups} k={k} stride={stride} pad={pad} "
           "(3x3, pad 1, stride 1|2, C % 32 == 0, C / groups in {4, 8, 16, 32})")
    return nv.GConvShape(B, H, W, C, groups, k, k, stride, pad)


def _gconv_out_hw(s: nv.GConvShape) -> tuple[int, int]:
    return conv_out_hw(s.H, s.W, s.KH, s.stride, s.pad)


def gconv_weight_pack(ws: list, groups: int | list) -> list:
    """Packed forms of grouped weights [C][C/groups][3][3] f32, one launch per SV_MAX_GPACK_SEGS weights
    (sv_gconv_weight_pack) -> per weight a bf16 tensor [2][C/32][9][2][64][8]: [0] the forward form, [1] the
    backward-data form (taps flipped, group blocks transposed)."""
    gs = list(groups) if isinstance(groups, (list, tuple)) else [groups] * len(ws)
    out = []
    for i in range(0, len(ws), nv.SV_MAX_GPACK_SEGS):
        chunk = list(zip(ws[i:i + nv.SV_MAX_GPACK_SEGS], gs[i:i + nv.SV_MAX_GPACK_SEGS]))
        segs = (nv.GConvPackSeg * len(chunk))()
        for j, (w, g) in enumerate(chunk):
            _check(w.dim() == 4 and w.dtype == torch.float32 and w.is_contiguous(),
                   "gconv_weight_pack: need contiguous f32 [C,C/groups,k,k]")
            C, Cg, KH, KW = w.shape
            _check(KH == KW and g > 0 and Cg * g == C, "gconv_weight_pack: weight shape does not match groups")
            gconv_shape(1, KH, KW, C, g, KH, 1, 1)
            wp = torch.empty(2, C // 32, 9, 2, 64, 8, device=w.device, dtype=torch.bfloat16)
            segs[j] = nv.GConvPackSeg(ptr(w), ptr(wp[0]), ptr(wp[1]), C, g)
            out.append(wp)
        call("sv_gconv_weight_pack", segs, len(chunk))
    return out


def _gconv_check(t: torch.Tensor, shape: tuple, who: str, what: str) -> None:
    _check(t.is_contiguous() and tuple(t.shape) == shape and t.dtype == torch.bfloat16 and t.data_ptr() % 16 == 0,
           f"{who}: {what} must be contiguous 16-byte aligned bf16 {shape}, got {tuple(t.shape)} {t.dtype}")


def _gconv_check_wp(wp: torch.Tensor, s: nv.GConvShape, who: str) -> None:
    _check(tuple(wp.shape) == (2, s.C // 32, 9, 2, 64, 8) and wp.dtype == torch.bfloat16 and wp.is_contiguous(),
           f"{who}: packed weight must be gconv_weight_pack's [2][C/32][9][2][64][8] bf16")


def gconv_fwd(x: torch.Tensor, wp: torch.Tensor, s: nv.GConvShape) -> torch.Tensor:
    """y = grouped conv(x) over NHWC bf16 (f32 accumulation)."""
    OH, OW = _gconv_out_hw(s)
    _gconv_check(x, (s.B, s.H, s.W, s.C), "gconv_fwd", "x")
    _gconv_check_wp(wp, s, "gconv_fwd")
    y = torch.empty(s.B, OH, OW, s.C, device=x.device, dtype=torch.bfloat16)
    _timed_call("gconv", 2.0 * (x.numel() + y.numel()), "sv_gconv_fwd", ptr(x), ptr(wp[0]), ptr(y), ctypes.byref(s))
    return y


def gconv_bwd_data(dy: torch.Tensor, wp: torch.Tensor, s: nv.GConvShape) -> torch.Tensor:
    """dx = the grouped conv's data gradient (bf16, a fresh buffer)."""
    OH, OW = _gconv_out_hw(s)
    _gconv_check(dy, (s.B, OH, OW, s.C), "gconv_bwd_data", "dy")
    _gconv_check_wp(wp, s, "gconv_bwd_data")
    dx = torch.empty(s.B, s.H, s.W, s.C, device=dy.device, dtype=torch.bfloat16)
    _timed_call("gconv", 2.0 * (dx.numel() + dy.numel()), "sv_gconv_bwd_data", ptr(dy), ptr(wp[1]), ptr(dx),
                ctypes.byref(s))
    return dx


def gconv_bwd_weight(dy: torch.Tensor, x: torch.Tensor, s: nv.GConvShape, *, dw: torch.Tensor,
                     accumulate: bool = True) -> torch.Tensor:
    """dw (+)= the grouped conv's weight gradient, torch layout [C][C/groups][3][3] f32."""
    OH, OW = _gconv_out_hw(s)
    _gconv_check(x, (s.B, s.H, s.W, s.C), "gconv_bwd_weight", "x")
    _gconv_check(dy, (s.B, OH, OW, s.C), "gconv_bwd_weight", "dy")
    _check(dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == (s.C, s.C // s.groups, 3, 3),
           "gconv_bwd_weight: dw must be f32 [C,C/groups,3,3]")
    nwork = value("sv_gconv_bwd_weight_work_floats", ctypes.byref(s))
    work = torch.empty(nwork, device=dy.device, dtype=torch.float32)
    _timed_call("gconv", 2.0 * (x.numel() + dy.numel()) + 8.0 * nwork, "sv_gconv_bwd_weight", ptr(dy), ptr(x),
                ptr(work), ptr(dw), int(accumulate), ctypes.byref(s))
    return dw


def grouped_as_dense(w: torch.Tensor, groups: int | None = None) -> torch.Tensor:
    """A grouped weight [C][Cg][k][k] embedded block-diagonally in the dense [C][C][k][k] weight of the same
    convolution (zeros across groups): the fp32 parity path of grouped convs and the SV_GCONV=dense arm run it through
    conv_fwd / conv_bwd_data / conv_bwd_weight."""
    C, Cg = w.shape[0], w.shape[1]
    g = C // Cg if groups is None else groups
    _check(g * Cg == C, "grouped_as_dense: weight shape does not match groups")
    dense = w.new_zeros(g, Cg, g, Cg, *w.shape[2:])
    idx = torch.arange(g, device=w.device)
    dense[idx, :, idx] = w.reshape(g, Cg, Cg, *w.shape[2:])
    return dense.view(C, C, *w.shape[2:])


def dense_group_blocks(dense: torch.Tensor, groups: int) -> torch.Tensor:
    """The in-group blocks [C][C/groups][k][k] of a dense [C][C][k][k] weight (gradient): grouped_as_dense's inverse."""
    C = dense.shape[0]
    Cg = C // groups
    _check(groups * Cg == C and dense.shape[1] == C, "dense_group_blocks: shape does not match groups")
    idx = torch.arange(groups, device=dense.device)
    v = dense.reshape(groups, Cg, groups, Cg, *dense.shape[2:])
    return v[idx, :, idx].reshape(C, Cg, *dense.shape[2:]).contiguous()


def image_u8_hwc_to_nhwc(img_u8: torch.Tensor, Cs: int, dtype: torch.dtype, *, mean=IMAGENET_MEAN,
                         std=IMAGENET_STD) -> torch.Tensor:
    """Device form of the classification transform tail (row f1): collated uint8 crops [B,H,W,3]
    (reference construct_3channel, training/datasets/classification.py:40-68) -> ToTensor -> Normalize
    -> the ResNet stem operand NHWC [B,H,W,Cs] (channels >= 3 zero)."""
    _check(img_u8.dtype == torch.uint8 and img_u8.dim() == 4 and img_u8.shape[-1] == 3 and img_u8.is_contiguous(),
           "image_u8_hwc_to_nhwc: expects contiguous uint8 [B,H,W,3]")
    B, H, W, _ = img_u8.shape
    _check((B * H * W) % 4 == 0, "image_u8_hwc_to_nhwc: B*H*W must be a multiple of 4")
    out = torch.empty(B, H, W, Cs, device=img_u8.device, dtype=dtype)
    call("sv_image_u8_hwc_to_nhwc", ptr(img_u8), _host3(mean), _host3(std), ptr(out), dt(out), B, H, W, Cs)
    return out


def image_to_nhwc(img: torch.Tensor, Cs: int, dtype: torch.dtype) -> torch.Tensor:
    B, C, H, W = img.shape
    _check(img.dtype == torch.float32 and img.is_contiguous() and Cs >= C, "image_to_nhwc: need contiguous f32 NCHW")
    out = torch.empty(B, H, W, Cs, device=img.device, dtype=dtype)
    call("sv_image_to_nhwc", ptr(img), ptr(out), dt(out), B, C, H, W, Cs)
    return out


def _bn_c_ok(C: int) -> bool:
    return C >= 4 and C % 4 == 0 and (C // 4 <= 256 or (C // 4) % 256 == 0)


# The caller's ``out=`` / ``part=`` / ``sums=`` buffers of the BatchNorm and pooling wrappers are checked with _conv_buf;
# without one, each wrapper evaluates the same torch.empty expression as before
def _bn_stat_out(out, C: int, device, who: str) -> tuple:
    return tuple(_conv_buf(t, (C,), torch.float32, device, f"{who}: out") for t in out)


def bn_stats(y2d: torch.Tensor, *, eps: float = EPS_BN, momentum: float = 0.1, running_mean=None, running_var=None,
             num_batches_tracked=None, out: tuple | None = None, part: torch.Tensor | None = None):
    """Train-mode batch statistics of y [rows, C] -> (mean, rstd) f32; running stats (and the int64
    num_batches_tracked counter) updated in place on the device.  ``out`` / ``part``: the caller's (mean, rstd) and
    partials [sv_bn_nparts][2][C] buffers (default: fresh allocations)."""
    rows, C = y2d.shape
    _check(_bn_c_ok(C) and y2d.is_contiguous() and rows > 0, f"bn_stats: unsupported C={C}")
    P = value("sv_bn_nparts", rows, C)
    part = (torch.empty(P, 2, C, device=y2d.device, dtype=torch.float32) if part is None
            else _conv_buf(part, (P, 2, C), torch.float32, y2d.device, "bn_stats: part"))
    call("sv_bn_stats", ptr(y2d), dt(y2d), rows, C, ptr(part))
    if out is None:
        mean = torch.empty(C, device=y2d.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
    else:
        mean, rstd = _bn_stat_out(out, C, y2d.device, "bn_stats")
    _fin("sv_bn_stats_finish", ptr(y2d), dt(y2d), ptr(part), P, rows, C, float(eps), float(momentum), ptr(mean),
         ptr(rstd), ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), *_fin_ws(part.device))
    return mean, rstd


def bn_eval_params(running_mean: torch.Tensor, running_var: torch.Tensor, eps: float = EPS_BN,
                   out: tuple | None = None):
    C = running_mean.numel()
    if out is None:
        mean = torch.empty(C, device=running_mean.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
    else:
        mean, rstd = _bn_stat_out(out, C, running_mean.device, "bn_eval_params")
    call("sv_bn_eval_params", ptr(running_mean), ptr(running_var), float(eps), ptr(mean), ptr(rstd), C)
    return mean, rstd


def bn_act(y2d, mean, rstd, gamma, beta, *, res=None, res_bn=None, relu=True, out_dtype=torch.float32,
           out=None) -> torch.Tensor:
    """act(gamma (y-mean) rstd + beta + r), r = res or BN(res) with res_bn = (mean, rstd, gamma, beta)."""
    rows, C = y2d.shape
    _check(C % 4 == 0 and y2d.is_contiguous(), "bn_act: C must be a multiple of 4")
    if res is not None:
        _check(res.is_contiguous() and res.numel() == rows * C, "bn_act: residual shape")
    rm, rr, rg, rb = res_bn if res_bn is not None else (None, None, None, None)
    if out is None:
        out = torch.empty(rows, C, device=y2d.device, dtype=out_dtype)
    _fin("sv_bn_act_fwd", ptr(y2d), dt(y2d), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(res),
         nv.dt_none(res), ptr(rm), ptr(rr), ptr(rg), ptr(rb), int(relu), ptr(out), dt(out), rows, C)
    return out


# One launch per BatchNorm where the rows are few (sv_bn_*_small: ResNet layers 3-4 at 256 px), bit for bit the
# multi-launch path.  Opt-in (SV_BN_SMALL=1): measured slower (classification 3524-3542 vs 3779-3806 img/s
# interleaved, profiles/round4/r8c_bn_small_ab.txt).  A workgroup that owns 8 channels over all rows reads 16 B per
# row, one cache line per lane, so it streams at the L1's line rate: layer3's output BatchNorm backward took 86 us
# in one launch against ~45 us in three; at layer4 the two forms are equal (r8d trace)
_BN_SMALL = os.environ.get("SV_BN_SMALL", "0") != "0"
_SMALL_OK: dict = {}


def bn_small_ok(rows: int, C: int) -> bool:
    """Whether (rows, C) has the one-launch BatchNorm geometry (sv_bn_small_ok)."""
    key = (rows, C)
    ok = _SMALL_OK.get(key)
    if ok is None:
        ok = _SMALL_OK[key] = bool(value("sv_bn_small_ok", rows, C))
    return _BN_SMALL and ok


def _bn_small_args_ok(*ts) -> bool:
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in ts)


# The statistics fold inside the consuming pass (sv_bn_act_fold / sv_bn_bwd_apply_fold): one launch fewer per
# BatchNorm, bit for bit the separate fold.  Opt-in (SV_BN_FOLD=1): measured slower -- classification 2713-2718 vs
# 4076-4093 img/s with up to 2048 workgroups (their ticket / exit atomics on one counter serialise), and a graph-timed
# launch at 256 workgroups still 1.1-2.2x the separate finish + activation (profiles/round5/r11e_fold_bench.txt):
# the fold's round trips sit in front of every workgroup's first load.  The separate fold's chunks run in parallel
# workgroups instead (_fin_ws).
_BN_FOLD = os.environ.get("SV_BN_FOLD", "0") != "0"
_FOLD_OK: dict = {}
_FOLD_WS: dict = {}


def _fin_ws(device) -> tuple:
    """(ctl, ws) pointers for a separate fold launch on the current stream: its chunks of 1024 partials then fold in
    parallel workgroups (sv_bn_stats_finish / sv_bn_bwd_finish; same bits)."""
    ctl, ws = _fold_ws(device)
    return ptr(ctl), ptr(ws)


def bn_fold_ok(rows: int, C: int, nparts: int) -> bool:
    """Whether (rows, C, nparts) has the fold kernels' geometry (sv_bn_fold_ok), and SV_BN_FOLD is on."""
    key = (rows, C, nparts)
    ok = _FOLD_OK.get(key)
    if ok is None:
        ok = _FOLD_OK[key] = bool(value("sv_bn_fold_ok", rows, C, nparts))
    return _BN_FOLD and ok


def _fold_ws(device):
    """(ctl, ws) of the fold kernels on the current stream: the counters start zero and every launch leaves them
    zero; never reallocated (a captured graph keeps the pointers)."""
    key = (device, nv._stream())
    t = _FOLD_WS.get(key)
    if t is None:
        t = _FOLD_WS[key] = (torch.zeros(nv.SV_BN_FOLD_CTL_INTS, device=device, dtype=torch.int32),
                             torch.empty(nv.SV_BN_FOLD_WS_FLOATS, device=device, dtype=torch.float32))
    return t


def bn_fold_timeouts(device) -> int:
    """Fold-kernel polls that timed out on any stream of ``device`` since the workspaces were made (0 expected)."""
    return sum(int(ctl[3].item()) for (d, _), (ctl, _) in _FOLD_WS.items() if d == device)


def _bn_act_args(y2d, part, bn_params, res, res_part, res_params, relu, out_dtype) -> tuple:
    """The outputs and the marshalled arguments that sv_bn_act_small and sv_bn_act_fold share (the fold appends its
    workspace) -> (args, (out, mean, rstd[, mean2, rstd2])); without ``res_part`` the shortcut's operands are NULL / 0."""
    rows, C = y2d.shape
    g, b, eps, mom, rm, rv, nbt = bn_params
    dev = y2d.device
    mean = torch.empty(C, device=dev, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    out = torch.empty(rows, C, device=dev, dtype=out_dtype)
    if res_part is not None:
        g2, b2, eps2, mom2, rm2, rv2, nbt2 = res_params
        mean2, rstd2 = torch.empty_like(mean), torch.empty_like(mean)
    else:
        g2 = b2 = rm2 = rv2 = nbt2 = mean2 = rstd2 = None
        eps2, mom2 = 0.0, 0.0
    args = (ptr(y2d), dt(y2d), ptr(part), part.shape[0], float(eps), float(mom), ptr(g), ptr(b), ptr(mean), ptr(rstd),
            ptr(rm), ptr(rv), ptr(nbt), ptr(res), nv.dt_none(res), ptr(res_part),
            res_part.shape[0] if res_part is not None else 0, float(eps2), float(mom2), ptr(g2), ptr(b2), ptr(mean2),
            ptr(rstd2), ptr(rm2), ptr(rv2), ptr(nbt2), int(relu), ptr(out), dt(out), rows, C)
    return args, ((out, mean, rstd, mean2, rstd2) if res_part is not None else (out, mean, rstd))


def bn_act_fold(y2d, part, bn_params: tuple, *, res=None, res_part=None, res_params: tuple | None = None,
                relu=True, out_dtype=torch.float32):
    """bn_act_small's contract at any row count the fold kernels take (bn_fold_ok): the statistics fold of the conv
    epilogue's partials inside the activation pass (sv_bn_act_fold) -- bit for bit ``bn_stats_from_partials`` +
    ``bn_act``.  -> (out, mean, rstd[, mean2, rstd2])."""
    args, ret = _bn_act_args(y2d, part, bn_params, res, res_part, res_params, relu, out_dtype)
    _fin("sv_bn_act_fold", *args, *_fin_ws(y2d.device))
    return ret


def bn_act_partials(y2d, part, bn_params: tuple, *, res=None, res_part=None, res_params: tuple | None = None,
                    relu=True, out_dtype=torch.float32):
    """Train-mode BatchNorm (+ residual, + ReLU) from the conv epilogue's partials with the fewest launches the shape
    allows: bn_act_small (rows <= 8192, opt-in SV_BN_SMALL), bn_act_fold, else bn_stats_from_partials + bn_act.  All
    three give the same bits.  -> (out, mean, rstd[, mean2, rstd2])."""
    rows, C = y2d.shape
    args = (y2d, part, res, res_part) + bn_params[:2] + (res_params[:2] if res_params else ())
    if bn_small_ok(rows, C) and _bn_small_args_ok(*args):
        return bn_act_small(y2d, part, bn_params, res=res, res_part=res_part, res_params=res_params, relu=relu,
                            out_dtype=out_dtype)
    if (bn_fold_ok(rows, C, part.shape[0]) and _bn_small_args_ok(*args)
            and (res_part is None or res_part.shape[0] == part.shape[0])):
        return bn_act_fold(y2d, part, bn_params, res=res, res_part=res_part, res_params=res_params, relu=relu,
                           out_dtype=out_dtype)
    g, b, eps, mom, rm, rv, nbt = bn_params
    mean, rstd = bn_stats_from_partials(part, rows, eps=eps, momentum=mom, running_mean=rm, running_var=rv,
                                        num_batches_tracked=nbt)
    res_bn = None
    if res_part is not None:
        g2, b2, eps2, mom2, rm2, rv2, nbt2 = res_params
        mean2, rstd2 = bn_stats_from_partials(res_part, rows, eps=eps2, momentum=mom2, running_mean=rm2,
                                              running_var=rv2, num_batches_tracked=nbt2)
        res_bn = (mean2, rstd2, g2, b2)
    out = bn_act(y2d, mean, rstd, g, b, res=res, res_bn=res_bn, relu=relu, out_dtype=out_dtype)
    if res_part is not None:
        return out, mean, rstd, mean2, rstd2
    return out, mean, rstd


def bn_act_small(y2d, part, bn_params: tuple, *, res=None, res_part=None, res_params: tuple | None = None,
                 relu=True, out_dtype=torch.float32):
    """Train-mode BatchNorm (+ residual, + its own ReLU) from the conv epilogue's unshifted statistics partials in
    ONE launch (sv_bn_act_small): bit for bit ``bn_stats_from_partials`` + ``bn_act``.  ``bn_params`` =
    (gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked); with ``res_part`` the residual is
    the projection shortcut's conv output and ``res_params`` its BatchNorm's.  -> (out, mean, rstd[, mean2, rstd2])."""
    args, ret = _bn_act_args(y2d, part, bn_params, res, res_part, res_params, relu, out_dtype)
    call("sv_bn_act_small", *args)
    return ret


# The two wide BatchNorm backward entry points, marshalled once each: operands a call site does not name are NULL / 0.
# ``y2 / mean2 / rstd2 / gamma2`` (the DUAL mode's second BatchNorm) make the result (dx, dx2).
def _bn_bwd_small(mode, dout, y, mean, rstd, gamma, *, dx_dtype, batch_stats, act=None, beta=None, y2=None, mean2=None,
                  rstd2=None, gamma2=None, part=None, dgamma=None, dbeta=None, dgamma2=None, dbeta2=None, out=None,
                  out2=None):
    """The whole BatchNorm backward in one launch (sv_bn_bwd_small); ``part``: statistics partials already summed."""
    rows, C = y.shape
    dx = (torch.empty(rows, C, device=y.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (rows, C), dx_dtype, y.device, "bn_bwd: out"))
    dx2 = None
    if y2 is not None:
        dx2 = (torch.empty_like(dx) if out2 is None else _conv_buf(out2, (rows, C), dx_dtype, y.device, "bn_bwd: out"))
    call("sv_bn_bwd_small", mode, ptr(dout), dt(dout), ptr(act), nv.dt_none(act), ptr(y), dt(y), ptr(mean), ptr(rstd),
         ptr(gamma), ptr(beta), ptr(y2), dt(y2) if y2 is not None else 0, ptr(mean2), ptr(rstd2), ptr(gamma2),
         ptr(part), part.shape[0] if part is not None else 0, ptr(dx), ptr(dx2), dt(dx), ptr(dgamma), ptr(dbeta),
         ptr(dgamma2), ptr(dbeta2), int(batch_stats), rows, C)
    return dx if y2 is None else (dx, dx2)


def _bn_bwd_apply_fold(mode, dout, y, mean, rstd, gamma, part, P, *, dx_dtype, batch_stats, idx=None, H=0, W=0,
                       beta=None, y2=None, mean2=None, rstd2=None, gamma2=None, part2=None, dgamma=None, dbeta=None,
                       dgamma2=None, dbeta2=None, out=None, out2=None):
    """The statistics finish inside the apply pass (sv_bn_bwd_apply_fold); ``idx / H / W``: dout is a max-pool's
    output gradient, gathered through the pool's indices."""
    rows, C = y.shape
    dx = (torch.empty(rows, C, device=y.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (rows, C), dx_dtype, y.device, "bn_bwd: out"))
    dx2 = None
    if y2 is not None:
        dx2 = (torch.empty_like(dx) if out2 is None else _conv_buf(out2, (rows, C), dx_dtype, y.device, "bn_bwd: out"))
    _fin("sv_bn_bwd_apply_fold", mode, ptr(dout), dt(dout), ptr(idx), H, W, ptr(y), dt(y), ptr(mean), ptr(rstd),
         ptr(gamma), ptr(beta), ptr(y2), dt(y2) if y2 is not None else 0, ptr(mean2), ptr(rstd2), ptr(gamma2),
         ptr(part), ptr(part2), P, ptr(dx), ptr(dx2), dt(dx), ptr(dgamma), ptr(dbeta), ptr(dgamma2), ptr(dbeta2),
         int(batch_stats), rows, C, *_fin_ws(y.device))
    return dx if y2 is None else (dx, dx2)


def _bn_bwd_sums(P: int, C: int, batch_stats: bool, *folds, sums: torch.Tensor | None = None) -> torch.Tensor:
    """The separate finish: one sv_bn_bwd_finish per (part, dgamma, dbeta) of ``folds`` into ONE buffer -> sums
    [len(folds)][2][C] for the apply pass (dgamma / dbeta accumulate); eval mode zeroes it with one launch."""
    dev = folds[0][0].device
    sums = (torch.empty(len(folds), 2, C, device=dev, dtype=torch.float32) if sums is None
            else _conv_buf(sums, (len(folds), 2, C), torch.float32, dev, "bn_bwd: sums"))
    ws = _fin_ws(dev)
    for i, (part, dgamma, dbeta) in enumerate(folds):  # into sums[i] (2 * C floats each), without a view per fold
        _fin("sv_bn_bwd_finish", ptr(part), P, C, ptr(sums) + i * 8 * C, ptr(dgamma), ptr(dbeta), *ws)
    if not batch_stats:
        sums.zero_()
    return sums


def bn_bwd(dout2d, y2d, mean, rstd, gamma, *, act=None, relu_beta=None, dgamma=None, dbeta=None,
           dx_dtype=torch.float32, gmask=None, mask_inplace: bool = False, batch_stats: bool = True,
           part: torch.Tensor | None = None, out: torch.Tensor | None = None, work: torch.Tensor | None = None,
           sums: torch.Tensor | None = None) -> torch.Tensor:
    """BatchNorm backward with an optional ReLU mask on dout; dgamma/dbeta accumulate.  The mask is
    act > 0, or -- ``relu_beta`` = the BN's beta, for a BN followed by its own ReLU -- recomputed from y
    like the forward's pre-activation (sv_bn_relu_bwd_*: the activation is not read again).
    ``mask_inplace`` (act form, f32 or bf16 dout): the statistics pass overwrites dout with the masked gradient
    (sv_bn_bwd_stats_mask), which the apply pass then reads without the mask and the caller keeps as the
    shortcut's gradient; ``gmask`` instead writes it to a separate f32 buffer from the apply pass.
    ``batch_stats``: train mode (mean / rstd are the batch's own, so dx carries the two mean corrections);
    False: eval mode (running statistics, an affine map: dx = gamma * rstd * dout, the apply kernel reading
    zero correction sums).
    ``part`` (relu_beta form): the backward statistics' partials [P][2][C] already summed by the producer of
    dout (conv_bwd_data_bn), so the statistics pass is skipped.
    ``out`` / ``work`` / ``sums``: the caller's dx, statistics partials [sv_bn_nparts][2][C] (where ``part`` is not
    given) and folded sums [1][2][C] buffers (default: fresh allocations)."""
    rows, C = y2d.shape
    _check(_bn_c_ok(C) and dout2d.numel() == rows * C and dout2d.is_contiguous(), "bn_bwd: bad shapes")
    _check(act is None or relu_beta is None, "bn_bwd: act and relu_beta are exclusive")
    if act is not None:
        _check(act.numel() == rows * C and act.is_contiguous(), "bn_bwd: act shape")
    if gmask is not None:
        _check(gmask.dtype == torch.float32 and gmask.numel() == rows * C and relu_beta is None,
               "bn_bwd: gmask must be f32 [rows,C] (act-mask form only)")
    if mask_inplace:
        _check(act is not None and gmask is None and dout2d.dtype in (torch.float32, torch.bfloat16),
               "bn_bwd: mask_inplace needs act, an f32 / bf16 dout and no gmask")
    if part is not None:
        _check(relu_beta is not None and part.dtype == torch.float32 and part.is_contiguous() and part.dim() == 3
               and tuple(part.shape[1:]) == (2, C), "bn_bwd: part must be f32 [P][2][C] (relu_beta form)")
    small_mode = (nv.SV_BN_SMALL_RELU if relu_beta is not None else nv.SV_BN_SMALL_MASK if mask_inplace else None)
    if (small_mode is not None and gmask is None and bn_small_ok(rows, C)
            and _bn_small_args_ok(dout2d, y2d, mean, rstd, gamma, act, relu_beta, part, dgamma, dbeta)):
        return _bn_bwd_small(small_mode, dout2d, y2d, mean, rstd, gamma, act=act, beta=relu_beta, part=part,
                             dgamma=dgamma, dbeta=dbeta, dx_dtype=dx_dtype, batch_stats=batch_stats, out=out)
    if part is not None:  # summed by dout's producer (conv_bwd_data_bn)
        P = part.shape[0]
    else:
        P = value("sv_bn_nparts", rows, C)
        part = (torch.empty(P, 2, C, device=y2d.device, dtype=torch.float32) if work is None
                else _conv_buf(work, (P, 2, C), torch.float32, y2d.device, "bn_bwd: work"))
        if relu_beta is not None:
            call("sv_bn_relu_bwd_stats", ptr(dout2d), dt(dout2d), ptr(y2d), dt(y2d), ptr(mean), ptr(rstd), ptr(gamma),
                 ptr(relu_beta), rows, C, ptr(part))
        elif mask_inplace:
            call("sv_bn_bwd_stats_mask", ptr(dout2d), dt(dout2d), ptr(act), dt(act), ptr(y2d), dt(y2d), ptr(mean),
                 ptr(rstd), rows, C, ptr(part))
            act = None  # dout now holds the masked gradient
        else:
            call("sv_bn_bwd_stats", ptr(dout2d), dt(dout2d), ptr(act), nv.dt_none(act), ptr(y2d), dt(y2d), ptr(mean),
                 ptr(rstd), rows, C, ptr(part))
    if ((relu_beta is not None or act is None) and gmask is None and bn_fold_ok(rows, C, P)
            and _bn_small_args_ok(dout2d, y2d, mean, rstd, gamma, relu_beta, part)):
        # MASK = dout already masked (mask_inplace)
        mode = nv.SV_BN_SMALL_RELU if relu_beta is not None else nv.SV_BN_SMALL_MASK
        return _bn_bwd_apply_fold(mode, dout2d, y2d, mean, rstd, gamma, part, P, beta=relu_beta, dgamma=dgamma,
                                  dbeta=dbeta, dx_dtype=dx_dtype, batch_stats=batch_stats, out=out)
    sums = _bn_bwd_sums(P, C, batch_stats, (part, dgamma, dbeta), sums=sums)
    dx = (torch.empty(rows, C, device=y2d.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (rows, C), dx_dtype, y2d.device, "bn_bwd: out"))
    if relu_beta is not None:
        call("sv_bn_relu_bwd_apply", ptr(dout2d), dt(dout2d), ptr(y2d), dt(y2d), ptr(mean), ptr(rstd), ptr(gamma),
             ptr(relu_beta), ptr(sums), ptr(dx), dt(dx), rows, C)
    else:
        call("sv_bn_bwd_apply", ptr(dout2d), dt(dout2d), ptr(act), nv.dt_none(act), ptr(y2d), dt(y2d), ptr(mean),
             ptr(rstd), ptr(gamma), ptr(sums), ptr(dx), dt(dx), ptr(gmask), rows, C)
    return dx


def bn_bwd_dual(gm, y2d, mean, rstd, gamma, act, y2, mean2, rstd2, gamma2, *, dgamma=None, dbeta=None,
                dgamma2=None, dbeta2=None, dx_dtype=torch.float32, batch_stats: bool = True,
                out: tuple | None = None, part: torch.Tensor | None = None, sums: torch.Tensor | None = None):
    """A projection-shortcut block's two output BatchNorms from one masked gradient: equals
    ``bn_bwd(gm, y2d, ..., act=act, mask_inplace=True)`` followed by ``bn_bwd(gm, y2, mean2, rstd2, gamma2)``
    bit for bit (gm, f32 or bf16, is overwritten with the masked gradient the same way), with gm read once per pass
    instead of twice (sv_bn_bwd_stats_mask_dual / sv_bn_bwd_apply_dual). -> (dx, dx2).
    ``out`` / ``part`` / ``sums``: the caller's (dx, dx2), partials [2][sv_bn_nparts][2][C] and folded sums [2][2][C]
    buffers (default: fresh allocations)."""
    rows, C = y2d.shape
    _check(_bn_c_ok(C) and gm.dtype in (torch.float32, torch.bfloat16) and gm.numel() == rows * C and gm.is_contiguous()
           and act.numel() == rows * C and act.is_contiguous() and y2.numel() == rows * C and y2.is_contiguous(),
           "bn_bwd_dual: bad shapes")
    both = dict(y2=y2, mean2=mean2, rstd2=rstd2, gamma2=gamma2, dgamma=dgamma, dbeta=dbeta, dgamma2=dgamma2,
                dbeta2=dbeta2, dx_dtype=dx_dtype, batch_stats=batch_stats)
    o1, o2 = out if out is not None else (None, None)
    if bn_small_ok(rows, C) and _bn_small_args_ok(gm, y2d, mean, rstd, gamma, act, y2, mean2, rstd2, gamma2, dgamma,
                                                   dbeta, dgamma2, dbeta2):
        return _bn_bwd_small(nv.SV_BN_SMALL_DUAL, gm, y2d, mean, rstd, gamma, act=act, out=o1, out2=o2, **both)
    P = value("sv_bn_nparts", rows, C)
    part = (torch.empty(2, P, 2, C, device=y2d.device, dtype=torch.float32) if part is None
            else _conv_buf(part, (2, P, 2, C), torch.float32, y2d.device, "bn_bwd_dual: part"))
    call("sv_bn_bwd_stats_mask_dual", ptr(gm), dt(gm), ptr(act), dt(act), ptr(y2d), dt(y2d), ptr(mean), ptr(rstd),
         ptr(y2), dt(y2), ptr(mean2), ptr(rstd2), rows, C, ptr(part[0]), ptr(part[1]))
    if bn_fold_ok(rows, C, P) and _bn_small_args_ok(gm, y2d, mean, rstd, gamma, y2, mean2, rstd2, gamma2):
        return _bn_bwd_apply_fold(nv.SV_BN_SMALL_DUAL, gm, y2d, mean, rstd, gamma, part[0], P, part2=part[1], out=o1,
                                  out2=o2, **both)
    sums = _bn_bwd_sums(P, C, batch_stats, (part[0], dgamma, dbeta), (part[1], dgamma2, dbeta2), sums=sums)
    dx = (torch.empty(rows, C, device=y2d.device, dtype=dx_dtype) if o1 is None
          else _conv_buf(o1, (rows, C), dx_dtype, y2d.device, "bn_bwd_dual: out"))
    dx2 = (torch.empty(rows, C, device=y2d.device, dtype=dx_dtype) if o2 is None
           else _conv_buf(o2, (rows, C), dx_dtype, y2d.device, "bn_bwd_dual: out"))
    call("sv_bn_bwd_apply_dual", ptr(gm), dt(gm), ptr(y2d), dt(y2d), ptr(mean), ptr(rstd), ptr(gamma), ptr(sums[0]),
         ptr(y2), dt(y2), ptr(mean2), ptr(rstd2), ptr(gamma2), ptr(sums[1]), ptr(dx), ptr(dx2), dt(dx), rows, C)
    return dx, dx2


def bn_relu_bwd_pooled(dpool4d: torch.Tensor, idx: torch.Tensor, H: int, W: int, y2d, mean, rstd, gamma, beta, *,
                       dgamma=None, dbeta=None, dx_dtype=torch.float32, batch_stats: bool = True,
                       out: torch.Tensor | None = None, part: torch.Tensor | None = None,
                       sums: torch.Tensor | None = None) -> torch.Tensor:
    """bn_bwd(maxpool_bwd(dpool, idx, H, W), y, ..., relu_beta=beta) without materialising the max-pool
    backward: both BatchNorm passes gather it from dpool / idx (sv_bn_relu_bwd_*_pool), bit for bit.
    ``out`` / ``part`` / ``sums``: the caller's dx, partials and folded sums [1][2][C] buffers (default: fresh)."""
    B, OH, OW, C = dpool4d.shape
    rows = y2d.shape[0]
    _check(dpool4d.dtype in (torch.float32, torch.bfloat16) and dpool4d.is_contiguous() and idx.shape == dpool4d.shape
           and idx.is_contiguous() and (OH, OW) == conv_out_hw(H, W, 3, 2, 1) and rows == B * H * W
           and y2d.shape[1] == C and _bn_c_ok(C), "bn_relu_bwd_pooled: shape mismatch")
    P = value("sv_bn_nparts", rows, C)
    part = (torch.empty(P, 2, C, device=y2d.device, dtype=torch.float32) if part is None
            else _conv_buf(part, (P, 2, C), torch.float32, y2d.device, "bn_relu_bwd_pooled: part"))
    call("sv_bn_relu_bwd_stats_pool", ptr(dpool4d), dt(dpool4d), ptr(idx), B, H, W, ptr(y2d), dt(y2d), ptr(mean),
         ptr(rstd), ptr(gamma), ptr(beta), C, ptr(part))
    if (bn_fold_ok(rows, C, P) and rows * C < 2 ** 31
            and _bn_small_args_ok(dpool4d, y2d, mean, rstd, gamma, beta)):
        return _bn_bwd_apply_fold(nv.SV_BN_SMALL_RELU, dpool4d, y2d, mean, rstd, gamma, part, P, idx=idx, H=H, W=W,
                                  beta=beta, dgamma=dgamma, dbeta=dbeta, dx_dtype=dx_dtype, batch_stats=batch_stats,
                                  out=out)
    sums = _bn_bwd_sums(P, C, batch_stats, (part, dgamma, dbeta), sums=sums)
    dx = (torch.empty(rows, C, device=y2d.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (rows, C), dx_dtype, y2d.device, "bn_relu_bwd_pooled: out"))
    call("sv_bn_relu_bwd_apply_pool", ptr(dpool4d), dt(dpool4d), ptr(idx), B, H, W, ptr(y2d), dt(y2d), ptr(mean),
         ptr(rstd), ptr(gamma), ptr(beta), ptr(sums), ptr(dx), dt(dx), C)
    return dx


def head_loss(logits: torch.Tensor, specs: list) -> tuple:
    """The multi-task classification loss and its logits gradient in one launch (sv_head_loss).  ``specs``: one
    (kind, offset, ncls, weight, label_smoothing, target) per task, kind nv.SV_HEAD_CE (target int64 [B]) or
    nv.SV_HEAD_BCE (target f32 / bf16 [B][ncls]).  -> (loss 0-dim f32, dlogits [B][K] f32)."""
    _check(logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous(), "head_loss: logits")
    B, Kc = logits.shape
    cover = 0
    tasks = []
    for kind, off, n, w, sm, t in specs:
        if kind == nv.SV_HEAD_CE:
            _check(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B, "head_loss: CE target int64 [B]")
        else:
            _check(t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous() and t.numel() == B * n,
                   "head_loss: BCE target f32 / bf16 [B][ncls]")
        tasks.append(nv.HeadTask(kind, off, n, float(w), float(sm), ptr(t), dt(t) if kind == nv.SV_HEAD_BCE else 0))
        cover += n
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dl = (torch.empty_like if cover == Kc else torch.zeros_like)(logits)
    call("sv_head_loss", ptr(logits), B, Kc, (nv.HeadTask * len(tasks))(*tasks), len(tasks), ptr(loss), ptr(dl))
    return loss, dl


def maxpool_fwd(x4d: torch.Tensor, *, out: tuple | None = None):
    """-> (y, idx uint8: the argmax tap 3 kh + kw); ``out``: the caller's (y, idx) buffers (default: fresh)."""
    B, H, W, C = x4d.shape
    _check(x4d.is_contiguous() and C % 4 == 0, "maxpool_fwd: need contiguous NHWC, C % 4 == 0")
    OH, OW = conv_out_hw(H, W, 3, 2, 1)
    if out is None:
        y = torch.empty(B, OH, OW, C, device=x4d.device, dtype=x4d.dtype)
        idx = torch.empty(B, OH, OW, C, device=x4d.device, dtype=torch.uint8)
    else:
        y = _conv_buf(out[0], (B, OH, OW, C), x4d.dtype, x4d.device, "maxpool_fwd: out")
        idx = _conv_buf(out[1], (B, OH, OW, C), torch.uint8, x4d.device, "maxpool_fwd: out")
    call("sv_maxpool3s2_fwd", ptr(x4d), dt(x4d), ptr(y), ptr(idx), B, H, W, C)
    return y, idx


def maxpool_bwd(dout4d: torch.Tensor, idx: torch.Tensor, H: int, W: int, dx_dtype=torch.float32, *,
                out: torch.Tensor | None = None) -> torch.Tensor:
    B, OH, OW, C = dout4d.shape
    _check(dout4d.is_contiguous() and idx.shape == dout4d.shape and (OH, OW) == conv_out_hw(H, W, 3, 2, 1),
           "maxpool_bwd: shape mismatch")
    dx = (torch.empty(B, H, W, C, device=dout4d.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (B, H, W, C), dx_dtype, dout4d.device, "maxpool_bwd: out"))
    call("sv_maxpool3s2_bwd", ptr(dout4d), dt(dout4d), ptr(idx), ptr(dx), dt(dx), B, H, W, C)
    return dx


def avgpool_fwd(x4d: torch.Tensor, *, out: torch.Tensor | None = None) -> torch.Tensor:
    B, H, W, C = x4d.shape
    _check(x4d.is_contiguous() and C % 4 == 0, "avgpool_fwd: need contiguous NHWC, C % 4 == 0")
    feat = (torch.empty(B, C, device=x4d.device, dtype=torch.float32) if out is None
            else _conv_buf(out, (B, C), torch.float32, x4d.device, "avgpool_fwd: out"))
    call("sv_avgpool_fwd", ptr(x4d), dt(x4d), ptr(feat), B, H * W, C)
    return feat


def avgpool_bwd(dfeat: torch.Tensor, shape: tuple, dx_dtype=torch.float32, *,
                out: torch.Tensor | None = None) -> torch.Tensor:
    B, H, W, C = shape
    dfeat = dfeat.float().contiguous()
    _check(tuple(dfeat.shape) == (B, C), "avgpool_bwd: dfeat shape")
    dx = (torch.empty(B, H, W, C, device=dfeat.device, dtype=dx_dtype) if out is None
          else _conv_buf(out, (B, H, W, C), dx_dtype, dfeat.device, "avgpool_bwd: out"))
    call("sv_avgpool_bwd", ptr(dfeat), ptr(dx), dt(dx), B, H * W, C)
    return dx


# ----------------------------------------------------------------------------------------------
# Squeeze-and-excitation on a bottleneck's last BatchNorm and the avg-pool shortcut (csrc/se.hip): ResNet-RS / -D
# SV_SE=torch: the same wrappers computed with torch ops on the device (A/B baseline and debugging aid, never the
# default)
SE_TORCH = os.environ.get("SV_SE", "") == "torch"


def _se_act(who: str, *ts) -> tuple:
    B, H, W, C = ts[0].shape
    _check(_is_pow2(C) and 16 <= C <= 2048, f"{who}: C must be a power of two in 16..2048, got {C}")
    for t in ts:
        _check(t.is_contiguous() and tuple(t.shape) == (B, H, W, C) and t.dtype in (torch.float32, torch.bfloat16)
               and t.data_ptr() % 16 == 0, f"{who}: need contiguous 16-B aligned f32 / bf16 [B,H,W,C]={(B, H, W, C)}")
    return B, H * W, C


def _se_f32(who: str, shape: tuple, *ts) -> None:
    for t in ts:
        _check(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == math.prod(shape)
               and t.data_ptr() % 16 == 0, f"{who}: need contiguous 16-B aligned f32 {shape}, got {tuple(t.shape)} {t.dtype}")


def _se_out(t, shape: tuple, dtype, device, who: str) -> torch.Tensor:
    """a fresh output, or the caller's ``out=`` buffer checked (as the BatchNorm wrappers' _conv_buf)"""
    return torch.empty(shape, device=device, dtype=dtype) if t is None else _conv_buf(t, shape, dtype, device, who)


def se_squeeze(y4d: torch.Tensor, *, part: torch.Tensor | None = None) -> torch.Tensor:
    """Per-image partial channel sums of the raw conv output y [B,H,W,C] -> part [B][P][C] f32 (se_excite folds them).
    ``part`` / ``out`` / ``work`` of this and the wrappers below: the caller's buffers (default: fresh allocations)."""
    B, HW, C = _se_act("se_squeeze", y4d)
    if SE_TORCH:
        return y4d.float().sum((1, 2)).view(B, 1, C)
    P = value("sv_se_nparts", HW, C)
    part = _se_out(part, (B, P, C), torch.float32, y4d.device, "se_squeeze: part")
    call("sv_se_squeeze", ptr(y4d), dt(y4d), ptr(part), B, HW, C)
    return part


def se_excite(part: torch.Tensor, HW: int, mean, rstd, gamma, beta, w1, b1, w2, b2, *, out: tuple | None = None) -> tuple:
    """-> (ymean, pooled, hidden, gate): ymean = mean_hw y from the squeeze partials, pooled = its BatchNorm (mean, rstd,
    gamma, beta), hidden = relu(w1 pooled + b1) [B][rd], gate = sigmoid(w2 hidden + b2) [B][C]; all f32."""
    B, P, C = part.shape
    rd = w1.shape[0]
    _se_f32("se_excite", (B, P, C), part)
    _se_f32("se_excite", (C,), mean, rstd, gamma, beta, b2)
    _se_f32("se_excite", (rd,), b1)
    _se_f32("se_excite", (rd, C), w1, w2)
    _check(w1.shape[:2] == (rd, C) and w2.shape[:2] == (C, rd) and rd % 4 == 0, "se_excite: w1 [rd,C,1,1], w2 [C,rd,1,1]")
    if SE_TORCH:
        ymean = part.sum(1) / HW
        pooled = (ymean - mean) * rstd * gamma + beta
        hidden = torch.relu(pooled @ w1.view(rd, C).t() + b1)
        return ymean, pooled, hidden, torch.sigmoid(hidden @ w2.view(C, rd).t() + b2)
    o = out if out is not None else (None,) * 4
    ymean, pooled, gate = (_se_out(t, (B, C), torch.float32, part.device, "se_excite: out") for t in (o[0], o[1], o[3]))
    hidden = _se_out(o[2], (B, rd), torch.float32, part.device, "se_excite: out")
    call("sv_se_excite", ptr(part), P, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
         ptr(ymean), ptr(pooled), ptr(hidden), ptr(gate), B, HW, C, rd)
    return ymean, pooled, hidden, gate


def se_join(y4d, mean, rstd, gamma, beta, gate, res, *, res_bn=None, out_dtype=torch.float32, out=None) -> torch.Tensor:
    """relu((gamma (y - mean) rstd + beta) * gate[b][c] + r), r = res or BN(res) with res_bn = (mean, rstd, gamma, beta)."""
    B, HW, C = _se_act("se_join", y4d)
    _check(res.is_contiguous() and tuple(res.shape) == tuple(y4d.shape) and res.data_ptr() % 16 == 0, "se_join: res shape")
    _se_f32("se_join", (B, C), gate)
    _se_f32("se_join", (C,), mean, rstd, gamma, beta, *(res_bn or ()))
    if SE_TORCH:
        z = ((y4d.float() - mean) * rstd * gamma + beta) * gate.view(B, 1, 1, C)
        r = res.float()
        if res_bn is not None:
            r = (r - res_bn[0]) * res_bn[1] * res_bn[2] + res_bn[3]
        return torch.relu(z + r).to(out_dtype)
    rm, rr, rg, rb = res_bn if res_bn is not None else (None, None, None, None)
    out = _se_out(out, tuple(y4d.shape), out_dtype, y4d.device, "se_join: out")
    call("sv_se_join_fwd", ptr(y4d), dt(y4d), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(gate), ptr(res), dt(res),
         ptr(rm), ptr(rr), ptr(rg), ptr(rb), ptr(out), dt(out), B, HW, C)
    return out


def se_bwd_stats(dout4d, act4d, y4d, mean, rstd, *, part: torch.Tensor | None = None) -> torch.Tensor:
    """Pass A of the backward: dout is OVERWRITTEN with g = dout * (act > 0) (the shortcut's gradient) -> part
    [B][P][2][C] f32 = per-image partial (sum g, sum g xhat)."""
    B, HW, C = _se_act("se_bwd_stats", y4d, dout4d, act4d)
    _se_f32("se_bwd_stats", (C,), mean, rstd)
    if SE_TORCH:
        g = dout4d.float() * (act4d > 0)
        dout4d.copy_(g)
        g = dout4d.float()
        xh = (y4d.float() - mean) * rstd
        return torch.stack((g.sum((1, 2)), (g * xh).sum((1, 2))), 1).view(B, 1, 2, C)
    P = value("sv_se_nparts", HW, C)
    part = _se_out(part, (B, P, 2, C), torch.float32, y4d.device, "se_bwd_stats: part")
    call("sv_se_bwd_stats", ptr(dout4d), dt(dout4d), ptr(act4d), dt(act4d), ptr(y4d), dt(y4d), ptr(mean), ptr(rstd),
         ptr(part), B, HW, C)
    return part


def se_bwd_gate(part, state: tuple, HW: int, mean, rstd, gamma, beta, w1, w2, *, dw1, db1, dw2, db2, dgamma=None,
                dbeta=None, batch_stats: bool = True, out: tuple | None = None, work: torch.Tensor | None = None) -> tuple:
    """The gate's backward from pass A's partials and the forward's ``state`` = (ymean, pooled, hidden, gate):
    -> (dpool [B][C], sums [2][C]) for se_bwd_apply; dw1 / db1 / dw2 / db2 / dgamma / dbeta accumulate."""
    ymean, pooled, hidden, gate = state
    B, P, _, C = part.shape
    rd = hidden.shape[1]
    _se_f32("se_bwd_gate", (B, P, 2, C), part)
    _se_f32("se_bwd_gate", (B, C), ymean, pooled, gate)
    _se_f32("se_bwd_gate", (B, rd), hidden)
    _se_f32("se_bwd_gate", (C,), mean, rstd, gamma, beta, db2, *(t for t in (dgamma, dbeta) if t is not None))
    _se_f32("se_bwd_gate", (rd,), db1)
    _se_f32("se_bwd_gate", (rd, C), w1, w2, dw1, dw2)
    if SE_TORCH:
        sg, sgx = part.sum(1).unbind(1)
        dsig = (gamma * sgx + beta * sg) * gate * (1 - gate)
        dh = (dsig @ w2.view(C, rd)) * (hidden > 0)
        dpool = dh @ w1.view(rd, C)
        dw2 += (dsig.t() @ hidden).view(dw2.shape)
        db2 += dsig.sum(0)
        dw1 += (dh.t() @ pooled).view(dw1.shape)
        db1 += dh.sum(0)
        s = torch.stack(((gate * sg + dpool).sum(0), (gate * sgx + dpool * (ymean - mean) * rstd).sum(0)))
        if dbeta is not None:
            dbeta += s[0]
        if dgamma is not None:
            dgamma += s[1]
        return dpool, s if batch_stats else torch.zeros_like(s)
    work = _se_out(work, (3 * B * C + B * rd,), torch.float32, part.device, "se_bwd_gate: work")
    dpool = _se_out(out[0] if out else None, (B, C), torch.float32, part.device, "se_bwd_gate: out")
    sums = _se_out(out[1] if out else None, (2, C), torch.float32, part.device, "se_bwd_gate: out")
    call("sv_se_bwd_gate", ptr(part), P, ptr(ymean), ptr(pooled), ptr(hidden), ptr(gate), ptr(mean), ptr(rstd), ptr(gamma),
         ptr(beta), ptr(w1), ptr(w2), ptr(work), ptr(dpool), ptr(sums), ptr(dgamma), ptr(dbeta), ptr(dw1), ptr(db1),
         ptr(dw2), ptr(db2), int(batch_stats), B, HW, C, rd)
    return dpool, sums


def se_bwd_apply(g4d, y4d, mean, rstd, gamma, gate, dpool, sums, *, dx_dtype=torch.float32, out=None) -> torch.Tensor:
    """Pass B: dy = gamma rstd (g gate + dpool / HW - sums[0] / n - xhat sums[1] / n), n = B HW; g = the masked gradient
    se_bwd_stats left in dout."""
    B, HW, C = _se_act("se_bwd_apply", y4d, g4d)
    _se_f32("se_bwd_apply", (C,), mean, rstd, gamma)
    _se_f32("se_bwd_apply", (B, C), gate, dpool)
    _se_f32("se_bwd_apply", (2, C), sums)
    if SE_TORCH:
        xh = (y4d.float() - mean) * rstd
        dz = g4d.float() * gate.view(B, 1, 1, C) + dpool.view(B, 1, 1, C) / HW
        return (gamma * rstd * (dz - sums[0] / (B * HW) - xh * sums[1] / (B * HW))).to(dx_dtype)
    dx = _se_out(out, tuple(y4d.shape), dx_dtype, y4d.device, "se_bwd_apply: out")
    call("sv_se_bwd_apply", ptr(g4d), dt(g4d), ptr(y4d), dt(y4d), ptr(mean), ptr(rstd), ptr(gamma), ptr(gate), ptr(dpool),
         ptr(sums), ptr(dx), dt(dx), B, HW, C)
    return dx


def _pool2_check(who: str, t: torch.Tensor) -> None:
    _check(t.dim() == 4 and t.is_contiguous() and t.shape[-1] % 8 == 0 and t.dtype in (torch.float32, torch.bfloat16)
           and t.data_ptr() % 16 == 0, f"{who}: need contiguous 16-B aligned f32 / bf16 NHWC, C % 8 == 0")


def avgpool2x2_fwd(x4d: torch.Tensor, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) over NHWC -> [B, ceil(H/2), ceil(W/2), C]."""
    _pool2_check("avgpool2x2_fwd", x4d)
    B, H, W, C = x4d.shape
    if SE_TORCH:
        y = torch.nn.functional.avg_pool2d(x4d.permute(0, 3, 1, 2).float(), 2, 2, ceil_mode=True, count_include_pad=False)
        return y.permute(0, 2, 3, 1).contiguous().to(x4d.dtype)
    y = _se_out(out, (B, (H + 1) // 2, (W + 1) // 2, C), x4d.dtype, x4d.device, "avgpool2x2_fwd: out")
    call("sv_avgpool2x2_fwd", ptr(x4d), dt(x4d), ptr(y), B, H, W, C)
    return y


def avgpool2x2_bwd(dout4d: torch.Tensor, H: int, W: int, dx_dtype=torch.float32, *, out=None) -> torch.Tensor:
    """-> dx [B,H,W,C]: every input pixel gets its window's gradient divided by the window's tap count (1, 2 or 4)."""
    _pool2_check("avgpool2x2_bwd", dout4d)
    B, OH, OW, C = dout4d.shape
    _check((OH, OW) == ((H + 1) // 2, (W + 1) // 2), "avgpool2x2_bwd: shape mismatch")
    if SE_TORCH:
        ones = torch.ones(1, 1, H, W, device=dout4d.device)
        cnt = torch.nn.functional.avg_pool2d(ones, 2, 2, ceil_mode=True, count_include_pad=False, divisor_override=1)
        d = (dout4d.float() / cnt.view(1, OH, OW, 1)).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
        return d.contiguous().to(dx_dtype)
    dx = _se_out(out, (B, H, W, C), dx_dtype, dout4d.device, "avgpool2x2_bwd: out")
    call("sv_avgpool2x2_bwd", ptr(dout4d), dt(dout4d), ptr(dx), dt(dx), B, H, W, C)
    return dx


# ----------------------------------------------------------------------------------------------
# MBConv (csrc/mbconv.hip, csrc/dwconv5.hip): depthwise 3x3 | 5x5, BatchNorm + SiLU and the gating squeeze-and-excitation
# of EfficientNetV2 and EfficientNet-B0..B4
# SV_MBCONV=torch: the same wrappers computed with torch ops on the device, f32 arithmetic and the same rounding points
# (A/B baseline and debugging aid, never the default)
MBCONV_TORCH = os.environ.get("SV_MBCONV", "") == "torch"
MB_MAX_C = 3840


def _mb_rows(who: str, C: int, *ts) -> None:
    _check(C % 32 == 0 and 32 <= C <= MB_MAX_C, f"{who}: C must be a multiple of 32 up to {MB_MAX_C}, got {C}")
    for t in ts:
        _check(t.is_contiguous() and t.shape[-1] == C and t.numel() == ts[0].numel()
               and t.dtype in (torch.float32, torch.bfloat16) and t.data_ptr() % 16 == 0,
               f"{who}: need contiguous 16-B aligned f32 / bf16 [..., {C}] tensors of one shape")


def _mb_bn(who: str, C: int, bn: tuple) -> tuple:
    """(mean, rstd, gamma, beta) of a BatchNorm, detached and checked"""
    bn = tuple(t.detach() for t in bn)
    _check(len(bn) == 4, f"{who}: bn = (mean, rstd, gamma, beta)")
    _se_f32(who, (C,), *bn)
    return bn


def _mb_pre(y, bn):
    mean, rstd, gamma, beta = bn
    return (gamma * rstd) * (y.float() - mean) + beta


def _silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def mbconv_nparts(rows: int, C: int) -> int:
    return value("sv_mbconv_nparts", rows, C)


def mb_bn_stats(y2d: torch.Tensor, *, eps: float = EPS_BN, momentum: float = 0.1, running_mean=None, running_var=None,
                num_batches_tracked=None):
    """bn_stats for any C % 32 == 0 (sv_bn_stats stops at 1024 channels): unshifted (sum, sum of squares) partials from
    csrc/mbconv.hip, folded by the existing sv_bn_stats_finish -> (mean, rstd) f32; running statistics updated."""
    rows, C = y2d.shape
    _mb_rows("mb_bn_stats", C, y2d)
    if MBCONV_TORCH:
        yf = y2d.float()
        part = torch.stack((yf.sum(0), (yf * yf).sum(0))).view(1, 2, C).contiguous()
    else:
        part = torch.empty(mbconv_nparts(rows, C), 2, C, device=y2d.device, dtype=torch.float32)
        call("sv_mbconv_bn_stats", ptr(y2d), dt(y2d), rows, C, ptr(part))
    return bn_stats_from_partials(part, rows, eps=eps, momentum=momentum, running_mean=running_mean,
                                  running_var=running_var, num_batches_tracked=num_batches_tracked)


def bn_silu_fwd(y2d, bn: tuple, *, res=None, out_dtype=torch.float32, out=None) -> torch.Tensor:
    """silu(gamma (y - mean) rstd + beta) (+ res, added after the activation); bn = (mean, rstd, gamma, beta)."""
    rows, C = y2d.shape
    _mb_rows("bn_silu_fwd", C, y2d, *(() if res is None else (res,)))
    bn = _mb_bn("bn_silu_fwd", C, bn)
    if MBCONV_TORCH:
        o = torch.nn.functional.silu(_mb_pre(y2d, bn))
        return (o if res is None else o + res.float().view(rows, C)).to(out_dtype)
    out = _se_out(out, (rows, C), out_dtype, y2d.device, "bn_silu_fwd: out")
    call("sv_bn_silu_fwd", ptr(y2d), dt(y2d), *map(ptr, bn), ptr(res), nv.dt_none(res), ptr(out), dt(out), rows, C)
    return out


def bn_silu_bwd_stats(dout2d, y2d, bn: tuple) -> torch.Tensor:
    """part [P][2][C] = partial (sum g, sum g xhat), g = dout silu'(pre)."""
    rows, C = y2d.shape
    _mb_rows("bn_silu_bwd_stats", C, y2d, dout2d)
    bn = _mb_bn("bn_silu_bwd_stats", C, bn)
    if MBCONV_TORCH:
        g = dout2d.float().view(rows, C) * _silu_grad(_mb_pre(y2d, bn))
        return torch.stack((g.sum(0), (g * ((y2d.float() - bn[0]) * bn[1])).sum(0))).view(1, 2, C).contiguous()
    part = torch.empty(mbconv_nparts(rows, C), 2, C, device=y2d.device, dtype=torch.float32)
    call("sv_bn_silu_bwd_stats", ptr(dout2d), dt(dout2d), ptr(y2d), dt(y2d), *map(ptr, bn), rows, C, ptr(part))
    return part


def bn_silu_bwd_apply(dout2d, y2d, bn: tuple, sums, *, dx_dtype=torch.float32, out=None) -> torch.Tensor:
    """dx = gamma rstd (g - sums[0] / n - xhat sums[1] / n), g = dout silu'(pre), n = rows."""
    rows, C = y2d.shape
    _mb_rows("bn_silu_bwd_apply", C, y2d, dout2d)
    bn = _mb_bn("bn_silu_bwd_apply", C, bn)
    _se_f32("bn_silu_bwd_apply", (2, C), sums)
    if MBCONV_TORCH:
        g = dout2d.float().view(rows, C) * _silu_grad(_mb_pre(y2d, bn))
        xh = (y2d.float() - bn[0]) * bn[1]
        s = sums.view(2, C)
        return ((bn[2] * bn[1]) * (g - s[0] / rows - xh * s[1] / rows)).to(dx_dtype)
    dx = _se_out(out, (rows, C), dx_dtype, y2d.device, "bn_silu_bwd_apply: out")
    call("sv_bn_silu_bwd_apply", ptr(dout2d), dt(dout2d), ptr(y2d), dt(y2d), *map(ptr, bn), ptr(sums), ptr(dx), dt(dx),
         rows, C)
    return dx


def bn_silu_bwd(dout2d, y2d, bn: tuple, *, dgamma=None, dbeta=None, dx_dtype=torch.float32,
                batch_stats: bool = True) -> torch.Tensor:
    """Backward of bn_silu_fwd (without its residual): statistics pass, the existing sv_bn_bwd_finish, apply pass;
    dgamma / dbeta accumulate."""
    part = bn_silu_bwd_stats(dout2d, y2d, bn)
    sums = _bn_bwd_sums(part.shape[0], y2d.shape[1], batch_stats, (part, dgamma, dbeta))
    return bn_silu_bwd_apply(dout2d, y2d, bn, sums, dx_dtype=dx_dtype)


def mb_add(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst += src (f32 sum, one rounding): the identity shortcut's gradient joining a block's input gradient."""
    _check(dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel() and dst.numel() % 8 == 0,
           "mb_add: contiguous tensors of one size, a multiple of 8")
    if MBCONV_TORCH:
        return dst.copy_(dst.float() + src.float().view(dst.shape))
    call("sv_mbconv_add", ptr(dst), dt(dst), ptr(src), dt(src), dst.numel())
    return dst


def _dw_check(who: str, x4d, w, stride: int, k: int) -> tuple:
    B, H, W, C = x4d.shape
    _mb_rows(who, C, x4d)
    _check(stride in (1, 2) and tuple(w.shape) == (C, 1, k, k) and w.dtype == torch.float32 and w.is_contiguous()
           and w.data_ptr() % 16 == 0, f"{who}: stride 1 | 2 and a contiguous f32 weight [C,1,{k},{k}]")
    return B, H, W, C


def _dwconv_fwd(k: int, x4d, w, stride: int, out_dtype, out) -> torch.Tensor:
    who = f"dwconv{k}_fwd"
    B, H, W, C = _dw_check(who, x4d, w, stride, k)
    out_dtype = out_dtype or x4d.dtype
    if MBCONV_TORCH:
        y = torch.nn.functional.conv2d(x4d.float().permute(0, 3, 1, 2), w, stride=stride, padding=k // 2, groups=C)
        return y.permute(0, 2, 3, 1).contiguous().to(out_dtype)
    y = _se_out(out, (B, (H - 1) // stride + 1, (W - 1) // stride + 1, C), out_dtype, x4d.device, f"{who}: out")
    call(f"sv_{who}", ptr(x4d), dt(x4d), ptr(w), ptr(y), dt(y), B, H, W, C, stride)
    return y


def _dwconv_bwd_data(k: int, dy4d, w, H: int, W: int, stride: int, dx_dtype, out) -> torch.Tensor:
    who = f"dwconv{k}_bwd_data"
    B, OH, OW, C = _dw_check(who, dy4d, w, stride, k)
    _check((OH, OW) == ((H - 1) // stride + 1, (W - 1) // stride + 1), f"{who}: shape mismatch")
    dx_dtype = dx_dtype or dy4d.dtype
    if MBCONV_TORCH:
        dx = torch.nn.grad.conv2d_input((B, C, H, W), w, dy4d.float().permute(0, 3, 1, 2), stride=stride,
                                        padding=k // 2, groups=C)
        return dx.permute(0, 2, 3, 1).contiguous().to(dx_dtype)
    dx = _se_out(out, (B, H, W, C), dx_dtype, dy4d.device, f"{who}: out")
    call(f"sv_{who}", ptr(dy4d), dt(dy4d), ptr(w), ptr(dx), dt(dx), B, H, W, C, stride)
    return dx


def _dwconv_bwd_weight(k: int, dy4d, x4d, stride: int, dw, accumulate: bool) -> torch.Tensor:
    who = f"dwconv{k}_bwd_weight"
    B, H, W, C = x4d.shape
    _mb_rows(who, C, x4d)
    _mb_rows(who, C, dy4d)
    _check(stride in (1, 2) and tuple(dy4d.shape) == (B, (H - 1) // stride + 1, (W - 1) // stride + 1, C)
           and tuple(dw.shape) == (C, 1, k, k) and dw.dtype == torch.float32 and dw.is_contiguous(),
           f"{who}: dy [B,OH,OW,C], dw f32 [C,1,{k},{k}]")
    if MBCONV_TORCH:
        g = torch.nn.grad.conv2d_weight(x4d.float().permute(0, 3, 1, 2), (C, 1, k, k), dy4d.float().permute(0, 3, 1, 2),
                                        stride=stride, padding=k // 2, groups=C)
        return dw.add_(g) if accumulate else dw.copy_(g)
    P = value(f"sv_{who}_nparts", B, H, W, C, stride)
    part = torch.empty(P, k * k, C, device=x4d.device, dtype=torch.float32)
    call(f"sv_{who}", ptr(dy4d), dt(dy4d), ptr(x4d), dt(x4d), ptr(part), ptr(dw), int(accumulate), B, H, W, C, stride)
    return dw


def dwconv3_fwd(x4d: torch.Tensor, w: torch.Tensor, stride: int, *, out_dtype=None, out=None) -> torch.Tensor:
    """Depthwise 3x3, pad 1 -> [B, (H-1)//stride+1, (W-1)//stride+1, C]."""
    return _dwconv_fwd(3, x4d, w, stride, out_dtype, out)


def dwconv3_bwd_data(dy4d: torch.Tensor, w: torch.Tensor, H: int, W: int, stride: int, *, dx_dtype=None,
                     out=None) -> torch.Tensor:
    return _dwconv_bwd_data(3, dy4d, w, H, W, stride, dx_dtype, out)


def dwconv3_bwd_weight(dy4d: torch.Tensor, x4d: torch.Tensor, stride: int, *, dw: torch.Tensor,
                       accumulate: bool = True) -> torch.Tensor:
    """dw [C,1,3,3] f32 (+)= the depthwise weight gradient (per-workgroup partials, folded in part order)."""
    return _dwconv_bwd_weight(3, dy4d, x4d, stride, dw, accumulate)


# depthwise 5x5, pad 2 (csrc/dwconv5.hip): the k = 5 blocks of EfficientNet-B0..B4; arguments as the 3x3 wrappers
def dwconv5_fwd(x4d: torch.Tensor, w: torch.Tensor, stride: int, *, out_dtype=None, out=None) -> torch.Tensor:
    """Depthwise 5x5, pad 2 -> [B, (H-1)//stride+1, (W-1)//stride+1, C]."""
    return _dwconv_fwd(5, x4d, w, stride, out_dtype, out)


def dwconv5_bwd_data(dy4d: torch.Tensor, w: torch.Tensor, H: int, W: int, stride: int, *, dx_dtype=None,
                     out=None) -> torch.Tensor:
    return _dwconv_bwd_data(5, dy4d, w, H, W, stride, dx_dtype, out)


def dwconv5_bwd_weight(dy4d: torch.Tensor, x4d: torch.Tensor, stride: int, *, dw: torch.Tensor,
                       accumulate: bool = True) -> torch.Tensor:
    """dw [C,1,5,5] f32 (+)= the depthwise weight gradient (per-workgroup partials [P][25][C], folded in part order)."""
    return _dwconv_bwd_weight(5, dy4d, x4d, stride, dw, accumulate)


def _mbse_act(who: str, *ts) -> tuple:
    B, H, W, C = ts[0].shape
    _mb_rows(who, C, *ts)
    return B, H * W, C


def mbse_squeeze(y4d: torch.Tensor, bn: tuple) -> torch.Tensor:
    """Per-image partial sums of s = silu(bn(y)) over the raw depthwise output y [B,H,W,C] -> part [B][P][C] f32."""
    B, HW, C = _mbse_act("mbse_squeeze", y4d)
    bn = _mb_bn("mbse_squeeze", C, bn)
    if MBCONV_TORCH:
        return torch.nn.functional.silu(_mb_pre(y4d, bn)).sum((1, 2)).view(B, 1, C)
    part = torch.empty(B, mbconv_nparts(HW, C), C, device=y4d.device, dtype=torch.float32)
    call("sv_mbse_squeeze", ptr(y4d), dt(y4d), *map(ptr, bn), ptr(part), B, HW, C)
    return part


def mbse_excite(part: torch.Tensor, HW: int, w1, b1, w2, b2) -> tuple:
    """-> (pooled [B][C], hpre [B][rd], hidden = silu(hpre), gate = sigmoid(w2 hidden + b2) [B][C]); all f32."""
    B, P, C = part.shape
    rd = w1.shape[0]
    w1, b1, w2, b2 = (t.detach() for t in (w1, b1, w2, b2))
    _se_f32("mbse_excite", (B, P, C), part)
    _se_f32("mbse_excite", (rd, C), w1, w2)
    _se_f32("mbse_excite", (rd,), b1)
    _se_f32("mbse_excite", (C,), b2)
    _check(w1.shape[:2] == (rd, C) and w2.shape[:2] == (C, rd) and rd % 4 == 0, "mbse_excite: w1 [rd,C,1,1], w2 [C,rd,1,1]")
    if MBCONV_TORCH:
        pooled = part.sum(1) / HW
        hpre = pooled @ w1.view(rd, C).t() + b1
        hidden = torch.nn.functional.silu(hpre)
        return pooled, hpre, hidden, torch.sigmoid(hidden @ w2.view(C, rd).t() + b2)
    pooled, gate = (torch.empty(B, C, device=part.device, dtype=torch.float32) for _ in range(2))
    hpre, hidden = (torch.empty(B, rd, device=part.device, dtype=torch.float32) for _ in range(2))
    call("sv_mbse_excite", ptr(part), P, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(pooled), ptr(hpre), ptr(hidden), ptr(gate),
         B, HW, C, rd)
    return pooled, hpre, hidden, gate


def mbse_scale(y4d, bn: tuple, gate, *, out_dtype=torch.float32, out=None) -> torch.Tensor:
    """a = silu(bn(y)) * gate[b][c]: the project convolution's operand."""
    B, HW, C = _mbse_act("mbse_scale", y4d)
    bn = _mb_bn("mbse_scale", C, bn)
    _se_f32("mbse_scale", (B, C), gate)
    if MBCONV_TORCH:
        return (torch.nn.functional.silu(_mb_pre(y4d, bn)) * gate.view(B, 1, 1, C)).to(out_dtype)
    out = _se_out(out, tuple(y4d.shape), out_dtype, y4d.device, "mbse_scale: out")
    call("sv_mbse_scale", ptr(y4d), dt(y4d), *map(ptr, bn), ptr(gate), ptr(out), dt(out), B, HW, C)
    return out


def mbse_bwd_stats(da4d, y4d, bn: tuple) -> torch.Tensor:
    """Backward pass A: part [B][P][C] = per-image partial sums of da * s."""
    B, HW, C = _mbse_act("mbse_bwd_stats", y4d, da4d)
    bn = _mb_bn("mbse_bwd_stats", C, bn)
    if MBCONV_TORCH:
        return (da4d.float() * torch.nn.functional.silu(_mb_pre(y4d, bn))).sum((1, 2)).view(B, 1, C)
    part = torch.empty(B, mbconv_nparts(HW, C), C, device=y4d.device, dtype=torch.float32)
    call("sv_mbse_bwd_stats", ptr(da4d), dt(da4d), ptr(y4d), dt(y4d), *map(ptr, bn), ptr(part), B, HW, C)
    return part


def mbse_bwd_gate(part, state: tuple, w1, w2, *, dw1, db1, dw2, db2) -> torch.Tensor:
    """The gate's backward from pass A's partials and the forward's ``state`` = (pooled, hpre, hidden, gate) -> dpool
    [B][C] (the gradient of the SUM's mean: pass B divides by HW); dw1 / db1 / dw2 / db2 accumulate."""
    pooled, hpre, hidden, gate = state
    B, P, C = part.shape
    rd = hidden.shape[1]
    w1, w2 = w1.detach(), w2.detach()
    _se_f32("mbse_bwd_gate", (B, P, C), part)
    _se_f32("mbse_bwd_gate", (B, C), pooled, gate)
    _se_f32("mbse_bwd_gate", (B, rd), hpre, hidden)
    _se_f32("mbse_bwd_gate", (rd, C), w1, w2, dw1, dw2)
    _se_f32("mbse_bwd_gate", (rd,), db1)
    _se_f32("mbse_bwd_gate", (C,), db2)
    if MBCONV_TORCH:
        dsig = part.sum(1) * gate * (1 - gate)
        dh = (dsig @ w2.view(C, rd)) * _silu_grad(hpre)
        dpool = dh @ w1.view(rd, C)
        dw2 += (dsig.t() @ hidden).view(dw2.shape)
        db2 += dsig.sum(0)
        dw1 += (dh.t() @ pooled).view(dw1.shape)
        db1 += dh.sum(0)
        return dpool
    work = torch.empty(B * C + B * rd, device=part.device, dtype=torch.float32)
    dpool = torch.empty(B, C, device=part.device, dtype=torch.float32)
    call("sv_mbse_bwd_gate", ptr(part), P, ptr(pooled), ptr(hpre), ptr(hidden), ptr(gate), ptr(w1), ptr(w2), ptr(work),
         ptr(dpool), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), B, C, rd)
    return dpool


def mbse_bwd_apply(da4d, y4d, bn: tuple, gate, dpool, *, out_dtype=torch.float32) -> tuple:
    """Backward pass B: dpre = (da gate + dpool / HW) silu'(pre) stored in ``out_dtype`` -> (dpre, part [B P][2][C]), the
    BatchNorm backward partials (sum, sum * xhat) of the stored dpre for bn_bwd(part=...)'s finish and apply."""
    B, HW, C = _mbse_act("mbse_bwd_apply", y4d, da4d)
    bn = _mb_bn("mbse_bwd_apply", C, bn)
    _se_f32("mbse_bwd_apply", (B, C), gate, dpool)
    if MBCONV_TORCH:
        dpre = ((da4d.float() * gate.view(B, 1, 1, C) + dpool.view(B, 1, 1, C) / HW) * _silu_grad(_mb_pre(y4d, bn))).to(out_dtype)
        r = dpre.float()
        xh = (y4d.float() - bn[0]) * bn[1]
        return dpre, torch.stack((r.sum((1, 2)), (r * xh).sum((1, 2))), 1).contiguous()
    P = mbconv_nparts(HW, C)
    dpre = torch.empty(tuple(y4d.shape), device=y4d.device, dtype=out_dtype)
    part = torch.empty(B * P, 2, C, device=y4d.device, dtype=torch.float32)
    call("sv_mbse_bwd_apply", ptr(da4d), dt(da4d), ptr(y4d), dt(y4d), *map(ptr, bn), ptr(gate), ptr(dpool), ptr(dpre),
         dt(dpre), ptr(part), B, HW, C)
    return dpre, part


def bn_bwd_from_partials(dout2d, y2d, mean, rstd, gamma, part, *, dgamma=None, dbeta=None, dx_dtype=torch.float32,
                         batch_stats: bool = True) -> torch.Tensor:
    """An activation-free BatchNorm's backward whose statistics partials [P][2][C] dout's producer already summed
    (mbse_bwd_apply): the existing sv_bn_bwd_finish and sv_bn_bwd_apply (act = NULL), unchanged."""
    rows, C = y2d.shape
    _check(part.dtype == torch.float32 and part.is_contiguous() and tuple(part.shape[1:]) == (2, C),
           "bn_bwd_from_partials: part must be f32 [P][2][C]")
    sums = _bn_bwd_sums(part.shape[0], C, batch_stats, (part, dgamma, dbeta))
    dx = torch.empty(rows, C, device=y2d.device, dtype=dx_dtype)
    call("sv_bn_bwd_apply", ptr(dout2d), dt(dout2d), None, SV_F32, ptr(y2d), dt(y2d), ptr(mean), ptr(rstd), ptr(gamma),
         ptr(sums), ptr(dx), dt(dx), None, rows, C)
    return dx
