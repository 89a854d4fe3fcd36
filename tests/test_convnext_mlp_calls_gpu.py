"""The pointwise side of a ConvNeXt block, one kernel call at a time through the ``spine_vision_amd.kernels`` wrapper
``backbone/convnext.py`` uses, with convnext.py's argument forms, every element of every output against a float64
evaluation of the same operation on the same rounded operands (torch float64 on the device), judged by
``_calls_harness.judge``: |got - ref| <= 2 x a derived bound for EVERY element.  The bit-equality tests between kernel
families (test_mlp_fused_gpu.py, test_gemm_family_gpu.py) share tile routines and epilogue code and say nothing about
the values; a relative L2 of 2e-3 cannot see one wrong row, one dropped hidden chunk in one tile or a wrong edge tile.

1. The fused kernels (csrc/mlp.hip, gemm9.hip's LayerNorm-backward epilogue)
    455  mlp_fwd(y, w1, b1, w2, b2, gamma, x, out=, gelu_grad=, gelu_out=), training and eval, C in {128, 192, 256, 512}
         (c128, general <192>, general <256>, c512; the SV_MLP128_V1 arm -- C = 128 on the general kernel -- is an A/B
         leftover read once per process and is left out).  gh = bf16(GELU'(h)), a = bf16(GELU(h)) against float64
         h = y W1^T + b1; x_out against gamma (a_got W2^T + b2) + x with a_got the kernel's own stored a (each stage is
         judged alone); the eval form's x_out bit for bit the training form's.  Rows 1, 127, 128, 129, 1000 and
         slots * 128 + 133 (slots = 2 CUs at C = 128, CUs otherwise): the smallest count at which a workgroup walks a
         second tile (the c128 next-tile y prefetch, the reuse of the weight rings) with a ragged last tile.
    590  mlp_bwd at C = 128, the operand images from transpose_scale_bf16 (405 / 406; checked per element, then taken
         as operands): dh against (d (W2 gamma)) gh; dz against the float64 LayerNorm backward of dy = dh_got W1; the
         per-wave partials (every row NaN before the call) and their folds through reduce_pair (597) and reduce_multi
         (577).  Rows 1, 127, 129, 1000 and 512 * 128 + 133 (the grid is min(tiles, 512)).
    615  linear_dgrad_ln (SV_EPI_LN_BWD), C = 512 and 1024 (2 and 4 column tiles per row block), M in {8, 256, 264,
         1000}, default policy and the backward's; only through the wrapper, which guarantees the residency the
         epilogue's polling needs; under the default policy it must take the fused form (16 tiles at most), under
         the backward's a None is the two-pass answer and leaves nothing to check.  dz and the partials are the
         wrapper's own allocations: torch.empty is replaced while the wrapper runs (and only then) so that they start
         as NaN, and the wrapper's cached exchange workspace is dropped before each call so that it is allocated, NaN-
         filled, by that call whatever ran earlier in the process; no sentinels are possible around them.
2. The unfused calls, bf16 compute, C in {96, 128, 256, 512, 1536} (C = 1536: M = 16 and 400 only), M in {16, 400,
   1400, 1600}
    466 / 470  fc1 forward BIAS_GELU_DUAL, BIAS_GELU bit for bit the dual's out2                    -> fc1_fwd
    484 / 481  fc2 forward BIAS_GAMMA_RES, random gamma / ls_ones on a bf16 u                       -> fc2_fwd, fc2_fwd_ones
    605        fc2 data gradient MUL_AUX with the scale_rows_bf16 weight (checked per element)      -> fc2_dgrad
    529        fc2 data gradient, V2: plain store, bf16 out                                         -> fc2_dgrad_v2
    621        fc1 data gradient, bf16 out                                                          -> fc1_dgrad
    570 / 577  linear_wgrad(accumulate, bias_out, defer=folds) + reduce_multi; without defer  -> fc1_wgrad_defer, fc1_wgrad
    565        layerscale_wgrad at K4 = 4C, wgrad_target 256                                        -> fc2_lswgrad
    437 / 685 / 686  downsample forward / data gradient / weight gradient, K = 4C, N = 2C, f32 out (C = 96 .. 512)
                                                                                        -> ds_fwd, ds_dgrad, ds_wgrad
    416        bf16 stem forward on stem_patchify's 64-wide rows and stem_weight_pack's weight      -> stem_fwd
    699        bf16 stem weight gradient, cols=48 into a [C0, 48] view, C0 in {96, 128, 192}        -> stem_wgrad
   Family per (shape, default policy), from csrc/gemm.hip's dispatch (tiles8 = ceil(M / 256) ceil(N / 256) < 256 at
   every M here, so neither v9 nor v8 is picked for a forward or data-gradient call by default):
       fc1_fwd (heavy epilogue), fc2_dgrad (MUL_AUX), fc2_dgrad_v2 / ds_dgrad / stem_fwd (store, K <= 2048) ... v3
       fc1_dgrad, ds_fwd (store): K = 4C <= 2048 v3; C = 1536 (K = 6144) v2, v3 under the backward's wg_per_cu = 1
       fc2_fwd (residual form) ................................................................ v2 (K = 4C, % 64 == 0)
       weight gradients: M = 16, 400, 1400 (M % 32 != 0) the generic launch_layout kernel, f32 slabs; M = 1600: v9
       where the output is at least 128 x 256 and tiles8 * split >= 128 or the slabs are bf16 (split in {5, 25}), else
       v3 32x4 (32x3 under wg_per_cu = 1); the stem's [C0, 48] output never reaches v9.
   C = 96 gives K = 96 (K % 64 != 0: v2 refuses, v3 takes 3 k-steps) and N = 96; C = 1536 gives fc2 K = 6144.
   Besides the default policy: nv.policy(impl=2 | 3 | 8 | 9) and impl=9, grid_cap=4 wherever the family's contract holds
   (v2: K % 64; v3, v8: K % 32; v9: K % (split * 64)), and the policies ConvNeXtHip's backward builds (data gradients,
   downsample and stem: wg_per_cu = 1; block weight gradients: the side stream's, priority 1).  The in-kernel split-K
   fold (SV_INKERNEL_FOLD, opt-in, measured slower) is out of scope.
3. The fp32-compute arm (compute_bf16=False, f32 operands and outputs, launch_layout<false, float, float>), the calls
   of 2 at C in {96, 128, 384}, M in {16, 400, 1400}; the fc2 data gradient is line 607's, a_scale_k = gamma, MUL_AUX.

Bound per element (test_vit_calls_gpu.py's rule): an f32-accumulated product of exact bf16 operands is within
K 2^-24 S of float64, S = |A| @ |B| (+ |bias|); times the epilogue's Lipschitz factor (1.13 GELU, 1 GELU', |aux|,
|gamma|); + 2^-8 |ref| for a bf16 store, 2^-23 on the addends for an f32 store of a two-term sum (2^-23 |ref| for a
plain one); + 2^-8 sum_s |slab_s| for bf16 slabs with the slices of kernels._wgrad_split_for; the two GELU outputs
+ 4 x the largest error of torch's float32 CPU erf-GELU / GELU' on the same h (at most its first 1024 rows; printed).
fp32 arm: v_mfma_f32_16x16x4_f32 adds four f32 products to the accumulator; the operand products are no longer exact
and the order and rounding of the four additions inside the instruction are not documented.  Each of the K terms
passes through at most one rounding of its product and then the chain of at most K additions, (K + 1) 2^-24 S to first
order; 2K roundings are used (the figure the issue allows without a tighter derivation), 2K + 1 where a_scale_k
multiplies the A operand first (one more rounding per term).
LayerNorm backward outputs (mlp_bwd, linear_dgrad_ln): the kernel's dy = bf16(f32 accumulation of dh_got W1) is not
stored; it differs from the float64 dy by at most e_j = 2^-8 |dy_j| + K 2^-24 S_j per column.  The float64 LayerNorm
backward of the float64 dy is the reference; its bound is _convnext_ref.ln_bwd_core's f32 chain (D = the row sums'
depth: mlp_bwd 32 columns per lane + 2 shuffles; the epilogue 16 columns per lane + 2 shuffles + 4 waves + C / 256
tiles) plus e through the backward, which is linear in dy: rstd (|w| e + mean(|w| e) + |xhat| mean(|w| e |xhat|)),
plus the bf16 store.  dw / db: red_bounds with n = the fragments a wave adds (8 per 128-row tile and per tile of the
workgroup's walk) + 4 shuffles + fold_depth(P), plus sum_m e |xhat| and sum_m e.  That sum of e over the rows is a
worst case that grows with M (2^-8 sum |dy xhat|: from about 30 rows on, a whole missing row is below it), so the same
dw / db are judged a second time (``*_rounded``) against the sums of bf16(dy), the operand the kernel does sum: the
kernel's dy differs from bf16(float64 dy) only where the float64 value lies within the accumulation's K 2^-24 S of a
rounding boundary, and there by one bf16 step (_convnext_ref.stored), which replaces e.  Both must hold.
Nothing is tuned on the kernels' output.

Inputs: GEMM operands uniform on [-0.25, 1] (x K^-1/2 for weights): signed, with a mean, so that one dropped k-step
moves an element by several times its own spread (the CPU-side condition (b) could not hold at a bf16 store for a
zero-mean contribution: a share of about 1.5 % of the elements would move by less than the store's bound); the fc1 bias
recentres h on [-2, 2] +- its spread so both GELU outputs run over their curved range.  The weights under a LayerNorm
backward are normal with a small mean (dy's mean about its spread: a larger one would make dz insensitive to dy;
none would leave a column tile's share of the row sums a zero-mean quantity).  fc1's weights are x 2 C^-1/2.
gamma in [0.05, 0.3], gh in [-0.2, 1.2], LayerNorm statistics the f32 roundings of the float64 ones.

Guards: every input and output between 256 sentinels (-7.0), outputs NaN before the call (accumulating ones a non-zero
prior the reference adds), inputs bit-unchanged, every call twice with bit-equal results.

test_reference_side_conditions (no GPU): on the smallest case of each call kind a float32 CPU evaluation with bf16
rounding at the kernel's rounding points stays within 1 x the bound in every element, and one dropped contribution (a
32-deep k-step; a 64-unit hidden chunk of the fused MLP; a row of a weight gradient; one column tile's or lane group's
share of the LayerNorm row sums) moves at least 0.99 of the affected elements by more than 4 x the bound.  Where the
smallest case has fewer than 1000 affected elements the share is taken on the next one.  Three of the conditions are
stated on what the reference can show:
  gh = GELU'(h) under a dropped k-step, on the elements whose h and shifted h lie on one monotone branch of GELU'
    (it rises on (-sqrt 2, sqrt 2) and falls outside).  A pair that straddles an extremum can have GELU'(h) =
    GELU'(h') exactly, so some share of the straddling pairs lies within the bf16 store's 4 x 2^-8 |gh| at any shift;
    a = GELU(h) of the same call is held to the condition on every element.
  the LayerNorm weight / bias sums under a dropped row, against the ``*_rounded`` bound, with the row's term taken as
    its RMS over the rows, per channel (as test_convnext_calls_gpu.py does for its reductions): a single term
    dy xhat is near zero for 5 to 15 % of the channels of any one row, and against the worst-case bound a whole row
    is invisible from about 30 rows on.
  mlp_bwd's dz under one lane group's share of the row sums (a wave's row sum is the sum over its four lane groups;
    the counterpart of the epilogue's column tile at C = 128, where a row lies in one wave).
One share is printed without being a condition: dz under a dropped 32-deep k-step of dy = dh W1 (0.56).  The LayerNorm
backward removes the row mean of the change, what is left is a zero-mean 1 / 16 of dy's spread, and the bound the
issue sets for dz carries the unstored rounding 2^-8 |dy| three times over (column, both means) besides dz's own
store.  On the GPU such an error still fails the 2 x assertion in about half of a tile's elements.  Figures:
profiles/convnext_mlp_calls/cpu_conditions.txt; the GPU run's: profiles/convnext_mlp_calls/parity.txt."""
import contextlib
import functools
import math

import pytest
import torch

import _convnext_ref as R
from _calls_harness import judge
from _gemm_ref import (BF, F32, F64, U8, U23, U24, Call, _bf, _bits, _equal_pairs, _erf_abs_terms, _gelu32, _gelu64,
                       _gelu_grad64, _guarded, _guards_intact, _run_guarded, _wgrad_terms)
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
TAG = "convnext_mlp_calls"
CPU = torch.device("cpu")
WGRAD_TARGET = 256  # ConvNeXtHip.wgrad_target
NAN = float("nan")
LO, HI = -0.25, 1.0  # the GEMM operands' interval
MU = 0.5 * (LO + HI)
W1_SCALE = 2.0  # fc1's weights: x 2 C^-1/2, so a k-step is a shift of h of 0.3 (C = 1536) to 0.9 (C = 96)
ERF_ROWS = 1024


# ------------------------------------------------------------------------------------------------------- operands
def _u(g, dev, *shape, lo=LO, hi=HI):
    """uniform float64, drawn on the CPU (the CPU-side conditions and the GPU tests see the same numbers)"""
    return (torch.rand(*shape, generator=g, dtype=F64) * (hi - lo) + lo).to(dev)


def _n(g, dev, *shape):
    return torch.randn(*shape, generator=g, dtype=F64).to(dev)


def _f32(t):
    return t.float().double()


def _ident(t, dt):
    return t


def _round32(t, dt):
    return t.to(dt).float()


def _mm(A, B, drop=0):
    """A [M, K] @ B [K, N] without its first ``drop`` k"""
    return A[:, drop:] @ B[drop:] if drop else A @ B


def _gelu_pair(h):
    return (_gelu64(h), _gelu_grad64(h)) if h.dtype == F64 else _gelu32(h)


def _store(ref, dt):
    return (U8 if dt == BF else U23) * ref.abs()


def _one_branch(ref, moved):
    """GELU' rises on (-sqrt 2, sqrt 2) and falls outside: the elements whose h and shifted h lie on one branch, where
    a shift of h cannot cancel in gh (across an extremum it can: GELU'(h) = GELU'(h') for a pair straddling it)"""
    r2 = math.sqrt(2.0)
    edges = torch.tensor([-r2, r2], dtype=F64)
    return torch.bucketize(ref["_h"], edges) == torch.bucketize(moved["_h"], edges)


def _erf_terms(h):
    return _erf_abs_terms(h[:ERF_ROWS])


class Case(Call):
    """A Call whose float64 reference, float32 emulation and dropped-contribution variant are one function:
    ``ev(t, rnd, got, drop)`` evaluates the operation on the inputs ``t`` (name -> tensor, float64 or float32) with
    ``rnd(value, dtype)`` at the kernel's rounding points (identity in float64), a later stage reading ``got`` (the
    stored outputs of an earlier one) where given, and ``drop`` naming a contribution to leave out; ``bounds(t, ref,
    got, slabs)`` -> name -> bound; ``drops``: (label, drop, affected outputs)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ev = self.bounds = None
        self.drops = []
        self.aliases = {}  # a second reference for an output: alias -> output name
        self.masks = {}  # output -> mask(ref values, moved values): the elements condition (b) is stated on

    def t64(self):
        return {n: t for n, (t, _) in self.inputs.items()}

    def make_refs(self, got=None, slabs=False):
        t = self.t64()
        ref = self.ev(t, _ident, got, None)
        b = self.bounds(t, ref, got, slabs)
        return {n: (ref[n], b[n]) for n in list(self.outputs) + list(self.aliases)}


@contextlib.contextmanager
def _nan_empty():
    """torch.empty returns NaN-filled floating tensors: what a wrapper allocates itself starts as NaN too"""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            t.fill_(NAN)
        return t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


# ------------------------------------------------------------------------------------------------- the fused forward
def build_mlp_fwd(C, M, dev):
    g = R._gen("mlp_fwd", C, M)
    H = 4 * C
    c = Case("mlp_fwd", M, C, H)
    y, w1 = _bf(_u(g, dev, M, C)), _bf(_u(g, dev, H, C) * W1_SCALE * C ** -0.5)
    b1 = _f32(_u(g, dev, H, lo=-2.0, hi=2.0) - W1_SCALE * MU * MU * math.sqrt(C))
    w2, b2 = _bf(_u(g, dev, C, H) * H ** -0.5), _f32(_u(g, dev, C, lo=-0.5, hi=0.5))
    gam, x = _f32(_u(g, dev, C, lo=0.05, hi=0.3)), _f32(_u(g, dev, M, C, lo=-2.0, hi=2.0))
    c.inputs = dict(y=(y, BF), w1=(w1, BF), b1=(b1, F32), w2=(w2, BF), b2=(b2, F32), gamma=(gam, F32), x=(x, F32))
    c.outputs = dict(gh=((M, H), BF, None), a=((M, H), BF, None), out=((M, C), F32, None), out_eval=((M, C), F32, None))
    c.equal = [("out_eval", "out")]

    def run(v, p):
        K.mlp_fwd(v["y"], v["w1"], v["b1"], v["w2"], v["b2"], v["gamma"], v["x"], out=v["out"], gelu_grad=v["gh"],
                  gelu_out=v["a"])
        K.mlp_fwd(v["y"], v["w1"], v["b1"], v["w2"], v["b2"], v["gamma"], v["x"], out=v["out_eval"])

    def ev(t, rnd, got, drop):
        h = _mm(t["y"], t["w1"].T, 32 if drop == "k" else 0) + t["b1"]
        ge, gd = _gelu_pair(h)
        gh, a = rnd(gd, BF), rnd(ge, BF)
        a2 = got["a"] if got is not None else a
        out = t["x"] + t["gamma"] * (_mm(a2, t["w2"].T, 64 if drop == "h" else 0) + t["b2"])
        return dict(gh=gh, a=a, out=out, out_eval=out, _h=h)

    def bounds(t, ref, got, slabs):
        Eh = C * U24 * (t["y"].abs() @ t["w1"].abs().T + t["b1"].abs())
        t_g, t_d = _erf_terms(ref["_h"])
        c.notes[:] = [f"erf terms: GELU {t_g:.2e} GELU' {t_d:.2e}"]
        a2 = got["a"] if got is not None else ref["a"]
        branch = ref["out"] - t["x"]
        bo = t["gamma"].abs() * H * U24 * (a2.abs() @ t["w2"].abs().T + t["b2"].abs()) + U23 * (t["x"].abs() + branch.abs())
        return dict(gh=Eh + t_d + U8 * ref["gh"].abs(), a=1.13 * Eh + t_g + U8 * ref["a"].abs(), out=bo, out_eval=bo)

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one 32-deep k-step of fc1", "k", ("a", "gh")), ("one 64-unit hidden chunk of fc2", "h", ("out",))]
    c.masks = dict(gh=_one_branch)
    return c


# ----------------------------------------------------------------------------------- the LayerNorm backward's pieces
def _ln_operands(g, dev, M, C):
    z = _bf(_n(g, dev, M, C) * _u(g, dev, M, 1, lo=0.5, hi=1.5) + _u(g, dev, M, 1, lo=-1.0, hi=1.0))
    mean = z.mean(1)
    var = ((z - mean[:, None]) ** 2).mean(1)
    return z, _f32(mean), _f32((var + K.EPS_LN).rsqrt()), _f32(_u(g, dev, C, lo=0.5, hi=1.5))


def _ln_weight(g, dev, Kh, C, mean_in):
    """[Kh, C] normal, K^-1/2, with the mean that puts dy's mean at about its spread"""
    e2 = (HI - LO) ** 2 / 12 + MU * MU
    return _n(g, dev, Kh, C) * Kh ** -0.5 + math.sqrt(e2) / (Kh * mean_in)


LN_SUMS = ("dw_pair", "db_pair", "dw_multi", "db_multi")
ROUNDED = {n + "_rounded": n for n in LN_SUMS}  # the same outputs against the reference that rounds dy to bf16


def _ln_ev(t, dy, rnd, drop, C, pr):
    """LayerNorm backward of dy over (z, mean, rstd, lnw): dz (bf16 store) and the weight / bias sums on their
    priors; ``*_rounded``: the sums of bf16(dy), the kernel's own operand (what the float32 evaluation sums anyway)"""
    rs = t["rstd"][:, None]
    xh = (t["z"] - t["mean"][:, None]) * rs
    gq = dy * t["lnw"]
    col = torch.arange(C, device=dy.device)
    # a share of the row sums left out: the first column tile's (gemm9's epilogue), or one of the wave's four lane
    # groups' (mlp_bwd: lane group gq holds the columns 16 cf + 4 gq .. + 3)
    keep = (col >= 256 if drop == "tile" else col % 16 >= 4 if drop == "lane" else col >= 0).to(dy.dtype)
    s1 = (gq * keep).sum(1, keepdim=True) / C
    s2 = (gq * xh * keep).sum(1, keepdim=True) / C
    out = dict(dz=rnd(rs * (gq - s1 - xh * s2), BF), _dy=dy)
    dyr = _bf(dy) if dy.dtype == F64 else dy
    sums = dict(w=(dy * xh).sum(0), b=dy.sum(0), wr=(dyr * xh).sum(0), br=dyr.sum(0))
    if drop == "row":  # a row's term left out, as the RMS over the rows of that term, per channel
        sums["wr"], sums["br"] = sums["wr"] - R._rms0(dyr * xh), sums["br"] - R._rms0(dyr)
    for n in LN_SUMS:
        out[n] = pr[n].to(dy.dtype) + sums[n[1]]
        out[n + "_rounded"] = pr[n].to(dy.dtype) + sums[n[1] + "r"]
    return out


def _ln_bounds(t, dy, e_acc, D, n_of, pr, n_part=None):
    """-> name -> bound for dz (store included) and the sums, and the bare sums' (ref, bound) for the partials; module
    docstring.  ``e_acc``: the f32 accumulation's share of dy's error, ``n_of(multi)``: the folded sums' depth,
    ``n_part``: the bare partials' (no fold, no prior)."""
    e = U8 * dy.abs() + e_acc
    dx, b, xh, dxh = R.ln_bwd_core(dy, t["z"], t["mean"], t["rstd"], t["lnw"], D)
    rs = t["rstd"][:, None]
    ge = t["lnw"].abs() * e
    ext = rs * (ge + ge.mean(1, keepdim=True) + xh.abs() * (ge * xh.abs()).mean(1, keepdim=True))
    out = dict(dz=b + ext + U8 * dx.abs())
    dyr, flip = R.stored(dy, e_acc, BF)
    parts = {}
    for multi, tag in ((False, "pair"), (True, "multi")):
        n = n_of(multi)
        for sfx, d_, err in (("", dy, e), ("_rounded", dyr, flip)):
            tw, bw, tb, bb = R.red_bounds(d_, xh, dxh, n)
            bw, bb = bw + (err * xh.abs()).sum(0), bb + err.sum(0)
            out[f"dw_{tag}{sfx}"] = bw + U23 * (pr["dw_" + tag].abs() + tw.abs())
            out[f"db_{tag}{sfx}"] = bb + U23 * (pr["db_" + tag].abs() + tb.abs())
    if n_part is not None:
        for sfx, d_, err in (("", dy, e), ("_rounded", dyr, flip)):
            tw, bw, tb, bb = R.red_bounds(d_, xh, dxh, n_part)
            parts["dw" + sfx], parts["db" + sfx] = (tw, bw + (err * xh.abs()).sum(0)), (tb, bb + err.sum(0))
    return out, parts


# ------------------------------------------------------------------------------------------------ the fused backward
def _image(where, W, scale, dev):
    """transpose_scale_bf16(W, scale) between sentinels, per element against bf16(W scale)^T, -> float64"""
    want = (W * scale[:, None] if scale is not None else W).T.contiguous()
    if dev.type == "cpu":
        return _bf(want.float())
    v, buf = _guarded(torch.full(tuple(want.shape), NAN, device=dev), BF)
    Wd, sd = W.float().contiguous(), None if scale is None else scale.float().contiguous()
    keep = Wd.clone()
    K.transpose_scale_bf16(Wd, sd, out=v)
    torch.cuda.synchronize()
    assert _guards_intact(buf) and torch.equal(Wd, keep), f"{where}: sentinel or input"
    judge(TAG, where, dict(out=v), dict(out=(want, (U8 + U24) * want.abs())))
    return v.double().clone()


def build_mlp_bwd(M, dev):
    C, H = 128, 512
    g = R._gen("mlp_bwd", M)
    c = Case("mlp_bwd", M, H, C)
    W2f, gam = _f32(_u(g, dev, C, H) * C ** -0.5), _f32(_u(g, dev, C, lo=0.05, hi=0.3))
    gh = _bf(_u(g, dev, M, H, lo=-0.2, hi=1.2))
    W1f = _f32(_ln_weight(g, dev, H, C, 0.5 * MU * C * MU * C ** -0.5 * 0.175))
    w2t = _image(f"transpose_scale_bf16 W2 gamma M={M}", W2f, gam, dev)  # [H, C]
    w1t = _image(f"transpose_scale_bf16 W1 M={M}", W1f, None, dev)  # [C, H]
    d = _bf(_u(g, dev, M, C))
    z, mean, rstd, lnw = _ln_operands(g, dev, M, C)
    pr = {n: _f32(_u(g, dev, C, lo=-3.0, hi=3.0)) for n in ("dw_pair", "db_pair", "dw_multi", "db_multi")}
    c.inputs = dict(d=(d, BF), w2t=(w2t, BF), gh=(gh, BF), w1t=(w1t, BF), z=(z, BF), mean=(mean, F32), rstd=(rstd, F32),
                    lnw=(lnw, F32))
    c.outputs = dict(dh=((M, H), BF, None), dz=((M, C), BF, None), **{n: ((C,), F32, p) for n, p in pr.items()})
    c.parts = []
    tiles = -(-M // 128)
    grid = min(tiles, 512)
    n_part = 8 * -(-tiles // grid) + 4  # a wave's fragments over its tiles, the 4 shuffles

    def run(v, p):
        with _nan_empty():
            part, P = K.mlp_bwd(v["d"], v["w2t"], v["gh"], v["w1t"], v["z"], v["mean"], v["rstd"], v["lnw"], dh=v["dh"],
                                dz=v["dz"])
        assert P == 4 * grid and tuple(part.shape) == (2, P, C), (P, grid, tuple(part.shape))
        K.reduce_pair(part[0], v["dw_pair"], part[1], v["db_pair"], P)
        K.reduce_multi([(part[0], v["dw_multi"], P, True), (part[1], v["db_multi"], P, True)])
        c.parts.append(part)

    def ev(t, rnd, got, drop):
        dh = rnd(_mm(t["d"], t["w2t"].T, 32 if drop == "k" else 0) * t["gh"], BF)
        dh2 = got["dh"] if got is not None else dh
        dy = rnd(_mm(dh2, t["w1t"].T, 32 if drop == "k2" else 0), BF)
        return dict(_ln_ev(t, dy, rnd, drop, C, pr), dh=dh)

    def bounds(t, ref, got, slabs):
        dh2 = got["dh"] if got is not None else ref["dh"]
        out, c.part_refs = _ln_bounds(t, ref["_dy"], H * U24 * (dh2.abs() @ t["w1t"].abs().T), 32 + 2,
                                      lambda multi: n_part + R.fold_depth(4 * grid, C, C, multi), pr, n_part)
        out["dh"] = t["gh"].abs() * C * U24 * (t["d"].abs() @ t["w2t"].abs().T) + U8 * ref["dh"].abs()
        return out

    c.run, c.ev, c.bounds = run, ev, bounds
    c.aliases = ROUNDED
    c.drops = [("one 32-deep k-step of the fc2 data gradient", "k", ("dh",)),
               ("one lane group's share of the row sums", "lane", ("dz",)),
               ("one 32-deep k-step of the fc1 data gradient", "k2", (), ("dz",)),
               ("one row of the LayerNorm weight / bias sums (the RMS over the rows of its term, per channel)", "row",
                tuple(ROUNDED))]
    return c


# ------------------------------------------------------------------------ the LayerNorm backward in the fc1 dgrad
def build_dgrad_ln(C, M, dev):
    Kh = 4 * C
    g = R._gen("dgrad_ln", C, M)
    c = Case("dgrad_ln", M, C, Kh)
    dh, w = _bf(_u(g, dev, M, Kh)), _bf(_ln_weight(g, dev, Kh, C, MU))
    z, mean, rstd, lnw = _ln_operands(g, dev, M, C)
    pr = {n: _f32(_u(g, dev, C, lo=-3.0, hi=3.0)) for n in ("dw_pair", "db_pair", "dw_multi", "db_multi")}
    c.inputs = dict(dh=(dh, BF), w=(w, BF), z=(z, BF), mean=(mean, F32), rstd=(rstd, F32), lnw=(lnw, F32))
    c.outputs = dict(dz=((M, C), BF, None), dz_multi=((M, C), BF, None), **{n: ((C,), F32, p) for n, p in pr.items()})
    c.equal = [("dz_multi", "dz")]
    c.taken = True
    P = -(-M // 128)

    def run(v, p):
        for tag in ("pair", "multi"):
            torch.cuda.synchronize()
            K._LN_XCH.clear()  # the wrapper caches its exchange workspace per stream: a fresh, NaN-filled one per call
            with _nan_empty():
                fused = K.linear_dgrad_ln(v["dh"], v["w"], v["z"], v["mean"], v["rstd"], v["lnw"], dw=v["dw_" + tag],
                                          db=v["db_" + tag], policy=p)
            if fused is None:  # the wrapper's two-pass answer: nothing to check
                c.taken = False
                return
            dz, finish = fused
            if tag == "pair":
                finish()
                v["dz"].copy_(dz)
            else:
                folds = []
                finish(defer=folds)
                K.reduce_multi(folds)
                v["dz_multi"].copy_(dz)

    def ev(t, rnd, got, drop):
        out = _ln_ev(t, rnd(t["dh"] @ t["w"], BF), rnd, drop, C, pr)
        return dict(out, dz_multi=out["dz"])

    def bounds(t, ref, got, slabs):
        out, _ = _ln_bounds(t, ref["_dy"], Kh * U24 * (t["dh"].abs() @ t["w"].abs()), 16 + 2 + 4 + C // 256,
                            lambda multi: 8 + 4 + R.fold_depth(P, C, C, multi), pr)
        return dict(out, dz_multi=out["dz"])

    c.run, c.ev, c.bounds = run, ev, bounds
    c.aliases = ROUNDED
    c.drops = [("the first column tile's share of the row sums", "tile", ("dz",)),
               ("one row of the LayerNorm weight / bias sums (the RMS over the rows of its term, per channel)", "row",
                tuple(ROUNDED))]
    return c


# ------------------------------------------------------------------------------------------------ the unfused calls
FWD = ("fc1_fwd", "fc2_fwd", "fc2_fwd_ones", "ds_fwd", "stem_fwd")
DGRAD = ("fc2_dgrad", "fc2_dgrad_v2", "fc1_dgrad", "ds_dgrad")
WGRAD = ("fc1_wgrad", "fc1_wgrad_defer", "fc2_lswgrad", "ds_wgrad", "stem_wgrad")
BLOCK_C, DS_C, STEM_C = (96, 128, 256, 512, 1536), (96, 128, 256, 512), (96, 128, 192)
ROWS = (16, 400, 1400, 1600)
STEM_IMG = {16: (1, 16, 16), 400: (1, 80, 80), 1400: (2, 100, 112), 1600: (1, 160, 160)}  # M = B (H / 4) (W / 4)
F32_C, F32_ROWS = (96, 128, 384), (16, 400, 1400)
F32_KINDS = ("fc1_fwd", "fc2_fwd", "ds_fwd", "fc2_dgrad", "fc1_dgrad", "ds_dgrad", "fc1_wgrad", "fc1_wgrad_defer",
             "fc2_lswgrad", "ds_wgrad")


def _stem_patches(g, dev, M):
    """stem_patchify's rows of an image uniform on [0.3, 1] (normalised: signed, mean about 0.9): [M, 64] bf16, k =
    ci 16 + kh 4 + kw, 48..63 zero -- the kernel's on the GPU, the same layout by torch for the CPU-side conditions"""
    B, H, W = STEM_IMG[M]
    img = _u(g, CPU, B, 3, H, W, lo=0.3, hi=1.0).float()
    if dev.type != "cpu":
        return K.stem_patchify(img.to(dev).contiguous()).double()
    mean, std = (torch.tensor(v_, dtype=F32).view(1, 3, 1, 1) for v_ in (K.IMAGENET_MEAN, K.IMAGENET_STD))
    p = ((img - mean) / std).view(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, 48)
    return _bf(torch.cat([p, torch.zeros(M, 16)], 1))


class _Arm:
    """The compute arm of one unfused call (bf16 or fp32 compute) and the case's operand stream."""

    def __init__(self, kind, C, M, dev, bf):
        self.g, self.dev, self.bf = R._gen(kind, C, M, bf), dev, bf
        self.adt = BF if bf else F32  # the activations' dtype
        self.cdt = dict(compute_bf16=bf)

    def rt(self, t):
        return _bf(t) if self.bf else _f32(t)

    def acc(self, Kd, extra=0):
        """the accumulation's roundings x 2^-24 (module docstring): K, or 2K (+ extra) on the fp32 arm"""
        return (Kd if self.bf else 2 * Kd + extra) * U24

    def u(self, *shape, lo=LO, hi=HI):
        return _u(self.g, self.dev, *shape, lo=lo, hi=hi)

    def op(self, *shape, k=None):
        return self.rt(self.u(*shape) * (k ** -0.5 if k else 1.0))

    def vec(self, n, lo, hi):
        return _f32(self.u(n, lo=lo, hi=hi))


def _fc1_fwd(a, kind, C, M):
    """466 / 470: gh = GELU'(h), a = GELU(h) of h = A W^T + b, dual and single-output forms"""
    H, adt = 4 * C, a.adt
    c = Case(kind, M, H, C)
    A, W = a.op(M, C), a.rt(a.u(H, C) * W1_SCALE * C ** -0.5)
    b = _f32(a.u(H, lo=-2.0, hi=2.0) - W1_SCALE * MU * MU * math.sqrt(C))
    c.inputs = dict(A=(A, adt), W=(W, adt), bias=(b, F32))
    c.outputs = dict(gh=((M, H), adt, None), a=((M, H), adt, None), a_eval=((M, H), adt, None))
    c.equal = [("a_eval", "a")]

    def run(v, p):
        K.linear_fwd(v["A"], v["W"], out=v["gh"], out2=v["a"], bias=v["bias"], epilogue=nv.SV_EPI_BIAS_GELU_DUAL,
                     policy=p, **a.cdt)
        K.linear_fwd(v["A"], v["W"], out=v["a_eval"], bias=v["bias"], epilogue=nv.SV_EPI_BIAS_GELU, policy=p, **a.cdt)

    def ev(t, rnd, got, drop):
        h = _mm(t["A"], t["W"].T, 32 if drop else 0) + t["bias"]
        ge, gd = _gelu_pair(h)
        return dict(gh=rnd(gd, adt), a=rnd(ge, adt), a_eval=rnd(ge, adt), _h=h)

    def bounds(t, ref, got, slabs):
        Eh = a.acc(C) * (A.abs() @ W.abs().T + b.abs())
        t_g, t_d = _erf_terms(ref["_h"])
        c.notes[:] = [f"erf terms: GELU {t_g:.2e} GELU' {t_d:.2e}"]
        ba = 1.13 * Eh + t_g + _store(ref["a"], adt)
        return dict(gh=Eh + t_d + _store(ref["gh"], adt), a=ba, a_eval=ba)

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one 32-deep k-step", "k", ("a", "gh"))]
    c.masks = dict(gh=_one_branch)
    return c


def _fc2_fwd(a, kind, C, M):
    """484 / 481: out = res + gamma (A W^T + b), gamma random or ones"""
    H, adt = 4 * C, a.adt
    c = Case(kind, M, C, H)
    A, W, b = a.op(M, H), a.op(C, H, k=H), a.vec(C, -0.5, 0.5)
    gam = torch.ones(C, device=a.dev, dtype=F64) if kind == "fc2_fwd_ones" else a.vec(C, 0.05, 0.3)
    res = _f32(a.u(M, C, lo=-2.0, hi=2.0))
    c.inputs = dict(A=(A, adt), W=(W, adt), bias=(b, F32), gamma=(gam, F32), res=(res, F32))
    c.outputs = dict(out=((M, C), F32, None))

    def run(v, p):
        K.linear_fwd(v["A"], v["W"], out=v["out"], bias=v["bias"], gamma=v["gamma"], residual=v["res"],
                     epilogue=nv.SV_EPI_BIAS_GAMMA_RES, policy=p, **a.cdt)

    def ev(t, rnd, got, drop):
        return dict(out=t["res"] + t["gamma"] * (_mm(t["A"], t["W"].T, 32 if drop else 0) + t["bias"]))

    def bounds(t, ref, got, slabs):
        branch = ref["out"] - res
        return dict(out=gam.abs() * a.acc(H) * (A.abs() @ W.abs().T + b.abs()) + U23 * (res.abs() + branch.abs()))

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one 32-deep k-step", "k", ("out",))]
    return c


def _scaled_weight(Wf, gam, dev):
    """scale_rows_bf16(Wf, gam) between sentinels, per element against bf16(Wf gam[:, None]), -> float64"""
    want = Wf * gam[:, None]
    if dev.type == "cpu":
        return _bf(want.float())
    wv, wb = _guarded(torch.full(tuple(Wf.shape), NAN, device=dev), BF)
    K.scale_rows_bf16(Wf.float(), gam.float(), out=wv)
    torch.cuda.synchronize()
    assert _guards_intact(wb), "scale_rows_bf16: sentinel overwritten"
    judge(TAG, f"scale_rows_bf16 C={Wf.shape[0]}", dict(out=wv), dict(out=(want, (U8 + U24) * want.abs())))
    return wv.double().clone()


def _fc2_dgrad(a, kind, C, M):
    """605: out = ((A) (W gamma)) aux with the scale_rows_bf16 weight; fp32 arm, 607: ((A gamma) W) aux, a_scale_k"""
    H, adt, bf = 4 * C, a.adt, a.bf
    c = Case(kind, M, H, C)
    A, aux = a.op(M, C), a.rt(a.u(M, H, lo=-0.2, hi=1.2))
    Wf, gam = _f32(a.u(C, H) * C ** -0.5), a.vec(C, 0.05, 0.3)
    W = _scaled_weight(Wf, gam, a.dev) if bf else Wf
    c.inputs = dict(A=(A, adt), W=(W, adt), aux=(aux, adt))
    if not bf:
        c.inputs["gamma"] = (gam, F32)
    c.outputs = dict(out=((M, H), adt, None))

    def run(v, p):
        K.linear_dgrad(v["A"], v["W"], out=v["out"], epilogue=nv.SV_EPI_MUL_AUX, a_scale_k=None if bf else v["gamma"],
                       aux=v["aux"], policy=p, **a.cdt)

    def ev(t, rnd, got, drop):
        As = t["A"] if bf else rnd(t["A"] * t["gamma"], F32)
        return dict(out=rnd(_mm(As, t["W"], 32 if drop else 0) * t["aux"], adt))

    def bounds(t, ref, got, slabs):
        As = A if bf else A * gam
        return dict(out=aux.abs() * a.acc(C, 1) * (As.abs() @ W.abs()) + _store(ref["out"], adt))

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one 32-deep k-step", "k", ("out",))]
    return c


def _plain(a, kind, C, M):
    """out = A [M, Kd] . W (+ bias), stored as is: the forward calls through linear_fwd (W [N, Kd], bias), the data
    gradients through linear_dgrad (W [Kd, N]).  529, 621, 685, 437, 416."""
    fwd, adt = kind.endswith("_fwd"), a.adt
    N, Kd, odt = {"fc2_dgrad_v2": (4 * C, C, adt), "fc1_dgrad": (C, 4 * C, adt), "ds_dgrad": (4 * C, 2 * C, F32),
                  "ds_fwd": (2 * C, 4 * C, F32), "stem_fwd": (C, 64, BF)}[kind]
    c = Case(kind, M, N, Kd)
    if kind == "stem_fwd":
        A = _stem_patches(a.g, a.dev, M)
        w4 = _f32(a.u(C, 3, 4, 4) * 48 ** -0.5)
        W = (K.stem_weight_pack(w4.float().contiguous()).double() if a.dev.type != "cpu"
             else _bf(torch.cat([w4.view(C, 48), torch.zeros(C, 16, dtype=F64)], 1)))
    else:
        A, W = a.op(M, Kd), a.op(*((N, Kd) if fwd else (Kd, N)), k=Kd)
    c.inputs = dict(A=(A, adt), W=(W, adt))
    b = a.vec(N, -0.5, 0.5) if fwd else None
    if fwd:
        c.inputs["bias"] = (b, F32)
    c.outputs = dict(out=((M, N), odt, None))

    def run(v, p):
        if fwd:
            K.linear_fwd(v["A"], v["W"], out=v["out"], bias=v["bias"], policy=p, **a.cdt)
        else:
            K.linear_dgrad(v["A"], v["W"], out=v["out"], policy=p, **a.cdt)

    def ev(t, rnd, got, drop):
        k0 = 32 if drop else 0
        return dict(out=rnd(_mm(t["A"], t["W"].T, k0) + t["bias"] if fwd else _mm(t["A"], t["W"], k0), odt))

    def bounds(t, ref, got, slabs):
        S = A.abs() @ W.abs().T + b.abs() if fwd else A.abs() @ W.abs()
        return dict(out=a.acc(Kd) * S + _store(ref["out"], odt))

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one 32-deep k-step", "k", ("out",))]
    return c


def _wgrad(a, kind, C, M):
    """570 / 577, 686, 699: dw = prior + dy^T x[:, :Kd], db = prior + colsum(dy) through linear_wgrad"""
    bf, adt = a.bf, a.adt
    N, Kd = {"fc1": (4 * C, C), "ds_": (2 * C, 4 * C), "ste": (C, 48)}[kind[:3]]
    target = WGRAD_TARGET if kind.startswith("fc1") else None
    split = K._wgrad_split_for(N, Kd, M, target)
    c = Case(kind, M, N, M, wgrad=True, split=split)
    c.slab_ok = lambda policy: K._bf16_slabs(N, Kd, M, split, bf, policy)
    dy = a.op(M, N)
    x = _stem_patches(a.g, a.dev, M) if kind == "stem_wgrad" else a.op(M, Kd)
    pw, pb = _f32(a.u(N, Kd, lo=-3.0, hi=3.0)), a.vec(N, -3.0, 3.0)
    c.inputs = dict(dy=(dy, adt), x=(x, adt))
    c.outputs = dict(dw=((N, Kd), F32, pw), db=((N,), F32, pb))
    kw = dict(accumulate=True, **a.cdt)
    if target:
        kw["wgrad_target"] = target
    if kind == "stem_wgrad":
        kw["cols"] = 48

    def run(v, p):
        if kind == "fc1_wgrad_defer":
            folds = []
            K.linear_wgrad(v["dy"], v["x"], out=v["dw"], bias_out=v["db"], defer=folds, policy=p, **kw)
            K.reduce_multi(folds)
        else:
            K.linear_wgrad(v["dy"], v["x"], out=v["dw"], bias_out=v["db"], policy=p, **kw)

    def ev(t, rnd, got, drop):
        r0 = 1 if drop else 0
        return dict(dw=pw.to(t["dy"].dtype) + t["dy"][r0:].T @ t["x"][r0:, :Kd],
                    db=pb.to(t["dy"].dtype) + t["dy"][r0:].sum(0))

    Gs = {}

    def bounds(t, ref, got, slabs):
        if not Gs:
            Gs["G"], Gs["E"] = _wgrad_terms(dy, x[:, :Kd], M, split)
        G, cs, f = Gs["G"], dy.sum(0), 1 if bf else 2
        return dict(dw=f * Gs["E"](slabs) + U23 * (pw.abs() + G.abs()),
                    db=f * M * U24 * dy.abs().sum(0) + U23 * (pb.abs() + cs.abs()))

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one row of the weight gradient", "row", ("dw", "db"))]
    return c


def _lswgrad(a, kind, C, M):
    """565: dw2 += gamma (.) G, dgamma += rowdot(W2, G) + b2 (.) colsum(d), db2 += gamma (.) colsum(d), G = d^T a"""
    bf, adt, K4 = a.bf, a.adt, 4 * C
    split = K._wgrad_split_for(C, K4, M, WGRAD_TARGET)
    c = Case(kind, M, C, M, wgrad=True, split=split)
    c.slab_ok = lambda policy: K._bf16_slabs(C, K4, M, split, bf, policy)
    dy, x = a.op(M, C), a.op(M, K4)
    W2, gam, b2 = _f32(a.u(C, K4) * K4 ** -0.5), a.vec(C, 0.05, 0.3), a.vec(C, -0.5, 0.5)
    pw, pg, pb = _f32(a.u(C, K4, lo=-3.0, hi=3.0)), a.vec(C, -3.0, 3.0), a.vec(C, -3.0, 3.0)
    c.inputs = dict(dy=(dy, adt), x=(x, adt), W2=(W2, F32), gamma=(gam, F32), b2=(b2, F32))
    c.outputs = dict(dw2=((C, K4), F32, pw), dgamma=((C,), F32, pg), db2=((C,), F32, pb))

    def run(v, p):
        K.layerscale_wgrad(v["dy"], v["x"], v["W2"], v["gamma"], v["b2"], dw2=v["dw2"], dgamma=v["dgamma"],
                           db2=v["db2"], policy=p, wgrad_target=WGRAD_TARGET, **a.cdt)

    def ev(t, rnd, got, drop):
        r0 = 1 if drop else 0
        P_ = t["dy"].dtype
        G, cs = t["dy"][r0:].T @ t["x"][r0:], t["dy"][r0:].sum(0)
        return dict(dw2=pw.to(P_) + t["gamma"][:, None] * G, dgamma=pg.to(P_) + (t["W2"] * G).sum(1) + t["b2"] * cs,
                    db2=pb.to(P_) + t["gamma"] * cs)

    Gs = {}

    def bounds(t, ref, got, slabs):
        if not Gs:
            Gs["G"], Gs["E"] = _wgrad_terms(dy, x, M, split)
        f = 1 if bf else 2
        G, E, cs, Ecs = Gs["G"], f * Gs["E"](slabs), dy.sum(0), f * M * U24 * dy.abs().sum(0)
        gG, dotabs = gam[:, None] * G, (W2 * G).abs().sum(1)
        return dict(dw2=gam.abs()[:, None] * E + U23 * (pw.abs() + gG.abs()),
                    dgamma=(W2.abs() * E).sum(1) + K4 * U24 * dotabs + b2.abs() * Ecs
                    + U23 * (pg.abs() + dotabs + (b2 * cs).abs()),
                    db2=gam.abs() * Ecs + U23 * (pb.abs() + (gam * cs).abs()))

    c.run, c.ev, c.bounds = run, ev, bounds
    c.drops = [("one row of the weight gradient", "row", ("dw2", "dgamma", "db2"))]
    return c


BUILDERS = dict(fc1_fwd=_fc1_fwd, fc2_fwd=_fc2_fwd, fc2_fwd_ones=_fc2_fwd, fc2_dgrad=_fc2_dgrad, fc2_dgrad_v2=_plain,
                fc1_dgrad=_plain, ds_dgrad=_plain, ds_fwd=_plain, stem_fwd=_plain, fc1_wgrad=_wgrad,
                fc1_wgrad_defer=_wgrad, ds_wgrad=_wgrad, stem_wgrad=_wgrad, fc2_lswgrad=_lswgrad)


def build_call(kind, C, M, dev, bf=True):
    """The unfused call ``kind`` at width C and M rows; ``bf``: the bf16-compute arm, else the fp32-compute one."""
    return BUILDERS[kind](_Arm(kind, C, M, dev, bf), kind, C, M)


# ------------------------------------------------------------------------------------------------------- policies
@functools.lru_cache(maxsize=None)
def _backward_policies():
    """(data-gradient policy, side-stream weight-gradient policy) as ConvNeXtHip._backward_impl builds them"""
    from spine_vision_amd.backbone import convnext as cx
    from spine_vision_amd.backbone import create_convnext

    hip = create_convnext("convnext_tiny", precision="bf16")
    assert hip.overlap_wgrad and hip.wgrad_target == WGRAD_TARGET and hip.merge_folds and hip.main_bwd_cap == 0
    pol = nv.policy(grid_cap=cx._comm_cap(torch.device("cuda:0"), hip.comm_reserve_cus), wg_per_cu=hip.side_wg_per_cu)
    return pol, cx._WgradSchedule(hip, None, None, False, pol).spol


def _policies(c, bf=True):
    out = {"default": None}
    if bf:
        if c.Kg % 64 == 0:
            out["v2"] = nv.policy(impl=2)
        if c.Kg % 32 == 0:
            out["v3"] = nv.policy(impl=3)
            out["v8"] = nv.policy(impl=8)
        if c.Kg % (c.split * 64) == 0:
            out["v9"] = nv.policy(impl=9)
            out["v9cap4"] = nv.policy(impl=9, grid_cap=4)
    if c.kind not in FWD:
        pol, spol = _backward_policies()
        out["bwd"] = spol if c.kind in ("fc1_wgrad", "fc1_wgrad_defer", "fc2_lswgrad") else pol
    return out


def _judge_case(c, policy, where, staged=False):
    first = _run_guarded(c, policy, where)
    got = {n: t.double() for n, t in first.items()} if staged else None
    judge(TAG, where, dict(first, **{a: first[n] for a, n in c.aliases.items()}), c.make_refs(got, c.slab_ok(policy)))
    _equal_pairs(c, first, where)
    for s in c.notes:
        print(f"[{TAG}] {where}: {s}")
    return first


def _unfused(dev, kind, C, M, bf):
    c = build_call(kind, C, M, dev, bf)
    for pname, pol in _policies(c, bf).items():
        slab = f" split {c.split}{' bf16 slabs' if c.slab_ok(pol) else ''}" if c.wgrad else ""
        _judge_case(c, pol, f"{kind}{'' if bf else '[f32]'} C={C} M={M}{slab} policy={pname}")


def _widths(kind):
    return STEM_C if kind.startswith("stem") else DS_C if kind.startswith("ds_") else BLOCK_C


GRID = [(k, C, M) for k in FWD + DGRAD + WGRAD for C in _widths(k) for M in ROWS if C < 1536 or M <= 400]


@gpu
@pytest.mark.parametrize("kind,C,M", GRID, ids=[f"{k}-C{C}-M{M}" for k, C, M in GRID])
def test_call_against_float64(dev, kind, C, M):
    """2: the bf16-compute calls, every policy whose contract the shape meets"""
    _unfused(dev, kind, C, M, True)


GRID32 = [(k, C, M) for k in F32_KINDS for C in F32_C for M in F32_ROWS]


@gpu
@pytest.mark.parametrize("kind,C,M", GRID32, ids=[f"{k}-C{C}-M{M}" for k, C, M in GRID32])
def test_f32_arm_against_float64(dev, kind, C, M):
    """3: compute_bf16=False, default policy and the backward's"""
    _unfused(dev, kind, C, M, False)


# ---------------------------------------------------------------------------------------------- the fused kernels
def _multi_tile_rows(dev, C):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return (2 * cus if C == 128 else cus) * 128 + 133


@gpu
@pytest.mark.parametrize("M", (1, 127, 128, 129, 1000, "multi"))
@pytest.mark.parametrize("C", K.MLP_FUSED_C)
def test_mlp_fwd(dev, C, M):
    """1: sv_mlp_fwd, training and eval forms; gh and a against float64 h, x_out against the kernel's own a"""
    M = _multi_tile_rows(dev, C) if M == "multi" else M
    c = build_mlp_fwd(C, M, dev)
    _judge_case(c, None, f"mlp_fwd C={C} M={M}", staged=True)
    del c
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("M", (1, 127, 129, 1000, 512 * 128 + 133))
def test_mlp_bwd(dev, M):
    """1: sv_mlp_bwd at C = 128: dh, dz, the per-wave partials (all rows written) and both folds"""
    c = build_mlp_bwd(M, dev)
    where = f"mlp_bwd C=128 M={M}"
    _judge_case(c, None, where, staged=True)
    a, b = c.parts
    assert torch.equal(_bits(a), _bits(b)), f"{where}: partials differ run to run"
    assert bool(torch.isfinite(a).all()), f"{where}: a partial row was not written"
    sw, sb = a[0].double().sum(0), a[1].double().sum(0)
    judge(TAG, where + " partials", dict(dw=sw, db=sb, dw_rounded=sw, db_rounded=sb), c.part_refs)
    del c
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("pname", ("default", "bwd"))
@pytest.mark.parametrize("M", (8, 256, 264, 1000))
@pytest.mark.parametrize("C", (512, 1024))
def test_linear_dgrad_ln(dev, C, M, pname):
    """1: SV_EPI_LN_BWD through kernels.linear_dgrad_ln only (the wrapper guarantees the residency its polling needs)"""
    c = build_dgrad_ln(C, M, dev)
    pol = None if pname == "default" else _backward_policies()[0]
    where = f"linear_dgrad_ln C={C} M={M} policy={pname}"
    views = {}
    for n, (t, dt_) in c.inputs.items():
        views[n] = _guarded(t, dt_)[0]
    for n, (shape, dt_, prior) in c.outputs.items():
        views[n] = _guarded(torch.zeros(shape, device=dev) if prior is None else prior, dt_)[0]
    c.run(views, pol)  # does the wrapper take the fused form here?
    torch.cuda.synchronize()
    # default policy: at most 4 x 4 tiles, every one resident on any chip with 16 CUs; None would be a regression
    assert c.taken or pname != "default", f"{where}: the wrapper declined a shape it must take"
    if not c.taken:
        print(f"[{TAG}] {where}: the wrapper returned None (two-pass form): nothing to check")
        return
    _judge_case(c, pol, where)


# ------------------------------------------------------------------------------------------------ CPU side, no GPU
def _conditions(label, c, lines, missed, need_share=True):
    """(a) the float32 evaluation within 1 x bound in every element; (b) each drop visible in >= 0.99 of its elements"""
    t64 = c.t64()
    emu = c.ev({n: t.float() for n, t in t64.items()}, _round32, None, None)
    got = {n: emu[n].double() for n in list(c.outputs) + list(c.aliases)}
    refs = c.make_refs(got, False)
    for n in got:
        ref, bound = refs[n]
        r = float(((got[n] - ref).abs() / bound.clamp_min(1e-300)).max())
        lines.append(f"{label} {n}: float32 evaluation, largest error / bound {r:.3f}")
        if not r <= 1.0:
            missed.append(lines[-1])
    if not need_share:
        return
    for what, drop, names, *info in c.drops:
        moved = c.ev(t64, _ident, got, drop)
        full = c.ev(t64, _ident, got, None)
        for n in names + (info[0] if info else ()):
            ref, bound = refs[n]
            vis = (moved[n] - ref).abs() > 4 * bound
            if n in c.masks:
                vis = vis[c.masks[n](full, moved)]
            share = float(vis.double().mean())
            lines.append(f"{label} {n}: without {what}, share of {vis.numel()} elements moved by > 4 x bound {share:.4f}"
                         + (" (on one branch of GELU')" if n in c.masks else "")
                         + ("" if n in names else " (reported, not a condition: module docstring)"))
            if n in names and not share >= 0.99:
                missed.append(lines[-1])


def test_reference_side_conditions():
    """Module docstring, last paragraph.  The figures printed here are profiles/convnext_mlp_calls/cpu_conditions.txt."""
    lines, missed = [], []
    for kind in FWD + DGRAD + WGRAD:
        C = _widths(kind)[0]
        for bf in (True, False) if kind in F32_KINDS else (True,):
            arm = "" if bf else "[f32]"
            c = build_call(kind, C, 16, CPU, bf)
            few = all(math.prod(c.outputs[n][0]) < 1000 for d_ in c.drops for n in d_[2])
            _conditions(f"{kind}{arm} C={C} M=16", c, lines, missed, need_share=not few)
            if few:
                _conditions(f"{kind}{arm} C={C} M=400", build_call(kind, C, 400, CPU, bf), lines, missed)
    _conditions("mlp_fwd C=128 M=1", build_mlp_fwd(128, 1, CPU), lines, missed, need_share=False)
    _conditions("mlp_fwd C=128 M=127", build_mlp_fwd(128, 127, CPU), lines, missed)
    _conditions("mlp_bwd C=128 M=1", build_mlp_bwd(1, CPU), lines, missed, need_share=False)
    _conditions("mlp_bwd C=128 M=127", build_mlp_bwd(127, CPU), lines, missed)
    _conditions("linear_dgrad_ln C=512 M=8", build_dgrad_ln(512, 8, CPU), lines, missed)
    print("\n".join(f"[{TAG} cpu] {s}" for s in lines))
    assert not missed, "\n".join(missed)
