"""Every dense-convolution kernel call of a ResNet step (csrc/conv.hip and the gathered modes 1-6 of csrc/gemm3.hip),
one call at a time through the ``spine_vision_amd.kernels`` wrapper and argument form ``backbone/resnet.py`` uses, each
output compared ELEMENT BY ELEMENT with a float64 CPU evaluation of the same operation on the same rounded operands
(tests/_conv_ref.py: ``F.conv2d``, ``conv_transpose2d`` and conv2d's autograd, cached per case).  The older tests bound
whole tensors in relative L2 (1.5e-2 in bf16) or compare one kernel arm with another; a wrong border row of one tap, a
slice that drops its last k-step, a wrong last row tile or an unwritten padded-channel column stays below those.

Calls (resnet.py line mirrored -> test here)
    314 / 320  conv_weight_pack(w f32, Cs, act_dtype)                               -> test_weight_pack
    398        conv_weight_pack_multi([(w, Cs), ...], act_dtype)                    -> test_weight_pack
    324        conv_fwd(x, wp, s, act_dtype) (eval; f32 y: the fp32 model)           -> test_conv_fwd
    322        conv_fwd_bn_stats(x, wp, s, bf16) -> (y, partials)                   -> test_conv_fwd
    581        conv_bwd_data(dy, wp, s, dx_dtype=act_dtype, policy=pol)             -> test_conv_bwd_data [store_bf16]
    599        conv_bwd_data(dy, wp, s, dx_dtype=grad_dtype, policy=pol)            -> test_conv_bwd_data [store_f32]
    600 / 604  conv_bwd_data(dy, wp, s, dx=dx, accumulate=True, policy=pol), dx bf16 (the bf16 gradient stream) or f32
                                                                                    -> test_conv_bwd_data [acc_bf16, acc_f32]
    577        conv_bwd_data_bn(dy, wp, s, y, mean, rstd, gamma, beta, policy=pol)  -> test_conv_bwd_data_bn
    488 / 491  conv_bwd_weight(dy, x, s, dw=dw, accumulate=True, policy=spol) onto a non-zero prior, and
               accumulate=False                                                     -> test_conv_bwd_weight
Policies: None, ``nv.policy(grid_cap=3)`` (asserted below tiles x split from the tile arithmetic: one persistent
workgroup walks several tiles; a case with too few tiles widens its GEMM N (Cout; Cs for a data gradient) or adds batch
images for this policy only, keeping its arm) and the model's own ``nv.policy(grid_cap=ncu * 3 // 4)``
(``_flush_wgrads``).  The register-staged kernels of conv.hip (fp32 mode, the weight-gradient fallback) launch one
workgroup per tile whatever the policy says, so they run ``policy=None`` alone.

Arms.  Tiles are 256 x 128 (register-staged: 128 x 128), k-steps 32 deep.  Every case names the arm it must take and
asserts it from the host predicates ``_pointwise``, ``_gathered``, ``_stem8``, ``_conv_split``, ``_s2_direct``,
``_s2_split``; the weight gradient from _conv_ref's restatement of ``wgrad_transposed`` / ``wgrad_split3`` /
``wgrad_split``, itself cross-checked against ``sv_conv_bwd_weight_work_floats`` - a retune makes the case fail instead
of silently testing another arm.  The case tables below give shape -> arm.

Bound, per element, derived (not tuned).  ``ref`` is the float64 result, ``S`` the same operation over |operands|.
  accumulation  bf16 products are exact in f32 and an f32 sum of n terms in any order errs by at most n 2^-24 S;
                n = the GEMM's K (taps x channels, the stem's padded to 416; pixels for a weight gradient).  Split-K:
                (kper + split) 2^-24 S, the slab sums and the fold bounded separately (kper: gemm3.hip / conv.hip round
                K / split up to whole k-steps).  fp32 mode: (n + 1) 2^-24 S, the products round too.
  store         + 2^-8 |ref| for a bf16 store, 2^-23 |ref| for an f32 one; accumulating forms take the f32 term on the
                addends, 2^-23 (|prior| + |term|), and a bf16 dx its store on top.
  partials      every kernel that emits statistics sums the ROUNDED STORED value, read from the code:
                wave_group_epilogue (gemm_common.h) kStats rounds each value through f2bf before cs1 / cs2, kBnb rounds
                ``slab[...]`` through f2bf before the mask; slab_finish_kernel and slab_finish_bnb_kernel (gemm.hip)
                unpack the bf16 word they just stored.  So the float64 partial is built from the kernel's own stored
                output (checked per element against float64 in the same run) and no 2^-8 sum |.| term applies:
                sum y within 64 2^-24 sum |y|; sum y^2 within 65 2^-24 sum y^2 (fmaf); sum g within
                64 2^-24 sum |g|; sum g xhat within 68 2^-24 sum |g xhat| (xhat = (y - mean) rstd: two roundings, the
                product one more).  Every partial row and channel is compared, in the layout [ceil(M/64)][2][C], for
                stride 2 [4][ceil(M/4/64)][2][C] (class c = 2 py + px, rows in the class's own (b, gy, gx) order).
                Mask: elements whose argument beta + gamma rstd (y - mean) lies within 4 x 2^-24 (|beta| + |gamma rstd
                (y - mean)|) of zero are excluded - the partial that holds one widens by that element's own |g| and
                |g xhat| - counted, printed, and capped at 0.1 % (the CPU test shows the drawn operands stay under it).
  assertion     |got - ref| <= 2 x bound for EVERY element.
  sensitivity   the worst-case bound grows as K^2, a dropped k-step's damage as sqrt(K); so each case asserts, from the
                reference side only, that for at least 99 % of its elements 2 x bound is below the RMS contribution of
                one 32-deep k-step, sqrt(32) rms(a) rms(b) of its operands (test_reference_side_conditions runs this
                and the mask cap for the whole case list without a GPU).

Guards: outputs start as NaN (accumulating ones as their non-zero prior); every input, output, workspace and partials
buffer sits between sentinels that must be intact; inputs must be unchanged; every call runs twice with bit-equal
results.  A 1x1 stride-2 plain store must leave the three tap-less parity classes exactly zero, an accumulate exactly
the prior.  The wrappers take ``out=`` / ``part=`` / ``work=`` for this; the default is a fresh allocation as before.

The figures of the first run are recorded in profiles/resnet_calls/parity.txt."""
import ctypes
import functools

import pytest
import torch

import _conv_ref as R
from _conv_ref import BF, F32, U23, U24, cdiv
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
SENTINEL = -7.0  # exactly representable in bf16 and f32
GUARD = 256  # sentinel elements on either side (keeps the views 16-byte aligned)
TORCH_DT = {"bf16": BF, "fp32": F32}


def sh(B, H, W, Cs, Cout, k, stride, pad, Cin=None):
    return (B, H, W, Cs, Cout, k, stride, pad, Cs if Cin is None else Cin)


def shape_str(shape):
    return ",".join(map(str, shape[:8])) + (f"(Cin {shape[8]})" if shape[8] != shape[3] else "")


def cshape(shape):
    return K.conv_shape(*shape)


# ------------------------------------------------------------------------------------------------------------ cases
# forward: name -> (shape, arm, slices or None for the host schedule); y in bf16 and f32, plus conv_fwd_bn_stats
FWD = {
    "mode1-3x3": (sh(2, 13, 11, 64, 64, 3, 1, 1), "mode1", None),  # M = 286: 2 row tiles (30 rows), 64-row group of 30
    "mode1-2coltiles": (sh(1, 9, 9, 32, 192, 3, 1, 1), "mode1", None),  # second column tile partial; Cs at the minimum
    "mode1-odd-s2": (sh(2, 15, 13, 64, 128, 3, 2, 1), "mode1", None),
    "mode1-1x1-s2": (sh(2, 14, 10, 64, 256, 1, 2, 0), "mode1", None),
    "pointwise": (sh(2, 9, 7, 64, 256, 1, 1, 0), "pointwise", None),
    "pointwise-split": (sh(2, 8, 8, 1024, 256, 1, 1, 0), "pointwise-split2", None),
    "mode1-split": (sh(2, 8, 8, 256, 256, 3, 1, 1), "mode1-split4", None),  # K = 2304: 72 k-steps
    "mode1-split5": (sh(2, 8, 8, 256, 256, 3, 1, 1), "mode1-split5", 5),  # kper 480, last slice 384
    "stem": (sh(2, 20, 18, 8, 64, 7, 2, 3, 3), "mode6", None),  # K = 392 -> 416 with zero-page chunks; M = 180
}
FWD_FP32 = {
    "mode1-3x3": (sh(2, 13, 11, 64, 64, 3, 1, 1), "staged", None),
    "mode1-odd-s2": (sh(2, 15, 13, 64, 128, 3, 2, 1), "staged", None),
    "stem": (sh(2, 20, 18, 4, 64, 7, 2, 3, 3), "staged", None),
}
FORMS = ("store_bf16", "store_f32", "acc_bf16", "acc_f32")
# data gradient: name -> (shape, {form: arm})
DGRAD = {
    "mode2-3x3": (sh(2, 13, 11, 64, 64, 3, 1, 1), dict.fromkeys(FORMS, "mode2")),
    # 1x1 stride 1: an accumulate onto bf16 dx leaves the pointwise arm for mode 2; onto f32 it stays pointwise, the
    # residual epilogue reading dx in place
    "1x1": (sh(2, 9, 7, 64, 256, 1, 1, 0), dict(store_bf16="pointwise", store_f32="pointwise", acc_bf16="mode2",
                                                acc_f32="pointwise")),
    "mode2-split": (sh(2, 9, 7, 64, 128, 3, 1, 1), dict.fromkeys(FORMS, "mode2-split2")),  # K = 1152
    "mode5-3x3": (sh(2, 14, 10, 64, 128, 3, 2, 1), dict.fromkeys(FORMS, "mode5")),  # 70 rows per class
    "mode5-1x1": (sh(2, 14, 10, 64, 256, 1, 2, 0), dict.fromkeys(FORMS, "mode5")),
    "odd-scatter": (sh(2, 15, 13, 64, 64, 3, 2, 1), dict.fromkeys(FORMS, "scatter")),  # class grids 8x7 7x7 8x6 7x6
    "odd-scatter-split": (sh(2, 7, 7, 64, 512, 3, 2, 1), dict.fromkeys(FORMS, "scatter-split2")),
}
DGRAD_FP32 = {
    "mode2-3x3": (sh(2, 13, 11, 64, 64, 3, 1, 1), dict(store_f32="staged", acc_f32="staged")),
    "odd-scatter": (sh(2, 15, 13, 64, 64, 3, 2, 1), dict(store_f32="staged", acc_f32="staged")),
}
# conv_bwd_data_bn: name -> (shape, arm)
DGRAD_BN = {
    "mode2-epilogue": (sh(2, 13, 11, 64, 64, 3, 1, 1), "mode2"),
    "pointwise-epilogue": (sh(2, 9, 7, 64, 256, 1, 1, 0), "pointwise"),
    "split-finish": (sh(2, 9, 7, 64, 128, 3, 1, 1), "mode2-split2"),
    "mode5-epilogue": (sh(2, 14, 10, 64, 128, 3, 2, 1), "mode5"),
}
# weight gradient: name -> (shape, (arm, slices, kper))
WGRAD = {
    "mode3": (sh(2, 8, 8, 64, 256, 3, 1, 1), ("mode3", 1, 128)),
    "mode3-split": (sh(3, 16, 22, 64, 256, 3, 1, 1), ("mode3", 2, 544)),  # 1056 pixels: last slice 512
    "mode4": (sh(2, 16, 16, 64, 64, 3, 1, 1), ("mode4", 1, 512)),
    "mode4-split": (sh(2, 26, 40, 64, 64, 3, 1, 1), ("mode4", 4, 544)),  # 2080 pixels: last slice 448
    "stem-mode4": (sh(2, 32, 32, 8, 64, 7, 2, 3, 3), ("mode4", 1, 512)),  # dw [64,3,7,7]: no padded channel leaks
    "strided": (sh(2, 16, 16, 64, 128, 3, 2, 1), ("mode4", 1, 128)),
    "staged": (sh(2, 13, 11, 64, 64, 3, 1, 1), ("staged", 1, 288)),  # 286 pixels, not a multiple of 32
    "staged-s2": (sh(2, 15, 13, 64, 64, 3, 2, 1), ("staged", 1, 128)),  # 112 pixels
    "staged-split": (sh(4, 13, 11, 64, 64, 3, 1, 1), ("staged", 2, 288)),  # 572 pixels: last slice 284
    "pointwise": (sh(2, 9, 7, 64, 256, 1, 1, 0), ("linear_wgrad", 1, 126)),
}
WGRAD_FP32 = {"staged": (sh(2, 13, 11, 64, 64, 3, 1, 1), ("staged", 1, 288))}


# ------------------------------------------------------------------------------------------- arms from the host side
def fwd_arm(shape, mode, split=None):
    """-> (arm, slices, tiles x slices, GEMM K) of conv_fwd / conv_fwd_bn_stats, from kernels.py's predicates"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    s, dt = cshape(shape), TORCH_DT[mode]
    OH, OW = R.out_hw(H, W, k, stride, pad)
    M, Kg = B * OH * OW, k * k * Cs
    tiles = cdiv(M, 256) * cdiv(Cout, 128)
    if K._pointwise(s, dt):
        sp = K._conv_split(M, Cout, Cs)
        return ("pointwise" if sp == 1 else f"pointwise-split{sp}"), sp, tiles * sp, Kg
    if K._stem8(s, dt):
        return "mode6", 1, tiles, cdiv(Kg, 32) * 32
    if K._gathered(s, dt):
        sp = K._conv_split(M, Cout, Kg, K._CONV_FWD_MIN_KSTEPS) if split is None else split
        return ("mode1" if sp == 1 else f"mode1-split{sp}"), sp, tiles * sp, Kg
    return "staged", 1, cdiv(M, 128) * cdiv(Cout, 128), Kg


def dgrad_arm(shape, mode, accumulate, dx_dtype):
    """-> (arm, slices, workgroups of the (largest) launch, GEMM K of the longest sum), following conv_bwd_data"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    s, dt = cshape(shape), TORCH_DT[mode]
    T, M = k * k, B * H * W
    if K._pointwise(s, dt) and (not accumulate or dx_dtype == F32):
        sp = K._conv_split(M, Cs, Cout)
        return ("pointwise" if sp == 1 else f"pointwise-split{sp}"), sp, cdiv(M, 256) * cdiv(Cs, 128) * sp, Cout
    if dt == BF and stride == 1 and Cout >= 32 and Cs % 8 == 0 and (T * Cout) % 32 == 0:
        sp = K._conv_split(M, Cs, T * Cout)
        return ("mode2" if sp == 1 else f"mode2-split{sp}"), sp, cdiv(M, 256) * cdiv(Cs, 128) * sp, T * Cout
    if dt == BF and stride == 2 and Cout >= 32 and Cs % 8 == 0:
        sp = K._s2_split(s, M, T)
        taps = max(len([1 for kh in range(k) for kw in range(k) if (py + pad - kh) % 2 == 0 and (px + pad - kw) % 2 == 0])
                   for py in (0, 1) for px in (0, 1))
        if sp == 1 and K._s2_direct(s):
            ncls = 1 if (accumulate and T == 1) else 4  # an accumulate skips trailing classes without taps
            return "mode5", 1, cdiv(M // 4, 256) * cdiv(Cs, 128) * ncls, taps * Cout
        assert H % 2 or W % 2, "an even grid with a split: the slab form of mode 5, which no case here means to reach"
        rows = B * cdiv(H, 2) * cdiv(W, 2)  # class (0, 0), the largest of the four launches
        return ("scatter" if sp == 1 else f"scatter-split{sp}"), sp, cdiv(rows, 256) * cdiv(Cs, 128) * sp, taps * Cout
    return "staged", 1, None, T * Cout


def wgrad_arm(shape, mode):
    """-> ((arm, slices, kper), tiles x slices)"""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    if K._pointwise(cshape(shape), TORCH_DT[mode]):
        M = B * H * W
        sp = K._wgrad_split_for(Cout, Cs, M)
        return ("linear_wgrad", sp, M if sp == 1 else R.split_kper(M, sp)), None
    arm, sp, kper, tiles = R.wgrad_arm(shape, mode)
    return (arm, sp, kper), tiles * sp


def widened(shape, total_of, arm_of, *, n_field):
    """the case for ``grid_cap=3``: the same shape if it already has more than 3 workgroups' worth of tiles x slices,
    else the GEMM's N (``n_field``: 4 = Cout, 3 = Cs) doubled up to 8 x, else batch images added - the first that
    reaches more than 3 while keeping the arm."""
    cands = [shape] + [shape[:n_field] + (shape[n_field] * f,) + shape[n_field + 1:8]
                       + ((shape[8] * f,) if n_field == 3 else (shape[8],)) for f in (2, 4, 8)]
    cands += [(shape[0] + b,) + shape[1:] for b in range(1, 25)]
    for c in cands:
        if arm_of(c) == arm_of(shape) and total_of(c) is not None and total_of(c) > 3:
            return c
    raise AssertionError(f"no widened form of {shape} reaches more than 3 tiles on the arm {arm_of(shape)}")


@functools.lru_cache(maxsize=None)
def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def policies(dev, staged):
    """name -> policy factory (a fresh ctypes struct per call)"""
    if staged:
        return {"default": lambda: None}
    return {"default": lambda: None, "cap3": lambda: nv.policy(grid_cap=3),
            "model": lambda: nv.policy(grid_cap=_ncu(dev) * 3 // 4)}


# ------------------------------------------------------------------------------------------------------ one call
class Call:
    """One kernel call: ``inputs`` name -> (float64 CPU values, dtype); ``outputs`` name -> (shape, dtype, prior or
    None); ``scratch`` name -> float count (f32 workspaces: NaN-filled, only their sentinels checked); ``run(views,
    policy)``; ``refs`` name -> (ref, bound) float64 CPU, or a function of the outputs read back (the partials);
    ``sens``: (output name, operand a, operand b) of the sensitivity condition; ``exact`` name -> (mask, values): the
    elements that must equal ``values`` bit for bit."""

    def __init__(self, where):
        self.where = where
        self.inputs, self.outputs, self.scratch, self.refs, self.exact, self.notes = {}, {}, {}, {}, {}, []
        self.run = self.sens = None


def _guarded(t, dtype, dev):
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=dev, dtype=dtype)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dtype))
    return view, buf


def _intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _check(where, name, got, ref, bound):
    """-> (largest error, largest error / bound, share bit-equal to bf16(ref) or None)"""
    g = got.double()
    err = (g - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    if not worst <= 2.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
        bad = (ratio > 2.0).nonzero()
        lo, hi = bad.min(0).values.tolist(), bad.max(0).values.tolist()
        pytest.fail(f"{where} {name}: {len(bad)} of {ratio.numel()} elements beyond 2 x bound (indices {lo} .. {hi}); "
                    f"worst at {idx}: got {float(g.reshape(-1)[flat]):.9g}, float64 {float(ref.reshape(-1)[flat]):.9g}, "
                    f"bound {float(bound.reshape(-1)[flat]):.3e}, error / bound {worst:.3g}")
    eq = float((got == ref.to(BF)).double().mean()) if got.dtype == BF else None
    return float(err.max()), worst, eq


def run_call(c, policy_of, dev):
    """c through its wrapper on guarded buffers, twice; guards, inputs and run-to-run bits checked; -> name -> figures"""
    views, bufs = {}, {}
    for n, (t, dt_) in c.inputs.items():
        views[n], bufs[n] = _guarded(t, dt_, dev)
    for n, (shape, dt_, prior) in c.outputs.items():
        views[n], bufs[n] = _guarded(torch.zeros(shape), dt_, dev)
    for n, count in c.scratch.items():
        views[n], bufs[n] = _guarded(torch.zeros(count), F32, dev)
    first = None
    for _ in range(2):
        for n, (shape, dt_, prior) in c.outputs.items():
            if prior is None:
                views[n].fill_(float("nan"))  # every element must be written
            else:
                views[n].copy_(prior.to(dt_))
        for n in c.scratch:
            views[n].fill_(float("nan"))
        c.run(views, policy_of())
        torch.cuda.synchronize()
        got = {n: views[n].detach().cpu() for n in c.outputs}
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(_bits(first[n]), _bits(got[n])), f"{c.where} {n}: differs run to run"
    for n, b_ in bufs.items():
        assert _intact(b_), f"{c.where}: sentinel around {n} overwritten"
    for n, (t, dt_) in c.inputs.items():
        assert torch.equal(views[n].cpu().double(), t), f"{c.where}: input {n} was modified"
    figs = {}
    for n in c.outputs:
        ref, bound = c.refs[n](first) if callable(c.refs[n]) else c.refs[n]
        figs[n] = _check(c.where, n, first[n], ref, bound)
    for n, (mask, values) in c.exact.items():
        dt_ = c.outputs[n][1]
        assert torch.equal(_bits(first[n])[mask], _bits(values.to(dt_))[mask]), \
            f"{c.where} {n}: the elements no tap reaches are not exactly {'the prior' if c.outputs[n][2] is not None else 'zero'}"
    return figs


def report(where, arm, figs_by_policy):
    parts = []
    for pname, figs in figs_by_policy.items():
        parts.append(pname + ": " + ", ".join(
            f"{n} err {e:.3e} ratio {r:.3f}" + (f" bf16-equal {q:.4f}" if q is not None else "") for n, (e, r, q) in figs.items()))
    print(f"[resnet_calls] {where} arm {arm}: " + "; ".join(parts))


def check_sens(c):
    name, a, b = c.sens
    ref, bound = c.refs[name]
    share = R.sensitive_share(bound, a, b)
    assert share >= 0.99, (f"{c.where}: only {share:.4f} of the elements have 2 x bound below one k-step's RMS "
                           f"contribution {R.kstep_rms(a, b):.3e}")
    return share


# ---------------------------------------------------------------------------------------------------- the builders
def stats_ref(y_name, M, C):
    """the float64 statistics partials [ceil(M/64)][2][C] of the kernel's own stored y, and their bound"""

    def ref(first):
        q = first[y_name].double().view(M, C)
        s1, s2, a1 = R.group_sums(q), R.group_sums(q * q), R.group_sums(q.abs())
        return torch.stack([s1, s2], 1), torch.stack([64 * U24 * a1, 65 * U24 * s2], 1)

    return ref


def build_fwd(name, shape, mode, out_dt, stats, split=None):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    arm, sp, total, Kg = fwd_arm(shape, mode, split)
    c = Call(f"conv_fwd{'_bn_stats' if stats else ''}[{name}] {mode} y {str(out_dt)[6:]} {shape_str(shape)}")
    x, w, _ = R.operands(shape, mode)
    wp = R.packed(w, Cs)
    ref, S = R.fwd_ref(shape, mode)
    OH, OW = ref.shape[1:3]
    M = B * OH * OW
    dt = TORCH_DT[mode]
    c.inputs = dict(x=(x, dt), wp=(wp, dt))
    c.outputs = dict(y=(tuple(ref.shape), out_dt, None))
    c.refs = dict(y=(ref, R.acc_bound(S, Kg, mode, sp, R.split_kper(Kg, sp)) + R.store_bound(ref, out_dt)))
    c.sens = ("y", x, wp)
    if sp > 1:
        c.scratch["work"] = sp * M * Cout
    s = cshape(shape)
    if stats:
        c.outputs["part"] = ((cdiv(M, 64), 2, Cout), F32, None)
        c.refs["part"] = stats_ref("y", M, Cout)

        def run(v, p):
            y, part = K.conv_fwd_bn_stats(v["x"], v["wp"], s, out_dt, p, out=v["y"], part=v["part"], work=v.get("work"),
                                          split=split)
            assert y.data_ptr() == v["y"].data_ptr() and part is not None and part.data_ptr() == v["part"].data_ptr()
    else:
        def run(v, p):
            y = K.conv_fwd(v["x"], v["wp"], s, out_dt, p, out=v["y"], work=v.get("work"), split=split)
            assert y.data_ptr() == v["y"].data_ptr()
    c.run = run
    return c, arm, total


def build_dgrad(name, shape, mode, form):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    acc, dx_dt = form.startswith("acc"), BF if form.endswith("bf16") else F32
    arm, sp, total, Kg = dgrad_arm(shape, mode, acc, dx_dt)
    c = Call(f"conv_bwd_data[{name}] {mode} {form} {shape_str(shape)}")
    _, w, dy = R.operands(shape, mode)
    wp = R.packed(w, Cs)
    term, S = R.dgrad_ref(shape, mode)
    dt = TORCH_DT[mode]
    c.inputs = dict(dy=(dy, dt), wp=(wp, dt))
    E = R.acc_bound(S, Kg, mode, sp, R.split_kper(Kg, sp))
    if acc:
        prior = R.prior(shape, "dx", "bf16" if dx_dt == BF else "f32")
        ref = prior + term
        c.outputs = dict(dx=(tuple(term.shape), dx_dt, prior))
        c.refs = dict(dx=(ref, E + R.store_bound(ref, dx_dt, prior, term)))
    else:
        prior = torch.zeros_like(term)
        c.outputs = dict(dx=(tuple(term.shape), dx_dt, None))
        c.refs = dict(dx=(term, E + R.store_bound(term, dx_dt)))
    if stride == 2 and k == 1:  # only parity class (0, 0) has a tap
        untouched = torch.ones(B, H, W, Cs, dtype=torch.bool)
        untouched[:, 0::2, 0::2] = False
        c.exact["dx"] = (untouched, prior)
    c.sens = ("dx", dy, wp)
    if arm.startswith("scatter") or sp > 1:
        c.scratch["work"] = sp * B * H * W * Cs
    s = cshape(shape)

    def run(v, p):
        if form == "store_bf16":  # resnet.py 581: a fresh dx in the activation dtype
            dx = K.conv_bwd_data(v["dy"], v["wp"], s, dx=v["dx"], dx_dtype=BF, policy=p, work=v.get("work"))
        elif form == "store_f32":  # 599
            dx = K.conv_bwd_data(v["dy"], v["wp"], s, dx=v["dx"], dx_dtype=F32, policy=p, work=v.get("work"))
        else:  # 600 / 604
            dx = K.conv_bwd_data(v["dy"], v["wp"], s, dx=v["dx"], accumulate=True, policy=p, work=v.get("work"))
        assert dx.data_ptr() == v["dx"].data_ptr()

    c.run = run
    return c, arm, total


def build_dgrad_bn(name, shape):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    arm, sp, total, Kg = dgrad_arm(shape, "bf16", False, BF)
    c = Call(f"conv_bwd_data_bn[{name}] {shape_str(shape)}")
    _, w, dy = R.operands(shape, "bf16")
    wp = R.packed(w, Cs)
    ref, S = R.dgrad_ref(shape, "bf16")
    y, mean, rstd, gamma, beta = R.bn_operands(shape)
    mask, unsure, xhat = R.bn_mask(shape)
    M = B * H * W
    s2 = stride == 2
    prows = 4 * cdiv(M // 4, 64) if s2 else cdiv(M, 64)
    c.inputs = dict(dy=(dy, BF), wp=(wp, BF), y=(y, BF), mean=(mean, F32), rstd=(rstd, F32), gamma=(gamma, F32),
                    beta=(beta, F32))
    c.outputs = dict(dx=(tuple(ref.shape), BF, None), part=((prows, 2, Cs), F32, None))
    c.refs = dict(dx=(ref, R.acc_bound(S, Kg, "bf16", sp, R.split_kper(Kg, sp)) + R.store_bound(ref, BF)))
    c.sens = ("dx", dy, wp)
    if sp > 1:
        c.scratch["work"] = sp * M * Cs
    share = float(unsure.double().mean())
    c.notes.append(f"{int(unsure.sum())} of {unsure.numel()} mask arguments within f32 rounding of zero")
    assert share <= 1e-3, f"{c.where}: {share:.2e} of the mask arguments cannot be decided in float64"

    def part_ref(first):
        q = first["dx"].double()  # the stored values the kernels sum
        g = torch.where(mask, q, torch.zeros_like(q))
        gx = g * xhat
        loose, loosex = torch.where(unsure, q.abs(), torch.zeros_like(q)), torch.where(unsure, (q * xhat).abs(), torch.zeros_like(q))
        g = torch.where(unsure, torch.zeros_like(g), g)  # an undecided element: left out, its size added to the bound
        gx = torch.where(unsure, torch.zeros_like(gx), gx)
        rows = (lambda t: torch.cat([R.group_sums(R.class_rows(t, cls)) for cls in range(4)])) if s2 else \
            (lambda t: R.group_sums(t.reshape(M, Cs)))
        s1, s2_ = rows(g), rows(gx)
        b1 = 64 * U24 * rows(g.abs()) + rows(loose) + U23 * s1.abs()
        b2 = 68 * U24 * rows(gx.abs()) + rows(loosex) + U23 * s2_.abs()
        return torch.stack([s1, s2_], 1), torch.stack([b1, b2], 1)

    c.refs["part"] = part_ref
    s = cshape(shape)

    def run(v, p):
        r = K.conv_bwd_data_bn(v["dy"], v["wp"], s, v["y"], v["mean"], v["rstd"], v["gamma"], v["beta"], policy=p,
                               out=v["dx"], part=v["part"], work=v.get("work"))
        assert r is not None, "conv_bwd_data_bn declined a shape on its path"
        assert r[0].data_ptr() == v["dx"].data_ptr() and r[1].data_ptr() == v["part"].data_ptr()

    c.run = run
    return c, arm, total


def build_wgrad(name, shape, mode, accumulate):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    (arm, sp, kper), total = wgrad_arm(shape, mode)
    c = Call(f"conv_bwd_weight[{name}] {mode} accumulate={accumulate} {shape_str(shape)}")
    x, _, dy = R.operands(shape, mode)
    term, S = R.wgrad_ref(shape, mode)
    OH, OW = dy.shape[1:3]
    npix = B * OH * OW
    dt = TORCH_DT[mode]
    c.inputs = dict(dy=(dy, dt), x=(x, dt))
    E = R.acc_bound(S, npix, mode, sp, kper)
    if accumulate:
        prior = R.prior(shape, "dw", "f32")
        c.outputs = dict(dw=(tuple(term.shape), F32, prior))
        c.refs = dict(dw=(prior + term, E + R.store_bound(prior + term, F32, prior, term)))
    else:
        c.outputs = dict(dw=(tuple(term.shape), F32, None))
        c.refs = dict(dw=(term, E + R.store_bound(term, F32)))
    c.sens = ("dw", dy, x)
    if arm != "linear_wgrad":
        c.scratch["work"] = R.wgrad_work_floats(shape)
    s = cshape(shape)

    def run(v, p):
        dw = K.conv_bwd_weight(v["dy"], v["x"], s, dw=v["dw"], accumulate=accumulate, policy=p, work=v.get("work"))
        assert dw.data_ptr() == v["dw"].data_ptr()

    c.run = run
    return c, (arm, sp, kper), total


# -------------------------------------------------------------------------------------------------------- the tests
def _fwd_calls(name, shape, mode, split):
    """the calls of one forward case: conv_fwd with bf16 and f32 y (fp32 mode: f32 y), conv_fwd_bn_stats"""
    if mode == "fp32":
        return [build_fwd(name, shape, mode, F32, False)]
    return [build_fwd(name, shape, mode, BF, False, split), build_fwd(name, shape, mode, F32, False, split),
            build_fwd(name, shape, mode, BF, True, split)]


def _fwd_widened(shape, mode, split):
    return widened(shape, lambda c_: fwd_arm(c_, mode, split)[2], lambda c_: fwd_arm(c_, mode, split)[0], n_field=4)


def _dgrad_widened(shape, acc, dx_dt):
    return widened(shape, lambda c_: dgrad_arm(c_, "bf16", acc, dx_dt)[2], lambda c_: dgrad_arm(c_, "bf16", acc, dx_dt)[0],
                   n_field=3)


def _wgrad_widened(shape):
    return widened(shape, lambda c_: wgrad_arm(c_, "bf16")[1], lambda c_: wgrad_arm(c_, "bf16")[0][0], n_field=4)


def _fwd_items():
    return [(n, "bf16") + FWD[n] for n in FWD] + [(n, "fp32") + FWD_FP32[n] for n in FWD_FP32]


def _run_policies(dev, want_arm, staged, build, widen):
    """``build(shape)`` -> (call, arm, tiles x slices) at the case's shape under the default and the model's policy, at
    ``widen()``'s shape under grid_cap=3"""
    figs, arm, where = {}, None, None
    for pname, pol in policies(dev, staged).items():
        c, arm, total = build(widen() if pname == "cap3" else None)
        where = where or c.where
        if pname == "cap3" and isinstance(arm, tuple):  # a weight gradient with batch images added: more slices
            assert arm[0] == want_arm[0], f"{c.where}: the host takes the arm {arm}, the case means {want_arm[0]}"
        else:
            assert arm == want_arm, f"{c.where}: the host takes the arm {arm}, the case means {want_arm}"
        if pname == "cap3":
            assert total is not None and total > 3, f"{c.where}: grid_cap=3 is not below its {total} tiles x slices"
        check_sens(c)
        figs[pname] = run_call(c, pol, dev)
        for note in c.notes:
            print(f"[resnet_calls] {c.where}: {note}")
    report(where, arm, figs)


@gpu
@pytest.mark.parametrize("name,mode,shape,arm,split", _fwd_items(), ids=[f"{n}-{m}" for n, m, *_ in _fwd_items()])
def test_conv_fwd(dev, name, mode, shape, arm, split):
    for i in range(1 if mode == "fp32" else 3):
        _run_policies(dev, arm, arm == "staged",
                      lambda s_, i=i: _fwd_calls(name, s_ or shape, mode, split)[i],
                      lambda: _fwd_widened(shape, mode, split))


def _dgrad_items():
    return [(n, "bf16", DGRAD[n][0], f, a) for n in DGRAD for f, a in DGRAD[n][1].items()] + \
        [(n, "fp32", DGRAD_FP32[n][0], f, a) for n in DGRAD_FP32 for f, a in DGRAD_FP32[n][1].items()]


@gpu
@pytest.mark.parametrize("name,mode,shape,form,arm", _dgrad_items(), ids=[f"{n}-{m}-{f}" for n, m, _, f, _ in _dgrad_items()])
def test_conv_bwd_data(dev, name, mode, shape, form, arm):
    acc, dx_dt = form.startswith("acc"), BF if form.endswith("bf16") else F32
    _run_policies(dev, arm, arm == "staged",
                  lambda s_: build_dgrad(name, s_ or shape, mode, form), lambda: _dgrad_widened(shape, acc, dx_dt))


@gpu
@pytest.mark.parametrize("name", list(DGRAD_BN))
def test_conv_bwd_data_bn(dev, name):
    shape, arm = DGRAD_BN[name]
    _run_policies(dev, arm, False, lambda s_: build_dgrad_bn(name, s_ or shape),
                  lambda: _dgrad_widened(shape, False, BF))


def _wgrad_items():
    return [(n, "bf16") + WGRAD[n] for n in WGRAD] + [(n, "fp32") + WGRAD_FP32[n] for n in WGRAD_FP32]


def _check_work_floats(shape):
    n = nv.value("sv_conv_bwd_weight_work_floats", ctypes.byref(cshape(shape)))
    assert n == R.wgrad_work_floats(shape), f"{shape}: the library's workspace {n} is not the restated schedule's"


@gpu
@pytest.mark.parametrize("name,mode,shape,arm", _wgrad_items(), ids=[f"{n}-{m}" for n, m, *_ in _wgrad_items()])
@pytest.mark.parametrize("accumulate", (True, False), ids=["accumulate", "store"])
def test_conv_bwd_weight(dev, name, mode, shape, arm, accumulate):
    _check_work_floats(shape)
    # the generic linear_wgrad kernel (rows not a multiple of 32) takes no grid cap either
    _run_policies(dev, arm, arm[0] in ("staged", "linear_wgrad"),
                  lambda s_: build_wgrad(name, s_ or shape, mode, accumulate), lambda: _wgrad_widened(shape))


PACKS = [(64, 64, 3, 64), (64, 3, 7, 8), (256, 64, 1, 64), (192, 32, 3, 32), (64, 3, 7, 4), (8, 5, 1, 8)]  # Cout Cin k Cs


@gpu
@pytest.mark.parametrize("dtype", (BF, F32), ids=["bf16", "f32"])
def test_weight_pack(dev, dtype):
    """conv_weight_pack and conv_weight_pack_multi (33 segments: two launches): bit for bit the f32 master rounded to
    ``dtype`` (round to nearest even) in the layout [Cout][k*k][Cs], stored channels >= Cin exactly zero; the masters
    between sentinels, unchanged."""
    g = torch.Generator().manual_seed(5)
    packs = [p_ for p_ in PACKS if dtype == F32 or p_[3] >= 8]
    ws = [torch.randn(co, ci, k, k, generator=g) for co, ci, k, cs in packs]
    guarded = [_guarded(w, F32, dev) for w in ws]
    want = [R.packed(w, cs).to(dtype) for w, (co, ci, k, cs) in zip(ws, packs)]
    for (view, _), (co, ci, k, cs), wt in zip(guarded, packs, want):
        for _ in range(2):
            got = K.conv_weight_pack(view, cs, dtype).cpu()
            assert got.shape == wt.shape and torch.equal(_bits(got), _bits(wt)), f"conv_weight_pack {co, ci, k, cs} {dtype}"
    n = nv.SV_MAX_PACK_SEGS + 1
    items = [(guarded[i % len(packs)][0], packs[i % len(packs)][3]) for i in range(n)]
    for _ in range(2):
        outs = K.conv_weight_pack_multi(items, dtype)
        assert len(outs) == n
        for i, o in enumerate(outs):
            assert torch.equal(_bits(o.cpu()), _bits(want[i % len(packs)])), f"conv_weight_pack_multi segment {i} {dtype}"
    torch.cuda.synchronize()
    for (view, buf), w in zip(guarded, ws):
        assert _intact(buf) and torch.equal(view.cpu(), w)


def test_reference_side_conditions():
    """No GPU: for every case (and its grid_cap=3 form) the arm named in the tables is the one the host takes, the
    restated weight-gradient schedule agrees with the library's workspace size, at least 99 % of the elements have
    2 x bound below one k-step's RMS contribution, and at most 0.1 % of the mask arguments are undecidable."""
    lines = []

    def note(c, arm):
        lines.append(f"{c.where} arm {arm}: sensitive share {check_sens(c):.4f}" + "".join(" | " + n for n in c.notes))

    for name, mode, shape, arm, split in _fwd_items():
        shapes = [shape] if arm == "staged" else [shape, _fwd_widened(shape, mode, split)]
        for s_ in dict.fromkeys(shapes):
            for c, got_arm, _ in _fwd_calls(name, s_, mode, split):
                assert got_arm == arm, (c.where, got_arm, arm)
                note(c, got_arm)
    for name, mode, shape, form, arm in _dgrad_items():
        acc, dx_dt = form.startswith("acc"), BF if form.endswith("bf16") else F32
        shapes = [shape] if arm == "staged" else [shape, _dgrad_widened(shape, acc, dx_dt)]
        for s_ in dict.fromkeys(shapes):
            c, got_arm, _ = build_dgrad(name, s_, mode, form)
            assert got_arm == arm, (c.where, got_arm, arm)
            note(c, got_arm)
    for name, (shape, arm) in DGRAD_BN.items():
        for s_ in dict.fromkeys([shape, _dgrad_widened(shape, False, BF)]):
            c, got_arm, _ = build_dgrad_bn(name, s_)
            assert got_arm == arm, (c.where, got_arm, arm)
            note(c, got_arm)
    for name, mode, shape, arm in _wgrad_items():
        _check_work_floats(shape)
        shapes = [shape] if arm[0] in ("staged", "linear_wgrad") else [shape, _wgrad_widened(shape)]
        for s_ in dict.fromkeys(shapes):
            for accumulate in (True, False):
                c, got_arm, _ = build_wgrad(name, s_, mode, accumulate)
                if s_ == shape:
                    assert got_arm == arm, (c.where, got_arm, arm)
                note(c, got_arm)
    print("\n".join("[resnet_calls] " + ln for ln in lines))
