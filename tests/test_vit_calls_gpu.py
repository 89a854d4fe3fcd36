"""Every bf16 kernel call of a ViT / DeiT-III step outside attention, one call at a time through the
``spine_vision_amd.kernels`` wrapper ``backbone/vit.py`` uses, with vit.py's argument forms, each output compared
ELEMENT BY ELEMENT with a float64 evaluation of the same operation on the same bf16-rounded operands (torch float64 on
the device).  The model tests bound whole tensors in relative L2 (2e-2 / 0.15) at B = 2; a wrong edge tile, a dropped
k-step in one column block or one wrong row stays far below those.

Calls (vit.py line mirrored -> kind here)
    349  patch embedding  linear_fwd(patches bf16 [M,768], W bf16 [C,768], out f32, bias)          -> patch_fwd
    318  qkv              linear_fwd(y1 bf16, W [3C,C], out bf16, bias)                            -> qkv_fwd
    322  proj             linear_fwd(o bf16, W [C,C], out f32, bias, gamma, residual f32, GAMMA_RES) -> proj_fwd
    330  fc1 (training)   linear_fwd(y2, W [4C,C], out=gh bf16, out2=a bf16, bias, BIAS_GELU_DUAL) -> fc1_fwd
    332  fc1 (eval)       linear_fwd(y2, W, out=a bf16, bias, BIAS_GELU): bit for bit the dual's out2 -> fc1_fwd
    334  fc2              linear_fwd(a bf16, W [C,4C], out f32, bias, gamma, residual f32, GAMMA_RES) -> fc2_fwd
    384 / 388 (from 405)  fc2 data gradient  linear_dgrad(dsrc bf16, W | scale_rows_bf16(W, gamma), out=dh bf16,
                          MUL_AUX, aux=gh bf16)                                                    -> fc2_dgrad
    409  fc1 data gradient linear_dgrad(dh bf16, W [4C,C], out f32)                                -> fc1_dgrad
    384 / 388 (from 415)  proj data gradient linear_dgrad(dsrc bf16, W [C,C], out=do bf16)         -> proj_dgrad
    419  qkv data gradient linear_dgrad(dqkv bf16, W [3C,C], out f32)                              -> qkv_dgrad
    379 / 406 / 424       linear_wgrad(dy, x, out=, accumulate=True, bias_out=) for fc2 and proj (379), fc1 (406),
                          qkv (424)                                      -> fc2_wgrad, proj_wgrad, fc1_wgrad, qkv_wgrad
    461  patch embedding  linear_wgrad(d bf16 [M,C], patches [M,768], out=, accumulate=True), no bias -> patch_wgrad
    375  DeiT proj / fc2  layerscale_wgrad(dsrc, o | a, W f32, gamma, b, dw2=, dgamma=, db2=)  -> proj_lswgrad, fc2_lswgrad
    316 / 324 / 361       layernorm_fwd f32 -> bf16 (blocks) and f32 -> f32 (final norm over the class rows)
    410 / 420             layernorm_bwd(f32, f32, f32, dx=d, accumulate_dx=True)
    351  vit_tokens
The residual forms run gamma = ones (ViT's ``ls_ones``) and gamma uniform in [0.05, 0.3] (DeiT-III); the fc2 data
gradient runs the plain bf16 weight and the ``scale_rows_bf16`` weight (that kernel's output is checked per element too
and then taken as the GEMM's operand).  ``wgrad_target`` is ViTHip's 256.

Widths C in {192, 384, 768, 1024}; rows M, chosen from csrc/gemm.hip's conditions (GEMM K = C, 3C, 4C or 768 for the
forward and data-gradient calls, always a multiple of 64; GEMM K = M for the weight gradients):
  (a) M = 16, 400: what the model tests run.  Forward / data gradients, default policy: v3 (heavy epilogues, plain
      store with K <= 2048) or v2 (the residual form; plain store with K > 2048: fc1 data gradient at C >= 768, qkv data
      gradient at C >= 768).  Weight gradients: 16 % 32 and 400 % 32 != 0, so v2, v3, v8 and v9 all refuse and the
      generic ``launch_layout`` kernel runs (f32 slabs).
  (b) M = 1400 = 7 x 200, a short last batch: M % 32 = 24, ragged 128- and 256-row tiles; weight gradients generic.
  (c) M = 1600 and 2112 = 8 x 264: whole 64-row K-tiles (25 and 33), a ragged last 256-row tile (64 of 256 rows).
      Weight gradients with an output of at least 128 x 256 take ``_wgrad_split_for``'s v9 branch; where a slice count
      above one divides the K-tiles (1600: 5, 25; 2112: 3, 11, 33) ``_bf16_slabs`` is true: v9 writes bf16 slabs and
      ``sv_reduce_partials_bf16`` / ``sv_layerscale_wgrad_reduce_bf16`` folds them.  proj at C = 192 (192 x 192) stays
      below that: f32 slabs on v3 32x4.
  (d) production size, default policy, M the smallest multiple of 8 with ceil(M / 256) * ceil(N / 256) >= 256 (so
      the last row tile holds 8 of 256 rows): v9 (N >= 256).  qkv C = 1024 (M = 5384) and C = 192 (M = 21768: N = 576
      ends in a 64-column partial tile); fc1 and the fc2 data gradient C = 1024 (M = 3848); proj, fc2, patch
      embedding and the fc1 / proj / qkv data gradients C = 1024 (M = 16136).  Weight gradients reach v9 already in
      (c); M = 6400 (B = 32 at 224 px) runs them at C = 768 as the bench does.
      v8 under the DEFAULT policy: gemm.hip tries v9 first (``impl == 9 || v9_pick``) whenever tiles8 >= 256 and
      N >= 256, and every ViT width has N >= 256 except C = 192's proj / fc2 / patch forward, whose K (192 / 768) is
      below v8's 2048; v9 refuses none of ViT's forms.  So no ViT call reaches v8 by default, at any row count; the
      production-size v8 cases here (fc1 C = 1024, fc2 C = 768 with K = 3072) therefore ask for it with
      ``policy(impl=8)``.
Besides the default policy, (a) to (c) run ``nv.policy(impl=2 | 3 | 8 | 9)``, ``impl=9, grid_cap=4`` (one persistent
workgroup walks several tiles) and, for the backward calls, the policies ``ViTHip._wgrads`` builds (``wg_per_cu=1`` for
the data gradients and the patch weight gradient, ``wg_per_cu=1, priority=1`` for the side-stream weight gradients),
wherever the family's contract holds (v2: GEMM K % 64; v3, v8: K % 32; v9: K % (split * 64)); a (family, shape) pair
outside the contract is left out, since it would measure the fallback.

Bound, per element, derived (not tuned).  ``ref`` is the float64 result and S = |A| @ |B| (+ |bias|) in float64.  An
f32-accumulated product of exact bf16 operands differs from float64 by at most K * 2^-24 * S; times the epilogue's
Lipschitz factor (1.13 for GELU, 1 for GELU' since |GELU''| <= 0.8, |aux| for MUL_AUX, |gamma| for the residual
form); a bf16 store adds 2^-8 |ref|, an f32 store 2^-23 |ref|; where the result is a sum of two f32 terms that may
cancel (residual + branch, prior + gradient) the f32 term is taken on the addends, 2^-23 (|t1| + |t2|), since each is
rounded before the sum; bf16 slabs add 2^-8 sum_s |slab_s| with the slices from ``kernels._wgrad_split_for`` (the host
schedule).  The layer-scale finish adds K4 * 2^-24 sum_k |W G| for its row dot.  The two GELU outputs get an absolute
term for the erf evaluation: 4 x the largest absolute error of torch's float32 CPU erf-GELU / GELU' against float64 on
the same h (computed from the reference side, printed).  The assertion is |got - ref| <= 2 x bound for EVERY element.

Guards: outputs start as NaN (accumulating ones as their non-zero prior), every input and output sits between
sentinels, inputs must be unchanged, every call runs twice with bit-equal results.

The figures of the first run are recorded in profiles/vit_calls/parity.txt."""
import functools

import pytest
import torch

from _gemm_ref import (BF, F32, F64, U8, U23, U24, Call, _bf, _check_output, _erf_abs_terms, _gelu64, _gelu_grad64,
                       _guarded, _guards_intact, _run_call, _wgrad_terms)
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

pytestmark = pytest.mark.gpu

WIDTHS = (192, 384, 768, 1024)
ROWS = (16, 400, 1400, 1600, 2112)
WGRAD_TARGET = 256  # ViTHip.wgrad_target

FWD = ("patch_fwd", "qkv_fwd", "proj_fwd", "fc1_fwd", "fc2_fwd")
DGRAD = ("fc2_dgrad", "fc1_dgrad", "proj_dgrad", "qkv_dgrad")
WGRAD = ("qkv_wgrad", "proj_wgrad", "fc1_wgrad", "fc2_wgrad", "patch_wgrad", "proj_lswgrad", "fc2_lswgrad")
# kinds with a ViT (gamma = ones / plain weight) and a DeiT-III (random gamma / scale_rows_bf16 weight) form
TWO_FORMS = ("proj_fwd", "fc2_fwd", "fc2_dgrad")


@functools.lru_cache(maxsize=None)
def _backward_policies(dev):
    """(data-gradient policy, side-stream weight-gradient policy) as ViTHip._wgrads builds them"""
    from spine_vision_amd.backbone import create_vit

    hip = create_vit("vit_tiny", precision="bf16", img_size=32).to(dev)
    assert hip.overlap_wgrad and hip.wgrad_target == WGRAD_TARGET
    wg = hip._wgrads()
    return wg.pol, wg.spol


def _rand(g, dev, *shape, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g, device=dev, dtype=F64) * (hi - lo) + lo


def _weight(g, dev, n, k):
    return _bf(torch.randn(n, k, generator=g, device=dev, dtype=F64) * k ** -0.5)


def _build(kind, C, M, form, dev):
    """The call ``kind`` at width C and M rows; ``form``: "vit" or "deit" (TWO_FORMS only)."""
    g = torch.Generator(device=dev).manual_seed(1000003 * WIDTHS.index(C) + 7919 * M + sum(map(ord, kind + form)))

    def gamma_of(n):
        return torch.ones(n, device=dev, dtype=F64) if form == "vit" else _rand(g, dev, n, lo=0.05, hi=0.3).float().double()

    if kind in ("patch_fwd", "qkv_fwd"):
        Kd, N = (768, C) if kind == "patch_fwd" else (C, 3 * C)
        c = Call(kind, M, N, Kd)
        A, W, b = _bf(_rand(g, dev, M, Kd)), _weight(g, dev, N, Kd), _rand(g, dev, N, lo=-0.5, hi=0.5).float().double()
        odt = F32 if kind == "patch_fwd" else BF
        c.inputs = dict(A=(A, BF), W=(W, BF), bias=(b, F32))
        c.outputs = dict(out=((M, N), odt, None))
        c.run = lambda v, p: K.linear_fwd(v["A"], v["W"], out=v["out"], bias=v["bias"], compute_bf16=True, policy=p)
        ref = A @ W.T + b
        S = A.abs() @ W.abs().T + b.abs()
        c.refs = dict(out=(ref, Kd * U24 * S + (U23 if odt == F32 else U8) * ref.abs()))
    elif kind in ("proj_fwd", "fc2_fwd"):
        Kd = C if kind == "proj_fwd" else 4 * C
        c = Call(kind, M, C, Kd)
        A, W = _bf(_rand(g, dev, M, Kd)), _weight(g, dev, C, Kd)
        b, gam = _rand(g, dev, C, lo=-0.5, hi=0.5).float().double(), gamma_of(C)
        res = _rand(g, dev, M, C, lo=-2.0, hi=2.0).float().double()
        c.inputs = dict(A=(A, BF), W=(W, BF), bias=(b, F32), gamma=(gam, F32), res=(res, F32))
        c.outputs = dict(out=((M, C), F32, None))
        c.run = lambda v, p: K.linear_fwd(v["A"], v["W"], out=v["out"], bias=v["bias"], gamma=v["gamma"],
                                          residual=v["res"], epilogue=nv.SV_EPI_BIAS_GAMMA_RES, compute_bf16=True, policy=p)
        branch = gam * (A @ W.T + b)
        S = A.abs() @ W.abs().T + b.abs()
        c.refs = dict(out=(res + branch, gam.abs() * Kd * U24 * S + U23 * (res.abs() + branch.abs())))
    elif kind == "fc1_fwd":
        c = Call(kind, M, 4 * C, C)
        A, W, b = _bf(_rand(g, dev, M, C)), _weight(g, dev, 4 * C, C), _rand(g, dev, 4 * C, lo=-0.5, hi=0.5).float().double()
        c.inputs = dict(A=(A, BF), W=(W, BF), bias=(b, F32))
        c.outputs = dict(gh=((M, 4 * C), BF, None), a=((M, 4 * C), BF, None), a_eval=((M, 4 * C), BF, None))

        def run(v, p):
            K.linear_fwd(v["A"], v["W"], out=v["gh"], out2=v["a"], bias=v["bias"], epilogue=nv.SV_EPI_BIAS_GELU_DUAL,
                         compute_bf16=True, policy=p)
            K.linear_fwd(v["A"], v["W"], out=v["a_eval"], bias=v["bias"], epilogue=nv.SV_EPI_BIAS_GELU, compute_bf16=True,
                         policy=p)

        c.run = run
        h = A @ W.T + b
        Eh = C * U24 * (A.abs() @ W.abs().T + b.abs())
        t_g, t_d = _erf_abs_terms(h)
        c.notes.append(f"erf terms: GELU {t_g:.2e} GELU' {t_d:.2e}")
        a, gh = _gelu64(h), _gelu_grad64(h)
        c.refs = dict(a=(a, 1.13 * Eh + t_g + U8 * a.abs()), gh=(gh, 1.0 * Eh + t_d + U8 * gh.abs()))
        c.refs["a_eval"] = c.refs["a"]
        c.equal = [("a_eval", "a")]  # the single-output form: the dual's out2 bit for bit
    elif kind == "fc2_dgrad":
        c = Call(kind, M, 4 * C, C)
        A, aux = _bf(_rand(g, dev, M, C)), _bf(_rand(g, dev, M, 4 * C, lo=-0.2, hi=1.2))
        if form == "vit":
            W = _weight(g, dev, C, 4 * C)
        else:  # gamma folded into a bf16 copy of the f32 weight by sv_scale_rows_bf16, checked here per element
            Wf = (torch.randn(C, 4 * C, generator=g, device=dev, dtype=F64) * (4 * C) ** -0.5).float()
            gam = _rand(g, dev, C, lo=0.05, hi=0.3).float()
            wv, wb = _guarded(torch.full((C, 4 * C), float("nan"), device=dev), BF)
            K.scale_rows_bf16(Wf, gam, out=wv)
            want = Wf.double() * gam.double()[:, None]
            bad = (wv.double() - want).abs() > U8 * want.abs()
            assert _guards_intact(wb) and not bool(bad.any()), "scale_rows_bf16 is not bf16(W * gamma[:, None])"
            W = wv.double().clone()
        c.inputs = dict(A=(A, BF), W=(W, BF), aux=(aux, BF))
        c.outputs = dict(out=((M, 4 * C), BF, None))
        c.run = lambda v, p: K.linear_dgrad(v["A"], v["W"], out=v["out"], epilogue=nv.SV_EPI_MUL_AUX, aux=v["aux"],
                                            compute_bf16=True, policy=p)
        ref = (A @ W) * aux
        c.refs = dict(out=(ref, aux.abs() * C * U24 * (A.abs() @ W.abs()) + U8 * ref.abs()))
    elif kind in ("fc1_dgrad", "proj_dgrad", "qkv_dgrad"):
        Nn = {"fc1_dgrad": 4 * C, "proj_dgrad": C, "qkv_dgrad": 3 * C}[kind]  # dy columns = the GEMM's K
        odt = BF if kind == "proj_dgrad" else F32
        c = Call(kind, M, C, Nn)
        A, W = _bf(_rand(g, dev, M, Nn)), _weight(g, dev, Nn, C)
        c.inputs = dict(A=(A, BF), W=(W, BF))
        c.outputs = dict(out=((M, C), odt, None))
        c.run = lambda v, p: K.linear_dgrad(v["A"], v["W"], out=v["out"], compute_bf16=True, policy=p)
        ref = A @ W
        c.refs = dict(out=(ref, Nn * U24 * (A.abs() @ W.abs()) + (U23 if odt == F32 else U8) * ref.abs()))
    elif kind in ("qkv_wgrad", "proj_wgrad", "fc1_wgrad", "fc2_wgrad", "patch_wgrad"):
        N, Kd = {"qkv_wgrad": (3 * C, C), "proj_wgrad": (C, C), "fc1_wgrad": (4 * C, C), "fc2_wgrad": (C, 4 * C),
                 "patch_wgrad": (C, 768)}[kind]
        split = K._wgrad_split_for(N, Kd, M, WGRAD_TARGET)
        c = Call(kind, M, N, M, wgrad=True, split=split)
        c.slab_ok = lambda policy: K._bf16_slabs(N, Kd, M, split, True, policy)
        dy, x = _bf(_rand(g, dev, M, N)), _bf(_rand(g, dev, M, Kd))
        prior = _rand(g, dev, N, Kd, lo=-3.0, hi=3.0).float().double()
        c.inputs = dict(dy=(dy, BF), x=(x, BF))
        c.outputs = dict(dw=((N, Kd), F32, prior))
        G, E = _wgrad_terms(dy, x, M, split)
        refs = {}
        c.refs_for = lambda slabs: dict(refs, dw=(prior + G, E(slabs) + U23 * (prior.abs() + G.abs())))
        if kind == "patch_wgrad":
            c.run = lambda v, p: K.linear_wgrad(v["dy"], v["x"], out=v["dw"], accumulate=True, compute_bf16=True, policy=p,
                                                wgrad_target=WGRAD_TARGET)
        else:
            pb = _rand(g, dev, N, lo=-3.0, hi=3.0).float().double()
            c.outputs["db"] = ((N,), F32, pb)
            c.run = lambda v, p: K.linear_wgrad(v["dy"], v["x"], out=v["dw"], accumulate=True, bias_out=v["db"],
                                                compute_bf16=True, policy=p, wgrad_target=WGRAD_TARGET)
            cs = dy.sum(0)
            refs["db"] = (pb + cs, M * U24 * dy.abs().sum(0) + U23 * (pb.abs() + cs.abs()))
    elif kind in ("proj_lswgrad", "fc2_lswgrad"):
        K4 = C if kind == "proj_lswgrad" else 4 * C
        split = K._wgrad_split_for(C, K4, M, WGRAD_TARGET)
        c = Call(kind, M, C, M, wgrad=True, split=split)
        c.slab_ok = lambda policy: K._bf16_slabs(C, K4, M, split, True, policy)
        dy, x = _bf(_rand(g, dev, M, C)), _bf(_rand(g, dev, M, K4))
        W2 = (torch.randn(C, K4, generator=g, device=dev, dtype=F64) * K4 ** -0.5).float().double()
        gam, b2 = _rand(g, dev, C, lo=0.05, hi=0.3).float().double(), _rand(g, dev, C, lo=-0.5, hi=0.5).float().double()
        pw = _rand(g, dev, C, K4, lo=-3.0, hi=3.0).float().double()
        pg, pb = _rand(g, dev, C, lo=-3.0, hi=3.0).float().double(), _rand(g, dev, C, lo=-3.0, hi=3.0).float().double()
        c.inputs = dict(dy=(dy, BF), x=(x, BF), W2=(W2, F32), gamma=(gam, F32), b2=(b2, F32))
        c.outputs = dict(dw2=((C, K4), F32, pw), dgamma=((C,), F32, pg), db2=((C,), F32, pb))
        c.run = lambda v, p: K.layerscale_wgrad(v["dy"], v["x"], v["W2"], v["gamma"], v["b2"], dw2=v["dw2"],
                                                dgamma=v["dgamma"], db2=v["db2"], compute_bf16=True, policy=p,
                                                wgrad_target=WGRAD_TARGET)
        G, E = _wgrad_terms(dy, x, M, split)
        cs, Ecs = dy.sum(0), M * U24 * dy.abs().sum(0)
        gG = gam[:, None] * G
        dot, dotabs = (W2 * G).sum(1), (W2 * G).abs().sum(1)
        c.refs_for = lambda slabs: dict(
            dw2=(pw + gG, gam.abs()[:, None] * E(slabs) + U23 * (pw.abs() + gG.abs())),
            dgamma=(pg + dot + b2 * cs, (W2.abs() * E(slabs)).sum(1) + K4 * U24 * dotabs + b2.abs() * Ecs
                    + U23 * (pg.abs() + dotabs + (b2 * cs).abs())),
            db2=(pb + gam * cs, gam.abs() * Ecs + U23 * (pb.abs() + (gam * cs).abs())))
    else:
        raise KeyError(kind)
    return c


def _policies(c, dev, production=False):
    """name -> policy for this call: default, the four families and the capped v9 where the contract holds, and the
    backward's own policy for the backward calls."""
    out = {"default": None}
    if production:
        return out
    if c.Kg % 64 == 0:
        out["v2"] = nv.policy(impl=2)
    if c.Kg % 32 == 0:
        out["v3"] = nv.policy(impl=3)
        out["v8"] = nv.policy(impl=8)
    if c.Kg % (c.split * 64) == 0:
        out["v9"] = nv.policy(impl=9)
        out["v9cap4"] = nv.policy(impl=9, grid_cap=4)
    if c.kind not in FWD:
        pol, spol = _backward_policies(dev)
        out["bwd"] = spol if c.wgrad and c.kind != "patch_wgrad" else pol
    return out


def _case(dev, kind, C, M, form, production=False, only=None):
    c = _build(kind, C, M, form, dev)
    pols = _policies(c, dev, production)
    if only is not None:
        pols = {only[0]: only[1]}
    parts = []
    for pname, pol in pols.items():
        where = f"{kind}[{form}] C={C} M={M} policy={pname}"
        worst = _run_call(c, pol, where, c.refs_for(c.slab_ok(pol)))  # v2 / v3 / v8 keep f32 slabs: no slab term
        parts.append(pname + " " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    slab = f" split {c.split}{' bf16 slabs' if c.slab_ok(None) else ''}" if c.wgrad else ""
    print(f"[vit_calls] {kind}[{form}] C={C} M={M}{slab}: worst error / bound: " + "; ".join(parts)
          + ("".join(" | " + s for s in c.notes)))


def _forms(kind):
    return ("vit", "deit") if kind in TWO_FORMS else ("deit",) if kind.endswith("lswgrad") else ("vit",)


GRID = [(k, C, M, f) for k in FWD + DGRAD + WGRAD for f in _forms(k) for C in WIDTHS for M in ROWS]


@pytest.mark.parametrize("kind,C,M,form", GRID, ids=[f"{k}-{f}-C{C}-M{M}" for k, C, M, f in GRID])
def test_call_against_float64(dev, kind, C, M, form):
    """(a) to (c): every policy whose contract the shape meets"""
    _case(dev, kind, C, M, form)


def _m9(N):
    """the smallest multiple of 8 rows with ceil(M / 256) * ceil(N / 256) >= 256 (gemm.hip's tiles8 >= 256)"""
    return (-(-256 // -(-N // 256)) - 1) * 256 + 8


PRODUCTION = [("qkv_fwd", 1024, _m9(3072), "vit", None), ("qkv_fwd", 192, _m9(576), "vit", None),
              ("patch_fwd", 1024, _m9(1024), "vit", None), ("proj_fwd", 1024, _m9(1024), "deit", None),
              ("fc1_fwd", 1024, _m9(4096), "vit", None), ("fc2_fwd", 1024, _m9(1024), "vit", None),
              ("fc2_dgrad", 1024, _m9(4096), "deit", None), ("fc1_dgrad", 1024, _m9(1024), "vit", None),
              ("proj_dgrad", 1024, _m9(1024), "vit", None), ("qkv_dgrad", 1024, _m9(1024), "vit", None),
              ("fc1_fwd", 1024, _m9(4096), "vit", 8), ("fc2_fwd", 768, _m9(768), "vit", 8)] \
    + [(k, 768, 6400, "deit" if k.endswith("lswgrad") else "vit", None) for k in WGRAD]


@pytest.mark.parametrize("kind,C,M,form,impl", PRODUCTION,
                         ids=[f"{k}-{f}-C{C}-M{M}" + (f"-v{i}" if i else "") for k, C, M, f, i in PRODUCTION])
def test_call_production_size(dev, kind, C, M, form, impl):
    """(d): the default policy at the row counts where gemm.hip picks v9 (tiles8 >= 256, N >= 256; weight gradients:
    tiles8 * split >= 128 or bf16 slabs), and v8 by request (module docstring)."""
    if impl is None:
        c = _build(kind, C, M, form, dev)
        if c.wgrad:
            tiles8 = -(-c.Ng // 256) * -(-c.outputs[next(iter(c.outputs))][0][1] // 256)
            assert c.slab_ok(None) or tiles8 * c.split >= 128, "this shape would not reach v9"
        else:
            assert -(-M // 256) * -(-c.Ng // 256) >= 256 and c.Ng >= 256, "this shape would not reach v9"
    _case(dev, kind, C, M, form, production=True, only=None if impl is None else (f"v{impl}", nv.policy(impl=impl)))


# ---------------------------------------------------------------------------------------- LayerNorm as ViT calls it
LN_ROWS = (1, 2, 7, 16, 400, 1400)  # the small counts: the final norm over the class rows


def _ln_inputs(dev, C, rows):
    g = torch.Generator(device=dev).manual_seed(31 * C + rows)
    x = (torch.randn(rows, C, generator=g, device=dev, dtype=F64) * 2 + 0.5).float()
    w = (torch.rand(C, generator=g, device=dev, dtype=F64) + 0.5).float()
    b = torch.randn(C, generator=g, device=dev, dtype=F64).float()
    dy = torch.randn(rows, C, generator=g, device=dev, dtype=F64).float()
    prior = torch.randn(rows, C, generator=g, device=dev, dtype=F64).float()
    return x, w, b, dy, prior


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_fwd_as_vit_calls_it(dev, C, rows):
    """f32 x -> bf16 y (blocks) and f32 y (final norm), per element against float64: the f32 kernel within 1e-5 of the
    row's largest |y| (test_layernorm_fwd_bwd's 1e-5, per element instead of over the tensor), plus 2^-8 |ref| for the
    bf16 store; mean and rstd within 1e-5 relative (mean: of the row's largest |x|)."""
    x, w, b, _, _ = _ln_inputs(dev, C, rows)
    xv, xb = _guarded(x, F32)
    x64 = x.double()
    mu = x64.mean(1)
    rs = (x64.var(1, unbiased=False) + K.EPS_LN).rsqrt()
    ref = (x64 - mu[:, None]) * rs[:, None] * w.double() + b.double()
    tol = 1e-5 * ref.abs().amax(1, keepdim=True)
    worst = {}
    for dt_, store in ((BF, U8), (F32, 0.0)):
        y, mean, rstd = K.layernorm_fwd(xv, w, b, out_dtype=dt_)
        y2, mean2, rstd2 = K.layernorm_fwd(xv, w, b, out_dtype=dt_)
        assert torch.equal(y.float(), y2.float()) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
        where = f"layernorm_fwd C={C} rows={rows} {dt_}"
        worst[str(dt_)] = _check_output(where, "y", y, ref, 0.5 * (tol + store * ref.abs()))
        _check_output(where, "mean", mean, mu, 0.5 * 1e-5 * x64.abs().amax(1))
        _check_output(where, "rstd", rstd, rs, 0.5 * 1e-5 * rs)
    assert _guards_intact(xb) and torch.equal(xv, x)
    print(f"[vit_calls] layernorm_fwd C={C} rows={rows}: worst error / tolerance "
          + " ".join(f"{k} {v / 2:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_bwd_accumulate_dx(dev, C, rows):
    """layernorm_bwd (f32, f32, f32) with accumulate_dx=True onto a non-zero prior: dx against prior + float64 per
    element at 1e-5 x the row's largest |prior + ref|; dw, db against float64 at test_layernorm_fwd_bwd's 1e-5 relative
    L2; accumulate_dx=False must not read the prior (NaN)."""
    x, w, b, dy, prior = _ln_inputs(dev, C, rows)
    _, mean, rstd = K.layernorm_fwd(x, w, b, out_dtype=F32)
    x64, dy64, w64 = x.double(), dy.double(), w.double()
    mu = x64.mean(1, keepdim=True)
    rs = (x64.var(1, unbiased=False, keepdim=True) + K.EPS_LN).rsqrt()
    xh = (x64 - mu) * rs
    gy = dy64 * w64
    dx_ref = rs * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    dw_ref, db_ref = (dy64 * xh).sum(0), dy64.sum(0)
    ins = {n: _guarded(t, F32) for n, t in dict(dy=dy, x=x, mean=mean, rstd=rstd, w=w).items()}
    dxv, dxb = _guarded(prior, F32)
    outs = []
    for acc, start in ((True, prior), (False, torch.full_like(prior, float("nan"))), (True, prior)):
        dxv.copy_(start)
        dw, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        got = K.layernorm_bwd(ins["dy"][0], ins["x"][0], ins["mean"][0], ins["rstd"][0], ins["w"][0], dw=dw, db=db,
                              dx=dxv, accumulate_dx=acc)
        torch.cuda.synchronize()
        assert got.data_ptr() == dxv.data_ptr()
        outs.append((dxv.clone(), dw, db))
        want = prior.double() + dx_ref if acc else dx_ref
        where = f"layernorm_bwd C={C} rows={rows} accumulate_dx={acc}"
        r = _check_output(where, "dx", dxv, want, 0.5 * 1e-5 * want.abs().amax(1, keepdim=True).expand_as(want))
        e_w, e_b = _rel(dw, dw_ref), _rel(db, db_ref)
        assert e_w < 1e-5 and e_b < 1e-5, (where, e_w, e_b)
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[2])), "differs run to run"
    assert _guards_intact(dxb) and all(_guards_intact(b_) for _, b_ in ins.values())
    for n, t in dict(dy=dy, x=x, mean=mean, rstd=rstd, w=w).items():
        assert torch.equal(ins[n][0], t), f"input {n} was modified"
    print(f"[vit_calls] layernorm_bwd C={C} rows={rows}: accumulate_dx worst dx error / tolerance {r / 2:.3f}, dw rel "
          f"{e_w:.2e}, db rel {e_b:.2e}")


# ---------------------------------------------------------------------------------------------------- vit_tokens
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("P,Np", [(4, 8), (25, 32), (196, 200), (576, 584)])
@pytest.mark.parametrize("pos_has_cls", (True, False), ids=["vit", "deit"])
def test_vit_tokens_bitwise(dev, B, P, Np, pos_has_cls):
    """Bit for bit torch's f32 adds; pad rows exactly zero; the class and pad rows of ``pe`` (NaN) are never read;
    sentinels around the output and the inputs intact."""
    C = 192
    g = torch.Generator(device=dev).manual_seed(17 * P + B)
    pe = torch.randn(B, Np, C, generator=g, device=dev)
    cls = torch.randn(C, generator=g, device=dev)
    pos = torch.randn(P + int(pos_has_cls), C, generator=g, device=dev)
    want = torch.zeros(B, Np, C, device=dev)
    want[:, 0] = cls + pos[0] if pos_has_cls else cls
    want[:, 1:P + 1] = pe[:, 1:P + 1] + (pos[1:] if pos_has_cls else pos)
    pe[:, 0] = float("nan")
    pe[:, P + 1:] = float("nan")
    pev, peb = _guarded(pe.view(B * Np, C), F32)
    cv, cb = _guarded(cls, F32)
    pv, pb = _guarded(pos, F32)
    ov, ob = _guarded(torch.full((B * Np, C), float("nan"), device=dev), F32)
    got = K.vit_tokens(pev, cv, pv, B, P, Np, pos_has_cls, out=ov)
    torch.cuda.synchronize()
    assert got.data_ptr() == ov.data_ptr()
    assert all(_guards_intact(b_) for b_ in (peb, cb, pb, ob)), "a sentinel was overwritten"
    assert torch.equal(ov.view(torch.int32), want.view(B * Np, C).view(torch.int32)), "not torch's f32 adds bit for bit"
    assert bool((ov.view(B, Np, C)[:, P + 1:] == 0).all()), "pad rows must be exactly zero"
    assert torch.equal(cv, cls) and torch.equal(pv, pos)
    assert torch.equal(pev.view(B, Np, C)[:, 1:P + 1], pe[:, 1:P + 1]) and bool(pev.view(B, Np, C)[:, 0].isnan().all())
    fresh = K.vit_tokens(pev, cv, pv, B, P, Np, pos_has_cls)  # the module's form: a fresh output
    assert torch.equal(fresh.view(torch.int32), ov.view(torch.int32))
