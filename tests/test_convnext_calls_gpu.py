"""Every depthwise, LayerNorm, downsample, pooling and stem call of a ConvNeXt step (csrc/dwconv.hip, csrc/dwmfma.hip,
csrc/norm.hip), one call at a time with the argument forms ``backbone/convnext.py`` uses, each output compared ELEMENT
BY ELEMENT (every channel and tap of every reduced output) with a float64 CPU evaluation of the same operation on the
same rounded operands (tests/_convnext_ref.py).  The older tests of these kernels bound whole tensors in relative L2 on
randn inputs, or hold two forms bit-equal that share the ring loader and the statistics butterflies.

Call site (backbone/convnext.py)                                                      -> test here
    446 dwconv7_ln_fwd(x f32, w, b, lnw, lnb, act_dtype, save_z)                       -> test_dw_fwd_valu, _onepass, _mfma
    638 dwconv7_bwd_data(dz, w, d, accumulate=True, dx_bf16=)                          -> test_dw_bwd_data_valu, _mfma
    575 dwconv7_bwd_weight(dz, x, dw=, db=, defer=)                                    -> test_dw_bwd_weight_valu, _mfma,
                                                                                          test_dw_bwd_weight_multi_tile
    418, 622, 697 layernorm_fwd / layernorm_bwd                                        -> test_layernorm_fwd, _bwd
    433, 688 downsample_fwd / downsample_bwd                                           -> test_downsample
    493, 659 pool_ln_fwd / pool_ln_bwd                                                 -> test_pool_ln
    423, 703 stem_fwd / stem_bwd                                                       -> test_stem
    414 stem_patchify / stem_weight_pack (bitwise in test_kernels_gpu.py)              -> test_stem_patchify_pack_guarded
    every wrapper's dtype codes and argument order                                     -> test_wrappers_bit_equal

Harness: every input and output sits between 256 sentinels (-7.0), intact after the call; outputs start as NaN,
accumulating outputs as a known non-zero prior the reference adds; inputs are bit-unchanged after the call; every call
runs twice with bit-equal results.  The wrappers allocate their own outputs, so each entry point is called through
``nv.call`` with the wrapper's exact argument list on guarded buffers, and test_wrappers_bit_equal holds each wrapper
bit-equal to that once per kind.  Partials buffers start as NaN too: a partial row no workgroup wrote shows in the fold.

Bounds (tests/_convnext_ref.py, asserted at 2 x for EVERY element): n 2^-24 S for an f32 sum, n the longest chain of
dependent roundings: 49 fmas for the VALU depthwise; 7 x 32 = 224 for the matrix-core depthwise (seven
v_mfma_f32_16x16x32_bf16 per output, K = 32 each, the zero taps of every window included; products of bf16 operands are
exact) and tiles x 384 (W <= 16) or 640 (W > 16) for its weight gradient (16 rows x IC columns, IC = 24 / 40); a wave's
serial steps + the shuffle fold + the 4 waves' LDS fold + the partials fold (ceil(P / PG) + PG / F + F + 1, read from
reduce_pair_kernel / reduce_multi_kernel) for the reduced outputs; LayerNorm's mean, variance, rsqrt and affine map one
rounding per operation, rsqrtf's own error 4 x that of torch's float32 CPU rsqrt (measured from the reference side,
printed); 2^-8 |ref| for a bf16 store, 2^-23 for an f32 one, the addends' for prior + gradient.

mean / rstd handed to backward calls are the f32 roundings of the float64 statistics, so each call is judged alone.

Not reached: ln_vec_bwd_grid's cap of 2048 workgroups needs 65 537 row groups (at least 65 537 rows at C >= 512, over a
million at C = 96), beyond a test of a few seconds with a float64 reference; ln_grid's cap (1024) likewise needs 4097
rows of the scalar kernel at C = 64, which test_layernorm_bwd does run.

The first runs' figures are in profiles/convnext_calls/parity.txt."""
import os
import subprocess
import sys

import pytest
import torch

import _convnext_ref as R
from _convnext_ref import BF, F32
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 256
NAN = float("nan")
DT = {"bf16": BF, "f32": F32}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cid(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ------------------------------------------------------------------------------------------------------ harness
class Buffers:
    """device buffers between sentinels; inputs are remembered and compared bit for bit after the call"""

    def __init__(self, dev):
        self.dev, self.bufs, self.inputs = dev, {}, {}

    def _make(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=self.dev, dtype=dtype)
        self.bufs[name] = buf
        return buf[GUARD:GUARD + n].view(shape)

    def put(self, name, t, dtype):
        v = self._make(name, tuple(t.shape), dtype)
        v.copy_(t.to(dtype))
        self.inputs[name] = (v, v.clone())
        return v

    def out(self, name, shape, dtype, fill=NAN):
        v = self._make(name, tuple(shape), dtype)
        v.fill_(fill)
        return v

    def prior(self, name, t):
        v = self._make(name, tuple(t.shape), F32)
        v.copy_(t.to(F32))
        return v

    def check(self, where):
        for n, b in self.bufs.items():
            assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), \
                f"{where}: sentinel around {n} overwritten"
        for n, (v, keep) in self.inputs.items():
            assert torch.equal(v.view(torch.uint8), keep.view(torch.uint8)), f"{where}: input {n} modified"


def twice(where, once):
    """``once(Buffers) -> name -> device tensor``, run twice on fresh guarded buffers; -> the first run's CPU results"""
    first = None
    for _ in range(2):
        b = Buffers(torch.device("cuda:0"))
        got = once(b)
        torch.cuda.synchronize()
        b.check(where)
        got = {n: t.detach().cpu() for n, t in got.items()}
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(first[n].view(torch.uint8), got[n].view(torch.uint8)), f"{where} {n}: differs run to run"
    return first


def judge(where, got, refs, store=None):
    """every element of every output within 2 x bound; prints the largest error / bound per output.  ``store``: the
    dtype an output is stored in (its store bound is added; absent for the outputs whose bound carries it already)"""
    figs = []
    for n, (ref, bound) in refs.items():
        g = got[n].double().reshape(ref.shape)
        if store and n in store:
            bound = bound + R.store_bound(ref, store[n])
        err = (g - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
        worst = float(ratio.max())
        figs.append(f"{n} err {float(err.max()):.3e} ratio {worst:.3f}")
        if not worst <= 2.0:
            flat = int(ratio.reshape(-1).argmax())
            idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
            print(f"[convnext_calls] {where}: " + ", ".join(figs))
            pytest.fail(f"{where} {n}: {int((ratio > 2).sum())} of {ratio.numel()} elements beyond 2 x bound; worst at "
                        f"{idx}: got {float(g.reshape(-1)[flat]):.9g}, float64 {float(ref.reshape(-1)[flat]):.9g}, "
                        f"bound {float(bound.reshape(-1)[flat]):.3e}, error / bound {worst:.3g}")
    print(f"[convnext_calls] {where}: " + ", ".join(figs))


def bf16_copy_is_rounding(where, got, f32_name, bf_name):
    assert torch.equal(got[bf_name].view(torch.int16), got[f32_name].to(BF).reshape(got[bf_name].shape).view(torch.int16)), \
        f"{where}: {bf_name} is not bf16({f32_name}) bit for bit"


def code(dtype):
    return nv.SV_BF16 if dtype == BF else nv.SV_F32


# ---------------------------------------------------------------------------------------------------- the cases
DW_VALU = {  # shape -> the strips and channel groups it must take
    (1, 1, 1, 64): "strips1x1x1 groups1", (1, 1, 9, 64): "strips3x1x1 groups1", (1, 9, 1, 64): "strips1x1x1 groups1",
    (2, 3, 3, 64): "strips1x1x2 groups1", (1, 16, 4, 64): "strips1x1x1 groups1", (1, 17, 5, 64): "strips2x2x1 groups1",
    (2, 19, 23, 128): "strips6x2x2 groups2", (1, 33, 6, 96): "strips2x3x1 groups2 half",
    (1, 7, 6, 512): "strips2x1x1 groups8", (1, 8, 8, 1024): "strips2x1x1 groups16", (2, 16, 16, 32): "strips4x1x2 groups1 half",
}
DW_ONEPASS = [(1, 19, 23, 128), (1, 16, 4, 128), (1, 1, 1, 128), (1, 13, 9, 256), (1, 16, 4, 256), (1, 1, 1, 256),
              (1, 7, 6, 512), (1, 16, 4, 512), (1, 1, 1, 512)]
DW_MFMA = {  # shape -> (forward arm, backward-data arm)
    (1, 16, 16, 32): ("mfma tile16x16 tiles1 CG16", "mfma tile16x16 tiles1 CG32"),
    (1, 17, 17, 64): ("mfma tile16x32 tiles2 CG16", "mfma tile16x32 tiles2 CG32"),
    (2, 16, 33, 96): ("mfma tile16x32 tiles4 CG16", "mfma tile16x32 tiles4 CG32"),
    (1, 33, 32, 256): ("mfma tile16x32 tiles3 CG16", "mfma tile16x32 tiles3 CG32"),
    (1, 17, 33, 512): ("mfma tile16x32 tiles4 CG16", "mfma tile16x32 tiles4 CG16"),
    (1, 1, 1, 32): ("mfma tile16x16 tiles1 CG16", "mfma tile16x16 tiles1 CG32"),
    (1, 3, 40, 64): ("mfma tile16x32 tiles2 CG16", "mfma tile16x32 tiles2 CG32"),
}
DW_MFMA_WGRAD = {(2, 33, 33, 1024): (12, 8), (1, 17, 17, 64): (2, 2), (2, 16, 33, 96): (4, 4), (1, 16, 16, 32): (1, 1),
                 (1, 3, 40, 64): (2, 2)}  # shape -> (tiles, nparts): the first runs the prefetching multi-tile loop
MULTI_TILE = ((1, 48, 176, 128), 64)  # with SV_DW_WGRAD_WGS=64: 132 tiles against 4 x 32 wave slots
LN_C = (32, 64, 96, 128, 160, 192, 256, 384, 512, 768, 1024, 1536, 2048)
LN_FWD_FORMS = (("bf16", "f32"), ("f32", "bf16"), ("f32", "f32"), ("bf16", "bf16"))
LN_BWD_FORMS = (("f32", "f32", "f32"), ("f32", "bf16", "f32"), ("f32", "bf16", "bf16"), ("bf16", "bf16", "f32"),
                ("bf16", "bf16", "bf16"))  # (dy, x, dx)
DS_C = (64, 96, 128, 192, 256, 384, 512, 768)
DS_CASES = [(2, 2, 2, C) for C in DS_C] + [(1, 6, 10, C) for C in DS_C] + [(2, 128, 66, 64), (1, 2, 6, 96)]
POOL_CASES = [(B, HW, C) for HW, C, B in (
    (1, 64, 1), (1, 1024, 3), (3, 64, 3), (3, 768, 1), (4, 64, 1), (4, 1536, 3), (5, 768, 1), (5, 1024, 3), (20, 64, 3),
    (20, 1536, 1), (29, 768, 3), (29, 1024, 1), (32, 64, 1), (32, 1536, 3), (33, 768, 1), (33, 1024, 3), (49, 64, 3),
    (49, 768, 1), (49, 1024, 3), (49, 1536, 1), (64, 64, 1), (64, 1024, 3), (100, 768, 3), (100, 1536, 1))]
STEM_IMGS = ((1, 4, 4), (1, 8, 12), (2, 128, 128))
STEM_FWD_C, STEM_BWD_C = (64, 96, 128, 192, 256), (64, 96, 128, 192)


def ln_row_counts(C):
    """1; RPW - 1, RPW, RPW + 1; 4 RPW -+ 1 (one workgroup of the forward); a count that gives the backward two
    workgroups with a ragged last group, so the last waves' prefetch runs past the end; a few thousand rows at C <= 256
    (at C = 64 past ln_grid's cap of 1024 workgroups: a second grid-stride pass of the scalar kernels)"""
    k = R.ln_vec_kind(C)
    rpw = 64 // k[0] if k else 1
    rows = {1, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw + 1, (36 * rpw + 1) if k else 7}
    if C <= 256:
        rows.add(4099 if C == 64 else 3001)
    return sorted(r for r in rows if r > 0)


# ------------------------------------------------------------------------------------------------------ geometry
@gpu
def test_nparts_match_library():
    shapes = list(DW_VALU) + list(DW_MFMA_WGRAD) + [MULTI_TILE[0], (64, 56, 56, 128), (1, 33, 344, 1024), (4, 9, 9, 96)]
    for s in shapes:
        assert R.dw_wgrad_nparts(*s) == nv.value("sv_dwconv7_bwd_weight_nparts", *s), s
        assert R.dwm_wgrad_nparts(*s) == nv.value("sv_dwconv7_bwd_weight_mfma_nparts", *s), s
    for C in LN_C:
        for rows in ln_row_counts(C) + [70000, 300000]:
            assert R.ln_bwd_nparts(rows, C) == nv.value("sv_layernorm_bwd_nparts", rows, C), (rows, C)
    for s in DS_CASES:
        assert R.ds_grid(*s) == nv.value("sv_downsample_ln_patch2_bwd_nparts", *s), s
    for B, H, W in STEM_IMGS + ((64, 224, 224),):
        for C in STEM_BWD_C:
            assert R.stem_bwd_nparts(B, H, W, C) == nv.value("sv_stem_patchify_ln_bwd_nparts", B, H, W, C), (B, H, W, C)
    # the loops the older tests never reached, each by a named case
    s, wgs = MULTI_TILE
    assert R.dw_geo(*s)[2] == 132 and R.dw_wgrad_nparts(*s, wgs) == 32 and R.dw_wgrad_tiles_per_wave(*s, wgs) == 2
    assert DW_MFMA_WGRAD[(2, 33, 33, 1024)] == (R.dwm_geo(2, 33, 33, 1024)[1], R.dwm_wgrad_nparts(2, 33, 33, 1024))
    assert R.stem_arm(2, 128, 128, 64) == "CPL1 fwd512 bwd256 passes2"
    assert R.ln_arm(7, 64).startswith("scalar") and R.ln_grid(4099) == 1024
    assert R.pool_arm(49) == "rows13/12/12/12 deep1 tail5" and R.pool_arm(3) == "rows1/1/1/0 deep0 tail1"


# ----------------------------------------------------------------------------------------------------- depthwise
def _dw_in(b, o, x_dt):
    return (b.put("x", o["x"], DT[x_dt]), b.put("w", o["w"].view(-1, 1, 7, 7), F32), b.put("bias", o["b"], F32),
            b.put("lnw", o["lnw"], F32), b.put("lnb", o["lnb"], F32))


def _dw_fwd_once(shape, x_dt, act, arm):
    """arm: "valu" (ring kernel + LayerNorm, z kept), "onepass" (no z), "mfma" (matrix cores + vectorised LayerNorm)"""
    B, H, W, C = shape
    o = R.dw_operands(shape, x_dt, "f32", arm == "mfma")

    def once(b):
        x, w, bias, lnw, lnb = _dw_in(b, o, x_dt)
        y = b.out("y", (B * H * W, C), DT[act])
        mean, rstd = b.out("mean", (B * H * W,), F32), b.out("rstd", (B * H * W,), F32)
        z = None if arm == "onepass" else b.out("z", shape, DT[act])
        if arm == "mfma":
            nv.call("sv_dwconv7_fwd_mfma", K.ptr(x), K.dt(x), K.ptr(w), K.ptr(bias), K.ptr(z), B, H, W, C)
            nv.call("sv_layernorm_fwd", K.ptr(z), K.dt(z), K.ptr(lnw), K.ptr(lnb), K.ptr(y), K.dt(y), K.ptr(mean),
                    K.ptr(rstd), B * H * W, C, K.EPS_LN)
        else:
            nv.call("sv_dwconv7_ln_fwd", K.ptr(x), K.dt(x), K.ptr(w), K.ptr(bias), K.ptr(lnw), K.ptr(lnb), K.EPS_LN,
                    K.ptr(z), K.dt(y) if z is None else K.dt(z), K.ptr(y), K.dt(y), K.ptr(mean), K.ptr(rstd), B, H, W, C)
        res = dict(y=y, mean=mean, rstd=rstd)
        if z is not None:
            res["z"] = z
        return res

    return once


def _dw_fwd(shape, x_dt, act, arm, armname):
    where = f"dwconv7_ln_fwd {cid(shape)} x {x_dt} act {act} [{arm}: {armname}]"
    got = twice(where, _dw_fwd_once(shape, x_dt, act, arm))
    refs, _ = R.dw_fwd_ref(shape, x_dt, act, arm == "mfma")
    if arm == "onepass":
        refs = {n: v for n, v in refs.items() if n != "z"}
    judge(where, got, refs, store=dict(z=DT[act], y=DT[act], mean=F32, rstd=F32))


@gpu
@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(DW_VALU), ids=cid)
def test_dw_fwd_valu(shape, act):
    assert R.dw_arm(*shape) == DW_VALU[shape], f"{shape} takes {R.dw_arm(*shape)}: the strip geometry was retuned"
    # z kept: the two launches whatever SV_DW_LN_FUSED's default split says (dw_ln_fused: m < 0 and keep_z)
    _dw_fwd(shape, "f32", act, "valu", R.dw_arm(*shape) + " + " + R.ln_arm(shape[0] * shape[1] * shape[2], shape[3]))


@gpu
@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("shape", DW_ONEPASS, ids=cid)
def test_dw_fwd_onepass(shape, act):
    B, H, W, C = shape
    assert R.dw_ln_fusable(C, F32, DT[act]) and os.environ.get("SV_DW_LN_FUSED") is None
    assert nv.value("sv_dwconv7_ln_fused_ok", B, H, W, C, nv.SV_F32, code(DT[act]), code(DT[act])) == 1
    _dw_fwd(shape, "f32", act, "onepass", R.dw_arm(*shape))


@gpu
@pytest.mark.parametrize("x_dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(DW_MFMA), ids=cid)
def test_dw_fwd_mfma(shape, x_dt):
    assert R.dwm_arm(0, *shape) == DW_MFMA[shape][0], f"{shape} takes {R.dwm_arm(0, *shape)}"
    assert K.DW_MFMA, "the training forward's bf16 arm is the matrix-core depthwise (SV_DW_MFMA unset)"
    _dw_fwd(shape, x_dt, "bf16", "mfma", R.dwm_arm(0, *shape))


def _dw_bwd_data(shape, dz_dt, mfma, accumulate, with_bf16, armname):
    B, H, W, C = shape
    o = R.dw_operands(shape, "f32", dz_dt, mfma)
    refs, _, p = R.dw_bwd_data_ref(shape, dz_dt, mfma, accumulate)
    where = (f"dwconv7_bwd_data {cid(shape)} dz {dz_dt} {'accumulate' if accumulate else 'store'}"
             f"{' + bf16 copy' if with_bf16 else ''} [{armname}]")

    def once(b):
        dz, w = b.put("dz", o["dz"], DT[dz_dt]), b.put("w", o["w"].view(-1, 1, 7, 7), F32)
        dx = b.prior("dx", p) if accumulate else b.out("dx", shape, F32)
        dxb = b.out("dxb", shape, BF) if with_bf16 else None
        if mfma:
            nv.call("sv_dwconv7_bwd_data_mfma", K.ptr(dz), K.ptr(w), K.ptr(dx), K.ptr(dxb), int(accumulate), B, H, W, C)
        else:
            nv.call("sv_dwconv7_bwd_data", K.ptr(dz), K.dt(dz), K.ptr(w), K.ptr(dx), K.ptr(dxb), int(accumulate), B, H,
                    W, C)
        return dict(dx=dx, dxb=dxb) if with_bf16 else dict(dx=dx)

    got = twice(where, once)
    judge(where, got, refs)
    if with_bf16:
        bf16_copy_is_rounding(where, got, "dx", "dxb")


BWD_DATA_FORMS = (("f32", True, True), ("bf16", True, False), ("f32", False, False), ("bf16", False, True))


@gpu
@pytest.mark.parametrize("form", BWD_DATA_FORMS, ids=lambda f: f"{f[0]}-{'acc' if f[1] else 'store'}{'-copy' if f[2] else ''}")
@pytest.mark.parametrize("shape", list(DW_VALU), ids=cid)
def test_dw_bwd_data_valu(shape, form):
    assert R.dw_arm(*shape) == DW_VALU[shape]
    _dw_bwd_data(shape, form[0], False, form[1], form[2], R.dw_arm(*shape))


@gpu
@pytest.mark.parametrize("form", [(True, True), (True, False), (False, True), (False, False)],
                         ids=lambda f: f"{'acc' if f[0] else 'store'}{'-copy' if f[1] else ''}")
@pytest.mark.parametrize("shape", list(DW_MFMA), ids=cid)
def test_dw_bwd_data_mfma(shape, form):
    mode = 2 if form[0] else 1
    assert R.dwm_arm(mode, *shape) == DW_MFMA[shape][1], f"{shape} takes {R.dwm_arm(mode, *shape)}"
    assert K.DW_MFMA and shape[3] % 32 == 0  # kernels.dwconv7_bwd_data: bf16 dz -> the matrix cores
    _dw_bwd_data(shape, "bf16", True, form[0], form[1], R.dwm_arm(mode, *shape))


def _dw_bwd_weight(shape, dz_dt, x_dt, mfma, multi, armname):
    """the partials kernel on NaN-filled guarded partials, folded into non-zero priors by reduce_pair, or (``multi``)
    by reduce_multi the way the ``defer=`` list is"""
    B, H, W, C = shape
    o = R.dw_operands(shape, x_dt, dz_dt, mfma)
    refs, _, pr = R.dw_bwd_weight_ref(shape, dz_dt, x_dt, mfma, multi=multi)
    P = R.dwm_wgrad_nparts(*shape) if mfma else R.dw_wgrad_nparts(*shape)
    where = f"dwconv7_bwd_weight {cid(shape)} dz {dz_dt} x {x_dt} {'reduce_multi' if multi else 'reduce_pair'} [{armname} P{P}]"

    def once(b):
        dz, x = b.put("dz", o["dz"], DT[dz_dt]), b.put("x", o["x"], DT[x_dt])
        pw, pb = b.out("pw", (P * C * 49,), F32), b.out("pb", (P * C,), F32)
        dw, db = b.prior("dw", pr["dw"]), b.prior("db", pr["db"])
        if mfma:
            nv.call("sv_dwconv7_bwd_weight_mfma", K.ptr(dz), K.ptr(x), K.dt(x), K.ptr(pw), K.ptr(pb), B, H, W, C)
        else:
            nv.call("sv_dwconv7_bwd_weight", K.ptr(dz), K.dt(dz), K.ptr(x), K.dt(x), K.ptr(pw), K.ptr(pb), B, H, W, C)
        if multi:
            K.reduce_multi([(pw, dw, P, True), (pb, db, P, True)])
        else:
            K.reduce_pair(pw, dw, pb, db, P)
        return dict(dw=dw, db=db, pw=pw, pb=pb)

    got = twice(where, once)
    assert bool(torch.isfinite(got["pw"]).all()) and bool(torch.isfinite(got["pb"]).all()), f"{where}: a partial was not written"
    judge(where, got, refs)


@gpu
@pytest.mark.parametrize("dts", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")], ids="-".join)
@pytest.mark.parametrize("shape", list(DW_VALU), ids=cid)
def test_dw_bwd_weight_valu(shape, dts):
    assert R.dw_arm(*shape) == DW_VALU[shape]
    # the bf16 pair folds through the deferred list's launch, the others through reduce_pair
    _dw_bwd_weight(shape, dts[0], dts[1], False, dts == ("bf16", "bf16"), R.dw_arm(*shape) + " tiles/wave 1")


@gpu
@pytest.mark.parametrize("x_dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(DW_MFMA_WGRAD), ids=cid)
def test_dw_bwd_weight_mfma(shape, x_dt, monkeypatch):
    monkeypatch.setattr(K, "DW_MFMA_WGRAD", True)  # opt-in in the product, as tests/test_dw_mfma_gpu.py
    tiles, P = DW_MFMA_WGRAD[shape]
    assert (R.dwm_geo(*shape)[1], R.dwm_wgrad_nparts(*shape)) == (tiles, P), f"{shape}: the matrix-core geometry was retuned"
    _dw_bwd_weight(shape, "bf16", x_dt, True, x_dt == "bf16", f"mfma tiles{tiles} {'multi-tile' if tiles > P else 'one tile'}")


_MULTI_TILE_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__
__graft_entry__.load_package()
import _convnext_ref as R
from spine_vision_amd import kernels as K
shape, out = eval(sys.argv[2]), {}
assert K.value("sv_dwconv7_bwd_weight_nparts", *shape) == 32
for dz_dt, x_dt in (("f32", "f32"), ("bf16", "f32")):
    o = R.dw_operands(shape, x_dt, dz_dt, False)
    C = shape[3]
    for rep in range(2):
        dw, db = R.prior((C, 49), "dw").float().cuda(), R.prior((C,), "db").float().cuda()
        K.dwconv7_bwd_weight(o["dz"].to(R.DTN[dz_dt]).cuda(), o["x"].to(R.DTN[x_dt]).cuda(), dw=dw, db=db)
        out[f"{dz_dt}-{x_dt}-{rep}"] = (dw.cpu(), db.cpu())
torch.save(out, sys.argv[3])
"""


@gpu
def test_dw_bwd_weight_multi_tile(tmp_path):
    """dwconv7_wgrad_ring_kernel's ``tile += gridDim.x * 4`` loop: a wave takes a second tile only when ntiles > 4
    nparts, which at the default 1024 workgroups needs over 11 M elements; SV_DW_WGRAD_WGS (read once by the library)
    is set in a child process instead: 132 tiles against 4 x 32 wave slots"""
    shape, wgs = MULTI_TILE
    assert R.dw_wgrad_tiles_per_wave(*shape, wgs) == 2 and os.environ.get("SV_DW_WGRAD_WGS") is None
    out_file = tmp_path / "multi_tile.pt"
    r = subprocess.run([sys.executable, "-c", _MULTI_TILE_CHILD, ROOT, repr(shape), str(out_file)],
                       env=dict(os.environ, SV_DW_WGRAD_WGS=str(wgs)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out_file, weights_only=True)
    for dz_dt, x_dt in (("f32", "f32"), ("bf16", "f32")):
        a, b2 = got[f"{dz_dt}-{x_dt}-0"], got[f"{dz_dt}-{x_dt}-1"]
        assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1]), "differs run to run"
        refs, _, _ = R.dw_bwd_weight_ref(shape, dz_dt, x_dt, False, wgs)
        judge(f"dwconv7_bwd_weight {cid(shape)} dz {dz_dt} x {x_dt} SV_DW_WGRAD_WGS={wgs} [{R.dw_arm(*shape)} P32 tiles/wave 2]",
              dict(dw=a[0], db=a[1]), refs)


# ----------------------------------------------------------------------------------------------------- LayerNorm
@gpu
@pytest.mark.parametrize("form", LN_FWD_FORMS, ids="-".join)
@pytest.mark.parametrize("C", LN_C)
def test_layernorm_fwd(C, form):
    x_dt, y_dt = form
    print(f"[convnext_calls] rsqrt term: 4 x torch f32 CPU rsqrt's largest relative error = {R.rsqrt_rel():.3e}")
    assert (R.ln_vec_kind(C) is None) == (C == 64), "ln_vec_kind was retuned: the scalar arm is no longer C = 64 alone"
    w64, b64 = R.ln_params(C)
    for rows in ln_row_counts(C):
        where = f"layernorm_fwd {rows}x{C} x {x_dt} y {y_dt} [{R.ln_arm(rows, C)}]"
        x64 = R.ln_rows(rows, C, x_dt)

        def once(b):
            x, w, bb = b.put("x", x64, DT[x_dt]), b.put("w", w64, F32), b.put("b", b64, F32)
            y, mean, rstd = b.out("y", (rows, C), DT[y_dt]), b.out("mean", (rows,), F32), b.out("rstd", (rows,), F32)
            nv.call("sv_layernorm_fwd", K.ptr(x), K.dt(x), K.ptr(w), K.ptr(bb), K.ptr(y), K.dt(y), K.ptr(mean),
                    K.ptr(rstd), rows, C, K.EPS_LN)
            return dict(y=y, mean=mean, rstd=rstd)

        got = twice(where, once)
        # (row 1 is exactly constant: its reference is rstd = eps^-1/2 and y = lnb, judged like every other row)
        judge(where, got, R.ln_fwd_ref(rows, C, x_dt)[0], store=dict(y=DT[y_dt], mean=F32, rstd=F32))


@gpu
@pytest.mark.parametrize("form", LN_BWD_FORMS, ids="-".join)
@pytest.mark.parametrize("C", LN_C)
def test_layernorm_bwd(C, form):
    dy_dt, x_dt, dx_dt = form
    multi = form in (("f32", "bf16", "f32"), ("bf16", "bf16", "bf16"))  # the deferred list's fold; else the direct one
    for rows in ln_row_counts(C):
        P = R.ln_bwd_nparts(rows, C)
        where = (f"layernorm_bwd {rows}x{C} dy {dy_dt} x {x_dt} dx {dx_dt} {'reduce_multi' if multi else 'reduce_pair'} "
                 f"[{R.ln_arm(rows, C)} P{P}]")
        o, refs, _, pr = R.ln_bwd_ref(rows, C, dy_dt, x_dt, multi)

        def once(b):
            dy, x = b.put("dy", o["dy"], DT[dy_dt]), b.put("x", o["x"], DT[x_dt])
            mean, rstd, w = b.put("mean", o["mean"], F32), b.put("rstd", o["rstd"], F32), b.put("w", o["w"], F32)
            dx = b.out("dx", (rows, C), DT[dx_dt])
            pw = b.out("pw", (2, P * C), F32)
            dw, db = b.prior("dw", pr["dw"]), b.prior("db", pr["db"])
            nv.call("sv_layernorm_bwd", K.ptr(dy), K.dt(dy), K.ptr(x), K.dt(x), K.ptr(mean), K.ptr(rstd), K.ptr(w),
                    K.ptr(dx), K.dt(dx), 0, K.ptr(pw[0]), K.ptr(pw[1]), rows, C)
            if multi:
                K.reduce_multi([(pw[0], dw, P, True), (pw[1], db, P, True)])
            else:
                K.reduce_pair(pw[0], dw, pw[1], db, P)
            return dict(dx=dx, dw=dw, db=db, pw=pw)

        got = twice(where, once)
        assert bool(torch.isfinite(got["pw"]).all()), f"{where}: a partial was not written"
        judge(where, got, refs, store=dict(dx=DT[dx_dt]))


# ---------------------------------------------------------------------------------------------------- downsample
@gpu
@pytest.mark.parametrize("shape", DS_CASES, ids=cid)
def test_downsample(shape):
    B, H, W, C = shape
    o, fwd, bwd, _, pr = R.ds_ref(shape)
    arm = R.ds_arm(shape)
    if shape == (2, 128, 66, 64):
        assert arm == "CPL1 grid1024 passes2 capped"
    if shape == (1, 2, 6, 96):
        assert arm == "g32 grid1 passes1" and B * (H // 2) * (W // 2) == 3  # the second wave's second half is empty
    np_, P = B * (H // 2) * (W // 2), R.ds_grid(*shape)
    for act in ("f32", "bf16"):
        where = f"downsample_fwd {cid(shape)} act {act} [{arm}]"

        def once(b):
            x, w, bb = b.put("x", o["x"].view(shape), F32), b.put("w", o["w"], F32), b.put("b", o["b"], F32)
            patches = b.out("patches", (np_, 4 * C), DT[act])
            mean, rstd = b.out("mean", (B * H * W,), F32), b.out("rstd", (B * H * W,), F32)
            nv.call("sv_downsample_ln_patch2_fwd", K.ptr(x), K.ptr(w), K.ptr(bb), K.EPS_LN, K.ptr(patches),
                    K.dt(patches), K.ptr(mean), K.ptr(rstd), B, H, W, C)
            return dict(patches=patches, mean=mean, rstd=rstd)

        judge(where, twice(where, once), fwd, store=dict(patches=DT[act], mean=F32, rstd=F32))
    for with_bf16 in (False, True):
        where = f"downsample_bwd {cid(shape)}{' + bf16 copy' if with_bf16 else ''} [{arm}]"

        def once(b):
            dp, x = b.put("dp", o["dp"], F32), b.put("x", o["x"].view(shape), F32)
            mean, rstd, w = b.put("mean", o["mean"], F32), b.put("rstd", o["rstd"], F32), b.put("w", o["w"], F32)
            dx = b.out("dx", shape, F32)
            dxb = b.out("dxb", shape, BF) if with_bf16 else None
            pv = b.out("pv", (2, P * C), F32)
            dlnw, dlnb = b.prior("dlnw", pr["dlnw"]), b.prior("dlnb", pr["dlnb"])
            nv.call("sv_downsample_ln_patch2_bwd", K.ptr(dp), K.ptr(x), K.ptr(mean), K.ptr(rstd), K.ptr(w), K.ptr(dx),
                    K.ptr(dxb), K.ptr(pv[0]), K.ptr(pv[1]), B, H, W, C)
            K.reduce_pair(pv[0], dlnw, pv[1], dlnb, P)
            res = dict(dx=dx, dlnw=dlnw, dlnb=dlnb, pv=pv)
            if with_bf16:
                res["dxb"] = dxb
            return res

        got = twice(where, once)
        assert bool(torch.isfinite(got["pv"]).all()), f"{where}: a partial was not written"
        judge(where, got, bwd, store=dict(dx=F32))
        if with_bf16:
            bf16_copy_is_rounding(where, got, "dx", "dxb")


# ---------------------------------------------------------------------------------------------------- pool + LN
@gpu
@pytest.mark.parametrize("case", POOL_CASES, ids=cid)
def test_pool_ln(case):
    B, HW, C = case
    o, fwd, bwd, _, pr = R.pool_ref(B, HW, C)
    arm = R.pool_arm(HW)
    where = f"pool_ln_fwd B{B} HW{HW} C{C} [{arm}]"

    def once(b):
        x, w, bb = b.put("x", o["x"], F32), b.put("w", o["w"], F32), b.put("b", o["b"], F32)
        pooled, feat = b.out("pooled", (B, C), F32), b.out("feat", (B, C), F32)
        mean, rstd = b.out("mean", (B,), F32), b.out("rstd", (B,), F32)
        nv.call("sv_pool_ln_fwd", K.ptr(x), K.ptr(w), K.ptr(bb), K.EPS_LN, K.ptr(pooled), K.ptr(feat), K.ptr(mean),
                K.ptr(rstd), B, HW, C)
        return dict(pooled=pooled, feat=feat, mean=mean, rstd=rstd)

    judge(where, twice(where, once), fwd, store=dict(pooled=F32, feat=F32, mean=F32, rstd=F32))
    for with_bf16 in (False, True):
        where = f"pool_ln_bwd B{B} HW{HW} C{C}{' + bf16 copy' if with_bf16 else ''} [workgroups {R.cdiv(HW, 16)}x{B}]"

        def once(b):
            dfeat, pooled = b.put("dfeat", o["dfeat"], F32), b.put("pooled", o["pooled"], F32)
            mean, rstd, w = b.put("mean", o["mean"], F32), b.put("rstd", o["rstd"], F32), b.put("w", o["w"], F32)
            dx = b.out("dx", (B, HW, C), F32)
            dxb = b.out("dxb", (B, HW, C), BF) if with_bf16 else None
            pv = b.out("pv", (2, B * C), F32)
            dlnw, dlnb = b.prior("dlnw", pr["dlnw"]), b.prior("dlnb", pr["dlnb"])
            nv.call("sv_pool_ln_bwd", K.ptr(dfeat), K.ptr(pooled), K.ptr(mean), K.ptr(rstd), K.ptr(w), K.ptr(dx),
                    K.ptr(dxb), K.ptr(pv[0]), K.ptr(pv[1]), B, HW, C)
            K.reduce_pair(pv[0], dlnw, pv[1], dlnb, B)
            res = dict(dx=dx, dlnw=dlnw, dlnb=dlnb, pv=pv)
            if with_bf16:
                res["dxb"] = dxb
            return res

        got = twice(where, once)
        assert bool(torch.isfinite(got["pv"]).all()), f"{where}: a partial was not written"
        judge(where, got, bwd, store=dict(dx=F32))
        if with_bf16:
            bf16_copy_is_rounding(where, got, "dx", "dxb")


# ---------------------------------------------------------------------------------------------------------- stem
@gpu
@pytest.mark.parametrize("img", STEM_IMGS, ids=cid)
@pytest.mark.parametrize("C", STEM_FWD_C)
def test_stem(C, img):
    B, H, W = img
    o, fwd, bwd, _, pr = R.stem_ref(B, H, W, C)
    arm = R.stem_arm(B, H, W, C)
    npix = B * (H // 4) * (W // 4)
    where = f"stem_fwd {B}x3x{H}x{W} C{C} [{arm}]"

    def once(b):
        im, w, bias = b.put("img", o["img"], F32), b.put("w", o["w"].view(C, 3, 4, 4), F32), b.put("b", o["b"], F32)
        lnw, lnb = b.put("lnw", o["lnw"], F32), b.put("lnb", o["lnb"], F32)
        y, mean, rstd = b.out("y", (npix, C), F32), b.out("mean", (npix,), F32), b.out("rstd", (npix,), F32)
        nv.call("sv_stem_patchify_ln_fwd", K.ptr(im), K.ptr(w), K.ptr(bias), K.ptr(lnw), K.ptr(lnb), K.EPS_LN, K.ptr(y),
                K.dt(y), K.ptr(mean), K.ptr(rstd), B, H, W, C)
        return dict(y=y, mean=mean, rstd=rstd)

    judge(where, twice(where, once), fwd, store=dict(y=F32, mean=F32, rstd=F32))
    if C not in STEM_BWD_C:
        return
    P = R.stem_bwd_nparts(B, H, W, C)
    where = f"stem_bwd {B}x3x{H}x{W} C{C} [{arm}]"

    def once(b):
        im, w, bias = b.put("img", o["img"], F32), b.put("w", o["w"].view(C, 3, 4, 4), F32), b.put("b", o["b"], F32)
        lnw, mean, rstd = b.put("lnw", o["lnw"], F32), b.put("mean", o["mean"], F32), b.put("rstd", o["rstd"], F32)
        dy = b.put("dy", o["dy"], F32)
        pw, pv = b.out("pw", (P * C * 48,), F32), b.out("pv", (3, P * C), F32)
        outs = {n: b.prior(n, pr[n]) for n in ("dw", "db", "dlnw", "dlnb")}
        nv.call("sv_stem_patchify_ln_bwd", K.ptr(im), K.ptr(w), K.ptr(bias), K.ptr(lnw), K.ptr(mean), K.ptr(rstd),
                K.ptr(dy), K.ptr(pw), K.ptr(pv[0]), K.ptr(pv[1]), K.ptr(pv[2]), B, H, W, C)
        K.reduce_pair(pw, outs["dw"], pv[0], outs["db"], P)
        K.reduce_pair(pv[1], outs["dlnw"], pv[2], outs["dlnb"], P)
        return dict(outs, pw=pw, pv=pv)

    got = twice(where, once)
    assert bool(torch.isfinite(got["pw"]).all()) and bool(torch.isfinite(got["pv"]).all()), f"{where}: a partial was not written"
    judge(where, got, bwd)


@gpu
def test_stem_patchify_pack_guarded():
    """stem_patchify / stem_weight_pack are held bitwise by tests/test_kernels_gpu.py; here under guards: the layout
    k = ci 16 + kh 4 + kw with k 48..63 zero, exact bf16 roundings, nothing written outside"""
    B, H, W, C = 2, 8, 12, 96
    o = R.stem_ref(B, H, W, C)[0]
    npix = B * (H // 4) * (W // 4)

    def once(b):
        im, w = b.put("img", o["img"], F32), b.put("w", o["w"].view(C, 3, 4, 4), F32)
        patches, wp = b.out("patches", (npix, 64), BF), b.out("wp", (C, 64), BF)
        nv.call("sv_stem_patchify", K.ptr(im), nv.SV_IMG_F32_NCHW, K._host3((0.0, 0.0, 0.0)), K._host3((1.0, 1.0, 1.0)),
                K.ptr(patches), B, H, W)
        nv.call("sv_stem_weight_pack", K.ptr(w), K.ptr(wp), C)
        return dict(patches=patches, wp=wp)

    got = twice("stem_patchify / stem_weight_pack", once)
    p = o["img"].view(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(npix, 48)
    for name, ref in (("patches", p), ("wp", o["w"])):
        exp = torch.zeros(ref.shape[0], 64, dtype=BF)
        exp[:, :48] = ref.to(BF)
        assert torch.equal(got[name].view(torch.int16), exp.view(torch.int16)), name


# ------------------------------------------------------------------------------------------------------ wrappers
def _eq(where, a, b):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), where


@gpu
def test_wrappers_bit_equal(monkeypatch):
    """each ``kernels.py`` wrapper against the entry point called with the same argument list on guarded buffers: the
    wrapper's dtype codes, argument order, arm selection and fold"""
    dev = torch.device("cuda:0")
    shape = (2, 19, 23, 128)
    B, H, W, C = shape
    rows = B * H * W
    for arm, act, x_dt, mfma_on, save_z in (("mfma", "bf16", "f32", True, True), ("valu", "bf16", "f32", False, True),
                                            ("valu", "f32", "f32", True, True), ("onepass", "bf16", "f32", False, False)):
        monkeypatch.setattr(K, "DW_MFMA", mfma_on)
        o = R.dw_operands(shape, x_dt, "f32", arm == "mfma")
        raw = twice(f"raw {arm}", _dw_fwd_once(shape, x_dt, act, arm))
        z, y, mean, rstd = K.dwconv7_ln_fwd(o["x"].to(DT[x_dt]).to(dev), o["w"].float().view(C, 1, 7, 7).to(dev),
                                            o["b"].float().to(dev), o["lnw"].float().to(dev), o["lnb"].float().to(dev),
                                            act_dtype=DT[act], save_z=save_z)
        assert (z is None) == (arm == "onepass"), arm
        for n, t in (("z", z), ("y", y), ("mean", mean), ("rstd", rstd)):
            if t is not None:
                _eq(f"dwconv7_ln_fwd {arm} {n}", t.cpu(), raw[n])
    # backward-data: bf16 dz -> the matrix cores, f32 dz -> the ring kernel
    monkeypatch.setattr(K, "DW_MFMA", True)
    for dz_dt, mfma in (("bf16", True), ("f32", False)):
        o = R.dw_operands(shape, "f32", dz_dt, mfma)
        p = R.dw_bwd_data_ref(shape, dz_dt, mfma, True)[2]
        dz, w = o["dz"].to(DT[dz_dt]).to(dev), o["w"].float().view(C, 1, 7, 7).to(dev)
        outs = []
        for use_wrapper in (True, False):
            dx, dxb = p.float().to(dev), torch.empty(shape, device=dev, dtype=BF)
            if use_wrapper:
                K.dwconv7_bwd_data(dz, w, dx, accumulate=True, dx_bf16=dxb)
            elif mfma:
                nv.call("sv_dwconv7_bwd_data_mfma", K.ptr(dz), K.ptr(w), K.ptr(dx), K.ptr(dxb), 1, B, H, W, C)
            else:
                nv.call("sv_dwconv7_bwd_data", K.ptr(dz), K.dt(dz), K.ptr(w), K.ptr(dx), K.ptr(dxb), 1, B, H, W, C)
            outs.append((dx.cpu(), dxb.cpu()))
        _eq(f"dwconv7_bwd_data dz {dz_dt} dx", *[t[0] for t in outs])
        _eq(f"dwconv7_bwd_data dz {dz_dt} dx_bf16", *[t[1] for t in outs])
    # backward-weight: direct and deferred, VALU and (opted in) the matrix cores
    for mfma in (False, True):
        monkeypatch.setattr(K, "DW_MFMA_WGRAD", mfma)
        o = R.dw_operands(shape, "f32", "bf16", mfma)
        dz, x = o["dz"].to(BF).to(dev), o["x"].float().to(dev)
        P = R.dwm_wgrad_nparts(*shape) if mfma else R.dw_wgrad_nparts(*shape)
        res = []
        for form in ("direct", "defer", "raw"):
            dw, db = R.prior((C, 49), "dw").float().to(dev), R.prior((C,), "db").float().to(dev)
            if form == "direct":
                K.dwconv7_bwd_weight(dz, x, dw=dw, db=db)
            elif form == "defer":
                folds = []
                K.dwconv7_bwd_weight(dz, x, dw=dw, db=db, defer=folds)
                assert [(s[2], s[3]) for s in folds] == [(P, True), (P, True)]
                K.reduce_pair(folds[0][0], folds[0][1], folds[1][0], folds[1][1], P)
            else:
                pw, pb = torch.empty(P * C * 49, device=dev), torch.empty(P * C, device=dev)
                if mfma:
                    nv.call("sv_dwconv7_bwd_weight_mfma", K.ptr(dz), K.ptr(x), K.dt(x), K.ptr(pw), K.ptr(pb), B, H, W, C)
                else:
                    nv.call("sv_dwconv7_bwd_weight", K.ptr(dz), K.dt(dz), K.ptr(x), K.dt(x), K.ptr(pw), K.ptr(pb), B, H, W, C)
                K.reduce_pair(pw, dw, pb, db, P)
            res.append((dw.cpu(), db.cpu()))
        for r in res[1:]:
            _eq(f"dwconv7_bwd_weight mfma={mfma} dw", r[0], res[0][0])
            _eq(f"dwconv7_bwd_weight mfma={mfma} db", r[1], res[0][1])
    # LayerNorm
    rows, C = 261, 128
    x64, (w64, b64) = R.ln_rows(rows, C, "bf16"), R.ln_params(C)
    x, w, bb = x64.to(BF).to(dev), w64.float().to(dev), b64.float().to(dev)
    y, mean, rstd = K.layernorm_fwd(x, w, bb, out_dtype=F32)
    y2, m2, r2 = (torch.empty(rows, C, device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev))
    nv.call("sv_layernorm_fwd", K.ptr(x), K.dt(x), K.ptr(w), K.ptr(bb), K.ptr(y2), K.dt(y2), K.ptr(m2), K.ptr(r2), rows, C,
            K.EPS_LN)
    for n, a, e in (("y", y, y2), ("mean", mean, m2), ("rstd", rstd, r2)):
        _eq(f"layernorm_fwd {n}", a.cpu(), e.cpu())
    o, _, _, pr = R.ln_bwd_ref(rows, C, "f32", "bf16")
    dy, mean, rstd = o["dy"].float().to(dev), o["mean"].float().to(dev), o["rstd"].float().to(dev)
    P = R.ln_bwd_nparts(rows, C)
    res = []
    for form in ("direct", "finish", "defer", "raw"):
        dw, db = pr["dw"].float().to(dev), pr["db"].float().to(dev)
        if form == "direct":
            dx = K.layernorm_bwd(dy, x, mean, rstd, w, dw=dw, db=db, out_dtype=BF)
        elif form == "raw":
            dx, pw = torch.empty(rows, C, device=dev, dtype=BF), torch.empty(2, P * C, device=dev)
            nv.call("sv_layernorm_bwd", K.ptr(dy), K.dt(dy), K.ptr(x), K.dt(x), K.ptr(mean), K.ptr(rstd), K.ptr(w),
                    K.ptr(dx), K.dt(dx), 0, K.ptr(pw[0]), K.ptr(pw[1]), rows, C)
            K.reduce_pair(pw[0], dw, pw[1], db, P)
        else:
            dx, finish = K.layernorm_bwd(dy, x, mean, rstd, w, dw=dw, db=db, out_dtype=BF, defer_reduce=True)
            if form == "finish":
                finish()
            else:
                folds = []
                finish(defer=folds)
                K.reduce_pair(folds[0][0], folds[0][1], folds[1][0], folds[1][1], P)
        res.append((dx.cpu(), dw.cpu(), db.cpu()))
    for r in res[1:]:
        for n, a, e in zip(("dx", "dw", "db"), r, res[0]):
            _eq(f"layernorm_bwd {n}", a, e)
    # downsample, pool, stem
    shape = (1, 6, 10, 96)
    B, H, W, C = shape
    o, _, _, _, pr = R.ds_ref(shape)
    x, w, bb = o["x"].float().view(shape).to(dev), o["w"].float().to(dev), o["b"].float().to(dev)
    patches, mean, rstd = K.downsample_fwd(x, w, bb, act_dtype=BF)
    p2, m2, r2 = torch.empty_like(patches), torch.empty_like(mean), torch.empty_like(rstd)
    nv.call("sv_downsample_ln_patch2_fwd", K.ptr(x), K.ptr(w), K.ptr(bb), K.EPS_LN, K.ptr(p2), K.dt(p2), K.ptr(m2),
            K.ptr(r2), B, H, W, C)
    for n, a, e in (("patches", patches, p2), ("mean", mean, m2), ("rstd", rstd, r2)):
        _eq(f"downsample_fwd {n}", a.cpu(), e.cpu())
    dp, mean, rstd = o["dp"].float().to(dev), o["mean"].float().to(dev), o["rstd"].float().to(dev)
    dlnw, dlnb = pr["dlnw"].float().to(dev), pr["dlnb"].float().to(dev)
    dx, dxb = K.downsample_bwd(dp, x, mean, rstd, w, dlnw=dlnw, dlnb=dlnb, with_bf16=True)
    P = R.ds_grid(*shape)
    dx2, dxb2, pv = torch.empty_like(dx), torch.empty_like(dxb), torch.empty(2, P * C, device=dev)
    l2, b2 = pr["dlnw"].float().to(dev), pr["dlnb"].float().to(dev)
    nv.call("sv_downsample_ln_patch2_bwd", K.ptr(dp), K.ptr(x), K.ptr(mean), K.ptr(rstd), K.ptr(w), K.ptr(dx2),
            K.ptr(dxb2), K.ptr(pv[0]), K.ptr(pv[1]), B, H, W, C)
    K.reduce_pair(pv[0], l2, pv[1], b2, P)
    for n, a, e in (("dx", dx, dx2), ("dxb", dxb, dxb2), ("dlnw", dlnw, l2), ("dlnb", dlnb, b2)):
        _eq(f"downsample_bwd {n}", a.cpu(), e.cpu())
    B, HW, C = 3, 49, 768
    o, _, _, _, pr = R.pool_ref(B, HW, C)
    x, w, bb = o["x"].float().view(B, 7, 7, C).to(dev), o["w"].float().to(dev), o["b"].float().to(dev)
    feat, pooled, mean, rstd = K.pool_ln_fwd(x, w, bb)
    f2, p2, m2, r2 = torch.empty_like(feat), torch.empty_like(pooled), torch.empty_like(mean), torch.empty_like(rstd)
    nv.call("sv_pool_ln_fwd", K.ptr(x), K.ptr(w), K.ptr(bb), K.EPS_LN, K.ptr(p2), K.ptr(f2), K.ptr(m2), K.ptr(r2), B, HW, C)
    for n, a, e in (("feat", feat, f2), ("pooled", pooled, p2), ("mean", mean, m2), ("rstd", rstd, r2)):
        _eq(f"pool_ln_fwd {n}", a.cpu(), e.cpu())
    dfeat, pooled = o["dfeat"].float().to(dev), o["pooled"].float().to(dev)
    mean, rstd = o["mean"].float().to(dev), o["rstd"].float().to(dev)
    dlnw, dlnb = pr["dlnw"].float().to(dev), pr["dlnb"].float().to(dev)
    dx, dxb = K.pool_ln_bwd(dfeat, pooled, mean, rstd, w, (B, 7, 7, C), dlnw=dlnw, dlnb=dlnb, with_bf16=True)
    dx2, dxb2, pv = torch.empty_like(dx), torch.empty_like(dxb), torch.empty(2, B * C, device=dev)
    l2, b2 = pr["dlnw"].float().to(dev), pr["dlnb"].float().to(dev)
    nv.call("sv_pool_ln_bwd", K.ptr(dfeat), K.ptr(pooled), K.ptr(mean), K.ptr(rstd), K.ptr(w), K.ptr(dx2), K.ptr(dxb2),
            K.ptr(pv[0]), K.ptr(pv[1]), B, HW, C)
    K.reduce_pair(pv[0], l2, pv[1], b2, B)
    for n, a, e in (("dx", dx, dx2), ("dxb", dxb, dxb2), ("dlnw", dlnw, l2), ("dlnb", dlnb, b2)):
        _eq(f"pool_ln_bwd {n}", a.cpu(), e.cpu())
    B, H, W, C = 1, 8, 12, 96
    o, _, _, _, pr = R.stem_ref(B, H, W, C)
    npix = B * (H // 4) * (W // 4)
    im, w, bias = o["img"].float().to(dev), o["w"].float().view(C, 3, 4, 4).to(dev), o["b"].float().to(dev)
    lnw, lnb = o["lnw"].float().to(dev), o["lnb"].float().to(dev)
    y, mean, rstd = K.stem_fwd(im, w, bias, lnw, lnb)
    y2, m2, r2 = torch.empty_like(y), torch.empty_like(mean), torch.empty_like(rstd)
    nv.call("sv_stem_patchify_ln_fwd", K.ptr(im), K.ptr(w), K.ptr(bias), K.ptr(lnw), K.ptr(lnb), K.EPS_LN, K.ptr(y2),
            K.dt(y2), K.ptr(m2), K.ptr(r2), B, H, W, C)
    for n, a, e in (("y", y, y2), ("mean", mean, m2), ("rstd", rstd, r2)):
        _eq(f"stem_fwd {n}", a.cpu(), e.cpu())
    mean, rstd, dy = o["mean"].float().to(dev), o["rstd"].float().to(dev), o["dy"].float().to(dev)
    outs = {n: pr[n].float().to(dev) for n in ("dw", "db", "dlnw", "dlnb")}
    K.stem_bwd(im, w, bias, lnw, mean, rstd, dy.view(B, H // 4, W // 4, C), dw=outs["dw"].view(C, 3, 4, 4), db=outs["db"],
               dlnw=outs["dlnw"], dlnb=outs["dlnb"])
    P = R.stem_bwd_nparts(B, H, W, C)
    o2 = {n: pr[n].float().to(dev) for n in ("dw", "db", "dlnw", "dlnb")}
    pw, pv = torch.empty(P * C * 48, device=dev), torch.empty(3, P * C, device=dev)
    nv.call("sv_stem_patchify_ln_bwd", K.ptr(im), K.ptr(w), K.ptr(bias), K.ptr(lnw), K.ptr(mean), K.ptr(rstd), K.ptr(dy),
            K.ptr(pw), K.ptr(pv[0]), K.ptr(pv[1]), K.ptr(pv[2]), B, H, W, C)
    K.reduce_pair(pw, o2["dw"], pv[0], o2["db"], P)
    K.reduce_pair(pv[1], o2["dlnw"], pv[2], o2["dlnb"], P)
    for n in outs:
        _eq(f"stem_bwd {n}", outs[n].cpu(), o2[n].cpu())


# ------------------------------------------------------------------------------------ reference-side conditions
_MISSED = []  # every condition is printed before the test asserts that none was missed


def _f32_within(where, emu, ref_bound, store=None):
    ref, bound = ref_bound
    if store is not None:
        bound = bound + R.store_bound(ref, store)
    ratio = float(((emu.double().reshape(ref.shape) - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"[convnext_calls cpu] {where}: f32 emulation error / bound {ratio:.3f}")
    if not ratio <= 1.0:
        _MISSED.append(f"{where}: a float32 evaluation misses the bound ({ratio:.3f}): the bound is too tight")


def _visible(where, sens):
    print(f"[convnext_calls cpu] {where}: share of elements a dropped contribution moves by > 4 x bound: "
          + ", ".join(f"{n} {s:.4f}" for n, s in sens.items()))
    for n, s in sens.items():
        if not s >= 0.99:
            _MISSED.append(f"{where} {n}: only {s:.4f} of the elements would show a dropped contribution")


def _ln_f32(x, w, b):
    """LayerNorm in float32 torch ops (the order of a sum does not enter the bound beyond its depth)"""
    x = x.float()
    mu = x.mean(1)
    d = x - mu[:, None]
    rs = ((d * d).mean(1) + EPS32).rsqrt()
    return d * rs[:, None] * w.float() + b.float(), mu, rs


EPS32 = torch.tensor(R.EPS, dtype=F32)


def test_reference_side_conditions():
    """On the CPU, per case and output: dropping one contribution (a tap; a pixel or row of a reduction; a channel of a
    row's statistics) moves the float64 value by more than 4 x the bound in at least 99 % of the affected elements, and
    a float32 evaluation of the operation stays within 1 x the bound.  Printed shares:
    profiles/convnext_calls/cpu_conditions.txt.  For a bf16-stored y a dropped channel of the statistics is visible in
    mean / rstd only (y's store bound 2^-8 |y| exceeds its effect at large C): the condition is stated on those."""
    print(f"[convnext_calls cpu] rsqrt term {R.rsqrt_rel():.3e}")
    _MISSED.clear()
    # depthwise
    for shape in [(2, 19, 23, 64)] + list(DW_VALU):
        for act in ("f32", "bf16"):
            refs, sens = R.dw_fwd_ref(shape, "f32", act, False)
            if min(shape[1:3]) >= 3:
                _visible(f"dw fwd valu {cid(shape)} act {act} (centre tap)", sens)
        o = R.dw_operands(shape, "f32", "f32", False)
        _f32_within(f"dw fwd valu {cid(shape)} z", R.dw_conv(o["x"].float(), o["w"].float()) + o["b"].float(), refs["z"], F32)
        for dz_dt, acc in (("f32", True), ("bf16", False)):
            refs, sens, p = R.dw_bwd_data_ref(shape, dz_dt, False, acc)
            _visible(f"dw bwd-data valu {cid(shape)} dz {dz_dt} (centre tap)", sens)
            od = R.dw_operands(shape, "f32", dz_dt, False)
            emu = R.dw_conv(od["dz"].float(), od["w"].float(), flip=True)
            _f32_within(f"dw bwd-data valu {cid(shape)} dz {dz_dt}", emu + p.float() if acc else emu, refs["dx"])
        for dts in (("f32", "f32"), ("bf16", "bf16")):
            refs, sens, pr = R.dw_bwd_weight_ref(shape, dts[0], dts[1], False)
            if shape[0] * shape[1] * shape[2] > 1:
                _visible(f"dw bwd-weight valu {cid(shape)} {dts} (one pixel)", sens)
            ow = R.dw_operands(shape, dts[1], dts[0], False)
            _f32_within(f"dw bwd-weight valu {cid(shape)} {dts} dw", R.dw_wgrad(ow["dz"].float(), ow["x"].float()) + pr["dw"].float(),
                        refs["dw"])
    s, wgs = MULTI_TILE
    _visible(f"dw bwd-weight valu {cid(s)} WGS {wgs} (one pixel)", R.dw_bwd_weight_ref(s, "f32", "f32", False, wgs)[1])
    for shape in DW_MFMA:
        for x_dt in ("f32", "bf16"):
            refs, sens = R.dw_fwd_ref(shape, x_dt, "bf16", True)
            if min(shape[1:3]) >= 3:
                _visible(f"dw fwd mfma {cid(shape)} x {x_dt} (centre tap)", sens)
        _visible(f"dw bwd-data mfma {cid(shape)} (centre tap)", R.dw_bwd_data_ref(shape, "bf16", True, True)[1])
    for shape in DW_MFMA_WGRAD:
        if shape[0] * shape[1] * shape[2] > 1:
            _visible(f"dw bwd-weight mfma {cid(shape)} (one pixel)", R.dw_bwd_weight_ref(shape, "bf16", "bf16", True)[1])
    # LayerNorm
    for C in LN_C:
        w, b = R.ln_params(C)
        for rows in ln_row_counts(C):
            for x_dt in ("f32", "bf16"):
                refs, sens = R.ln_fwd_ref(rows, C, x_dt)
                _visible(f"ln fwd {rows}x{C} x {x_dt} (one channel of the statistics)", sens)
                y, mu, rs = _ln_f32(R.ln_rows(rows, C, x_dt), w, b)
                for n, t in (("y", y), ("mean", mu), ("rstd", rs)):
                    _f32_within(f"ln fwd {rows}x{C} x {x_dt} {n}", t, refs[n], F32)
            o, refs, sens, pr = R.ln_bwd_ref(rows, C, "f32", "bf16")
            if rows >= 8:  # with fewer rows a channel's candidates are too few for an RMS
                _visible(f"ln bwd {rows}x{C} (one row)", sens)
            xh = ((o["x"].float() - o["mean"].float()[:, None]) * o["rstd"].float()[:, None])
            d = o["dy"].float()
            g = d * o["w"].float()
            dx = o["rstd"].float()[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
            _f32_within(f"ln bwd {rows}x{C} dx", dx, refs["dx"], F32)
            _f32_within(f"ln bwd {rows}x{C} dw", (d * xh).sum(0) + pr["dw"].float(), refs["dw"])
            _f32_within(f"ln bwd {rows}x{C} db", d.sum(0) + pr["db"].float(), refs["db"])
    # downsample, pool, stem: the reductions' sensitivity and the forward in float32
    for shape in DS_CASES:
        o, fwd, bwd, sens, pr = R.ds_ref(shape)
        if shape[0] * shape[1] * shape[2] >= 8:
            _visible(f"downsample bwd {cid(shape)} (one pixel)", sens)
        y, mu, rs = _ln_f32(o["x"], o["w"], o["b"])
        _f32_within(f"downsample fwd {cid(shape)} mean", mu, fwd["mean"], F32)
        _f32_within(f"downsample fwd {cid(shape)} rstd", rs, fwd["rstd"], F32)
    for B, HW, C in POOL_CASES:
        o, fwd, bwd, sens, pr = R.pool_ref(B, HW, C)
        vis = {n: s for n, s in sens.items() if n == "pooled" or B >= 3}  # dlnw / dlnb: the RMS over three images
        _visible(f"pool B{B} HW{HW} C{C} (one row of the pool" + (", one image of dlnw / dlnb)" if B >= 3 else ")"), vis)
        pooled = o["x"].float().mean(1)
        _f32_within(f"pool B{B} HW{HW} C{C} pooled", pooled, fwd["pooled"], F32)
        y, mu, rs = _ln_f32(pooled, o["w"], o["b"])
        _f32_within(f"pool B{B} HW{HW} C{C} feat", y, fwd["feat"], F32)
    for B, H, W in STEM_IMGS:
        for C in STEM_BWD_C:
            o, fwd, bwd, sens, pr = R.stem_ref(B, H, W, C)
            vis = {n: s for n, s in sens.items() if n == "y" or B * (H // 4) * (W // 4) >= 6}
            _visible(f"stem {B}x3x{H}x{W} C{C} (one patch element of y; one pixel of the gradients)", vis)
            p = o["img"].float().view(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 48)
            y, mu, rs = _ln_f32(p @ o["w"].float().t() + o["b"].float(), o["lnw"], o["lnb"])
            _f32_within(f"stem {B}x3x{H}x{W} C{C} y", y, fwd["y"], F32)
    assert not _MISSED, "\n".join(_MISSED)
