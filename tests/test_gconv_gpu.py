"""The grouped 3x3 convolution kernels (csrc/gconv.hip: sv_gconv_weight_pack / _fwd / _bwd_data / _bwd_weight) -- timm
Bottleneck.conv2 of ResNeXt-50 (groups 32; C = 128 / 256 / 512 / 1024, so 4 / 8 / 16 / 32 channels per group) --
against float64 ``F.conv2d(..., groups=32)`` and its autograd over the same bf16-rounded operands.

Bounds.  The kernels multiply bf16 operands exactly and sum in f32, so a bf16 output differs from bf16(reference) only
where the f32 sum's rounding flips the bf16 rounding: per element one bf16 rounding step of the result (2^-8 relative
to the float64 value, the form tests/test_dw_mfma_gpu.py uses) plus the f32 sum's own error (1e-6 of the largest
result: 288 products at most).  The f32 weight gradient: relative L2 < 1e-4, the project's f32 convolution bound.
Cases: the smallest images at which borders (5 x 7), tile edges (17 x 18: 612 pixels = 38 tiles of 16 and a quarter
tile, 19 chunks of 32 and a part) and the strided parities (9 x 9 odd, 8 x 10 even) can go wrong."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

pytestmark = pytest.mark.gpu

GROUPS = 32
IMAGES = [(2, 5, 7, 1), (2, 17, 18, 1), (2, 9, 9, 2), (2, 8, 10, 2)]
CHANNELS = [128, 256, 512, 1024]
CASES = [(B, H, W, C, s) for (B, H, W, s) in IMAGES for C in CHANNELS]
IDS = ["x".join(map(str, c)) for c in CASES]


def _q(t):
    return t.to(torch.bfloat16).to(torch.float64)


@functools.lru_cache(maxsize=None)
def _case(case):
    """bf16-rounded operands (NHWC x / dy, torch-layout w) and the float64 reference y, dx, dw; computed once per case
    and shared by the tests (never modified)."""
    B, H, W, C, s = case
    g = torch.Generator().manual_seed(1000 * C + 100 * H + 10 * W + s)
    Cg = C // GROUPS
    x = _q(torch.randn(B, H, W, C, generator=g))
    w = _q(torch.randn(C, Cg, 3, 3, generator=g) / (3.0 * Cg ** 0.5))
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=1, groups=GROUPS)
    dy = _q(torch.randn(y.shape, generator=g) * 0.5)
    y.backward(dy)
    return dict(x=x, w=w, dy=dy.permute(0, 2, 3, 1).contiguous(), y=y.detach().permute(0, 2, 3, 1).contiguous(),
                dx=xr.grad.permute(0, 2, 3, 1).contiguous(), dw=wr.grad)


def _dev(case, dev):
    r = _case(case)
    B, H, W, C, s = case
    x = r["x"].to(dev, torch.bfloat16)
    dy = r["dy"].to(dev, torch.bfloat16)
    w = r["w"].float().to(dev)
    shape = K.gconv_shape(B, H, W, C, GROUPS, 3, s, 1)
    wp, = K.gconv_weight_pack([w], GROUPS)
    return r, x, dy, w, shape, wp


def _assert_bf16_step(got, ref, what):
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-6 * float(ref.abs().max())
    print(f"[gconv] {what}: max err {float(err.max()):.3e}, largest |ref| {float(ref.abs().max()):.3e}, "
          f"{float((got.cpu() == ref.to(torch.bfloat16)).float().mean()):.5f} equal bf16(ref)")
    assert not (err > bound).any(), (what, int((err > bound).sum()), float(err.max()))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_fwd_dgrad_wgrad(dev, case):
    r, x, dy, w, shape, wp = _dev(case, dev)
    y = K.gconv_fwd(x, wp, shape)
    assert y.shape == r["y"].shape and y.dtype == torch.bfloat16
    _assert_bf16_step(y, r["y"], f"{case} y")
    dx = K.gconv_bwd_data(dy, wp, shape)
    assert dx.shape == r["dx"].shape and dx.dtype == torch.bfloat16
    _assert_bf16_step(dx, r["dx"], f"{case} dx")
    dw = torch.zeros_like(w)
    K.gconv_bwd_weight(dy, x, shape, dw=dw, accumulate=False)
    e = _rel(dw, r["dw"])
    print(f"[gconv] {case} dw rel L2 {e:.3e}")
    assert e < 1e-4
    base = torch.ones_like(w)
    K.gconv_bwd_weight(dy, x, shape, dw=base, accumulate=True)
    assert _rel(base - 1.0, dw) < 1e-6
    # run to run, each pass
    assert torch.equal(K.gconv_fwd(x, wp, shape), y)
    assert torch.equal(K.gconv_bwd_data(dy, wp, shape), dx)
    dw2 = torch.empty_like(w)
    K.gconv_bwd_weight(dy, x, shape, dw=dw2, accumulate=False)
    assert torch.equal(dw2, dw)


@pytest.mark.parametrize("case", [(2, 5, 7, 128, 1), (2, 9, 9, 256, 2), (2, 8, 10, 512, 2), (2, 5, 7, 1024, 1)],
                         ids=lambda c: "x".join(map(str, c)))
def test_gconv_group_isolation(dev, case):
    """Changing one group's input channels changes only that group's output channels (the others bitwise equal); the
    same for dx from dy."""
    r, x, dy, w, shape, wp = _dev(case, dev)
    C = case[3]
    Cg = C // GROUPS
    grp = 5
    lo, hi = grp * Cg, (grp + 1) * Cg
    other = torch.ones(C, dtype=torch.bool, device=dev)
    other[lo:hi] = False
    for fn, t in ((K.gconv_fwd, x), (K.gconv_bwd_data, dy)):
        a = fn(t, wp, shape)
        t2 = t.clone()
        t2[..., lo:hi] = (t2[..., lo:hi].float() * -1.5 + 0.25).to(torch.bfloat16)
        b = fn(t2, wp, shape)
        assert torch.equal(a[..., other], b[..., other])
        assert not torch.equal(a[..., lo:hi], b[..., lo:hi])


def _assert_adjacent_bf16(a, b, what):
    """Two bf16 roundings of f32 sums that differ by f32 summation error are equal or adjacent bf16 values (2^-7
    relative at most), except below that summation error itself (1e-6 of the largest value)."""
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    bound = b.abs() * 2.0 ** -7 + 1e-6 * float(b.abs().max())
    print(f"[gconv vs dense] {what}: max diff {float(err.max()):.3e}, {float((a == b).float().mean()):.5f} equal")
    assert not (err > bound).any(), (what, int((err > bound).sum()), float(err.max()))


@pytest.mark.parametrize("case", [(2, 8, 10, 128, 2), (2, 17, 18, 256, 1), (2, 8, 10, 512, 2), (2, 17, 18, 1024, 1)],
                         ids=lambda c: "x".join(map(str, c)))
def test_gconv_matches_dense_embedding(dev, case):
    r, x, dy, w, shape, wp = _dev(case, dev)
    B, H, W, C, s = case
    ds = K.conv_shape(B, H, W, C, C, 3, s, 1)
    dwp = K.conv_weight_pack(K.grouped_as_dense(w, GROUPS).contiguous(), C, torch.bfloat16)
    _assert_adjacent_bf16(K.gconv_fwd(x, wp, shape), K.conv_fwd(x, dwp, ds, torch.bfloat16), f"{case} y")
    _assert_adjacent_bf16(K.gconv_bwd_data(dy, wp, shape), K.conv_bwd_data(dy, dwp, ds, dx_dtype=torch.bfloat16),
                          f"{case} dx")
    dw = torch.zeros_like(w)
    K.gconv_bwd_weight(dy, x, shape, dw=dw, accumulate=False)
    dense_dw = torch.zeros(C, C, 3, 3, device=dev)
    K.conv_bwd_weight(dy, x, ds, dw=dense_dw, accumulate=False)
    e = _rel(dw, K.dense_group_blocks(dense_dw, GROUPS))
    print(f"[gconv vs dense] {case} dw rel L2 {e:.3e}")
    assert e < 1e-4


@pytest.mark.parametrize("bad", [dict(C=2048, groups=32), dict(C=144, groups=36), dict(C=128, groups=32, k=5)],
                         ids=["Cg64", "C144", "k5"])
def test_gconv_rejects_unsupported(dev, bad):
    """Cg = 64, C % 32 != 0 and a 5x5 kernel: SV_ERR_UNSUPPORTED (2) from every entry point, nothing launched (the
    output keeps its fill)."""
    C, groups, k = bad["C"], bad["groups"], bad.get("k", 3)
    with pytest.raises(ValueError):
        K.gconv_shape(2, 8, 8, C, groups, k, 1, k // 2 if k != 5 else 1)
    s = nv.GConvShape(2, 8, 8, C, groups, k, k, 1, 1)
    x = torch.zeros(2, 8, 8, C, device=dev, dtype=torch.bfloat16)
    y = torch.full_like(x, 7.0)
    wp = torch.zeros(2, (C + 31) // 32, 9, 2, 64, 8, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(C, C // groups, k, k, device=dev)
    dw = torch.full((C, C // groups, 3, 3), 7.0, device=dev)
    work = torch.zeros(1 << 16, device=dev)
    seg = (nv.GConvPackSeg * 1)(nv.GConvPackSeg(K.ptr(w), K.ptr(wp[0]), K.ptr(wp[1]), C, groups))
    calls = [("sv_gconv_fwd", K.ptr(x), K.ptr(wp[0]), K.ptr(y), ctypes.byref(s)),
             ("sv_gconv_bwd_data", K.ptr(x), K.ptr(wp[1]), K.ptr(y), ctypes.byref(s)),
             ("sv_gconv_bwd_weight", K.ptr(x), K.ptr(x), K.ptr(work), K.ptr(dw), 0, ctypes.byref(s))]
    if k == 3:
        calls.append(("sv_gconv_weight_pack", seg, 1))
    for c in calls:
        with pytest.raises(RuntimeError, match=r"status 2"):
            K.call(*c)
    assert nv.value("sv_gconv_bwd_weight_nparts", ctypes.byref(s)) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dw == 7.0).all()) and bool((wp == 0).all())
