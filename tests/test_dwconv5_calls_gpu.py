"""The three csrc/dwconv5.hip calls (depthwise 5x5, pad 2, stride 1 | 2) one at a time through their
``spine_vision_amd.kernels`` wrappers, each output compared ELEMENT BY ELEMENT with a float64 CPU evaluation of the same
operation on the same rounded operands -- in the manner of tests/test_mbconv_calls_gpu.py, whose guarded buffers and
run-twice harness are reused.

Bounds, derived from the summation orders at the top of csrc/dwconv5.hip and asserted at 2 x for EVERY element
(u = 2^-24; S = the same operation over the operands' absolute values):
    forward, data gradient   25 u S: one fmaf chain of at most 25 links per element (bf16 products are exact in f32, an
                             f32 product rounds inside the fmaf)
    weight gradient          (depth + P - 1) u S, depth = 4 ceil(spp / 16) + 15: a thread's strips of 4 pixels, then lane 0
                             adding lanes 1 .. 15; the fold of the P parts adds (P - 1) u sum |part| <= (P - 1) u S;
                             accumulate adds u |ref| for dw + sum
    stores                   2^-8 |ref| for a bf16 store
Guards: outputs start as NaN (the accumulating dw as a known prior) between sentinels; every call runs twice with
bit-equal results.  The figures of a GPU run are recorded in profiles/efficientnet_b/parity.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _calls_harness import f32, judge as _judge, store
from _conv_ref import BF, F32, F64, U24
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv
from test_mbconv_calls_gpu import DT, NAN, Buffers, nhwc, twice

gpu = pytest.mark.gpu
judge = functools.partial(_judge, "dwconv5_calls")

# (B, H, W, C)
SHAPES = [(2, 5, 7, 96),     # odd sizes, C not a power of two
          (3, 6, 6, 32),     # even sizes: at stride 2 the last window overhangs by one
          (1, 1, 1, 64),     # only the centre tap is inside
          (1, 2, 2, 32),     # the grid is narrower than the window
          (2, 3, 4, 1152),   # wide C
          (1, 33, 17, 64),   # several workgroups, ragged tails
          (1, 40, 40, 32)]   # 400 strips at stride 1: six weight-gradient parts of 67 strips, the last one short
CASES = [(s, m) for s in SHAPES for m in ("bf16", "fp32") if m == "bf16" or s in SHAPES[:2]]
IDS = ["x".join(map(str, s)) + "-" + m for s, m in CASES]


def geo(B, OH, OW):
    """(P, spp, depth) of the weight gradient (csrc/dwconv5.hip nparts_for / bwd_weight_kernel)"""
    strips = B * OH * (-(-OW // 4))
    P = max(1, min(64, strips // 64))
    spp = -(-strips // P)
    return P, spp, 4 * (-(-spp // 16)) + 15


@functools.lru_cache(maxsize=None)
def operands(shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    g = torch.Generator().manual_seed(11 * B + 100 * H + 10 * W + C + stride + len(mode))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, C, H, W, generator=g, dtype=F64).to(dt).double()
    w = f32(torch.randn(C, 1, 5, 5, generator=g, dtype=F64) / 5)
    dy = (torch.rand(B, C, OH, OW, generator=g, dtype=F64) * 2 - 1).to(dt).double()
    prior = f32(torch.randn(C, 1, 5, 5, generator=g, dtype=F64))
    return x, w, dy, prior, OH, OW


@gpu
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_dwconv5_fwd(dev, shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    x, w, _, _, OH, OW = operands(shape, mode, stride)

    def once(b):
        y = K.dwconv5_fwd(b.put("x", nhwc(x), dt), b.put("w", w), stride, out_dtype=dt, out=b.out("y", (B, OH, OW, C), dt))
        return dict(y=y)

    got = twice(f"dwconv5_fwd {shape} s{stride} {mode}", once)
    ref = nhwc(F.conv2d(x, w, stride=stride, padding=2, groups=C))
    S = nhwc(F.conv2d(x.abs(), w.abs(), stride=stride, padding=2, groups=C))
    judge(f"dwconv5_fwd {shape} s{stride} {mode}", got, dict(y=(ref, 25 * U24 * S + store(ref, dt))))


@gpu
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_dwconv5_bwd_data(dev, shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    _, w, dy, _, OH, OW = operands(shape, mode, stride)

    def once(b):
        dx = K.dwconv5_bwd_data(b.put("dy", nhwc(dy), dt), b.put("w", w), H, W, stride, dx_dtype=dt,
                                out=b.out("dx", (B, H, W, C), dt))
        return dict(dx=dx)

    got = twice(f"dwconv5_bwd_data {shape} s{stride} {mode}", once)
    ref = nhwc(torch.nn.grad.conv2d_input((B, C, H, W), w, dy, stride=stride, padding=2, groups=C))
    S = nhwc(torch.nn.grad.conv2d_input((B, C, H, W), w.abs(), dy.abs(), stride=stride, padding=2, groups=C))
    judge(f"dwconv5_bwd_data {shape} s{stride} {mode}", got, dict(dx=(ref, 25 * U24 * S + store(ref, dt))))


@gpu
@pytest.mark.parametrize("accumulate", (True, False), ids=("acc", "store"))
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_dwconv5_bwd_weight(dev, shape, mode, stride, accumulate):
    B, H, W, C = shape
    dt = DT[mode]
    x, _, dy, prior, OH, OW = operands(shape, mode, stride)
    P, spp, depth = geo(B, OH, OW)
    assert P == nv.value("sv_dwconv5_bwd_weight_nparts", B, H, W, C, stride)

    def once(b):
        dw = b.put("dw", prior) if accumulate else b.out("dw", (C, 1, 5, 5))
        K.dwconv5_bwd_weight(b.put("dy", nhwc(dy), dt), b.put("x", nhwc(x), dt), stride, dw=dw, accumulate=accumulate)
        return dict(dw=dw)

    got = twice(f"dwconv5_bwd_weight {shape} s{stride} {mode}", once)
    term = torch.nn.grad.conv2d_weight(x, (C, 1, 5, 5), dy, stride=stride, padding=2, groups=C)
    S = torch.nn.grad.conv2d_weight(x.abs(), (C, 1, 5, 5), dy.abs(), stride=stride, padding=2, groups=C)
    bound = (depth + P - 1) * U24 * S
    ref = term
    if accumulate:
        ref = prior + term
        bound = bound + U24 * ref.abs()
    judge(f"dwconv5_bwd_weight {shape} s{stride} {mode} P{P} spp{spp} depth{depth}", got, dict(dw=(ref, bound)))


@gpu
def test_nparts_matches_library():
    for B, H, W in ((1, 1, 1), (1, 40, 40), (2, 33, 17), (32, 64, 64), (32, 8, 8), (64, 128, 128)):
        for stride in (1, 2):
            OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
            for C in (32, 96, 1152, 3840):
                assert geo(B, OH, OW)[0] == nv.value("sv_dwconv5_bwd_weight_nparts", B, H, W, C, stride), (B, H, W, C, stride)
    assert geo(1, 40, 40)[0] == 6  # the short-last-part case of SHAPES
    for C, stride in ((24, 1), (3872, 1), (64, 3)):
        assert nv.value("sv_dwconv5_bwd_weight_nparts", 2, 4, 4, C, stride) == 0


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


@gpu
@pytest.mark.parametrize("C,stride", ((24, 1), (3872, 1), (64, 3)), ids=("C24", "C3872", "stride3"))
def test_unsupported_shapes_are_refused(dev, C, stride):
    """the wrappers refuse before the library, the library refuses (SV_ERR_UNSUPPORTED = status 2) before any launch; the
    outputs keep their NaN pre-fill either way"""
    B, H, W = 1, 4, 4
    b = Buffers()
    x, dy = b.put("x", torch.zeros(B, H, W, C)), b.put("dy", torch.zeros(B, H, W, C))
    w = b.put("w", torch.zeros(C, 1, 5, 5))
    y, dx, dw = b.out("y", (B, H, W, C)), b.out("dx", (B, H, W, C)), b.out("dw", (C, 1, 5, 5))
    part = b.out("part", (1, 25, C))
    for call in (lambda: K.dwconv5_fwd(x, w, stride, out=y),
                 lambda: K.dwconv5_bwd_data(dy, w, H, W, stride, out=dx),
                 lambda: K.dwconv5_bwd_weight(dy, x, stride, dw=dw, accumulate=False)):
        with pytest.raises(ValueError):
            call()
    p = lambda t: t.data_ptr()  # noqa: E731
    for name, args in (("sv_dwconv5_fwd", (p(x), nv.SV_F32, p(w), p(y), nv.SV_F32)),
                       ("sv_dwconv5_bwd_data", (p(dy), nv.SV_F32, p(w), p(dx), nv.SV_F32)),
                       ("sv_dwconv5_bwd_weight", (p(dy), nv.SV_F32, p(x), nv.SV_F32, p(part), p(dw), 0))):
        with pytest.raises(RuntimeError, match="status 2"):
            nv.call(name, *args, B, H, W, C, stride)
    torch.cuda.synchronize()
    b.check(f"refusals C{C} s{stride}")
    assert all(_all_nan(t) for t in (y, dx, dw, part)), "a refused call wrote its output"


@gpu
def test_non_contiguous_input_is_refused(dev):
    B, H, W, C = 1, 4, 4, 64
    b = Buffers()
    wide = b.put("wide", torch.zeros(B, H, W, 2 * C))
    view = wide[..., :C]  # channel stride 1, row stride 2 C
    full = b.put("full", torch.zeros(B, H, W, C))
    w = b.put("w", torch.zeros(C, 1, 5, 5))
    y, dx, dw = b.out("y", (B, H, W, C)), b.out("dx", (B, H, W, C)), b.out("dw", (C, 1, 5, 5))
    for call in (lambda: K.dwconv5_fwd(view, w, 1, out=y),
                 lambda: K.dwconv5_bwd_data(view, w, H, W, 1, out=dx),
                 lambda: K.dwconv5_bwd_weight(view, full, 1, dw=dw, accumulate=False),
                 lambda: K.dwconv5_bwd_weight(full, view, 1, dw=dw, accumulate=False)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    b.check("non-contiguous refusals")
    assert all(_all_nan(t) for t in (y, dx, dw)), "a refused call wrote its output"
