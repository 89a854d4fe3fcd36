"""Every csrc/mbconv.hip call of an EfficientNetV2 step, one call at a time through its ``spine_vision_amd.kernels``
wrapper, each output compared ELEMENT BY ELEMENT with a float64 CPU evaluation of the same operation on the same rounded
operands; and one dense 3x3 (24 -> 96, stride 2, 7 x 9) through the padded-stride scheme of backbone/efficientnet.py.

Calls                                                   -> test here
    dwconv3_fwd / dwconv3_bwd_data / dwconv3_bwd_weight  -> test_dwconv3_*
    mb_bn_stats                                          -> test_bn_stats
    bn_silu_fwd (plain and residual form)                -> test_bn_silu_fwd
    bn_silu_bwd_stats / bn_silu_bwd_apply                -> test_bn_silu_bwd_stats / test_bn_silu_bwd_apply
    mbse_squeeze / mbse_excite / mbse_scale              -> test_squeeze / test_excite / test_scale, test_batch_independence
    mbse_bwd_stats / mbse_bwd_gate / mbse_bwd_apply      -> test_bwd_stats / test_bwd_gate / test_bwd_apply
    mb_add                                               -> test_add
    _conv3 + conv_bwd_data + conv_bwd_weight, padded     -> test_padded_dense_conv

Inputs.  Each call is judged alone: its inputs are the f32 (or bf16) roundings of the float64 results of the calls before
it, not those calls' outputs.  SiLU has no ties, so no element is excluded.

Bounds, derived from the summation orders and rounding points documented at the top of csrc/mbconv.hip and
csrc/se_core.h and asserted at 2 x for EVERY element (u = 2^-24):
    pre              e_pre = u (3 |t| + |pre|), t = gamma rstd (y - mean): gamma rstd, y - mean, the fmaf
    sigmoid          4 u sig (expf within 1 ulp = 2 u, one add, one correctly rounded division), slope <= 1/4 on the argument
    silu             |silu'| <= 1.1 on the argument's bound, plus 5 u |silu| (the sigmoid and the product)
    silu'            |silu''| <= 1/2 on the argument's bound, plus u (5 sig |x| + 6 |silu'|) (1 - sig, the fmaf, two products)
    depthwise taps   9 u sum |x w| (one fmaf chain of at most 9)
    channel sums     depth u sum |t|, depth = ceil(rpp / 64) + 7 + 7 (a thread's serial rows, then the two lane levels);
                     the consumer's fold of P parts adds (P - 1) u sum |part|
    matvec           depth u sum |w x|, depth = 4 ceil(K / 256) + 6 + 1; transposed: depth = ceil(K / 16) + 15
    elementwise      one u |value| per rounded operation, written out per formula below
    stores           2^-8 |ref| for a bf16 store
Guards: outputs start as NaN (accumulating ones as a known prior); every buffer sits between sentinels; every call runs
twice with bit-equal results.  The figures of a GPU run are recorded in profiles/efficientnetv2/parity.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _calls_harness import f32, judge as _judge, mv_depth, store, tm_depth
from _conv_ref import BF, F32, F64, U24, acc_bound
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
SENTINEL, GUARD, NAN = -7.0, 256, float("nan")
DT = {"bf16": BF, "fp32": F32}
DEV = "cuda:0"

# (B, H, W, C)
DW_SHAPES = [(2, 5, 7, 96),    # odd sizes, C not a power of two
             (3, 6, 6, 32),    # even sizes, narrowest C
             (1, 1, 1, 64),    # every tap but the centre lies in the padding
             (2, 2, 3, 960),
             (1, 33, 17, 64),  # several workgroups, ragged tails
             (1, 40, 40, 32)]  # 1600 rows: three parts of 534 rows, the last one short
SE_SHAPES = DW_SHAPES + [(2, 4, 4, 3840), (5, 3, 3, 256)]
RD = {96: 8, 32: 4, 64: 16, 960: 40, 3840: 160, 256: 16}


def _cases(shapes):
    cs = [(s, m) for s in shapes for m in ("bf16", "fp32") if m == "bf16" or s in DW_SHAPES[:2]]
    return cs, ["x".join(map(str, s)) + "-" + m for s, m in cs]


DW_CASES, DW_IDS = _cases(DW_SHAPES)
SE_CASES, SE_IDS = _cases(SE_SHAPES)
STAT_CASES, STAT_IDS = _cases([s for s in SE_SHAPES if s[0] * s[1] * s[2] > 1])  # batch statistics need two rows


# ------------------------------------------------------------------------------------------------------ harness
class Buffers:
    """device buffers between sentinels"""

    def __init__(self):
        self.dev, self.bufs = torch.device(DEV), {}

    def _make(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=self.dev, dtype=dtype)
        self.bufs[name] = buf
        return buf[GUARD:GUARD + n].view(shape)

    def put(self, name, t, dtype=F32):
        v = self._make(name, tuple(t.shape), dtype)
        v.copy_(t.to(dtype))
        return v

    def out(self, name, shape, dtype=F32):
        v = self._make(name, tuple(shape), dtype)
        v.fill_(NAN)
        return v

    def check(self, where):
        for n, b in self.bufs.items():
            assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), \
                f"{where}: sentinel around {n} overwritten"


def twice(where, once):
    """``once(Buffers) -> name -> device tensor``, run twice on fresh guarded buffers; -> the first run's CPU results"""
    first = None
    for _ in range(2):
        b = Buffers()
        got = once(b)
        if b.dev.type == "cuda":
            torch.cuda.synchronize()
        b.check(where)
        got = {n: t.detach().cpu() for n, t in got.items()}
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(first[n].view(torch.uint8), got[n].view(torch.uint8)), f"{where} {n}: differs run to run"
    return first


judge = functools.partial(_judge, "mbconv_calls")


# -------------------------------------------------------------------------------------------- geometry, restated
def geo(rows):
    """(P, rpp, depth) of the channel sums over ``rows`` rows (csrc/mbconv.hip nparts_for / sums_kernel / lanes_sum)"""
    P = max(1, min(64, rows // 512))
    rpp = -(-rows // P)
    return P, rpp, -(-rpp // 64) + 14


def part_sums(t, P, rpp):
    """[B, rows, C] float64 -> [B, P, C]: sums over runs of rpp rows (the last one short)"""
    return torch.stack([t[:, p * rpp:(p + 1) * rpp].sum(1) for p in range(P)], 1)


# ---------------------------------------------------------------------------------------- float64 formulas, bounds
def pre_of(o):
    a = o["gamma"] * o["rstd"]
    t = a * (o["y"] - o["mean"])
    pre = t + o["beta"]
    return pre, U24 * (3 * t.abs() + pre.abs())


def silu_of(x, e_x):
    s = x * torch.sigmoid(x)
    return s, 1.1 * e_x + 5 * U24 * s.abs()


def silu_grad_of(x, e_x):
    sg = torch.sigmoid(x)
    d = sg * (1 + x * (1 - sg))
    return d, 0.5 * e_x + U24 * (5 * sg * x.abs() + 6 * d.abs())


def xhat_of(o):
    xh = (o["y"] - o["mean"]) * o["rstd"]
    return xh, 2 * U24 * xh.abs()


# ------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(shape, mode):
    """everything a block's BatchNorm + SiLU and SE calls read, float64 holding values of the dtype the kernels see, and
    the float64 chain (each stage's f32 rounding feeds the next call's test)"""
    B, H, W, C = shape
    HW, rd = H * W, RD[C]
    dt = DT[mode]
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + C + len(mode))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    o = {}
    o["y"] = (rnd(B, HW, C) * 1.5 + rnd(C) * 0.5).to(dt).double()
    yb = o["y"].reshape(-1, C)
    o["mean"] = f32(yb.mean(0))
    o["rstd"] = f32((yb.var(0, unbiased=False) + 1e-5).rsqrt()) if B * HW > 1 else f32(torch.rand(C, generator=g, dtype=F64) + 0.5)
    o["gamma"] = f32((torch.rand(C, generator=g, dtype=F64) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0))
    o["beta"] = f32(rnd(C) * 0.4)
    o["w1"], o["b1"] = f32(rnd(rd, C) * (2.0 / rd) ** 0.5), f32(rnd(rd) * 0.1)
    o["w2"], o["b2"] = f32(rnd(C, rd) * (2.0 / C) ** 0.5 * 4), f32(rnd(C) * 0.5)
    o["res"] = rnd(B, HW, C).to(dt).double()
    o["dout"] = (torch.rand(B, HW, C, generator=g, dtype=F64) * 2 - 1).to(dt).double()
    P, rpp, _ = geo(HW)
    pre, e_pre = pre_of(o)
    s, _ = silu_of(pre, e_pre)
    o["part"] = f32(part_sums(s, P, rpp))
    o["pooled"] = f32(o["part"].sum(1) / HW)
    o["hpre"] = f32(o["pooled"] @ o["w1"].t() + o["b1"])
    o["hidden"] = f32(o["hpre"] * torch.sigmoid(o["hpre"]))
    o["gate"] = f32(torch.sigmoid(o["hidden"] @ o["w2"].t() + o["b2"]))
    o["bpart"] = f32(part_sums(o["dout"] * s, P, rpp))
    ds = o["bpart"].sum(1) * o["gate"] * (1 - o["gate"])
    dh = (ds @ o["w2"]) * silu_grad_of(o["hpre"], 0)[0]
    o["dpool"] = f32(dh @ o["w1"])
    return o


def bn_put(b, o):
    return tuple(b.put(k, o[k]) for k in ("mean", "rstd", "gamma", "beta"))


# ---------------------------------------------------------------------------------------------- depthwise 3 x 3
@functools.lru_cache(maxsize=None)
def dw_operands(shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    g = torch.Generator().manual_seed(7 * B + 100 * H + 10 * W + C + stride + len(mode))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, C, H, W, generator=g, dtype=F64).to(dt).double()
    w = f32(torch.randn(C, 1, 3, 3, generator=g, dtype=F64) / 3)
    dy = (torch.rand(B, C, OH, OW, generator=g, dtype=F64) * 2 - 1).to(dt).double()
    prior = f32(torch.randn(C, 1, 3, 3, generator=g, dtype=F64))
    return x, w, dy, prior, OH, OW


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@gpu
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", DW_CASES, ids=DW_IDS)
def test_dwconv3_fwd(dev, shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    x, w, _, _, OH, OW = dw_operands(shape, mode, stride)

    def once(b):
        y = K.dwconv3_fwd(b.put("x", nhwc(x), dt), b.put("w", w), stride, out_dtype=dt, out=b.out("y", (B, OH, OW, C), dt))
        return dict(y=y)

    got = twice(f"dwconv3_fwd {shape} s{stride} {mode}", once)
    ref = nhwc(F.conv2d(x, w, stride=stride, padding=1, groups=C))
    S = nhwc(F.conv2d(x.abs(), w.abs(), stride=stride, padding=1, groups=C))
    judge(f"dwconv3_fwd {shape} s{stride} {mode}", got, dict(y=(ref, 9 * U24 * S + store(ref, dt))))


@gpu
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", DW_CASES, ids=DW_IDS)
def test_dwconv3_bwd_data(dev, shape, mode, stride):
    B, H, W, C = shape
    dt = DT[mode]
    _, w, dy, _, OH, OW = dw_operands(shape, mode, stride)

    def once(b):
        dx = K.dwconv3_bwd_data(b.put("dy", nhwc(dy), dt), b.put("w", w), H, W, stride, dx_dtype=dt,
                                out=b.out("dx", (B, H, W, C), dt))
        return dict(dx=dx)

    got = twice(f"dwconv3_bwd_data {shape} s{stride} {mode}", once)
    ref = nhwc(torch.nn.grad.conv2d_input((B, C, H, W), w, dy, stride=stride, padding=1, groups=C))
    S = nhwc(torch.nn.grad.conv2d_input((B, C, H, W), w.abs(), dy.abs(), stride=stride, padding=1, groups=C))
    judge(f"dwconv3_bwd_data {shape} s{stride} {mode}", got, dict(dx=(ref, 9 * U24 * S + store(ref, dt))))


@gpu
@pytest.mark.parametrize("accumulate", (True, False), ids=("acc", "store"))
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape,mode", DW_CASES, ids=DW_IDS)
def test_dwconv3_bwd_weight(dev, shape, mode, stride, accumulate):
    B, H, W, C = shape
    dt = DT[mode]
    x, _, dy, prior, OH, OW = dw_operands(shape, mode, stride)
    P, rpp, depth = geo(B * OH * OW)
    assert P == nv.value("sv_dwconv3_bwd_weight_nparts", B, H, W, C, stride)

    def once(b):
        dw = b.put("dw", prior) if accumulate else b.out("dw", (C, 1, 3, 3))
        K.dwconv3_bwd_weight(b.put("dy", nhwc(dy), dt), b.put("x", nhwc(x), dt), stride, dw=dw, accumulate=accumulate)
        return dict(dw=dw)

    got = twice(f"dwconv3_bwd_weight {shape} s{stride} {mode}", once)
    term = torch.nn.grad.conv2d_weight(x, (C, 1, 3, 3), dy, stride=stride, padding=1, groups=C)
    S = torch.nn.grad.conv2d_weight(x.abs(), (C, 1, 3, 3), dy.abs(), stride=stride, padding=1, groups=C)
    bound = (depth + P) * U24 * S
    ref = term
    if accumulate:
        ref = prior + term
        bound = bound + U24 * (prior.abs() + ref.abs())
    judge(f"dwconv3_bwd_weight {shape} s{stride} {mode} P{P} depth{depth}", got, dict(dw=(ref, bound)))


# --------------------------------------------------------------------------------------------- BatchNorm + SiLU
@gpu
def test_nparts_matches_library():
    for rows in (1, 4, 35, 511, 512, 1023, 1024, 4096, 32768, 524288):
        for C in (32, 96, 960, 3840):
            assert geo(rows)[0] == nv.value("sv_mbconv_nparts", rows, C), (rows, C)
    assert nv.value("sv_mbconv_nparts", 64, 24) == 0 and nv.value("sv_mbconv_nparts", 64, 3872) == 0


@gpu
def test_unsupported_shapes_are_refused(dev):
    y = torch.zeros(4, 2, 2, 24, device=dev)
    with pytest.raises(ValueError):
        K.dwconv3_fwd(y, torch.zeros(24, 1, 3, 3, device=dev), 1)
    y = torch.zeros(8, 40, device=dev)
    v = torch.zeros(40, device=dev)
    with pytest.raises(RuntimeError, match="status 2"):  # SV_ERR_UNSUPPORTED from the library itself, before any launch
        nv.call("sv_bn_silu_fwd", y.data_ptr(), nv.SV_F32, *(v.data_ptr(),) * 4, None, nv.SV_F32, y.data_ptr(), nv.SV_F32,
                8, 40)
    with pytest.raises(RuntimeError, match="status 2"):
        nv.call("sv_dwconv3_fwd", y.data_ptr(), nv.SV_F32, v.data_ptr(), y.data_ptr(), nv.SV_F32, 1, 2, 2, 64, 3)


@gpu
@pytest.mark.parametrize("shape,mode", STAT_CASES, ids=STAT_IDS)
def test_bn_stats(dev, shape, mode):
    """mb_bn_stats: csrc/mbconv.hip's unshifted (sum, sum of squares) partials through the existing sv_bn_stats_finish"""
    B, H, W, C = shape
    rows = B * H * W
    o = operands(shape, mode)
    P, rpp, depth = geo(rows)

    def once(b):
        rm, rv = b.put("rm", torch.zeros(C)), b.put("rv", torch.ones(C))
        mean, rstd = K.mb_bn_stats(b.put("y", o["y"].view(rows, C), DT[mode]), running_mean=rm, running_var=rv)
        return dict(mean=mean, rstd=rstd, rm=rm, rv=rv)

    got = twice(f"mb_bn_stats {shape} {mode}", once)
    y = o["y"].view(rows, C)
    m, ms = y.mean(0), (y * y).mean(0)
    var = ms - m * m
    e_m = (depth + P) * U24 * y.abs().mean(0) + 2 * U24 * m.abs()
    e_var = (depth + P + 1) * U24 * ms + 2 * m.abs() * e_m + 4 * U24 * (ms + m * m)
    rstd = (var + 1e-5).rsqrt()
    e_r = 0.5 * rstd ** 3 * e_var + 4 * U24 * rstd
    unb = var * rows / (rows - 1)
    judge(f"mb_bn_stats {shape} {mode} P{P} depth{depth}", got,
          dict(mean=(m, e_m), rstd=(rstd, e_r), rm=(0.1 * m, 0.1 * e_m + 3 * U24 * m.abs()),
               rv=(0.9 + 0.1 * unb, 0.1 * e_var * rows / (rows - 1) + 4 * U24 * (0.9 + 0.1 * unb))))


@gpu
@pytest.mark.parametrize("with_res", (False, True), ids=("plain", "res"))
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bn_silu_fwd(dev, shape, mode, with_res):
    """out = silu(bn(y)) (+ res AFTER the activation: the ConvBnAct block)"""
    B, H, W, C = shape
    rows, dt = B * H * W, DT[mode]
    o = operands(shape, mode)

    def once(b):
        res = b.put("res", o["res"].view(rows, C), dt) if with_res else None
        out = K.bn_silu_fwd(b.put("y", o["y"].view(rows, C), dt), bn_put(b, o), res=res, out_dtype=dt,
                            out=b.out("out", (rows, C), dt))
        return dict(out=out)

    got = twice(f"bn_silu_fwd {shape} {mode} res={with_res}", once)
    s, e_s = silu_of(*pre_of(o))
    ref, bound = s, e_s
    if with_res:
        ref = s + o["res"]
        bound = e_s + U24 * ref.abs()
    judge(f"bn_silu_fwd {shape} {mode} res={with_res}", got, dict(out=(ref, bound + store(ref, dt))))


def silu_bwd_terms(o):
    """g = dout silu'(pre), g xhat and their per-element error bounds"""
    sg, e_sg = silu_grad_of(*pre_of(o))
    xh, e_xh = xhat_of(o)
    g = o["dout"] * sg
    e_g = o["dout"].abs() * e_sg + U24 * g.abs()
    gx = g * xh
    return g, e_g, gx, e_g * xh.abs() + g.abs() * e_xh, xh, e_xh


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bn_silu_bwd_stats(dev, shape, mode):
    B, H, W, C = shape
    rows, dt = B * H * W, DT[mode]
    o = operands(shape, mode)
    P, rpp, depth = geo(rows)

    def once(b):
        part = K.bn_silu_bwd_stats(b.put("dout", o["dout"].view(rows, C), dt), b.put("y", o["y"].view(rows, C), dt), bn_put(b, o))
        assert tuple(part.shape) == (P, 2, C)
        return dict(part=part)

    got = twice(f"bn_silu_bwd_stats {shape} {mode}", once)
    g, e_g, gx, e_gx, _, _ = silu_bwd_terms(o)
    flat = lambda t: part_sums(t.reshape(1, rows, C), P, rpp)[0]  # noqa: E731
    ref = torch.stack([flat(g), flat(gx)], 1)
    bound = torch.stack([depth * U24 * flat(g.abs()) + flat(e_g), (depth + 1) * U24 * flat(gx.abs()) + flat(e_gx)], 1)
    judge(f"bn_silu_bwd_stats {shape} {mode} P{P} depth{depth}", got, dict(part=(ref, bound)))


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bn_silu_bwd_apply(dev, shape, mode):
    B, H, W, C = shape
    rows, dt = B * H * W, DT[mode]
    o = operands(shape, mode)
    g, e_g, gx, _, xh, e_xh = silu_bwd_terms(o)
    sums = f32(torch.stack([g.sum((0, 1)), gx.sum((0, 1))]))

    def once(b):
        dx = K.bn_silu_bwd_apply(b.put("dout", o["dout"].view(rows, C), dt), b.put("y", o["y"].view(rows, C), dt),
                                 bn_put(b, o), b.put("sums", sums), dx_dtype=dt, out=b.out("dx", (rows, C), dt))
        return dict(dx=dx)

    got = twice(f"bn_silu_bwd_apply {shape} {mode}", once)
    a = o["gamma"] * o["rstd"]
    c0, xs = sums[0] / rows, xh * sums[1]
    a1 = g - c0
    inner = a1 - xs / rows
    ref = a * inner
    e_a1 = e_g + U24 * (c0.abs() + a1.abs())                       # 1 / n rounded; the fmaf
    e_xs = e_xh * sums[1].abs() + U24 * xs.abs()
    e_in = e_a1 + (e_xs + U24 * xs.abs()) / rows + U24 * inner.abs()
    bound = a.abs() * e_in + 2 * U24 * ref.abs() + store(ref, dt)
    judge(f"bn_silu_bwd_apply {shape} {mode}", got, dict(dx=(ref.view(rows, C), bound.view(rows, C))))


@gpu
def test_add(dev):
    g = torch.Generator().manual_seed(5)
    for dt in (BF, F32):
        a, c = (torch.randn(3, 5, 7, 96, generator=g, dtype=F64).to(dt).double() for _ in range(2))

        def once(b):
            dst = b.put("dst", a, dt)
            K.mb_add(dst, b.put("src", c, dt))
            return dict(dst=dst)

        got = twice(f"mb_add {dt}", once)
        ref = a + c
        judge(f"mb_add {dt}", got, dict(dst=(ref, U24 * ref.abs() + store(ref, dt))))


# ------------------------------------------------------------------------------------- squeeze-and-excitation
@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_squeeze(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    P, rpp, depth = geo(H * W)

    def once(b):
        y = b.put("y", o["y"].view(B, H, W, C), DT[mode])
        part = K.mbse_squeeze(y, bn_put(b, o))
        assert tuple(part.shape) == (B, P, C)
        return dict(part=part, y=y)

    got = twice(f"mbse_squeeze {shape} {mode}", once)
    assert torch.equal(got["y"].double().view(B, H * W, C), o["y"]), "input changed"
    s, e_s = silu_of(*pre_of(o))
    judge(f"mbse_squeeze {shape} {mode} P{P} rpp{rpp} depth{depth}", got,
          dict(part=(part_sums(s, P, rpp), depth * U24 * part_sums(s.abs(), P, rpp) + part_sums(e_s, P, rpp))))


def excite_refs(o, HW):
    part, w1, b1, w2, b2 = (o[k] for k in ("part", "w1", "b1", "w2", "b2"))
    P, C, rd = part.shape[1], part.shape[2], w1.shape[0]
    pooled = part.sum(1) / HW
    e_m = (P - 1) * U24 * part.abs().sum(1) / HW + 3 * U24 * pooled.abs()  # the fold; 1 / HW rounded; the product
    v1 = pooled @ w1.t() + b1
    e_v1 = e_m @ w1.abs().t() + mv_depth(C) * U24 * (pooled.abs() @ w1.abs().t() + b1.abs())
    hidden, e_h = silu_of(v1, e_v1)
    v2 = hidden @ w2.t() + b2
    e_v2 = e_h @ w2.abs().t() + mv_depth(rd) * U24 * (hidden.abs() @ w2.abs().t() + b2.abs())
    gate = torch.sigmoid(v2)
    return dict(pooled=(pooled, e_m), hpre=(v1, e_v1), hidden=(hidden, e_h), gate=(gate, 0.25 * e_v2 + 4 * U24 * gate))


def excite_call(b, o, C, HW):
    rd = RD[C]
    w1, w2 = b.put("w1", o["w1"].view(rd, C, 1, 1)), b.put("w2", o["w2"].view(C, rd, 1, 1))
    return K.mbse_excite(b.put("part", o["part"]), HW, w1, b.put("b1", o["b1"]), w2, b.put("b2", o["b2"]))


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_excite(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    got = twice(f"mbse_excite {shape} {mode}",
                lambda b: dict(zip(("pooled", "hpre", "hidden", "gate"), excite_call(b, o, C, H * W))))
    judge(f"mbse_excite {shape} {mode}", got, excite_refs(o, H * W))


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_scale(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    dt = DT[mode]

    def once(b):
        out = K.mbse_scale(b.put("y", o["y"].view(B, H, W, C), dt), bn_put(b, o), b.put("gate", o["gate"]), out_dtype=dt,
                           out=b.out("out", (B, H, W, C), dt))
        return dict(out=out)

    got = twice(f"mbse_scale {shape} {mode}", once)
    s, e_s = silu_of(*pre_of(o))
    gate = o["gate"][:, None]
    ref = s * gate
    judge(f"mbse_scale {shape} {mode}", got, dict(out=(ref, gate * e_s + U24 * ref.abs() + store(ref, dt))))


@gpu
def test_batch_independence(dev):
    """changing image 1 leaves image 0's gate and scaled activation bit-equal (mean / rstd given)"""
    shape, mode = SE_SHAPES[0], "bf16"
    B, H, W, C = shape
    o = operands(shape, mode)
    rd = RD[C]

    def run(y):
        d = lambda k: o[k].float().to(dev)  # noqa: E731
        y = y.reshape(B, H, W, C).to(dev, BF).contiguous()
        bn = (d("mean"), d("rstd"), d("gamma"), d("beta"))
        st = K.mbse_excite(K.mbse_squeeze(y, bn), H * W, d("w1").view(rd, C, 1, 1).contiguous(), d("b1"),
                           d("w2").view(C, rd, 1, 1).contiguous(), d("b2"))
        out = K.mbse_scale(y, bn, st[3], out_dtype=BF)
        torch.cuda.synchronize()
        return st[3].cpu(), out.cpu()

    g_a, o_a = run(o["y"])
    y2 = o["y"].clone()
    y2[1] = -2 * y2[1] + 0.5
    g_b, o_b = run(y2)
    assert torch.equal(g_a[0], g_b[0]) and torch.equal(o_a[0], o_b[0])
    assert not torch.equal(g_a[1], g_b[1])


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bwd_stats(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    dt = DT[mode]
    P, rpp, depth = geo(H * W)

    def once(b):
        part = K.mbse_bwd_stats(b.put("da", o["dout"].view(B, H, W, C), dt), b.put("y", o["y"].view(B, H, W, C), dt), bn_put(b, o))
        assert tuple(part.shape) == (B, P, C)
        return dict(part=part)

    got = twice(f"mbse_bwd_stats {shape} {mode}", once)
    s, e_s = silu_of(*pre_of(o))
    t = o["dout"] * s
    judge(f"mbse_bwd_stats {shape} {mode} depth{depth}", got,
          dict(part=(part_sums(t, P, rpp), (depth + 1) * U24 * part_sums(t.abs(), P, rpp) + part_sums(o["dout"].abs() * e_s, P, rpp))))


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bwd_gate(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    rd = RD[C]
    g = torch.Generator().manual_seed(C + B)
    priors = {n: f32(torch.randn(*s, generator=g, dtype=F64)) for n, s in
              (("dw1", (rd, C)), ("db1", (rd,)), ("dw2", (C, rd)), ("db2", (C,)))}

    def once(b):
        acc = {n: b.put(n, t.view(*t.shape, 1, 1) if t.dim() == 2 else t) for n, t in priors.items()}
        state = tuple(b.put(k, o[k]) for k in ("pooled", "hpre", "hidden", "gate"))
        dpool = K.mbse_bwd_gate(b.put("part", o["bpart"]), state, b.put("w1", o["w1"].view(rd, C, 1, 1)),
                                b.put("w2", o["w2"].view(C, rd, 1, 1)), **acc)
        return dict(dpool=dpool, **acc)

    got = twice(f"mbse_bwd_gate {shape} {mode}", once)
    part, pooled, hpre, hidden, gate, w1, w2 = (o[k] for k in ("bpart", "pooled", "hpre", "hidden", "gate", "w1", "w2"))
    P = part.shape[1]
    dgate = part.sum(1)
    e_dg = (P - 1) * U24 * part.abs().sum(1)
    sp = gate * (1 - gate)
    ds = dgate * sp
    e_ds = e_dg * sp + 3 * U24 * ds.abs()
    dh0 = ds @ w2
    e_dh0 = e_ds @ w2.abs() + tm_depth(C) * U24 * (ds.abs() @ w2.abs())
    sg, e_sg = silu_grad_of(hpre, torch.zeros_like(hpre))
    dh = dh0 * sg
    e_dh = e_dh0 * sg.abs() + dh0.abs() * e_sg + U24 * dh.abs()
    dpool = dh @ w1
    e_dp = e_dh @ w1.abs() + tm_depth(rd) * U24 * (dh.abs() @ w1.abs())

    def acc(name, term, e_term, tabs):
        ref = priors[name] + term
        return ref, e_term + (B + 1) * U24 * tabs + U24 * (priors[name].abs() + ref.abs())

    refs = dict(dpool=(dpool, e_dp))
    refs["dw2"] = acc("dw2", ds.t() @ hidden, e_ds.t() @ hidden.abs(), ds.abs().t() @ hidden.abs())
    refs["db2"] = acc("db2", ds.sum(0), e_ds.sum(0), ds.abs().sum(0))
    refs["dw1"] = acc("dw1", dh.t() @ pooled, e_dh.t() @ pooled.abs(), dh.abs().t() @ pooled.abs())
    refs["db1"] = acc("db1", dh.sum(0), e_dh.sum(0), dh.abs().sum(0))
    judge(f"mbse_bwd_gate {shape} {mode}", got, refs)


@gpu
@pytest.mark.parametrize("shape,mode", SE_CASES, ids=SE_IDS)
def test_bwd_apply(dev, shape, mode):
    """dpre = (da gate + dpool / HW) silu'(pre) per element, and the BatchNorm backward partials: the sums of the STORED
    dpre (the reference sums the call's own stored tensor in float64: that consistency is what the apply pass needs)"""
    B, H, W, C = shape
    HW, dt = H * W, DT[mode]
    o = operands(shape, mode)
    P, rpp, depth = geo(HW)

    def once(b):
        dpre, part = K.mbse_bwd_apply(b.put("da", o["dout"].view(B, H, W, C), dt), b.put("y", o["y"].view(B, H, W, C), dt),
                                      bn_put(b, o), b.put("gate", o["gate"]), b.put("dpool", o["dpool"]), out_dtype=dt)
        assert tuple(part.shape) == (B * P, 2, C)
        return dict(dpre=dpre, part=part)

    got = twice(f"mbse_bwd_apply {shape} {mode}", once)
    sg, e_sg = silu_grad_of(*pre_of(o))
    xh, e_xh = xhat_of(o)
    gate, dp = o["gate"][:, None], o["dpool"][:, None] / HW
    v = o["dout"] * gate + dp
    dpre = v * sg
    e = v.abs() * e_sg + U24 * (2 * dp.abs() + v.abs()) * sg.abs() + U24 * dpre.abs() + store(dpre, dt)
    r = got["dpre"].double().view(B, HW, C)
    rx = r * xh
    ref = torch.stack([part_sums(r, P, rpp), part_sums(rx, P, rpp)], 2).view(B * P, 2, C)
    bound = torch.stack([depth * U24 * part_sums(r.abs(), P, rpp),
                         (depth + 1) * U24 * part_sums(rx.abs(), P, rpp) + part_sums(r.abs() * e_xh, P, rpp)], 2).view(B * P, 2, C)
    judge(f"mbse_bwd_apply {shape} {mode} depth{depth}", got, dict(dpre=(dpre, e), part=(ref, bound)))


# ------------------------------------------------------------------------------ dense 3 x 3, padded channel strides
@gpu
def test_padded_dense_conv(dev):
    """EdgeResidual's conv_exp 24 -> 96 at stride 2 on a 7 x 9 grid through the padded-stride scheme (stored strides 32 and
    128, zero weight rows / columns): forward, data gradient and weight gradient against float64, the padded channels
    exactly zero and the weight gradient delivered in the parameter's own shape."""
    from spine_vision_amd.backbone.efficientnet import EfficientNetV2Hip

    B, H, W, Cin, Cout, Cs, Cos = 2, 7, 9, 24, 96, 32, 128
    model = EfficientNetV2Hip(24, (("er", 1, 2, 4, 48),), precision="bf16").to(dev).train()
    conv = model.blocks[0][0].conv_exp
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=F64).to(BF).double()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64) / (9 * Cin) ** 0.5).to(BF).double()
    OH, OW = 4, 5
    dy = (torch.rand(B, Cout, OH, OW, generator=g, dtype=F64) * 2 - 1).to(BF).double()
    with torch.no_grad():
        conv.weight.copy_(w.float())
    xp = torch.zeros(B, H, W, Cs, dtype=F64)
    xp[..., :Cin] = nhwc(x)
    dyp = torch.zeros(B, OH, OW, Cos, dtype=F64)
    dyp[..., :Cout] = nhwc(dy)

    def once(b):
        xd, dyd = b.put("x", xp, BF), b.put("dy", dyp, BF)
        y, wp, s, part = model._conv3(xd, conv, Cos)
        dx = K.conv_bwd_data(dyd, wp, s, dx_dtype=BF)
        conv.weight.grad = None
        model._conv_wgrad(conv, dyd, xd, s)(None)
        return dict(y=y, dx=dx, dw=conv.weight.grad)

    got = twice("padded dense conv 24->96 s2 7x9", once)
    assert tuple(got["y"].shape) == (B, OH, OW, Cos) and tuple(got["dx"].shape) == (B, H, W, Cs)
    assert tuple(got["dw"].shape) == (Cout, Cin, 3, 3)
    assert not got["y"][..., Cout:].any() and not got["dx"][..., Cin:].any(), "padded channels must be exactly zero"
    n = 9 * Cs
    y_ref = nhwc(F.conv2d(x, w, stride=2, padding=1))
    y_S = nhwc(F.conv2d(x.abs(), w.abs(), stride=2, padding=1))
    dx_ref = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w, dy, stride=2, padding=1))
    dx_S = nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w.abs(), dy.abs(), stride=2, padding=1))
    dw_ref = torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, stride=2, padding=1)
    dw_S = torch.nn.grad.conv2d_weight(x.abs(), (Cout, Cin, 3, 3), dy.abs(), stride=2, padding=1)
    real = dict(y=got["y"][..., :Cout], dx=got["dx"][..., :Cin], dw=got["dw"])
    judge("padded dense conv 24->96 s2 7x9", real,
          dict(y=(y_ref, acc_bound(y_S, n) + store(y_ref, BF)), dx=(dx_ref, acc_bound(dx_S, 9 * Cos) + store(dx_ref, BF)),
               dw=(dw_ref, acc_bound(dw_S, B * OH * OW + 64, split=1) + 2 * U24 * dw_ref.abs())))
