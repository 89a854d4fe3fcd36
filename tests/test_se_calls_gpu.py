"""Every squeeze-and-excitation and avg-pool-shortcut call of a ResNet-RS step (csrc/se.hip), one call at a time through
its ``spine_vision_amd.kernels`` wrapper, each output compared ELEMENT BY ELEMENT with a float64 CPU evaluation of the
same operation on the same rounded operands; and the deep stem's first convolution (3 -> 32, 3x3 stride 2) on the
8-channel gathered path of csrc/conv.hip.

Calls                                                       -> test here
    se_squeeze(y)                                            -> test_squeeze
    se_excite(part, HW, mean, rstd, gamma, beta, w1..b2)     -> test_excite, test_batch_independence
    se_join(y, ..., gate, res, res_bn=)                      -> test_join, test_batch_independence
    se_bwd_stats(dout, act, y, mean, rstd)                   -> test_bwd_stats
    se_bwd_gate(part, state, ...)                            -> test_bwd_gate
    se_bwd_apply(g, y, ..., gate, dpool, sums)               -> test_bwd_apply
    avgpool2x2_fwd / avgpool2x2_bwd                          -> test_avgpool2x2
    conv_fwd / conv_fwd_bn_stats / conv_bwd_weight, Cs = 8, k = 3; conv_bwd_data of the stem's 32 -> 32 3x3
                                                             -> test_deep_stem_conv

Inputs.  Each call is judged alone: its inputs are the f32 (or bf16) roundings of the float64 results of the calls
before it, not those calls' outputs.  The join and the three backward calls run with both shortcut forms (identity and
BN'd: the backward's mask is that form's stored output).  ReLU ties need no mask: the backward takes its mask from the ``act`` input, which
the reference shares.

Bounds, derived from the summation orders and rounding points documented at the top of csrc/se.hip and csrc/se_core.h
and asserted at 2 x for EVERY element (u = 2^-24):
    per-image sums   depth u sum |t|, depth = ceil(rpp / rp) + (rp - 1) (a thread's serial rows, then the rp row groups);
                     the consumer's fold of P parts adds (P - 1) u sum |part|
    matvec           depth u sum |w x|, depth = 4 ceil(K / 256) + 6 + 1 (the lane's fmaf chain, the 64-lane butterfly,
                     the bias), plus sum |w| E_x for an input that carries error E_x
    transposed       depth = ceil(K / 16) + 15
    sigmoid          slope <= 1/4 on the argument's bound, plus 4 u gate (expf within 1 ulp = 2 u, one add, one
                     correctly rounded division)
    elementwise      one u |value| per rounded operation, written out per formula below
    stores           2^-8 |ref| for a bf16 store
Guards: outputs start as NaN (accumulating ones as a known prior); every buffer sits between sentinels; every call runs
twice with bit-equal results.  The figures of a GPU run are recorded in profiles/resnetrs/parity.txt."""
import functools

import pytest
import torch

import _conv_ref as CR
from _calls_harness import f32, judge as _judge, mv_depth, store, tm_depth
from _conv_ref import BF, F32, F64, U8, U24
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
SENTINEL, GUARD, NAN = -7.0, 256, float("nan")
DT = {"bf16": BF, "fp32": F32}

# (B, H, W, C), rd = C / 4
SHAPES = [(3, 5, 7, 256),    # odd spatial size, HW below a wave
          (2, 1, 1, 2048),   # HW = 1, widest C, rd = 512
          (2, 2, 2, 2048),   # layer4 at the test model's size
          (1, 64, 64, 256),  # long per-image reduction, several workgroups per image
          (5, 9, 9, 512)]    # B not a power of two
BOTH = (SHAPES[0], SHAPES[3])
CASES = [(s, m) for s in SHAPES for m in ("bf16", "fp32") if m == "bf16" or s in BOTH]
IDS = ["x".join(map(str, s)) + "-" + m for s, m in CASES]
FORMS = ("identity", "bn")  # the block's shortcut: its input, or BN(conv_ds(.))


# ------------------------------------------------------------------------------------------------------ harness
class Buffers:
    """device buffers between sentinels"""

    def __init__(self):
        self.dev, self.bufs = torch.device("cuda:0"), {}

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
        torch.cuda.synchronize()
        b.check(where)
        got = {n: t.detach().cpu() for n, t in got.items()}
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(first[n].view(torch.uint8), got[n].view(torch.uint8)), f"{where} {n}: differs run to run"
    return first


judge = functools.partial(_judge, "se_calls")


# -------------------------------------------------------------------------------------------- geometry, restated
def geo(HW, C):
    """(P, rpp, rp, depth) of the per-image sums (csrc/se.hip nparts_for / sums_kernel)"""
    rp = 256 // (C // 8)
    P = max(1, min(32, HW // (8 * rp)))
    rpp = -(-HW // P)
    return P, rpp, rp, -(-rpp // rp) + rp - 1


def part_sums(t, P, rpp):
    """[B, HW, C] float64 -> [B, P, C]: sums over runs of rpp rows (the last one short)"""
    return torch.stack([t[:, p * rpp:(p + 1) * rpp].sum(1) for p in range(P)], 1)


# ------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(shape, mode):
    """everything a block's SE forward and backward read, float64 holding values of the dtype the kernels see; the
    float64 forward and backward of the whole chain (each stage's f32 rounding feeds the next call's test)"""
    B, H, W, C = shape
    HW, rd = H * W, C // 4
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
    o["res"] = (rnd(B, HW, C)).to(dt).double()
    o["rbn"] = tuple(f32(t) for t in (rnd(C) * 0.3, torch.rand(C, generator=g, dtype=F64) + 0.5, rnd(C), rnd(C) * 0.4))
    o["dout"] = (torch.rand(B, HW, C, generator=g, dtype=F64) * 2 - 1).to(dt).double()
    # forward chain in float64, each stage from the f32 rounding of the one before
    P, rpp, _, _ = geo(HW, C)
    o["part"] = f32(part_sums(o["y"], P, rpp))
    a = o["gamma"] * o["rstd"]
    o["ymean"] = f32(o["part"].sum(1) / HW)
    o["pooled"] = f32(a * (o["ymean"] - o["mean"]) + o["beta"])
    o["hidden"] = f32(torch.relu(o["pooled"] @ o["w1"].t() + o["b1"]))
    o["gate"] = f32(torch.sigmoid(o["hidden"] @ o["w2"].t() + o["b2"]))
    for form in FORMS:
        r = o["res"]
        if form == "bn":
            m2, r2, g2, b2 = o["rbn"]
            r = g2 * r2 * (r - m2) + b2
        z = a * (o["y"] - o["mean"]) + o["beta"]
        o["out_" + form] = torch.relu(z * o["gate"][:, None] + r)
    xh = (o["y"] - o["mean"]) * o["rstd"]
    for form in FORMS:  # the backward of both shortcut forms: the mask is the stored output of that form's join
        o["act_" + form] = o["out_" + form].to(dt).double()
        gm = o["dout"] * (o["act_" + form] > 0)
        o["gm_" + form] = gm  # exact in the gradient dtype
        o["bpart_" + form] = f32(torch.stack([part_sums(gm, P, rpp), part_sums(gm * xh, P, rpp)], 2))  # [B][P][2][C]
    return o


# ------------------------------------------------------------------------------------------------------- forward
@gpu
def test_nparts_matches_library():
    for HW in (1, 4, 35, 49, 63, 64, 81, 256, 1024, 4096, 12544):
        for C in (16, 64, 256, 512, 1024, 2048):
            assert geo(HW, C)[0] == nv.value("sv_se_nparts", HW, C), (HW, C)


@gpu
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_squeeze(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    P, rpp, _, depth = geo(H * W, C)

    def once(b):
        y = b.put("y", o["y"].view(B, H, W, C), DT[mode])
        part = K.se_squeeze(y, part=b.out("part", (B, P, C)))
        return dict(part=part, y=y)

    got = twice(f"se_squeeze {shape} {mode}", once)
    assert torch.equal(got["y"].double().view(B, H * W, C), o["y"]), "input changed"
    ref, S = part_sums(o["y"], P, rpp), part_sums(o["y"].abs(), P, rpp)
    judge(f"se_squeeze {shape} {mode} P{P} rpp{rpp} depth{depth}", got, dict(part=(ref, depth * U24 * S)))


def excite_refs(o, HW):
    """float64 references and bounds of se_excite's four outputs from its inputs (part, BN parameters, weights)"""
    part, mean, rstd, gamma, beta = (o[k] for k in ("part", "mean", "rstd", "gamma", "beta"))
    w1, b1, w2, b2 = (o[k] for k in ("w1", "b1", "w2", "b2"))
    P, C, rd = part.shape[1], part.shape[2], w1.shape[0]
    ymean = part.sum(1) / HW
    e_m = (P - 1) * U24 * part.abs().sum(1) / HW + 3 * U24 * ymean.abs()  # the fold; 1 / HW rounded; the product
    a = gamma * rstd
    pooled = a * (ymean - mean) + beta
    e_p = a.abs() * e_m + 2 * U24 * (a * (ymean - mean)).abs() + 2 * U24 * pooled.abs()
    v1 = pooled @ w1.t() + b1
    e_v1 = e_p @ w1.abs().t() + mv_depth(C) * U24 * (pooled.abs() @ w1.abs().t() + b1.abs())
    hidden = torch.relu(v1)
    v2 = hidden @ w2.t() + b2
    e_v2 = e_v1 @ w2.abs().t() + mv_depth(rd) * U24 * (hidden.abs() @ w2.abs().t() + b2.abs())
    gate = torch.sigmoid(v2)
    return dict(ymean=(ymean, e_m), pooled=(pooled, e_p), hidden=(hidden, e_v1), gate=(gate, 0.25 * e_v2 + 4 * U24 * gate))


@gpu
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_excite(dev, shape, mode):
    B, H, W, C = shape
    o = operands(shape, mode)
    names = ("ymean", "pooled", "hidden", "gate")

    def once(b):
        v = {k: b.put(k, o[k]) for k in ("part", "mean", "rstd", "gamma", "beta", "b1", "b2")}
        w1, w2 = b.put("w1", o["w1"].view(C // 4, C, 1, 1)), b.put("w2", o["w2"].view(C, C // 4, 1, 1))
        outs = tuple(b.out(n, (B, C // 4 if n == "hidden" else C)) for n in names)
        st = K.se_excite(v["part"], H * W, v["mean"], v["rstd"], v["gamma"], v["beta"], w1, v["b1"], w2, v["b2"], out=outs)
        assert all(a.data_ptr() == o_.data_ptr() for a, o_ in zip(st, outs))
        return dict(zip(names, st))

    got = twice(f"se_excite {shape} {mode}", once)
    judge(f"se_excite {shape} {mode}", got, excite_refs(o, H * W))


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_join(dev, shape, mode, form):
    B, H, W, C = shape
    o = operands(shape, mode)
    dt = DT[mode]

    def once(b):
        v = {k: b.put(k, o[k]) for k in ("mean", "rstd", "gamma", "beta", "gate")}
        y, res = b.put("y", o["y"].view(B, H, W, C), dt), b.put("res", o["res"].view(B, H, W, C), dt)
        rbn = tuple(b.put(f"rbn{i}", t) for i, t in enumerate(o["rbn"])) if form == "bn" else None
        out = K.se_join(y, v["mean"], v["rstd"], v["gamma"], v["beta"], v["gate"], res, res_bn=rbn, out_dtype=dt,
                        out=b.out("out", (B, H, W, C), dt))
        return dict(out=out)

    got = twice(f"se_join {shape} {mode} {form}", once)
    a = o["gamma"] * o["rstd"]
    t = a * (o["y"] - o["mean"])
    z = t + o["beta"]
    e_z = U24 * (3 * t.abs() + z.abs())  # gamma rstd, y - mean, the fmaf
    r, e_r = o["res"], torch.zeros_like(o["res"])
    if form == "bn":
        m2, r2, g2, b2 = o["rbn"]
        t2 = g2 * r2 * (r - m2)
        r = t2 + b2
        e_r = U24 * (3 * t2.abs() + r.abs())
    gate = o["gate"][:, None]
    pre = z * gate + r
    ref = torch.relu(pre)
    bound = gate * e_z + e_r + U24 * pre.abs() + store(ref, dt)
    judge(f"se_join {shape} {mode} {form}", got, dict(out=(ref, bound)))


@gpu
def test_batch_independence(dev):
    """an image's gate and output are bit-equal alone (B = 1) and inside a batch of three when mean / rstd are given"""
    shape, mode = SHAPES[0], "bf16"
    B, H, W, C = shape
    o = operands(shape, mode)

    def run(sel):
        d = lambda k: o[k].float().to(dev)  # noqa: E731
        y = o["y"][sel].reshape(-1, H, W, C).to(dev, BF).contiguous()
        res = o["res"][sel].reshape(-1, H, W, C).to(dev, BF).contiguous()
        part = K.se_squeeze(y)
        st = K.se_excite(part, H * W, d("mean"), d("rstd"), d("gamma"), d("beta"), d("w1").view(C // 4, C, 1, 1).contiguous(),
                         d("b1"), d("w2").view(C, C // 4, 1, 1).contiguous(), d("b2"))
        out = K.se_join(y, d("mean"), d("rstd"), d("gamma"), d("beta"), st[3], res, out_dtype=BF)
        torch.cuda.synchronize()
        return st[3].cpu(), out.cpu()

    g3, o3 = run(slice(0, 3))
    for i in range(3):
        g1, o1 = run(slice(i, i + 1))
        assert torch.equal(g1[0], g3[i]) and torch.equal(o1[0], o3[i]), i


# ------------------------------------------------------------------------------------------------------ backward
@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_bwd_stats(dev, shape, mode, form):
    B, H, W, C = shape
    o = operands(shape, mode)
    dt = DT[mode]
    P, rpp, _, depth = geo(H * W, C)

    def once(b):
        dout, act, y = (b.put(k, o[k].view(B, H, W, C), dt) for k in ("dout", "act_" + form, "y"))
        part = K.se_bwd_stats(dout, act, y, b.put("mean", o["mean"]), b.put("rstd", o["rstd"]),
                              part=b.out("part", (B, P, 2, C)))
        return dict(part=part, gm=dout)

    got = twice(f"se_bwd_stats {shape} {mode} {form}", once)
    assert torch.equal(got["gm"].double().view(B, H * W, C), o["gm_" + form]), "masked gradient is not dout * (act > 0) exactly"
    gm = o["gm_" + form]
    gx = gm * (o["y"] - o["mean"]) * o["rstd"]
    ref = torch.stack([part_sums(gm, P, rpp), part_sums(gx, P, rpp)], 2)
    bound = torch.stack([depth * U24 * part_sums(gm.abs(), P, rpp), (depth + 2) * U24 * part_sums(gx.abs(), P, rpp)], 2)
    judge(f"se_bwd_stats {shape} {mode} {form} depth{depth}", got, dict(part=(ref, bound)))


def gate_bwd_refs(o, HW, priors, form, batch_stats=True):
    """float64 references and bounds of se_bwd_gate from its inputs (the partials, the forward state, the weights)"""
    part, ymean, pooled, hidden, gate = (o[k] for k in ("bpart_" + form, "ymean", "pooled", "hidden", "gate"))
    mean, rstd, gamma, beta, w1, w2 = (o[k] for k in ("mean", "rstd", "gamma", "beta", "w1", "w2"))
    B, P, _, C = part.shape
    rd = w1.shape[0]
    s = part.sum(1)
    e_s = (P - 1) * U24 * part.abs().sum(1)
    s1, s2, e1, e2 = s[:, 0], s[:, 1], e_s[:, 0], e_s[:, 1]
    dgate = gamma * s2 + beta * s1
    e_dg = gamma.abs() * e2 + beta.abs() * e1 + U24 * ((beta * s1).abs() + dgate.abs())
    sp = gate * (1 - gate)
    ds = dgate * sp
    e_ds = e_dg * sp + 3 * U24 * ds.abs()
    mask = (hidden > 0).double()
    dh = (ds @ w2) * mask
    e_dh = (e_ds @ w2.abs() + tm_depth(C) * U24 * (ds.abs() @ w2.abs())) * mask
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
    xm = (ymean - mean) * rstd
    t0 = gate * s1 + dpool
    e_t0 = gate * e1 + e_dp + U24 * t0.abs()
    t1 = gate * s2 + dpool * xm
    e_t1 = gate * e2 + e_dp * xm.abs() + 3 * U24 * (dpool * xm).abs() + U24 * t1.abs()
    refs["dbeta"] = acc("dbeta", t0.sum(0), e_t0.sum(0), t0.abs().sum(0))
    refs["dgamma"] = acc("dgamma", t1.sum(0), e_t1.sum(0), t1.abs().sum(0))
    z = torch.zeros(2, C, dtype=F64)
    sums = torch.stack([t0.sum(0), t1.sum(0)])
    e_sums = torch.stack([e_t0.sum(0) + B * U24 * t0.abs().sum(0), e_t1.sum(0) + B * U24 * t1.abs().sum(0)])
    refs["sums"] = (sums, e_sums) if batch_stats else (z, z)
    return refs


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch_stats", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_bwd_gate(dev, shape, mode, batch_stats, form):
    B, H, W, C = shape
    rd = C // 4
    o = operands(shape, mode)
    g = torch.Generator().manual_seed(7)
    priors = {n: f32(torch.randn(*s, generator=g, dtype=F64) * 0.5) for n, s in
              dict(dw1=(rd, C), db1=(rd,), dw2=(C, rd), db2=(C,), dgamma=(C,), dbeta=(C,)).items()}

    def once(b):
        v = {k: b.put(k, o[k]) for k in ("ymean", "pooled", "hidden", "gate", "mean", "rstd", "gamma", "beta")}
        v["bpart"] = b.put("bpart", o["bpart_" + form])
        w1, w2 = b.put("w1", o["w1"].view(rd, C, 1, 1)), b.put("w2", o["w2"].view(C, rd, 1, 1))
        acc = {n: b.put(n, t) for n, t in priors.items()}
        dpool, sums = K.se_bwd_gate(v["bpart"], (v["ymean"], v["pooled"], v["hidden"], v["gate"]), H * W, v["mean"],
                                    v["rstd"], v["gamma"], v["beta"], w1, w2, dw1=acc["dw1"].view(rd, C, 1, 1),
                                    db1=acc["db1"], dw2=acc["dw2"].view(C, rd, 1, 1), db2=acc["db2"],
                                    dgamma=acc["dgamma"], dbeta=acc["dbeta"], batch_stats=batch_stats,
                                    out=(b.out("dpool", (B, C)), b.out("sums", (2, C))),
                                    work=b.out("work", (3 * B * C + B * rd,)))
        return dict(acc, dpool=dpool, sums=sums)

    got = twice(f"se_bwd_gate {shape} {mode} {form}", once)
    judge(f"se_bwd_gate {shape} {mode} {form} {'train' if batch_stats else 'eval'}", got,
          gate_bwd_refs(o, H * W, priors, form, batch_stats))


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_bwd_apply(dev, shape, mode, form):
    B, H, W, C = shape
    HW = H * W
    o = operands(shape, mode)
    dt = DT[mode]
    refs = gate_bwd_refs(o, HW, {n: torch.zeros(()) for n in ("dw1", "db1", "dw2", "db2", "dgamma", "dbeta")}, form)
    dpool, sums = f32(refs["dpool"][0]), f32(refs["sums"][0])

    def once(b):
        v = {k: b.put(k, o[k]) for k in ("mean", "rstd", "gamma", "gate")}
        gm, y = b.put("gm", o["gm_" + form].view(B, H, W, C), dt), b.put("y", o["y"].view(B, H, W, C), dt)
        dy = K.se_bwd_apply(gm, y, v["mean"], v["rstd"], v["gamma"], v["gate"], b.put("dpool", dpool), b.put("sums", sums),
                            dx_dtype=dt, out=b.out("dy", (B, H, W, C), dt))
        return dict(dy=dy)

    got = twice(f"se_bwd_apply {shape} {mode} {form}", once)
    n = B * HW
    dp = dpool[:, None] / HW
    dz = o["gm_" + form] * o["gate"][:, None] + dp
    a1 = dz - sums[0] / n
    xs = (o["y"] - o["mean"]) * o["rstd"] * sums[1]
    inner = a1 - xs / n
    e_in = U24 * (2 * dp.abs() + dz.abs() + (sums[0] / n).abs() + a1.abs() + 4 * (xs / n).abs() + inner.abs())
    a = o["gamma"] * o["rstd"]
    ref = a * inner
    judge(f"se_bwd_apply {shape} {mode} {form}", got, dict(dy=(ref, a.abs() * e_in + 2 * U24 * ref.abs() + store(ref, dt))))


# ------------------------------------------------------------------------------------------------ avg-pool shortcut
POOL = [(2, 9, 7, 64), (2, 8, 10, 256), (1, 1, 1, 64), (3, 5, 5, 2048)]


@gpu
@pytest.mark.parametrize("mode", ("bf16", "fp32"))
@pytest.mark.parametrize("shape", POOL, ids=["x".join(map(str, s)) for s in POOL])
def test_avgpool2x2(dev, shape, mode):
    B, H, W, C = shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    dt = DT[mode]
    g = torch.Generator().manual_seed(H * 100 + W)
    x = (torch.rand(B, H, W, C, generator=g, dtype=F64) * 2 - 1).to(dt).double()
    dout = (torch.rand(B, OH, OW, C, generator=g, dtype=F64) * 2 - 1).to(dt).double()

    def once(b):
        y = K.avgpool2x2_fwd(b.put("x", x, dt), out=b.out("y", (B, OH, OW, C), dt))
        dx = K.avgpool2x2_bwd(b.put("dout", dout, dt), H, W, dx_dtype=dt, out=b.out("dx", (B, H, W, C), dt))
        return dict(y=y, dx=dx)

    got = twice(f"avgpool2x2 {shape} {mode}", once)
    # tap counts, explicitly: 4 inside, 2 on an odd edge, 1 in the odd-odd corner
    cnt = torch.full((OH, OW), 4.0, dtype=F64)
    if H % 2:
        cnt[-1] /= 2
    if W % 2:
        cnt[:, -1] /= 2
    assert H % 2 == 0 or W % 2 == 0 or float(cnt[-1, -1]) == 1.0
    pad = torch.zeros(B, 2 * OH, 2 * OW, C, dtype=F64)
    pad[:, :H, :W] = x
    tot = pad.view(B, OH, 2, OW, 2, C).sum((2, 4))
    pa = torch.zeros_like(pad)
    pa[:, :H, :W] = x.abs()
    ref = tot / cnt[None, :, :, None]
    S = pa.view(B, OH, 2, OW, 2, C).sum((2, 4)) / cnt[None, :, :, None]
    # the backward is exact: a power-of-two divisor of a value of the same dtype
    dref = (dout / cnt[None, :, :, None]).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    assert torch.equal(got["dx"].double(), dref.to(dt).double())
    judge(f"avgpool2x2 {shape} {mode}", got, dict(y=(ref, 3 * U24 * S + (U8 if dt == BF else U24) * ref.abs())))
    if H % 2 and W % 2:  # the corner window holds one tap: its input, unchanged
        assert torch.equal(got["y"][:, -1, -1].double(), x[:, -1, -1])


# ------------------------------------------------------------------------------------------------------ deep stem
def _cshape(shape):
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    return K.conv_shape(B, H, W, Cs, Cout, k, stride, pad, Cin)


STEM = [(2, 17, 18, 8, 32, 3, 2, 1, 3), (2, 64, 64, 8, 32, 3, 2, 1, 3)]


@gpu
@pytest.mark.parametrize("shape", STEM, ids=["2x17x18", "2x64x64"])
def test_deep_stem_conv(dev, shape):
    """conv1.0 of the deep stem, 3 -> 32 3x3 stride 2 over the 8-channel zero-padded image: forward (plain and with the
    BatchNorm partials) on the Cs = 8 gathered path (K = 72, padded to 96 with zero-page chunks) and the weight gradient,
    against float64 F.conv2d on the bf16-rounded operands.  The image has no gradient: no data gradient is launched."""
    B, H, W, Cs, Cout, k, stride, pad, Cin = shape
    s = _cshape(shape)
    assert K._stem8(s, BF), "conv1.0 must take the 8-channel gathered path"
    x, w, dy = CR.operands(shape, "bf16")
    ref, S = CR.fwd_ref(shape, "bf16")
    OH, OW = ref.shape[1:3]
    M = B * OH * OW
    wref, wS = CR.wgrad_ref(shape, "bf16")
    prior = CR.prior(shape, "dw", "f32")

    def once(b):
        xd, wp = b.put("x", x, BF), b.put("wp", CR.packed(w, Cs), BF)
        y = K.conv_fwd(xd, wp, s, BF)
        y2, part = K.conv_fwd_bn_stats(xd, wp, s, BF)
        assert part is not None and tuple(part.shape) == (CR.cdiv(M, 64), 2, Cout)
        dw = b.put("dw", prior)
        K.conv_bwd_weight(b.put("dy", dy, BF), xd, s, dw=dw, accumulate=True)
        return dict(y=b.put("y", y, BF), y2=b.put("y2", y2, BF), part=b.put("part", part), dw=dw)

    got = twice(f"deep stem conv {shape}", once)
    ybound = CR.acc_bound(S, 96) + CR.store_bound(ref, BF)
    q = got["y2"].double().view(M, Cout)
    pref = torch.stack([CR.group_sums(q), CR.group_sums(q * q)], 1)
    pbound = torch.stack([64 * U24 * CR.group_sums(q.abs()), 65 * U24 * CR.group_sums(q * q)], 1)
    arm, sp, kper, _ = CR.wgrad_arm(shape, "bf16")
    wb = CR.acc_bound(wS, M, "bf16", sp, kper) + CR.store_bound(prior + wref, F32, prior, wref)
    judge(f"deep stem conv {shape} wgrad {arm} split {sp}", got,
          dict(y=(ref, ybound), y2=(ref, ybound), part=(pref, pbound), dw=(prior + wref, wb)))


@gpu
def test_deep_stem_second_conv_dgrad(dev):
    """conv1.3 of the deep stem, 32 -> 32 3x3 (the narrowest data gradient the model launches), odd grid"""
    shape = (2, 9, 9, 32, 32, 3, 1, 1, 32)
    s = _cshape(shape)
    _, w, dy = CR.operands(shape, "bf16")
    ref, S = CR.dgrad_ref(shape, "bf16")

    def once(b):
        dx = K.conv_bwd_data(b.put("dy", dy, BF), b.put("wp", CR.packed(w, 32), BF), s, dx_dtype=BF)
        return dict(dx=b.put("dx", dx, BF))

    got = twice("deep stem conv1.3 dgrad", once)
    judge("deep stem conv1.3 dgrad", got, dict(dx=(ref, CR.acc_bound(S, 9 * 32) + CR.store_bound(ref, BF))))
