"""Every BatchNorm and pooling call of a ResNet step (csrc/bn.hip), one call at a time through the
``spine_vision_amd.kernels`` wrapper and argument form ``backbone/resnet.py`` uses, each output compared ELEMENT BY
ELEMENT (every channel of every reduced output) with a float64 CPU evaluation of the same operation on the same rounded
operands (tests/_bn_ref.py).  The older BatchNorm tests bound whole tensors in relative L2 at 126 rows, or hold two kernel
forms bit-equal; the forms share ``bn_pre``, ``bn_dx``, ``reduce_write``, ``fold_chunk``, ``fold_partials`` and
``pool_grad``, so a defect in one of those moves every form together and every equality still holds.

Calls                                                                               -> test here
    bn_stats(y, running_mean=, running_var=, num_batches_tracked=) (shifted sums)    -> test_bn_stats
    bn_stats_from_partials(part, rows, ...) (the conv epilogue's unshifted sums)     -> test_bn_stats_from_partials,
                                                                                        test_conv_stats_chain
    bn_eval_params(running_mean, running_var, eps)                                   -> test_bn_eval_params
    bn_act(y, mean, rstd, gamma, beta, res=, res_bn=, relu=, out_dtype=)             -> test_bn_act
    bn_bwd(...) plain / act + gmask / act + mask_inplace / relu_beta                 -> test_bn_bwd
    bn_bwd(..., relu_beta=, part=) on synthesised and on conv_bwd_data_bn's partials -> test_bn_bwd_part,
                                                                                        test_bn_bwd_part_from_conv
    bn_bwd_dual(...)                                                                 -> test_bn_bwd_dual
    bn_relu_bwd_pooled(...)                                                          -> test_bn_relu_bwd_pooled
    maxpool_fwd / maxpool_bwd, avgpool_fwd / avgpool_bwd                             -> test_maxpool, test_avgpool

Inputs.  mean and rstd handed to the act and backward calls are the f32 roundings of the float64 batch statistics, not
the statistics kernel's output, so each call is judged alone; the bound carries that rounding's 2^-24.  |mean| / std is
0, 1 and 4 across the channels of every case.  ReLU ties need no comparison mask: where the float64 |pre-activation| lies
below tau (twice the f32 error bound of ``bn_pre`` at that element) the cotangent is set to exactly 0, so either sign
gives the same g, sums and dx; the act forms take the mask from their ``act`` input, which the reference shares.

Bounds (tests/_bn_ref.py, derived from the kernels' documented summation order and elementwise roundings, asserted at
2 x for EVERY element): sums within depth 2^-24 sum |t|, depth = ceil(rpp / rp) + (rp - 1) + the fold's
ceil(ceil(q / 128) / 4) + 2 + 128 + (chunks - 1); the finish's dvar / (2 (var + eps)) with dvar proportional to s2 / n;
bn_pre within 2^-24 (|A mean| + 3 |A (y - mean)| + |pre|); bn_dx from the sums' bounds and one rounding per operation;
2^-8 |ref| for a bf16 store.  Max pool values and the masked gradient are exact.

Guards: outputs start as NaN (dgamma / dbeta as a known prior); every input, output, partials and sums buffer the test
owns sits between sentinels; every call runs twice with bit-equal results.  Each case names the arm it expects from the
host geometry restated in _bn_ref.py; ``nparts_for`` is cross-checked against ``sv_bn_nparts``.

The figures of the first runs are recorded in profiles/bn_calls/parity.txt."""
import pytest
import torch

import _bn_ref as R
import _conv_ref as CR
from _bn_ref import BF, F32, F64, U24
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

gpu = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 256
DT = {"bf16": BF, "fp32": F32}
NAN = float("nan")

# (rows, C) -> the statistics arm and the elementwise arm the case must take
CASES = {
    (5, 64): ("V8 tpr8 rp32 slices1 P1 rpp5", "V8 fixc grid"),  # most row-groups empty
    (255, 64): ("V8 tpr8 rp32 slices1 P1 rpp255", "V8 fixc grid"),  # one row short of 8 full sweeps
    (257, 64): ("V8 tpr8 rp32 slices1 P1 rpp257", "V8 fixc grid"),  # one row into the 9th: tail of the two-row loop
    (1000, 64): ("V8 tpr8 rp32 slices1 P3 rpp334", "V8 fixc grid"),  # short last part (332 rows)
    (4099, 256): ("V8 tpr32 rp8 slices1 P64 rpp65", "V8 fixc grid"),  # odd rpp, many parts
    (17, 1024): ("V8 tpr128 rp2 slices1 P1 rpp17", "V8 fixc grid"),
    (1000, 1024): ("V8 tpr128 rp2 slices1 P62 rpp17", "V8 fixc grid"),
    (17, 2048): ("V8 tpr256 rp1 slices1 P2 rpp9", "V8 fixc grid"),
    (1000, 2048): ("V8 tpr256 rp1 slices1 P125 rpp8", "V8 fixc grid"),
    (1000, 128): ("V8 tpr16 rp16 slices1 P7 rpp143", "V8 fixc grid"),
    (1000, 512): ("V8 tpr64 rp4 slices1 P31 rpp33", "V8 fixc grid"),
    # nparts at its cap of 1024 with a short last part (8 rows); grid_for capped at 8192: a second grid-stride step
    (8200, 2048): ("V8 tpr256 rp1 slices1 P1024 rpp9", "V8 fixc capped"),
    # contract edges no ResNet reaches: the V = 4 kernels and the kernels without hoisted parameters
    (37, 12): ("V4 tpr3 rp85 slices1 P1 rpp37", "V4 anyc grid"),
    (1500, 12): ("V4 tpr3 rp85 slices1 P2 rpp750", "V4 fixc grid"),
    (33, 4): ("V4 tpr1 rp256 slices1 P1 rpp33", "V4 fixc grid"),
    (400, 96): ("V8 tpr12 rp21 slices1 P2 rpp200", "V8 anyc grid"),  # grid 19: not a multiple of 3
}
BIG = (8200, 2048)
SMALL = [(257, 64), (1000, 64), (37, 12)]  # every dtype / mode combination runs on these
PARTIALS = [(P, 64) for P in (1, 127, 129, 1024, 1025, 2050, 16384, 16385)] + \
           [(P, 2048) for P in (1, 127, 129, 1024, 1025, 2050)]
FOLD_ARMS = {1: "chunks1 one-workgroup", 127: "chunks1 one-workgroup", 129: "chunks1 one-workgroup",
             1024: "chunks1 one-workgroup", 1025: "chunks2 split", 2050: "chunks3 split", 16384: "chunks16 split",
             16385: "chunks17 one-workgroup"}
POOLED = [(2, 5, 7, 64), (2, 8, 10, 64), (1, 33, 30, 64), (3, 17, 21, 12)]
BWD_PART = [(1, 64), (129, 64), (1025, 64)]


def cid(c):
    return "x".join(map(str, c))


def arms(rows, C):
    assert (R.stats_arm(rows, C), R.apply_arm(rows, C)) == CASES[(rows, C)], \
        f"({rows}, {C}) takes {R.stats_arm(rows, C)} / {R.apply_arm(rows, C)}: the host geometry was retuned"
    return f"{R.stats_arm(rows, C)} | {R.apply_arm(rows, C)}"


# ------------------------------------------------------------------------------------------------------ harness
def _sentinel(dtype):
    return 249 if dtype == torch.uint8 else int(SENTINEL) if dtype == torch.int64 else SENTINEL


class Buffers:
    """device buffers between sentinels"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def _make(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), _sentinel(dtype), device=self.dev, dtype=dtype)
        self.bufs[name] = buf
        return buf[GUARD:GUARD + n].view(shape)

    def put(self, name, t, dtype):
        v = self._make(name, tuple(t.shape), dtype)
        v.copy_(t.to(dtype))
        return v

    def out(self, name, shape, dtype, fill=NAN):
        v = self._make(name, tuple(shape), dtype)
        v.fill_(fill)
        return v

    def check(self, where):
        for n, b in self.bufs.items():
            assert bool((b[:GUARD] == _sentinel(b.dtype)).all()) and bool((b[-GUARD:] == _sentinel(b.dtype)).all()), \
                f"{where}: sentinel around {n} overwritten"


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


def judge(where, got, refs, store=None, priors=None):
    """every element of every output within 2 x bound; prints the largest error / bound per output"""
    figs = []
    for n, (ref, bound) in refs.items():
        g = got[n].double().view(ref.shape)
        if priors and n in priors:
            ref = ref + priors[n]
            bound = bound + CR.store_bound(ref, F32, priors[n], refs[n][0])
        elif store:
            bound = bound + CR.store_bound(ref, store.get(n, F32))
        err = (g - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
        worst = float(ratio.max())
        figs.append(f"{n} err {float(err.max()):.3e} ratio {worst:.3f}")
        if not worst <= 2.0:
            flat = int(ratio.reshape(-1).argmax())
            idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
            print(f"[bn_calls] {where}: " + ", ".join(figs))
            pytest.fail(f"{where} {n}: {int((ratio > 2).sum())} of {ratio.numel()} elements beyond 2 x bound; worst at "
                        f"{idx}: got {float(g.reshape(-1)[flat]):.9g}, float64 {float(ref.reshape(-1)[flat]):.9g}, "
                        f"bound {float(bound.reshape(-1)[flat]):.3e}, error / bound {worst:.3g}")
    print(f"[bn_calls] {where}: " + ", ".join(figs))


def same(a, b):
    assert a.data_ptr() == b.data_ptr()


def stat_inputs(b, rows, C, mode):
    """mean / rstd as call inputs: the f32 roundings of the float64 batch statistics"""
    o = R.operands(rows, C, mode)
    mean, var, rstd = R.batch_stats(o["y"])
    return o, b.put("mean", mean, F32), b.put("rstd", rstd, F32)


@pytest.fixture(autouse=True)
def _drop_capped_case(request):
    """the capped case's float64 operands and references (about 1.5 GB) are used by one test per family: dropped after"""
    yield
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    if params.get("case") == BIG:
        for f in (R.operands, R.stats_ref, R.act_ref, R.bwd_ref):
            f.cache_clear()


# ------------------------------------------------------------------------------------------------------ geometry
@gpu
def test_nparts_matches_library():
    for rows, C in list(CASES) + [(r, c) for c in (4, 12, 64, 96, 256, 1024, 2048, 4096) for r in (1, 7, 64, 300, 70000)]:
        assert R.nparts_for(rows, C) == nv.value("sv_bn_nparts", rows, C), (rows, C)


# ---------------------------------------------------------------------------------------------------- statistics
STATS_CASES = [(c, m, r) for c in CASES for m in ("bf16", "fp32") for r in (True, False)
               if c != BIG or (m == "bf16" and r)]  # the capped case once per family


@gpu
@pytest.mark.parametrize("case,mode,running", STATS_CASES,
                         ids=[f"{cid(c)}-{m}-{'running' if r else 'norunning'}" for c, m, r in STATS_CASES])
def test_bn_stats(case, mode, running):
    rows, C = case
    where = f"bn_stats {rows}x{C} y {mode} {'running' if running else 'plain'} [{arms(rows, C)}]"
    o = R.operands(rows, C, mode)
    refs, sens = R.stats_ref(rows, C, mode)
    P = R.nparts_for(rows, C)

    def once(b):
        y = b.put("y", o["y"], DT[mode])
        mean, rstd = b.out("mean", (C,), F32), b.out("rstd", (C,), F32)
        part = b.out("part", (P, 2, C), F32)
        kw = {}
        if running:
            kw = dict(running_mean=b.put("rm", o["rm0"], F32), running_var=b.put("rv", o["rv0"], F32),
                      num_batches_tracked=b.out("nbt", (1,), torch.int64, 41))
        m, r = K.bn_stats(y, eps=R.EPS, momentum=R.MOM, out=(mean, rstd), part=part, **kw)
        same(m, mean), same(r, rstd)
        res = dict(mean=mean, rstd=rstd, part=part)
        if running:
            res.update(rm=kw["running_mean"], rv=kw["running_var"], nbt=kw["num_batches_tracked"])
        return res

    got = twice(where, once)
    assert bool(torch.isfinite(got["part"]).all()), f"{where}: a partial was not written"
    if running:
        assert int(got["nbt"]) == 42, f"{where}: num_batches_tracked {int(got['nbt'])}, expected 42"
    judge(where, got, refs if running else {n: refs[n] for n in ("mean", "rstd")})


def _finish_once(part64, rows, C, o, running):
    def once(b):
        part = b.put("part", part64, F32)
        mean, rstd = b.out("mean", (C,), F32), b.out("rstd", (C,), F32)
        kw = {}
        if running:
            kw = dict(running_mean=b.put("rm", o["rm0"], F32), running_var=b.put("rv", o["rv0"], F32),
                      num_batches_tracked=b.out("nbt", (1,), torch.int64, 41))
        m, r = K.bn_stats_from_partials(part, rows, eps=R.EPS, momentum=R.MOM, out=(mean, rstd), **kw)
        same(m, mean), same(r, rstd)
        res = dict(mean=mean, rstd=rstd, part=part)
        if running:
            res.update(rm=kw["running_mean"], rv=kw["running_var"], nbt=kw["num_batches_tracked"])
        return res

    return once


@gpu
@pytest.mark.parametrize("case", PARTIALS, ids=cid)
def test_bn_stats_from_partials(case):
    P, C = case
    assert R.fold_arm(P, C) == FOLD_ARMS[P], f"P = {P} folds as {R.fold_arm(P, C)}: the fold was retuned"
    c = R.partials_case(P, C)
    where = f"bn_stats_from_partials P {P} C {C} rows {c['rows']} [{R.fold_arm(P, C)}]"
    got = twice(where, _finish_once(c["part"], c["rows"], C, c, True))
    assert torch.equal(got["part"].double(), c["part"]), f"{where}: the partials were modified"
    assert int(got["nbt"]) == 42
    judge(where, got, c["refs"])
    # the rstd error of the unshifted finish by |mean| / std, beside its bound (DESIGN.md records these)
    err = (got["rstd"].double() - c["refs"]["rstd"][0]).abs() / c["refs"]["rstd"][0]
    bnd = c["refs"]["rstd"][1] / c["refs"]["rstd"][0]
    rat = R.ratios(C)
    print(f"[bn_calls] {where}: relative rstd error / bound at |mean|/std " + ", ".join(
        f"{int(v)}: {float(err[rat == v].max()):.3e} / {float(bnd[rat == v].max()):.3e}" for v in (0, 1, 4)))


@gpu
def test_bn_stats_shifted_rstd_by_ratio():
    """the shifted statistics' relative rstd error by |mean| / std, printed beside the unshifted finish's (no assertion
    beyond test_bn_stats': a figure for DESIGN.md)"""
    rows, C = 1000, 64
    o = R.operands(rows, C, "bf16")
    refs, _ = R.stats_ref(rows, C, "bf16")
    mean, rstd = K.bn_stats(o["y"].to("cuda:0", BF), eps=R.EPS)
    err = (rstd.cpu().double() - refs["rstd"][0]).abs() / refs["rstd"][0]
    rat = R.ratios(C)
    print("[bn_calls] bn_stats 1000x64 relative rstd error at |mean|/std " + ", ".join(
        f"{int(v)}: {float(err[rat == v].max()):.3e}" for v in (0, 1, 4)))
    assert bool((err <= 2 * refs["rstd"][1] / refs["rstd"][0]).all())


@gpu
def test_conv_stats_chain():
    """conv_fwd_bn_stats -> bn_stats_from_partials at the smallest pointwise shape of test_resnet_calls_gpu.py: the
    finish judged on the partials the conv epilogue produced (their float64 sums are the reference)"""
    shape = (2, 9, 7, 64, 256, 1, 1, 0, 64)
    x, w, _ = CR.operands(shape, "bf16")
    dev = torch.device("cuda:0")
    s = K.conv_shape(*shape)
    y, part = K.conv_fwd_bn_stats(x.to(dev, BF), CR.packed(w, 64).to(dev, BF), s, BF)
    assert part is not None and tuple(part.shape) == (2, 2, 256)
    rows, C = 126, 256
    o = R.operands(rows, C, "bf16")
    p64 = part.cpu().double()
    where = "conv_fwd_bn_stats -> bn_stats_from_partials 2,9,7,64,256,1,1,0"
    got = twice(where, _finish_once(p64, rows, C, o, True))
    judge(where, got, R.finish_of(part.cpu(), rows, o["rm0"], o["rv0"]))
    # and against the float64 statistics of the stored y itself: the 64-row partials within test_resnet_calls' bound
    yy = y.cpu().double().view(rows, C)
    mean, var, rstd = R.batch_stats(yy)
    D = 64 + R.fold_depth(2)
    dmean, dvar, drstd = R.finish_bounds(yy.sum(0), (yy * yy).sum(0), torch.zeros(C, dtype=F64), rows,
                                         D * U24 * yy.abs().sum(0), (D + 1) * U24 * (yy * yy).sum(0))
    judge(where + " (against y)", got, dict(mean=(mean, dmean), rstd=(rstd, drstd)))


@gpu
@pytest.mark.parametrize("C", [4, 64, 2048, 1000])
def test_bn_eval_params(C):
    g = torch.Generator().manual_seed(C)
    rm = R.f32r(torch.randn(C, generator=g, dtype=F64))
    rv = R.f32r(torch.rand(C, generator=g, dtype=F64) * 2 + 1e-3)
    rv[0] = 0.0
    where = f"bn_eval_params C {C}"

    def once(b):
        mean, rstd = b.out("mean", (C,), F32), b.out("rstd", (C,), F32)
        m, r = K.bn_eval_params(b.put("rm", rm, F32), b.put("rv", rv, F32), R.EPS, out=(mean, rstd))
        same(m, mean), same(r, rstd)
        return dict(mean=mean, rstd=rstd)

    got = twice(where, once)
    assert torch.equal(got["mean"].double(), rm), f"{where}: mean is not the running mean bit for bit"
    ref = (rv + R.EPS).rsqrt()  # f32(eps) and the sum round once each; sqrtf and the division are correctly rounded
    judge(where, got, dict(rstd=(ref, ref * (U24 * (R.EPS + (rv + R.EPS)) / (2 * (rv + R.EPS)) + 2 * U24))))


# ------------------------------------------------------------------------------------------------------- forward
ACT_FULL = [(m, od, rk, relu) for m, od in (("bf16", BF), ("bf16", F32), ("fp32", F32))
            for rk in ("", "res", "res_bn") for relu in (True, False)]
ACT_MODEL = [("bf16", BF, "", True), ("bf16", BF, "res", True), ("bf16", BF, "res_bn", True), ("bf16", BF, "", False),
             ("fp32", F32, "res", True)]
ACT_CASES = [(c, f) for c in CASES for f in (ACT_FULL if c in SMALL else ACT_MODEL if c != BIG else ACT_MODEL[1:2])]


@gpu
@pytest.mark.parametrize("case,form", ACT_CASES,
                         ids=[f"{cid(c)}-{f[0]}-out{str(f[1])[6:]}-{f[2] or 'plain'}-{'relu' if f[3] else 'linear'}"
                              for c, f in ACT_CASES])
def test_bn_act(case, form):
    rows, C = case
    mode, out_dt, res_kind, relu = form
    where = (f"bn_act {rows}x{C} {mode} out {str(out_dt)[6:]} {res_kind or 'plain'} {'relu' if relu else 'linear'} "
             f"[{arms(rows, C)}]")
    ref, bound = R.act_ref(rows, C, mode, res_kind, relu)

    def once(b):
        o, mean, rstd = stat_inputs(b, rows, C, mode)
        y = b.put("y", o["y"], DT[mode])
        kw = {}
        if res_kind == "res":
            kw = dict(res=b.put("res", o["res"], DT[mode]))
        elif res_kind == "res_bn":
            m2, v2, r2 = R.batch_stats(o["y2"])
            kw = dict(res=b.put("res", o["y2"], DT[mode]),
                      res_bn=(b.put("mean2", m2, F32), b.put("rstd2", r2, F32), b.put("gamma2", o["gamma2"], F32),
                              b.put("beta2", o["beta2"], F32)))
        out = b.out("out", (rows, C), out_dt)
        same(K.bn_act(y, mean, rstd, b.put("gamma", o["gamma"], F32), b.put("beta", o["beta"], F32), relu=relu,
                      out_dtype=out_dt, out=out, **kw), out)
        return dict(out=out)

    judge(where, twice(where, once), dict(out=(ref, bound)), store=dict(out=out_dt))


# ------------------------------------------------------------------------------------------------------ backward
BWD_FORMS = ("plain", "gmask", "inplace", "relu")
DT_FULL = [(m, dd, xd, tr) for m in ("bf16",) for dd in (F32, BF) for xd in (F32, BF) for tr in (True, False)]
DT_MODEL = [("bf16", BF, BF, True), ("fp32", F32, F32, True)]
BWD_CASES = [(c, f, d) for c in CASES for f in (BWD_FORMS if c != BIG else ("relu",))
             for d in (DT_FULL + DT_MODEL[1:] if c in SMALL else DT_MODEL if c != BIG else DT_MODEL[:1])]


def _dt_id(d):
    return f"{d[0]}-dout{str(d[1])[6:]}-dx{str(d[2])[6:]}-{'train' if d[3] else 'eval'}"


def _bwd_once(rows, C, mode, form, dout_dt, dx_dt, train, r, part64=None):
    kind = {"plain": "plain", "gmask": "act", "inplace": "act", "relu": "relu"}[form]
    P = R.nparts_for(rows, C)

    def once(b):
        o, mean, rstd = stat_inputs(b, rows, C, mode)
        y = b.put("y", o["y"], DT[mode])
        dout = b.put("dout", r["dout"], dout_dt)
        gamma = b.put("gamma", o["gamma"], F32)
        dg, db = b.put("dgamma", R.prior(C, "dg"), F32), b.put("dbeta", R.prior(C, "db"), F32)
        dx = b.out("dx", (rows, C), dx_dt)
        sums = b.out("sums", (1, 2, C), F32)
        kw = dict(dgamma=dg, dbeta=db, dx_dtype=dx_dt, batch_stats=train, out=dx, sums=sums)
        res = dict(dx=dx, dgamma=dg, dbeta=db, dout=dout)
        if part64 is not None:
            kw["part"] = b.put("part", part64, F32)
        else:
            kw["work"] = b.out("work", (P, 2, C), F32)
        if kind == "act":
            kw["act"] = b.put("act", r["act"], DT[mode])
            if form == "gmask":
                res["gmask"] = kw["gmask"] = b.out("gmask", (rows, C), F32)
            else:
                kw["mask_inplace"] = True
        elif kind == "relu":
            kw["relu_beta"] = b.put("beta", o["beta"], F32)
        same(K.bn_bwd(dout, y, mean, rstd, gamma, **kw), dx)
        return res

    return once


def _bwd_judge(where, got, r, form, dout_dt, dx_dt, C, suffixes=("",)):
    priors = {}
    for s in suffixes:
        priors["dgamma" + s], priors["dbeta" + s] = R.prior(C, "dg" + s), R.prior(C, "db" + s)
    judge(where, got, {n: v for n, v in r["refs"].items() if n.startswith("d") and not n.startswith("dx")}, priors=priors)
    judge(where, got, {n: v for n, v in r["refs"].items() if n.startswith("dx")},
          store={n: dx_dt for n in r["refs"]})
    g_dt = r["g"].to(dout_dt).double()  # masking an element keeps or zeroes it: exact in dout's dtype
    if form == "gmask":
        assert torch.equal(got["gmask"].double(), r["g"]), f"{where}: gmask is not dout (act > 0) exactly"
    if form in ("inplace", "dual"):
        assert torch.equal(got["dout"].double(), g_dt), f"{where}: dout was not overwritten with dout (act > 0) exactly"
    else:
        assert torch.equal(got["dout"].double(), r["dout"]), f"{where}: dout was modified"


@gpu
@pytest.mark.parametrize("case,form,dts", BWD_CASES, ids=[f"{cid(c)}-{f}-{_dt_id(d)}" for c, f, d in BWD_CASES])
def test_bn_bwd(case, form, dts):
    rows, C = case
    mode, dout_dt, dx_dt, train = dts
    where = f"bn_bwd {form} {rows}x{C} {_dt_id(dts)} [{arms(rows, C)}]"
    kind = {"plain": "plain", "gmask": "act", "inplace": "act", "relu": "relu"}[form]
    r = R.bwd_ref(rows, C, mode, kind, dout_dt, train)
    assert r["ties"] <= 1e-3
    got = twice(where, _bwd_once(rows, C, mode, form, dout_dt, dx_dt, train, r))
    _bwd_judge(where, got, r, form, dout_dt, dx_dt, C)


@gpu
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", BWD_PART, ids=cid)
def test_bn_bwd_part(case, train):
    """relu_beta + part=: the statistics partials [P][2][C] given (synthesised from the float64 masked gradient over P
    groups of 2 - 3 rows, rounded to f32), so only the fold and the apply pass run"""
    P, C = case
    starts, ends = R.group_bounds(P)
    rows = int(ends[-1])
    where = f"bn_bwd relu + part P {P} {rows}x{C} {'train' if train else 'eval'} [{R.fold_arm(P, C)}]"
    r = R.bwd_ref(rows, C, "bf16", "relu", BF, train, D=R.fold_depth(P) + 1)
    o = R.operands(rows, C, "bf16")
    mean, var, rstd = R.batch_stats(o["y"])
    z = torch.zeros(1, C, dtype=F64)
    c1, c2 = torch.cat([z, r["g"].cumsum(0)]), torch.cat([z, (r["g"] * (o["y"] - mean) * rstd).cumsum(0)])
    part = torch.stack([R.f32r(c1[ends] - c1[starts]), R.f32r(c2[ends] - c2[starts])], 1)
    got = twice(where, _bwd_once(rows, C, "bf16", "relu", BF, BF, train, r, part64=part))
    _bwd_judge(where, got, r, "relu", BF, BF, C)


@gpu
def test_bn_bwd_part_from_conv():
    """conv_bwd_data_bn -> bn_bwd(relu_beta=, part=) at the smallest pointwise shape test_resnet_calls_gpu.py builds:
    the BatchNorm backward judged alone on the gradient and the partials the data-gradient epilogue produced (their
    float64 sums are the reference sums; that file checks the partials themselves)"""
    shape = (2, 9, 7, 64, 256, 1, 1, 0, 64)
    rows, C = 126, 64
    _, w, dy = CR.operands(shape, "bf16")
    y, mean, rstd, gamma, beta = CR.bn_operands(shape)
    mask, unsure, xhat = CR.bn_mask(shape)
    dev = torch.device("cuda:0")
    f = lambda t: t.to(dev, F32)  # noqa: E731
    r = K.conv_bwd_data_bn(dy.to(dev, BF), CR.packed(w, 64).to(dev, BF), K.conv_shape(*shape), y.to(dev, BF), f(mean),
                           f(rstd), f(gamma), f(beta))
    assert r is not None, "conv_bwd_data_bn declined a shape on its path"
    dout, p64 = r[0].cpu().double().view(rows, C), r[1].cpu().double()
    P = p64.shape[0]
    where = f"conv_bwd_data_bn -> bn_bwd relu + part 2,9,7,64,256,1,1,0 P {P}"
    y2, xh, m2, u2 = y.view(rows, C), xhat.view(rows, C), mask.view(rows, C), unsure.view(rows, C)
    g = dout * m2
    sg, sgx = p64[:, 0].sum(0), p64[:, 1].sum(0)
    D = R.fold_depth(P)
    dsg, dsgx = D * U24 * p64[:, 0].abs().sum(0), D * U24 * p64[:, 1].abs().sum(0)
    A = gamma * rstd
    dx = A * (g - sg / rows - xh * sgx / rows)
    dxh = U24 * (3 * xh.abs() + mean.abs() * rstd)
    bdx = R.dx_bound(A.abs(), g, xh, dxh, sg, sgx, dsg, dsgx, rows, dx) + u2 * A.abs() * dout.abs()
    rr = dict(dout=dout, g=g, refs=dict(dx=(dx, bdx), dgamma=(sgx, dsgx), dbeta=(sg, dsg)))

    def once(b):
        d = b.put("dout", dout, BF)
        dg, db = b.put("dgamma", R.prior(C, "dg"), F32), b.put("dbeta", R.prior(C, "db"), F32)
        out = b.out("dx", (rows, C), BF)
        same(K.bn_bwd(d, b.put("y", y2, BF), b.put("mean", mean, F32), b.put("rstd", rstd, F32),
                      b.put("gamma", gamma, F32), relu_beta=b.put("beta", beta, F32), dgamma=dg, dbeta=db, dx_dtype=BF,
                      batch_stats=True, part=b.put("part", p64, F32), out=out, sums=b.out("sums", (1, 2, C), F32)), out)
        return dict(dx=out, dgamma=dg, dbeta=db, dout=d)

    _bwd_judge(where, twice(where, once), rr, "relu", BF, BF, C)


DUAL_CASES = [(c, d) for c in CASES if c != BIG for d in (DT_FULL if c in SMALL else DT_MODEL)]


@gpu
@pytest.mark.parametrize("case,dts", DUAL_CASES, ids=[f"{cid(c)}-{_dt_id(d)}" for c, d in DUAL_CASES])
def test_bn_bwd_dual(case, dts):
    rows, C = case
    mode, dout_dt, dx_dt, train = dts
    where = f"bn_bwd_dual {rows}x{C} {_dt_id(dts)} [{arms(rows, C)}]"
    r = R.bwd_ref(rows, C, mode, "dual", dout_dt, train)
    P = R.nparts_for(rows, C)

    def once(b):
        o, mean, rstd = stat_inputs(b, rows, C, mode)
        m2, v2, r2 = R.batch_stats(o["y2"])
        gm = b.put("dout", r["dout"], dout_dt)
        ps = {n: b.put(n, R.prior(C, p), F32) for n, p in (("dgamma", "dg"), ("dbeta", "db"), ("dgamma2", "dg2"),
                                                           ("dbeta2", "db2"))}
        dx, dx2 = b.out("dx", (rows, C), dx_dt), b.out("dx2", (rows, C), dx_dt)
        a, a2 = K.bn_bwd_dual(gm, b.put("y", o["y"], DT[mode]), mean, rstd, b.put("gamma", o["gamma"], F32),
                              b.put("act", r["act"], DT[mode]), b.put("y2", o["y2"], DT[mode]), b.put("mean2", m2, F32),
                              b.put("rstd2", r2, F32), b.put("gamma2", o["gamma2"], F32), dx_dtype=dx_dt,
                              batch_stats=train, out=(dx, dx2), part=b.out("part", (2, P, 2, C), F32),
                              sums=b.out("sums", (2, 2, C), F32), **ps)
        same(a, dx), same(a2, dx2)
        return dict(dx=dx, dx2=dx2, dout=gm, **ps)

    got = twice(where, once)
    _bwd_judge(where, got, r, "dual", dout_dt, dx_dt, C, suffixes=("", "2"))


# ------------------------------------------------------------------------------------------------------- pooling
POOL_DTS = [("bf16", BF, BF, True), ("bf16", F32, F32, True), ("bf16", BF, F32, False), ("fp32", F32, F32, True)]


@gpu
@pytest.mark.parametrize("dts", POOL_DTS, ids=_dt_id)
@pytest.mark.parametrize("shape", POOLED, ids=cid)
def test_bn_relu_bwd_pooled(shape, dts):
    B, H, W, C = shape
    mode, dp_dt, dx_dt, train = dts
    rows = B * H * W
    where = f"bn_relu_bwd_pooled {cid(shape)} {_dt_id(dts)} [{R.stats_arm(rows, C)} | {R.apply_arm(rows, C)}]"
    r = R.pooled_ref(B, H, W, C, mode, dp_dt, train)
    assert r["ties"] <= 1e-3
    P = R.nparts_for(rows, C)

    def once(b):
        o, mean, rstd = stat_inputs(b, rows, C, mode)
        dg, db = b.put("dgamma", R.prior(C, "dg"), F32), b.put("dbeta", R.prior(C, "db"), F32)
        dx = b.out("dx", (rows, C), dx_dt)
        dpool = b.put("dpool", r["dpool"], dp_dt)
        same(K.bn_relu_bwd_pooled(dpool, b.put("idx", r["idx"], torch.uint8), H, W, b.put("y", o["y"], DT[mode]), mean,
                                  rstd, b.put("gamma", o["gamma"], F32), b.put("beta", o["beta"], F32), dgamma=dg,
                                  dbeta=db, dx_dtype=dx_dt, batch_stats=train, out=dx,
                                  part=b.out("part", (P, 2, C), F32), sums=b.out("sums", (1, 2, C), F32)), dx)
        return dict(dx=dx, dgamma=dg, dbeta=db, dpool=dpool)

    got = twice(where, once)
    assert torch.equal(got["dpool"].double(), r["dpool"]), f"{where}: dpool was modified"
    priors = dict(dgamma=R.prior(C, "dg"), dbeta=R.prior(C, "db"))
    judge(where, got, {n: r["refs"][n] for n in ("dgamma", "dbeta")}, priors=priors)
    judge(where, got, dict(dx=r["refs"]["dx"]), store=dict(dx=dx_dt))


@gpu
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", POOLED, ids=cid)
def test_maxpool(shape, mode):
    B, H, W, C = shape
    where = f"maxpool {cid(shape)} {mode}"
    x = R.pool_input(B, H, W, C, mode)
    yref, iref, taps = R.maxpool_ref(x)
    assert float((taps == yref.unsqueeze(-1)).sum(-1).gt(1).double().mean()) > 0.05, "the input must hold tied windows"
    OH, OW = yref.shape[1:3]
    g = torch.Generator().manual_seed(B * H * W * C)
    d = (torch.randn(B, OH, OW, C, generator=g, dtype=F64) + 0.5).to(DT[mode]).double()

    def once(b):
        y, idx = b.out("y", (B, OH, OW, C), DT[mode]), b.out("idx", (B, OH, OW, C), torch.uint8, 255)
        a, i = K.maxpool_fwd(b.put("x", x, DT[mode]), out=(y, idx))
        same(a, y), same(i, idx)
        res = dict(y=y, idx=idx)
        for n, dd, xd in (("dx_model", DT[mode], DT[mode]), ("dx_f32", DT[mode], F32)):
            dx = b.out(n, (B, H, W, C), xd)
            same(K.maxpool_bwd(b.put("d" + n, d, dd), idx, H, W, dx_dtype=xd, out=dx), dx)
            res[n] = dx
        return res

    got = twice(where, once)
    assert torch.equal(got["y"].double(), yref), f"{where}: a pooled value is not the window's maximum exactly"
    held = taps.gather(-1, got["idx"].long().clamp_max(8).unsqueeze(-1)).squeeze(-1)
    assert bool((got["idx"] < 9).all()) and torch.equal(held, yref), f"{where}: idx points at a tap without the maximum"
    assert torch.equal(got["idx"], iref), f"{where}: under ties idx is not the first tap in scan order"
    ref = R.maxpool_bwd_ref(d, iref, H, W)
    absr = R.maxpool_bwd_ref(d.abs(), iref, H, W)
    judge(where, got, dict(dx_model=(ref, 3 * U24 * absr), dx_f32=(ref, 3 * U24 * absr)),
          store=dict(dx_model=DT[mode], dx_f32=F32))
    print(f"[bn_calls] {where}: values and indices exact")


@gpu
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(3, 7, 7, 64), (2, 7, 7, 2048), (5, 1, 1, 512), (130, 1, 1, 12), (2, 3, 5, 4)], ids=cid)
def test_avgpool(shape, mode):
    B, H, W, C = shape
    where = f"avgpool {cid(shape)} {mode}"
    g = torch.Generator().manual_seed(B * H * W * C + 1)
    x = (torch.randn(B, H, W, C, generator=g, dtype=F64) + 0.5).to(DT[mode]).double()
    df = R.f32r(torch.randn(B, C, generator=g, dtype=F64))
    HW = H * W

    def once(b):
        feat = b.out("feat", (B, C), F32)
        same(K.avgpool_fwd(b.put("x", x, DT[mode]), out=feat), feat)
        dx = b.out("dx", (B, H, W, C), DT[mode])
        same(K.avgpool_bwd(b.put("dfeat", df, F32), (B, H, W, C), dx_dtype=DT[mode], out=dx), dx)
        return dict(feat=feat, dx=dx)

    got = twice(where, once)
    xs = x.view(B, HW, C)
    # a serial f32 sum of HW terms, then one product with the rounded 1 / HW
    fref = xs.mean(1)
    fb = (HW - 1) * U24 * xs.abs().mean(1) + 2 * U24 * fref.abs()
    dref = (df / HW).view(B, 1, 1, C).expand(B, H, W, C).contiguous()
    judge(where, got, dict(feat=(fref, fb)))
    judge(where, got, dict(dx=(dref, 2 * U24 * dref.abs())), store=dict(dx=DT[mode]))


# ------------------------------------------------------------------------------- conditions that need no GPU
def test_reference_side_conditions():
    """For the whole case list: every case's arms are the ones its table names; the zeroed-cotangent share stays at or
    below 0.1 %; dropping one thread's last row of a part (one partial, or from 16384 partials one stream of a chunk)
    moves every reduced output's float64 value by more than 4 x its bound in at least 99 % of the channels (the RMS over
    the candidate rows, over the channels whose candidate rows hold any unmasked gradient; for dx: some element of the
    channel); every production (C, arm) pair of the ResNet family
    appears among the cases."""
    from spine_vision_amd.backbone.resnet import create_resnet

    lines = []

    def record(where, ties, sens):
        lines.append(f"{where}: zeroed share {ties:.2e}, sensitivity " + ", ".join(f"{n} {v:.4f}" for n, v in sens.items()))
        assert ties <= 1e-3, f"{where}: {ties:.2e} of the cotangents zeroed"
        for n, v in sens.items():
            assert v >= 0.99, f"{where}: only {v:.4f} of the channels have a dropped row's change in {n} above 4 x bound"

    for (rows, C) in CASES:
        if (rows, C) == BIG:
            continue  # the capped case's float64 reference is built where it runs; its geometry is asserted here
        arms(rows, C)
        for mode in ("bf16", "fp32"):
            record(f"bn_stats {rows}x{C} {mode}", 0.0, R.stats_ref(rows, C, mode)[1])
        for kind in ("plain", "act", "relu", "dual"):
            for dd in (BF, F32):
                r = R.bwd_ref(rows, C, "bf16", kind, dd, True)
                record(f"bn_bwd {kind} {rows}x{C} dout {str(dd)[6:]}", r["ties"], r["sens"])
    arms(*BIG)
    for P, C in PARTIALS:
        assert R.fold_arm(P, C) == FOLD_ARMS[P]
        if C == 64:
            record(f"bn_stats_from_partials P {P} C {C}", 0.0, R.partials_case(P, C)["sens"])
    for shape in POOLED:
        r = R.pooled_ref(*shape, "bf16", BF, True)
        record(f"bn_relu_bwd_pooled {cid(shape)}", r["ties"], r["sens"])
    # the reference scatter against autograd on a tie-free input
    x = torch.randn(2, 9, 11, 8, dtype=F64).requires_grad_(True)
    yy, idx, _ = R.maxpool_ref(x.detach())
    d = torch.randn_like(yy)
    gx, = torch.autograd.grad(torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1), x, d)
    assert torch.allclose(gx, R.maxpool_bwd_ref(d, idx, 9, 11), rtol=1e-14, atol=1e-14)
    have = {(C, R.channel_arm(C)) for (_, C) in CASES}
    for C in R.production_channels(create_resnet):
        assert (C, R.channel_arm(C)) in have, f"no case covers C = {C} on the arm {R.channel_arm(C)}"
        lines.append(f"production C {C}: {R.channel_arm(C)} covered")
    print("\n".join("[bn_calls] " + ln for ln in lines))
