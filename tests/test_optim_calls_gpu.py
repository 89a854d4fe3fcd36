"""What runs after the backward kernels, once per step and for every model (csrc/optim.hip), one call at a time through
the wrappers the trainers use, every element of every output against float64 evaluated on the CPU from the very values
the kernel was given, judged by ``_calls_harness.judge``: |got - ref| <= 2 x a bound derived in tests/_optim_ref.py for
EVERY element.  test_kernels_gpu.py::test_adamw_and_clip allows 1e-5 |p|, which is the whole weight-decay term of its
one case; the other optimizer tests compare the kernel with itself.

1. sv_adamw_flat / sv_adamw_flat_dev (kernels.adamw_flat).  One buffer mixes six element classes (_optim_ref.classes):
   generic, first step (m = v = 0), g = 0, arena padding (all zero: must stay +0 in p, m, v and the shadow), eps-dominated
   (|g sc| ~ 1e-9, v ~ 1e-18) and a nearly cancelling moment update.  Four hyper-parameter sets (_optim_ref.HYPERS; at
   (1e-4, 1e-5, step 1) the kernel's 1 - lr wd rounds to 1.0f as torch's float32 does, the float64 value is expected
   within the bound), no gradient scale / a device coefficient below 1 / exactly 1, shadow present and absent, lengths
   1, 3, 4, 5, 1023, 1024, 1027 and 2 x 2 097 152 + 1024 + 3 (two laps of the grid-stride loop, a partial third and a
   scalar tail).  The device arm runs the same cases from a row of a [runs][4] tensor filled from adamw_hyper and must
   equal the host arm bit for bit; the shadow is bf16 of the GPU's own p', bit for bit.  A slice [s, e) of a larger
   arena (s, e multiples of 16, as FlatAdamW._runs cuts them) leaves everything outside it bit-unchanged in all five
   buffers.
2. sv_sqnorm_partial + sv_clip_coef (kernels.grad_clip_coef): random and one-hot gradients, zero, norms below and just
   above max_norm, a max_norm other than 1.
3. sv_cast_f32_bf16 against torch's CPU cast, bit for bit (NaN stays NaN).
4. The folds: sv_reduce_partials_pair at each of its seven column widths, its wide arm and that arm's neighbours,
   every depth class, ragged and short n, an unaligned output; sv_reduce_partials_multi; _bf16; the grouped
   sv_reduce_partials; sv_colsum's partials and colsum_into.  256 sentinels behind every output.
5. FlatAdamW over a toy arena with a parameter frozen for two steps, five clipped steps, each judged from the GPU's own
   pre-step state; step counts and state_dict layout against torch.optim.AdamW in float64.

The reference-side conditions (the float32 CPU evaluation inside 1 x the bound; which faults the bound can see) are
tests/test_optim_calls_cpu.py.  Figures of the GPU run: profiles/optim_calls/parity.txt."""
import pytest
import torch

import _optim_ref as R
from _calls_harness import judge
from _conv_ref import BF, F32, U24
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv
from spine_vision_amd.training.flat import FlatArena
from spine_vision_amd.training.optim import FlatAdamW

pytestmark = pytest.mark.gpu
TAG = "optim_calls"
GUARD, SENT = 256, -7.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _plus_zero(t):
    return bool((_bits(t) == 0).all())


# ---------------------------------------------------------------------------------------------------------- AdamW
def _scale(dev, sc):
    """(device operand, the f32 value read back)"""
    if sc is None:
        return None, 1.0
    t = torch.tensor([sc], dtype=F32).to(dev)
    return t, float(t.cpu()[0])


def _adamw_run(dev, ins, lr, wd, step, scale_t, shadow, arm, lo=0, hi=None):
    """the update of [lo, hi) of copies of ``ins`` on the device -> (p, m, v, shadow or None) whole buffers"""
    p, g, m, v = (t.to(dev) for t in ins)
    hi = p.numel() if hi is None else hi
    pb = torch.full((p.numel(),), SENT, dtype=BF, device=dev) if shadow else None
    kw = dict(lr=lr, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS, weight_decay=wd, step=step, grad_scale=scale_t)
    if arm == "dev":
        rows = [[0.0] * 4, K.adamw_hyper(lr, R.BETA1, R.BETA2, step) + [0.0], [9.0] * 4]
        assert rows[1][:3] == R.hyper_row(lr, step)
        kw.update(lr=0.0, step=1, hyper=torch.tensor(rows, dtype=F32).to(dev)[1])
    K.adamw_flat(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi] if shadow else None, **kw)
    torch.cuda.synchronize()
    assert _same(g, ins[1]), "the gradient was written"
    return p, m, v, pb


def _adamw_case(dev, n, hyper, sc, where):
    lr, wd, step = hyper
    scale_t, scv = _scale(dev, sc)
    p, g, m, v, cls = R.adamw_inputs(n, scv)
    ref, bound = R.adamw_ref(p, g, m, v, lr, wd, step, scv)
    pad = cls == R.PAD
    first = None
    for shadow in (True, False):
        for arm in ("host", "dev"):
            gp, gm, gv, gb = _adamw_run(dev, (p, g, m, v), lr, wd, step, scale_t, shadow, arm)
            got = dict(p=gp.cpu(), m=gm.cpu(), v=gv.cpu())
            judge(TAG, f"adamw {where} n={n} shadow={int(shadow)} {arm}", got, {k: (ref[k], bound[k]) for k in ref})
            for k in got:
                assert _plus_zero(got[k][pad]), f"{k}: arena padding did not stay +0"
            if shadow:
                assert _same(gb, gp.cpu().to(BF)), "shadow != bf16(p')"
                assert _plus_zero(gb.cpu()[pad])
            if first is None:
                first = got
            else:  # the device arm, and the run without a shadow, bit for bit the first
                for k in got:
                    assert _same(got[k], first[k]), f"{k}: {arm} arm, shadow={int(shadow)} differs from the host arm's bits"


@pytest.mark.parametrize("sc", R.SCALES, ids=["noscale", "coef<1", "coef=1"])
@pytest.mark.parametrize("hyper", R.HYPERS, ids=[f"lr{h[0]:g}-wd{h[1]:g}-step{h[2]}" for h in R.HYPERS])
def test_adamw_small_lengths(dev, hyper, sc):
    for n in R.SMALL:
        _adamw_case(dev, n, hyper, sc, f"{hyper} sc={sc}")


@pytest.mark.parametrize("hyper,sc", [(R.HYPERS[0], R.SCALES[1]), (R.HYPERS[1], R.SCALES[0]), (R.HYPERS[2], R.SCALES[1]),
                                      (R.HYPERS[3], R.SCALES[2])],
                         ids=["defaults-coef<1", "oracle-noscale", "late-coef<1", "nodecay-coef=1"])
def test_adamw_three_laps_and_a_tail(dev, hyper, sc):
    """n = 2 x 2 097 152 + 1024 + 3: two full laps of the 2048 x 256 x 4 grid, a partial third and a scalar tail"""
    _adamw_case(dev, R.ADAMW_BIG, hyper, sc, f"{hyper} sc={sc}")


@pytest.mark.parametrize("arm", ["host", "dev"])
@pytest.mark.parametrize("lo,hi", [(16, 1072), (2048, 2064), (0, 4096), (4096, 4096 + 1040)])
def test_adamw_slice_leaves_the_rest_of_the_arena(dev, lo, hi, arm):
    N = 8192
    lr, wd, step = R.HYPERS[0]
    scale_t, scv = _scale(dev, R.SCALES[1])
    p, g, m, v, _ = R.adamw_inputs(N, scv, seed=1)
    ref, bound = R.adamw_ref(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr, wd, step, scv)
    gp, gm, gv, gb = _adamw_run(dev, (p, g, m, v), lr, wd, step, scale_t, True, arm, lo, hi)
    got = dict(p=gp.cpu(), m=gm.cpu(), v=gv.cpu())
    judge(TAG, f"adamw slice [{lo}, {hi}) {arm}", {k: t[lo:hi] for k, t in got.items()},
          {k: (ref[k], bound[k]) for k in ref})
    outside = torch.ones(N, dtype=torch.bool)
    outside[lo:hi] = False
    for k, before in (("p", p), ("m", m), ("v", v)):
        assert _same(got[k][outside], before[outside]), f"{k} changed outside [{lo}, {hi})"
    sh = gb.cpu()
    assert _same(sh[outside], torch.full((int(outside.sum()),), SENT, dtype=BF)), "shadow changed outside the slice"
    assert _same(sh[lo:hi], got["p"][lo:hi].to(BF))


# ----------------------------------------------------------------------------------------------------------- clip
def _clip(dev, g, max_norm):
    out = K.grad_clip_coef(g.to(dev), max_norm).cpu()
    return float(out[0]), float(out[1])


def _clip_judge(where, g, max_norm, norm, coef):
    rn, rc, bn, bc = R.clip_ref(g, max_norm)
    en = abs(norm - rn) / (bn * rn) if rn else float(norm != 0)
    raw = R.f32v(max_norm) / (rn + R.f32v(1e-6))
    if raw > 1.0 + bc:
        ec = 0.0 if coef == 1.0 else float("inf")  # a norm below max_norm: exactly 1
    elif raw < 1.0 - bc:
        ec = abs(coef - rc) / (bc * rc)
        assert coef < 1.0
    else:
        ec = min(abs(coef - raw) / (bc * raw), float(coef != 1.0))
    print(f"[{TAG}] clip {where}: norm {norm:.9g} float64 {rn:.9g} ratio {en:.3f}, coef {coef:.9g} float64 {rc:.9g} ratio {ec:.3f}")
    assert en <= 2.0 and ec <= 2.0, (where, norm, rn, coef, rc)


@pytest.mark.parametrize("n", R.SMALL + [R.ADAMW_BIG, R.SQ_BIG])
def test_clip_random_gradient(dev, n):
    g = R.clip_gradient(n)
    rn = float(g.double().norm())
    # max_norm 1 and 0.25 (the norm is far above both), twice the norm (exactly 1), and a norm just above max_norm
    for max_norm in (1.0, 0.25, 2.0 * rn, 0.9999 * rn):
        norm, coef = _clip(dev, g, max_norm)
        _clip_judge(f"random n={n} max_norm={max_norm:.6g}", g, max_norm, norm, coef)
        if max_norm == 2.0 * rn:
            assert coef == 1.0
        if max_norm == 0.9999 * rn:
            assert coef < 1.0


@pytest.mark.parametrize("n", [5, 1027, R.SQ_BIG])
def test_clip_one_hot_gradient(dev, n):
    val = R.f32v(-3.7)
    for i in R.one_hot_positions(n):
        g = torch.zeros(n)
        g[i] = val
        norm, coef = _clip(dev, g, 1.0)
        err = abs(norm - abs(val)) / (U24 * abs(val))
        print(f"[{TAG}] clip one-hot n={n} at {i}: norm {norm:.9g}, error {err:.3f} u")
        assert err <= 2.0, (n, i, norm)
        _clip_judge(f"one-hot n={n} at {i}", g, 1.0, norm, coef)


@pytest.mark.parametrize("n", [1, 5, 1027, R.SQ_BIG])
def test_clip_zero_gradient(dev, n):
    norm, coef = _clip(dev, torch.zeros(n), 1.0)
    assert norm == 0.0 and coef == 1.0


# ----------------------------------------------------------------------------------------------------------- cast
def _cast_check(dev, x, where):
    n = x.numel()
    out = torch.full((n + GUARD,), SENT, dtype=BF, device=dev)
    K.cast_bf16(x.to(dev), out[:n])
    got = out.cpu()
    want = x.to(BF)
    nan = torch.isnan(x)
    assert bool(torch.isnan(got[:n][nan].float()).all()), f"{where}: NaN did not stay NaN"
    diff = (_bits(got[:n]) != _bits(want)) & ~nan
    if bool(diff.any()):
        i = int(diff.nonzero()[0])
        pytest.fail(f"{where}: {int(diff.sum())} of {n} differ from torch's cast; first at {i}: f32 {float(x[i])!r} "
                    f"(bits {int(_bits(x)[i]) & 0xffffffff:#010x}) -> {int(_bits(got)[i]) & 0xffff:#06x}, torch "
                    f"{int(_bits(want)[i]) & 0xffff:#06x}")
    assert _same(got[n:], torch.full((GUARD,), SENT, dtype=BF)), f"{where}: wrote behind the output"


def test_cast_two_laps_and_a_tail(dev):
    _cast_check(dev, R.cast_input(R.CAST_BIG), f"n={R.CAST_BIG}")


@pytest.mark.parametrize("n", [1, 3])
def test_cast_short(dev, n):
    sp = R.cast_specials()
    sp = torch.cat([sp, R.cast_input(64, seed=n)])
    for at in range(0, sp.numel() - n + 1, n):
        _cast_check(dev, sp[at: at + n].clone(), f"n={n} specials[{at}:{at + n}]")


# ---------------------------------------------------------------------------------------------------------- folds
def _out_buf(dev, n, prior, off=0):
    """a device buffer [off][n][GUARD] of sentinels with the prior (or NaN) in the middle -> (buffer, the output view)"""
    buf = torch.full((off + n + GUARD,), SENT, dtype=F32)
    buf[off: off + n] = prior if prior is not None else float("nan")
    buf = buf.to(dev)
    return buf, buf[off: off + n]


def _guards(buf, n, off, where):
    b = buf.cpu()
    assert bool((b[:off] == SENT).all()) and bool((b[off + n:] == SENT).all()), f"{where}: wrote outside the output"


def _seg_depth(P, n, n_other, aligned, wide_possible=True):
    """the depth of the body sv_reduce_partials_pair runs for a segment (n_other: the other segment of the launch)"""
    return R.wide_depth(P) if wide_possible and R.takes_wide(P, n, aligned) else R.pair_depth(P, R.pair_cols(P, n, n_other))


def _pair(dev, P, n_a, n_b, accumulate, alpha, where, off_a=0, cols=None, wide=None, seed=0):
    """reduce_pair (reduce_into when n_b is None) on fresh inputs; ``cols`` / ``wide``: what the launcher's rule must
    pick for the a segment (asserted against the restated rule)"""
    pa, qa = R.fold_inputs(P, n_a, seed)
    aligned = off_a % 4 == 0
    is_wide = R.takes_wide(P, n_a, aligned)
    if wide is not None:
        assert is_wide == wide, f"{where}: the wide arm is {'not ' if wide else ''}what the launcher's rule picks"
    nb = n_b or 0
    if is_wide:  # the a segment runs reduce_partials_kernel, the b segment follows alone
        da, db = R.wide_depth(P), R.pair_depth(P, R.pair_cols(P, nb, 0))
    else:
        c = R.pair_cols(P, n_a, nb)
        if cols is not None:
            assert c == cols, f"{where}: the launcher's rule picks {c} columns, the case says {cols}"
        da = db = R.pair_depth(P, c)
    bufa, outa = _out_buf(dev, n_a, qa if accumulate else None, off_a)
    refs = {"a": R.fold_ref(pa, alpha, qa if accumulate else None, da)}
    if n_b is None:
        K.reduce_into(pa.to(dev).reshape(-1), P, outa, accumulate=accumulate, alpha=alpha)
        got = {"a": outa.cpu()}
    else:
        pb, qb = R.fold_inputs(P, n_b, seed + 1)
        bufb, outb = _out_buf(dev, n_b, qb if accumulate else None)
        refs["b"] = R.fold_ref(pb, alpha, qb if accumulate else None, db)
        K.reduce_pair(pa.to(dev).reshape(-1), outa, pb.to(dev).reshape(-1), outb, P, accumulate=accumulate, alpha=alpha)
        got = {"a": outa.cpu(), "b": outb.cpu()}
        _guards(bufb, n_b, 0, where)
    _guards(bufa, n_a, off_a, where)
    judge(TAG, where, got, refs)


# (P, n_a, n_b, the column width sv_reduce_partials_pair's rule picks): cols starts at 256 (P <= 4), 128 (P <= 8) or
# 64 and halves while ceil(n_a / cols) + ceil(n_b / cols) < 512 and cols > 4
WIDTHS = [
    (3, 65532, 65540, 256),   # 256 + 257 = 513 workgroups at 256 columns (n_a < 65536: not the wide arm)
    (8, 40000, 25600, 128),   # P <= 8 starts at 128: 313 + 200
    (3, 40000, 25600, 128),   # P <= 4 starts at 256: 157 + 100 < 512, then 128
    (17, 20001, 12801, 64),   # P > 8 starts at 64: 313 + 201; a ragged a segment
    (5, 10001, 6400, 32),     # 157 + 100 at 64, 313 + 200 at 32
    (2, 5003, 3200, 16),      # 313 + 200 at 16
    (9, 2501, 1600, 8),       # 313 + 200 at 8
    (16, 96, 7, 4),           # nothing gives 512 workgroups: 4
]


@pytest.mark.parametrize("alpha", [1.0, 0.5, -1.25])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", WIDTHS, ids=[f"P{c[0]}-{c[1]}+{c[2]}-cols{c[3]}" for c in WIDTHS])
def test_reduce_pair_each_column_width(dev, case, accumulate, alpha):
    P, n_a, n_b, cols = case
    _pair(dev, P, n_a, n_b, accumulate, alpha, f"pair cols={cols} P={P} n=({n_a}, {n_b}) acc={int(accumulate)} alpha={alpha}",
          cols=cols, wide=False)


DEPTHS = [1, 2, 15, 16, 17, 63, 64, 65, 300, 1025]


@pytest.mark.parametrize("P", DEPTHS)
def test_reduce_pair_depths_and_ragged_lengths(dev, P):
    """every depth at 4 columns per workgroup (256 partial-row groups: P = 1025 reaches the four-deep unroll),
    n % 4 in {0, 1, 2, 3} and n < 4, through reduce_pair and reduce_into, accumulate and alpha alternating"""
    for k, (n_a, n_b) in enumerate([(96, 18), (97, 3), (98, 1), (99, 2), (3, 96), (1, None), (2, None), (100, None)]):
        acc, alpha = bool(k & 1), (1.0, 0.5, -1.25)[k % 3]
        _pair(dev, P, n_a, n_b, acc, alpha, f"pair P={P} n=({n_a}, {n_b}) acc={int(acc)} alpha={alpha}", cols=4, seed=k)


@pytest.mark.parametrize("P", [17, 65, 300])
def test_reduce_pair_depths_at_64_columns(dev, P):
    """16 partial-row groups: the four-deep unroll from P = 49 on, its remainder loop at 65 and 300"""
    _pair(dev, P, 20004, 12801, True, -1.25, f"pair cols=64 P={P}", cols=64)
    _pair(dev, P, 32768, None, False, 1.0, f"into cols=64 P={P}", cols=64)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("P,n_a,n_b,cols", [(3, 96, 20, 4), (17, 20000, 12800, 64), (3, 65532, 65540, 256), (300, 4, 5, 4)])
def test_reduce_pair_output_off_16_bytes(dev, P, n_a, n_b, cols, accumulate):
    """an output view one element into its buffer: whole column groups take the scalar store branch"""
    _pair(dev, P, n_a, n_b, accumulate, 0.5, f"pair off-by-one out P={P} n=({n_a}, {n_b}) acc={int(accumulate)}",
          off_a=1, cols=cols)


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("P", [3, 8, 9, 64])
@pytest.mark.parametrize("n", [65536, 65540])
def test_reduce_pair_wide_arm(dev, n, P, with_b):
    """P <= 64, n >= 65536, n % 4 == 0, a 16-B aligned output: reduce_partials_kernel's body (8 rows in flight, then
    the remainder loop: P = 3 all remainder, 8 none, 9 one row, 64 eight rounds), the b segment behind it"""
    for k, (acc, alpha) in enumerate([(False, 1.0), (True, -1.25)]):
        _pair(dev, P, n, 100 if with_b else None, acc, alpha, f"wide P={P} n={n} b={int(with_b)} acc={int(acc)}", wide=True,
              seed=k)


@pytest.mark.parametrize("P,n,off", [(65, 65536, 0), (64, 65532, 0), (8, 65536, 1), (64, 65540, 1)],
                         ids=["P65", "n65532", "P8-unaligned", "P64-unaligned"])
def test_reduce_pair_wide_arm_neighbours(dev, P, n, off):
    """one condition of the wide arm fails: the partial-row-group kernel runs"""
    _pair(dev, P, n, 20, True, 0.5, f"not wide P={P} n={n} off={off}", off_a=off, wide=False)


def _multi(dev, specs, alpha, where):
    """specs: (P, n, accumulate, off); one reduce_multi call over all of them"""
    segs, checks = [], []
    for k, (P, n, acc, off) in enumerate(specs):
        part, prior = R.fold_inputs(P, max(n, 1), seed=50 + k)
        part = part[:, :n]
        prior = prior[:n]
        wide = R.takes_wide(P, n, off % 4 == 0)
        d = R.wide_depth(P) if wide else R.pair_depth(P, 64)
        buf, out = _out_buf(dev, n, prior if acc else None, off)
        pd = part.contiguous().to(dev).reshape(-1) if n else torch.zeros(4, device=dev)
        segs.append((pd, out if n else buf, P, acc))
        checks.append((k, buf, out, n, off, R.fold_ref(part.contiguous(), alpha, prior if acc else None, d), wide))
    if all(sp[1] for sp in specs):
        K.reduce_multi(segs, alpha=alpha)
    else:
        # torch gives a zero-length view a null data pointer, which the entry point refuses as a bad segment (as it
        # does any null pointer): a zero-length segment goes through the ABI with its buffers' pointers and n = 0
        assert len(segs) <= nv.SV_MAX_RED_SEGS
        arr = (nv.RedSeg * len(segs))(*[nv.RedSeg(nv.ptr(pd), nv.ptr(o), sp[1], int(P), int(acc))
                                       for (pd, o, P, acc), sp in zip(segs, specs)])
        nv.call("sv_reduce_partials_multi", arr, len(segs), alpha)
    for k, buf, out, n, off, ref, wide in checks:
        _guards(buf, n, off, f"{where} segment {k}")
        if n:
            judge(TAG, f"{where} segment {k} P={specs[k][0]} n={n} {'wide' if wide else 'deep'}", {"out": out.cpu()},
                  {"out": ref})


EIGHT = [(8, 65536, False, 0), (300, 96, True, 0), (64, 65540, True, 0), (1025, 7, False, 0), (17, 0, True, 0),
         (3, 65536, True, 4), (65, 65536, False, 0), (16, 20001, True, 1)]


@pytest.mark.parametrize("alpha", [1.0, -1.25])
def test_reduce_multi_eight_segments(dev, alpha):
    """SV_MAX_RED_SEGS segments, wide and deep mixed, accumulate per segment, a zero-length one in the middle, one
    unaligned output"""
    assert len(EIGHT) == nv.SV_MAX_RED_SEGS
    _multi(dev, EIGHT, alpha, f"multi x8 alpha={alpha}")


def test_reduce_multi_nine_segments_two_launches(dev):
    nine = [sp if sp[1] else (17, 130, True, 0) for sp in EIGHT] + [(9, 65536, True, 0)]
    _multi(dev, nine, 0.5, "multi x9")


def test_reduce_multi_single_and_all_empty(dev):
    _multi(dev, [(64, 65536, False, 0)], 1.0, "multi x1")
    _multi(dev, [(5, 0, False, 0), (7, 0, True, 0)], 1.0, "multi empty")


@pytest.mark.parametrize("n", [4096, 4099, 3, 1028])
@pytest.mark.parametrize("P", [1, 7, 8, 9, 16])
def test_reduce_partials_bf16(dev, P, n):
    for k, (acc, alpha) in enumerate([(False, 1.0), (True, 0.5), (True, -1.25)]):
        part, prior = R.fold_inputs(P, n, seed=80 + k, dtype=BF)
        buf, out = _out_buf(dev, n, prior if acc else None)
        pd = part.to(dev)
        nv.call("sv_reduce_partials_bf16", nv.ptr(pd), P, n, nv.ptr(out), alpha, int(acc))
        where = f"bf16 slabs P={P} n={n} acc={int(acc)} alpha={alpha}"
        _guards(buf, n, 0, where)
        judge(TAG, where, {"out": out.cpu()}, {"out": R.fold_ref(part, alpha, prior if acc else None, R.wide_depth(P))})


@pytest.mark.parametrize("P,group", [(12, 4), (13, 4), (17, 8), (9, 9), (9, 1), (5, 0), (20, 16)])
@pytest.mark.parametrize("n", [1024, 1027, 2])
def test_reduce_partials_grouped(dev, P, group, n):
    """out[g] (+)= alpha x the sum of group g's rows; the last group short at (13, 4), (17, 8), (20, 16); group 0 = P"""
    gl = group if 0 < group <= P else P
    G = R.cdiv(P, gl)
    for k, (acc, alpha) in enumerate([(False, 1.0), (True, -1.25)]):
        part, _ = R.fold_inputs(P, n, seed=90 + k)
        prior = R.fold_inputs(1, G * n, seed=95 + k)[1]
        buf, out = _out_buf(dev, G * n, prior if acc else None)
        pd = part.to(dev)
        K.call("sv_reduce_partials", K.ptr(pd), P, group, n, K.ptr(out), alpha, int(acc))
        where = f"grouped P={P} group={group} n={n} acc={int(acc)}"
        _guards(buf, G * n, 0, where)
        got = out.cpu().view(G, n)
        for gi in range(G):
            rows = part[gi * gl: (gi + 1) * gl]
            ref = R.fold_ref(rows, alpha, prior.view(G, n)[gi] if acc else None, R.wide_depth(rows.shape[0]))
            judge(TAG, f"{where} group {gi} ({rows.shape[0]} rows)", {"out": got[gi]}, {"out": ref})


@pytest.mark.parametrize("rows", [1, 511, 512, 513, 1025])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_colsum(dev, dtype, rows):
    for C in (1, 96, 255, 256, 257, 1000):
        gen = torch.Generator().manual_seed(rows * 1009 + C)
        x = R.signed((rows, C), gen).to(dtype)
        xd = x.to(dev)
        rpb, nparts = R.colsum_geometry(rows)
        assert nv.value("sv_colsum_nparts", rows, C) == nparts
        buf, part = _out_buf(dev, nparts * C, None)
        nv.call("sv_colsum", nv.ptr(xd), nv.dt(xd), rows, C, nv.ptr(part))
        where = f"colsum {'bf16' if dtype == BF else 'f32'} rows={rows} C={C}"
        _guards(buf, nparts * C, 0, where + " partials")
        ps, pS = R.colsum_parts(x.double(), rows)
        judge(TAG, where + " partials", {"part": part.cpu()}, {"part": (ps, (rpb - 1 + 2) * U24 * pS)})
        d = rpb - 1 + R.pair_depth(nparts, R.pair_cols(nparts, C))
        for acc in (False, True):
            prior = R.fold_inputs(1, C, seed=rows + C)[1]
            buf, out = _out_buf(dev, C, prior if acc else None)
            K.colsum_into(xd, out, accumulate=acc)
            _guards(buf, C, 0, where + " into")
            judge(TAG, f"{where} into acc={int(acc)}", {"out": out.cpu()},
                  {"out": R.fold_ref(x, 1.0, prior if acc else None, d)})
            if not acc:  # colsum() is colsum_into(accumulate=False) into a fresh output
                assert _same(K.colsum(xd), out)


# --------------------------------------------------------------------------------------- FlatAdamW over a toy arena
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(11)
        for i, shape in enumerate([(1,), (7,), (10,), (96, 64), (33,)]):
            self.register_parameter(f"w{i}", torch.nn.Parameter(torch.randn(*shape, generator=gen)))


def test_flat_adamw_toy_arena_five_clipped_steps(dev):
    """sizes 1, 7, 10, 96 x 64, 33 (arena offsets 0, 16, 32, 48, 6192; 6240 elements with the padding); the middle
    parameter is frozen for two steps, which cuts the arena into two runs and then gives it a step count of its own.
    Every step is judged from the GPU's own state before it."""
    lr, wd, max_norm = 1e-3, 1e-2, 1.0
    model = _Toy()
    twin = [p.detach().double().clone().requires_grad_(True) for p in model.parameters()]
    arena = FlatArena(model, dev, with_shadow=True)
    opt = FlatAdamW(arena, lr=lr, weight_decay=wd)
    topt = torch.optim.AdamW(twin, lr=lr, weight_decay=wd)
    frozen = arena.params[2]
    sizes = [p.numel() for p in arena.params]
    assert arena.offsets == [0, 16, 32, 48, 6192] and arena.numel == 6240
    real = torch.zeros(arena.numel, dtype=torch.bool)
    for o, n in zip(arena.offsets, sizes):
        real[o: o + n] = True
    gen = torch.Generator().manual_seed(12)
    steps = [0] * 5
    for it in range(5):
        frozen.requires_grad_(it >= 2)
        twin[2].requires_grad_(it >= 2)
        grad = torch.zeros(arena.numel)
        for i, (o, n) in enumerate(zip(arena.offsets, sizes)):
            if arena.params[i].requires_grad:
                grad[o: o + n] = torch.randn(n, generator=gen) * (0.02 if it % 2 else 3.0)
                steps[i] += 1
        arena.grad_flat.copy_(grad.to(dev))
        before = [t.cpu().clone() for t in (arena.param_flat, opt.exp_avg, opt.exp_avg_sq)]
        clip = K.grad_clip_coef(arena.grad_flat, max_norm)
        opt.step(grad_scale=clip[1:2])
        torch.cuda.synchronize()
        norm, coef = (float(x) for x in clip.cpu())
        _clip_judge(f"toy step {it + 1}", grad, max_norm, norm, coef)
        after = dict(p=arena.param_flat.cpu(), m=opt.exp_avg.cpu(), v=opt.exp_avg_sq.cpu())
        for i, (o, n) in enumerate(zip(arena.offsets, sizes)):
            e = o + (n + 15) // 16 * 16
            sl = slice(o, e)
            if not arena.params[i].requires_grad:
                for k, b in zip(("p", "m", "v"), before):
                    assert _same(after[k][sl], b[sl]), f"step {it + 1}: frozen parameter {i} changed in {k}"
                continue
            ref, bound = R.adamw_ref(before[0][sl], grad[sl], before[1][sl], before[2][sl], lr, wd, steps[i], coef)
            judge(TAG, f"toy step {it + 1} parameter {i} (its step {steps[i]})", {k: t[sl] for k, t in after.items()},
                  {k: (ref[k], bound[k]) for k in ref})
        for k, t in after.items():
            assert _plus_zero(t[~real]), f"step {it + 1}: arena padding not +0 in {k}"
        assert _same(arena.shadow_flat, after["p"].to(BF)), f"step {it + 1}: shadow != bf16(p)"
        for i, (t, o, n) in enumerate(zip(twin, arena.offsets, sizes)):
            t.grad = (grad[o: o + n].double() * coef).view_as(t) if t.requires_grad else None
        topt.step()
    assert opt._steps == steps == [5, 5, 3, 5, 5]
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert sorted(sd["state"]) == sorted(tsd["state"]) == [0, 1, 2, 3, 4]
    assert sd["param_groups"][0]["params"] == tsd["param_groups"][0]["params"]
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert sd["param_groups"][0][k] == tsd["param_groups"][0][k]
    for i in range(5):
        a, b = sd["state"][i], tsd["state"][i]
        assert sorted(a) == sorted(b) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(a["step"]) == float(b["step"]) == steps[i]
        assert a["exp_avg"].shape == b["exp_avg"].shape == model.get_parameter(f"w{i}").shape
        assert a["exp_avg_sq"].shape == b["exp_avg_sq"].shape
