"""The window-attention calls of csrc/swin.hip one at a time, every output element against float64, the window walk
included: sv_swin_bias_expand, sv_winattn_fwd, sv_winattn_bwd, sv_swin_bias_grad.

A workgroup is one wave that handles the windows part, part + nparts, ... of one head, nparts = min(1024 // heads,
B * nW).  tests/test_winattn_gpu.py and the Swin model tests never give a wave a second window; training does (224 px,
swin_tiny stage 0, from batch 6 on).  The walking shapes below are the smallest that reach each form of that loop;
each asserts B * nW > nparts and its walk depths, from the restated nparts and from sv_winattn_bwd_nparts.

Each call runs alone on operands in sentinel-guarded buffers; outputs and partials start as NaN, dtable as a non-zero
prior that the fold adds onto; inputs must be bit-unchanged, the guards intact, two runs bit-equal.  The reference is
float64 of the same function on the same operands (tests/_swin_ref.py, written with torch.roll / window_partition and
timm's slice-built mask, not the kernels' index formula).  For the backward, ``out`` (bf16) and ``lse`` (f32) are
operands: D = rowsum(dout . out) from the given out, P = exp(score - lse) from the given lse.  It runs twice: on
CPU-made operands (the float64 forward, rounded) and on the forward kernel's own outputs, the reference evaluated on
those downloaded tensors.  dbias_part[p] is held against the float64 sum of T over exactly the windows p, p + nparts,
...; dtable against the float64 fold of the downloaded partials and against prior + the sum of T over all windows.

The assertion is |got - ref| <= 2 x bound for EVERY element (the factor 2 is the project's rule, as in
tests/test_swin_gpu.py and tests/test_vit_calls_gpu.py).  u = 2^-24 (f32), b = 2^-8 (bf16), tiny = 2^-126.

Bound, from the kernels' order of operations (second-order products of these terms are left to the factor 2):
  score     ds = 32 u scale sum_d |q_d||k_d|     a 32-term f32 MFMA sum of exact bf16 products
               + u |scale q.k + bias|             the fma with the bias
               + u |score|                        the addition of the mask (shifted blocks only)
  exp       e_k = exp2((s_k - m) log2 e): relative error ds_k + 3 u |s_k - m| (the subtraction, the rounded constant
            and the product form the argument in f32) + 2^-21 for the hardware exp2 (documented at 1 ulp; at these
            inputs the whole term stays near 1e-6, three orders of magnitude below b = 3.9e-3); absolute tiny where
            the result is a flushed denormal: masked pairs underflow in f32 and not in float64, so there the bound is
            absolute, never relative.
  out       with pv = sum_k p_k |v_kd| and dmax the row's largest relative error of an e_k (m is common to the row
            and cancels in e / l):
               b pv                               P rounded to bf16 before P V
               + 2 dmax pv                        the softmax's sensitivity to the score and exp errors
               + 2 N u pv                         f32 accumulation over N keys, in P V and in l
               + 3 u |out|                        1 / l and the product with it
               then the bf16 store: b (|out| + the above) + tiny
  lse       1e-3 absolute, the project's existing bound (the fast log's accuracy cannot be read from the code); the
            measured maximum is printed and recorded in profiles/swin_calls/parity.txt (7.5e-7 at the uniform
            inputs, 1.7e-6 at table amplitude 16, 1.3e-5 at scores near +-102)
  P (bwd)   dP_ = P (ds + 3 u |score - lse| + 2^-21) + tiny
  T         dT = dP_ |dP - D|                     P's error
               + P 32 u (sum_d |do_d||v_d| + sum_d |do_d||o_d|)   dP's MFMA sum and D's 32-term fma chain
               + 2 u |T| + tiny                   the subtraction and the product
  dS        ddS = (scale dT + u |dS|)(1 + b) + b |dS| + tiny      the product with scale, then bf16 as MFMA operand
  dq / dk   sum ddS |k| (|q|) + N u sum |dS||k| (|q|), then the bf16 store as for out
  dv        sum (dP_ (1 + b) + b P) |do| + N u sum P |do|, then the bf16 store
  dbias_part[p]   the sum of dT over the part's windows + depth u sum |T|: one f32 addition per window of the walk
  dtable    folding given partials: (nparts + w*w) u sum |partial| (nparts additions per lane, then up to w*w in lane
            order) + u |dtable| for the prior; from the operands of the backward: the partials' bounds on top.

Shapes (B, H, W, w, shift, heads): the walking ones (windows / nparts / depths): (1,12,12,2,1,32) 36 / 32 / {1,2}, N = 4
below one tile, shifted; (5,8,8,4,2,128) 20 / 8 / {2,3}, a ragged last round; (3,28,28,7,3,24) 48 / 42 / {1,2}, the
two-tile ragged window at the stage-3 head count, masked windows in the second round; (2,32,32,8,4,64) 32 / 16 / {2},
full 64-token windows; (6,56,56,7,3|0,3) 384 / 341 / {1,2}, swin_tiny's stage 0 at the smallest batch that walks.  And
every non-walking case of tests/test_winattn_gpu.py with its table16 / shift_up / shift_down inputs."""
import pytest
import torch

import _swin_ref as ref
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

pytestmark = pytest.mark.gpu

# shape -> the walk depths it must reach
WALKING = {(1, 12, 12, 2, 1, 32): {1, 2}, (5, 8, 8, 4, 2, 128): {2, 3}, (3, 28, 28, 7, 3, 24): {1, 2},
           (2, 32, 32, 8, 4, 64): {2}, (6, 56, 56, 7, 3, 3): {1, 2}, (6, 56, 56, 7, 0, 3): {1, 2}}
PLAIN = [(1, 1, 1, 1, 0, 1), (2, 2, 2, 2, 0, 1), (1, 4, 4, 2, 1, 1), (2, 7, 7, 7, 0, 3), (2, 14, 14, 7, 0, 3),
         (2, 14, 14, 7, 3, 3), (1, 28, 14, 7, 3, 2), (2, 8, 8, 8, 0, 2), (1, 16, 16, 8, 4, 4), (1, 14, 14, 7, 3, 24)]
CASES = [(s, "uniform") for s in list(WALKING) + PLAIN] + [((2, 14, 14, 7, 3, 3), "table16"),
                                                            ((1, 14, 14, 7, 3, 2), "shift_up"),
                                                            ((1, 14, 14, 7, 3, 2), "shift_down")]


def _id(case):
    return "x".join(map(str, case[0])) + ("" if case[1] == "uniform" else "-" + case[1])


IDS = [_id(c) for c in CASES]
SENTINEL = -7.0
GUARD = 256
BF = torch.bfloat16
F32 = torch.float32
NAN = float("nan")


class Buf:
    """a tensor inside a larger sentinel-filled buffer"""

    def __init__(self, t, dtype, fill=None):
        self.whole = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device="cuda", dtype=dtype)
        self.v = self.whole[GUARD:GUARD + t.numel()].view(t.shape)
        self.v.copy_(t.to("cuda", dtype)) if fill is None else self.v.fill_(fill)
        self.start = None if fill is not None else self.v.clone()

    def intact(self):
        ok = bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[-GUARD:] == SENTINEL).all())
        return ok and (self.start is None or torch.equal(self.v.view(torch.uint8), self.start.view(torch.uint8)))


def _intact(**bufs):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"{name}: a guard was overwritten or an input modified"


def _pad(t, rows):
    return torch.cat([t, torch.full((rows - t.shape[0], t.shape[1]), NAN, dtype=t.dtype)]) if rows > t.shape[0] else t


def _expand(table, w, heads):
    tb, bb = Buf(table, F32), Buf(torch.zeros(heads, w * w, w * w), F32, fill=NAN)
    nv.call("sv_swin_bias_expand", nv.ptr(tb.v), nv.ptr(bb.v), w, heads)
    _intact(table=tb, bias=bb)
    return bb.v


def _forward(c, geom, rows=None):
    """sv_winattn_fwd alone -> (out, lse) device tensors"""
    B, H, W, w, shift, heads = geom
    n, C, nwin = B * H * W, heads * 32, B * (H // w) * (W // w)
    rows = n if rows is None else rows
    qb, bb = Buf(_pad(c["qkv"], rows), BF), Buf(c["bias"], F32)
    ob, lb = Buf(torch.zeros(rows, C), BF, fill=NAN), Buf(torch.zeros(nwin, heads, w * w), F32, fill=NAN)
    nv.call("sv_winattn_fwd", nv.ptr(qb.v), nv.ptr(ob.v), nv.ptr(lb.v), nv.ptr(bb.v), B, H, W, w, shift, heads, 32,
            c["scale"], rows)
    _intact(qkv=qb, bias=bb, out=ob, lse=lb)
    return ob.v, lb.v


def _backward(c, geom, out, lse, rows=None):
    """sv_winattn_bwd alone, then sv_swin_bias_grad onto the prior -> (dqkv, part, dtable) device tensors"""
    B, H, W, w, shift, heads = geom
    n, C, N = B * H * W, heads * 32, w * w
    rows = n if rows is None else rows
    nparts = c["nparts"]
    qb, gb, bb = Buf(_pad(c["qkv"], rows), BF), Buf(_pad(c["dout"], rows), BF), Buf(c["bias"], F32)
    ob, lb = Buf(_pad(out, rows), BF), Buf(lse, F32)
    db, pb = Buf(torch.zeros(rows, 3 * C), BF, fill=NAN), Buf(torch.zeros(nparts, heads, N, N), F32, fill=NAN)
    nv.call("sv_winattn_bwd", nv.ptr(qb.v), nv.ptr(ob.v), nv.ptr(lb.v), nv.ptr(gb.v), nv.ptr(bb.v), nv.ptr(db.v),
            nv.ptr(pb.v), B, H, W, w, shift, heads, 32, c["scale"], rows)
    _intact(qkv=qb, dout=gb, bias=bb, out=ob, lse=lb, dqkv=db, dbias_part=pb)
    tb = Buf(c["prior"], F32)
    tb.start = None  # the one buffer that is read and written
    part_in = Buf(pb.v.cpu(), F32)
    nv.call("sv_swin_bias_grad", nv.ptr(part_in.v), nv.ptr(tb.v), nparts, w, heads, 1)
    _intact(dbias_part=part_in, dtable=tb)
    return db.v, pb.v, tb.v


def _check(case, name, got, want, bound):
    """print the figures, then hold every element to 2 x bound"""
    got = got.detach().cpu().double()
    r = ref.ratio(got, want, bound)
    i = int(r.argmax())
    print(f"swin_calls {_id(case)} {name}: err {float((got - want).abs().max()):.3e} ratio {float(r.max()):.3f}")
    assert float(r.max()) <= 2.0, (name, float(r.max()), i, float(got.view(-1)[i]), float(want.reshape(-1)[i]),
                                   float(bound.reshape(-1)[i]))


def _check_backward(case, c, geom, b, dqkv, part, dtable, where):
    n, w = geom[0] * geom[1] * geom[2], geom[3]
    _check(case, f"dqkv [{where}]", dqkv[:n], b["dqkv"], b["dqkv_bound"])
    _check(case, f"dbias_part [{where}]", part, b["part"], b["part_bound"])
    _check(case, f"dtable fold [{where}]", dtable, *ref.bias_grad_ref(part.cpu(), c["prior"], w, True))
    _check(case, f"dtable [{where}]", dtable, *ref.dtable_chain_ref(b, c["prior"], w, c["nparts"]))


def _assert_walk(geom):
    """a walking shape has more windows than waves per head and reaches exactly the depths listed for it"""
    B, H, W, w, shift, heads = geom
    total = B * (H // w) * (W // w)
    nparts = min(1024 // heads, total)
    assert nparts == ref.win_nparts(B, H, W, w, heads) == nv.value("sv_winattn_bwd_nparts", B, H, W, w, heads)
    assert total > nparts
    assert ref.walk_depths(total, nparts) == WALKING[geom]


@pytest.mark.parametrize("geom", list(WALKING), ids=["x".join(map(str, g)) for g in WALKING])
def test_the_shape_walks(geom):
    _assert_walk(geom)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bias_expand_and_forward(case):
    geom, variant = case
    if geom in WALKING:
        _assert_walk(geom)
    c = ref.calls_case(geom, variant)
    w, heads, n = geom[3], geom[5], geom[0] * geom[1] * geom[2]
    bias = _expand(c["table"], w, heads)
    assert torch.equal(bias.cpu().double(), c["bias"]), "the dense bias is not the table through timm's index"
    out, lse = _forward(c, geom)
    out2, lse2 = _forward(c, geom)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(lse, lse2), "two runs differ"
    f = c["fwd"]
    _check(case, "out", out[:n], f["out"], f["out_bound"])
    _check(case, "lse", lse, f["lse"], torch.full_like(f["lse"], ref.LSE_ABS))


@pytest.mark.parametrize("operands", ["cpu", "kernel"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_and_bias_grad(case, operands):
    geom, variant = case
    if geom in WALKING:
        _assert_walk(geom)
    c = ref.calls_case(geom, variant)
    if operands == "cpu":
        out, lse, b = c["out"], c["lse"], c["bwd"]
    else:
        o, l = _forward(c, geom)
        out, lse = o.cpu().double(), l.cpu().double()
        b = ref.winattn_bwd_ref(c["qkv"], out, lse, c["dout"], c["bias"], geom, c["scale"], c["nparts"])
    dqkv, part, dtable = _backward(c, geom, out, lse)
    again = _backward(c, geom, out, lse)
    for x, y in zip((dqkv, part, dtable), again):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "two runs differ"
    _check_backward(case, c, geom, b, dqkv, part, dtable, operands)


def test_tail_rows_are_zero_and_never_read():
    """rows_total > B*H*W on a walking shape (144 -> 152 rows): NaN in the tail rows of qkv, dout and (for the
    backward) out; the real rows bit-equal the unpadded call and stay inside the bound; the tails of out and dqkv are
    zeros."""
    case = ((1, 12, 12, 2, 1, 32), "uniform")
    geom = case[0]
    _assert_walk(geom)
    c = ref.calls_case(*case)
    n, rows = 144, 152
    out, lse = _forward(c, geom, rows)
    plain_out, plain_lse = _forward(c, geom)
    assert not out[n:].any(), "tail of out not zero"
    assert torch.equal(out[:n].view(torch.int16), plain_out.view(torch.int16)) and torch.equal(lse, plain_lse)
    _check(case, "out [tail]", out[:n], c["fwd"]["out"], c["fwd"]["out_bound"])
    dqkv, part, dtable = _backward(c, geom, c["out"], c["lse"], rows)  # _pad gives out a NaN tail
    plain = _backward(c, geom, c["out"], c["lse"])
    assert not dqkv[n:].any(), "tail of dqkv not zero"
    for x, y in zip((dqkv[:n], part, dtable), plain):
        assert torch.equal(x.view(torch.uint8), y.contiguous().view(torch.uint8))
    _check_backward(case, c, geom, c["bwd"], dqkv, part, dtable, "tail")


def test_kernels_py_wrappers_are_the_entry_points():
    geom = (1, 12, 12, 2, 1, 32)
    B, H, W, w, shift, heads = geom
    c = ref.calls_case(geom)
    table, qkv, dout = c["table"].to("cuda", F32), c["qkv"].to("cuda", BF), c["dout"].to("cuda", BF)
    bias = K.swin_bias_expand(table, w)
    assert torch.equal(bias, _expand(c["table"], w, heads))
    out, lse = K.winattn_fwd(qkv, bias, B, H, W, w, shift, heads, scale=c["scale"], torch_arm=False)
    o, l = _forward(c, geom)
    assert torch.equal(out.view(torch.int16), o.view(torch.int16)) and torch.equal(lse, l)
    dqkv, part = K.winattn_bwd(qkv, out, lse, dout, bias, B, H, W, w, shift, heads, scale=c["scale"], torch_arm=False)
    dtable = K.swin_bias_grad(part, c["prior"].to("cuda", F32), w, accumulate=True)
    want = _backward(c, geom, o.cpu().double(), l.cpu().double())
    assert part.shape[0] == c["nparts"]
    for x, y in zip((dqkv, part, dtable), want):
        assert torch.equal(x.view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "store"])
@pytest.mark.parametrize("nparts,w,heads", [(341, 7, 3), (42, 7, 24)])
def test_bias_grad_alone_at_production_part_counts(nparts, w, heads, accumulate):
    """random partials in [-1, 1] at the part counts of swin_tiny's stage 0 (341) and stage 3 (42 = 1024 // 24)"""
    g = torch.Generator().manual_seed(nparts * 10 + heads)
    N = w * w
    part = torch.rand(nparts, heads, N, N, generator=g) * 2 - 1
    prior = torch.rand((2 * w - 1) ** 2, heads, generator=g) * 2 - 1
    got = []
    for _ in range(2):
        pb = Buf(part, F32)
        tb = Buf(prior, F32) if accumulate else Buf(prior, F32, fill=NAN)
        tb.start = None
        nv.call("sv_swin_bias_grad", nv.ptr(pb.v), nv.ptr(tb.v), nparts, w, heads, int(accumulate))
        _intact(dbias_part=pb, dtable=tb)
        got.append(tb.v)
    assert torch.equal(got[0], got[1]), "two runs differ"
    case = ((nparts, w, heads), "accumulate" if accumulate else "store")
    print(f"swin_calls bias_grad nparts {nparts} w {w} heads {heads}:")
    _check(case, "dtable alone", got[0], *ref.bias_grad_ref(part, prior, w, accumulate))


def test_torch_arm_per_element():
    """The SV_WINATTN=torch arm on a shifted case under the same rule; its backward returns one part, the sum of T
    over all windows."""
    case = ((2, 14, 14, 7, 3, 3), "uniform")
    geom = case[0]
    B, H, W, w, shift, heads = geom
    c = ref.calls_case(*case)
    qkv, dout, bias = c["qkv"].to("cuda", BF), c["dout"].to("cuda", BF), c["bias"].to("cuda", F32)
    out, lse = K.winattn_fwd(qkv, bias, B, H, W, w, shift, heads, scale=c["scale"], torch_arm=True)
    _check(case, "out [torch arm]", out, c["fwd"]["out"], c["fwd"]["out_bound"])
    _check(case, "lse [torch arm]", lse, c["fwd"]["lse"], torch.full_like(c["fwd"]["lse"], ref.LSE_ABS))
    o, l = out.cpu().double(), lse.cpu().double()
    b = ref.winattn_bwd_ref(c["qkv"], o, l, c["dout"], c["bias"], geom, c["scale"], 1)
    dqkv, part = K.winattn_bwd(qkv, out, lse, dout, bias, B, H, W, w, shift, heads, scale=c["scale"], torch_arm=True)
    assert part.shape[0] == 1
    dtable = K.swin_bias_grad(part, c["prior"].to("cuda", F32), w, accumulate=True)
    _check(case, "dqkv [torch arm]", dqkv, b["dqkv"], b["dqkv_bound"])
    _check(case, "dbias_part [torch arm]", part, b["part"], b["part_bound"])
    _check(case, "dtable fold [torch arm]", dtable, *ref.bias_grad_ref(part.cpu(), c["prior"], w, True))
    _check(case, "dtable [torch arm]", dtable, *ref.dtable_chain_ref(b, c["prior"], w, 1))
