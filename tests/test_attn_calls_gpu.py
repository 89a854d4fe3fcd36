"""The ViT attention calls one at a time, every output element against float64, streamed tiles included:
sv_attn_fwd / sv_attn_bwd (csrc/attn.hip, one pass, N <= 256) and sv_attn_stream_fwd / sv_attn_stream_bwd
(csrc/attn_stream.hip, 64-key tiles, N <= 2048).  tests/test_attn_gpu.py and tests/test_attn_stream_gpu.py hold the
same kernels to a whole-tensor relative L2, which sees a fault that is in every row and not one confined to a few rows
of a large N (profiles/attn_calls/mutations.txt); tests/test_vit_calls_gpu.py checks every other ViT call per element.

Each call runs through kernels.attn_fwd / attn_bwd / attn_stream_fwd / attn_stream_bwd (torch_arm=False) on operands in
sentinel-guarded buffers; outputs start as NaN; inputs must be bit-unchanged, the guards intact, and every call of
every test below runs twice on fresh buffers with bit-equal results (``_forward`` / ``_backward`` do all of this).
The streamed backward runs once more per case through the entry point itself with a guarded, NaN-filled workspace of
the test's own, so that D = rowsum(dout . out) is checked per element and must be all that is written there.  The
reference is float64 of the same function on the same operands (tests/_attn_ref.py).  For the backward ``out`` (bf16)
and ``lse`` (f32) are operands; it runs on CPU-made ones (the float64 forward, rounded: a backward defect cannot hide
behind a forward one) and on the forward kernel's own, the reference recomputed from those downloaded tensors:
test_backward on both sets at every case, the padded-row and both-pairs tests on the CPU-made set, the torch arm on its
own forward's.

The assertion is |got - ref| <= 2 x bound for EVERY element (the project's rule, as in tests/test_swin_calls_gpu.py),
lse within 1e-3.  The bound's terms, the inputs (uniform, shift, ramp and the three spike variants in which single keys
carry a row's weight) and the cases are derived in tests/_attn_ref.py's docstring; tests/test_attn_calls_cpu.py shows
that a float32 restatement stays within 1 x the bound and that each of ten faults leaves 4 x.  The worst ratio of
every output and its (image, head, token, column) are printed and recorded in profiles/attn_calls/parity.txt.

The torch arm (SV_ATTN=torch) is held to the same bound: it rounds the normalised P = exp(s - lse) to bf16 where the
kernels round e = exp(s - m) and divide by l afterwards; both are one bf16 rounding of relative size b on every
term of P V, the bound's b pv term, so it needs no term of its own."""
import pytest
import torch

import _attn_ref as ref
from spine_vision_amd import kernels as K

pytestmark = pytest.mark.gpu

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


def _pad(t, B, N, rows):
    """[B * N, c] -> [B * rows, c], NaN in the pad rows of every image"""
    if rows == N:
        return t
    p = torch.full((B, rows, t.shape[1]), NAN, dtype=t.dtype)
    p[:, :N] = t.view(B, N, -1)
    return p.view(B * rows, -1)


def _tokens(t, B, N, rows):
    return t.view(B, rows, -1)[:, :N].reshape(B * N, -1)


def _same(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _forward(pair, c, shape, rows=None, torch_arm=False):
    """the forward alone, run twice on fresh buffers with bit-equal results -> (out [B * rows, C], lse) device tensors"""
    first, again = (_forward_once(pair, c, shape, rows, torch_arm) for _ in range(2))
    assert _same(first[0], again[0]) and _same(first[1], again[1]), "two runs differ"
    return first


def _forward_once(pair, c, shape, rows, torch_arm):
    B, heads, N = shape
    rows = N if rows is None else rows
    qb = Buf(_pad(c["qkv"], B, N, rows), BF)
    ob, lb = Buf(torch.zeros(B * rows, heads * ref.HD), BF, fill=NAN), Buf(torch.zeros(B, heads, N), F32, fill=NAN)
    fn = K.attn_stream_fwd if pair == "stream" else K.attn_fwd
    fn(qb.v, B, N, heads, img_rows=rows, scale=c["scale"], out=ob.v, lse=lb.v, torch_arm=torch_arm)
    _intact(qkv=qb, out=ob, lse=lb)
    return ob.v, lb.v


def _backward(pair, c, shape, out, lse, rows=None, torch_arm=False, entry=False):
    """the backward alone on the operands ``out`` [B * N, C], ``lse`` (CPU float64 of bf16 / f32 values), run twice on
    fresh buffers with bit-equal results -> (dqkv, D) device tensors; ``entry``: sv_attn_stream_bwd itself with a
    workspace of the test's own (D: None otherwise)"""
    first, again = (_backward_once(pair, c, shape, out, lse, rows, torch_arm, entry) for _ in range(2))
    assert _same(first[0], again[0]) and (not entry or _same(first[1], again[1])), "two runs differ"
    return first


def _backward_once(pair, c, shape, out, lse, rows, torch_arm, entry):
    B, heads, N = shape
    rows = N if rows is None else rows
    qb, gb = Buf(_pad(c["qkv"], B, N, rows), BF), Buf(_pad(c["dout"], B, N, rows), BF)
    ob, lb = Buf(_pad(out, B, N, rows), BF), Buf(lse, F32)
    db = Buf(torch.zeros(B * rows, 3 * heads * ref.HD), BF, fill=NAN)
    bufs = dict(qkv=qb, dout=gb, out=ob, lse=lb, dqkv=db)
    if entry:
        wb = bufs["dws"] = Buf(torch.zeros(B, heads, N), F32, fill=NAN)
        K.call("sv_attn_stream_bwd", K.ptr(qb.v), K.ptr(ob.v), K.ptr(lb.v), K.ptr(gb.v), K.ptr(db.v), K.ptr(wb.v), B, N,
               rows, heads, ref.HD, c["scale"])
    else:
        fn = K.attn_stream_bwd if pair == "stream" else K.attn_bwd
        fn(qb.v, ob.v, lb.v, gb.v, B, N, heads, img_rows=rows, scale=c["scale"], dqkv=db.v, torch_arm=torch_arm)
    _intact(**bufs)
    return db.v, (wb.v if entry else None)


def _check(tag, name, got, want, bound, shape, cols=None):
    """print the worst error / bound and where it is, then hold every element to 2 x bound"""
    got = got.detach().cpu().double().reshape(want.shape)
    r = ref.ratio(got, want, bound)
    i = int(r.argmax())
    if cols is None:  # [B, heads, N]
        at = (i // (shape[1] * shape[2]), i // shape[2] % shape[1], i % shape[2])
    else:
        at = ref.where(i, shape, cols)
    print(f"attn_calls {tag} {name}: err {float((got - want).abs().max()):.3e} ratio {float(r.max()):.3f} at {at}")
    assert float(r.max()) <= 2.0, (name, float(r.max()), at, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
                                   float(bound.reshape(-1)[i]), f"{int((r > 2).sum())} of {r.numel()} elements beyond")


def _check_forward(tag, pair, c, shape, out, lse, where=""):
    f = c["fwd"]
    _check(tag, "out" + where, out, f["out"], f["out_bound_stream" if pair == "stream" else "out_bound"], shape, 1)
    _check(tag, "lse" + where, lse, f["lse"], torch.full_like(f["lse"], ref.LSE_ABS), shape)


def _check_backward(tag, b, shape, dqkv, D, where):
    C = shape[1] * ref.HD
    got = dqkv.detach().cpu().double()
    for j, name in enumerate(("dq", "dk", "dv")):  # one line per gradient; the location is in dqkv's columns
        sel = torch.zeros(3 * C, dtype=torch.bool)
        sel[j * C:(j + 1) * C] = True
        r = ref.ratio(got, b["dqkv"], b["dqkv_bound"]).masked_fill(~sel, 0.0)
        i = int(r.argmax())
        print(f"attn_calls {tag} {name} [{where}]: err {float((got - b['dqkv'])[:, sel].abs().max()):.3e} "
              f"ratio {float(r.max()):.3f} at {ref.where(i, shape, 3)}")
    _check(tag, f"dqkv [{where}]", dqkv, b["dqkv"], b["dqkv_bound"], shape, 3)
    if D is not None:
        _check(tag, f"D [{where}]", D, b["D"], b["D_bound"], shape)


@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_forward(case):
    pair, shape, variant = case
    c = ref.calls_case(shape, variant)
    out, lse = _forward(pair, c, shape)
    _check_forward(ref.case_id(case), pair, c, shape, out, lse)


@pytest.mark.parametrize("operands", ["cpu", "kernel"])
@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_backward(case, operands):
    pair, shape, variant = case
    c = ref.calls_case(shape, variant)
    if operands == "cpu":
        out, lse, b = c["out"], c["lse"], c["bwd"]
    else:
        o, l = _forward(pair, c, shape)
        out, lse = o.cpu().double(), l.cpu().double()
        b = ref.attn_bwd_ref(c["qkv"], out, lse, c["dout"], shape, c["scale"])
    dqkv, _ = _backward(pair, c, shape, out, lse)
    D = None
    if pair == "stream":  # the entry point with the test's own workspace: the same gradients, and D per element
        direct, D = _backward(pair, c, shape, out, lse, entry=True)
        assert _same(dqkv, direct), "kernels.attn_stream_bwd and sv_attn_stream_bwd differ"
    _check_backward(ref.case_id(case), b, shape, dqkv, D, operands)


@pytest.mark.parametrize("pair,shape", [("stream", (2, 2, 257)), ("onepass", (2, 3, 197))], ids=["stream-2x2x257",
                                                                                                  "onepass-2x3x197"])
def test_padded_rows(pair, shape):
    """img_rows = the next multiple of 8 plus 8 (the ViT module's layout), NaN in the pad rows of qkv, dout and out:
    token rows under the per-element rule, pad rows of out and dqkv exactly zero."""
    B, heads, N = shape
    rows = (N + 7) // 8 * 8 + 8
    c = ref.calls_case(shape, "uniform")
    tag = f"{pair}-{'x'.join(map(str, shape))}-rows{rows}"
    out, lse = _forward(pair, c, shape, rows)
    assert not out.view(B, rows, -1)[:, N:].any(), "pad rows of out must be written as zeros"
    _check_forward(tag, pair, c, shape, _tokens(out, B, N, rows), lse, " [padded]")
    dqkv, _ = _backward(pair, c, shape, c["out"], c["lse"], rows)
    assert not dqkv.view(B, rows, -1)[:, N:].any(), "pad rows of dqkv must be written as zeros"
    D = None
    if pair == "stream":
        direct, D = _backward(pair, c, shape, c["out"], c["lse"], rows, entry=True)
        assert _same(dqkv, direct)
    _check_backward(tag, c["bwd"], shape, _tokens(dqkv, B, N, rows), D, "padded")


@pytest.mark.parametrize("shape,variant", [((2, 3, 197), "uniform"), ((2, 3, 197), "spike_edges"),
                                           ((1, 2, 129), "spike_edges")],
                         ids=["2x3x197-uniform", "2x3x197-spike_edges", "1x2x129-spike_edges"])
def test_both_pairs_on_the_same_operands(shape, variant):
    """ViT reaches the streamed pair at small N under SV_ATTN=stream: each pair against the reference, on the same
    operands (no bitwise claim between them)."""
    c = ref.calls_case(shape, variant)
    for pair in ("onepass", "stream"):
        tag = f"both-{pair}-{'x'.join(map(str, shape))}-{variant}"
        out, lse = _forward(pair, c, shape)
        _check_forward(tag, pair, c, shape, out, lse)
        dqkv, _ = _backward(pair, c, shape, c["out"], c["lse"])
        _check_backward(tag, c["bwd"], shape, dqkv, None, "cpu")


@pytest.mark.parametrize("pair,shape,variant", [("onepass", (2, 3, 197), "uniform"), ("onepass", (2, 3, 197), "spike_edges"),
                                                ("stream", (2, 2, 65), "spike_edges")],
                         ids=["onepass-2x3x197-uniform", "onepass-2x3x197-spike_edges", "stream-2x2x65-spike_edges"])
def test_torch_arm_per_element(pair, shape, variant):
    """torch_arm=True through the same wrappers under the same rule (the module docstring says why the kernels' bound
    holds for it); its backward on its own forward's out and lse, the reference recomputed from them."""
    c = ref.calls_case(shape, variant)
    tag = f"torch-{pair}-{'x'.join(map(str, shape))}-{variant}"
    out, lse = _forward(pair, c, shape, torch_arm=True)
    _check_forward(tag, pair, c, shape, out, lse)
    o, l = out.cpu().double(), lse.cpu().double()
    b = ref.attn_bwd_ref(c["qkv"], o, l, c["dout"], shape, c["scale"])
    dqkv, _ = _backward(pair, c, shape, o, l, torch_arm=True)
    _check_backward(tag, b, shape, dqkv, None, "torch arm")
