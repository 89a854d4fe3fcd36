"""The fused multi-head attention kernels (csrc/attn.hip: sv_attn_fwd / sv_attn_bwd) against float64 softmax
attention and its autograd over the same bf16-rounded qkv and dout.

Shapes (B, heads, N): every boundary of the 32-wide MFMA tiles and of the 128-query forward workgroup (1, 16, 17, 33,
64, 256) and the real ViT shape (197 tokens; 3 and 16 heads).

Bound.  A second CPU restatement rounds P, O, dS and the gradients to bf16 where the kernel does; its distance from
float64 is the error that rounding alone causes.  Each of out, dq, dk, dv must be within max(1e-3, 3 x that) in
relative L2 of float64 (the rule of test_family_fp32_forward_backward); lse within 1e-3 absolute.  At N = 1 the
softmax is the constant 1, so dq and dk are exactly zero in float64; the kernel computes them as P (dP - D) with dP
and D two f32 sums of the same 64 products in different orders (terms below 1.5, so |dP - D| < 64 * 1.5 * 2^-23 ~
1e-5, times scale 0.125 and |k|, |q| < 1.5): the bound there is 5e-6 absolute.

Inputs: q, k uniform in [-1.5, 1.5] (scaled scores within about +-4: no softmax row underflows in f32 or f64), v and
dout uniform in [-1, 1].  Two more input sets at (1, 2, 129) shift every score of a head by +-98 and leave softmax
unchanged in exact arithmetic: q[..., 0] = 28 for every query and k[..., 0] = +28 ("shift_up") or -28 ("shift_down")
for every key, both exact in bf16, so the scaled scores lie in [94, 102] or [-102, -94] and lse is about +-98 + log N:
a forward without the max subtraction overflows or underflows, a backward that mishandles a large lse loses P.  Same
checks and bound rule; each own error of these two must stay below 2e-2 (measured on the CPU at N = 65 and 257: out
2.4e-3, dq 1.2e-2, dk 2.2e-3, dv 2.5e-3), so that the 3 x own bound cannot become vacuous.  The first scaled-score
line above describes the uniform sets only.  Operands and outputs sit inside larger buffers filled with a sentinel; the
exact-size views are passed and the sentinel elements before and after must be unchanged.

The ViT module keeps each image's tokens in rows padded to a multiple of 8 (DESIGN.md "ViT / DeiT-III"), so the
GEMM and LayerNorm row counts stay multiples of 8 as they always were; the padded form of the kernels is checked
here: token rows bitwise equal to the unpadded call, pad rows of out and dqkv exactly zero and never read (NaN in the
pad rows of every input)."""
import functools

import pytest
import torch

from spine_vision_amd import kernels as K

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 16), (2, 3, 17), (1, 2, 33), (3, 3, 64), (2, 3, 197), (1, 16, 197), (2, 2, 256)]
CASES = [(s, "uniform") for s in SHAPES] + [((1, 2, 129), "shift_up"), ((1, 2, 129), "shift_down")]
IDS = ["x".join(map(str, s)) + ("" if v == "uniform" else "-" + v) for s, v in CASES]
SHIFT = 28.0  # exact in bf16; 28 * 28 * SCALE = 98
SCALE = 0.125
SENTINEL = -7.0  # exactly representable in bf16 and f32
GUARD = 256  # sentinel elements on either side (keeps the views 16-byte aligned)


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _split(qkv, B, N, heads):
    """[B*N, 3*heads*64] -> q, k, v [B, heads, N, 64]"""
    v = qkv.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return v[0], v[1], v[2]


def _merge(t):
    """[B, heads, N, 64] -> [B*N, heads*64]"""
    B, h, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, h * 64)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _case(case):
    """bf16-rounded qkv / dout (float64 values), the float64 reference and the rounding-only restatement's error;
    computed once per case on the CPU, shared by the tests, never modified."""
    (B, heads, N), variant = case
    g = torch.Generator().manual_seed(7919 * B + 131 * heads + N)
    C = heads * 64
    qkv = torch.rand(B * N, 3 * C, generator=g, dtype=torch.float64) * 2 - 1
    qkv.view(B * N, 3, C)[:, :2] *= 1.5
    if variant != "uniform":
        qk = qkv.view(B, N, 3, heads, 64)
        qk[:, :, 0, :, 0] = SHIFT
        qk[:, :, 1, :, 0] = SHIFT if variant == "shift_up" else -SHIFT
    qkv = _bf(qkv)
    dout = _bf(torch.rand(B * N, C, generator=g, dtype=torch.float64) * 2 - 1)
    x = qkv.clone().requires_grad_(True)
    q, k, v = _split(x, B, N, heads)
    s = q @ k.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(s, -1)
    out = _merge(torch.softmax(s, -1) @ v)
    out.backward(dout)
    ref = dict(out=out.detach(), lse=lse.detach(), dqkv=x.grad)
    # the restatement: float64 arithmetic, bf16 rounding at the kernel's rounding points
    q, k, v = _split(qkv, B, N, heads)
    do = _split(dout.repeat(1, 3), B, N, heads)[0]
    p = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    o = _bf(_bf(p) @ v)
    dp = do @ v.transpose(-1, -2)
    ds = _bf(p * (dp - (do * o).sum(-1, keepdim=True)) * SCALE)
    dq, dk, dv = _bf(ds @ k), _bf(ds.transpose(-1, -2) @ q), _bf(_bf(p).transpose(-1, -2) @ do)
    rq, rk, rv = _split(ref["dqkv"], B, N, heads)
    own = dict(out=_rel(_merge(o), ref["out"]), dq=_rel(dq, rq), dk=_rel(dk, rk), dv=_rel(dv, rv))
    return dict(qkv=qkv, dout=dout, ref=ref, own=own)


def _guarded(t, dev, dtype):
    """t inside a larger sentinel-filled buffer: (the exact-size view, the whole buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=dev, dtype=dtype)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dev, dtype))
    return view, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _run(dev, qkv, dout, B, N, heads, *, torch_arm=False, img_rows=None):
    """forward and backward through kernels.py on guarded buffers -> out, lse, dqkv (device views)"""
    rows = N if img_rows is None else img_rows
    bf = torch.bfloat16
    qv, qb = _guarded(qkv, dev, bf)
    dv_, db = _guarded(dout, dev, bf)
    ov, ob = _guarded(torch.zeros(B * rows, heads * 64), dev, bf)
    lv, lb = _guarded(torch.zeros(B, heads, N), dev, torch.float32)
    gv, gb = _guarded(torch.zeros(B * rows, 3 * heads * 64), dev, bf)
    ov.fill_(SENTINEL), lv.fill_(SENTINEL), gv.fill_(SENTINEL)  # every element must be written
    K.attn_fwd(qv, B, N, heads, img_rows=img_rows, scale=SCALE, out=ov, lse=lv, torch_arm=torch_arm)
    K.attn_bwd(qv, ov, lv, dv_, B, N, heads, img_rows=img_rows, scale=SCALE, dqkv=gv, torch_arm=torch_arm)
    torch.cuda.synchronize()
    for name, b_ in (("qkv", qb), ("dout", db), ("out", ob), ("lse", lb), ("dqkv", gb)):
        assert _guards_intact(b_), f"sentinel around {name} overwritten"
    assert torch.equal(qv.cpu().double(), qkv) and torch.equal(dv_.cpu().double(), dout), "an input was modified"
    return ov, lv, gv


def _errors(case, out, lse, dqkv):
    (B, heads, N), _ = case
    c = _case(case)
    ref = c["ref"]
    gq, gk, gv = _split(dqkv.cpu().double(), B, N, heads)
    rq, rk, rv = _split(ref["dqkv"], B, N, heads)
    e = dict(out=_rel(out.cpu(), ref["out"]), dv=_rel(gv, rv))
    if N == 1:  # dq = dk = 0 exactly in float64 (module docstring): absolute
        e["dq_abs"], e["dk_abs"] = float(gq.abs().max()), float(gk.abs().max())
    else:
        e["dq"], e["dk"] = _rel(gq, rq), _rel(gk, rk)
    e["lse_abs"] = float((lse.cpu().double() - ref["lse"]).abs().max())
    return e


def _bound(case, name):
    return max(1e-3, 3.0 * _case(case)["own"][name])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_against_float64(dev, case):
    (B, heads, N), _ = case
    c = _case(case)
    out, lse, dqkv = _run(dev, c["qkv"], c["dout"], B, N, heads)
    e = _errors(case, out, lse, dqkv)
    print(f"[attn] {case}: kernel " + ", ".join(f"{k} {v:.3e}" for k, v in e.items())
          + " | rounding-only restatement " + ", ".join(f"{k} {v:.3e}" for k, v in c["own"].items()))
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
    if case[1] != "uniform":
        assert all(v < 2e-2 for v in c["own"].values()), ("the restatement's own error makes the bound vacuous", c["own"])
    for name in ("out", "dq", "dk", "dv"):
        if name in e:
            assert e[name] <= _bound(case, name), (name, e[name], _bound(case, name))
    if N == 1:
        assert e["dq_abs"] <= 5e-6 and e["dk_abs"] <= 5e-6, e
    assert e["lse_abs"] <= 1e-3, e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_bitwise_run_to_run_and_batch_independent(dev, case):
    (B, heads, N), _ = case
    c = _case(case)
    a = _run(dev, c["qkv"], c["dout"], B, N, heads)
    b = _run(dev, c["qkv"], c["dout"], B, N, heads)
    for x, y, name in zip(a, b, ("out", "lse", "dqkv")):
        assert torch.equal(x, y), f"{name} differs run to run"
    # the last image alone (its rows end the allocation in both calls)
    i = B - 1
    one = _run(dev, c["qkv"][i * N:(i + 1) * N], c["dout"][i * N:(i + 1) * N], 1, N, heads)
    assert torch.equal(one[0], a[0][i * N:(i + 1) * N]), "out depends on the batch"
    assert torch.equal(one[1], a[1][i:i + 1]), "lse depends on the batch"
    assert torch.equal(one[2], a[2][i * N:(i + 1) * N]), "dqkv depends on the batch"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_torch_arm_no_further_from_float64(dev, case):
    """SV_ATTN=torch (kernels.attn_*(torch_arm=True)): the same maths as torch ops on the same buffers."""
    (B, heads, N), _ = case
    c = _case(case)
    e_hip = _errors(case, *_run(dev, c["qkv"], c["dout"], B, N, heads))
    e_t = _errors(case, *_run(dev, c["qkv"], c["dout"], B, N, heads, torch_arm=True))
    print(f"[attn] {case}: torch arm " + ", ".join(f"{k} {v:.3e}" for k, v in e_t.items()))
    for name, v in e_t.items():
        if name.endswith("_abs"):
            assert v <= (1e-3 if name == "lse_abs" else 5e-6), (name, v)
        else:
            assert v <= 3.0 * max(e_hip[name], 1e-3 / 3), (name, v, e_hip[name])


@pytest.mark.parametrize("shape", [(2, 3, 17), (2, 3, 197), (2, 2, 256)], ids=["2x3x17", "2x3x197", "2x2x256"])
def test_attn_padded_rows(dev, shape):
    """img_rows > N (the ViT module's layout): token rows bitwise the unpadded call's, pad rows of out and dqkv exactly
    zero, pad rows of the inputs (NaN here) never read."""
    B, heads, N = shape
    rows = (N + 7) // 8 * 8 + 8
    c = _case((shape, "uniform"))
    ref = _run(dev, c["qkv"], c["dout"], B, N, heads)

    def pad(t):
        p = torch.full((B, rows, t.shape[1]), float("nan"), dtype=torch.float64)
        p[:, :N] = t.view(B, N, -1)
        return p.view(B * rows, -1)

    qkv_p, dout_p = pad(c["qkv"]), pad(c["dout"])
    bf = torch.bfloat16
    qv = qkv_p.to(dev, bf)
    dv_ = dout_p.to(dev, bf)
    out, lse = K.attn_fwd(qv, B, N, heads, img_rows=rows, scale=SCALE, torch_arm=False)
    dqkv = K.attn_bwd(qv, out, lse, dv_, B, N, heads, img_rows=rows, scale=SCALE, torch_arm=False)
    o3, g3 = out.view(B, rows, -1), dqkv.view(B, rows, -1)
    assert torch.equal(o3[:, :N].reshape(B * N, -1), ref[0]) and torch.equal(lse, ref[1])
    assert torch.equal(g3[:, :N].reshape(B * N, -1), ref[2])
    assert bool((o3[:, N:] == 0).all()) and bool((g3[:, N:] == 0).all()), "pad rows must be written as zeros"


def test_attn_refuses_unsupported_before_launch(dev):
    qkv = torch.zeros(300, 192, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="at most 256"):
        K.attn_fwd(qkv, 1, 300, 1, torch_arm=False)
