"""The streaming attention kernels (csrc/attn_stream.hip: sv_attn_stream_fwd / sv_attn_stream_bwd) against float64
softmax attention and its autograd over the same bf16-rounded qkv and dout: the checks, inputs and bounds of
tests/test_attn_gpu.py, at the sizes where the streamed tiles can go wrong.

Shapes (B, heads, N): the kernels own 128 tokens per workgroup (32 per wave) and stream the other side in 64-token
tiles, so N = 63, 64, 65 and 127, 128, 129 sit on every edge; 1, 33 are the small ends; 257, 577 and 1025 are the
token counts of 256, 384 and 512 px images; 2048 is the largest N the entry points accept.

Bound (the rule of test_attn_gpu): a CPU restatement rounds P, O, dS and the gradients to bf16 where the kernel does;
each of out, dq, dk, dv must be within max(1e-3, 3 x the restatement's error) in relative L2 of float64, lse within
1e-3 absolute, and at N = 1 (softmax = 1, dq = dk = 0 in float64) dq and dk within 5e-6 absolute.

Inputs: q, k uniform in [-1.5, 1.5], v and dout uniform in [-1, 1], bf16-rounded.  Two more input sets at (2, 2, 257)
scale the key rows by a ramp along the key index: rising (0.25 -> 1), so that the running max tends to keep growing
up to the last key tile and every tile rescales the accumulator, and falling (1 -> 0.25), so that the max tends to sit
in the first tile and later tiles rescale by one.  Two more at (2, 2, 257) shift every score of a head by +-98 and leave
softmax unchanged in exact arithmetic: q[..., 0] = 28 for every query and k[..., 0] = +28 ("shift_up") or -28
("shift_down") for every key, both exact in bf16, so the scaled scores lie in [94, 102] or [-102, -94] and lse is about
+-98 + log N: a forward without the max subtraction overflows or underflows, and a backward that mishandles a large lse
loses P.  Same checks and the same bound rule; each own error of these two must stay below 2e-2 (measured on the CPU at
N = 65 and 257: out 2.4e-3, dq 1.2e-2, dk 2.2e-3, dv 2.5e-3), so that the 3 x own bound cannot become vacuous.

The measured figures of the first run are recorded in profiles/vit_hires/parity.txt."""
import functools

import pytest
import torch

from spine_vision_amd import kernels as K

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 2, 33), (1, 1, 63), (1, 3, 64), (2, 2, 65), (1, 2, 127), (1, 1, 128), (1, 2, 129),
          (2, 3, 257), (1, 2, 577), (1, 1, 1025), (1, 1, 2048)]
CASES = [(s, "uniform") for s in SHAPES] + [((2, 2, 257), "ramp_up"), ((2, 2, 257), "ramp_down"),
                                            ((2, 2, 257), "shift_up"), ((2, 2, 257), "shift_down")]
SHIFT = 28.0  # exact in bf16; 28 * 28 * SCALE = 98
IDS = ["x".join(map(str, s)) + ("" if v == "uniform" else "-" + v) for s, v in CASES]
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
    if variant.startswith("shift"):
        qk = qkv.view(B, N, 3, heads, 64)
        qk[:, :, 0, :, 0] = SHIFT
        qk[:, :, 1, :, 0] = SHIFT if variant == "shift_up" else -SHIFT
    elif variant != "uniform":
        ramp = torch.linspace(0.25, 1.0, N, dtype=torch.float64)
        if variant == "ramp_down":
            ramp = ramp.flip(0)
        qkv.view(B, N, 3, C)[:, :, 1] *= ramp.view(1, N, 1)
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


def _run(dev, qkv, dout, B, N, heads, *, torch_arm=False):
    """forward and backward through kernels.py on guarded buffers -> out, lse, dqkv (device views)"""
    bf = torch.bfloat16
    qv, qb = _guarded(qkv, dev, bf)
    dv_, db = _guarded(dout, dev, bf)
    ov, ob = _guarded(torch.zeros(B * N, heads * 64), dev, bf)
    lv, lb = _guarded(torch.zeros(B, heads, N), dev, torch.float32)
    gv, gb = _guarded(torch.zeros(B * N, 3 * heads * 64), dev, bf)
    ov.fill_(float("nan")), lv.fill_(float("nan")), gv.fill_(float("nan"))  # every element must be written
    K.attn_stream_fwd(qv, B, N, heads, scale=SCALE, out=ov, lse=lv, torch_arm=torch_arm)
    K.attn_stream_bwd(qv, ov, lv, dv_, B, N, heads, scale=SCALE, dqkv=gv, torch_arm=torch_arm)
    torch.cuda.synchronize()
    for name, b_ in (("qkv", qb), ("dout", db), ("out", ob), ("lse", lb), ("dqkv", gb)):
        assert _guards_intact(b_), f"sentinel around {name} overwritten"
    assert torch.equal(qv.cpu().double(), qkv) and torch.equal(dv_.cpu().double(), dout), "an input was modified"
    return ov, lv, gv


def _errors(case, out, lse, dqkv):
    (B, heads, N), _ = case
    ref = _case(case)["ref"]
    gq, gk, gv = _split(dqkv.cpu().double(), B, N, heads)
    rq, rk, rv = _split(ref["dqkv"], B, N, heads)
    e = dict(out=_rel(out.cpu(), ref["out"]), dv=_rel(gv, rv))
    if N == 1:  # dq = dk = 0 exactly in float64: absolute
        e["dq_abs"], e["dk_abs"] = float(gq.abs().max()), float(gk.abs().max())
    else:
        e["dq"], e["dk"] = _rel(gq, rq), _rel(gk, rk)
    e["lse_abs"] = float((lse.cpu().double() - ref["lse"]).abs().max())
    return e


def _bound(case, name):
    return max(1e-3, 3.0 * _case(case)["own"][name])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stream_against_float64(dev, case):
    (B, heads, N), _ = case
    c = _case(case)
    out, lse, dqkv = _run(dev, c["qkv"], c["dout"], B, N, heads)
    e = _errors(case, out, lse, dqkv)
    print(f"[attn_stream] {case}: kernel " + ", ".join(f"{k} {v:.3e}" for k, v in e.items())
          + " | rounding-only restatement " + ", ".join(f"{k} {v:.3e}" for k, v in c["own"].items()))
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all() and torch.isfinite(lse).all(), \
        "an output element was not written (the outputs start as NaN) or is not finite"
    if case[1].startswith("shift"):
        assert all(v < 2e-2 for v in c["own"].values()), ("the restatement's own error makes the bound vacuous", c["own"])
    for name in ("out", "dq", "dk", "dv"):
        if name in e:
            assert e[name] <= _bound(case, name), (name, e[name], _bound(case, name))
    if N == 1:
        assert e["dq_abs"] <= 5e-6 and e["dk_abs"] <= 5e-6, e
    assert e["lse_abs"] <= 1e-3, e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stream_bitwise_run_to_run_and_batch_independent(dev, case):
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
def test_stream_torch_arm_no_further_from_float64(dev, case):
    """SV_ATTN=torch (torch_arm=True) on the same buffers: no further from float64 than 3 x the kernels."""
    (B, heads, N), _ = case
    c = _case(case)
    e_hip = _errors(case, *_run(dev, c["qkv"], c["dout"], B, N, heads))
    e_t = _errors(case, *_run(dev, c["qkv"], c["dout"], B, N, heads, torch_arm=True))
    print(f"[attn_stream] {case}: torch arm " + ", ".join(f"{k} {v:.3e}" for k, v in e_t.items()))
    for name, v in e_t.items():
        if name.endswith("_abs"):
            assert v <= (1e-3 if name == "lse_abs" else 5e-6), (name, v)
        else:
            assert v <= 3.0 * max(e_hip[name], 1e-3 / 3), (name, v, e_hip[name])


@pytest.mark.parametrize("shape", [(2, 2, 257), (1, 2, 577)], ids=["2x2x257", "1x2x577"])
def test_stream_padded_rows(dev, shape):
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

    bf = torch.bfloat16
    qv = pad(c["qkv"]).to(dev, bf)
    dv_ = pad(c["dout"]).to(dev, bf)
    out = torch.full((B * rows, heads * 64), float("nan"), device=dev, dtype=bf)
    dqkv = torch.full((B * rows, 3 * heads * 64), float("nan"), device=dev, dtype=bf)
    out, lse = K.attn_stream_fwd(qv, B, N, heads, img_rows=rows, scale=SCALE, out=out, torch_arm=False)
    K.attn_stream_bwd(qv, out, lse, dv_, B, N, heads, img_rows=rows, scale=SCALE, dqkv=dqkv, torch_arm=False)
    o3, g3 = out.view(B, rows, -1), dqkv.view(B, rows, -1)
    assert torch.equal(o3[:, :N].reshape(B * N, -1), ref[0]) and torch.equal(lse, ref[1])
    assert torch.equal(g3[:, :N].reshape(B * N, -1), ref[2])
    assert bool((o3[:, N:] == 0).all()) and bool((g3[:, N:] == 0).all()), "pad rows must be written as zeros"


def test_stream_refuses_unsupported_before_launch(dev):
    qkv = torch.zeros(2049, 192, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="at most 2048"):
        K.attn_stream_fwd(qkv, 1, 2049, 1, torch_arm=False)
    with pytest.raises(ValueError, match="at most 2048"):
        K.attn_stream_bwd(qkv, qkv[:, :64].contiguous(), torch.zeros(1, 1, 2049, device=dev), qkv[:, :64].contiguous(),
                          1, 2049, 1, torch_arm=False)
