"""The Swin kernels of csrc/swin.hip.

Window attention (sv_winattn_fwd / sv_winattn_bwd, with sv_swin_bias_expand / sv_swin_bias_grad around them) against
float64 windowed attention and its autograd over the same bf16-rounded qkv / dout and f32 table, written as timm
writes it (torch.roll, window_partition, a slice-built mask: tests/_swin_ref.py).

Shapes (B, H, W, w, shift, heads): N = 1; windows below, at and above one 32-token MFMA tile (4, 49, 64 tokens);
window = grid; shifted grids with masked windows; H != W; the stage-4 head count.

Bound.  ``_swin_ref.winattn_restated`` rounds P, O, dS and dq / dk / dv to bf16 where the kernel does (and takes the
rounded O inside D); its distance from float64 is the error that rounding alone causes.  Each of out, dq, dk, dv and
dtable must be within max(1e-3, 3 x that) in relative L2 of float64 (the rule of tests/test_attn_gpu.py); lse within
1e-3 absolute; each own error must stay below 2e-2 so that the rule cannot go vacuous.  At N = 1 the softmax is the
constant 1, so dq, dk and dtable are exactly zero in float64; the kernel computes them from P (dP - D) with dP and D
two f32 sums of the same 32 products (terms below 1) in different orders, |dP - D| < 32 * 2^-23 ~ 4e-6: the bound
there is 5e-6 absolute.

Inputs: q, k uniform in [-1.5, 1.5], v and dout in [-1, 1], the table uniform in [-2, 2] (not symmetric in (i, j): a
transposed bias index fails); one case with table amplitude 16; two cases at (1,14,14,7,3,2) with q[..., 0] = 24 and
k[..., 0] = +-24 (exact in bf16; scaled scores near +-102: a forward without the max subtraction overflows).
Operands and outputs sit inside sentinel-filled buffers whose guard elements must stay intact."""
import functools

import pytest
import torch

import _swin_ref as ref
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 0, 1), (2, 2, 2, 2, 0, 1), (1, 4, 4, 2, 1, 1), (2, 7, 7, 7, 0, 3), (2, 14, 14, 7, 0, 3),
          (2, 14, 14, 7, 3, 3), (1, 28, 14, 7, 3, 2), (2, 8, 8, 8, 0, 2), (1, 16, 16, 8, 4, 4), (1, 14, 14, 7, 3, 24)]
CASES = [(s, "uniform") for s in SHAPES] + [((2, 14, 14, 7, 3, 3), "table16"), ((1, 14, 14, 7, 3, 2), "shift_up"),
                                            ((1, 14, 14, 7, 3, 2), "shift_down")]
IDS = ["x".join(map(str, s)) + ("" if v == "uniform" else "-" + v) for s, v in CASES]
BIG = 24.0  # exact in bf16; 24 * 24 * 32^-0.5 = 101.8
SCALE = 32 ** -0.5
SENTINEL = -7.0
GUARD = 256
BF = torch.bfloat16


def _bf(t):
    return t.to(BF).to(torch.float64)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands (float64 values, bf16-representable except the f32 table), the float64 reference and the own error
    of the rounding-only restatement; computed once per case on the CPU, shared, never modified."""
    (B, H, W, w, shift, heads), variant = case
    g = torch.Generator().manual_seed(104729 * B + 7919 * H + 131 * W + 17 * w + 5 * shift + heads)
    C, n = heads * 32, B * H * W
    qkv = torch.rand(n, 3 * C, generator=g, dtype=torch.float64) * 2 - 1
    qkv.view(n, 3, C)[:, :2] *= 1.5
    if variant.startswith("shift"):
        qk = qkv.view(n, 3, heads, 32)
        qk[:, 0, :, 0] = BIG
        qk[:, 1, :, 0] = BIG if variant == "shift_up" else -BIG
    qkv = _bf(qkv)
    dout = _bf(torch.rand(n, C, generator=g, dtype=torch.float64) * 2 - 1)
    amp = 16.0 if variant == "table16" else 2.0
    table = ((torch.rand((2 * w - 1) ** 2, heads, generator=g, dtype=torch.float64) * 2 - 1) * amp).float().double()
    names = ("out", "lse", "dqkv", "dtable")
    r = dict(zip(names, ref.winattn_f64(qkv, table, dout, B, H, W, w, shift, heads, SCALE)))
    o = dict(zip(names, ref.winattn_restated(qkv, table, dout, B, H, W, w, shift, heads, SCALE)))
    return dict(qkv=qkv, dout=dout, table=table, ref=r, own=_errors(case, o, r))


def _errors(case, got, r):
    (B, H, W, w, shift, heads), _ = case
    C = heads * 32
    e = dict(out=_rel(got["out"], r["out"]), dv=_rel(got["dqkv"][:, 2 * C:], r["dqkv"][:, 2 * C:]))
    if w == 1:  # exactly zero in float64 (module docstring): absolute
        e["dq_abs"] = float(got["dqkv"][:, :C].abs().max())
        e["dk_abs"] = float(got["dqkv"][:, C:2 * C].abs().max())
        e["dtable_abs"] = float(got["dtable"].abs().max())
    else:
        e["dq"] = _rel(got["dqkv"][:, :C], r["dqkv"][:, :C])
        e["dk"] = _rel(got["dqkv"][:, C:2 * C], r["dqkv"][:, C:2 * C])
        e["dtable"] = _rel(got["dtable"], r["dtable"])
    e["lse_abs"] = float((got["lse"].double() - r["lse"]).abs().max())
    return e


def _guarded(t, dev, dtype, fill=None):
    """t inside a larger sentinel-filled buffer: (the exact-size view, the whole buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=dev, dtype=dtype)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dev, dtype)) if fill is None else view.fill_(fill)
    return view, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _run(dev, qkv, dout, table, B, H, W, w, shift, heads, *, rows_total=None, tail=float("nan")):
    """The library's entry points on guarded buffers -> dict(out, lse, dqkv, dtable, part) of device tensors.  Every
    output starts as the sentinel, so an element the kernels skip shows."""
    n, C, N = B * H * W, heads * 32, w * w
    rows = n if rows_total is None else rows_total

    def padded(t):
        return torch.cat([t, torch.full((rows - n, t.shape[1]), tail, dtype=t.dtype)]) if rows > n else t

    qv, qb = _guarded(padded(qkv), dev, BF)
    dv_, db = _guarded(padded(dout), dev, BF)
    tv, tb = _guarded(table, dev, torch.float32)
    nwin = B * (H // w) * (W // w)
    nparts = nv.value("sv_winattn_bwd_nparts", B, H, W, w, heads)
    assert 1 <= nparts <= nwin
    bv, bb = _guarded(torch.zeros(heads, N, N), dev, torch.float32, fill=SENTINEL)
    ov, ob = _guarded(torch.zeros(rows, C), dev, BF, fill=SENTINEL)
    lv, lb = _guarded(torch.zeros(nwin, heads, N), dev, torch.float32, fill=SENTINEL)
    gv, gb = _guarded(torch.zeros(rows, 3 * C), dev, BF, fill=SENTINEL)
    pv, pb = _guarded(torch.zeros(nparts, heads, N, N), dev, torch.float32, fill=SENTINEL)
    dtv, dtb = _guarded(torch.zeros_like(table), dev, torch.float32, fill=SENTINEL)
    p = nv.ptr
    nv.call("sv_swin_bias_expand", p(tv), p(bv), w, heads)
    nv.call("sv_winattn_fwd", p(qv), p(ov), p(lv), p(bv), B, H, W, w, shift, heads, 32, SCALE, rows)
    if rows > n:  # the tail of `out` is written as zeros; the backward must not read it
        assert not ov[n:].any()
        ov[n:] = tail
    nv.call("sv_winattn_bwd", p(qv), p(ov), p(lv), p(dv_), p(bv), p(gv), p(pv), B, H, W, w, shift, heads, 32, SCALE, rows)
    nv.call("sv_swin_bias_grad", p(pv), p(dtv), nparts, w, heads, 0)
    torch.cuda.synchronize()
    for name, b_ in (("qkv", qb), ("dout", db), ("table", tb), ("bias", bb), ("out", ob), ("lse", lb), ("dqkv", gb),
                     ("dbias_part", pb), ("dtable", dtb)):
        assert _guards_intact(b_), f"sentinel around {name} overwritten"
    assert torch.equal(qv[:n].cpu().double(), qkv) and torch.equal(dv_[:n].cpu().double(), dout), "an input was modified"
    return dict(out=ov, lse=lv, dqkv=gv, dtable=dtv, part=pv, bias=bv)


def _check(case, got):
    c = _case(case)
    (B, H, W, w, shift, heads), _ = case
    n = B * H * W
    e = _errors(case, {k: (v[:n] if k in ("out", "dqkv") else v).cpu().double() for k, v in got.items()}, c["ref"])
    own = c["own"]
    print(f"{case}: " + "  ".join(f"{k} {e[k]:.2e} (own {own[k]:.2e})" for k in e))
    for k in e:
        if k.endswith("_abs"):
            assert e[k] <= (1e-3 if k == "lse_abs" else 5e-6), (k, e[k])
        else:
            assert own[k] < 2e-2, (k, own[k])
            assert e[k] <= max(1e-3, 3 * own[k]), (k, e[k], own[k])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_window_attention_matches_float64(case):
    (B, H, W, w, shift, heads), _ = case
    c = _case(case)
    got = _run("cuda", c["qkv"], c["dout"], c["table"], B, H, W, w, shift, heads)
    for k in ("out", "lse", "dqkv", "dtable", "part", "bias"):
        assert bool(torch.isfinite(got[k].float()).all()) and not bool((got[k] == SENTINEL).all()), f"{k} not written"
    _check(case, got)


@pytest.mark.parametrize("case", [CASES[5], CASES[8]], ids=[IDS[5], IDS[8]])
def test_torch_arm_matches_float64(case):
    """The SV_WINATTN=torch arm (the fp32 parity mode's attention and the speed baseline) under the same rule."""
    (B, H, W, w, shift, heads), _ = case
    c = _case(case)
    qkv, dout, table = c["qkv"].to("cuda", BF), c["dout"].to("cuda", BF), c["table"].to("cuda", torch.float32)
    bias = K.swin_bias_expand(table, w)
    out, lse = K.winattn_fwd(qkv, bias, B, H, W, w, shift, heads, scale=SCALE, torch_arm=True)
    dqkv, part = K.winattn_bwd(qkv, out, lse, dout, bias, B, H, W, w, shift, heads, scale=SCALE, torch_arm=True)
    dtable = K.swin_bias_grad(part, torch.zeros_like(table), w, accumulate=False)
    _check(case, dict(out=out, lse=lse, dqkv=dqkv, dtable=dtable))


def test_bitwise_repeatable_and_independent_of_the_batch():
    case = CASES[5]  # (2,14,14,7,3,3)
    (B, H, W, w, shift, heads), _ = case
    c = _case(case)
    a = _run("cuda", c["qkv"], c["dout"], c["table"], B, H, W, w, shift, heads)
    b = _run("cuda", c["qkv"], c["dout"], c["table"], B, H, W, w, shift, heads)
    for k in ("out", "lse", "dqkv", "part", "dtable"):
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"
    n = H * W
    one = _run("cuda", c["qkv"][n:], c["dout"][n:], c["table"], 1, H, W, w, shift, heads)
    assert torch.equal(one["out"], a["out"][n:]) and torch.equal(one["dqkv"], a["dqkv"][n:])
    assert torch.equal(one["lse"], a["lse"][(H // w) * (W // w):])


@pytest.mark.parametrize("case", [CASES[3], CASES[6]], ids=[IDS[3], IDS[6]])
def test_tail_rows_are_zero_and_never_read(case):
    """rows_total > B*H*W (2x7x7 = 98 -> 104 rows): NaN in the tail rows of every input; the real rows bitwise equal
    the unpadded call and the tails of out and dqkv are zeros."""
    (B, H, W, w, shift, heads), _ = case
    c = _case(case)
    n = B * H * W
    plain = _run("cuda", c["qkv"], c["dout"], c["table"], B, H, W, w, shift, heads)
    pad = _run("cuda", c["qkv"], c["dout"], c["table"], B, H, W, w, shift, heads, rows_total=-(-(n + 1) // 8) * 8)
    for k in ("out", "dqkv"):
        assert torch.equal(pad[k][:n], plain[k]) and pad[k].shape[0] > n
    assert not pad["dqkv"][n:].any(), "tail of dqkv not zero"
    for k in ("lse", "part", "dtable"):
        assert torch.equal(pad[k], plain[k])


@pytest.mark.parametrize("w,heads", [(1, 1), (2, 3), (7, 3), (8, 4), (7, 24)])
def test_bias_expand_and_grad_round_trip(w, heads):
    """expand against index_select through timm's relative_position_index (exact); grad against index_add_ in float64
    over the folded partials (f32 sums of up to nparts * w*w terms: 1e-5 relative), accumulate on and off."""
    g = torch.Generator().manual_seed(w * 100 + heads)
    N, E = w * w, (2 * w - 1) ** 2
    table = torch.rand(E, heads, generator=g) * 4 - 2
    idx = ref.relative_position_index(w).view(-1)
    dense = K.swin_bias_expand(table.cuda(), w)
    assert torch.equal(dense.cpu(), table[idx].view(N, N, heads).permute(2, 0, 1))
    nparts = 5
    part = torch.rand(nparts, heads, N, N, generator=g) * 2 - 1
    want = torch.zeros(E, heads, dtype=torch.float64).index_add_(
        0, idx, part.double().sum(0).permute(1, 2, 0).reshape(N * N, heads))
    base = torch.rand(E, heads, generator=g)
    got = K.swin_bias_grad(part.cuda(), base.clone().cuda(), w, accumulate=False)
    assert _rel(got.cpu(), want) < 1e-5 or float((got.cpu().double() - want).abs().max()) < 1e-5
    acc = K.swin_bias_grad(part.cuda(), base.clone().cuda(), w, accumulate=True)
    assert torch.equal(acc.cpu(), base + got.cpu())
    assert torch.equal(K.swin_bias_grad(part.cuda(), base.clone().cuda(), w, accumulate=False), got)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (3, 14, 14, 96), (2, 6, 10, 128), (1, 56, 56, 96)])
def test_patch_merge_and_its_inverse_are_the_torch_permute(B, H, W, C, dtype):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C)
    x = (torch.rand(B * H * W, C, generator=g) * 2 - 1).to(dtype)
    want = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3).reshape(-1, 4 * C)
    n2 = want.shape[0]
    rows_out = -(-(n2 + 1) // 8) * 8
    y = K.patch_merge(x.cuda(), B, H, W, rows_out=rows_out)
    assert torch.equal(y[:n2].cpu(), want) and not y[n2:].any() and y.shape == (rows_out, 4 * C)
    assert torch.equal(K.patch_merge(x.cuda(), B, H, W).cpu(), want)
    # the inverse, from a padded merged matrix whose tail is NaN, into a padded pixel matrix
    ypad = torch.cat([want, torch.full((rows_out - n2, 4 * C), float("nan"), dtype=dtype)])
    rows_in = -(-(B * H * W + 1) // 8) * 8
    dx = K.patch_merge_bwd(ypad.cuda(), B, H, W, rows_in=rows_in)
    assert torch.equal(dx[:B * H * W].cpu(), x) and not dx[B * H * W:].any() and dx.shape == (rows_in, C)


@pytest.mark.parametrize("B,hw,C,tail", [(1, 1, 4, 0), (3, 49, 96, 5), (4, 196, 128, 0), (2, 64, 1024, 8)])
def test_rowscale_kernels_round_once(B, hw, C, tail):
    """x + s t in f32 (one fma: within one f32 rounding of float64) and bf16(s d) (the f32 product rounded to bf16:
    2^-8 relative plus the f32 rounding); dropped samples and tail rows are exact copies / zeros and are not read."""
    g = torch.Generator().manual_seed(B * 100 + hw + C)
    rows = B * hw + tail
    x, t = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    s = torch.tensor([0.0 if b % 3 == 1 else 1 / (1 - 0.03 * (b + 1)) for b in range(B)])
    t[B * hw:] = float("nan")
    if B > 1:
        t[hw:2 * hw] = float("nan")  # sample 1 is dropped
    srow = torch.cat([s.repeat_interleave(hw), torch.zeros(tail)]).double().unsqueeze(1)
    want = x.double() + torch.where(srow == 0, torch.zeros((), dtype=torch.float64), srow * t.double())
    got = K.rowscale_add(x.cuda(), t.cuda(), s.cuda(), hw).cpu()
    assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs().clamp_min(2.0 ** -126)).all())
    assert torch.equal(got[B * hw:], x[B * hw:]) and (B == 1 or torch.equal(got[hw:2 * hw], x[hw:2 * hw]))
    wantc = torch.where(srow == 0, torch.zeros((), dtype=torch.float64), srow * t.double())
    gotc = K.rowscale_cast_bf16(t.cuda(), s.cuda(), hw).cpu()
    assert gotc.dtype == BF and bool(((gotc.double() - wantc).abs() <= (2.0 ** -8 + 2.0 ** -22) * wantc.abs()).all())
    assert not gotc[B * hw:].any() and (B == 1 or not gotc[hw:2 * hw].any())
