"""GPU: the six Global Response Normalization kernels (csrc/grn.hip) against float64 torch over the same stored
operand values.

Bounds (none calibrated on the kernels' own output).  The statistics are f32 sums of at most HW <= 1024 terms per
(image, channel), in any order: error <= 1024 * 2^-24 = 6.1e-5 of the sum of the terms' magnitudes, so
  G, N                within 1e-4 relative (the terms a^2 are non-negative),
  S, sum du           within 1e-4 x sum |terms|,
  dgamma, dbeta       within 1e-4 x sum |terms|, the terms being those of the sums they are made of
                      (dgamma[c] = sum_{b,p} du a N[b,c]: sum |du a| N; dbeta[c]: sum |du|).
bf16 outputs u and dh: every element within one bf16 step of the reference, 2^-7 |ref|, plus 1e-6 max|ref| for
near-zero cancellations, and at most 0.1 % of the elements different from bf16(ref) at all.
f32 outputs: within 1e-5 of max|ref|.  One channel of one image is all zeros in every case (G = 0, k = 0)."""

import functools

import pytest
import torch

from spine_vision_amd import kernels as K

pytestmark = pytest.mark.gpu

SHAPES = [(3, 36, 512),    # odd batch, two short chunks per image
          (2, 1024, 512),  # several chunks per image
          (3, 60, 768),    # HW and n no powers of two: a ragged last chunk and a part-filled column tile
          (2, 4, 6144)]    # the widest channel mean, fewer rows than a wave
DTYPES = [torch.bfloat16, torch.float32]
DEAD = (-1, 5)  # (image, channel) whose activations are all zero


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs (host, stored dtype) and the float64 reference of every intermediate and output."""
    B, HW, n = shape
    gen = torch.Generator().manual_seed(1000 * B + HW + n)
    a = torch.nn.functional.gelu(torch.randn(B, HW, n, generator=gen))
    a[DEAD[0], :, DEAD[1]] = 0.0
    a = a.to(dtype)
    du = (0.1 * torch.randn(B, HW, n, generator=gen)).to(dtype)
    gh = (torch.rand(B, HW, n, generator=gen) * 1.3 - 0.2).to(dtype)
    gamma = torch.rand(n, generator=gen) * 0.4 + 0.8
    beta = torch.rand(n, generator=gen) * 0.2 - 0.1
    A, DU, GH, g64, b64 = a.double(), du.double(), gh.double(), gamma.double(), beta.double()
    G = A.pow(2).sum(1).sqrt()
    D = G.mean(-1) + 1e-6
    N = G / D[:, None]
    scale = 1 + g64 * N
    u = A * scale[:, None] + b64
    S, T = (DU * A).sum(1), DU.sum(1)
    dN = g64 * S
    dG = dN / D[:, None] - (dN * G).sum(-1, keepdim=True) / (n * D[:, None] ** 2)
    k = torch.where(G > 0, dG / G.clamp_min(1e-300), torch.zeros_like(G))
    dh = (DU * scale[:, None] + A * k[:, None]) * GH
    ref = dict(G=G, N=N, D=D, scale=scale, u=u, S=S, T=T, S_abs=(DU * A).abs().sum(1), T_abs=DU.abs().sum(1),
               dgamma=(S * N).sum(0), dbeta=T.sum(0), dgamma_abs=((DU * A).abs().sum(1) * N).sum(0),
               dbeta_abs=DU.abs().sum((0, 1)), k=k, dh=dh)
    return dict(a=a, du=du, gh=gh, gamma=gamma, beta=beta), ref


def _dev(inp, dev):
    B, HW, n = inp["a"].shape
    t = {k: v.to(dev) for k, v in inp.items()}
    for k in ("a", "du", "gh"):
        t[k] = t[k].view(B * HW, n)
    return t, B


def _finite(*ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


def _check_out(name, got, ref, dtype):
    got, scale = got.detach().cpu(), float(ref.abs().max())
    err = (got.double() - ref.view_as(got)).abs()
    if dtype == torch.bfloat16:
        lim = 2.0 ** -7 * ref.view_as(got).abs() + 1e-6 * scale
        differ = float((got != ref.view_as(got).to(torch.bfloat16)).float().mean())
        print(f"{name}: worst err / limit {float((err / lim).max()):.3f}, {100 * differ:.4f} % differ from bf16(ref)")
        assert (err <= lim).all(), name
        assert differ <= 1e-3, (name, differ)
    else:
        print(f"{name}: max err {float(err.max()):.3e} on scale {scale:.3e}")
        assert float(err.max()) <= 1e-5 * scale, name


def _within(name, got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    print(f"{name}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert (err <= bound).all(), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grn_forward(dev, shape, dtype):
    inp, ref = _case(shape, dtype)
    t, B = _dev(inp, dev)
    part = K.grn_stats(t["a"], B)
    assert tuple(part.shape) == (B, K.grn_nparts(shape[1], shape[2]), shape[2])
    G, N, scale, D = K.grn_finish(part, t["gamma"])
    u = K.grn_apply(t["a"], scale, t["beta"])
    torch.cuda.synchronize()
    _finite(part, G, N, scale, D, u)
    _within("G", G, ref["G"], 1e-4 * ref["G"])
    _within("N", N, ref["N"], 1e-4 * ref["N"])
    _within("D", D, ref["D"], 1e-4 * ref["D"])
    _within("scale", scale, ref["scale"], 1e-4 * ref["scale"].abs())
    assert float(G[DEAD]) == 0.0 and float(N[DEAD]) == 0.0 and float(scale[DEAD]) == 1.0
    assert u.dtype == dtype
    _check_out("u", u.view(shape), ref["u"], dtype)
    # in place over a, and a second launch: bit for bit
    a2 = t["a"].clone()
    u2 = K.grn_apply(a2, scale, t["beta"], out=a2)
    assert u2.data_ptr() == a2.data_ptr() and torch.equal(u2, u)
    st2 = K.grn_finish(K.grn_stats(t["a"], B), t["gamma"])
    assert all(torch.equal(x, y) for x, y in zip(st2, (G, N, scale, D)))
    assert torch.equal(K.grn_apply(t["a"], scale, t["beta"]), u)
    u3, st3 = K.grn_fwd(t["a"].clone(), B, t["gamma"], t["beta"], inplace=True)
    assert torch.equal(u3, u) and torch.equal(st3[2], scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grn_backward(dev, shape, dtype):
    inp, ref = _case(shape, dtype)
    t, B = _dev(inp, dev)
    n = shape[2]
    G, N, scale, D = K.grn_finish(K.grn_stats(t["a"], B), t["gamma"])

    def run(du, out):
        sp, dp = K.grn_bwd_stats(du, t["a"], B)
        folded = sp.double().sum(1).cpu(), dp.double().sum(1).cpu()
        dgamma, dbeta = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
        k = K.grn_bwd_finish(sp, dp, t["gamma"], G, N, D, dgamma=dgamma, dbeta=dbeta, accumulate=False)
        dh = K.grn_bwd_apply(du, t["a"], t["gh"], scale, k, out=out)
        torch.cuda.synchronize()
        return folded, (sp[:, 0].clone(), dp[:, 0].clone()), k, dgamma, dbeta, dh

    folded, totals, k, dgamma, dbeta, dh = run(t["du"], None)
    _finite(k, dgamma, dbeta, dh, *totals)
    _within("S (partials)", folded[0], ref["S"], 1e-4 * ref["S_abs"])
    _within("sum du (partials)", folded[1], ref["T"], 1e-4 * ref["T_abs"])
    _within("S (folded)", totals[0], ref["S"], 1e-4 * ref["S_abs"])
    _within("sum du (folded)", totals[1], ref["T"], 1e-4 * ref["T_abs"])
    _within("dgamma", dgamma, ref["dgamma"], 1e-4 * ref["dgamma_abs"])
    _within("dbeta", dbeta, ref["dbeta"], 1e-4 * ref["dbeta_abs"])
    assert float(k[DEAD]) == 0.0
    assert dh.dtype == dtype
    _check_out("dh", dh.view(shape), ref["dh"], dtype)
    # accumulate = 1 (what the backbone's backward does into the gradient views): one f32 add onto what was there
    sp, dp = K.grn_bwd_stats(t["du"], t["a"], B)
    dg1, db1 = torch.full((n,), 0.5, device=dev), torch.full((n,), -0.25, device=dev)
    k1 = K.grn_bwd_finish(sp, dp, t["gamma"], G, N, D, dgamma=dg1, dbeta=db1, accumulate=True)
    assert torch.equal(dg1, 0.5 + dgamma) and torch.equal(db1, -0.25 + dbeta) and torch.equal(k1, k)
    # in place over du, and a second launch: bit for bit
    du2 = t["du"].clone()
    _, totals2, k2, dgamma2, dbeta2, dh2 = run(du2, du2)
    assert dh2.data_ptr() == du2.data_ptr()
    for x, y in zip((*totals2, k2, dgamma2, dbeta2, dh2), (*totals, k, dgamma, dbeta, dh)):
        assert torch.equal(x, y)
    dh3 = K.grn_bwd(t["du"].clone(), t["a"], t["gh"], B, t["gamma"], (G, N, scale, D),
                    dgamma=torch.zeros(n, device=dev), dbeta=torch.zeros(n, device=dev))
    assert torch.equal(dh3, dh)
