"""What tests/test_vit_calls_gpu.py and tests/test_convnext_mlp_calls_gpu.py share: the description of one GEMM-side
kernel call (``Call``), the guarded run (sentinels on either side of every buffer, NaN or prior in every output, inputs
unchanged, two runs bit for bit), the per-element verdict of the ViT file, the float64 GELU pair with its measured erf
term, and the weight gradient's float64 value with its slab-dependent bound.  Test infrastructure only: no kernel is
called from here."""
import math

import pytest
import torch

U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8
SENTINEL = -7.0  # exactly representable in bf16 and f32
GUARD = 256  # sentinel elements on either side (keeps the views 16-byte aligned)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _bf(t):
    return t.to(BF).to(F64)


def _guarded(t, dtype):
    """t inside a larger sentinel-filled buffer: (the exact-size view, the whole buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=t.device, dtype=dtype)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dtype))
    return view, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


class Call:
    """One kernel call: named inputs (float64 values exactly representable in their dtype), outputs (shape, dtype,
    prior or None), ``run(views, policy)``, and float64 ``refs`` name -> (ref, bound)."""

    def __init__(self, kind, M, Ng, Kg, wgrad=False, split=1):
        self.kind, self.M, self.Ng, self.Kg, self.wgrad, self.split = kind, M, Ng, Kg, wgrad, split
        self.inputs, self.outputs, self.refs, self.notes, self.equal = {}, {}, {}, [], []
        self.run = None
        self.slab_ok = lambda policy: False  # weight gradients: whether this policy's call takes bf16 slabs
        self.refs_for = lambda slabs: self.refs


def _gelu64(h):
    return h * 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))


def _gelu_grad64(h):
    return 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def _gelu32(h32):
    """torch's float32 CPU erf-GELU and GELU' (the evaluation the erf terms are measured on)"""
    g32 = torch.nn.functional.gelu(h32)
    phi = 0.5 * (1.0 + torch.erf(h32 * math.sqrt(0.5)))
    return g32, phi + h32 * torch.exp(-0.5 * h32 * h32) * (1.0 / math.sqrt(2.0 * math.pi))


def _erf_abs_terms(h):
    """4 x the largest absolute error of torch's float32 CPU erf-GELU and GELU' against float64 on the same h"""
    h64 = h.cpu()
    g32, d32 = _gelu32(h64.float())
    return (4.0 * float((g32.double() - _gelu64(h64)).abs().max()),
            4.0 * float((d32.double() - _gelu_grad64(h64)).abs().max()))


def _wgrad_terms(dy, x, M, split):
    """G = dy^T x in float64 and the bound of its kernel value before the final store, as a function of the slab form:
    M 2^-24 |dy|^T |x|, plus, with bf16 slabs, 2^-8 sum_s |slab_s| over the ``split`` equal row slices."""
    G = dy.T @ x
    E = M * U24 * (dy.abs().T @ x.abs())
    mag = None
    if split > 1 and M % (split * 64) == 0:  # _bf16_slabs' row condition: whole 64-row K-tiles per slice
        rows = M // split
        mag = torch.zeros_like(G)
        for s in range(split):
            mag += (dy[s * rows:(s + 1) * rows].T @ x[s * rows:(s + 1) * rows]).abs()
    return G, lambda slabs: E + U8 * mag if slabs else E


def _check_output(where, name, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    if not worst <= 2.0:
        flat = int(ratio.reshape(-1).argmax())
        cols = ref.shape[-1] if ref.dim() > 1 else ref.numel()
        r, col = (flat // cols, flat % cols) if ref.dim() > 1 else (0, flat)
        nbad = int((ratio > 2.0).sum())
        badrows = (ratio.reshape(-1, cols) > 2.0).any(1).nonzero().flatten()
        badcols = (ratio.reshape(-1, cols) > 2.0).any(0).nonzero().flatten()
        pytest.fail(f"{where} {name}: {nbad} of {ratio.numel()} elements beyond 2 x bound (rows {int(badrows.min())}.."
                    f"{int(badrows.max())}, columns {int(badcols.min())}..{int(badcols.max())}); worst at row {r}, column "
                    f"{col}: got {float(got.reshape(-1)[flat]):.9g}, float64 {float(ref.reshape(-1)[flat]):.9g}, bound "
                    f"{float(bound.reshape(-1)[flat]):.3e}, error / bound {worst:.3g}")
    return worst


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _equal_pairs(c, first, where):
    for x, y in c.equal:
        assert torch.equal(_bits(first[x]), _bits(first[y])), f"{where}: {x} is not {y} bit for bit"


def _run_guarded(c, policy, where):
    """c through its wrapper on guarded buffers, twice; guards, inputs and run-to-run bits checked; -> the first run's
    outputs"""
    views, bufs = {}, {}
    for n, (t, dt_) in c.inputs.items():
        views[n], bufs[n] = _guarded(t, dt_)
    dev = next(iter(views.values())).device
    for n, (shape, dt_, prior) in c.outputs.items():
        views[n], bufs[n] = _guarded(torch.zeros(shape, device=dev), dt_)
    first = None
    for _ in range(2):
        for n, (shape, dt_, prior) in c.outputs.items():
            if prior is None:
                views[n].fill_(float("nan"))  # every element must be written
            else:
                views[n].copy_(prior.to(dt_))
        c.run(views, policy)
        torch.cuda.synchronize()
        got = {n: views[n].clone() for n in c.outputs}
        if first is None:
            first = got
        else:
            for n in got:
                assert torch.equal(_bits(first[n]), _bits(got[n])), f"{where} {n}: differs run to run"
    for n, b_ in bufs.items():
        assert _guards_intact(b_), f"{where}: sentinel around {n} overwritten"
    for n, (t, dt_) in c.inputs.items():
        assert torch.equal(views[n].double(), t), f"{where}: input {n} was modified"
    return first


def _run_call(c, policy, where, refs):
    """``_run_guarded``, then every output against its float64 reference; -> worst error / bound per output"""
    first = _run_guarded(c, policy, where)
    worst = {n: _check_output(where, n, first[n], *refs[n]) for n in c.outputs}
    _equal_pairs(c, first, where)
    return worst
