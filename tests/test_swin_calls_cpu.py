"""The bounds of tests/test_swin_calls_gpu.py, checked without a GPU on the walking shapes (all but the 384-window
production form, which only repeats them at depth 2 with more data).

1. ``_swin_ref.winattn_*_restated32`` computes the three calls in float32 with the kernels' index formula and rounding
   points (bf16 P before P V, bf16 out, bf16 dS and P as operands, bf16 dq / dk / dv, f32 partials per wave, f32 fold)
   and torch's summation orders.  Every element of every output must lie within 1 x the bound of the float64 reference
   (the GPU test allows 2 x), lse within 1e-3.
2. Each fault below, put into that restatement, must leave 2 x the bound in at least one element of one output, so the
   bounds are not so wide that the GPU test would pass a kernel with that fault.

The backward runs on CPU-made operands: the float64 forward rounded to bf16 (out) and f32 (lse).  The printed ratios
are recorded in profiles/swin_calls/cpu_conditions.txt."""
import pytest
import torch

import _swin_ref as ref

WALKING = [(1, 12, 12, 2, 1, 32), (5, 8, 8, 4, 2, 128), (3, 28, 28, 7, 3, 24), (2, 32, 32, 8, 4, 64)]
IDS = ["x".join(map(str, s)) for s in WALKING]
SCALE = ref.f32_scale(32 ** -0.5)


def _ratios(geom, fault=None, variant="uniform"):
    """the restatement with ``fault`` -> the largest error / bound of every output"""
    c = ref.calls_case(geom, variant)
    w, nparts, f = geom[3], c["nparts"], c["fwd"]
    out, lse = ref.winattn_fwd_restated32(c["qkv"], c["bias"], geom, SCALE, nparts, fault)
    r = dict(out=float(ref.ratio(out, f["out"], f["out_bound"]).max()),
             lse=float(ref.ratio(lse, f["lse"], torch.full_like(f["lse"], ref.LSE_ABS)).max()))
    if variant != "uniform":
        return r
    b = c["bwd"]
    dqkv, part = ref.winattn_bwd_restated32(c["qkv"], c["out"], c["lse"], c["dout"], c["bias"], geom, SCALE, nparts, fault,
                                            out_unrounded=f["out"])
    r["dqkv"] = float(ref.ratio(dqkv, b["dqkv"], b["dqkv_bound"]).max())
    r["dbias_part"] = float(ref.ratio(part, b["part"], b["part_bound"]).max())
    dtable = ref.bias_grad_restated32(part, c["prior"], w, True)
    r["dtable"] = float(ref.ratio(dtable, *c["dtable"]).max())
    alone, alone_bound = ref.bias_grad_ref(part, c["prior"], w, True)
    r["dtable_fold"] = float(ref.ratio(dtable, alone, alone_bound).max())
    return r


def _line(geom, what, r):
    return f"swin_calls_cpu {'x'.join(map(str, geom))} {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("geom", WALKING, ids=IDS)
def test_every_shape_walks(geom):
    B, H, W, w, shift, heads = geom
    total, nparts = B * (H // w) * (W // w), ref.win_nparts(B, H, W, w, heads)
    assert total > nparts and max(ref.walk_depths(total, nparts)) >= 2


@pytest.mark.parametrize("geom", WALKING, ids=IDS)
def test_float32_restatement_is_inside_the_bound(geom):
    r = _ratios(geom)
    print(_line(geom, "restatement", r))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("geom", WALKING, ids=IDS)
def test_float32_restatement_is_inside_the_bound_at_large_scores(geom):
    r = _ratios(geom, variant="shift_up")
    print(_line(geom, "restatement shift_up", r))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("fault", ref.FAULTS)
@pytest.mark.parametrize("geom", WALKING, ids=IDS)
def test_fault_leaves_the_bound(geom, fault):
    """``no_max`` is the softmax without the max subtraction: it shows at the shift_up inputs (scores near 102)."""
    r = _ratios(geom, fault, variant="shift_up" if fault == "no_max" else "uniform")
    print(_line(geom, fault, r))
    assert max(r.values()) > 2.0, r
