"""The bounds of tests/test_attn_calls_gpu.py, checked without a GPU over that file's cases.

1. ``_attn_ref.attn_*_restated32`` computes the calls in float32 with the kernels' rounding points (bf16 P per key tile
   before P V, the running max and alpha of the streamed forward, bf16 out, lse log2e rounded before the fma, bf16 dS
   and P as operands, bf16 dq / dk / dv) and torch's summation orders.  Every element of out, D, dq, dk, dv must lie
   within 1 x the bound of the float64 reference (the GPU test allows 2 x; the second factor is for summation orders
   the restatement does not reproduce), lse within 1e-3.
2. Each fault of ``_attn_ref.FAULTS``, put into that restatement, must leave MORE THAN 4 x the bound where it acts,
   at the cases and the input variant named for it in FAULT_PLAN: a correct kernel may sit 2 x away on the other side,
   so 4 x cannot be absorbed.  "Where it acts" is a set of rows defined from the float64 reference alone (``_acts``);
   it must be at least half the rows of the output, and a row counts when one of its 64 elements (or, for the
   forward, its lse) is beyond 4 x.

The backward runs on CPU-made operands: the float64 forward rounded to bf16 (out) and f32 (lse).  The printed ratios
are recorded in profiles/attn_calls/cpu_conditions.txt."""
import math

import pytest
import torch

import _attn_ref as ref

CASES, _id = ref.CASES, ref.case_id
# N in {1, 33, 65, 129, 257, 577} under every variant
SWEEP = [(1, 1, 1), (2, 3, 33), (2, 2, 65), (1, 2, 129), (2, 3, 257), (1, 2, 577)]


def _restated(pair, shape, variant, ffault=None, bfault=None):
    """the restatement's outputs and their |error| / bound per element: dict name -> ratio tensor"""
    c = ref.calls_case(shape, variant)
    stream = pair == "stream"
    f, b = c["fwd"], c["bwd"]
    out, lse = ref.attn_fwd_restated32(c["qkv"], shape, c["scale"], stream=stream, fault=ffault)
    dqkv, D = ref.attn_bwd_restated32(c["qkv"], c["out"], c["lse"], c["dout"], shape, c["scale"], stream=stream,
                                      fault=bfault, out_unrounded=f["out"])
    B, heads, N = shape
    g = ref.ratio(dqkv, b["dqkv"], b["dqkv_bound"]).view(B, N, 3, heads, ref.HD)
    return dict(out=ref.ratio(out, f["out"], f["out_bound_stream" if stream else "out_bound"]).view(B, N, heads, ref.HD),
                lse=ref.ratio(lse, f["lse"], torch.full_like(f["lse"], ref.LSE_ABS)).transpose(1, 2),  # [B, N, heads]
                D=ref.ratio(D, b["D"], b["D_bound"]).transpose(1, 2), dq=g[:, :, 0], dk=g[:, :, 1], dv=g[:, :, 2])


def _worst(r):
    return {k: float(v.max()) for k, v in r.items()}


def _line(pair, shape, variant, what, figs):
    return (f"attn_calls_cpu {pair} {'x'.join(map(str, shape))} {variant} {what}: "
            + "  ".join(f"{k} {v:.3g}" for k, v in figs.items()))


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_float32_restatement_is_inside_the_bound(case):
    pair, shape, variant = case
    w = _worst(_restated(pair, shape, variant))
    print(_line(pair, shape, variant, "restatement", w))
    assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_float32_restatement_is_inside_the_bound_at_every_variant(variant):
    """the streamed restatement at N in {1, 33, 65, 129, 257, 577} under every variant (2048: the case list above)"""
    for shape in SWEEP:
        w = _worst(_restated("stream", shape, variant))
        print(_line("stream", shape, variant, "restatement", w))
        assert all(v <= 1.0 for v in w.values()), (shape, w)


# ---- faults
S33, S65, S129, S257, S577, S2048 = (2, 3, 33), (2, 2, 65), (1, 2, 129), (2, 3, 257), (1, 2, 577), (1, 1, 2048)
O129, O197 = (1, 2, 129), (2, 3, 197)
SPIKED_DROP = [("stream", s) for s in (S33, S65, S129, S257, S577, S2048)] + [("onepass", s) for s in (O129, O197)]
# fault -> (pass, variant, [(pair, shape)], why that variant)
FAULT_PLAN = {
    "dropped_last_key": [("fwd", "spike_last", SPIKED_DROP), ("fwd", "spike_edges", SPIKED_DROP),
                         ("bwd", "spike_last", SPIKED_DROP), ("bwd", "spike_edges", SPIKED_DROP)],
    # at (1, 1, 2048) seven keys share a row's weight and the forward leaves 2047 of the 2048 out rows beyond 4 x, one
    # short of "every row": that run is held to FLOOR instead, and the summary says so
    "dropped_tile_first_key": [("fwd", "spike_edges", SPIKED_DROP), ("bwd", "spike_edges", SPIKED_DROP)],
    # the pad key's score is 0 and it takes 1 / (N + 1) of a uniform row: lse moves by log((N + 1) / N), beyond
    # 4 x LSE_ABS up to N = 129; under a spike it would take e^-8 of that
    "pad_key_counted": [("fwd", "uniform", [("stream", S33), ("stream", S65), ("stream", S129), ("onepass", (1, 2, 33)),
                                            ("onepass", O129)])],
    "no_rescale_last": [("fwd", "spike_last", [("stream", s) for s in (S65, S129, S257, S577, S2048)])],
    "half_max": [("fwd", "spike_last", [("stream", s) for s in (S33, S65, S129, S257, S2048)]
                  + [("onepass", O129), ("onepass", O197)])],
    "no_max": [("fwd", "shift_up", [("stream", S65), ("stream", S257), ("onepass", O129), ("onepass", O197)])],
    # lse differs from query row to query row by O(1) under a spike (the 63 other columns of the spiked key's score),
    # by 0.85 / sqrt(N) under the uniform inputs.  Named from the N at which at least half the query rows sit in a
    # tile after the first (at N = 65 one query of 65 is stale, and a key's sum over the queries barely moves)
    "stale_tile_stats": [("bwd", "spike_first", [("stream", s) for s in (S129, S257, S577, S2048)]
                          + [("onepass", O129), ("onepass", O197)])],
    "d_unrounded": [("bwd", "uniform", [("stream", s) for s in (S33, S65, S257, S2048)] + [("onepass", O197)])],
    "lse_other_head": [("bwd", "spike_first", [("stream", s) for s in (S33, S65, S129, S257, S577)]
                        + [("onepass", O129), ("onepass", O197)])],
    "ds_unscaled": [("bwd", "uniform", [("stream", s) for s in (S33, S65, S257, S2048)] + [("onepass", O197)])],
}
FAULT_RUNS = [(fault, which, variant, pair, shape) for fault, plans in FAULT_PLAN.items()
              for which, variant, where in plans for pair, shape in where]
# the one run that cannot meet "every acting row": the share of rows it does reach (2047 / 2048), so that it cannot get worse
FLOOR = {("dropped_tile_first_key", "fwd", "spike_edges", "stream", S2048): 0.999}


def _scores(shape, variant):
    c = ref.calls_case(shape, variant)
    B, heads, N = shape
    q, k, _ = ref.split(c["qkv"], B, N, heads)
    return (q @ k.transpose(-1, -2)) * c["scale"]  # [B, heads, N(query), N(key)]


def _acts(fault, which, pair, shape, variant):
    """dict output -> (rows [B, N, heads] the fault acts on, the share of them that must be displaced; None: the
    figure is printed only).  From the float64 reference and the geometry alone."""
    B, heads, N = shape
    every = torch.ones(B, N, heads, dtype=torch.bool)
    pad = ref.KT if pair == "stream" else ref.SUB
    if fault in ("dropped_last_key", "dropped_tile_first_key"):
        j = N - 1 if fault == "dropped_last_key" else pad * ((N - 1) // pad)
        if which == "fwd":
            return dict(out=(every, 1.0))
        own = torch.zeros_like(every)
        own[:, j] = True  # the dropped key's own gradient rows
        return dict(dq=(every, 0.9), dk=(own, 1.0), dv=(own, 1.0))
    if fault == "pad_key_counted" or fault == "no_max":
        return dict(out_or_lse=(every, 1.0))
    if fault == "no_rescale_last":  # rows whose running max rises in the last tile so that the earlier tiles' sums,
        s = _scores(shape, variant)  # left unscaled, weigh at least twice what they should
        k0 = pad * ((N - 1) // pad)
        rise = s[..., k0:].max(-1).values - s[..., :k0].max(-1).values
        return dict(out_or_lse=((rise >= math.log(2.0)).transpose(1, 2), 1.0))
    if fault == "half_max":  # rows whose two key halves (arow(i, h)) have maxima at least log 2 apart
        s = _scores(shape, variant)
        half = ref.lane_half(torch.arange(N)).bool()
        gap = (s[..., half].max(-1).values - s[..., ~half].max(-1).values).abs()
        return dict(out_or_lse=((gap >= math.log(2.0)).transpose(1, 2), 1.0))
    if fault == "stale_tile_stats":  # every key sums over every query tile, all but the first of them stale
        return dict(dk=(every, 1.0), dv=(every, 1.0))
    if fault == "d_unrounded":  # D moves by sum_d do_d (o_d - bf16(o_d)), a random sum that is near zero in some rows:
        # nine tenths of the rows of D.  dq sees it through P dD scale, below dS's own bf16 rounding: printed only, so
        # this fault is visible where D is (the streamed pair's dws) and not through attn.hip's outputs
        return dict(D=(every, 0.9), dq=(every, None))
    if fault == "lse_other_head":
        return dict(dq=(every, 0.9), dk=(every, 0.9), dv=(every, 0.9))
    if fault == "ds_unscaled":
        return dict(dq=(every, 1.0), dk=(every, 1.0))
    raise KeyError(fault)


@pytest.mark.parametrize("run", FAULT_RUNS, ids=["-".join([r[0], r[1], r[2], r[3], "x".join(map(str, r[4]))])
                                                 for r in FAULT_RUNS])
def test_fault_is_displaced_where_it_acts(run):
    fault, which, variant, pair, shape = run
    r = _restated(pair, shape, variant, ffault=fault if which == "fwd" else None, bfault=fault if which == "bwd" else None)
    hit = {k: (v > 4.0) if v.dim() == 3 else (v > 4.0).any(-1) for k, v in r.items()}  # per row [B, N, heads]
    hit["out_or_lse"] = hit["out"] | hit["lse"]
    figs, ok = {}, True
    for name, (rows, share) in _acts(fault, which, pair, shape, variant).items():
        share = FLOOR.get(run, share) if share == 1.0 else share
        acting = float(rows.float().mean())
        got = float(hit[name][rows].float().mean()) if rows.any() else 0.0
        figs[f"{name} acts"] = acting
        figs[f"{name} rows>4x"] = got
        single = int(rows.sum()) == shape[0] * shape[1]  # one row per (image, head): the dropped key's own
        ok = ok and (share is None or (got >= share and (acting >= 0.5 or single)))
    if which == "fwd":
        figs["out elements>4x"] = float((r["out"] > 4.0).float().mean())
    print(_line(pair, shape, variant, f"{which} {fault}", figs))
    assert ok, figs
