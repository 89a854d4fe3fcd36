"""The ViT attention calls one at a time (csrc/attn.hip: sv_attn_fwd / sv_attn_bwd, one pass over N <= 256 keys;
csrc/attn_stream.hip: sv_attn_stream_fwd / sv_attn_stream_bwd, 64-key tiles, N <= 2048): float64 references with a
per-element error bound, inputs in which single keys carry weight, and a float32 restatement with faults that can be
switched on (tests/test_attn_calls_gpu.py, tests/test_attn_calls_cpu.py).  The pattern, the constants and the helpers
that fit unchanged are those of the last section of tests/_swin_ref.py; the rest is head dimension 64, no bias, no
mask, layout [B][img_rows][3 * heads * 64] and ``scale`` as a C float.

u = 2^-24 (f32), b = 2^-8 (bf16), tiny = 2^-126.  Every term below is read from the kernels' order of operations;
second-order products of the terms are left to the factor 2 of the GPU test.

Forward (``attn_fwd_ref``).  The kernels keep the RAW dot S = q . k in the accumulator, take the row (or running)
max m of it and form e_k = exp2((S_k - m) sl2), sl2 = scale log2e.  With s = scale S:
  score     ds = 64 u scale sum_d |q_d||k_d|        a 64-term f32 MFMA sum of exact bf16 products
  exp       relative error of e_k: ds_k + 4 u |s_k - m| + 2^-21: the subtraction, sl2 (the rounded constant and its
            product with scale) and the product form the argument in f32; the hardware exp2 as in _swin_ref
  out       Swin's ``softmax_out_bound`` with nkeys = N: b pv (P rounded to bf16 before P V) + 2 dmax pv + 2 N u pv
            (f32 accumulation over N keys in P V and in l) + 3 u |out| (1 / l and the product), pv = sum_k p_k |v_kd|
  streamed  attn_stream.hip multiplies l and O by alpha = exp2((m_old - m_new) sl2) once per key tile:
            + nkt (2 u + 2^-21) pv, nkt = ceil(N / 64): per tile the rounding of O alpha, the fma of l and alpha's exp2.
            attn.hip has no such term.
  store     b (|out| + the above) + tiny
  lse       1e-3 absolute (LSE_ABS), the project's bound: the fast log's accuracy cannot be read from the code.

Backward (``attn_bwd_ref``; ``out`` bf16 and ``lse`` f32 are operands).  Swin's chain with hd = 64 and one difference
in the exponent: the kernels round L2 = lse log2e to f32 and then take exp2(fmaf(S, sl2, -L2)), so the argument's error
is carried by |s| and |lse| separately, not by |s - lse| (at the shift inputs both are near 98):
  P         dP_ = P (ds + 2 u |s| + 2 u |lse| + u |s - lse| + 2^-21) + tiny: sl2's two roundings on s, the constant's
            and the product's on lse, the fma's one rounding
  D         64 u sum_d |do_d o_d| + tiny: row_dot64's 64-step fmaf chain (checked alone on the streamed pair's dws)
  T         dT = dP_ |dP - D| + P 64 u (sum_d |do_d||v_d| + sum_d |do_d||o_d|) + 2 u |T| + tiny
  dS        ddS = (scale dT + u |dS|)(1 + b) + b |dS| + tiny       the product with scale, then bf16 as MFMA operand
  dq / dk   sum ddS |k| (|q|) + N u sum |dS||k| (|q|), then the bf16 store
  dv        sum (dP_ (1 + b) + b P) |do| + N u sum P |do|, then the bf16 store

Inputs (``calls_inputs``): bf16-exact float64, q and k uniform in [-1.5, 1.5], v and dout in [-1, 1], one draw for the
whole matrix, so every (image, head) has its own data and a wrong stride shows.  ``shift_up`` / ``shift_down`` put
q[..., 0] = 28 and k[..., 0] = +-28 (scores near +-98); ``ramp_up`` scales key row j by 0.25 -> 1.  With all keys
alike a softmax spreads a row's weight over N keys: a key dropped from a row moves an out element of that row by about
|v_j - out| / N = 0.6 / N, against a per-element allowance of 2 x b sum_k p_k |v_kd| = 4e-3, so from N of about 150 on
no element shows it.  (out itself is a mean of N signed values, about 0.6 / sqrt(N), so the row moves by 1 / sqrt(N) of
itself: a relative L2 over the whole tensor sees a key dropped in EVERY row and not one dropped in a few rows.)  The
spike variants give single keys the weight, and then one row is enough: q[..., 0] = 8 for every
query, k[..., 0] clamped to [-1, 1], then k[j, 0] = 8 (exact in bf16) for the spiked keys j: that column alone puts a
spiked key's scaled score 7 above every other key's.
  spike_edges   j in {0, 63, 64, 127, 128, the first key of the last 64-key tile, N - 1} (those below N)
  spike_last    j = N - 1: every earlier tile's sums are rescaled by about e^-7 at the last step
  spike_first   j = 0: alpha is exactly 1 from the second tile on, the later tiles add little

Restatement (``attn_fwd_restated32`` / ``attn_bwd_restated32``): float32 with the kernels' rounding points and torch's
summation orders; streamed, the forward runs 64-key tiles with a running max, alpha and bf16 P per tile; FAULTS names
what can be switched on."""
import functools
import math

import torch

from _swin_ref import EXP2_REL, LSE_ABS, TINY, U16, U32, f32_scale, ratio, softmax_out_bound, stored_bf16  # noqa: F401

HD = 64  # head dimension
KT = 64  # keys of a streamed tile (attn_stream.hip kT)
SUB = 32  # keys / queries of an MFMA tile
SCALE = 0.125
SHIFT = 28.0  # exact in bf16; 28 * 28 * SCALE = 98
SPIKE = 8.0  # exact in bf16; 8 * 8 * SCALE = 8
VARIANTS = ("uniform", "shift_up", "shift_down", "ramp_up", "spike_edges", "spike_last", "spike_first")
FWD_FAULTS = ("dropped_last_key", "dropped_tile_first_key", "pad_key_counted", "no_rescale_last", "half_max", "no_max")
BWD_FAULTS = ("dropped_last_key", "dropped_tile_first_key", "stale_tile_stats", "d_unrounded", "lse_other_head",
              "ds_unscaled")
FAULTS = FWD_FAULTS + BWD_FAULTS[2:]
# (B, heads, N), variant: the smallest shapes at which each structure of the kernels exists.  Streamed pair: 1, 33 the
# small ends; 63, 64, 65 the 64-key tile edge (65: a one-key last tile); 127, 128, 129 the 128-token workgroup edge (129:
# a second workgroup with one live wave of one live query and three waves that only stage); 257 three workgroups and five
# tiles; 577 more of both; 2048 the contract's end, 32 rescale steps.  One-pass pair: the 32-token MFMA tile and the
# 128-query workgroup edges, ViT's 197 tokens, the contract's end 256.
STREAM_CASES = ([(s, "uniform") for s in [(1, 1, 1), (2, 3, 33), (1, 1, 63), (1, 3, 64), (2, 2, 65), (1, 2, 127),
                                          (1, 1, 128), (1, 2, 129), (2, 3, 257), (1, 1, 2048)]]
                + [(s, v) for s in [(2, 2, 65), (1, 2, 129)] for v in ("spike_edges", "spike_last", "spike_first")]
                + [((2, 3, 257), v) for v in ("ramp_up", "shift_up", "shift_down", "spike_edges")]
                + [((1, 2, 577), "spike_edges"), ((1, 1, 2048), "spike_last")])
ONEPASS_CASES = ([(s, "uniform") for s in [(1, 1, 1), (2, 3, 17), (1, 2, 32), (1, 2, 33), (1, 2, 129), (2, 3, 197),
                                           (2, 2, 256)]]
                 + [(s, v) for s in [(1, 2, 129), (2, 3, 197)] for v in ("spike_edges", "shift_up", "shift_down")])
CASES = [("stream",) + c for c in STREAM_CASES] + [("onepass",) + c for c in ONEPASS_CASES]


def case_id(c):
    return c[0] + "-" + "x".join(map(str, c[1])) + "-" + c[2]


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def split(t2d, B, N, heads, parts=3):
    """[B * N, parts * heads * 64] -> ``parts`` tensors [B, heads, N, 64]"""
    v = t2d.reshape(B, N, parts, heads, HD).permute(2, 0, 3, 1, 4)
    return tuple(v[i] for i in range(parts))


def merge(t):
    """[B, heads, N, 64] -> [B * N, heads * 64]"""
    B, h, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, h * HD)


def spiked_keys(N, variant):
    if variant == "spike_edges":
        return sorted({j for j in (0, 63, 64, 127, 128, KT * ((N - 1) // KT), N - 1) if j < N})
    return {"spike_last": [N - 1], "spike_first": [0]}.get(variant, [])


def calls_inputs(shape, variant="uniform"):
    """qkv [B * N, 3 * heads * 64] and dout [B * N, heads * 64], bf16-exact float64"""
    B, heads, N = shape
    assert variant in VARIANTS, variant
    g = torch.Generator().manual_seed(32452843 + 7919 * B + 131 * heads + N)
    C = heads * HD
    qkv = torch.rand(B * N, 3 * C, generator=g, dtype=torch.float64) * 2 - 1
    qkv.view(B * N, 3, C)[:, :2] *= 1.5
    qk = qkv.view(B, N, 3, heads, HD)
    if variant.startswith("shift"):
        qk[:, :, 0, :, 0] = SHIFT
        qk[:, :, 1, :, 0] = SHIFT if variant == "shift_up" else -SHIFT
    elif variant == "ramp_up":
        qkv.view(B, N, 3, C)[:, :, 1] *= torch.linspace(0.25, 1.0, N, dtype=torch.float64).view(1, N, 1)
    elif variant.startswith("spike"):
        qk[:, :, 0, :, 0] = SPIKE
        qk[:, :, 1, :, 0].clamp_(-1.0, 1.0)
        qk[:, spiked_keys(N, variant), 1, :, 0] = SPIKE
    qkv = _bf(qkv)
    dout = _bf(torch.rand(B * N, C, generator=g, dtype=torch.float64) * 2 - 1)
    return qkv, dout


def nkt_of(N):
    return -(-N // KT)


def attn_fwd_ref(qkv, shape, scale):
    """float64 of the forward on its operands -> dict(out, out_bound (attn.hip), out_bound_stream [B * N, C];
    lse [B, heads, N])"""
    B, heads, N = shape
    q, k, v = split(qkv.double(), B, N, heads)
    s = (q @ k.transpose(-1, -2)) * scale
    ds = HD * U32 * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = p @ v
    arg = s - s.max(-1, keepdim=True).values
    err = softmax_out_bound(p, v, out, ds + U32 * arg.abs(), arg, N)  # Swin's 3 u |arg| and sl2's second rounding
    tiles = nkt_of(N) * (2 * U32 + EXP2_REL) * (p @ v.abs())
    return dict(out=merge(out), out_bound=merge(stored_bf16(out, err)), out_bound_stream=merge(stored_bf16(out, err + tiles)),
                lse=lse)


def attn_bwd_ref(qkv, out, lse, dout, shape, scale):
    """float64 of the backward on its operands -> dict(dqkv, dqkv_bound [B * N, 3 C]; D, D_bound [B, heads, N])"""
    B, heads, N = shape
    q, k, v = split(qkv.double(), B, N, heads)
    (do,), (o,) = split(dout.double(), B, N, heads, 1), split(out.double(), B, N, heads, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    ds = HD * U32 * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    ls = lse.double().unsqueeze(-1)
    arg = s - ls
    p = torch.exp(arg)
    ep = p * (ds + 2 * U32 * s.abs() + 2 * U32 * ls.abs() + U32 * arg.abs() + EXP2_REL) + TINY
    del s, ds, arg
    D = (do * o).sum(-1)
    D_bound = HD * U32 * (do * o).abs().sum(-1) + TINY
    g = do @ v.transpose(-1, -2) - D.unsqueeze(-1)  # dP - D
    eg = HD * U32 * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * o.abs()).sum(-1, keepdim=True))
    t = p * g
    et = ep * g.abs() + p * eg + 2 * U32 * t.abs() + TINY
    del g, eg
    dS = t * scale
    edS = (scale * et + U32 * dS.abs()) * (1 + U16) + U16 * dS.abs() + TINY
    epb = ep * (1 + U16) + U16 * p
    del ep, t, et
    acc = N * U32
    dq, edq = dS @ k, edS @ k.abs() + acc * (dS.abs() @ k.abs())
    dk, edk = dS.transpose(-1, -2) @ q, edS.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs())
    dv, edv = p.transpose(-1, -2) @ do, epb.transpose(-1, -2) @ do.abs() + acc * (p.transpose(-1, -2) @ do.abs())
    dqkv = torch.cat([merge(x) for x in (dq, dk, dv)], dim=1)
    bound = torch.cat([merge(stored_bf16(x, e)) for x, e in ((dq, edq), (dk, edk), (dv, edv))], dim=1)
    # columns (q|k|v, head, d): the three merged blocks side by side are that order
    return dict(dqkv=dqkv, dqkv_bound=bound, D=D, D_bound=D_bound)


# ---- the float32 restatement
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


LOG2E32 = _f32(1.4426950408889634)  # kLog2e as the kernels hold it


def lane_half(idx):
    """the lane half that holds row ``idx`` of a 32-row accumulator tile: arow(i, h) = (i & 3) + 8 (i >> 2) + 4 h"""
    return (idx >> 2) & 1


def attn_fwd_restated32(qkv, shape, scale, *, stream, fault=None):
    """-> (out [B * N, C] of bf16 values, lse [B, heads, N] of f32 values), as float64.  ``stream``: 64-key tiles with
    a running max and alpha (attn_stream.hip); otherwise one pass over the keys, padded to 32 (attn.hip)."""
    B, heads, N = shape
    assert fault is None or fault in FWD_FAULTS, fault
    q, k, v = (t.float() for t in split(qkv, B, N, heads))
    pad = KT if stream else SUB
    npad = -(-N // pad) * pad
    T = KT if stream else npad
    nt = npad // T
    zeros = torch.zeros(B, heads, npad - N, HD)
    k, v = torch.cat([k, zeros], 2), torch.cat([v, zeros], 2)  # the zero-filled tile rows
    valid = torch.arange(npad) < N
    if fault == "dropped_last_key":
        valid[N - 1] = False
    elif fault == "dropped_tile_first_key":
        valid[pad * ((N - 1) // pad)] = False
    elif fault == "pad_key_counted" and N < npad:
        valid[N] = True
    ng = 2 if fault == "half_max" else 1  # the groups that keep a max of their own
    kgroup = lane_half(torch.arange(npad)) if ng == 2 else torch.zeros(npad, dtype=torch.long)
    dgroup = lane_half(torch.arange(HD)) if ng == 2 else torch.zeros(HD, dtype=torch.long)
    sl2 = _f32(scale) * LOG2E32
    m = torch.full((B, heads, N, ng), -math.inf)
    l = torch.zeros(B, heads, N, ng)
    O = torch.zeros(B, heads, N, HD)
    for t in range(nt):
        sel = slice(t * T, (t + 1) * T)
        S = q @ k[:, :, sel].transpose(-1, -2)
        masks = [valid[sel] & (kgroup[sel] == g) for g in range(ng)]
        tm = torch.stack([S.masked_fill(~mk, -math.inf).max(-1).values for mk in masks], -1)
        mn = torch.zeros_like(m) if fault == "no_max" else torch.maximum(m, tm)
        alpha = torch.exp2((m - mn) * sl2)
        if fault == "no_rescale_last" and t == nt - 1 and nt > 1:
            alpha = torch.ones_like(alpha)
        p = torch.where(valid[sel], torch.exp2((S - mn[..., kgroup[sel]]) * sl2), torch.zeros(()))
        ts = torch.stack([(p * mk).sum(-1) for mk in masks], -1)
        l = l * alpha + ts
        O = O * alpha[..., dgroup] + p.bfloat16().float() @ v[:, :, sel]
        m = mn
    lt = l.sum(-1)
    lse = m[..., 0] * _f32(scale) + torch.log(lt)
    out = (O * (1.0 / lt).unsqueeze(-1)).bfloat16().float()
    return merge(out).double(), lse.double()


def attn_bwd_restated32(qkv, out, lse, dout, shape, scale, *, stream, fault=None, out_unrounded=None):
    """-> (dqkv [B * N, 3 C] of bf16 values, D [B, heads, N] of f32 values), as float64.  ``stream`` only sets the
    query tile of ``stale_tile_stats`` (64; attn.hip indexes its whole-N image by 32-query tiles)."""
    B, heads, N = shape
    assert fault is None or fault in BWD_FAULTS, fault
    q, k, v = (t.float() for t in split(qkv, B, N, heads))
    (do,) = split(dout.float(), B, N, heads, 1)
    (o,) = split((out_unrounded if fault == "d_unrounded" else out).float(), B, N, heads, 1)
    D = (do * o).sum(-1)
    ls = lse.float()
    if fault == "lse_other_head":
        ls = ls.roll(-1, dims=1)
    L2 = ls * LOG2E32
    sc = _f32(scale)
    sl2 = sc * LOG2E32
    S = q @ k.transpose(-1, -2)
    dP = do @ v.transpose(-1, -2)
    pad = KT if stream else SUB
    dropped = {"dropped_last_key": N - 1, "dropped_tile_first_key": pad * ((N - 1) // pad)}.get(fault)

    def p_ds(L2, D):
        p = torch.exp2((S.double() * sl2.double() - L2.double().unsqueeze(-1)).float())  # fmaf: one rounding
        if dropped is not None:
            p[..., dropped] = 0
        t = p * (dP - D.unsqueeze(-1))
        return p, (t if fault == "ds_unscaled" else t * sc).bfloat16().float()

    p, dS = p_ds(L2, D)
    dq = dS @ k
    if fault == "stale_tile_stats":  # the dK / dV kernel's staged per-tile copies, one tile late
        idx = torch.arange(N)
        src = torch.where(idx >= pad, idx - pad, idx)
        p, dS = p_ds(L2[..., src], D[..., src])
    dk, dv = dS.transpose(-1, -2) @ q, p.bfloat16().float().transpose(-1, -2) @ do
    dqkv = torch.cat([merge(x.bfloat16().float()) for x in (dq, dk, dv)], dim=1)
    return dqkv.double(), D.double()


def where(flat, shape, cols):
    """(image, head, token, column) of flat index ``flat`` into a [B * N, cols * heads * 64] matrix; for cols = 3 the
    head is prefixed by q / k / v"""
    B, heads, N = shape
    row, col = divmod(flat, cols * heads * HD)
    part, c = divmod(col, heads * HD)
    loc = (row // N, c // HD, row % N, c % HD)
    return ("qkv"[part],) + loc if cols == 3 else loc


@functools.lru_cache(maxsize=None)
def calls_case(shape, variant="uniform"):
    """Operands, float64 references and bounds of both pairs' calls, the backward's on CPU-made operands (the float64
    forward rounded to bf16 / f32); computed once per case, shared by the tests of both files, never modified."""
    scale = f32_scale(SCALE)
    qkv, dout = calls_inputs(shape, variant)
    f = attn_fwd_ref(qkv, shape, scale)
    out, lse = _bf(f["out"]), f["lse"].float().double()
    return dict(qkv=qkv, dout=dout, scale=scale, fwd=f, out=out, lse=lse, bwd=attn_bwd_ref(qkv, out, lse, dout, shape, scale))
