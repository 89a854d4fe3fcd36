"""Standalone timing of the fused attention kernels (csrc/attn.hip; --arm stream: csrc/attn_stream.hip) against the SV_ATTN=torch arm (the same maths as
torch matmul / softmax ops on views of the same buffers) at the ViT shapes: N = 197 tokens in the module's 200-row
layout, batch 32, heads 3 / 6 / 12 / 16 (vit_tiny / small / base / large).  HIP events; per shape and pass the arms
alternate, and the whole table runs --rounds times.

    python tools/attn_bench.py [--iters 30] [--rounds 2] [--batch 32] [--heads 3,6,12,16] [--tokens 197]
    python tools/attn_bench.py --arm stream --tokens 197,257,577,1025      # 224 / 256 / 384 / 512 px

--arm stream times the streaming pair as the HIP column at every token count (at most 2048); where the one-pass
kernels also run (N <= 256) they are one more column (``onepass_us``), alternated with the others, not part of the bar.

One JSON line per (round, heads, pass).  Bytes are algorithmic (forward: qkv read, out and lse written; backward: qkv,
out, dout, lse read, dqkv written) against the 6.3 TB/s an HBM-bound kernel reaches on the MI355X; FLOPs are the
products the maths needs (forward 4 B h N^2 d, backward 10 B h N^2 d -- the kernel's recomputation of S and dP in its
dQ phase is not counted) against the 2.5 PF/s bf16 MFMA peak.  F.scaled_dot_product_attention, where this torch build
runs it on views of the same qkv buffer, is a third column (forward, and backward through autograd); it is not part
of the bar.  Each arm walks a ring of --ring operand sets so that a timed launch does not find its own previous
output in the caches."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from spine_vision_amd import kernels as K  # noqa: E402

ACHIEVABLE_TBS = 6.3
BF16_PEAK_TFS = 2500.0


def timeit(fns, iters):
    """microseconds per call of the ring of closures fns (round-robin)"""
    for f in fns:
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _sdpa_arms(sets, B, N, rows, heads):
    """(forward closures, backward closures) of F.scaled_dot_product_attention on views of qkv, or None"""
    import torch.nn.functional as F

    def views(qkv):
        v = qkv.view(B, rows, 3, heads, 64)[:, :N].permute(2, 0, 3, 1, 4)
        return v[0], v[1], v[2]

    try:
        with torch.no_grad():
            F.scaled_dot_product_attention(*views(sets[0][0]))
        torch.cuda.synchronize()
    except Exception as err:  # noqa: BLE001 - reported, not part of the bar
        print(json.dumps({"sdpa": "unavailable", "error": str(err)[:200]}), flush=True)
        return None

    def fwd(qkv):
        with torch.no_grad():
            F.scaled_dot_product_attention(*views(qkv))

    def bwd(qkv, dout):
        leaf = qkv.detach().requires_grad_(True)
        o = F.scaled_dot_product_attention(*views(leaf))
        o.backward(dout.view(B, rows, heads, 64)[:, :N].permute(0, 2, 1, 3))

    return [lambda s=s: fwd(s[0]) for s in sets], [lambda s=s: bwd(s[0], s[1]) for s in sets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="3,6,12,16")
    ap.add_argument("--tokens", default="197", help="comma-separated token counts N")
    ap.add_argument("--arm", choices=("onepass", "stream"), default="onepass",
                    help="the HIP column: the one-pass kernels (N <= 256) or the streaming pair (N <= 2048)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench needs a GPU")
    dev = torch.device("cuda:0")
    B = args.batch
    stream = args.arm == "stream"
    hip_fwd, hip_bwd = (K.attn_stream_fwd, K.attn_stream_bwd) if stream else (K.attn_fwd, K.attn_bwd)
    bf = torch.bfloat16
    worst = {}
    shapes = [(int(h), int(n)) for n in args.tokens.split(",") for h in args.heads.split(",")]
    for rnd in range(args.rounds):
        for heads, N in shapes:
            rows = -(-N // 8) * 8
            C = heads * 64
            sets = []
            for _ in range(args.ring):
                qkv = (torch.rand(B * rows, 3 * C, device=dev) * 2 - 1).to(bf)
                dout = (torch.rand(B * rows, C, device=dev) * 2 - 1).to(bf)
                out, lse = hip_fwd(qkv, B, N, heads, img_rows=rows, torch_arm=False)
                sets.append((qkv, dout, out, lse, torch.empty_like(out), torch.empty_like(lse), torch.empty_like(qkv)))
            tok = B * N
            nbytes = {"fwd": 2.0 * tok * 4 * C + 4.0 * tok * heads, "bwd": 2.0 * tok * 8 * C + 4.0 * tok * heads}
            flops = {"fwd": 4.0 * B * heads * N * N * 64, "bwd": 10.0 * B * heads * N * N * 64}

            def arms(fwd, bwd, torch_arm):
                return {
                    "fwd": [lambda s=s: fwd(s[0], B, N, heads, img_rows=rows, out=s[4], lse=s[5], torch_arm=torch_arm)
                            for s in sets],
                    "bwd": [lambda s=s: bwd(s[0], s[2], s[3], s[1], B, N, heads, img_rows=rows, dqkv=s[6],
                                            torch_arm=torch_arm) for s in sets],
                }

            cols = {"hip": arms(hip_fwd, hip_bwd, False), "torch": arms(hip_fwd, hip_bwd, True)}
            if stream and N <= K.ATTN_MAX_N:
                cols["onepass"] = arms(K.attn_fwd, K.attn_bwd, False)
            sd = _sdpa_arms(sets, B, N, rows, heads)
            for i, pname in enumerate(("fwd", "bwd")):
                t = {c: [] for c in cols}
                for _ in range(2):  # the arms alternate
                    for c in cols:
                        t[c].append(timeit(cols[c][pname], args.iters))
                hus, tus = min(t["hip"]), min(t["torch"])
                rec = {"round": rnd, "arm": args.arm, "B": B, "N": N, "img_rows": rows, "heads": heads, "pass": pname,
                       "hip_us": round(hus, 2), "torch_us": round(tus, 2), "hip_us_all": [round(v, 2) for v in t["hip"]],
                       "torch_us_all": [round(v, 2) for v in t["torch"]], "speedup": round(tus / hus, 2),
                       "algorithmic_MB": round(nbytes[pname] / 1e6, 2), "hip_TBs": round(nbytes[pname] / hus / 1e6, 3),
                       "share_of_6.3TBs": round(nbytes[pname] / hus / 1e6 / ACHIEVABLE_TBS, 3),
                       "GFLOP": round(flops[pname] / 1e9, 2), "hip_TFs": round(flops[pname] / hus / 1e6, 1),
                       "share_of_bf16_peak": round(flops[pname] / hus / 1e6 / BF16_PEAK_TFS, 4),
                       "hip_faster": bool(hus < tus)}
                if "onepass" in t:
                    rec["onepass_us"] = round(min(t["onepass"]), 2)
                    rec["onepass_us_all"] = [round(v, 2) for v in t["onepass"]]
                if sd is not None:
                    rec["sdpa_us"] = round(timeit(sd[i], args.iters), 2)
                if not stream or N > K.ATTN_MAX_N:  # the streaming pair's bar is set above the one-pass kernels' range
                    worst[(heads, N, pname)] = worst.get((heads, N, pname), True) and rec["hip_faster"]
                print(json.dumps(rec), flush=True)
            del sets, cols, sd
            torch.cuda.empty_cache()
    lost = sorted(k for k, v in worst.items() if not v)
    print(json.dumps({"bar": "the HIP kernel faster than the torch arm on every shape and pass in every round",
                      "met": not lost, "lost": [f"heads{a}/N{n}/{b}" for a, n, b in lost]}), flush=True)


if __name__ == "__main__":
    main()
