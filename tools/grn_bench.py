"""Standalone timing of the six Global Response Normalization kernels (csrc/grn.hip) at the hidden-activation shapes
of the ConvNeXt V2-base @512 bs32 stages (HIP events), against the 6.3 TB/s an HBM-bound kernel can reach on the
MI355X, with the LayerNorm forward on the same row counts in the same run as the comparator.

    python tools/grn_bench.py [--stages S1,S3] [--iters 20] [--batch 32] [--dtype bf16]

Bytes are algorithmic: every activation read or written once; the per-chunk partial sums a pass chooses to write for
the finish pass are not counted (the finish passes move only those and are reported in microseconds)."""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from spine_vision_amd import kernels as K  # noqa: E402

STAGES = {"S1": (128, 128), "S2": (64, 256), "S3": (32, 512), "S4": (16, 1024)}  # (feature-map side, C); n = 4C
ACHIEVABLE_TBS = 6.3


def timeit(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", default="S1,S2,S3,S4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    es = 2 if args.dtype == "bf16" else 4
    B = args.batch
    for st in args.stages.split(","):
        S, C = STAGES[st]
        HW, n = S * S, 4 * C
        M = B * HW
        a = torch.nn.functional.gelu(torch.randn(M, n, device=dev)).to(dtype)
        du = (0.1 * torch.randn(M, n, device=dev)).to(dtype)
        gh = torch.rand(M, n, device=dev).to(dtype)
        u, dh = torch.empty_like(a), torch.empty_like(a)
        gamma, beta = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) - 0.5
        dgamma, dbeta = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        part = K.grn_stats(a, B)
        G, N, scale, D = K.grn_finish(part, gamma)
        sp, dp = K.grn_bwd_stats(du, a, B)
        k = K.grn_bwd_finish(sp, dp, gamma, G, N, D, dgamma=dgamma, dbeta=dbeta)
        e = M * n
        x = torch.randn(M, C, device=dev).to(dtype)
        lnw, lnb = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        cases = [
            ("grn_stats", es * e, lambda: K.grn_stats(a, B)),
            ("grn_finish", 0, lambda: K.grn_finish(part, gamma)),
            ("grn_apply", 2 * es * e, lambda: K.grn_apply(a, scale, beta, out=u)),
            ("grn_bwd_stats", 2 * es * e, lambda: K.grn_bwd_stats(du, a, B)),
            ("grn_bwd_finish", 0, lambda: K.grn_bwd_finish(sp, dp, gamma, G, N, D, dgamma=dgamma, dbeta=dbeta)),
            ("grn_bwd_apply", 4 * es * e, lambda: K.grn_bwd_apply(du, a, gh, scale, k, out=dh)),
            ("ln_fwd [M, C] (comparator)", 2 * es * M * C + 8 * M, lambda: K.layernorm_fwd(x, lnw, lnb, out_dtype=dtype)),
        ]
        print(f"{st}: B {B} HW {HW} n {n} ({args.dtype}), {part.shape[1]} chunks per image", flush=True)
        for name, nbytes, fn in cases:
            us = timeit(fn, args.iters)
            if nbytes:
                tbs = nbytes / us / 1e6
                print(f"  {name:28s} {us:9.1f} us  {tbs:6.2f} TB/s  {100 * tbs / ACHIEVABLE_TBS:5.1f} % of "
                      f"{ACHIEVABLE_TBS} TB/s", flush=True)
            else:
                print(f"  {name:28s} {us:9.1f} us", flush=True)
        del a, du, gh, u, dh, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
