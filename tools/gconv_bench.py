"""Standalone timing of the grouped 3x3 convolution kernels (csrc/gconv.hip) against the dense embedding of the same
weights through the bf16 implicit-GEMM kernels (the SV_GCONV=dense arm), at the seven distinct conv2 shapes of
ResNeXt-50 (32x4d) at 256 px, batch 32: the four stride-1 shapes of layers 1-4 and the three strided ones that open
layers 2-4.  HIP events; per shape and pass the two arms alternate, and the whole table runs --rounds times.

    python tools/gconv_bench.py [--iters 30] [--rounds 2] [--batch 32] [--shapes l1,l4s]

One JSON line per (round, shape, pass).  Bytes are algorithmic: the input activation read once and the output written
once (forward: x + y, backward-data: dy + dx, backward-weight: x + dy; weights, packed forms and the weight gradient's
partials are not counted), against the 6.3 TB/s an HBM-bound kernel reaches on the MI355X.  Each arm walks a ring of
--ring operand sets so that a timed launch does not find its own previous output in the caches; the weight pack is
outside the timed region for both arms (the model packs once per forward in one launch)."""

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

# name -> (input side, C, stride); groups 32
SHAPES = {"l1": (64, 128, 1), "l2": (32, 256, 1), "l3": (16, 512, 1), "l4": (8, 1024, 1),
          "l2s": (64, 256, 2), "l3s": (32, 512, 2), "l4s": (16, 1024, 2)}
GROUPS = 32
ACHIEVABLE_TBS = 6.3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench needs a GPU")
    dev = torch.device("cuda:0")
    B = args.batch
    worst = {}
    for rnd in range(args.rounds):
        for name in args.shapes.split(","):
            S, C, stride = SHAPES[name]
            gs = K.gconv_shape(B, S, S, C, GROUPS, 3, stride, 1)
            ds = K.conv_shape(B, S, S, C, C, 3, stride, 1)
            OS = (S - 1) // stride + 1
            g = torch.Generator(device="cpu").manual_seed(1)
            w = (torch.randn(C, C // GROUPS, 3, 3, generator=g) / (3.0 * (C // GROUPS) ** 0.5)).to(dev)
            gwp, = K.gconv_weight_pack([w], GROUPS)
            dwp = K.conv_weight_pack(K.grouped_as_dense(w, GROUPS).contiguous(), C, torch.bfloat16)
            xs = [torch.randn(B, S, S, C, device=dev).to(torch.bfloat16) for _ in range(args.ring)]
            dys = [(0.5 * torch.randn(B, OS, OS, C, device=dev)).to(torch.bfloat16) for _ in range(args.ring)]
            gdw, ddw = torch.zeros_like(w), torch.zeros(C, C, 3, 3, device=dev)
            nbytes = 2.0 * (xs[0].numel() + dys[0].numel())
            passes = {
                "fwd": ([lambda x=x: K.gconv_fwd(x, gwp, gs) for x in xs],
                        [lambda x=x: K.conv_fwd(x, dwp, ds, torch.bfloat16) for x in xs]),
                "bwd_data": ([lambda d=d: K.gconv_bwd_data(d, gwp, gs) for d in dys],
                             [lambda d=d: K.conv_bwd_data(d, dwp, ds, dx_dtype=torch.bfloat16) for d in dys]),
                "bwd_weight": ([lambda d=d, x=x: K.gconv_bwd_weight(d, x, gs, dw=gdw, accumulate=True)
                                for d, x in zip(dys, xs)],
                               [lambda d=d, x=x: K.conv_bwd_weight(d, x, ds, dw=ddw, accumulate=True)
                                for d, x in zip(dys, xs)]),
            }
            for pname, (garm, darm) in passes.items():
                t = {"grouped": [], "dense": []}
                for _ in range(2):  # the arms alternate
                    t["grouped"].append(timeit(garm, args.iters))
                    t["dense"].append(timeit(darm, args.iters))
                gus, dus = min(t["grouped"]), min(t["dense"])
                tbs = nbytes / gus / 1e6
                rec = {"round": rnd, "shape": name, "B": B, "side": S, "C": C, "stride": stride, "pass": pname,
                       "grouped_us": round(gus, 2), "dense_us": round(dus, 2), "grouped_us_all": [round(v, 2) for v in t["grouped"]],
                       "dense_us_all": [round(v, 2) for v in t["dense"]], "speedup": round(dus / gus, 2),
                       "algorithmic_MB": round(nbytes / 1e6, 2), "grouped_TBs": round(tbs, 3),
                       "share_of_6.3TBs": round(tbs / ACHIEVABLE_TBS, 3), "grouped_faster": bool(gus < dus)}
                worst[(name, pname)] = worst.get((name, pname), True) and rec["grouped_faster"]
                print(json.dumps(rec), flush=True)
            del xs, dys
            torch.cuda.empty_cache()
    lost = sorted(k for k, v in worst.items() if not v)
    print(json.dumps({"bar": "grouped faster than dense on every shape and pass in every round", "met": not lost,
                      "lost": [f"{a}/{b}" for a, b in lost]}), flush=True)


if __name__ == "__main__":
    main()
