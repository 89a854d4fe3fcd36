"""Standalone timing of the depthwise 5x5 kernels (csrc/dwconv5.hip) against the same wrappers computed with torch ops
(the SV_MBCONV=torch arm), at EfficientNet-B0's five distinct 5x5 shapes for a 256 px input, batch 32, with the stored
(zero-padded) widths: the expanded activation in front of the depthwise convolution (side x side x C) and, behind it,
side / stride.  HIP events; per shape and call the two arms alternate over a ring of operand sets, and the whole table
runs --rounds times, in the manner of tools/mbconv_bench.py.

    python tools/dwconv5_bench.py [--iters 30] [--rounds 2] [--batch 32] [--shapes s2,s5]

One JSON line per (round, shape, call).  Bytes are algorithmic: the activation operand read once and the activation
output written once in bf16 (input + output for all three calls), against the 6.3 TB/s an HBM-bound kernel reaches on the
MI355X.  ``hip_not_slower`` is the bar: the HIP arm's best time against the torch arm's best time."""

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

from mbconv_bench import ACHIEVABLE_TBS, BF, arm, timeit  # noqa: E402

# name -> (side in front of the depthwise conv, stored C, stride): B0 stages 2 (40 x 6 = 240 -> 256; its first block
# 24 x 6 = 144 -> 160), 4 (80 x 6 = 480, 112 x 6 = 672) and 5 (672 at stride 2, 192 x 6 = 1152)
SHAPES = {"s2a": (64, 160, 2), "s2": (32, 256, 1), "s4a": (16, 480, 1), "s4": (16, 672, 1), "s5a": (16, 672, 2),
          "s5": (8, 1152, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv5_bench needs a GPU")
    dev = torch.device("cuda:0")
    B = args.batch
    ok = True
    for rnd in range(args.rounds):
        for name in args.shapes.split(","):
            S, C, st = SHAPES[name]
            O = (S - 1) // st + 1
            g = torch.Generator(device="cpu").manual_seed(1)
            wdw, gdw = (torch.randn(C, 1, 5, 5, generator=g) / 5).to(dev), torch.zeros(C, 1, 5, 5, device=dev)
            xs = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]
            ds = [torch.randn(B, O, O, C, device=dev).to(BF) for _ in range(args.ring)]
            nbytes = 2.0 * (xs[0].numel() + ds[0].numel())
            calls = {
                "dwconv5_fwd": lambda t: [arm(t, lambda x=x: K.dwconv5_fwd(x, wdw, st)) for x in xs],
                "dwconv5_bwd_data": lambda t: [arm(t, lambda d=d: K.dwconv5_bwd_data(d, wdw, S, S, st)) for d in ds],
                "dwconv5_bwd_weight": lambda t: [arm(t, lambda d=d, x=x: K.dwconv5_bwd_weight(d, x, st, dw=gdw))
                                                 for d, x in zip(ds, xs)],
            }
            for cname, make in calls.items():
                harm, tarm = make(False), make(True)
                t = {"hip": [], "torch": []}
                for _ in range(2):  # the arms alternate
                    t["hip"].append(timeit(harm, args.iters))
                    t["torch"].append(timeit(tarm, args.iters))
                hus, tus = min(t["hip"]), min(t["torch"])
                tbs = nbytes / hus / 1e6
                ok = ok and hus <= tus
                print(json.dumps({"round": rnd, "shape": name, "B": B, "side": S, "C": C, "stride": st, "call": cname,
                                  "hip_us": round(hus, 2), "torch_us": round(tus, 2),
                                  "hip_us_all": [round(v, 2) for v in t["hip"]],
                                  "torch_us_all": [round(v, 2) for v in t["torch"]], "speedup": round(tus / hus, 2),
                                  "hip_not_slower": hus <= tus, "algorithmic_MB": round(nbytes / 1e6, 2),
                                  "hip_TBs": round(tbs, 3), "share_of_6.3TBs": round(tbs / ACHIEVABLE_TBS, 3)}), flush=True)
            K.MBCONV_TORCH = False
            del xs, ds
            torch.cuda.empty_cache()
    print(json.dumps({"bar": "hip not slower than torch on every shape, call and round", "holds": ok}), flush=True)


if __name__ == "__main__":
    main()
