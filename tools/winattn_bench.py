"""Standalone timing of the Swin window-attention kernels (csrc/swin.hip: sv_winattn_fwd / sv_winattn_bwd with the
bias-table gradient fold sv_swin_bias_grad) against the SV_WINATTN=torch arm (the same maths as torch gather / matmul
/ softmax / scatter ops) at the four stage shapes of swin_small and swin_base at 224 px: grids 56, 28, 14, 7 with
window 7, heads 3, 6, 12, 24 (small) and 4, 8, 16, 32 (base), shift 3 where the grid exceeds the window, batch 32.
HIP events; per shape and pass the arms alternate, and the whole table runs --rounds times.

    python tools/winattn_bench.py [--iters 20] [--rounds 2] [--batch 32] [--models swin_small,swin_base] [--size 224]

One JSON line per (round, model, stage, pass).  The backward of both arms includes the fold of the bias gradient into
the table.  Bytes are algorithmic (forward: qkv read, out and lse written; backward: qkv, out, dout, lse read, dqkv
written) against the 6.3 TB/s an HBM-bound kernel reaches on the MI355X.  Each arm walks a ring of --ring operand sets
so that a timed launch does not find its own previous output in the caches."""

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
from spine_vision_amd.backbone.swin import PATCH, SWIN_CFGS, window_for  # noqa: E402

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
    ap.add_argument("--models", default="swin_small,swin_base")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("winattn_bench needs a GPU")
    dev = torch.device("cuda:0")
    B, bf = args.batch, torch.bfloat16
    wfull = window_for(args.size)
    shapes = []
    for model in args.models.split(","):
        for s, heads in enumerate(SWIN_CFGS[model][2]):
            g = args.size // PATCH // 2 ** s
            w = min(wfull, g)
            shapes.append((model, s, g, w, wfull // 2 if g > wfull else 0, heads))
    lost = []
    for rnd in range(args.rounds):
        for model, stage, g, w, shift, heads in shapes:
            C, rows = heads * 32, -(-(B * g * g) // 8) * 8
            table = (torch.rand((2 * w - 1) ** 2, heads, device=dev) * 2 - 1) * 0.5
            bias = K.swin_bias_expand(table, w)
            sets = []
            for _ in range(args.ring):
                qkv = (torch.rand(rows, 3 * C, device=dev) * 2 - 1).to(bf)
                dout = (torch.rand(rows, C, device=dev) * 2 - 1).to(bf)
                out, lse = K.winattn_fwd(qkv, bias, B, g, g, w, shift, heads, torch_arm=False)
                sets.append((qkv, dout, out, lse))
            dtable = torch.zeros_like(table)

            def fwd(s, arm):
                K.winattn_fwd(s[0], bias, B, g, g, w, shift, heads, torch_arm=arm)

            def bwd(s, arm):
                _, part = K.winattn_bwd(s[0], s[2], s[3], s[1], bias, B, g, g, w, shift, heads, torch_arm=arm)
                K.swin_bias_grad(part, dtable, w, accumulate=True)

            tok = B * g * g
            nbytes = {"fwd": 2.0 * tok * 4 * C + 4.0 * tok * heads, "bwd": 2.0 * tok * 8 * C + 4.0 * tok * heads}
            for pname, fn in (("fwd", fwd), ("bwd", bwd)):
                cols = {"hip": [lambda s=s: fn(s, False) for s in sets], "torch": [lambda s=s: fn(s, True) for s in sets]}
                t = {c: [] for c in cols}
                for _ in range(2):  # the arms alternate
                    for c in cols:
                        t[c].append(timeit(cols[c], args.iters))
                hus, tus = min(t["hip"]), min(t["torch"])
                rec = {"round": rnd, "model": model, "stage": stage, "B": B, "grid": g, "window": w, "shift": shift,
                       "heads": heads, "pass": pname, "hip_us": round(hus, 2), "torch_us": round(tus, 2),
                       "hip_us_all": [round(v, 2) for v in t["hip"]], "torch_us_all": [round(v, 2) for v in t["torch"]],
                       "speedup": round(tus / hus, 2), "algorithmic_MB": round(nbytes[pname] / 1e6, 2),
                       "hip_TBs": round(nbytes[pname] / hus / 1e6, 3),
                       "share_of_6.3TBs": round(nbytes[pname] / hus / 1e6 / ACHIEVABLE_TBS, 3),
                       "hip_faster": bool(hus < tus)}
                if not rec["hip_faster"]:
                    lost.append(f"round{rnd}/{model}/stage{stage}/{pname}")
                print(json.dumps(rec), flush=True)
            del sets
            torch.cuda.empty_cache()
    print(json.dumps({"bar": "the HIP kernel faster than the torch arm on every shape and pass in every round",
                      "met": not lost, "lost": lost}), flush=True)


if __name__ == "__main__":
    main()
