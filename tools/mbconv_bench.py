"""Standalone timing of the MBConv kernels (csrc/mbconv.hip) against the same wrappers computed with torch ops (the
SV_MBCONV=torch arm), at the InvertedResidual shapes of EfficientNetV2-S at 256 px, batch 32: the expanded activation in
front of the depthwise 3x3 (side x side x C) and, behind it, side / stride.  HIP events; per shape and pass the two arms
alternate, and the whole table runs --rounds times.

    python tools/mbconv_bench.py [--iters 30] [--rounds 2] [--batch 32] [--shapes s3a,s5]

One JSON line per (round, shape, pass).  Bytes are algorithmic: every activation operand read once and every activation
output written once in bf16 (the depthwise passes: input + output; BatchNorm + SiLU forward: y + out; its backward
statistics: dout + y; its apply: dout + y + dx; squeeze and forward statistics: y; scale: y + out; backward pass A: da +
y; pass B: da + y + dpre), the excite and the gate backward by their f32 weights, against the 6.3 TB/s an HBM-bound kernel
reaches on the MI355X.  Each arm walks a ring of --ring operand sets so that a timed launch does not find its own
previous output in the caches."""

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

# name -> (side in front of the depthwise conv, C, stride, rd): the first and the later blocks of S's stages 3, 4, 5
SHAPES = {"s3a": (32, 256, 2, 16), "s3": (16, 512, 1, 32), "s4a": (16, 768, 1, 32), "s4": (16, 960, 1, 40),
          "s5a": (16, 960, 2, 40), "s5": (8, 1536, 1, 64)}
ACHIEVABLE_TBS = 6.3
BF = torch.bfloat16


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


def arm(torch_arm, fn):
    def run():
        K.MBCONV_TORCH = torch_arm
        fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mbconv_bench needs a GPU")
    dev = torch.device("cuda:0")
    B = args.batch
    for rnd in range(args.rounds):
        for name in args.shapes.split(","):
            S, C, st, rd = SHAPES[name]
            O = (S - 1) // st + 1
            g = torch.Generator(device="cpu").manual_seed(1)
            f = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
            bn = (f(C) * 0.1, torch.rand(C, generator=g).to(dev) + 0.5, f(C), f(C) * 0.1)
            w1, b1, w2, b2 = f(rd, C, 1, 1) * (2 / rd) ** 0.5, f(rd) * 0.1, f(C, rd, 1, 1) * (2 / C) ** 0.5, f(C) * 0.1
            wdw, gdw = f(C, 1, 3, 3) / 3, torch.zeros(C, 1, 3, 3, device=dev)
            xs = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]   # the depthwise conv's side
            dxs = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]
            ys = [torch.randn(B, O, O, C, device=dev).to(BF) for _ in range(args.ring)]   # behind it
            ds = [torch.randn(B, O, O, C, device=dev).to(BF) for _ in range(args.ring)]
            sums = torch.zeros(2, C, device=dev)
            parts, states, bparts, dpools = {}, {}, {}, {}
            for t in (False, True):  # each arm's own partials (the torch arm's have one part per image)
                K.MBCONV_TORCH = t
                parts[t] = K.mbse_squeeze(ys[0], bn)
                states[t] = K.mbse_excite(parts[t], O * O, w1, b1, w2, b2)
                bparts[t] = K.mbse_bwd_stats(ds[0], ys[0], bn)
                gk = dict(dw1=torch.zeros_like(w1), db1=torch.zeros_like(b1), dw2=torch.zeros_like(w2), db2=torch.zeros_like(b2))
                dpools[t] = K.mbse_bwd_gate(bparts[t], states[t], w1, w2, **gk)
            K.MBCONV_TORCH = False
            n_in, n_out, wb = 2.0 * xs[0].numel(), 2.0 * ys[0].numel(), 4.0 * 2 * rd * C
            v2 = lambda t: t.view(-1, C)  # noqa: E731
            passes = {
                "dwconv3_fwd": (n_in + n_out, lambda t: [arm(t, lambda x=x: K.dwconv3_fwd(x, wdw, st)) for x in xs]),
                "dwconv3_bwd_data": (n_in + n_out, lambda t: [arm(t, lambda d=d: K.dwconv3_bwd_data(d, wdw, S, S, st)) for d in ds]),
                "dwconv3_bwd_weight": (n_in + n_out, lambda t: [arm(t, lambda d=d, x=x: K.dwconv3_bwd_weight(d, x, st, dw=gdw))
                                                                for d, x in zip(ds, xs)]),
                "bn_stats": (n_out, lambda t: [arm(t, lambda y=y: K.mb_bn_stats(v2(y))) for y in ys]),
                "bn_silu_fwd": (2 * n_in, lambda t: [arm(t, lambda x=x: K.bn_silu_fwd(v2(x), bn, out_dtype=BF)) for x in xs]),
                "bn_silu_bwd_stats": (2 * n_in, lambda t: [arm(t, lambda d=d, x=x: K.bn_silu_bwd_stats(v2(d), v2(x), bn))
                                                           for d, x in zip(dxs, xs)]),
                "bn_silu_bwd_apply": (3 * n_in, lambda t: [arm(t, lambda d=d, x=x: K.bn_silu_bwd_apply(v2(d), v2(x), bn, sums,
                                                                                                     dx_dtype=BF))
                                                           for d, x in zip(dxs, xs)]),
                "se_squeeze": (n_out, lambda t: [arm(t, lambda y=y: K.mbse_squeeze(y, bn)) for y in ys]),
                "se_excite": (wb, lambda t: [arm(t, lambda: K.mbse_excite(parts[t], O * O, w1, b1, w2, b2))]),
                "se_scale": (2 * n_out, lambda t: [arm(t, lambda y=y: K.mbse_scale(y, bn, states[t][3], out_dtype=BF)) for y in ys]),
                "se_bwd_stats": (2 * n_out, lambda t: [arm(t, lambda d=d, y=y: K.mbse_bwd_stats(d, y, bn)) for d, y in zip(ds, ys)]),
                "se_bwd_gate": (3 * wb, lambda t: [arm(t, lambda: K.mbse_bwd_gate(bparts[t], states[t], w1, w2, **gk))]),
                "se_bwd_apply": (3 * n_out, lambda t: [arm(t, lambda d=d, y=y: K.mbse_bwd_apply(d, y, bn, states[t][3], dpools[t],
                                                                                              out_dtype=BF))
                                                       for d, y in zip(ds, ys)]),
            }
            for pname, (nbytes, make) in passes.items():
                harm, tarm = make(False), make(True)
                t = {"hip": [], "torch": []}
                for _ in range(2):  # the arms alternate
                    t["hip"].append(timeit(harm, args.iters))
                    t["torch"].append(timeit(tarm, args.iters))
                hus, tus = min(t["hip"]), min(t["torch"])
                tbs = nbytes / hus / 1e6
                print(json.dumps({"round": rnd, "shape": name, "B": B, "side": S, "C": C, "stride": st, "rd": rd, "pass": pname,
                                  "hip_us": round(hus, 2), "torch_us": round(tus, 2),
                                  "hip_us_all": [round(v, 2) for v in t["hip"]],
                                  "torch_us_all": [round(v, 2) for v in t["torch"]], "speedup": round(tus / hus, 2),
                                  "algorithmic_MB": round(nbytes / 1e6, 2), "hip_TBs": round(tbs, 3),
                                  "share_of_6.3TBs": round(tbs / ACHIEVABLE_TBS, 3)}), flush=True)
            K.MBCONV_TORCH = False
            del xs, dxs, ys, ds
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
