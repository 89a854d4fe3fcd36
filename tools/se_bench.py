"""Standalone timing of the squeeze-and-excitation and avg-pool-shortcut kernels (csrc/se.hip) against the same
wrappers computed with torch ops (the SV_SE=torch arm), at the four bottleneck-output shapes of ResNet-RS at 256 px,
batch 32 (64x64x256, 32x32x512, 16x16x1024, 8x8x2048; rd = C / 4) and, for the pool, at the three shortcut inputs it
halves.  HIP events; per shape and pass the two arms alternate, and the whole table runs --rounds times.

    python tools/se_bench.py [--iters 30] [--rounds 2] [--batch 32] [--shapes l1,l4]

One JSON line per (round, shape, pass).  Bytes are algorithmic: every activation operand read once and every activation
output written once in bf16 (squeeze: y; join: y + shortcut + out; pass A: dout read and written + out + y; pass B:
g + y + dy; pool: input + output), the excite and the gate backward by their f32 weights (read once; the gate backward
also reads and writes both weight gradients), against the 6.3 TB/s an HBM-bound kernel reaches on the MI355X.  Each
arm walks a ring of --ring operand sets so that a timed launch does not find its own previous output in the caches."""

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

# name -> (side, C) of the bottleneck output; the pool halves the previous stage's output into this stage's shortcut
SHAPES = {"l1": (64, 256), "l2": (32, 512), "l3": (16, 1024), "l4": (8, 2048)}
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
        K.SE_TORCH = torch_arm
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
        raise SystemExit("se_bench needs a GPU")
    dev = torch.device("cuda:0")
    B = args.batch
    worst = {}
    for rnd in range(args.rounds):
        for name in args.shapes.split(","):
            S, C = SHAPES[name]
            rd, HW = C // 4, S * S
            g = torch.Generator(device="cpu").manual_seed(1)
            f = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
            mean, rstd, gamma, beta = f(C) * 0.1, torch.rand(C, generator=g).to(dev) + 0.5, f(C), f(C) * 0.1
            w1, b1, w2, b2 = f(rd, C, 1, 1) * (2 / rd) ** 0.5, f(rd) * 0.1, f(C, rd, 1, 1) * (2 / C) ** 0.5, f(C) * 0.1
            ys = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]
            rs = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]
            ds = [torch.randn(B, S, S, C, device=dev).to(BF) for _ in range(args.ring)]
            K.SE_TORCH = False
            part = K.se_squeeze(ys[0])
            st = K.se_excite(part, HW, mean, rstd, gamma, beta, w1, b1, w2, b2)
            outs = [K.se_join(y, mean, rstd, gamma, beta, st[3], r, out_dtype=BF) for y, r in zip(ys, rs)]
            bpart = K.se_bwd_stats(ds[0].clone(), outs[0], ys[0], mean, rstd)
            dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
            dgm, dbt = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            gate_kw = dict(dw1=dw1, db1=db1, dw2=dw2, db2=db2, dgamma=dgm, dbeta=dbt)
            dpool, sums = K.se_bwd_gate(bpart, st, HW, mean, rstd, gamma, beta, w1, w2, **gate_kw)
            # the torch arm's partials have one part per image
            K.SE_TORCH = True
            tpart, tbpart = K.se_squeeze(ys[0]), K.se_bwd_stats(ds[0].clone(), outs[0], ys[0], mean, rstd)
            K.SE_TORCH = False
            n2 = 2.0 * ys[0].numel()
            wb = 4.0 * 2 * rd * C
            passes = {
                "squeeze": (n2, lambda t: [arm(t, lambda y=y: K.se_squeeze(y)) for y in ys]),
                "excite": (wb, lambda t: [arm(t, lambda: K.se_excite(tpart if t else part, HW, mean, rstd, gamma, beta,
                                                                    w1, b1, w2, b2))]),
                "join": (3 * n2, lambda t: [arm(t, lambda y=y, r=r: K.se_join(y, mean, rstd, gamma, beta, st[3], r,
                                                                            out_dtype=BF)) for y, r in zip(ys, rs)]),
                "bwd_stats": (4 * n2, lambda t: [arm(t, lambda d=d, o=o, y=y: K.se_bwd_stats(d, o, y, mean, rstd))
                                                 for d, o, y in zip(ds, outs, ys)]),
                "bwd_gate": (3 * wb, lambda t: [arm(t, lambda: K.se_bwd_gate(tbpart if t else bpart, st, HW, mean, rstd,
                                                                            gamma, beta, w1, w2, **gate_kw))]),
                "bwd_apply": (3 * n2, lambda t: [arm(t, lambda d=d, y=y: K.se_bwd_apply(d, y, mean, rstd, gamma, st[3],
                                                                                      dpool, sums, dx_dtype=BF))
                                                 for d, y in zip(ds, ys)]),
            }
            if name != "l1":  # the shortcut pool of this stage's first block: the previous stage's output, halved
                xs = [torch.randn(B, 2 * S, 2 * S, C // 2, device=dev).to(BF) for _ in range(args.ring)]
                dps = [torch.randn(B, S, S, C // 2, device=dev).to(BF) for _ in range(args.ring)]
                pb = 2.0 * (xs[0].numel() + dps[0].numel())
                passes["avgpool2x2_fwd"] = (pb, lambda t: [arm(t, lambda x=x: K.avgpool2x2_fwd(x)) for x in xs])
                passes["avgpool2x2_bwd"] = (pb, lambda t: [arm(t, lambda d=d: K.avgpool2x2_bwd(d, 2 * S, 2 * S, dx_dtype=BF))
                                                           for d in dps])
            for pname, (nbytes, make) in passes.items():
                harm, tarm = make(False), make(True)
                t = {"hip": [], "torch": []}
                for _ in range(2):  # the arms alternate
                    t["hip"].append(timeit(harm, args.iters))
                    t["torch"].append(timeit(tarm, args.iters))
                hus, tus = min(t["hip"]), min(t["torch"])
                tbs = nbytes / hus / 1e6
                rec = {"round": rnd, "shape": name, "B": B, "side": S, "C": C, "rd": rd, "pass": pname,
                       "hip_us": round(hus, 2), "torch_us": round(tus, 2), "hip_us_all": [round(v, 2) for v in t["hip"]],
                       "torch_us_all": [round(v, 2) for v in t["torch"]], "speedup": round(tus / hus, 2),
                       "algorithmic_MB": round(nbytes / 1e6, 2), "hip_TBs": round(tbs, 3),
                       "share_of_6.3TBs": round(tbs / ACHIEVABLE_TBS, 3), "hip_faster": bool(hus < tus)}
                worst[(name, pname)] = worst.get((name, pname), True) and rec["hip_faster"]
                print(json.dumps(rec), flush=True)
            K.SE_TORCH = False
            del ys, rs, ds, outs
            torch.cuda.empty_cache()
    lost = sorted(k for k, v in worst.items() if not v)
    print(json.dumps({"bar": "HIP arm faster than the torch arm on every shape and pass in every round", "met": not lost,
                      "lost": [f"{a}/{b}" for a, b in lost]}), flush=True)


if __name__ == "__main__":
    main()
