"""bf16 train step (forward + explicit backward of the backbone, features -> a fixed feature gradient) of
``efficientnet_b0`` / ``efficientnet_b4`` at 256 px, batch 32: the HIP arm against the SV_MBCONV=torch arm (every
csrc/mbconv.hip and csrc/dwconv5.hip wrapper computed with torch ops), interleaved.  bench.py goes through the gated
factory, so this script builds the backbone with ``create_efficientnet``.

    python tools/effnet_b_step_bench.py [--models efficientnet_b0,efficientnet_b4] [--steps 10] [--warmup 3] [--rounds 2]

One JSON line per (round, model); the bar is ``hip_not_slower``."""

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
from spine_vision_amd.backbone import create_efficientnet  # noqa: E402


def step_ms(model, img, dfeat, torch_arm, steps, warmup):
    K.MBCONV_TORCH = torch_arm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            e0.record()
        model(img).backward(dfeat)
    e1.record()
    torch.cuda.synchronize()
    K.MBCONV_TORCH = False
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="efficientnet_b0,efficientnet_b4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("effnet_b_step_bench needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = create_efficientnet(name, precision="bf16").to(dev).train()
        img = torch.randn(args.batch, 3, args.size, args.size, device=dev)
        dfeat = torch.randn(args.batch, model.num_features, device=dev) / model.num_features
        for rnd in range(args.rounds):
            hip = step_ms(model, img, dfeat, False, args.steps, args.warmup)
            tor = step_ms(model, img, dfeat, True, args.steps, args.warmup)
            print(json.dumps({"round": rnd, "model": name, "batch": args.batch, "size": args.size, "precision": "bf16",
                              "hip_step_ms": round(hip, 3), "torch_arm_step_ms": round(tor, 3),
                              "hip_img_s": round(args.batch / hip * 1e3, 1), "ratio_torch_over_hip": round(tor / hip, 3),
                              "hip_not_slower": hip <= tor}), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
