"""What tests/test_se_calls_gpu.py and tests/test_mbconv_calls_gpu.py share: the per-element verdict and the depths of the
squeeze-and-excitation gate's sums, whose orders csrc/se_core.h states once for both kernel files."""
import pytest
import torch

from _conv_ref import BF, U8


def judge(tag, where, got, refs):
    """every element of every output within 2 x bound; prints the largest error / bound per output"""
    figs = []
    for n, (ref, bound) in refs.items():
        g = got[n].double().reshape(ref.shape)
        err = (g - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
        worst = float(ratio.max())
        figs.append(f"{n} err {float(err.max()):.3e} ratio {worst:.3f}")
        if not worst <= 2.0:
            flat = int(ratio.reshape(-1).argmax())
            print(f"[{tag}] {where}: " + ", ".join(figs))
            pytest.fail(f"{where} {n}: {int((ratio > 2).sum())} of {ratio.numel()} elements beyond 2 x bound; worst at flat "
                        f"{flat}: got {float(g.reshape(-1)[flat]):.9g}, float64 {float(ref.reshape(-1)[flat]):.9g}, "
                        f"bound {float(bound.reshape(-1)[flat]):.3e}, error / bound {worst:.3g}")
    print(f"[{tag}] {where}: " + ", ".join(figs))


def store(ref, dtype):
    return U8 * ref.abs() if dtype == BF else torch.zeros_like(ref)


def f32(t):
    return t.float().double()


def mv_depth(Kd):
    return 4 * (-(-Kd // 256)) + 7


def tm_depth(Kd):
    return -(-Kd // 16) + 15
