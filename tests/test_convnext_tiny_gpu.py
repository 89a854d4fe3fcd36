"""GPU: the ConvNeXt-tiny / small backbones (stage-1 width C = 96) through the HIP path against the oracle module
(oracle/convnext.py) on identical generated weights (oracle.weights.fill_module).  Everything at 2 x 64 x 64.

fp32 bounds are the V1 ones of tests/test_backbone_gpu.py (features 1e-4, every gradient 1e-3, relative L2 per
tensor).  bf16 is held against the reference recipe's own rounding as in tests/test_convnextv2_gpu.py: the oracle
module under torch.autocast(bf16) on the CPU, whose distance to its fp32 result is computed in the same test; the HIP
distance may be at most 1.5 x it (features; median and worst per-tensor gradient)."""

import functools
import math

import numpy as np
import pytest
import torch

from oracle import convnext as oc
from oracle import heads as oh
from oracle import step as ostep
from oracle import weights as ow
from spine_vision_amd.backbone import create_convnext

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _dfeat(f):
    return torch.from_numpy(ow.uniform("dfeat", f.numel(), -1, 1).reshape(f.shape))


def _oracle(name):
    if name == "convnext_small":  # the oracle registry has no entry for it: tiny's dims at base's depths
        return oc.ConvNeXt((3, 3, 27, 3), (96, 192, 384, 768))
    return oc.create(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle module, its fp32 features and gradients on the shared batch (computed once per backbone)."""
    ref = ow.fill_module(_oracle(name))
    img, _, _ = ow.localization_batch(2, 64, 64)
    f = ref(img)
    f.backward(_dfeat(f))
    grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    ref.zero_grad(set_to_none=True)
    return ref, img, f.detach(), grads


def _hip(name, precision, dev):
    ref = _reference(name)[0]
    hip = create_convnext(name, precision=precision)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.to(dev)


def _hip_grads(hip, img, dev):
    f = hip(img.to(dev))
    f.backward(_dfeat(f).to(dev))
    torch.cuda.synchronize()
    return f.detach(), {n: p.grad.detach().clone() for n, p in hip.named_parameters()}


@pytest.mark.parametrize("name", ["convnext_tiny", "convnext_small"])
def test_tiny_fp32_forward_backward(dev, name):
    ref, img, f_ref, g_ref = _reference(name)
    f_hip, g_hip = _hip_grads(_hip(name, "fp32", dev), img, dev)
    assert tuple(f_hip.shape) == (2, 768)
    assert list(g_hip) == list(g_ref)
    errs = {n: rel(g_hip[n], g) for n, g in g_ref.items()}
    print(f"{name}@64 fp32: features {rel(f_hip, f_ref):.2e}, worst grad {max(errs.values()):.2e} "
          f"({max(errs, key=errs.get)})")
    assert rel(f_hip, f_ref) < 1e-4
    bad = {n: e for n, e in errs.items() if not e < 1e-3}
    assert not bad, bad


def test_tiny_bf16_no_farther_than_autocast(dev):
    name = "convnext_tiny"
    ref, img, f_ref, g_ref = _reference(name)
    # the reference's own mixed-precision recipe at bf16 width, on the CPU
    with torch.autocast("cpu", dtype=torch.bfloat16):
        f_auto = ref(img)
    f_auto.float().backward(_dfeat(f_auto))
    g_auto = {n: p.grad.detach().float().clone() for n, p in ref.named_parameters()}
    ref.zero_grad(set_to_none=True)
    fa = rel(f_auto.float(), f_ref)
    ea = {n: rel(g_auto[n], g) for n, g in g_ref.items()}
    ma = float(np.median(list(ea.values())))
    wa = max(ea, key=ea.get)
    # the yardstick itself: finite, and a bf16-sized distance (not zero, not garbage)
    assert all(math.isfinite(v) for v in [fa, ma, *ea.values()])
    assert 1e-4 < fa < 0.1 and 1e-4 < ma < 0.1 and ea[wa] < 0.5, (fa, ma, ea[wa])
    f_hip, g_hip = _hip_grads(_hip(name, "bf16", dev), img, dev)
    fh = rel(f_hip, f_ref)
    eh = {n: rel(g_hip[n], g) for n, g in g_ref.items()}
    mh = float(np.median(list(eh.values())))
    wh = max(eh, key=eh.get)
    print(f"[parity] {name}@64 B2 bf16 vs fp32 -- autocast: features {fa:.3e} grad median {ma:.3e} worst {ea[wa]:.3e} "
          f"({wa}); HIP: features {fh:.3e} grad median {mh:.3e} worst {eh[wh]:.3e} ({wh}); ratios features "
          f"{fh / fa:.2f} median {mh / ma:.2f} worst {eh[wh] / ea[wa]:.2f}")
    assert fh <= 1.5 * fa, (fh, fa)
    assert mh <= 1.5 * ma, (mh, ma)
    assert eh[wh] <= 1.5 * ea[wa], (wh, eh[wh], wa, ea[wa])


def test_tiny_bf16_schedules_bitwise_equal(dev):
    """The lean side-stream backward, the inline one (weight gradients on the main stream) and the eager side-stream
    one run the same kernels: features and every gradient equal bit for bit."""
    _, img, _, _ = _reference("convnext_tiny")
    out = []
    for overlap, lean in ((True, True), (False, True), (True, False)):
        hip = _hip("convnext_tiny", "bf16", dev)
        assert hip.lean_sync
        hip.overlap_wgrad, hip.lean_sync = overlap, lean
        out.append(_hip_grads(hip, img, dev))
    for f, grads in out[1:]:
        assert torch.equal(out[0][0], f)
        for n in out[0][1]:
            assert torch.equal(out[0][1][n], grads[n]), n


@pytest.mark.parametrize("precision,overlap", [("bf16", True), ("bf16", False), ("fp32", True)])
def test_tiny_reports_every_parameter_ready(dev, precision, overlap):
    """grad_ready_hook sees every trainable parameter exactly once (a missing report leaves a DDP bucket open)."""
    _, img, _, _ = _reference("convnext_tiny")
    hip = _hip("convnext_tiny", precision, dev)
    hip.overlap_wgrad = overlap
    seen: list = []
    hip.grad_ready_hook = seen.extend
    _hip_grads(hip, img, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert all(id(p) in names for p in seen)
    reported = sorted(names[id(p)] for p in seen)
    assert reported == sorted(n for n, p in hip.named_parameters() if p.requires_grad)


def test_tiny_eval_forward_equals_training_forward(dev):
    """The tape-free forward gives the training forward's features bit for bit (fp32)."""
    _, img, f_ref, _ = _reference("convnext_tiny")
    hip = _hip("convnext_tiny", "fp32", dev)
    f_train = hip(img.to(dev)).detach()
    with torch.no_grad():
        f_eval = hip.eval()(img.to(dev))
    assert torch.equal(f_train, f_eval)
    assert rel(f_eval, f_ref) < 1e-4


def test_tiny_train_step_matches_torch(dev):
    """One fp32 StepEngine.step_localization on CoordinateRegressor(convnext_tiny) against the torch reference step
    (as __graft_entry__.smoke does for convnext_base)."""
    from spine_vision_amd.training import CoordinateRegressor, StepEngine

    ref = oh.CoordinateRegressor(oc.create("convnext_tiny"), 768, dropout=0.0)
    ow.fill_module(ref)
    hip = CoordinateRegressor("convnext_tiny", pretrained=False, dropout=0.0, precision="fp32")
    missing, unexpected = hip.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and not [k for k in missing if "num_batches" not in k]
    hip = hip.to(dev).train()
    ref.train()
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    img, coords, mask = ow.localization_batch(2, 64, 64)
    opt = ostep.make_optimizer(ref)
    loss_ref, pred_ref, norm_ref = ostep.train_step_localization(ref, opt, img, coords, mask)
    eng = StepEngine(hip, dev, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    with torch.no_grad():
        pred = hip(img.to(dev))
    loss = eng.step_localization(img.to(dev), coords.to(dev), mask.to(dev))
    torch.cuda.synchronize()
    r_pred = rel(pred, pred_ref)
    r_loss = abs(float(loss) - loss_ref) / abs(loss_ref)
    r_norm = abs(float(eng.last_grad_norm) - float(norm_ref)) / float(norm_ref)
    print(f"convnext_tiny fp32 step: pred rel {r_pred:.2e}  loss rel {r_loss:.2e}  grad-norm rel {r_norm:.2e}")
    assert r_pred < 1e-3 and r_loss < 1e-3 and r_norm < 1e-3
    # a stage-1 (C = 96) parameter took the AdamW update
    k = next(k for k in init if k.endswith("stages.0.blocks.0.conv_dw.weight"))
    assert not torch.equal(hip.state_dict()[k].cpu(), init[k]), k


def test_tiny_inference_checkpoint_round_trip(dev, tmp_path):
    from spine_vision_amd.inference import load_localization_model
    from spine_vision_amd.training import CoordinateRegressor

    m = CoordinateRegressor("convnext_tiny", pretrained=False, dropout=0.0, precision="fp32")
    ow.fill_module(m)
    path = tmp_path / "best_model.pt"
    torch.save({"model_state_dict": m.state_dict(), "epoch": 0}, path)
    model = load_localization_model(path, "tiny", "cuda", precision="fp32")
    assert not model.training
    for k, v in m.state_dict().items():
        assert torch.equal(model.state_dict()[k].cpu(), v), k
    img, _, _ = ow.localization_batch(2, 64, 64)
    with torch.no_grad():
        out = model(img.to(dev))
        want = m.to(dev).eval()(img.to(dev))
    assert tuple(out.shape) == (2, 5, 2) and torch.isfinite(out).all()
    assert torch.equal(out, want)
