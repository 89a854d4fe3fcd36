"""GPU: the ConvNeXt V2 backbones (GRN blocks, no layer scale) through the HIP path against the timm-keyed fp32
torch restatement tests/_convnextv2_ref.py on identical generated weights (oracle.weights.fill_module: grn.weight in
U(0.8, 1.2), grn.bias in U(-0.1, 0.1), so GRN is far from the identity).  Everything at 2 x 64 x 64.

fp32 bounds are the V1 ones of tests/test_backbone_gpu.py (features 1e-4, every gradient 1e-3, relative L2 per
tensor).  bf16 misses 1e-3 by construction; it is held against the reference recipe's own rounding, the reference
module under torch.autocast(bf16) on the CPU, whose distance to its fp32 result is computed in the same test: the
HIP distance may be at most 1.5 x it (features; median and worst per-tensor gradient).  The HIP path rounds a, u, du
and dh to bf16 where autocast keeps some of them wider, and at B = 2 the per-tensor worst is noisy
(tests/test_bs32_parity_gpu.py holds 1.10 at B = 32)."""

import functools

import numpy as np
import pytest
import torch

import _convnextv2_ref as v2ref
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


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The reference module, its fp32 features and gradients on the shared batch (computed once per backbone)."""
    ref = ow.fill_module(v2ref.create(name))
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


@pytest.mark.parametrize("name", ["convnextv2_base", "convnextv2_large"])
def test_v2_fp32_forward_backward(dev, name):
    ref, img, f_ref, g_ref = _reference(name)
    f_hip, g_hip = _hip_grads(_hip(name, "fp32", dev), img, dev)
    assert rel(f_hip, f_ref) < 1e-4
    assert list(g_hip) == list(g_ref)
    assert sum(n.endswith("mlp.grn.weight") for n in g_ref) == sum(n.endswith("mlp.grn.bias") for n in g_ref) == 36
    errs = {n: rel(g_hip[n], g) for n, g in g_ref.items()}
    grn = {n: e for n, e in errs.items() if ".grn." in n}
    print(f"{name}@64 fp32: features {rel(f_hip, f_ref):.2e}, worst grad {max(errs.values()):.2e} "
          f"({max(errs, key=errs.get)}), worst grn grad {max(grn.values()):.2e} ({max(grn, key=grn.get)})")
    bad = {n: e for n, e in errs.items() if not e < 1e-3}
    assert not bad, bad


def test_v2_bf16_no_farther_than_autocast(dev):
    name = "convnextv2_base"
    ref, img, f_ref, g_ref = _reference(name)
    # the reference's own mixed-precision recipe at bf16 width, on the CPU
    with torch.autocast("cpu", dtype=torch.bfloat16):
        f_auto = ref(img)
    f_auto.float().backward(_dfeat(f_auto))
    g_auto = {n: p.grad.detach().float().clone() for n, p in ref.named_parameters()}
    ref.zero_grad(set_to_none=True)
    f_hip, g_hip = _hip_grads(_hip(name, "bf16", dev), img, dev)
    fa, fh = rel(f_auto.float(), f_ref), rel(f_hip, f_ref)
    ea = {n: rel(g_auto[n], g) for n, g in g_ref.items()}
    eh = {n: rel(g_hip[n], g) for n, g in g_ref.items()}
    ma, mh = float(np.median(list(ea.values()))), float(np.median(list(eh.values())))
    wa, wh = max(ea, key=ea.get), max(eh, key=eh.get)
    print(f"[parity] {name}@64 B2 bf16 vs fp32 -- autocast: features {fa:.3e} grad median {ma:.3e} worst {ea[wa]:.3e} "
          f"({wa}); HIP: features {fh:.3e} grad median {mh:.3e} worst {eh[wh]:.3e} ({wh}); ratios features "
          f"{fh / fa:.2f} median {mh / ma:.2f} worst {eh[wh] / ea[wa]:.2f}")
    assert fh <= 1.5 * fa, (fh, fa)
    assert mh <= 1.5 * ma, (mh, ma)
    assert eh[wh] <= 1.5 * ea[wa], (wh, eh[wh], wa, ea[wa])


def test_v2_bf16_schedules_bitwise_equal(dev):
    """The lean side-stream backward, the inline one (weight gradients on the main stream: SV_SIDE_STREAM=0, set
    through the model attribute) and the eager side-stream one (SV_LEAN_SYNC=0) run the same kernels: every gradient
    equal bit for bit."""
    _, img, _, _ = _reference("convnextv2_base")
    out = []
    for overlap, lean in ((True, True), (False, True), (True, False)):
        hip = _hip("convnextv2_base", "bf16", dev)
        assert hip.lean_sync
        hip.overlap_wgrad, hip.lean_sync = overlap, lean
        out.append(_hip_grads(hip, img, dev))
    for f, grads in out[1:]:
        assert torch.equal(out[0][0], f)
        for n in out[0][1]:
            assert torch.equal(out[0][1][n], grads[n]), n


@pytest.mark.parametrize("precision,overlap", [("bf16", True), ("bf16", False), ("fp32", True)])
def test_v2_reports_every_parameter_ready(dev, precision, overlap):
    """grad_ready_hook sees every trainable parameter exactly once (a missing report leaves a DDP bucket open)."""
    _, img, _, _ = _reference("convnextv2_base")
    hip = _hip("convnextv2_base", precision, dev)
    hip.overlap_wgrad = overlap
    seen: list = []
    hip.grad_ready_hook = seen.extend
    _hip_grads(hip, img, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert all(id(p) in names for p in seen)
    reported = sorted(names[id(p)] for p in seen)
    assert reported == sorted(n for n, p in hip.named_parameters() if p.requires_grad)
    assert any(n.endswith("mlp.grn.weight") for n in reported) and any(n.endswith("mlp.grn.bias") for n in reported)


def test_v2_eval_forward_equals_training_forward(dev):
    """The tape-free forward (GRN applied in place, no GELU' store) gives the training forward's features bit for bit."""
    _, img, f_ref, _ = _reference("convnextv2_base")
    hip = _hip("convnextv2_base", "fp32", dev)
    f_train = hip(img.to(dev)).detach()
    with torch.no_grad():
        f_eval = hip.eval()(img.to(dev))
    assert torch.equal(f_train, f_eval)
    assert rel(f_eval, f_ref) < 1e-4
    assert "ls_ones" not in hip.state_dict() and hip.ls_ones.is_cuda


def test_v2_train_step_matches_torch(dev):
    """One fp32 StepEngine.step_localization on CoordinateRegressor(convnextv2_base) against the torch reference
    step (the reference module under oracle.heads / oracle.step, as __graft_entry__.smoke does for V1)."""
    from spine_vision_amd.training import CoordinateRegressor, StepEngine

    ref = oh.CoordinateRegressor(v2ref.create("convnextv2_base"), 1024, dropout=0.0)
    ow.fill_module(ref)
    hip = CoordinateRegressor("convnextv2_base", pretrained=False, dropout=0.0, precision="fp32")
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
    print(f"convnextv2_base fp32 step: pred rel {r_pred:.2e}  loss rel {r_loss:.2e}  grad-norm rel {r_norm:.2e}")
    assert r_pred < 1e-3 and r_loss < 1e-3 and r_norm < 1e-3
    # the GRN parameters took the AdamW update
    for leaf in ("mlp.grn.weight", "mlp.grn.bias"):
        k = next(k for k in init if k.endswith("stages.0.blocks.0." + leaf))
        assert not torch.equal(hip.state_dict()[k].cpu(), init[k]), k


def test_v2_inference_checkpoint_round_trip(dev, tmp_path):
    from spine_vision_amd.inference import load_localization_model
    from spine_vision_amd.training import CoordinateRegressor

    m = CoordinateRegressor("convnextv2_base", pretrained=False, dropout=0.0, precision="fp32")
    ow.fill_module(m)
    path = tmp_path / "best_model.pt"
    torch.save({"model_state_dict": m.state_dict(), "epoch": 0}, path)
    assert not [k for k in m.state_dict() if "ls_ones" in k or k.endswith(".gamma")]
    model = load_localization_model(path, "v2_base", "cuda", precision="fp32")
    assert not model.training and model.backbone.use_grn
    for k, v in m.state_dict().items():
        assert torch.equal(model.state_dict()[k].cpu(), v), k
    img, _, _ = ow.localization_batch(2, 64, 64)
    with torch.no_grad():
        out = model(img.to(dev))
        want = m.to(dev).eval()(img.to(dev))
    assert tuple(out.shape) == (2, 5, 2) and torch.isfinite(out).all()
    assert torch.equal(out, want)
