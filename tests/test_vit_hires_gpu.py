"""ViT / DeiT-III above 256 tokens on the GPU (attention on csrc/attn_stream.hip) against the plain torch.nn reference
of tests/_vit_ref.py, with the bounds of tests/test_vit_gpu.py: fp32 parity mode features < 1e-4 and every gradient
against float64 within max(1e-3, 3 x the fp32 reference's own error); bf16 teacher-forced per block outputs < 2e-2,
every input / parameter gradient < 0.15 and the pad rows of each block's input gradient exactly zero.

Sizes: 272 x 272 (N = 290 tokens in Np = 296 rows: three 128-token workgroups, five 64-token tiles, the last one
partial) and 384 x 384 (N = 577 in 584 rows); B = 2.  The streaming pair forced at 224 (``attn_stream``, what
SV_ATTN=stream sets) meets the same bounds as the one-pass kernels."""
import copy
import functools

import pytest
import torch

import _vit_ref as ref
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import create_vit

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _reference(name, size, grads=False):
    """The filled reference module (untouched), its input and output gradient, and with ``grads`` one fp32 + one
    float64 forward / backward of it at 2 x size x size; computed once per case, shared, never modified."""
    r = ow.fill_module(ref.create(name, size)).train()
    img = ow.classification_batch(2, size, size)[0]
    out = dict(ref=r, state=copy.deepcopy(r.state_dict()), img=img,
               dfeat=torch.from_numpy(ow.uniform("dfeat", 2 * ref.FEATURE_DIMS[name], -1, 1).reshape(2, -1)))
    if grads:
        r32, r64 = copy.deepcopy(r), copy.deepcopy(r).double()
        f32, f64 = r32(img), r64(img.double())
        f32.backward(out["dfeat"])
        f64.backward(out["dfeat"].double())
        out.update(feat=f32.detach(), g32={n: p.grad for n, p in r32.named_parameters()},
                   g64={n: p.grad for n, p in r64.named_parameters()})
    return out


def _hip(name, size, precision, dev, state):
    hip = create_vit(name, precision=precision, img_size=size)
    hip.load_state_dict(state, strict=True)
    return hip.to(dev).train()


def _grads(hip, r, dev):
    for p in hip.parameters():
        p.grad = None
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f.detach(), {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


def test_vit_tiny_272_fp32_forward_backward(dev):
    r = _reference("vit_tiny", 272, True)
    hip = _hip("vit_tiny", 272, "fp32", dev, r["state"])
    assert (hip.num_tokens, hip.rows_per_img) == (290, 296)
    f_hip, g = _grads(hip, r, dev)
    e_f = rel(f_hip, r["feat"])
    worst = 0.0
    for n, g64 in r["g64"].items():
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        worst = max(worst, e_hip / max(1e-3, 3.0 * e_ref))
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    print(f"[vit hires] vit_tiny@272 fp32: features rel {e_f:.2e}, worst gradient error / bound {worst:.3f}")
    assert e_f < 1e-4


def _pad_rows(t, Np):
    """[B, N, C] -> the module's token matrix [B * Np, C] (pad rows zero)"""
    B, N, C = t.shape
    out = torch.zeros(B, Np, C, dtype=t.dtype)
    out[:, :N] = t
    return out.view(B * Np, C)


@pytest.mark.parametrize("name,size,stream", [("deit_small", 272, False), ("vit_tiny", 384, False),
                                              ("vit_tiny", 224, True)],
                         ids=["deit_small@272", "vit_tiny@384", "vit_tiny@224-stream"])
def test_vit_bf16_teacher_forced(dev, monkeypatch, name, size, stream):
    """bf16 mode, every block fed the SAME input as the fp32 reference block, then the SAME output gradient; the
    attention of every block must go through the streaming pair."""
    r = _reference(name, size)
    hip = _hip(name, size, "bf16", dev, r["state"])
    hip.attn_stream = hip.attn_stream or stream
    assert hip._use_stream()

    calls = {"fwd": 0, "bwd": 0}

    def counted(which, fn):
        def wrapper(*a, **k):
            calls[which] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(K, "attn_stream_fwd", counted("fwd", K.attn_stream_fwd))
    monkeypatch.setattr(K, "attn_stream_bwd", counted("bwd", K.attn_stream_bwd))
    N, Np, B = hip.num_tokens, hip.rows_per_img, 2
    with torch.no_grad():
        x = r["ref"].tokens(r["img"])
    worst_f = worst_b = 0.0
    for i, (rb, hb) in enumerate(zip(r["ref"].blocks, hip.blocks)):
        xr = x.clone().requires_grad_(True)
        rbc = copy.deepcopy(rb)
        o = rbc(xr)
        with torch.no_grad():
            xo, saved = hip._block_forward(hb, _pad_rows(x, Np).to(dev), B, {}, save=True)
        e = rel(xo.view(B, Np, -1)[:, :N], o)
        worst_f = max(worst_f, e)
        assert e < 2e-2, (i, e)
        d = torch.randn(o.shape, generator=torch.Generator().manual_seed(i))
        o.backward(d)
        for p in hb.parameters():
            p.grad = torch.zeros_like(p)
        with torch.no_grad():
            wg = hip._wgrads()
            dx = hip._block_backward(hb, saved, _pad_rows(d, Np).to(dev), B, wg, {}, ready=False)
            wg.join()
        torch.cuda.synchronize()
        dx = dx.view(B, Np, -1)
        assert bool((dx[:, N:] == 0).all()), f"block {i}: pad rows of the input gradient are not zero"
        hp = dict(hb.named_parameters())
        errs = {"dx": rel(dx[:, :N], xr.grad)}
        errs.update({n: rel(hp[n].grad, p.grad) for n, p in rbc.named_parameters()})
        for n, e in errs.items():
            worst_b = max(worst_b, e)
            assert e < 0.15, (i, n, e)
        x = o.detach()
    assert calls == {"fwd": hip.depth, "bwd": hip.depth}, calls
    print(f"[vit hires] {name}@{size} B2 bf16{' (stream forced)' if stream else ''}: worst block output rel "
          f"{worst_f:.2e}, worst block-backward rel {worst_b:.2e}")


def test_streams_ready_hook_and_eval_at_272(dev):
    """deit_small@272: the weight gradients on the side stream against every kernel on one stream (SV_SIDE_STREAM=0),
    bit for bit; every parameter is reported through grad_ready_hook; the eval forward is the training forward."""
    r = _reference("deit_small", 272)
    hip = _hip("deit_small", 272, "bf16", dev, r["state"])
    assert hip.overlap_wgrad and not hip.graph_safe
    seen: list = []
    hip.grad_ready_hook = seen.extend
    f_a, g_a = _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert sorted(names[id(p)] for p in seen) == sorted(names.values())
    hip.grad_ready_hook = None
    hip.overlap_wgrad = False
    f_b, g_b = _grads(hip, r, dev)
    assert torch.equal(f_a, f_b)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), f"{n}: side stream and single stream differ"
    with torch.no_grad():
        assert torch.equal(hip.eval()(r["img"].to(dev)), f_a)
    with pytest.raises(ValueError, match="LocalizationConfig.image_size"):
        hip(torch.zeros(1, 3, 224, 224, device=dev))


def test_step_engine_localization_at_272(dev):
    """CoordinateRegressor("vit_small", img_size=272) with the device-transform uint8 input through StepEngine: the
    loss decreases over three steps on a fixed batch."""
    from spine_vision_amd.training import CoordinateRegressor, StepEngine

    torch.manual_seed(0)
    m = CoordinateRegressor("vit_small", pretrained=False, dropout=0.0, img_size=272).to(dev).train()
    u8 = torch.from_numpy(ow.uint8_images("loc.image", 2, 272, 272)).to(dev)
    _, coords, mask = ow.localization_batch(2, 272, 272)
    eng = StepEngine(m, dev, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    losses = [float(eng.step_localization(u8, coords.to(dev), mask.to(dev))) for _ in range(3)]
    print(f"[vit hires] CoordinateRegressor(vit_small@272) losses {losses}")
    assert all(torch.isfinite(torch.tensor(losses))) and losses[2] < losses[0]


def test_localization_trainer_builds_the_configured_size(dev, tmp_path):
    from spine_vision_amd.training import LocalizationConfig, LocalizationTrainer
    from spine_vision_amd.training.datasets import SyntheticLocalizationDataset

    cfg = LocalizationConfig(output_path=tmp_path, backbone="vit_tiny", batch_size=2, num_epochs=1, num_workers=0,
                             image_size=(272, 272), pretrained=False)
    tr = LocalizationTrainer(cfg, train_dataset=SyntheticLocalizationDataset(2, (272, 272), seed=1),
                             val_dataset=SyntheticLocalizationDataset(2, (272, 272), seed=2))
    assert tr.model.backbone.img_size == 272 and tr.model.backbone.num_tokens == 290
