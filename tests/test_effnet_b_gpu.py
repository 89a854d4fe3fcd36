"""EfficientNet-B0 .. B4 (MBConv on csrc/mbconv.hip, 5x5 depthwise on csrc/dwconv5.hip, 1x1 convolutions on sv_gemm,
zero-padded channel strides for the widths the kernels refuse) on the GPU against the plain torch.nn restatement of
tests/_effnet_ref.py, with the bounds of tests/test_effnetv2_gpu.py.  All weights are filled; the models are shallow
stage tables (one block per stage unless a case says otherwise) unless a test names the full model.  At 64 x 64 the last
5x5 stages run on 4 x 4 and 2 x 2 grids; 72 x 56 puts odd grids (9 x 7, 5 x 4, 3 x 2) in front of the stride-2 ones."""
import copy
import functools

import pytest
import torch

import _effnet_ref as eref
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import EfficientNetHip, create_efficientnet

pytestmark = pytest.mark.gpu
ONE = (1, 1, 1, 1, 1, 1, 1)
SKIP5 = (1, 2, 2, 1, 2, 1, 1)   # identity skips around 5x5 blocks (stages 2 and 4)
DS2 = (2, 1, 1, 1, 1, 1, 1)     # B1's second ds block: the ds skip
NAMES = tuple(f"efficientnet_b{i}" for i in range(5))


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _reference(H, W, repeats=ONE, name="efficientnet_b0"):
    """The filled shallow reference (train mode, untouched) and one fp32 + one float64 forward / backward of it at
    2 x H x W.  Computed once per (size, depth, widths), shared, never modified."""
    stages = eref.shallow(name, repeats)
    ref = ow.fill_module(eref.create(name, stages)).train()
    state = copy.deepcopy(ref.state_dict())
    img, _ = ow.classification_batch(2, H, W)
    r32, r64 = copy.deepcopy(ref), copy.deepcopy(ref).double()
    f32, f64 = r32(img), r64(img.double())
    dfeat = torch.from_numpy(ow.uniform("dfeat", f32.numel(), -1, 1).reshape(f32.shape))
    f32.backward(dfeat)
    f64.backward(dfeat.double())
    stem, _, nf, _ = eref.CFGS[name]
    return dict(ref=ref, state=state, stages=stages, stem=stem, nf=nf, img=img, dfeat=dfeat, feat=f32.detach(),
                g32={n: p.grad for n, p in r32.named_parameters()}, g64={n: p.grad for n, p in r64.named_parameters()},
                buffers=dict(r32.named_buffers()))


def _hip(precision, dev, r, train=True):
    hip = EfficientNetHip(r["stem"], r["stages"], r["nf"], precision=precision)
    missing, unexpected = hip.load_state_dict(r["state"], strict=True)
    assert not missing and not unexpected
    return hip.to(dev).train(train)


def _grads(hip, r, dev):
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f, {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


@pytest.mark.parametrize("H,W,repeats,name", [(64, 64, ONE, "efficientnet_b0"), (72, 56, ONE, "efficientnet_b0"),
                                              (64, 64, SKIP5, "efficientnet_b0"), (64, 64, DS2, "efficientnet_b1"),
                                              (64, 64, ONE, "efficientnet_b2"), (64, 64, ONE, "efficientnet_b3")])
def test_fp32_forward_backward(dev, H, W, repeats, name):
    """fp32 parity mode: features < 1e-4, each gradient against the float64 reference within max(1e-3, 3 x the fp32
    reference's own error), buffers 1e-5.  B2: widths 88 / 120 / 208 and SE widths 22 / 30 / 52; B3: the 40-wide stem
    stored as 64 and an SE width of 10."""
    r = _reference(H, W, repeats, name)
    hip = _hip("fp32", dev, r)
    f_hip, g = _grads(hip, r, dev)
    e_f = rel(f_hip, r["feat"])
    print(f"[parity] {name}{list(repeats)}@{H}x{W} fp32: features rel {e_f:.2e}")
    assert e_f < 1e-4
    worst = 0.0
    for n, g64 in r["g64"].items():
        assert g[n].shape == g64.shape, n
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        worst = max(worst, e_hip / max(1e-3, 3.0 * e_ref))
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    print(f"[parity] {name}{list(repeats)}@{H}x{W} fp32: worst gradient error / bound {worst:.3f}")
    hb = dict(hip.named_buffers())
    for n, b in r["buffers"].items():
        if b.is_floating_point():
            assert rel(hb[n], b) < 1e-5, n
        else:
            assert int(hb[n]) == int(b), n


@pytest.mark.parametrize("H,W,repeats,name", [(64, 64, SKIP5, "efficientnet_b0"), (72, 56, DS2, "efficientnet_b1"),
                                              (64, 64, ONE, "efficientnet_b3")])
def test_bf16_teacher_forced(dev, H, W, repeats, name):
    """bf16 mode, every block fed the SAME (bf16) input as the fp32 reference block: outputs < 2e-2, and with the SAME
    output gradient every input / parameter gradient < 0.15; the padded channels of x_in, out and dx are exactly zero."""
    r = _reference(H, W, repeats, name)
    hip = _hip("bf16", dev, r)
    with torch.no_grad():
        _, tape = hip._forward_impl(r["img"].to(dev), save=True)
    rblocks = r["ref"].block_list()
    assert len(rblocks) == len(tape.blocks) == sum(repeats)
    worst_f = worst_b = 0.0
    padded = 0
    for i, (rb, hb, sb) in enumerate(zip(rblocks, hip.block_list(), tape.blocks)):
        x_in, _, out = sb
        cin = hb.conv_dw.in_channels if hb.kind == "ds" else hb.conv_pw.in_channels
        cout = (hb.conv_pw if hb.kind == "ds" else hb.conv_pwl).out_channels
        assert x_in.shape[-1] % 32 == 0 and out.shape[-1] % 32 == 0 and out.shape[-1] == hip._out_cs(hb)
        padded += int(x_in.shape[-1] > cin) + int(out.shape[-1] > cout)
        assert not x_in[..., cin:].any() and not out[..., cout:].any(), (i, "padded channels must be exactly zero")
        xr = x_in[..., :cin].float().permute(0, 3, 1, 2).cpu().clone().requires_grad_(True)
        rbc = copy.deepcopy(rb)
        o = rbc(xr)
        e = rel(out[..., :cout].permute(0, 3, 1, 2), o)
        worst_f = max(worst_f, e)
        assert e < 2e-2, (i, hb.kind, e)
        d = torch.randn(o.shape, generator=torch.Generator().manual_seed(i)).to(hip.grad_dtype).float()
        o.backward(d)
        for p in hb.parameters():
            p.grad = torch.zeros_like(p)
        dp = torch.zeros(out.shape, device=dev, dtype=hip.grad_dtype)
        dp[..., :cout] = d.permute(0, 2, 3, 1).to(dev, hip.grad_dtype)
        dx = hip._block_backward(hb, sb, dp, batch_stats=True)
        torch.cuda.synchronize()
        assert not dx[..., cin:].any(), (i, "the padded channels of dx must be exactly zero")
        hp = dict(hb.named_parameters())
        errs = {"dx": rel(dx[..., :cin].permute(0, 3, 1, 2), xr.grad)}
        errs.update({n: rel(hp[n].grad, p.grad) for n, p in rbc.named_parameters()})
        for n, e in errs.items():
            worst_b = max(worst_b, e)
            assert e < 0.15, (i, hb.kind, n, e)
    assert padded > 0
    print(f"[parity] {name}{list(repeats)}@{H}x{W} B2 bf16: worst block output rel {worst_f:.2e}, "
          f"worst block-backward rel {worst_b:.2e}")


def test_fp32_eval_forward_full_depth(dev):
    """the full-depth efficientnet_b0 in eval mode (running statistics, tape-free forward): < 1e-4"""
    ref = ow.fill_module(eref.create("efficientnet_b0")).eval()
    hip = create_efficientnet("efficientnet_b0", precision="fp32")
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    img, _ = ow.classification_batch(2, 64, 64)
    with torch.no_grad():
        e = rel(hip(img.to(dev)), ref(img))
    print(f"[parity] efficientnet_b0@64 fp32 eval: features rel {e:.2e}")
    assert e < 1e-4


def test_full_depth_b4_train_step_is_finite(dev):
    hip = create_efficientnet("efficientnet_b4", precision="bf16").to(dev).train()
    assert len(hip.block_list()) == 32
    img, _ = ow.classification_batch(2, 64, 64)
    f = hip(img.to(dev))
    assert tuple(f.shape) == (2, 1792)
    f.backward(torch.ones_like(f))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f).all())
    for n, p in hip.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
        assert bool(p.grad.any()), n


def test_uint8_hwc_input_matches_normalised_float(dev):
    r = _reference(64, 64)
    hip = _hip("bf16", dev, r, train=False)
    u8 = torch.from_numpy(ow.uint8_images("u8", 2, 64, 64)).reshape(2, 64, 64, 1).expand(2, 64, 64, 3).contiguous()
    mean, std = torch.tensor(K.IMAGENET_MEAN), torch.tensor(K.IMAGENET_STD)
    img = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        a, b = hip(u8.to(dev)), hip(img.to(dev))
    assert rel(a, b) < 1e-2 and bool(torch.isfinite(a).all())


def test_side_stream_matches_single_stream(dev):
    r = _reference(64, 64, SKIP5)
    out = []
    for overlap in (True, False):
        hip = _hip("bf16", dev, r)
        hip.overlap_wgrad = overlap
        _, g = _grads(hip, r, dev)
        out.append(list(g.values()) + [b.detach().cpu().clone() for b in hip.buffers()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_repeated_steps_are_bit_equal(dev):
    """no atomics, no order that depends on scheduling: the same step twice gives the same bits"""
    r = _reference(72, 56, ONE)
    runs = [_grads(_hip("bf16", dev, r), r, dev) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_reports_every_parameter_ready_once(dev):
    r = _reference(64, 64, DS2, "efficientnet_b1")
    hip = _hip("bf16", dev, r)
    seen: list = []
    hip.grad_ready_hook = seen.extend
    _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert all(id(p) in names for p in seen)
    assert sorted(names[id(p)] for p in seen) == sorted(n for n, p in hip.named_parameters() if p.requires_grad)


def test_hip_arm_no_less_accurate_than_torch_arm(dev, monkeypatch):
    """SV_MBCONV=torch computes the csrc/mbconv.hip and csrc/dwconv5.hip wrappers as torch ops with the same f32
    arithmetic and rounding points: per parameter the HIP arm's error against the fp32 reference is at most 2 x the torch
    arm's (the bound of tests/test_effnetv2_gpu.py)."""
    r = _reference(64, 64, SKIP5)
    assert not K.MBCONV_TORCH
    _, g_def = _grads(_hip("bf16", dev, r), r, dev)
    monkeypatch.setattr(K, "MBCONV_TORCH", True)
    _, g_t = _grads(_hip("bf16", dev, r), r, dev)
    worst = 0.0
    for n, g32 in r["g32"].items():
        e_def = float((g_def[n].double() - g32.double()).norm())
        e_t = float((g_t[n].double() - g32.double()).norm())
        worst = max(worst, e_def / (e_t + 1e-30))
        assert e_def <= 2.0 * e_t, (n, e_def, e_t)
    print(f"[mbconv arms] efficientnet_b0{list(SKIP5)} bf16: worst (default - fp32) / (torch - fp32) = {worst:.3f}")


def _lift_gate(monkeypatch):
    import spine_vision_amd.training.models.backbone as bb

    monkeypatch.setattr(bb, "NATIVE", bb.NATIVE + NAMES)


def test_classification_trainer_steps_and_checkpoint(dev, tmp_path, monkeypatch):
    """Classifier(backbone="efficientnet_b0"), the factory gate lifted for this test, through ClassificationTrainer (flat
    AdamW, bf16 shadows) for two steps: every parameter is finite and has moved; the checkpoint has timm's keys (it loads
    strictly into the restatement) and loads back."""
    from spine_vision_amd.training import ClassificationConfig, ClassificationTrainer
    from spine_vision_amd.training.datasets import SyntheticClassificationDataset

    _lift_gate(monkeypatch)
    cfg = ClassificationConfig(output_path=tmp_path, batch_size=4, num_epochs=1, num_workers=0, output_size=(64, 64),
                               backbone="efficientnet_b0", pretrained=False, precision="bf16", save_frequency=1,
                               early_stopping=False)
    tr = ClassificationTrainer(cfg, train_dataset=SyntheticClassificationDataset(8, (64, 64), seed=1),
                               val_dataset=SyntheticClassificationDataset(4, (64, 64), seed=2))
    bb = tr.model.backbone
    assert isinstance(bb, EfficientNetHip) and len(bb.block_list()) == 16
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    labelled = set(SyntheticClassificationDataset(1).target_labels)
    res = tr.train()
    assert res.final_train_loss == res.final_train_loss and res.final_train_loss > 0
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if n.startswith("backbone.") or n.split(".")[1] in labelled:
            assert not torch.equal(before[n], p.detach()), n
    ck = torch.load(tmp_path / "checkpoint_epoch_1.pt", weights_only=False)
    sd = {k[len("backbone."):]: v for k, v in ck["model_state_dict"].items() if k.startswith("backbone.")}
    back = eref.create("efficientnet_b0")
    missing, unexpected = back.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert len(ck["optimizer_state_dict"]["state"]) == len(list(tr.model.parameters()))
    with torch.no_grad():
        bb.blocks[2][0].se.conv_reduce.weight.zero_()
    tr._load_checkpoint(tmp_path / "checkpoint_epoch_1.pt")
    assert torch.equal(bb.blocks[2][0].se.conv_reduce.weight.detach().cpu(), sd["blocks.2.0.se.conv_reduce.weight"].cpu())


def test_localization_trainer_step(dev, tmp_path, monkeypatch):
    from spine_vision_amd.training import LocalizationConfig, LocalizationTrainer
    from spine_vision_amd.training.datasets import SyntheticLocalizationDataset

    _lift_gate(monkeypatch)
    cfg = LocalizationConfig(output_path=tmp_path, backbone="efficientnet_b0", batch_size=4, num_epochs=1, num_workers=0,
                             image_size=(64, 64), pretrained=False, precision="bf16", save_frequency=1, early_stopping=False)
    tr = LocalizationTrainer(cfg, train_dataset=SyntheticLocalizationDataset(8, (64, 64), seed=1),
                             val_dataset=SyntheticLocalizationDataset(4, (64, 64), seed=2))
    bb = tr.model.backbone
    assert isinstance(bb, EfficientNetHip)
    before = bb.conv_stem.weight.detach().clone()
    res = tr.train()
    assert res.final_train_loss == res.final_train_loss and res.final_train_loss > 0
    assert not torch.equal(before, bb.conv_stem.weight.detach())
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
