"""ResNet-RS (deep stem, conv stem pool, avg-pool shortcut, squeeze-and-excitation on csrc/se.hip) and ResNet-50-D on
the GPU against the plain torch.nn restatement of tests/_resnetrs_ref.py, with the bounds tests/test_resnet_gpu.py and
tests/test_resnet_family_gpu.py use for ResNet-50 / wide_resnet50.  All weights are filled (so bn3.weight != 0); layers
are (1, 1, 1, 1) -- every block the first of its layer, with a BN'd shortcut -- or (2, 1, 1, 1), whose second block is a
squeeze-and-excitation block with an identity shortcut, unless a test names the full model."""
import copy
import functools

import pytest
import torch

import _resnetrs_ref as rsref
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import create_resnet
from spine_vision_amd.backbone.resnet import RESNET_CFGS, ResNetHip

pytestmark = pytest.mark.gpu
SHALLOW = (1, 1, 1, 1)
IDENT = (2, 1, 1, 1)  # layer1.1: an identity-shortcut block (its dx is the masked gradient with conv1's data gradient added)


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, layers=SHALLOW):
    """The filled shallow reference (train mode, untouched) and one fp32 + one float64 forward / backward of it at
    2 x H x W.  Computed once per (name, size, depth), shared, never modified."""
    ref = ow.fill_module(rsref.create(name, layers)).train()
    state = copy.deepcopy(ref.state_dict())
    img, _ = ow.classification_batch(2, H, W)
    r32, r64 = copy.deepcopy(ref), copy.deepcopy(ref).double()
    f32, f64 = r32(img), r64(img.double())
    dfeat = torch.from_numpy(ow.uniform("dfeat", f32.numel(), -1, 1).reshape(f32.shape))
    f32.backward(dfeat)
    f64.backward(dfeat.double())
    return dict(ref=ref, state=state, layers=layers, img=img, dfeat=dfeat, feat=f32.detach(),
                g32={n: p.grad for n, p in r32.named_parameters()}, g64={n: p.grad for n, p in r64.named_parameters()},
                buffers=dict(r32.named_buffers()))


def _hip(name, precision, dev, r, train=True):
    hip = ResNetHip("bottleneck", r["layers"], precision=precision, **RESNET_CFGS[name][4])
    missing, unexpected = hip.load_state_dict(r["state"], strict=True)
    assert not missing and not unexpected
    return hip.to(dev).train(train)


def _grads(hip, r, dev):
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f, {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


@pytest.mark.parametrize("name,H,W,layers", [("resnetrs50", 64, 64, SHALLOW), ("resnetrs50", 72, 56, SHALLOW),
                                             ("resnet50_d", 64, 64, SHALLOW), ("resnetrs50", 64, 64, IDENT),
                                             ("resnet50_d", 64, 64, IDENT)])
def test_fp32_forward_backward(dev, name, H, W, layers):
    """fp32 parity mode: features < 1e-4, each gradient against the float64 reference within max(1e-3, 3 x the fp32
    reference's own error), buffers 1e-5 -- the bounds of test_resnet_fp32_forward_backward, the SE weights included.
    72 x 56 puts 9 x 7 and 5 x 4 grids in front of the ceil-mode pool (9 -> 5, 7 -> 4, 5 -> 3); layers (2, 1, 1, 1) adds
    an identity-shortcut block."""
    r = _reference(name, H, W, layers)
    hip = _hip(name, "fp32", dev, r)
    f_hip, g = _grads(hip, r, dev)
    e_f = rel(f_hip, r["feat"])
    print(f"[parity] {name}{list(layers)}@{H}x{W} fp32: features rel {e_f:.2e}")
    assert e_f < 1e-4
    worst = 0.0
    for n, g64 in r["g64"].items():
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        worst = max(worst, e_hip / max(1e-3, 3.0 * e_ref))
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    print(f"[parity] {name}{list(layers)}@{H}x{W} fp32: worst gradient error / bound {worst:.3f}")
    hb = dict(hip.named_buffers())
    for n, b in r["buffers"].items():
        if b.is_floating_point():
            assert rel(hb[n], b) < 1e-5, n
        else:
            assert int(hb[n]) == int(b), n


@pytest.mark.parametrize("name,layers", [("resnetrs50", SHALLOW), ("resnet50_d", SHALLOW), ("resnetrs50", IDENT)])
def test_bf16_teacher_forced(dev, name, layers):
    """bf16 mode, every block fed the SAME (bf16) input as the fp32 reference block: outputs < 2e-2, and with the SAME
    output gradient every input / parameter gradient < 0.15 (the bounds test_resnet_family_gpu.py uses for
    wide_resnet50).  With layers (2, 1, 1, 1) the second block is an SE block with an identity shortcut."""
    r = _reference(name, 64, 64, layers)
    hip = _hip(name, "bf16", dev, r)
    assert len(list(hip.blocks())) == sum(layers) and (layers == SHALLOW or hip.layer1[1].downsample is None)
    with torch.no_grad():
        _, tape = hip._forward_impl(r["img"].to(dev), save=True)
    rblocks = [b for b in r["ref"].modules() if isinstance(b, rsref.Bottleneck)]
    worst_f = worst_b = 0.0
    for i, (rb, hb, sb) in enumerate(zip(rblocks, hip.blocks(), tape.blocks)):
        xr = sb[0].float().permute(0, 3, 1, 2).cpu().clone().requires_grad_(True)
        rbc = copy.deepcopy(rb)
        o = rbc(xr)
        e = rel(sb[3].permute(0, 3, 1, 2), o)
        worst_f = max(worst_f, e)
        assert e < 2e-2, (i, e)
        d = torch.randn(o.shape, generator=torch.Generator().manual_seed(i)).to(hip.grad_dtype).float()
        o.backward(d)
        for p in hb.parameters():
            p.grad = torch.zeros_like(p)
        dx = hip._block_backward(hb, sb, d.permute(0, 2, 3, 1).contiguous().to(dev, hip.grad_dtype))
        hp = dict(hb.named_parameters())
        errs = {"dx": rel(dx.permute(0, 3, 1, 2), xr.grad)}
        errs.update({n: rel(hp[n].grad, p.grad) for n, p in rbc.named_parameters()})
        for n, e in errs.items():
            worst_b = max(worst_b, e)
            assert e < 0.15, (i, n, e)
    print(f"[parity] {name}{list(layers)}@64 B2 bf16: worst block output rel {worst_f:.2e}, worst block-backward rel {worst_b:.2e}")


def test_resnetrs101_fp32_eval_forward(dev):
    """the full-depth model in eval mode (running statistics, tape-free forward): < 1e-4, the bound resnet101 has"""
    ref = ow.fill_module(rsref.create("resnetrs101")).eval()
    hip = create_resnet("resnetrs101", precision="fp32")
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    img, _ = ow.classification_batch(2, 64, 64)
    with torch.no_grad():
        e = rel(hip(img.to(dev)), ref(img))
    print(f"[parity] resnetrs101@64 fp32 eval: features rel {e:.2e}")
    assert e < 1e-4


def test_side_stream_matches_single_stream(dev):
    r = _reference("resnetrs50", 64, 64)
    out = []
    for overlap in (True, False):
        hip = _hip("resnetrs50", "bf16", dev, r)
        hip.overlap_wgrad = overlap
        _, g = _grads(hip, r, dev)
        out.append(list(g.values()) + [b.detach().cpu().clone() for b in hip.buffers()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_graph_forward_matches_eager(dev):
    """The training forward replayed from its captured graph equals the eager forward bit for bit (features, gradients,
    running statistics) over several inputs: the SE and avg-pool kernels do no host synchronisation."""
    r = _reference("resnetrs50", 64, 64)
    a, b = _hip("resnetrs50", "bf16", dev, r), _hip("resnetrs50", "bf16", dev, r)
    assert a.graph_safe
    a.graph_forward, b.graph_forward = True, False
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = torch.rand(2, 3, 64, 64, generator=gen).to(dev)
        outs = []
        for m in (a, b):
            m.zero_grad(set_to_none=True)
            f = m(x)
            f.backward(torch.ones_like(f))
            torch.cuda.synchronize()
            outs.append(f)
        assert torch.equal(outs[0], outs[1])
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa.grad, pb.grad)
    assert len(a._fgraphs) == 1
    for ba, bb in zip(a.buffers(), b.buffers()):
        assert torch.equal(ba, bb)


def test_reports_every_parameter_ready(dev):
    r = _reference("resnetrs50", 64, 64)
    hip = _hip("resnetrs50", "bf16", dev, r)
    seen: list = []
    hip.grad_ready_hook = seen.extend
    _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert all(id(p) in names for p in seen)
    assert sorted(names[id(p)] for p in seen) == sorted(n for n, p in hip.named_parameters() if p.requires_grad)


def test_torch_arm_within_precision_noise(dev, monkeypatch):
    """SV_SE=torch (squeeze / excite / scale and the pooled shortcut as torch ops) against the default (csrc/se.hip):
    per parameter the two arms' gradients are no further apart than the default arm is from the fp32 reference."""
    r = _reference("resnetrs50", 64, 64)
    assert not K.SE_TORCH
    _, g_def = _grads(_hip("resnetrs50", "bf16", dev, r), r, dev)
    monkeypatch.setattr(K, "SE_TORCH", True)
    _, g_t = _grads(_hip("resnetrs50", "bf16", dev, r), r, dev)
    worst = 0.0
    for n, g32 in r["g32"].items():
        arms = float((g_t[n].double() - g_def[n].double()).norm())
        noise = float((g_def[n].double() - g32.double()).norm())
        worst = max(worst, arms / (noise + 1e-30))
        assert arms <= noise, (n, arms, noise)
    print(f"[se arms] resnetrs50 bf16: worst (torch - default) / (default - fp32) = {worst:.3f}")


def test_resnetrs101_trainer_steps_and_checkpoint(dev, tmp_path):
    """Classifier(backbone="resnetrs101") through ClassificationTrainer (flat AdamW) for two steps: every parameter is
    finite and has moved, the SE weights included; the checkpoint it writes is in the reference format (timm keys: it
    loads strictly into the restatement) and loads back."""
    from spine_vision_amd.training import ClassificationConfig, ClassificationTrainer
    from spine_vision_amd.training.datasets import SyntheticClassificationDataset

    cfg = ClassificationConfig(output_path=tmp_path, batch_size=4, num_epochs=1, num_workers=0, output_size=(64, 64),
                               backbone="resnetrs101", pretrained=False, precision="bf16", save_frequency=1,
                               early_stopping=False)
    tr = ClassificationTrainer(cfg, train_dataset=SyntheticClassificationDataset(8, (64, 64), seed=1),
                               val_dataset=SyntheticClassificationDataset(4, (64, 64), seed=2))
    bb = tr.model.backbone
    assert hasattr(bb.layer3[22], "se") and len(bb.layer3) == 23
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    labelled = set(SyntheticClassificationDataset(1).target_labels)
    assert labelled == {"pfirrmann", "modic", "herniation"}
    res = tr.train()
    assert res.final_train_loss == res.final_train_loss and res.final_train_loss > 0
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        # a head gets a gradient only where the dataset labels its task: exactly those heads may stand still
        if n.startswith("backbone.") or n.split(".")[1] in labelled:
            assert not torch.equal(before[n], p.detach()), n
        else:
            assert n.startswith("heads."), n
    ck = torch.load(tmp_path / "checkpoint_epoch_1.pt", weights_only=False)
    sd = {k[len("backbone."):]: v for k, v in ck["model_state_dict"].items() if k.startswith("backbone.")}
    back = rsref.create("resnetrs101")
    missing, unexpected = back.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert len(ck["optimizer_state_dict"]["state"]) == len(list(tr.model.parameters()))
    with torch.no_grad():
        bb.layer1[0].se.fc1.weight.zero_()
    tr._load_checkpoint(tmp_path / "checkpoint_epoch_1.pt")
    assert torch.equal(bb.layer1[0].se.fc1.weight.detach().cpu(), sd["layer1.0.se.fc1.weight"].cpu())


def test_resnetrs101_graphed_step_matches_eager(dev):
    """StepEngine(cuda_graph=True) captures the whole step of Classifier("resnetrs101") (``graph_safe``: no SE or pool
    kernel synchronises with the host): eager warm-up, capture + replay, two replays -- losses and every parameter
    equal the eager engine's bit for bit."""
    from spine_vision_amd.training import Classifier, StepEngine
    from spine_vision_amd.training.trainers.classification import _create_tasks_for_training

    tasks = _create_tasks_for_training(target_labels=["pfirrmann", "modic", "herniation"], label_smoothing=0.1)
    runs = []
    for graphed in (False, True):
        torch.manual_seed(7)
        model = Classifier("resnetrs101", tasks=tasks, pretrained=False, dropout=0.0, precision="bf16").to(dev).train()
        assert model.backbone.graph_safe
        eng = StepEngine(model, dev, lr=1e-4, weight_decay=1e-5, grad_clip=1.0, cuda_graph=graphed)
        g = torch.Generator().manual_seed(3)
        losses = []
        for _ in range(4):
            img = torch.rand(4, 3, 64, 64, generator=g).to(dev)
            tg = {"pfirrmann": torch.randint(0, 5, (4,), generator=g).to(dev),
                  "modic": torch.randint(0, 4, (4,), generator=g).to(dev),
                  "herniation": torch.randint(0, 2, (4,), generator=g).float().to(dev)}
            losses.append(float(eng.step_classification(img, tg)))
        torch.cuda.synchronize()
        assert len(eng._graphs) == (1 if graphed else 0)
        runs.append((losses, [p.detach().cpu().clone() for p in model.parameters()]))
    (la, pa), (lb, pb) = runs
    assert la == lb
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert not torch.equal(pa[-1], torch.zeros_like(pa[-1]))
