"""The ResNet-family backbones beyond resnet18 / resnet50 on the GPU, at 4 x 64 x 64: resnet34 (BasicBlock [3,4,6,3]),
resnet101, wide_resnet50 (base_width 128) and resnext50 (32 groups x 4: the grouped 3x3 on csrc/gconv.hip in bf16,
as its dense embedding in fp32), against the plain torch.nn reference of tests/_resnet_family_ref.py with the bounds
of tests/test_resnet_gpu.py."""
import copy
import functools

import pytest
import torch

import _resnet_family_ref as fam
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import create_resnet

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The filled reference module (train mode, untouched) and one fp32 + one float64 forward / backward of it at
    4 x 64 x 64: features, gradients and the updated buffers.  Computed once per name, shared, never modified."""
    ref = ow.fill_module(fam.create(name)).train()
    state = copy.deepcopy(ref.state_dict())
    img, _ = ow.classification_batch(4, 64, 64)
    r32, r64 = copy.deepcopy(ref), copy.deepcopy(ref).double()
    f32, f64 = r32(img), r64(img.double())
    dfeat = torch.from_numpy(ow.uniform("dfeat", f32.numel(), -1, 1).reshape(f32.shape))
    f32.backward(dfeat)
    f64.backward(dfeat.double())
    return dict(ref=ref, state=state, img=img, dfeat=dfeat, feat=f32.detach(),
                g32={n: p.grad for n, p in r32.named_parameters()}, g64={n: p.grad for n, p in r64.named_parameters()},
                buffers=dict(r32.named_buffers()))


def _hip(name, precision, dev, train=True):
    hip = create_resnet(name, precision=precision)
    missing, unexpected = hip.load_state_dict(_reference(name)["state"], strict=True)
    assert not missing and not unexpected
    return hip.to(dev).train(train)


def _grads(hip, r, dev):
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f, {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


@pytest.mark.parametrize("name", ["resnet34", "resnext50", "wide_resnet50"])
def test_family_fp32_forward_backward(dev, name):
    """fp32 parity mode (resnext50: the grouped 3x3 as its dense embedding through the f32 conv kernels): features <
    1e-4, each gradient against the float64 reference within max(1e-3, 3 x the fp32 reference's own error), buffers
    1e-5 -- the bounds of test_resnet_fp32_forward_backward."""
    r = _reference(name)
    hip = _hip(name, "fp32", dev)
    f_hip, g = _grads(hip, r, dev)
    assert rel(f_hip, r["feat"]) < 1e-4
    for n, g64 in r["g64"].items():
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    hb = dict(hip.named_buffers())
    for n, b in r["buffers"].items():
        if b.is_floating_point():
            assert rel(hb[n], b) < 1e-5, n
        else:
            assert int(hb[n]) == int(b), n


def test_resnet101_fp32_eval_forward(dev):
    ref = copy.deepcopy(_reference("resnet101")["ref"]).eval()
    hip = _hip("resnet101", "fp32", dev, train=False)
    img, _ = ow.classification_batch(2, 64, 64)
    with torch.no_grad():
        assert rel(hip(img.to(dev)), ref(img)) < 1e-4


class _MaskedReLU(torch.nn.Module):
    """ReLU with a fixed mask (NCHW bool): the reference takes the HIP forward's branch."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype)


@pytest.mark.parametrize("name", ["resnext50", "wide_resnet50"])
def test_family_bf16_teacher_forced(dev, name):
    """bf16 mode, every block fed the SAME (bf16) input as the fp32 reference block: outputs < 2e-2
    (test_resnet50_bf16_blockwise), and with the SAME output gradient every input / parameter gradient < 0.15
    (test_resnet_block_backward_teacher_forced)."""
    r = _reference(name)
    hip = _hip(name, "bf16", dev)
    with torch.no_grad():
        _, tape = hip._forward_impl(r["img"].to(dev), save=True)
    rblocks = [b for b in r["ref"].modules() if isinstance(b, (fam.BasicBlock, fam.Bottleneck))]
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
    print(f"[parity] {name}@64 B4 bf16: worst block output rel {worst_f:.2e}, worst block-backward rel {worst_b:.2e}")


def test_resnext50_bf16_dense_arm_within_precision_noise(dev, monkeypatch):
    """SV_GCONV=dense (the grouped 3x3s as dense embeddings through the bf16 conv kernels) against the default (the
    grouped kernels): per parameter the two arms' gradients are no further apart than the default arm is from the fp32
    reference -- the implementation switch sits below the precision noise."""
    r = _reference("resnext50")
    assert not K.GCONV_DENSE
    _, g_def = _grads(_hip("resnext50", "bf16", dev), r, dev)
    monkeypatch.setattr(K, "GCONV_DENSE", True)
    hip = _hip("resnext50", "bf16", dev)
    assert not hip._gconv_native
    _, g_dense = _grads(hip, r, dev)
    worst = 0.0
    for n, g32 in r["g32"].items():
        arms = float((g_dense[n].double() - g_def[n].double()).norm())
        noise = float((g_def[n].double() - g32.double()).norm())
        worst = max(worst, arms / (noise + 1e-30))
        assert arms <= noise, (n, arms, noise)
    print(f"[gconv arms] resnext50 bf16: worst (dense - default) / (default - fp32) = {worst:.3f}")


def test_resnext50_reports_every_parameter_ready(dev):
    r = _reference("resnext50")
    hip = _hip("resnext50", "bf16", dev)
    seen: list = []
    hip.grad_ready_hook = seen.extend
    _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert all(id(p) in names for p in seen)
    assert sorted(names[id(p)] for p in seen) == sorted(n for n, p in hip.named_parameters() if p.requires_grad)


def test_resnext50_side_stream_matches_single_stream(dev):
    """The per-block weight gradients on the side stream (default) against every kernel on the current stream
    (SV_SIDE_STREAM=0): the same kernels, so gradients and buffers are equal bit for bit."""
    r = _reference("resnext50")
    out = []
    for overlap in (True, False):
        hip = _hip("resnext50", "bf16", dev)
        hip.overlap_wgrad = overlap
        _, g = _grads(hip, r, dev)
        out.append(list(g.values()) + [b.detach().cpu().clone() for b in hip.buffers()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_resnext50_graph_forward_matches_eager(dev):
    """The training forward replayed from its captured graph equals the eager forward bit for bit (features,
    gradients, running statistics), over several inputs."""
    a, b = _hip("resnext50", "bf16", dev), _hip("resnext50", "bf16", dev)
    a.graph_forward, b.graph_forward = True, False
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = torch.rand(4, 3, 64, 64, generator=gen).to(dev)
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


def test_resnext50_classification_trainer_step(dev, tmp_path):
    """Classifier(backbone="resnext50") through ClassificationTrainer on the synthetic dataset: the steps run, nothing
    becomes NaN, and the grouped weight moves (from the second step on: timm's zero-initialised last BatchNorm scale
    gives a block's inner convs an exactly zero gradient in the first)."""
    from spine_vision_amd.training import ClassificationConfig, ClassificationTrainer
    from spine_vision_amd.training.datasets import SyntheticClassificationDataset

    cfg = ClassificationConfig(output_path=tmp_path, batch_size=4, num_epochs=2, num_workers=0, output_size=(64, 64),
                               backbone="resnext50", pretrained=False, precision="bf16", save_frequency=1,
                               early_stopping=False)
    tr = ClassificationTrainer(cfg, train_dataset=SyntheticClassificationDataset(8, (64, 64), seed=1),
                               val_dataset=SyntheticClassificationDataset(4, (64, 64), seed=2))
    assert tr.model.backbone.layer1[0].conv2.groups == 32
    before = tr.model.backbone.layer1[0].conv2.weight.detach().clone()
    res = tr.train()
    assert res.final_train_loss == res.final_train_loss and res.final_train_loss > 0
    assert not torch.equal(before, tr.model.backbone.layer1[0].conv2.weight.detach())
    for n, t in tr.model.state_dict().items():
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), n
