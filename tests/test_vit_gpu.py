"""ViT / DeiT-III backbones on the GPU against the plain torch.nn reference of tests/_vit_ref.py, with the project's
bounds: fp32 parity mode features < 1e-4 and every gradient against float64 within max(1e-3, 3 x the fp32 reference's
own error); bf16 teacher-forced per block outputs < 2e-2 and every input / parameter gradient < 0.15.  At 224 x 224
(N = 197 tokens in Np = 200 rows) and, for speed, at 32 x 32 (N = 5 in 8 rows) and 80 x 80 (N = 26 in 32 rows).

test_vit_bf16_block_against_restatement tightens the bf16 bound with the rule of tests/test_attn_gpu.py: the float64
restatement of a block (_vit_ref.block_restated) rounds to bf16 exactly where the module stores bf16; its distance from
float64 is what rounding alone causes, and the block output, dx and every parameter gradient of the first and last
block must be within max(1e-3, 3 x that) of float64 in relative L2, for vit_tiny, deit_small, vit_base and vit_large at
32 px with B = 2 and B = 8, and for vit_tiny and deit_small at 224 px with B = 8 (M = 1600 rows: the weight gradients
leave the generic kernel for the bf16 split-K slabs).  Figures of the first run: profiles/vit_calls/parity.txt.

The module keeps every image's tokens in rows padded to a multiple of 8 (DESIGN.md "ViT / DeiT-III"): the
teacher-forced backward also checks that the pad rows of the block input gradient are exactly zero."""
import copy
import functools

import pytest
import torch

import _vit_ref as ref
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import create_vit
from spine_vision_amd.backbone.vit import VIT_CFGS, ViTHip

pytestmark = pytest.mark.gpu

MODELS = [("vit_tiny", 224), ("deit_small", 224), ("vit_tiny", 32), ("deit_small", 80)]
IDS = [f"{n}@{s}" for n, s in MODELS]


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _image(B, size):
    return ow.classification_batch(B, size, size)[0]


@functools.lru_cache(maxsize=None)
def _reference(name, size):
    """The filled reference module (untouched) and one fp32 + one float64 forward / backward of it at 2 x size x size;
    computed once per (name, size), shared, never modified."""
    r = ow.fill_module(ref.create(name, size)).train()
    state = copy.deepcopy(r.state_dict())
    img = _image(2, size)
    r32, r64 = copy.deepcopy(r), copy.deepcopy(r).double()
    f32, f64 = r32(img), r64(img.double())
    dfeat = torch.from_numpy(ow.uniform("dfeat", f32.numel(), -1, 1).reshape(f32.shape))
    f32.backward(dfeat)
    f64.backward(dfeat.double())
    return dict(ref=r, state=state, img=img, dfeat=dfeat, feat=f32.detach(),
                g32={n: p.grad for n, p in r32.named_parameters()}, g64={n: p.grad for n, p in r64.named_parameters()})


def _hip(name, size, precision, dev, train=True):
    hip = create_vit(name, precision=precision, img_size=size)
    hip.load_state_dict(_reference(name, size)["state"], strict=True)
    return hip.to(dev).train(train)


def _grads(hip, r, dev):
    for p in hip.parameters():
        p.grad = None
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f.detach(), {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


@pytest.mark.parametrize("name,size", MODELS, ids=IDS)
def test_vit_fp32_forward_backward(dev, name, size):
    r = _reference(name, size)
    f_hip, g = _grads(_hip(name, size, "fp32", dev), r, dev)
    e_f = rel(f_hip, r["feat"])
    worst = 0.0
    for n, g64 in r["g64"].items():
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        worst = max(worst, e_hip / max(1e-3, 3.0 * e_ref))
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    print(f"[vit parity] {name}@{size} fp32: features rel {e_f:.2e}, worst gradient error / bound {worst:.3f}")
    assert e_f < 1e-4


def test_vit_base_fp32_eval_forward(dev):
    r = ow.fill_module(ref.create("vit_base")).eval()
    hip = create_vit("vit_base", precision="fp32")
    hip.load_state_dict(r.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    img = _image(2, 224)
    with torch.no_grad():
        e = rel(hip(img.to(dev)), r(img))
    print(f"[vit parity] vit_base@224 fp32 eval forward rel {e:.2e}")
    assert e < 1e-4


def _pad_rows(t, Np):
    """[B, N, C] -> the module's token matrix [B * Np, C] (pad rows zero)"""
    B, N, C = t.shape
    out = torch.zeros(B, Np, C, dtype=t.dtype)
    out[:, :N] = t
    return out.view(B * Np, C)


@pytest.mark.parametrize("name,size", MODELS, ids=IDS)
def test_vit_bf16_teacher_forced(dev, name, size):
    """bf16 mode, every block fed the SAME input as the fp32 reference block, then the SAME output gradient."""
    r = _reference(name, size)
    hip = _hip(name, size, "bf16", dev)
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
    print(f"[vit parity] {name}@{size} B2 bf16: worst block output rel {worst_f:.2e}, worst block-backward rel "
          f"{worst_b:.2e}")


RESTATED = [(n, 32, B) for n in ("vit_tiny", "deit_small", "vit_base", "vit_large") for B in (2, 8)] \
    + [("vit_tiny", 224, 8), ("deit_small", 224, 8)]


@functools.lru_cache(maxsize=2)
def _filled(name, size):
    """the filled fp32 reference module alone (no forward): shared by the B = 2 and B = 8 cases, never modified"""
    return ow.fill_module(ref.create(name, size)).train()


@pytest.mark.parametrize("name,size,B", RESTATED, ids=[f"{n}@{s}-B{B}" for n, s, B in RESTATED])
def test_vit_bf16_block_against_restatement(dev, name, size, B):
    """bf16 mode, the first and the last block, teacher-forced as test_vit_bf16_teacher_forced (the block input from
    the fp32 reference chain, a fixed random output gradient) against the float64 block; bound: max(1e-3, 3 x the error
    of the rounding-only restatement), for the block output, dx and every parameter gradient."""
    r = _filled(name, size)
    C, depth, heads, ls_init, no_embed_class = VIT_CFGS[name]
    hip = ViTHip(C, 2, heads, ls_init=ls_init, no_embed_class=no_embed_class, img_size=size, precision="bf16")
    hip.blocks[0].load_state_dict(r.blocks[0].state_dict(), strict=True)
    hip.blocks[1].load_state_dict(r.blocks[depth - 1].state_dict(), strict=True)
    hip = hip.to(dev).train()
    N, Np = hip.num_tokens, hip.rows_per_img
    M = B * Np
    wg = hip._wgrads()

    def slab_split(n, k):  # the host schedule of kernels.linear_wgrad / layerscale_wgrad for this module
        split = K._wgrad_split_for(n, k, M, hip.wgrad_target)
        return split if K._bf16_slabs(n, k, M, split, True, wg.spol) else 1

    with torch.no_grad():
        x = r.tokens(_image(B, size))
        inputs = {}
        for i, rb in enumerate(r.blocks):
            if i in (0, depth - 1):
                inputs[i] = x
            x = rb(x)
    worst = 0.0
    for j, i in enumerate((0, depth - 1)):
        rb, hb, x = r.blocks[i], hip.blocks[j], inputs[i]
        b64 = copy.deepcopy(rb).double()
        xr = x.double().requires_grad_(True)
        o = b64(xr)
        d = torch.randn(o.shape, generator=torch.Generator().manual_seed(i))
        o.backward(d.double())
        f64 = {"out": o.detach(), "dx": xr.grad, **{n: p.grad for n, p in b64.named_parameters()}}
        rs = ref.block_restated(rb, x, d, rows_per_img=Np, slab_split=slab_split)
        own = {"out": rel(rs["out"], f64["out"]), "dx": rel(rs["dx"], f64["dx"]),
               **{n: rel(g, f64[n]) for n, g in rs["grads"].items()}}
        for p in hb.parameters():
            p.grad = torch.zeros_like(p)
        with torch.no_grad():
            xo, saved = hip._block_forward(hb, _pad_rows(x, Np).to(dev), B, {}, save=True)
            dx = hip._block_backward(hb, saved, _pad_rows(d, Np).to(dev), B, wg, {}, ready=False)
            wg.join()
        torch.cuda.synchronize()
        dx = dx.view(B, Np, -1)
        assert bool((dx[:, N:] == 0).all()), f"block {i}: pad rows of the input gradient are not zero"
        got = {"out": xo.view(B, Np, -1)[:, :N], "dx": dx[:, :N], **{n: p.grad for n, p in hb.named_parameters()}}
        assert sorted(got) == sorted(f64) == sorted(own)
        errs = {n: rel(got[n], f64[n]) for n in f64}
        slabs = sorted(n for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
                       if slab_split(*dict(hb.named_parameters())[n + ".weight"].shape) > 1)
        print(f"[vit restated] {name}@{size} B{B} block {i} (M = {M}, bf16 slabs: {', '.join(slabs) or 'none'}): "
              "kernel / restatement error: " + ", ".join(f"{n} {errs[n]:.2e} / {own[n]:.2e}" for n in f64))
        for n in f64:
            bound = max(1e-3, 3.0 * own[n])
            worst = max(worst, errs[n] / bound)
            assert errs[n] <= bound, (name, size, B, i, n, errs[n], own[n])
    print(f"[vit restated] {name}@{size} B{B}: worst error / bound {worst:.3f}")


def test_patchify16_bitwise(dev):
    """sv_patchify16 against the host transform followed by unfold, bit for bit, for the three input forms, in both
    output dtypes, plain and inside padded token rows."""
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 48, 32
    mean = torch.tensor(K.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(K.IMAGENET_STD).view(1, 3, 1, 1)
    rgb = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    gray = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    f32 = torch.randn(B, 3, H, W, generator=g)
    host = {
        "f32": (f32, f32),
        "u8 hwc": (rgb, (rgb.permute(0, 3, 1, 2).float() / 255.0 - mean) / std),
        "u8 gray": (gray, (gray[:, None].expand(-1, 3, -1, -1).float() / 255.0 - mean) / std),
    }
    P = (H // 16) * (W // 16)
    for what, (inp, x) in host.items():
        want = torch.nn.functional.unfold(x, kernel_size=16, stride=16).transpose(1, 2).reshape(B * P, 768)
        for dtype in (torch.float32, torch.bfloat16):
            got = K.patchify16(inp.to(dev), out_dtype=dtype)
            assert torch.equal(got.cpu(), want.to(dtype)), (what, dtype)
            padded = K.patchify16(inp.to(dev), out_dtype=dtype, rows_per_img=P + 2, row0=1).view(B, P + 2, 768).cpu()
            assert torch.equal(padded[:, 1:P + 1].reshape(B * P, 768), want.to(dtype)), (what, dtype, "padded")
            assert bool((padded[:, 0] == 0).all()) and bool((padded[:, P + 1] == 0).all())


@pytest.mark.parametrize("name,size", [("vit_tiny", 224), ("deit_small", 80)], ids=["vit_tiny@224", "deit_small@80"])
def test_vit_side_stream_matches_single_stream(dev, name, size):
    """The weight gradients on the side stream (default) against every kernel on the current stream
    (SV_SIDE_STREAM=0): the same kernels, so features and gradients are equal bit for bit; run to run too."""
    r = _reference(name, size)
    hip = _hip(name, size, "bf16", dev)
    assert hip.overlap_wgrad
    f_a, g_a = _grads(hip, r, dev)
    f_b, g_b = _grads(hip, r, dev)
    hip.overlap_wgrad = False
    f_c, g_c = _grads(hip, r, dev)
    assert torch.equal(f_a, f_b) and torch.equal(f_a, f_c)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), f"{n} differs run to run"
        assert torch.equal(g_a[n], g_c[n]), f"{n}: side stream and single stream differ"


def test_vit_reports_every_parameter_ready_and_eval_matches(dev):
    r = _reference("deit_small", 80)
    hip = _hip("deit_small", 80, "bf16", dev)
    seen: list = []
    hip.grad_ready_hook = seen.extend
    f_train, _ = _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert sorted(names[id(p)] for p in seen) == sorted(names.values())
    with torch.no_grad():  # the tape-free forward (fc1 writes GELU(h) only) gives the training forward's features
        assert torch.equal(hip.eval()(r["img"].to(dev)), f_train)
    with pytest.raises(ValueError, match="LocalizationConfig.image_size"):
        hip(torch.zeros(1, 3, 96, 96, device=dev))


def test_vit_step_engine_classification_and_localization(dev):
    """Classifier("vit_base") and CoordinateRegressor("vit_small") through StepEngine at 2 x 224 x 224, unchanged
    trainers' step calls: the loss decreases over three steps on a fixed batch."""
    from spine_vision_amd.training import Classifier, CoordinateRegressor, StepEngine
    from spine_vision_amd.training.trainers.classification import _create_tasks_for_training

    torch.manual_seed(0)
    tasks = _create_tasks_for_training(target_labels=["pfirrmann", "modic", "herniation"], label_smoothing=0.1)
    m = Classifier(backbone="vit_base", tasks=tasks, pretrained=False, dropout=0.0).to(dev).train()
    img, targets = ow.classification_batch(2, 224, 224)
    img, tg = img.to(dev), {k: v.to(dev) for k, v in targets.items()}
    eng = StepEngine(m, dev, lr=2e-5, weight_decay=1e-5, grad_clip=1.0)
    cls_losses = [float(eng.step_classification(img, tg)) for _ in range(3)]
    print(f"[vit step] Classifier(vit_base) losses {cls_losses}")
    assert all(torch.isfinite(torch.tensor(cls_losses))) and cls_losses[2] < cls_losses[0]

    m = CoordinateRegressor("vit_small", pretrained=False, dropout=0.0).to(dev).train()
    u8 = torch.from_numpy(ow.uint8_images("loc.image", 2, 224, 224)).to(dev)  # the device-transform input form
    _, coords, mask = ow.localization_batch(2, 224, 224)
    eng = StepEngine(m, dev, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    loc_losses = [float(eng.step_localization(u8, coords.to(dev), mask.to(dev))) for _ in range(3)]
    print(f"[vit step] CoordinateRegressor(vit_small) losses {loc_losses}")
    assert all(torch.isfinite(torch.tensor(loc_losses))) and loc_losses[2] < loc_losses[0]
