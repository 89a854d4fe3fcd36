"""Swin backbones on the GPU against the plain torch.nn reference of tests/_swin_ref.py, with the bounds of
tests/test_vit_gpu.py: fp32 parity mode features < 1e-4 and every gradient (the relative-position tables included)
against float64 within max(1e-3, 3 x the fp32 reference's own error); bf16 blocks, teacher-forced from the fp32
reference chain, against the float64 block within max(1e-3, 3 x the error of the restatement that rounds where the
module rounds: _swin_ref.block_restated), capped by the flat teacher-forced bounds (block output < 2e-2, every
gradient < 0.15).

The residual stream of a stage has B * H * W rows rounded up to a multiple of 8 (DESIGN.md "Swin"); at 224 px the
last stage has 49 rows per image, so B = 1, 2 and 3 all carry tail rows there: their gradient must be exactly zero.

Stochastic depth runs with fixed scale vectors through the ``drop_path_scales`` hook on both sides.

The call forms of a Swin step that no other test reaches (the K = 96 -> N = 288 qkv GEMM, the bias-free 4C -> 2C
reduction with its two gradients, LayerNorm at eps 1e-5) are compared per element with float64 on the same
bf16-rounded operands under the bound rule of tests/test_vit_calls_gpu.py: an f32-accumulated product of exact bf16
operands differs from float64 by at most K * 2^-24 * S, S = |A| @ |B| (+ |bias|); a bf16 store adds 2^-8 |ref|, an f32
store 2^-23 |ref|; bf16 slabs add 2^-8 sum_s |slab_s|; the assertion is |got - ref| <= 2 x bound for every element."""
import copy
import functools

import pytest
import torch

import _swin_ref as ref
from oracle import weights as ow
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone.swin import EPS, create_swin

pytestmark = pytest.mark.gpu

# (name, image size, depths or None for the variant's own)
MODELS = [("swin_tiny", 224, None), ("swin_base", 224, None), ("swin_tiny", 256, (2, 2, 2, 2))]
IDS = ["swin_tiny@224", "swin_base@224", "swin_tiny-2222@256"]
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _image(B, size):
    return ow.classification_batch(B, size, size)[0]


def _fixed_scales(index, branch, B):
    """Deterministic stochastic-depth draws: sample (index + branch + b) % 3 == 0 is dropped (never in block 0),
    the others scaled by 1 / (1 - p) with p = 0.05 + 0.01 * index."""
    if index == 0:
        return torch.ones(B, dtype=torch.float32)
    keep = 1.0 - (0.05 + 0.01 * index)
    return torch.tensor([0.0 if (index + branch + b) % 3 == 0 else 1.0 / keep for b in range(B)], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _reference(name, size, depths, scales=False):
    """The filled reference module (untouched) and one fp32 + one float64 forward / backward of it at 2 x size x size;
    computed once per case, shared, never modified."""
    r = ow.fill_module(ref.create(name, size, drop_path_rate=0.1 if scales else 0.0, depths=depths)).train()
    if scales:
        r.set_drop_path_scales(_fixed_scales)
    state = copy.deepcopy(r.state_dict())
    img = _image(2, size)
    r32, r64 = copy.deepcopy(r), copy.deepcopy(r).double()
    f32, f64 = r32(img), r64(img.double())
    dfeat = torch.from_numpy(ow.uniform("dfeat", f32.numel(), -1, 1).reshape(f32.shape))
    f32.backward(dfeat)
    f64.backward(dfeat.double())
    return dict(ref=r, state=state, img=img, dfeat=dfeat, feat=f32.detach(),
                g32={n: p.grad for n, p in r32.named_parameters()}, g64={n: p.grad for n, p in r64.named_parameters()})


def _hip(name, size, depths, precision, dev, scales=False):
    hip = create_swin(name, precision=precision, img_size=size, depths=depths, drop_path_rate=0.1 if scales else 0.0)
    hip.load_state_dict(_reference(name, size, depths, scales)["state"], strict=True)
    if scales:
        hip.drop_path_scales = _fixed_scales
    return hip.to(dev).train()


def _grads(hip, r, dev):
    for p in hip.parameters():
        p.grad = None
    f = hip(r["img"].to(dev))
    f.backward(r["dfeat"].to(dev))
    torch.cuda.synchronize()
    return f.detach(), {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters()}


def _assert_fp32_parity(tag, f_hip, g, r):
    e_f = rel(f_hip, r["feat"])
    worst = 0.0
    assert sorted(g) == sorted(r["g64"])
    for n, g64 in r["g64"].items():
        e_hip, e_ref = rel(g[n].double(), g64), rel(r["g32"][n].double(), g64)
        worst = max(worst, e_hip / max(1e-3, 3.0 * e_ref))
        assert e_hip < max(1e-3, 3.0 * e_ref), f"{n}: hip {e_hip} vs fp32 reference {e_ref}"
    print(f"[swin parity] {tag} fp32: features rel {e_f:.2e}, worst gradient error / bound {worst:.3f}")
    assert e_f < 1e-4


@pytest.mark.parametrize("name,size,depths", MODELS, ids=IDS)
def test_swin_fp32_forward_backward(dev, name, size, depths):
    r = _reference(name, size, depths)
    f_hip, g = _grads(_hip(name, size, depths, "fp32", dev), r, dev)
    _assert_fp32_parity(f"{name}@{size}", f_hip, g, r)


def test_swin_fp32_stochastic_depth_with_fixed_scales(dev):
    """Some samples dropped in some blocks, on both sides; model.eval() ignores the scales."""
    name, size, depths = "swin_tiny", 224, (2, 2, 2, 2)
    r = _reference(name, size, depths, True)
    plain = _reference(name, size, depths)
    assert rel(r["feat"], plain["feat"]) > 1e-3, "the fixed scales drop nothing"
    hip = _hip(name, size, depths, "fp32", dev, scales=True)
    f_hip, g = _grads(hip, r, dev)
    _assert_fp32_parity(f"{name}@{size} drop-path", f_hip, g, r)
    with torch.no_grad():
        e = rel(hip.eval()(r["img"].to(dev)), copy.deepcopy(r["ref"]).eval()(r["img"]))
    assert e < 1e-4, e


def _rows(t, rows):
    """[B, H, W, C] -> the module's stream [rows, C] (tail rows zero)"""
    C = t.shape[-1]
    out = torch.zeros(rows, C, dtype=t.dtype)
    out[:t.numel() // C] = t.reshape(-1, C)
    return out


@functools.lru_cache(maxsize=2)
def _chain(B):
    """The filled fp32 swin_tiny reference at 224 and the input of every block along its fp32 chain for B images."""
    r = ow.fill_module(ref.create("swin_tiny", 224, drop_path_rate=0.0)).train()
    inputs = {}
    with torch.no_grad():
        x = r.patch_embed(_image(B, 224))
        for s, st in enumerate(r.layers):
            x = st.downsample(x)
            for j, blk in enumerate(st.blocks):
                inputs[(s, j)] = x
                x = blk(x)
    return r, inputs


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("scales", [False, True], ids=["plain", "drop-path"])
def test_swin_bf16_block_against_restatement(dev, B, scales):
    """bf16 mode, the first (unshifted) and the last (shifted, except in the last stage where the window is the grid)
    block of each stage of swin_tiny at 224 px; with ``scales`` each branch drops some samples (B >= 2)."""
    r, inputs = _chain(B)
    hip = create_swin("swin_tiny", precision="bf16", img_size=224).to(dev).train()
    hip.load_state_dict(r.state_dict(), strict=True)
    wg = hip._wgrads()
    worst = 0.0
    for s, st in enumerate(r.layers):
        for j in (0, len(st.blocks) - 1):
            rb, hb, x = st.blocks[j], hip.layers[s].blocks[j], inputs[(s, j)]
            assert (hb.window, hb.shift) == (rb.w, rb.shift)
            g_, C = x.shape[1], x.shape[-1]
            n, rows = B * g_ * g_, -(-(B * g_ * g_) // 8) * 8
            s1 = s2 = None
            if scales:
                s1 = torch.tensor([0.0 if b % 2 == 0 else 1.25 for b in range(B)]) if B > 1 else torch.tensor([1.25])
                s2 = torch.tensor([1.25 if b != 1 else 0.0 for b in range(B)])
            d = torch.randn(x.shape, generator=torch.Generator().manual_seed(10 * s + j))

            def slab_split(n_, k_):  # the host schedule of kernels.linear_wgrad for this module
                split = K._wgrad_split_for(n_, k_, rows, hip.wgrad_target)
                return split if K._bf16_slabs(n_, k_, rows, split, True, wg.spol) else 1

            f64 = ref.block_restated(rb, x, d, rows=rows, s1=s1, s2=s2, rounded=False)
            rs = ref.block_restated(rb, x, d, rows=rows, slab_split=slab_split, s1=s1, s2=s2)
            own = {"out": rel(rs["out"], f64["out"]), "dx": rel(rs["dx"], f64["dx"]),
                   **{k: rel(v, f64["grads"][k]) for k, v in rs["grads"].items()}}
            for p in hb.parameters():
                p.grad = torch.zeros_like(p)
            hip.drop_path_scales = (lambda i, br, B_: (s1, s2)[br]) if scales else None
            hb.drop_path = 0.2 if scales else 0.0
            with torch.no_grad():
                xo, saved = hip._block_forward(hb, _rows(x, rows).to(dev), B, getattr(hip, f"ls_ones{s}"), {}, save=True)
                dx = hip._block_backward(hb, saved, _rows(d, rows).to(dev), B, wg, {})
                wg.join()
            torch.cuda.synchronize()
            assert rows == n or bool((dx[n:] == 0).all()), f"stage {s} block {j}: tail rows of dx are not zero"
            got = {"out": xo[:n].view(x.shape), "dx": dx[:n].view(x.shape), **{k: p.grad for k, p in hb.named_parameters()}}
            want = {"out": f64["out"], "dx": f64["dx"], **f64["grads"]}
            assert sorted(got) == sorted(want) == sorted(own)
            errs = {k: rel(got[k], want[k]) for k in want}
            print(f"[swin restated] B{B} stage {s} block {j} (rows {rows}, shift {hb.shift}): kernel / restatement "
                  "error: " + ", ".join(f"{k} {errs[k]:.2e} / {own[k]:.2e}" for k in want))
            for k in want:
                bound = min(max(1e-3, 3.0 * own[k]), 2e-2 if k == "out" else 0.15)
                worst = max(worst, errs[k] / bound)
                assert errs[k] <= bound, (B, s, j, k, errs[k], own[k])
    print(f"[swin restated] B{B} {'drop-path' if scales else 'plain'}: worst error / bound {worst:.3f}")


def test_a_dropped_branch_contributes_exactly_nothing(dev):
    """Every sample dropped in both branches of a block: the output is the input, dx is d, and every gradient of the
    block is exactly zero -- the scratch GEMM result (and NaN-free garbage in it) never reaches anything."""
    r, inputs = _chain(2)
    hip = create_swin("swin_tiny", precision="bf16", img_size=224).to(dev).train()
    hip.load_state_dict(r.state_dict(), strict=True)
    hb, x = hip.layers[2].blocks[1], inputs[(2, 1)]
    hb.drop_path = 0.5
    hip.drop_path_scales = lambda i, br, B: torch.zeros(B)
    d = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    for p in hb.parameters():
        p.grad = torch.zeros_like(p)
    wg = hip._wgrads()
    with torch.no_grad():
        xin, din = _rows(x, 392).to(dev), _rows(d, 392).to(dev)
        xo, saved = hip._block_forward(hb, xin, 2, hip.ls_ones2, {}, save=True)
        dx = hip._block_backward(hb, saved, din.clone(), 2, wg, {})
        wg.join()
    torch.cuda.synchronize()
    assert torch.equal(xo, xin) and torch.equal(dx, din)
    for n, p in hb.named_parameters():
        assert not p.grad.any(), f"{n} got a gradient from a dropped branch"


@pytest.mark.parametrize("B", [1, 3])
def test_swin_bf16_whole_model_with_tail_rows(dev, B):
    """B = 1 and B = 3 at 224 px: 196 B and 49 B rows are no multiples of 8 in the last two stages.  The whole bf16
    step runs, every gradient is finite, an image's features do not depend on the batch it is in, and the result is
    bitwise repeatable."""
    torch.manual_seed(0)
    hip = create_swin("swin_tiny", precision="bf16", img_size=224, depths=(2, 2, 2, 2), drop_path_rate=0.0).to(dev).train()
    img = _image(3, 224)[:B].to(dev)
    f = hip(img)
    f.backward(torch.ones_like(f))
    torch.cuda.synchronize()
    g1 = {n: p.grad.clone() for n, p in hip.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in g1.values())
    with torch.no_grad():
        assert torch.equal(hip(img[:1]), f[:1].detach())
    for p in hip.parameters():
        p.grad = None
    f2 = hip(img)
    f2.backward(torch.ones_like(f2))
    torch.cuda.synchronize()
    assert torch.equal(f2, f) and all(torch.equal(p.grad, g1[n]) for n, p in hip.named_parameters())


def test_swin_side_stream_matches_single_stream(dev):
    """The weight gradients on the side stream (default) against every kernel on the current stream
    (SV_SIDE_STREAM=0): the same kernels, so features and gradients are equal bit for bit; run to run too."""
    name, size, depths = "swin_tiny", 224, (2, 2, 2, 2)
    r = _reference(name, size, depths, True)
    hip = _hip(name, size, depths, "bf16", dev, scales=True)
    assert hip.overlap_wgrad and hip.graph_safe is False
    seen: list = []
    hip.grad_ready_hook = seen.extend
    f_a, g_a = _grads(hip, r, dev)
    names = {id(p): n for n, p in hip.named_parameters()}
    assert sorted(names[id(p)] for p in seen) == sorted(names.values())
    hip.grad_ready_hook = None
    f_b, g_b = _grads(hip, r, dev)
    hip.overlap_wgrad = False
    f_c, g_c = _grads(hip, r, dev)
    assert torch.equal(f_a, f_b) and torch.equal(f_a, f_c)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), f"{n} differs run to run"
        assert torch.equal(g_a[n], g_c[n]), f"{n}: side stream and single stream differ"


# ---- the call forms no other test reaches, per element against float64
def _operands(M, Kd, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(M, Kd, generator=g) * 2 - 1).to(BF).to(dev)
    w = ((torch.rand(N, Kd, generator=g) * 2 - 1) * Kd ** -0.5).to(BF).to(dev)
    return a, w


def _within(got, want, bound, what):
    bad = (got.to(F64) - want).abs() > 2 * bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond 2 x bound, worst " \
        f"{float(((got.to(F64) - want).abs() / bound.clamp_min(1e-300)).max()):.2f} x bound"


@pytest.mark.parametrize("M", [104, 6272])
def test_qkv_forward_k96_n288(dev, M):
    """Swin stage 0: linear_fwd(y1 bf16 [M, 96], W bf16 [288, 96], out bf16, bias f32)."""
    a, w = _operands(M, 96, 288, M, dev)
    bias = (torch.rand(288, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
    out = torch.full((M, 288), float("nan"), device=dev, dtype=BF)
    K.linear_fwd(a, w, out=out, bias=bias, compute_bf16=True)
    want = a.to(F64) @ w.to(F64).T + bias.to(F64)
    S = a.to(F64).abs() @ w.to(F64).abs().T + bias.to(F64).abs()
    _within(out, want, 96 * U24 * S + U8 * want.abs(), "qkv forward")
    again = torch.empty_like(out)
    K.linear_fwd(a, w, out=again, bias=bias, compute_bf16=True)
    assert torch.equal(out, again)


@pytest.mark.parametrize("M,C", [(104, 96), (1568, 96), (400, 384)])
def test_patch_merging_reduction_calls(dev, M, C):
    """The bias-free reduction Linear(4C, 2C): forward to f32, data gradient to f32 [M, 4C], weight gradient
    accumulated into f32 (no bias gradient), as SwinHip calls them."""
    ym, w = _operands(M, 4 * C, 2 * C, M + C, dev)
    x = torch.full((M, 2 * C), float("nan"), device=dev, dtype=F32)
    K.linear_fwd(ym, w, out=x, compute_bf16=True)
    want = ym.to(F64) @ w.to(F64).T
    S = ym.to(F64).abs() @ w.to(F64).abs().T
    _within(x, want, 4 * C * U24 * S + U23 * want.abs(), "reduction forward")
    dsrc = (torch.rand(M, 2 * C, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(BF).to(dev)
    dym = torch.full((M, 4 * C), float("nan"), device=dev, dtype=F32)
    K.linear_dgrad(dsrc, w, out=dym, compute_bf16=True)
    want = dsrc.to(F64) @ w.to(F64)
    S = dsrc.to(F64).abs() @ w.to(F64).abs()
    _within(dym, want, 2 * C * U24 * S + U23 * want.abs(), "reduction data gradient")
    prior = torch.rand(2 * C, 4 * C, generator=torch.Generator().manual_seed(3)).to(dev)
    dw = prior.clone()
    K.linear_wgrad(dsrc, ym, out=dw, accumulate=True, compute_bf16=True, wgrad_target=256)
    G = dsrc.to(F64).T @ ym.to(F64)
    S = dsrc.to(F64).abs().T @ ym.to(F64).abs()
    split = K._wgrad_split_for(2 * C, 4 * C, M, 256)
    bound = M * U24 * S + U23 * (G.abs() + prior.to(F64))
    if K._bf16_slabs(2 * C, 4 * C, M, split, True, None):
        per = M // split
        bound = bound + U8 * sum((dsrc[s * per:(s + 1) * per].to(F64).T @ ym[s * per:(s + 1) * per].to(F64)).abs()
                                 for s in range(split))
    _within(dw, G + prior.to(F64), bound, "reduction weight gradient")


@pytest.mark.parametrize("C", [96, 384, 1024])
def test_layernorm_at_eps_1e5(dev, C):
    """layernorm_fwd(f32 -> bf16, eps = 1e-5) on rows whose variance is about eps, where 1e-5 against 1e-6 changes
    the result by tens of percent.  f32 statistics over C terms: the normalised value carries at most C * 2^-23
    relative error (mean, variance and rsqrt), the affine one more rounding, the store 2^-8."""
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(208, C, generator=g) * 3e-3 + 0.5).to(dev)
    w, b = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) - 0.5).to(dev)
    y, mean, rstd = K.layernorm_fwd(x, w, b, out_dtype=BF, eps=EPS)
    x64 = x.to(F64)
    mu = x64.mean(-1, keepdim=True)
    rs = (x64.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xh = (x64 - mu) * rs
    want = xh * w.to(F64) + b.to(F64)
    # x - mean cancels: the f32 error of the mean (C terms of magnitude |x|) enters as C * 2^-24 * |x| * rstd
    bound = U8 * want.abs() + w.to(F64).abs() * (C * U23 * xh.abs() + C * U24 * x64.abs() * rs) + U23 * want.abs()
    _within(y, want, bound, "layernorm forward")
    other = (x64 - mu) * (x64.var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt() * w.to(F64) + b.to(F64)
    assert rel(other, want) > 0.05, "the case does not tell eps 1e-5 from 1e-6"
    assert rel(mean, mu.squeeze(-1)) < C * U24 and rstd.shape == (208,)


def test_swin_step_engine_classification_and_localization(dev):
    """Classifier("swin_small") at 2 x 224 x 224 and CoordinateRegressor("swin_base") at 2 x 256 x 256 from uint8
    input through StepEngine, unchanged trainers' step calls, stochastic depth at its default rate: the loss
    decreases over three steps on a fixed batch."""
    from spine_vision_amd.training import Classifier, CoordinateRegressor, StepEngine
    from spine_vision_amd.training.trainers.classification import _create_tasks_for_training

    torch.manual_seed(0)
    tasks = _create_tasks_for_training(target_labels=["pfirrmann", "modic", "herniation"], label_smoothing=0.1)
    m = Classifier(backbone="swin_small", tasks=tasks, pretrained=False, dropout=0.0).to(dev).train()
    img, targets = ow.classification_batch(2, 224, 224)
    img, tg = img.to(dev), {k: v.to(dev) for k, v in targets.items()}
    eng = StepEngine(m, dev, lr=2e-5, weight_decay=1e-5, grad_clip=1.0)
    cls_losses = [float(eng.step_classification(img, tg)) for _ in range(3)]
    print(f"[swin step] Classifier(swin_small) losses {cls_losses}")
    assert all(torch.isfinite(torch.tensor(cls_losses))) and cls_losses[2] < cls_losses[0]

    m = CoordinateRegressor("swin_base", pretrained=False, dropout=0.0, img_size=256).to(dev).train()
    u8 = torch.from_numpy(ow.uint8_images("loc.image", 2, 256, 256)).to(dev)  # the device-transform input form
    _, coords, mask = ow.localization_batch(2, 256, 256)
    eng = StepEngine(m, dev, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    loc_losses = [float(eng.step_localization(u8, coords.to(dev), mask.to(dev))) for _ in range(3)]
    print(f"[swin step] CoordinateRegressor(swin_base) losses {loc_losses}")
    assert all(torch.isfinite(torch.tensor(loc_losses))) and loc_losses[2] < loc_losses[0]
