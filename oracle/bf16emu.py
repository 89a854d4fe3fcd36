"""bf16-emulating restatement of the HIP bf16 paths (TEST INFRASTRUCTURE ONLY).

The fp32 oracle (``resnet.py``, ``convnext.py``) is the reference's arithmetic.  The HIP ``precision="bf16"``
path rounds to bf16 at fixed points -- every tensor it STORES in bf16: GEMM / convolution operands, saved
activations, the bf16 gradient copies the GEMMs read -- and accumulates everything else in f32.  Against the
fp32 oracle its error is therefore the bf16 rounding itself, amplified by the network (VERDICT r3, weak 2:
the train-mode ResNet gradients came out 0.37 median off fp32, so a bound on that distance pins nothing).
This module runs the oracle's arithmetic in float64 with a round-to-nearest-even bf16 rounding at EXACTLY
the HIP path's store points, forward and backward, so a HIP-vs-emulation distance measures the HIP
kernels (accumulation order, a misplaced rounding, a wrong epilogue), not bf16 itself.

Rounding points restated from spine-vision_amd/backbone/resnet.py (``_forward_impl``, ``_block_backward``,
``_backward_impl``), which restate timm ResNet (reference spine_vision/training/models/backbone.py:27,29):

  forward   x0 = bf16(image, NHWC);  every conv: y = bf16(conv(x, bf16(w)))  (f32 accumulate);
            BN statistics of the bf16 y;  inner BN + ReLU -> bf16 a;  block output
            out = bf16(ReLU(BN(y_last) + shortcut)), shortcut = x_in or BN(bf16(conv_ds(x_in)));
            stem a0 = bf16(ReLU(BN(y0))) -> max-pool;  features = avgpool(out) in f32.
  backward  the gradient stream -- into every block output (avg-pool backward / the next block's dx) and
            into the max-pool output -- is stored bf16 (``grad_bf16``, the default, as resnet.py's grad_dtype;
            False: f32, the round-4 layout); a projection block's conv1 data gradient is stored bf16 into dx
            before the shortcut's is added (two roundings), an identity block's dx is the f32 sum of the
            masked stream and conv1's data gradient, rounded once; the gradient at every conv OUTPUT y (BN
            backward result) and at every inner activation a (conv data gradient) is stored bf16; weight
            gradients are f32 products of the bf16 operands.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to bf16 and back (exact for float32 / float64 inputs in bf16 range)."""
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundFwd(torch.autograd.Function):
    """bf16 store of a forward value; the gradient passes through unchanged."""

    @staticmethod
    def forward(ctx, x):  # noqa: D401
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """Identity forward; the gradient arriving here is stored bf16 (rounded) before it flows on."""

    @staticmethod
    def forward(ctx, x):  # noqa: D401
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


def qf(x: torch.Tensor) -> torch.Tensor:
    return _RoundFwd.apply(x)


def qg(x: torch.Tensor) -> torch.Tensor:
    return _RoundGrad.apply(x)


def _conv(x, conv, params, stride, pad):
    return qf(F.conv2d(x, qf(params[id(conv.weight)]), None, stride, pad))


class ResNetBf16Emu:
    """Functional emulation over an ``oracle.resnet.ResNet`` (its parameters, promoted to ``dtype``, are leaf
    tensors with ``.grad``).  ``forward(img)`` -> features; call ``.backward`` on a loss of them."""

    def __init__(self, model: torch.nn.Module, dtype=torch.float64, train: bool = True, grad_bf16: bool = True) -> None:
        self.model = model
        self.dtype = dtype
        self.train = train
        self.grad_bf16 = grad_bf16
        self.params = {id(p): p.detach().to(dtype).clone().requires_grad_(True) for p in model.parameters()}
        # BN buffers promoted too (updated in place in train mode)
        self.state = {}
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                self.state[id(m)] = (m.running_mean.detach().to(dtype).clone(), m.running_var.detach().to(dtype).clone())

    def named_grads(self) -> dict:
        return {n: self.params[id(p)].grad for n, p in self.model.named_parameters()}

    def named_buffers(self) -> dict:
        out = {}
        for n, m in self.model.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                rm, rv = self.state[id(m)]
                out[f"{n}.running_mean"] = rm
                out[f"{n}.running_var"] = rv
        return out

    def _bn_w(self, bn):
        return self.params[id(bn.weight)], self.params[id(bn.bias)]

    def _bnf(self, y, bn):
        rm, rv = self.state[id(bn)]
        w, b = self._bn_w(bn)
        return F.batch_norm(y, rm, rv, w, b, training=self.train, momentum=0.1 if bn.momentum is None else bn.momentum,
                            eps=bn.eps)

    def _block(self, blk, x_in):
        P = self.params
        # a projection block stores conv1's data gradient into the bf16 dx before adding the shortcut's
        xc = qg(x_in) if (self.grad_bf16 and blk.downsample is not None) else x_in
        if hasattr(blk, "conv3"):  # Bottleneck: stride on the 3x3
            y1 = qg(_conv(xc, blk.conv1, P, 1, 0))
            a1 = qg(qf(F.relu(self._bnf(y1, blk.bn1))))
            y2 = qg(_conv(a1, blk.conv2, P, blk.conv2.stride, 1))
            a2 = qg(qf(F.relu(self._bnf(y2, blk.bn2))))
            y_last = qg(_conv(a2, blk.conv3, P, 1, 0))
            bn_last = blk.bn3
        else:  # BasicBlock
            y1 = qg(_conv(xc, blk.conv1, P, blk.conv1.stride, 1))
            a1 = qg(qf(F.relu(self._bnf(y1, blk.bn1))))
            y_last = qg(_conv(a1, blk.conv2, P, 1, 1))
            bn_last = blk.bn2
        if blk.downsample is not None:
            dconv, dbn = blk.downsample[0], blk.downsample[1]
            yd = qg(_conv(x_in, dconv, P, dconv.stride, 0))
            sc = self._bnf(yd, dbn)
        else:
            sc = x_in
        out = qf(F.relu(self._bnf(y_last, bn_last) + sc))
        return qg(out) if self.grad_bf16 else out

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        m = self.model
        x0 = qf(img.to(self.dtype))
        y0 = qg(_conv(x0, m.conv1, self.params, 2, 3))
        a0 = qf(F.relu(self._bnf(y0, m.bn1)))
        x = F.max_pool2d(a0, 3, 2, 1)
        if self.grad_bf16:
            x = qg(x)  # the stem's max-pool backward reads the bf16 stream
        for i in range(1, 5):
            for blk in getattr(m, f"layer{i}"):
                x = self._block(blk, x)
        return x.mean((2, 3))


def classifier_forward(emu: ResNetBf16Emu, heads: torch.nn.ModuleDict, img: torch.Tensor) -> tuple[dict, dict]:
    """The Classifier around the emulated backbone (dropout 0): per-task logits and the promoted head
    parameters {name: leaf} (the HIP heads run in f32 on the f32 features)."""
    f = emu.forward(img)
    hp = {}
    out = {}
    for t, h in heads.items():
        w = h.weight.detach().to(emu.dtype).clone().requires_grad_(True)
        b = h.bias.detach().to(emu.dtype).clone().requires_grad_(True)
        hp[f"heads.{t}.weight"], hp[f"heads.{t}.bias"] = w, b
        out[t] = F.linear(f, w, b)
    return out, hp


def classifier_loss(out: dict, targets: dict, task_names, label_smoothing: float = 0.1) -> torch.Tensor:
    """The reference multi-task loss (oracle.heads.Classifier.get_loss) on emulated logits."""
    loss = 0.0
    for t in task_names:
        y = targets[t]
        if y.dtype.is_floating_point:  # binary head: BCEWithLogits on [B, 1]
            y = y.to(out[t].dtype)
            loss = loss + F.binary_cross_entropy_with_logits(out[t], y.unsqueeze(-1) if y.dim() == 1 else y)
        else:
            loss = loss + F.cross_entropy(out[t], y.long(), label_smoothing=label_smoothing)
    return loss


def classifier_grads(ref: torch.nn.Module, img: torch.Tensor, targets: dict, dtype=torch.float64,
                     train: bool = True, grad_bf16: bool = True) -> tuple[dict, dict, dict]:
    """One forward + backward of an ``oracle.heads.Classifier`` over a ResNet backbone with the HIP bf16 path's
    rounding points, the arithmetic in ``dtype``.  -> (logits {task}, grads {param name}, BN buffers {name}).
    ``ref`` is not modified."""
    emu = ResNetBf16Emu(ref.backbone, dtype=dtype, train=train, grad_bf16=grad_bf16)
    out, hp = classifier_forward(emu, ref.heads, img)
    classifier_loss(out, targets, ref.task_names).backward()
    grads = {"backbone." + n: g for n, g in emu.named_grads().items()}
    grads.update({n: v.grad for n, v in hp.items()})
    bufs = {"backbone." + n: b for n, b in emu.named_buffers().items()}
    return {t: o.detach() for t, o in out.items()}, grads, bufs


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cosine(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def floor_check(hip: dict, emu64: dict, emu32: dict, *, ratio_median: float, ratio_max: float, min_floor: float,
                min_cos: float) -> dict:
    """bf16 parity against the emulation, relative to the bf16 NOISE FLOOR.

    Two computations that round at the same points but accumulate differently (the emulation in float64 and in
    float32) flip a few bf16 roundings, and in a deep network those flips compound until the two are about one
    bf16 rounding apart (measured on ResNet-50: 0.24-0.26 median relative difference of the train-mode
    gradients, 0.03 in eval mode; a 1e-9 input perturbation that flips nothing gives 0.0).  The HIP path is a
    third such computation, so its distance to the float64 emulation is bounded by a multiple of that floor,
    per tensor: ``hip_err <= ratio_max * max(floor, min_floor)`` and the median ratio <= ``ratio_median``;
    a dropped, zeroed or mis-scaled gradient also fails the cosine / norm-ratio guard (cosine >= ``min_cos``,
    norm within 2x).  -> {name: (hip_err, floor, ratio, cos, norm ratio)}."""
    import numpy as np

    out = {}
    for n, ref in emu64.items():
        h = hip[n]
        e, f = rel(h, ref), rel(emu32[n], ref)
        nr = float(h.detach().double().norm() / (ref.double().norm() + 1e-300))
        out[n] = (e, f, e / max(f, min_floor), cosine(h, ref), nr)
    ratios = [v[2] for v in out.values()]
    bad = {n: v for n, v in out.items() if v[2] > ratio_max or v[3] < min_cos or not (0.5 < v[4] < 2.0)}
    assert not bad, bad
    assert float(np.median(ratios)) <= ratio_median, float(np.median(ratios))
    return out


# ==============================================================================================================
# ConvNeXt: the HIP bf16 path's store points, restated from spine-vision_amd/backbone/
# convnext.py (``_forward_impl``, ``_block_backward``, ``_backward_impl``) and the kernels it calls
# (spine-vision_amd/kernels.py), over the timm ConvNeXt of oracle/convnext.py (reference backbone.py:50,164-170):
#
#   forward   stem     P = bf16(image patches);  z0 = bf16(P . bf16(W)^T + b);  x = LN(z0) (f32, stats of bf16 z0)
#             block    z = bf16(dwconv7(x) + b_dw) (f32 x, f32 taps);  y = bf16(LN(z)) (stats of the bf16 z);
#                      h = y . bf16(W1)^T + b1 (f32);  a = bf16(GELU(h)),  g' = bf16(GELU'(h))  (one erf);
#                      x_out = gamma * (a . bf16(W2)^T + b2) + x   (f32 residual stream)
#             downs.   Pd = bf16(LN(x));  x = Pd . bf16(Wd)^T + bd (f32)
#             head     feat = LN(mean_hw(x)) (f32)
#   backward  the gradient stream d into every block / stage output is f32, and its bf16 copy db is the GEMMs'
#             operand;  block: dh = bf16((db . bf16(W2 * gamma)) * g');  dy = bf16(dh . bf16(W1));
#             dz = bf16(LN_bwd(dy; bf16 z));  d += dwconv7^T(dz) (f32), db = bf16(d);
#             dW_dw = sum dz * x (f32), LN / bias gradients f32 sums of the bf16 operands;
#             weight gradients dW = sum_s bf16(A_s^T B_s): each split-K slice's partial over its contiguous rows
#             rounded to bf16 once, the slices summed in f32 (bf16 slabs, kernels._bf16_slabs), or the plain f32
#             product where the build keeps f32 slabs (the stem's 48-column gradient); fc2: dW2 = gamma * G,
#             dgamma = rowdot(W2, G) + b2 * colsum(db), db2 = gamma * colsum(db) with G = d^T a in slabs;
#             downsample: dPd = db . bf16(Wd) (f32), LN backward to f32 d;  stem: dz0 = bf16(LN_bwd(d; bf16 z0)).
# The split-K geometry is the implementation's (a pure function of the shapes): the caller passes it in as
# ``wgrad_split(N, K, M, target) -> (split, bf16_slabs)``.
# ==============================================================================================================

def _ln_fwd(z, w, b, eps):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (z - mean) * rstd * w + b, mean, rstd


def _ln_bwd(dy, z, mean, rstd, w):
    """-> dz, dw (sum over rows), db for LayerNorm over the last dim (rows flattened by the caller)."""
    xh = (z - mean) * rstd
    g = dy * w
    dz = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dz, (dy * xh).reshape(-1, z.shape[-1]).sum(0), dy.reshape(-1, z.shape[-1]).sum(0)


def _gelu_pair(h):
    c = 0.7071067811865476
    cdf = 0.5 * (1.0 + torch.erf(h * c))
    return h * cdf, cdf + h * torch.exp(-0.5 * h * h) * 0.3989422804014327


def _dw(x, w, b=None):
    """depthwise 7x7, pad 3, NHWC in / out"""
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=x.shape[-1])
    return y.permute(0, 2, 3, 1)


def _slab_wgrad(A, Bm, split: int, bf16_slabs: bool):
    """G = A^T B over rows M (A [M,N], B [M,K]) in ``split`` contiguous row slices, each partial rounded to bf16 when
    ``bf16_slabs`` (the v9 weight gradient's P8 slab store), summed in slice order."""
    M = A.shape[0]
    if not bf16_slabs or split <= 1:
        return A.t() @ Bm
    per = M // split
    G = None
    for s in range(split):
        part = bf16_round(A[s * per:(s + 1) * per].t() @ Bm[s * per:(s + 1) * per])
        G = part if G is None else G + part
    return G


# The depthwise conv's operands: the matrix-core kernels (csrc/dwmfma.hip, SV_DW_MFMA=1 in the product) round x / dz's
# partner and the taps to bf16 -- torch.autocast's precision for conv_dw -- where the VALU kernels take f32 x and taps.
# Same switch and default as spine_vision_amd/kernels.py DW_MFMA (tests/test_bf16emu_cpu.py checks they agree).
DW_BF16_OPERANDS = os.environ.get("SV_DW_MFMA", "1") != "0"
# ... and the weight gradient's x, when the product's matrix-core weight gradient is on (SV_DW_MFMA_WGRAD, opt-in)
DW_BF16_WGRAD = DW_BF16_OPERANDS and os.environ.get("SV_DW_MFMA_WGRAD", "0") != "0"

# the tape keeps the bf16-rounded tensors as bf16 (exact, a quarter of float64's memory); a check that disables the
# rounding (bf16_round -> identity, test_oracle_golden) must keep them in the working dtype
STORE_BF16 = True


class ConvNeXtBf16Emu:
    """Functional emulation over an ``oracle.convnext.ConvNeXt`` in ``dtype`` (float64 = the reference for the floor
    check, float32 = the floor itself).  ``forward(img)`` -> features (tape kept); ``backward(dfeat)`` -> {name: grad}.
    ``device``: where the arithmetic runs (the float64 restatement of a 512x512 bs32 step is ~15 TFLOP; tests run
    the large cases on the GPU's float64 units, the small ones on the CPU -- the same code either way)."""

    def __init__(self, model: torch.nn.Module, dtype=torch.float64, wgrad_split=None, block_wgrad_target: int = 256,
                 device="cpu", dw_bf16: bool | None = None) -> None:
        self.model = model
        self.dw_bf16 = DW_BF16_OPERANDS if dw_bf16 is None else dw_bf16
        self.dw_bf16_wgrad = self.dw_bf16 and DW_BF16_WGRAD
        self.dtype = dtype
        self.device = torch.device(device)
        self.P = {n: p.detach().to(self.device, dtype).clone() for n, p in model.named_parameters()}
        self.wgrad_split = wgrad_split or (lambda N, K, M, target: (1, False))
        self.block_target = block_wgrad_target
        self.tape = None

    def _q(self, t):
        return bf16_round(t)

    def _st(self, t):  # tape storage of a bf16-rounded tensor
        return t.to(torch.bfloat16) if STORE_BF16 else t

    def _lin_w(self, name):  # bf16 shadow of a GEMM weight
        return bf16_round(self.P[name])

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        P, q = self.P, self._q
        x0 = img.to(self.device, self.dtype)
        tape = {"stages": []}
        # stem: bf16 patch rows x bf16 packed weight, bf16 conv output, f32 LayerNorm2d
        pimg = q(x0)
        z0 = q(F.conv2d(pimg, self._lin_w("stem.0.weight"), P["stem.0.bias"], stride=4).permute(0, 2, 3, 1))
        x, m0, r0 = _ln_fwd(z0, P["stem.1.weight"], P["stem.1.bias"], 1e-6)
        tape["stem"] = (pimg, self._st(z0), m0, r0)
        for si, st in enumerate(self.model.stages):
            pre = f"stages.{si}."
            ds = None
            if not isinstance(st.downsample, torch.nn.Identity):
                xn_, dm, dr = _ln_fwd(x, P[pre + "downsample.0.weight"], P[pre + "downsample.0.bias"], 1e-6)
                pd = q(xn_)
                xo = F.conv2d(pd.permute(0, 3, 1, 2), self._lin_w(pre + "downsample.1.weight"),
                              P[pre + "downsample.1.bias"], stride=2).permute(0, 2, 3, 1).contiguous()
                ds = (x, self._st(pd), dm, dr)
                x = xo
            blocks = []
            for bi in range(len(st.blocks)):
                bp = f"{pre}blocks.{bi}."
                wdw = P[bp + "conv_dw.weight"]
                z = q(_dw(q(x), q(wdw), P[bp + "conv_dw.bias"]) if self.dw_bf16 else _dw(x, wdw, P[bp + "conv_dw.bias"]))
                yf, mean, rstd = _ln_fwd(z, P[bp + "norm.weight"], P[bp + "norm.bias"], 1e-6)
                y = q(yf)
                h = y @ self._lin_w(bp + "mlp.fc1.weight").t() + P[bp + "mlp.fc1.bias"]
                gl, gp = _gelu_pair(h)
                a, gh = q(gl), q(gp)
                del h, gl, gp
                xo = P[bp + "gamma"] * (a @ self._lin_w(bp + "mlp.fc2.weight").t() + P[bp + "mlp.fc2.bias"]) + x
                blocks.append((x, self._st(z), self._st(y), mean, rstd, self._st(a), self._st(gh)))
                x = xo
            tape["stages"].append((ds, blocks))
        pooled = x.mean((1, 2))
        feat, pm, pr = _ln_fwd(pooled, P["head.norm.weight"], P["head.norm.bias"], 1e-6)
        tape["pool"] = (pooled, pm, pr, tuple(x.shape))
        self.tape = tape
        return feat

    def backward(self, dfeat: torch.Tensor) -> dict:
        P, q, dt = self.P, self._q, self.dtype
        T, self.tape = self.tape, None
        G = {}
        pooled, pm, pr, shape = T["pool"]
        dpool, G["head.norm.weight"], G["head.norm.bias"] = _ln_bwd(dfeat.to(self.device, dt), pooled, pm, pr,
                                                                    P["head.norm.weight"])
        B, H, W, C = shape
        d = (dpool / (H * W)).view(B, 1, 1, C).expand(B, H, W, C).contiguous()
        for si in range(len(T["stages"]) - 1, -1, -1):
            ds, blocks = T["stages"][si]
            pre = f"stages.{si}."
            for bi in range(len(blocks) - 1, -1, -1):
                bp = f"{pre}blocks.{bi}."
                x, z, y, mean, rstd, a, gh = blocks[bi]
                blocks[bi] = None
                z, y, a, gh = (t.to(dt) for t in (z, y, a, gh))
                B, H, W, C = x.shape
                M = B * H * W
                db = q(d)
                db2 = db.reshape(M, C)
                w2 = P[bp + "mlp.fc2.weight"]
                gam = P[bp + "gamma"]
                dh = q((db2 @ q(w2 * gam[:, None])) * gh.reshape(M, 4 * C))
                dy = q(dh @ self._lin_w(bp + "mlp.fc1.weight")).reshape(B, H, W, C)
                dz, G[bp + "norm.weight"], G[bp + "norm.bias"] = _ln_bwd(dy, z, mean, rstd, P[bp + "norm.weight"])
                dz = q(dz)
                # side stream: fc2 (layer-scale) and fc1 weight gradients in bf16 slabs, depthwise weight gradient
                s2, b2s = self.wgrad_split(C, 4 * C, M, self.block_target)
                Gm = _slab_wgrad(db2, a.reshape(M, 4 * C), s2, b2s)
                cs = db2.sum(0)
                G[bp + "mlp.fc2.weight"] = gam[:, None] * Gm
                G[bp + "gamma"] = (w2 * Gm).sum(1) + P[bp + "mlp.fc2.bias"] * cs
                G[bp + "mlp.fc2.bias"] = gam * cs
                s1, b1s = self.wgrad_split(4 * C, C, M, self.block_target)
                G[bp + "mlp.fc1.weight"] = _slab_wgrad(dh, y.reshape(M, C), s1, b1s)
                G[bp + "mlp.fc1.bias"] = dh.sum(0)
                wdw = P[bp + "conv_dw.weight"]
                dzc = dz.permute(0, 3, 1, 2)
                G[bp + "conv_dw.weight"] = torch.nn.grad.conv2d_weight((q(x) if self.dw_bf16_wgrad else x).permute(0, 3, 1, 2),
                                                                       wdw.shape, dzc, padding=3, groups=C)
                G[bp + "conv_dw.bias"] = dz.reshape(M, C).sum(0)
                d = d + torch.nn.grad.conv2d_input((B, C, H, W), q(wdw) if self.dw_bf16 else wdw, dzc, padding=3,
                                                   groups=C).permute(0, 2, 3, 1)
            if ds is not None:
                x_prev, pd, dm, dr = ds
                pd = pd.to(dt)
                B, Ho, Wo, Co = d.shape
                Ci = x_prev.shape[-1]
                db = q(d)
                wd = P[pre + "downsample.1.weight"]
                dpd = torch.nn.grad.conv2d_input(tuple(pd.permute(0, 3, 1, 2).shape), q(wd), db.permute(0, 3, 1, 2),
                                                 stride=2).permute(0, 2, 3, 1)
                Mo = B * Ho * Wo
                sd, bsd = self.wgrad_split(Co, 4 * Ci, Mo, None)
                # patch rows in the GEMM's k order (ci, kh, kw) -- the reshape of the timm weight [Co, Ci, 2, 2]
                prow = pd.reshape(B, Ho, 2, Wo, 2, Ci).permute(0, 1, 3, 5, 2, 4).reshape(Mo, 4 * Ci)
                G[pre + "downsample.1.weight"] = _slab_wgrad(db.reshape(Mo, Co), prow, sd, bsd).view_as(wd)
                G[pre + "downsample.1.bias"] = db.reshape(Mo, Co).sum(0)
                dxp, G[pre + "downsample.0.weight"], G[pre + "downsample.0.bias"] = _ln_bwd(
                    dpd, x_prev, dm, dr, P[pre + "downsample.0.weight"])
                d = dxp
        pimg, z0, m0, r0 = T["stem"]
        z0 = z0.to(dt)
        dz0, G["stem.1.weight"], G["stem.1.bias"] = _ln_bwd(d, z0, m0, r0, P["stem.1.weight"])
        dz0 = q(dz0)
        w0 = P["stem.0.weight"]
        G["stem.0.weight"] = torch.nn.grad.conv2d_weight(pimg, w0.shape, dz0.permute(0, 3, 1, 2), stride=4)
        G["stem.0.bias"] = dz0.reshape(-1, w0.shape[0]).sum(0)
        return G


def regressor_grads(ref: torch.nn.Module, img: torch.Tensor, coords: torch.Tensor, mask: torch.Tensor,
                    dtype=torch.float64, wgrad_split=None, block_wgrad_target: int = 256, device="cpu"):
    """One forward + backward of an ``oracle.heads.CoordinateRegressor`` over a ConvNeXt backbone with the HIP bf16
    path's rounding points (ConvNeXtBf16Emu), the head and the masked loss in ``dtype`` (the HIP head runs f32 torch
    on the f32 features).  -> (pred, {param name: grad}).  ``ref`` is not modified."""
    emu = ConvNeXtBf16Emu(ref.backbone, dtype, wgrad_split, block_wgrad_target, device)
    feat = emu.forward(img).detach().requires_grad_(True)
    head = {n: p.detach().to(emu.device, dtype).clone().requires_grad_(True) for n, p in ref.head.named_parameters()}
    hn = ref.head[0]
    o = F.layer_norm(feat, hn.normalized_shape, head["0.weight"], head["0.bias"], hn.eps)
    o = F.gelu(F.linear(o, head["2.weight"], head["2.bias"]))
    pred = torch.sigmoid(F.linear(o, head["5.weight"], head["5.bias"])).view(-1, ref.num_levels, ref.num_outputs)
    m = mask.to(emu.device).unsqueeze(-1).expand_as(pred).bool()
    loss = F.smooth_l1_loss(pred[m], coords.to(emu.device, dtype)[m])
    loss.backward()
    grads = {"backbone." + n: g for n, g in emu.backward(feat.grad).items()}
    grads.update({"head." + n: v.grad for n, v in head.items()})
    return pred.detach(), grads
