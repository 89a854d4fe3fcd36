"""EfficientNetV2-S / M / L construction against the plain torch.nn restatement of tests/_effnetv2_ref.py: no GPU."""
import pytest
import torch
import torch.nn as nn

import _effnetv2_ref as eref
from spine_vision_amd.backbone import EFFNETV2_CFGS, EfficientNetV2Hip, create_efficientnetv2
from spine_vision_amd.backbone import efficientnet as effnet
from spine_vision_amd.training.models.backbone import BACKBONES, NATIVE, BackboneFactory

NAMES = ("efficientnetv2_s", "efficientnetv2_m", "efficientnetv2_l")


@pytest.fixture(scope="module")
def models():
    return {n: BackboneFactory.create(n, pretrained=False) for n in NAMES}


def test_create_returns_1280_features(models):
    for n in NAMES:
        model, feats = models[n]
        assert isinstance(model, EfficientNetV2Hip)
        assert feats == model.num_features == 1280 == BackboneFactory.get_feature_dim(n)
        assert n in NATIVE


@pytest.mark.parametrize("name", NAMES)
def test_parameter_and_block_counts(models, name):
    model = models[name][0]
    _, _, nparams, nblocks = eref.CFGS[name]
    assert sum(p.numel() for p in model.parameters()) == nparams
    assert len(model.block_list()) == nblocks
    assert EFFNETV2_CFGS[name] == eref.CFGS[name][:2]


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_matches_restatement(models, name):
    model = models[name][0]
    ref = eref.create(name)
    sd, rsd = model.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    missing, unexpected = ref.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    missing, unexpected = model.load_state_dict(rsd, strict=True)
    assert not missing and not unexpected
    for key in ("conv_stem.weight", "bn1.running_var", "blocks.0.0.conv.weight", "blocks.1.0.conv_exp.weight",
                "blocks.1.0.conv_pwl.weight", "blocks.3.0.conv_dw.weight", "blocks.3.0.se.conv_reduce.bias",
                "blocks.3.1.se.conv_expand.weight", "blocks.5.0.bn3.num_batches_tracked", "conv_head.weight", "bn2.bias"):
        assert key in sd, key


def test_init_follows_goog_scheme():
    torch.manual_seed(0)
    model = create_efficientnetv2("efficientnetv2_s", precision="fp32")
    for n, m in model.named_modules():
        if isinstance(m, nn.Conv2d):
            fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
            std = (2.0 / fan_out) ** 0.5
            w = m.weight.detach()
            if w.numel() >= 4096:  # the sample standard deviation of n values is within ~1 / sqrt(2 n): 5 sigma
                tol = 5.0 / (2.0 * w.numel()) ** 0.5
                assert abs(float(w.std()) / std - 1.0) < tol, (n, float(w.std()), std)
                assert abs(float(w.mean())) < 5.0 * std / w.numel() ** 0.5, n
            if m.bias is not None:
                assert not m.bias.detach().any(), n
        elif isinstance(m, nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and not m.bias.detach().any(), n
            assert m.eps == 1e-5 and m.momentum == 0.1
    dw = model.blocks[3][0].conv_dw
    assert dw.groups == dw.out_channels == 256 and tuple(dw.weight.shape) == (256, 1, 3, 3)


@pytest.mark.parametrize("name", NAMES)
def test_se_width_comes_from_the_block_input(models, name):
    model = models[name][0]
    stem, stages = EFFNETV2_CFGS[name]
    cin = stem
    for si, (kind, repeats, stride, e, cout) in enumerate(stages):
        if kind == "ir":
            first, second = model.blocks[si][0], model.blocks[si][1]
            assert first.se.conv_reduce.out_channels == cin // 4
            assert tuple(first.se.conv_reduce.weight.shape) == (cin // 4, cin * e, 1, 1)
            assert tuple(first.se.conv_expand.weight.shape) == (cin * e, cin // 4, 1, 1)
            assert second.se.conv_reduce.out_channels == cout // 4
            assert second.conv_dw.out_channels == cout * e and second.has_skip and not first.has_skip
            assert first.conv_dw.out_channels % 32 == 0 and second.conv_dw.out_channels % 32 == 0
            assert first.se.conv_reduce.out_channels % 4 == 0 and second.se.conv_reduce.out_channels % 4 == 0
        cin = cout


def test_skip_rules_and_stage_table_argument():
    model = EfficientNetV2Hip(24, eref.shallow("efficientnetv2_s", (2, 2, 2, 2, 1, 1)), precision="fp32")
    kinds = [(b.kind, b.has_skip, b.stride) for b in model.block_list()]
    assert kinds == [("cn", True, 1), ("cn", True, 1), ("er", False, 2), ("er", True, 1), ("er", False, 2), ("er", True, 1),
                     ("ir", False, 2), ("ir", True, 1), ("ir", False, 1), ("ir", False, 2)]
    with pytest.raises(ValueError):
        EfficientNetV2Hip(24, (("xx", 1, 1, 1, 24),))
    with pytest.raises(ValueError):
        EfficientNetV2Hip(24, (("ir", 1, 1, 1, 24),))  # a depthwise width of 24 is not on csrc/mbconv.hip
    with pytest.raises(ValueError):
        EfficientNetV2Hip(precision="fp16")


def test_padded_strides():
    """the stored channel stride of every tensor a dense 3x3 touches is a power of two >= 32"""
    assert [effnet._pow2(c) for c in (3, 24, 32, 48, 64, 80, 96, 192, 320, 384)] == [32, 32, 32, 64, 64, 128, 128, 256, 512, 512]
    for name in NAMES:
        model = create_efficientnetv2(name, precision="bf16")
        for blk in model.block_list():
            cs = model._out_cs(blk)
            cout = (blk.conv if blk.kind == "cn" else blk.conv_pwl).out_channels
            assert cs == cout if blk.kind == "ir" else (cs >= max(cout, 32) and cs & (cs - 1) == 0)


def test_cpu_tensor_is_refused():
    model = create_efficientnetv2("efficientnetv2_s")
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 3, 32, 32))


def test_other_efficient_names_still_raise():
    for n in ("efficientnet_b0", "efficientnet_b1", "efficientnet_b4", "mobilenetv3_small", "mobilenetv3_large"):
        assert n in BACKBONES
        with pytest.raises(ValueError):
            BackboneFactory.create(n, pretrained=False)


def test_list_backbones_unchanged():
    names = BackboneFactory.list_backbones()
    assert len(names) == 46 and names == sorted(BACKBONES)  # the reference registry, as before
    assert BackboneFactory.list_backbones("efficientnetv2") == sorted(NAMES)
    assert len(NATIVE) == 31 and len(set(NATIVE)) == 31
