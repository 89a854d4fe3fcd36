"""ResNet-RS-50/101/152 and ResNet-50-D: factory surface, timm state_dict layout, parameter counts and init rules
against the plain restatement of tests/_resnetrs_ref.py.  No GPU."""
import math

import pytest
import torch

import _resnetrs_ref as rsref
from spine_vision_amd.backbone import create_resnet
from spine_vision_amd.backbone.resnet import SEModule
from spine_vision_amd.training.models.backbone import BACKBONES, NATIVE, BackboneFactory

NAMES = sorted(rsref.CFGS)


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_is_timms(name):
    ref = rsref.create(name)
    hip = create_resnet(name, precision="fp32")
    rs, hs = ref.state_dict(), hip.state_dict()
    assert sorted(rs) == sorted(hs), set(rs) ^ set(hs)
    assert all(rs[k].shape == hs[k].shape for k in rs)
    n = rsref.CFGS[name][3]
    assert sum(p.numel() for p in hip.parameters()) == n
    assert sum(p.numel() for p in ref.parameters()) == n
    assert hip.num_features == ref.num_features == rsref.CFGS[name][4]
    # strict in both directions
    r = hip.load_state_dict(rs, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    r = ref.load_state_dict(hs, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


def test_key_layout_of_the_new_parts():
    sd = create_resnet("resnetrs50", precision="fp32").state_dict()
    assert tuple(sd["conv1.0.weight"].shape) == (32, 3, 3, 3)
    assert tuple(sd["conv1.3.weight"].shape) == (32, 32, 3, 3)
    assert tuple(sd["conv1.6.weight"].shape) == (64, 32, 3, 3)
    assert tuple(sd["conv1.1.weight"].shape) == tuple(sd["conv1.4.weight"].shape) == (32,)
    assert tuple(sd["bn1.weight"].shape) == (64,)
    assert tuple(sd["maxpool.0.weight"].shape) == (64, 64, 3, 3) and tuple(sd["maxpool.1.weight"].shape) == (64,)
    for i, (c, rd) in enumerate(((256, 64), (512, 128), (1024, 256), (2048, 512)), start=1):
        assert tuple(sd[f"layer{i}.0.se.fc1.weight"].shape) == (rd, c, 1, 1)
        assert tuple(sd[f"layer{i}.0.se.fc1.bias"].shape) == (rd,)
        assert tuple(sd[f"layer{i}.0.se.fc2.weight"].shape) == (c, rd, 1, 1)
        assert tuple(sd[f"layer{i}.0.se.fc2.bias"].shape) == (c,)
        assert tuple(sd[f"layer{i}.0.downsample.1.weight"].shape)[2:] == (1, 1)
        assert f"layer{i}.0.downsample.2.running_var" in sd and f"layer{i}.0.downsample.0.weight" not in sd
        assert f"layer{i}.1.downsample.1.weight" not in sd
    d = create_resnet("resnet50_d", precision="fp32")
    assert not any(k.startswith("maxpool") or ".se." in k for k in d.state_dict())
    assert isinstance(d.layer1[0].downsample[0], torch.nn.Identity)
    pool = d.layer2[0].downsample[0]
    assert isinstance(pool, torch.nn.AvgPool2d) and pool.ceil_mode and not pool.count_include_pad
    assert d.layer2[0].downsample[1].stride == (1, 1)


@pytest.mark.parametrize("name", ["resnetrs101", "resnetrs152"])
def test_factory_creates_resnetrs(name):
    """Fails on the parent commit: the factory raises for these names there."""
    assert name in NATIVE and name in BACKBONES
    BackboneFactory._feature_dims.pop(name, None)
    assert BackboneFactory.get_feature_dim(name) == 2048  # from the table: nothing has been constructed
    assert name not in BackboneFactory._feature_dims
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert dim == 2048 and model.num_features == 2048
    assert sum(p.numel() for p in model.parameters()) == rsref.CFGS[name][3]


def test_resnetrs50_and_resnet50_d_build_but_stay_gated():
    for name in ("resnetrs50", "resnet50_d"):
        assert name in BACKBONES and name not in NATIVE
        assert create_resnet(name).num_features == 2048
        with pytest.raises(ValueError, match="not on the MI355X training path"):
            BackboneFactory.create(name, pretrained=False)


def test_init_rules():
    """timm init: kaiming_normal_(fan_out, relu) on every Conv2d (the SE convs included, their biases Conv2d's default),
    BatchNorm 1 / 0, zero_init_last on bn3."""
    torch.manual_seed(0)
    m = create_resnet("resnetrs50", precision="fp32")
    for n, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv2d):
            co, _, kh, kw = mod.weight.shape
            std = math.sqrt(2.0 / (co * kh * kw))
            if mod.weight.numel() >= 4096:
                assert abs(float(mod.weight.std()) / std - 1) < 0.1, n
            if mod.bias is not None:  # Conv2d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                bound = 1 / math.sqrt(mod.weight.shape[1])
                assert float(mod.bias.abs().max()) <= bound and float(mod.bias.abs().max()) > 0, n
        elif isinstance(mod, torch.nn.BatchNorm2d):
            last = n.endswith(".bn3")
            assert bool((mod.weight == (0.0 if last else 1.0)).all()) and bool((mod.bias == 0).all()), n
    se = m.layer3[0].se
    assert isinstance(se, SEModule) and se.fc1.bias is not None and se.fc2.bias is not None


def test_resnet50_is_unchanged():
    hip = create_resnet("resnet50", precision="bf16")
    assert sum(p.numel() for p in hip.parameters()) == 23_508_032
    assert isinstance(hip.conv1, torch.nn.Conv2d) and tuple(hip.conv1.weight.shape) == (64, 3, 7, 7)
    assert not hasattr(hip, "maxpool")
    assert not any(isinstance(mod, SEModule) for mod in hip.modules())
    assert not any(hasattr(b, "se") for b in hip.blocks())
    assert len(hip.layer2[0].downsample) == 2 and hip.layer2[0].downsample[0].stride == (2, 2)
