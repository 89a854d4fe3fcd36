"""The ResNet-family names of the reference registry beyond resnet18 / resnet50 (resnet34 / 101 / 152, the resnet50
recipes, the wide ResNets and ResNeXt-50): factory surface, timm state_dict layout and parameter counts, and the dense
embedding of a grouped weight (the fp32 parity path of ResNeXt's grouped 3x3).  No GPU."""
import pytest
import torch

import _resnet_family_ref as fam
from spine_vision_amd import kernels as K
from spine_vision_amd.backbone import create_resnet
from spine_vision_amd.training.models.backbone import BACKBONES, NATIVE, BackboneFactory

NAMES = sorted(fam.FAMILY)


@pytest.mark.parametrize("name", NAMES)
def test_factory_creates_the_family(name):
    assert name in NATIVE and name in BACKBONES
    nf = fam.FAMILY[name][5]
    BackboneFactory._feature_dims.pop(name, None)
    assert BackboneFactory.get_feature_dim(name) == nf  # from the table: nothing has been constructed
    assert name not in BackboneFactory._feature_dims
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert dim == nf and model.num_features == nf
    assert BackboneFactory.get_feature_dim(name) == nf


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_is_timms(name):
    ref = fam.create(name)
    hip = create_resnet(name, precision="fp32")
    rs, hs = ref.state_dict(), hip.state_dict()
    assert list(rs) == list(hs), set(rs) ^ set(hs)
    assert all(rs[k].shape == hs[k].shape for k in rs)
    assert sum(p.numel() for p in hip.parameters()) == fam.FAMILY[name][4]
    assert sum(p.numel() for p in ref.parameters()) == fam.FAMILY[name][4]
    assert not hip.load_state_dict(rs, strict=True).missing_keys


def test_resnext50_conv2_is_grouped():
    hip = create_resnet("resnext50", precision="bf16")
    widths = [getattr(hip, f"layer{i}")[0].conv2 for i in range(1, 5)]
    assert [c.groups for c in widths] == [32] * 4
    assert [tuple(c.weight.shape) for c in widths] == [(128, 4, 3, 3), (256, 8, 3, 3), (512, 16, 3, 3), (1024, 32, 3, 3)]
    wide = create_resnet("wide_resnet50", precision="bf16")
    assert [tuple(getattr(wide, f"layer{i}")[0].conv2.weight.shape) for i in range(1, 5)] == [
        (128, 128, 3, 3), (256, 256, 3, 3), (512, 512, 3, 3), (1024, 1024, 3, 3)]


def test_resnet50_module_is_unchanged():
    """The defaults of Bottleneck(groups, base_width) reproduce the resnet50 module."""
    hip = create_resnet("resnet50", precision="bf16")
    assert sum(p.numel() for p in hip.parameters()) == 23_508_032
    assert all(m.groups == 1 for m in hip.modules() if isinstance(m, torch.nn.Conv2d))
    assert tuple(hip.layer1[0].conv2.weight.shape) == (64, 64, 3, 3)


@pytest.mark.parametrize("name", ["resnext101", "resnet50_d", "resnetrs50"])
def test_names_outside_the_kernel_set_still_raise(name):
    with pytest.raises(ValueError, match="not on the MI355X training path"):
        BackboneFactory.create(name, pretrained=False)


@pytest.mark.parametrize("C,groups", [(128, 32), (256, 32), (512, 32), (1024, 32), (64, 2)])
def test_grouped_as_dense_roundtrip(C, groups):
    Cg = C // groups
    w = torch.randn(C, Cg, 3, 3, generator=torch.Generator().manual_seed(C + groups))
    dense = K.grouped_as_dense(w, groups)
    assert dense.shape == (C, C, 3, 3)
    assert torch.equal(K.dense_group_blocks(dense, groups), w)
    same = (torch.arange(C)[:, None] // Cg) == (torch.arange(C)[None, :] // Cg)
    assert bool((dense[~same] == 0).all()) and int((dense != 0).sum()) == int((w != 0).sum())
    # the dense embedding computes the grouped convolution
    x = torch.randn(1, C, 5, 4, generator=torch.Generator().manual_seed(1))
    a = torch.nn.functional.conv2d(x, w, padding=1, groups=groups)
    b = torch.nn.functional.conv2d(x, dense, padding=1)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
