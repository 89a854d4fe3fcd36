"""CPU: the ViT / DeiT-III names of the backbone factory (module tree, state_dict, parameter counts, image-size
contract) and the argument validation of the attention entry points (no launch is reached)."""
import ctypes

import pytest
import torch

import _vit_ref as ref
from spine_vision_amd import native as nv
from spine_vision_amd.training.models.backbone import BACKBONES, NATIVE, BackboneFactory

NAMES = list(ref.CFGS)


@pytest.mark.parametrize("name", NAMES)
def test_factory_creates_vit(name, monkeypatch):
    assert name in NATIVE and name in BACKBONES
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert dim == model.num_features == ref.FEATURE_DIMS[name]
    # the table answers without constructing
    monkeypatch.setattr(BackboneFactory, "_feature_dims", {})
    monkeypatch.setattr(BackboneFactory, "create", classmethod(lambda *a, **k: pytest.fail("constructed")))
    assert BackboneFactory.get_feature_dim(name) == ref.FEATURE_DIMS[name]


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_and_parameter_count_match_reference(name):
    model, _ = BackboneFactory.create(name, pretrained=False)
    r = ref.create(name)
    sd, rsd = model.state_dict(), r.state_dict()
    assert list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    model.load_state_dict(rsd, strict=True)
    r.load_state_dict(sd, strict=True)
    n = sum(p.numel() for p in model.parameters())
    assert n == sum(p.numel() for p in r.parameters()) == ref.CFGS[name][5]
    has_ls = any(k.endswith("ls1.gamma") for k in sd)
    assert has_ls == (ref.CFGS[name][3] is not None)
    assert tuple(sd["pos_embed"].shape) == (1, 196 if ref.CFGS[name][4] else 197, ref.CFGS[name][0])


def test_init_follows_the_specification():
    model, _ = BackboneFactory.create("deit_small", pretrained=False)
    blk = model.blocks[0]
    assert float(model.cls_token.abs().max()) < 1e-4 and float(model.cls_token.abs().max()) > 0
    assert 0.015 < float(model.pos_embed.std()) < 0.025 and float(model.pos_embed.abs().max()) <= 2.0
    assert 0.015 < float(blk.attn.qkv.weight.std()) < 0.025
    assert all(float(m.bias.abs().max()) == 0 for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2))
    assert torch.equal(blk.ls1.gamma, torch.full((384,), 1e-6)) and torch.equal(blk.ls2.gamma, torch.full((384,), 1e-6))


@pytest.mark.parametrize("name", ["swin_tiny", "efficientnet_b0", "mobilenetv3_small"])
def test_other_families_still_raise(name):
    with pytest.raises(ValueError, match="not on the MI355X training path"):
        BackboneFactory.create(name, pretrained=False)


def test_image_size_is_strict():
    model, _ = BackboneFactory.create("vit_tiny", pretrained=False)
    for x in (torch.zeros(1, 3, 256, 256), torch.zeros(1, 256, 256, dtype=torch.uint8),
              torch.zeros(1, 256, 256, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="ClassificationConfig.output_size.*LocalizationConfig.image_size"):
            model(x)
    with pytest.raises(ValueError, match="head dimension"):
        from spine_vision_amd.backbone import ViTHip

        ViTHip(dim=192, heads=4)


def test_attention_entry_points_validate_before_launch():
    """Null pointers, N = 0, N = 257 (unsupported) and a head dimension other than 64 are refused by argument
    validation; the pointers are never dereferenced (there is no GPU here)."""
    L = nv.lib()
    p = 1 << 20
    fwd = lambda *a: L.sv_attn_fwd(*a, None)  # noqa: E731
    bwd = lambda *a: L.sv_attn_bwd(*a, None)  # noqa: E731
    assert fwd(None, p, p, 1, 5, 0, 1, 64, 0.125) == 1 and "null" in L.sv_last_error_string().decode()
    assert fwd(p, None, p, 1, 5, 0, 1, 64, 0.125) == 1
    assert fwd(p, p, None, 1, 5, 0, 1, 64, 0.125) == 1
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert bwd(*args, 1, 5, 0, 1, 64, 0.125) == 1 and "null" in L.sv_last_error_string().decode()
    for f, ptrs in ((fwd, [p] * 3), (bwd, [p] * 5)):
        assert f(*ptrs, 1, 0, 0, 1, 64, 0.125) == 1  # N = 0
        assert f(*ptrs, 1, 257, 0, 1, 64, 0.125) == 2 and "at most 256" in L.sv_last_error_string().decode()
        assert f(*ptrs, 1, 5, 0, 1, 32, 0.125) == 2 and "head dimension" in L.sv_last_error_string().decode()
        assert f(*ptrs, 1, 5, 4, 1, 64, 0.125) == 1  # img_rows < N
        assert f(*ptrs, 1, 5, 0, 1, 64, 0.0) == 1  # scale
        assert f(p + 2, *ptrs[1:], 1, 5, 0, 1, 64, 0.125) == 1 and "aligned" in L.sv_last_error_string().decode()
    assert L.sv_patchify16(None, 0, None, None, p, 1, 1, 224, 224, 0, 0, None) == 1
    assert L.sv_patchify16(p, 0, None, None, p, 1, 1, 100, 224, 0, 0, None) == 1  # H not a multiple of 16
    assert L.sv_patchify16(p, 2, None, None, p, 1, 1, 224, 224, 0, 0, None) == 1  # u8 needs mean / std
    assert L.sv_vit_tokens(p, p, p, None, 1, 196, 200, 192, 1, None) == 1
    assert L.sv_vit_tokens(p, p, p, p, 1, 196, 196, 192, 1, None) == 1  # no room for the class row


def test_models_and_inference_variants_construct():
    from spine_vision_amd.inference import _backbone_name
    from spine_vision_amd.training import Classifier, CoordinateRegressor

    assert _backbone_name("vit_small") == "vit_small" and _backbone_name("deit_base") == "deit_base"
    assert _backbone_name("base") == "convnext_base" and _backbone_name("v2_base") == "convnextv2_base"
    m = CoordinateRegressor(backbone=_backbone_name("vit_small"), pretrained=False, num_levels=5)
    assert m.feature_dim == 384 and type(m.backbone).__name__ == "ViTHip"
    c = Classifier(backbone="vit_tiny", pretrained=False)
    assert c.feature_dim == 192
