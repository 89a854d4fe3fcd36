"""CPU: the ConvNeXt V2 backbones exist with timm's module tree (no GPU needed to construct or to load weights), the
test reference module (tests/_convnextv2_ref.py) agrees with an independent implementation, and the GRN entry points
validate their arguments before any launch."""

import ctypes

import pytest
import torch

import _convnextv2_ref as v2ref
from oracle import weights as ow
from spine_vision_amd import inference
from spine_vision_amd import native as nv
from spine_vision_amd.backbone import create_convnext
from spine_vision_amd.training.models.backbone import BackboneFactory


@pytest.mark.parametrize("name,nf", [("convnextv2_base", 1024), ("convnextv2_large", 1536)])
def test_factory_creates_v2(name, nf):
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert dim == nf and model.num_features == nf
    assert BackboneFactory.get_feature_dim(name) == nf


@pytest.mark.parametrize("name", ["convnextv2_tiny", "convnextv2_small", "convnextv2_huge"])
def test_other_v2_sizes_still_raise(name):
    with pytest.raises(ValueError, match="not on the MI355X training path"):
        BackboneFactory.create(name, pretrained=False)


@pytest.mark.parametrize("name", ["convnextv2_base", "convnextv2_large"])
def test_state_dict_is_timms(name):
    ref = ow.fill_module(v2ref.create(name))
    hip = create_convnext(name, precision="fp32")
    rs, hs = ref.state_dict(), hip.state_dict()
    assert set(rs) == set(hs), set(rs) ^ set(hs)
    assert all(rs[k].shape == hs[k].shape for k in rs)
    assert not [k for k in hs if k.endswith(".gamma") or "ls_ones" in k]
    n_blocks = sum(hip.depths)
    assert sum(k.endswith(".mlp.grn.weight") for k in hs) == n_blocks
    assert sum(k.endswith(".mlp.grn.bias") for k in hs) == n_blocks
    for st, c in zip(hip.stages, hip.dims):  # [4C], zeros at init like timm
        g = st.blocks[0].mlp.grn
        assert tuple(g.weight.shape) == tuple(g.bias.shape) == (4 * c,)
        assert not g.weight.any() and not g.bias.any()
    # strict load both ways
    hip.load_state_dict(rs, strict=True)
    assert all(torch.equal(hip.state_dict()[k], rs[k]) for k in rs)
    ref2 = v2ref.create(name)
    ref2.load_state_dict(hip.state_dict(), strict=True)
    assert all(torch.equal(ref2.state_dict()[k], rs[k]) for k in rs)


def test_v1_keeps_gamma():
    hip = create_convnext("convnext_base", precision="fp32")
    assert "stages.0.blocks.0.gamma" in hip.state_dict()
    assert not [k for k in hip.state_dict() if ".grn." in k]


def test_inference_variant_constructs():
    from spine_vision_amd.training.models.generic import CoordinateRegressor

    name = inference._backbone_name("v2_base")
    assert name == "convnextv2_base"
    model = CoordinateRegressor(backbone=name, pretrained=False, num_levels=5)
    assert model.backbone.use_grn and model.backbone.num_features == 1024


def test_reference_module_matches_hf_convnextv2():
    """tests/_convnextv2_ref.py against HF transformers' ConvNextV2Model (an independent implementation of the
    architecture) on the same generated weights, 2 x 64 x 64: max-abs <= 1e-5 x max|features|."""
    tr = pytest.importorskip("transformers")
    ref = ow.fill_module(v2ref.create("convnextv2_base")).eval()
    cfg = tr.ConvNextV2Config(depths=[3, 3, 27, 3], hidden_sizes=[128, 256, 512, 1024], layer_norm_eps=1e-6)
    hf = tr.ConvNextV2Model(cfg).eval()
    sd = {}
    for k, v in ref.state_dict().items():
        k2 = k.replace("head.norm.", "layernorm.")
        k2 = k2.replace("stem.0.", "embeddings.patch_embeddings.").replace("stem.1.", "embeddings.layernorm.")
        k2 = k2.replace("stages.", "encoder.stages.").replace(".downsample.0.", ".downsampling_layer.0.")
        k2 = k2.replace(".downsample.1.", ".downsampling_layer.1.").replace(".blocks.", ".layers.")
        k2 = k2.replace(".conv_dw.", ".dwconv.").replace(".norm.", ".layernorm.").replace(".mlp.fc1.", ".pwconv1.")
        k2 = k2.replace(".mlp.fc2.", ".pwconv2.")
        if ".mlp.grn." in k2:
            k2, v = k2.replace(".mlp.grn.", ".grn."), v.reshape(1, 1, 1, -1)
        sd[k2] = v
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert not missing, missing
    img, _, _ = ow.localization_batch(2, 64, 64)
    with torch.no_grad():
        a = ref(img)
        b = hf(img).pooler_output
    err, scale = float((a - b).abs().max()), float(a.abs().max())
    print(f"reference V2-base vs HF ConvNextV2Model: max-abs {err:.2e} on scale {scale:.2f}")
    assert err <= 1e-5 * scale


_P = ctypes.c_void_p(1 << 20)  # 16-byte aligned, never dereferenced: validation fails first


def _err(L):
    return L.sv_last_error_string().decode()


def test_grn_entry_points_validate_arguments():
    """A null pointer and n % 8 != 0 are refused with a message before anything is launched (no GPU here)."""
    L = nv.lib()
    walkers = {
        "sv_grn_stats": lambda a, n: L.sv_grn_stats(a, nv.SV_BF16, _P, 2, 36, n, None),
        "sv_grn_apply": lambda a, n: L.sv_grn_apply(a, nv.SV_BF16, _P, _P, _P, 2, 36, n, None),
        "sv_grn_bwd_stats": lambda a, n: L.sv_grn_bwd_stats(a, _P, nv.SV_BF16, _P, _P, 2, 36, n, None),
        "sv_grn_bwd_apply": lambda a, n: L.sv_grn_bwd_apply(a, _P, _P, nv.SV_BF16, _P, _P, _P, 2, 36, n, None),
    }
    for name, fn in walkers.items():
        assert fn(None, 512) == 1, name
        assert name in _err(L) and "null" in _err(L)
        assert fn(_P, 516) == 1, name
        assert name in _err(L) and "multiple of 8" in _err(L)
        assert fn(ctypes.c_void_p((1 << 20) + 8), 512) == 1, name
        assert "aligned" in _err(L)
    assert L.sv_grn_finish(None, 1, _P, _P, _P, _P, _P, 2, 512, 1e-6, None) == 1
    assert "sv_grn_finish" in _err(L) and "null" in _err(L)
    assert L.sv_grn_bwd_finish(_P, _P, 1, _P, _P, _P, _P, _P, None, _P, 1, 2, 512, None) == 1
    assert "sv_grn_bwd_finish" in _err(L) and "null" in _err(L)
    assert L.sv_grn_stats(_P, 7, _P, 2, 36, 512, None) == 1
    assert "dtype" in _err(L)


def test_grn_nparts_and_wrapper_checks():
    assert nv.value("sv_grn_nparts", 36, 512) == 2
    assert nv.value("sv_grn_nparts", 1024, 512) == 16
    assert nv.value("sv_grn_nparts", 4, 6144) == 1
    from spine_vision_amd import kernels as K

    with pytest.raises(ValueError, match="device tensors"):  # no CPU fall-back
        K.grn_stats(torch.zeros(8, 16), 2)
    with pytest.raises(ValueError, match="multiple of 8"):
        K.grn_stats(torch.zeros(8, 12), 2)
    with pytest.raises(ValueError, match="dividing the rows"):
        K.grn_stats(torch.zeros(9, 16), 2)
