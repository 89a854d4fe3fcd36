"""CPU: the ConvNeXt-tiny / small backbones (stage-1 width C = 96) exist with timm's module tree -- no GPU needed to
construct them or to load weights -- and the entry points widened to C = 96 validate their arguments before any
launch."""

import ctypes

import pytest
import torch

from oracle import convnext as oc
from oracle import weights as ow
from spine_vision_amd import inference
from spine_vision_amd import native as nv
from spine_vision_amd.backbone import create_convnext
from spine_vision_amd.training.models.backbone import NATIVE, BackboneFactory


def _oracle(name):
    if name == "convnext_small":  # the oracle registry has no entry for it: tiny's dims at base's depths
        return oc.ConvNeXt((3, 3, 27, 3), (96, 192, 384, 768))
    return oc.create(name)


@pytest.mark.parametrize("name", ["convnext_tiny", "convnext_small"])
def test_factory_creates_tiny_and_small(name):
    assert name in NATIVE
    BackboneFactory._feature_dims.pop(name, None)
    assert BackboneFactory.get_feature_dim(name) == 768  # from the table: nothing has been constructed
    assert name not in BackboneFactory._feature_dims
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert dim == 768 and model.num_features == 768
    assert model.dims == (96, 192, 384, 768)


@pytest.mark.parametrize("name", ["convnext_xlarge", "convnextv2_huge"])
def test_sizes_outside_the_kernel_set_still_raise(name):
    with pytest.raises(ValueError, match="not on the MI355X training path"):
        BackboneFactory.create(name, pretrained=False)


@pytest.mark.parametrize("name,params,entries", [("convnext_tiny", 27_820_128, 180),
                                                 ("convnext_small", 49_454_688, 342)])
def test_state_dict_is_the_oracles(name, params, entries):
    ref = ow.fill_module(_oracle(name))
    hip = create_convnext(name, precision="fp32")
    rs, hs = ref.state_dict(), hip.state_dict()
    assert set(rs) == set(hs), set(rs) ^ set(hs)
    assert all(rs[k].shape == hs[k].shape for k in rs)
    assert len(hs) == entries
    assert sum(p.numel() for p in hip.parameters()) == params
    # strict load both ways
    hip.load_state_dict(rs, strict=True)
    assert all(torch.equal(hip.state_dict()[k], rs[k]) for k in rs)
    ref2 = _oracle(name)
    ref2.load_state_dict(hip.state_dict(), strict=True)
    assert all(torch.equal(ref2.state_dict()[k], rs[k]) for k in rs)


def test_inference_variants_construct():
    from spine_vision_amd.training.models.generic import CoordinateRegressor

    assert inference._backbone_name("tiny") == "convnext_tiny"
    assert inference._backbone_name("small") == "convnext_small"
    model = CoordinateRegressor(backbone="convnext_small", pretrained=False, num_levels=5)
    assert model.backbone.num_features == 768 and not model.backbone.use_grn
    assert model.backbone.depths == (3, 3, 27, 3)


def test_block_level_gates_decline_c96():
    """The choices keyed on the channel count: none of the fused forms takes C = 96."""
    from spine_vision_amd import kernels as K

    hip = create_convnext("convnext_tiny", precision="bf16")
    blk = hip.stages[0].blocks[0]
    assert blk.conv_dw.weight.shape[0] == 96
    assert 96 not in K.MLP_FUSED_C and 96 not in hip.fused_mlp_c and 96 not in K.MLP_BWD_FUSED_C
    assert not hip._fused_bwd(blk)


_P = ctypes.c_void_p(1 << 20)  # 16-byte aligned, never dereferenced: validation fails first


def _err(L):
    return L.sv_last_error_string().decode()


def test_widened_entry_points_validate_arguments():
    """A null pointer and a still-unsupported C are refused with a fresh message before anything is launched (no GPU
    here).  80 is a multiple of 16 but not of 32; 48 is half a 96."""
    L = nv.lib()
    F32 = nv.SV_F32
    calls = {
        "sv_layernorm_fwd": lambda p, C: L.sv_layernorm_fwd(p, F32, _P, _P, _P, F32, _P, _P, 64, C, 1e-6, None),
        "sv_layernorm_bwd": lambda p, C: L.sv_layernorm_bwd(p, F32, _P, F32, _P, _P, _P, _P, F32, 0, _P, _P, 64, C, None),
        "sv_stem_patchify_ln_fwd": lambda p, C: L.sv_stem_patchify_ln_fwd(p, _P, _P, _P, _P, 1e-6, _P, F32, _P, _P, 2, 8,
                                                                          8, C, None),
        "sv_stem_patchify_ln_bwd": lambda p, C: L.sv_stem_patchify_ln_bwd(p, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, 2, 8,
                                                                          8, C, None),
        "sv_downsample_ln_patch2_fwd": lambda p, C: L.sv_downsample_ln_patch2_fwd(p, _P, _P, 1e-6, _P, F32, _P, _P, 2, 8,
                                                                                  8, C, None),
        "sv_downsample_ln_patch2_bwd": lambda p, C: L.sv_downsample_ln_patch2_bwd(p, _P, _P, _P, _P, _P, None, _P, _P, 2,
                                                                                  8, 8, C, None),
        "sv_dwconv7_ln_fwd": lambda p, C: L.sv_dwconv7_ln_fwd(p, F32, _P, _P, _P, _P, 1e-6, _P, F32, _P, F32, _P, _P, 2, 8,
                                                              8, C, None),
        "sv_dwconv7_bwd_data": lambda p, C: L.sv_dwconv7_bwd_data(p, F32, _P, ctypes.c_void_p(2 << 20), None, 0, 2, 8, 8,
                                                                  C, None),
        "sv_dwconv7_bwd_weight": lambda p, C: L.sv_dwconv7_bwd_weight(p, F32, _P, F32, _P, _P, 2, 8, 8, C, None),
    }
    for name, fn in calls.items():
        assert fn(None, 96) != 0, name
        assert name in _err(L) and "null" in _err(L), (name, _err(L))
        for C in (80, 48):
            assert fn(_P, C) != 0, (name, C)
            msg = _err(L)
            assert name in msg and f"C={C}" in msg and "null" not in msg, (name, C, msg)


def test_partial_counts_follow_the_c96_grids():
    """The *_nparts queries answer for the grid the C = 96 launch uses: two rows per wave in the 32-lane-group
    downsample / stem kernels, 16 rows per wave in the LayerNorm backward, two channel groups in the depthwise
    weight gradient."""
    v = nv.value
    # downsample 2 x 8 x 6 -> 24 patches: 4 per workgroup at C = 128, 8 at C = 96
    assert v("sv_downsample_ln_patch2_bwd_nparts", 2, 8, 6, 128) == 6
    assert v("sv_downsample_ln_patch2_bwd_nparts", 2, 8, 6, 96) == 3
    # stem 2 x 32 x 24 -> 96 pixels
    assert v("sv_stem_patchify_ln_bwd_nparts", 2, 32, 24, 128) == 24
    assert v("sv_stem_patchify_ln_bwd_nparts", 2, 32, 24, 96) == 12
    # LayerNorm backward: ceil(rows / 16) row groups, 32 per workgroup
    assert v("sv_layernorm_bwd_nparts", 9001, 96) == 18
    assert v("sv_layernorm_bwd_nparts", 15, 96) == 1
    # depthwise weight gradient: the 1024-workgroup target over ceil(C / 64) channel groups
    assert v("sv_dwconv7_bwd_weight_nparts", 32, 128, 128, 64) == 1024
    assert v("sv_dwconv7_bwd_weight_nparts", 32, 128, 128, 96) == 512
    assert v("sv_dwconv7_bwd_weight_nparts", 32, 128, 128, 128) == 512
