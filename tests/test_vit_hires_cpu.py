"""CPU: ViT / DeiT-III at image sizes other than 224 -- the argument validation of the streaming attention entry
points (no launch is reached), the ``img_size`` contract of the constructor, the factory and the models (also through
env SV_VIT_IMG_SIZE), loading weights trained at another size (``pos_embed`` resampled as timm does) and the
inference loader's choice of the image size from the checkpoint."""
import math

import pytest
import torch
import torch.nn.functional as F

import _vit_ref as ref
from spine_vision_amd import kernels as K
from spine_vision_amd import native as nv
from spine_vision_amd.backbone import create_vit
from spine_vision_amd.backbone.vit import resample_abs_pos_embed
from spine_vision_amd.training.models.backbone import BackboneFactory


def test_stream_entry_points_validate_before_launch():
    """Null pointers, N = 0, img_rows < N, a misaligned pointer and scale 0 are invalid (1); N = 2049 and a head
    dimension other than 64 are unsupported (2); the pointers are never dereferenced (there is no GPU here)."""
    L = nv.lib()
    p = 1 << 20
    fwd = lambda *a: L.sv_attn_stream_fwd(*a, None)  # noqa: E731
    bwd = lambda *a: L.sv_attn_stream_bwd(*a, None)  # noqa: E731
    for i in range(3):
        args = [p] * 3
        args[i] = None
        assert fwd(*args, 1, 5, 0, 1, 64, 0.125) == 1 and "null" in L.sv_last_error_string().decode()
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert bwd(*args, 1, 5, 0, 1, 64, 0.125) == 1 and "null" in L.sv_last_error_string().decode()
    for f, ptrs in ((fwd, [p] * 3), (bwd, [p] * 6)):
        assert f(*ptrs, 1, 0, 0, 1, 64, 0.125) == 1  # N = 0
        assert f(*ptrs, 1, 2049, 0, 1, 64, 0.125) == 2 and "at most 2048" in L.sv_last_error_string().decode()
        assert f(*ptrs, 1, 5, 0, 1, 32, 0.125) == 2 and "head dimension" in L.sv_last_error_string().decode()
        assert f(*ptrs, 1, 5, 4, 1, 64, 0.125) == 1  # img_rows < N
        assert f(*ptrs, 1, 5, 0, 1, 64, 0.0) == 1  # scale
        assert f(p + 2, *ptrs[1:], 1, 5, 0, 1, 64, 0.125) == 1 and "aligned" in L.sv_last_error_string().decode()
    assert K.ATTN_STREAM_MAX_N == 2048 and K.ATTN_MAX_N == 256


def test_create_vit_at_384_matches_reference_state_dict():
    model = create_vit("vit_tiny", img_size=384)
    r = ref.create("vit_tiny", 384)
    sd, rsd = model.state_dict(), r.state_dict()
    assert list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    assert model.img_size == 384 and model.num_tokens == 577 and model.rows_per_img == 584
    assert create_vit("deit_small", img_size=(512, 512)).num_tokens == 1025


@pytest.mark.parametrize("size", [(384, 256), 100, 0, 736], ids=["384x256", "100", "0", "736"])
def test_unsupported_image_sizes_raise(size):
    """A non-square pair, a size that is no positive multiple of 16, and 736 px (46 x 46 + 1 = 2117 tokens > 2048)."""
    with pytest.raises(ValueError):
        create_vit("vit_tiny", img_size=size)
    with pytest.raises(ValueError):
        BackboneFactory.create("vit_tiny", pretrained=False, img_size=size)


def test_largest_supported_size_constructs():
    assert create_vit("vit_tiny", img_size=720).num_tokens == 2026  # 45 x 45 + 1 <= 2048


def test_env_sets_the_default_image_size(monkeypatch):
    from spine_vision_amd.training import Classifier, CoordinateRegressor

    assert BackboneFactory.create("vit_tiny", pretrained=False)[0].img_size == 224
    monkeypatch.setenv("SV_VIT_IMG_SIZE", "384")
    assert BackboneFactory.create("vit_tiny", pretrained=False)[0].img_size == 384
    assert Classifier(backbone="vit_tiny", pretrained=False).backbone.img_size == 384
    assert CoordinateRegressor(backbone="deit_small", pretrained=False).backbone.img_size == 384
    # an explicit size wins; the other families ignore both
    assert CoordinateRegressor(backbone="vit_tiny", pretrained=False, img_size=272).backbone.img_size == 272
    assert Classifier(backbone="vit_tiny", pretrained=False, img_size=(256, 256)).backbone.img_size == 256
    m, _ = BackboneFactory.create("resnet18", pretrained=False, img_size=(384, 256))
    assert not hasattr(m, "img_size")


def _resampled(pe, new, prefix):
    """timm's resample_abs_pos_embed, restated: the grid part as a [1, C, g, g] image, bicubic with antialias"""
    head, grid = pe[:, :prefix], pe[:, prefix:]
    g = math.isqrt(grid.shape[1])
    img = grid.reshape(1, g, g, -1).permute(0, 3, 1, 2).float()
    img = F.interpolate(img, size=(new, new), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([head, img.permute(0, 2, 3, 1).reshape(1, new * new, -1).to(pe.dtype)], dim=1)


@pytest.mark.parametrize("name", ["vit_tiny", "deit_small"])
def test_loading_224_weights_at_384_resamples_pos_embed(name):
    from spine_vision_amd.training import CoordinateRegressor

    torch.manual_seed(3)
    src = create_vit(name, img_size=224)
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn_like(p))
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    prefix = 0 if src.no_embed_class else 1
    want = _resampled(sd["pos_embed"], 24, prefix)
    assert tuple(want.shape) == (1, 576 + prefix, src.dim)
    assert torch.equal(resample_abs_pos_embed(sd["pos_embed"], (24, 24), prefix), want)
    # bare
    dst = create_vit(name, img_size=384)
    dst.load_state_dict(sd, strict=True)
    got = dst.state_dict()
    assert torch.equal(got["pos_embed"], want)
    assert all(torch.equal(got[k], v) for k, v in sd.items() if k != "pos_embed")
    assert tuple(sd["pos_embed"].shape) == (1, 196 + prefix, src.dim), "the caller's tensor was modified"
    # under the `backbone.` prefix of a model
    model = CoordinateRegressor(backbone=name, pretrained=False, img_size=384)
    msd = model.state_dict()
    msd.update({"backbone." + k: v for k, v in sd.items()})
    model.load_state_dict(msd, strict=True)
    got = model.backbone.state_dict()
    assert torch.equal(got["pos_embed"], want)
    assert all(torch.equal(got[k], v) for k, v in sd.items() if k != "pos_embed")
    # the prefix token row is copied, not interpolated
    if prefix:
        assert torch.equal(got["pos_embed"][:, 0], sd["pos_embed"][:, 0])


def test_other_pos_embed_mismatches_stay_errors():
    dst = create_vit("vit_tiny", img_size=384)
    sd = create_vit("vit_tiny", img_size=224).state_dict()
    bad = dict(sd)
    bad["pos_embed"] = torch.zeros(1, 1 + 14 * 13, 192)  # not a square grid
    with pytest.raises(RuntimeError, match="pos_embed"):
        dst.load_state_dict(bad)
    bad["pos_embed"] = torch.zeros(1, 197, 96)  # another width
    with pytest.raises(RuntimeError, match="pos_embed"):
        dst.load_state_dict(bad)
    bad = dict(sd)
    bad["cls_token"] = torch.zeros(1, 2, 192)
    with pytest.raises(RuntimeError, match="cls_token"):
        dst.load_state_dict(bad)


def test_load_localization_model_rebuilds_the_checkpoints_size(tmp_path):
    from spine_vision_amd.inference import load_localization_model
    from spine_vision_amd.training import CoordinateRegressor

    m = CoordinateRegressor("vit_tiny", pretrained=False, img_size=272)
    path = tmp_path / "loc.pt"
    torch.save({"model_state_dict": m.state_dict()}, path)
    got = load_localization_model(path, "vit_tiny", "cpu")
    assert got.backbone.img_size == 272 and got.backbone.num_tokens == 290 and not got.training
    a, b = m.state_dict(), got.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
