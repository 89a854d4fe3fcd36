"""Swin backbones without a GPU: factory, state_dict / parameter counts against tests/_swin_ref.py, the load hooks,
image-size strictness, init statistics, the stochastic-depth schedule, argument validation of the new entry points,
and the reference's own roll + partition + mask against the index formula the kernels implement."""
import pytest
import torch

import _swin_ref as ref
from spine_vision_amd import native as nv
from spine_vision_amd.backbone.swin import SwinHip, create_swin
from spine_vision_amd.training.models.backbone import BACKBONES, NATIVE, BackboneFactory


@pytest.mark.parametrize("name", ["swin_small", "swin_base"])
def test_factory_creates_swin(name, monkeypatch):
    assert name in NATIVE and name in BACKBONES
    model, dim = BackboneFactory.create(name, pretrained=False)
    assert isinstance(model, SwinHip) and dim == model.num_features == ref.FEATURE_DIMS[name]
    assert model.graph_safe is False and model.drop_path_rate == 0.1
    monkeypatch.setattr(BackboneFactory, "_feature_dims", {})
    monkeypatch.setattr(BackboneFactory, "create", classmethod(lambda *a, **k: pytest.fail("constructed")))
    assert BackboneFactory.get_feature_dim(name) == ref.FEATURE_DIMS[name]


def test_swin_tiny_is_built_by_the_module_but_gated_in_the_factory():
    assert "swin_tiny" not in NATIVE
    with pytest.raises(ValueError, match="not on the MI355X training path"):
        BackboneFactory.create("swin_tiny", pretrained=False)
    assert create_swin("swin_tiny").num_features == 768


@pytest.mark.parametrize("name,size", [("swin_tiny", 224), ("swin_small", 224), ("swin_base", 224), ("swin_tiny", 256),
                                       ("swin_base", 256)])
def test_state_dict_and_parameter_count_match_reference(name, size):
    model, r = create_swin(name, img_size=size), ref.create(name, img_size=size)
    sd, rsd = model.state_dict(), r.state_dict()
    assert list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    assert not any(k.endswith(("relative_position_index", "attn_mask")) for k in sd)
    model.load_state_dict(rsd, strict=True)
    r.load_state_dict(sd, strict=True)
    n = sum(p.numel() for p in model.parameters())
    assert n == sum(p.numel() for p in r.parameters())
    w = 7 if size == 224 else 8
    assert model.window == w and tuple(sd["layers.0.blocks.0.attn.relative_position_bias_table"].shape) == \
        ((2 * w - 1) ** 2, ref.CFGS[name][2][0])
    if size == 224:
        assert n == ref.CFGS[name][3]
    assert "layers.0.downsample.norm.weight" not in sd and "layers.1.downsample.reduction.bias" not in sd
    assert tuple(sd["layers.1.downsample.reduction.weight"].shape) == (2 * ref.CFGS[name][0], 4 * ref.CFGS[name][0])
    # shifts as timm resolves them: odd blocks shift by w // 2, except where the grid is the window
    blocks = model.all_blocks()
    assert [b.shift for b in blocks[:4]] == [0, w // 2, 0, w // 2] and [b.shift for b in blocks[-2:]] == [0, 0]
    assert [(b.window, b.shift) for b in blocks] == [(b.w, b.shift) for b in r.all_blocks()]


def test_stale_buffers_in_a_checkpoint_are_dropped():
    model = create_swin("swin_tiny")
    sd = dict(model.state_dict())
    sd["layers.0.blocks.1.attn_mask"] = torch.zeros(64, 49, 49)
    for s, st in enumerate(model.layers):
        for j in range(len(st.blocks)):
            sd[f"layers.{s}.blocks.{j}.attn.relative_position_index"] = ref.relative_position_index(7)
    model.load_state_dict(sd, strict=True)


def test_a_window7_table_does_not_load_into_a_window8_model():
    sd = create_swin("swin_tiny", img_size=224).state_dict()
    with pytest.raises(ValueError, match="window 8.*resampling"):
        create_swin("swin_tiny", img_size=256).load_state_dict(sd)


def test_image_size_is_strict(monkeypatch):
    for size, w in ((224, 7), (448, 7), (256, 8), (512, 8)):
        assert create_swin("swin_tiny", img_size=size, depths=(1, 1, 1, 1)).window == w
    for bad in (192, 320, 0, (224, 256)):
        with pytest.raises(ValueError, match="ClassificationConfig.output_size.*LocalizationConfig.image_size"):
            create_swin("swin_tiny", img_size=bad)
    model = create_swin("swin_tiny", depths=(1, 1, 1, 1))
    for x in (torch.zeros(1, 3, 256, 256), torch.zeros(1, 256, 256, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="ClassificationConfig.output_size.*LocalizationConfig.image_size"):
            model(x)
    monkeypatch.setenv("SV_SWIN_IMG_SIZE", "256")
    assert create_swin("swin_tiny", depths=(1, 1, 1, 1)).img_size == 256
    assert BackboneFactory.create("swin_small", pretrained=False, img_size=512)[0].img_size == 512
    with pytest.raises(ValueError, match="head dimension"):
        SwinHip(dim=96, heads=(4, 6, 12, 24))


def test_init_follows_the_specification():
    model = create_swin("swin_tiny")
    blk = model.layers[2].blocks[1]
    assert 0.015 < float(blk.attn.qkv.weight.std()) < 0.025 and float(blk.attn.qkv.weight.abs().max()) <= 2.0
    assert 0.015 < float(blk.attn.relative_position_bias_table.std()) < 0.025
    assert 0.015 < float(model.layers[2].downsample.reduction.weight.std()) < 0.025
    assert all(float(m.bias.abs().max()) == 0 for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2))
    assert blk.norm1.eps == model.norm.eps == model.patch_embed.norm.eps == model.layers[1].downsample.norm.eps == 1e-5


@pytest.mark.parametrize("name", ["swin_tiny", "swin_small"])
def test_drop_path_schedule(name):
    model = create_swin(name)
    total = sum(ref.CFGS[name][1])
    want = torch.linspace(0, 0.1, total).tolist()
    blocks = model.all_blocks()
    assert [b.index for b in blocks] == list(range(total)) and [b.drop_path for b in blocks] == want
    assert blocks[0].drop_path == 0.0 and abs(blocks[-1].drop_path - 0.1) < 1e-7
    assert all(b.drop_path == 0.0 for b in create_swin(name, drop_path_rate=0.0).all_blocks())
    # inactive in eval, and for a branch that never drops
    model.eval()
    assert model._scales(blocks[-1], 0, 4, "cpu") is None
    model.train()
    assert model._scales(blocks[0], 0, 4, "cpu") is None
    s = model._scales(blocks[-1], 1, 64, "cpu")
    assert s.dtype == torch.float32 and all(v == 0.0 or abs(v - 1 / 0.9) < 1e-6 for v in s.tolist())


def test_new_entry_points_validate_before_launch():
    """Null pointers, head_dim != 32, w > 8, shift >= w, H % w != 0 and short rows_total are refused by argument
    validation; the pointers are never dereferenced (there is no GPU here)."""
    L = nv.lib()
    p = 1 << 20
    sc = 32 ** -0.5
    fwd = lambda ptrs, *a: L.sv_winattn_fwd(*ptrs, *a, None)  # noqa: E731
    bwd = lambda ptrs, *a: L.sv_winattn_bwd(*ptrs, *a, None)  # noqa: E731
    good = (2, 14, 14, 7, 3, 3, 32, sc, 392)
    for f, n in ((fwd, 4), (bwd, 7)):
        for i in range(n):
            ptrs = [p] * n
            ptrs[i] = None
            assert f(ptrs, *good) == 1 and "null" in L.sv_last_error_string().decode()
        ptrs = [p] * n
        assert f(ptrs, 2, 14, 14, 7, 3, 3, 64, sc, 392) == 2 and "head dimension" in L.sv_last_error_string().decode()
        assert f(ptrs, 2, 18, 18, 9, 3, 3, 32, sc, 648) == 2 and "at most 8" in L.sv_last_error_string().decode()
        assert f(ptrs, 2, 14, 14, 7, 7, 3, 32, sc, 392) == 1 and "shift" in L.sv_last_error_string().decode()
        assert f(ptrs, 2, 14, 14, 7, -1, 3, 32, sc, 392) == 1
        assert f(ptrs, 2, 15, 14, 7, 0, 3, 32, sc, 420) == 1 and "multiples" in L.sv_last_error_string().decode()
        assert f(ptrs, 2, 14, 15, 7, 0, 3, 32, sc, 420) == 1
        assert f(ptrs, 2, 14, 14, 7, 3, 3, 32, sc, 391) == 1 and "rows_total" in L.sv_last_error_string().decode()
        assert f(ptrs, 2, 14, 14, 7, 3, 3, 32, 0.0, 392) == 1
        assert f(ptrs, 0, 14, 14, 7, 3, 3, 32, sc, 392) == 1
        assert f([p + 2] + ptrs[1:], *good) == 1 and "aligned" in L.sv_last_error_string().decode()
    assert L.sv_winattn_bwd_nparts(32, 56, 56, 7, 3) == 341 and L.sv_winattn_bwd_nparts(1, 7, 7, 7, 24) == 1
    assert L.sv_swin_bias_expand(None, p, 7, 3, None) == 1 and L.sv_swin_bias_expand(p, p, 9, 3, None) == 1
    assert L.sv_swin_bias_grad(p, None, 4, 7, 3, 1, None) == 1 and L.sv_swin_bias_grad(p, p, 0, 7, 3, 1, None) == 1
    for f in (L.sv_patch_merge, L.sv_patch_merge_bwd):
        assert f(None, p, 0, 1, 4, 4, 96, 16, None) == 1 and f(p, None, 0, 1, 4, 4, 96, 16, None) == 1
        assert f(p, p, 0, 1, 5, 4, 96, 16, None) == 1  # odd H
        assert f(p, p, 1, 1, 4, 4, 4, 16, None) == 1  # 8-byte rows
        assert f(p, p, 7, 1, 4, 4, 96, 16, None) == 1  # dtype
    assert L.sv_patch_merge(p, p, 0, 1, 4, 4, 96, 3, None) == 1 and L.sv_patch_merge_bwd(p, p, 0, 1, 4, 4, 96, 15, None) == 1
    assert L.sv_rowscale_add(p, p, None, p, 8, 4, 2, 96, None) == 1 and L.sv_rowscale_add(p, p, p, p, 8, 4, 2, 98, None) == 1
    assert L.sv_rowscale_cast_bf16(p, p, None, 8, 4, 2, 96, None) == 1
    assert L.sv_rowscale_cast_bf16(p, p, p, 8, 0, 2, 96, None) == 1


@pytest.mark.parametrize("B,H,W,w,shift", [(1, 1, 1, 1, 0), (2, 4, 4, 2, 1), (2, 14, 14, 7, 0), (2, 14, 14, 7, 3),
                                           (1, 28, 14, 7, 3), (1, 16, 16, 8, 4), (1, 7, 7, 7, 0), (1, 24, 16, 8, 4)])
def test_reference_roll_partition_and_mask_equal_the_index_formula(B, H, W, w, shift):
    """timm's torch.roll + window_partition and its slice-built mask (as _swin_ref runs them) against: token (i, j) of
    window (wy, wx) is pixel ((wy w + i + shift) mod H, (wx w + j + shift) mod W), masked where the region labels of
    the rolled coordinates differ -- and window_reverse + roll back is the inverse."""
    ids = torch.arange(B * H * W, dtype=torch.float32).view(B, H, W, 1)
    rolled = torch.roll(ids, shifts=(-shift, -shift), dims=(1, 2)) if shift else ids
    got = ref.window_partition(rolled, w).view(-1, w * w).long()
    rows = ref.token_rows(B, H, W, w, shift)
    assert torch.equal(got, rows)
    back = ref.window_reverse(got.view(-1, w, w, 1).float(), w, H, W)
    back = torch.roll(back, shifts=(shift, shift), dims=(1, 2)) if shift else back
    assert torch.equal(back, ids)
    assert sorted(rows.view(-1).tolist()) == list(range(B * H * W))
    mask, lab = ref.attn_mask(H, W, w, shift), ref.token_regions(H, W, w, shift)
    want = (lab[:, :, None] != lab[:, None, :]).float() * -100.0
    if shift == 0:
        assert mask is None and not want.any()
    else:
        assert torch.equal(mask, want) and want.any()
    # the package's own torch arm builds the same rows and mask
    from spine_vision_amd import kernels as K

    krows, kmask = K.window_rows(B, H, W, w, shift, "cpu")
    assert torch.equal(krows.view(-1, w * w), rows)
    assert (kmask is None) if shift == 0 else torch.equal(kmask, want)
    # the dense bias index: (yi - yj + w - 1) (2w - 1) + (xi - xj + w - 1)
    idx = ref.relative_position_index(w)
    for i in (0, w * w - 1, (w * w) // 2):
        for j in (0, w * w - 1, (w * w) // 3):
            assert int(idx[i, j]) == (i // w - j // w + w - 1) * (2 * w - 1) + (i % w - j % w + w - 1)
