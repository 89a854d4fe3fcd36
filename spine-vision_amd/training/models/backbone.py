"""Backbone constructor -- drop-in for ``BackboneFactory`` (spine_vision/training/models/backbone.py:
137-225), whose ``create`` calls ``timm.create_model(BACKBONES[name], pretrained, num_classes=0)``
(backbone.py:166-170) and returns ``(module, module.num_features)``.

Here ``create`` returns the MI355X-native module (HIP kernels, timm module tree and state_dict keys)
for the backbones on the north-star path -- ConvNeXt-tiny/small/base/large and ConvNeXt V2-base/large
(localization) and the ResNet family (classification): ResNet-18/34/50/101/152, the ``resnet50_a2`` / ``_b`` /
``_c`` recipes of ResNet-50, Wide-ResNet-50/101, ResNeXt-50 (32x4d, its grouped 3x3 on csrc/gconv.hip) and
ResNet-RS-101/152 (deep stem, conv stem pool, avg-pool shortcut and squeeze-and-excitation on csrc/se.hip) -- and
the plain transformers: ViT-tiny/small/base/large (patch 16) and DeiT-III small/base (``deit_tiny`` is the
reference's alias of deit3_small), their attention on csrc/attn.hip (up to 256 tokens) and csrc/attn_stream.hip (up to 2048); these are
strict about the image size: one square ``img_size``, a multiple of 16 up to 2048 tokens (224, 256, 384, 512, ...),
given to ``create`` / ``Classifier`` / ``CoordinateRegressor`` or through env ``SV_VIT_IMG_SIZE`` (default 224) --
and Swin-small/base (patch 4, window 7, head dimension 32; shifted-window attention with its relative-position bias on
csrc/swin.hip), strict in the same way: a square ``img_size`` that is a multiple of 224 (window 7) or 256 (window 8),
from ``create`` / the models or env ``SV_SWIN_IMG_SIZE`` (default 224) -- and EfficientNetV2-S/M/L (any input size):
their 1x1 convolutions are GEMMs, the depthwise 3x3, BatchNorm + SiLU and the gating squeeze-and-excitation run on
csrc/mbconv.hip, and the dense 3x3 convolutions of the first stages go through the ResNet convolution path with the
channel stride of the tensors they touch padded to a power of two.  ``swin_tiny`` is built by
``backbone.swin.create_swin`` but still raises here: an existing test pins that, and lifting the gate is adding the
name to ``NATIVE``; ``resnetrs50`` and ``resnet50_d`` are built by ``backbone.resnet.create_resnet`` and raise here for
the same reason, and so do ``efficientnet_b0`` .. ``efficientnet_b4``, built by ``backbone.efficientnet.create_efficientnet``
(5x5 depthwise on csrc/dwconv5.hip, widths 16 / 40 / 112 stored with zero-padded channel strides): the dispatch arm below
is in place, and lifting the gate is adding the five names to ``NATIVE`` and ``_FEATURE_DIMS``.  Every other name of the
reference registry is recognised (``list_backbones`` returns the reference's full list) but raises: those (MobileNetV3
-- hard-swish --; and ConvNeXt-xlarge, the other ConvNeXt V2 sizes and ``resnext101``) are outside this build's scope.
``pretrained=True`` cannot download weights offline; pass ``pretrained=False`` or load a timm
state_dict with ``load_state_dict`` (keys match).
"""

from __future__ import annotations

import torch.nn as nn

# reference name -> timm model id (backbone.py:25-85), grouped by family
_FAMILIES: dict[str, dict[str, str]] = {
    "resnet": {
        "resnet18": "resnet18.a1_in1k", "resnet34": "resnet34.a1_in1k", "resnet50": "resnet50.a1_in1k",
        "resnet101": "resnet101.a1_in1k", "resnet152": "resnet152.a1_in1k", "resnet50_a2": "resnet50.a2_in1k",
        "resnet50_b": "resnet50.b1k_in1k", "resnet50_c": "resnet50.c1_in1k", "resnet50_d": "resnet50.d_in1k",
        "resnext50": "resnext50_32x4d.a1h_in1k", "resnext101": "resnext101_32x8d.fb_wsl_ig1b_ft_in1k",
        "wide_resnet50": "wide_resnet50_2.racm_in1k", "wide_resnet101": "wide_resnet101_2.tv2_in1k",
        "resnetrs50": "resnetrs50.tf_in1k", "resnetrs101": "resnetrs101.tf_in1k",
        "resnetrs152": "resnetrs152.tf_in1k",
    },
    "convnext": {
        f"convnext_{s}": f"convnext_{s}.fb_in22k_ft_in1k" for s in ("tiny", "small", "base", "large", "xlarge")
    },
    "convnextv2": {
        "convnextv2_tiny": "convnextv2_tiny.fcmae_ft_in22k_in1k", "convnextv2_small": "convnextv2_small.fcmae",
        "convnextv2_base": "convnextv2_base.fcmae_ft_in22k_in1k",
        "convnextv2_large": "convnextv2_large.fcmae_ft_in22k_in1k",
        "convnextv2_huge": "convnextv2_huge.fcmae_ft_in22k_in1k",
    },
    "vit": {
        "vit_tiny": "vit_tiny_patch16_224.augreg_in21k_ft_in1k", "vit_small": "vit_small_patch16_224.augreg_in21k_ft_in1k",
        "vit_base": "vit_base_patch16_224.augreg2_in21k_ft_in1k", "vit_large": "vit_large_patch16_224.augreg_in21k_ft_in1k",
        "deit_tiny": "deit3_small_patch16_224.fb_in22k_ft_in1k", "deit_small": "deit3_small_patch16_224.fb_in22k_ft_in1k",
        "deit_base": "deit3_base_patch16_224.fb_in22k_ft_in1k",
        "swin_tiny": "swin_tiny_patch4_window7_224.ms_in22k_ft_in1k",
        "swin_small": "swin_small_patch4_window7_224.ms_in22k_ft_in1k",
        "swin_base": "swin_base_patch4_window7_224.ms_in22k_ft_in1k",
    },
    "efficient": {
        **{f"efficientnet_b{i}": f"efficientnet_b{i}.ra_in1k" for i in range(5)},
        **{f"efficientnetv2_{s}": f"efficientnetv2_{s}.ra_in1k" for s in ("s", "m", "l")},
        "mobilenetv3_small": "mobilenetv3_small_100.lamb_in1k", "mobilenetv3_large": "mobilenetv3_large_100.ra_in1k",
    },
}
BACKBONES: dict[str, str] = {k: v for fam in _FAMILIES.values() for k, v in fam.items()}

# names built natively on MI355X (the north-star backbones)
NATIVE = ("convnext_tiny", "convnext_small", "convnext_base", "convnext_large", "convnextv2_base", "convnextv2_large",
          "resnet18", "resnet50", "resnet34", "resnet101", "resnet152", "resnet50_a2", "resnet50_b", "resnet50_c",
          "wide_resnet50", "wide_resnet101", "resnext50", "resnetrs101", "resnetrs152",
          "vit_tiny", "vit_small", "vit_base", "vit_large", "deit_tiny", "deit_small", "deit_base",
          "swin_small", "swin_base", "efficientnetv2_s", "efficientnetv2_m", "efficientnetv2_l")
_FEATURE_DIMS = {"convnext_tiny": 768, "convnext_small": 768, "convnext_base": 1024, "convnext_large": 1536, "convnextv2_base": 1024, "convnextv2_large": 1536,
                 "resnet18": 512, "resnet50": 2048, "resnet34": 512, "resnet101": 2048, "resnet152": 2048,
                 "resnet50_a2": 2048, "resnet50_b": 2048, "resnet50_c": 2048, "wide_resnet50": 2048,
                 "wide_resnet101": 2048, "resnext50": 2048, "resnetrs101": 2048, "resnetrs152": 2048,
                 "vit_tiny": 192, "vit_small": 384, "vit_base": 768, "vit_large": 1024, "deit_tiny": 384,
                 "deit_small": 384, "deit_base": 768, "swin_small": 768, "swin_base": 1024,
                 "efficientnetv2_s": 1280, "efficientnetv2_m": 1280, "efficientnetv2_l": 1280}


class BackboneFactory:
    _feature_dims: dict[str, int] = {}
    precision: str = "bf16"  # default compute precision of created backbones ("bf16" | "fp32")

    @classmethod
    def create(cls, name: str, pretrained: bool = True, precision: str | None = None,
               img_size=None) -> tuple[nn.Module, int]:
        """``img_size`` (an int or a square pair) sizes a ViT / DeiT-III or Swin backbone, which are strict about their
        input size (None: env SV_VIT_IMG_SIZE / SV_SWIN_IMG_SIZE, else 224); every other family takes any size and
        ignores it."""
        if name not in BACKBONES:
            raise ValueError(f"Unknown backbone: {name}. Available: {', '.join(sorted(BACKBONES))}")
        if name not in NATIVE:
            raise ValueError(
                f"Backbone {name!r} is not on the MI355X training path (supported: {', '.join(NATIVE)})"
            )
        prec = precision or cls.precision
        if name.startswith("convnext"):
            from ...backbone.convnext import create_convnext

            model = create_convnext(name, precision=prec)
        elif name.startswith(("vit_", "deit_")):
            from ...backbone.vit import create_vit

            model = create_vit(name, precision=prec, img_size=img_size)
        elif name.startswith("swin_"):
            from ...backbone.swin import create_swin

            model = create_swin(name, precision=prec, img_size=img_size)
        elif name.startswith("efficientnetv2_"):
            from ...backbone.efficientnet import create_efficientnetv2

            model = create_efficientnetv2(name, precision=prec)
        elif name.startswith("efficientnet_b"):
            from ...backbone.efficientnet import create_efficientnet

            model = create_efficientnet(name, precision=prec)
        else:
            from ...backbone.resnet import create_resnet

            model = create_resnet(name, precision=prec)
        if pretrained:
            import warnings

            warnings.warn(
                f"pretrained weights for {BACKBONES[name]} cannot be downloaded offline; using random init "
                "(load a timm state_dict with load_state_dict to use pretrained weights)",
                stacklevel=2,
            )
        cls._feature_dims[name] = model.num_features
        return model, model.num_features

    @classmethod
    def get_feature_dim(cls, name: str) -> int:
        if name in cls._feature_dims:
            return cls._feature_dims[name]
        if name in _FEATURE_DIMS:
            return _FEATURE_DIMS[name]
        return cls.create(name, pretrained=False)[1]

    @classmethod
    def list_backbones(cls, family: str | None = None) -> list[str]:
        names = sorted(BACKBONES)
        return names if family is None else [n for n in names if n.startswith(family.lower())]

    @classmethod
    def get_timm_name(cls, name: str) -> str:
        if name not in BACKBONES:
            raise ValueError(f"Unknown backbone: {name}")
        return BACKBONES[name]
