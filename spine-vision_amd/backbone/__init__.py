"""HIP-backed backbones with timm module trees and state_dict keys."""

from .convnext import CONVNEXT_CFGS, ConvNeXtHip, create_convnext
from .efficientnet import (EFFNET_CFGS, EFFNETV2_CFGS, EfficientNetHip, EfficientNetV2Hip, create_efficientnet,
                           create_efficientnetv2)
from .resnet import RESNET_CFGS, ResNetHip, create_resnet
from .swin import SWIN_CFGS, SwinHip, create_swin
from .vit import VIT_CFGS, ViTHip, create_vit

__all__ = ["CONVNEXT_CFGS", "ConvNeXtHip", "create_convnext", "EFFNET_CFGS", "EFFNETV2_CFGS", "EfficientNetHip",
           "EfficientNetV2Hip", "create_efficientnet", "create_efficientnetv2", "RESNET_CFGS", "ResNetHip", "create_resnet",
           "SWIN_CFGS", "SwinHip", "create_swin", "VIT_CFGS", "ViTHip", "create_vit"]
