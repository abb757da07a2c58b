"""Twin of the QuickGELU CLIP towers (`vit_*_clip_quickgelu_*`) for their tests: the CLIP twin of tests/vit_options_reference.py with
each block's Mlp swapped for one that applies x * sigmoid(1.702 x) between fc1 and fc2 — what timm calls act_layer="quick_gelu",
restated from memory of timm (timm is not installed, so parity with it is unpinned).  The activation has no parameter: keys, shapes and
counts are those of the matching `vit_*_clip_*` member (GELU_TWIN)."""
import torch
from torch import nn

import vit_options_reference as vor
from oracle.torch_models import Mlp

_CLIP = dict(pre_norm=True, ln_eps=1e-5)
QUICK_GELU_A = 1.702

# name: (img, patch, dim, depth, heads, options, backbone parameters or None) — the row format of vit_options_reference.MEMBERS
MEMBERS = {
    "vit_base_patch32_clip_quickgelu_224": (224, 32, 768, 12, 12, _CLIP, 87_456_000),
    "vit_base_patch16_clip_quickgelu_224": (224, 16, 768, 12, 12, _CLIP, 85_799_424),
    "vit_large_patch14_clip_quickgelu_224": (224, 14, 1024, 24, 16, _CLIP, 303_179_776),
    "vit_large_patch14_clip_quickgelu_336": (336, 14, 1024, 24, 16, _CLIP, 303_507_456),
    "vit_clip_quickgelu_test": (64, 16, 128, 2, 2, _CLIP, None),
    "vit_clip_quickgelu_f8_test": (64, 16, 256, 2, 4, _CLIP, None),
}
# the member with the same parameters and exact-erf GELU
GELU_TWIN = {
    "vit_base_patch32_clip_quickgelu_224": "vit_base_patch32_clip_224",
    "vit_base_patch16_clip_quickgelu_224": "vit_base_patch16_clip_224",
    "vit_large_patch14_clip_quickgelu_224": "vit_large_patch14_clip_224",
    "vit_large_patch14_clip_quickgelu_336": "vit_large_patch14_clip_336",
    "vit_clip_quickgelu_test": "vit_clip_test",
}


def quick_gelu(x):
    return x * torch.sigmoid(QUICK_GELU_A * x)


def quick_gelu_grad(x):
    s = torch.sigmoid(QUICK_GELU_A * x)
    return s * (1 + QUICK_GELU_A * x * (1 - s))


class QuickGELU(nn.Module):
    def forward(self, x):
        return quick_gelu(x)


class QuickGELUMlp(Mlp):
    """oracle.torch_models.Mlp (fc1 -> act -> drop1 -> fc2 -> drop2, same keys) with QuickGELU as its activation."""

    def __init__(self, dim: int, hidden: int):
        super().__init__(dim, hidden)
        self.act = QuickGELU()


class VisionTransformer(vor.VisionTransformer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        for blk in self.blocks:
            fc1 = blk.mlp.fc1
            blk.mlp = QuickGELUMlp(fc1.in_features, fc1.out_features)
            for lin in (blk.mlp.fc1, blk.mlp.fc2):                  # the parent's initialisation of every Linear
                nn.init.trunc_normal_(lin.weight, std=0.02)
                nn.init.zeros_(lin.bias)


class ViTClassifier(vor.ViTClassifier):
    """vit_options_reference.ViTClassifier (the reference's SingletaskClassifier wrapper) around the QuickGELU twin; a name of
    vit_options_reference.MEMBERS still builds that module's own twin, so a test can put both side by side."""

    def __init__(self, name: str, n_classes: int):
        if name not in MEMBERS:
            super().__init__(name, n_classes)
            return
        nn.Module.__init__(self)
        img, patch, dim, depth, heads, opts, _ = MEMBERS[name]
        self.emb_model = VisionTransformer(img, patch, dim, depth, heads, **opts)
        self.emb_size = dim
        self.classifier = nn.Sequential(nn.Dropout(0.0), nn.Linear(dim, n_classes))
        nn.init.kaiming_normal_(self.classifier[1].weight, nonlinearity="relu")
        nn.init.zeros_(self.classifier[1].bias)
