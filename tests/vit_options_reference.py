"""Twin of the CLIP, DINOv2 and DeiT-III ViT members for their tests: timm's VisionTransformer with its pre_norm, init_values
(LayerScale) and no_embed_class options, restated from memory of timm (timm is not installed, so parity with it is unpinned), on
the Attention / Mlp of oracle.torch_models, under emb_model. with the reference's single-task head.

Order of timm's forward_features: patch_embed -> class token / position embedding (no_embed_class: the position embedding covers
the patch tokens only and the class token is prepended after it) -> pos_drop -> norm_pre -> blocks -> norm; the embedding is x[:, 0].
Block: x + ls1(attn(norm1(x))), then x + ls2(mlp(norm2(x))); proj_drop and mlp.drop2 sit inside attn / mlp, before the scale."""
import torch
from torch import nn

from oracle.torch_models import Attention, Mlp

_CLIP = dict(pre_norm=True, ln_eps=1e-5)
_DEIT3 = dict(init_values=1e-6, no_embed_class=True)

# name: (img, patch, dim, depth, heads, options, backbone parameters of the issue's table or None)
MEMBERS = {
    "vit_base_patch32_clip_224": (224, 32, 768, 12, 12, _CLIP, 87_456_000),
    "vit_base_patch16_clip_224": (224, 16, 768, 12, 12, _CLIP, 85_799_424),
    "vit_large_patch14_clip_224": (224, 14, 1024, 24, 16, _CLIP, 303_179_776),
    "vit_large_patch14_clip_336": (336, 14, 1024, 24, 16, _CLIP, 303_507_456),
    "vit_small_patch14_dinov2": (518, 14, 384, 12, 6, dict(init_values=1e-5), 22_056_192),
    "vit_base_patch14_dinov2": (518, 14, 768, 12, 12, dict(init_values=1e-5), 86_579_712),
    "vit_large_patch14_dinov2": (518, 14, 1024, 24, 16, dict(init_values=1e-5), 304_367_616),
    "deit3_small_patch16_224": (224, 16, 384, 12, 6, _DEIT3, 21_674_496),
    "deit3_base_patch16_224": (224, 16, 768, 12, 12, _DEIT3, 85_816_320),
    "deit3_large_patch16_224": (224, 16, 1024, 24, 16, _DEIT3, 303_349_760),
    "vit_clip_test": (64, 16, 128, 2, 2, _CLIP, None),
    "vit_dinov2_test": (70, 14, 128, 2, 2, dict(init_values=1e-5), None),
    "deit3_test": (64, 16, 128, 2, 2, _DEIT3, None),
    "vit_dinov2_long_test": (238, 14, 128, 1, 2, dict(init_values=1e-5), None),
}
REDUCED = [n for n in MEMBERS if n.endswith("_test")]


class PatchEmbed(nn.Module):
    def __init__(self, patch: int, in_chans: int, dim: int, bias: bool = True):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, patch, patch, bias=bias)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, ln_eps, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=ln_eps)
        self.attn = Attention(dim, heads)
        self.ls1 = LayerScale(dim, init_values) if init_values is not None else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=ln_eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim, init_values) if init_values is not None else nn.Identity()

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class VisionTransformer(nn.Module):
    def __init__(self, img=224, patch=16, dim=768, depth=12, heads=12, mlp_ratio=4.0, pre_norm=False, ln_eps=1e-6, init_values=None,
                 no_embed_class=False):
        super().__init__()
        self.num_features = dim
        self.no_embed_class = no_embed_class
        self.patch_embed = PatchEmbed(patch, 3, dim, bias=not pre_norm)
        n_tok = (img // patch) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.randn(1, n_tok if no_embed_class else n_tok + 1, dim) * 0.02)
        self.pos_drop = nn.Dropout(0.0)
        self.norm_pre = nn.LayerNorm(dim, eps=ln_eps) if pre_norm else nn.Identity()
        self.blocks = nn.Sequential(*[Block(dim, heads, mlp_ratio, ln_eps, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=ln_eps)
        self.head_drop = nn.Dropout(0.0)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.patch_embed(x)
        cls = self.cls_token.expand(x.shape[0], -1, -1)
        if self.no_embed_class:
            x = torch.cat((cls, x + self.pos_embed), dim=1)
        else:
            x = torch.cat((cls, x), dim=1) + self.pos_embed
        x = self.blocks(self.norm_pre(self.pos_drop(x)))
        return self.head_drop(self.norm(x)[:, 0])


class ViTClassifier(nn.Module):
    """The reference's SingletaskClassifier wrapper (model.py:17-159) around the twin."""

    def __init__(self, name: str, n_classes: int):
        super().__init__()
        img, patch, dim, depth, heads, opts, _ = MEMBERS[name]
        self.emb_model = VisionTransformer(img, patch, dim, depth, heads, **opts)
        self.emb_size = dim
        self.classifier = nn.Sequential(nn.Dropout(0.0), nn.Linear(dim, n_classes))
        nn.init.kaiming_normal_(self.classifier[1].weight, nonlinearity="relu")
        nn.init.zeros_(self.classifier[1].bias)

    def set_backbone_state(self, state: str):
        for p in self.emb_model.parameters():
            p.requires_grad = state != "freeze"

    def forward(self, x):
        return self.classifier(self.emb_model(x))
