"""Twin of the ViT members for their tests: oracle.torch_models.VisionTransformer (our own restatement of timm's VisionTransformer
layout; timm is not installed, so parity with it is unpinned) under emb_model., plus the reference's single-task head."""
from torch import nn

from oracle.torch_models import VisionTransformer

# name: (img, patch, dim, depth, heads, backbone parameters of the issue's table or None)
MEMBERS = {
    "vit_tiny_patch16_224": (224, 16, 192, 12, 3, 5_524_416),
    "deit_tiny_patch16_224": (224, 16, 192, 12, 3, 5_524_416),
    "vit_tiny_patch16_384": (384, 16, 192, 12, 3, 5_597_376),
    "vit_small_patch32_224": (224, 32, 384, 12, 6, 22_493_952),
    "vit_small_patch16_384": (384, 16, 384, 12, 6, 21_811_584),
    "vit_base_patch32_224": (224, 32, 768, 12, 12, 87_455_232),
    "vit_base_patch16_384": (384, 16, 768, 12, 12, 86_090_496),
    "deit_small_patch16_224": (224, 16, 384, 12, 6, None),
    "deit_base_patch16_224": (224, 16, 768, 12, 12, None),
    "vit_tiny192_test": (64, 16, 192, 2, 3, None),
    "vit_tiny192_p32_test": (96, 32, 192, 1, 3, None),
}


class ViTClassifier(nn.Module):
    """The reference's SingletaskClassifier wrapper (model.py:17-159) around the twin."""

    def __init__(self, name: str, n_classes: int):
        super().__init__()
        img, patch, dim, depth, heads, _ = MEMBERS[name]
        self.emb_model = VisionTransformer(img, patch, dim, depth, heads)
        self.emb_size = dim
        self.classifier = nn.Sequential(nn.Dropout(0.0), nn.Linear(dim, n_classes))
        nn.init.kaiming_normal_(self.classifier[1].weight, nonlinearity="relu")
        nn.init.zeros_(self.classifier[1].bias)

    def forward(self, x):
        return self.classifier(self.emb_model(x))
