"""Pure-torch ConvNeXt V2 twin of nkb_classification/convnext.py (use_grn members): the truth of the ConvNeXt V2 tests (float64 on
the CPU, fp32 and autocast-bf16 on the GPU).  Same state-dict key names (`emb_model.` + timm's, `classifier.1.`), torch's own kernels.

Restated from timm's GlobalResponseNorm / GlobalResponseNormMlp, parity unpinned (timm is not available offline): the MLP is
fc1 -> GELU -> drop1 -> grn -> fc2 -> drop2, the block is x + mlp(norm(conv_dw(x))) with no gamma, and
    grn(x) = x + bias + weight * x * G / (mean_c G + 1e-6),   G = the L2 norm of one channel over the pixels of one image.
Cross-check: convnextv2_base has 378 backbone tensors / 87 692 800 elements = timm's published 88 717 800 minus its fc."""
import torch
import torch.nn.functional as F
from torch import nn

from convnext_reference import ConvNeXtClassifier, Head, LayerNorm2d

CONVNEXTV2S = {
    "convnextv2_base": dict(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024)),
    "convnextv2_test": dict(depths=(1, 1, 2, 1), dims=(128, 128, 256, 256)),
}


def grn(x, weight, bias, eps=1e-6):
    """x: [N, H, W, C] (or [N, HW, C]); the norm runs over every axis between the first and the last."""
    dims = tuple(range(1, x.dim() - 1))
    g = x.norm(p=2, dim=dims, keepdim=True)
    n = g / (g.mean(dim=-1, keepdim=True) + eps)
    return x + torch.addcmul(bias, weight, x * n)


class GRN(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        return grn(x, self.weight, self.bias)


class GRNMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.drop1 = nn.Dropout(0.0)
        self.grn = GRN(hidden)
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):                                    # x: [N, H, W, C]
        return self.drop2(self.fc2(self.grn(self.drop1(F.gelu(self.fc1(x))))))


class Block(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = GRNMlp(dim, 4 * dim)

    def forward(self, x):                                    # x: NCHW
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        return x + self.mlp(self.norm(y)).permute(0, 3, 1, 2)


class Stage(nn.Module):
    def __init__(self, in_dim, dim, depth, downsample):
        super().__init__()
        if downsample:
            self.downsample = nn.Sequential(LayerNorm2d(in_dim, eps=1e-6), nn.Conv2d(in_dim, dim, 2, 2))
        else:
            self.downsample = nn.Identity()
        self.blocks = nn.Sequential(*[Block(dim) for _ in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class ConvNeXtV2(nn.Module):
    def __init__(self, depths, dims):
        super().__init__()
        self.num_features = dims[-1]
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), LayerNorm2d(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[Stage(dims[max(i - 1, 0)], dims[i], depths[i], i > 0) for i in range(len(dims))])
        self.head = Head(dims[-1])
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.head(self.stages(self.stem(x)))


class ConvNeXtV2Classifier(ConvNeXtClassifier):
    """The reference's classifier wrapper (model.py:17-159) around the V2 twin: the V1 wrapper with another backbone."""

    def __init__(self, cfg_model: dict, classes):
        nn.Module.__init__(self)
        self.emb_model = ConvNeXtV2(**CONVNEXTV2S[cfg_model["model"]])
        self.emb_size = self.emb_model.num_features
        self.set_dropout(self.emb_model, cfg_model.get("backbone_dropout", 0.0))
        p = cfg_model.get("classifier_dropout", 0.0)
        if isinstance(classes, dict):
            self.classifier = nn.ModuleDict({t: nn.Sequential(nn.Dropout(p), nn.Linear(self.emb_size, len(c))) for t, c in classes.items()})
        else:
            self.classifier = nn.Sequential(nn.Dropout(p), nn.Linear(self.emb_size, len(classes)))
        for q in self.classifier.parameters():
            if q.ndim >= 2:
                nn.init.kaiming_normal_(q, nonlinearity="relu")
            else:
                nn.init.zeros_(q)
