"""Pure-torch ConvNeXt twin of nkb_classification/convnext.py: the truth of the ConvNeXt tests (float64 on the CPU, fp32 and
autocast-bf16 on the GPU).  Same state-dict key names (`emb_model.` + timm's, `classifier.1.`), same operations in the same
order as the scripted export twin (nkb_classification/scripted.py), torch's own kernels.

Restated from memory of timm's ConvNeXt, parity unpinned (timm is not available offline): convnext_base has 342 backbone
tensors / 87 566 464 elements, which equals timm's published 88 591 464 for the 1000-class model minus its fc."""
from typing import Dict

import torch
import torch.nn.functional as F
from torch import nn

CONVNEXTS = {
    "convnext_base": dict(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024)),
    "convnext_test": dict(depths=(1, 1, 2, 1), dims=(128, 128, 256, 256)),
}


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor."""

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.drop1 = nn.Dropout(0.0)
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(F.gelu(self.fc1(x)))))


class Block(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, 4 * dim)
        self.gamma = nn.Parameter(1e-6 * torch.ones(dim))

    def forward(self, x):                                    # x: NCHW
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        y = self.mlp(self.norm(y)).permute(0, 3, 1, 2)
        return x + y * self.gamma.reshape(1, -1, 1, 1)


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


class Head(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.drop = nn.Dropout(0.0)

    def forward(self, x):
        return self.drop(self.norm(x.mean((2, 3))))


class ConvNeXt(nn.Module):
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


class ConvNeXtClassifier(nn.Module):
    """The reference's SingletaskClassifier / MultitaskClassifier wrapper (model.py:17-159) around the twin."""

    def __init__(self, cfg_model: dict, classes):
        super().__init__()
        self.emb_model = ConvNeXt(**CONVNEXTS[cfg_model["model"]])
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

    @staticmethod
    def set_dropout(model: nn.Module, drop_rate: float) -> None:
        for child in model.children():
            if isinstance(child, nn.Dropout):
                child.p = drop_rate
            ConvNeXtClassifier.set_dropout(child, drop_rate)

    def set_backbone_state(self, state: str):
        for p in self.emb_model.parameters():
            p.requires_grad = state == "unfreeze"

    def forward(self, x):
        emb = self.emb_model(x)
        if isinstance(self.classifier, nn.ModuleDict):
            out: Dict[str, torch.Tensor] = {t: head(emb) for t, head in self.classifier.items()}
            return out
        return self.classifier(emb)
