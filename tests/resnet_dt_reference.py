"""Pure-torch twin of the ResNet-D/T members of nkb_classification/backbones.py (resnet14t, resnet26t, resnet26d, resnet50d and
the other D members): the truth of the ResNet-D/T tests (float64 / fp32 / autocast-bf16, torch's own kernels on the CPU).  Same
state-dict key names (`emb_model.` + timm's, `classifier.1.`) and the same operations in the same order as the scripted export twin.

Restated from memory of timm's ResNet (deep stem `stem_type="deep"` / `"deep_tiered"`, `avg_down=True`), parity unpinned: timm is
not available offline.  Cross-check: resnet14t has 8 032 632 backbone parameters, which with a 1000-class fc is timm's published
10.08 M; resnet50d 23 527 264 (25 576 264 with the fc)."""
from typing import Dict

import torch
from torch import nn

RESNETS_DT = {
    "resnet14t": dict(bottleneck=True, layers=(1, 1, 1, 1), stem=(24, 32)),
    "resnet26t": dict(bottleneck=True, layers=(2, 2, 2, 2), stem=(24, 32)),
    "resnet26d": dict(bottleneck=True, layers=(2, 2, 2, 2), stem=(32, 32)),
    "resnet50d": dict(bottleneck=True, layers=(3, 4, 6, 3), stem=(32, 32)),
    "resnet101d": dict(bottleneck=True, layers=(3, 4, 23, 3), stem=(32, 32)),
    "resnet18d": dict(bottleneck=False, layers=(2, 2, 2, 2), stem=(32, 32)),
    "resnet34d": dict(bottleneck=False, layers=(3, 4, 6, 3), stem=(32, 32)),
}


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        y = torch.relu(self.bn1(self.conv1(x)))
        y = torch.relu(self.bn2(self.conv2(y)))
        return torch.relu(self.bn3(self.conv3(y)) + sc)

    def last_bn(self):
        return self.bn3


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        y = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(y)) + sc)

    def last_bn(self):
        return self.bn2


class ResNetDT(nn.Module):
    def __init__(self, bottleneck, layers, stem):
        super().__init__()
        block = Bottleneck if bottleneck else BasicBlock
        c1, c2 = stem
        self.conv1 = nn.Sequential(nn.Conv2d(3, c1, 3, 2, 1, bias=False), nn.BatchNorm2d(c1), nn.ReLU(),
                                   nn.Conv2d(c1, c2, 3, 1, 1, bias=False), nn.BatchNorm2d(c2), nn.ReLU(),
                                   nn.Conv2d(c2, 64, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            blocks = []
            for b in range(n):
                s = (1 if i == 0 else 2) if b == 0 else 1
                down = None
                if s != 1 or inplanes != planes * block.expansion:
                    pool = nn.Identity() if s == 1 else nn.AvgPool2d(2, s, ceil_mode=True, count_include_pad=False)
                    down = nn.Sequential(pool, nn.Conv2d(inplanes, planes * block.expansion, 1, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(inplanes, planes, s, down))
                inplanes = planes * block.expansion
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.num_features = inplanes
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        for m in self.modules():
            if isinstance(m, (Bottleneck, BasicBlock)):
                nn.init.zeros_(m.last_bn().weight)           # zero_init_last

    def forward(self, x):
        x = self.maxpool(torch.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return x.mean((2, 3))


class ResNetDTClassifier(nn.Module):
    """The reference's SingletaskClassifier / MultitaskClassifier wrapper (model.py:17-159) around the twin."""

    def __init__(self, cfg_model: dict, classes):
        super().__init__()
        self.emb_model = ResNetDT(**RESNETS_DT[cfg_model["model"]])
        self.emb_size = self.emb_model.num_features
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

    def set_backbone_state(self, state: str):
        for p in self.emb_model.parameters():
            p.requires_grad = state == "unfreeze"

    def forward(self, x):
        emb = self.emb_model(x)
        if isinstance(self.classifier, nn.ModuleDict):
            out: Dict[str, torch.Tensor] = {t: head(emb) for t, head in self.classifier.items()}
            return out
        return self.classifier(emb)
