"""Pure-torch twin of the SE / ECA members of nkb_classification/backbones.py (seresnet*, ecaresnet*): the truth of the SE-ResNet tests
(float64 / fp32 / autocast-bf16, torch's own kernels on the CPU).  Same state-dict key names (`emb_model.` + timm's, `classifier.1.`)
and the same operations in the same order as the scripted export twin.

Restated from memory of timm (resnet.py blocks with `attn_layer="se"` / `"eca"`, SEModule, EcaModule), parity unpinned: timm is not
available offline.  The block gets an attribute `se` between its last BatchNorm and `downsample`; forward is
act(se(bn_last(conv_last(.))) + shortcut).  Cross-checks: seresnet50 has 26 039 024 backbone parameters (28 088 024 with a 1000-class
fc, timm's published 28.09 M), seresnet18 11 266 624, ecaresnet50d 23 527 350 (resnet50d + 86)."""
import math
from typing import Dict

import torch
from torch import nn

SERESNETS = {
    "seresnet18": dict(bottleneck=False, layers=(2, 2, 2, 2), attn="se"),
    "seresnet34": dict(bottleneck=False, layers=(3, 4, 6, 3), attn="se"),
    "seresnet50": dict(bottleneck=True, layers=(3, 4, 6, 3), attn="se"),
    "seresnet101": dict(bottleneck=True, layers=(3, 4, 23, 3), attn="se"),
    "seresnet152": dict(bottleneck=True, layers=(3, 8, 36, 3), attn="se"),
    "seresnet50t": dict(bottleneck=True, layers=(3, 4, 6, 3), attn="se", stem=(24, 32)),
    "seresnet152d": dict(bottleneck=True, layers=(3, 8, 36, 3), attn="se", stem=(32, 32)),
    "ecaresnet26t": dict(bottleneck=True, layers=(2, 2, 2, 2), attn="eca", stem=(24, 32)),
    "ecaresnet50t": dict(bottleneck=True, layers=(3, 4, 6, 3), attn="eca", stem=(24, 32)),
    "ecaresnet50d": dict(bottleneck=True, layers=(3, 4, 6, 3), attn="eca", stem=(32, 32)),
    "ecaresnet101d": dict(bottleneck=True, layers=(3, 4, 23, 3), attn="eca", stem=(32, 32)),
    "seresnet_tiny_basic": dict(bottleneck=False, layers=(1, 1, 1, 1), attn="se"),
    "seresnet_tiny_bottleneck": dict(bottleneck=True, layers=(1, 1, 1, 1), attn="se"),
    "ecaresnet_tiny_bottleneck": dict(bottleneck=True, layers=(1, 1, 1, 1), attn="eca"),
}
TINY = tuple(k for k in SERESNETS if "_tiny_" in k)
FULL = tuple(k for k in SERESNETS if "_tiny_" not in k)


def se_rd(channels: int) -> int:
    return max(8, int(channels / 16 + 4) // 8 * 8)            # make_divisible(C / 16, 8)


def eca_k(channels: int) -> int:
    t = int(abs(math.log2(channels) + 1) / 2)
    return max(t if t % 2 else t + 1, 3)


class SEModule(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, se_rd(channels), 1, bias=True)
        self.fc2 = nn.Conv2d(se_rd(channels), channels, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.fc2(torch.relu(self.fc1(s))))


class EcaModule(nn.Module):
    def __init__(self, channels):
        super().__init__()
        k = eca_k(channels)
        self.conv = nn.Conv1d(1, 1, k, padding=(k - 1) // 2, bias=False)

    def forward(self, x):
        s = x.mean((2, 3)).unsqueeze(1)
        return x * torch.sigmoid(self.conv(s)).squeeze(1)[:, :, None, None]


ATTN = {"se": SEModule, "eca": EcaModule}


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample, attn):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.se = ATTN[attn](planes * 4)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        y = torch.relu(self.bn1(self.conv1(x)))
        y = torch.relu(self.bn2(self.conv2(y)))
        return torch.relu(self.se(self.bn3(self.conv3(y))) + sc)

    def last_bn(self):
        return self.bn3


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample, attn):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.se = ATTN[attn](planes)
        self.downsample = downsample

    def forward(self, x):
        sc = x if self.downsample is None else self.downsample(x)
        y = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.se(self.bn2(self.conv2(y))) + sc)

    def last_bn(self):
        return self.bn2


class SEResNet(nn.Module):
    def __init__(self, bottleneck, layers, attn, stem=None):
        super().__init__()
        block = Bottleneck if bottleneck else BasicBlock
        if stem is None:
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        else:
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
                if (s != 1 or inplanes != planes * block.expansion) and stem is not None:      # avg_down comes with the deep stems
                    pool = nn.Identity() if s == 1 else nn.AvgPool2d(2, s, ceil_mode=True, count_include_pad=False)
                    down = nn.Sequential(pool, nn.Conv2d(inplanes, planes * block.expansion, 1, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                elif s != 1 or inplanes != planes * block.expansion:
                    down = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, s, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(inplanes, planes, s, down, attn))
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


class SEResNetClassifier(nn.Module):
    """The reference's SingletaskClassifier / MultitaskClassifier wrapper (model.py:17-159) around the twin."""

    def __init__(self, cfg_model: dict, classes):
        super().__init__()
        self.emb_model = SEResNet(**SERESNETS[cfg_model["model"]])
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
