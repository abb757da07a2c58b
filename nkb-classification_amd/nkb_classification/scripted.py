"""TorchScript export of a trained HIP model — the `scripted_{best,last}.pt` archives of the reference's train loop
(/root/reference/train.py:66-73: `torch.jit.script(model)` saved next to every state-dict checkpoint).

The HIP classifier is one custom autograd node over a flat parameter arena, not a torch module graph, so there is
nothing for `torch.jit.script` to trace.  What the reference's downstream tools (`inference.py`, `export.py`,
`get_model(..., scripted=True)`, model.py:163-165) need from the archive is a self-contained module with the same
`forward` contract and the trained weights; this file builds exactly that: a plain `torch.nn` module with timm's
parameter names (so `load_state_dict(hip_model.state_dict())` is exact) which torch scripts and runs with its own
kernels on any device.  It is an export artefact only — never used by `train_epoch` / `val_epoch`.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
from torch import nn


class _SEModule(nn.Module):
    """timm SEModule: x * sigmoid(fc2(relu(fc1(mean over the map)))), rd = make_divisible(C / 16, 8)."""

    def __init__(self, channels: int):
        super().__init__()
        rd = max(8, int(channels / 16 + 4) // 8 * 8)
        self.fc1 = nn.Conv2d(channels, rd, 1, bias=True)
        self.fc2 = nn.Conv2d(rd, channels, 1, bias=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.fc2(torch.relu(self.fc1(s))))


class _EcaModule(nn.Module):
    """timm EcaModule: x * sigmoid(Conv1d(1, 1, k, zero padding) along the channel axis of the pooled vector)."""

    def __init__(self, channels: int):
        super().__init__()
        t = int(abs(math.log2(channels) + 1) / 2)
        k = max(t if t % 2 else t + 1, 3)
        self.conv = nn.Conv1d(1, 1, k, padding=(k - 1) // 2, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = x.mean((2, 3)).unsqueeze(1)                       # [N][1][C]
        return x * torch.sigmoid(self.conv(s)).squeeze(1).unsqueeze(-1).unsqueeze(-1)


def _attn_module(attn: Optional[str], channels: int) -> nn.Module:
    if attn == "se":
        return _SEModule(channels)
    if attn == "eca":
        return _EcaModule(channels)
    return nn.Identity()


class _BasicBlock(nn.Module):
    def __init__(self, inplanes: int, planes: int, stride: int, downsample: Optional[nn.Module], attn: Optional[str] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.se = _attn_module(attn, planes)
        self.downsample = downsample if downsample is not None else nn.Identity()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.relu(self.bn1(self.conv1(x)))
        y = self.se(self.bn2(self.conv2(y)))
        return torch.relu(y + self.downsample(x))


class _Bottleneck(nn.Module):
    def __init__(self, inplanes: int, planes: int, stride: int, downsample: Optional[nn.Module], attn: Optional[str] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.se = _attn_module(attn, planes * 4)
        self.downsample = downsample if downsample is not None else nn.Identity()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.relu(self.bn1(self.conv1(x)))
        y = torch.relu(self.bn2(self.conv2(y)))
        y = self.se(self.bn3(self.conv3(y)))
        return torch.relu(y + self.downsample(x))


class _ResNet(nn.Module):
    def __init__(self, bottleneck: bool, layers, stem: Optional[List[int]] = None, avg_down: bool = False, attn: Optional[str] = None):
        super().__init__()
        exp = 4 if bottleneck else 1
        block = _Bottleneck if bottleneck else _BasicBlock
        if stem is None:
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        else:                                              # deep stem of the D / T members
            self.conv1 = nn.Sequential(nn.Conv2d(3, stem[0], 3, 2, 1, bias=False), nn.BatchNorm2d(stem[0]), nn.ReLU(),
                                       nn.Conv2d(stem[0], stem[1], 3, 1, 1, bias=False), nn.BatchNorm2d(stem[1]), nn.ReLU(),
                                       nn.Conv2d(stem[1], 64, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            blocks: List[nn.Module] = []
            for b in range(n):
                stride = 2 if (b == 0 and li > 0) else 1
                ds = None
                if b == 0 and (stride != 1 or inplanes != planes * exp) and avg_down:
                    pool: nn.Module = nn.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False) if stride != 1 else nn.Identity()
                    ds = nn.Sequential(pool, nn.Conv2d(inplanes, planes * exp, 1, 1, bias=False), nn.BatchNorm2d(planes * exp))
                elif b == 0 and (stride != 1 or inplanes != planes * exp):
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * exp, 1, stride, bias=False), nn.BatchNorm2d(planes * exp))
                blocks.append(block(inplanes, planes, stride, ds, attn))
                inplanes = planes * exp
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
        self.num_features = inplanes

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(torch.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return x.mean((2, 3))


class _Attention(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        qkv = self.qkv(x).reshape(B, T, 3, self.num_heads, D // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = (q @ k.transpose(-2, -1)) * (float(D // self.num_heads) ** -0.5)
        y = (att.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, D)
        return self.proj(y)


class _Mlp(nn.Module):
    """act: "gelu" (exact erf) or "quick_gelu" (x * sigmoid(1.702 x): the OpenAI-weight CLIP towers)."""

    def __init__(self, dim: int, hidden: int, act: str = "gelu"):
        super().__init__()
        if act not in ("gelu", "quick_gelu"):
            raise ValueError(f"unknown MLP activation {act!r}")
        self.quick_gelu = act == "quick_gelu"
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h = self.fc1(x)
        if self.quick_gelu:
            h = h * torch.sigmoid(1.702 * h)
        else:
            h = torch.nn.functional.gelu(h)
        return self.fc2(h)


class _LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x * self.gamma


class _Block(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: float, ln_eps: float = 1e-6, init_values: Optional[float] = None,
                 act: str = "gelu"):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=ln_eps)
        self.attn = _Attention(dim, heads)
        self.ls1 = _LayerScale(dim, init_values) if init_values is not None else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=ln_eps)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio), act)
        self.ls2 = _LayerScale(dim, init_values) if init_values is not None else nn.Identity()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class _PatchEmbed(nn.Module):
    def __init__(self, patch: int, dim: int, bias: bool = True):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, patch, patch, bias=bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(x).flatten(2).transpose(1, 2)


class _ViT(nn.Module):
    """timm VisionTransformer with its pre_norm / init_values (LayerScale) / no_embed_class / act_layer options
    (nkb_classification/vit.py)."""

    def __init__(self, img: int, patch: int, dim: int, depth: int, heads: int, mlp_ratio: float = 4.0, pre_norm: bool = False,
                 ln_eps: float = 1e-6, init_values: Optional[float] = None, no_embed_class: bool = False, act: str = "gelu"):
        super().__init__()
        self.num_features = dim
        self.no_embed_class = no_embed_class
        self.patch_embed = _PatchEmbed(patch, dim, bias=not pre_norm)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img // patch) ** 2 + (0 if no_embed_class else 1), dim))
        self.norm_pre = nn.LayerNorm(dim, eps=ln_eps) if pre_norm else nn.Identity()
        self.blocks = nn.Sequential(*[_Block(dim, heads, mlp_ratio, ln_eps, init_values, act) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=ln_eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.patch_embed(x)
        cls = self.cls_token.expand(x.shape[0], -1, -1)
        if self.no_embed_class:
            x = torch.cat((cls, x + self.pos_embed), dim=1)
        else:
            x = torch.cat((cls, x), dim=1) + self.pos_embed
        return self.norm(self.blocks(self.norm_pre(x)))[:, 0]


class _UnicomAttention(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        qkv = self.qkv(x).reshape(B, T, 3, self.num_heads, D // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = (q @ k.transpose(-2, -1)) * (float(D // self.num_heads) ** -0.5)
        y = (att.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, D)
        return self.proj(y)


class _UnicomMlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2(torch.nn.functional.relu6(self.fc1(x)))


class _UnicomBlock(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _UnicomAttention(dim, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _UnicomMlp(dim, dim * 4)

    def forward(self, x: torch.Tensor) -> torch.Tensor:      # stochastic depth is the identity at inference
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class _UnicomViT(nn.Module):
    def __init__(self, img: int, patch: int, dim: int, emb: int, depth: int, heads: int):
        super().__init__()
        self.patch_embed = _PatchEmbed(patch, dim)
        T = (img // patch) ** 2
        self.pos_embed = nn.Parameter(torch.zeros(1, T, dim))
        self.blocks = nn.Sequential(*[_UnicomBlock(dim, heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)
        self.feature = nn.Sequential(nn.Linear(dim * T, dim, bias=False), nn.BatchNorm1d(dim, eps=2e-5),
                                     nn.Linear(dim, emb, bias=False), nn.BatchNorm1d(emb, eps=2e-5))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.norm(self.blocks(self.patch_embed(x) + self.pos_embed))
        return self.feature(x.reshape(x.shape[0], -1))


class _CNLayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor (ConvNeXt stem / downsample)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.nn.functional.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps)
        return y.permute(0, 3, 1, 2)


class _CNBlock(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim)
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        y = self.mlp(self.norm(y)).permute(0, 3, 1, 2)
        return x + y * self.gamma.reshape(1, -1, 1, 1)


class _GRN(nn.Module):
    """timm GlobalResponseNorm over [N, H, W, C] (ConvNeXt V2): x + bias + weight * x * G / (mean_c G + eps), G the L2 norm of a
    channel over the pixels of one image."""

    def __init__(self, dim: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        g = torch.sqrt((x * x).sum(dim=[1, 2], keepdim=True))
        n = g / (g.mean(dim=-1, keepdim=True) + 1e-6)
        return x + (self.bias + self.weight * (x * n))


class _GRNMlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.grn = _GRN(hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2(self.grn(torch.nn.functional.gelu(self.fc1(x))))


class _CNBlockV2(nn.Module):
    """ConvNeXt V2 block: GRN inside the MLP, no layer scale."""

    def __init__(self, dim: int):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _GRNMlp(dim, 4 * dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        return x + self.mlp(self.norm(y)).permute(0, 3, 1, 2)


class _CNStage(nn.Module):
    def __init__(self, in_dim: int, dim: int, depth: int, downsample: bool, use_grn: bool = False):
        super().__init__()
        if downsample:
            self.downsample = nn.Sequential(_CNLayerNorm2d(in_dim, eps=1e-6), nn.Conv2d(in_dim, dim, 2, 2))
        else:
            self.downsample = nn.Identity()
        self.blocks = nn.Sequential(*[_CNBlockV2(dim) if use_grn else _CNBlock(dim) for _ in range(depth)])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.blocks(self.downsample(x))


class _CNHead(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.norm(x.mean((2, 3)))


class _ConvNeXt(nn.Module):
    """timm ConvNeXt layout, restated from memory, parity unpinned (see nkb_classification/convnext.py); dropout is the
    identity at inference, so the nn.Dropout children (parameter-free) are left out.  use_grn: the V2 members (GRN in the MLP, no gamma)."""

    def __init__(self, depths: List[int], dims: List[int], use_grn: bool = False):
        super().__init__()
        self.num_features = dims[-1]
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), _CNLayerNorm2d(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[_CNStage(dims[max(i - 1, 0)], dims[i], depths[i], i > 0, use_grn) for i in range(len(dims))])
        self.head = _CNHead(dims[-1])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.head(self.stages(self.stem(x)))


class _SingleHead(nn.Module):
    def __init__(self, emb_model: nn.Module, emb: int, n: int):
        super().__init__()
        self.emb_model = emb_model
        self.classifier = nn.Sequential(nn.Dropout(0.0), nn.Linear(emb, n))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.classifier(self.emb_model(x))


class _MultiHead(nn.Module):
    def __init__(self, emb_model: nn.Module, emb: int, sizes: Dict[str, int]):
        super().__init__()
        self.emb_model = emb_model
        self.classifier = nn.ModuleDict({t: nn.Sequential(nn.Dropout(0.0), nn.Linear(emb, n)) for t, n in sizes.items()})

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        emb = self.emb_model(x)
        out: Dict[str, torch.Tensor] = {}
        for name, head in self.classifier.items():
            out[name] = head(emb)
        return out


def _backbone_like(hip_backbone) -> nn.Module:
    if getattr(hip_backbone, "family", "") == "unicom":
        return _UnicomViT(hip_backbone.img, hip_backbone.patch, hip_backbone.dim, hip_backbone.num_features,
                          len(hip_backbone.blocks), hip_backbone.heads)
    if getattr(hip_backbone, "family", "") == "vit":
        return _ViT(hip_backbone.img, hip_backbone.patch, hip_backbone.num_features, len(hip_backbone.blocks), hip_backbone.heads,
                    pre_norm=hip_backbone.pre_norm, ln_eps=hip_backbone.ln_eps, init_values=hip_backbone.init_values,
                    no_embed_class=hip_backbone.no_embed_class, act=getattr(hip_backbone, "act", "gelu"))
    if getattr(hip_backbone, "family", "") == "convnext":
        return _ConvNeXt(list(hip_backbone.depths), list(hip_backbone.dims), bool(getattr(hip_backbone, "use_grn", False)))
    layers = [len(getattr(hip_backbone, f"layer{i}")) for i in (1, 2, 3, 4)]
    bottleneck = hasattr(getattr(hip_backbone, "layer1")[0], "conv3")
    stem = None
    if getattr(hip_backbone, "deep_stem", False):
        stem = [hip_backbone.conv1[0].out_channels, hip_backbone.conv1[3].out_channels]
    se = getattr(getattr(hip_backbone, "layer1")[0], "se", None)             # the SE / ECA members: channel attention in every block
    return _ResNet(bottleneck, layers, stem, bool(getattr(hip_backbone, "avg_down", False)), getattr(se, "kind", None))


def build_scriptable(hip_model) -> nn.Module:
    """Plain-torch module with the HIP model's architecture, weights and forward contract (eval mode, CPU)."""
    emb = _backbone_like(hip_model.emb_model)
    if isinstance(hip_model.classifier, nn.ModuleDict):
        twin = _MultiHead(emb, hip_model.emb_size, {t: h[1].out_features for t, h in hip_model.classifier.items()})
    else:
        twin = _SingleHead(emb, hip_model.emb_size, hip_model.classifier[1].out_features)
    state = {k: v.detach().to("cpu") for k, v in hip_model.state_dict().items()}
    twin.load_state_dict(state, strict=True)
    return twin.eval()


def save_scripted(hip_model, path) -> None:
    """`torch.jit.script` archive of the trained model, as train.py:66-73 writes per epoch."""
    torch.jit.script(build_scriptable(hip_model)).save(str(path))
