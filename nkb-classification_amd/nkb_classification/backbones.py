"""Backbone definitions for the HIP engine.

The reference builds its backbone with `timm.create_model(name, pretrained=..., num_classes=0)`
(/root/reference/nkb_classification/model.py:82).  timm is a third-party dependency that is not part of the
reference tree; the modules below keep timm's parameter names and shapes (so `state_dict()` checkpoints are
interchangeable, train.py:70-72 / model.py:172) but hold parameters only — their arithmetic is executed by
HipEngine through libnkbhip, never by torch.nn forward methods.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
from torch import nn

from .hipnet import HipEngine


class _ParamOnly(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("this module only stores parameters; it is executed by the owning HIP classifier "
                           "(call the classifier returned by get_model, on a cuda device)")


def transformer_layer_groups(backbone: nn.Module) -> List[List[nn.Parameter]]:
    """Layer ids of a transformer backbone for layer-wise lr decay (utils.get_optimizer, `layer_decay`): entry k lists the
    parameters of id k in `parameters()` order.  Id 0 holds what sits in front of the blocks (cls_token, pos_embed, patch_embed.*,
    norm_pre.*), id i + 1 is blocks.i.*, id depth + 1 everything after the blocks (the final norm, unicom's feature head).  The
    usual fine-tuning rule restated (BEiT / MAE / DINOv2 recipes), not pinned against timm's own grouping."""
    depth = len(backbone.blocks)
    groups: List[List[nn.Parameter]] = [[] for _ in range(depth + 2)]
    for name, p in backbone.named_parameters():
        head = name.split(".")[0]
        if head == "blocks":
            k = int(name.split(".")[1]) + 1
        elif head in ("cls_token", "pos_embed", "patch_embed", "norm_pre"):
            k = 0
        else:
            k = depth + 1
        groups[k].append(p)
    return groups


def _make_divisible(v: float, divisor: int = 8) -> int:
    return max(divisor, int(v + divisor / 2) // divisor * divisor)


class _SE(_ParamOnly):
    """timm SEModule: fc1 = Conv2d(C, rd, 1), ReLU, fc2 = Conv2d(rd, C, 1), sigmoid, on the spatial mean; rd = make_divisible(C / 16, 8)."""
    kind = "se"

    def __init__(self, channels: int):
        super().__init__()
        rd = _make_divisible(channels / 16, 8)
        self.fc1 = nn.Conv2d(channels, rd, 1, bias=True)
        self.fc2 = nn.Conv2d(rd, channels, 1, bias=True)


class _ECA(_ParamOnly):
    """timm EcaModule: one Conv1d(1, 1, k, zero padding (k - 1) / 2, no bias) along the channel axis of the pooled vector, sigmoid."""
    kind = "eca"

    def __init__(self, channels: int):
        super().__init__()
        t = int(abs(math.log2(channels) + 1) / 2)
        k = max(t if t % 2 else t + 1, 3)
        self.conv = nn.Conv1d(1, 1, k, padding=(k - 1) // 2, bias=False)


_ATTN = {"se": _SE, "eca": _ECA}


class _Basic(_ParamOnly):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample, attn=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        if attn is not None:                       # registered between the last BatchNorm and downsample: keys bn2.*, se.*, downsample.*
            self.se = _ATTN[attn](planes)
        self.downsample = downsample

    def stages(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]

    def last_bn(self):
        return self.bn2


class _Bottle(_ParamOnly):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample, attn=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        if attn is not None:                       # keys bn3.*, se.*, downsample.*
            self.se = _ATTN[attn](planes * 4)
        self.downsample = downsample

    def stages(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]

    def last_bn(self):
        return self.bn3


class HipResNet(_ParamOnly):
    """timm `resnet*` parameter layout: conv1/bn1, layer1..4.{i}.conv{j}/bn{j}/downsample.{0,1}.

    The D / T members (resnet14t, resnet26t, resnet26d, resnet50d, ...) differ in two places, restated here from memory of timm
    (timm is not available offline: parity unpinned, as for ConvNeXt):
      stem=(c1, c2)  deep stem, conv1 = Sequential(Conv(3,c1,3,s2,p1), BN, ReLU, Conv(c1,c2,3,1,1), BN, ReLU, Conv(c2,64,3,1,1)) without
                     bias, then bn1 / ReLU / max-pool as before: keys conv1.{0,3,6}.weight, conv1.{1,4}.*, bn1.*.  (24, 32) is the
                     "tiered" stem of the T members, (32, 32) the D stem.
      avg_down       projection shortcut = Sequential(AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) in a stride-2 block /
                     Identity in a stride-1 block, Conv 1x1 stride 1, BN): keys downsample.1.weight, downsample.2.* (index 0 holds
                     no parameters).
    The second and third stem convolution run on csrc/stem3.hip, the pool on nkb_avgpool2x2; everything else is the plain members' path.

    The SE / ECA members (seresnet*, ecaresnet*; attn="se" / "eca") put timm's channel attention between the closing BatchNorm of every
    block and the residual add: the block gains an attribute `se` registered after the last BatchNorm and before `downsample` (keys
    ... bn3.*, se.fc1.{weight,bias}, se.fc2.{weight,bias}, downsample.* for SE with 4-D 1x1 Conv2d weights and rd = make_divisible(C / 16,
    8); se.conv.weight [1][1][k] for ECA), forward act(se(bn_last(conv_last(.))) + shortcut).  Restated from memory of timm as well: parity
    unpinned.  The attention weights are fp32 masters read by csrc/se.hip: no bf16 shadow, no data-gradient filter, not in gemm_convs()."""

    family = "resnet"

    def __init__(self, block, layers: Sequence[int], zero_init_last: bool = True, stem: Optional[Sequence[int]] = None,
                 avg_down: bool = False, attn: Optional[str] = None):
        super().__init__()
        self.deep_stem, self.avg_down = stem is not None, avg_down
        if stem is None:
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        else:
            c1, c2 = stem
            self.conv1 = nn.Sequential(nn.Conv2d(3, c1, 3, 2, 1, bias=False), nn.BatchNorm2d(c1), nn.ReLU(inplace=True),
                                       nn.Conv2d(c1, c2, 3, 1, 1, bias=False), nn.BatchNorm2d(c2), nn.ReLU(inplace=True),
                                       nn.Conv2d(c2, 64, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            blocks = []
            for b in range(n):
                s = stride if b == 0 else 1
                down = None
                if (s != 1 or inplanes != planes * block.expansion) and avg_down:
                    pool = nn.AvgPool2d(2, s, ceil_mode=True, count_include_pad=False) if s != 1 else nn.Identity()
                    down = nn.Sequential(pool, nn.Conv2d(inplanes, planes * block.expansion, 1, 1, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                elif s != 1 or inplanes != planes * block.expansion:
                    down = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, s, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(inplanes, planes, s, down, attn) if attn is not None else block(inplanes, planes, s, down))
                inplanes = planes * block.expansion
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.num_features = inplanes
        for m in self.modules():
            if isinstance(m, nn.Conv2d):           # (the SE excitation's 1x1 convolutions included; their biases and ECA's Conv1d keep torch's default)
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if zero_init_last:
            for m in self.modules():
                if isinstance(m, (_Basic, _Bottle)):
                    nn.init.zeros_(m.last_bn().weight)

    def blocks(self):
        for i in range(1, 5):
            for j, blk in enumerate(getattr(self, f"layer{i}")):
                yield f"layer{i}.{j}", blk

    def shortcut(self, blk):
        """(pool or None, conv, bn) of a block's projection shortcut: downsample.{0,1} of the plain members, .{1,2} behind the
        parameter-free pool / Identity of the avg_down members."""
        ds = blk.downsample
        if not self.avg_down:
            return None, ds[0], ds[1]
        return (ds[0] if isinstance(ds[0], nn.AvgPool2d) else None), ds[1], ds[2]

    def gemm_convs(self) -> List[nn.Conv2d]:
        """Convolutions that need a data-gradient filter (everything but the im2row stem convolution)."""
        out = [self.conv1[3], self.conv1[6]] if self.deep_stem else []
        for _, blk in self.blocks():
            out += [c for c, _ in blk.stages()]
            if blk.downsample is not None:
                out.append(self.shortcut(blk)[1])
        return out

    def stem_convs(self) -> List[nn.Conv2d]:
        return [self.conv1[0]] if self.deep_stem else [self.conv1]

    def _deep_stem_forward(self, eng: HipEngine, img: torch.Tensor, train: bool) -> torch.Tensor:
        """3x3/2 through im2row, then the two narrow 3x3/1 convolutions (csrc/stem3.hip); bn1 + ReLU + max-pool close the third."""
        from . import hip
        N, C, H, W = img.shape
        c0, b0, _, c1, b1, _, c2 = self.conv1
        P, Q = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        kp = eng.kpad(C * 9)
        col = eng.ws.get("stem.col", (N, P, Q, kp), eng.T)
        hip.im2row(eng.d, img, col, N, C, H, W, 3, 3, 2, 1, kp)
        x = eng.conv_bn("stem0", col, c0, b0, True, None, train, col_input=True).view(N, P, Q, c0.out_channels)
        x = eng.conv_bn("stem1", x, c1, b1, True, None, train)
        return eng.conv_bn("stem", x, c2, self.bn1, True, None, train, pool=True)

    # ---- execution plan ---------------------------------------------------------------
    def run_forward(self, eng: HipEngine, img: torch.Tensor, train: bool) -> torch.Tensor:
        from . import hip
        N, C, H, W = img.shape
        conv = self.conv1
        # bn1 -> ReLU -> max-pool close the stem convolution as one kernel each way (pool=True)
        if self.deep_stem:
            x = self._deep_stem_forward(eng, img, train)
        elif eng.packed_stem(conv):
            xp = eng.ws.get("stem.xp", (N, H, (W + 1) // 2 * 2, 4), eng.T)
            hip.stem_pack(eng.d, img, xp, N, C, H, W)
            x = eng.conv_bn("stem", xp, conv, self.bn1, True, None, train, pool=True, stem_packed=(N, H, W))
        else:
            R, st, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
            kp = eng.kpad(C * R * R)
            col = eng.ws.get("stem.col", (N, P, Q, kp), eng.T)
            hip.im2row(eng.d, img, col, N, C, H, W, R, R, st, pad, kp)
            x = eng.conv_bn("stem", col, conv, self.bn1, True, None, train, col_input=True, pool=True)
        all_blocks = list(self.blocks())
        nblocks = len(all_blocks)
        for bi, (name, blk) in enumerate(all_blocks):
            inp = x
            stages = blk.stages()
            short, short_affine = inp, None
            # the Gram form's backward needs the masked output gradient WITH its sums from the next block's first data gradient
            # (HipEngine.can_fuse_residual_bn_backward): decide on that producer here, where the forward form is chosen — a next
            # block whose first convolution takes the parity-class data gradient (3x3 / stride 2) cannot supply them
            se = getattr(blk, "se", None)          # channel attention: its own closing stage, never the Gram form
            want_gram = (isinstance(blk, _Bottle) and bi + 1 < nblocks and train and se is None
                         and not eng.s2_classes(all_blocks[bi + 1][1].stages()[0][0]))
            proj = None
            dpool, dconv, dbn = self.shortcut(blk) if blk.downsample is not None else (None, None, None)
            if blk.downsample is not None and dpool is None and want_gram and eng.gram_proj_ok(dconv, stages[-1][0]):
                proj = (dconv, dbn, inp, f"{name}.ds")     # rides inside the closing convolution
            elif blk.downsample is not None:
                # projection shortcut: its BatchNorm is applied inside the closing stage's pass (never materialised);
                # the convolution itself only depends on the block input, so it runs on the side stream next to the
                # main branch (the forward pass has nothing else to overlap)
                box = {}

                def shortcut(key=f"{name}.ds", src=inp, pool=dpool, cv=dconv, bn=dbn):
                    if pool is not None:                   # avg_down, stride-2 block: the 1x1 convolution reads the pooled map
                        src = eng.avgpool2(key + "p", src, train)
                    box["r"] = eng.conv_bn(key, src, cv, bn, False, None, train, defer_apply=True)
                eng.on_side(shortcut)
            # Gram form of the closing stage (hipnet._conv_bn_gram): every bottleneck but the last — its backward needs the masked
            # output gradient + sums that the NEXT block's conv1 data gradient leaves (can_fuse_residual_bn_backward)
            for k, (cv, bn) in enumerate(stages[:-1]):
                x = eng.conv_bn(f"{name}.{k}", x, cv, bn, True, None, train, gram_out=want_gram and k == len(stages) - 2)
            if blk.downsample is not None and proj is None:
                eng.join_side()
                short, s_scale, s_shift = box["r"]
                short_affine = (s_scale, s_shift) if s_scale is not None else None     # None: eval mode, already normalised
            cv, bn = stages[-1]
            gram = want_gram and eng.can_fuse_bn_backward(f"{name}.{len(stages) - 2}")
            if proj is not None and not gram:
                raise RuntimeError(f"{name}: projection shortcut planned into a Gram-form closing stage that did not qualify")
            if se is not None:
                x = eng.conv_bn_se(f"{name}.{len(stages) - 1}", x, cv, bn, se, short, short_affine, train)
                continue
            x = eng.conv_bn(f"{name}.{len(stages) - 1}", x, cv, bn, True, short, train, res_affine=short_affine, gram=gram, proj=proj)
        return eng.avgpool("gap", x)

    def run_backward(self, eng: HipEngine, g_emb: torch.Tensor, on_done=None):
        """on_done(module) is called as soon as every parameter gradient of `module` (layer4 .. layer1, then the
        stem) is final, so the data-parallel reducer can start exchanging it while backward continues."""
        g = eng.avgpool_backward("gap", g_emb, "g0")
        flip = 1
        blocks = list(self.blocks())
        g_stats = None        # set when g arrives already masked, with its BN reduction done by the producing dgrad
        for bi in range(len(blocks) - 1, -1, -1):
            name, blk = blocks[bi]
            eng.begin_block(bi)
            n = len(blk.stages())
            # last stage: ReLU(bn(conv) + shortcut); the masked incoming gradient also feeds the shortcut
            last = f"{name}.{n - 1}"
            top = n - 1
            if eng.saved[last].get("gram") is not None:
                # Gram-form closing stage: no BN-backward apply pass, no gradient of the raw conv output — R = g^T a, the small
                # algebra, and one data gradient over [g | a] that lands directly on the stage before
                if g_stats is None:
                    raise RuntimeError(f"{last}: the Gram-form closing stage needs the fused residual BN-backward producer")
                prev = f"{name}.{n - 2}"
                ga, st = eng.gram_closing_backward(last, g, g_stats, prev, f"a{n - 1}")
                gc = eng.bn_backward_fused(prev, ga, st, f"c{n - 1}")
                bits = None
                top = n - 2
            elif eng.saved[last].get("se") is not None:
                assert g_stats is None             # (can_fuse_residual_bn_backward: g arrives unmasked and un-reduced)
                gc = eng.se_closing_backward(last, g, "t0")
                bits = eng.saved[last]["bits"]
            elif g_stats is not None:
                gc = eng.bn_backward_fused(last, g, g_stats, "t0")
                bits = None                              # g is masked already
            else:
                gc = eng.bn_backward(last, g, "t0")
                bits = eng.saved[last]["bits"]           # g is NOT masked in place: consumers apply the bits
            for k in range(top, 0, -1):
                prev = f"{name}.{k - 1}"
                if eng.can_fuse_bn_backward(prev):
                    ga, st = eng.conv_backward(f"{name}.{k}", gc, f"a{k}", fuse_bn=prev)
                    gc = eng.bn_backward_fused(prev, ga, st, f"c{k}")
                else:
                    ga = eng.conv_backward(f"{name}.{k}", gc, f"a{k}")
                    gc = eng.bn_backward(prev, ga, f"c{k}")
            add, add_hw, add_bits = g, (0, 0), bits
            if blk.downsample is not None and eng.saved[last].get("gram_ds") is not None:
                add, add_bits, eng._gram_ds_grad = eng._gram_ds_grad, None, None      # formed by gram_closing_backward
            elif blk.downsample is not None:
                add_bits = None
                gcd = eng.bn_backward(f"{name}.ds", g, "t5", g_bits=bits)
                dpool, dconv, _ = self.shortcut(blk)
                sub = dconv.stride[0] == 2 and dconv.kernel_size[0] == 1 and dconv.padding[0] == 0
                add = eng.conv_backward(f"{name}.ds", gcd, "t6", subgrid=sub)
                if sub:
                    add_hw = (add.shape[1], add.shape[2])
                elif dpool is not None:                    # back through the pool: a full-grid `add` for conv1's data gradient
                    add = eng.avgpool2_backward(f"{name}.dsp", add, "t7")
            # the gradient leaving this block is the output gradient of the previous block's closing stage: let the
            # epilogue that forms it also mask it and reduce it for that stage's BatchNorm backward
            g_stats = None
            if bi > 0:
                pname, pblk = blocks[bi - 1]
                plast = f"{pname}.{len(pblk.stages()) - 1}"
                if eng.can_fuse_residual_bn_backward(plast, f"{name}.0"):
                    g, g_stats = eng.conv_backward(f"{name}.0", gc, f"g{flip}", add=add, add_hw=add_hw, add_bits=add_bits,
                                                   fuse_bn=plast)
            if g_stats is None:
                g = eng.conv_backward(f"{name}.0", gc, f"g{flip}", add=add, add_hw=add_hw, add_bits=add_bits)
            flip ^= 1
            eng.end_block(bi)
            if on_done is not None and name.endswith(".0"):
                on_done(getattr(self, name.split(".")[0]))
        eng.begin_block(-1)
        gc = eng.bn_pool_backward("stem", g, "t0")
        if self.deep_stem:
            # plain chain: narrow data gradient -> BatchNorm backward, twice; the three weight gradients go to the side stream
            ga = eng.conv_backward("stem", gc, "a2")
            gc = eng.bn_backward("stem1", ga, "c2")
            ga = eng.conv_backward("stem1", gc, "a1")
            gc = eng.bn_backward("stem0", ga.view(eng.saved["stem0"]["c"].shape), "c1")
            eng.conv_backward("stem0", gc, None)
        else:
            eng.conv_backward("stem", gc, None)
        if on_done is not None:
            on_done(self.conv1)
            on_done(self.bn1)


_RESNETS = {
    "resnet18": (_Basic, (2, 2, 2, 2)),
    "resnet34": (_Basic, (3, 4, 6, 3)),
    "resnet50": (_Bottle, (3, 4, 6, 3)),
    "resnet101": (_Bottle, (3, 4, 23, 3)),
    "resnet152": (_Bottle, (3, 8, 36, 3)),
    # deep 3x3 stem (T: 24-32-64 "tiered", D: 32-32-64) and average-pool projection shortcuts
    "resnet14t": (_Bottle, (1, 1, 1, 1), dict(stem=(24, 32), avg_down=True)),
    "resnet26t": (_Bottle, (2, 2, 2, 2), dict(stem=(24, 32), avg_down=True)),
    "resnet26d": (_Bottle, (2, 2, 2, 2), dict(stem=(32, 32), avg_down=True)),
    "resnet50d": (_Bottle, (3, 4, 6, 3), dict(stem=(32, 32), avg_down=True)),
    "resnet18d": (_Basic, (2, 2, 2, 2), dict(stem=(32, 32), avg_down=True)),
    "resnet34d": (_Basic, (3, 4, 6, 3), dict(stem=(32, 32), avg_down=True)),
    "resnet101d": (_Bottle, (3, 4, 23, 3), dict(stem=(32, 32), avg_down=True)),
    # reduced members of the family used by the fast parity tests (same blocks, one per stage)
    "resnet_tiny_basic": (_Basic, (1, 1, 1, 1)),
    "resnet_tiny_bottleneck": (_Bottle, (1, 1, 1, 1)),
}

# the SE / ECA siblings: the same blocks with channel attention in front of the residual add (csrc/se.hip)
_SE_RESNETS = {
    "seresnet18": (_Basic, (2, 2, 2, 2), dict(attn="se")),
    "seresnet34": (_Basic, (3, 4, 6, 3), dict(attn="se")),
    "seresnet50": (_Bottle, (3, 4, 6, 3), dict(attn="se")),
    "seresnet101": (_Bottle, (3, 4, 23, 3), dict(attn="se")),
    "seresnet152": (_Bottle, (3, 8, 36, 3), dict(attn="se")),
    "seresnet50t": (_Bottle, (3, 4, 6, 3), dict(attn="se", stem=(24, 32), avg_down=True)),
    "seresnet152d": (_Bottle, (3, 8, 36, 3), dict(attn="se", stem=(32, 32), avg_down=True)),
    "ecaresnet26t": (_Bottle, (2, 2, 2, 2), dict(attn="eca", stem=(24, 32), avg_down=True)),
    "ecaresnet50t": (_Bottle, (3, 4, 6, 3), dict(attn="eca", stem=(24, 32), avg_down=True)),
    "ecaresnet50d": (_Bottle, (3, 4, 6, 3), dict(attn="eca", stem=(32, 32), avg_down=True)),
    "ecaresnet101d": (_Bottle, (3, 4, 23, 3), dict(attn="eca", stem=(32, 32), avg_down=True)),
    # reduced members for the fast tests
    "seresnet_tiny_basic": (_Basic, (1, 1, 1, 1), dict(attn="se")),
    "seresnet_tiny_bottleneck": (_Bottle, (1, 1, 1, 1), dict(attn="se")),
    "ecaresnet_tiny_bottleneck": (_Bottle, (1, 1, 1, 1), dict(attn="eca")),
}


def create_backbone(name: str, pretrained: bool = False) -> nn.Module:
    """Counterpart of timm.create_model(name, pretrained=..., num_classes=0) for the families this engine runs."""
    key = name.lower()
    if pretrained:
        raise RuntimeError(f"pretrained=True needs timm's weight hub, which this offline engine does not ship; "
                           f"load a timm-format state_dict through cfg.model['checkpoint'] instead ({name})")
    if key in _RESNETS or key in _SE_RESNETS:
        blk, layers, *extra = _RESNETS[key] if key in _RESNETS else _SE_RESNETS[key]
        return HipResNet(blk, layers, **(extra[0] if extra else {}))
    from .vit import create_vit, vit_members
    m = create_vit(key)
    if m is None:
        from .convnext import _CONVNEXTS, create_convnext
        m = create_convnext(key)
    if m is None:
        se_members = sorted(k for k in _SE_RESNETS if "_tiny_" not in k)
        raise NotImplementedError(f"backbone {name!r} is not implemented by the HIP engine "
                                  f"(available: {sorted(_RESNETS)} + {se_members} + {vit_members()} + {sorted(_CONVNEXTS)})")
    return m
