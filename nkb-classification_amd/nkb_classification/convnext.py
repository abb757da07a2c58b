"""timm ConvNeXt family (convnext_base layout, num_classes=0) for the HIP engine: parameter containers with timm's state-dict
names + the forward / backward execution plan.

Reference call site: timm.create_model("convnext_base", ...) at /root/reference/nkb_classification/model.py:82 (the
reference's configs/trtconfig.py trains this member).  The architecture is restated from memory, parity unpinned: timm is
not available offline, so the layout below (stem 4x4/s4 conv + LayerNorm; per stage a LayerNorm + 2x2/s2 conv downsample
and blocks of depthwise 7x7 conv -> LayerNorm -> Linear(C, 4C) -> exact-erf GELU -> Linear(4C, C) -> gamma -> residual; head
LayerNorm of the global average pool; LayerNorm eps 1e-6; layer-scale init 1e-6) is pinned against a twin of our own
(tests/convnext_reference.py), not against timm.  Cross-check: 342 tensors / 87 566 464 elements for convnext_base, which
is timm's published 88 591 464 for the 1000-class model minus its 1 025 000-element fc.

Activations stay [N*H*W, C] rows (NHWC) throughout, so the Linear / LayerNorm / GELU / dropout steps are the ViT's; the new
HIP of this family is the depthwise convolution and the layer scale (csrc/dwconv.hip).

ConvNeXt V2 (convnextv2_*, the FCMAE checkpoints): the same stages with timm's GlobalResponseNormMlp — fc1 -> GELU -> drop1 -> grn
-> fc2 -> drop2, `mlp.grn.weight` / `mlp.grn.bias` of the hidden width, both zero at init, eps 1e-6 — and NO layer scale: the block is
x + mlp(norm(conv_dw(x))).  Restated from timm's GlobalResponseNorm, parity unpinned like the rest; the twin is
tests/convnextv2_reference.py.  Cross-check: 378 tensors / 87 692 800 elements for convnextv2_base = timm's published 88 717 800 minus
the fc.  The new HIP is the response normalisation (csrc/grn.hip).
"""
from __future__ import annotations

import torch
from torch import nn

from .backbones import _ParamOnly
from .hipnet import HipEngine


class _GRN(_ParamOnly):
    """The two parameters of timm's GlobalResponseNorm (both zero at init: the operator starts as the identity)."""
    eps = 1e-6

    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _Mlp(_ParamOnly):
    def __init__(self, dim, hidden, use_grn=False):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.drop1 = nn.Dropout(0.0)
        if use_grn:
            self.grn = _GRN(hidden)
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)


class _Block(_ParamOnly):
    def __init__(self, dim, ls_init=1e-6, use_grn=False):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim, use_grn)
        if not use_grn:                                      # (the V2 block has no layer scale)
            self.gamma = nn.Parameter(ls_init * torch.ones(dim))


class _Stage(_ParamOnly):
    def __init__(self, in_dim, dim, depth, downsample, use_grn=False):
        super().__init__()
        if downsample:
            self.downsample = nn.Sequential(nn.LayerNorm(in_dim, eps=1e-6), nn.Conv2d(in_dim, dim, 2, 2))
        else:
            self.downsample = nn.Identity()
        self.blocks = nn.Sequential(*[_Block(dim, use_grn=use_grn) for _ in range(depth)])


class _Head(_ParamOnly):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.drop = nn.Dropout(0.0)


class HipConvNeXt(_ParamOnly):
    family = "convnext"

    def __init__(self, depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024), use_grn=False):
        super().__init__()
        self.depths, self.dims, self.use_grn = tuple(depths), tuple(dims), bool(use_grn)
        self.num_features = dims[-1]
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), nn.LayerNorm(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[_Stage(dims[max(i - 1, 0)], dims[i], depths[i], i > 0, use_grn) for i in range(len(dims))])
        self.head = _Head(dims[-1])
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def gemm_convs(self):
        """The Linear layers and the three 2x2 / stride-2 downsample convolutions (generic implicit-GEMM kernels); the depthwise
        filters are read as fp32 masters by their own kernel and need no weight preparation."""
        out = [m for m in self.modules() if isinstance(m, nn.Linear)]
        out += [st.downsample[1] for st in self.stages if not isinstance(st.downsample, nn.Identity)]
        return out

    def stem_convs(self):
        return [self.stem[0]]

    def fp8_linears(self):
        """fp8 contractions are out of scope for this family, so cfg.amp_dtype = "fp8" runs it in bf16.  The empty list is what says
        so: a backbone WITHOUT this method leaves HipEngine.fp8_candidates at None, and the engine then takes every registered
        2-D weight (gemm_convs(): this family's Linear layers) as an fp8 candidate."""
        return []

    # ---- execution plan ---------------------------------------------------------------
    def run_forward(self, eng: HipEngine, img: torch.Tensor, train: bool) -> torch.Tensor:
        """Dropout sites are the nn.Dropout children the reference's set_dropout rewrites (model.py:66-72): mlp.drop1 after the
        GELU, mlp.drop2 before the layer scale, head.drop on the embedding.  Stochastic depth is off (drop_path_rate = 0).
        V2 blocks: the response normalisation sits between drop1 and fc2, and the residual is fc2's epilogue (drop2's, when active)."""
        for k in [k for k in eng.saved if k.endswith("_drop")]:
            del eng.saved[k]                                 # masks of a previous step must not leak into this backward
        B, _, Hh, Ww = img.shape
        cv = self.stem[0]
        ps = cv.kernel_size[0]
        H, W = Hh // ps, Ww // ps
        if H < 8 or W < 8:
            raise RuntimeError(f"ConvNeXt needs images of at least {8 * ps}x{8 * ps} (three 2x2 downsamples), got {Hh}x{Ww}")
        tok, _ = eng.patch_embed("stem", img, cv, train)
        x = eng.layernorm("stem.ln", tok, self.stem[1], train)
        for si, st in enumerate(self.stages):
            C = self.dims[si]
            if si > 0:
                h = eng.layernorm(f"s{si}.ds.ln", x, st.downsample[0], train)
                y = eng.conv_bias(f"s{si}.ds", h.view(B, H, W, self.dims[si - 1]), st.downsample[1], train)
                H, W = y.shape[1], y.shape[2]
                x = y.view(B * H * W, C)
            for bi, blk in enumerate(st.blocks):
                k, mlp = f"s{si}.b{bi}", blk.mlp
                y = eng.dwconv(f"{k}.dw", x, blk.conv_dw, B, H, W, train)
                h = eng.layernorm(f"{k}.ln", y, blk.norm, train)
                u = eng.mlp_gelu_fc1(k, h, mlp, train)
                if self.use_grn:
                    v = eng.grn(f"{k}.grn", u, mlp.grn, B, H * W, train)
                    if train and mlp.drop2.p > 0:
                        z = eng.linear(f"{k}.fc2", v, mlp.fc2, train)
                        x = eng.dropout(f"{k}.mlp2_drop", z, mlp.drop2.p, train, add=x)
                    else:
                        x = eng.linear(f"{k}.fc2", v, mlp.fc2, train, add=x)
                    continue
                z = eng.linear(f"{k}.fc2", u, mlp.fc2, train)
                z = eng.dropout(f"{k}.mlp2_drop", z, mlp.drop2.p, train)
                x = eng.layer_scale(f"{k}.ls", z, blk.gamma, x, train)
        pooled = eng.avgpool("gap", x.view(B, H, W, self.dims[-1]))
        emb = eng.layernorm("head.ln", pooled, self.head.norm, train)
        return eng.dropout("head_drop", emb, self.head.drop.p, train)

    def run_backward(self, eng: HipEngine, g_emb: torch.Tensor, on_done=None):
        """on_done(module) is called as soon as every parameter gradient of `module` (head norm, stages 3 .. 0, stem) is final,
        so the data-parallel reducer can start exchanging it while backward continues."""
        sv = eng.saved["stem"]
        B = sv["B"]
        D = self.dims[-1]
        g_emb = eng.dropout_backward("head_drop", g_emb, "gemb")
        gp = eng.layernorm_backward("head.ln", g_emb, eng.scratch("gpool", (B, D)), D)
        gx = eng.avgpool_backward("gap", gp, "g0")
        gx = gx.view(-1, D)
        if on_done is not None:
            on_done(self.head)
        # one unit per block or downsample: begin_block gives consecutive units scratch sets of opposite parity, so a unit's output
        # ("gx") never aliases its input (the previous unit's "gx") nor what the side-stream work of the unit before still reads
        unit = sum(self.depths) + len(self.dims) - 1
        for si in range(len(self.stages) - 1, -1, -1):
            st, C = self.stages[si], self.dims[si]
            M = gx.shape[0]
            for bi in range(len(st.blocks) - 1, -1, -1):
                unit -= 1
                eng.begin_block(unit)
                k = f"s{si}.b{bi}"
                if self.use_grn:
                    g2 = eng.dropout_backward(f"{k}.mlp2_drop", gx, "g2")          # branch gradient; the residual path keeps gx
                    d_v = eng.linear_backward(f"{k}.fc2", g2, "du")
                    if "gp" in eng.saved[f"{k}.act"]:
                        d_a = eng.grn_backward(f"{k}.grn", d_v, "da", mul=eng.saved[f"{k}.act"]["gp"])   # GELU backward rides along
                    else:
                        d_u = eng.dropout_backward(f"{k}.mlp_drop", eng.grn_backward(f"{k}.grn", d_v, "du3"), "du2")
                        d_a = eng.gelu_backward(f"{k}.act", d_u, "da")
                    d_h = eng.linear_backward(f"{k}.fc1", d_a, "dh")
                    gy = eng.layernorm_backward(f"{k}.ln", d_h, eng.scratch("gy", (M, C)), C)
                    gx = eng.dwconv_backward(f"{k}.dw", gy, "gx", add=gx)
                    eng.end_block(unit)
                    continue
                gz = eng.layer_scale_backward(f"{k}.ls", gx, "gz")             # branch gradient; the residual path keeps gx
                g2 = eng.dropout_backward(f"{k}.mlp2_drop", gz, "g2")
                d_h = eng.mlp_gelu_fc1_backward(k, g2)
                gy = eng.layernorm_backward(f"{k}.ln", d_h, eng.scratch("gy", (M, C)), C)
                gx = eng.dwconv_backward(f"{k}.dw", gy, "gx", add=gx)
                eng.end_block(unit)
            if si > 0:
                unit -= 1
                eng.begin_block(unit)
                gsv = eng.saved[f"s{si}.ds"]["geom"]
                gh = eng.conv_bias_backward(f"s{si}.ds", gx.view(B, gsv["P"], gsv["Q"], C), "gds")
                Cp = self.dims[si - 1]
                gx = eng.layernorm_backward(f"s{si}.ds.ln", gh.view(-1, Cp), eng.scratch("gx", (gh.numel() // Cp, Cp)), Cp)
                eng.end_block(unit)
            if on_done is not None:
                on_done(st)
        eng.begin_block(-1)
        D0, rows = self.dims[0], sv["B"] * sv["H"] * sv["W"]
        d_tok = eng.layernorm_backward("stem.ln", gx, eng.scratch("dtok", (rows, D0)), D0)
        eng.patch_embed_backward("stem", d_tok, self.stem[0])
        if on_done is not None:
            on_done(self.stem)


_CONVNEXTS = {
    "convnext_base": dict(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024)),
    "convnext_test": dict(depths=(1, 1, 2, 1), dims=(128, 128, 256, 256)),   # reduced member for fast parity tests
    "convnextv2_base": dict(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024), use_grn=True),
    "convnextv2_test": dict(depths=(1, 1, 2, 1), dims=(128, 128, 256, 256), use_grn=True),
}
# members that stay refused.  nkb_layernorm takes their widths (any D % 8 == 0 up to 2048); what still blocks them: the depthwise
# 7x7 and layer-scale kernels need C % 64 == 0 (C = 96 in tiny / small), the bf16 GEMMs need K % 64 == 0 (K = 96), and
# tests/test_convnext_cpu.py pins this refusal (the only thing left for large, whose widths no test has run)
_CONVNEXTS_UNSUPPORTED = {
    "convnext_tiny": (96, 192, 384, 768), "convnext_small": (96, 192, 384, 768), "convnext_large": (192, 384, 768, 1536),
    # V2: atto .. nano are built by timm with conv_mlp (their fc weights are 4-D 1x1 convolutions, another state-dict layout) at widths
    # 40 / 48 / 64 / 80; tiny is 96 wide; large and huge are widths no test has run
    "convnextv2_atto": (40, 80, 160, 320), "convnextv2_femto": (48, 96, 192, 384), "convnextv2_pico": (64, 128, 256, 512),
    "convnextv2_nano": (80, 160, 320, 640), "convnextv2_tiny": (96, 192, 384, 768), "convnextv2_large": (192, 384, 768, 1536),
    "convnextv2_huge": (352, 704, 1408, 2816),
}


# what else stands between a refused V2 member and the engine, said in its refusal
_CONVNEXTS_NOTE = {
    **{n: "; timm builds this member with conv_mlp, so its fc weights are 4-D" for n in
       ("convnextv2_atto", "convnextv2_femto", "convnextv2_pico", "convnextv2_nano")},
    "convnextv2_large": "; no test has run these widths", "convnextv2_huge": "; no test has run these widths",
}


def create_convnext(name: str):
    if name in _CONVNEXTS_UNSUPPORTED:
        raise NotImplementedError(f"backbone {name!r}: widths {_CONVNEXTS_UNSUPPORTED[name]} are not all multiples of 128, outside what the "
                                  f"HIP engine's ConvNeXt path (depthwise, layer-scale and GEMM kernels) is built and tested for (available ConvNeXt members: {sorted(_CONVNEXTS)})"
                                  + _CONVNEXTS_NOTE.get(name, ""))
    cfg = _CONVNEXTS.get(name)
    return HipConvNeXt(**cfg) if cfg else None
