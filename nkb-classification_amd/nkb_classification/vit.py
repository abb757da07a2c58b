"""timm VisionTransformer family (vit_base_patch16_224 layout, num_classes=0, class-token pooling) for the HIP
engine: parameter containers with timm's state-dict names + the forward / backward execution plan.

Reference call site: timm.create_model("vit_base_patch16_224", ...) at
/root/reference/nkb_classification/model.py:82; architecture per SURVEY.md §8 A8 (LayerNorm eps 1e-6, qkv with
bias, exact-erf GELU, pre-norm residual blocks, x[:, 0] of the final norm as the embedding).

Four constructor options of timm's VisionTransformer cover the foundation-model members (restated from memory of timm, parity
unpinned; the twin they are checked against is tests/vit_options_reference.py):
  pre_norm         CLIP image towers: bias-free patch projection, LayerNorm `norm_pre` in front of block 0 (ln_eps 1e-5)
  init_values      DINOv2 / DeiT-III: LayerScale, x + ls1(attn(norm1(x))), x + ls2(mlp(norm2(x))), gamma initialised to the value
  no_embed_class   DeiT-III: pos_embed covers the patch tokens only; the class token is prepended without one
  act              "gelu" (exact erf) | "quick_gelu" (x * sigmoid(1.702 x)): the CLIP towers trained by OpenAI, MetaCLIP and DFN.
                   timm keeps them under names of their own (`*_clip_quickgelu_*`, act_layer="quick_gelu") because the activation is
                   part of the model: a QuickGELU checkpoint in the GELU twin silently evaluates another function.  No parameter
                   depends on it, so the keys and shapes are the GELU twin's (twin: tests/vit_quickgelu_reference.py)
"""
from __future__ import annotations

import torch
from torch import nn

from . import hip
from .backbones import _ParamOnly, transformer_layer_groups
from .hipnet import HipEngine


class _PatchEmbed(_ParamOnly):
    def __init__(self, patch, in_chans, dim, bias=True):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, patch, patch, bias=bias)


class _Attention(_ParamOnly):
    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, dim * 3)
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)


class _Mlp(_ParamOnly):
    def __init__(self, dim, hidden, act="gelu"):
        super().__init__()
        self.act = act                                            # what HipEngine.mlp_gelu_fc1 applies between fc1 and fc2
        self.fc1 = nn.Linear(dim, hidden)
        self.drop1 = nn.Dropout(0.0)
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)


class _LayerScale(_ParamOnly):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class _Block(_ParamOnly):
    def __init__(self, dim, heads, mlp_ratio, ln_eps=1e-6, init_values=None, act="gelu"):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=ln_eps)
        self.attn = _Attention(dim, heads)
        if init_values is not None:
            self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=ln_eps)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio), act)
        if init_values is not None:
            self.ls2 = _LayerScale(dim, init_values)


class HipViT(_ParamOnly):
    family = "vit"

    def __init__(self, img=224, patch=16, dim=768, depth=12, heads=12, mlp_ratio=4.0, pre_norm=False, ln_eps=1e-6,
                 init_values=None, no_embed_class=False, act="gelu"):
        super().__init__()
        if act not in hip.ACT_KINDS:
            raise ValueError(f"unknown MLP activation {act!r}: one of {sorted(hip.ACT_KINDS)}")
        self.act = act
        self.num_features = dim
        self.img, self.patch, self.heads = img, patch, heads
        self.pre_norm, self.ln_eps, self.init_values, self.no_embed_class = pre_norm, ln_eps, init_values, no_embed_class
        self.patch_embed = _PatchEmbed(patch, 3, dim, bias=not pre_norm)
        n_tok = (img // patch) ** 2
        self.n_tokens = n_tok + 1                                  # class token + patches: the rows per image of every block
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.randn(1, n_tok if no_embed_class else n_tok + 1, dim) * 0.02)
        self.pos_drop = nn.Dropout(0.0)
        if pre_norm:
            self.norm_pre = nn.LayerNorm(dim, eps=ln_eps)
        self.blocks = nn.Sequential(*[_Block(dim, heads, mlp_ratio, ln_eps, init_values, act) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=ln_eps)
        self.head_drop = nn.Dropout(0.0)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def layer_groups(self):
        """Parameters per layer id (embeddings, one id per block, what follows the blocks) for `layer_decay`."""
        return transformer_layer_groups(self)

    def gemm_convs(self):
        return [m for m in self.modules() if isinstance(m, nn.Linear)]

    def stem_convs(self):
        return [self.patch_embed.proj]

    def fp8_linears(self):
        """The Linear layers of the transformer blocks: the contractions that cfg.amp_dtype = "fp8" moves to fp8 operands."""
        return [m for blk in self.blocks for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)]

    def refresh_derived(self, eng: HipEngine):
        """no_embed_class: nkb_vit_assemble adds pos[0] to the class row, so it reads an engine-owned [T, D] copy of pos_embed whose
        row 0 is zero.  Called by HipEngine.refresh_weights when the arena version moved (once per optimizer step, outside the
        recorded plans), never per launch."""
        if not self.no_embed_class:
            return
        T, D = self.n_tokens, self.num_features
        pos0 = eng.ws.get("pe.pos0", (T, D), torch.float32, zero=True)      # row 0 is written here only: at allocation
        pos0[1:].copy_(eng.arena.param_flat(self.pos_embed).view(T - 1, D))

    def _residual_branch(self, eng: HipEngine, key: str, drop_key: str, ls_key: str, h, lin, drop_p: float, ls, x, train: bool):
        """x + ls(drop(lin(h))): members without LayerScale keep the residual in the GEMM epilogue (or in the dropout pass);
        with LayerScale the Linear runs bare and nkb_layer_scale scales and adds."""
        if ls is not None:
            z = eng.dropout(drop_key, eng.linear(key, h, lin, train), drop_p, train)
            return eng.layer_scale(ls_key, z, ls.gamma, x, train)
        if train and drop_p > 0:
            return eng.dropout(drop_key, eng.linear(key, h, lin, train), drop_p, train, add=x)
        return eng.linear(key, h, lin, train, add=x)

    def run_forward(self, eng: HipEngine, img: torch.Tensor, train: bool) -> torch.Tensor:
        """Dropout sites follow timm's VisionTransformer (every nn.Dropout the reference's set_dropout rewrites,
        model.py:66-72): pos_drop after the position embedding, attn_drop on the attention probabilities, proj_drop and
        mlp.drop2 before the residual additions, mlp.drop1 after the GELU, head_drop on the pooled embedding."""
        for k in [k for k in eng.saved if k.endswith(".drop") or k.endswith("_drop")]:
            del eng.saved[k]                                 # masks of a previous step must not leak into this backward
        B, _, Hh, Ww = img.shape
        if Hh != self.img or Ww != self.img:
            raise RuntimeError(f"this ViT expects {self.img}x{self.img} inputs (pos_embed is fixed), got {Hh}x{Ww}")
        D, T = self.num_features, self.n_tokens
        a = eng.arena
        tok, _ = eng.patch_embed("pe", img, self.patch_embed.proj, train)
        x = eng.ws.get("pe.x", (B * T, D), eng.T)
        pos = eng.ws.get("pe.pos0", (T, D), torch.float32) if self.no_embed_class else a.param_flat(self.pos_embed)
        hip.vit_assemble(eng.d, False, tok, a.param_flat(self.cls_token), pos, x, B, T, D)
        x = eng.dropout("pos_drop", x, self.pos_drop.p, train)
        if self.pre_norm:
            x = eng.layernorm("norm_pre", x, self.norm_pre, train)
        scaled = self.init_values is not None
        for i, blk in enumerate(self.blocks):
            at, mlp = blk.attn, blk.mlp
            h = eng.layernorm(f"b{i}.ln1", x, blk.norm1, train, q_for=f"b{i}.qkv.f8x")
            qkv = eng.linear(f"b{i}.qkv", h, at.qkv, train)
            o = eng.attention(f"b{i}.attn", qkv, B, T, self.heads, train, drop_p=at.attn_drop.p, q_for=f"b{i}.proj.f8x")
            x = self._residual_branch(eng, f"b{i}.proj", f"b{i}.proj_drop", f"b{i}.ls1", o, at.proj, at.proj_drop.p,
                                      blk.ls1 if scaled else None, x, train)
            h = eng.layernorm(f"b{i}.ln2", x, blk.norm2, train, q_for=f"b{i}.fc1.f8x")
            u = eng.mlp_gelu_fc1(f"b{i}", h, mlp, train)
            x = self._residual_branch(eng, f"b{i}.fc2", f"b{i}.mlp2_drop", f"b{i}.ls2", u, mlp.fc2, mlp.drop2.p,
                                      blk.ls2 if scaled else None, x, train)
        # final norm on the class-token rows only (x[:, 0]); the other rows never reach the head
        emb = eng.layernorm("norm", x, self.norm, train, rows=B, x_stride=T * D)
        return eng.dropout("head_drop", emb, self.head_drop.p, train)

    def run_backward(self, eng: HipEngine, g_emb: torch.Tensor, on_done=None):
        B, T = eng.saved["pe"]["B"], self.n_tokens
        D = self.num_features
        M = B * T
        a = eng.arena
        scaled = self.init_values is not None
        gx = eng.scratch("gx0", (M, D))
        hip.zero_(gx)
        g_emb = eng.dropout_backward("head_drop", g_emb, "gemb")
        eng.layernorm_backward("norm", g_emb, gx, T * D)          # rows b*T (class tokens); everything else stays 0
        if on_done is not None:
            on_done(self.norm)
        flip = 1
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            eng.begin_block(i)
            # branch gradient (through LayerScale where the member has it: gamma * gx, dgamma += sum gx * z); the residual path keeps gx
            g2 = eng.layer_scale_backward(f"b{i}.ls2", gx, "gz2") if scaled else gx
            g2 = eng.dropout_backward(f"b{i}.mlp2_drop", g2, "g2")
            d_h = eng.mlp_gelu_fc1_backward(f"b{i}", g2)
            gmid = eng.layernorm_backward(f"b{i}.ln2", d_h, eng.scratch("gmid", (M, D)), D, add=gx)
            g1 = eng.layer_scale_backward(f"b{i}.ls1", gmid, "gz1") if scaled else gmid
            d_o = eng.linear_backward(f"b{i}.proj", eng.dropout_backward(f"b{i}.proj_drop", g1, "g1"), "do")
            d_qkv = eng.attention_backward(f"b{i}.attn", d_o, "dqkv", q_for=f"b{i}.qkv.f8g")
            d_h = eng.linear_backward(f"b{i}.qkv", d_qkv, "dh")
            gx = eng.layernorm_backward(f"b{i}.ln1", d_h, eng.scratch(f"gx{flip}", (M, D)), D, add=gmid)
            flip ^= 1
            eng.end_block(i)
            if on_done is not None:
                on_done(blk)
        eng.begin_block(-1)
        if self.pre_norm:
            gx = eng.layernorm_backward("norm_pre", gx, eng.scratch("gpre", (M, D)), D)
        gx = eng.dropout_backward("pos_drop", gx, "gpos")
        # embedding: d_pos = sum_b gx[b], d_cls = sum_b gx[b, 0], d_tok = gx[:, 1:], then the patch projection
        if self.no_embed_class:                                   # rows 1 .. T-1 only: the class row carries no position
            eng.colsum2d(gx.view(-1)[D:], a.grad_flat(self.pos_embed), B, (T - 1) * D, T * D)
        else:
            eng.colsum2d(gx, a.grad_flat(self.pos_embed), B, T * D, T * D)
        eng.colsum2d(gx, a.grad_flat(self.cls_token), B, D, T * D)
        d_tok = eng.scratch("dtok", (B * (T - 1), D))
        hip.vit_assemble(eng.d, True, d_tok, None, None, gx, B, T, D)
        eng.patch_embed_backward("pe", d_tok, self.patch_embed.proj)
        if on_done is not None:
            on_done(self.patch_embed)
            on_done([self.cls_token, self.pos_embed])
            if self.pre_norm:
                on_done(self.norm_pre)                             # (its own range: the patch projection lies between in the arena)


_CLIP = dict(pre_norm=True, ln_eps=1e-5)
_DEIT3 = dict(init_values=1e-6, no_embed_class=True)
_VITS = {
    "vit_base_patch16_224": dict(img=224, patch=16, dim=768, depth=12, heads=12),
    "vit_small_patch16_224": dict(img=224, patch=16, dim=384, depth=12, heads=6),
    "vit_large_patch16_224": dict(img=224, patch=16, dim=1024, depth=24, heads=16),
    # dim 192 (three heads of 64): LayerNorm rows on the masked-tail kernels, no GEMM inside the gemm8p envelope, no fp8
    "vit_tiny_patch16_224": dict(img=224, patch=16, dim=192, depth=12, heads=3),
    "vit_tiny_patch16_384": dict(img=384, patch=16, dim=192, depth=12, heads=3),
    # patch 32 (T = 50) and 384 px (T = 577: the unfused attention path, as unicom ViT-L/14@336px)
    "vit_small_patch32_224": dict(img=224, patch=32, dim=384, depth=12, heads=6),
    "vit_small_patch16_384": dict(img=384, patch=16, dim=384, depth=12, heads=6),
    "vit_base_patch32_224": dict(img=224, patch=32, dim=768, depth=12, heads=12),
    "vit_base_patch16_384": dict(img=384, patch=16, dim=768, depth=12, heads=12),
    # CLIP image towers (pre_norm, plain nn.LayerNorm eps), DINOv2 (LayerScale, patch 14 at 518 px: T = 1370 on the unfused attention
    # path) and DeiT-III (LayerScale, position embedding on the patch tokens only)
    "vit_base_patch32_clip_224": dict(img=224, patch=32, dim=768, depth=12, heads=12, **_CLIP),
    "vit_base_patch16_clip_224": dict(img=224, patch=16, dim=768, depth=12, heads=12, **_CLIP),
    "vit_large_patch14_clip_224": dict(img=224, patch=14, dim=1024, depth=24, heads=16, **_CLIP),
    "vit_large_patch14_clip_336": dict(img=336, patch=14, dim=1024, depth=24, heads=16, **_CLIP),
    # the same towers with QuickGELU in the MLP (the OpenAI ViT-B/32, B/16, L/14, L/14@336 weights; MetaCLIP, DFN): same keys and shapes
    "vit_base_patch32_clip_quickgelu_224": dict(img=224, patch=32, dim=768, depth=12, heads=12, **_CLIP, act="quick_gelu"),
    "vit_base_patch16_clip_quickgelu_224": dict(img=224, patch=16, dim=768, depth=12, heads=12, **_CLIP, act="quick_gelu"),
    "vit_large_patch14_clip_quickgelu_224": dict(img=224, patch=14, dim=1024, depth=24, heads=16, **_CLIP, act="quick_gelu"),
    "vit_large_patch14_clip_quickgelu_336": dict(img=336, patch=14, dim=1024, depth=24, heads=16, **_CLIP, act="quick_gelu"),
    "vit_small_patch14_dinov2": dict(img=518, patch=14, dim=384, depth=12, heads=6, init_values=1e-5),
    "vit_base_patch14_dinov2": dict(img=518, patch=14, dim=768, depth=12, heads=12, init_values=1e-5),
    "vit_large_patch14_dinov2": dict(img=518, patch=14, dim=1024, depth=24, heads=16, init_values=1e-5),
    "deit3_small_patch16_224": dict(img=224, patch=16, dim=384, depth=12, heads=6, **_DEIT3),
    "deit3_base_patch16_224": dict(img=224, patch=16, dim=768, depth=12, heads=12, **_DEIT3),
    "deit3_large_patch16_224": dict(img=224, patch=16, dim=1024, depth=24, heads=16, **_DEIT3),
    "vit_tiny_test": dict(img=64, patch=16, dim=128, depth=2, heads=2),   # reduced member for fast parity tests
    "vit_small_test": dict(img=64, patch=16, dim=256, depth=2, heads=4),  # reduced member inside the fp8 GEMM envelope (dim 256)
    "vit_tiny192_test": dict(img=64, patch=16, dim=192, depth=2, heads=3),       # reduced ViT-Tiny width (T = 17)
    "vit_tiny192_p32_test": dict(img=96, patch=32, dim=192, depth=1, heads=3),   # ... with 32-pixel patches (T = 10)
    "vit_clip_test": dict(img=64, patch=16, dim=128, depth=2, heads=2, **_CLIP),                  # reduced CLIP tower (T = 17)
    "vit_clip_quickgelu_test": dict(img=64, patch=16, dim=128, depth=2, heads=2, **_CLIP, act="quick_gelu"),     # ... with QuickGELU
    # the same inside the eight-phase (fc1 epilogue, act 9) and fp8 envelopes (dim 256)
    "vit_clip_quickgelu_f8_test": dict(img=64, patch=16, dim=256, depth=2, heads=4, **_CLIP, act="quick_gelu"),
    "vit_dinov2_test": dict(img=70, patch=14, dim=128, depth=2, heads=2, init_values=1e-5),       # reduced DINOv2 (T = 26)
    "deit3_test": dict(img=64, patch=16, dim=128, depth=2, heads=2, **_DEIT3),                    # reduced DeiT-III (T = 17)
    "vit_dinov2_long_test": dict(img=238, patch=14, dim=128, depth=1, heads=2, init_values=1e-5),  # T = 290: unfused attention
}
# DeiT (no distillation token) is the same module under timm's VisionTransformer keys: the names differ in the pretrained weights only
_ALIASES = {
    "deit_tiny_patch16_224": "vit_tiny_patch16_224",
    "deit_small_patch16_224": "vit_small_patch16_224",
    "deit_base_patch16_224": "vit_base_patch16_224",
}


def vit_members():
    """The names create_backbone answers for this family (reduced test members left out)."""
    return sorted(k for k in list(_VITS) + list(_ALIASES) if not k.endswith("_test"))


def create_vit(name: str):
    cfg = _VITS.get(_ALIASES.get(name, name))
    return HipViT(**cfg) if cfg else None
