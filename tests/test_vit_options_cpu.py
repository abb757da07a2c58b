"""The CLIP, DINOv2 and DeiT-III ViT members without a GPU: every member resolves, its parameter layout and count equal the twin of
tests/vit_options_reference.py (our own restatement of timm's layout; timm is not installed, so parity with it is unpinned) and the
issue's table, the per-option keys and shapes are there, the TorchScript twin of each reduced member gives the reference twin's eval
logits, and the plain members and the unknown-name refusal are as they were."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from vit_options_reference import MEMBERS, REDUCED, ViTClassifier  # noqa: E402
from nkb_classification.model import SingletaskClassifier, get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402

CLASSES = ["a", "b", "c"]


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _formula(img, patch, dim, depth, pre_norm=False, ln_eps=1e-6, init_values=None, no_embed_class=False):
    """Counted by hand from the layout: patch projection (bias unless pre_norm), class token, position embedding (one row less with
    no_embed_class), norm_pre, per block 12 D^2 + 13 D (+ 2 D of LayerScale), final norm."""
    n = (img // patch) ** 2
    total = 3 * patch * patch * dim + (0 if pre_norm else dim) + dim + (n if no_embed_class else n + 1) * dim
    total += 2 * dim if pre_norm else 0
    total += depth * (12 * dim * dim + 13 * dim + (2 * dim if init_values is not None else 0))
    return total + 2 * dim


@pytest.fixture(scope="module")
def built():
    """(model, twin) per member, built once.  The 768- and 1024-wide members are built on the meta device: keys, shapes and counts
    without allocating or initialising up to 304 M parameters twice; values are checked on the 384-wide and reduced members."""
    cache = {}

    def get(name):
        if name not in cache:
            torch.manual_seed(0)
            if MEMBERS[name][2] >= 768:
                with torch.device("meta"):
                    cache[name] = (SingletaskClassifier(_cfg(name), CLASSES), ViTClassifier(name, len(CLASSES)))
            else:
                cache[name] = (get_model(_cfg(name), CLASSES, "cpu"), ViTClassifier(name, len(CLASSES)))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(MEMBERS))
def test_member_layout_equals_the_twin_and_the_table(name, built):
    img, patch, dim, depth, heads, opts, count = MEMBERS[name]
    model, twin = built(name)
    sd, td = model.state_dict(), twin.state_dict()
    n = sum(v.numel() for k, v in sd.items() if k.startswith("emb_model."))
    assert n == _formula(img, patch, dim, depth, **opts)
    if count is not None:
        assert n == count
    assert model.emb_size == dim and model.emb_model.family == "vit" and model.emb_model.heads == heads
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    assert tuple(sd["emb_model.patch_embed.proj.weight"].shape) == (dim, 3, patch, patch)
    ntok = (img // patch) ** 2
    # per option
    if opts.get("pre_norm"):
        assert tuple(sd["emb_model.norm_pre.weight"].shape) == (dim,) and tuple(sd["emb_model.norm_pre.bias"].shape) == (dim,)
        assert "emb_model.patch_embed.proj.bias" not in sd
        assert model.emb_model.norm_pre.eps == 1e-5 and model.emb_model.norm.eps == 1e-5
        assert model.emb_model.blocks[0].norm1.eps == 1e-5 and model.emb_model.blocks[depth - 1].norm2.eps == 1e-5
    else:
        assert "emb_model.norm_pre.weight" not in sd and "emb_model.patch_embed.proj.bias" in sd
        assert model.emb_model.norm.eps == 1e-6 and model.emb_model.blocks[0].norm1.eps == 1e-6
    if opts.get("init_values") is not None:
        for i in range(depth):
            for ls in ("ls1", "ls2"):
                g = sd[f"emb_model.blocks.{i}.{ls}.gamma"]
                assert tuple(g.shape) == (dim,) and (g.is_meta or torch.equal(g, torch.full((dim,), opts["init_values"])))
    else:
        assert not any(".ls1." in k or ".ls2." in k for k in sd)
    assert tuple(sd["emb_model.pos_embed"].shape) == ((1, ntok, dim) if opts.get("no_embed_class") else (1, ntok + 1, dim))
    assert tuple(sd["emb_model.cls_token"].shape) == (1, 1, dim)


@pytest.mark.parametrize("name", ["vit_small_patch14_dinov2", "deit3_small_patch16_224"] + REDUCED)
def test_state_dicts_load_strictly_in_both_directions(name, built):
    model, twin = built(name)
    td = {k: v.clone() for k, v in twin.state_dict().items()}
    model.load_state_dict(td, strict=True)
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k
    twin.load_state_dict(model.state_dict(), strict=True)


def test_deit3_position_embedding_covers_the_patch_tokens_only(built):
    for name, dim in (("deit3_small_patch16_224", 384), ("deit3_base_patch16_224", 768), ("deit3_large_patch16_224", 1024)):
        assert tuple(built(name)[0].state_dict()["emb_model.pos_embed"].shape) == (1, 196, dim)
        assert built(name)[0].emb_model.n_tokens == 197


@pytest.mark.parametrize("name", REDUCED)
def test_scripted_twin_matches_the_reference_twin_in_eval(name):
    """scripted_last.pt of a new member reproduces its eval logits: 1-D parameters (LayerNorm, LayerScale, biases) are randomised so
    that every option shows in the logits."""
    torch.manual_seed(0)
    twin = ViTClassifier(name, len(CLASSES)).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg(name), CLASSES, "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model)).eval()
    hw = MEMBERS[name][0]
    x = torch.randn(2, 3, hw, hw)
    with torch.no_grad():
        torch.testing.assert_close(scripted(x), twin(x), rtol=1e-5, atol=1e-5)


def test_key_list_of_vit_base_patch16_224_is_unchanged():
    """Defaults reproduce the module as it was: the keys of oracle.torch_models.VisionTransformer, no option's key among them."""
    from oracle.torch_models import VisionTransformer
    model = get_model(_cfg("vit_base_patch16_224"), CLASSES, "cpu")
    keys = [k[len("emb_model."):] for k in model.state_dict() if k.startswith("emb_model.")]
    assert keys == list(VisionTransformer().state_dict())
    assert len(keys) == 4 + 12 * 12 + 2
    assert not any("norm_pre" in k or ".ls" in k for k in keys)
    em = model.emb_model
    assert (em.pre_norm, em.ln_eps, em.init_values, em.no_embed_class) == (False, 1e-6, None, False)
    assert tuple(em.pos_embed.shape) == (1, 197, 768) and em.patch_embed.proj.bias is not None


def test_unknown_name_still_raises_and_lists_the_new_members():
    from nkb_classification.vit import vit_members
    with pytest.raises(NotImplementedError) as e:
        get_model(_cfg("vit_so400m_patch14_siglip_224"), CLASSES, "cpu")
    text = str(e.value)
    for name in MEMBERS:
        assert (name in text) == (not name.endswith("_test")), name
        assert (name in vit_members()) == (not name.endswith("_test")), name
    assert "vit_base_patch16_224" in text and "convnext_base" in text
