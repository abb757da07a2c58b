"""The ViT-Tiny, patch-32, 384-px and DeiT members without a GPU: parameter layout and counts of get_model(name) against
oracle.torch_models.VisionTransformer (our own restatement of timm's layout; timm is not installed, so parity with it is unpinned),
the TorchScript twin of the reduced 192-wide member, and the host side of nkb_layernorm / nkb_layernorm_param_reduce at the widths
they now take (any D % 8 == 0 up to 2048) and still refuse — answered before any launch."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from vit_members_reference import MEMBERS, ViTClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402

CLASSES = ["a", "b", "c"]


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _formula(img, patch, dim, depth):
    T = (img // patch) ** 2 + 1
    return 3 * patch * patch * dim + dim + dim + T * dim + depth * (12 * dim * dim + 13 * dim) + 2 * dim


@pytest.mark.parametrize("name", list(MEMBERS))
def test_member_layout_equals_the_oracle_twin(name):
    img, patch, dim, depth, heads, count = MEMBERS[name]
    model = get_model(_cfg(name), CLASSES, "cpu")
    twin = ViTClassifier(name, len(CLASSES))
    sd, td = model.state_dict(), twin.state_dict()
    bb = {k: v for k, v in sd.items() if k.startswith("emb_model.")}
    n = sum(v.numel() for v in bb.values())
    assert n == _formula(img, patch, dim, depth)
    if count is not None:
        assert n == count
    assert model.emb_size == dim and model.emb_model.family == "vit"
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    T = (img // patch) ** 2 + 1
    assert tuple(sd["emb_model.pos_embed"].shape) == (1, T, dim)
    assert tuple(sd["emb_model.patch_embed.proj.weight"].shape) == (dim, 3, patch, patch)
    assert tuple(sd["emb_model.blocks.0.attn.qkv.weight"].shape) == (3 * dim, dim) and model.emb_model.heads == heads
    model.load_state_dict(td)                               # both directions, strict
    twin.load_state_dict(model.state_dict())
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k


def test_deit_names_are_the_vit_members():
    """DeiT without a distillation token is timm's VisionTransformer under another name: same configuration, same keys."""
    from nkb_classification import vit
    for deit, name in (("deit_tiny_patch16_224", "vit_tiny_patch16_224"), ("deit_small_patch16_224", "vit_small_patch16_224"),
                       ("deit_base_patch16_224", "vit_base_patch16_224")):
        assert vit._ALIASES[deit] == name and name in vit._VITS and deit not in vit._VITS
        assert MEMBERS[deit][:5] == tuple(vit._VITS[name][k] for k in ("img", "patch", "dim", "depth", "heads"))


def test_unknown_backbone_message_lists_the_real_members():
    with pytest.raises(NotImplementedError) as e:
        get_model(_cfg("vit_huge_patch14_224"), CLASSES, "cpu")
    text = str(e.value)
    for name in MEMBERS:
        assert (name in text) == (not name.endswith("_test")), name
    for name in ("resnet14t", "convnext_base", "vit_small_patch16_224", "vit_base_patch16_224", "vit_large_patch16_224"):
        assert name in text, name


def test_scripted_twin_of_the_192_wide_member_matches_eval_logits():
    torch.manual_seed(0)
    twin = ViTClassifier("vit_tiny192_test", len(CLASSES)).eval()
    model = get_model(_cfg("vit_tiny192_test"), CLASSES, "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model)).eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        torch.testing.assert_close(scripted(x), twin(x), rtol=1e-5, atol=1e-5)


_P = ctypes.c_void_p(64)


def _ln(dtype=1, backward=0, D=192, in_stride=None, x_stride=None, out_stride=None, yq=None, q_state=None, q_kind=0):
    s = lambda v: D if v is None else v
    return (dtype, backward, None, s(in_stride), None, s(x_stride), None, None, None, None, None, None, s(out_stride), None, None,
            16, D, 1e-6, None, yq, q_state, q_kind, None, 0, None, None)


_REJECTIONS = [
    ("nkb_layernorm", _ln(D=100), b"layernorm: D=100 must be a multiple of 8"),
    ("nkb_layernorm", _ln(D=4), b"layernorm: D=4 must be a multiple of 8"),
    ("nkb_layernorm", _ln(D=2056), b"layernorm: D=2056 must be a multiple of 8"),
    ("nkb_layernorm", _ln(dtype=0, backward=1, D=2056), b"layernorm: D=2056"),
    ("nkb_layernorm", _ln(D=192, in_stride=194), b"in_stride=194"),
    ("nkb_layernorm", _ln(D=192, backward=1, out_stride=198), b"out_stride=198"),
    ("nkb_layernorm", _ln(D=192, yq=_P, q_state=_P), b"D % 256 == 0"),
    ("nkb_layernorm", _ln(D=192, backward=1, yq=_P, q_kind=2), b"D % 256 == 0"),
    ("nkb_layernorm_param_reduce", (_P, 16, 100, 2, _P, _P, None, None), b"D=100"),
    ("nkb_layernorm_param_reduce", (_P, 16, 2056, 2, _P, _P, None, None), b"D=2056"),
]


@pytest.mark.parametrize("name,args,text", _REJECTIONS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(_REJECTIONS)])
def test_host_side_rejections_answer_without_a_launch(name, args, text):
    """Every call returns before it touches an operand (null / dummy pointers), with its message in nkb_last_error."""
    lib = hip.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0 and text in lib.nkb_last_error(), (name, rc, lib.nkb_last_error())


def test_workspace_formula_is_unchanged():
    lib = hip.load()
    for D in (8, 192, 768, 2040):
        assert lib.nkb_layernorm_workspace_floats(D) == 2048 * 2 * D
