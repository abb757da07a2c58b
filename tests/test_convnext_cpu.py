"""ConvNeXt family without a GPU: the parameter layout of get_model("convnext_base") against the twin of tests/convnext_reference.py,
the members that are refused, set_dropout's reach, the TorchScript export twin, and the host side of the new entry points
(nkb_dwconv, nkb_dwconv_wgrad, nkb_layer_scale: declared, exported, bound, and rejecting bad geometry before any launch)."""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from convnext_reference import ConvNeXtClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402

NEW = ["nkb_dwconv", "nkb_dwconv_wgrad", "nkb_dwconv_wgrad_workspace_floats", "nkb_layer_scale", "nkb_layer_scale_workspace_floats"]


def _cfg(name, drop=0.0):
    return dict(model=name, pretrained=False, backbone_dropout=drop, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def test_convnext_base_layout_equals_the_twin():
    model = get_model(_cfg("convnext_base"), ["a", "b"], "cpu")
    twin = ConvNeXtClassifier(_cfg("convnext_base"), ["a", "b"])
    sd, td = model.state_dict(), twin.state_dict()
    bb = {k: v for k, v in sd.items() if k.startswith("emb_model.")}
    assert len(bb) == 342
    assert sum(v.numel() for v in bb.values()) == 87_566_464
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    assert tuple(sd["emb_model.stages.2.blocks.26.conv_dw.weight"].shape) == (512, 1, 7, 7)
    assert tuple(sd["emb_model.stages.3.downsample.1.weight"].shape) == (1024, 512, 2, 2)
    assert torch.all(sd["emb_model.stages.0.blocks.0.gamma"] == 1e-6)
    model.load_state_dict(td)                               # both directions, strict
    twin.load_state_dict(model.state_dict())
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k
    assert model.emb_size == 1024 and model.emb_model.family == "convnext"


def test_members_outside_the_layernorm_widths_are_refused():
    for name in ("convnext_tiny", "convnext_small", "convnext_large"):
        with pytest.raises(NotImplementedError, match="multiples of 128"):
            get_model(_cfg(name), ["a", "b"], "cpu")
    with pytest.raises(NotImplementedError, match="convnext_base"):
        get_model(_cfg("no_such_backbone"), ["a", "b"], "cpu")


def test_set_dropout_reaches_every_site():
    model = get_model(_cfg("convnext_test", drop=0.1), ["a", "b"], "cpu")
    em = model.emb_model
    n = 0
    for st in em.stages:
        for blk in st.blocks:
            assert isinstance(blk.mlp.drop1, torch.nn.Dropout) and blk.mlp.drop1.p == 0.1
            assert isinstance(blk.mlp.drop2, torch.nn.Dropout) and blk.mlp.drop2.p == 0.1
            n += 1
    assert n == 5 and isinstance(em.head.drop, torch.nn.Dropout) and em.head.drop.p == 0.1
    model.set_dropout(em, 0.3)
    assert em.stages[2].blocks[1].mlp.drop2.p == 0.3 and em.head.drop.p == 0.3


def test_scripted_twin_reproduces_the_reference_twin():
    torch.manual_seed(0)
    twin = ConvNeXtClassifier(_cfg("convnext_test"), ["a", "b", "c"])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:                                # gamma = 1e-6 would silence every branch
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg("convnext_test"), ["a", "b", "c"], "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model))
    twin.eval()
    for shape in ((2, 3, 64, 64), (2, 3, 70, 73)):
        x = torch.randn(*shape, generator=g)
        with torch.no_grad():
            torch.testing.assert_close(scripted(x), twin(x))


def test_new_entry_points_are_declared_exported_and_bound():
    text = (ROOT / "include" / "nkbhip.h").read_text()
    assert "model.py:82" in text[text.index("nkb_dwconv") - 1200:text.index("nkb_dwconv")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(", text))
    lib = hip.load()
    ids = hip._plan_fn_ids()
    for name in NEW:
        assert name in declared and name in hip._SIGS and hasattr(lib, name), name
    for name in ("nkb_dwconv", "nkb_dwconv_wgrad", "nkb_layer_scale"):
        assert name in ids, name                            # recorded plans replay the new launches
    names = [lib.nkb_kernel_name(k) for k in range(32)]
    assert lib.nkb_kernel_name(0) == b"conv_igemm_fwd"      # appended, not inserted
    for k in (b"dwconv_fwd", b"dwconv_dgrad", b"dwconv_wgrad", b"layer_scale"):
        assert k in names
    assert lib.nkb_dwconv_wgrad_workspace_floats(1, 2, 56, 56, 128, 7) >= 50 * 128
    assert lib.nkb_dwconv_wgrad_workspace_floats(1, 2, 56, 56, 72, 7) == 0


_P = ctypes.c_void_p(64)


def _dw(dtype=1, dgrad=0, bias=None, N=1, H=8, W=8, C=128, ldx=128, ldy=128, R=7, pad=3):
    return (dtype, dgrad, None, None, bias, None, None, N, H, W, C, ldx, ldy, R, pad, None)


def _dww(dtype=1, N=1, H=8, W=8, C=128, ldg=128, ldx=128, R=7, pad=3, work=None, floats=0):
    return (dtype, None, None, None, None, N, H, W, C, ldg, ldx, R, pad, work, floats, None)


def _ls(dtype=1, backward=0, a=None, dgamma=None, rows=64, C=128, work=None, floats=0):
    return (dtype, backward, None, a, None, None, dgamma, rows, C, work, floats, None)


_REJECTIONS = [
    ("nkb_dwconv", _dw(dtype=7), b"dwconv: bad dtype 7"),
    ("nkb_dwconv", _dw(C=72, ldx=72, ldy=72), b"dwconv: C=72 must be a multiple of 64"),
    ("nkb_dwconv", _dw(N=1 << 14, H=64, W=64), b"dwconv: operand exceeds 2^31"),
    ("nkb_dwconv", _dw(ldy=64), b"must be >= C=128"),
    ("nkb_dwconv", _dw(R=5, pad=2), b"got R=5 pad=2"),
    ("nkb_dwconv", _dw(dgrad=1, bias=_P), b"the data gradient takes no bias"),
    ("nkb_dwconv_wgrad", _dww(dtype=7), b"dwconv_wgrad: bad dtype 7"),
    ("nkb_dwconv_wgrad", _dww(C=72, ldg=72, ldx=72), b"dwconv_wgrad: C=72 must be a multiple of 64"),
    ("nkb_dwconv_wgrad", _dww(N=1 << 14, H=64, W=64), b"dwconv_wgrad: operand exceeds 2^31"),
    ("nkb_dwconv_wgrad", _dww(), b"dwconv_wgrad: workspace of 0 floats given, 12800 needed"),
    ("nkb_dwconv_wgrad", _dww(work=_P, floats=100), b"dwconv_wgrad: workspace of 100 floats given, 12800 needed"),
    ("nkb_layer_scale", _ls(dtype=7), b"layer_scale: bad dtype 7"),
    ("nkb_layer_scale", _ls(C=72), b"layer_scale: C=72 must be a multiple of 64"),
    ("nkb_layer_scale", _ls(rows=1 << 24), b"outside 1 .. 2^31"),
    ("nkb_layer_scale", _ls(backward=1), b"backward needs the incoming gradient"),
    ("nkb_layer_scale", _ls(backward=1, a=_P, dgamma=_P, work=_P, floats=1), b"layer_scale: workspace of 1 floats given"),
]


@pytest.mark.parametrize("name,args,text", _REJECTIONS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(_REJECTIONS)])
def test_host_side_rejections_answer_without_a_launch(name, args, text):
    """Every call returns before it touches an operand (null / dummy pointers), with its message in nkb_last_error."""
    lib = hip.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0 and text in lib.nkb_last_error(), (name, rc, lib.nkb_last_error())
