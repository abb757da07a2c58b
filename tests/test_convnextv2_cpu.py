"""ConvNeXt V2 without a GPU: the parameter layout of get_model("convnextv2_base") against the twin of tests/convnextv2_reference.py,
the members that are refused, set_dropout's reach, the TorchScript export twin, the appended profiler names, and the host side of the
GRN passes of nkb_avgpool (modes NKB_GRN_*: bad geometry is refused before any launch)."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from convnextv2_reference import ConvNeXtV2Classifier  # noqa: E402
from nkb_classification import cabi, hip  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402


def _cfg(name, drop=0.0):
    return dict(model=name, pretrained=False, backbone_dropout=drop, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def test_convnextv2_base_layout_equals_the_twin():
    model = get_model(_cfg("convnextv2_base"), ["a", "b"], "cpu")
    twin = ConvNeXtV2Classifier(_cfg("convnextv2_base"), ["a", "b"])
    sd, td = model.state_dict(), twin.state_dict()
    bb = {k: v for k, v in sd.items() if k.startswith("emb_model.")}
    assert len(bb) == 378                                    # convnext_base's 342 - 36 gammas + 72 GRN vectors
    assert sum(v.numel() for v in bb.values()) == 87_692_800  # timm's published 88 717 800 minus the 1 025 000-element fc
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    assert not [k for k in sd if k.endswith(".gamma")]
    grn_keys = [k for k in sd if ".mlp.grn." in k]
    assert len(grn_keys) == 72
    for si, C in enumerate((128, 256, 512, 1024)):
        for leaf in ("weight", "bias"):
            v = sd[f"emb_model.stages.{si}.blocks.0.mlp.grn.{leaf}"]
            assert tuple(v.shape) == (4 * C,) and torch.all(v == 0)
    keys = list(sd)
    i = keys.index("emb_model.stages.2.blocks.26.mlp.grn.weight")
    assert keys[i - 1].endswith("blocks.26.mlp.fc1.bias") and keys[i + 2].endswith("blocks.26.mlp.fc2.weight")
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, v in twin.state_dict().items():
            if ".grn." in k:
                v.copy_(torch.rand(v.shape, generator=g))
    td = twin.state_dict()
    model.load_state_dict(td)                               # both directions, strict
    twin.load_state_dict(model.state_dict())
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k
    assert model.emb_size == 1024 and model.emb_model.family == "convnext" and model.emb_model.use_grn
    assert model.emb_model.fp8_linears() == []


def test_v1_members_keep_their_layout():
    em = get_model(_cfg("convnext_test"), ["a", "b"], "cpu").emb_model
    assert not em.use_grn and hasattr(em.stages[0].blocks[0], "gamma") and not hasattr(em.stages[0].blocks[0].mlp, "grn")


@pytest.mark.parametrize("name", ["convnextv2_atto", "convnextv2_femto", "convnextv2_pico", "convnextv2_nano", "convnextv2_tiny",
                                  "convnextv2_large", "convnextv2_huge"])
def test_other_v2_members_are_refused(name):
    with pytest.raises(NotImplementedError, match="multiples of 128") as e:
        get_model(_cfg(name), ["a", "b"], "cpu")
    assert "convnextv2_base" in str(e.value) and "convnext_base" in str(e.value)


def test_unknown_backbone_lists_both_generations():
    with pytest.raises(NotImplementedError, match="convnext_base") as e:
        get_model(_cfg("no_such_backbone"), ["a", "b"], "cpu")
    assert "convnextv2_base" in str(e.value)


def test_set_dropout_reaches_every_site():
    model = get_model(_cfg("convnextv2_test", drop=0.1), ["a", "b"], "cpu")
    em = model.emb_model
    n = 0
    for st in em.stages:
        for blk in st.blocks:
            assert isinstance(blk.mlp.drop1, torch.nn.Dropout) and blk.mlp.drop1.p == 0.1
            assert isinstance(blk.mlp.drop2, torch.nn.Dropout) and blk.mlp.drop2.p == 0.1
            n += 1
    assert n == 5 and isinstance(em.head.drop, torch.nn.Dropout) and em.head.drop.p == 0.1
    model.set_dropout(em, 0.3)
    assert em.stages[2].blocks[1].mlp.drop1.p == 0.3 and em.stages[2].blocks[1].mlp.drop2.p == 0.3 and em.head.drop.p == 0.3


def test_scripted_twin_reproduces_the_reference_twin():
    torch.manual_seed(0)
    twin = ConvNeXtV2Classifier(_cfg("convnextv2_test"), ["a", "b", "c"])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if p.dim() == 1:                                # grn.weight = grn.bias = 0 would make the operator the identity
                p.copy_(torch.rand(p.shape, generator=g) * (2.0 if ".grn." in name else 0.5) + (-1.0 if ".grn." in name else 0.5))
    model = get_model(_cfg("convnextv2_test"), ["a", "b", "c"], "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model))
    assert any(k.endswith("mlp.grn.weight") for k in scripted.state_dict())
    twin.eval()
    for shape in ((2, 3, 64, 64), (2, 3, 70, 73)):
        x = torch.randn(*shape, generator=g)
        with torch.no_grad():
            torch.testing.assert_close(scripted(x), twin(x))


def test_kernel_names_are_appended_and_the_modes_are_in_the_header():
    lib = hip.load()
    names = [lib.nkb_kernel_name(k) for k in range(32)]
    assert names[0] == b"conv_igemm_fwd" and names[21] == b"layer_scale" and names[24] == b"avgpool2x2"
    assert names[25:28] == [b"grn_reduce", b"grn_apply", b"grn_param"] and names[28] == b"?"
    modes = cabi.parse_enum(cabi.header_text(), "NkbPoolMode")
    assert modes == {"NKB_POOL_AVG_FWD": 0, "NKB_POOL_AVG_BWD": 1, "NKB_GRN_FWD_REDUCE": 2, "NKB_GRN_FWD_APPLY": 3,
                     "NKB_GRN_BWD_REDUCE": 4, "NKB_GRN_BWD_APPLY": 5, "NKB_GRN_PARAM": 6}
    assert "nkb_avgpool" in hip._plan_fn_ids()              # recorded plans replay the GRN launches
    assert len(hip._SIGS["nkb_avgpool"][1]) == 18
    assert hip.grn_workspace(3, 49, 4096) == 2 * 3 * 4096 + 3


_P = ctypes.c_void_p(64)
f32 = ctypes.c_float


def _grn(mode, dtype=1, inp=_P, out=_P, N=2, HW=49, C=512, in2=_P, weight=_P, bias=_P, sumsq=_P, dweight=_P, dbias=_P, mul=None,
         eps=1e-6, work=_P, floats=1 << 20):
    return (dtype, mode, inp, out, N, HW, C, in2, weight, bias, sumsq, dweight, dbias, mul, f32(eps), work, floats, None)


_REJECTIONS = [
    (_grn(7), b"avgpool: bad mode 7"),
    (_grn(-1), b"avgpool: bad mode -1"),
    (_grn(2, dtype=7), b"grn: bad dtype 7"),
    (_grn(3, C=72), b"grn: C=72 must be a multiple of 64 up to 4096"),
    (_grn(3, C=8192), b"grn: C=8192 must be a multiple of 64 up to 4096"),
    (_grn(2, N=1 << 10, HW=1 << 10, C=2048), b"outside 1 .. 2^31 elements"),
    (_grn(2, HW=0), b"outside 1 .. 2^31 elements"),
    (_grn(3, eps=0.0), b"grn: eps=0 must be positive"),
    (_grn(2, sumsq=None), b"grn: mode 2 needs the sum-of-squares table"),
    (_grn(6, sumsq=None), b"grn: mode 6 needs the sum-of-squares table"),
    (_grn(2, inp=None), b"grn: mode 2 needs its input tensor"),
    (_grn(4, in2=None), b"grn: mode 4 needs the forward input next to the gradient"),
    (_grn(5, in2=None), b"grn: mode 5 needs the forward input next to the gradient"),
    (_grn(3, bias=None), b"grn: mode 3 needs out, weight and bias"),
    (_grn(3, out=None), b"grn: mode 3 needs out, weight and bias"),
    (_grn(5, weight=None), b"grn: mode 5 needs out, weight"),
    (_grn(6, dweight=None, dbias=None), b"grn: the parameter pass needs dweight or dbias"),
    (_grn(4, work=None, floats=0), b"grn: workspace of 0 floats given, 2050 needed"),
    (_grn(5, floats=2049), b"grn: workspace of 2049 floats given, 2050 needed"),
    (_grn(6, floats=100), b"grn: workspace of 100 floats given, 2050 needed"),
]


@pytest.mark.parametrize("args,text", _REJECTIONS, ids=[f"grn-{i}" for i in range(len(_REJECTIONS))])
def test_host_side_rejections_answer_without_a_launch(args, text):
    """Every call returns before it touches an operand (null / dummy pointers), with its message in nkb_last_error."""
    lib = hip.load()
    rc = lib.nkb_avgpool(*args)
    assert rc != 0 and text in lib.nkb_last_error(), (rc, lib.nkb_last_error())
