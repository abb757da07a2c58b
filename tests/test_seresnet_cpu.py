"""SE / ECA ResNet members without a GPU: the parameter layout of get_model("seresnet50" ...) against the twin of
tests/seresnet_reference.py, the parameter counts, rd / k per stage, what stays refused, the TorchScript export twin, and the host side of
the channel-attention passes of nkb_avgpool (modes NKB_SE_* / NKB_ECA_*: bad geometry is refused before any launch)."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from seresnet_reference import FULL, SERESNETS, TINY, SEResNetClassifier, eca_k, se_rd  # noqa: E402
from nkb_classification import cabi, hip  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402

COUNTS = {"seresnet50": 26_039_024, "seresnet18": 11_266_624, "ecaresnet50d": 23_527_350}
MODES = {"NKB_SE_POOL": 16, "NKB_SE_GATE": 17, "NKB_ECA_GATE": 18, "NKB_SE_FWD_APPLY": 19, "NKB_SE_BWD_REDUCE": 20,
         "NKB_SE_BWD_GATE": 21, "NKB_ECA_BWD_GATE": 22, "NKB_SE_BWD_APPLY": 23}


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


@pytest.mark.parametrize("name", sorted(SERESNETS))
def test_layout_equals_the_twin(name):
    spec = SERESNETS[name]
    model = get_model(_cfg(name), ["a", "b"], "cpu")
    twin = SEResNetClassifier(_cfg(name), ["a", "b"])
    sd, td = model.state_dict(), twin.state_dict()
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    if name in COUNTS:
        assert sum(p.numel() for p in model.emb_model.parameters()) == COUNTS[name]
    # the block's keys: ... last BatchNorm, se.*, downsample.*
    keys = [k for k in sd if k.startswith("emb_model.layer2.0.")]
    last = "bn3" if spec["bottleneck"] else "bn2"
    i = keys.index(f"emb_model.layer2.0.{last}.num_batches_tracked")
    assert keys[i + 1].startswith("emb_model.layer2.0.se.")
    j = max(n for n, k in enumerate(keys) if ".se." in k)
    assert keys[j + 1].startswith("emb_model.layer2.0.downsample.")
    exp = 4 if spec["bottleneck"] else 1
    em = model.emb_model
    for li, planes in enumerate((64, 128, 256, 512)):
        C = planes * exp
        for blk in getattr(em, f"layer{li + 1}"):
            if spec["attn"] == "se":
                assert tuple(blk.se.fc1.weight.shape) == (se_rd(C), C, 1, 1) and tuple(blk.se.fc1.bias.shape) == (se_rd(C),)
                assert tuple(blk.se.fc2.weight.shape) == (C, se_rd(C), 1, 1) and tuple(blk.se.fc2.bias.shape) == (C,)
            else:
                k = eca_k(C)
                assert tuple(blk.se.conv.weight.shape) == (1, 1, k) and blk.se.conv.padding == ((k - 1) // 2,) and blk.se.conv.bias is None
                assert blk.se.conv.padding_mode == "zeros"
    if "stem" in spec:
        assert tuple(sd["emb_model.conv1.0.weight"].shape) == (spec["stem"][0], 3, 3, 3) and "emb_model.layer2.0.downsample.1.weight" in sd
    else:
        assert tuple(sd["emb_model.conv1.weight"].shape) == (64, 3, 7, 7) and "emb_model.layer2.0.downsample.0.weight" in sd
    assert torch.all(sd[f"emb_model.layer3.0.{last}.weight"] == 0)      # zero_init_last
    model.load_state_dict(td)                               # both directions, strict
    twin.load_state_dict(model.state_dict())
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k
    assert model.emb_size == 512 * exp and em.family == "resnet"
    # the attention weights are fp32 masters of csrc/se.hip: no data-gradient filter, no GEMM
    gemm = {id(c.weight) for c in em.gemm_convs()} | {id(c.weight) for c in em.stem_convs()}
    se_params = [p for n, p in em.named_parameters() if ".se." in n]
    assert se_params and not any(id(p) in gemm for p in se_params)
    assert len(em.gemm_convs()) == len([k for k in sd if k.startswith("emb_model.layer") and k.endswith(".weight") and sd[k].dim() == 4
                                        and ".se." not in k]) + (2 if "stem" in spec else 0)


def test_rd_and_k_tables():
    assert [se_rd(c) for c in (64, 128, 256, 512, 1024, 2048)] == [8, 8, 16, 32, 64, 128]
    assert [eca_k(c) for c in (256, 512, 1024, 2048)] == [5, 5, 5, 7]
    em = get_model(_cfg("seresnet50"), ["a", "b"], "cpu").emb_model
    assert [getattr(em, f"layer{i}")[0].se.fc1.out_channels for i in (1, 2, 3, 4)] == [16, 32, 64, 128]
    em = get_model(_cfg("seresnet18"), ["a", "b"], "cpu").emb_model
    assert [getattr(em, f"layer{i}")[0].se.fc1.out_channels for i in (1, 2, 3, 4)] == [8, 8, 16, 32]
    em = get_model(_cfg("ecaresnet50d"), ["a", "b"], "cpu").emb_model
    assert [getattr(em, f"layer{i}")[0].se.conv.kernel_size[0] for i in (1, 2, 3, 4)] == [5, 5, 5, 7]


def test_unknown_name_message_and_what_stays_refused():
    with pytest.raises(NotImplementedError, match="resnet14t") as e:
        get_model(_cfg("no_such_backbone"), ["a", "b"], "cpu")
    text = str(e.value)
    for name in FULL:
        assert repr(name) in text, name
    for name in TINY:
        assert name not in text, name
    for name in ("mobilenetv3_large_100", "seresnext50_32x4d", "seresnet200d", "ecaresnetlight", "convnextv2_tiny"):
        with pytest.raises(NotImplementedError):
            get_model(_cfg(name), ["a", "b"], "cpu")
    plain = get_model(_cfg("resnet_tiny_bottleneck"), ["a", "b"], "cpu").emb_model
    assert not hasattr(plain.layer1[0], "se")


@pytest.mark.parametrize("name", TINY + ("ecaresnet26t",))
def test_scripted_twin_reproduces_the_reference_twin(name):
    torch.manual_seed(0)
    twin = SEResNetClassifier(_cfg(name), ["a", "b", "c"])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:                                # zero_init_last would silence every residual branch and the operator with it
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
        for n, b in twin.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
    model = get_model(_cfg(name), ["a", "b", "c"], "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model))
    assert any(".se." in k for k in scripted.state_dict())
    twin.eval()
    for shape in ((2, 3, 64, 64), (2, 3, 70, 73)):
        x = torch.randn(*shape, generator=g)
        with torch.no_grad():
            torch.testing.assert_close(scripted(x), twin(x))


def test_the_modes_are_in_the_header_and_the_surface_is_unchanged():
    modes = cabi.parse_enum(cabi.header_text(), "NkbSeMode")
    for name, value in MODES.items():
        assert modes.get(name) == value, name
    assert hip._SE_MODES == modes
    assert not set(modes.values()) & set(cabi.parse_enum(cabi.header_text(), "NkbPoolMode").values())
    assert "nkb_avgpool" in hip._plan_fn_ids()              # recorded plans replay the new launches
    assert len(hip._SIGS["nkb_avgpool"][1]) == 18
    assert hip.se_workspace(3, 2048, 128) == 6 * 3 * 2048 + 2 * 2048 + 512 + 2 * 3 * 128 and hip.se_workspace(2, 256) == 6 * 2 * 256 + 512 + 64


_P = ctypes.c_void_p(64)
f32 = ctypes.c_float


def _se(mode, dtype=1, inp=_P, out=_P, N=2, HW=49, C=512, in2=_P, weight=_P, bias=_P, sumsq=_P, dweight=_P, dbias=_P, mul=_P, work=_P,
        floats=1 << 24):
    return (dtype, MODES[mode], inp, out, N, HW, C, in2, weight, bias, sumsq, dweight, dbias, mul, f32(0.0), work, floats, None)


_BIG = ("NKB_SE_POOL", "NKB_SE_FWD_APPLY", "NKB_SE_BWD_REDUCE", "NKB_SE_BWD_APPLY")
_REJECTIONS = [(_se(m, C=96, HW=(32 if "GATE" in m else 49)), b"se: C=96 must be a multiple of 64 up to 2048") for m in MODES]
_REJECTIONS += [(_se(m, C=4096, HW=(32 if "GATE" in m else 49)), b"se: C=4096 must be a multiple of 64 up to 2048") for m in MODES]
_REJECTIONS += [(_se(m, dtype=7), b"se: bad dtype 7") for m in MODES]
_REJECTIONS += [(_se(m, HW=12), b"se: rd=12 must be a multiple of 8 up to 128") for m in ("NKB_SE_GATE", "NKB_SE_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=136), b"se: rd=136 must be a multiple of 8 up to 128") for m in ("NKB_SE_GATE", "NKB_SE_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=4), b"se: k=4 must be odd, 1 .. 9") for m in ("NKB_ECA_GATE", "NKB_ECA_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=11), b"se: k=11 must be odd, 1 .. 9") for m in ("NKB_ECA_GATE", "NKB_ECA_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=0), b"outside 1 .. 2^31 elements") for m in _BIG]
_REJECTIONS += [(_se(m, N=1 << 10, HW=1 << 10, C=2048), b"outside 1 .. 2^31 elements") for m in _BIG]
_REJECTIONS += [(_se(m, floats=6 * 2 * 512 + 2 * 512 + 128 - 1), b"workspace of 7295 floats given, 7296 needed") for m in _BIG]
_REJECTIONS += [(_se(m, HW=5, floats=7295), b"workspace of 7295 floats given, 7296 needed") for m in ("NKB_ECA_GATE", "NKB_ECA_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=32, floats=7296 + 2 * 2 * 32 - 1), b"workspace of 7423 floats given, 7424 needed")
                for m in ("NKB_SE_GATE", "NKB_SE_BWD_GATE")]
_REJECTIONS += [(_se(m, HW=(32 if "SE_" in m and "GATE" in m else 5 if "GATE" in m else 49), work=None, floats=0),
                 b"workspace of 0 floats given") for m in MODES]
_REJECTIONS += [
    (_se("NKB_SE_POOL", inp=None), b"se: mode 16 needs its input tensor"),
    (_se("NKB_SE_GATE", HW=32, inp=None), b"se: mode 17 needs W1 (in), W2 (in2), b1 (bias) and b2 (mul)"),
    (_se("NKB_SE_GATE", HW=32, in2=None), b"se: mode 17 needs W1"),
    (_se("NKB_SE_GATE", HW=32, bias=None), b"se: mode 17 needs W1"),
    (_se("NKB_SE_GATE", HW=32, mul=None), b"se: mode 17 needs W1"),
    (_se("NKB_ECA_GATE", HW=5, inp=None), b"se: mode 18 needs the taps (in)"),
    (_se("NKB_SE_FWD_APPLY", inp=None), b"se: mode 19 needs in, in2 and out"),
    (_se("NKB_SE_FWD_APPLY", in2=None), b"se: mode 19 needs in, in2 and out"),
    (_se("NKB_SE_FWD_APPLY", out=None), b"se: mode 19 needs in, in2 and out"),
    (_se("NKB_SE_BWD_REDUCE", inp=None), b"se: mode 20 needs its input tensor"),
    (_se("NKB_SE_BWD_REDUCE", in2=None), b"se: the backward reduction needs c (in2) and the ReLU bits"),
    (_se("NKB_SE_BWD_REDUCE", sumsq=None), b"se: the backward reduction needs c (in2) and the ReLU bits"),
    (_se("NKB_SE_BWD_GATE", HW=32, inp=None), b"se: mode 21 needs W1 (in) and W2 (in2)"),
    (_se("NKB_SE_BWD_GATE", HW=32, in2=None), b"se: mode 21 needs W1 (in) and W2 (in2)"),
    (_se("NKB_SE_BWD_GATE", HW=32, out=None), b"se: dW1 (out) and dW2 (dweight) come together or not at all"),
    (_se("NKB_ECA_BWD_GATE", HW=5, inp=None), b"se: mode 22 needs the taps (in)"),
    (_se("NKB_SE_BWD_APPLY", out=None), b"se: mode 23 needs in, in2 and out"),
    (_se("NKB_SE_BWD_APPLY", weight=None), b"se: the backward apply needs the BatchNorm vectors"),
    (_se("NKB_SE_BWD_APPLY", sumsq=None), b"se: the backward apply needs the BatchNorm vectors"),
    (_se("NKB_SE_GATE", HW=32, N=0), b"se: N=0 must be positive"),
]


@pytest.mark.parametrize("args,text", _REJECTIONS, ids=[f"se-{i}" for i in range(len(_REJECTIONS))])
def test_host_side_rejections_answer_without_a_launch(args, text):
    """Every call returns before it touches an operand (null / dummy pointers), with its message in nkb_last_error."""
    lib = hip.load()
    rc = lib.nkb_avgpool(*args)
    assert rc != 0 and text in lib.nkb_last_error(), (rc, lib.nkb_last_error())
