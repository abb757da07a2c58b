"""ResNet-D/T members without a GPU: the parameter layout of get_model("resnet14t" ...) against the twin of tests/resnet_dt_reference.py,
the TorchScript export twin (deep stem, avg_down with ceil_mode and partial windows), and the host side of the new entry points
(nkb_stem3_tiles, nkb_stem3_conv, nkb_avgpool2x2: declared, exported, bound, in the plan table, refusing bad geometry before any launch)."""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from resnet_dt_reference import RESNETS_DT, ResNetDTClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402

NEW = ["nkb_stem3_tiles", "nkb_stem3_conv", "nkb_avgpool2x2"]
# name: (backbone parameters, state-dict entries of the backbone); the first four are the issue's table (timm's published totals minus
# the 1000-class fc), the other D members were counted from the same layout
COUNTS = {"resnet14t": (8_032_632, 114), "resnet26t": (13_962_872, 186), "resnet26d": (13_965_408, 186),
          "resnet50d": (23_527_264, 330)}


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


@pytest.mark.parametrize("name", sorted(RESNETS_DT))
def test_layout_equals_the_twin(name):
    model = get_model(_cfg(name), ["a", "b"], "cpu")
    twin = ResNetDTClassifier(_cfg(name), ["a", "b"])
    sd, td = model.state_dict(), twin.state_dict()
    assert list(sd) == list(td)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in td.items()}
    bb = {k: v for k, v in sd.items() if k.startswith("emb_model.")}
    if name in COUNTS:
        nparam = sum(p.numel() for p in model.emb_model.parameters())
        assert (nparam, len(bb)) == COUNTS[name]
    c1, c2 = RESNETS_DT[name]["stem"]
    assert tuple(sd["emb_model.conv1.0.weight"].shape) == (c1, 3, 3, 3)
    assert tuple(sd["emb_model.conv1.3.weight"].shape) == (c2, c1, 3, 3)
    assert tuple(sd["emb_model.conv1.6.weight"].shape) == (64, c2, 3, 3)
    for k in ("conv1.1.weight", "conv1.1.running_var", "conv1.4.bias", "bn1.running_mean", "layer2.0.downsample.1.weight",
              "layer2.0.downsample.2.running_mean", "layer1.0.downsample.1.weight"):
        if "layer1.0.downsample" in k and not RESNETS_DT[name]["bottleneck"]:
            continue                                        # BasicBlock layer1 keeps 64 channels: identity shortcut
        assert "emb_model." + k in sd, k
    assert not any(".downsample.0." in k for k in sd)       # index 0 (pool / Identity) holds no parameters
    assert tuple(sd["emb_model.layer2.0.downsample.1.weight"].shape)[2:] == (1, 1)
    last = "bn3" if RESNETS_DT[name]["bottleneck"] else "bn2"
    assert torch.all(sd[f"emb_model.layer3.0.{last}.weight"] == 0)      # zero_init_last
    model.load_state_dict(td)                               # both directions, strict
    twin.load_state_dict(model.state_dict())
    for k in td:
        assert torch.equal(model.state_dict()[k], td[k]), k
    assert model.emb_size == (2048 if RESNETS_DT[name]["bottleneck"] else 512) and model.emb_model.family == "resnet"


def test_plain_members_and_the_unknown_name_message_are_unchanged():
    model = get_model(_cfg("resnet_tiny_bottleneck"), ["a", "b"], "cpu")
    sd = model.state_dict()
    assert tuple(sd["emb_model.conv1.weight"].shape) == (64, 3, 7, 7) and "emb_model.layer2.0.downsample.0.weight" in sd
    assert tuple(sd["emb_model.layer2.0.downsample.0.weight"].shape) == (512, 256, 1, 1)
    with pytest.raises(NotImplementedError, match="resnet14t"):
        get_model(_cfg("no_such_backbone"), ["a", "b"], "cpu")
    with pytest.raises(NotImplementedError):
        get_model(_cfg("mobilenetv3_large_100"), ["a", "b"], "cpu")


@pytest.mark.parametrize("name", ["resnet14t", "resnet26d", "resnet18d"])
def test_scripted_twin_reproduces_the_reference_twin(name):
    torch.manual_seed(0)
    twin = ResNetDTClassifier(_cfg(name), ["a", "b", "c"])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:                                # zero_init_last would silence every residual branch
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
        for n, b in twin.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
    model = get_model(_cfg(name), ["a", "b", "c"], "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model))
    twin.eval()
    for shape in ((2, 3, 64, 64), (2, 3, 70, 73)):          # 70x73: 35x37 -> 18x19 -> 9x10 -> 5x5 -> 3x3 maps (ceil_mode, partial windows)
        x = torch.randn(*shape, generator=g)
        with torch.no_grad():
            torch.testing.assert_close(scripted(x), twin(x))


def test_new_entry_points_are_declared_exported_and_bound():
    text = (ROOT / "include" / "nkbhip.h").read_text()
    for name in ("nkb_stem3_tiles", "nkb_avgpool2x2"):
        before = text[text.index("int " + name) - 2000:text.index("int " + name)]
        assert "model.py:82" in before and "configs/singletask_config.py:227" in before, name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(", text))
    lib = hip.load()
    ids = hip._plan_fn_ids()
    for name in NEW:
        assert name in declared and name in hip._SIGS and hasattr(lib, name), name
    for name in ("nkb_stem3_conv", "nkb_avgpool2x2"):
        assert name in ids, name                            # recorded plans replay the new launches
    assert "nkb_stem3_tiles" not in ids and "nkb_stem3_tiles" in hip._PURE
    names = [lib.nkb_kernel_name(k) for k in range(32)]
    assert lib.nkb_kernel_name(0) == b"conv_igemm_fwd" and names[21] == b"layer_scale"      # appended, not inserted
    assert names[22:25] == [b"stem3_fwd", b"stem3_dgrad", b"avgpool2x2"]
    assert hip.kernel_launches("stem3") >= 0 and hip.kernel_launches("avgpool2") >= 0       # counters 15 and 16 exist (-1: no such slot)
    for dt in (0, 1):
        for ci, co in ((24, 32), (32, 32), (32, 64), (32, 24), (64, 32)):
            assert lib.nkb_stem3_tiles(dt, 2, 9, 11, ci, co) == 2 * (3 if dt == 0 else 2), (dt, ci, co)    # tiles of 4 (fp32) / 8 rows
        for ci, co in ((64, 64), (24, 24), (16, 32), (32, 128), (3, 24)):
            assert lib.nkb_stem3_tiles(dt, 2, 9, 11, ci, co) == 0, (dt, ci, co)
    assert lib.nkb_stem3_tiles(7, 2, 9, 11, 32, 32) == 0


_P = ctypes.c_void_p(64)


def _s3(dtype=1, dgrad=0, N=1, H=8, W=8, Cin=32, ldx=32, Cout=64, ldy=64, R=3, relu=0, stats=None, tiles=0):
    return (dtype, dgrad, None, None, None, None, stats, N, H, W, Cin, ldx, Cout, ldy, R, relu, tiles, None)


def _ap(dtype=1, backward=0, N=1, H=8, W=8, C=64):
    return (dtype, backward, None, None, N, H, W, C, None)


_REJECTIONS = [
    ("nkb_stem3_conv", _s3(dtype=7), b"stem3_conv: bad dtype 7"),
    ("nkb_stem3_conv", _s3(R=5), b"got R=5"),
    ("nkb_stem3_conv", _s3(Cin=64, ldx=64, Cout=64), b"channel pair 64 -> 64 not served"),
    ("nkb_stem3_conv", _s3(Cin=24, ldx=24, Cout=24, ldy=24), b"channel pair 24 -> 24 not served"),
    ("nkb_stem3_conv", _s3(Cin=20, ldx=24), b"must be multiples of 8 up to 64"),
    ("nkb_stem3_conv", _s3(Cout=128, ldy=128), b"must be multiples of 8 up to 64"),
    ("nkb_stem3_conv", _s3(ldx=24), b"must be >= Cin=32 / Cout=64"),
    ("nkb_stem3_conv", _s3(ldy=32), b"must be >= Cin=32 / Cout=64"),
    ("nkb_stem3_conv", _s3(dtype=0, ldy=66), b"multiples of 4"),
    ("nkb_stem3_conv", _s3(N=1 << 12, H=1 << 10, W=1 << 10), b"stem3_conv: operand exceeds 2^31"),
    ("nkb_stem3_conv", _s3(stats=_P, tiles=5), b"stats sized for 5 partial-sum rows, the launch has 1"),
    ("nkb_avgpool2x2", _ap(dtype=7), b"avgpool2x2: bad dtype 7"),
    ("nkb_avgpool2x2", _ap(C=12), b"avgpool2x2: C=12 not a multiple of 8"),
    ("nkb_avgpool2x2", _ap(dtype=0, C=6), b"avgpool2x2: C=6 not a multiple of 4"),
    ("nkb_avgpool2x2", _ap(N=1 << 12, H=1 << 8, W=1 << 8, C=64), b"avgpool2x2: operand exceeds 2^31"),
]


@pytest.mark.parametrize("name,args,text", _REJECTIONS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(_REJECTIONS)])
def test_host_side_rejections_answer_without_a_launch(name, args, text):
    """Every call returns before it touches an operand (null / dummy pointers), with its message in nkb_last_error."""
    lib = hip.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0 and text in lib.nkb_last_error(), (name, rc, lib.nkb_last_error())
