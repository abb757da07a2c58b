"""ResNet-D/T members on the HIP engine against the twin of tests/resnet_dt_reference.py (our own pure-torch restatement; timm parity
unpinned), on resnet14t: single-step gradients in fp32 against the float64 twin, a NAdam trajectory through train_epoch, eval mode on
the folded path, a frozen backbone, bit-reproducibility, recorded plans against the Python path, a bf16 step against the autocast
yardstick (the form of tests/test_parity_bench_size_gpu.py), train.py end to end, the plain members' untouched path and the
3-4-6-3 wiring of resnet50d.

The 1-D parameters are randomised into [0.5, 1] as tests/test_model_gpu.py does: zero_init_last would silence every residual branch."""
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from resnet_dt_reference import ResNetDTClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification import model as model_mod  # noqa: E402
from nkb_classification.engine import train_epoch  # noqa: E402
from nkb_classification.logging import BaseLogger  # noqa: E402
from nkb_classification.losses import get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.utils import get_optimizer  # noqa: E402
from oracle import torch_engine  # noqa: E402

DEV = "cuda:0"
CLASSES = ["a", "b", "c"]


def _cfg_model(name="resnet14t"):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pair(name="resnet14t", seed=0):
    torch.manual_seed(seed)
    twin = ResNetDTClassifier(_cfg_model(name), CLASSES)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg_model(name), CLASSES, DEV)
    model.load_state_dict(twin.state_dict())
    return twin, model


def _batch(shape=(4, 3, 64, 64), seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randint(0, len(CLASSES), (shape[0],), generator=g)


def _hip_step(model, x, y):
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    out = model(x.to(DEV))
    crit(out, y.to(DEV)).backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu()


@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (4, 3, 70, 73)], ids=["64x64", "70x73"])
def test_single_step_gradients_match_the_float64_twin(shape):
    """The fp32 bars of tests/test_model_gpu.py: logits within 1e-3 of the fp32 twin with the same argmax; every tensor's gradient
    within max(2e-2, 4 x the fp32 twin's own error) of the float64 twin; the whole gradient within 3e-3 in L2.  70x73 gives
    35x37 -> 18x19 -> 9x10 -> 5x5 -> 3x3 maps: ceil_mode and partial pooling windows in every avg_down shortcut."""
    t32, model = _pair()
    t64 = ResNetDTClassifier(_cfg_model(), CLASSES).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(shape)
    t32.train(); t64.train(); model.train()
    ref32 = t32(x)
    torch.nn.functional.cross_entropy(ref32, y).backward()
    torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
    n_s3, n_ap = hip.kernel_launches("stem3"), hip.kernel_launches("avgpool2")
    out = _hip_step(model, x, y)
    # two narrow forwards + two narrow data gradients; layer2 / 3 / 4 shortcut pools forward + backward
    assert hip.kernel_launches("stem3") - n_s3 == 4 and hip.kernel_launches("avgpool2") - n_ap == 6
    assert _relerr(out, ref32.detach()) < 1e-3
    assert out.argmax(-1).tolist() == ref32.argmax(-1).tolist()
    p64, p32 = dict(t64.named_parameters()), dict(t32.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in p64.values())
    num = den = 0.0
    worst = (0.0, "")
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        assert p.grad.shape == p32[name].grad.shape
        ref = p64[name].grad
        scale = max(ref.abs().max().item(), 1e-6 * gmax)
        e_hip = (p.grad.cpu().double() - ref).abs().max().item() / scale
        e_cpu = (p32[name].grad.double() - ref).abs().max().item() / scale
        worst = max(worst, (e_hip, name))
        assert e_hip <= max(2e-2, 4 * e_cpu), (name, e_hip, e_cpu)
        num += (p.grad.cpu().double() - ref).pow(2).sum().item()
        den += ref.pow(2).sum().item()
    print(f"\n[resnet14t {shape}] logits {_relerr(out, ref32.detach()):.2e}  gradient L2 {(num / den) ** 0.5:.2e}  worst tensor {worst}")
    assert (num / den) ** 0.5 < 3e-3, (num / den) ** 0.5


def test_three_nadam_steps_follow_the_twin():
    """train_epoch with NAdam, three steps, fp32: running losses, the final eval logits and the norms of every parameter and buffer
    (the running statistics of the two new stem BatchNorms and of the shortcut BatchNorms under their new keys included) follow the
    twin's own fp32 trajectory at the 1e-3 bar of the golden-trajectory tests."""
    twin, model = _pair()
    batches = torch_engine.synthetic_batches(12, 4, len(CLASSES), seed=1234, hw=64)
    opt_cfg = dict(type="nadam", lr=1e-4, weight_decay=0.01)
    cfg = types.SimpleNamespace(task="single", enable_mixed_presicion=False, log_gradients=False, show_full_current_loss_in_terminal=False)
    opt = get_optimizer(model, opt_cfg)
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    tr = train_epoch(model, batches, opt, None, torch.amp.GradScaler("cuda", enabled=False), crit, DEV, cfg, BaseLogger(cfg, CLASSES))
    ref = torch_engine.train_epoch(twin, batches, torch_engine.make_optimizer(twin, opt_cfg), None,
                                   torch_engine.Criterion(dict(task="single", type="CrossEntropyLoss")), torch_engine.EpochLog(False))
    assert len(tr["running_loss"]) == 3
    assert _relerr(tr["running_loss"], ref["running_loss"]) < 1e-3
    assert tr["ground_truth"] == ref["ground_truth"]
    model.eval(); twin.eval()
    x, _ = _batch(seed=11)
    with torch.no_grad():
        out, want = model(x.to(DEV)).cpu(), twin(x)
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    sd, td = model.state_dict(), twin.state_dict()
    for k in ("emb_model.conv1.1.running_mean", "emb_model.conv1.4.running_var", "emb_model.layer2.0.downsample.2.running_var"):
        assert k in td and float((td[k] - (1.0 if k.endswith("var") else 0.0)).abs().max()) > 0, k       # they moved
    for k, v in td.items():
        assert abs(float(sd[k].float().norm()) - float(v.float().norm())) <= 1e-3 * max(1.0, float(v.float().norm())), k


def test_eval_mode_matches_the_twin_on_the_folded_path_and_saves_nothing():
    twin, model = _pair()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, b in twin.named_buffers():                         # running statistics away from (0, 1)
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
    model.load_state_dict(twin.state_dict())
    model.eval(); twin.eval()
    for shape in ((4, 3, 64, 64), (2, 3, 70, 73)):
        x, _ = _batch(shape, seed=2)
        with torch.no_grad():
            n_s3 = hip.kernel_launches("stem3")
            out, ref = model(x.to(DEV)).cpu(), twin(x)
            assert hip.kernel_launches("stem3") - n_s3 == 2       # conv + shift + ReLU in one launch, and the conv before the pooled tail
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out16 = model(x.to(DEV)).float().cpu()
        assert _relerr(out, ref) < 1e-3 and out.argmax(-1).tolist() == ref.argmax(-1).tolist()
        assert _relerr(out16, ref) < 5e-2
    for eng in model._engines.values():
        assert "stem1" in eng._fold and "layer2.0.ds" in eng._fold                  # BatchNorm folded into the narrow conv / the shortcut
        assert not any("x" in v or "mask" in v for v in eng.saved.values() if isinstance(v, dict)), list(eng.saved)


def test_frozen_backbone_only_updates_head():
    twin, model = _pair()
    model.set_backbone_state("freeze"); twin.set_backbone_state("freeze")
    x, y = _batch(seed=9)
    model.train(); twin.train()
    _hip_step(model, x, y)
    torch.nn.functional.cross_entropy(twin(x), y).backward()
    assert all(p.grad is None for p in model.emb_model.parameters())
    for (n, p), (_, q) in zip(model.classifier.named_parameters(), twin.classifier.named_parameters()):
        assert _relerr(p.grad.cpu(), q.grad) < 1e-3, n


def _grads(model, x, y, steps):
    """Gradients of the last of `steps` identical steps (no optimizer step in between: the weights never move)."""
    out = None
    for _ in range(steps):
        for p in model.parameters():
            p.grad = None
        out = _hip_step(model, x, y)
    return out, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_same_step_twice_and_recorded_plans_give_identical_gradients(amp, monkeypatch):
    """The same step twice gives bit-identical gradients (no float atomics in the new kernels), and the recorded-plan path (default;
    the fourth step replays the plans) gives the gradients of the Python path (NKB_PLAN=0) bit for bit."""
    twin, model = _pair()
    x, y = _batch(seed=4)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        o1, g1 = _grads(model, x, y, 1)
        o4, g4 = _grads(model, x, y, 3)                            # steps 2, 3 (records), 4 (replays)
        assert len(model._active.plans) >= 2
        monkeypatch.setattr(model_mod, "_PLANS", False)
        fresh = get_model(_cfg_model(), CLASSES, DEV)
        fresh.load_state_dict(twin.state_dict())
        fresh.train()
        o0, g0 = _grads(fresh, x, y, 2)
        assert len(fresh._active.plans) == 0
    assert torch.equal(o1, o4) and torch.equal(o1, o0)
    for n in g1:
        assert torch.equal(g1[n], g4[n]), n
        assert torch.equal(g1[n], g0[n]), n


def test_bf16_step_against_the_autocast_yardstick():
    """Batch 8, 64x64, bf16: the engine's gradient L2 error against the float64 twin is at most 1.25 x the error of the twin run under
    torch.autocast("cpu", bfloat16) on the same batch, + 5e-3 (the form of tests/test_parity_bench_size_gpu.py)."""
    t32, model = _pair()
    t64 = ResNetDTClassifier(_cfg_model(), CLASSES).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch((8, 3, 64, 64), seed=21)
    t32.train(); t64.train(); model.train()
    torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        yl = t32(x)
    torch.nn.functional.cross_entropy(yl.float(), y).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = _hip_step(model, x, y)
    names = [n for n, _ in t64.named_parameters()]
    p64, p32, ph = dict(t64.named_parameters()), dict(t32.named_parameters()), dict(model.named_parameters())
    truth = torch.cat([p64[n].grad.flatten() for n in names])
    yard = torch.cat([p32[n].grad.double().flatten() for n in names])
    got = torch.cat([ph[n].grad.detach().cpu().double().flatten() for n in names])
    assert torch.isfinite(got).all() and torch.isfinite(out).all()
    l2, yl2 = ((got - truth).norm() / truth.norm()).item(), ((yard - truth).norm() / truth.norm()).item()
    print(f"\n[resnet14t bs 8 bf16] gradient L2 error {l2:.3e}, autocast yardstick {yl2:.3e}")
    assert l2 <= 1.25 * yl2 + 5e-3, (l2, yl2)


def test_train_py_end_to_end_writes_checkpoint_and_scripted_twin(tmp_path):
    """train.py on the synthetic config with resnet14t: last.pth (timm's D/T keys) and scripted_last.pt are written, and their logits agree."""
    root = ROOT / "nkb-classification_amd"
    cfg = (root / "configs" / "synthetic_singletask_config.py").read_text()
    assert '"model": "resnet18"' in cfg and '"n_images": 256' in cfg
    cfg = cfg.replace('"runs/synthetic_single"', repr(str(tmp_path / "exp"))).replace('"model": "resnet18"', '"model": "resnet14t"')
    (tmp_path / "cfg_e2e.py").write_text(cfg)
    r = subprocess.run([sys.executable, str(root / "train.py"), "-cfg", str(tmp_path / "cfg_e2e.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    exp = tmp_path / "exp"
    assert (exp / "weights" / "last.pth").exists() and (exp / "weights" / "scripted_last.pt").exists()
    sd = torch.load(exp / "weights" / "last.pth", map_location="cpu")
    for k in ("emb_model.conv1.0.weight", "emb_model.conv1.4.running_var", "emb_model.conv1.6.weight", "emb_model.bn1.weight",
              "emb_model.layer1.0.downsample.1.weight", "emb_model.layer4.0.downsample.2.running_mean", "classifier.1.weight"):
        assert k in sd, k
    assert tuple(sd["emb_model.conv1.3.weight"].shape) == (32, 24, 3, 3)
    scripted = torch.jit.load(str(exp / "weights" / "scripted_last.pt"), map_location="cpu").eval()
    hip_model = get_model(dict(_cfg_model(), checkpoint=str(exp / "weights" / "last.pth")), [str(i) for i in range(10)], DEV).eval()
    xb = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        ref_logits = scripted(xb)
        hip_logits = hip_model(xb.to(DEV)).float().cpu()
    assert ref_logits.shape == hip_logits.shape == (6, 10)
    assert _relerr(hip_logits, ref_logits) < 1e-3
    assert hip_logits.argmax(-1).tolist() == ref_logits.argmax(-1).tolist()


def test_plain_members_never_reach_the_new_kernels():
    model = get_model(_cfg_model("resnet_tiny_bottleneck"), CLASSES, DEV)
    x, y = _batch(seed=8)
    model.train()
    n_s3, n_ap = hip.kernel_launches("stem3"), hip.kernel_launches("avgpool2")
    for amp in (False, True):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            _hip_step(model, x, y)
    assert hip.kernel_launches("stem3") == n_s3 and hip.kernel_launches("avgpool2") == n_ap


def test_resnet50d_forward_backward_bf16():
    """The 3-4-6-3 wiring with the D stem (32-32-64) at (2, 3, 64, 64) in bf16: finite gradients of the right shapes."""
    twin, model = _pair("resnet50d")
    x, y = _batch((2, 3, 64, 64), seed=13)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = _hip_step(model, x, y)
    assert out.shape == (2, len(CLASSES)) and torch.isfinite(out).all()
    shapes = {n: p.shape for n, p in twin.named_parameters()}
    seen = 0
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == shapes[n], n
        assert torch.isfinite(p.grad).all(), n
        seen += 1
    assert seen == len(shapes) and float(dict(model.named_parameters())["emb_model.conv1.3.weight"].grad.abs().max()) > 0
