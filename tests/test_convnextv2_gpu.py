"""ConvNeXt V2 on the HIP engine against the twin of tests/convnextv2_reference.py (our own pure-torch restatement; timm parity
unpinned), in the form and with the bars of tests/test_convnext_gpu.py: single-step gradients in fp32 against the float64 twin with the
GRN launches counted, a NAdam trajectory through train_epoch, dropout with replayed masks (the backward path without the fused
multiplier), eval mode, a frozen backbone, train.py end to end, bit-reproducibility, recorded plans against the Python path, and
convnextv2_base at real widths and grids in bf16.

The 1-D parameters are randomised: grn.weight and grn.bias into U(-1, 1) (zero at init, which would silence the whole t path of the
backward pass), the others into [0.5, 1] as tests/test_model_gpu.py does."""
import argparse
import math
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

from convnextv2_reference import ConvNeXtV2Classifier as ConvNeXtClassifier  # noqa: E402
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


def _cfg_model(name="convnextv2_test", drop=0.0):
    return dict(model=name, pretrained=False, backbone_dropout=drop, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pair(drop=0.0, seed=0):
    torch.manual_seed(seed)
    twin = ConvNeXtClassifier(_cfg_model(drop=drop), CLASSES)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if ".grn." in name:
                p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)
            elif p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg_model(drop=drop), CLASSES, DEV)
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
    return out.detach().cpu()


@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (4, 3, 70, 73)], ids=["64x64", "70x73"])
def test_single_step_gradients_match_the_float64_twin(shape):
    """The fp32 bars of tests/test_model_gpu.py: logits within 1e-3 of the fp32 twin with the same argmax; every tensor's gradient
    within max(2e-2, 4 x the fp32 twin's own error) of the float64 twin; the whole gradient within 3e-3 in L2.  70x73 has
    floor-clipped stem (17x18) and downsample (8x9, 4x4, 2x2) grids."""
    t32, model = _pair()
    t64 = ConvNeXtClassifier(_cfg_model(), CLASSES).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(shape)
    t32.train(); t64.train(); model.train()
    ref32 = t32(x)
    torch.nn.functional.cross_entropy(ref32, y).backward()
    torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
    n_dw, n_ls = hip.kernel_launches("dwconv"), hip.kernel_launches("layer_scale")
    hip.prof_collect()
    hip.prof_enable(True)
    try:
        out = _hip_step(model, x, y)
    finally:
        hip.prof_enable(False)
    prof = hip.prof_collect()
    assert hip.kernel_launches("dwconv") - n_dw == 15 and hip.kernel_launches("layer_scale") == n_ls          # 5 blocks, no layer scale
    # per block: reduce + apply forward (exactly 2), reduce + apply backward and the parameter launch (2 or 3)
    n_red, n_app, n_par = (prof[k]["launches"] if k in prof else 0 for k in ("grn_reduce", "grn_apply", "grn_param"))
    assert n_red == 10 and n_app == 10 and n_par == 5, prof
    assert prof["grn_reduce"]["bytes"] > 0 and prof["grn_apply"]["bytes"] > 0
    assert "layer_scale" not in prof
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
    print(f"\n[convnextv2_test {shape}] logits {_relerr(out, ref32.detach()):.2e}  gradient L2 {(num / den) ** 0.5:.2e}  worst tensor {worst}")
    assert (num / den) ** 0.5 < 3e-3, (num / den) ** 0.5


def test_three_nadam_steps_follow_the_twin():
    """train_epoch with NAdam, three steps, fp32: running losses, the final eval logits and the parameter norms follow the twin's
    own fp32 trajectory (torch's optimizer, the oracle's train loop) at the 1e-3 bar of the golden-trajectory tests."""
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
    for k, v in td.items():
        assert abs(float(sd[k].float().norm()) - float(v.norm())) <= 1e-3 * max(1.0, float(v.norm())), k


def test_backbone_dropout_matches_the_twin_with_replayed_masks():
    """backbone_dropout = 0.25 (set_dropout rewrites mlp.drop1, mlp.drop2 and head.drop): the HIP step's keep masks are replayed
    inside the twin at the same sites; logits and every gradient must then agree (fp32).  With drop1 active the activation derivative
    is not kept: GRN backward runs without the fused multiplier, followed by dropout and GELU backward."""
    p = 0.25
    twin, model = _pair(drop=p, seed=3)
    x, y = _batch(seed=6)
    model.train(); twin.train()
    out = _hip_step(model, x, y)
    saved = model._active.saved
    assert "gp" not in saved["s0.b0.act"]

    class Replay(torch.nn.Module):
        def __init__(self, mask):
            super().__init__()
            self.mask = mask.float().cpu()

        def forward(self, t):
            return t * self.mask.reshape(t.shape) / (1 - p)

    keys = ["head_drop"]
    twin.emb_model.head.drop = Replay(saved["head_drop"]["mask"])
    for si, st in enumerate(twin.emb_model.stages):
        for bi, blk in enumerate(st.blocks):
            blk.mlp.drop1 = Replay(saved[f"s{si}.b{bi}.mlp_drop"]["mask"])
            blk.mlp.drop2 = Replay(saved[f"s{si}.b{bi}.mlp2_drop"]["mask"])
            keys += [f"s{si}.b{bi}.mlp_drop", f"s{si}.b{bi}.mlp2_drop"]
    assert len(keys) == 11
    for k in keys:
        keep = saved[k]["mask"].float().mean().item()
        assert 0.6 < keep < 0.9, (k, keep)
    ref = twin(x)
    torch.nn.functional.cross_entropy(ref, y).backward()
    assert _relerr(out, ref.detach()) < 1e-3
    po = dict(twin.named_parameters())
    num = den = 0.0
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        num += (prm.grad.detach().cpu().double() - po[name].grad.double()).pow(2).sum().item()
        den += po[name].grad.double().pow(2).sum().item()
    assert (num / den) ** 0.5 < 2e-3, (num / den) ** 0.5
    model.eval()
    with torch.no_grad():
        e1, e2 = model(x.to(DEV)), model(x.to(DEV))
    assert torch.equal(e1, e2)                                    # eval: every dropout is the identity


def test_eval_mode_matches_the_twin_and_saves_nothing():
    twin, model = _pair(drop=0.1)
    model.eval(); twin.eval()
    for shape in ((4, 3, 64, 64), (2, 3, 70, 73)):
        x, _ = _batch(shape, seed=2)
        with torch.no_grad():
            out, ref = model(x.to(DEV)).cpu(), twin(x)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out16 = model(x.to(DEV)).float().cpu()
        assert _relerr(out, ref) < 1e-3 and out.argmax(-1).tolist() == ref.argmax(-1).tolist()
        assert _relerr(out16, ref) < 5e-2
    for eng in model._engines.values():
        assert not any("x" in v or "mask" in v or "u" in v or "sumsq" in v for v in eng.saved.values() if isinstance(v, dict)), list(eng.saved)
        assert not any(k.endswith(".grn") for k in eng.saved)


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
    """The same step twice gives bit-identical gradients (no float atomics anywhere in the GRN kernels), and the recorded-plan path
    (default; the fourth step replays the plans) gives the gradients of the Python path (NKB_PLAN=0) bit for bit."""
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


def test_train_py_end_to_end_writes_checkpoint_and_scripted_twin(tmp_path):
    """train.py on the synthetic config with convnextv2_test: last.pth and scripted_last.pt are written, their logits agree, and the
    checkpoint carries the GRN parameters."""
    root = ROOT / "nkb-classification_amd"
    cfg = (root / "configs" / "synthetic_singletask_config.py").read_text()
    assert '"model": "resnet18"' in cfg and '"n_images": 256' in cfg
    cfg = cfg.replace('"runs/synthetic_single"', repr(str(tmp_path / "exp"))).replace('"model": "resnet18"', '"model": "convnextv2_test"')
    cfg = cfg.replace('"backbone_dropout": 0.0', '"backbone_dropout": 0.1')
    (tmp_path / "cfg_e2e.py").write_text(cfg)
    r = subprocess.run([sys.executable, str(root / "train.py"), "-cfg", str(tmp_path / "cfg_e2e.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    exp = tmp_path / "exp"
    assert (exp / "weights" / "last.pth").exists() and (exp / "weights" / "scripted_last.pt").exists()
    sd = torch.load(exp / "weights" / "last.pth", map_location="cpu")
    assert "emb_model.stages.2.blocks.1.conv_dw.weight" in sd and "emb_model.head.norm.bias" in sd and "classifier.1.weight" in sd
    assert "emb_model.stages.2.blocks.1.mlp.grn.weight" in sd and not [k for k in sd if k.endswith(".gamma")]
    assert float(sd["emb_model.stages.2.blocks.1.mlp.grn.bias"].abs().max()) > 0          # zero at init: it was trained
    scripted = torch.jit.load(str(exp / "weights" / "scripted_last.pt"), map_location="cpu").eval()
    hip_model = get_model(dict(_cfg_model(), checkpoint=str(exp / "weights" / "last.pth")), [str(i) for i in range(10)], DEV).eval()
    xb = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        ref_logits = scripted(xb)
        hip_logits = hip_model(xb.to(DEV)).float().cpu()
    assert ref_logits.shape == hip_logits.shape == (6, 10)
    assert _relerr(hip_logits, ref_logits) < 1e-3
    assert hip_logits.argmax(-1).tolist() == ref_logits.argmax(-1).tolist()


# ---- convnextv2_base at real widths and grids (the form of tests/test_parity_bench_size_gpu.py) -----------------------------------
BASE_BATCH = 8                     # kept small: the operator test covers large N
OPT = dict(type="nadam", lr=1e-4, backbone_lr=1e-5, classifier_lr=1e-4, weight_decay=0.01, backbone_weight_decay=0.01,
           classifier_weight_decay=0.2)          # bench.build


def _flat(named):
    return torch.cat([g.detach().float().flatten() for _, g in named])


def _dist(g, truth):
    return torch.nn.functional.cosine_similarity(g, truth, dim=0).item(), ((g - truth).norm() / truth.norm()).item()


def test_convnextv2_base_matches_the_twin():
    """bench.py's configuration but for the batch (convnextv2_base, batch 8, bf16, 224 x 224, NAdam, plans and side stream on), four
    steps next to two runs of the twin on the same GPU from the same state and batch: truth = torch's kernels in fp32, yardstick =
    the twin under torch.autocast(bfloat16).  grn.weight / grn.bias are U(-1, 1) in all three.  Bars of the bench-size parity file:
    gradient L2 <= 1.25 x the yardstick's + 5e-3, cosine >= the yardstick's - 1e-3, loss within 1e-2 relative — on the whole gradient,
    on the GRN parameters as a group of their own and on the conv_dw tensors; step 1 runs eager, step 4 replays the recorded plans."""
    import bench
    batch, classes = BASE_BATCH, 1000
    args = argparse.Namespace(model="convnextv2_base", classes=classes, batch=batch, dtype="bf16", heads="")
    device = torch.device(DEV)
    model, opt, crit = bench.build(args, device)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".grn." in n:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1).to(p.device))
    twins = []
    for _ in range(2):
        t = ConvNeXtClassifier(_cfg_model("convnextv2_base"), [str(i) for i in range(classes)])
        t.load_state_dict(model.state_dict())
        t = t.to(device).train()
        twins.append((t, torch_engine.make_optimizer(t, OPT)))
    g = torch.Generator().manual_seed(1234)
    img = torch.randn(batch, 3, 224, 224, generator=g).to(device)
    tgt = torch.randint(0, classes, (batch,), generator=g).to(device)
    names = [n for n, _ in twins[0][0].named_parameters()]
    dw_names = [n for n in names if ".conv_dw." in n]
    ga_names = [n for n in names if ".mlp.grn." in n]
    assert len(dw_names) == 2 * 36 and len(ga_names) == 2 * 36
    for k in ("dwconv", "layer_scale", "gemm8p"):
        hip.kernel_launches(k, reset=True)
    model.train()
    out = []
    for step in range(4):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            log = model(img)
            loss = crit(log, tgt)
        res = []
        for k, (t, to) in enumerate(twins):
            to.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(k == 1)):
                ls = torch.nn.functional.cross_entropy(t(img).float(), tgt)
            ls.backward()
            tp = dict(t.named_parameters())
            res.append((ls.item(), _flat([(n, p.grad) for n, p in t.named_parameters()]), _flat([(n, tp[n].grad) for n in dw_names]),
                        _flat([(n, tp[n].grad) for n in ga_names])))
        loss.backward()
        torch.cuda.synchronize()
        hp = dict(model.named_parameters())
        gh = _flat([(n, hp[n].grad) for n in names])
        (tloss, tg, tdw, tga), (yloss, yg, ydw, yga) = res
        cos, l2 = _dist(gh, tg)
        ycos, yl2 = _dist(yg, tg)
        dcos, dl2 = _dist(_flat([(n, hp[n].grad) for n in dw_names]), tdw)
        ydcos, ydl2 = _dist(ydw, tdw)
        gcos, gl2 = _dist(_flat([(n, hp[n].grad) for n in ga_names]), tga)
        ygcos, ygl2 = _dist(yga, tga)
        out.append(dict(step=step + 1, loss=loss.item(), ref_loss=tloss, yard_loss=yloss, cos=cos, l2=l2, ycos=ycos, yl2=yl2,
                        dcos=dcos, dl2=dl2, ydcos=ydcos, ydl2=ydl2, gcos=gcos, gl2=gl2, ygcos=ygcos, ygl2=ygl2,
                        finite=bool(torch.isfinite(gh).all().item())))
        for _, to in twins:
            to.step()
        opt.step()
    print(f"\n[convnextv2_base bs {batch} bf16] " + "  ".join(
        f"step {o['step']}: loss {o['loss']:.4f} (truth {o['ref_loss']:.4f}, autocast {o['yard_loss']:.4f}) grad cos {o['cos']:.5f} "
        f"({o['ycos']:.5f}) L2 {o['l2']:.3e} ({o['yl2']:.3e}); conv_dw only: cos {o['dcos']:.5f} ({o['ydcos']:.5f}) "
        f"L2 {o['dl2']:.3e} ({o['ydl2']:.3e}); grn only: cos {o['gcos']:.5f} ({o['ygcos']:.5f}) L2 {o['gl2']:.3e} ({o['ygl2']:.3e})" for o in out) + f"  plans {len(model._active.plans)}  gemm8p launches {hip.kernel_launches('gemm8p')}")
    for o in (out[0], out[-1]):
        assert o["finite"] and math.isfinite(o["loss"])
        assert abs(o["loss"] - o["ref_loss"]) <= 1e-2 * abs(o["ref_loss"]), o
        assert o["l2"] <= 1.25 * o["yl2"] + 5e-3 and o["cos"] >= o["ycos"] - 1e-3, o
        assert o["dl2"] <= 1.25 * o["ydl2"] + 5e-3 and o["dcos"] >= o["ydcos"] - 1e-3, o       # the same bars on the conv_dw tensors
        assert o["gl2"] <= 1.25 * o["ygl2"] + 5e-3 and o["gcos"] >= o["ygcos"] - 1e-3, o       # and on the GRN parameters, each group on its own
    assert len(model._active.plans) >= 2
    # per step 36 forward + 36 data-gradient + 36 weight-gradient depthwise launches, and no layer scale at all
    assert hip.kernel_launches("dwconv") == 4 * 108 and hip.kernel_launches("layer_scale") == 0
