"""Host side of the optimizer options (no GPU): the group defaults `get_optimizer` builds for the new config keys against the torch
class of the same name built with the same arguments, torch's refusals, the layer ids behind `layer_decay`, and that a config
without any new key builds the two groups it built before."""
import pytest
import torch

from nkb_classification import utils
from nkb_classification.model import get_model

KEYS = ("lr", "weight_decay", "betas", "eps", "momentum", "dampening", "nesterov")


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


@pytest.fixture(scope="module")
def resnet():
    return get_model(_cfg("resnet_tiny_bottleneck"), ["a", "b", "c"], "cpu")


def _torch_groups(model, blr, bwd, clr, cwd):
    return [dict(params=list(model.emb_model.parameters()), lr=blr, weight_decay=bwd),
            dict(params=list(model.classifier.parameters()), lr=clr, weight_decay=cwd)]


NEW_CONFIGS = [
    (dict(type="adamw", lr=3e-4, weight_decay=0.05), torch.optim.AdamW, {}),
    (dict(type="adamw"), torch.optim.AdamW, {}),      # get_optimizer passes the config's weight decay: 0.0 when absent
    (dict(type="AdamW", lr=1e-3, backbone_lr=1e-4, classifier_weight_decay=0.1, betas=(0.8, 0.95), eps=1e-6), torch.optim.AdamW,
     dict(betas=(0.8, 0.95), eps=1e-6)),
    (dict(type="adam", lr=1e-3, weight_decay=0.02, decoupled_weight_decay=True, betas=[0.85, 0.99]), torch.optim.Adam,
     dict(decoupled_weight_decay=True, betas=(0.85, 0.99))),
    (dict(type="radam", lr=1e-3, weight_decay=0.02, decoupled_weight_decay=True, eps=1e-7), torch.optim.RAdam,
     dict(decoupled_weight_decay=True, eps=1e-7)),
    (dict(type="sgd", lr=0.1, momentum=0.9), torch.optim.SGD, dict(momentum=0.9)),
    (dict(type="sgd", lr=0.1, backbone_weight_decay=1e-4, momentum=0.9, dampening=0.1), torch.optim.SGD, dict(momentum=0.9, dampening=0.1)),
    (dict(type="sgd", lr=0.1, momentum=0.9, nesterov=True), torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
]


@pytest.mark.parametrize("cfg,cls,kw", NEW_CONFIGS, ids=[f"{i}_{c[0]['type'].lower()}" for i, c in enumerate(NEW_CONFIGS)])
def test_group_defaults_equal_the_torch_class(resnet, cfg, cls, kw):
    lr, wd = cfg.get("lr", 0.001), cfg.get("weight_decay", 0.0)
    ref = cls(_torch_groups(resnet, cfg.get("backbone_lr", lr), cfg.get("backbone_weight_decay", wd), cfg.get("classifier_lr", lr),
                            cfg.get("classifier_weight_decay", wd)), **kw)
    opt = utils.get_optimizer(resnet, cfg)
    assert isinstance(opt, utils.FusedOptimizer) and len(opt.param_groups) == 2
    for got, want in zip(opt.param_groups, ref.param_groups):
        assert [id(p) for p in got["params"]] == [id(p) for p in want["params"]]
        for k in KEYS:
            assert (k in got) == (k in want), k
            if k in want:
                assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])
        if "decoupled_weight_decay" in want:
            assert got["decoupled_weight_decay"] == want["decoupled_weight_decay"]


def test_constructor_defaults_equal_the_torch_class():
    """FusedOptimizer built bare: the defaults of torch's class, AdamW's weight_decay = 1e-2 included."""
    p = torch.nn.Parameter(torch.zeros(3))
    for kind, cls in (("adamw", torch.optim.AdamW), ("adam", torch.optim.Adam), ("radam", torch.optim.RAdam), ("sgd", torch.optim.SGD)):
        got, want = utils.FusedOptimizer([p], kind).defaults, cls([p]).defaults
        for k in KEYS + ("decoupled_weight_decay", "amsgrad"):
            assert (k in got) == (k in want), (kind, k)
            if k in want:
                assert got[k] == want[k], (kind, k)


def test_step_scalars_of_the_new_modes():
    """adamw is adam with c3 = 1; decoupled radam keeps radam's scalars with c3 = 1; SGD momentum passes 1 on the step torch clones
    the gradient, 1 - dampening afterwards, and c1 = 1 for Nesterov; plain SGD and the old kinds keep c3 = 0."""
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
    for step in range(1, 4):
        sa, sw, sr, sd = {"step": step - 1}, {"step": step - 1}, {"step": step - 1}, {"step": step - 1}
        ka, ca = utils._step_scalars("adam", sa, **kw)
        kw_, cw = utils._step_scalars("adamw", sw, **kw)
        assert ka == kw_ == 0 and ca[:3] == cw[:3] and ca[3] == 0.0 and cw[3] == 1.0
        assert utils._step_scalars("adam", {"step": step - 1}, decoupled=True, **kw) == (0, cw)
        kr, cr = utils._step_scalars("radam", sr, **kw)
        kd, cd = utils._step_scalars("radam", sd, decoupled=True, **kw)
        assert kr == kd == 2 and cr[:3] == cd[:3] and cr[3] == 0.0 and cd[3] == 1.0
    st = {}
    seq = [utils._step_scalars("sgd", st, lr=1e-2, beta1=0.0, beta2=0.0, eps=0.0, momentum=0.9, dampening=0.25) for _ in range(3)]
    assert seq == [(3, (1.0, 0.0, 0.0, 0.0)), (3, (0.75, 0.0, 0.0, 0.0)), (3, (0.75, 0.0, 0.0, 0.0))] and st["step"] == 3
    assert utils._step_scalars("sgd", {}, lr=1e-2, beta1=0.0, beta2=0.0, eps=0.0, momentum=0.9, nesterov=True) == (3, (1.0, 1.0, 0.0, 0.0))
    # without a momentum sgd keeps its zeros whatever beta1 holds: callers hand it Adam's betas (tests/test_ops_gpu.py)
    assert utils._step_scalars("sgd", {}, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8) == (3, (0.0, 0.0, 0.0, 0.0))
    assert utils._step_scalars("nadam", {}, **kw)[1][3] == 0.0


def test_refusals(resnet):
    with pytest.raises(NotImplementedError, match="amsgrad"):
        utils.get_optimizer(resnet, dict(type="adamw", amsgrad=True))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        utils.get_optimizer(resnet, dict(type="adam", amsgrad=True))
    assert utils.get_optimizer(resnet, dict(type="adamw", amsgrad=False)).defaults["amsgrad"] is False
    for bad in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(nesterov=True, momentum=0.0)):
        with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
            utils.get_optimizer(resnet, dict(type="sgd", lr=0.1, **bad))
        with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
            torch.optim.SGD(list(resnet.parameters()), lr=0.1, **bad)        # torch's wording, from torch
    with pytest.raises(NotImplementedError, match="dampening=1"):      # the kernel reads c0 = 1 - dampening = 0 as plain SGD
        utils.get_optimizer(resnet, dict(type="sgd", momentum=0.9, dampening=1))
    with pytest.raises(ValueError, match="Invalid momentum value: -0.5"):
        utils.get_optimizer(resnet, dict(type="sgd", momentum=-0.5))
    with pytest.raises(ValueError, match="Invalid beta parameter at index 1: 1.0"):
        utils.get_optimizer(resnet, dict(type="adamw", betas=(0.9, 1.0)))
    with pytest.raises(NotImplementedError, match="layer_decay"):
        utils.get_optimizer(get_model(_cfg("resnet50"), ["a", "b"], "cpu"), dict(type="adamw", layer_decay=0.75))
    with pytest.raises(ValueError, match="layer_decay"):
        utils.get_optimizer(get_model(_cfg("vit_clip_test"), ["a", "b"], "cpu"), dict(type="adamw", layer_decay=1.5))
    with pytest.raises(NotImplementedError, match="Unknown optimizer in config: lion"):
        utils.get_optimizer(resnet, dict(type="lion", betas=(0.9, 0.99)))
    with pytest.raises(TypeError, match="momentum"):              # as torch.optim.AdamW(momentum=...) is a TypeError
        utils.get_optimizer(resnet, dict(type="adamw", momentum=0.9))


def _check_layer_ids(model, expect_id0, expect_top):
    bb = model.emb_model
    depth = len(bb.blocks)
    groups = bb.layer_groups()
    assert len(groups) == depth + 2
    names = {id(p): n for n, p in bb.named_parameters()}
    order = [id(p) for p in bb.parameters()]
    flat = [id(p) for g in groups for p in g]
    assert sorted(flat) == sorted(order) and len(set(flat)) == len(flat)          # every backbone parameter exactly once
    ids = {id(p): k for k, g in enumerate(groups) for p in g}
    seq = [ids[i] for i in order]
    assert seq == sorted(seq)                                                      # non-decreasing in parameters() order
    assert flat == order                                                           # ... and each id keeps that order
    assert {names[id(p)] for p in groups[0]} == expect_id0
    for i in range(depth):
        got = {names[id(p)] for p in groups[i + 1]}
        assert got and all(n.startswith(f"blocks.{i}.") for n in got)
        assert got == {n for n in names.values() if n.startswith(f"blocks.{i}.")}
    assert {names[id(p)] for p in groups[depth + 1]} == expect_top
    return depth


def test_layer_ids_of_a_pre_norm_member_and_groups():
    model = get_model(_cfg("vit_clip_test"), ["a", "b", "c"], "cpu")
    depth = _check_layer_ids(model, {"cls_token", "pos_embed", "patch_embed.proj.weight", "norm_pre.weight", "norm_pre.bias"},
                             {"norm.weight", "norm.bias"})
    opt = utils.get_optimizer(model, dict(type="adamw", lr=1e-3, backbone_lr=2e-4, weight_decay=0.05, classifier_weight_decay=0.0,
                                          layer_decay=0.75))
    g = opt.param_groups
    assert len(g) == depth + 3
    for k in range(depth + 2):
        assert g[k]["lr"] == 2e-4 * 0.75 ** (depth + 1 - k) and g[k]["weight_decay"] == 0.05
        assert [id(p) for p in g[k]["params"]] == [id(p) for p in model.emb_model.layer_groups()[k]]
    assert g[-1]["lr"] == 1e-3 and g[-1]["weight_decay"] == 0.0
    assert [id(p) for p in g[-1]["params"]] == [id(p) for p in model.classifier.parameters()]
    assert g[depth + 1]["lr"] == 2e-4                       # the last backbone id trains at the backbone lr itself


def test_layer_ids_of_a_unicom_member():
    model = get_model(_cfg("unicom ViT-Tiny-Test"), ["a", "b", "c"], "cpu")
    depth = _check_layer_ids(model, {"pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"},
                             {"norm.weight", "norm.bias", "feature.0.weight", "feature.1.weight", "feature.1.bias", "feature.2.weight",
                              "feature.3.weight", "feature.3.bias"})
    opt = utils.get_optimizer(model, dict(type="sgd", lr=0.1, momentum=0.9, layer_decay=0.5))
    assert [g["lr"] for g in opt.param_groups] == [0.1 * 0.5 ** (depth + 1 - k) for k in range(depth + 2)] + [0.1]
    assert all(g["momentum"] == 0.9 for g in opt.param_groups)


def test_configs_without_new_keys_build_what_they_built(resnet):
    """Two groups, backbone then classifier, with exactly the keys and values the four reference kinds had."""
    common = dict(lr=1e-3, weight_decay=0.0, maximize=False)
    want = {
        "adam": dict(common, betas=(0.9, 0.999), eps=1e-8, decoupled_weight_decay=False, amsgrad=False),
        "nadam": dict(common, betas=(0.9, 0.999), eps=1e-8, decoupled_weight_decay=True, momentum_decay=4e-3),
        "radam": dict(common, betas=(0.9, 0.999), eps=1e-8, decoupled_weight_decay=False),
        "sgd": dict(common, momentum=0, dampening=0, nesterov=False),
    }
    for kind, defaults in want.items():
        opt = utils.get_optimizer(resnet, dict(type=kind, lr=1e-2, backbone_lr=1e-3, classifier_weight_decay=0.1))
        assert opt.defaults == defaults, kind
        assert len(opt.param_groups) == 2
        g0, g1 = opt.param_groups
        assert [id(p) for p in g0["params"]] == [id(p) for p in resnet.emb_model.parameters()]
        assert [id(p) for p in g1["params"]] == [id(p) for p in resnet.classifier.parameters()]
        assert (g0["lr"], g0["weight_decay"], g1["lr"], g1["weight_decay"]) == (1e-3, 0.0, 1e-2, 0.1)
        for g in (g0, g1):
            assert {k: v for k, v in g.items() if k not in ("params", "lr", "weight_decay")} == \
                {k: v for k, v in defaults.items() if k not in ("lr", "weight_decay")}, kind
