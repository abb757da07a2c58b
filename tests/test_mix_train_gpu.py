"""engine.train_epoch over a DeviceLoader that mixes its batches (Mixup / CutMix inside nkb_image_prep, MixedTarget labels) with a
label-smoothing cross entropy: finite losses, the logger's ground truth are the images' own labels, the same seed gives the same
losses, and with prob = 0 and no smoothing the losses are those of a run without the keys, bit for bit."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nkb_classification import dataset as D  # noqa: E402
from nkb_classification.engine import train_epoch  # noqa: E402
from nkb_classification.logging import BaseLogger  # noqa: E402
from nkb_classification.losses import MixedTarget, get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.utils import get_optimizer  # noqa: E402

DEV = "cuda:0"
SIZE, NB, B = 64, 3, 6
CLASSES = ["a", "b", "c"]
CFG = types.SimpleNamespace(task="single", enable_mixed_presicion=False, log_gradients=False, show_full_current_loss_in_terminal=False)
CFG_MODEL = dict(model="resnet18", pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0,
                 classifier_initialization="kaiming_normal_", task="single")


def _batches():
    rng = np.random.default_rng(2)
    out = []
    for k in range(NB):
        raw = torch.from_numpy(rng.integers(0, 256, (B, SIZE, SIZE, 3), dtype=np.uint8))
        sizes = torch.tensor([[SIZE - (k + i) % 7, SIZE - (2 * k + i) % 5] for i in range(B)], dtype=torch.int32)
        out.append((raw, sizes, torch.tensor([(i + k) % 3 for i in range(B)])))
    return out


def _epoch(loss_cfg, **loader_kw):
    torch.manual_seed(0)
    model = get_model(CFG_MODEL, CLASSES, DEV)
    opt = get_optimizer(model, dict(type="sgd", lr=0.01))
    crit = get_loss(dict(task="single", type="CrossEntropyLoss", **loss_cfg), DEV)
    loader = D.DeviceLoader(_batches(), DEV, SIZE, hflip_p=0.5, seed=3, **loader_kw)
    res = train_epoch(model, loader, opt, None, torch.amp.GradScaler("cuda", enabled=False), crit, DEV, CFG, BaseLogger(CFG, CLASSES))
    return res


@pytest.mark.parametrize("spec", [dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"), dict(mixup_alpha=0.8, mode="batch"),
                                  dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="pair")], ids=["elem-both", "batch-mixup", "pair-cutmix"])
def test_train_epoch_with_mixup_and_label_smoothing(spec):
    runs = []
    for _ in range(2):
        res = _epoch(dict(label_smoothing=0.1), mixup=spec)
        losses = [float(v) for v in res["running_loss"]]
        assert len(losses) == NB and all(math.isfinite(v) for v in losses), losses
        assert [int(v) for v in res["ground_truth"]] == [(i + k) % 3 for k in range(NB) for i in range(B)]
        runs.append(losses)
    assert runs[0] == runs[1], runs
    plain = [float(v) for v in _epoch(dict(label_smoothing=0.1))["running_loss"]]
    assert plain[0] != runs[0][0], "the mixing loader's first loss equals the plain one"


def test_the_loader_hands_over_mixed_targets_and_mixed_images():
    spec = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")
    mixed = list(D.DeviceLoader(_batches(), DEV, SIZE, hflip_p=0.5, seed=3, mixup=spec))
    plain = list(D.DeviceLoader(_batches(), DEV, SIZE, hflip_p=0.5, seed=3))
    rng = np.random.default_rng(5)
    for k, ((img, tgt), (pimg, ptgt)) in enumerate(zip(mixed, plain)):
        bits, words, partner, lam = D.draw_batch_mix(rng, B, SIZE, spec)
        assert isinstance(tgt, MixedTarget) and tgt.device.type == "cuda"
        assert torch.equal(tgt.y.cpu(), ptgt.cpu()) and torch.equal(tgt.y2.cpu(), ptgt.cpu()[partner]) and torch.equal(tgt.lam.cpu(), lam)
        for i in range(B):
            assert torch.equal(img[i], pimg[i]) == (not bits[i]), (k, i)
    multi = list(D.DeviceLoader([(r, s, {"t1": y, "t2": y + 1}) for r, s, y in _batches()], DEV, SIZE, seed=3, mixup=spec))
    for img, tgt in multi:
        assert set(tgt) == {"t1", "t2"} and all(isinstance(v, MixedTarget) for v in tgt.values())
        assert torch.equal(tgt["t1"].lam, tgt["t2"].lam) and torch.equal(tgt["t1"].y + 1, tgt["t2"].y) and torch.equal(tgt["t1"].y2 + 1, tgt["t2"].y2)


def test_prob_zero_without_smoothing_is_the_plain_run():
    a = [float(v) for v in _epoch({})["running_loss"]]
    b = [float(v) for v in _epoch(dict(label_smoothing=0.0), mixup=dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0))["running_loss"]]
    assert a == b, (a, b)
