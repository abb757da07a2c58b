"""One ViT train step from a resident uint8 batch, timed with and without Mixup / CutMix and label smoothing: nkb_image_prep
(flips only | every image mixed with its partner, blends and boxes as dataset.draw_batch_mix draws them) -> model -> cross entropy
(plain labels | MixedTarget with label_smoothing 0.1) -> backward -> optimizer; vit_base_patch16_224, batch 256, bf16, AdamW.
The two variants share model and optimizer and alternate block by block.  Prints one JSON line: ms per step, median and
min .. max over ROUNDS blocks of STEPS steps, for each variant.
Usage: python scripts/vit_mix_step.py [--batch 256] [--model vit_base_patch16_224]"""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(R, "nkb-classification_amd"))
from nkb_classification import dataset, hip
from nkb_classification.losses import MixedTarget, get_loss
from nkb_classification.model import get_model
from nkb_classification.utils import get_optimizer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--model", default="vit_base_patch16_224")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=6)
args = ap.parse_args()
dev, B, S = "cuda:0", args.batch, 224
torch.manual_seed(0)
cfg = dict(task="single", model=args.model, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0,
           classifier_initialization="kaiming_normal_")
model = get_model(cfg, [str(i) for i in range(1000)], dev)
opt = get_optimizer(model, dict(type="adamw", lr=1e-4, backbone_lr=1e-5, classifier_lr=1e-4, weight_decay=0.05,
                                backbone_weight_decay=0.05, classifier_weight_decay=0.05))
crit = {"plain": get_loss(dict(task="single", type="CrossEntropyLoss"), dev),
        "mixed": get_loss(dict(task="single", type="CrossEntropyLoss", label_smoothing=0.1), dev)}
rng = np.random.default_rng(0)
src = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
y = torch.randint(0, 1000, (B,))
flips = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8))
mbits, words, partner, lam = dataset.draw_batch_mix(np.random.default_rng(2), B, S, dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"))
rec = torch.zeros(B, hip.IMAGE_AUG_WORDS, dtype=torch.int32)
rec[:, 10:16] = words
flags = {"plain": flips.to(dev), "mixed": hip.pack_image_aug(flips | mbits, rec).to(dev)}
target = {"plain": y.to(dev), "mixed": MixedTarget.build(y, y[partner], lam).to(dev)}
mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
model.train()


def step(k):
    img = torch.empty(B, 3, S, S, device=dev)
    hip.image_prep(src, None, flags[k], img, B, S, S, S, S, mean, std, 0.0)
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = crit[k](model(img), target[k])
    loss.backward()
    opt.step()
    return loss


for _ in range(args.warmup):
    for k in flags:
        step(k)
torch.cuda.synchronize()
blocks = {k: [] for k in flags}
for r in range(args.rounds):
    for k in (("plain", "mixed") if r % 2 == 0 else ("mixed", "plain")):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step(k)
        torch.cuda.synchronize()
        blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        assert torch.isfinite(loss).item()
print(json.dumps(dict(model=args.model, batch=B, mixed_images=int((mbits != 0).sum()),
                      **{k: dict(ms_per_step=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3))
                         for k, v in blocks.items()})))
