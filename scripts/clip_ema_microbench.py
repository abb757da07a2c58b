"""Time the streaming passes behind gradient clipping and weight EMA, alone and inside a train step.

Standalone (default): on arenas the size of ResNet-50's, ViT-B/16's and 573 M elements (unicom ViT-L/14's), the clip-norm pass
(nkb_segment_sumsq over the equal chunks of hip.clip_chunks, 4 B per parameter), the EMA launch without and with its bf16 shadow
(12 / 14 B), and the Adam launch without and with NKB_OPTIM_CLIP_NORM (30 B), each in us and GB/s.  HIP events around groups of
launches, warm-up first, the variants in rotating order, median and spread over the rounds.

--step: one bf16 vit_base_patch16_224 train step at batch 256 (the setup of scripts/vit_mix_step.py: resident uint8 batch ->
nkb_image_prep -> model -> cross entropy -> backward -> AdamW), plain, with clip_grad_norm_(1.0) and with clipping and
ModelEma.update(), alternating block by block, plus the launch counts of one step of each.  On a tree from before the feature only
the plain step runs, so the same command in a checkout of the parent commit gives the figure to set beside it.
Usage (GPU box): python scripts/clip_ema_microbench.py [--step] [--sizes 25600000,86600000,573000000] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nkb-classification_amd"))
from nkb_classification import hip  # noqa: E402


def standalone(a):
    dev = "cuda:0"
    result = dict(launches=a.launches, rounds=a.rounds, sizes={})
    for n in [int(s) for s in a.sizes.split(",")]:
        n = (n + 63) // 64 * 64
        p, g, m, e = (torch.randn(n, device=dev) * 0.02 for _ in range(4))
        v = torch.rand(n, device=dev) * 1e-4
        shadow, eshadow = (torch.empty(n, device=dev, dtype=torch.bfloat16) for _ in range(2))
        offs = hip.clip_chunk_offsets(n)
        P = len(offs) - 1
        offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
        rec = torch.zeros(hip.OPTIM_RECORD_HEAD + P, device=dev)
        rec[1], rec[2] = 1.0, float(P)
        adam = (1e-9, 0.0, 0.9, 0.999, 1e-8, 1.0, 1e-9, 1.0)        # lr, wd, betas, eps, grad_scale, c0, c1: the weights barely move
        variants = {
            "adam": (30, lambda: hip.optim_step(0, p, g, m, v, shadow, n, *adam)),
            "adam_clip_norm": (30, lambda: hip.optim_step(hip.OPTIM_CLIP_NORM, p, g, m, v, shadow, n, *adam, skip_flag=rec)),
            "norm_pass": (4, lambda: hip.segment_sumsq(g, offsets, P, rec[hip.OPTIM_RECORD_HEAD:])),
            "ema": (12, lambda: hip.ema_step(e, p, None, n, 0.9998)),
            "ema_shadow": (14, lambda: hip.ema_step(e, p, eshadow, n, 0.9998)),
        }
        for _, run in variants.values():
            for _ in range(a.launches):
                run()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        names = list(variants)
        for r in range(a.rounds):
            order = names[r % len(names):] + names[:r % len(names)]
            if (r // len(names)) % 2:
                order.reverse()
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    variants[k][1]()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.launches * 1e3)
        row = dict(chunks=P, chunk_len=offs[1] - offs[0])
        for k, t in times.items():
            med = statistics.median(t)
            gbs = variants[k][0] * n / med / 1e3
            row[k] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2), gb_per_s=round(gbs, 1))
            print(f"n {n:>11d}  {k:15s} median {med:9.2f} us  (min {min(t):9.2f}, max {max(t):9.2f})  {gbs:7.1f} GB/s")
        result["sizes"][str(n)] = row
        del p, g, m, v, e, shadow, eshadow
        torch.cuda.empty_cache()
    return result


def whole_step(a):
    from nkb_classification import utils
    from nkb_classification.losses import get_loss
    from nkb_classification.model import get_model
    dev, B, S = "cuda:0", a.batch, 224
    torch.manual_seed(0)
    cfg = dict(task="single", model=a.model, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0,
               classifier_initialization="kaiming_normal_")
    model = get_model(cfg, [str(i) for i in range(1000)], dev)
    opt = utils.get_optimizer(model, dict(type="adamw", lr=1e-4, backbone_lr=1e-5, classifier_lr=1e-4, weight_decay=0.05,
                                          backbone_weight_decay=0.05, classifier_weight_decay=0.05))
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), dev)
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    y = torch.randint(0, 1000, (B,)).to(dev)
    flips = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).to(dev)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    model.train()
    kinds = ["plain"]
    ema = None
    if hasattr(opt, "clip_grad_norm_"):
        from nkb_classification.ema import ModelEma
        ema = ModelEma(model, decay=0.9998)
        kinds += ["clip", "clip_ema"]

    def step(k):
        img = torch.empty(B, 3, S, S, device=dev)
        hip.image_prep(src, None, flips, img, B, S, S, S, S, mean, std, 0.0)
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(model(img), y)
        loss.backward()
        if k != "plain":
            opt.clip_grad_norm_(1.0)
        opt.step()
        if k == "clip_ema":
            ema.update()
        return loss

    for _ in range(a.warmup):
        for k in kinds:
            step(k)
    torch.cuda.synchronize()
    launches = {}
    hip.prof_collect()
    for k in kinds:                              # launches of one step of each kind, per kernel family, from the library's profiler
        hip.prof_enable(True)
        step(k)
        torch.cuda.synchronize()
        launches[k] = {name: row["launches"] for name, row in sorted(hip.prof_collect().items())}
        hip.prof_enable(False)
        launches[k]["total"] = sum(launches[k].values())
    blocks = {k: [] for k in kinds}
    for r in range(a.rounds):
        order = kinds[r % len(kinds):] + kinds[:r % len(kinds)]
        for k in order:
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step(k)
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert torch.isfinite(loss).item()
    return dict(model=a.model, batch=B, arena=model.arena.total, launches_per_step=launches,
                **{k: dict(ms_per_step=round(statistics.median(t), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
                   for k, t in blocks.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--sizes", default="25600000,86600000,573000000")
    ap.add_argument("--launches", type=int, default=10, help="launches per timed group")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    result = whole_step(a) if a.step else standalone(a)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
