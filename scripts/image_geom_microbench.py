"""Time nkb_image_prep at 256 x 224 x 224 in eight configurations: the four of scripts/image_mix_microbench.py — plain (flip flags
only), records (every image with brightness/contrast, HSV shift and four holes), blend (Mixup with the partner B - 1 - b), box
(CutMix) — and four with geometry records (flag bit 4): resample (every image a RandomResizedCrop box cut from a 288-pixel source
canvas), blur3 and blur7 (every image blurred over a 3- / 7-tap line), and all (resample + 7 taps + records + blend).  HIP events
around groups of launches, warm-up first, the variants run in rotating order, median and spread over the rounds reported; bytes/s
from the bytes each configuration has to move per output pixel: 12 written, and read 3 (plain, records, box), 6 (blend), about 4
source bytes per bilinear footprint (resample: the box is read once however often its pixels are reused; counted as 3 x the mean
box area / output area), 3 (blur: the taps of neighbouring pixels overlap in cache).

--parent-lib PATH adds the first four launches through another build of libnkbhip.so (the parent commit's), TWICE — through two
handles of that library — to the alternation.  Both builds must give the same bits for the four; the spread is what the parent
differs from itself by (the 90th percentile over the rounds of |handle 1 - handle 2|), and the new build's median may exceed
the parent's by no more than that: the script exits with status 1 otherwise.
Usage (GPU box): python scripts/image_geom_microbench.py [--parent-lib path/to/libnkbhip.so] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nkb-classification_amd"))
from nkb_classification import dataset, hip  # noqa: E402

SHARED = ("plain", "records", "blend", "box")


def bind(path):
    lib = C.CDLL(path)
    res, args = hip._SIGS["nkb_image_prep"]
    lib.nkb_image_prep.restype, lib.nkb_image_prep.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--source", type=int, default=288)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed group")
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev, B, S, S2 = "cuda:0", a.batch, a.size, a.source
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    src2 = torch.from_numpy(rng.integers(0, 256, (B, S2, S2, 3), dtype=np.uint8)).to(dev)
    hw = torch.tensor([[S - (i % 9), S - (i % 5) * 3] for i in range(B)], dtype=torch.int32)
    hw2 = torch.tensor([[S2 - (i % 9), S2 - (i % 5) * 3] for i in range(B)], dtype=torch.int32)
    sizes, sizes2 = hw.to(dev), hw2.to(dev)
    flips = torch.from_numpy(rng.integers(0, 4, B).astype(np.uint8))
    spec = dict(brightness_contrast=dict(brightness_limit=(-0.2, 0.2), contrast_limit=(0.1, -0.5), p=1.0),
                hue_saturation_value=dict(hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20, p=1.0),
                coarse_dropout=dict(max_holes=4, min_holes=4, max_height=0.2, min_height=0.05, max_width=0.2, min_width=0.05,
                                    fill_value=[0, 0.5, 1], p=1.0))
    bits, rec = dataset.draw_image_aug(torch.Generator().manual_seed(1), B, S, spec)
    assert int(bits.min()) == 4 and bool((rec[:, 0] == 7).all())
    # name -> (flags buffer, source batch, sizes, source side, bytes read per output pixel)
    cfg = {"plain": (flips.to(dev), src, sizes, S, 3.0), "records": (hip.pack_image_aug(flips | bits, rec).to(dev), src, sizes, S, 3.0)}
    mixes = {}
    for name, mix in (("blend", dict(mixup_alpha=0.8, cutmix_alpha=0.0, mode="elem")), ("box", dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem"))):
        mbits, words, _, lam = dataset.draw_batch_mix(np.random.default_rng(2), B, S, mix)
        r = torch.zeros(B, hip.IMAGE_AUG_WORDS, dtype=torch.int32)
        r[:, 10:16] = words
        mixes[name] = (mbits, words)
        print(f"{name}: {int((mbits != 0).sum())} of {B} images mixed, mean lam {float(lam.mean()):.3f}")
        cfg[name] = (hip.pack_image_aug(flips | mbits, r).to(dev), src, sizes, S, 6.0 if name == "blend" else 3.0)
    crop = dict(random_resized_crop=dict(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), p=1.0))
    cbits, crec = dataset.draw_image_geom(torch.Generator().manual_seed(3), B, hw2, S, crop)
    area = float((crec[:, 3].double() * crec[:, 4].double()).mean()) / (S * S)
    print(f"resample: mean box area {area:.3f} of the output's")
    cfg["resample"] = (hip.pack_image_geom(flips | cbits, None, crec, sizes=hw2).to(dev), src2, sizes2, S2, 3.0 * area)
    blurs = {}
    for k in (3, 7):
        # a full-length line in every record, horizontal or diagonal by turns (the lines draw_image_geom draws are shorter on average)
        brec = torch.from_numpy(np.stack([hip.image_geom_record(
            taps=[((0, d - k // 2) if b % 2 else (d - k // 2, d - k // 2)) for d in range(k)]) for b in range(B)]))
        bbits = torch.full((B,), hip.IMAGE_GEOM_BIT, dtype=torch.uint8)
        assert bool((brec[:, 7] == k).all())
        blurs[k] = brec
        cfg[f"blur{k}"] = (hip.pack_image_geom(flips | bbits, None, brec, sizes=hw).to(dev), src, sizes, S, 3.0)
    allrec = rec.clone()
    allrec[:, 10:16] = mixes["blend"][1]
    allgeom = crec.clone()
    allgeom[:, 7:16] = blurs[7][:, 7:16]
    allgeom[:, 0] |= hip.IMAGE_GEOM_BLUR
    cfg["all"] = (hip.pack_image_geom(flips | bits | mixes["blend"][0] | cbits, allrec, allgeom, sizes=hw2).to(dev), src2, sizes2, S2,
                  6.0 * area)
    out = torch.empty(B, 3, S, S, device=dev)
    mean, std = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    stream = torch.cuda.current_stream().cuda_stream

    def launcher(lib, name):
        flags, s, sz, side, _ = cfg[name]
        fn, args = lib.nkb_image_prep, (s.data_ptr(), sz.data_ptr(), flags.data_ptr(), out.data_ptr(), B, side, side, S, S,
                                        C.cast(mean, C.c_void_p), C.cast(std, C.c_void_p), 0.0, stream)

        def run():
            if fn(*args):
                raise RuntimeError("nkb_image_prep failed")
        return run

    new = hip.load()
    variants = {k: launcher(new, k) for k in cfg}
    tmp = None
    if a.parent_lib:
        tmp = tempfile.mkdtemp()
        second = shutil.copy(a.parent_lib, os.path.join(tmp, "libnkbhip_parent2.so"))
        parent, parent2 = bind(a.parent_lib), bind(second)
        assert len({parent._handle, parent2._handle, new._handle}) == 3, "the three libraries must be three handles"
        for k in SHARED:
            variants[k + "_parent"], variants[k + "_parent2"] = launcher(parent, k), launcher(parent2, k)
            variants[k]()
            torch.cuda.synchronize()
            keep = out.clone()
            variants[k + "_parent"]()
            torch.cuda.synchronize()
            assert torch.equal(keep, out), f"the {k} launch differs between the two builds"
        print("plain, records, blend and box launches: both builds give the same bits")
    for run in variants.values():                      # warm-up: code objects loaded, clocks up
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
                variants[k]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.launches * 1e3)
    result = dict(batch=B, size=S, source=S2, launches=a.launches, rounds=a.rounds, mean_box_area=round(area, 4))
    for k, v in times.items():
        med = statistics.median(v)
        nbytes = B * S * S * (12.0 + cfg[k.split("_")[0]][4])
        result[k] = dict(median_us=round(med, 2), min_us=round(min(v), 2), max_us=round(max(v), 2), bytes_per_launch=int(nbytes),
                         tb_per_s=round(nbytes / med / 1e6, 3))
        print(f"{k:16s} median {med:8.2f} us  (min {min(v):8.2f}, max {max(v):8.2f} over {a.rounds} rounds of {a.launches})  "
              f"{nbytes / 1e6:6.1f} MB  {nbytes / med / 1e6:5.2f} TB/s")
    ok = True
    if a.parent_lib:
        for k in SHARED:
            diffs = sorted(abs(x - y) for x, y in zip(times[k + "_parent"], times[k + "_parent2"]))
            spread = diffs[min(len(diffs) - 1, int(0.9 * len(diffs)))]
            over = result[k]["median_us"] - result[k + "_parent"]["median_us"]
            result[k]["parent_spread_us"], result[k]["over_parent_us"], result[k]["within_spread"] = round(spread, 2), round(over, 2), over <= spread
            print(f"{k:16s} new - parent = {over:+7.2f} us, parent against itself {spread:6.2f} us: {'ok' if over <= spread else 'SLOWER'}")
            ok = ok and over <= spread
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
