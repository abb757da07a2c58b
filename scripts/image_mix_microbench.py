"""Time nkb_image_prep at 256 x 224 x 224 in four configurations: plain (flip flags only), records (every image with
brightness/contrast, HSV shift and four holes), blend (every image mixed with its partner B - 1 - b, Mixup) and box (every
image cut from its partner, CutMix, boxes drawn as dataset.draw_batch_mix draws them).  HIP events around groups of launches,
warm-up first, the variants run in rotating order, median and spread over the rounds reported; bytes/s from the 15 bytes per
output pixel an un-mixed launch has to move (a blend reads 3 more per pixel).

--parent-lib PATH adds the plain and the records launch through another build of libnkbhip.so (the parent commit's) to the
alternation and checks that both builds give the same bits for them.
Usage (GPU box): python scripts/image_mix_microbench.py [--parent-lib path/to/libnkbhip.so] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nkb-classification_amd"))
from nkb_classification import dataset, hip  # noqa: E402


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
    ap.add_argument("--launches", type=int, default=20, help="launches per timed group")
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev, B, S = "cuda:0", a.batch, a.size
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    sizes = torch.tensor([[S - (i % 9), S - (i % 5) * 3] for i in range(B)], dtype=torch.int32, device=dev)
    flips = torch.from_numpy(rng.integers(0, 4, B).astype(np.uint8))
    spec = dict(brightness_contrast=dict(brightness_limit=(-0.2, 0.2), contrast_limit=(0.1, -0.5), p=1.0),
                hue_saturation_value=dict(hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20, p=1.0),
                coarse_dropout=dict(max_holes=4, min_holes=4, max_height=0.2, min_height=0.05, max_width=0.2, min_width=0.05,
                                    fill_value=[0, 0.5, 1], p=1.0))
    bits, rec = dataset.draw_image_aug(torch.Generator().manual_seed(1), B, S, spec)
    assert int(bits.min()) == 4 and bool((rec[:, 0] == 7).all())
    buffers = {"plain": flips.to(dev), "records": hip.pack_image_aug(flips | bits, rec).to(dev)}
    for name, mix in (("blend", dict(mixup_alpha=0.8, cutmix_alpha=0.0, mode="elem")), ("box", dict(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem"))):
        mbits, words, _, lam = dataset.draw_batch_mix(np.random.default_rng(2), B, S, mix)
        r = torch.zeros(B, hip.IMAGE_AUG_WORDS, dtype=torch.int32)
        r[:, 10:16] = words
        print(f"{name}: {int((mbits != 0).sum())} of {B} images mixed, mean lam {float(lam.mean()):.3f}")
        buffers[name] = hip.pack_image_aug(flips | mbits, r).to(dev)
    out = torch.empty(B, 3, S, S, device=dev)
    mean, std = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    stream = torch.cuda.current_stream().cuda_stream

    def launcher(lib, flags):
        fn, args = lib.nkb_image_prep, (src.data_ptr(), sizes.data_ptr(), flags.data_ptr(), out.data_ptr(), B, S, S, S, S,
                                        C.cast(mean, C.c_void_p), C.cast(std, C.c_void_p), 0.0, stream)

        def run():
            if fn(*args):
                raise RuntimeError("nkb_image_prep failed")
        return run

    new = hip.load()
    variants = {k: launcher(new, v) for k, v in buffers.items()}
    if a.parent_lib:
        parent = bind(a.parent_lib)
        assert parent._handle != new._handle, "--parent-lib resolved to the library that is already loaded"
        for k in ("plain", "records"):
            variants[k + "_parent"] = launcher(parent, buffers[k])
            variants[k]()
            torch.cuda.synchronize()
            keep = out.clone()
            variants[k + "_parent"]()
            torch.cuda.synchronize()
            assert torch.equal(keep, out), f"the {k} launch differs between the two builds"
        print("plain and records launches: both builds give the same bits")
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
    nbytes = B * S * S * 15
    result = dict(batch=B, size=S, launches=a.launches, rounds=a.rounds, bytes_per_launch=nbytes)
    for k, v in times.items():
        med = statistics.median(v)
        result[k] = dict(median_us=round(med, 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                         tb_per_s=round(nbytes / med / 1e6, 3))
        print(f"{k:15s} median {med:7.2f} us  (min {min(v):7.2f}, max {max(v):7.2f} over {a.rounds} rounds of {a.launches})  "
              f"{nbytes / med / 1e6:5.2f} TB/s")
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
