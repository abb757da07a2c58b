"""Minimal input side for train.py: `get_dataset(data, pipeline) -> DataLoader` (signature of
/root/reference/nkb_classification/dataset.py:541-629).

The reference's five annotation-file dataset types stay CPU-side input code outside the accelerated path and are not
rebuilt, and of its albumentations stack only what its two training configs use is.  What IS here:
  * `DeviceLoader`: the loader hands over pinned **uint8** HWC batches; the H2D copy runs on a copy stream one batch
    ahead of the train step, and everything behind LongestMaxSize in the stack of configs/singletask_config.py:162-201 —
    PadIfNeeded -> HorizontalFlip -> VerticalFlip -> RandomBrightnessContrast -> HueSaturationValue -> CoarseDropout ->
    Normalize -> ToTensorV2 — runs on the GPU in one launch (`nkb_image_prep`), so engine.py:40's `img.to(device)` finds
    the batch already resident.  The three augmentations are per-image records drawn here (`draw_image_aug`, from a
    second generator seeded `seed + 1`) and carried behind the flag bytes (`hip.pack_image_aug`); `translate_pipeline`
    reads them off an albumentations-style Compose.  Sampling rules and attribute names restate albumentations 1.x, the
    kernel's 8-bit HSV conversions restate OpenCV's — from memory, neither is a dependency: parity with them is UNPINNED;
    the geometry of the archived stacks and of the timm recipes rides in a second table of per-image records in the same
    launch: PadIfNeeded's BORDER_REFLECT_101 (`pad_border`), MotionBlur (`motion_blur`) and RandomResizedCrop
    (`random_resized_crop`, cut from a host canvas of `source_size` pixels), drawn by `draw_image_geom` from a fourth
    generator seeded `seed + 3` (`hip.pack_image_geom`); applied as crop -> flips -> blur -> colour -> mix;
  * `ImbalancedDatasetSampler` (dataset.py:27-86: weights 1 / count[label], `torch.multinomial` with replacement) and
    `ShardedSampler` (one process per GPU: rank r takes indices r::W of a seed-shared permutation);
  * `get_dataset` honours `shuffle`, `weighted_sampling`, `drop_last`, `num_workers` (dataset.py:606-628).
Two sources are provided so the config-driven train.py runs end to end:
  * type "synthetic": seeded randn images / randint labels held in memory (the benchmark's input);
  * default (no/unknown "type" with a "root"): an ImageFolder walk (root/<class>/<image>) decoded with PIL,
    resized, scaled to [0,1] and normalised — `loader.dataset.classes` is the sorted class-folder list, as
    train.py:94 expects.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Sampler

_EXT = {".png", ".jpg", ".jpeg", ".bmp", ".webp"}


class SyntheticDataset(Dataset):
    def __init__(self, n_images, classes, size=224, seed=1234):
        g = torch.Generator().manual_seed(seed)
        self.classes = classes
        self.images = torch.randn(n_images, 3, size, size, generator=g)
        if isinstance(classes, dict):
            self.labels = {t: torch.randint(0, len(c), (n_images,), generator=g) for t, c in classes.items()}
        else:
            self.labels = torch.randint(0, len(classes), (n_images,), generator=g)

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        if isinstance(self.labels, dict):
            return self.images[i], {t: int(v[i]) for t, v in self.labels.items()}
        return self.images[i], int(self.labels[i])


class FolderDataset(Dataset):
    """raw=True: items are (uint8 HWC image resized so that its longest side is `source_size` and placed top-left in a
    source_size x source_size canvas, (h, w), label) for DeviceLoader; raw=False: normalised float CHW, squashed to size x size.
    source_size (default: size) is the host's LongestMaxSize target; a larger one than `size` gives the device's
    RandomResizedCrop more pixels to cut from than it writes."""

    def __init__(self, root, size=224, classes=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), raw=False,
                 source_size=None):
        self.raw = raw
        self.source_size = int(size if source_size is None else source_size)
        if self.source_size != size and not raw:
            raise ValueError("FolderDataset: source_size belongs to raw=True (the device pipeline)")
        root = Path(root)
        self.classes = classes or sorted(d.name for d in root.iterdir() if d.is_dir())
        self.items = [(p, i) for i, c in enumerate(self.classes) for p in sorted((root / c).iterdir())
                      if p.suffix.lower() in _EXT]
        self.size = size
        self.mean = np.asarray(mean, np.float32).reshape(3, 1, 1)
        self.std = np.asarray(std, np.float32).reshape(3, 1, 1)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        path, label = self.items[i]
        img = Image.open(path).convert("RGB")
        if self.raw:
            # A.LongestMaxSize(source_size): scale so that max(h, w) == source_size (host side; decoding is here anyway)
            k = self.source_size / max(img.size)
            w, h = max(1, round(img.size[0] * k)), max(1, round(img.size[1] * k))
            canvas = np.zeros((self.source_size, self.source_size, 3), np.uint8)
            canvas[:h, :w] = np.asarray(img.resize((w, h)), np.uint8)
            return torch.from_numpy(canvas), torch.tensor([h, w], dtype=torch.int32), label
        arr = np.asarray(img.resize((self.size, self.size)), np.float32).transpose(2, 0, 1) / 255.0
        return torch.from_numpy((arr - self.mean) / self.std), label

    def get_labels(self):
        return [label for _, label in self.items]


class ImbalancedDatasetSampler(Sampler):
    """dataset.py:27-86: every index is drawn with probability proportional to 1 / (number of samples of its label),
    `num_samples` draws with replacement per epoch.  With world > 1 each rank draws its own `num_samples / world`
    from a generator seeded `seed + rank`."""

    def __init__(self, dataset, labels=None, indices=None, num_samples=None, seed=None, rank=0, world=1):
        self.indices = list(range(len(dataset))) if indices is None else list(indices)
        labels = dataset.get_labels() if labels is None else labels
        labels = [int(labels[i]) for i in self.indices]
        counts = {}
        for v in labels:
            counts[v] = counts.get(v, 0) + 1
        self.weights = torch.DoubleTensor([1.0 / counts[v] for v in labels])
        total = len(self.indices) if num_samples is None else num_samples
        self.num_samples = total if world == 1 else (total + world - 1) // world
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator().manual_seed(int(seed) + rank)

    def __iter__(self):
        draws = torch.multinomial(self.weights, self.num_samples, replacement=True, generator=self.generator)
        return (self.indices[i] for i in draws)

    def __len__(self):
        return self.num_samples


class ShardedSampler(Sampler):
    """Data-parallel split: the same seeded permutation on every rank (re-drawn per epoch through set_epoch), rank r taking
    positions r::world.  pad=True (training: every rank must run the same number of steps, the gradient exchange is a
    collective) repeats the first indices up to a multiple of the world size — `real_len` tells how many of this rank's samples
    are NOT such repeats, so that gathered epoch results can drop them; pad=False (validation: no collective runs inside
    val_epoch) leaves the shards uneven and every sample is seen exactly once."""

    def __init__(self, n, rank, world, shuffle=True, seed=0, pad=True):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0
        self.pad = pad
        self.real_len = max(0, (n - rank + world - 1) // world)
        self.num_samples = (n + world - 1) // world if pad else self.real_len

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        if self.shuffle:
            order = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + self.epoch)).tolist()
        else:
            order = list(range(self.n))
        if self.pad:
            order += order[: self.num_samples * self.world - self.n]
        return iter(order[self.rank::self.world])

    def __len__(self):
        return self.num_samples


# ---- device-side colour augmentations and CoarseDropout: the host draws -------------------------------------------------------------
# The kernel applies what a per-image record says (include/nkbhip.h); this is where the records come from.  Argument names
# and sampling rules restate albumentations 1.x from memory (the library is not a dependency): parity with it is UNPINNED.
AUG_KEYS = ("brightness_contrast", "hue_saturation_value", "coarse_dropout")
MAX_HOLES = 12
_AUG_DEFAULTS = {
    "brightness_contrast": dict(brightness_limit=0.2, contrast_limit=0.2, brightness_by_max=True, p=0.5),
    "hue_saturation_value": dict(hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20, p=0.5),
    "coarse_dropout": dict(max_holes=8, max_height=8, max_width=8, min_holes=None, min_height=None, min_width=None,
                           fill_value=0, p=0.5),
}


def _limit(x):
    """a scalar limit x means (-x, x); a pair is kept in its order (random.uniform takes reversed bounds as they are)"""
    if isinstance(x, (tuple, list)):
        if len(x) != 2:
            raise ValueError(f"a limit is a number or a pair, got {x!r}")
        return (x[0], x[1])
    return (-x, x)


def normalise_aug_spec(spec):
    """{key of AUG_KEYS: None or dict of albumentations' argument names plus p} -> the same with defaults filled in, limits as
    pairs and the fill value as three uint8 levels; None when no transform is asked for.  Refuses what the kernel cannot do."""
    spec = spec or {}
    unknown = set(spec) - set(AUG_KEYS)
    if unknown:
        raise ValueError(f"unknown augmentation keys {sorted(unknown)}; known: {AUG_KEYS}")
    out = {}
    for key in AUG_KEYS:
        if spec.get(key) is None:
            continue
        extra = set(spec[key]) - set(_AUG_DEFAULTS[key])
        if extra:
            raise ValueError(f"{key}: unknown arguments {sorted(extra)}; known: {sorted(_AUG_DEFAULTS[key])}")
        out[key] = {**_AUG_DEFAULTS[key], **spec[key]}
    if not out:
        return None
    bc, hsv, cd = (out.get(k) for k in AUG_KEYS)
    if bc is not None:
        if not bc["brightness_by_max"]:
            raise NotImplementedError("brightness_contrast: only brightness_by_max=True (offset = beta * 255) is built")
        bc["brightness_limit"], bc["contrast_limit"] = _limit(bc["brightness_limit"]), _limit(bc["contrast_limit"])
    if hsv is not None:
        for k in ("hue_shift_limit", "sat_shift_limit", "val_shift_limit"):
            hsv[k] = _limit(hsv[k])
    if cd is not None:
        for k in ("holes", "height", "width"):
            if cd["min_" + k] is None:
                cd["min_" + k] = cd["max_" + k]
        if cd["max_holes"] > MAX_HOLES:
            raise ValueError(f"coarse_dropout: max_holes = {cd['max_holes']} exceeds the {MAX_HOLES} boxes a record holds")
        if not 0 <= cd["min_holes"] <= cd["max_holes"]:
            raise ValueError(f"coarse_dropout: need 0 <= min_holes <= max_holes, got {cd['min_holes']}, {cd['max_holes']}")
        for k in ("height", "width"):
            lo, hi = cd["min_" + k], cd["max_" + k]
            if isinstance(lo, float) != isinstance(hi, float) or not 0 <= lo <= hi or (isinstance(hi, float) and hi >= 1.0):
                raise ValueError(f"coarse_dropout: min_{k} / max_{k} are both pixel counts or both fractions below 1 with "
                                 f"min <= max, got {lo!r}, {hi!r}")
        fv = cd["fill_value"]
        if isinstance(fv, str):
            raise NotImplementedError(f"coarse_dropout: fill_value {fv!r} is not built (numbers only)")
        fv = np.broadcast_to(np.asarray(fv, np.float64), (3,))
        cd["fill_value"] = tuple(int(a) for a in fv.astype(np.int64).astype(np.uint8))    # as numpy casts into a uint8 image
    return out


def aug_table_columns(spec):
    """K of the per-batch torch.rand(B, K) table (spec: normalised)"""
    k = 0
    if "brightness_contrast" in spec:
        k += 3
    if "hue_saturation_value" in spec:
        k += 4
    if "coarse_dropout" in spec:
        k += 2 + 4 * spec["coarse_dropout"]["max_holes"]
    return k


def _uniform(lim, u):
    return lim[0] + (lim[1] - lim[0]) * u


def _randint(lo, hi, u):
    """random.randint(lo, hi) (both ends included) from a uniform u in [0, 1)"""
    return np.minimum(lo + np.floor(u * (hi - lo + 1)).astype(np.int64), hi)


def draw_image_aug(gen, B, size, spec):
    """The augmentation draws of one batch -> (bits uint8 [B]: 4 where the image has a record, records int32 [B, 64]).

    ONE table u = torch.rand(B, K, generator=gen) per batch, K = aug_table_columns(spec), columns in this fixed order (a
    transform that is None takes no columns; every column is drawn whether or not its transform applies to the image):
      brightness_contrast   [apply, contrast, brightness]: applied where apply < p; alpha = 1 + U(contrast_limit),
                            beta = U(brightness_limit), offset = float32(beta * 255);
      hue_saturation_value  [apply, hue, sat, val]: float shifts U(limit);
      coarse_dropout        [apply, count, then (height, width, y, x) for each of max_holes boxes]: n = randint(min_holes,
                            max_holes) boxes, the first n quadruples; hole height int(size * U(min, max)) for fractions,
                            randint(min, max) for pixel counts (width alike); y1 = randint(0, size - height), x1 alike.
    U(lo, hi) = lo + (hi - lo) u and randint(lo, hi) = lo + floor(u (hi - lo + 1)), as random.uniform / random.randint."""
    from .hip import IMAGE_AUG_BIT, IMAGE_AUG_WORDS
    spec = normalise_aug_spec(spec)
    rec = np.zeros((B, IMAGE_AUG_WORDS), np.int32)
    if spec is None:
        return torch.zeros(B, dtype=torch.uint8), torch.from_numpy(rec)
    u = torch.rand(B, aug_table_columns(spec), generator=gen).double().numpy()
    f = rec.view(np.float32)
    f[:, 1] = 1.0
    col = 0
    bc, hsv, cd = (spec.get(k) for k in AUG_KEYS)
    if bc is not None:
        on = u[:, col] < bc["p"]
        alpha = 1.0 + _uniform(bc["contrast_limit"], u[:, col + 1])
        beta = _uniform(bc["brightness_limit"], u[:, col + 2])
        rec[:, 0] |= on.astype(np.int32)
        f[:, 1] = np.where(on, alpha, 1.0).astype(np.float32)
        f[:, 2] = np.where(on, beta * 255.0, 0.0).astype(np.float32)
        col += 3
    if hsv is not None:
        on = u[:, col] < hsv["p"]
        rec[:, 0] |= on.astype(np.int32) << 1
        for j, k in enumerate(("hue_shift_limit", "sat_shift_limit", "val_shift_limit")):
            f[:, 3 + j] = np.where(on, _uniform(hsv[k], u[:, col + 1 + j]), 0.0).astype(np.float32)
        col += 4
    if cd is not None:
        on = u[:, col] < cd["p"]
        rec[:, 0] |= on.astype(np.int32) << 2
        n = _randint(cd["min_holes"], cd["max_holes"], u[:, col + 1])
        rec[:, 6] = np.where(on, n, 0)
        rec[:, 7:10] = np.where(on[:, None], np.asarray(cd["fill_value"], np.int32), 0)
        col += 2
        for k in range(cd["max_holes"]):
            ext = []
            for j, name in enumerate(("height", "width")):
                lo, hi = cd["min_" + name], cd["max_" + name]
                if isinstance(hi, float):
                    ext.append((size * _uniform((lo, hi), u[:, col + j])).astype(np.int64))
                else:
                    ext.append(np.minimum(_randint(lo, hi, u[:, col + j]), size))
            y1 = _randint(0, size - ext[0], u[:, col + 2])
            x1 = _randint(0, size - ext[1], u[:, col + 3])
            box = np.stack([y1, x1, y1 + ext[0], x1 + ext[1]], 1)
            rec[:, 16 + 4 * k:20 + 4 * k] = np.where((on & (k < n))[:, None], box, 0)
            col += 4
    bits = np.where(rec[:, 0] != 0, IMAGE_AUG_BIT, 0).astype(np.uint8)
    return torch.from_numpy(bits), torch.from_numpy(rec)


# ---- device-side geometry: RandomResizedCrop, MotionBlur and the reflect-101 pad border: the host draws ----------------------------------
# The kernel applies what a per-image geometry record says (flag bit 4, include/nkbhip.h); this is where those records come from.
# Argument names and sampling rules restate torchvision / albumentations 1.x from memory: parity with them is UNPINNED.
GEOM_KEYS = ("random_resized_crop", "motion_blur")
PAD_BORDERS = ("constant", "reflect_101")
CROP_ATTEMPTS = 10
_GEOM_DEFAULTS = {
    "random_resized_crop": dict(scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p=1.0),
    "motion_blur": dict(blur_limit=7, allow_shifted=True, p=0.5),
}


def normalise_geom_spec(spec):
    """{random_resized_crop, motion_blur: None or a dict of albumentations' argument names plus p; pad_border: None, "constant" or
    "reflect_101"} -> the same with defaults filled in, blur_limit as a pair of odd kernel sizes (a scalar limit means (3, limit))
    and pad_border always present; None when nothing is asked for (no transform, constant border).  Refuses what the kernel
    cannot do: kernel sizes that are even, below 3 or above 15 (a record holds 16 taps), scale / ratio outside 0 < lo <= hi."""
    spec = spec or {}
    unknown = set(spec) - set(GEOM_KEYS) - {"pad_border"}
    if unknown:
        raise ValueError(f"unknown geometry keys {sorted(unknown)}; known: {GEOM_KEYS + ('pad_border',)}")
    border = spec.get("pad_border") or "constant"
    if border not in PAD_BORDERS:
        raise ValueError(f"pad_border {border!r}; known: {PAD_BORDERS}")
    out = {}
    for key in GEOM_KEYS:
        if spec.get(key) is None:
            continue
        extra = set(spec[key]) - set(_GEOM_DEFAULTS[key])
        if extra:
            raise ValueError(f"{key}: unknown arguments {sorted(extra)}; known: {sorted(_GEOM_DEFAULTS[key])}")
        out[key] = {**_GEOM_DEFAULTS[key], **spec[key]}
        if not 0.0 <= out[key]["p"] <= 1.0:
            raise ValueError(f"{key}: p = {out[key]['p']!r} is no probability")
    if not out and border == "constant":
        return None
    rrc, mb = (out.get(k) for k in GEOM_KEYS)
    if rrc is not None:
        for k in ("scale", "ratio"):
            v = rrc[k]
            if not isinstance(v, (tuple, list)) or len(v) != 2 or not 0 < v[0] <= v[1]:
                raise ValueError(f"random_resized_crop: {k} must be a pair with 0 < lo <= hi, got {v!r}")
            rrc[k] = (float(v[0]), float(v[1]))
    if mb is not None:
        lim = mb["blur_limit"]
        lim = tuple(lim) if isinstance(lim, (tuple, list)) else (3, lim)
        if len(lim) != 2 or any(int(k) != k or k % 2 == 0 or k < 3 or k > 15 for k in lim) or lim[0] > lim[1]:
            raise ValueError(f"motion_blur: blur_limit needs odd kernel sizes in 3..15 with lo <= hi, got {mb['blur_limit']!r}")
        mb["blur_limit"] = (int(lim[0]), int(lim[1]))
        mb["allow_shifted"] = bool(mb["allow_shifted"])
    out["pad_border"] = border
    return out


def geom_table_columns(spec):
    """K of the per-batch torch.rand(B, K) table of draw_image_geom (spec: normalised)"""
    return (1 + 4 * CROP_ATTEMPTS if "random_resized_crop" in spec else 0) + (8 if "motion_blur" in spec else 0)


def line_taps(y1, x1, y2, x2):
    """The 8-connected pixels of the line (x1, y1) -> (x2, y2) as [(y, x)]: one pixel per step along the longer axis,
    max(|dx|, |dy|) + 1 in all; the other coordinate is k * d / L rounded half up over the first half of the steps and mirrored over
    the second, so that a line whose ends are point-symmetric about a centre has point-symmetric pixels (Bresenham's pixels up to
    the tie rule; cv2.line's own tie rule is not restated)."""
    dy, dx = y2 - y1, x2 - x1
    L = max(abs(dx), abs(dy))
    if L == 0:
        return [(y1, x1)]
    along_x = abs(dx) >= abs(dy)
    d_major, d_minor = (dx, dy) if along_x else (dy, dx)
    D, s_major, s_minor = abs(d_minor), (1 if d_major > 0 else -1), (1 if d_minor > 0 else -1)
    out = []
    for k in range(L + 1):
        kk = k if 2 * k <= L else L - k
        m = (2 * kk * D + L) // (2 * L)
        if 2 * k > L:
            m = D - m
        a, b = s_major * k, s_minor * m
        out.append((y1 + b, x1 + a) if along_x else (y1 + a, x1 + b))
    return out


def _make_odd(v1, v2):
    """albumentations' make_odd_val: an even number of pixels between v1 and v2 loses one at the larger end"""
    if (abs(v1 - v2) + 1) % 2 != 1:
        if v2 > v1:
            v2 -= 1
        else:
            v1 -= 1
    return v1, v2


def draw_image_geom(gen, B, sizes, size, spec):
    """The geometry draws of one batch -> (bits uint8 [B]: 16 where the image has a geometry record, records int32 [B, 16]).
    sizes: None (every image is size x size) or [B, 2], the h and w of each image in its source slot; size: the output side.

    ONE table u = torch.rand(B, K, generator=gen) per batch, K = geom_table_columns(spec), columns in this fixed order (a transform
    that is None takes no columns; every column is drawn whether or not it is used):
      random_resized_crop  [apply, then 10 x (area, log-ratio, row, col)], applied where apply < p.  torchvision's / albumentations'
                           rule on the image's own h x w: area = U(scale) h w, aspect = exp(U(log r0, log r1)),
                           bw = round(sqrt(area aspect)), bh = round(sqrt(area / aspect)); the first attempt with 0 < bw <= w and
                           0 < bh <= h wins with y0 = randint(0, h - bh), x0 = randint(0, w - bw) from ITS row and col columns;
                           after ten misses the central crop with the aspect clamped into `ratio`.  The record carries the box
                           and the two scales float32(bh) / float32(size), float32(bw) / float32(size).
      motion_blur          [apply, ksize, x1, x2, y1, y2, shift_x, shift_y], applied where apply < p.  Restated from albumentations
                           1.x MotionBlur.get_params: ksize = a uniform choice among the odd sizes of blur_limit; the endpoints x1,
                           x2 = randint(0, ksize - 1) each; y1 likewise; y2 likewise where x1 != x2, else one of the ksize - 1
                           OTHER rows (random.sample of two rows), so the endpoints are distinct.  allow_shifted=False: both
                           extents are made odd in length (make_odd_val) and the line is centred in the kernel.
                           allow_shifted=True: the line is translated by shift_x = randint(-min(x1, x2), ksize - 1 - max(x1, x2))
                           and shift_y alike, which keeps it inside the kernel — the explicit shift columns are this
                           restatement's (1.x leaves the drawn endpoints where they are; both place the line uniformly).  The
                           kernel's ones are line_taps(endpoints) in place of cv2.line; the record carries them as (dy, dx)
                           offsets from the kernel centre ksize // 2, equal weights (kernel / kernel.sum()).
    pad_border "reflect_101" sets mask bit 2 in every record and draws nothing.  U and randint as in draw_image_aug."""
    from .hip import IMAGE_GEOM_BIT, IMAGE_GEOM_BLUR, IMAGE_GEOM_REFLECT, IMAGE_GEOM_WORDS, image_geom_record
    spec = normalise_geom_spec(spec)
    rec = np.zeros((B, IMAGE_GEOM_WORDS), np.int32)
    if spec is None or B == 0:
        return torch.zeros(B, dtype=torch.uint8), torch.from_numpy(rec)
    K = geom_table_columns(spec)
    u = torch.rand(B, K, generator=gen).double().numpy() if K else None
    hw = np.full((B, 2), size, np.int64) if sizes is None else np.asarray(sizes).astype(np.int64).reshape(B, 2)
    h, w = hw[:, 0], hw[:, 1]
    col = 0
    rrc, mb = (spec.get(k) for k in GEOM_KEYS)
    if spec["pad_border"] == "reflect_101":
        rec[:, 0] |= IMAGE_GEOM_REFLECT
    if rrc is not None:
        on = u[:, col] < rrc["p"]
        logr = (np.log(rrc["ratio"][0]), np.log(rrc["ratio"][1]))
        done = np.zeros(B, bool)
        box = np.zeros((B, 4), np.int64)
        for a in range(CROP_ATTEMPTS):
            c = col + 1 + 4 * a
            area = _uniform(rrc["scale"], u[:, c]) * h * w
            aspect = np.exp(_uniform(logr, u[:, c + 1]))
            bw = np.rint(np.sqrt(area * aspect)).astype(np.int64)
            bh = np.rint(np.sqrt(area / aspect)).astype(np.int64)
            ok = (bw > 0) & (bw <= w) & (bh > 0) & (bh <= h) & ~done
            y0 = _randint(0, np.maximum(h - bh, 0), u[:, c + 2])
            x0 = _randint(0, np.maximum(w - bw, 0), u[:, c + 3])
            box[ok] = np.stack([y0, x0, bh, bw], 1)[ok]
            done |= ok
        in_ratio = w / h
        fw = np.where(in_ratio > rrc["ratio"][1], np.rint(h * rrc["ratio"][1]), w).astype(np.int64)
        fh = np.where(in_ratio < rrc["ratio"][0], np.rint(w / rrc["ratio"][0]), h).astype(np.int64)
        fh, fw = np.clip(fh, 1, h), np.clip(fw, 1, w)
        box[~done] = np.stack([(h - fh) // 2, (w - fw) // 2, fh, fw], 1)[~done]
        rec[:, 0] |= on.astype(np.int32)
        rec[:, 1:5] = np.where(on[:, None], box, 0)
        f = rec.view(np.float32)
        f[:, 5] = np.where(on, box[:, 2].astype(np.float32) / np.float32(size), np.float32(0))
        f[:, 6] = np.where(on, box[:, 3].astype(np.float32) / np.float32(size), np.float32(0))
        col += 1 + 4 * CROP_ATTEMPTS
    if mb is not None:
        lo, hi = mb["blur_limit"]
        on = u[:, col] < mb["p"]
        ks = lo + 2 * _randint(0, (hi - lo) // 2, u[:, col + 1])
        for b in np.nonzero(on)[0]:
            k = int(ks[b])
            x1, x2, y1 = (int(_randint(0, k - 1, u[b, col + j])) for j in (2, 3, 4))
            if x1 == x2:
                y2 = int(_randint(0, k - 2, u[b, col + 5]))
                y2 += y2 >= y1
            else:
                y2 = int(_randint(0, k - 1, u[b, col + 5]))
            if mb["allow_shifted"]:
                sx = int(_randint(-min(x1, x2), k - 1 - max(x1, x2), u[b, col + 6]))
                sy = int(_randint(-min(y1, y2), k - 1 - max(y1, y2), u[b, col + 7]))
            else:
                (x1, x2), (y1, y2) = _make_odd(x1, x2), _make_odd(y1, y2)
                sx, sy = k // 2 - (x1 + x2) // 2, k // 2 - (y1 + y2) // 2
            taps = [(y - k // 2, x - k // 2) for y, x in line_taps(y1 + sy, x1 + sx, y2 + sy, x2 + sx)]
            rec[b, 7:16] = image_geom_record(taps=taps)[7:16]
            rec[b, 0] |= IMAGE_GEOM_BLUR
        col += 8
    bits = np.where(rec[:, 0] != 0, IMAGE_GEOM_BIT, 0).astype(np.uint8)
    return torch.from_numpy(bits), torch.from_numpy(rec)


MIX_MODES = ("batch", "pair", "elem")
_MIX_DEFAULTS = dict(mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch",
                     correct_lam=True)


def normalise_mix_spec(spec):
    """None, or a dict of timm.data.Mixup's argument names -> the same with defaults filled in; None when nothing can mix.
    label_smoothing and num_classes are not taken here: smoothing belongs to the loss (`loss["label_smoothing"]`)."""
    if spec is None:
        return None
    unknown = set(spec) - set(_MIX_DEFAULTS)
    if unknown:
        raise ValueError(f"mixup: unknown arguments {sorted(unknown)}; known: {sorted(_MIX_DEFAULTS)}")
    out = {**_MIX_DEFAULTS, **spec}
    if out["cutmix_minmax"] is not None:
        raise NotImplementedError("mixup: cutmix_minmax is not built (boxes come from lam, as timm's rand_bbox draws them)")
    if not out["correct_lam"]:
        raise NotImplementedError("mixup: correct_lam=False is not built (lam is always corrected to the clipped box)")
    if out["mode"] not in MIX_MODES:
        raise ValueError(f"mixup: mode {out['mode']!r}; known: {MIX_MODES}")
    if out["mixup_alpha"] < 0 or out["cutmix_alpha"] < 0 or not 0.0 <= out["prob"] <= 1.0 or not 0.0 <= out["switch_prob"] <= 1.0:
        raise ValueError(f"mixup: need alphas >= 0 and probabilities in [0, 1], got {out!r}")
    if out["mixup_alpha"] == 0 and out["cutmix_alpha"] == 0:
        return None
    return out


def draw_batch_mix(rng, B, size, spec):
    """The Mixup / CutMix draws of one batch (timm.data.Mixup's rules restated from memory: parity UNPINNED) ->
    (bits uint8 [B]: 8 where the image is mixed, words int32 [B, 6]: words 10..15 of its record, partner int64 [B],
    lam float64 [B]: the weight of the image's own label).

    rng: numpy Generator.  Image b's partner is B - 1 - b.  A unit is the batch ("batch"), a pair (b, B - 1 - b) ("pair") or an
    image ("elem"); n units draw, in this order and whatever they decide: rng.random((n, 2)) [apply, switch], rng.beta(mixup_alpha,
    mixup_alpha, n) if mixup_alpha > 0, rng.beta(cutmix_alpha, cutmix_alpha, n) if cutmix_alpha > 0, rng.integers(0, size, (n, 2))
    [cy, cx].  A unit mixes where apply < prob; with both alphas set it cuts where switch < switch_prob.  Blend: lam is the
    float32 of the draw (what the record holds).  Box (rand_bbox): cut = int(size * sqrt(1 - lam)), edges clip(c -+ cut // 2, 0, size),
    lam corrected to 1 - area / size^2.  An image that is its own partner, a unit that does not mix and a box without area leave
    the image unmixed: lam = 1, words zero, no bit."""
    from .hip import IMAGE_MIX_BIT, IMAGE_MIX_BLEND, IMAGE_MIX_BOX
    spec = normalise_mix_spec(spec)
    bits, words = np.zeros(B, np.uint8), np.zeros((B, 6), np.int32)
    partner, lam = B - 1 - np.arange(B, dtype=np.int64), np.ones(B, np.float64)
    if spec is None or B == 0:
        return torch.from_numpy(bits), torch.from_numpy(words), torch.from_numpy(partner), torch.from_numpy(lam)
    mode, ma, ca = spec["mode"], float(spec["mixup_alpha"]), float(spec["cutmix_alpha"])
    n = 1 if mode == "batch" else (B + 1) // 2 if mode == "pair" else B
    u = rng.random((n, 2))
    lam_mix = rng.beta(ma, ma, n) if ma > 0 else None
    lam_cut = rng.beta(ca, ca, n) if ca > 0 else None
    centre = rng.integers(0, size, (n, 2))
    idx = np.arange(B)
    unit = np.zeros(B, np.int64) if mode == "batch" else np.minimum(idx, B - 1 - idx) if mode == "pair" else idx
    apply = u[unit, 0] < spec["prob"]
    cut = (u[unit, 1] < spec["switch_prob"]) if (ma > 0 and ca > 0) else np.full(B, ca > 0)
    # box of every image, from its unit's cut draw
    raw = (lam_cut if lam_cut is not None else np.ones(n))[unit]
    ext = (size * np.sqrt(1.0 - raw)).astype(np.int64)
    cy, cx = centre[unit, 0], centre[unit, 1]
    y1, y2 = np.clip(cy - ext // 2, 0, size), np.clip(cy + ext // 2, 0, size)
    x1, x2 = np.clip(cx - ext // 2, 0, size), np.clip(cx + ext // 2, 0, size)
    area = (y2 - y1) * (x2 - x1)
    blend = (lam_mix if lam_mix is not None else np.ones(n))[unit].astype(np.float32)
    mixed = apply & (partner != idx) & np.where(cut, area > 0, True)
    box, mix = mixed & cut, mixed & ~cut
    lam = np.where(box, 1.0 - area / float(size * size), np.where(mix, blend.astype(np.float64), 1.0))
    bits[mixed] = IMAGE_MIX_BIT
    words[:, 0] = np.where(mixed, partner, 0)
    words[:, 1] = np.where(box, IMAGE_MIX_BOX, np.where(mix, IMAGE_MIX_BLEND, 0))
    f = words.view(np.float32)
    f[mix, 2] = blend[mix]
    f[mix, 3] = np.float32(1.0) - blend[mix]
    words[box, 2:6] = np.stack([y1, x1, y2, x2], 1)[box]
    return torch.from_numpy(bits), torch.from_numpy(words), torch.from_numpy(partner), torch.from_numpy(lam)


# transforms of the reference stack, in the only order the kernel applies them
_PIPELINE_ORDER = ("LongestMaxSize", "PadIfNeeded", "Resize", "RandomResizedCrop", "HorizontalFlip", "VerticalFlip", "MotionBlur",
                   "RandomBrightnessContrast", "HueSaturationValue", "CoarseDropout", "Normalize", "ToTensorV2")
_BORDER_MODES = {0: "constant", 4: "reflect_101"}          # cv2.BORDER_CONSTANT, cv2.BORDER_REFLECT_101


def translate_pipeline(pipeline):
    """An albumentations-style Compose (anything with a `.transforms` list) -> the `data` keys of the device pipeline.
    Duck-typed on type(t).__name__ and on the attributes p, max_size, value, brightness_limit, contrast_limit,
    hue_shift_limit, sat_shift_limit, val_shift_limit, min/max_holes, min/max_height, min/max_width, fill_value, mean, std,
    border_mode, height, width, size, scale, ratio, blur_limit, allow_shifted (restated from memory of albumentations 1.x:
    UNPINNED).  A transform outside the reference stack, or one out of the stack's order, raises NotImplementedError; so does a
    PadIfNeeded border other than constant (0) or reflect-101 (4) and a Resize to anything but the stack's own square size (the
    reference's archived stacks resize the padded square to its own size: a no-op).  A PadIfNeeded without a border_mode
    attribute keeps the constant border.  RandomResizedCrop to a size other than LongestMaxSize's makes that one the
    `source_size` of the host and its own the output `size`."""
    out, last = {}, -1
    for t in pipeline.transforms:
        name = type(t).__name__
        if name not in _PIPELINE_ORDER:
            raise NotImplementedError(f"device pipeline: transform {name} is not built (known: {', '.join(_PIPELINE_ORDER)})")
        rank = _PIPELINE_ORDER.index(name)
        if rank <= last:
            raise NotImplementedError(f"device pipeline: {name} after {_PIPELINE_ORDER[last]} — the kernel applies the stack "
                                      f"in the order {' -> '.join(_PIPELINE_ORDER)} only")
        last = rank
        p = float(getattr(t, "p", 1.0))
        if name == "LongestMaxSize":
            if getattr(t, "max_size", None) is not None:
                out["size"] = int(t.max_size)
        elif name == "PadIfNeeded":
            if getattr(t, "value", None) is not None:
                out["fill"] = float(t.value)
            mode = getattr(t, "border_mode", None)
            if mode is not None:
                if mode not in _BORDER_MODES:
                    raise NotImplementedError(f"device pipeline: PadIfNeeded border_mode {mode!r} is not built (0 = constant and "
                                              f"4 = reflect-101 are)")
                out["pad_border"] = _BORDER_MODES[mode]
        elif name == "Resize":
            if "size" not in out or not (int(t.height) == int(t.width) == out["size"]):
                raise NotImplementedError(f"device pipeline: Resize to {t.height} x {t.width} is not built: only the no-op onto the "
                                          f"stack's own {out.get('size', '(unset)')}-pixel square is accepted")
        elif name == "RandomResizedCrop":
            side = getattr(t, "size", None)
            hh, ww = (side if isinstance(side, (tuple, list)) else (side, side)) if side is not None else (t.height, t.width)
            if int(hh) != int(ww):
                raise NotImplementedError(f"device pipeline: RandomResizedCrop to {hh} x {ww} is not built (square outputs only)")
            if "size" in out and out["size"] != int(hh):
                out["source_size"] = out["size"]
            out["size"] = int(hh)
            out["random_resized_crop"] = dict(scale=tuple(t.scale), ratio=tuple(t.ratio), p=p)
        elif name == "MotionBlur":
            out["motion_blur"] = dict(blur_limit=t.blur_limit, allow_shifted=getattr(t, "allow_shifted", True), p=p)
        elif name == "HorizontalFlip":
            out["hflip_p"] = p
        elif name == "VerticalFlip":
            out["vflip_p"] = p
        elif name == "RandomBrightnessContrast":
            out["brightness_contrast"] = dict(brightness_limit=t.brightness_limit, contrast_limit=t.contrast_limit, p=p,
                                              brightness_by_max=getattr(t, "brightness_by_max", True))
        elif name == "HueSaturationValue":
            out["hue_saturation_value"] = dict(hue_shift_limit=t.hue_shift_limit, sat_shift_limit=t.sat_shift_limit,
                                               val_shift_limit=t.val_shift_limit, p=p)
        elif name == "CoarseDropout":
            out["coarse_dropout"] = dict(p=p, **{k: getattr(t, k) for k in ("max_holes", "min_holes", "max_height", "min_height",
                                                                          "max_width", "min_width", "fill_value") if hasattr(t, k)})
        elif name == "Normalize":
            out["mean"], out["std"] = tuple(t.mean), tuple(t.std)
    return out


class DeviceLoader:
    """Wraps a host loader that yields (uint8 [B,H,W,3], sizes int32 [B,2] or None, target) and yields
    (float32 [B,3,size,size] on `device`, target) — the batch format engine.train_epoch consumes (engine.py:39-41).

    Batch k+1 is pinned and copied on a dedicated copy stream while batch k trains; the prep kernel runs on the compute
    stream after an event wait, so no host synchronisation is added.  Flip draws come from a host generator (one
    Bernoulli per image and axis, A.HorizontalFlip / A.VerticalFlip(p)).

    brightness_contrast / hue_saturation_value / coarse_dropout: None or a dict of albumentations' argument names plus `p`
    (normalise_aug_spec).  Their draws (draw_image_aug) come from a SECOND generator seeded `seed + 1`, never from the flip
    generator; the records ride behind the flag bytes (hip.pack_image_aug) on the copy stream.  With all three None nothing
    changes: same draws, same buffers.

    mixup: None or a dict of timm.data.Mixup's argument names (normalise_mix_spec).  Its draws (draw_batch_mix) come from a
    THIRD generator, numpy's default_rng(seed + 2); the mixing instructions ride in words 10..15 of the records, the image is
    mixed inside the prep launch, and the target of a batch with a mixed image becomes a losses.MixedTarget (a dict of them
    for dict targets: one lam and one partner shared by all tasks) uploaded with the batch.  A batch without a mixed image keeps
    its plain labels.  With mixup None nothing changes: same draws, same buffers.

    random_resized_crop / motion_blur: None or a dict of albumentations' argument names plus `p`; pad_border: None, "constant" or
    "reflect_101" (normalise_geom_spec).  Their draws (draw_image_geom) come from a FOURTH generator seeded `seed + 3`; the
    geometry records ride in a second table behind the first (hip.pack_image_geom) and are applied in the same launch, in front
    of the flips: crop -> flips -> blur -> colour -> mix.  A batch whose source canvas is larger than `size` needs
    random_resized_crop with p == 1.  With all three None nothing changes: same draws, same buffers, same launch arguments."""

    def __init__(self, loader, device, size, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), hflip_p=0.0,
                 vflip_p=0.0, fill=0.0, seed=0, brightness_contrast=None, hue_saturation_value=None, coarse_dropout=None,
                 mixup=None, random_resized_crop=None, motion_blur=None, pad_border=None):
        self.loader, self.device = loader, torch.device(device)
        self.size, self.mean, self.std, self.fill = size, tuple(mean), tuple(std), float(fill)
        self.hflip_p, self.vflip_p = float(hflip_p), float(vflip_p)
        self.gen = torch.Generator().manual_seed(seed)
        self.aug = normalise_aug_spec(dict(brightness_contrast=brightness_contrast, hue_saturation_value=hue_saturation_value,
                                           coarse_dropout=coarse_dropout))
        self.aug_gen = torch.Generator().manual_seed(seed + 1)
        self.mixup = normalise_mix_spec(mixup)
        self.mix_rng = np.random.default_rng(seed + 2)
        self.geom = normalise_geom_spec(dict(random_resized_crop=random_resized_crop, motion_blur=motion_blur, pad_border=pad_border))
        self.geom_gen = torch.Generator().manual_seed(seed + 3)
        self.dataset = getattr(loader, "dataset", None)
        self._copy = None

    def __len__(self):
        return len(self.loader)

    def draw_flags(self, B, sizes=None):
        """The host draws of one batch -> what nkb_image_prep takes as `flags`: None, uint8 [B] flip bits (one torch.rand(B, 2)
        from the flip generator), or, with augmentations or mixup on, those bits | the record bits with the record table behind
        them; with a geometry transform on, the geometry bits and table as well (sizes: the batch's [B, 2] h and w, None =
        every image fills the size x size canvas)."""
        return self._draw(B, sizes)[0]

    def _draw(self, B, sizes=None):
        """(flags as draw_flags returns them, None or the (partner int64 [B], lam float64 [B]) of a batch with a mixed image)"""
        flags = None
        if self.hflip_p > 0 or self.vflip_p > 0:
            u = torch.rand(B, 2, generator=self.gen)
            flags = ((u[:, 0] < self.hflip_p).to(torch.uint8) | ((u[:, 1] < self.vflip_p).to(torch.uint8) << 1))
        bits = records = mix = None
        if self.aug is not None:
            bits, records = draw_image_aug(self.aug_gen, B, self.size, self.aug)
        if self.mixup is not None:
            from .hip import IMAGE_AUG_WORDS
            mbits, words, partner, lam = draw_batch_mix(self.mix_rng, B, self.size, self.mixup)
            if records is None:
                bits, records = torch.zeros(B, dtype=torch.uint8), torch.zeros(B, IMAGE_AUG_WORDS, dtype=torch.int32)
            records[:, 10:16] = words
            bits = bits | mbits
            if bool(mbits.any()):
                mix = (partner, lam)
        if self.geom is not None:
            from . import hip
            gbits, grec = draw_image_geom(self.geom_gen, B, sizes, self.size, self.geom)
            for other in (flags, bits):
                if other is not None:
                    gbits = gbits | other
            flags = hip.pack_image_geom(gbits, records, grec, sizes=sizes)
        elif records is not None:
            from . import hip
            flags = hip.pack_image_aug(bits if flags is None else flags | bits, records)
        return flags, mix

    @staticmethod
    def _mixed_target(labels, mix):
        """labels [B] and the batch's (partner, lam) -> the host table of a MixedTarget"""
        from .losses import MixedTarget
        partner, lam = mix
        y = torch.as_tensor(labels).to(torch.int64).reshape(-1)
        return MixedTarget.build(y, y[partner], lam)

    def _stage(self, item):
        """Pinned host batch -> device uint8 on the copy stream; returns what the compute stream needs."""
        if len(item) == 3:
            raw, sizes, target = item
        else:
            (raw, target), sizes = item, None
        if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[-1] != 3:
            raise RuntimeError(f"DeviceLoader expects uint8 [B,H,W,3] batches, got {tuple(raw.shape)} {raw.dtype}")
        B, Hs, Ws = raw.shape[:3]
        if max(Hs, Ws) > self.size and not (self.geom is not None and self.geom.get("random_resized_crop", {}).get("p") == 1.0):
            raise ValueError(f"DeviceLoader: a {Hs} x {Ws} source canvas is larger than the {self.size}-pixel output; that needs "
                             f"random_resized_crop with p = 1, so that every image is resampled")
        own = sizes
        if self.geom is not None and own is None:
            own = torch.tensor([[Hs, Ws]], dtype=torch.int32).expand(B, 2)
        flags, mix = self._draw(B, own)
        if mix is not None:
            if isinstance(target, dict):
                target = {k: self._mixed_target(v, mix).pin_memory() for k, v in target.items()}
            else:
                target = self._mixed_target(target, mix).pin_memory()
        if self._copy is None:
            self._copy = torch.cuda.Stream(device=self.device)
        pin = lambda t: t if t is None or t.is_pinned() else t.contiguous().pin_memory()       # noqa: E731
        raw, sizes, flags = pin(raw), pin(sizes), pin(flags)
        with torch.cuda.stream(self._copy):
            d_raw = raw.to(self.device, non_blocking=True)
            d_sizes = sizes.to(self.device, non_blocking=True) if sizes is not None else None
            d_flags = flags.to(self.device, non_blocking=True) if flags is not None else None
            if isinstance(target, dict):
                d_target = {k: (v if mix is not None else torch.as_tensor(v)).to(self.device, non_blocking=True)
                            for k, v in target.items()}
            else:
                d_target = (target if mix is not None else torch.as_tensor(target)).to(self.device, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self._copy)
        return dict(raw=d_raw, sizes=d_sizes, flags=d_flags, target=d_target, ready=ready, host=(raw, sizes, flags, target))

    def _finish(self, st):
        from . import hip
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(st["ready"])
        raw = st["raw"]
        B, Hs, Ws, _ = raw.shape
        out = torch.empty(B, 3, self.size, self.size, device=self.device, dtype=torch.float32)
        hip.image_prep(raw, st["sizes"], st["flags"], out, B, Hs, Ws, self.size, self.size, self.mean, self.std, self.fill)
        tgt = st["target"]
        for t in (raw, st["sizes"], st["flags"], *(tgt.values() if isinstance(tgt, dict) else (tgt,))):
            if t is not None:
                # allocated on the copy stream, consumed on the compute stream: without this the caching allocator hands the
                # block to the NEXT staged batch as soon as Python drops the tensor — while the loss kernel that reads it is still
                # queued (labels overwritten by another batch's flip flags: out-of-range classes, a NaN loss; bench.py --input
                # host-uint8 ran into it, a loop that synchronises every step does not)
                t.record_stream(cur)
        return out, tgt

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            try:
                nxt = self._stage(next(it))      # copy of batch k+1 overlaps the step on batch k
            except StopIteration:
                nxt = None
            yield self._finish(cur)


def get_dataset(data, pipeline=None):
    """dataset.py:541-629.  Extra keys: `device_pipeline=True` (+ `device`, `hflip_p`, `vflip_p`, `mean`, `std`) wraps the
    folder loader in a DeviceLoader; `rank` / `world` (+ `shard_seed`, the seed of the permutation all ranks share) shard the data for one-process-per-GPU
    training.  `mixup` (None or a dict of timm.data.Mixup's argument names: mixup_alpha, cutmix_alpha, prob, switch_prob, mode) mixes
    the batch inside the device pipeline and needs `device_pipeline`.  With `device_pipeline` the keys `brightness_contrast`, `hue_saturation_value`, `coarse_dropout` (None or a dict of
    albumentations' argument names plus `p`) and `fill` go to the DeviceLoader too, and a `pipeline` that has a `.transforms`
    list is translated into all of these keys (translate_pipeline); explicit `data` keys win over the translated ones.
    `random_resized_crop`, `motion_blur` (None or a dict of albumentations' argument names plus `p`) and `pad_border` ("constant" or
    "reflect_101") are the device pipeline's geometry; `source_size` (default `size`) is the host's LongestMaxSize target and canvas
    side, and a larger one than `size` needs random_resized_crop with p == 1."""
    kind = data.get("type", "folder")
    on_device = bool(data.get("device_pipeline", False))
    if on_device and isinstance(getattr(pipeline, "transforms", None), (list, tuple)):
        data = {**translate_pipeline(pipeline), **data}
    size = data.get("size", 224)
    if data.get("mixup") is not None and not (on_device and kind != "synthetic"):
        raise NotImplementedError("mixup is built into the device pipeline only: set device_pipeline=True on a folder dataset")
    geom = normalise_geom_spec({k: data.get(k) for k in GEOM_KEYS + ("pad_border",)})
    if geom is not None and not (on_device and kind != "synthetic"):
        raise NotImplementedError("random_resized_crop, motion_blur and pad_border are built into the device pipeline only: set "
                                  "device_pipeline=True on a folder dataset")
    source_size = int(data.get("source_size", size))
    if source_size != size and not on_device:
        raise ValueError("source_size belongs to the device pipeline (device_pipeline=True)")
    if source_size < size:
        raise ValueError(f"source_size = {source_size} is smaller than size = {size}: the host would upscale what the device crops")
    if source_size > size and not (geom is not None and geom.get("random_resized_crop", {}).get("p") == 1.0):
        raise ValueError(f"source_size = {source_size} > size = {size} needs random_resized_crop with p = 1, so that every image is "
                         f"resampled onto the output; anything else has no {size}-pixel image to show")
    if kind == "synthetic":
        ds = SyntheticDataset(data["n_images"], data["classes"], size=size, seed=data.get("seed", 1234))
        on_device = False
    elif "root" in data:
        ds = FolderDataset(data["root"], size=size, classes=data.get("classes"), raw=on_device,
                           source_size=source_size if on_device else None)
    else:
        raise NotImplementedError(
            f"dataset type {kind!r}: the reference's annotation / augmentation datasets (dataset.py:183-538) are "
            "input-pipeline code outside the accelerated path and are not part of this package")
    rank, world = int(data.get("rank", 0)), int(data.get("world", 1))
    sampler, shuffle = None, data.get("shuffle", False)
    if data.get("weighted_sampling", False):              # dataset.py:607-617
        sampler, shuffle = ImbalancedDatasetSampler(ds, seed=data.get("shard_seed", 0) if world > 1 else None, rank=rank,
                                                    world=world), False
    elif world > 1:
        sampler, shuffle = ShardedSampler(len(ds), rank, world, shuffle=shuffle, seed=data.get("shard_seed", 0),
                                          pad=bool(data.get("shard_pad", True))), False
    loader = DataLoader(ds, batch_size=data["batch_size"], shuffle=shuffle, sampler=sampler,
                        num_workers=data.get("num_workers", 0), drop_last=data.get("drop_last", False), pin_memory=True)
    if on_device:
        return DeviceLoader(loader, data.get("device", "cuda:0"), size, mean=data.get("mean", (0.485, 0.456, 0.406)),
                            std=data.get("std", (0.229, 0.224, 0.225)), hflip_p=data.get("hflip_p", 0.0),
                            vflip_p=data.get("vflip_p", 0.0), fill=data.get("fill", 0.0), seed=data.get("seed", 0),
                            **{k: data.get(k) for k in AUG_KEYS}, mixup=data.get("mixup"),
                            **{k: data.get(k) for k in GEOM_KEYS + ("pad_border",)})
    return loader
