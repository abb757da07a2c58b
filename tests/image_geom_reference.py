"""numpy restatement of the geometry record of nkb_image_prep (flag bit 4; csrc/imgprep.hip, the contract is the header comment of
include/nkbhip.h): stage canvas (integer bilinear resample of a crop box, or the centred pad stage with a constant or reflect-101
border) -> flips -> blur over up to 16 taps.  Every step is integer arithmetic or a single float32 operation, so the kernel is held
to these levels bit for bit.  The colour stages, Normalize and the mixing rule are tests/image_aug_reference.py's and
tests/mix_reference.py's, composed here by import.  No test lives here, and nothing of the package is imported."""
import numpy as np

import image_aug_reference as R
import mix_reference as M

GEOM_BIT, GEOM_WORDS, MAX_TAPS = 16, 16, 16
RESAMPLE, BLUR, REFLECT = 1, 2, 4
F32 = np.float32


def make_geom(box=None, out=None, taps=None, reflect=False):
    """int32[16] geometry record.  box: (y0, x0, bh, bw) resampled onto out = (Ho, Wo); taps: [(dy, dx), ..]; reflect: the pad
    stage's border is reflect-101"""
    g = np.zeros(GEOM_WORDS, np.int32)
    if box is not None:
        g[0] |= RESAMPLE
        g[1:5] = box
        f = g.view(F32)
        f[5] = F32(box[2]) / F32(out[0])
        f[6] = F32(box[3]) / F32(out[1])
    if taps is not None:
        assert 1 <= len(taps) <= MAX_TAPS
        g[0] |= BLUR
        g[7] = len(taps)
        words = np.zeros(8, np.uint32)
        for t, (dy, dx) in enumerate(taps):
            assert -127 <= dy <= 127 and -127 <= dx <= 127
            words[t // 2] |= np.uint32(((dy & 0xFF) | ((dx & 0xFF) << 8)) << (16 * (t % 2)))
        g[8:16] = words.view(np.int32)
    if reflect:
        g[0] |= REFLECT
    return g


def taps_of(g):
    """[(dy, dx)] of a record, the count clamped to 1..16"""
    g = np.asarray(g, np.int32)
    n = min(max(int(g[7]), 1), MAX_TAPS)
    out = []
    for t in range(n):
        half = (int(g[8 + t // 2]) >> (16 * (t % 2))) & 0xFFFF
        dy, dx = half & 0xFF, half >> 8
        out.append((dy - 256 if dy > 127 else dy, dx - 256 if dx > 127 else dx))
    return out


def reflect101(i, n):
    """i < 0 -> -i, i >= n -> 2 (n - 1) - i, repeated until in range; n == 1 -> 0"""
    i = np.array(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    while True:
        low, high = i < 0, i >= n
        if not (low.any() or high.any()):
            return i
        i = np.where(low, -i, np.where(high, 2 * (n - 1) - i, i))


def axis_coords(N, s, n):
    """canvas coordinates 0..N-1 of one axis -> (i, i', c1): f = (X + 0.5) * s - 0.5 in three float32 operations, clamped at both
    ends of the box extent n, c1 = rint(t * 2048)"""
    X = np.arange(N).astype(F32)
    f = (X + F32(0.5)) * F32(s) - F32(0.5)
    assert f.dtype == F32
    fl = np.floor(f)
    i, t = fl.astype(np.int64), f - fl
    low, high = i < 0, i >= n - 1
    i = np.where(low, 0, np.where(high, n - 1, i))
    t = np.where(low | high, F32(0), t).astype(F32)
    c1 = np.rint(t * F32(2048.0)).astype(np.int64)
    return i, np.minimum(i + 1, n - 1), c1


def resample(slot, g, Ho, Wo):
    """the box of record g stretched over Ho x Wo: 11-bit coefficients, one rounding at the end"""
    g = np.asarray(g, np.int32)
    y0, x0, bh, bw = (int(v) for v in g[1:5])
    sy, sx = g.view(F32)[5], g.view(F32)[6]
    iy, iy1, cy1 = axis_coords(Ho, sy, bh)
    ix, ix1, cx1 = axis_coords(Wo, sx, bw)
    cy0, cx0 = 2048 - cy1, 2048 - cx1
    P = np.asarray(slot).astype(np.int64)
    acc = np.zeros((Ho, Wo, 3), np.int64)
    for ys, cy in ((iy, cy0), (iy1, cy1)):
        for xs, cx in ((ix, cx0), (ix1, cx1)):
            acc += (cy[:, None] * cx[None, :])[..., None] * P[y0 + ys][:, x0 + xs]
    assert acc.max() + (1 << 21) < 1 << 31
    return (acc + (1 << 21)) >> 22


def cdiv2(a):
    """a / 2 as C divides: towards zero"""
    return a // 2 if a >= 0 else -((-a) // 2)


def pad_stage(img, Ho, Wo, pad, reflect, dtype=np.int64):
    """the h x w image centred in Ho x Wo (a window of it where it is larger); outside it `pad`, or the reflect-101 pixel"""
    h, w, _ = img.shape
    ys, xs = np.arange(Ho) - cdiv2(Ho - h), np.arange(Wo) - cdiv2(Wo - w)
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    if reflect:
        return np.asarray(img).astype(dtype)[reflect101(ys, h)][:, reflect101(xs, w)]
    got = np.asarray(img).astype(dtype)[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    return np.where(inside[..., None], got, dtype(pad))


def flip(C, flag):
    if flag & 1:
        C = C[:, ::-1]
    if flag & 2:
        C = C[::-1]
    return C


def blur(F, taps):
    """(2 sum_t F(r(y + dy), r(x + dx)) + n) / (2 n), r = reflect-101 at the canvas edge"""
    Ho, Wo, _ = F.shape
    acc, n = np.zeros(F.shape, np.int64), len(taps)
    for dy, dx in taps:
        acc += F[reflect101(np.arange(Ho) + dy, Ho)][:, reflect101(np.arange(Wo) + dx, Wo)]
    return (2 * acc + n) // (2 * n)


def pad_level(fill):
    return min(max(int(fill), 0), 255)


def canvas_levels(slot, h, w, flag, g, Ho, Wo, fill):
    """levels [Ho, Wo, 3] in front of the colour stages.  slot: the image's Hs x Ws source slot, the image its top-left h x w;
    flag: the flag byte; g: its geometry record (ignored without bit 4)"""
    g = np.asarray(g, np.int32) if flag & GEOM_BIT else np.zeros(GEOM_WORDS, np.int32)
    mask = int(g[0])
    if mask & RESAMPLE:
        C = resample(slot, g, Ho, Wo)
    else:
        C = pad_stage(slot[:h, :w], Ho, Wo, pad_level(fill), bool(mask & REFLECT))
    F = flip(C, flag)
    return blur(F, taps_of(g)) if mask & BLUR else F


def plain_of(slot, h, w, flag, arec, g, Ho, Wo, mean, std, fill):
    """plain(k) of the header: float32 [3, Ho, Wo] from k's sizes, flips (bits 0, 1), augmentation record (bit 2) and geometry
    record (bit 4).  Without either record the pad value is the float `fill` itself."""
    if not flag & (4 | GEOM_BIT):
        return R.normalise(flip(pad_stage(slot[:h, :w], Ho, Wo, fill, False, F32), flag), mean, std)
    lv = canvas_levels(slot, h, w, flag, g, Ho, Wo, fill)
    if flag & 4:
        lv = R.augment(lv, arec)
    return R.normalise(lv, mean, std)


def batch(src, sizes, flags, arecs, grecs, Ho, Wo, mean, std, fill):
    """out [B, 3, Ho, Wo] float32 of one launch: plain_of per image, then the mixing rule of mix_reference"""
    B = len(flags)
    zero_a, zero_g = np.zeros(R.RECORD_WORDS, np.int32), np.zeros(GEOM_WORDS, np.int32)

    def one(k, fl):
        h, w = (int(v) for v in sizes[k]) if sizes is not None else src.shape[1:3]
        fl = fl | (int(flags[k]) & GEOM_BIT)                  # mix_images hands bits 0..2 on; bit 4 belongs to plain(k) too
        return plain_of(src[k], h, w, fl, arecs[k] if arecs is not None else zero_a, grecs[k] if grecs is not None else zero_g,
                        Ho, Wo, mean, std, fill)

    records = arecs if arecs is not None else [zero_a] * B
    return M.mix_images(one, [int(f) for f in flags], records, Ho, Wo)
