"""numpy restatement of the augmenting path of nkb_image_prep (csrc/imgprep.hip; the contract is the header comment of
include/nkbhip.h), written twice:

  * order="f32": every floating-point step in float32 in the documented order, one rounding per operation.  The kernel is
    built with -ffp-contract=off and uses only IEEE add / multiply / fmod / rint, so it is expected to give these levels;
  * order="f64": the same steps in float64 (the record's float32 parameters are data and enter as they are; the constants
    6/180 and 1/255 are the float64 ones).  It also returns the TIE BAND: which output values depend on a float64
    pre-rounding value that lies within BAND of a rounding boundary (an integer for the truncations, a half-integer for the
    final round-half-even) — the only places where float32 rounding can move a level.  A truncated value whose whole
    float64 chain is exactly representable in float32 is computed without any rounding in either order and is not in the band,
    however close (integer shifts put every value ON a boundary).

Stages, uint8 levels in and out (the albumentations stack of the reference's configs: RandomBrightnessContrast ->
HueSaturationValue -> CoarseDropout, on the padded and flipped canvas).  The 8-bit HSV conversions restate OpenCV's
(cv2 is not a dependency: parity with it is unpinned).
"""
import numpy as np

BAND = 1e-3
MAX_HOLES = 12
RECORD_WORDS = 64
APPLY_BC, APPLY_HSV, APPLY_HOLES = 1, 2, 4

_n = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint(255.0 * 4096.0 / _n)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint(180.0 * 4096.0 / (6.0 * _n))]).astype(np.int64)
# (b, g, r) = tab[SECTOR[sector]], tab = [v, v(1-s), v(1-s f), v(1-s(1-f))]
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def make_record(alpha=None, offset=None, hsv=None, holes=None, hole_fill=(0, 0, 0)):
    """int32[64] record; a transform left None is not applied"""
    rec = np.zeros(RECORD_WORDS, np.int32)
    f = rec.view(np.float32)
    f[1] = 1.0
    if alpha is not None or offset is not None:
        rec[0] |= APPLY_BC
        f[1], f[2] = 1.0 if alpha is None else alpha, 0.0 if offset is None else offset
    if hsv is not None:
        rec[0] |= APPLY_HSV
        f[3:6] = hsv
    if holes is not None:
        assert len(holes) <= MAX_HOLES
        rec[0] |= APPLY_HOLES
        rec[6] = len(holes)
        rec[7:10] = hole_fill
        for k, box in enumerate(holes):
            rec[16 + 4 * k:20 + 4 * k] = box
    return rec


def rgb_to_hsv(rgb):
    """OpenCV's 8-bit RGB -> HSV (H in 0..179), integer arithmetic"""
    rgb = np.asarray(rgb).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = (d * SDIV[v] + 2048) >> 12
    hraw = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (hraw * HDIV[d] + 2048) >> 12            # numpy's >> on signed integers is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def _near(x, boundary_offset):
    """distance of x to the nearest boundary (integers + boundary_offset) below BAND"""
    t = x - boundary_offset
    return np.abs(t - np.rint(t)) < BAND


def _is_f32(x):
    return x.astype(np.float32).astype(np.float64) == x


def brightness_contrast(P, alpha, offset, order="f32"):
    """albumentations' uint8 LUT path (brightness_by_max=True): lut = clip(arange(256) * alpha + beta * 255); offset = beta * 255"""
    ft = np.float32 if order == "f32" else np.float64
    t = np.asarray(P).astype(ft)
    exact = np.ones(t.shape, bool)
    if np.float32(alpha) != np.float32(1.0):
        t = t * ft(np.float32(alpha))
        exact &= _is_f32(t.astype(np.float64))
    if np.float32(offset) != np.float32(0.0):
        t = t + ft(np.float32(offset))
        exact &= _is_f32(t.astype(np.float64))
    lv = np.trunc(np.clip(t, ft(0), ft(255))).astype(np.int64)
    if order == "f32":
        return lv
    return lv, _near(t.astype(np.float64), 0.0) & ~exact & (t > -1) & (t < 256)


def hsv_shift(h, s, v, hue, sat, val, order="f32"):
    ft = np.float32 if order == "f32" else np.float64
    hue, sat, val = (ft(np.float32(a)) for a in (hue, sat, val))
    hs = h.astype(ft) + hue
    m = np.fmod(hs, ft(180))
    m = np.where(m < 0, m + ft(180), m)
    h2 = np.trunc(m).astype(np.int64)
    h2 = np.where(h2 >= 180, h2 - 180, h2)
    ss = s.astype(ft) + sat
    s2 = np.trunc(np.clip(ss, ft(0), ft(255))).astype(np.int64)
    vs = v.astype(ft) + val
    v2 = np.trunc(np.clip(vs, ft(0), ft(255))).astype(np.int64)
    if order == "f32":
        return h2, s2, v2
    band = np.zeros(h.shape, bool)
    for x, inside in ((m, np.ones(h.shape, bool)), (ss, (ss > -1) & (ss < 256)), (vs, (vs > -1) & (vs < 256))):
        band |= _near(x, 0.0) & ~_is_f32(x) & inside
    return h2, s2, v2, band


def hsv_to_rgb(h, s, v, order="f32"):
    """OpenCV's HSV -> RGB for 8-bit images: float arithmetic on h * 6/180, s / 255, v / 255, rounded to levels"""
    ft = np.float32 if order == "f32" else np.float64
    one = ft(1)
    hf = h.astype(ft) * (ft(6) / ft(180))
    sf = s.astype(ft) * (one / ft(255))
    vf = v.astype(ft) * (one / ft(255))
    sector = np.floor(hf)
    f = hf - sector
    sector = np.clip(sector.astype(np.int64), 0, 5)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], -1)
    idx = SECTOR[sector]                                        # [..., 3] in b, g, r order
    bgr = np.take_along_axis(tab, idx, -1)
    bgr = np.where((s == 0)[..., None], vf[..., None], bgr)
    pre = bgr[..., ::-1] * ft(255)                              # r, g, b
    lv = np.clip(np.rint(pre), 0, 255).astype(np.int64)
    if order == "f32":
        return lv
    return lv, _near(pre, 0.5)


def augment(levels, rec, order="f32"):
    """levels: int [H, W, 3] (the padded, flipped canvas); rec: int32[64].  Returns levels, and for order="f64" also the tie band
    [H, W, 3] (a brightness/contrast or HSV-shift tie of a pixel puts its three values in the band when the HSV stage mixes them)."""
    rec = np.asarray(rec, np.int32)
    f = rec.view(np.float32)
    lv = np.asarray(levels).astype(np.int64)
    band = np.zeros(lv.shape, bool)
    mask = int(rec[0])
    if mask & APPLY_BC:
        if order == "f32":
            lv = brightness_contrast(lv, f[1], f[2])
        else:
            lv, band = brightness_contrast(lv, f[1], f[2], order)
    if mask & APPLY_HSV and (f[3] != 0 or f[4] != 0 or f[5] != 0):
        h, s, v = rgb_to_hsv(lv)
        if order == "f32":
            lv = hsv_to_rgb(*hsv_shift(h, s, v, f[3], f[4], f[5]))
        else:
            h, s, v, b1 = hsv_shift(h, s, v, f[3], f[4], f[5], order)
            lv, b2 = hsv_to_rgb(h, s, v, order)
            band = b2 | b1[..., None] | band.any(-1, keepdims=True)
    if mask & APPLY_HOLES:
        H, W, _ = lv.shape
        yy, xx = np.mgrid[0:H, 0:W]
        inside = np.zeros((H, W), bool)
        for k in range(min(max(int(rec[6]), 0), MAX_HOLES)):
            y1, x1, y2, x2 = (int(a) for a in rec[16 + 4 * k:20 + 4 * k])
            inside |= (yy >= y1) & (yy < y2) & (xx >= x1) & (xx < x2)
        lv = np.where(inside[..., None], rec[7:10].astype(np.int64), lv)
        band = band & ~inside[..., None]
    return lv if order == "f32" else (lv, band)


def canvas(img, Ho, Wo, flag, fill):
    """PadIfNeeded(centre, constant) -> HorizontalFlip (bit 0) / VerticalFlip (bit 1), in levels; the pad level of the
    augmenting path is clamp((int)fill, 0, 255)"""
    h, w, _ = img.shape
    top, left = (Ho - h) // 2, (Wo - w) // 2
    out = np.full((Ho, Wo, 3), min(max(int(fill), 0), 255), np.int64)
    out[top:top + h, left:left + w] = img
    if flag & 1:
        out = out[:, ::-1]
    if flag & 2:
        out = out[::-1]
    return out


def normalise(levels, mean, std):
    """Normalize(max_pixel_value=255) -> ToTensorV2 in float32, the kernel's order: (level - 255 mean) * (1 / (255 std))"""
    m = np.asarray(mean, np.float32) * np.float32(255.0)
    r = np.float32(1.0) / (np.asarray(std, np.float32) * np.float32(255.0))
    return np.ascontiguousarray(((np.asarray(levels).astype(np.float32) - m) * r).transpose(2, 0, 1))


def plain(img, Ho, Wo, flag, mean, std, fill):
    """the path without a record: float32 pad value `fill` itself, no level stages"""
    h, w, _ = img.shape
    top, left = (Ho - h) // 2, (Wo - w) // 2
    out = np.full((Ho, Wo, 3), fill, np.float32)
    out[top:top + h, left:left + w] = img
    if flag & 1:
        out = out[:, ::-1]
    if flag & 2:
        out = out[::-1]
    return normalise(out, mean, std)


def levels_of(img, Ho, Wo, flag, rec, fill, order="f32"):
    """levels [Ho, Wo, 3] of one image (flag: the whole flag byte; bit 2 clear -> rec is ignored); order="f64" adds the band"""
    lv = canvas(img, Ho, Wo, flag, fill)
    if flag & 4:
        return augment(lv, rec, order)
    return lv if order == "f32" else (lv, np.zeros(lv.shape, bool))


def lattice():
    """the 16^3 lattice {0, 17, ..., 255}^3 as a 64 x 64 RGB image"""
    a = np.arange(0, 256, 17)
    r, g, b = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([r, g, b], -1).reshape(64, 64, 3).astype(np.uint8)


SHIFT_TRIPLES = ((0, 10, 50), (0, -10, -50), (37.3, -20.5, 12.25), (-91.7, 33.3, -7.5), (179.9, 255, 0), (0.4, 0.6, -0.2))
