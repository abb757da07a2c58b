"""Device-side geometry (RandomResizedCrop, MotionBlur, reflect-101 pad), the parts that need no GPU: self-checks of the numpy
restatement of the kernel's geometry record (tests/image_geom_reference.py), the host draws of dataset.draw_image_geom, the packed
two-table layout and the pipeline translation."""
import numpy as np
import pytest
import torch

import image_geom_reference as G
from nkb_classification import dataset as D
from nkb_classification import hip

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = np.array([[24, 20], [7, 24], [24, 1], [13, 13], [1, 1], [24, 24]])


# ---- the reference against itself ------------------------------------------------------------------------------------------------
def test_a_same_size_box_is_the_identity():
    rng = np.random.default_rng(0)
    slot = rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)
    iy, iy1, c1 = G.axis_coords(16, np.float32(16) / np.float32(16), 16)
    assert np.array_equal(iy, np.arange(16)) and not c1.any()
    got = G.resample(slot, G.make_geom(box=(5, 3, 16, 16), out=(16, 16)), 16, 16)
    assert np.array_equal(got, slot[5:21, 3:19])
    # on one axis only: the rows are copied, the columns are blended
    got = G.resample(slot, G.make_geom(box=(8, 0, 16, 20), out=(16, 16)), 16, 16)
    ix, ix1, cx1 = G.axis_coords(16, np.float32(20) / np.float32(16), 20)
    rows = slot[8:24].astype(np.int64)
    want = ((2048 - cx1)[None, :, None] * rows[:, ix] + cx1[None, :, None] * rows[:, ix1]) * 2048
    assert np.array_equal(got, (want + (1 << 21)) >> 22) and cx1.any()
    # through the whole canvas path, flips included
    for flag in range(4):
        lv = G.canvas_levels(slot, 24, 20, 16 | flag, G.make_geom(box=(5, 3, 16, 16), out=(16, 16)), 16, 16, 0.0)
        assert np.array_equal(lv, G.flip(slot[5:21, 3:19].astype(np.int64), flag))


def test_a_single_centre_tap_is_the_identity():
    rng = np.random.default_rng(1)
    F = rng.integers(0, 256, (9, 7, 3)).astype(np.int64)
    assert np.array_equal(G.blur(F, [(0, 0)]), F)
    g = G.make_geom(taps=[(0, 0)])
    assert G.taps_of(g) == [(0, 0)] and g[0] == G.BLUR and g[7] == 1
    # a flat canvas stays flat under any taps; two taps round half up
    assert np.array_equal(G.blur(np.full((5, 5, 3), 77), [(-3, 2), (1, 1), (4, -4)]), np.full((5, 5, 3), 77))
    two = np.zeros((1, 2, 3), np.int64)
    two[0, 1] = 5
    assert G.blur(two, [(0, 0), (0, 1)])[0, 0, 0] == 3          # (0 + 5) / 2 = 2.5 -> 3


def test_reflect_101_equals_numpy_pad():
    assert G.reflect101(np.arange(-6, 10), 3).tolist() == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert not G.reflect101(np.arange(-5, 6), 1).any()
    for n, before, after in ((3, 6, 7), (16, 2, 3), (7, 4, 5), (2, 9, 9), (5, 0, 0)):
        want = np.pad(np.arange(n), (before, after), mode="reflect")
        assert np.array_equal(G.reflect101(np.arange(-before, n + after), n), want), (n, before, after)
    # the pad stage: a 3 x 16 image in 16 x 16 reflects more than once (top = 6, bottom = 7)
    img = np.random.default_rng(2).integers(0, 256, (3, 16, 3), dtype=np.uint8)
    got = G.pad_stage(img, 16, 16, 0, True)
    assert np.array_equal(got, np.pad(img, ((6, 7), (0, 0), (0, 0)), mode="reflect"))
    one = np.random.default_rng(3).integers(0, 256, (1, 7, 3), dtype=np.uint8)
    assert np.array_equal(G.pad_stage(one, 16, 16, 0, True), np.pad(np.repeat(one, 16, 0)[:, :, :], ((0, 0), (4, 5), (0, 0)), mode="reflect"))
    # constant border, and the centred window of a larger image (C division: (16 - 21) / 2 = -2)
    const = G.pad_stage(img, 16, 16, 114, False)
    assert np.all(const[:6] == 114) and np.all(const[9:] == 114) and np.array_equal(const[6:9], img)
    big = np.random.default_rng(4).integers(0, 256, (21, 19, 3), dtype=np.uint8)
    assert G.cdiv2(-5) == -2 and G.cdiv2(-3) == -1 and G.cdiv2(5) == 2
    assert np.array_equal(G.pad_stage(big, 16, 16, 0, False), big[2:18, 1:17])


def _bilinear_f64(slot, box, Ho, Wo):
    """float64 bilinear with the same half-pixel centres and the same edge clamp"""
    y0, x0, bh, bw = box

    def axis(N, n):
        f = (np.arange(N) + 0.5) * (n / N) - 0.5
        i = np.floor(f).astype(np.int64)
        t = f - i
        low, high = i < 0, i >= n - 1
        i = np.where(low, 0, np.where(high, n - 1, i))
        return i, np.minimum(i + 1, n - 1), np.where(low | high, 0.0, t)

    iy, iy1, ty = axis(Ho, bh)
    ix, ix1, tx = axis(Wo, bw)
    P = slot.astype(np.float64)[y0:y0 + bh, x0:x0 + bw]
    top = P[iy][:, ix] * (1 - tx)[None, :, None] + P[iy][:, ix1] * tx[None, :, None]
    bot = P[iy1][:, ix] * (1 - tx)[None, :, None] + P[iy1][:, ix1] * tx[None, :, None]
    return top * (1 - ty)[:, None, None] + bot * ty[:, None, None]


def test_integer_bilinear_against_float64():
    """at most 1 level: 0.5 from the final rounding, and each of the two 11-bit coefficient roundings moves a weight by at most
    2^-12, which a 255-level difference between the blended pixels turns into at most 255 / 4096 levels"""
    rng = np.random.default_rng(5)
    slot = rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)
    worst = 0.0
    for box in ((0, 0, 24, 20), (3, 2, 3, 5), (8, 4, 16, 7), (23, 19, 1, 1), (11, 0, 13, 20)):
        got = G.resample(slot, G.make_geom(box=box, out=(16, 16)), 16, 16)
        err = float(np.abs(got - _bilinear_f64(slot, box, 16, 16)).max())
        print(f"box {box}: worst {err:.4f} levels")
        worst = max(worst, err)
        assert got.min() >= 0 and got.max() <= 255
    assert worst <= 0.5 + 2 * 255 / 4096 + 1e-9 <= 1.0


def test_records_round_trip_and_geometry_composes_with_the_colour_stages():
    taps = [(-7, -7), (0, 0), (7, 7), (-127, 127), (1, -1)]
    g = G.make_geom(box=(1, 2, 3, 5), out=(16, 12), taps=taps, reflect=True)
    assert g[0] == 7 and g[1:5].tolist() == [1, 2, 3, 5] and g[7] == 5 and G.taps_of(g) == taps
    assert g.view(np.float32)[5] == np.float32(3) / np.float32(16) and g.view(np.float32)[6] == np.float32(5) / np.float32(12)
    assert np.array_equal(g, hip.image_geom_record(box=(1, 2, 3, 5), out_size=(16, 12), taps=taps, reflect=True))
    # bit 4 with mask 0 is the constant pad stage in levels; without either record the float fill itself is padded
    img = np.random.default_rng(6).integers(0, 256, (5, 9, 3), dtype=np.uint8)
    import image_aug_reference as R
    zero = np.zeros(16, np.int32)
    for flag in range(4):
        a = G.plain_of(img, 5, 9, 16 | flag, None, zero, 12, 12, MEAN, STD, 114.7)
        assert np.array_equal(a, R.normalise(R.canvas(img, 12, 12, flag, 114.7), MEAN, STD))
        b = G.plain_of(img, 5, 9, flag, None, zero, 12, 12, MEAN, STD, 114.7)
        assert np.array_equal(b, R.plain(img, 12, 12, flag, MEAN, STD, 114.7)) and not np.array_equal(a, b)


# ---- the draws -------------------------------------------------------------------------------------------------------------------
FULL = dict(random_resized_crop=dict(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), p=0.75), motion_blur=dict(blur_limit=15, p=0.75),
            pad_border="reflect_101")


def test_draw_table_is_fixed_and_seeded():
    assert D.GEOM_KEYS == ("random_resized_crop", "motion_blur")
    spec = D.normalise_geom_spec(FULL)
    assert D.geom_table_columns(spec) == 41 + 8
    assert D.geom_table_columns(D.normalise_geom_spec(dict(motion_blur={}))) == 8
    assert D.geom_table_columns(D.normalise_geom_spec(dict(random_resized_crop={}))) == 41
    assert D.normalise_geom_spec(dict(motion_blur={}))["motion_blur"] == dict(blur_limit=(3, 7), allow_shifted=True, p=0.5)
    assert D.normalise_geom_spec(dict(random_resized_crop={}))["random_resized_crop"] == dict(scale=(0.08, 1.0), ratio=(0.75, 4 / 3), p=1.0)
    assert D.normalise_geom_spec({}) is None and D.normalise_geom_spec(dict(pad_border="constant")) is None
    B = len(SIZES)
    a = D.draw_image_geom(torch.Generator().manual_seed(3), B, SIZES, 16, FULL)
    b = D.draw_image_geom(torch.Generator().manual_seed(3), B, SIZES, 16, FULL)
    c = D.draw_image_geom(torch.Generator().manual_seed(4), B, SIZES, 16, FULL)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[1], c[1])
    assert a[0].dtype == torch.uint8 and a[1].dtype == torch.int32 and tuple(a[1].shape) == (B, 16)
    # the generator moves by exactly one B x K table, whatever the draws decide
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    D.draw_image_geom(g1, B, SIZES, 16, FULL)
    torch.rand(B, 49, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    # nothing asked for, or only the border: nothing is drawn
    for spec in ({}, dict(pad_border="reflect_101")):
        g = torch.Generator().manual_seed(1)
        state = g.get_state()
        bits, rec = D.draw_image_geom(g, B, SIZES, 16, spec)
        assert torch.equal(g.get_state(), state)
        assert bits.tolist() == ([16] * B if spec else [0] * B) and (rec[:, 0] == (4 if spec else 0)).all() and not rec[:, 1:].any()
    for bad in (dict(motion_blur=dict(blur_limit=4)), dict(motion_blur=dict(blur_limit=(1, 5))), dict(motion_blur=dict(blur_limit=17)),
                dict(motion_blur=dict(sigma=1)), dict(random_resized_crop=dict(scale=(0.0, 1.0))),
                dict(random_resized_crop=dict(ratio=(2.0, 1.0))), dict(random_resized_crop=dict(size=3)), dict(pad_border="wrap"),
                dict(shift_scale_rotate={})):
        with pytest.raises(ValueError):
            D.normalise_geom_spec(bad)


def test_turning_geometry_on_leaves_the_other_draws_alone():
    aug = dict(brightness_contrast=dict(p=0.5), coarse_dropout=dict(p=0.5))
    mix = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")
    B = 6
    old = D.DeviceLoader([], "cpu", 16, hflip_p=0.5, vflip_p=0.5, seed=9, mixup=mix, **aug)
    new = D.DeviceLoader([], "cpu", 16, hflip_p=0.5, vflip_p=0.5, seed=9, mixup=mix, **aug, **FULL)
    assert old.geom is None and new.geom == D.normalise_geom_spec(FULL)
    gen = torch.Generator().manual_seed(12)
    sizes = torch.from_numpy(SIZES.astype(np.int32))
    off = (B + 15) // 16 * 16
    for _ in range(3):
        a, amix = old._draw(B)
        b, bmix = new._draw(B, sizes)
        assert a.numel() == hip.image_aug_bytes(B) and b.numel() == hip.image_geom_bytes(B)
        assert torch.equal(a[:B], b[:B] & 15) and torch.equal(a[B:], b[B:a.numel()])
        assert (amix is None) == (bmix is None) and all(torch.equal(x, y) for x, y in zip(amix or (), bmix or ()))
        gbits, grec = D.draw_image_geom(gen, B, SIZES, 16, FULL)
        assert torch.equal(b[:B] & 16, gbits)
        assert np.array_equal(b[off + 256 * B:].numpy().view("<i4").reshape(B, 16), grec.numpy())
    # with no geometry key the buffers are the ones of pack_image_aug, and without any key there are none
    assert D.DeviceLoader([], "cpu", 16).draw_flags(B) is None
    only = D.DeviceLoader([], "cpu", 16, motion_blur=dict(p=1.0), seed=1).draw_flags(B)
    assert only.numel() == hip.image_geom_bytes(B) and (only[:B] == 16).all() and not only[off:off + 256 * B].any()


def test_boxes_lie_inside_each_image():
    B = 600
    sizes = np.stack([1 + np.arange(B) % 24, 1 + (np.arange(B) * 7) % 20], 1)
    spec = dict(random_resized_crop=dict(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), p=1.0))
    bits, rec = D.draw_image_geom(torch.Generator().manual_seed(0), B, sizes, 16, spec)
    rec = rec.numpy()
    y0, x0, bh, bw = (rec[:, k] for k in range(1, 5))
    assert (bits == 16).all() and (rec[:, 0] == 1).all()
    assert y0.min() >= 0 and x0.min() >= 0 and bh.min() >= 1 and bw.min() >= 1
    assert (y0 + bh <= sizes[:, 0]).all() and (x0 + bw <= sizes[:, 1]).all()
    f = rec.view(np.float32)
    assert np.array_equal(f[:, 5], bh.astype(np.float32) / np.float32(16)) and np.array_equal(f[:, 6], bw.astype(np.float32) / np.float32(16))
    assert len({(a, b) for a, b in zip(bh[sizes.min(1) > 12], bw[sizes.min(1) > 12])}) > 20         # the boxes do vary
    hip.pack_image_geom(bits, None, torch.from_numpy(rec), sizes=torch.from_numpy(sizes.astype(np.int32)))
    # p below 1: the images left alone carry no box
    bits, rec = D.draw_image_geom(torch.Generator().manual_seed(0), B, sizes, 16, dict(random_resized_crop=dict(p=0.5)))
    off = bits.numpy() == 0
    assert 0.4 < off.mean() < 0.6 and not rec.numpy()[off].any() and (rec.numpy()[~off, 0] == 1).all()


def test_the_fallback_crop():
    """a scale of 4 asks every attempt for four times the image's area: no attempt fits, the central crop with the aspect clamped
    into `ratio` is taken"""
    sizes = np.array([[24, 20], [6, 24], [24, 3], [10, 10]])
    spec = dict(random_resized_crop=dict(scale=(4.0, 4.0), ratio=(3 / 4, 4 / 3), p=1.0))
    _, rec = D.draw_image_geom(torch.Generator().manual_seed(0), 4, sizes, 16, spec)
    assert rec[:, 1:5].tolist() == [[0, 0, 24, 20],           # 20 / 24 lies inside the ratio: the whole image
                                    [0, 8, 6, 8],             # too wide: bh = h, bw = round(6 * 4 / 3), centred
                                    [10, 0, 4, 3],            # too tall: bw = w, bh = round(3 / (3 / 4)), centred
                                    [0, 0, 10, 10]]


def _tap_properties(rec, ksize_hi, symmetric):
    for r in rec:
        if not r[0] & 2:
            assert not r[7:].any()
            continue
        taps = G.taps_of(r)
        n = int(r[7])
        assert 1 <= n <= ksize_hi and len(taps) == n
        ys, xs = np.array([t[0] for t in taps]), np.array([t[1] for t in taps])
        c = ksize_hi // 2
        assert np.abs(ys).max() <= c and np.abs(xs).max() <= c                                        # inside the kernel
        assert n == max(abs(xs[-1] - xs[0]), abs(ys[-1] - ys[0])) + 1                                # one per major-axis step
        if n > 1:
            step = np.maximum(np.abs(np.diff(ys)), np.abs(np.diff(xs)))
            assert (step == 1).all()                                                                  # 8-adjacent
        assert len(set(taps)) == n
        if symmetric:
            assert n % 2 == 1 and sorted(taps) == sorted((-a, -b) for a, b in taps)
        # unused halves of the tap words are zero
        assert not (r[8:16].view(np.uint16)[n:]).any()


@pytest.mark.parametrize("allow_shifted", [True, False])
def test_motion_blur_taps(allow_shifted):
    B = 400
    for limit in (3, 7, (9, 15), (15, 15)):
        spec = dict(motion_blur=dict(blur_limit=limit, allow_shifted=allow_shifted, p=0.9))
        bits, rec = D.draw_image_geom(torch.Generator().manual_seed(7), B, None, 32, spec)
        rec = rec.numpy()
        hi = limit[1] if isinstance(limit, tuple) else limit
        assert np.array_equal(bits.numpy() == 16, rec[:, 0] == 2) and 0.8 < (rec[:, 0] == 2).mean() < 0.97
        _tap_properties(rec, hi, symmetric=not allow_shifted)
        counts = set(rec[rec[:, 0] == 2, 7].tolist())
        assert max(counts) <= hi and min(counts) >= (2 if allow_shifted else 1) and len(counts) > 1, counts
        if hi <= 7:
            assert max(counts) == hi and min(counts) == (2 if allow_shifted else 1), counts
    # the line pixels by hand: a shallow line rounds half up in its first half and mirrors it in the second
    assert D.line_taps(0, 0, 2, 4) == [(0, 0), (1, 1), (1, 2), (1, 3), (2, 4)]
    assert D.line_taps(3, 3, 3, 3) == [(3, 3)]
    assert D.line_taps(4, 0, 0, 1) == [(4, 0), (3, 0), (2, 1), (1, 1), (0, 1)]


# ---- the packed layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 16, 17])
def test_pack_image_geom_layout(B):
    assert (hip.IMAGE_GEOM_BIT, hip.IMAGE_GEOM_WORDS, hip.IMAGE_GEOM_MAX_TAPS) == (16, 16, 16)
    flags = ((torch.arange(B) % 16) | 16 * (torch.arange(B) % 2)).to(torch.uint8)
    rec = torch.arange(B * 64, dtype=torch.int32).reshape(B, 64) * 65537 - 5
    rec[:, 10] = (torch.arange(B) + 1) % B
    rec[:, 11] = 1 + torch.arange(B) % 2
    geom = torch.from_numpy(np.stack([G.make_geom(box=(b % 3, 1, 2 + b % 4, 3), out=(16, 16), taps=[(b % 5 - 2, -1), (0, 0), (1, 127)])
                                      for b in range(B)]))
    buf = hip.pack_image_geom(flags, rec, geom)
    off = (B + 15) // 16 * 16
    assert buf.dtype == torch.uint8 and buf.numel() == off + 256 * B + 64 * B == hip.image_geom_bytes(B) and buf.data_ptr() % 16 == 0
    assert torch.equal(buf[:off + 256 * B], hip.pack_image_aug(flags, rec))
    for b in (0, B - 1):
        assert np.array_equal(buf[off + 256 * B + 64 * b:off + 256 * B + 64 * (b + 1)].numpy().view("<i4"), geom[b].numpy())
    # tap t sits in half t % 2 of word 8 + t / 2: low byte dy, high byte dx
    raw = buf[off + 256 * B:].numpy().reshape(B, 64)
    assert raw[0, 32:38].view(np.int8).tolist() == [-2, -1, 0, 0, 1, 127]
    # no first table given: zero-filled, still present
    bare = hip.pack_image_geom(flags & 0x13, None, geom)
    assert bare.numel() == buf.numel() and not bare[B:off + 256 * B].any() and torch.equal(bare[off + 256 * B:], buf[off + 256 * B:])


def test_pack_image_geom_refusals():
    flags = torch.tensor([16, 16, 0], dtype=torch.uint8)
    sizes = torch.tensor([[10, 12], [10, 12], [10, 12]], dtype=torch.int32)

    def geom(**kw):
        return torch.from_numpy(np.stack([G.make_geom(**kw)] * 3))

    hip.pack_image_geom(flags, None, geom(box=(2, 3, 8, 9), out=(16, 16)), sizes=sizes)
    with pytest.raises(RuntimeError, match="outside its image"):
        hip.pack_image_geom(flags, None, geom(box=(3, 3, 8, 9), out=(16, 16)), sizes=sizes)
    with pytest.raises(RuntimeError, match="outside its image"):
        hip.pack_image_geom(flags, None, geom(box=(2, 4, 8, 9), out=(16, 16)), sizes=sizes)
    bad = geom(box=(2, 3, 8, 9), out=(16, 16))
    bad[1, 3] = 0
    with pytest.raises(RuntimeError, match="empty"):
        hip.pack_image_geom(flags, None, bad)
    for n in (0, 17, -1):
        bad = geom(taps=[(0, 0)])
        bad[0, 7] = n
        with pytest.raises(RuntimeError, match="tap count"):
            hip.pack_image_geom(flags, None, bad)
    bad = geom(taps=[(0, 0), (1, 1)])
    bad[1, 8] = 0x0180_0000                                  # tap 1: dy = -128
    with pytest.raises(RuntimeError, match="127"):
        hip.pack_image_geom(flags, None, bad)
    bad[2] = bad[1]
    bad[1] = geom(taps=[(0, 0)])[1]
    hip.pack_image_geom(flags, None, bad)                    # behind a clear bit 4 nothing is looked at
    for taps in ([], [(0, 0)] * 17, [(0, 128)], [(-128, 0)]):
        with pytest.raises(ValueError):
            hip.image_geom_record(taps=taps)
    with pytest.raises(RuntimeError, match="pack_image_geom"):
        hip.pack_image_geom(flags, None, geom(taps=[(0, 0)])[:, :15])


# ---- translation and plumbing ------------------------------------------------------------------------------------------------------
class _T:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _named(name, **kw):
    return type(name, (_T,), {})(**kw)


def _archived_stack(resize=256, border_mode=4, extra=None):
    """LongestMaxSize -> PadIfNeeded(BORDER_REFLECT_101) -> Resize(same size) -> MotionBlur -> RandomBrightnessContrast ->
    Normalize -> ToTensorV2, as the reference's archived configs build it"""
    ts = [_named("LongestMaxSize", max_size=256, p=1),
          _named("PadIfNeeded", min_height=256, min_width=256, border_mode=border_mode, value=None, p=1),
          _named("Resize", height=resize, width=resize, p=1),
          _named("MotionBlur", blur_limit=(3, 3), allow_shifted=True, p=0.5),
          _named("RandomBrightnessContrast", brightness_limit=(-0.2, 0.2), contrast_limit=(-0.2, 0.2), brightness_by_max=True, p=0.5),
          _named("Normalize", mean=MEAN, std=STD, p=1), _named("ToTensorV2", p=1)]
    if extra is not None:
        ts.insert(5, extra)                                  # behind RandomBrightnessContrast
    return _named("Compose", transforms=ts)


def test_pipeline_translation():
    keys = D.translate_pipeline(_archived_stack())
    assert keys["size"] == 256 and "source_size" not in keys and keys["pad_border"] == "reflect_101" and "fill" not in keys
    assert keys["motion_blur"] == dict(blur_limit=(3, 3), allow_shifted=True, p=0.5)
    assert D.normalise_geom_spec({k: keys.get(k) for k in D.GEOM_KEYS + ("pad_border",)}) == dict(
        motion_blur=dict(blur_limit=(3, 3), allow_shifted=True, p=0.5), pad_border="reflect_101")
    assert keys["brightness_contrast"]["p"] == 0.5 and keys["mean"] == MEAN
    assert D.translate_pipeline(_archived_stack(border_mode=0))["pad_border"] == "constant"
    with pytest.raises(NotImplementedError, match="Resize to 224 x 224"):
        D.translate_pipeline(_archived_stack(resize=224))
    with pytest.raises(NotImplementedError, match="border_mode 2"):
        D.translate_pipeline(_archived_stack(border_mode=2))
    with pytest.raises(NotImplementedError, match="GaussNoise"):
        D.translate_pipeline(_archived_stack(extra=_named("GaussNoise", p=0.5)))
    with pytest.raises(NotImplementedError, match="MotionBlur after RandomBrightnessContrast"):
        D.translate_pipeline(_archived_stack(extra=_named("MotionBlur", blur_limit=3, p=0.5)))
    # the timm-style stack: a crop from a larger host canvas
    timm = _named("Compose", transforms=[_named("LongestMaxSize", max_size=288, p=1), _named("PadIfNeeded", border_mode=0, value=0, p=1),
                                         _named("RandomResizedCrop", size=(224, 224), scale=(0.08, 1.0), ratio=(0.75, 4 / 3), p=1.0),
                                         _named("HorizontalFlip", p=0.5), _named("Normalize", mean=MEAN, std=STD, p=1)])
    keys = D.translate_pipeline(timm)
    assert keys["size"] == 224 and keys["source_size"] == 288 and keys["hflip_p"] == 0.5
    assert keys["random_resized_crop"] == dict(scale=(0.08, 1.0), ratio=(0.75, 4 / 3), p=1.0)
    old = _named("Compose", transforms=[_named("RandomResizedCrop", height=64, width=64, scale=(0.5, 1.0), ratio=(1.0, 1.0), p=1.0)])
    assert D.translate_pipeline(old)["size"] == 64


def _folder(tmp_path, shapes=((8, 8),)):
    from PIL import Image
    (tmp_path / "a").mkdir()
    rng = np.random.default_rng(0)
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "a" / f"{i}.png")


def test_get_dataset_plumbs_the_geometry_keys(tmp_path):
    _folder(tmp_path, ((30, 60), (40, 20)))
    base = dict(root=str(tmp_path), batch_size=2, device_pipeline=True, device="cpu")
    dl = D.get_dataset(base, _archived_stack())
    assert dl.size == 256 and dl.geom == dict(motion_blur=dict(blur_limit=(3, 3), allow_shifted=True, p=0.5), pad_border="reflect_101")
    assert D.get_dataset(base).geom is None
    dl = D.get_dataset(dict(base, size=16, source_size=24, random_resized_crop=dict(scale=(0.5, 1.0)), pad_border="constant"))
    assert dl.geom["random_resized_crop"]["p"] == 1.0 and dl.dataset.source_size == 24 and dl.dataset.size == 16
    raw, hw, _ = dl.dataset[0]
    assert tuple(raw.shape) == (24, 24, 3) and hw.tolist() == [12, 24]
    assert D.get_dataset(dict(base, size=16)).dataset[1][1].tolist() == [16, 8]
    for bad in (dict(source_size=24), dict(source_size=24, random_resized_crop=dict(p=0.5)), dict(source_size=24, motion_blur={}),
                dict(source_size=8, random_resized_crop={})):
        with pytest.raises(ValueError, match="source_size"):
            D.get_dataset(dict(base, size=16, **bad))
    with pytest.raises(NotImplementedError, match="device pipeline only"):
        D.get_dataset(dict(root=str(tmp_path), batch_size=2, motion_blur={}))


def test_sample_config_expresses_the_archived_stack(tmp_path):
    import runpy
    from pathlib import Path
    cfg = runpy.run_path(str(Path(__file__).resolve().parents[1] / "nkb-classification_amd" / "configs" / "folder_geometry_config.py"))
    _folder(tmp_path)
    dl = D.get_dataset(dict(cfg["train_data"], root=str(tmp_path), device="cpu", num_workers=0), cfg["train_pipeline"])
    assert dl.geom == dict(motion_blur=dict(blur_limit=(3, 3), allow_shifted=True, p=0.5), pad_border="reflect_101")
    assert dl.aug == D.normalise_aug_spec(dict(brightness_contrast=dict(brightness_limit=0.2, contrast_limit=0.2, p=0.5)))
    assert dl.size == cfg["img_size"] and dl.dataset.source_size == dl.size
    assert D.get_dataset(dict(cfg["val_data"], root=str(tmp_path), device="cpu", num_workers=0), cfg["val_pipeline"]).geom == dict(
        pad_border="reflect_101")
