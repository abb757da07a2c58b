"""Flag bit 4 of nkb_image_prep (the geometry record: crop-and-resample, reflect-101 pad, blur over taps; csrc/imgprep.hip, contract
in include/nkbhip.h) against the numpy restatement of tests/image_geom_reference.py, with torch.equal on the fp32 output: every
stage is integer arithmetic or a single rounded fp32 operation, so there is no tolerance.  The augmentation records used with it
are the ones whose arithmetic has no rounding (tests/test_image_mix_gpu.py explains the choice); the HSV stage is held through the
kernel's own un-geometried output.  Every output sits between guard zones that must survive and starts as NaN."""
import numpy as np
import pytest
import torch

import image_aug_reference as R
import image_geom_reference as G
import mix_reference as M

pytestmark = pytest.mark.gpu

from nkb_classification import dataset as D  # noqa: E402
from nkb_classification import hip  # noqa: E402

DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GUARD, SENT = 64, -12345.0
EXACT_BC = dict(alpha=0.5, offset=12.0)            # level * 0.5 + 12: no rounding in float32
ZERO_A = np.zeros(64, np.int32)


def _launch(src, sizes, flags, arecs, grecs, Ho, Wo, off=0, fill=114.0, second_table=True):
    B, Hs, Ws, _ = src.shape
    n = B * 3 * Ho * Wo
    buf = torch.full((GUARD + off + n + GUARD,), SENT, device=DEV)
    lo = GUARD + off
    buf[lo:lo + n] = float("nan")
    assert buf.data_ptr() % 16 == 0
    fl = torch.tensor(flags, dtype=torch.uint8)
    a = torch.from_numpy(np.stack(arecs).astype(np.int32)) if arecs is not None else None
    if second_table:
        packed = hip.pack_image_geom(fl, a, torch.from_numpy(np.stack(grecs).astype(np.int32)),
                                     sizes=torch.tensor(sizes, dtype=torch.int32) if sizes is not None else None)
        assert packed.numel() == (B + 15) // 16 * 16 + 256 * B + 64 * B
    else:
        packed = hip.pack_image_aug(fl, a) if a is not None else fl
    hip.image_prep(torch.from_numpy(src).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV) if sizes is not None else None,
                   packed.to(DEV), buf[lo:], B, Hs, Ws, Ho, Wo, MEAN, STD, fill)
    torch.cuda.synchronize()
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), "wrote outside the output"
    out = buf[lo:lo + n].cpu().reshape(B, 3, Ho, Wo)
    assert bool(torch.isfinite(out).all()), "output not written everywhere"
    return out


def _check(name, src, sizes, flags, arecs, grecs, Ho, Wo, off=0, fill=114.0):
    got = _launch(src, sizes, flags, arecs, grecs, Ho, Wo, off, fill)
    want = torch.from_numpy(G.batch(src, sizes, flags, arecs, grecs, Ho, Wo, MEAN, STD, fill))
    assert got.dtype == want.dtype == torch.float32
    if not torch.equal(got, want):
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{name}: images {bad} differ from the reference, worst {float((got - want).abs().max()):.4g}")
    return got


def _src(seed, B, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)


# B = 5 puts the tables at offsets 16 and 16 + 1280; the boxes: the whole image (downscale), one pixel, 3 x 5 (upscale), flush with the
# bottom-right corner (the i + 1 clamp), and bh == Ho on one axis only
RESAMPLE_SIZES = [(24, 20), (24, 20), (20, 17), (24, 20), (24, 20)]
RESAMPLE_BOXES = [(0, 0, 24, 20), (7, 3, 1, 1), (4, 9, 3, 5), (13, 11, 11, 9), (5, 2, 16, 13)]


@pytest.mark.parametrize("Wo,off", [(16, 0), (18, 1), (12, 0)], ids=["16-vec", "18-off1", "12-wave"])
def test_resample(Wo, off):
    """24 x 20 slots onto 16 x Wo.  Wo = 18 behind an `out` offset by one float takes the element stores, and its last group
    straddles the row end; with Wo = 12 a wave covers more than one image, and images with and without bit 4 alternate"""
    Ho = 16
    src = _src(Wo, 5, 24, 20)
    if Wo == 12:
        sizes = [(16, 12), (24, 20), (9, 12), (24, 20), (16, 5)]                       # the images without a box must fit
        flags = [0, 16 | 1, 2, 16 | 3, 4]
        arecs = [ZERO_A] * 4 + [R.make_record(**EXACT_BC)]
    else:
        sizes, flags, arecs = RESAMPLE_SIZES, [16, 16 | 1, 16 | 2, 16 | 3, 16], None
    boxes = [(0, 0, 16, 13) if Wo == 18 and b == 4 else box for b, box in enumerate(RESAMPLE_BOXES)]
    grecs = [G.make_geom(box=box, out=(Ho, Wo)) if flags[b] & 16 else np.full(16, 0x7F7F7F7F, np.int32) for b, box in enumerate(boxes)]
    got = _check(f"resample-{Wo}", src, sizes, flags, arecs, grecs, Ho, Wo, off)
    if Wo == 16:
        one = torch.from_numpy(R.normalise(np.broadcast_to(src[1, 7, 3].astype(np.int64), (16, 16, 3)), MEAN, STD))
        assert torch.equal(got[1], one), "a 1 x 1 box is not its pixel everywhere"


def test_reflect_101_pad():
    """3 x 16 and 1 x 7 in 16 x 16: more than one reflection, and the one-pixel axis; every flip; the same images with the constant
    border (in levels, and on the plain path) in the same batch"""
    S = 16
    src = _src(1, 12, 3, 16)
    src[6:] = src[:6]
    sizes = [(3, 16), (1, 7)] * 6
    flags = [16, 16, 16 | 1, 16 | 2, 16 | 3, 16 | 3, 16, 16 | 3, 0, 3, 16 | 2, 16 | 1]
    refl, const = G.make_geom(reflect=True), G.make_geom()
    grecs = [refl] * 6 + [const] * 6
    got = _check("reflect", src, sizes, flags, None, grecs, S, S)
    assert not torch.equal(got[0], got[6]) and not torch.equal(got[5], got[7])
    want0 = np.pad(src[0], ((6, 7), (0, 0), (0, 0)), mode="reflect")
    assert torch.equal(got[0], torch.from_numpy(R.normalise(want0, MEAN, STD)))


TAPS = {"n1": [(0, 0)], "diag15": [(d, d) for d in range(-7, 8)], "n16": [(d // 2 - 4, 7 - d) for d in range(16)],
        "far": [(-127, 127), (0, 0), (127, -127)]}


@pytest.mark.parametrize("Wo,off", [(16, 0), (18, 1)], ids=["16-vec", "18-off1"])
def test_blur(Wo, off):
    """one tap (the identity), 15 on the diagonal -7..7 (across both canvas edges and into the pad), 16, and offsets far beyond the
    canvas; both flips on; over a constant pad, a reflected pad and a resampled box"""
    Ho = 16
    src = _src(2 + Wo, 8, 24, 20)
    sizes = [(10, 13), (16, 7), (5, 16), (9, 9), (24, 20), (24, 20), (12, 12), (12, 12)]
    flags = [16 | 3] * 6 + [16 | 3, 3]
    grecs = [G.make_geom(taps=TAPS["n1"]), G.make_geom(taps=TAPS["diag15"]), G.make_geom(taps=TAPS["n16"], reflect=True),
             G.make_geom(taps=TAPS["far"], reflect=True), G.make_geom(taps=TAPS["diag15"], box=(2, 1, 20, 17), out=(Ho, Wo)),
             G.make_geom(taps=TAPS["n16"], box=(0, 0, 3, 4), out=(Ho, Wo)), G.make_geom(), G.make_geom()]
    got = _check(f"blur-{Wo}", src, sizes, flags, None, grecs, Ho, Wo, off)
    # one centre tap changes nothing: image 0 equals the launch without its blur bit
    bare = _launch(src[:1], sizes[:1], [16 | 3], None, [G.make_geom()], Ho, Wo, off)
    assert torch.equal(got[0], bare[0])


def test_composition():
    """geometry with an augmentation record (brightness/contrast + holes exactly, HSV through the kernel's own levels), a blend, a box
    whose partner has another geometry record, a partner without one, and an image with bit 4 and mask 0"""
    S = 16
    src = _src(3, 6, 24, 20)
    sizes = [(24, 20), (16, 16), (24, 20), (11, 16), (16, 9), (24, 20)]
    aug = dict(EXACT_BC, holes=[(1, 1, 4, 6), (10, 3, 16, 5)], hole_fill=(9, 200, 30))
    words = [M.make_mix_words(1, lam=0.3), M.make_mix_words(2, box=(2, 3, 13, 11)), M.make_mix_words(3, box=(0, 0, 16, 9)),
             M.make_mix_words(0, lam=0.75), None, M.make_mix_words(4, lam=0.5)]
    arecs = []
    for b, wd in enumerate(words):
        rec = R.make_record(**(aug if b in (0, 2, 5) else {}))
        if wd is not None:
            rec[10:16] = wd
        arecs.append(rec)
    #        crop+blur+aug, blend   mask 0, box     crop, box     no geometry, blend   reflect+blur   crop+aug, blend with 4
    flags = [16 | 8 | 4 | 1, 16 | 8 | 2, 16 | 8 | 4 | 3, 8 | 1, 16 | 2, 16 | 8 | 4]
    grecs = [G.make_geom(box=(3, 2, 18, 15), out=(S, S), taps=TAPS["diag15"][5:10]), G.make_geom(),
             G.make_geom(box=(0, 5, 24, 12), out=(S, S)), np.full(16, 0x7F7F7F7F, np.int32),
             G.make_geom(reflect=True, taps=[(0, -1), (0, 0), (0, 1)]), G.make_geom(box=(20, 16, 4, 4), out=(S, S))]
    got = _check("composition", src, sizes, flags, arecs, grecs, S, S)
    unmixed = _check("composition-unmixed", src, sizes, [f & ~8 for f in flags], arecs, grecs, S, S)
    assert all(not torch.equal(got[b], unmixed[b]) for b in (0, 1, 2, 3, 5)) and torch.equal(got[4], unmixed[4])
    # the HSV stage on geometry levels: the kernel's own record path on the levels the reference gives.  A source batch that IS
    # the reference's canvas (bit 4 off, full size) must give the bits of the geometry launch
    hsv = R.make_record(alpha=0.8, offset=-17.3, hsv=(37.3, -20.5, 12.25))
    geo = _launch(src[:3], sizes[:3], [16 | 4 | 1, 16 | 4, 16 | 4 | 2], [hsv] * 3, grecs[:1] + [grecs[4], grecs[2]], S, S)
    canv = np.stack([G.canvas_levels(src[b], *sizes[b], fl, g, S, S, 114.0) for b, fl, g in
                     ((0, 16 | 1, grecs[0]), (1, 16, grecs[4]), (2, 16 | 2, grecs[2]))]).astype(np.uint8)
    own = _launch(canv, None, [4, 4, 4], [hsv] * 3, None, S, S, second_table=False)
    assert torch.equal(geo, own)


def test_second_table_without_bit_4_changes_nothing():
    S = 16
    src = _src(4, 5, 14, 15)
    sizes = [(14, 15), (11, 15), (14, 11), (1, 1), (13, 13)]
    arecs = [R.make_record(**EXACT_BC, holes=[(2, 2, 5, 6)]) for _ in range(5)]
    arecs[1][10:16] = M.make_mix_words(3, lam=0.4)
    arecs[2][10:16] = M.make_mix_words(0, box=(1, 2, 9, 12))
    flags = [0, 8 | 1, 8 | 4 | 2, 3, 4]
    garbage = [np.full(16, 0x7F7F7F7F, np.int32)] * 5
    a = _launch(src, sizes, flags, arecs, garbage, S, S)
    b = _launch(src, sizes, flags, arecs, None, S, S, second_table=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _check("no-bit-4", src, sizes, flags, arecs, garbage, S, S)
    for off in (0, 1):
        a = _launch(src, sizes, [0, 1, 2, 3, 0], None, garbage, S, S, off)
        b = _launch(src, sizes, [0, 1, 2, 3, 0], None, None, S, S, off, second_table=False)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_source_canvas_larger_than_the_output():
    """Hs x Ws = 24 x 20 onto 16 x 16: crops from the whole slot, and images without the resample bit — with a record, with mask 0,
    with no bit at all — take their centred window ((16 - 21) / 2 = -2 as C divides)"""
    S = 16
    src = _src(5, 6, 24, 20)
    sizes = [(24, 20), (21, 19), (21, 19), (21, 19), (24, 9), (7, 20)]
    flags = [16 | 1, 16 | 2, 3, 4 | 1, 16 | 3, 0]
    arecs = [ZERO_A] * 3 + [R.make_record(**EXACT_BC)] + [ZERO_A] * 2
    grecs = [G.make_geom(box=(0, 0, 24, 20), out=(S, S)), G.make_geom(), G.make_geom(), G.make_geom(),
             G.make_geom(reflect=True, taps=TAPS["diag15"][6:9]), G.make_geom()]
    got = _check("larger-source", src, sizes, flags, arecs, grecs, S, S)
    assert torch.equal(got[1], torch.from_numpy(R.normalise(src[1, 2:18, 1:17][::-1], MEAN, STD)))
    # without flags the refusal stays
    with pytest.raises(RuntimeError, match="image_prep"):
        hip.image_prep(torch.from_numpy(src).to(DEV), None, None, torch.empty(6, 3, S, S, device=DEV), 6, 24, 20, S, S, MEAN, STD, 0.0)


def test_device_loader_end_to_end(tmp_path):
    """six seeded PNGs of unequal sizes through get_dataset: the first batch must equal the reference applied to the loader's own
    draws (a second loader with the same seed gives them)"""
    from PIL import Image
    (tmp_path / "a").mkdir()
    rng = np.random.default_rng(6)
    for i, (h, w) in enumerate(((30, 60), (40, 20), (24, 24), (5, 50), (33, 31), (48, 47))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "a" / f"{i}.png")
    data = dict(root=str(tmp_path), batch_size=6, device_pipeline=True, device=DEV, size=16, source_size=24, seed=5, fill=114.0,
                hflip_p=0.5, vflip_p=0.5, random_resized_crop=dict(scale=(0.3, 1.0), p=1.0), motion_blur=dict(blur_limit=7, p=0.7),
                brightness_contrast=dict(brightness_limit=(0.0, 0.0), contrast_limit=(-0.5, -0.5), p=0.5),
                coarse_dropout=dict(max_holes=3, max_height=5, max_width=4, fill_value=7, p=0.5),
                mixup=dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"))
    out, target = next(iter(D.get_dataset(data)))
    torch.cuda.synchronize()
    twin = D.get_dataset(dict(data, device="cpu"))
    raw, sizes, labels = next(iter(twin.loader))
    assert tuple(raw.shape) == (6, 24, 24, 3) and sizes[0].tolist() == [12, 24]
    packed, mix = twin._draw(6, sizes)
    off = 16
    flags = packed[:6].tolist()
    arecs = packed[off:off + 256 * 6].numpy().view("<i4").reshape(6, 64)
    grecs = packed[off + 256 * 6:].numpy().view("<i4").reshape(6, 16)
    assert all(f & 16 for f in flags) and (grecs[:, 0] & 1).all() and (grecs[:, 0] & 2).any() and any(f & 4 for f in flags)
    want = torch.from_numpy(G.batch(raw.numpy(), sizes.numpy(), flags, arecs, grecs, 16, 16, MEAN, STD, 114.0))
    assert torch.equal(out.cpu(), want)
    if mix is None:
        assert torch.equal(target.cpu(), torch.as_tensor(labels))
