"""nkb_image_prep with augmentation records (flag bit 2; csrc/imgprep.hip) against the numpy restatement of
tests/image_aug_reference.py.

Acceptance: with mean 0 and std 1 the levels are round(255 out).  They equal the float32-order reference everywhere outside the
float64 tie band; inside the band one level of difference is allowed; band membership comes from the float64 reference and its
share is at most 2 % (tests/test_image_aug_cpu.py shows on the reference alone that the two orders differ only there).  The same
launch with the ImageNet mean and std equals Normalize of the levels to rtol = atol = 1e-6.  Every output sits between guard zones
that must survive, starts as NaN, and every case runs on the 16-byte stores ((32, 32), aligned) and on the element stores
((30, 37), `out` one float off its 16-byte boundary).  Every image is smaller than its canvas, so pad pixels exist."""
import math

import numpy as np
import pytest
import torch

import image_aug_reference as R

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402
from nkb_classification import dataset as D  # noqa: E402

DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GUARD, SENT = 64, -12345.0
GEOMETRIES = [pytest.param((32, 32, 0), id="32x32-vec"), pytest.param((30, 37, 1), id="30x37-off1")]
GARBAGE = np.full(64, 0x7F7F7F7F, np.int32)
BAND_CAP = 0.02


def _launch(src, sizes, flag_bytes, records, Ho, Wo, mean, std, fill, off):
    """one launch into a guarded output `off` floats behind a 16-byte boundary; records None: the flags go alone"""
    B, Hs, Ws, _ = src.shape
    n = B * 3 * Ho * Wo
    buf = torch.full((GUARD + off + n + GUARD,), SENT, device=DEV)
    lo = GUARD + off
    buf[lo:lo + n] = float("nan")
    assert buf.data_ptr() % 16 == 0
    flags = None
    if flag_bytes is not None:
        flags = torch.tensor(flag_bytes, dtype=torch.uint8)
        if records is not None:
            flags = hip.pack_image_aug(flags, torch.from_numpy(np.stack(records).astype(np.int32)))
        flags = flags.to(DEV)
    hip.image_prep(torch.from_numpy(src).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV) if sizes is not None else None,
                   flags, buf[lo:], B, Hs, Ws, Ho, Wo, mean, std, fill)
    torch.cuda.synchronize()
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), "wrote outside the output"
    return buf[lo:lo + n].cpu().numpy().reshape(B, 3, Ho, Wo)


def _reference(src, sizes, flag_bytes, records, Ho, Wo, fill):
    lv, band = [], []
    for b in range(src.shape[0]):
        h, w = sizes[b] if sizes is not None else src.shape[1:3]
        a = R.levels_of(src[b, :h, :w], Ho, Wo, flag_bytes[b], records[b], fill)
        a64, bd = R.levels_of(src[b, :h, :w], Ho, Wo, flag_bytes[b], records[b], fill, "f64")
        assert np.abs(a - a64).max() <= 1 and not ((a != a64) & ~bd).any()
        lv.append(a)
        band.append(bd)
    return np.stack(lv), np.stack(band)


def _judge(name, src, sizes, flag_bytes, records, Ho, Wo, fill, off):
    """the acceptance of the module docstring for one batch"""
    ref, band = _reference(src, sizes, flag_bytes, records, Ho, Wo, fill)
    share = band.mean()
    out = _launch(src, sizes, flag_bytes, records, Ho, Wo, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), fill, off)
    assert np.isfinite(out).all(), f"{name}: output not written everywhere"
    got = np.rint(out.astype(np.float64) * 255.0).astype(np.int64).transpose(0, 2, 3, 1)
    assert np.abs(got / 255.0 - out.transpose(0, 2, 3, 1)).max() < 1e-6, f"{name}: outputs are not levels / 255"
    diff = np.abs(got - ref)
    outside, inside = int(diff[~band].max(initial=0)), int(diff[band].max(initial=0))
    print(f"LEVELS {name}: {int((diff != 0).sum())} of {diff.size} differ from the float32 order (outside the band: worst {outside}; "
          f"inside: worst {inside}), band share {share:.4f}")
    assert share <= BAND_CAP, f"{name}: tie band share {share:.4f}"
    assert outside == 0, f"{name}: {int((diff[~band] != 0).sum())} levels differ outside the tie band, worst {outside}"
    assert inside <= 1, f"{name}: a level inside the tie band differs by {inside}"
    out2 = _launch(src, sizes, flag_bytes, records, Ho, Wo, MEAN, STD, fill, off)
    want = np.stack([R.normalise(g, MEAN, STD) for g in got])
    torch.testing.assert_close(torch.from_numpy(out2), torch.from_numpy(want), rtol=1e-6, atol=1e-6)
    return got


def _images(rng, B, Ho, Wo):
    """B random images, every one smaller than the canvas in at least one direction, odd and even margins"""
    Hs, Ws = Ho - 2, Wo - 1
    sizes = [(Hs, Ws), (Hs - 5, Ws), (Hs, Ws - 9), (1, 1), (Hs - 3, Ws - 4), (7, Ws)][:B]
    return rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8), sizes


@pytest.mark.parametrize("fill", [0.0, 114.0])
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_per_image_mixes_in_one_batch(geom, fill):
    """no record (garbage behind the clear bit), brightness/contrast only, HSV only, holes only, all three, all three with both
    flips — one wave straddles images that take different paths"""
    Ho, Wo, off = geom
    src, sizes = _images(np.random.default_rng(3), 6, Ho, Wo)
    holes = [(2, 3, 9, 11), (Ho - 6, Wo - 7, Ho, Wo), (10, 0, 14, 5)]
    records = [GARBAGE,
               R.make_record(alpha=0.8, offset=-17.3),
               R.make_record(hsv=(37.3, -20.5, 12.25)),
               R.make_record(holes=holes, hole_fill=(0, 0, 1)),
               R.make_record(alpha=1.0625, offset=30.5, hsv=(-5.5, 8.25, 41.0), holes=holes[:2], hole_fill=(255, 128, 7)),
               R.make_record(alpha=0.5625, offset=12.75, hsv=(91.0, -3.0, -22.5), holes=holes, hole_fill=(9, 8, 7))]
    flag_bytes = [2, 4 | 1, 4, 4 | 2, 4, 4 | 3]
    got = _judge(f"mix-{Ho}x{Wo}-fill{fill:g}", src, sizes, flag_bytes, records, Ho, Wo, fill, off)
    plain = _launch(src, sizes, [f & 3 for f in flag_bytes], None, Ho, Wo, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), fill, off)
    plain = np.rint(plain * 255.0).astype(np.int64).transpose(0, 2, 3, 1)
    assert np.array_equal(got[0], plain[0]), "the record behind a clear bit 2 was not ignored"
    for b in range(1, 6):
        assert (got[b] != plain[b]).mean() > 0.02, f"image {b} left the kernel unaugmented"


@pytest.mark.parametrize("geom", [pytest.param((66, 68, 0), id="66x68-vec"), pytest.param((65, 67, 1), id="65x67-off1")])
def test_lattice_under_the_six_shift_triples(geom):
    Ho, Wo, off = geom
    src = np.stack([R.lattice()] * 6)
    records = [R.make_record(hsv=t) for t in R.SHIFT_TRIPLES]
    _judge(f"lattice-{Ho}x{Wo}", src, None, [4, 5, 6, 7, 4, 7], records, Ho, Wo, 114.0, off)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_saturating_brightness_contrast(geom):
    Ho, Wo, off = geom
    src, sizes = _images(np.random.default_rng(4), 6, Ho, Wo)
    src[0, :4, :4] = np.arange(48, dtype=np.uint8).reshape(4, 4, 3) * 5
    records = [R.make_record(alpha=3.0, offset=-100.0), R.make_record(alpha=0.0, offset=300.0), R.make_record(alpha=1.0, offset=-300.0),
               R.make_record(alpha=0.5, offset=0.0), R.make_record(alpha=1.5, offset=25.5), R.make_record(alpha=1.0, offset=0.0)]
    got = _judge(f"saturate-{Ho}x{Wo}", src, sizes, [4, 5, 6, 7, 4, 4], records, Ho, Wo, 114.0, off)
    assert np.all(got[1] == 255) and np.all(got[2] == 0) and got[0].min() == 0 and got[0].max() == 255


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_holes(geom):
    """none and twelve of them, one across the image / pad edge, one at each canvas border, one of zero area, and boxes that
    reach past the canvas (only comparisons touch them)"""
    Ho, Wo, off = geom
    src, sizes = _images(np.random.default_rng(5), 6, Ho, Wo)
    rng = np.random.default_rng(6)
    twelve = []
    for _ in range(12):
        y1, x1 = int(rng.integers(0, Ho - 4)), int(rng.integers(0, Wo - 4))
        twelve.append((y1, x1, y1 + int(rng.integers(1, 5)), x1 + int(rng.integers(1, 5))))
    h2, w2 = sizes[2]
    left2 = (Wo - w2) // 2
    borders = [(0, 5, 3, 11), (Ho - 3, 5, Ho, 11), (5, 0, 11, 3), (5, Wo - 3, 11, Wo)]
    records = [R.make_record(holes=[], hole_fill=(1, 2, 3)),
               R.make_record(holes=twelve, hole_fill=(0, 0, 1)),
               R.make_record(holes=[(8, left2 - 3, 14, left2 + 4)], hole_fill=(255, 0, 128)),
               R.make_record(holes=borders, hole_fill=(7, 7, 7)),
               R.make_record(holes=[(6, 6, 6, 20), (9, 12, 20, 12), (3, 3, 5, 6)], hole_fill=(200, 100, 50)),
               R.make_record(holes=[(-4, -4, 2, 2), (Ho - 2, Wo - 2, Ho + 9, Wo + 9)], hole_fill=(11, 22, 33))]
    got = _judge(f"holes-{Ho}x{Wo}", src, sizes, [4, 5, 6, 7, 4, 4], records, Ho, Wo, 114.0, off)
    assert (got[4] == (200, 100, 50)).all(-1).sum() == 6                # only the 2 x 3 box has area


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_flags_without_a_record_are_bit_identical(geom):
    Ho, Wo, off = geom
    src, sizes = _images(np.random.default_rng(7), 6, Ho, Wo)
    flag_bytes = [0, 1, 2, 3, 3, 1]
    for fill in (0.0, 114.0):
        out = _launch(src, sizes, flag_bytes, None, Ho, Wo, MEAN, STD, fill, off)
        for b in range(6):
            h, w = sizes[b]
            assert np.array_equal(out[b], R.plain(src[b, :h, :w], Ho, Wo, flag_bytes[b], MEAN, STD, fill)), (b, fill)
    out = _launch(src, None, None, None, Ho, Wo, MEAN, STD, 114.0, off)
    assert np.array_equal(out[2], R.plain(src[2], Ho, Wo, 0, MEAN, STD, 114.0))
    with pytest.raises(RuntimeError, match="pack_image_aug"):
        hip.image_prep(torch.from_numpy(src).to(DEV), None, torch.zeros(7, dtype=torch.uint8, device=DEV),
                       torch.empty(6 * 3 * Ho * Wo, device=DEV), 6, src.shape[1], src.shape[2], Ho, Wo, MEAN, STD)


SINGLETASK = dict(
    brightness_contrast=dict(brightness_limit=(-0.2, 0.2), contrast_limit=(0.1, -0.5), p=0.5),
    hue_saturation_value=dict(hue_shift_limit=0, sat_shift_limit=10, val_shift_limit=50, p=0.5),
    coarse_dropout=dict(max_holes=4, min_holes=1, max_height=0.2, min_height=0.05, max_width=0.2, min_width=0.05,
                        fill_value=[0, 0.5, 1], p=0.5))


def test_device_loader_with_all_three_options():
    """five batches of 4 at size 40, seed 9: flips replayed from Generator(9), records from Generator(10); the tie band share is
    that of a launch (one batch), as in _judge: a single small image whose offset is drawn next to an integer can exceed it"""
    rng = np.random.default_rng(5)
    size, nb, B = 40, 5, 4
    batches = []
    for k in range(nb):
        raw = torch.from_numpy(rng.integers(0, 256, (B, size, size, 3), dtype=np.uint8))
        sizes = torch.tensor([[size - (k + i) % 7, size - (2 * k + i) % 5] for i in range(B)], dtype=torch.int32)
        batches.append((raw, sizes, torch.arange(B) + 10 * k))
    spec = dict(SINGLETASK, hue_saturation_value=dict(hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20, p=0.7))
    dl = D.DeviceLoader(batches, DEV, size, hflip_p=0.5, vflip_p=0.5, seed=9, **spec)
    g_flip, g_aug = torch.Generator().manual_seed(9), torch.Generator().manual_seed(10)
    seen = augmented = 0
    for k, (img, target) in enumerate(dl):
        assert img.is_cuda and img.dtype == torch.float32 and img.shape == (B, 3, size, size)
        assert target.tolist() == (torch.arange(B) + 10 * k).tolist()
        u = torch.rand(B, 2, generator=g_flip)
        bits, rec = D.draw_image_aug(g_aug, B, size, spec)
        raw, sizes, _ = batches[k]
        got = img.cpu().numpy()
        shares = []
        for i in range(B):
            flag = int(u[i, 0] < 0.5) | (int(u[i, 1] < 0.5) << 1) | int(bits[i])
            h, w = sizes[i].tolist()
            lv = R.levels_of(raw[i, :h, :w].numpy(), size, size, flag, rec[i].numpy(), 0.0)
            _, band = R.levels_of(raw[i, :h, :w].numpy(), size, size, flag, rec[i].numpy(), 0.0, "f64")
            shares.append(band.mean())
            want = R.normalise(lv, MEAN, STD)
            level = (1.0 / (255.0 * np.asarray(STD)))[:, None, None]
            err = np.abs(got[i] - want)
            tol = 1e-6 + 1e-6 * np.abs(want)
            bd = band.transpose(2, 0, 1)
            assert (err[~bd] <= tol[~bd]).all(), f"batch {k} image {i}: worst {err[~bd].max():.3e} outside the tie band"
            assert (err <= tol + level * 1.000001).all(), f"batch {k} image {i}: more than one level inside the tie band"
            augmented += int(bits[i]) // 4
        print(f"batch {k}: band share {np.mean(shares):.4f}")
        assert np.mean(shares) <= BAND_CAP, f"batch {k}: tie band share {np.mean(shares):.4f}"
        seen += 1
    assert seen == nb and 0 < augmented <= nb * B


def test_train_epoch_with_augmenting_device_pipeline(tmp_path):
    """get_dataset on a PNG folder with the three keys set drives one train_epoch of resnet_tiny_basic: finite losses, and the
    same loss list from a second run with the same seeds"""
    import types
    from PIL import Image
    from nkb_classification.engine import train_epoch
    from nkb_classification.logging import BaseLogger
    from nkb_classification.losses import get_loss
    from nkb_classification.model import get_model
    from nkb_classification.utils import get_optimizer
    rng = np.random.default_rng(1)
    for cls, n in (("a", 5), ("b", 3)):
        (tmp_path / cls).mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (64, 48 + 2 * i, 3), dtype=np.uint8)).save(tmp_path / cls / f"{i}.png")
    data = dict(root=str(tmp_path), size=64, batch_size=4, num_workers=0, shuffle=False, device_pipeline=True, device=DEV,
                hflip_p=0.5, vflip_p=0.5, seed=3, **{k: dict(v, p=1.0) for k, v in SINGLETASK.items()})
    cfg = types.SimpleNamespace(task="single", enable_mixed_presicion=False, log_gradients=False,
                                show_full_current_loss_in_terminal=False)
    cfg_model = dict(model="resnet_tiny_basic", pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0,
                     classifier_initialization="kaiming_normal_", task="single")
    runs, first = [], []
    for _ in range(2):
        loader = D.get_dataset(data)
        assert loader.aug is not None and loader.dataset.classes == ["a", "b"]
        first.append(next(iter(D.get_dataset(data)))[0].cpu())
        torch.manual_seed(0)
        model = get_model(cfg_model, ["a", "b"], DEV)
        opt = get_optimizer(model, dict(type="sgd", lr=0.01))
        crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
        res = train_epoch(model, loader, opt, None, torch.amp.GradScaler("cuda", enabled=False), crit, DEV, cfg,
                          BaseLogger(cfg, ["a", "b"]))
        assert len(res["running_loss"]) == 2 and all(math.isfinite(v) for v in res["running_loss"])
        runs.append([float(v) for v in res["running_loss"]])
    assert runs[0] == runs[1], runs
    assert torch.equal(first[0], first[1])
    plain = next(iter(D.get_dataset({k: v for k, v in data.items() if k not in D.AUG_KEYS})))[0].cpu()
    assert (plain != first[0]).float().mean() > 0.5, "the augmenting loader's batch equals the plain one"
