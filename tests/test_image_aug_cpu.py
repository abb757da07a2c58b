"""Device-side colour augmentations and CoarseDropout, the parts that need no GPU: the numpy restatement of the kernel's
record path (tests/image_aug_reference.py) against hand-computed answers, its float32 order against its float64 order (the tie
band the GPU test relies on), the host draws of dataset.draw_image_aug, the pipeline translation and the packed layout."""
import numpy as np
import pytest
import torch

import image_aug_reference as R
from nkb_classification import dataset as D
from nkb_classification import hip

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# the reference's single-task training stack (configs/singletask_config.py:162-201) in this package's keys
SINGLETASK = dict(
    brightness_contrast=dict(brightness_limit=(-0.2, 0.2), contrast_limit=(0.1, -0.5), p=0.5),
    hue_saturation_value=dict(hue_shift_limit=0, sat_shift_limit=10, val_shift_limit=50, p=0.5),
    coarse_dropout=dict(max_holes=4, min_holes=1, max_height=0.2, min_height=0.05, max_width=0.2, min_width=0.05,
                        fill_value=[0, 0.5, 1], p=0.5))


def _px(*rgb):
    return np.array([[rgb]], np.int64)


def test_hand_computed_answers():
    assert R.brightness_contrast(np.array([100, 200]), 1.5, 25.5).tolist() == [175, 255]
    assert [int(a) for a in R.rgb_to_hsv(np.array([255, 0, 0]))] == [0, 255, 255]
    assert R.augment(_px(255, 0, 0), R.make_record(hsv=(60, 0, 0))).tolist() == [[[0, 255, 0]]]
    grey = np.stack([np.arange(256)] * 3, -1)[None]
    # grey has s == 0: any hue shift and any saturation shift that leaves s at 0 (a clamped negative one; a positive one tints
    # grey towards h == 0, in OpenCV's tables as here) give the level back
    for hue, sat in ((123.0, 0.0), (-33.3, 0.0), (0.0, -255.0), (77.7, -40.5)):
        assert np.array_equal(R.augment(grey, R.make_record(hsv=(hue, sat, 0.0))), grey), (hue, sat)
    assert np.array_equal(R.augment(grey, R.make_record(hsv=(0.0, 0.0, 30.0))), np.minimum(grey + 30, 255))
    assert np.array_equal(R.augment(grey, R.make_record(hsv=(0.0, 0.0, -30.5))), np.maximum(np.trunc(grey - 30.5), 0))
    # a record that changes nothing equals the plain pad / flip / normalise path
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    rec = R.make_record(alpha=1.0, offset=0.0, hsv=(0, 0, 0), holes=[])
    assert rec[0] == 7
    for flag in range(4):
        for fill in (0.0, 114.0):
            a = R.normalise(R.levels_of(img, 16, 20, flag | 4, rec, fill), MEAN, STD)
            assert np.array_equal(a, R.plain(img, 16, 20, flag, MEAN, STD, fill))
    # a box paints the fill levels, half-open, in canvas coordinates
    lv = R.augment(np.full((6, 8, 3), 9), R.make_record(holes=[(1, 2, 3, 5), (4, 4, 4, 8)], hole_fill=(1, 2, 3)))
    want = np.full((6, 8, 3), 9)
    want[1:3, 2:5] = (1, 2, 3)
    assert np.array_equal(lv, want)


def test_hsv_round_trip_on_the_lattice():
    """zero shift: one hue step of 2 degrees moves a channel by at most 255 / 30 = 8.5 levels, a saturation step by one"""
    lat = R.lattice().astype(np.int64)
    back = R.hsv_to_rgb(*R.rgb_to_hsv(lat))
    worst = int(np.abs(back - lat).max())
    print(f"worst round-trip error {worst} levels")
    assert worst <= 10


def test_float32_order_against_float64_tie_band():
    lat = R.lattice()
    differ = in_band = total = 0
    for triple in R.SHIFT_TRIPLES:
        rec = R.make_record(hsv=triple)
        a = R.augment(lat, rec)
        b, band = R.augment(lat, rec, "f64")
        d = a != b
        print(f"{triple}: {int(d.sum())} differ, band {int(band.sum())}")
        assert np.abs(a - b).max() <= 1
        assert not (d & ~band).any(), "the two orders differ outside the tie band"
        differ, in_band, total = differ + int(d.sum()), in_band + int(band.sum()), total + band.size
    print(f"{differ} of {total} differ, band share {in_band / total:.4f}")
    assert total == 73728 and in_band <= 0.02 * total


def test_draw_ranges_and_geometry():
    B, size = 4096, 128
    bits, rec = D.draw_image_aug(torch.Generator().manual_seed(3), B, size, SINGLETASK)
    bits2, rec2 = D.draw_image_aug(torch.Generator().manual_seed(3), B, size, SINGLETASK)
    assert torch.equal(bits, bits2) and torch.equal(rec, rec2)
    assert bits.dtype == torch.uint8 and rec.dtype == torch.int32 and tuple(rec.shape) == (B, 64)
    rec = rec.numpy()
    f = rec.view(np.float32)
    mask = rec[:, 0]
    assert np.array_equal(bits.numpy(), np.where(mask != 0, 4, 0)) and set(np.unique(mask)) == set(range(8))
    for bit in range(3):
        share = ((mask >> bit) & 1).mean()
        assert abs(share - 0.5) < 0.05, (bit, share)
    bc, hsv, cd = (mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0
    # contrast_limit (0.1, -0.5) is the interval [-0.5, 0.1]: alpha in [0.5, 1.1]
    assert f[bc, 1].min() >= 0.5 and f[bc, 1].max() <= np.float32(1.1) and f[bc, 1].min() < 0.55 and f[bc, 1].max() > 1.05
    assert np.abs(f[bc, 2]).max() <= 51.0 and f[bc, 2].min() < -45 and f[bc, 2].max() > 45
    assert np.all(f[~bc, 1] == 1) and np.all(f[~bc, 2] == 0)
    assert np.all(f[:, 3] == 0) and np.abs(f[hsv, 4]).max() <= 10 and np.abs(f[hsv, 5]).max() <= 50 and np.abs(f[hsv, 5]).max() > 45
    assert np.all(f[~hsv, 3:6] == 0)
    assert set(np.unique(rec[cd, 6])) == {1, 2, 3, 4} and np.all(rec[~cd, 6] == 0)
    assert np.all(rec[cd, 7:10] == (0, 0, 1)) and np.all(rec[:, 10:16] == 0)
    boxes = rec[:, 16:64].reshape(B, 12, 4)
    used = np.arange(12)[None] < rec[:, 6][:, None]
    assert np.all(boxes[~used] == 0)
    y1, x1, y2, x2 = (boxes[used][:, k] for k in range(4))
    assert y1.min() >= 0 and x1.min() >= 0 and y2.max() <= size and x2.max() <= size
    for ext in (y2 - y1, x2 - x1):
        assert ext.min() >= int(size * 0.05) and ext.max() <= int(size * 0.2) and ext.min() < ext.max()
    # pixel-count limits: randint with both ends
    _, r2 = D.draw_image_aug(torch.Generator().manual_seed(4), 2048, 40, dict(coarse_dropout=dict(
        max_holes=12, min_holes=12, max_height=9, min_height=3, max_width=5, min_width=5, fill_value=300.7, p=1.0)))
    r2 = r2.numpy()
    bx = r2[:, 16:64].reshape(-1, 4)
    assert np.all(r2[:, 6] == 12) and np.all(r2[:, 7:10] == 300 % 256)
    assert set(np.unique(bx[:, 2] - bx[:, 0])) == set(range(3, 10)) and np.all(bx[:, 3] - bx[:, 1] == 5)
    assert bx[:, 0].min() == 0 and bx[:, 2].max() == 40 and bx[:, 1].min() == 0 and bx[:, 3].max() == 40
    with pytest.raises(ValueError, match="12"):
        D.draw_image_aug(torch.Generator(), 4, 40, dict(coarse_dropout=dict(max_holes=13)))
    with pytest.raises(ValueError, match="12"):
        D.DeviceLoader([], "cpu", 40, coarse_dropout=dict(max_holes=13))
    # no transform: nothing is drawn
    g = torch.Generator().manual_seed(1)
    state = g.get_state()
    bits, rec = D.draw_image_aug(g, 5, 40, {})
    assert not bits.any() and not rec.any() and torch.equal(g.get_state(), state)


def test_device_loader_draws_come_from_two_generators():
    B = 6
    plain = D.DeviceLoader([], "cpu", 40, hflip_p=0.5, vflip_p=0.5, seed=9)
    full = D.DeviceLoader([], "cpu", 40, hflip_p=0.5, vflip_p=0.5, seed=9, **SINGLETASK)
    assert plain.aug is None
    g0, g1 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(10)
    for _ in range(3):
        u = torch.rand(B, 2, generator=g0)
        flips = (u[:, 0] < 0.5).to(torch.uint8) | ((u[:, 1] < 0.5).to(torch.uint8) << 1)
        got = plain.draw_flags(B)
        assert got.dtype == torch.uint8 and torch.equal(got, flips)
        bits, rec = D.draw_image_aug(g1, B, 40, SINGLETASK)
        assert torch.equal(full.draw_flags(B), hip.pack_image_aug(flips | bits, rec))
    assert D.DeviceLoader([], "cpu", 40).draw_flags(B) is None


class _T:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _named(name, **kw):
    return type(name, (_T,), {})(**kw)


def _singletask_pipeline(extra=None):
    ts = [_named("LongestMaxSize", max_size=128, p=1), _named("PadIfNeeded", min_height=128, min_width=128, value=0, p=1),
          _named("HorizontalFlip", p=0.5), _named("VerticalFlip", p=0.5),
          _named("RandomBrightnessContrast", brightness_limit=(-0.2, 0.2), contrast_limit=(0.1, -0.5), brightness_by_max=True, p=0.5),
          _named("HueSaturationValue", hue_shift_limit=0, sat_shift_limit=10, val_shift_limit=50, p=0.5),
          _named("CoarseDropout", max_holes=4, min_holes=1, max_height=0.2, min_height=0.05, max_width=0.2, min_width=0.05,
                 fill_value=[0, 0.5, 1], p=0.5),
          _named("Normalize", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), p=1), _named("ToTensorV2", p=1)]
    if extra is not None:
        ts.insert(4, extra)
    return _named("Compose", transforms=ts)


def test_pipeline_translation():
    keys = D.translate_pipeline(_singletask_pipeline())
    assert keys["size"] == 128 and keys["fill"] == 0.0 and keys["hflip_p"] == keys["vflip_p"] == 0.5
    assert keys["mean"] == MEAN and keys["std"] == STD
    assert D.normalise_aug_spec({k: keys[k] for k in D.AUG_KEYS}) == D.normalise_aug_spec(SINGLETASK)
    assert D.normalise_aug_spec(SINGLETASK)["hue_saturation_value"]["sat_shift_limit"] == (-10, 10)
    assert D.normalise_aug_spec(SINGLETASK)["coarse_dropout"]["fill_value"] == (0, 0, 1)
    with pytest.raises(NotImplementedError, match="GaussNoise"):
        D.translate_pipeline(_singletask_pipeline(_named("GaussNoise", p=0.5)))
    swapped = _singletask_pipeline()
    swapped.transforms[4], swapped.transforms[5] = swapped.transforms[5], swapped.transforms[4]
    with pytest.raises(NotImplementedError, match="RandomBrightnessContrast after HueSaturationValue"):
        D.translate_pipeline(swapped)


def test_get_dataset_translates_pipeline_and_explicit_keys_win(tmp_path):
    from PIL import Image
    (tmp_path / "a").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "a" / "0.png")
    base = dict(root=str(tmp_path), batch_size=1, device_pipeline=True, device="cpu")
    dl = D.get_dataset(base, _singletask_pipeline())
    assert dl.size == 128 and dl.hflip_p == 0.5 and dl.aug == D.normalise_aug_spec(SINGLETASK)
    dl = D.get_dataset(dict(base, size=64, coarse_dropout=None, hue_saturation_value=dict(hue_shift_limit=5, p=1.0)),
                       _singletask_pipeline())
    assert dl.size == 64 and "coarse_dropout" not in dl.aug and dl.aug["hue_saturation_value"]["hue_shift_limit"] == (-5, 5)
    assert dl.aug["brightness_contrast"] == D.normalise_aug_spec(SINGLETASK)["brightness_contrast"]
    dl = D.get_dataset(dict(base, **SINGLETASK))
    assert dl.aug == D.normalise_aug_spec(SINGLETASK) and dl.hflip_p == 0.0
    assert D.get_dataset(base).aug is None


def test_sample_config_expresses_the_reference_stack(tmp_path):
    import runpy
    from pathlib import Path
    from PIL import Image
    cfg = runpy.run_path(str(Path(__file__).resolve().parents[1] / "nkb-classification_amd" / "configs" / "folder_device_pipeline_config.py"))
    (tmp_path / "a").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "a" / "0.png")
    dl = D.get_dataset(dict(cfg["train_data"], root=str(tmp_path), device="cpu", num_workers=0), cfg["train_pipeline"])
    assert dl.aug == D.normalise_aug_spec(SINGLETASK) and dl.size == 128 and (dl.hflip_p, dl.vflip_p, dl.fill) == (0.5, 0.5, 0.0)
    assert dl.mean == MEAN and dl.std == STD
    assert D.get_dataset(dict(cfg["val_data"], root=str(tmp_path), device="cpu", num_workers=0), cfg["val_pipeline"]).aug is None


@pytest.mark.parametrize("B", [1, 6, 16, 17])
def test_pack_image_aug_layout(B):
    flags = (torch.arange(B) % 8).to(torch.uint8)
    rec = torch.arange(B * 64, dtype=torch.int32).reshape(B, 64) * 65537 - 5
    buf = hip.pack_image_aug(flags, rec)
    off = (B + 15) // 16 * 16
    assert buf.dtype == torch.uint8 and buf.numel() == off + 256 * B == hip.image_aug_bytes(B)
    assert off % 16 == 0 and buf.data_ptr() % 16 == 0
    assert torch.equal(buf[:B], flags) and not buf[B:off].any()
    assert np.array_equal(buf[off:].numpy().view("<i4").reshape(B, 64), rec.numpy())
    for b in (0, B - 1):
        assert np.array_equal(buf[off + 256 * b:off + 256 * (b + 1)].numpy().view("<i4"), rec[b].numpy())
    with pytest.raises(RuntimeError, match="pack_image_aug"):
        hip.pack_image_aug(flags, rec[:, :63])
