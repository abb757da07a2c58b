"""Flag bit 3 of nkb_image_prep (Mixup / CutMix inside the prep launch; csrc/imgprep.hip, contract in include/nkbhip.h), bit for bit
against the blend / box rule of tests/mix_reference.py applied to
  (a) the same kernel's un-mixed output (the launch with bit 3 cleared in every flag byte), and
  (b) the numpy restatement of tests/image_aug_reference.py.
(b) is held bit for bit where that restatement is exact by construction: images without a record (R.plain), and records whose
arithmetic has no rounding — brightness/contrast with alpha 0.5 and an integer offset, and holes — so no tie band exists; the HSV
stage, whose parity is allowed one level inside a tie band by tests/test_image_aug_gpu.py, enters through (a) only.
Every output sits between guard zones that must survive and starts as NaN."""
import numpy as np
import pytest
import torch

import image_aug_reference as R
import mix_reference as M

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GUARD, SENT = 64, -12345.0
GARBAGE = np.full(64, 0x7F7F7F7F, np.int32)
# canvas, floats `out` starts behind a 16-byte boundary: 16-byte stores, element stores (Wo % 4 != 0), element stores (alignment)
GEOMETRIES = [pytest.param((8, 0), id="8-vec"), pytest.param((10, 0), id="10-elem"), pytest.param((32, 0), id="32-vec"),
              pytest.param((32, 1), id="32-off1")]


def _launch(src, sizes, flag_bytes, records, S, off, fill=114.0):
    B, Hs, Ws, _ = src.shape
    n = B * 3 * S * S
    buf = torch.full((GUARD + off + n + GUARD,), SENT, device=DEV)
    lo = GUARD + off
    buf[lo:lo + n] = float("nan")
    assert buf.data_ptr() % 16 == 0
    flags = torch.tensor(flag_bytes, dtype=torch.uint8)
    if records is not None:
        flags = hip.pack_image_aug(flags, torch.from_numpy(np.stack(records).astype(np.int32)))
    hip.image_prep(torch.from_numpy(src).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV) if sizes is not None else None,
                   flags.to(DEV), buf[lo:], B, Hs, Ws, S, S, MEAN, STD, fill)
    torch.cuda.synchronize()
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), "wrote outside the output"
    out = buf[lo:lo + n].cpu().numpy().reshape(B, 3, S, S)
    assert np.isfinite(out).all(), "output not written everywhere"
    return out


def _reference_plain(src, sizes, records, S, fill):
    """plain_of(k, fl) from the numpy restatement: exact for the records this file uses with it"""
    def plain_of(k, fl):
        h, w = sizes[k] if sizes is not None else src.shape[1:3]
        img = src[k, :h, :w]
        if fl & 4:
            return R.normalise(R.levels_of(img, S, S, fl, records[k], fill), MEAN, STD)
        return R.plain(img, S, S, fl & 3, MEAN, STD, fill)
    return plain_of


def _check(name, src, sizes, flag_bytes, records, S, off, exact_reference=True, fill=114.0):
    got = _launch(src, sizes, flag_bytes, records, S, off, fill)
    unmixed = _launch(src, sizes, [f & 7 for f in flag_bytes], records, S, off, fill)
    want_a = M.mix_images(lambda k, fl: unmixed[k], flag_bytes, records, S, S)
    assert np.array_equal(got.view(np.int32), want_a.view(np.int32)), f"{name}: differs from the rule on the kernel's own un-mixed output"
    if exact_reference:
        want_b = M.mix_images(_reference_plain(src, sizes, records, S, fill), flag_bytes, records, S, S)
        assert np.array_equal(got.view(np.int32), want_b.view(np.int32)), f"{name}: differs from the rule on the numpy restatement"
    return got, unmixed


def _images(rng, B, S, smaller=True):
    Hs, Ws = (S - 2, S - 1) if smaller else (S, S)
    sizes = [(Hs, Ws), (Hs - 3, Ws), (Hs, Ws - 4), (1, 1), (Hs - 1, Ws - 2)][:B]
    return rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8), sizes


def _rec(words=None, **kw):
    rec = R.make_record(**kw)
    if words is not None:
        rec[10:16] = words
    return rec


EXACT_BC = dict(alpha=0.5, offset=12.0)            # level * 0.5 + 12: no rounding in float32, so the restatement has no tie band


@pytest.mark.parametrize("with_sizes", [True, False], ids=["sizes", "nosizes"])
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_blend_and_box_over_a_permutation(geom, B, with_sizes):
    """every image mixed, blends and boxes alternating, partners a non-involutive permutation (b -> b + 2 mod B for B = 5; the
    swap for B = 2; itself, a no-op, for B = 1); flips and exact records spread so that image and partner differ in both"""
    S, off = geom
    src, sizes = _images(np.random.default_rng(B * 100 + S), B, S)
    perm = [(b + 2) % B for b in range(B)] if B > 2 else [B - 1 - b for b in range(B)]
    boxes = [(1, 2, S - 2, S - 1), (0, 0, S // 2, 5), (3, 1, 7, 7), (2, 3, 6, 6), (S - 3, S - 5, S, S)]
    records, flag_bytes = [], []
    for b in range(B):
        words = M.make_mix_words(perm[b], lam=(0.3, 0.75, 0.123456)[b % 3]) if b % 2 == 0 else M.make_mix_words(perm[b], box=boxes[b])
        has_rec = b % 3 == 1
        records.append(_rec(words, **(dict(EXACT_BC, holes=[(1, 1, 4, 6)], hole_fill=(9, 200, 30)) if has_rec else {})))
        flag_bytes.append(8 | (b % 4) | (4 if has_rec else 0))
    got, unmixed = _check(f"perm-S{S}-B{B}", src, sizes if with_sizes else None, flag_bytes, records, S, off)
    if B > 1:
        assert all(not np.array_equal(got[b], unmixed[b]) for b in range(B)), "an image left the kernel unmixed"
    else:
        assert np.array_equal(got, unmixed), "p == b is not a no-op"


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_flips_and_records_on_one_side_only(geom):
    """image 0 (plain) blends with partner 1 (both flips, record); image 1 is cut from 0; image 2 (flips, record) blends with the
    plain image 3; image 3 is cut from 2; the partners' own bit 3 is ignored (no chaining); image 4 is not mixed"""
    S, off = geom
    src, sizes = _images(np.random.default_rng(7 + S), 5, S)
    rec_kw = dict(EXACT_BC, holes=[(0, 0, 3, S)], hole_fill=(1, 2, 3))
    records = [_rec(M.make_mix_words(1, lam=0.4)), _rec(M.make_mix_words(0, box=(2, 1, S - 1, 6)), **rec_kw),
               _rec(M.make_mix_words(3, lam=0.9), **rec_kw), _rec(M.make_mix_words(2, box=(0, 3, 5, S))), _rec(**rec_kw)]
    flag_bytes = [8, 8 | 4 | 3, 8 | 4 | 3, 8, 4 | 1]
    got, unmixed = _check(f"sides-S{S}", src, sizes, flag_bytes, records, S, off)
    assert np.array_equal(got[4], unmixed[4])
    lam, oml = np.float32(0.4), np.float32(1.0) - np.float32(0.4)
    assert np.array_equal(got[0], lam * unmixed[0] + oml * unmixed[1]), "the partner's own mixing leaked in (chaining)"


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_hsv_records_through_the_kernels_own_output(geom):
    S, off = geom
    src, sizes = _images(np.random.default_rng(9 + S), 2, S)
    records = [_rec(M.make_mix_words(1, lam=0.6), alpha=0.8, offset=-17.3, hsv=(37.3, -20.5, 12.25)),
               _rec(M.make_mix_words(0, box=(1, 1, S - 1, S - 2)), hsv=(-5.5, 8.25, 41.0))]
    _check(f"hsv-S{S}", src, sizes, [8 | 4 | 1, 8 | 4 | 2], records, S, off, exact_reference=False)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_boxes(geom):
    """empty boxes (zero height, zero width, reversed), the full canvas, edges that cut a 4-pixel group on either side, a single
    pixel, and boxes that reach past the canvas (only comparisons touch them)"""
    S, off = geom
    boxes = [(3, 3, 3, 7), (2, 5, 6, 5), (6, 6, 2, 2), (0, 0, S, S), (1, 1, S - 1, 3), (0, 2, 4, 7), (2, 5, 3, 6), (-4, -3, 3, 2),
             (S - 2, S - 3, S + 9, S + 9)]
    B = len(boxes) + 1
    rng = np.random.default_rng(11 + S)
    src = rng.integers(0, 256, (B, S - 1, S, 3), dtype=np.uint8)
    records = [_rec(M.make_mix_words((b + 1) % B, box=boxes[b])) for b in range(B - 1)] + [_rec()]
    flag_bytes = [8 | (b % 4) for b in range(B - 1)] + [3]
    got, unmixed = _check(f"boxes-S{S}", src, None, flag_bytes, records, S, off)
    for b in range(3):
        assert np.array_equal(got[b], unmixed[b]), f"empty box {boxes[b]} changed the image"
    assert np.array_equal(got[3], unmixed[4]), "the full-canvas box is not the partner"
    assert (got[6] != unmixed[6]).any(axis=0).sum() <= 1, "the one-pixel box changed more than one pixel"


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_without_bit_3_nothing_changes(geom):
    """flag values 0..7 with garbage in words 10..15 (and whole garbage records behind clear bits 2 and 3): the bits of the launch
    whose words 10..15 are zero, and for the flags without a record the bits of the launch without any table"""
    S, off = geom
    src, sizes = _images(np.random.default_rng(13 + S), 5, S)
    rec_kw = dict(EXACT_BC, holes=[(2, 2, 5, 6)], hole_fill=(7, 8, 9))
    for flag_bytes in ([0, 1, 2, 3, 4], [5, 6, 7, 4, 0]):
        clean = [_rec(**rec_kw) if f & 4 else _rec() for f in flag_bytes]
        dirty = [np.where((np.arange(64) >= 10) & (np.arange(64) < 16), GARBAGE, r) if f & 4 else GARBAGE.copy()
                 for f, r in zip(flag_bytes, clean)]
        a = _launch(src, sizes, flag_bytes, clean, S, off)
        b = _launch(src, sizes, flag_bytes, dirty, S, off)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), flag_bytes
        want = M.mix_images(_reference_plain(src, sizes, clean, S, 114.0), flag_bytes, clean, S, S)
        assert np.array_equal(a.view(np.int32), want.view(np.int32)), flag_bytes
    bare = _launch(src, sizes, [0, 1, 2, 3, 0], None, S, off)
    tabled = _launch(src, sizes, [0, 1, 2, 3, 0], [GARBAGE] * 5, S, off)
    assert np.array_equal(bare.view(np.int32), tabled.view(np.int32))
