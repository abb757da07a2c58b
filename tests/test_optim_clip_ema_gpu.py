"""nkb_optim_step's clip forms (kind | NKB_OPTIM_CLIP_NORM, kind | NKB_OPTIM_CLIP_VALUE) and its EMA form (kind NKB_OPTIM_EMA) on
the GPU, bit for bit.

Clip forms: the expected coefficient is computed in numpy fp32 in the order nkbhip.h specifies (thread t of 256 adds partials
t, t + 256, .. in rising order, the wave's xor butterfly, the four wave sums in wave order, sqrtf, one multiplication, one
addition, one division); the expected update is the PLAIN launch (the kernel the float64 tests of tests/test_loss_optim_gpu.py
already pin) with grad_scale = 1 on gradients pre-multiplied in fp32, fl(fl(g * gs) * coef), respectively clamped by torch.clamp.
Every operand is compared whole, guard words included, with equal bits or a NaN on both sides.  That is exact because
+ - * / and sqrtf round once in this build (tests/loss_optim_reference.py relies on the same).

EMA form: numpy fp32 (d * e) + (omd * w), three roundings; the shadow is torch's .to(bfloat16) of the result.

Shapes: n = 1 and 5 (tail only / one group and a tail), 1027 (one workgroup, single group in flight, n % 4 = 3) and
2 * 256 * 8 + 3 (two workgroups, two groups in flight, tail), each starting on a 16-byte boundary (vector kernel) and 4 bytes
past one (one-element-per-thread kernel)."""
import functools

import numpy as np
import pytest
import torch

from nkb_classification import hip
from nkb_classification.utils import _step_scalars

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, WD = 1e-2, 0.05
GUARD = 4
SENTINEL = -7.0
NS = [1, 5, 1027, 2 * 256 * 8 + 3]
OFFSETS = [0, 1]
f32 = np.float32

# name -> (kind for _step_scalars, its keyword arguments, beta1 handed to the kernel)
KINDS = {
    "adam": ("adam", {}, 0.9), "adamw": ("adamw", {}, 0.9), "nadam": ("nadam", {}, 0.9), "radam": ("radam", {}, 0.9),
    "sgd": ("sgd", {}, 0.9), "sgd_momentum": ("sgd", dict(momentum=0.9), 0.9),
    "sgd_nesterov": ("sgd", dict(momentum=0.9, nesterov=True), 0.9),
}


def _guarded(values: torch.Tensor, offset: int):
    """(whole buffer, view holding `values` that starts `offset` elements past a 16-byte boundary), sentinels around the view"""
    n = values.numel()
    whole = torch.full((n + 2 * GUARD + 4,), SENTINEL, device=DEV, dtype=values.dtype)
    view = whole[GUARD + offset:GUARD + offset + n]
    view.copy_(values)
    return whole, view


def _guards_intact(whole, n, offset):
    lo = GUARD + offset
    return bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all())


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal bits, or a NaN on both sides"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return bool(((a.view(it) == b.view(it)) | (torch.isnan(a) & torch.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def _operands(n):
    """host operands of one launch, read-only: parameters, gradients, first and second moment"""
    gen = torch.Generator().manual_seed(100 + n)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1,
            torch.rand(n, generator=gen) * 0.1)


@functools.lru_cache(maxsize=None)
def _partials(P, with_inf):
    gen = np.random.default_rng(P)
    part = (gen.random(P, dtype=f32) * f32(3.0) + f32(1.0)).astype(f32)       # every partial >= 1: the norm is >= 0.5 at gs = 0.5
    if with_inf:
        part[(2 * P) // 3] = f32(np.inf)
    part.setflags(write=False)
    return part


def expected_coef(partials: np.ndarray, max_norm: float, grad_scale: float) -> np.float32:
    """nkbhip.h's order, one fp32 rounding per operation"""
    with np.errstate(all="ignore"):
        t = np.zeros(256, dtype=f32)
        for lo in range(0, len(partials), 256):            # thread t adds partials t, t + 256, .. in rising order
            row = partials[lo:lo + 256]
            t[:len(row)] = t[:len(row)] + row
        w = t.reshape(4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):                     # the wave's xor butterfly
            w = w + w[:, lane ^ o]
        s = w[:, 0]
        total = f32(f32(f32(s[0] + s[1]) + s[2]) + s[3])
        norm = f32(np.sqrt(total) * f32(abs(grad_scale)))
        coef = f32(f32(max_norm) / f32(norm + f32(1e-6)))
        return f32(1.0) if coef >= f32(1.0) else coef


def _record(bound, partials=None, skip=0.0):
    P = 0 if partials is None else len(partials)
    rec = np.zeros(4 + P, dtype=f32)
    rec[0], rec[1], rec[2] = skip, bound, P
    if P:
        rec[4:] = partials
    return torch.from_numpy(rec).to(DEV)


class _Launch:
    """one set of guarded device operands and a launch over them"""

    def __init__(self, name, n, offset, grad=None):
        kind, kw, beta1 = KINDS[name]
        self.sgd = kind == "sgd"
        self.n, self.offset, self.beta1 = n, offset, beta1
        p, g, m, v = _operands(n)
        self.whole, self.view = {}, {}
        for key, val in (("p", p), ("g", g if grad is None else grad), ("m", m), ("v", v), ("shadow", torch.zeros(n, dtype=torch.bfloat16))):
            self.whole[key], self.view[key] = _guarded(val.to(DEV), offset)
        self.code, self.sc = _step_scalars(kind, {"step": 7, "momentum_buffer": True}, lr=LR, beta1=beta1, beta2=0.999, eps=1e-8, **kw)

    def run(self, bits=0, grad_scale=1.0, rec=None):
        x = self.view
        hip.optim_step(self.code | bits, x["p"], x["g"], x["m"], None if self.sgd else x["v"], x["shadow"], self.n, LR, WD, self.beta1,
                       0.999, 1e-8, grad_scale, *self.sc, skip_flag=rec)
        torch.cuda.synchronize()
        return self

    def assert_same(self, other, what):
        for key in ("p", "m", "v", "shadow"):
            assert _same(self.whole[key], other.whole[key]), (what, key)
            assert _guards_intact(self.whole[key], self.n, self.offset), (what, key, "guard")
        assert _guards_intact(self.whole["g"], self.n, self.offset), (what, "g", "guard")


# (label, max_norm, an inf among the partials)
NORM_CASES = [("below", 1e6, False), ("above", 0.37, False), ("inf_partial", 0.37, True), ("nan_coef", float("inf"), True)]


@pytest.mark.parametrize("P", [1, 3, 256, 257, 4096])
@pytest.mark.parametrize("name", list(KINDS))
def test_clip_norm_equals_plain_launch_on_scaled_gradients(name, P):
    for label, max_norm, with_inf in NORM_CASES:
        part = _partials(P, with_inf)
        for gs in (1.0, 0.5):
            coef = expected_coef(part, max_norm, gs)
            if label == "below":
                assert coef == 1.0
            elif label == "above":
                assert 0.0 < coef < 1.0
            elif label == "inf_partial":
                assert coef == 0.0
            else:
                assert np.isnan(coef)
            rec = _record(max_norm, part)
            rec_before = rec.clone()
            for n in NS:
                g = _operands(n)[1]
                with np.errstate(all="ignore"):
                    scaled = torch.from_numpy(((g.numpy() * f32(gs)).astype(f32) * coef).astype(f32))
                for offset in OFFSETS:
                    what = (name, P, label, gs, n, offset)
                    got = _Launch(name, n, offset).run(hip.OPTIM_CLIP_NORM, gs, rec)
                    want = _Launch(name, n, offset, grad=scaled).run()
                    got.assert_same(want, what)
                    if label == "below":            # coef >= 1: exactly the unclipped launch's bits
                        got.assert_same(_Launch(name, n, offset).run(0, gs), what + ("unclipped",))
                    assert torch.equal(got.view["g"], g.to(DEV)), what         # the gradient itself is never scaled in place
            assert torch.equal(rec.view(torch.int32), rec_before.view(torch.int32))       # the record is read-only


def test_clip_norm_partial_count_is_capped_at_4096():
    """rec[2] above 4096 reads min(P, 4096) partials: the words behind them (here huge) never enter the sum"""
    part = _partials(4096, False)
    rec = torch.cat([_record(0.37, part), torch.full((64,), 1e30, device=DEV)])
    rec[2] = 5000.0
    coef = expected_coef(part, 0.37, 1.0)
    n = NS[-1]
    g = _operands(n)[1]
    scaled = torch.from_numpy((g.numpy() * coef).astype(f32))
    _Launch("adam", n, 0).run(hip.OPTIM_CLIP_NORM, 1.0, rec).assert_same(_Launch("adam", n, 0, grad=scaled).run(), "capped")


@pytest.mark.parametrize("bits", [hip.OPTIM_CLIP_NORM, hip.OPTIM_CLIP_VALUE], ids=["norm", "value"])
@pytest.mark.parametrize("name", ["adamw", "sgd_nesterov", "sgd"])
def test_record_skip_word_writes_nothing(name, bits):
    for n in NS:
        for offset in OFFSETS:
            run = _Launch(name, n, offset)
            before = {k: w.clone() for k, w in run.whole.items()}
            run.run(bits, 1.0, _record(0.5, _partials(3, False), skip=1.0))
            for k, w in run.whole.items():
                assert torch.equal(w.view(torch.int16 if k == "shadow" else torch.int32),
                                   before[k].view(torch.int16 if k == "shadow" else torch.int32)), (name, n, offset, k)
            run.run(bits, 1.0, _record(0.5, _partials(3, False), skip=0.0))           # flag down: the same launch does move them
            assert not torch.equal(run.view["p"], before["p"][GUARD + offset:GUARD + offset + n])


@pytest.mark.parametrize("name", list(KINDS))
def test_clip_value_equals_plain_launch_on_clamped_gradients(name):
    for clip_value in (0.5, 0.0, 1e9):
        rec = _record(clip_value)                      # four words: the value form reads nothing behind rec[1]
        for gs in (1.0, 0.5):
            for n in NS:
                g = _operands(n)[1].clone()
                g[0] = float("nan")                    # a NaN stays NaN (torch.clamp keeps it too)
                if n > 4:
                    g[1], g[2], g[4] = float("inf"), float("-inf"), 0.5 / gs
                clamped = torch.clamp(g * gs, -clip_value, clip_value)
                assert bool(torch.isnan(clamped[0]))
                for offset in OFFSETS:
                    what = (name, clip_value, gs, n, offset)
                    got = _Launch(name, n, offset, grad=g).run(hip.OPTIM_CLIP_VALUE, gs, rec)
                    want = _Launch(name, n, offset, grad=clamped).run()
                    got.assert_same(want, what)
                    assert bool(torch.isnan(got.view["p"][0]))


@pytest.mark.parametrize("d", [0.0, 0.5, 0.9998, 1.0])
def test_ema_matches_numpy_fp32(d):
    d32, omd32 = f32(d), f32(1.0 - d)              # the host subtracts in double and rounds once
    for n in NS:
        gen = torch.Generator().manual_seed(7 + n)
        e0, w0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        want = torch.from_numpy(((d32 * e0.numpy()).astype(f32) + (omd32 * w0.numpy()).astype(f32)).astype(f32))
        for offset in OFFSETS:
            for with_shadow in (True, False):
                ew, e = _guarded(e0.to(DEV), offset)
                ww, w = _guarded(w0.to(DEV), offset)
                sw, sh = _guarded(torch.zeros(n, dtype=torch.bfloat16).to(DEV), offset)
                hip.ema_step(e, w, sh if with_shadow else None, n, d)
                torch.cuda.synchronize()
                what = (d, n, offset, with_shadow)
                assert torch.equal(e.cpu().view(torch.int32), want.view(torch.int32)), what
                assert torch.equal(w.cpu(), w0), what
                assert torch.equal(sh.cpu(), want.to(torch.bfloat16) if with_shadow else torch.zeros(n, dtype=torch.bfloat16)), what
                assert _guards_intact(ew, n, offset) and _guards_intact(ww, n, offset) and _guards_intact(sw, n, offset), what
    if d == 1.0:
        assert torch.equal(want, e0)
    if d == 0.0:
        assert torch.equal(want, w0)


def test_ema_skip_flag_and_ignored_arguments():
    n = NS[-1]
    e0, w0 = _operands(n)[0], _operands(n)[1]
    ew, e = _guarded(e0.to(DEV), 0)
    _, w = _guarded(w0.to(DEV), 0)
    hip.ema_step(e, w, None, n, 0.5, skip_flag=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), e0)
    # every float but beta1 / beta2 is ignored, and so are m and v
    hip.optim_step(hip.OPTIM_EMA, e, w, None, None, None, n, 123.0, 4.0, 0.5, 0.5, 7.0, 9.0, 1.0, 2.0, 3.0, 4.0,
                   skip_flag=torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), e0 * 0.5 + w0 * 0.5) and _guards_intact(ew, n, 0)


def test_clipped_step_and_partial_pass_are_bit_reproducible():
    total = 100_003                                           # 7 chunks of 16384 elements, the last one short and odd
    offs = hip.clip_chunk_offsets(total)
    P = len(offs) - 1
    assert P == 7
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(total, generator=gen)
    xd, od = x.to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV)
    recs = []
    for _ in range(2):
        rec = _record(0.37, np.zeros(P, dtype=f32))
        hip.segment_sumsq(xd, od, P, rec[4:])
        torch.cuda.synchronize()
        recs.append(rec)
    assert torch.equal(recs[0].view(torch.int32), recs[1].view(torch.int32))
    # any order of fp32 additions of once-rounded squares: (len + 3) * 2^-24 relative (tests/loss_optim_reference.py)
    exact = torch.stack([(x[a:b].double() ** 2).sum() for a, b in zip(offs, offs[1:])])
    err = (recs[0][4:].cpu().double() - exact).abs() / exact
    assert bool((err <= (16384 + 3) * 2.0 ** -24).all()), err
    runs = [_Launch("adamw", NS[-1], 0).run(hip.OPTIM_CLIP_NORM, 0.5, recs[0]) for _ in range(2)]
    runs[0].assert_same(runs[1], "twice")
    for key in ("p", "m", "v", "shadow"):
        it = torch.int16 if key == "shadow" else torch.int32
        assert torch.equal(runs[0].whole[key].view(it), runs[1].whole[key].view(it))
