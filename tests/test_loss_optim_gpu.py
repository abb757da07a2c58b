"""nkb_loss_forward / nkb_loss_backward (csrc/loss.hip), nkb_optim_step, nkb_grad_unscale_check, nkb_scaler_update,
nkb_bucket_sum_bf16, nkb_segment_sumsq (csrc/optim.hip) and nkb_image_prep (csrc/imgprep.hip) against the float64 reference and the
fp32 yardstick of tests/loss_optim_reference.py, at the smallest shapes at which each path can go wrong: the `j += 64` walk of the
loss rows and its tail, four rows to a block, the second trips of the 256-thread reduce and of the capped backward grid, three
different leading dimensions, every optimizer variant on the vector and the scalar kernel past their grid caps, with and without
the second in-flight group, the 16-byte stores of image_prep next to its element stores with `out` off its 16-byte boundary.

Outputs sit inside guard zones of a finite sentinel that must survive; output regions start as NaN (for the optimizer's in-place
operands the guard zones sit around the range); finite garbage lies behind every input and in the pad columns of the logits;
row_state is exactly nkb_loss_row_state_bytes(B) long with a sentinel tail.  Every case runs twice and must repeat bit for bit (none
of these kernels accumulates with atomics).  Every case prints "RATIO kernel case output err= bound= ratio=" for its worst element
(visible with -rP).  tests/test_loss_optim_reference.py proves on the CPU that these checks reject subtly wrong kernels."""
import pytest
import torch

import loss_optim_reference as lo
from test_transformer_ops_gpu import DEV, GF, NAN, SENT, TAIL, Out, _flat, _input, _raw

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

KERNEL = dict(loss="nkb_loss", optim="nkb_optim_step", unscale="nkb_grad_unscale_check", scaler="nkb_scaler_update",
              bucket="nkb_bucket_sum_bf16", segsq="nkb_segment_sumsq", prep="nkb_image_prep")
INT_FILL, INT_SENT = -7, -8192


class Range:
    """n elements starting `off` elements behind an aligned boundary, between guard zones of the sentinel"""

    def __init__(self, n, dtype, fill=NAN, off=0, sent=SENT):
        self.n, self.lo = n, GF + off
        self.guard = torch.full((1,), sent, device=DEV, dtype=dtype)
        self.buf = torch.full((GF + off + n + GF,), sent, device=DEV, dtype=dtype)
        self.buf[self.lo:self.lo + n] = fill.to(DEV) if isinstance(fill, torch.Tensor) else fill
        self.view = self.buf[self.lo:]
        self.data = self.buf[self.lo:self.lo + n]
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (off * self.buf.element_size()) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == self.guard).all()) and bool((self.buf[self.lo + self.n:] == self.guard).all())


def _cpu(t):
    return t.double().cpu()


def _loss_launch(c, d):
    B, C = c.B, c.C
    ld, ldp, ldd = C + c.pad[0], C + c.pad[1], C + c.pad[2]
    logger = c.form == "logger"
    x = _input(d.x.to(DEV), c.pad[0])
    tgt = None if logger else torch.cat([d.target, torch.full((8,), 12345)]).to(DEV)
    w = _input(d.weight.to(DEV)) if c.weight else None
    o = {"argmax": Out(1, B, torch.int32, INT_FILL, INT_SENT)}
    if c.form != "noprobs":
        o["probs"] = Out(B, C, torch.float32, pad=c.pad[1])
    rs = out2 = None
    if not logger:
        nbytes = hip.load().nkb_loss_row_state_bytes(B)
        assert nbytes == 12 * B
        rs = torch.full((3 * B + TAIL,), SENT, device=DEV)
        rs[:3 * B] = NAN
        o["row_state"] = (rs, 3 * B)
        out2 = o["out2"] = _flat(2, torch.float32)
    hip.loss_forward(int(c.focal), x, ld, tgt, B, C, w, c.gamma, lo.ignore_value(c), o["probs"].view if "probs" in o else None, ldp,
                     o["argmax"].view, rs, out2.view if out2 else None, c.reduction)
    got = {"argmax": _cpu(o["argmax"].data[0])}
    if "probs" in o:
        got["probs"] = _cpu(o["probs"].data)
    if not logger:
        if c.form == "train":
            o["dlogits"] = Out(B, C, torch.float32, pad=c.pad[2])
            hip.loss_backward(o["probs"].view, ldp, tgt, rs, out2.view, _input(d.gout.to(DEV)), B, C, o["dlogits"].view, ldd, per_row=c.per_row)
            got["dlogits"] = _cpu(o["dlogits"].data)
        rows = _cpu(rs[:3 * B]).reshape(B, 3)
        got.update(loss_rows=rows[:, 0], wsum=rows[:, 1], coef=rows[:, 2], out0=_cpu(out2.data[:1]), out1=_cpu(out2.data[1:]))
    return o, got


def _optim_launch(c, d):
    code, a = lo.step_scalars(c)
    o = {k: Range(c.n, torch.float32, getattr(d, k), c.offset) for k in ("w", "m", "v")}
    g = torch.cat([torch.full((GF + c.offset,), lo.GARBAGE), d.g, torch.full((GF,), lo.GARBAGE)]).to(DEV)[GF + c.offset:]
    assert g.data_ptr() % 16 == (4 * c.offset) % 16
    sh = None
    if c.shadow != "none":
        sh = o["shadow"] = Range(c.n, torch.bfloat16, NAN, 1 if c.shadow == "odd" else 0)
        assert sh.view.data_ptr() % 8 == (2 if c.shadow == "odd" else 0)
    skip = None if c.skip == "none" else _input(torch.tensor([float(c.skip)], device=DEV))
    hip.optim_step(code, o["w"].view, g, o["m"].view, o["v"].view, sh.view if sh else None, c.n, a["lr"], a["wd"], a["beta1"], a["beta2"],
                   a["eps"], a["gs"], a["c0"], a["c1"], a["c2"], a["c3"], skip_flag=skip)
    return o, {k: _cpu(v.data) for k, v in o.items()}


def _other_launch(c, d):
    f32 = torch.float32
    if c.kind == "unscale":
        o = {"g": Range(c.n, f32, d.g), "found": _flat(1, f32, c.found0)}
        hip.grad_unscale_check(o["g"].view, c.n, _input(torch.tensor([c.scale], device=DEV)), o["found"].view)
    elif c.kind == "scaler":
        found, tracker, interval, scale = c.scaler
        o = {"scale": _flat(1, f32, scale), "tracker": Out(1, 1, torch.int32, tracker, INT_SENT), "found": _flat(1, f32, found), "last": _flat(1, f32)}
        hip.scaler_update(o["scale"].view, o["tracker"].view, o["found"].view, o["last"].view, 2.0, 0.5, interval)
        return o, {k: _cpu(v.data.reshape(-1)) for k, v in o.items()}
    elif c.kind == "bucket":
        parts = _input(d.parts.reshape(-1).to(DEV))
        o = {}
        if c.form3 != "bf16":
            o["out"] = Range(c.n, f32)
        if c.form3 != "f32":
            o["out16"] = Range(c.n, torch.bfloat16)
        hip.bucket_sum_bf16(parts, d.stride, c.nparts, o["out"].view if "out" in o else None, o["out16"].view if "out16" in o else None, c.n)
    elif c.kind == "segsq":
        nseg = len(c.lengths)
        o = {"out": _flat(nseg, f32)}
        hip.segment_sumsq(_input(d.x.to(DEV)), d.offsets.to(DEV), nseg, o["out"].view)
    else:
        Bn, Hs, Ws, Ho, Wo = c.img
        o = {"out": Range(Bn * 3 * Ho * Wo, f32, NAN, c.out_offset)}
        src = torch.cat([d.src.reshape(-1), torch.full((64,), 200, dtype=torch.uint8)]).to(DEV)
        hip.image_prep(src, d.sizes.to(DEV) if d.sizes is not None else None, d.flags.to(DEV) if d.flags is not None else None, o["out"].view,
                       Bn, Hs, Ws, Ho, Wo, d.mean, d.std, c.fillv)
        return o, {"out": _cpu(o["out"].data).reshape(Bn, 3, Ho, Wo)}
    return o, {k: _cpu(v.data) for k, v in o.items()}


def _launch(c, d):
    return _loss_launch(c, d) if c.kind == "loss" else _optim_launch(c, d) if c.kind == "optim" else _other_launch(c, d)


def _judge(c, d, ref, got, yard=None):
    bad = []
    for name, (ratio, err, bound) in lo.verdict(c, d, ref, got, yard).items():
        print(f"RATIO {KERNEL[c.kind]} {c.name} {name} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
        if not ratio <= 1.0:
            bad.append(f"{name}: error {err:.3e} > bound {bound:.3e}")
    return bad


@pytest.mark.parametrize("case", lo.CASES, ids=lambda c: c.name)
def test_kernel_against_float64_reference(case):
    c = case
    d = lo.make(c, seed=11)
    runs = []
    for _ in range(2):
        runs.append(_launch(c, d))
        torch.cuda.synchronize()
    (a, got), (b, _) = runs
    for name, v in a.items():
        x, y = (v.buf, b[name].buf) if not isinstance(v, tuple) else (v[0], b[name][0])
        assert torch.equal(_raw(x), _raw(y)), f"{c.name}: {name} differs between two launches"
    for name, v in a.items():
        if isinstance(v, tuple):
            assert bool((v[0][v[1]:] == SENT).all()), f"{c.name}: {name} written past its {v[1]} advertised floats"
        else:
            assert v.intact(), f"{c.name}: {name} wrote outside its region"
    if c.kind in lo.BIT_EXACT:        # the yardstick is the target; the CPU file ties it to the float64 reference
        bad = _judge(c, d, {}, got, lo.outputs(c, d, exact=False))
    else:
        bad = _judge(c, d, lo.outputs(c, d, exact=True), got)
    assert set(got) and not bad, f"{c.name}: {bad}"


def _smallest_allowance(q, err, which):
    """per element, the smallest A at which lo.focal_terms(q, A)[which] covers err (inf where none below 2^20 does)"""
    low, high = torch.zeros_like(err), torch.full_like(err, 2.0 ** 20)
    fits = lambda A: err <= lo.focal_terms(q, A)[which] + lo.TINY["f32"]
    none = ~fits(high)
    for _ in range(48):
        mid = 0.5 * (low + high)
        ok = fits(mid)
        high, low = torch.where(ok, mid, high), torch.where(ok, low, mid)
    return torch.where(none, torch.full_like(err, lo.INF), torch.where(fits(torch.zeros_like(err)), torch.zeros_like(err), high))


def test_library_function_error():
    """The basis of A_LOG and A_POW (loss_optim_reference's docstring).  logf: rows of k zeros and -inf elsewhere, label 0, so
    se == k exactly and the stored row loss is logf(k) itself, k = 1..2048: the error in ulps of |log k|.  powf: focal rows (0, a),
    a on a grid of 2^15 points in [-88, 0], labels alternating, gamma in {0.5, 1, 2, 5}: the smallest allowance at which the derived
    bound of loss_r (powf at gamma) and of coef_r (powf at gamma - 1) holds.  Each allowance is at least twice the measured worst."""
    c = lo.Case("loss", "measure-logf", B=2048, C=2048, form="noprobs", fill="ksame")
    d = lo.make(c, seed=11)
    _, got = _loss_launch(c, d)
    torch.cuda.synchronize()
    want = torch.log(torch.arange(1, 2049, dtype=torch.float64))
    log_err = ((got["loss_rows"] - want).abs() / lo.ulp32(want)).max().item()
    assert bool((got["wsum"] == 1).all()) and got["loss_rows"][0].item() == 0.0
    a_log, keep = lo.allowance(log_err), lo.A_LOG
    worst = dict(pow=0.0, pow_m1=0.0)
    try:
        lo.A_LOG = a_log                    # the bound of log p_y inside the focal terms uses the allowance just measured
        for gamma in lo.GAMMAS[1:]:
            c = lo.Case("loss", f"measure-powf-{gamma}", B=1 << 15, C=2, focal=True, gamma=gamma, form="noprobs", fill="grid", reduction=1)
            d = lo.make(c, seed=11)
            _, got = _loss_launch(c, d)
            torch.cuda.synchronize()
            ref = lo.outputs(c, d, exact=True)
            for key, out, which in (("pow", "loss_rows", 0), ("pow_m1", "coef", 1)):
                A = _smallest_allowance(ref["focal_q"], (got[out] - ref[out]).abs(), which)
                print(f"MEASURED gamma={gamma} {key}={A.max().item():.3f} (row {int(A.argmax())})")
                worst[key] = max(worst[key], A.max().item())
    finally:
        lo.A_LOG = keep
    print(f"MEASURED log={log_err:.3f} pow={worst['pow']:.3f} pow_m1={worst['pow_m1']:.3f} -> A_LOG={a_log:g} A_POW={lo.allowance(worst['pow'], worst['pow_m1']):g}")
    assert 2 * log_err <= lo.A_LOG and 2 * max(worst.values()) <= lo.A_POW, "measure, then record the values in MEASURED"


def test_zero_extents_and_refusals():
    """B == 0 / C == 0 / nseg == 0 return before the launch (an empty grid is a launch error) and write nothing; negative extents,
    a kind outside {0, 1}, a reduction outside 0..2 and row_state without target are refused; so is every bad call of bucket_sum_bf16"""
    keep = torch.full((64,), 3.0, device=DEV)
    out = keep.clone()
    y = torch.zeros(8, dtype=torch.int64, device=DEV)
    am = torch.full((8,), INT_FILL, dtype=torch.int32, device=DEV)
    hip.loss_forward(0, keep, 8, y, 0, 8, None, 0.0, -100, out, 8, am, out, out)
    hip.loss_forward(0, keep, 8, y, 4, 0, None, 0.0, -100, out, 8, am, out, out)
    hip.loss_backward(keep, 8, y, keep, keep, keep, 0, 8, out, 8)
    hip.loss_backward(keep, 8, y, keep, keep, keep, 4, 0, out, 8)
    hip.segment_sumsq(keep, y, 0, out)
    hip.bucket_sum_bf16(keep, 8, 1, out, None, 0)
    hip.grad_unscale_check(out, 0, keep, out)
    hip.optim_step(0, out, keep, out, out, None, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(out, keep) and bool((am == INT_FILL).all())
    p16 = keep.to(torch.bfloat16)
    calls = (("negative extent", lambda: hip.loss_forward(0, keep, 8, y, -1, 8, None, 0.0, -100, out, 8, am, out, out)),
             ("negative extent", lambda: hip.loss_forward(0, keep, 8, y, 4, -1, None, 0.0, -100, out, 8, am, out, out)),
             ("negative extent", lambda: hip.loss_backward(keep, 8, y, keep, keep, keep, -1, 8, out, 8)),
             ("kind 2", lambda: hip.loss_forward(2, keep, 8, y, 4, 8, None, 0.0, -100, out, 8, am, out, out)),
             ("kind -1", lambda: hip.loss_forward(-1, keep, 8, y, 4, 8, None, 0.0, -100, out, 8, am, out, out)),
             ("reduction 3", lambda: hip.loss_forward(0, keep, 8, y, 4, 8, None, 0.0, -100, out, 8, am, out, out, 3)),
             ("row_state needs target", lambda: hip.loss_forward(0, keep, 8, None, 4, 8, None, 0.0, -100, out, 8, am, out, out)),
             ("negative segment count", lambda: hip.segment_sumsq(keep, y, -1, out)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16, 8, 0, out, None, 8)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16, 8, 1, None, None, 8)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16, 12, 2, out, None, 8)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16[1:], 8, 1, out, None, 8)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16, 8, 1, out[1:], None, 8)),
             ("bucket_sum_bf16", lambda: hip.bucket_sum_bf16(p16, 8, 1, None, p16[1:], 8)),
             ("16-byte aligned", lambda: hip.grad_unscale_check(out[1:], 8, keep, out)),
             ("kind 4", lambda: hip.optim_step(4, out, keep, out, out, None, 8, 1e-3, 0.0, 0.9, 0.999, 1e-8, 1.0)))
    for what, call in calls:
        with pytest.raises(RuntimeError, match=what):
            call()
    torch.cuda.synchronize()
    assert torch.equal(out, keep) and bool((am == INT_FILL).all())
