"""nkb_loss_forward with NKB_LOSS_MIXED (kinds 16 | 0 and 16 | 1) and nkb_loss_backward with bit 1 (csrc/loss.hip) against the float64
reference and the fp32 yardstick of tests/mix_reference.py: four rows to a block and its tail, the `j += 64` walk and its tail,
three leading dimensions, weights absent and present, smoothing 0 and 0.1, lam all 1, all 0, 0.5 and per-row random, y2 == y on
some rows, rows dropped through either label, an all-dropped batch, a label out of range, the three reductions and per-row grad_out.

Outputs sit inside guard zones of a finite sentinel that must survive and start as NaN; finite garbage lies behind every input and
in the pad columns of the logits; row_state is exactly hip.loss_mixed_state_bytes(B, C) long with a sentinel tail.  Every case runs
twice and must repeat bit for bit.  Every case prints "RATIO case output err= bound= ratio=" for its worst element (-rP).
tests/test_mix_cpu.py proves on the CPU that these checks reject subtly wrong kernels."""
import pytest
import torch

import loss_optim_reference as lo
import mix_reference as M
from test_transformer_ops_gpu import DEV, NAN, SENT, TAIL, Out, _flat, _input, _raw

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

INT_FILL, INT_SENT = -7, -8192


def _cpu(t):
    return t.double().cpu()


def _launch(c, d):
    B, C = c.B, c.C
    ld, ldp, ldd = C + c.pad[0], C + c.pad[1], C + c.pad[2]
    x = _input(d.x.to(DEV), c.pad[0])
    table = d.table.to(DEV).contiguous()
    w = _input(d.weight.to(DEV)) if c.weight else None
    o = {"argmax": Out(1, B, torch.int32, INT_FILL, INT_SENT), "probs": Out(B, C, torch.float32, pad=c.pad[1])}
    nbytes = hip.loss_mixed_state_bytes(B, C)
    assert nbytes == 32 * B + 4 * C
    nf = nbytes // 4
    rs = torch.full((nf + TAIL,), SENT, device=DEV)
    rs[:nf] = NAN
    o["row_state"] = (rs, nf)
    out2 = o["out2"] = _flat(2, torch.float32)
    hip.loss_forward(c.kind_arg, x, ld, table, B, C, w, c.gamma_arg, M.ignore_value(c), o["probs"].view, ldp, o["argmax"].view, rs,
                     out2.view, c.reduction)
    o["dlogits"] = Out(B, C, torch.float32, pad=c.pad[2])
    hip.loss_backward(o["probs"].view, ldp, table, rs, out2.view, _input(d.gout.to(DEV)), B, C, o["dlogits"].view, ldd,
                      per_row=int(c.per_row) | 2)
    rec = rs[:8 * B].reshape(B, 8)
    ints = rec[:, 5:].contiguous().view(torch.int32)
    got = dict(argmax=_cpu(o["argmax"].data[0]), probs=_cpu(o["probs"].data), dlogits=_cpu(o["dlogits"].data),
               loss_rows=_cpu(rec[:, 0]), wsum=_cpu(rec[:, 1]), A=_cpu(rec[:, 2]), c1=_cpu(rec[:, 3]), c2=_cpu(rec[:, 4]),
               sm=_cpu(ints[:, 0]), pad=_cpu(ints[:, 1:].reshape(-1)), ew=_cpu(rs[8 * B:nf]), out0=_cpu(out2.data[:1]),
               out1=_cpu(out2.data[1:]))
    return o, got


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_mixed_loss_against_float64_reference(case):
    c = case
    d = M.make(c, seed=11)
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
    bad = []
    for name, (ratio, err, bound) in M.verdict(c, d, M.outputs(c, d, exact=True), got, M.outputs(c, d, exact=False)).items():
        print(f"RATIO {c.name} {name} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
        if not ratio <= 1.0:
            bad.append(f"{name}: error {err:.3e} > bound {bound:.3e}")
    assert not bad, f"{c.name}: {bad}"
    if c.ignored == "all":
        assert float(got["out0"]) == 0.0 and (float(got["out1"]) == 0.0 or c.reduction != 0) and not bool(got["dlogits"].any())
    if c.bad != "none":
        r = 0 if c.B < 3 else 2
        assert bool(torch.isnan(got["out0"]).all()) and bool(torch.isnan(got["dlogits"][r]).all())


def test_other_kinds_stay_refused():
    x, t = torch.zeros(2, 3, device=DEV), torch.zeros(3, 2, dtype=torch.int64, device=DEV)
    rs, o2 = torch.zeros(64, device=DEV), torch.zeros(2, device=DEV)
    for kind in (2, 3, -1, 16 | 2, 16 | 3, 32, 32 | 16):
        with pytest.raises(RuntimeError, match="kind"):
            hip.loss_forward(kind, x, 3, t, 2, 3, None, 0.0, -100, None, 3, None, rs, o2, 0)
    for eps in (1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="smoothing"):
            hip.loss_forward(16, x, 3, t, 2, 3, None, eps, -100, None, 3, None, rs, o2, 0)
    with pytest.raises(RuntimeError, match="grad_out_per_row"):
        hip.loss_backward(x, 3, t, rs, o2, o2, 2, 3, x.clone(), 3, per_row=4)
    assert hip.load().nkb_loss_row_state_bytes(5) == 60


@pytest.mark.parametrize("focal", [False, True])
def test_plain_kinds_unchanged_on_the_same_inputs(focal):
    """kind 0 / 1 on the inputs of a mixed case: still the 12-byte records and the bits of loss_optim_reference's yardstick
    checks; and the mixed form at lam = 1, y2 = y, eps = 0 gives the same loss and factor bits as the plain form, for unweighted
    cross entropy (coefficient 1) the same dlogits bits as well: g (1 p - 1) and (g 1) (p - 1) round alike"""
    mc = next(c for c in M.CASES if c.focal == focal and c.B == 5 and c.C == 65 and c.lam == "one" and c.eps == 0.0 and c.ignored == "none" and not c.weight)
    d = M.make(mc, 11)
    c = lo.Case(kind="loss", name="plain", B=mc.B, C=mc.C, focal=focal, pad=mc.pad, weight=mc.weight, gamma=mc.gamma, reduction=mc.reduction)
    pd = lo.make(c, 11)
    pd.x, pd.target, pd.weight, pd.gout = d.x, d.y, d.weight, d.gout
    import test_loss_optim_gpu as T
    _, got = T._launch(c, pd)
    torch.cuda.synchronize()
    bad = T._judge(c, pd, lo.outputs(c, pd, exact=True), got)
    assert not bad, bad
    d.y2 = d.y.clone()
    d.table = torch.stack([d.y, d.y2, d.lam.view(torch.int64)])
    _, mixed = _launch(mc, d)
    torch.cuda.synchronize()
    for name in ("out0", "out1", "probs", "argmax", "loss_rows", "wsum") + (() if focal else ("dlogits",)):
        assert torch.equal(mixed[name], got[name]), name
