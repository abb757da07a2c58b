"""CPU proof that tests/test_bn_pool_gpu.py can fail: the float64 reference of tests/bn_reference.py equals torch's batch_norm,
max_pool2d and adaptive_avg_pool2d and their autograd in float64 on every case below 2^21 elements (the larger ones are the same
formulas at another size), the fp32 yardstick sits inside every bound at every
case of the GPU table (also with its reductions accumulated in a second order), the share of recomputed-mask elements left out
stays within its cap, the reference of every exact case is representable in its output type, and every mutant of the yardstick is
rejected by the check of the output it corrupts."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as br

DEV = "cpu"
_CACHE = {}
SMALL = [c for c in br.CASES if not c.big]


def _setup(case):
    """(operands, reference, yardstick) of a case; small cases are computed once and left unchanged, large ones are not kept"""
    if case.name in _CACHE:
        return _CACHE[case.name]
    d = br.make(case, DEV, seed=7)
    r = (d, br.outputs(case, d, exact=True), br.outputs(case, d, exact=False))
    if not case.big:
        _CACHE[case.name] = r
    return r


def _close(a, b, tol=1e-11):
    a, b = a.double(), b.double()
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    scale = max(torch.nan_to_num(b).abs().max().item(), 1.0)
    return (torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max().item() <= tol * scale


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind in ("bwd", "fs", "apply") and c.rows > 1], ids=lambda c: c.name)
def test_batchnorm_reference_equals_torch_autograd_in_float64(case):
    """apply and backward composed are batch_norm (+ residual, ReLU) and its autograd once scale / shift / mean / invstd are the
    batch's own; the reference is evaluated with those statistics and compared with F.batch_norm in training mode"""
    c = case
    d = br.make(c, DEV, seed=3)
    x = d.x.double().clone().requires_grad_(True)
    gamma = (d.scale if c.kind == "apply" else d.gamma).double().clone().requires_grad_(True)
    beta = (d.shift if c.kind == "apply" else torch.full((c.C,), 0.25)).double().clone().requires_grad_(True)
    eps = 1e-5
    mean, var = x.detach().mean(0), x.detach().var(0, unbiased=False)
    invstd = (var + eps).rsqrt()
    y = F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)
    if c.kind == "apply":
        # the reference with scale = gamma invstd, shift = beta - mean scale is batch_norm (+ residual) (+ ReLU)
        d2 = br.make(c, DEV, seed=3)
        d2.scale, d2.shift = (gamma.detach() * invstd), (beta.detach() - mean * gamma.detach() * invstd)
        want = y.detach()
        if d.res is not None:
            q = d.res.double()
            if d.res_scale is not None:
                q = br.rnd(q * d.res_scale.double() + d.res_shift.double(), c.dtype)
            want = want + q
        want = want.clamp_min(0.0) if c.relu else want
        got = br.outputs(c, d2, exact=True)
        assert _close(got["y"], want)
        return
    # backward: with the batch's own statistics as the stored mean / invstd (kept in float64 here) the reference is the autograd
    # of F.batch_norm for the output gradient g' (dy under the case's mask)
    d.mean, d.invstd = mean, invstd
    if c.kind == "fs":      # the tile sums of this very g' and g' (x - mean), rows dealt to the tiles in turn (float64: the formula)
        t = torch.arange(c.rows) % c.tiles
        g64, x64 = d.dy.double(), d.x.double()
        d.stats = torch.stack([torch.zeros(c.tiles, c.C, dtype=torch.float64).index_add_(0, t, v) for v in (g64, g64 * (x64 - mean))], 1)
    ref = br.outputs(c, d, exact=True)
    (gx, gg, gb) = torch.autograd.grad(y, (x, gamma, beta), ref["g"])
    assert _close(ref["sums"][0], gb) and _close(ref["sums"][1], gg)
    assert _close(ref["dbeta"] - d.dbeta0.double(), gb, 1e-9) and _close(ref["dgamma"] - d.dgamma0.double(), gg, 1e-9)
    if c.dx:
        assert _close(ref["dx"], gx, 1e-10)
    if "dym" in ref:
        assert torch.equal(ref["dym"], ref["g"])


@pytest.mark.parametrize("case", [c for c in br.CASES if c.kind == "fin" and not c.big], ids=lambda c: c.name)
def test_finalize_reference_equals_torch_batch_norm_statistics(case):
    """x with exactly these per-tile sums is not available, so the identity is checked on data: partials of a random x give the
    statistics F.batch_norm computes (saved through its running-stat update) and its scale / shift reproduce its output"""
    c = case
    gen = torch.Generator().manual_seed(5)
    R = max(c.count // c.tiles, 1)
    x = torch.randn(c.tiles, R, c.C, generator=gen, dtype=torch.float64) * 1.5 + 0.3
    d = br.make(c, DEV, seed=3)
    d.partials = torch.stack([x.sum(1), (x * x).sum(1)], 1)          # float64 partials: the formulas, not the fp32 storage
    ref = br.outputs(c, d, exact=True)
    rm, rv = d.rm.double().clone(), d.rv.double().clone()
    flat = x.reshape(-1, c.C)
    if c.training and c.count > 1:
        y = F.batch_norm(flat, rm, rv, d.gamma.double(), d.beta.double(), training=True, momentum=d.momentum, eps=d.eps)
        assert _close(ref["running_mean"], rm, 1e-9) and _close(ref["running_var"], rv, 1e-9)
        assert _close(flat * ref["scale"] + ref["shift"], y, 1e-7)
    elif not c.training:
        y = F.batch_norm(flat, rm, rv, d.gamma.double(), d.beta.double(), training=False, eps=d.eps)
        assert _close(flat * ref["scale"] + ref["shift"], y, 1e-9)
        assert set(ref) == {"scale", "shift"}
    else:       # count == 1: the biased variance (0) enters the running statistic
        assert _close(ref["running_var"], (1 - d.momentum) * d.rv.double(), 1e-9)


@pytest.mark.parametrize("case", [c for c in br.CASES if c.kind in ("maxpool", "avgpool") and not c.big], ids=lambda c: c.name)
def test_pool_reference_equals_torch_autograd_in_float64(case):
    c = case
    d = br.make(c, DEV, seed=3)
    ref = br.outputs(c, d, exact=True)
    if c.kind == "maxpool":
        x = d.x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.max_pool2d(x, 3, 2, 1)
        assert torch.equal(torch.isnan(y), torch.isnan(ref["y"].permute(0, 3, 1, 2)))
        assert torch.equal(torch.nan_to_num(y.detach()), torch.nan_to_num(ref["y"].permute(0, 3, 1, 2)))
        (gx,) = torch.autograd.grad(y, x, d.g.double().permute(0, 3, 1, 2))
        if not c.fill.startswith("nan"):     # torch's backward of a NaN window is its own business; the slot rule is asserted below
            assert _close(ref["dx"], gx.permute(0, 2, 3, 1))
        _, ti = F.max_pool2d(d.x.double().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
        P, Q = ref["idx"].shape[1:3]
        hh = (2 * torch.arange(P) - 1)[None, :, None, None] + ref["idx"] // 3
        ww = (2 * torch.arange(Q) - 1)[None, None, :, None] + ref["idx"] % 3
        assert torch.equal((hh * c.W + ww).permute(0, 3, 1, 2), ti)
    else:
        x = d.x.double().reshape(c.N, c.H, 1, c.C).permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.adaptive_avg_pool2d(x, 1)
        assert _close(ref["y"], y.detach().reshape(c.N, c.C))
        (gx,) = torch.autograd.grad(y, x, d.g.double().reshape(c.N, c.C, 1, 1))
        assert _close(ref["dx"], gx.permute(0, 2, 3, 1).reshape(c.N, c.H, c.C))


@pytest.mark.parametrize("case", br.CASES, ids=lambda c: c.name)
def test_yardstick_is_inside_every_bound(case):
    d, ref, yard = _setup(case)
    for label, y in (("torch's order", yard), ("second order", br.outputs(case, d, exact=False, order="strided"))):
        v = br.verdict(case, d, ref, y)
        print(case.name, label, {k: f"{r:.3f}" for k, (r, _, _) in v.items()})
        assert all(r <= 1.0 for r, _, _ in v.values()), (label, v)
    share = br.mask_share(case, ref)
    assert share <= br.MASK_SHARE, f"{share:.2e} of the mask elements sit on the edge"
    if case.exact:
        assert share == 0.0
        assert br.representable(case, d, ref), "an exact case whose float64 reference is no number of its output type"


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_mutant_is_rejected_by_the_output_it_corrupts(mutant):
    """Every exact case at which the mutant changes the yardstick rejects it, and so does every random case for the mutants of a
    formula; the check that rejects belongs to an output br.REJECTED_BY names.  The large cases are left to one mutant."""
    hit = 0
    for case in br.CASES:
        if case.big and not (mutant == "drop_last_row" and case.kind == "bwd" and case.exact and case.mask == "bits"):
            continue
        if not br.mutant_applies(case, mutant):
            continue
        d, ref, yard = _setup(case)
        rej = br.rejecting(case, d, mutant, ref, yard)
        if rej is None:
            continue
        if not (case.exact or mutant in br.FORMULA_MUTANTS):
            continue
        hit += 1
        assert any(k in br.REJECTED_BY[mutant] for k in rej), f"{case.name}: {mutant} is not rejected by {br.REJECTED_BY[mutant]} (rejected by: {rej})"
    assert hit >= 1, f"{mutant} exists at no case"


def test_table_covers_what_the_kernels_dispatch_on():
    names = {c.name for c in br.CASES}
    assert len(names) == len(br.CASES)
    assert br.BWD_FORMS == {(a, b) for a in (True, False) for b in ("none", "sep", "inplace")}
    blocks = {br.bwd_geometry(c.rows, c.C, c.dtype)[3] for c in br.CASES if c.kind == "bwd"}
    assert {1, 63, 64, 193, 256, 257, 512} <= blocks
    assert any(br.bwd_geometry(c.rows, c.C, c.dtype)[1] > 256 for c in br.CASES if c.kind == "bwd")
    assert any((c.C + 63) // 64 > 32 and c.tiles > 128 for c in br.CASES if c.kind in ("fin", "fs"))
    for c in br.CASES:
        if c.exact and c.kind in ("bwd", "fs"):
            assert c.rows * 3 * 10 * 2 < 2 ** 24


def test_sizing_rules_match_the_library():
    """the host-side sizing the table relies on is the library's (these entry points launch nothing)"""
    from nkb_classification import hip
    for rows, C in ((1, 64), (144, 64), (9729, 2048), (196613, 64), (53, 4096)):
        assert br.bwd_ws_floats(rows, C) == hip.bn_backward_ws(rows, C)
        for dt in ("bf16", "f32"):
            blocks = br.bwd_geometry(rows, C, dt)[3]
            assert blocks * 2 * C + 2 * C <= br.bwd_ws_floats(rows, C)
    for tiles, C in ((1, 64), (128, 72), (129, 64), (129, 2112), (392, 4096), (1568, 256)):
        assert br.stats_floats(tiles, C) == hip.bn_stats_floats(tiles, C)
