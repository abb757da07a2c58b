"""CPU proof that tests/test_wgrad_gpu.py can fail: the float64 reference of tests/wgrad_reference.py equals torch's weight gradient
(torch.nn.grad.conv2d_weight in float64) on every convolution-shaped case — the packed stem after folding its chunk view back to
7 x 7 taps — and a plain einsum on the GEMM-shaped and batched ones; the reference rounded the way the kernels round sits inside
the positive-regime bound and equals the reference bit for bit in the exact regime; every mutant is rejected by the regime and
check REJECTED_BY names, in every kernel family where it exists; and the host-only queries answer without a GPU."""
import pytest
import torch

import conv_reference as cr
import wgrad_reference as wr

DEV = "cpu"
CPU_CUS = 136           # a chip of 136 CUs: with 128 reserved the wide wgradr form starts at 2017 rows (the proof's size of that case)
ALL = tuple(wr.resolve(c, CPU_CUS) for c in wr.CASES + wr.PROBE_CASES)
BIG_MUTANTS = ("drop_pixel", "acc_bf16", "bias_not_reduced")        # what the large cases (1024 x 1024 channels) are left
_CACHE = {}


def _plan(c):
    return wr.plan(c, CPU_CUS if c.wide_m else 256)


def _data(c, regime):
    if (c.name, regime) not in _CACHE:
        _CACHE[c.name, regime] = wr.make(c, DEV, regime, seed=7)
    return _CACHE[c.name, regime]


def _form(c, mutant=None):
    return "direct" if c.entry == "tn" else "assign" if mutant == "assign_accumulates" else "slab"


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_reference_equals_torch_in_float64(case):
    c = case
    d = wr.make(c, DEV, "positive", seed=3)
    g = wr.geom(c)
    form = _form(c)
    got = wr.reference(c, replace_pre(d), form, pl=_plan(c)) if form != "direct" else None
    if c.entry == "tn":
        out = wr.totals(c, d, "direct")[0].reshape(-1, c.Cout, c.Cin)
        want = torch.einsum("zma,zmb->zab", d.dy.double(), d.x.double())
        assert (out - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        return
    dw = got["dw"]
    if c.R == 1 and c.S == 1 and c.stride == 1 and c.entry == "conv":
        want = torch.einsum("ma,mb->ab", d.dy.double(), d.x.double())
    elif c.entry == "conv":
        x = d.x.double().reshape(c.N, c.H, c.W, c.Cin).permute(0, 3, 1, 2)
        dy = d.dy.double().reshape(c.N, g.P, g.Q, c.Cout).permute(0, 3, 1, 2)
        want = torch.nn.grad.conv2d_weight(x, (c.Cout, c.Cin, c.R, c.S), dy, stride=c.stride, padding=c.pad)
        want = want.permute(0, 2, 3, 1).reshape(c.Cout, -1)
    else:
        # the packed stem: xp[N][H][Wp][4] is an ordinary 4-channel image; fold dwp's (r, chunk, j) columns back to (r, tap, channel):
        # pixel offset inside the window = chunk * (EPC / 4) + j / 4, channel = j % 4, tap = offset - 1 (bf16: the window starts one
        # pixel early) or offset (fp32); the column of the tap outside 0 .. 6 holds a product too, and is compared with a 7 x 8 filter
        epc, Wp = g.Cin, (c.W + 1) // 2 * 2
        x = d.x.double().reshape(c.N, c.H, Wp, 4).permute(0, 3, 1, 2)
        dy = d.dy.double().reshape(c.N, g.P, g.Q, c.Cout).permute(0, 3, 1, 2)
        lead = 1 if c.dtype == "bf16" else 0                  # the 8-pixel window starts at image pixel 2q - 3 - lead
        xw = torch.nn.functional.pad(x, (3 + lead, 4 - lead, 3, 3))
        want = torch.nn.grad.conv2d_weight(xw, (c.Cout, 4, 7, 8), dy, stride=2, padding=0)        # [Cout][4][7][8 window pixels]
        want = want.permute(0, 2, 3, 1).reshape(c.Cout, -1)                                          # (r, window pixel, channel)
        assert g.S * epc == 32 and g.Ntot == 224
    assert dw.shape == want.shape
    assert (dw - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    if c.bias:
        assert (got["dbias"] - d.dy.double().sum(0)).abs().max().item() <= 1e-12 * g.M


def replace_pre(d):
    """the operands with empty previous contents: the product alone"""
    return wr.Data(d.x, d.dy, torch.zeros_like(d.pre_dw), None if d.pre_db is None else torch.zeros_like(d.pre_db))


def test_stem_view_folds_to_the_seven_taps():
    """the columns of dwp that nkb_stem_wfold keeps are torch's 7 x 7 stem weight gradient of the unpadded image"""
    for c in ALL:
        if c.entry != "stem":
            continue
        g = wr.geom(c)
        d = replace_pre(wr.make(c, DEV, "exact", seed=5))
        dwp = wr.reference(c, d, "slab")["dw"].reshape(c.Cout, 7, 8, 4)
        lead = 1 if c.dtype == "bf16" else 0
        Wp = (c.W + 1) // 2 * 2
        x = d.x.double().reshape(c.N, c.H, Wp, 4).permute(0, 3, 1, 2)
        dy = d.dy.double().reshape(c.N, g.P, g.Q, c.Cout).permute(0, 3, 1, 2)
        want = torch.nn.grad.conv2d_weight(x, (c.Cout, 4, 7, 7), dy, stride=2, padding=3).permute(0, 2, 3, 1)
        assert torch.equal(dwp[:, :, lead:lead + 7], want), c.name


@pytest.mark.parametrize("case", [c for c in ALL if c.entry == "conv"], ids=lambda c: c.name)
def test_general_gather_equals_conv_reference(case):
    a, b = wr.gather_general(case, DEV), cr.gather_index(wr._cr_case(case), DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_rounded_reference_is_inside_both_verdicts(case):
    c = case
    pl = _plan(c)
    for form in wr.forms(c):
        for regime in ("exact", "positive"):
            d = _data(c, regime)
            for order in ("split",) if c.big else ("split", "stage"):
                y = wr.reference(c, d, form, pl=pl, rounded=order)
                v = wr.verdict(c, d, regime, form, y, pl)
                print(c.name, form, regime, order, {k: f"{r:.3f}" for k, (r, _, _) in v.items()})
                assert all(r <= 1.0 for r, _, _ in v.values()), (form, regime, order, v)


@pytest.mark.parametrize("mutant", wr.MUTANTS)
def test_mutant_is_rejected_by_the_check_it_corrupts(mutant):
    """Every case at which the mutant exists rejects it by the regime and check REJECTED_BY names, and the mutant exists in at least
    one case of every kernel family that has the feature."""
    regime, check = wr.REJECTED_BY[mutant]
    hit = set()
    for c in ALL:
        if c.big and mutant not in BIG_MUTANTS:
            continue
        if mutant == "empty_split_garbage":
            continue                                   # (no plan leaves a split without rows: see the test below)
        if mutant == "acc_bf16" and wr.geom(c).M + _plan(c).splits + 2 >= 8192:
            # one bf16 rounding leaves up to 2^-9 of the accumulator; the worst-case bound A (K + S + c) 2^-24 passes 2^-10, half of
            # that, at K + S + c = 8192: beyond it (the 49-split cases of 12 325 rows) the bound cannot be counted on to see the mutant
            continue
        rej = wr.rejecting(c, _data(c, regime), regime, _form(c, mutant), mutant, _plan(c))
        if rej is None:
            continue
        hit.add(wr.family_of(c))
        assert check in rej, f"{c.name}: {mutant} is not rejected by {regime} / {check} (rejected by: {rej})"
    if mutant == "empty_split_garbage":
        return
    want = {
        "f32_operands_bf16": {"conv_f32", "stem", "tn"},
        "acc_bf16": {"conv_bf16", "stem", "tn", "wgrad3x3", "wgradr", "wgrad8p"},
        "batch_stride_swapped": {"tn"},
        "bias_one_tile": {"conv_bf16", "conv_f32"},
        "bias_not_reduced": {"conv_bf16", "conv_f32", "wgradr", "wgrad8p"},
        "assign_accumulates": {"conv_bf16", "conv_f32", "wgrad3x3", "wgradr"},
        "accumulate_assigns": {"conv_bf16", "conv_f32", "stem", "wgrad3x3", "wgradr"},
        "split_dropped": {"conv_bf16", "conv_f32", "stem", "wgrad3x3", "wgradr"},
        "split_twice": {"conv_bf16", "conv_f32", "stem", "wgrad3x3", "wgradr"},
        "halo_wrap": {"conv_bf16", "conv_f32", "wgrad3x3"},
        "image_bleed": {"conv_bf16", "conv_f32", "wgrad3x3"},
        "hw_swapped": {"conv_bf16", "conv_f32", "wgrad3x3"},
        "tap_shifted": {"conv_bf16", "conv_f32", "stem", "wgrad3x3"},
        "stride_ignored": {"conv_bf16", "conv_f32", "stem"},
        "cout_tail_dropped": {"conv_bf16", "conv_f32", "stem", "tn"},
        "ntot_tail_dropped": {"conv_bf16", "conv_f32", "stem", "tn", "wgrad3x3"},
        "drop_pixel": set(wr.FAMILIES),
    }.get(mutant, set(wr.FAMILIES) - {"wgrad8p"})
    assert want <= hit, f"{mutant}: not exercised in {sorted(want - hit)}"


def test_positive_regime_rejects_truncated_operands_in_the_small_fp32_cases():
    n = 0
    for c in ALL:
        if c.dtype == "f32" and wr.geom(c).M <= 400:
            rej = wr.rejecting(c, _data(c, "positive"), "positive", _form(c), "f32_operands_bf16", _plan(c))
            assert "dw" in rej, c.name
            n += 1
    assert n >= 6


def test_an_unwritten_slab_of_an_empty_split_is_rejected():
    """No launcher's plan leaves a split without rows today (each takes ceil(M / rows) splits), so the mutant exists at no case; under
    a plan that has such a split the exact regime rejects the slab that was never written."""
    for c in ALL:
        assert not any(b <= a for a, b in _plan(c).bounds), c.name
    c = next(c for c in ALL if c.name == "g_3x3_b_2splits")
    pl = wr.plan(c)
    M = wr.geom(c).M
    pl = wr.Plan(pl.splits + 1, pl.bounds + ((M, M),), pl.stage, pl.tilesN, pl.bias_parts)
    d = _data(c, "exact")
    assert wr.reference(c, d, "slab", "empty_split_garbage", wr.plan(c)) is None
    assert "dw" in wr.rejecting(c, d, "exact", "slab", "empty_split_garbage", pl)
    v = wr.verdict(c, d, "exact", "slab", wr.reference(c, d, "slab", pl=pl), pl)          # an empty split that stores zeros is fine
    assert all(r <= 1.0 for r, _, _ in v.values())


def test_table_claims_every_kernel_and_every_reduce_path():
    assert {c.kern for c in wr.CASES + wr.PROBE_CASES} == set(wr.KERNELS)
    assert len({k.code for k in wr.KERNELS}) == len(wr.KERNELS)
    names = [c.name for c in wr.CASES + wr.PROBE_CASES]
    assert len(set(names)) == len(names)
    reached = set()
    for c in wr.CASES:
        c = wr.resolve(c, 256)
        pl = wr.plan(c, 256)
        assert 4 * wr.geom(c).M + 3 < 2 ** 24, c.name                  # the exact regime's sums stay exact in fp32
        for form in wr.forms(c):
            if form in ("slab", "assign"):
                reached.add(wr.expected_reduce(c, pl, form == "assign"))
    assert reached == set(wr.REDUCES), sorted(reached ^ set(wr.REDUCES))
    splits = {wr.plan(wr.resolve(c, 256), 256).splits for c in wr.CASES if c.kern.family == "generic" and c.entry == "conv"}
    assert 1 in splits and any(6 <= s < 48 for s in splits) and any(s >= 48 for s in splits)


def test_launch_query_code_round_trips():
    for k in wr.KERNELS:
        code = k.code | 1 << 8 | 3 << 9 | 1 << 12 | 1 << 13 | 49 << 16
        assert wr.decode(code) == dict(kern=k.code, slabs=True, reduce=3, assign=True, two=True, splits=49)


def test_host_queries_answer_without_a_gpu():
    """nkb_wgrad_last_kernel is -1 before any launch, and the workspace queries answer (and cover the restated plans' slabs)"""
    from nkb_classification import hip
    lib = hip.load()
    assert lib.nkb_wgrad_last_kernel() == -1 and hip.wgrad_last_kernel() == -1
    for c in ALL:
        g = wr.geom(c)
        if c.entry == "conv":
            need = hip.conv_wgrad_workspace(1 if c.dtype == "bf16" else 0, N=c.N, P=g.P, Q=g.Q, Cin=c.Cin, Cout=c.Cout, R=c.R, S=c.S,
                                            stride=c.stride, pad=c.pad, has_bias=c.bias)
            assert need > 0, c.name
            if c.kern.family in ("generic", "wgrad3x3"):               # (wgradr's count follows the CU budget, wgrad8p's the switch)
                pl = wr.plan(c)
                assert need >= pl.splits * c.Cout * g.Ntot + (pl.bias_parts * c.Cout if c.bias else 0), c.name
        elif c.entry == "stem":
            need = hip.stem_wgrad_workspace(1 if c.dtype == "bf16" else 0, c.N, c.H, c.W, c.Cout)
            assert need == wr.plan(c).splits * c.Cout * g.Ntot, c.name
    assert lib.nkb_wgrad_last_kernel() == -1
