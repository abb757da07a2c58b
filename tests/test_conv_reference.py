"""CPU proof that tests/test_conv_igemm_gpu.py can fail: the float64 gather + matmul reference of tests/conv_reference.py equals
torch's convolution and its autograd on every convolution case, the rounding yardstick sits inside every bound at every case of the
GPU table (also with its product accumulated in another order), the share of BN-mask elements left out stays within its cap, and
every mutant of the yardstick is rejected by the bound of the output it corrupts."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr

DEV = "cpu"
_CACHE = {}


def _setup(case):
    """(operands, reference, yardstick) of a case, computed once and left unchanged"""
    if case.name not in _CACHE:
        d = cr.make(case, DEV, seed=7)
        _CACHE[case.name] = (d, cr.outputs(case, d, exact=True), cr.outputs(case, d, exact=False))
    return _CACHE[case.name]


CONV_CASES = [c for c in cr.CASES if c.entry in cr.CONV_ENTRIES and not c.grouped]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.name)
def test_gather_reference_equals_torch_convolution_in_float64(case):
    d = cr.make(case, DEV, seed=3)
    P, Q, M, Mfull, *_ = cr.dims(case)
    src, val = cr.gather_index(case, DEV)
    rows = (d.x.double()[src] * val[:, :, None]).reshape(M, -1)
    got = rows @ d.w.double().t()                                             # [M][Cout]
    x = d.x.double().reshape(case.N, case.H, case.W, case.Cin).permute(0, 3, 1, 2)
    w = d.w.double().reshape(case.Cout, case.R, case.S, case.Cin)
    if case.mode == 0:
        want = F.conv2d(x, w.permute(0, 3, 1, 2), stride=case.stride, padding=case.pad)
        assert want.shape == (case.N, case.Cout, P, Q)
        want = want.permute(0, 2, 3, 1).reshape(M, case.Cout)
    else:
        # the data gradient of conv(inp, wc) for the output gradient x: the launch's filter is wc as [Cin_conv][R][S][Cout_conv]
        if case.cls is not None:
            full = torch.zeros(case.Cout, 3, 3, case.Cin, dtype=torch.float64)
            rs, ss = cr.class_taps(*case.cls)
            for i, r in enumerate(rs):
                for j, s in enumerate(ss):
                    full[:, r, s] = w[:, i, j]
            assert torch.equal(cr.class_filter(full, *case.cls), w)
            w, stride, pad, (Ho, Wo) = full, 2, 1, case.out
        else:
            stride, pad, (Ho, Wo) = case.stride, case.pad, (P, Q)
        inp = torch.zeros(case.N, case.Cout, Ho, Wo, dtype=torch.float64, requires_grad=True)
        out = F.conv2d(inp, w.permute(3, 0, 1, 2), stride=stride, padding=pad)
        assert out.shape == x.shape
        (grad,) = torch.autograd.grad(out, inp, x)
        want = grad.permute(0, 2, 3, 1).reshape(-1, case.Cout)
        if case.cls is not None:
            want = want[cr.out_rows(case, DEV)]
    scale = want.abs().max().item()
    assert (got - want).abs().max().item() <= 1e-12 * max(scale, 1.0)


@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_yardstick_is_inside_every_bound(case):
    d, ref, yard = _setup(case)
    for label, y in (("float64 product", yard), ("k-tile partial sums", cr.outputs(case, d, exact=False, order="ktile"))):
        v = cr.verdict(case, d, ref, yard, y)
        print(case.name, label, {k: f"{r:.3f}" for k, (r, _, _) in v.items()})
        assert all(r <= 1.0 for r, _, _ in v.values()), (label, v)
    share = ref["skip"].float().mean().item()
    assert share <= cr.MASK_SHARE, f"{share:.2e} of the mask elements sit on the edge"


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_mutant_is_rejected_by_the_output_it_corrupts(mutant):
    """Every case at which the mutant exists rejects it (the grouped-walk case is left to one mutant: it is the only large one),
    and the rejecting check belongs to the output cr.REJECTED_BY names."""
    hit = 0
    for case in cr.CASES:
        if case.grouped and mutant != "drop_tap":
            continue
        d, ref, yard = _setup(case)
        rej = cr.rejecting(case, d, mutant, ref, yard)
        if rej is None:
            continue
        hit += 1
        want = cr.REJECTED_BY[mutant]
        names = {"y": ("y_elem", "y_tile", "y2_elem", "y2_tile", "y_untouched", "bits")}.get(want, (want,))
        assert any(k in names for k in rej), f"{case.name}: {mutant} is not rejected by {want} (rejected by: {rej})"
    assert hit >= 1, f"{mutant} exists at no case"


def test_every_instance_is_claimed_and_known():
    claimed = {c.inst for c in cr.CASES}
    assert claimed == set(cr.INSTANCES), (sorted(map(str, set(cr.INSTANCES) - claimed)), sorted(map(str, claimed - set(cr.INSTANCES))))
    assert len({i.code for i in cr.INSTANCES}) == len(cr.INSTANCES)
    assert sum(c.grouped for c in cr.CASES) == 1
    assert len({c.name for c in cr.CASES}) == len(cr.CASES)


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """The relative part of the element bound: a correctly rounded bf16 store is off by up to 2^-8 of the value (8 significant
    bits), not 2^-9, so r = 2^-9 would reject an ideal kernel; r = 2^-8 is attained and never exceeded."""
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, 2.0 + 2.0 ** -7 + 2.0 ** -19], dtype=torch.float64)
    rel = ((cr.bf(v) - v).abs() / v).tolist()
    assert all(2.0 ** -9 * 1.9 < r <= 2.0 ** -8 for r in rel), rel
    torch.manual_seed(1)
    w = torch.randn(100000, dtype=torch.float64) * 3
    assert ((cr.bf(w) - w).abs() <= cr.R_BF16 * w.abs()).all()
    assert cr.R_BF16 == 2.0 ** -8


def test_bit_layouts_round_trip():
    torch.manual_seed(0)
    m = torch.rand(5, 24) < 0.5
    for dt, nb in (("bf16", 3), ("f32", 6)):
        b = cr.pack_bits(m, dt, 40, fill=0x5A)
        assert b.shape == (5, 40 // (8 if dt == "bf16" else 4)) and bool((b[:, nb:] == 0x5A).all())
        assert torch.equal(cr.unpack_bits(b, dt, 24), m)
    assert cr.pack_bits(torch.tensor([[True, False, False, True, True, False, False, False]]), "bf16", 8).item() == 0b00011001
    assert cr.pack_bits(torch.tensor([[True, False, False, True, True, False, False, False]]), "f32", 8).tolist() == [[0b1001, 0b0001]]


def test_entries_refuse_what_the_table_cannot_hold():
    """Two pairings one would look for in the table do not exist: nkb_conv_cat_relu_bits below 65 output channels and
    nkb_linear_residual_scaled outside the eight-phase core (N = 192).  Both are refused on the host with a message."""
    from nkb_classification import hip
    lib = hip.load()
    p = ctypes.c_void_p(64)
    assert lib.nkb_conv_cat_relu_bits(1, None, 72, 64, None, 136, 128, None, p, None, p, 286, 40, 56, None) != 0
    assert b"Cout=40 > 64" in lib.nkb_last_error()
    assert lib.nkb_linear_residual_scaled(1, None, None, None, p, p, 1, None, 200, 128, 192, None) != 0
    assert b"eight-phase core" in lib.nkb_last_error()
    assert lib.nkb_conv_last_instance() >= -1
