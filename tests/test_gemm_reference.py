"""CPU proof that tests/test_gemm8p_gpu.py can fail: the float64 GEMM reference of tests/gemm_reference.py is exact where exactness
is known and agrees with an independent einsum + elementwise epilogue, the rounding yardstick sits inside the bound at every case of
the GPU table, and every mutant of the yardstick (a dropped or stale K slice, an uncleared accumulator, bias / residual / row-scale
indices off by one, double rounding, an inclusive ReLU6 mask, a missing K split of the companion, a missing dequantisation factor)
lands outside it, at the real K and N of each case with M cut to two row blocks plus a ragged rest."""
import math

import pytest
import torch

import gemm_reference as gr

# (case, mutant) pairs where the mistake changes nothing in exact arithmetic, so no bound can see it
EXACT_EXCEPTIONS = {
    # bf16(bf16(p)) == bf16(p): with nothing between the product and the store, rounding twice is rounding once; a 0/1 mask
    # (ReLU6 mask, mask bits) or a ReLU / clamp without a bias in front keeps that
    ("vit_fc1_dgrad", "double_round"), ("vit_qkv_dgrad", "double_round"), ("uni_fc2_dgrad", "double_round"),
    ("ragged_R65", "double_round"), ("uni8_fc2_dgrad_m0", "double_round"), ("uni8_fc2_dgrad_m1", "double_round"),
    ("f8_ragged_m1", "double_round"), ("rn50_l3_stats", "double_round"), ("strided_stats", "double_round"),
    ("small8_M257", "double_round"), ("strided8_q_m1", "double_round"),
    # one row: there is no row m + 1 to read from
    ("small_M1", "operand_next_row"), ("small8_M1", "operand_next_row"),
}


def test_reference_is_exact_on_small_integers():
    """bf16-exact small-integer operands: every product and sum is an integer far below 2^53, so the float64 reference IS the
    answer, and so is the yardstick where nothing rounds (|y| < 256 integers are bf16-exact)"""
    torch.manual_seed(0)
    M, N, K = 150, 64, 96
    x = torch.randint(-3, 4, (M, K)).float()
    w = torch.randint(-3, 4, (N, K)).float()
    bias = torch.randint(-5, 6, (N,)).float()
    add = torch.randint(-9, 10, (M, N)).float()
    want = (x.long() @ w.long().t() + bias.long() + add.long()).double()
    ep = gr.Epi(bias=bias, add=add)
    p = gr.product(x, w)
    assert torch.equal(p, (x.long() @ w.long().t()).double())
    ref = gr.outputs(p, ep, exact=True)
    assert torch.equal(ref["y"], want)
    yard = gr.outputs(p, ep, exact=False)
    if want.abs().max() < 256:
        assert torch.equal(yard["y"].double(), want)
    st = gr.outputs(p, gr.Epi(stats=True), exact=True)
    y = p
    torch.testing.assert_close(st["stats_sum"], torch.stack([y[:128].sum(0), y[128:].sum(0)]), rtol=0, atol=0)
    torch.testing.assert_close(st["stats_sq"], torch.stack([(y[:128] ** 2).sum(0), (y[128:] ** 2).sum(0)]), rtol=0, atol=0)


@pytest.mark.parametrize("case", [c for c in gr.CASES if c.M <= 2000 or c.N <= 512][:6] + [gr.CASES[0]], ids=lambda c: c.name)
def test_reference_matches_einsum_and_elementwise_epilogue(case):
    """an independent float64 einsum and the epilogue written out element by element, at a small M"""
    M = min(case.M, 20)
    x, w, xv, wv, ep = gr.make(case, M, "cpu", seed=3)
    p = gr.product(xv, wv)
    p2 = torch.einsum("mk,nk->mn", xv, wv)
    torch.testing.assert_close(p, p2, rtol=1e-15, atol=1e-12)
    ref = gr.outputs(p, ep, exact=True)
    v = p2.clone()
    if ep.deq:
        v = v * ep.deq[0] * ep.deq[1]
    for m in range(M):
        for n in range(case.N):
            t = v[m, n].item()
            if ep.bias is not None:
                t += ep.bias[n].item()
            if ep.add is not None:
                if ep.row_scale is not None:
                    t *= ep.row_scale[m // ep.rows_per_sample].item()
                t += ep.add[m, n].item()
            if ep.aux is not None:
                a = ep.aux[m, n].item()
                t = t * a if ep.aux_mode == 0 else (t if 0 < a < 6 else 0.0)
            if ep.mask_in is not None and not ep.mask_in[m, n]:
                t = 0.0
            if ep.relu == 1:
                t = max(t, 0.0)
            elif ep.relu == 2:
                t = min(max(t, 0.0), 6.0)
            elif ep.relu == 3:
                t = t * 0.5 * (1 + math.erf(t / math.sqrt(2)))
            v[m, n] = t
    torch.testing.assert_close(ref["y"], v, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.name)
def test_yardstick_inside_and_every_mutant_outside_the_bound(case):
    M = gr.cpu_M(case)
    x, w, xv, wv, ep = gr.make(case, M, "cpu", seed=1)
    geo = gr.geo_of(case, M)
    p = gr.product(xv, wv)
    ref = gr.outputs(p, ep, exact=True)
    yard = gr.outputs(p, ep, exact=False)
    for o in gr.outputs_of(ep):
        r, err, bound = gr.ratio(yard[o], ref[o], yard[o], o, geo)
        assert r <= 1 / gr.C_BOUND + 1e-12, (o, r)
        assert err < 3e-3 or o == "yq", (o, err)                     # the yardstick's error is bf16 rounding, nothing more
    if ep.mask_out:
        assert gr.bits_agree(yard["bits"], ref["pre"])
    if ep.yq is not None:
        assert gr.amax_agrees(yard["amax"], ref["y"])
    survived = []
    for mu in gr.MUTANTS:
        r = gr.worst_mutant_ratio(p, ep, xv, wv, geo, mu)
        if r is None:
            continue
        print(f"MUTANT {case.name} {mu} ratio={r:.2f}")
        if r <= 1.0:
            survived.append(mu)
    expected = sorted(m for (c, m) in EXACT_EXCEPTIONS if c == case.name)
    assert sorted(survived) == expected, f"{case.name}: mutants inside the bound {survived}, exact-arithmetic exceptions {expected}"


def test_every_mutant_is_caught_somewhere_and_every_instance_is_covered():
    assert set(c.instance for c in gr.CASES) == set(gr.INSTANCES)
    assert {c.M % 256 for c in gr.CASES if c.companion} >= {1, 63, 64, 65, 127, 128}
    S = {gr.ragged_split(c.K, c.N) for c in gr.CASES if c.companion}
    assert min(S) == 1 and max(S) == 16
    assert {m for (_, m) in EXACT_EXCEPTIONS} <= set(gr.MUTANTS)
