"""CPU proof that tests/test_attention_gpu.py can fail: the float64 attention reference of tests/attn_reference.py is right
(autograd), the bf16 rounding yardstick sits inside the bound, and every mutant of the reference — a kernel that counts the
padding keys, drops the last key, reads a query row of the next image, swaps two heads' K, or stores the lse of one extra key —
lands outside it at every T of the GPU sweep and in every input regime, unless the mistake changes nothing measurable there."""
import math

import pytest
import torch

import attn_reference as ar

B, H = ar.SWEEP_BH


def test_sweep_covers_every_key_block_count():
    assert {(T + 15) // 16 for T in ar.SWEEP} == set(range(1, 17))
    assert any(T % 16 for T in ar.SWEEP) and 256 in ar.SWEEP


@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 17, 3), (1, 40, 2)], ids=lambda s: "B%dT%dH%d" % s)
def test_reference_backward_matches_autograd(shape):
    b, T, h = shape
    qkv, do = ar.inputs("random", b, T, h, seed=1)
    qkv = qkv.double().requires_grad_(True)
    q, k, v = ar.split_qkv(qkv, b, T, h)
    s = (q @ k.transpose(-2, -1)) * ar.SCALE
    o = ar.rows(s.softmax(-1) @ v)
    o.backward(do.double())
    ref = ar.reference(qkv.detach(), do, b, T, h)
    torch.testing.assert_close(ref["o"], o.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["lse"], torch.logsumexp(s.detach(), -1).reshape(b * h, T), rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["dqkv"], qkv.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["colsum"], qkv.grad.sum(0), rtol=0, atol=1e-11)
    # P and dS as the backward kernels write them: dS = P o (dP - rowsum(dO o O)) * scale
    P = s.detach().softmax(-1)
    dP = ar.heads(do.double(), b, T, h) @ v.detach().transpose(-2, -1)
    torch.testing.assert_close(ref["P"], P, rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["dS"], P * (dP - (P * dP).sum(-1, keepdim=True)) * ar.SCALE, rtol=0, atol=1e-12)


@pytest.mark.parametrize("regime", ar.REGIMES)
def test_regimes_are_what_they_claim(regime):
    T = 97
    qkv, do = ar.inputs(regime, B, T, H, seed=2)
    ref = ar.reference(qkv, do, B, T, H)
    assert torch.equal(qkv, ar.bf(qkv)) and torch.equal(do, ar.bf(do))
    if regime == "uniform":   # o is the mean of V over exactly T keys; lse = log T
        _, _, v = ar.split_qkv(qkv.double(), B, T, H)
        torch.testing.assert_close(ref["o"], ar.rows(v.mean(2, keepdim=True).expand(-1, -1, T, -1)), rtol=0, atol=1e-12)
        torch.testing.assert_close(ref["lse"], torch.full_like(ref["lse"], math.log(T)), rtol=0, atol=1e-12)
    if regime == "sharp":     # near one-hot rows
        assert ref["P"].amax(-1).median() > 0.8


@pytest.mark.parametrize("delta_from", ["o", "p", "pb"])
@pytest.mark.parametrize("regime", ar.REGIMES)
def test_yardstick_inside_the_bound_and_the_bound_tight(regime, delta_from):
    """the yardstick passes its own bound (C_BOUND > 1), its lse passes LSE_RTOL, and the bound is a bf16-sized one"""
    for T in (1, 17, 128, 197, 256):
        qkv, do = ar.inputs(regime, B, T, H, seed=T)
        ref = ar.reference(qkv, do, B, T, H)
        yard = ar.yardstick(qkv, do, B, T, H, delta_from=delta_from)
        for n in ("o", "dq", "dk", "dv", "P", "dS", "colsum"):
            e = ar.rel_err(n, yard[n], ref[n], B, T, H)
            assert e <= ar.bound(e) < 3e-2, (T, n, e)
        assert ar.lse_err(yard["lse"], ref["lse"]) < ar.LSE_RTOL / 10


def _below_resolution(mut, ref, B_, T, H_, lse=True):
    """in exact arithmetic, the mistake moves no output by more than the test's floors (FLOOR, LSE_RTOL) can resolve"""
    return (all(ar.rel_err(n, mut[n], ref[n], B_, T, H_) <= ar.FLOOR for n in ("o",) + ar.GRADS)
            and (not lse or ar.lse_err(mut["lse"], ref["lse"]) <= ar.LSE_RTOL))


@pytest.mark.parametrize("T", ar.SWEEP)
def test_every_mutant_fails_the_bound(T):
    """For each mutant, regime and T: what a kernel carrying the mistake would compute (the yardstick on the mutated
    operands) fails the test — or, in exact arithmetic, the mistake moves nothing by more than the floors resolve, which is
    only allowed where the scores make it so: zero padding keys and an extra zero key weigh e^-10 and less against near
    one-hot rows (sharp), and K is invisible at T = 1 with Q = 0.  In the random and uniform regimes o / dq / dk / dv alone must fail, without the lse check (unless
    only the lse moves: at T = 1 every K gives P = 1); the lse mutant must also fail the lse tolerance there."""
    inert = []
    for regime in ar.REGIMES:
        qkv, do = ar.inputs(regime, B, T, H, seed=T)
        ref = ar.reference(qkv, do, B, T, H)
        yard = ar.yardstick(qkv, do, B, T, H)
        for m in ar.MUTANTS:
            mut = ar.yardstick(qkv, do, B, T, H, mutant=m)
            if mut is None:
                assert m == "pad_keys" and T % 32 == 0
                continue
            r = ar.worst_ratio(mut, ref, yard, B, T, H)
            exact = ar.reference(qkv, do, B, T, H, mutant=m)
            if max(r.values()) <= 1:
                assert _below_resolution(exact, ref, B, T, H), (regime, m, r)
                inert.append((regime, m))
                continue
            if regime != "sharp" and not _below_resolution(exact, ref, B, T, H, lse=False):
                assert max(v for k, v in r.items() if k != "lse") > 1, (regime, m, r)
                if m == "lse_extra_key":
                    assert r["lse"] > 1, (regime, r)
    allowed = {("sharp", "pad_keys"), ("sharp", "lse_extra_key")} | ({("uniform", "swap_k_heads")} if T == 1 else set())
    assert set(inert) <= allowed, inert      # (T = 1 and Q = 0: no score depends on K, and dQ = dS K with dS = 0)


@pytest.mark.parametrize("geom", [(2, 197, 12), (2, 256, 16)], ids=lambda g: "B%dT%dH%d" % g)
def test_mutants_fail_at_production_geometry(geom):
    b, T, h = geom
    qkv, do = ar.inputs("random", b, T, h, seed=3)
    ref = ar.reference(qkv, do, b, T, h)
    yard = ar.yardstick(qkv, do, b, T, h)
    assert max(ar.worst_ratio(yard, ref, yard, b, T, h).values()) <= 1
    for m in ar.MUTANTS:
        mut = ar.yardstick(qkv, do, b, T, h, mutant=m)
        if mut is not None:
            r = ar.worst_ratio(mut, ref, yard, b, T, h)
            assert max(v for k, v in r.items() if k != "lse") > 1, (m, r)
