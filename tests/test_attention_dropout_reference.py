"""CPU proof that tests/test_attention_dropout_gpu.py can fail: the float64 reference of attention with dropout
(tests/attn_dropout_reference.py) is right (autograd), its bf16 yardstick sits inside attn_reference's bound, and every mutant — the
mask transposed, the next head's mask, 1/(1-p) missing from dP, dV from the undropped P, delta without the mask, the index pitch T
instead of drop_ld — lands outside it on at least one of o, dq, dk, dv."""
import pytest
import torch

import attn_dropout_reference as adr
import attn_reference as ar

B, H = 2, 2
P_DROP = 0.25
SHAPES = (17, 64, 197)


def _mask(T, seed):
    """a flat Bernoulli(1 - p) array for a [B*H, T, drop_ld] tensor, drop_ld = roundup(T, 64), and keep [B, H, T, T] cut from it"""
    drop_ld = (T + 63) // 64 * 64
    g = torch.Generator().manual_seed(seed)
    flat = torch.rand(B * H * T * drop_ld, generator=g) >= P_DROP
    return flat, drop_ld, adr.keep_from_flat(flat, B, T, H, drop_ld)


def test_reference_matches_autograd():
    T = 17
    qkv, do = ar.inputs("random", B, T, H, seed=5)
    _, _, keep = _mask(T, 5)
    qkv = qkv.double().requires_grad_(True)
    q, k, v = ar.split_qkv(qkv, B, T, H)
    s = (q @ k.transpose(-2, -1)) * ar.SCALE
    o = ar.rows((s.softmax(-1) * keep.double() / (1 - P_DROP)) @ v)
    o.backward(do.double())
    ref = adr.reference(qkv.detach(), do, keep, P_DROP, B, T, H)
    torch.testing.assert_close(ref["o"], o.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["lse"], torch.logsumexp(s.detach(), -1).reshape(B * H, T), rtol=0, atol=1e-12)
    torch.testing.assert_close(ref["dqkv"], qkv.grad, rtol=0, atol=1e-12)


def test_no_dropout_is_the_plain_reference():
    T = 33
    qkv, do = ar.inputs("random", B, T, H, seed=6)
    ones = torch.ones(B, H, T, T, dtype=torch.bool)
    for fn, plain in ((adr.reference, ar.reference(qkv, do, B, T, H)), (adr.yardstick, ar.yardstick(qkv, do, B, T, H))):
        got = fn(qkv, do, ones, 0.0, B, T, H)
        for n in ("o", "lse", "dqkv"):
            assert torch.equal(got[n], plain[n]), n


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T", SHAPES)
def test_yardstick_inside_the_bound_and_every_mutant_outside(T, regime):
    qkv, do = ar.inputs(regime, B, T, H, seed=T)
    flat, drop_ld, keep = _mask(T, T)
    ref = adr.reference(qkv, do, keep, P_DROP, B, T, H)
    yard = adr.yardstick(qkv, do, keep, P_DROP, B, T, H)
    for n in ("o",) + ar.GRADS:
        e = ar.rel_err(n, yard[n], ref[n], B, T, H)
        assert e <= ar.bound(e) < 3e-2, (T, n, e)
    assert ar.lse_err(yard["lse"], ref["lse"]) < ar.LSE_RTOL / 10
    # lse is that of the undropped scores
    assert torch.equal(ref["lse"], ar.reference(qkv, do, B, T, H)["lse"])
    missing = []
    for m in adr.MUTANTS:
        mut = adr.yardstick(qkv, do, keep, P_DROP, B, T, H, mutant=m, flat=flat, drop_ld=drop_ld)
        if mut is None:
            missing.append(m)
            continue
        r = ar.worst_ratio(mut, ref, yard, B, T, H)
        assert max(v for k, v in r.items() if k != "lse") > 1, (T, regime, m, r)
    assert missing == (["pitch_T"] if drop_ld == T else []), missing
