"""Float64 reference and bf16 rounding yardstick of the ViT attention WITH attention dropout, on the layout, metric and bound of
tests/attn_reference.py, and mutants for the ways a kernel that regenerates the dropout mask goes wrong.
tests/test_attention_dropout_reference.py proves on the CPU that the bound rejects every mutant; tests/test_attention_dropout_gpu.py
holds the HIP kernels to it.  No test lives here.

With P = softmax(scale * Q K^T), keep in {0, 1} [B, H, T, T] (query, key) and c = 1 / (1 - p):
  forward:  Pd = P o keep * c, O = Pd V; lse is the log-sum-exp of the undropped scores.
  backward: dPd = dO V^T, dP = dPd o keep * c, delta = rowsum(P o dP) = rowsum(dO o O), dS = P o (dP - delta) * scale,
            dV = Pd^T dO, dQ = dS K, dK = dS^T Q.
The yardstick rounds to bf16 where the fused kernels round: Pd (not P) before Pd V and before Pd^T dO, dS before its two products,
every stored output; delta comes from the bf16 forward output (attn_reference._attend with delta_from="o").
path="materialised" rounds where the engine's materialised path does instead: P to bf16 (nkb_attn_softmax), then Pd = bf16(P) o keep * c
to bf16 (nkb_dropout), the same stored Pd in dV, and delta and dS from the bf16 P (delta_from="pb").
"""
import torch

import attn_reference as ar

MUTANTS = ("mask_transposed", "mask_next_head", "c_not_in_dp", "dv_from_p", "delta_unmasked", "pitch_T")


def keep_from_flat(flat, B, T, H, pitch):
    """keep[b, h, q, k] = flat[((b * H + h) * T + q) * pitch + k]: the decisions of a [B*H, T, pitch] mask tensor for the T keys"""
    return flat[:B * H * T * pitch].reshape(B, H, T, pitch)[..., :T]


def _attend(q, k, v, do, keep, c, *, exact, mutant=None, path="fused"):
    r = (lambda x: x) if exact else ar.bf
    mat = path == "materialised" and not exact
    if mutant == "mask_transposed":           # 1. keep[k][q]
        keep = keep.transpose(-2, -1)
    elif mutant == "mask_next_head":          # 2. the mask of the next head
        keep = torch.roll(keep, -1, 1)
    keep = keep.to(q.dtype)
    s = (q @ k.transpose(-2, -1)) * ar.SCALE
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    lse = (m + torch.log(z)).squeeze(-1)
    pn = r(e / z) if mat else e / z
    pd = r(pn * keep * c)
    o = r(pd @ v)
    p = pn if mat else torch.exp(s - lse[..., None])
    dpd = do @ v.transpose(-2, -1)
    dp = dpd * keep * (1.0 if mutant == "c_not_in_dp" else c)       # 3. c in the forward pass only
    if mutant == "delta_unmasked":            # 5. delta from the undropped products
        delta = (p * dpd).sum(-1, keepdim=True)
    elif mat:
        delta = (p * dp).sum(-1, keepdim=True)
    else:
        delta = (do * o).sum(-1, keepdim=True)
    ds = r(p * (dp - delta) * ar.SCALE)
    pdb = pd if mat else r(p if mutant == "dv_from_p" else p * keep * c)            # 4. dV from the undropped P
    return dict(o=o, lse=lse, P=r(p), dS=ds, dq=r(ds @ k), dk=r(ds.transpose(-2, -1) @ q), dv=r(pdb.transpose(-2, -1) @ do))


def _run(qkv, do, keep, p, B, T, H, exact, mutant, flat, drop_ld, path="fused"):
    if mutant == "pitch_T":                   # 6. the element index formed with the pitch T instead of drop_ld
        if flat is None or drop_ld == T:
            return None
        keep, mutant = keep_from_flat(flat, B, T, H, T), None
    if mutant == "mask_next_head" and H < 2:
        return None
    dt = torch.float64 if exact else torch.float32
    q, k, v = ar.split_qkv(qkv.to(dt), B, T, H)
    return ar._finish(_attend(q, k, v, ar.heads(do.to(dt), B, T, H), keep, 1.0 / (1.0 - p), exact=exact, mutant=mutant, path=path),
                      B, T, H)


def reference(qkv, do, keep, p, B, T, H, mutant=None, flat=None, drop_ld=None):
    """float64 truth (outputs as attn_reference.reference); with `mutant`, the exact effect of that mistake (None where it does not
    exist at this shape).  flat / drop_ld: the flat mask array keep was cut from and its pitch, for the pitch mutant."""
    return _run(qkv, do, keep, p, B, T, H, True, mutant, flat, drop_ld)


def yardstick(qkv, do, keep, p, B, T, H, mutant=None, flat=None, drop_ld=None, path="fused"):
    """the same math in float32 rounded to bf16 where the fused kernels round (path="materialised": where the engine's materialised
    path rounds); with `mutant`, what a kernel carrying it computes"""
    return _run(qkv, do, keep, p, B, T, H, False, mutant, flat, drop_ld, path)
