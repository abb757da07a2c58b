"""QuickGELU epilogue (nkb_linear_gelu acts 7 / 8 / 9) on the yardstick, metric and bound of tests/gemm_reference.py.  No test lives here.

The launch: v = x w^T + bias;  y = bf16(q(v)),  y2 = bf16(q'(v))  with  q(v) = v s,  q'(v) = s (1 + 1.702 v (1 - s)),
s = 1 / (1 + exp(-1.702 v)).  The reference does this in float64 and rounds nothing.  The yardstick is gemm_reference's: the float64
product rounded to fp32 (the accumulator), the epilogue in fp32, bf16 rounding of y and y2 where the kernel rounds.  What it leaves
out of the kernel's arithmetic — exp2 / rcp at one fp32 ulp each, the order of the fp32 accumulation — is three orders of magnitude
below the bf16 rounding (2^-9) that makes up the yardstick's own error.

MUTANTS are the yardstick with the activation subtly wrong, in the ways this feature can go wrong: the exact-erf GELU in its place
(what a QuickGELU checkpoint got before these members existed), a derivative that is the sigmoid alone, and the factor 1.702 missing
from the derivative's second term.  tests/test_quickgelu_cpu.py proves that the bound rejects each."""
import torch

import gemm_reference as gr

A = 1.702
MUTANTS = ("erf_gelu", "derivative_without_second_term", "derivative_factor_missing")


def quick_gelu_pair(v: torch.Tensor, mutant=None):
    """(q(v), q'(v)) in v's dtype"""
    if mutant == "erf_gelu":
        return gr._gelu(v)
    s = torch.sigmoid(A * v)
    if mutant == "derivative_without_second_term":
        return v * s, s
    if mutant == "derivative_factor_missing":
        return v * s, s * (1 + v * (1 - s))
    assert mutant is None, mutant
    return v * s, s * (1 + A * v * (1 - s))


def outputs(p: torch.Tensor, bias, *, exact: bool, mutant=None):
    """{y, y2, pre} of the act-9 launch from the float64 product p [M][N]: exact = the float64 reference, else the yardstick"""
    dt = torch.float64 if exact else torch.float32
    v = p.to(dt)
    if bias is not None:
        v = v + bias.to(dt)
    u, d = quick_gelu_pair(v, mutant)
    r = (lambda t: t) if exact else gr.bf
    return {"y": r(u), "y2": r(d), "pre": v}


def hold(tag, out, got, ref, yard, geo=gr.Geo()):
    """gemm_reference's verdict on one output: prints the figure, then asserts ratio <= 1 in the worst tile"""
    r, err, bound = gr.ratio(got, ref, yard, out, geo)
    print(f"RATIO {tag} {out} err={err:.3e} bound={bound:.3e} ratio={r:.3f}")
    assert r <= 1.0, f"{tag}: {out} error {err:.3e} > bound {bound:.3e} in its worst tile"
