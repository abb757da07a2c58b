"""nkb_layernorm at the widths of the masked-tail kernels (csrc/transformer.hip: any D % 8 == 0 up to 2048 that is not a full-lane
instantiation) against torch's CPU LayerNorm on the same rounded inputs, at the bounds of tests/test_ops_gpu.py (fp32: rtol 2e-5,
atol 2e-5 sqrt(k); bf16: rtol 2e-2, atol 5e-3 sqrt(k); k = 1 for y, 4 for dx, rows for dgamma / dbeta).

mean and rstd are fp32 statistics of at most 2040 rounded inputs in both dtypes: they are held to the fp32 bound with k = 1."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-6
SENTINEL = -1024.0                      # exact in bf16


def tol(dtype, k=1):
    return dict(rtol=2e-5, atol=2e-5 * math.sqrt(k)) if dtype == torch.float32 else dict(rtol=2e-2, atol=5e-3 * math.sqrt(k))


def rnd(t, dtype):
    return t.to(dtype).float()


def _reference(dtype, rows, D, seed, with_add=True):
    """torch CPU LayerNorm forward / backward on inputs rounded to `dtype` (computed once per case)."""
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(rows, D, generator=g) * 1.5 + 0.3, dtype).requires_grad_(True)
    ln = torch.nn.LayerNorm(D, eps=EPS)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(D, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(D, generator=g))
    dy = rnd(torch.randn(rows, D, generator=g), dtype)
    add = rnd(torch.randn(rows, D, generator=g), dtype) if with_add else None
    y = ln(x)
    y.backward(dy)
    xd = x.detach().double()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + EPS)
    return dict(x=x.detach(), dy=dy, add=add, gamma=ln.weight.detach(), beta=ln.bias.detach(), y=y.detach(),
                dx=x.grad + (add if with_add else 0), dgamma=ln.weight.grad, dbeta=ln.bias.grad, mean=mean.float(), rstd=rstd.float())


def _padded(t, ld, dtype, fill=0.0):
    out = torch.full((t.shape[0], ld), fill, device=DEV, dtype=dtype)
    out[:, :t.shape[1]] = t.to(DEV, dtype)
    return out


def _backward_forms(d, dy, ldg, x, ldx, gamma, mean, rstd, add, ldo, rows, D, dtype, fill=0.0):
    """The three parameter-gradient forms: atomic, workspace, partial rows + param_reduce; the workspace form twice."""
    work = torch.empty(hip.layernorm_ws(D), device=DEV)
    res = []
    for form in ("atomic", "work", "work", "split"):
        dx = torch.full((rows, ldo), fill, device=DEV, dtype=dtype)
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        if form == "atomic":
            hip.layernorm_bwd(d, dy, ldg, x, ldx, gamma, mean, rstd, add, dx, ldo, dg, db, rows, D)
        elif form == "work":
            hip.layernorm_bwd(d, dy, ldg, x, ldx, gamma, mean, rstd, add, dx, ldo, dg, db, rows, D, workspace=work)
        else:
            hip.layernorm_bwd(d, dy, ldg, x, ldx, gamma, mean, rstd, add, dx, ldo, None, None, rows, D, workspace=work)
            hip.layernorm_param_reduce(work, rows, D, 2, dg, db)
        torch.cuda.synchronize()
        res.append((dx, dg, db))
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [8, 72, 192, 264, 1032, 2040])
def test_forward_and_the_three_backward_forms(dtype, D):
    """8, 72, 192: one pass with 2, 18, 48 active lanes; 264, 1032: full pass(es) + a 2-lane tail; 2040: eight passes."""
    rows = 37
    r = _reference(dtype, rows, D, seed=100 + D)
    d = hip.dt(dtype)
    x, dy, add = (r[k].to(DEV, dtype) for k in ("x", "dy", "add"))
    gamma, beta = r["gamma"].to(DEV), r["beta"].to(DEV)
    y = torch.empty(rows, D, device=DEV, dtype=dtype)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    hip.layernorm_fwd(d, x, D, gamma, beta, y, D, mean, rstd, rows, D, EPS)
    torch.cuda.synchronize()
    torch.testing.assert_close(y.float().cpu(), r["y"], **tol(dtype))
    torch.testing.assert_close(mean.cpu(), r["mean"], **tol(torch.float32))
    torch.testing.assert_close(rstd.cpu(), r["rstd"], **tol(torch.float32))
    atomic, work, work2, split = _backward_forms(d, dy, D, x, D, gamma, mean, rstd, add, D, rows, D, dtype)
    for dx, dg, db in (atomic, work, split):
        torch.testing.assert_close(dx.float().cpu(), r["dx"], **tol(dtype, 4))
        torch.testing.assert_close(dg.cpu(), r["dgamma"], **tol(dtype, rows))
        torch.testing.assert_close(db.cpu(), r["dbeta"], **tol(dtype, rows))
    assert torch.equal(atomic[0], work[0]) and torch.equal(work[0], split[0])           # dx does not depend on the form
    assert all(torch.equal(a, b) for a, b in zip(work, work2))                          # no float atomics: same bits twice
    assert torch.equal(work[1], split[1]) and torch.equal(work[2], split[2])            # the same ordered sums in one call or two


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
def test_many_rows_with_padded_strides_leave_the_pad_columns_alone(dtype, with_add):
    """5037 rows of 192 in rows of 200: many rows per wave, 115 partial rows; the pad columns of y and dx hold a sentinel that a
    masked lane must not overwrite."""
    rows, D = 5037, 192
    ld = D + 8
    r = _reference(dtype, rows, D, seed=7, with_add=with_add)
    d = hip.dt(dtype)
    x, dy = _padded(r["x"], ld, dtype), _padded(r["dy"], ld, dtype)
    add = _padded(r["add"], ld, dtype) if with_add else None
    gamma, beta = r["gamma"].to(DEV), r["beta"].to(DEV)
    y = torch.full((rows, ld), SENTINEL, device=DEV, dtype=dtype)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    hip.layernorm_fwd(d, x, ld, gamma, beta, y, ld, mean, rstd, rows, D, EPS)
    torch.cuda.synchronize()
    assert bool((y[:, D:] == SENTINEL).all())
    torch.testing.assert_close(y[:, :D].float().cpu(), r["y"], **tol(dtype))
    torch.testing.assert_close(mean.cpu(), r["mean"], **tol(torch.float32))
    torch.testing.assert_close(rstd.cpu(), r["rstd"], **tol(torch.float32))
    atomic, work, work2, split = _backward_forms(d, dy, ld, x, ld, gamma, mean, rstd, add, ld, rows, D, dtype, fill=SENTINEL)
    for dx, dg, db in (atomic, work, split):
        assert bool((dx[:, D:] == SENTINEL).all())
        torch.testing.assert_close(dx[:, :D].float().cpu(), r["dx"], **tol(dtype, 4))
        torch.testing.assert_close(dg.cpu(), r["dgamma"], **tol(dtype, rows))
        torch.testing.assert_close(db.cpu(), r["dbeta"], **tol(dtype, rows))
    assert torch.equal(atomic[0], work[0]) and torch.equal(work[0], split[0])
    assert all(torch.equal(a, b) for a, b in zip(work, work2))
    assert torch.equal(work[1], split[1]) and torch.equal(work[2], split[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_class_token_rows(dtype):
    """The final norm of the ViT: 5 rows taken at stride 17 * 192 out of a [5 * 17, 192] token tensor; the backward writes the
    class-token rows of a zeroed gradient tensor and nothing else."""
    B, T, D = 5, 17, 192
    r = _reference(dtype, B, D, seed=3, with_add=False)
    d = hip.dt(dtype)
    g = torch.Generator().manual_seed(4)
    tokens = torch.randn(B * T, D, generator=g).to(DEV, dtype)
    tokens[::T] = r["x"].to(DEV, dtype)
    dy = r["dy"].to(DEV, dtype)
    gamma, beta = r["gamma"].to(DEV), r["beta"].to(DEV)
    y = torch.empty(B, D, device=DEV, dtype=dtype)
    mean, rstd = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    hip.layernorm_fwd(d, tokens, T * D, gamma, beta, y, D, mean, rstd, B, D, EPS)
    torch.cuda.synchronize()
    torch.testing.assert_close(y.float().cpu(), r["y"], **tol(dtype))
    work = torch.empty(hip.layernorm_ws(D), device=DEV)
    gx = torch.zeros(B * T, D, device=DEV, dtype=dtype)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    hip.layernorm_bwd(d, dy, D, tokens, T * D, gamma, mean, rstd, None, gx, T * D, dg, db, B, D, workspace=work)
    torch.cuda.synchronize()
    torch.testing.assert_close(gx[::T].float().cpu(), r["dx"], **tol(dtype, 4))
    other = torch.ones(B * T, dtype=torch.bool)
    other[::T] = False
    assert bool((gx[other.to(DEV)] == 0).all())
    torch.testing.assert_close(dg.cpu(), r["dgamma"], **tol(dtype, B))
    torch.testing.assert_close(db.cpu(), r["dbeta"], **tol(dtype, B))


def test_width_beyond_2048_is_refused():
    D, rows = 2056, 4
    x = torch.zeros(rows, D, device=DEV)
    y = torch.empty_like(x)
    g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    with pytest.raises(RuntimeError, match="layernorm"):
        hip.layernorm_fwd(hip.dt(torch.float32), x, D, g, b, y, D, mean, rstd, rows, D, EPS)
