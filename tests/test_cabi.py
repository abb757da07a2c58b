"""The C-ABI shared library loads (no GPU needed) and exports exactly the symbols include/nkbhip.h declares."""
import ctypes
import re
from pathlib import Path

from nkb_classification import hip

ROOT = Path(__file__).resolve().parents[1]


def _declared():
    text = (ROOT / "include" / "nkbhip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_header_symbols():
    lib = hip.load()
    declared = _declared()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/nkbhip.h but not exported by libnkbhip.so"
    assert sorted(hip.exported_symbols()) == declared, "ctypes binding table and header disagree"
    assert lib.nkb_version() >= 100
    assert lib.nkb_last_error() is not None
    assert lib.nkb_conv_gemm_stat_tiles(1, 802816, 64) == 3136 and lib.nkb_conv_gemm_stat_tiles(0, 12544, 2048) == 98
    assert lib.nkb_kernel_name(0) == b"conv_igemm_fwd"


# One rejected call per nkb_set_error branch of the convolution / GEMM / weight-gradient entry points in csrc/conv_igemm.hip:
# (entry point, arguments, a distinctive part of the message).  Every call returns before it touches an operand, so a
# non-null pointer is any non-zero address.
_P = ctypes.c_void_p(64)
_BIG = 1 << 20


def _conv_gemm(dtype=1, add=None, N=1, H=8, W=8, Cin=64, ldx=64, P=8, Q=8, Cout=64, ldy=64, ldadd=0, R=1, S=1, stride=1, pad=0,
               add_h=0, add_w=0, add_bits=None):
    return (dtype, 0, None, None, None, add, None, None, N, H, W, Cin, ldx, P, Q, Cout, ldy, ldadd, R, S, stride, pad, 0, 0,
            add_h, add_w, add_bits, None)


def _dgrad_bn(dtype=1, scale=_P, shift=_P, relu_bits=None, add=None, ldadd=0, add_bits=None, add_h=0, add_w=0, N=1, H=8, W=8, Cin=64,
              ldx=64, P=8, Q=8, Cout=64, ldy=64, R=1, S=1, stride=1, pad=0):
    return (dtype, None, None, None, None, scale, shift, None, None, relu_bits, add, ldadd, add_bits, add_h, add_w, N, H, W, Cin, ldx,
            P, Q, Cout, ldy, R, S, stride, pad, None)


def _affine_residual(dtype=1, N=1, H=8, W=8, Cin=64, ldx=64, P=8, Q=8, Cout=128, ldy=128, ldres=128, R=1, S=1, stride=1, pad=0):
    return (dtype, None, None, None, _P, _P, _P, ldres, None, None, _P, N, H, W, Cin, ldx, P, Q, Cout, ldy, R, S, stride, pad, None)


def _cat_relu_bits(dtype=1, lda=64, K1=64, ldx=64, K2=64, M=64, Cout=128, ldy=128):
    return (dtype, None, lda, K1, None, ldx, K2, None, _P, None, _P, M, Cout, ldy, None)


def _cat_bias(dtype=1, lda=64, K1=64, ldx=64, K2=64, M=64, Cout=128, ldy=128):
    return (dtype, None, lda, K1, None, ldx, K2, None, None, None, M, Cout, ldy, None)


def _dgrad_bn_cat(dtype=1, ldg=64, K1=64, lda=64, K2=64, M=64, Cout=128, ldy=128):
    return (dtype, None, ldg, K1, None, lda, K2, None, None, None, _P, _P, _P, _P, _P, M, Cout, ldy, None)


def _dgrad_bn_add(dtype=1, lda=64, K=64, ldt=128, M=64, Cout=128, ldy=128):
    return (dtype, None, lda, K, None, None, _P, ldt, None, _P, _P, _P, _P, _P, M, Cout, ldy, None)


def _s2class(dtype=1, add=None, N=1, Hdy=4, Wdy=4, K=64, ldx=64, Hout=8, Wout=8, C=64, ldy=64, ldadd=64, ph=0, pw=0, add_h=0, add_w=0):
    return (dtype, None, None, None, add, None, None, None, None, None, N, Hdy, Wdy, K, ldx, Hout, Wout, C, ldy, ldadd, ph, pw,
            add_h, add_w, None)


def _linear_gelu(dtype=1, act=1, y2=None, M=64, K=64, N=64):
    return (dtype, act, None, None, None, None, None, y2, M, K, N, None)


def _gemm_batched(dtype=1, M=64, N=64, K=64, ldx=64, ldw=64, ldy=64, outer=1, inner=1):
    return (dtype, None, None, None, M, N, K, ldx, ldw, ldy, outer, inner, 0, 0, 0, 0, 0, 0, 0, None)


def _gemm_tn_batched(dtype=1, M=64, Na=64, Nb=64, lda=64, ldb=64, ldo=64, outer=1, inner=1):
    return (dtype, None, None, None, M, Na, Nb, lda, ldb, ldo, outer, inner, 0, 0, 0, 0, 0, 0, None)


def _wgrad(dtype=1, N=1, H=8, W=8, Cin=64, ldx=64, P=8, Q=8, Cout=64, lddy=64, R=1, S=1, stride=1, pad=0, workspace=None,
           workspace_floats=0):
    return (dtype, None, None, None, None, N, H, W, Cin, ldx, P, Q, Cout, lddy, R, S, stride, pad, workspace, workspace_floats, None)


_CONV_HOST_REJECTIONS = [
    ("nkb_conv_gemm", _conv_gemm(dtype=7), b"conv_gemm: bad dtype 7"),
    ("nkb_conv_gemm", _conv_gemm(ldx=68), b"ldx=68"),
    ("nkb_conv_gemm", _conv_gemm(R=33), b"33x1 filter exceeds"),
    ("nkb_conv_gemm", _conv_gemm(N=_BIG, ldx=64), b"conv_gemm: operand exceeds the 4 GiB"),
    ("nkb_conv_gemm", _conv_gemm(N=4096, H=64, W=64, P=128, Q=128, ldy=64), b"conv_gemm: tensor exceeds 2^31"),
    ("nkb_conv_gemm", _conv_gemm(add_bits=_P), b"conv_gemm: add_bits needs a full-grid add"),
    ("nkb_conv_gemm", _conv_gemm(add=_P, ldadd=60, add_bits=_P), b"conv_gemm: add_bits needs a full-grid add"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(dtype=7), b"conv_dgrad_bn: bad dtype 7"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(Cout=60), b"conv_dgrad_bn: Cin=64 must be a multiple of 64, Cout=60"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(stride=3), b"conv_dgrad_bn: stride 3"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(S=33), b"conv_dgrad_bn: filter too large"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(N=_BIG), b"conv_dgrad_bn: operand exceeds the addressing range"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(scale=None), b"conv_dgrad_bn: the recomputed-mask form"),
    ("nkb_conv_dgrad_bn", _dgrad_bn(relu_bits=_P, add=_P, ldadd=60), b"conv_dgrad_bn: bad add operand (ldadd=60)"),
    ("nkb_conv_affine_residual", _affine_residual(Cout=64, ldy=64), b"conv_affine_residual: bf16 only, Cout=64"),
    ("nkb_conv_affine_residual", _affine_residual(dtype=0), b"conv_affine_residual: bf16 only"),
    ("nkb_conv_affine_residual", _affine_residual(stride=4), b"conv_affine_residual: stride 4"),
    ("nkb_conv_affine_residual", _affine_residual(N=_BIG), b"conv_affine_residual: operand exceeds"),
    ("nkb_conv_cat_relu_bits", _cat_relu_bits(K2=0), b"conv_cat_relu_bits: bf16, Cout=128 > 64 and % 8, K1=64 / K2=0"),
    ("nkb_conv_cat_relu_bits", _cat_relu_bits(M=1 << 26), b"conv_cat_relu_bits: operand too large"),
    ("nkb_conv_cat_bias", _cat_bias(K1=32), b"conv_cat_bias: bf16, Cout=128 % 8, K1=32"),
    ("nkb_conv_cat_bias", _cat_bias(M=1 << 26), b"conv_cat_bias: operand too large"),
    ("nkb_conv_dgrad_bn_cat", _dgrad_bn_cat(dtype=7), b"conv_dgrad_bn_cat: bad dtype 7"),
    ("nkb_conv_dgrad_bn_cat", _dgrad_bn_cat(K1=96), b"conv_dgrad_bn_cat: K1=96"),
    ("nkb_conv_dgrad_bn_cat", _dgrad_bn_cat(M=1 << 26), b"conv_dgrad_bn_cat: operand exceeds"),
    ("nkb_conv_dgrad_bn_add", _dgrad_bn_add(dtype=7), b"conv_dgrad_bn_add: bad dtype 7"),
    ("nkb_conv_dgrad_bn_add", _dgrad_bn_add(ldt=100), b"ldt=100 of 8"),
    ("nkb_conv_dgrad_bn_add", _dgrad_bn_add(M=1 << 26), b"conv_dgrad_bn_add: operand exceeds"),
    ("nkb_conv_dgrad_s2class", _s2class(dtype=7), b"conv_dgrad_s2class: bad dtype 7"),
    ("nkb_conv_dgrad_s2class", _s2class(ph=2), b"conv_dgrad_s2class: unsupported K=64 ldx=64 C=64 ldy=64 class (2,0)"),
    ("nkb_conv_dgrad_s2class", _s2class(N=_BIG), b"conv_dgrad_s2class: operand exceeds"),
    ("nkb_conv_dgrad_s2class", _s2class(add=_P, add_h=3, add_w=4), b"conv_dgrad_s2class: sub-grid add must be"),
    ("nkb_linear_residual_scaled", (1, None, None, None, None, _P, 1, None, 64, 64, 64, None), b"linear_residual_scaled: needs add"),
    ("nkb_linear_gelu", _linear_gelu(act=6), b"linear_gelu: unsupported dtype/act/shape (K=64 N=64)"),
    ("nkb_linear_gelu", _linear_gelu(act=5), b"linear_gelu: act 5 needs y2"),
    ("nkb_linear_gelu", _linear_gelu(M=1 << 26), b"linear_gelu: operand exceeds"),
    ("nkb_gemm_batched", _gemm_batched(dtype=7), b"gemm_batched: bad dtype 7"),
    ("nkb_gemm_batched", _gemm_batched(outer=300, inner=300), b"gemm_batched: K=64 must be a multiple of 64"),
    ("nkb_gemm_tn_batched", _gemm_tn_batched(dtype=7), b"gemm_tn_batched: bad dtype 7"),
    ("nkb_gemm_tn_batched", _gemm_tn_batched(Na=72), b"lda >= roundup(Na=72)"),
    ("nkb_conv_wgrad", _wgrad(dtype=7), b"conv_wgrad: bad dtype 7"),
    ("nkb_conv_wgrad", _wgrad(Cout=72), b"lddy >= roundup(Cout=72)"),
    ("nkb_conv_wgrad", _wgrad(N=_BIG), b"conv_wgrad: tensor exceeds 2^31"),
    ("nkb_conv_wgrad", _wgrad(workspace=_P, workspace_floats=1), b"conv_wgrad: workspace of 1 floats given, 4096 needed"),
    ("nkb_conv_wgrad_assign", _wgrad(), b"conv_wgrad_assign: needs the slab workspace"),
    ("nkb_conv_wgrad_assign", _wgrad(workspace=_P, workspace_floats=1), b"conv_wgrad: workspace of 1 floats given, 4096 needed"),
    ("nkb_stem_conv", (7, None, None, None, None, 1, 32, 32, 64, 64, None), b"stem_conv: bad dtype 7"),
    ("nkb_stem_conv", (1, None, None, None, None, 1 << 14, 512, 512, 64, 64, None), b"stem_conv: image batch exceeds"),
    ("nkb_stem_wgrad", (7, None, None, None, 1, 32, 32, 64, 64, None, 0, None), b"stem_wgrad: bad dtype 7"),
    ("nkb_stem_wgrad", (1, None, None, None, 1, 32, 32, 64, 60, None, 0, None), b"stem_wgrad: bad lddy=60"),
    ("nkb_stem_wgrad", (1, None, None, None, 1, 32, 32, 64, 64, _P, 1, None), b"stem_wgrad: workspace too small"),
]


def test_argument_validation_without_gpu():
    """Entry points validate geometry on the host before any launch (error text through nkb_last_error)."""
    lib = hip.load()
    rc = lib.nkb_conv_gemm(1, 0, None, None, None, None, None, None, 1, 8, 8, 48, 48, 8, 8, 64, 64, 0, 1, 1, 1, 0, 0, 0, 0, 0, None, None)
    assert rc != 0 and b"Cin=48" in lib.nkb_last_error()
    rc = lib.nkb_conv_gemm(1, 0, None, None, None, None, None, None, 1, 8, 8, 64, 64, 8, 8, 64, 64, 0, 3, 3, 3, 1, 0, 0, 0, 0, None, None)
    assert rc != 0 and b"stride" in lib.nkb_last_error()
    rc = lib.nkb_bn_apply(1, None, None, None, None, None, 10, 12, 0, None, None, None, None)
    assert rc != 0 and b"C=12" in lib.nkb_last_error()
    for name, args, text in _CONV_HOST_REJECTIONS:
        rc = getattr(lib, name)(*args)
        assert rc != 0 and text in lib.nkb_last_error(), (name, args, rc, lib.nkb_last_error())


def test_binding_arity_matches_header():
    """Every ctypes signature in hip._SIGS has as many arguments as the prototype in include/nkbhip.h (a changed entry point
    whose binding was not updated would otherwise corrupt the call's argument registers silently)."""
    text = (ROOT / "include" / "nkbhip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert len(protos) >= 50
    for name, (_, argtypes) in hip._SIGS.items():
        params = protos[name].strip()
        n = 0 if params in ("", "void") else len([a for a in params.split(",") if a.strip()])
        assert n == len(argtypes), f"{name}: header has {n} parameters, binding {len(argtypes)}"


def test_plan_dispatch_table_is_current_and_validates_entries():
    """csrc/plan_dispatch.inc (the typed call table behind nkb_plan_run) is what scripts/gen_plan_dispatch.py generates from the
    binding's signature table; the library's table agrees with the binding name by name; a table walk on the host rejects a
    bad function id / argument count before calling anything, validates an entry's geometry through the entry point itself and
    reports the failing index."""
    import subprocess
    import sys
    assert subprocess.run([sys.executable, str(ROOT / "scripts" / "gen_plan_dispatch.py"), "--check"]).returncode == 0, \
        "plan_dispatch.inc is stale: run python scripts/gen_plan_dispatch.py and rebuild"
    lib = hip.load()
    ids = hip._plan_fn_ids()
    recordable = {n for n, (res, _) in hip._SIGS.items() if res is ctypes.c_int and n not in hip._PURE}
    assert set(ids) == recordable and lib.nkb_plan_fn_count() == len(ids)
    failed = ctypes.c_int(-1)
    assert lib.nkb_plan_run(None, 0, ctypes.byref(failed)) == 0
    tab = (hip._PlanEntry * 3)()
    # entry 0: a well-formed nkb_bn_apply whose C = 12 the entry point itself refuses (host-side validation, no launch)
    tab[0].fn, tab[0].nargs = ids["nkb_bn_apply"], len(hip._SIGS["nkb_bn_apply"][1])
    tab[0].a[0].i, tab[0].a[6].i, tab[0].a[7].i = 1, 10, 12
    assert lib.nkb_plan_run(tab, 1, ctypes.byref(failed)) != 0 and failed.value == 0 and b"C=12" in lib.nkb_last_error()
    tab[0].fn, tab[0].nargs = lib.nkb_plan_fn_count() + 5, 2
    assert lib.nkb_plan_run(tab, 1, ctypes.byref(failed)) != 0 and b"bad function id" in lib.nkb_last_error()
    tab[0].fn, tab[0].nargs = ids["nkb_bn_apply"], 3            # wrong argument count for that function
    assert lib.nkb_plan_run(tab, 1, ctypes.byref(failed)) != 0 and failed.value == 0
    tab[0].fn = -77
    assert lib.nkb_plan_run(tab, 1, ctypes.byref(failed)) != 0 and b"unknown operation" in lib.nkb_last_error()
