"""The C-ABI shared library loads (no GPU needed) and exports exactly the symbols include/nkbhip.h declares."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from nkb_classification import cabi, hip

ROOT = Path(__file__).resolve().parents[1]
vp, i32, i64, f32, sz, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t, ctypes.c_ulonglong


def _declared():
    text = (ROOT / "include" / "nkbhip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(", text)))


def _same(row, restype, argtypes):
    """A signature row equals the literal one class by class (`is`: hip.record_end sorts arguments by class identity)."""
    return row[0] is restype and len(row[1]) == len(argtypes) and all(a is b for a, b in zip(row[1], argtypes))


# ---- the header parser, on literal declarations (independent of the real header) ------------------------------------------
_DECLS = """
/* a block comment with a prototype inside: int nkb_ghost(int a); */
#ifndef X_H
#define X_H
#define NKB_TWO_LINES(a) \\
    int nkb_macro_body(a);
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t* nkb_stream_t; /* hipStream_t */
typedef union { void* p; long long i; float f; } Arg;
typedef struct { int fn; int nargs; Arg a[32]; } Entry;
struct Opaque;
enum Counter { COUNTER_A = 0, /* first */ COUNTER_B = 1, COUNTER_C, COUNTER_TEN = 0x0a, COUNTER_ELEVEN };
int nkb_three_lines(int dtype, const void* x,   /* the input */
                    // a line comment between parameters: float* ghost,
                    float* y, long long rows,
                    nkb_stream_t stream);
int nkb_no_args(void);
const char* nkb_text(void);
void nkb_nothing(int on);
size_t nkb_by_value(unsigned long long seed, size_t bytes, long long n, float p);
long long nkb_pointers(const unsigned char* bits, int* out, double* ms, const long long* jobs, unsigned char *mask, int);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_literal_declarations():
    protos = cabi.parse(_DECLS)
    assert list(protos) == ["nkb_three_lines", "nkb_no_args", "nkb_text", "nkb_nothing", "nkb_by_value", "nkb_pointers"]
    p = protos["nkb_three_lines"]
    assert _same(p[:2], i32, [i32, vp, vp, i64, vp])
    assert (p.ret, p.params) == ("int", ["int", "const void*", "float*", "long long", "nkb_stream_t"])
    assert _same(protos["nkb_no_args"][:2], i32, []) and protos["nkb_no_args"].params == []
    assert _same(protos["nkb_text"][:2], ctypes.c_char_p, [])
    assert _same(protos["nkb_nothing"][:2], None, [i32]) and protos["nkb_nothing"].ret == "void"
    p = protos["nkb_by_value"]
    assert _same(p[:2], sz, [u64, sz, i64, f32]) and p.params == ["unsigned long long", "size_t", "long long", "float"]
    p = protos["nkb_pointers"]
    assert _same(p[:2], i64, [vp, vp, vp, vp, vp, i32])
    assert p.params == ["const unsigned char*", "int*", "double*", "const long long*", "unsigned char*", "int"]
    assert cabi.parse_enum(_DECLS, "Counter") == {"COUNTER_A": 0, "COUNTER_B": 1, "COUNTER_C": 2, "COUNTER_TEN": 10, "COUNTER_ELEVEN": 11}
    with pytest.raises(ValueError, match="Missing"):
        cabi.parse_enum(_DECLS, "Missing")


@pytest.mark.parametrize("decl", ["int nkb_odd(int a, double x, nkb_stream_t stream);", "int nkb_odd(hipStream_t stream);",
                                  "int nkb_odd(unsigned n);", "int nkb_odd(float mean[3]);", "double nkb_odd(int a);",
                                  "float* nkb_odd(int a);", "int nkb_odd(NkbPlanArg a);"])
def test_parser_refuses_what_it_does_not_know(decl):
    """A by-value type outside the ABI's vocabulary is an error that names the function, never a guess."""
    with pytest.raises(ValueError, match="nkb_odd"):
        cabi.parse("int nkb_fine(int a);\n" + decl)


def test_missing_header_is_a_loud_error(monkeypatch, tmp_path):
    monkeypatch.setattr(cabi, "HEADER", tmp_path / "nkbhip.h")
    with pytest.raises(RuntimeError, match="nkbhip.h"):
        cabi.header_text()


# ---- the derived binding against literals from the hand-written table it replaced ------------------------------------------
_PINNED = {
    "nkb_dropout": (i32, [i32, i32, vp, vp, vp, vp, i64, f32, u64, vp]),
    "nkb_bn_backward": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, sz, vp]),
    "nkb_layernorm": (i32, [i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, f32, vp, vp, vp, i32, vp, i32, vp, vp]),
    "nkb_optim_step": (i32, [i32, vp, vp, vp, vp, vp, i64] + [f32] * 10 + [vp, vp]),
    "nkb_last_error": (ctypes.c_char_p, []),
    "nkb_convp_config": (None, [i32, i32]),
    "nkb_bn_stats_floats": (sz, [i32, i32]),
    "nkb_conv_gemm": (i32, [i32, i32, vp, vp, vp, vp, vp, vp] + [i32] * 18 + [vp, vp]),
    "nkb_conv1p_tiles": (i32, [i32, i64, i32, i32, i32, i32]),
    "nkb_image_prep": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, f32, vp]),
    "nkb_gemm_batched": (i32, [i32, vp, vp, vp] + [i32] * 8 + [i64] * 6 + [i32, vp]),
    "nkb_kernel_launches": (i64, [i32, i32]),
    "nkb_plan_run": (i32, [vp, i32, vp]),
}


@pytest.mark.parametrize("name", sorted(_PINNED))
def test_derived_signature_equals_pinned_literal(name):
    assert len(_PINNED["nkb_layernorm"][1]) == 26
    assert _same(hip._SIGS[name], *_PINNED[name]), (name, hip._SIGS[name])


def test_pure_is_declared_without_a_stream():
    """hip._PURE (called, never recorded into a launch plan) = the entry points whose prototype has no nkb_stream_t parameter."""
    for name in ("nkb_stem3_tiles", "nkb_gemm8p_config", "nkb_plan_run", "nkb_kernel_name", "nkb_bn_stats_floats", "nkb_last_error",
                 "nkb_conv_last_instance", "nkb_wgrad_last_kernel"):
        assert name in hip._PURE, name
    for name in ("nkb_stem3_conv", "nkb_bn_apply", "nkb_dropout", "nkb_optim_step", "nkb_fp8_scale_update"):
        assert name not in hip._PURE, name
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "nkbhip.h").read_text(), flags=re.S)
    protos = dict(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert hip._PURE == frozenset(n for n, params in protos.items() if "nkb_stream_t" not in params)
    assert isinstance(hip._PURE, frozenset) and len(hip._PURE) == 45 and len(hip._SIGS) == 125


_LAUNCH_COUNTERS = {"gemm8p": 0, "wgrad8p": 1, "wgrad3x3": 2, "wgrad8f": 3, "gram_conv": 4, "gram_bn_apply": 5, "convp": 6, "conv1p": 7,
                    "stemp": 8, "gramr": 9, "wgradr": 10, "gemm8p_ragged": 11, "gemm_fp8": 12, "dwconv": 13, "layer_scale": 14,
                    "stem3": 15, "avgpool2": 16}


def test_launch_counter_names_and_numbers():
    """The string keys of hip.kernel_launches come from enum NkbLaunchCounter of the header; numbers are part of the ABI."""
    enum = cabi.parse_enum(cabi.header_text(), "NkbLaunchCounter")
    assert {k[len("NKB_LAUNCH_"):].lower(): v for k, v in enum.items()} == _LAUNCH_COUNTERS
    assert all(k.startswith("NKB_LAUNCH_") for k in enum)
    for name in _LAUNCH_COUNTERS:
        assert hip.kernel_launches(name) >= 0, name
    with pytest.raises(KeyError):
        hip.kernel_launches("no_such_family")


def _dynamic_exports():
    """Defined dynamic symbols of libnkbhip.so (names only), read with nm or ROCm's llvm-readelf; no tool is a failure."""
    lib = str(hip.lib_path())
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    readelf = shutil.which("llvm-readelf") or shutil.which("llvm-readelf", path="/opt/rocm/llvm/bin") or shutil.which("readelf")
    assert readelf, "neither nm nor llvm-readelf / readelf found: cannot list the exports of libnkbhip.so"
    out = subprocess.run([readelf, "--dyn-syms", "-W", lib], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) >= 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def test_unmangled_exports_are_exactly_the_header():
    """Both directions: nothing declared is missing from the library, and no internal helper leaks out as an unmangled nkb_*
    symbol (an `extern "C"` helper outside the header is an ABI nobody described)."""
    exported = {s for s in _dynamic_exports() if s.startswith("nkb_")}
    assert len(exported) >= 100
    declared = set(cabi.parse(cabi.header_text()))
    assert exported - declared == set(), f"exported but not declared in include/nkbhip.h: {sorted(exported - declared)}"
    assert declared - exported == set(), f"declared in include/nkbhip.h but not exported: {sorted(declared - exported)}"
    assert declared == set(_declared())


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
    """Every ctypes signature in hip._SIGS (derived from include/nkbhip.h by nkb_classification/cabi.py) has as many arguments as
    this independent regex count of the prototype's parameters: a check of the parser, which splits statements its own way."""
    text = (ROOT / "include" / "nkbhip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(nkb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert len(protos) >= 50
    assert set(protos) == set(hip._SIGS)
    for name, (_, argtypes) in hip._SIGS.items():
        params = protos[name].strip()
        n = 0 if params in ("", "void") else len([a for a in params.split(",") if a.strip()])
        assert n == len(argtypes), f"{name}: header has {n} parameters, binding {len(argtypes)}"


def test_plan_dispatch_table_is_current_and_validates_entries():
    """csrc/plan_dispatch.inc (the typed call table behind nkb_plan_run) is what scripts/gen_plan_dispatch.py generates from the
    binding's signature table; the library's table agrees with the binding name by name; a table walk on the host rejects a
    bad function id / argument count before calling anything, validates an entry's geometry through the entry point itself and
    reports the failing index."""
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
