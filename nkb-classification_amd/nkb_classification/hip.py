"""ctypes binding of libnkbhip.so (include/nkbhip.h) — the only compute backend of this package.

There is deliberately no CPU or eager-torch fallback: if the shared library is missing or a call
fails, the caller gets a RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

from . import cabi

F32, BF16 = 0, 1
_TORCH_DT = {torch.float32: F32, torch.bfloat16: BF16}

_LIB = None
_LIB_PATH = Path(__file__).resolve().parents[1] / "lib" / "libnkbhip.so"

# The binding is read off include/nkbhip.h, the header the kernel sources are compiled against (cabi.py).
_HEADER = cabi.header_text()
_PROTOS = cabi.parse(_HEADER)
_SIGS = {name: (p.restype, p.argtypes) for name, p in _PROTOS.items()}      # {entry point: (ctypes restype, [ctypes argtypes])}


def lib_path() -> Path:
    return Path(os.environ.get("NKBHIP_LIB", _LIB_PATH))


def load():
    """Load libnkbhip.so once; raise loudly when it is absent (no fallback exists)."""
    global _LIB
    if _REC is not None:
        return _REC_LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not path.exists():
        raise RuntimeError(
            f"libnkbhip.so not found at {path}: build it with `make -C nkb-classification_amd/csrc` "
            "(or __graft_entry__.build()). This package has no CPU / eager fallback."
        )
    lib = C.CDLL(str(path))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def exported_symbols():
    return sorted(_SIGS)


# ---- launch plans --------------------------------------------------------------------------------------------------------
# One train step is ~600 kernel launches, each reached through a few layers of Python (geometry dicts, workspace lookups,
# pointer extraction, ctypes marshalling): 17 ms of host time per ResNet-50 step against 21 ms of GPU time (BENCH_r01).  All
# of it is a pure function of (model, shapes, mode): every buffer lives in the persistent workspace / parameter arena, so the
# C-ABI calls of one step can be RECORDED once — function pointer + argument tuple + the stream / event operations between
# them — and replayed by a flat loop.  What changes from step to step is patched in: pointers into the caller's tensors
# (input images, logits, logits gradient) and dropout seeds.
_REC = None            # list of plan entries while recording
_REC_LIB = None
# entry points that enqueue nothing (declared without a stream parameter): queries and switches, called but never recorded
_PURE = frozenset(name for name, p in _PROTOS.items() if cabi.STREAM not in p.params)


class Seed(int):
    """A dropout seed drawn from torch's host generator; a recorded plan draws a fresh one at every replay."""


def fresh_seed() -> "Seed":
    return Seed(int(torch.randint(0, 2 ** 62, (1,)).item()))


class _RecLib:
    def __getattr__(self, name):
        fn = getattr(_LIB, name)
        if name in _PURE:
            return fn

        def call(*args):
            _REC.append(["call", fn, name, list(args)])
            return fn(*args)
        return call


# The replay itself runs in C (csrc/plan.hip: nkb_plan_run walks a flat table of {function id, arguments}); Python only
# patches the few per-step values and steps from segment to segment — a segment ends where a Python-side operation sits
# between launches (the DDP bucket hooks, a counter bump).  NKB_PLAN_C=0 keeps the old per-entry ctypes loop (A/B, debugging).
_PLAN_C = os.environ.get("NKB_PLAN_C", "1") != "0"
_PLAN_MAX_ARGS = 32
OP_EVENT_RECORD, OP_STREAM_WAIT_EVENT, OP_MEMSET = -1, -2, -3


class _PlanArg(C.Union):
    _fields_ = [("p", C.c_void_p), ("i", C.c_longlong), ("f", C.c_float)]


class _PlanEntry(C.Structure):
    _fields_ = [("fn", C.c_int), ("nargs", C.c_int), ("a", _PlanArg * _PLAN_MAX_ARGS)]


_PLAN_FN = None        # {entry point name: function id of csrc/plan_dispatch.inc}


def _plan_fn_ids():
    global _PLAN_FN
    if _PLAN_FN is None:
        lib = _LIB if _LIB is not None else load()
        if lib.nkb_plan_max_args() != _PLAN_MAX_ARGS or lib.nkb_plan_entry_bytes() != C.sizeof(_PlanEntry):
            raise RuntimeError("nkbhip: NkbPlanEntry layout of libnkbhip.so differs from the binding's (rebuild the library)")
        ids = {}
        for k in range(lib.nkb_plan_fn_count()):
            name = lib.nkb_plan_fn_name(k).decode()
            if name not in _SIGS or lib.nkb_plan_fn_args(k) != len(_SIGS[name][1]):
                raise RuntimeError(f"nkbhip: plan dispatch table is stale for {name} (python scripts/gen_plan_dispatch.py; rebuild)")
            ids[name] = k
        _PLAN_FN = ids
    return _PLAN_FN


class Plan:
    __slots__ = ("segments", "dyn_names", "keep", "entries")

    def __init__(self, segments, dyn_names, keep, entries):
        # entries: number of recorded operations (diagnostics); keep: the torch events / streams / tensors the table points at
        self.segments, self.dyn_names, self.keep, self.entries = segments, dyn_names, keep, entries


_REC_MAIN = None       # the compute stream of the step being recorded


def record_begin():
    global _REC, _REC_LIB, _REC_MAIN
    load()
    _REC_MAIN = torch.cuda.current_stream()
    _REC, _REC_LIB = [], _RecLib()


def record_abort():
    global _REC
    _REC = None


def record_end(dynamic: dict) -> Plan:
    """dynamic: {name: tensor} — every recorded pointer argument that points into one of these tensors becomes a slot that
    replay() fills from the tensor passed under the same name."""
    global _REC
    rec, _REC = _REC, None
    ranges = [(name, t.data_ptr(), t.data_ptr() + max(t.numel() * t.element_size(), 1)) for name, t in dynamic.items()]
    ids = _plan_fn_ids() if _PLAN_C else {}
    segments, keep = [], []
    cur = []            # entries of the C segment being built: (fn id, [(kind, value)], name, patches)

    def flush():
        if not cur:
            return
        arr = (_PlanEntry * len(cur))()
        patches, names = [], []
        for k, (fid, vals, name, pt) in enumerate(cur):
            e = arr[k]
            e.fn, e.nargs = fid, len(vals)
            for ai, (kind, v) in enumerate(vals):
                if kind == "f":
                    e.a[ai].f = float(v)
                elif kind == "p":
                    e.a[ai].p = v
                else:
                    e.a[ai].i = int(v)
            names.append(name)
            patches += [(k, ai, dn, off) for ai, dn, off in pt]
        segments.append((0, arr, len(cur), tuple(patches), tuple(names)))
        cur.clear()

    for e in rec:
        if e[0] == "py":
            flush()
            segments.append((2, e[1], None, None, None))
            continue
        if e[0] == "op":
            _, code, vals, alive = e
            keep.append(alive)
            if _PLAN_C:
                kinds = ("p", "i", "p") if code == OP_MEMSET else ("p", "p")
                cur.append((code, list(zip(kinds, vals)), "stream operation %d" % code, ()))
            else:
                segments.append((2, _op_closure(code, alive), None, None, None))
            continue
        _, fn, name, args = e
        patches = []
        for i, a in enumerate(args):
            if isinstance(a, Seed):
                patches.append((i, None, 0))
            elif isinstance(a, int) and a >= (1 << 32):
                for dn, lo, hi in ranges:
                    if lo <= a < hi:
                        patches.append((i, dn, a - lo))
                        break
        if name in ids and len(args) <= _PLAN_MAX_ARGS:
            types = _SIGS[name][1]
            vals = [("f" if t is C.c_float else ("p" if t is C.c_void_p else "i"), (0 if a is None and t is not C.c_void_p else a)) for t, a in zip(types, args)]
            cur.append((ids[name], vals, name, patches))
        else:
            flush()
            segments.append((1, fn, list(args), tuple(patches), name))
    flush()
    return Plan(segments, tuple(dynamic), keep, len(rec))


def _op_closure(code, alive):
    """Python form of a recorded stream operation (NKB_PLAN_C=0)."""
    if code == OP_EVENT_RECORD:
        ev, st = alive
        return lambda: ev.record(st)
    if code == OP_STREAM_WAIT_EVENT:
        ev, st = alive
        return lambda: st.wait_event(ev)
    t, st = alive

    def memset():
        with torch.cuda.stream(st):
            t.zero_()
    return memset


_FAILED = C.c_int(0)


def replay(plan: Plan, dynamic: dict):
    base = {name: t.data_ptr() for name, t in dynamic.items()}
    for kind, a, b, patches, names in plan.segments:
        if kind == 0:
            for ei, ai, dn, off in patches:
                a[ei].a[ai].i = base[dn] + off if dn is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            if _LIB.nkb_plan_run(a, b, C.byref(_FAILED)):
                raise RuntimeError(f"nkbhip {names[_FAILED.value]} failed during plan replay: {_LIB.nkb_last_error().decode()}")
        elif kind == 1:
            for i, dn, off in patches:
                b[i] = base[dn] + off if dn is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            if a(*b):
                raise RuntimeError(f"nkbhip {names} failed during plan replay: {_LIB.nkb_last_error().decode()}")
        else:
            a()


# ---- stream operations between launches, recordable (a host_op closure would end the C segment) --------------------------------
def event_record(ev: "torch.cuda.Event", st: "torch.cuda.Stream"):
    ev.record(st)
    if _REC is not None:
        _REC.append(["op", OP_EVENT_RECORD, (ev.cuda_event, st.cuda_stream), (ev, st)])


def stream_wait_event(st: "torch.cuda.Stream", ev: "torch.cuda.Event"):
    st.wait_event(ev)
    if _REC is not None and ev.cuda_event:          # (an event that was never recorded: torch's wait is a no-op, so is the plan's)
        _REC.append(["op", OP_STREAM_WAIT_EVENT, (st.cuda_stream, ev.cuda_event), (ev, st)])


def stream_wait_stream(st: "torch.cuda.Stream", other: "torch.cuda.Stream"):
    """st waits for everything enqueued on `other` so far (torch's Stream.wait_stream with a recordable event)."""
    ev = torch.cuda.Event()
    event_record(ev, other)
    stream_wait_event(st, ev)


def zero_(t: torch.Tensor):
    """t.zero_() on the current stream, as a recordable memset."""
    t.zero_()
    if _REC is not None:
        if not t.is_contiguous():
            raise RuntimeError("hip.zero_: recorded memsets need a contiguous tensor")
        st = torch.cuda.current_stream()
        _REC.append(["op", OP_MEMSET, (t.data_ptr(), t.numel() * t.element_size(), st.cuda_stream), (t, st)])


def recording() -> bool:
    return _REC is not None


def host_op(fn):
    """A torch-side operation between launches (memset, counter bump, stream / event call): run now, and re-run at this
    point of the sequence when the plan is replayed — on the stream that is current now."""
    global _REC
    if _REC is not None:
        cur = torch.cuda.current_stream()
        if cur == _REC_MAIN:
            _REC.append(["py", fn])
        else:
            def on_stream(fn=fn, cur=cur):
                with torch.cuda.stream(cur):
                    fn()
            _REC.append(["py", on_stream])
        # fn itself is what the plan re-runs: library calls it makes now (the bf16 gradient exchange of parallel.GradReducer
        # casts and sums through libnkbhip on temporaries) must not ALSO be recorded as table entries — replayed, they would
        # run a second time on pointers that were freed when fn returned
        rec, _REC = _REC, None
        before = _device_allocs()
        try:
            fn()
        finally:
            _REC = rec
            # what fn allocated is fn's own business (it runs again, allocating afresh, at every replay): the model's "the recorded
            # run allocated nothing" test (model.py) must not count it, or a plan with a bucket hook in it would never be kept
            global host_op_allocs
            host_op_allocs += _device_allocs() - before
        return
    fn()


host_op_allocs = 0     # device allocations made inside host_op closures while a plan was being recorded (monotone)


def _device_allocs() -> int:
    if not torch.cuda.is_available():
        return 0
    return int(torch.cuda.memory_stats(torch.cuda.current_device()).get("allocation.all.allocated", 0))


# {"gemm8p": 0, ...}: enum NkbLaunchCounter of the header, NKB_LAUNCH_GEMM8P -> "gemm8p"
_LAUNCH_COUNTERS = {k[len("NKB_LAUNCH_"):].lower(): v for k, v in cabi.parse_enum(_HEADER, "NkbLaunchCounter").items()}


def kernel_launches(which: str, reset: bool = False) -> int:
    """Launch count of a specialised kernel family; `which` is an enumerator of NkbLaunchCounter (include/nkbhip.h, one comment per
    family) without its NKB_LAUNCH_ prefix, in lower case: "gemm8p", "convp", "stem3", ..."""
    idx = _LAUNCH_COUNTERS[which]
    return int(load().nkb_kernel_launches(idx, int(reset)))


def dt(t) -> int:
    d = t if isinstance(t, torch.dtype) else t.dtype
    if d not in _TORCH_DT:
        raise RuntimeError(f"nkbhip: unsupported dtype {d}")
    return _TORCH_DT[d]


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    # the current stream of the CURRENT device: entry points run under torch.cuda.device(<tensor device>) (model._logits,
    # FusedOptimizer.step, train.py's set_device), so this is the stream of the device that holds the operands
    return torch.cuda.current_stream().cuda_stream


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"nkbhip {what} failed (code {rc}): {load().nkb_last_error().decode()}")


def require_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP engine runs on cuda devices only "
                           "(there is no CPU fallback)")


# ------------------------------------------------------------------ thin typed wrappers ----
def conv_gemm(dtype, mode, x, w, y, *, N, H, W, Cin, ldx, P, Q, Cout, ldy, R=1, S=1, stride=1, pad=0, add=None,
              ldadd=0, bias=None, stats=None, relu=False, out_f32=False, add_hw=(0, 0), add_bits=None):
    check(load().nkb_conv_gemm(dtype, mode, ptr(x), ptr(w), ptr(y), ptr(add), ptr(bias), ptr(stats), N, H, W, Cin, ldx,
                               P, Q, Cout, ldy, ldadd, R, S, stride, pad, int(relu), int(out_f32), add_hw[0], add_hw[1],
                               ptr(add_bits), stream()), "conv_gemm")


def stat_tiles(dtype, M, Cout):
    return load().nkb_conv_gemm_stat_tiles(dtype, M, Cout)


def conv_last_instance() -> int:
    """The conv_igemm_kernel instance of the last launch of that family (bit 0 bf16, bit 1 the 64 x 256 tile, bit 2 HALO, bit 3
    grouped walk, bits 4.. the epilogue selector); -1 before any launch."""
    return int(load().nkb_conv_last_instance())


def convp_tiles(dtype, kind, *, N, H, W, Cin, ldx, Cout, ldy, R, S, stride, pad) -> int:
    """Partial-sum rows of the row-balanced 3x3 core for this launch (kind 0 forward, 1 data gradient); 0 = not eligible."""
    return int(load().nkb_convp_tiles(dtype, kind, N, H, W, Cin, ldx, Cout, ldy, R, S, stride, pad))


def convp_config(on: bool = True, tc128: bool = False, c64: bool = True, c64_dgrad: bool = False, conv1p: bool = True, stemp: bool = True,
                 gramr: bool = True):
    """Envelope of the row-resident kernel family (convp / conv1p / stemp / gramr); the defaults are the train step's."""
    load().nkb_convp_config(int(on), int(tc128) | (2 if c64 else 0) | (4 if c64_dgrad else 0) | (0 if conv1p else 16) | (0 if stemp else 32)
                            | (0 if gramr else 64))


_geometry_epoch = 0


def geometry_epoch() -> int:
    """Bumped whenever a setting that sizes grids (and through them stats / slab buffers) changes: runtime.Workspace.generation
    carries it, so launch plans recorded under the old setting are dropped instead of replayed."""
    return _geometry_epoch


def rowres_reserve_cus(cus: int):
    """Data-parallel runs: CUs the row-resident family's backward kernels (convp data gradient, gramr, wgradr) leave to the
    collective.  Changing it after a step has run is allowed: recorded plans are invalidated and the next eager pass re-sizes the
    partial-sum / slab buffers; a stale buffer handed to the library is refused by the launch itself."""
    global _geometry_epoch
    lib = load()
    if int(lib.nkb_rowres_reserved_cus()) != max(0, min(128, int(cus))):
        _geometry_epoch += 1
    lib.nkb_rowres_reserve_cus(int(cus))


def conv1p_tiles(dtype, M, Cin, ldx, Cout, ldy) -> int:
    """Partial-sum rows of conv1p_fwd for this 1x1 shape; 0: not eligible (use conv_gemm)."""
    return int(load().nkb_conv1p_tiles(dtype, M, Cin, ldx, Cout, ldy))


def conv1p_fwd(dtype, x, w, y, stats, *, M, Cin, ldx, Cout, ldy):
    check(load().nkb_conv1p_fwd(dtype, ptr(x), ptr(w), ptr(y), ptr(stats), M, Cin, ldx, Cout, ldy, stream()), "conv1p_fwd")


def convp_fwd(dtype, x, w, y, stats, *, N, H, W, Cin, ldx, Cout, ldy, tiles):
    """tiles: the partial-sum rows `stats` was sized for (convp_tiles at that time); the launch is refused if its grid differs."""
    check(load().nkb_convp_fwd(dtype, ptr(x), ptr(w), ptr(y), ptr(stats), N, H, W, Cin, ldx, Cout, ldy, int(tiles), stream()), "convp_fwd")


def convp_dgrad_bn(dtype, dy, w, g_masked, c, scale, shift, mean, stats, *, N, H, W, Cin, ldx, Cout, ldy, tiles):
    check(load().nkb_convp_dgrad_bn(dtype, ptr(dy), ptr(w), ptr(g_masked), ptr(c), ptr(scale), ptr(shift), ptr(mean), ptr(stats),
                                    N, H, W, Cin, ldx, Cout, ldy, int(tiles), stream()), "convp_dgrad_bn")


def conv_wgrad(dtype, dy, x, dw, *, N, H, W, Cin, ldx, P, Q, Cout, lddy, R=1, S=1, stride=1, pad=0, dbias=None,
               workspace=None, assign=False):
    """workspace: fp32 scratch of at least conv_wgrad_workspace(...) floats -> deterministic two-stage accumulation; None ->
    fp32 atomics.  assign: dw / dbias are overwritten instead of accumulated into (needs the workspace)."""
    fn = load().nkb_conv_wgrad_assign if assign else load().nkb_conv_wgrad
    check(fn(dtype, ptr(dy), ptr(x), ptr(dw), ptr(dbias), N, H, W, Cin, ldx, P, Q, Cout, lddy, R, S, stride, pad,
                                ptr(workspace), workspace.numel() if workspace is not None else 0, stream()), "conv_wgrad")


def conv_wgrad_workspace(dtype, *, N, P, Q, Cin, Cout, R=1, S=1, stride=1, pad=0, has_bias=False) -> int:
    return int(load().nkb_conv_wgrad_workspace_floats(dtype, N, P, Q, Cin, Cout, R, S, stride, pad, int(has_bias)))


def wgrad_last_kernel() -> int:
    """The weight-gradient kernel of the last conv_wgrad / stem_wgrad / gemm_tn_batched launch and the reduce kernel launched last
    (encoding: nkb_wgrad_last_kernel in include/nkbhip.h); -1 before any launch."""
    return int(load().nkb_wgrad_last_kernel())


def stem_wgrad_workspace(dtype, N, H, W, Cout) -> int:
    return int(load().nkb_stem_wgrad_workspace_floats(dtype, N, H, W, Cout))


def bn_finalize(partials, tiles, C_, count, gamma, beta, rm, rv, momentum, eps, training, scale, shift, mean, invstd):
    check(load().nkb_bn_finalize(ptr(partials), tiles, C_, count, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), momentum, eps,
                                 int(training), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), stream()), "bn_finalize")


def bn_apply(dtype, x, res, y, scale, shift, rows, C_, relu, relu_bits=None, res_scale=None, res_shift=None):
    check(load().nkb_bn_apply(dtype, ptr(x), ptr(res), ptr(y), ptr(scale), ptr(shift), rows, C_, int(relu),
                              ptr(relu_bits), ptr(res_scale), ptr(res_shift), stream()), "bn_apply")


def bn_stats_floats(tiles, C_):
    return load().nkb_bn_stats_floats(tiles, C_)


def bn_backward(dtype, dy, x, yact, mean, invstd, gamma, rows, C_, dgamma, dbeta, dx, dy_masked, workspace,
                fscale=None, fshift=None, relu_bits=None):
    check(load().nkb_bn_backward(dtype, ptr(dy), ptr(x), ptr(yact), ptr(relu_bits), ptr(fscale), ptr(fshift), ptr(mean),
                                 ptr(invstd),
                                 ptr(gamma), rows, C_,
                                 ptr(dgamma), ptr(dbeta), ptr(dx), ptr(dy_masked), ptr(workspace), workspace.numel(),
                                 stream()), "bn_backward")


def conv_dgrad_bn(dtype, dy, w, g_masked, c, scale, shift, mean, stats, *, N, H, W, Cin, ldx, P, Q, Cout, ldy, R, S,
                  stride, pad, relu_bits=None, add=None, ldadd=0, add_bits=None, add_hw=(0, 0)):
    check(load().nkb_conv_dgrad_bn(dtype, ptr(dy), ptr(w), ptr(g_masked), ptr(c), ptr(scale), ptr(shift), ptr(mean),
                                   ptr(stats), ptr(relu_bits), ptr(add), ldadd, ptr(add_bits), add_hw[0], add_hw[1],
                                   N, H, W, Cin, ldx, P, Q, Cout, ldy, R, S, stride, pad, stream()),
          "conv_dgrad_bn")


def conv_dgrad_s2class(dtype, dy, w_class, y, add, c, scale, shift, mean, stats, N, Hdy, Wdy, K, ldx, Hout, Wout, C_, ldy,
                       ldadd, ph, pw, add_h=0, add_w=0):
    check(load().nkb_conv_dgrad_s2class(dtype, ptr(dy), ptr(w_class), ptr(y), ptr(add), ptr(c), ptr(scale), ptr(shift),
                                        ptr(mean), ptr(stats), N, Hdy, Wdy, K, ldx, Hout, Wout, C_, ldy, ldadd, ph, pw,
                                        add_h, add_w, stream()), "conv_dgrad_s2class")


def bn_backward_from_stats(dtype, g, x, stats, tiles, mean, invstd, gamma, rows, C_, dgamma, dbeta, dx, sums):
    check(load().nkb_bn_backward_from_stats(dtype, ptr(g), ptr(x), ptr(stats), tiles, ptr(mean), ptr(invstd), ptr(gamma),
                                            rows, C_, ptr(dgamma), ptr(dbeta), ptr(dx), ptr(sums), stream()),
          "bn_backward_from_stats")


def gram_bn_stats(dtype, w, gram, colsum, count, Cin, Cout, gamma, beta, rm, rv, momentum, eps, cov, mu, T, scale, shift, mean, invstd):
    check(load().nkb_gram_bn_stats(dtype, ptr(w), ptr(gram), ptr(colsum), count, Cin, Cout, ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                                   momentum, eps, ptr(cov), ptr(mu), ptr(T), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), stream()),
          "gram_bn_stats")


def bn_apply_gram_ws(rows, C_) -> int:
    return int(load().nkb_bn_apply_gram_workspace_floats(rows, C_))


def bn_apply_gram(dtype, c, y, scale, shift, rows, C_, gram, work):
    check(load().nkb_bn_apply_gram(dtype, ptr(c), ptr(y), ptr(scale), ptr(shift), rows, C_, ptr(gram), ptr(work), work.numel(), stream()),
          "bn_apply_gram")


def conv_affine_residual(dtype, x, w, y, scale, shift, res, ldres, res_scale, res_shift, relu_bits, *, N, H, W, Cin, ldx, P, Q, Cout,
                         ldy, R=1, S=1, stride=1, pad=0):
    check(load().nkb_conv_affine_residual(dtype, ptr(x), ptr(w), ptr(y), ptr(scale), ptr(shift), ptr(res), ldres, ptr(res_scale),
                                          ptr(res_shift), ptr(relu_bits), N, H, W, Cin, ldx, P, Q, Cout, ldy, R, S, stride, pad,
                                          stream()), "conv_affine_residual")


def gram_bn_backward_ws(Cin, Cout) -> int:
    return int(load().nkb_gram_bn_backward_workspace_floats(Cin, Cout))


def gram_bn_backward(dtype, w, R, T, mu, gstats, tiles, count, Cin, Cout, gamma, mean, invstd, dgamma, dbeta, dw, wcat, cbias, coef, q=None):
    check(load().nkb_gram_bn_backward(dtype, ptr(w), ptr(R), ptr(T), ptr(mu), ptr(gstats), tiles, count, Cin, Cout, ptr(gamma), ptr(mean),
                                      ptr(invstd), ptr(dgamma), ptr(dbeta), ptr(dw), ptr(wcat), ptr(q), ptr(cbias), ptr(coef), stream()),
          "gram_bn_backward")


def gram_k1w(dtype, w, k1, Cin, Cout, out):
    check(load().nkb_gram_k1w(dtype, ptr(w), ptr(k1), Cin, Cout, ptr(out), stream()), "gram_k1w")


def conv_dgrad_bn_add(dtype, a, lda, K, q, cbias, t, ldt, g_masked, c_prev, scale, shift, mean, stats, M, Cout, ldy):
    check(load().nkb_conv_dgrad_bn_add(dtype, ptr(a), lda, K, ptr(q), ptr(cbias), ptr(t), ldt, ptr(g_masked), ptr(c_prev), ptr(scale),
                                       ptr(shift), ptr(mean), ptr(stats), M, Cout, ldy, stream()), "conv_dgrad_bn_add")


def conv_dgrad_bn_cat(dtype, g, ldg, K1, a, lda, K2, wcat, cbias, g_masked, c_prev, scale, shift, mean, stats, M, Cout, ldy):
    check(load().nkb_conv_dgrad_bn_cat(dtype, ptr(g), ldg, K1, ptr(a), lda, K2, ptr(wcat), ptr(cbias), ptr(g_masked), ptr(c_prev),
                                       ptr(scale), ptr(shift), ptr(mean), ptr(stats), M, Cout, ldy, stream()), "conv_dgrad_bn_cat")


def gram_fold2(dtype, w1, s1, K1, w2, s2, K2, Cout, out, shift1, shift2, shift_out):
    check(load().nkb_gram_fold2(dtype, ptr(w1), ptr(s1), K1, ptr(w2), ptr(s2), K2, Cout, ptr(out), ptr(shift1), ptr(shift2), ptr(shift_out),
                                stream()), "gram_fold2")


def conv_cat_relu_bits(dtype, a, lda, K1, x, ldx, K2, wf, shift, y, relu_bits, M, Cout, ldy):
    check(load().nkb_conv_cat_relu_bits(dtype, ptr(a), lda, K1, ptr(x), ldx, K2, ptr(wf), ptr(shift), ptr(y), ptr(relu_bits), M, Cout, ldy,
                                        stream()), "conv_cat_relu_bits")


def conv_cat_bias(dtype, a, lda, K1, x, ldx, K2, w, bias, y, M, Cout, ldy):
    check(load().nkb_conv_cat_bias(dtype, ptr(a), lda, K1, ptr(x), ldx, K2, ptr(w), ptr(bias), ptr(y), M, Cout, ldy, stream()), "conv_cat_bias")


def bn_backward_ws(rows, C_):
    return load().nkb_bn_backward_workspace_floats(rows, C_)


def bn_relu_maxpool(dtype, backward, c, scale, shift, mean, invstd, gamma, y_or_g, idx, dc, dgamma, dbeta, work, N, H, W, C_, xsel=None):
    """xsel [N][P][Q][C]: written by the forward call (raw conv output behind every pooled winner), read by the backward call."""
    check(load().nkb_bn_relu_maxpool_sel(dtype, int(backward), ptr(c), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                                         ptr(gamma), ptr(y_or_g), ptr(idx), ptr(dc), ptr(dgamma), ptr(dbeta), ptr(work),
                                         work.numel() if work is not None else 0, ptr(xsel), N, H, W, C_, stream()), "bn_relu_maxpool")


def bn_relu_maxpool_ws(N, H, W, C_) -> int:
    return int(load().nkb_bn_relu_maxpool_workspace_floats(N, H, W, C_))


def maxpool(dtype, backward, src, dst, idx, N, H, W, C_):
    check(load().nkb_maxpool3x3s2(dtype, int(backward), ptr(src), ptr(dst), ptr(idx), N, H, W, C_, stream()), "maxpool")


# enum NkbPoolMode of the header: the passes of nkb_avgpool ({"NKB_POOL_AVG_FWD": 0, ..., "NKB_GRN_PARAM": 6})
_POOL_MODES = cabi.parse_enum(_HEADER, "NkbPoolMode")


def _pool(what, dtype, mode, src, dst, N, HW, C_, in2=None, weight=None, bias=None, sumsq=None, dweight=None, dbias=None, mul=None,
          eps=0.0, workspace=None):
    check(load().nkb_avgpool(dtype, _POOL_MODES[mode], ptr(src), ptr(dst), N, HW, C_, ptr(in2), ptr(weight), ptr(bias), ptr(sumsq),
                             ptr(dweight), ptr(dbias), ptr(mul), eps, ptr(workspace), workspace.numel() if workspace is not None else 0,
                             stream()), what)


def avgpool(dtype, backward, src, dst, N, HW, C_):
    _pool("avgpool", dtype, "NKB_POOL_AVG_BWD" if backward else "NKB_POOL_AVG_FWD", src, dst, N, HW, C_)


def grn_workspace(N, HW, C_) -> int:
    """Floats of fp32 workspace grn_backward / grn_param need: the tables P, Q [N][C] and m [N] (include/nkbhip.h, nkb_avgpool)."""
    return 2 * N * C_ + N


def grn(dtype, u, weight, bias, out, sumsq, N, HW, C_, eps=1e-6, workspace=None):
    """Global response normalisation over [N][HW][C] rows, two launches: sumsq [N][C] fp32 (kept for backward), then
    out = u * (1 + weight * G / mean_c G) + bias.  The forward pass needs no workspace."""
    _pool("grn", dtype, "NKB_GRN_FWD_REDUCE", u, None, N, HW, C_, sumsq=sumsq, eps=eps)
    _pool("grn", dtype, "NKB_GRN_FWD_APPLY", u, out, N, HW, C_, weight=weight, bias=bias, sumsq=sumsq, eps=eps)


def grn_backward(dtype, g, u, weight, sumsq, out, dweight, dbias, N, HW, C_, eps=1e-6, mul=None, workspace=None):
    """out = d(loss)/du (* mul, e.g. the activation derivative in front of the GRN); dweight / dbias are accumulated into unless
    both are None (grn_param makes that launch on its own, on another stream, from the same workspace).  workspace: at least
    grn_workspace(N, HW, C) fp32."""
    _pool("grn_backward", dtype, "NKB_GRN_BWD_REDUCE", g, None, N, HW, C_, in2=u, sumsq=sumsq, eps=eps, workspace=workspace)
    _pool("grn_backward", dtype, "NKB_GRN_BWD_APPLY", g, out, N, HW, C_, in2=u, weight=weight, sumsq=sumsq, mul=mul, eps=eps,
          workspace=workspace)
    if dweight is not None or dbias is not None:
        grn_param(dtype, sumsq, dweight, dbias, N, HW, C_, workspace, eps=eps)


def grn_param(dtype, sumsq, dweight, dbias, N, HW, C_, workspace, eps=1e-6):
    """dweight / dbias += their sums over the images, from the tables grn_backward left in `workspace`."""
    _pool("grn_param", dtype, "NKB_GRN_PARAM", None, None, N, HW, C_, sumsq=sumsq, dweight=dweight, dbias=dbias, eps=eps,
          workspace=workspace)


# enum NkbSeMode of the header: the channel-attention passes of nkb_avgpool ({"NKB_SE_POOL": 16, ..., "NKB_SE_BWD_APPLY": 23})
_SE_MODES = cabi.parse_enum(_HEADER, "NkbSeMode")


def se_workspace(N, C_, rd=0) -> int:
    """Floats of the fp32 block one SE / ECA closing stage keeps (include/nkbhip.h, NkbSeMode): six [N][C] tables cm, s, A, B, dz, ds,
    the vectors S1, S2 [C], C / 4 floats of per-workgroup partial sums, then h, dh [N][rd] (rd = 0 for ECA).  cm, s and h live from
    forward to backward."""
    return 6 * N * C_ + 2 * C_ + C_ // 4 + 2 * N * rd


def _se(what, dtype, mode, N, hw, C_, workspace, src=None, dst=None, in2=None, weight=None, bias=None, sumsq=None, dweight=None,
        dbias=None, mul=None):
    check(load().nkb_avgpool(dtype, _SE_MODES[mode], ptr(src), ptr(dst), N, hw, C_, ptr(in2), ptr(weight), ptr(bias), ptr(sumsq),
                             ptr(dweight), ptr(dbias), ptr(mul), 0.0, ptr(workspace), workspace.numel() if workspace is not None else 0,
                             stream()), what)


def se_forward(dtype, c, short, out, bnvec, workspace, N, HW, C_, w1, b1=None, w2=None, b2=None, bits=None, res_bnvec=None):
    """out = relu((c scale + shift) s[b] + shortcut) in three launches: pool, gate, apply.  w2 is None: ECA with the taps w1, else SE
    (w1 [rd][C], b1, w2 [C][rd], b2, fp32 masters).  bnvec None: eval form on a normalised c.  res_bnvec: the shortcut is a raw
    projection output with these [scale | shift | ...] rows."""
    _se("se_pool", dtype, "NKB_SE_POOL", N, HW, C_, workspace, src=c)
    if w2 is None:
        _se("eca_gate", dtype, "NKB_ECA_GATE", N, w1.numel(), C_, workspace, src=w1, weight=bnvec)
    else:
        _se("se_gate", dtype, "NKB_SE_GATE", N, w1.shape[0], C_, workspace, src=w1, in2=w2, bias=b1, mul=b2, weight=bnvec)
    _se("se_apply", dtype, "NKB_SE_FWD_APPLY", N, HW, C_, workspace, src=c, dst=out, in2=short, weight=bnvec, bias=res_bnvec, sumsq=bits)


def se_backward(dtype, g, c, bits, dc, bnvec, workspace, N, HW, C_, w1, w2=None, dw1=None, db1=None, dw2=None, db2=None, dgamma=None,
                dbeta=None):
    """dc = gradient of the raw closing-convolution output from g, the (unmasked) gradient of the block output, in three launches:
    reduce, gate, apply.  The parameter gradients accumulate (+=); the workspace is the one se_forward filled."""
    _se("se_bwd_reduce", dtype, "NKB_SE_BWD_REDUCE", N, HW, C_, workspace, src=g, in2=c, sumsq=bits)
    if w2 is None:
        _se("eca_bwd_gate", dtype, "NKB_ECA_BWD_GATE", N, w1.numel(), C_, workspace, src=w1, weight=bnvec, dweight=dw1)
    else:
        _se("se_bwd_gate", dtype, "NKB_SE_BWD_GATE", N, w1.shape[0], C_, workspace, src=w1, in2=w2, weight=bnvec, dst=dw1, sumsq=db1,
            dweight=dw2, dbias=db2)
    _se("se_bwd_apply", dtype, "NKB_SE_BWD_APPLY", N, HW, C_, workspace, src=g, dst=dc, in2=c, weight=bnvec, sumsq=bits, dweight=dgamma,
        dbias=dbeta)


def stem_pack(dtype, x, out, N, C_, H, W):
    check(load().nkb_stem_pack(dtype, ptr(x), ptr(out), N, C_, H, W, stream()), "stem_pack")


def stem_wprep(dtype, w, wp, Cout, C_):
    check(load().nkb_stem_wprep(dtype, ptr(w), ptr(wp), Cout, C_, stream()), "stem_wprep")


def stem_weight_cols(dtype) -> int:
    return int(load().nkb_stem_weight_cols(dtype))


def stem_conv(dtype, xp, wp, y, stats, N, H, W, Cout, ldy):
    check(load().nkb_stem_conv(dtype, ptr(xp), ptr(wp), ptr(y), ptr(stats), N, H, W, Cout, ldy, stream()), "stem_conv")


def gramr_workspace(dtype, M, co, ci) -> int:
    """Slab floats of gramr for R[co][ci] = g^T a over M pixels; 0: not eligible (use conv_wgrad(assign=True))."""
    return int(load().nkb_gramr_workspace_floats(dtype, M, co, ci))


def gramr(dtype, g, ldg, a, lda, R, M, co, ci, workspace, assign=True, transposed=False):
    """R = g^T a (assign: overwritten, else accumulated into; transposed: stored [ci][co] = a 1x1 weight gradient with g = the input)."""
    check(load().nkb_gramr(dtype, ptr(g), ldg, ptr(a), lda, ptr(R), M, co, ci, int(assign) | (2 if transposed else 0), ptr(workspace),
                           workspace.numel(), stream()), "gramr")


def stemp_tiles(dtype, N, H, W, Cout) -> int:
    """Partial-sum rows of stemp_conv for this stem; 0: not eligible (use stem_conv)."""
    return int(load().nkb_stemp_tiles(dtype, N, H, W, Cout))


def stemp_conv(dtype, xp, wp, y, stats, N, H, W, Cout, ldy):
    check(load().nkb_stemp_conv(dtype, ptr(xp), ptr(wp), ptr(y), ptr(stats), N, H, W, Cout, ldy, stream()), "stemp_conv")


def stemp_wgrad_workspace(dtype, N, H, W, Cout) -> int:
    """Slab floats of stemp_wgrad; 0: not eligible (use stem_wgrad)."""
    return int(load().nkb_stemp_wgrad_workspace_floats(dtype, N, H, W, Cout))


def stemp_wgrad(dtype, dy, xp, dwp, N, H, W, Cout, lddy, workspace):
    check(load().nkb_stemp_wgrad(dtype, ptr(dy), ptr(xp), ptr(dwp), N, H, W, Cout, lddy, ptr(workspace), workspace.numel(), stream()),
          "stemp_wgrad")


def stem_wgrad(dtype, dy, xp, dwp, N, H, W, Cout, lddy, workspace=None):
    check(load().nkb_stem_wgrad(dtype, ptr(dy), ptr(xp), ptr(dwp), N, H, W, Cout, lddy, ptr(workspace),
                                workspace.numel() if workspace is not None else 0, stream()), "stem_wgrad")


def stem_wfold(dtype, dwp, dw, Cout, C_):
    check(load().nkb_stem_wfold(dtype, ptr(dwp), ptr(dw), Cout, C_, stream()), "stem_wfold")


def im2row(dtype, x, col, N, Cin, H, W, R, S, stride, pad, Kp):
    check(load().nkb_im2row(dtype, ptr(x), ptr(col), N, Cin, H, W, R, S, stride, pad, Kp, stream()), "im2row")


def wprep_multi(dtype, base, jobs, njobs, total_blocks, shadow=None):
    """shadow: optional bf16 mirror of `base` (same element offsets) to read the transposing jobs' sources from."""
    check(load().nkb_wprep_multi(dtype, ptr(base), ptr(jobs), njobs, total_blocks, ptr(shadow), stream()), "wprep_multi")


def wprep_block_elems() -> int:
    return int(load().nkb_wprep_block_elems())


def wprep_job_blocks(A, B, C_, ld, mode) -> int:
    return int(load().nkb_wprep_job_blocks(A, B, C_, ld, mode))


def wprep(dtype, src, dst, A, B, C_, ld, mode):
    check(load().nkb_wprep(dtype, ptr(src), ptr(dst), A, B, C_, ld, mode, stream()), "wprep")


def add2d(src, dst, rows, cols, ld_src, ld_dst):
    check(load().nkb_add2d(ptr(src), ptr(dst), rows, cols, ld_src, ld_dst, stream()), "add2d")


def colsum(dtype, x, out, rows, C_, ld):
    check(load().nkb_colsum(dtype, ptr(x), ptr(out), rows, C_, ld, stream()), "colsum")


def pad_cast(dtype, src, dst, rows, C_, ld_src, ld_dst, mul=1.0):
    check(load().nkb_pad_cast(dtype, ptr(src), ptr(dst), rows, C_, ld_src, ld_dst, mul, stream()), "pad_cast")


LOSS_MIXED = 16                     # NKB_LOSS_MIXED of nkbhip.h: kind | 16 is the two-label form of kind 0 / 1


def loss_mixed_state_bytes(B, C_):
    """row_state of a mixed launch: 32 bytes per row, then the C floats ew[j] (layout in nkbhip.h)"""
    return 32 * B + 4 * C_


def loss_forward(kind, logits, ld, target, B, C_, class_weight, gamma, ignore_index, probs, ldp, argmax, row_state, out2,
                 reduction=0):
    """kind | LOSS_MIXED: target is the int64 table [3][B] (y, y2, float64 bits of lam), row_state loss_mixed_state_bytes(B, C)
    long, and for kind 0 `gamma` carries the label-smoothing eps"""
    check(load().nkb_loss_forward(kind, ptr(logits), ld, ptr(target), B, C_, ptr(class_weight), gamma, ignore_index,
                                  ptr(probs), ldp, ptr(argmax), ptr(row_state), ptr(out2), reduction, stream()),
          "loss_forward")


def loss_backward(probs, ldp, target, row_state, out2, grad_out, B, C_, dlogits, ldd, per_row=False):
    """per_row is the bit field of nkbhip.h: bit 0 one grad_out per row, bit 1 (value 2) the records and target of a mixed forward"""
    check(load().nkb_loss_backward(ptr(probs), ldp, ptr(target), ptr(row_state), ptr(out2), ptr(grad_out), int(per_row), B,
                                   C_, ptr(dlogits), ldd, stream()), "loss_backward")


# NKB_OPTIM_* of nkbhip.h: kind | 16 / kind | 64 clip the gradient inside the launch (skip_flag is then the device record
# {skip, bound, P, 0, partials[P]}), kind == 32 is the weight-EMA form
OPTIM_CLIP_NORM, OPTIM_CLIP_VALUE, OPTIM_EMA = 16, 64, 32
OPTIM_MAX_PARTIALS = 4096           # most partial sums of squares a clip-norm record may carry
OPTIM_RECORD_HEAD = 4               # words of the record in front of the partials


def clip_chunks(total: int):
    """(chunk length, P): the gradient arena cut into P equal chunks for the clip-norm pass (nkb_segment_sumsq, one workgroup per
    chunk).  At least 16384 elements per chunk, a multiple of 4 (every chunk starts on 16 bytes), and P <= 4096."""
    if total < 1:
        raise ValueError(f"clip_chunks: total must be positive, got {total}")
    per = -(-total // OPTIM_MAX_PARTIALS)
    chunk = max(16384, (per + 3) // 4 * 4)
    return chunk, -(-total // chunk)


def clip_chunk_offsets(total: int):
    """The P + 1 segment offsets of clip_chunks(total): they tile [0, total) exactly (host list; the caller uploads it once)."""
    chunk, P = clip_chunks(total)
    return [min(k * chunk, total) for k in range(P + 1)]


def optim_step(kind, p, g, m, v, shadow, n, lr, wd, beta1, beta2, eps, grad_scale, c0=0.0, c1=0.0, c2=0.0, c3=0.0,
               skip_flag=None):
    """kind | OPTIM_CLIP_NORM / OPTIM_CLIP_VALUE: skip_flag is the clip record; kind == OPTIM_EMA: see ema_step"""
    check(load().nkb_optim_step(kind, ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), n, lr, wd, beta1, beta2, eps,
                                grad_scale, c0, c1, c2, c3, ptr(skip_flag), stream()), "optim_step")


def ema_step(ema, weights, shadow, n, decay, skip_flag=None):
    """ema = (d * ema) + ((1 - d) * weights) over n fp32 elements (nkb_optim_step, kind NKB_OPTIM_EMA); 1 - d is subtracted in
    double here and rounded to fp32 once, by the call"""
    d = float(decay)
    optim_step(OPTIM_EMA, ema, weights, None, None, shadow, n, 0.0, 0.0, d, 1.0 - d, 0.0, 1.0, skip_flag=skip_flag)


def bucket_sum_bf16(parts, stride, nparts, out, out_bf16, n):
    check(load().nkb_bucket_sum_bf16(ptr(parts), stride, nparts, ptr(out), ptr(out_bf16), n, stream()), "bucket_sum_bf16")


def grad_unscale_check(g, n, scale, found_inf):
    check(load().nkb_grad_unscale_check(ptr(g), n, ptr(scale), ptr(found_inf), stream()), "grad_unscale_check")


def scaler_update(scale, tracker, found_inf, last_found_inf, growth, backoff, interval):
    check(load().nkb_scaler_update(ptr(scale), ptr(tracker), ptr(found_inf), ptr(last_found_inf), growth, backoff,
                                   interval, stream()), "scaler_update")


def segment_sumsq(x, offsets, nseg, out):
    check(load().nkb_segment_sumsq(ptr(x), ptr(offsets), nseg, ptr(out), stream()), "segment_sumsq")


def gemm8p_config(on: bool, min_tiles: int = 0, min_k: int = 0):
    load().nkb_gemm8p_config(int(on), min_tiles, min_k)


def gemm8p_ragged(on: bool):
    """The M % 256 ragged rows of a persistent GEMM launch on their own small kernel where that saves a round (tests / A-B timing)."""
    load().nkb_gemm8p_ragged(int(on))


# ---- fp8 (per-tensor scaled e4m3 / e5m2 operands, configs[4]) -----------------------------------------------------------
E4M3, E5M2 = 0, 1


def fp8_quantize(dtype, kind, src, n, state, dst):
    check(load().nkb_fp8_quantize(dtype, kind, ptr(src), n, ptr(state), ptr(dst), stream()), "fp8_quantize")


def fp8_amax(dtype, src, n, state):
    check(load().nkb_fp8_amax(dtype, ptr(src), n, ptr(state), stream()), "fp8_amax")


def fp8_scale_update(state, kind):
    check(load().nkb_fp8_scale_update(ptr(state), kind, stream()), "fp8_scale_update")


def fp8_job_blocks(n) -> int:
    return int(load().nkb_fp8_job_blocks(n))


def fp8_multi(pass_, jobs, njobs, total_blocks):
    """pass 0: amax only, 1: quantise (+ amax), 2: scales from amax, 3: clear amax — over a device job table."""
    check(load().nkb_fp8_multi(pass_, ptr(jobs), njobs, total_blocks, stream()), "fp8_multi")


def gemm_fp8(mode, xq, wq, y, M, K, N, *, deq_x, deq_w, bias=None, add=None, aux=None, aux_mode=0, yq=None, q_state=None, q_kind=0,
             row_scale=None, rows_per_sample=0, mask_out=None, mask_in=None, colsum=None, colsum_work=None, ldx=None, ldw=None, ldy=None,
             ldadd=0, relu=0):
    """aux ([M][ldy], bf16): aux_mode 0 multiplies the result by it, 1 keeps the result where 0 < aux < 6 (ReLU6 backward).
    yq / q_state / q_kind: optional fp8 copy of the result (scale q_state[0], amax into q_state[2]) for the next fp8 GEMM.
    mask_out / mask_in: the ReLU6 mask as bits ([M][N / 8] bytes, with yq); y may be None when mask_out is given.
    colsum / colsum_work (with mask_in, yq): colsum[N] += column sums of the result, workspace [M / 256][N] fp32; y may be None."""
    check(load().nkb_gemm_fp8(mode, ptr(xq), ptr(wq), ptr(y), ptr(bias), ptr(add), ptr(aux), int(aux_mode), ptr(yq), ptr(q_state),
                              int(q_kind), ptr(row_scale), int(rows_per_sample), ptr(mask_out), ptr(mask_in), ptr(colsum), ptr(colsum_work),
                              ptr(deq_x), ptr(deq_w),
                              M, K, N,
                              K if ldx is None else ldx, K if ldw is None else ldw, N if ldy is None else ldy, ldadd,
                              int(relu), stream()), "gemm_fp8")


def fp8_quantize_colsum_workspace(rows, C) -> int:
    return int(load().nkb_fp8_quantize_colsum_workspace_floats(rows, C))


def fp8_quantize_colsum(kind, src, rows, C, ld, state, dst, colsum, workspace, row_scale=None, rows_per_sample=0):
    """fp8_quantize of a [rows][C] bf16 matrix + colsum[C] += its column sums (a Linear's bias gradient when src = dY); with
    row_scale the matrix is row_scale[row // rows_per_sample] * src."""
    check(load().nkb_fp8_quantize_colsum(kind, ptr(src), rows, C, ld, ptr(state), ptr(dst), ptr(colsum), ptr(workspace),
                                         ptr(row_scale), int(rows_per_sample), stream()), "fp8_quantize_colsum")


def wgrad_fp8_workspace(M, Cin, Cout) -> int:
    """Floats of workspace nkb_wgrad_fp8 needs, -1 when the shape is outside its envelope."""
    return int(load().nkb_wgrad_fp8_workspace_floats(M, Cin, Cout))


def wgrad_fp8(gq, xq, dw, M, Cin, Cout, *, deq_g, deq_x, workspace, ldx=None, ldg=None):
    """dw += deq_g * deq_x * gq^T xq (gq e5m2 [M][Cout], xq e4m3 [M][Cin], fp32 accumulation, deterministic)."""
    check(load().nkb_wgrad_fp8(ptr(gq), ptr(xq), ptr(dw), ptr(deq_g), ptr(deq_x), M, Cin, Cin if ldx is None else ldx, Cout,
                               Cout if ldg is None else ldg, ptr(workspace), workspace.numel(), stream()), "wgrad_fp8")


def prof_enable(on: bool):
    load().nkb_prof_enable(int(on))


def prof_collect():
    n = 32
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    work = (C.c_double * n)()
    byts = (C.c_double * n)()
    k = load().nkb_prof_collect(ms, cnt, work, byts, n)
    out = {}
    for i in range(k):
        if cnt[i]:
            out[load().nkb_kernel_name(i).decode()] = dict(ms=ms[i], launches=cnt[i], work=work[i], bytes=byts[i])
    return out


def prof_collect_raw(cap: int = 1 << 16, with_bytes: bool = False):
    """[(kernel name, ms, work)] per launch, in launch order (with_bytes: + the launch's algorithmic bytes)."""
    kid = (C.c_int * cap)()
    ms = (C.c_double * cap)()
    work = (C.c_double * cap)()
    byt = (C.c_double * cap)()
    n = load().nkb_prof_collect_raw(kid, ms, work, byt, cap)
    if with_bytes:
        return [(load().nkb_kernel_name(kid[i]).decode(), ms[i], work[i], byt[i]) for i in range(n)]
    return [(load().nkb_kernel_name(kid[i]).decode(), ms[i], work[i]) for i in range(n)]


# ---- transformer ----------------------------------------------------------------------------------
def gemm_batched(dtype, x, w, y, M, N, K, ldx, ldw, ldy, outer, inner, sx, sw, sy, out_f32=False):
    check(load().nkb_gemm_batched(dtype, ptr(x), ptr(w), ptr(y), M, N, K, ldx, ldw, ldy, outer, inner, sx[0], sx[1],
                                  sw[0], sw[1], sy[0], sy[1], int(out_f32), stream()), "gemm_batched")


def gemm_tn_batched(dtype, a, b, out, M, Na, Nb, lda, ldb, ldo, outer, inner, sa, sb, so):
    check(load().nkb_gemm_tn_batched(dtype, ptr(a), ptr(b), ptr(out), M, Na, Nb, lda, ldb, ldo, outer, inner, sa[0], sa[1],
                                     sb[0], sb[1], so[0], so[1], stream()), "gemm_tn_batched")


def layernorm_fwd(dtype, x, x_stride, gamma, beta, y, y_stride, mean, rstd, rows, D, eps, yq=None, q_state=None, q_kind=0):
    """yq / q_state / q_kind: optional fp8 copy of y for the fp8 GEMM that consumes it (see fp8_quantize)."""
    check(load().nkb_layernorm(dtype, 0, ptr(x), x_stride, None, 0, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), None,
                               ptr(y), y_stride, None, None, rows, D, eps, None, ptr(yq), ptr(q_state), int(q_kind), None, 0, None,
                               stream()), "layernorm_fwd")


def layernorm_bwd(dtype, dy, dy_stride, x, x_stride, gamma, mean, rstd, add, dx, dx_stride, dgamma, dbeta, rows, D,
                  workspace=None, yq=None, q_state=None, q_kind=0, row_scale=None, rows_per_sample=0, colsum=None):
    """yq / q_state / q_kind / row_scale / colsum: fp8 copy of (row_scale *) dx and its column sums (+= colsum) for the Linear
    backward that consumes this gradient — what fp8_quantize_colsum would make of dx."""
    check(load().nkb_layernorm(dtype, 1, ptr(dy), dy_stride, ptr(x), x_stride, ptr(gamma), None, ptr(mean), ptr(rstd),
                               ptr(add), ptr(dx), dx_stride, ptr(dgamma), ptr(dbeta), rows, D, 0.0, ptr(workspace),
                               ptr(yq), ptr(q_state), int(q_kind), ptr(row_scale), int(rows_per_sample), ptr(colsum),
                               stream()), "layernorm_bwd")


def layernorm_param_reduce(workspace, rows, D, planes, dgamma, dbeta, colsum=None):
    """Second half of layernorm_bwd(dgamma=None, dbeta=None, workspace=...): ordered sums of its partial rows into the gradients."""
    check(load().nkb_layernorm_param_reduce(ptr(workspace), rows, D, planes, ptr(dgamma), ptr(dbeta), ptr(colsum), stream()),
          "layernorm_param_reduce")


def layernorm_ws(D):
    return load().nkb_layernorm_workspace_floats(D)


# `kind` of gelu / gelu_fwd_dgelu (NKB_ACT_* of include/nkbhip.h): the MLP activation of a transformer block
ACT_GELU, ACT_QUICK_GELU = 0, 1
ACT_KINDS = {"gelu": ACT_GELU, "quick_gelu": ACT_QUICK_GELU}


def gelu(dtype, x, dy, out, n, kind=ACT_GELU):
    check(load().nkb_gelu(dtype, ptr(x), ptr(dy), ptr(out), n, kind, stream()), "gelu")


def splitk_reduce(dtype, partial, splits, M, N, y, ldy, bias, stats):
    check(load().nkb_splitk_reduce(dtype, ptr(partial), splits, M, N, ptr(y), ldy, ptr(bias), ptr(stats), stream()), "splitk_reduce")


def wfold(dtype, w, scale, dst, Cout, K):
    check(load().nkb_wfold(dtype, ptr(w), ptr(scale), ptr(dst), Cout, K, stream()), "wfold")


IMAGE_AUG_BIT, IMAGE_AUG_WORDS, IMAGE_AUG_MAX_HOLES = 4, 64, 12     # flag bit 2, words per record, boxes per record (nkbhip.h)
IMAGE_MIX_BIT, IMAGE_MIX_BLEND, IMAGE_MIX_BOX = 8, 1, 2             # flag bit 3: words 10..15 of the record mix the image (nkbhip.h)


def image_aug_bytes(B):
    """length of a flags buffer that carries records: the B flag bytes rounded up to 16, then 256 bytes per image"""
    return (B + 15) // 16 * 16 + 4 * IMAGE_AUG_WORDS * B


def pack_image_aug(flags, records):
    """flags uint8 [B] (bit 0 / 1 flips, bit 2 = IMAGE_AUG_BIT: this image has a record), records int32 [B, 64] (host tensors)
    -> the uint8 buffer nkb_image_prep reads when a bit 2 is set: flags, zero pad to 16 bytes, the record table.  Pinned when
    both inputs are pinned.  The kernel reads record b only where flags[b] has bit 2, whatever the other records hold, and
    words 10..15 only where it has bit 3 (IMAGE_MIX_BIT): there word 10 must be a partner index in [0, B) and word 11 a mode."""
    B = flags.numel()
    if flags.dtype != torch.uint8 or records.dtype != torch.int32 or tuple(records.shape) != (B, IMAGE_AUG_WORDS):
        raise RuntimeError(f"pack_image_aug: expected uint8 [B] flags and int32 [B, {IMAGE_AUG_WORDS}] records, got "
                           f"{tuple(flags.shape)} {flags.dtype} and {tuple(records.shape)} {records.dtype}")
    if flags.is_cuda or records.is_cuda:
        raise RuntimeError("pack_image_aug: packs host tensors (the buffer then crosses with the batch)")
    mixed = (flags.reshape(-1) & IMAGE_MIX_BIT) != 0
    if bool(mixed.any()):
        partner, mode = records[mixed, 10], records[mixed, 11]
        if bool(((partner < 0) | (partner >= B)).any()):
            raise RuntimeError(f"pack_image_aug: a partner index (word 10) lies outside [0, {B})")
        if bool(((mode != IMAGE_MIX_BLEND) & (mode != IMAGE_MIX_BOX)).any()):
            raise RuntimeError("pack_image_aug: a mix mode (word 11) is neither 1 (blend) nor 2 (box)")
    off = (B + 15) // 16 * 16
    buf = torch.zeros(image_aug_bytes(B), dtype=torch.uint8, pin_memory=flags.is_pinned() and records.is_pinned())
    buf[:B] = flags.reshape(-1)
    buf[off:] = records.contiguous().view(torch.uint8).reshape(-1)
    return buf


IMAGE_GEOM_BIT, IMAGE_GEOM_WORDS, IMAGE_GEOM_MAX_TAPS = 16, 16, 16    # flag bit 4, words per geometry record, blur taps per record (nkbhip.h)
IMAGE_GEOM_RESAMPLE, IMAGE_GEOM_BLUR, IMAGE_GEOM_REFLECT = 1, 2, 4    # word 0 of a geometry record


def image_geom_bytes(B):
    """length of a flags buffer that carries geometry records: image_aug_bytes(B), then 64 bytes per image"""
    return image_aug_bytes(B) + 4 * IMAGE_GEOM_WORDS * B


def image_geom_record(box=None, out_size=None, taps=None, reflect=False):
    """One geometry record, int32 numpy [16].  box: (y0, x0, bh, bw) in the image's source coordinates, resampled onto out_size =
    (Ho, Wo) — the two scales are divided here, in float32; taps: [(dy, dx), ..], 1..16 of them within +-127; reflect: the pad stage
    reflects (BORDER_REFLECT_101) instead of filling."""
    import numpy as np
    g = np.zeros(IMAGE_GEOM_WORDS, np.int32)
    if box is not None:
        y0, x0, bh, bw = (int(v) for v in box)
        if y0 < 0 or x0 < 0 or bh < 1 or bw < 1:
            raise ValueError(f"image_geom_record: box {tuple(box)} needs y0, x0 >= 0 and bh, bw >= 1")
        g[0] |= IMAGE_GEOM_RESAMPLE
        g[1:5] = (y0, x0, bh, bw)
        f = g.view(np.float32)
        f[5] = np.float32(bh) / np.float32(out_size[0])
        f[6] = np.float32(bw) / np.float32(out_size[1])
    if taps is not None:
        if not 1 <= len(taps) <= IMAGE_GEOM_MAX_TAPS:
            raise ValueError(f"image_geom_record: {len(taps)} taps; a record holds 1..{IMAGE_GEOM_MAX_TAPS}")
        g[0] |= IMAGE_GEOM_BLUR
        g[7] = len(taps)
        words = np.zeros(8, np.uint32)
        for t, (dy, dx) in enumerate(taps):
            if not (-127 <= int(dy) <= 127 and -127 <= int(dx) <= 127):
                raise ValueError(f"image_geom_record: tap ({dy}, {dx}) lies outside +-127")
            words[t // 2] |= np.uint32(((int(dy) & 0xFF) | ((int(dx) & 0xFF) << 8)) << (16 * (t % 2)))
        g[8:16] = words.view(np.int32)
    if reflect:
        g[0] |= IMAGE_GEOM_REFLECT
    return g


def pack_image_geom(flags, records, geom, sizes=None):
    """flags uint8 [B] (bit 4 = IMAGE_GEOM_BIT: this image has a geometry record), records int32 [B, 64] or None (no augmentation
    or mixing record anywhere: the table is zero-filled), geom int32 [B, 16] (host tensors) -> the uint8 buffer nkb_image_prep reads
    when a bit 4 is set: the layout of pack_image_aug, then the geometry table.  Of the images with bit 4 it refuses a crop box that
    is empty, negative or — where sizes (int32 [B, 2], h and w per image) are given — outside the image, a tap count outside
    1..16 and a tap offset of -128."""
    B = flags.numel()
    if geom.dtype != torch.int32 or tuple(geom.shape) != (B, IMAGE_GEOM_WORDS) or geom.is_cuda:
        raise RuntimeError(f"pack_image_geom: expected host int32 [B, {IMAGE_GEOM_WORDS}] geometry records, got "
                           f"{tuple(geom.shape)} {geom.dtype}")
    if records is None:
        records = torch.zeros(B, IMAGE_AUG_WORDS, dtype=torch.int32)
    head = pack_image_aug(flags, records)
    on = (flags.reshape(-1) & IMAGE_GEOM_BIT) != 0
    crop = on & ((geom[:, 0] & IMAGE_GEOM_RESAMPLE) != 0)
    if bool(crop.any()):
        y0, x0, bh, bw = (geom[crop, j].long() for j in range(1, 5))
        if bool(((y0 < 0) | (x0 < 0) | (bh < 1) | (bw < 1)).any()):
            raise RuntimeError("pack_image_geom: a crop box (words 1..4) is empty or starts below 0")
        if sizes is not None:
            hw = sizes.reshape(B, 2)[crop].long()
            if bool(((y0 + bh > hw[:, 0]) | (x0 + bw > hw[:, 1])).any()):
                raise RuntimeError("pack_image_geom: a crop box (words 1..4) reaches outside its image's h x w")
    blur = on & ((geom[:, 0] & IMAGE_GEOM_BLUR) != 0)
    if bool(blur.any()):
        n = geom[blur, 7]
        if bool(((n < 1) | (n > IMAGE_GEOM_MAX_TAPS)).any()):
            raise RuntimeError(f"pack_image_geom: a tap count (word 7) lies outside 1..{IMAGE_GEOM_MAX_TAPS}")
        offs = geom[blur, 8:16].contiguous().view(torch.int8).reshape(-1, 2 * IMAGE_GEOM_MAX_TAPS)
        used = torch.arange(2 * IMAGE_GEOM_MAX_TAPS)[None, :] < 2 * n.long()[:, None]
        if bool(((offs == -128) & used).any()):
            raise RuntimeError("pack_image_geom: a tap offset lies outside +-127")
    buf = torch.zeros(image_geom_bytes(B), dtype=torch.uint8, pin_memory=head.is_pinned() and geom.is_pinned())
    buf[:head.numel()] = head
    buf[head.numel():] = geom.contiguous().view(torch.uint8).reshape(-1)
    return buf


def image_prep(src, sizes, flags, out, B, Hs, Ws, Ho, Wo, mean, std, fill=0.0):
    """flags: None, uint8 [B], or the buffer of pack_image_aug / pack_image_geom (the C side cannot see device bits: the layout is
    kept here)"""
    if flags is not None and flags.numel() > B and (flags.numel() not in (image_aug_bytes(B), image_geom_bytes(B))
                                                    or flags.data_ptr() % 16):
        raise RuntimeError(f"image_prep: a flags buffer longer than B = {B} must be the 16-byte aligned {image_aug_bytes(B)}-byte "
                           f"layout of pack_image_aug or the {image_geom_bytes(B)}-byte one of pack_image_geom, got "
                           f"{flags.numel()} bytes at offset {flags.data_ptr() % 16}")
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(load().nkb_image_prep(ptr(src), ptr(sizes), ptr(flags), ptr(out), B, Hs, Ws, Ho, Wo, C.cast(m, C.c_void_p),
                                C.cast(sd, C.c_void_p), float(fill), stream()), "image_prep")


def gelu_fwd_dgelu(dtype, x, y, gp, n, kind=ACT_GELU):
    check(load().nkb_gelu_fwd_dgelu(dtype, ptr(x), ptr(y), ptr(gp), n, kind, stream()), "gelu_fwd_dgelu")


def relu6(dtype, x, dy, out, n):
    check(load().nkb_relu6(dtype, ptr(x), ptr(dy), ptr(out), n, stream()), "relu6")


def scale_rows(dtype, x, add, out, scale, rows, inner):
    check(load().nkb_scale_rows(dtype, ptr(x), ptr(add), ptr(out), ptr(scale), rows, inner, stream()), "scale_rows")


def attn_softmax(dtype, backward, s, lds, p_in, out, ldp, rows, cols, scale):
    check(load().nkb_attn_softmax(dtype, int(backward), ptr(s), lds, ptr(p_in), ptr(out), ldp, rows, cols, scale, stream()),
          "attn_softmax")


def head_transpose(dtype, src, ld_in, sio, sii, outer, inner, out, T, dh, ldt):
    check(load().nkb_head_transpose(dtype, ptr(src), ld_in, sio, sii, outer, inner, ptr(out), T, dh, ldt, stream()),
          "head_transpose")


def vit_assemble(dtype, backward, tok, cls, pos, x, B, Tn, D):
    check(load().nkb_vit_assemble(dtype, int(backward), ptr(tok), ptr(cls), ptr(pos), ptr(x), B, Tn, D, stream()), "vit_assemble")


def colsum2d(dtype, x, out, rows, C_, ld, workspace=None):
    if workspace is not None and workspace.numel() < 256 * C_:
        raise RuntimeError("colsum2d: workspace needs 256 * C floats")
    check(load().nkb_colsum2d(dtype, ptr(x), ptr(out), rows, C_, ld, ptr(workspace), stream()), "colsum2d")


def dropout(dtype, backward, src, add, out, mask, n, p, seed=0):
    check(load().nkb_dropout(dtype, int(backward), ptr(src), ptr(add), ptr(out), ptr(mask), n, p, seed, stream()), "dropout")


def attn_forward(dtype, qkv, out, lse, B, T, H, dh, scale, outq=None, q_state=None, drop_p=0.0, seed=0, drop_ld=0, seed_out=None):
    """outq / q_state: optional e4m3 copy of out for an fp8 projection (see fp8_quantize).
    drop_p > 0: attention dropout with nkb_dropout's mask of a [B*H, T, drop_ld] tensor under `seed` (a Seed from fresh_seed() is
    redrawn at every plan replay); seed_out: one int64 on the device that receives the seed for attn_backward."""
    check(load().nkb_attn_forward(dtype, ptr(qkv), ptr(out), ptr(lse), B, T, H, dh, scale, ptr(outq), ptr(q_state),
                                  drop_p, seed, drop_ld, ptr(seed_out), stream()), "attn_forward")


def attn_backward(dtype, qkv, dout, out, lse, dqkv, B, T, H, dh, scale, dqkv_q=None, q_state=None, colsum=None, colsum_work=None,
                  drop_p=0.0, seed_dev=None, drop_ld=0):
    """dqkv_q / q_state: optional e5m2 copy of dqkv for the fp8 qkv gradients.  colsum / colsum_work ([B][3 H dh] scratch):
    colsum += the column sums of dqkv (the qkv bias gradient).  drop_p / drop_ld: as in the forward call; seed_dev: its seed_out."""
    check(load().nkb_attn_backward(dtype, ptr(qkv), ptr(dout), ptr(out), ptr(lse), ptr(dqkv), B, T, H, dh, scale, ptr(dqkv_q),
                                   ptr(q_state), ptr(colsum), ptr(colsum_work), drop_p, ptr(seed_dev), drop_ld, stream()), "attn_backward")


def attn_backward_ds(dtype, qkv, dout, lse, P, dS, ldp, B, T, H, dh, scale, dq=None, ld_dq=0):
    check(load().nkb_attn_backward_ds(dtype, ptr(qkv), ptr(dout), ptr(lse), ptr(P), ptr(dS), ldp, B, T, H, dh, scale,
                                      ptr(dq), ld_dq, stream()), "attn_backward_ds")


def linear_gelu_fused_ok(dtype, M, K, N) -> bool:
    """act 5 of linear_gelu (y = gelu(pre), y2 = gelu'(pre) in the fc1 epilogue) is available for this shape."""
    return bool(load().nkb_linear_gelu_fused_ok(dtype, M, K, N))


def linear_residual_scaled(dtype, x, w, bias, add, row_scale, rows_per_sample, y, M, K, N):
    """y = add + row_scale[m // rows_per_sample] * (x @ w^T + bias) in one launch (shapes with linear_gelu_fused_ok)."""
    check(load().nkb_linear_residual_scaled(dtype, ptr(x), ptr(w), ptr(bias), ptr(add), ptr(row_scale), int(rows_per_sample),
                                            ptr(y), M, K, N, stream()), "linear_residual_scaled")


def linear_gelu(dtype, act, x, w, bias, aux, y, y2, M, K, N):
    check(load().nkb_linear_gelu(dtype, act, ptr(x), ptr(w), ptr(bias), ptr(aux), ptr(y), ptr(y2), M, K, N, stream()),
          "linear_gelu")


# ---- ConvNeXt: depthwise 7x7 convolution and layer scale (csrc/dwconv.hip) ------------------------
def dwconv(dtype, x, w, bias, y, *, N, H, W, C, ldx, ldy, R=7, pad=3, dgrad=False, add=None):
    """y = depthwise conv(x) + bias (+ add); dgrad: the data gradient (taps flipped, bias must be None).  w / bias: fp32 masters."""
    check(load().nkb_dwconv(dtype, int(dgrad), ptr(x), ptr(w), ptr(bias), ptr(add), ptr(y), N, H, W, C, ldx, ldy, R, pad, stream()), "dwconv")


def dwconv_wgrad_workspace(dtype, N, H, W, C, R=7) -> int:
    return int(load().nkb_dwconv_wgrad_workspace_floats(dtype, N, H, W, C, R))


def dwconv_wgrad(dtype, g, x, dw, dbias, *, N, H, W, C, ldg, ldx, workspace, R=7, pad=3):
    """dw += g (*) x, dbias += sum g through per-wave slabs and an ordered sum (bit-identical across launches)."""
    check(load().nkb_dwconv_wgrad(dtype, ptr(g), ptr(x), ptr(dw), ptr(dbias), N, H, W, C, ldg, ldx, R, pad, ptr(workspace),
                                  workspace.numel() if workspace is not None else 0, stream()), "dwconv_wgrad")


def layer_scale_workspace(rows, C_) -> int:
    return int(load().nkb_layer_scale_workspace_floats(rows, C_))


def layer_scale(dtype, backward, z, a, gamma, out, rows, C_, dgamma=None, workspace=None):
    """forward: out = a + gamma * z; backward: out = gamma * a (a: incoming gradient), dgamma += sum_m a * z."""
    check(load().nkb_layer_scale(dtype, int(backward), ptr(z), ptr(a), ptr(gamma), ptr(out), ptr(dgamma), rows, C_, ptr(workspace),
                                 workspace.numel() if workspace is not None else 0, stream()), "layer_scale")


# ---- ResNet-D/T: narrow 3x3 stem convolutions (csrc/stem3.hip) and the 2x2 average pool of the avg_down shortcut ----
def stem3_tiles(dtype, N, H, W, Cin, Cout) -> int:
    """Partial-sum rows (= workgroups) of stem3_conv for this launch; 0: the channel pair is not served."""
    return int(load().nkb_stem3_tiles(dtype, N, H, W, Cin, Cout))


def stem3_conv(dtype, x, w, y, *, N, H, W, Cin, ldx, Cout, ldy, dgrad=False, bias=None, stats=None, relu=False, tiles=0, R=3):
    """y = conv3x3/1/1(x, w) (+ bias) (ReLU); dgrad: w is the [Cin][3][3][Cout] data-gradient filter, its taps are read flipped.
    stats: per-workgroup sums of the stored y and y^2, sized for `tiles` = stem3_tiles(...) rows."""
    check(load().nkb_stem3_conv(dtype, int(dgrad), ptr(x), ptr(w), ptr(y), ptr(bias), ptr(stats), N, H, W, Cin, ldx, Cout, ldy, R,
                                int(relu), int(tiles), stream()), "stem3_conv")


def avgpool2x2(dtype, backward, src, dst, N, H, W, C_):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) on NHWC; backward: dst[N][H][W][C] = src[h/2][w/2] / count (written)."""
    check(load().nkb_avgpool2x2(dtype, int(backward), ptr(src), ptr(dst), N, H, W, C_, stream()), "avgpool2x2")
