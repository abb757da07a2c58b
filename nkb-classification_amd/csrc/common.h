// Shared device/host helpers for libnkbhip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "nkbhip.h"   // the public C ABI: every extern "C" definition is compiled against its prototype (and NKB_DT_*, NkbLaunchCounter)

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // 8 packed bf16 (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short bf16x4;   // 4 packed bf16 (2 VGPRs)
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

typedef unsigned short bf16_t;  // storage type of a bfloat16 value

// ---- bf16 <-> f32 (round-to-nearest-even; NaN stays NaN through the hw cvt) ----
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
// gfx950 converts in hardware (v_cvt_pk_bf16_f32, round-to-nearest-even, NaN stays NaN): one instruction per two
// values instead of ~6 integer ops per value
typedef __bf16 nkb_bf2 __attribute__((ext_vector_type(2)));
typedef float nkb_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf2(float lo, float hi) {
    const nkb_f2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, nkb_bf2));
}
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }

template <typename T> struct DT;
template <> struct DT<float> {
    static constexpr int EPC = 4;  // elements per 16-byte chunk
    static constexpr int code = NKB_DT_F32;
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
    __device__ static __forceinline__ float rnd(float v) { return v; }
};
template <> struct DT<bf16_t> {
    static constexpr int EPC = 8;
    static constexpr int code = NKB_DT_BF16;
    __device__ static __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
    __device__ static __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
    __device__ static __forceinline__ float rnd(float v) { return bf2f(f2bf(v)); }
};

// unpack one 16-byte chunk into floats
__device__ __forceinline__ void unpack8(const u32x4& c, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(c[i] << 16);
        f[2 * i + 1] = __uint_as_float(c[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
    u32x4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = pack_bf2(f[2 * i], f[2 * i + 1]);
    return c;
}

// ---- one 16-byte chunk of an activation tensor (8 bf16 / 4 fp32) as floats: the vector I/O of the HBM-bound kernels ----
template <typename T> struct Chunk;
template <> struct Chunk<bf16_t> {
    static constexpr int N = 8;
    typedef u32x4 Raw;                                      // a chunk as loaded: kept packed while the load is in flight
    __device__ static __forceinline__ Raw ldraw(const bf16_t* p) { return *(const u32x4*)p; }
    __device__ static __forceinline__ void unpack(const Raw& r, float* f) { unpack8(r, f); }
    __device__ static __forceinline__ void load(const bf16_t* p, float* f) { unpack8(*(const u32x4*)p, f); }
    __device__ static __forceinline__ void store(bf16_t* p, const float* f) { *(u32x4*)p = pack8(f); }
};
template <> struct Chunk<float> {
    static constexpr int N = 4;
    typedef f32x4 Raw;
    __device__ static __forceinline__ Raw ldraw(const float* p) { return *(const f32x4*)p; }
    __device__ static __forceinline__ void unpack(const Raw& r, float* f) { f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3]; }
    __device__ static __forceinline__ void load(const float* p, float* f) {
        const f32x4 v = *(const f32x4*)p;
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    }
    __device__ static __forceinline__ void store(float* p, const float* f) { *(f32x4*)p = (f32x4){f[0], f[1], f[2], f[3]}; }
};

// ---- QuickGELU (the MLP activation of the OpenAI / MetaCLIP / DFN CLIP towers): u = x s with s = 1 / (1 + exp(-1.702 x)), and
// u' = s (1 + 1.702 x (1 - s)).  ONE definition in two forms: the GEMM epilogues (csrc/gemm8p.hip, csrc/conv_igemm.hip) and the
// elementwise kernels (csrc/transformer.hip) all take the pair from here.  For large negative x the exponential overflows to +inf:
// then s = 1 / inf = 0 and both results are (signed) zeros.  The derivative is evaluated as s + 1.702 (u (1 - s)): |u| <= |x| and
// |u (1 - s)| < 0.3 are finite for every finite x, where 1.702 x itself overflows from |x| = 2e38 on and would meet a zero factor
// (inf * 0).  The only infinity that can appear is the exponential, and it is consumed by the reciprocal: no finite x gives a NaN.
constexpr float NKB_QGELU_A = 1.702f;
// packed form for bf16 outputs, two elements per instruction: two quarter-rate instructions per element (exp2, rcp) and six packed
// multiplies / adds / FMAs per PAIR (g8_gelu2's erf chain needs thirteen, and two sign transfers)
__device__ __forceinline__ void quick_gelu2(nkb_f2 x, nkb_f2& u, nkb_f2& du) {
    constexpr float c = (float)(-1.702 * 1.4426950408889634);                                 // -1.702 log2(e)
    const nkb_f2 one = {1.f, 1.f};
    const nkb_f2 z = x * (nkb_f2){c, c};
    const nkb_f2 den = (nkb_f2){__builtin_amdgcn_exp2f(z[0]), __builtin_amdgcn_exp2f(z[1])} + one;   // 1 + exp(-1.702 x), +inf at most
    const nkb_f2 s = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
    u = x * s;
    du = __builtin_elementwise_fma((nkb_f2){NKB_QGELU_A, NKB_QGELU_A}, u * (one - s), s);
}
// fp32 form (the parity mode): libm's expf and a true division
__device__ __forceinline__ void quick_gelu_f32(float x, float& u, float& du) {
    const float s = 1.f / (1.f + expf(-NKB_QGELU_A * x));
    u = x * s;
    du = s + NKB_QGELU_A * (u * (1.f - s));
}
// N (even) values in the dtype's form: T = bf16_t packed, T = float exact; u / du may be x
template <typename T, int N>
__device__ __forceinline__ void quick_gelu_n(const float* x, float* u, float* du) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int e = 0; e < N; e += 2) {
            nkb_f2 uu, dd;
            quick_gelu2((nkb_f2){x[e], x[e + 1]}, uu, dd);
            u[e] = uu[0]; u[e + 1] = uu[1]; du[e] = dd[0]; du[e + 1] = dd[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) { const float xe = x[e]; quick_gelu_f32(xe, u[e], du[e]); }
    }
}

// ---- dropout's counter-based generator: keep(seed, i) is a stateless hash of the 64-bit seed and the 64-bit element index i, so a
// mask never has to be stored to be applied again.  ONE definition: nkb_dropout (csrc/transformer.hip) writes the mask bytes with it,
// the fused attention kernels (csrc/attention.hip) regenerate the same decisions for the score elements a lane holds ----
__host__ __device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
// an element is kept where its hash is >= this (p in [0, 1))
__host__ __device__ __forceinline__ unsigned dropout_thresh(float p) {
    return (unsigned)((double)p * 4294967296.0 > 4294967295.0 ? 4294967295.0 : (double)p * 4294967296.0);
}
// the hash in two steps: what depends on the high word of the index alone, then the rest (a caller that walks a short run of
// indices computes the first step once per run)
__host__ __device__ __forceinline__ unsigned dropout_hi_term(unsigned i_hi, unsigned seed_hi) { return i_hi * 0x9e3779b9u + seed_hi; }
__host__ __device__ __forceinline__ unsigned dropout_hash(unsigned i_lo, unsigned hi_term, unsigned seed_lo) {
    return mix32(mix32(i_lo ^ seed_lo) + hi_term);
}
__host__ __device__ __forceinline__ bool dropout_keep(unsigned long long i, unsigned seed_lo, unsigned seed_hi, unsigned thresh) {
    return dropout_hash((unsigned)i, dropout_hi_term((unsigned)(i >> 32), seed_hi), seed_lo) >= thresh;
}

// ---- division by a runtime constant (32-bit, exact for n < 2^31) ----
struct FastDiv {
    unsigned d, mul, sh;
};
static inline FastDiv make_fastdiv(unsigned d) {
    FastDiv f;
    f.d = d;
    if (d <= 1) { f.mul = 0; f.sh = 0; return f; }
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    unsigned long long m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    f.mul = (unsigned)m;
    f.sh = l;
    return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& f) {
    if (f.d <= 1) return n;
    unsigned t = __umulhi(n, f.mul);
    // (t + ((n - t) >> 1)) >> (sh - 1)   (Granlund–Montgomery round-up form)
    return (t + ((n - t) >> 1)) >> (f.sh - 1);
}

// ---- wave64 reductions ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// XCD-aware bijective block remap: consecutive logical ids land on one XCD (same L2).
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7, x = bid & 7, o = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
}

// ---- host-side error plumbing ----
void nkb_set_error(const char* fmt, ...);
int nkb_check_launch(const char* what);
// compute units of the current device (256 if the query fails); asked once per process, for whichever device was current then
int nkb_cu_count();
// dst[i] += sum over s < splits of part[s * slab + i], i < n, in split order (conv_igemm.hip): second stage of the
// deterministic weight gradients.  assign: dst is overwritten ("=", scratch products) instead of accumulated into ("+=")
int nkb_launch_wgrad_reduce(const float* part, long long slab, int splits, float* dst, long long n, bool assign, hipStream_t stream);
// the same for two ranges in ONE launch (weight slabs + the bias partials behind them)
int nkb_launch_wgrad_reduce2(const float* part, long long slab, int splits, float* dst, long long n, const float* part2, long long slab2,
                             float* dst2, long long n2, bool assign, hipStream_t stream);
// records what nkb_wgrad_last_kernel answers (conv_igemm.hip): family NKB_WGRAD_*, its variant (bits 4-7 of the code), slab form, splits
void nkb_wgrad_note_kernel(int family, int variant, bool slabs, int splits);

// the global-response-normalisation passes of nkb_avgpool (csrc/grn.hip): modes NKB_GRN_* of include/nkbhip.h
int nkb_grn(int dtype, int mode, const void* in, void* out, int N, int HW, int C, const void* in2, const float* weight, const float* bias,
            float* sumsq, float* dweight, float* dbias, const void* mul, float eps, float* workspace, long long workspace_floats,
            hipStream_t stream);

// the channel-attention passes of nkb_avgpool (csrc/se.hip): modes NKB_SE_* / NKB_ECA_* of include/nkbhip.h
int nkb_se(int dtype, int mode, const void* in, void* out, int N, int HW, int C, const void* in2, const float* weight, const float* bias,
           float* sumsq, float* dweight, float* dbias, const void* mul, float* workspace, long long workspace_floats, hipStream_t stream);

// bumps a launch counter of nkb_kernel_launches (api.hip); which: an NkbLaunchCounter of include/nkbhip.h
void nkb_count_launch(int which);

// per-launch HIP-event profiler (enabled from bench.py); see api.hip
struct NkbProfScope {
    int slot;
    hipStream_t stream;
    NkbProfScope(int kernel_id, hipStream_t s, double work, double bytes = 0.0);   // algorithmic FLOPs / bytes of the launch
    ~NkbProfScope();
};
// Profiler kernel ids and the names nkb_kernel_name reports for them (profiles and tests key on both): one row per id, in id order.
// A new id is appended; the enum below and the name table in api.hip are both expansions of this list.
#define NKB_KERNEL_IDS(X) \
    X(NKB_K_CONV_FWD, "conv_igemm_fwd") \
    X(NKB_K_CONV_DGRAD, "conv_igemm_dgrad") \
    X(NKB_K_CONV_WGRAD, "conv_wgrad") \
    X(NKB_K_BN_APPLY, "bn_apply") \
    X(NKB_K_BN_BWD_REDUCE, "bn_bwd_reduce") \
    X(NKB_K_BN_BWD_APPLY, "bn_bwd_apply") \
    X(NKB_K_BN_FINALIZE, "bn_finalize") \
    X(NKB_K_MAXPOOL, "maxpool") \
    X(NKB_K_AVGPOOL, "avgpool") \
    X(NKB_K_IM2COL, "im2row") \
    X(NKB_K_WPREP, "wprep") \
    X(NKB_K_LOSS, "loss") \
    X(NKB_K_OPTIM, "optim") \
    X(NKB_K_MISC, "misc") \
    X(NKB_K_LN, "layernorm") \
    X(NKB_K_ATTN, "attention") \
    X(NKB_K_GELU, "gelu") \
    X(NKB_K_WGRAD_REDUCE, "wgrad_reduce") \
    X(NKB_K_DWCONV_FWD, "dwconv_fwd") \
    X(NKB_K_DWCONV_DGRAD, "dwconv_dgrad") \
    X(NKB_K_DWCONV_WGRAD, "dwconv_wgrad") \
    X(NKB_K_LAYER_SCALE, "layer_scale") \
    X(NKB_K_STEM3_FWD, "stem3_fwd") \
    X(NKB_K_STEM3_DGRAD, "stem3_dgrad") \
    X(NKB_K_AVGPOOL2, "avgpool2x2") \
    X(NKB_K_GRN_REDUCE, "grn_reduce") \
    X(NKB_K_GRN_APPLY, "grn_apply") \
    X(NKB_K_GRN_PARAM, "grn_param")
#define NKB_KERNEL_ID_ENUM(id, name) id,
enum NkbKernelId { NKB_KERNEL_IDS(NKB_KERNEL_ID_ENUM) NKB_K_COUNT };
#undef NKB_KERNEL_ID_ENUM
