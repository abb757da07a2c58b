// 3x3 / stride 1 / pad 1 convolution for NARROW NHWC tensors (24 / 32 / 64 channels): the second and third convolution of timm's
// deep ResNet stem (resnet14t / 26t / 26d / 50d: 3 -> 24|32 -> 32 -> 64 on 112 x 112 maps), forward and data gradient.
//
// One kernel family, bf16 (v_mfma_f32_16x16x32_bf16) and exact fp32 (v_mfma_f32_16x16x4_f32).  A 256-thread workgroup keeps the WHOLE
// filter in LDS and walks output tiles of TH rows x 32 columns: it stages the (TH + 2) x 35-pixel input window once (zeros outside the
// image), so every activation is loaded from memory once per tile and nothing goes through an im2row matrix.  The window of the NEXT
// tile is fetched into registers while the current one is multiplied.  In NHWC the (column tap,
// channel) pairs of one filter row are contiguous on both sides, so the contraction runs over three runs of 3 * Cin elements; a run is
// padded to the k-slice on the WEIGHT side with zeros (72 -> 96 at 24 channels), and what the activation side reads against those zeros
// is the next staged pixel (always written: data or zero), never stale LDS.
// MFMA roles: A = filter rows (M = 16 output channels), B = pixels (N = 16 consecutive columns of one output row); the filter rows are
// dealt to the channel tiles so that a lane ends up with 4 * Cout/16 CONSECUTIVE channels of one pixel: 16-byte stores.
// The data gradient is the same kernel on the [Cin][3][3][Cout] filter with the taps flipped while the filter is staged.
// BatchNorm partial sums (of the STORED values) leave as one row per workgroup, summed in a fixed order: no float atomics.
#include "prims.h"

namespace {

constexpr int S3_TW = 32;             // output columns of a tile
constexpr int S3_PW = S3_TW + 3;      // staged pixels per window row: left / right halo + the pixel the padded k-slices reach into

struct S3Params {
    const void* x; const void* w; void* y; const float* bias; float* stats;
    int N, H, W, ldx, ldy, flip, relu, tiles_h, tiles_w, ntiles;
};

template <int N> struct Int {};
template <typename T> struct S3;
template <> struct S3<bf16_t> {
    static constexpr int KS = 32, FR = 8;                  // k-slice, elements per lane per slice
    typedef bf16x8 frag;
    __device__ static __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    // n consecutive channels of one pixel as 16-byte stores
    template <int N> __device__ static __forceinline__ void store(bf16_t* p, const float* v, Int<N>) {
#pragma unroll
        for (int k = 0; k < N; k += 8) *(u32x4*)(p + k) = pack8(v + k);
    }
};
template <> struct S3<float> {
    static constexpr int KS = 4, FR = 1;
    typedef float frag;
    __device__ static __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    template <int N> __device__ static __forceinline__ void store(float* p, const float* v, Int<N>) {
#pragma unroll
        for (int k = 0; k < N; k += 4) *(f32x4*)(p + k) = (f32x4){v[k], v[k + 1], v[k + 2], v[k + 3]};
    }
};

template <typename T, int CIN, int COUT> struct S3Geom {
    static constexpr int ESZ = sizeof(T);
    // tile rows: the window + the filter of two workgroups fit one CU's 160 KB in bf16 (6 rows at 64 contraction channels); fp32
    // (parity mode) holds a 75 KB filter and runs one workgroup per CU on 4-row tiles
    static constexpr int TH = ESZ == 4 ? 4 : (CIN == 64 ? 6 : 8);
    static constexpr int KR = 3 * CIN;                                              // one filter row: (column tap, channel)
    static constexpr int KRP = (KR + S3<T>::KS - 1) / S3<T>::KS * S3<T>::KS;        // ... padded to the k-slice (weights: zeros)
    static constexpr int WS = KRP + 16 / ESZ;                                       // LDS stride of a filter row (+16 bytes: bank spread)
    static constexpr int NT = (COUT + 15) / 16, COP = NT * 16;
    static constexpr int MT = TH * (S3_TW / 16) / 4;                                // 16-pixel tiles per wave
    static constexpr int PXB = CIN * ESZ;
    static constexpr int NCH = (TH + 2) * S3_PW * (PXB / 16);                       // 16-byte chunks of a window
    static constexpr int WINB = (NCH * 16 + 2047) / 2048 * 2048;
    static constexpr int FLTB = 3 * COP * WS * ESZ;
    static constexpr int LDS = WINB + FLTB + 4 * 2 * COP * 4;
};

template <typename T, int CIN, int COUT>
__global__ __launch_bounds__(256, 2) void stem3_kernel(S3Params p) {
    typedef S3<T> D;
    typedef S3Geom<T, CIN, COUT> G;
    typedef T vec4 __attribute__((ext_vector_type(4)));
    constexpr int TH = G::TH, KS = D::KS, FR = D::FR, ESZ = G::ESZ, KR = G::KR, KRP = G::KRP, WS = G::WS, NT = G::NT, COP = G::COP,
                  MT = G::MT, PXB = G::PXB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // window | filter [3][COP][WS] | [4 waves][2][COP] floats
    unsigned char* win = smem;
    T* wl = (T*)(smem + G::WINB);
    float* red = (float*)(smem + G::WINB + G::FLTB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
    const int H = p.H, W = p.W;
    // MFMA row m of channel tile j is output channel (m / 4) * 4 * NT + j * 4 + m % 4: the 4 * NT values a lane ends up with are
    // CONSECUTIVE channels lg * 4 * NT .. of its pixel (16-byte stores)
    const int arow = (lm >> 2) * 4 * NT + (lm & 3);

    // ---- the filter, once per workgroup: wl[r][co][(s, c)], taps flipped for the data gradient, zero rows / zero k-padding ----
    {
        const T* w = (const T*)p.w;
        constexpr int K4 = KRP / 4, NV = 3 * COP * K4;
        for (int i0 = tid; i0 < NV; i0 += 256 * 8) {       // eight loads of a thread in flight together
            vec4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                const int kk = (i % K4) * 4, co = (i / K4) % COP, r = i / (K4 * COP);
                v[u] = (vec4){0, 0, 0, 0};
                if (i < NV && co < COUT && kk < KR) {
                    const int s = kk / CIN, c = kk - s * CIN;
                    const int rr = p.flip ? 2 - r : r, ss = p.flip ? 2 - s : s;
                    v[u] = *(const vec4*)(w + ((size_t)(co * 3 + rr) * 3 + ss) * CIN + c);
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                if (i < NV) *(vec4*)(wl + (size_t)(i / K4) * WS + (i % K4) * 4) = v[u];      // row i / K4 = r * COP + co
            }
        }
    }
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[j][e] = 0.f; s2[j][e] = 0.f; }

    const unsigned char* xb = (const unsigned char*)p.x;
    T* y = (T*)p.y;
    // ---- the input window of a tile: rows h0 - 1 .. h0 + TH, pixels w0 - 1 .. w0 + 33, zeros outside the image.  It is fetched into
    // registers one tile AHEAD (all loads of a thread in flight together, behind the current tile's MFMAs) and committed to LDS
    // between two barriers; chunk i of the window sits at byte 16 * i ----
    constexpr int CPP = PXB / 16, NLD = (G::NCH + 255) / 256;
    constexpr int UNR = KRP / KS <= 6 ? KRP / KS : 2;      // k-slices of a filter row: 3 or 6 in bf16 (unrolled), 18 .. 48 in fp32
    u32x4 stage[NLD];
    auto fetch = [&](int t) {
        const int tw = t % p.tiles_w, th = (t / p.tiles_w) % p.tiles_h, n = t / (p.tiles_w * p.tiles_h);
        const int h0 = th * TH, w0 = tw * S3_TW;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = tid + 256 * k;
            const int ch = i % CPP, pc = (i / CPP) % S3_PW, hr = i / (CPP * S3_PW);
            const int h = h0 - 1 + hr, wc = w0 - 1 + pc;
            stage[k] = (u32x4){0u, 0u, 0u, 0u};
            if (i < G::NCH && (unsigned)h < (unsigned)H && (unsigned)wc < (unsigned)W)
                stage[k] = *(const u32x4*)(xb + ((((size_t)n * H + h) * W + wc) * p.ldx) * ESZ + ch * 16);
        }
    };
    fetch(blockIdx.x);
    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int tw = t % p.tiles_w, th = (t / p.tiles_w) % p.tiles_h, n = t / (p.tiles_w * p.tiles_h);
        const int h0 = th * TH, w0 = tw * S3_TW;
        // raw barriers: __syncthreads would also drain the previous tile's global stores (vmcnt(0)) twice per tile
        NKB_BARRIER();                                     // the previous tile's fragment reads are done (their MFMAs have issued)
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = tid + 256 * k;
            if (i < G::NCH) *(u32x4*)(win + swz_lin(16 * i)) = stage[k];
        }
        NKB_LGKM(0);                                       // this wave's window (and, first time round, filter) writes have landed
        NKB_BARRIER();
        if (t + (int)gridDim.x < p.ntiles) fetch(t + (int)gridDim.x);

        f32x4 acc[MT][NT];
        bool live[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int g = wave * MT + i;
            live[i] = h0 + (g >> 1) < H && w0 + (g & 1) * 16 < W;             // wave-uniform: tiles wholly outside are skipped
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        for (int r = 0; r < 3; ++r) {
#pragma unroll UNR
            for (int ks = 0; ks < KRP / KS; ++ks) {
                const int kof = ks * KS + lg * FR;
                typename D::frag a[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) a[j] = *(const typename D::frag*)(wl + (r * COP + arow + j * 4) * WS + kof);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    if (!live[i]) continue;
                    const int g = wave * MT + i;
                    const int off = (((g >> 1) + r) * S3_PW + (g & 1) * 16 + lm) * PXB + kof * ESZ;
                    const typename D::frag b = *(const typename D::frag*)(win + swz_lin(off));
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = D::mma(a[j], b, acc[i][j]);
                }
            }
        }
        // ---- epilogue: lane = pixel lm of the tile, channels lg * 4 * NT + j * 4 .. + 3 ----
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (!live[i]) continue;
            const int g = wave * MT + i;
            const int h = h0 + (g >> 1), wc = w0 + (g & 1) * 16 + lm;
            const bool ok = wc < W;
            T* yp = y + (((size_t)n * H + h) * W + wc) * p.ldy;
            if (lg * 4 * NT >= COUT) continue;                 // (24 output channels: the last lane group holds zero rows only)
            float v[NT * 4];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[i][j][e] + (p.bias ? p.bias[lg * 4 * NT + j * 4 + e] : 0.f);
                    if (p.relu) t = fmaxf(t, 0.f);
                    v[j * 4 + e] = DT<T>::rnd(t);
                }
            if (ok) {
                D::store(yp + lg * 4 * NT, v, Int<NT * 4>());
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s1[j][e] += v[j * 4 + e]; s2[j][e] = fmaf(v[j * 4 + e], v[j * 4 + e], s2[j][e]); }
            }
        }
    }
    if (!p.stats) return;
    // ---- one partial-sum row per workgroup: 16 pixel lanes (DPP), then the four waves in order ----
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = row16_sum(s1[j][e]), b = row16_sum(s2[j][e]);
            if (lm == 0) { red[(wave * 2 + 0) * COP + lg * 4 * NT + j * 4 + e] = a; red[(wave * 2 + 1) * COP + lg * 4 * NT + j * 4 + e] = b; }
        }
    __syncthreads();
    for (int i = tid; i < 2 * COUT; i += 256) {
        const int pl = i / COUT, c = i - pl * COUT;
        float s = red[(0 * 2 + pl) * COP + c];
        for (int wv = 1; wv < 4; ++wv) s += red[(wv * 2 + pl) * COP + c];
        p.stats[((size_t)blockIdx.x * 2 + pl) * COUT + c] = s;
    }
}

struct S3Plan { int grid, lds, tiles_h, tiles_w, ntiles; };

// the six (contraction channels -> output channels) pairs of the deep stem: forward 24->32, 32->32, 32->64; data gradient 32->24, 32->32, 64->32
#define S3_PAIRS(X) X(24, 32) X(32, 32) X(32, 64) X(32, 24) X(64, 32)

bool s3_plan(int dtype, int N, int H, int W, int Cin, int Cout, S3Plan& g) {
    int lds = 0, th = 0;
#define S3_LDS(CI, CO)                                                                                              \
    if (Cin == CI && Cout == CO) {                                                                                  \
        lds = dtype == NKB_DT_BF16 ? S3Geom<bf16_t, CI, CO>::LDS : S3Geom<float, CI, CO>::LDS;                      \
        th = dtype == NKB_DT_BF16 ? S3Geom<bf16_t, CI, CO>::TH : S3Geom<float, CI, CO>::TH;                         \
    }
    S3_PAIRS(S3_LDS)
#undef S3_LDS
    if (!lds || lds > 160 * 1024 || N < 1 || H < 1 || W < 1) return false;
    g.tiles_h = (H + th - 1) / th;
    g.tiles_w = (W + S3_TW - 1) / S3_TW;
    const long long nt = (long long)N * g.tiles_h * g.tiles_w;
    if (nt >= (1ll << 31)) return false;
    g.ntiles = (int)nt;
    g.lds = lds;
    const int per_cu = 160 * 1024 / lds;                                               // resident workgroups: LDS decides
    const long long cap = (long long)nkb_cu_count() * (per_cu > 3 ? 3 : per_cu);
    g.grid = (int)(nt < cap ? nt : cap);
    return true;
}

}  // namespace

// Partial-sum rows (= workgroups) of nkb_stem3_conv for this launch; 0: dtype / channel pair not served.
extern "C" int nkb_stem3_tiles(int dtype, int N, int H, int W, int Cin, int Cout) {
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) return 0;
    S3Plan g;
    return s3_plan(dtype, N, H, W, Cin, Cout, g) ? g.grid : 0;
}

extern "C" int nkb_stem3_conv(int dtype, int dgrad, const void* x, const void* w, void* y, const float* bias, float* stats, int N, int H,
                              int W, int Cin, int ldx, int Cout, int ldy, int R, int relu, int tiles, hipStream_t stream) {
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) { nkb_set_error("stem3_conv: bad dtype %d", dtype); return 1; }
    if (R != 3) { nkb_set_error("stem3_conv: 3x3 / stride 1 / pad 1 only, got R=%d", R); return 1; }
    if (Cin % 8 != 0 || Cout % 8 != 0 || Cin < 8 || Cout < 8 || Cin > 64 || Cout > 64) {
        nkb_set_error("stem3_conv: Cin=%d / Cout=%d must be multiples of 8 up to 64", Cin, Cout);
        return 1;
    }
    const int al = dtype == NKB_DT_BF16 ? 8 : 4;
    if (ldx < Cin || ldy < Cout || ldx % al != 0 || ldy % al != 0) {
        nkb_set_error("stem3_conv: ldx=%d / ldy=%d must be >= Cin=%d / Cout=%d and multiples of %d", ldx, ldy, Cin, Cout, al);
        return 1;
    }
    if (N < 1 || H < 1 || W < 1 || (double)N * H * W * (ldx > ldy ? ldx : ldy) >= 2147483648.0) {
        nkb_set_error("stem3_conv: operand exceeds 2^31 elements (N=%d H=%d W=%d)", N, H, W);
        return 1;
    }
    S3Plan g;
    if (!s3_plan(dtype, N, H, W, Cin, Cout, g)) {
        nkb_set_error("stem3_conv: channel pair %d -> %d not served (24->32, 32->32, 32->64, 32->24, 64->32)", Cin, Cout);
        return 1;
    }
    if (stats && tiles != g.grid) { nkb_set_error("stem3_conv: stats sized for %d partial-sum rows, the launch has %d", tiles, g.grid); return 1; }
    S3Params p;
    p.x = x; p.w = w; p.y = y; p.bias = bias; p.stats = stats;
    p.N = N; p.H = H; p.W = W; p.ldx = ldx; p.ldy = ldy; p.flip = dgrad ? 1 : 0; p.relu = relu ? 1 : 0;
    p.tiles_h = g.tiles_h; p.tiles_w = g.tiles_w; p.ntiles = g.ntiles;
    static bool once = [] {
#define S3_ATTR(CI, CO)                                                                                                                        \
    (void)hipFuncSetAttribute((const void*)stem3_kernel<bf16_t, CI, CO>, hipFuncAttributeMaxDynamicSharedMemorySize, S3Geom<bf16_t, CI, CO>::LDS); \
    (void)hipFuncSetAttribute((const void*)stem3_kernel<float, CI, CO>, hipFuncAttributeMaxDynamicSharedMemorySize, S3Geom<float, CI, CO>::LDS);
        S3_PAIRS(S3_ATTR)
#undef S3_ATTR
        return true;
    }();
    (void)once;
    const double M = (double)N * H * W, esz = dtype == NKB_DT_BF16 ? 2.0 : 4.0;
    NkbProfScope prof(dgrad ? NKB_K_STEM3_DGRAD : NKB_K_STEM3_FWD, stream, 2.0 * M * 9 * Cin * Cout, esz * M * (Cin + Cout));
    nkb_count_launch(NKB_LAUNCH_STEM3);
#define S3_GO(CI, CO)                                                                                                         \
    if (Cin == CI && Cout == CO) {                                                                                            \
        if (dtype == NKB_DT_BF16) hipLaunchKernelGGL((stem3_kernel<bf16_t, CI, CO>), dim3(g.grid), dim3(256), g.lds, stream, p); \
        else hipLaunchKernelGGL((stem3_kernel<float, CI, CO>), dim3(g.grid), dim3(256), g.lds, stream, p);                      \
    }
    S3_PAIRS(S3_GO)
#undef S3_GO
    return nkb_check_launch("stem3_conv");
}
