// Global Response Normalisation of the ConvNeXt V2 block (timm GlobalResponseNorm, channels-last; reached through
// timm.create_model("convnextv2_*") at nkb_classification/model.py:82 of the reference), forward and backward, fp32 and bf16.
//
// u: [N][HW][Ch] rows (NHWC), Ch = 4C the MLP's hidden width.
//   S[b][c] = sum_p u^2      G = sqrt(S)      m[b] = mean_c G + eps      s[b][c] = 1 + weight[c] G / m[b]      out = u s + bias[c]
// backward, g the gradient of out:
//   P[b][c] = sum_p g u      Q[b][c] = sum_p g      dbias[c] += sum_b Q      dweight[c] += sum_b (G / m) P
//   dN = weight[c] P     A[b] = sum_c dN G     dG = dN / m - A / (Ch m^2)     t = dG / G (0 where S == 0)     du = (g s + u t) (* mul)
//
// Three kernels, all sums fp32, every summation order a function of the shape alone (no float atomics, nothing depends on the grid):
//   grn_reduce  one work item per (image, 64-channel group), walked by a grid-stride loop.  256 threads = (64 / EPC channel lanes) x
//               (pixel lanes): a thread owns one 16-byte chunk of channels and every LP-th pixel, sums them in pixel order, and the LP
//               partial sums of a channel are added in lane order through LDS (an in-wave shuffle butterfly in front of a four-wave
//               LDS sum measured slower at HW = 49: DESIGN.md 3.15).  Forward: S.  Backward: P and Q from one read of g, u.
//   grn_apply   one workgroup per (image, chunk of the image's elements).  It first rebuilds the per-image scalars from the Ch floats
//               of S[b] (and P[b]): G into LDS, m (and A) by a fixed-order block sum, then the tables s[c] and bias[c] (forward) or
//               s[c] and t[c] (backward) in LDS; then it streams its chunk with 16-byte loads and stores, rounding once.
//               Backward takes an optional multiplier tensor (act'(pre) of the MLP: GELU backward rides along) and leaves m[b] behind
//               for the parameter launch.
//   grn_param   dweight / dbias: 64 channels x 4 image lanes per workgroup, images in order, "+=" into the gradient arena.
#include "common.h"

#define GRN_CG 64                    // channels per reduce work item
#define GRN_MAX_CH 4096              // two fp32 tables of Ch floats in LDS (32 KB at the widest)

// sum over the 256 threads of a workgroup in a fixed order (xor butterfly inside a wave, waves in index order); every thread
// gets the total.  `slot`: 4 floats of LDS that nothing else touches between the two barriers
__device__ __forceinline__ float grn_block_sum(float v, float* slot) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void grn_reduce_kernel(const T* __restrict__ a, const T* __restrict__ u, float* __restrict__ out1,
                                                         float* __restrict__ out2, int HW, int Ch, long long items) {
    constexpr int EPC = Chunk<T>::N, LC = GRN_CG / EPC, LP = 256 / LC;
    __shared__ float red[(BWD ? 2 : 1) * 256 * EPC];
    const int tc = threadIdx.x % LC, tp = threadIdx.x / LC;
    const int CGs = Ch / GRN_CG;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / CGs), cg = (int)(item % CGs);
        const size_t base = (size_t)b * HW * Ch + cg * GRN_CG + tc * EPC;
        float acc1[EPC], acc2[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc1[e] = acc2[e] = 0.f;
#pragma unroll 4
        for (int p = tp; p < HW; p += LP) {
            float uf[EPC], af[EPC];
            Chunk<T>::load(u + base + (size_t)p * Ch, uf);
            if (BWD) Chunk<T>::load(a + base + (size_t)p * Ch, af);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                if (BWD) { acc1[e] = fmaf(af[e], uf[e], acc1[e]); acc2[e] += af[e]; }
                else acc1[e] = fmaf(uf[e], uf[e], acc1[e]);
            }
        }
        __syncthreads();                 // (the previous item's readers are done with red)
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            red[threadIdx.x * EPC + e] = acc1[e];
            if (BWD) red[(256 + threadIdx.x) * EPC + e] = acc2[e];
        }
        __syncthreads();
        if (threadIdx.x < GRN_CG) {
            const int lc = threadIdx.x / EPC, e = threadIdx.x % EPC;
            float s1 = 0.f, s2 = 0.f;
            for (int j = 0; j < LP; ++j) {
                s1 += red[(j * LC + lc) * EPC + e];
                if (BWD) s2 += red[(256 + j * LC + lc) * EPC + e];
            }
            const size_t o = (size_t)b * Ch + cg * GRN_CG + threadIdx.x;
            out1[o] = s1;
            if (BWD) out2[o] = s2;
        }
    }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void grn_apply_kernel(const T* __restrict__ a, const T* __restrict__ u, const T* __restrict__ mul,
                                                        const float* __restrict__ weight, const float* __restrict__ bias,
                                                        const float* __restrict__ S, const float* __restrict__ Pt, float* __restrict__ mvec,
                                                        T* __restrict__ out, int HW, int Ch, float eps, int cpi, long long vpc) {
    constexpr int EPC = Chunk<T>::N;
    extern __shared__ __attribute__((aligned(16))) float grn_tab[];     // 2 Ch floats, sized by the launch (narrow stages keep their occupancy)
    float* tab0 = grn_tab;                                              // G, then s
    float* tab1 = grn_tab + Ch;                                         // forward: bias; backward: weight * P, then t
    __shared__ float slot[8];
    const int b = blockIdx.x / cpi, k = blockIdx.x % cpi;
    const float* Sb = S + (size_t)b * Ch;
    float pm = 0.f, pa = 0.f;
    for (int c = threadIdx.x; c < Ch; c += 256) {
        const float G = sqrtf(Sb[c]);
        tab0[c] = G;
        pm += G;
        if (BWD) {
            const float dN = weight[c] * Pt[(size_t)b * Ch + c];
            tab1[c] = dN;
            pa = fmaf(dN, G, pa);
        }
    }
    const float m = grn_block_sum(pm, slot) / (float)Ch + eps;
    float k2 = 0.f;
    if (BWD) {
        const float A = grn_block_sum(pa, slot + 4);
        k2 = A / ((float)Ch * m * m);
        if (mvec && k == 0 && threadIdx.x == 0) mvec[b] = m;
    }
    for (int c = threadIdx.x; c < Ch; c += 256) {          // (each thread rewrites the entries it wrote above)
        const float G = tab0[c];
        tab0[c] = fmaf(weight[c], G / m, 1.f);
        if (BWD) tab1[c] = G > 0.f ? (tab1[c] / m - k2) / G : 0.f;
        else tab1[c] = bias[c];
    }
    __syncthreads();
    const long long nv = (long long)HW * Ch / EPC;
    const long long v0 = k * vpc, v1 = min(nv, v0 + vpc);
    const size_t img = (size_t)b * HW * Ch;
    const int step = (256 * EPC) % Ch;
    int c = (int)(((v0 + threadIdx.x) * EPC) % Ch);
#pragma unroll 2
    for (long long v = v0 + threadIdx.x; v < v1; v += 256) {
        const size_t off = img + (size_t)v * EPC;
        float uf[EPC], af[EPC], mf[EPC], of[EPC];
        Chunk<T>::load(u + off, uf);
        if (BWD) {
            Chunk<T>::load(a + off, af);
            if (mul) Chunk<T>::load(mul + off, mf);
        }
#pragma unroll
        for (int e = 0; e < EPC; e += 4) {
            const f32x4 s4 = *(const f32x4*)(tab0 + c + e), t4 = *(const f32x4*)(tab1 + c + e);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (BWD) {
                    const float d = fmaf(uf[e + i], t4[i], af[e + i] * s4[i]);
                    of[e + i] = mul ? d * mf[e + i] : d;
                } else {
                    of[e + i] = fmaf(uf[e + i], s4[i], t4[i]);
                }
            }
        }
        Chunk<T>::store(out + off, of);
        c += step;
        if (c >= Ch) c -= Ch;
    }
}

__global__ __launch_bounds__(256) void grn_param_kernel(const float* __restrict__ S, const float* __restrict__ Pt, const float* __restrict__ Qt,
                                                        const float* __restrict__ mvec, float* __restrict__ dweight,
                                                        float* __restrict__ dbias, int N, int Ch) {
    __shared__ float red[2 * 256];
    const int c = blockIdx.x * GRN_CG + (threadIdx.x & 63), j = threadIdx.x >> 6;
    float aw = 0.f, ab = 0.f;
#pragma unroll 4
    for (int b = j; b < N; b += 4) {
        const size_t o = (size_t)b * Ch + c;
        aw = fmaf(sqrtf(S[o]) / mvec[b], Pt[o], aw);
        ab += Qt[o];
    }
    red[threadIdx.x] = aw;
    red[256 + threadIdx.x] = ab;
    __syncthreads();
    if (j == 0) {
        const int t = threadIdx.x;
        if (dweight) dweight[c] += ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t];
        if (dbias) dbias[c] += ((red[256 + t] + red[320 + t]) + red[384 + t]) + red[448 + t];
    }
}

static long long grn_workspace_floats(int N, int C) { return 2ll * N * C + N; }        // P, Q: [N][C]; m: [N]

// The GRN passes of nkb_avgpool (modes 2 .. 6, include/nkbhip.h); every argument is checked before anything is launched.
int nkb_grn(int dtype, int mode, const void* in, void* out, int N, int HW, int C, const void* in2, const float* weight, const float* bias,
            float* sumsq, float* dweight, float* dbias, const void* mul, float eps, float* workspace, long long workspace_floats,
            hipStream_t stream) {
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) { nkb_set_error("grn: bad dtype %d", dtype); return 1; }
    if (C < GRN_CG || C % GRN_CG != 0 || C > GRN_MAX_CH) {
        nkb_set_error("grn: C=%d must be a multiple of %d up to %d", C, GRN_CG, GRN_MAX_CH);
        return 1;
    }
    if (N < 1 || HW < 1 || (long long)N * HW * C >= (1ll << 31)) {
        nkb_set_error("grn: N=%d x HW=%d x C=%d outside 1 .. 2^31 elements", N, HW, C);
        return 1;
    }
    if (!(eps > 0.f)) { nkb_set_error("grn: eps=%g must be positive", (double)eps); return 1; }
    if (!sumsq) { nkb_set_error("grn: mode %d needs the sum-of-squares table", mode); return 1; }
    if (mode != NKB_GRN_PARAM && !in) { nkb_set_error("grn: mode %d needs its input tensor", mode); return 1; }
    if ((mode == NKB_GRN_BWD_REDUCE || mode == NKB_GRN_BWD_APPLY) && !in2) {
        nkb_set_error("grn: mode %d needs the forward input next to the gradient", mode);
        return 1;
    }
    if ((mode == NKB_GRN_FWD_APPLY || mode == NKB_GRN_BWD_APPLY) && (!out || !weight || (mode == NKB_GRN_FWD_APPLY && !bias))) {
        nkb_set_error("grn: mode %d needs out, weight%s", mode, mode == NKB_GRN_FWD_APPLY ? " and bias" : "");
        return 1;
    }
    if (mode == NKB_GRN_PARAM && !dweight && !dbias) { nkb_set_error("grn: the parameter pass needs dweight or dbias"); return 1; }
    const long long need = grn_workspace_floats(N, C);
    if (mode >= NKB_GRN_BWD_REDUCE && (!workspace || workspace_floats < need)) {
        nkb_set_error("grn: workspace of %lld floats given, %lld needed", workspace ? workspace_floats : 0ll, need);
        return 1;
    }
    const bool bf = dtype == NKB_DT_BF16;
    const double esz = bf ? 2.0 : 4.0, el = (double)N * HW * C, tab = 4.0 * N * C;
    float *Pt = workspace, *Qt = workspace ? workspace + (size_t)N * C : nullptr, *mvec = workspace ? workspace + 2 * (size_t)N * C : nullptr;
    if (mode == NKB_GRN_FWD_REDUCE || mode == NKB_GRN_BWD_REDUCE) {
        const bool bwd = mode == NKB_GRN_BWD_REDUCE;
        const long long items = (long long)N * (C / GRN_CG);
        const long long cap = (long long)nkb_cu_count() * 8;
        const unsigned grid = (unsigned)(items < cap ? items : cap);
        NkbProfScope prof(NKB_K_GRN_REDUCE, stream, (bwd ? 3.0 : 2.0) * el, (bwd ? 2.0 : 1.0) * (esz * el + tab));
#define GRN_REDUCE(T) do { \
            if (bwd) hipLaunchKernelGGL((grn_reduce_kernel<T, true>), dim3(grid), dim3(256), 0, stream, (const T*)in, (const T*)in2, Pt, Qt, HW, C, items); \
            else hipLaunchKernelGGL((grn_reduce_kernel<T, false>), dim3(grid), dim3(256), 0, stream, (const T*)nullptr, (const T*)in, sumsq, (float*)nullptr, HW, C, items); \
        } while (0)
        if (bf) GRN_REDUCE(bf16_t); else GRN_REDUCE(float);
#undef GRN_REDUCE
        return nkb_check_launch("grn_reduce");
    }
    if (mode == NKB_GRN_FWD_APPLY || mode == NKB_GRN_BWD_APPLY) {
        const bool bwd = mode == NKB_GRN_BWD_APPLY;
        const long long nv = (long long)HW * C / (bf ? 8 : 4);
        long long cpi = ((long long)nkb_cu_count() * 8 + N - 1) / N, most = (nv + 1023) / 1024;      // >= 4 chunks per thread where the image has them
        if (cpi > most) cpi = most;
        if (cpi < 1) cpi = 1;
        const long long vpc = (nv + cpi - 1) / cpi;
        cpi = (nv + vpc - 1) / vpc;
        const unsigned grid = (unsigned)(N * cpi);
        const size_t lds = 2 * sizeof(float) * (size_t)C;
        NkbProfScope prof(NKB_K_GRN_APPLY, stream, (bwd ? (mul ? 4.0 : 3.0) : 2.0) * el,
                          esz * el * (bwd ? (mul ? 4.0 : 3.0) : 2.0) + tab * (bwd ? 2.0 : 1.0));
#define GRN_APPLY(T) do { \
            if (bwd) hipLaunchKernelGGL((grn_apply_kernel<T, true>), dim3(grid), dim3(256), lds, stream, (const T*)in, (const T*)in2, (const T*)mul, weight, \
                                        (const float*)nullptr, sumsq, Pt, mvec, (T*)out, HW, C, eps, (int)cpi, vpc); \
            else hipLaunchKernelGGL((grn_apply_kernel<T, false>), dim3(grid), dim3(256), lds, stream, (const T*)nullptr, (const T*)in, (const T*)nullptr, weight, \
                                    bias, sumsq, (const float*)nullptr, (float*)nullptr, (T*)out, HW, C, eps, (int)cpi, vpc); \
        } while (0)
        if (bf) GRN_APPLY(bf16_t); else GRN_APPLY(float);
#undef GRN_APPLY
        return nkb_check_launch("grn_apply");
    }
    if (mode == NKB_GRN_PARAM) {
        NkbProfScope prof(NKB_K_GRN_PARAM, stream, 4.0 * N * C, 3.0 * tab + 4.0 * N + 16.0 * C);
        hipLaunchKernelGGL(grn_param_kernel, dim3(C / GRN_CG), dim3(256), 0, stream, sumsq, Pt, Qt, mvec, dweight, dbias, N, C);
        return nkb_check_launch("grn_param");
    }
    nkb_set_error("grn: bad mode %d", mode);
    return 1;
}
