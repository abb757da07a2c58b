// Channel attention of the SE / ECA members of the ResNet family (timm SEModule / EcaModule between the closing BatchNorm of a block and
// its residual add; reached through timm.create_model("seresnet*" / "ecaresnet*") at nkb_classification/model.py:82 of the reference),
// forward and backward, fp32 and bf16.
//
// c: raw output of the closing convolution, [N][HW][C] rows (NHWC); bnvec = [scale | shift | mean | invstd] of its BatchNorm (absent in
// eval mode: the folded convolution delivered y already, scale = 1, shift = 0); y = c scale + shift is never written.
//   cm[b][ch] = mean_p c         z = scale cm + shift        SE:  h = relu(W1 z + b1), s = sigmoid(W2 h + b2)
//                                                            ECA: s = sigmoid(sum_j w[j] z[ch + j - pad]), zero padded
//   out = relu(y s[b] + r), r the shortcut (finished, or rnd(res rscale + rshift) as in nkb_bn_apply), ReLU bits in nkb_bn_apply's format
// backward, g the gradient of out, gm = g under the bits, M = N HW:
//   A[b] = sum_p gm     B[b] = sum_p gm c     ds = (scale B + shift A) s (1 - s)
//   SE:  dW2 += ds^T h, db2 += sum_b ds, dh = (ds W2) [h > 0], dW1 += dh^T z, db1 += sum_b dh, dz = dh W1
//   ECA: dw[j] += sum_{b,ch} ds[b][ch] z[b][ch + j - pad],  dz[b][ch] = sum_j w[j] ds[b][ch - j + pad]
//   S1 = sum_b (s A + dz)     S2 = sum_b (s (B - mean A) + dz (cm - mean))       (the BatchNorm-backward sums, without a pass of their own)
//   dc = scale (gm s[b] + dz[b] / HW - S1 / M - (c - mean) invstd^2 S2 / M)       dgamma += invstd S2, dbeta += S1
//
// Kernels; all sums, gates, excitation weights and their gradients fp32, every summation order a function of the shape alone (no float
// atomics, nothing depends on the grid):
//   se_reduce     one work item per (image, 64-channel group), walked by a grid-stride loop (the layout of grn_reduce): a thread owns one
//                 16-byte chunk of channels and every LP-th pixel; forward cm, backward A and B from one read of g, c and the bits.
//   se_gate       forward gate, SE_IPG images per workgroup: z of the group in LDS, every row of W1 / W2 read once per group.
//   se_gate_bwd   per-image half of the gate's backward (ds, dh, dz), same grouping; se_param the cross-image half: one workgroup per 64
//                 channels and 32 hidden units sums S1, S2, db2 and its tiles of dW2 / dW1 over the images in image order (ECA: the tap
//                 sums of its channels, which se_eca_dw adds up in workgroup order).
//   se_apply      one workgroup per (image, chunk of the image's elements): per-channel coefficient tables of the image in LDS, then one
//                 streaming pass with 16-byte loads and stores.  Forward out = relu(c a + b + r) with the bits; backward dc = k1 gm + k2 c + k3.
#include "prims.h"

#define SE_CG 64                     // channels per reduce work item / per parameter workgroup
#define SE_MAX_C 2048
#define SE_MAX_RD 128
#define SE_MAX_K 9
#define SE_IPG 4                     // images per gate workgroup (z of the group: SE_IPG * SE_MAX_C floats of LDS)
#define SE_PB 16                     // images staged per step of the parameter sums
#define SE_JS 32                     // hidden units per parameter workgroup
#define SE_PART 16                   // floats per workgroup row of the ECA partial tap sums (k <= 9)

__device__ __forceinline__ float se_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void se_reduce_kernel(const T* __restrict__ g, const T* __restrict__ c, const unsigned char* __restrict__ bits,
                                                        float* __restrict__ out1, float* __restrict__ out2, int HW, int C, long long items) {
    constexpr int EPC = Chunk<T>::N, LC = SE_CG / EPC, LP = 256 / LC;
    __shared__ float red[(BWD ? 2 : 1) * 256 * EPC];
    const int tc = threadIdx.x % LC, tp = threadIdx.x / LC;
    const int CGs = C / SE_CG, cpr = C / EPC;
    const float inv = 1.f / (float)HW;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / CGs), cg = (int)(item % CGs);
        const size_t base = (size_t)b * HW * C + cg * SE_CG + tc * EPC;
        const size_t bbase = (size_t)b * HW * cpr + cg * LC + tc;
        float acc1[EPC], acc2[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc1[e] = acc2[e] = 0.f;
#pragma unroll 4
        for (int p = tp; p < HW; p += LP) {
            float cf[EPC], gf[EPC];
            Chunk<T>::load(c + base + (size_t)p * C, cf);
            if (BWD) {
                Chunk<T>::load(g + base + (size_t)p * C, gf);
                const unsigned m = bits[bbase + (size_t)p * cpr];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float gm = ((m >> e) & 1u) ? gf[e] : 0.f;
                    acc1[e] += gm;
                    acc2[e] = fmaf(gm, cf[e], acc2[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc1[e] += cf[e];
            }
        }
        __syncthreads();                 // (the previous item's readers are done with red)
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            red[threadIdx.x * EPC + e] = acc1[e];
            if (BWD) red[(256 + threadIdx.x) * EPC + e] = acc2[e];
        }
        __syncthreads();
        if (threadIdx.x < SE_CG) {
            const int lc = threadIdx.x / EPC, e = threadIdx.x % EPC;
            float s1 = 0.f, s2 = 0.f;
            for (int j = 0; j < LP; ++j) {
                s1 += red[(j * LC + lc) * EPC + e];
                if (BWD) s2 += red[(256 + j * LC + lc) * EPC + e];
            }
            const size_t o = (size_t)b * C + cg * SE_CG + threadIdx.x;
            out1[o] = BWD ? s1 : s1 * inv;
            if (BWD) out2[o] = s2;
        }
    }
}

// z of the group's images into LDS (zero rows behind the last image)
__device__ __forceinline__ void se_load_z(float (*zs)[SE_MAX_C], const float* __restrict__ bnvec, const float* __restrict__ cm, int b0, int nb,
                                          int C) {
    for (int c = threadIdx.x; c < C; c += 256) {
        const float sc = bnvec ? bnvec[c] : 1.f, sh = bnvec ? bnvec[C + c] : 0.f;
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) zs[i][c] = i < nb ? fmaf(sc, cm[(size_t)(b0 + i) * C + c], sh) : 0.f;
    }
}

// k == 0: SE (W1 [rd][C], b1 [rd], W2 [C][rd], b2 [C]; h [N][rd] is kept); k > 0: ECA (W1 = the k taps)
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ bnvec, const float* __restrict__ W1, const float* __restrict__ b1,
                                                      const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ cm,
                                                      float* __restrict__ s, float* __restrict__ h, int N, int C, int rd, int k) {
    __shared__ __attribute__((aligned(16))) float zs[SE_IPG][SE_MAX_C];
    __shared__ __attribute__((aligned(16))) float hs[SE_IPG][SE_MAX_RD];
    const int b0 = blockIdx.x * SE_IPG, nb = min(SE_IPG, N - b0);
    se_load_z(zs, bnvec, cm, b0, nb, C);
    __syncthreads();
    if (k > 0) {
        const int pad = (k - 1) / 2;
        float w[SE_MAX_K];
#pragma unroll
        for (int j = 0; j < SE_MAX_K; ++j) w[j] = j < k ? W1[j] : 0.f;
        for (int c = threadIdx.x; c < C; c += 256)
            for (int i = 0; i < nb; ++i) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < SE_MAX_K; ++j) {
                    const int cc = c + j - pad;
                    if (j < k && cc >= 0 && cc < C) a = fmaf(w[j], zs[i][cc], a);
                }
                s[(size_t)(b0 + i) * C + c] = se_sigmoid(a);
            }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < rd; j += 4) {
        float acc[SE_IPG];
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) acc[i] = 0.f;
#pragma unroll 8
        for (int c = lane * 4; c < C; c += 256) {             // (unrolled: the loop is bound by the latency of its one load otherwise)
            const f32x4 w4 = *(const f32x4*)(W1 + (size_t)j * C + c);
#pragma unroll
            for (int i = 0; i < SE_IPG; ++i) {
                const f32x4 z4 = *(const f32x4*)(&zs[i][c]);
                acc[i] = fmaf(w4[0], z4[0], fmaf(w4[1], z4[1], fmaf(w4[2], z4[2], fmaf(w4[3], z4[3], acc[i]))));
            }
        }
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) acc[i] = wave_sum(acc[i]);
        if (lane == 0) {
            const float bj = b1[j];
#pragma unroll
            for (int i = 0; i < SE_IPG; ++i) {
                const float v = fmaxf(acc[i] + bj, 0.f);
                hs[i][j] = v;
                if (i < nb) h[(size_t)(b0 + i) * rd + j] = v;
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc[SE_IPG];
        const float bc = b2[c];
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) acc[i] = bc;
#pragma unroll 8
        for (int j = 0; j < rd; j += 4) {
            const f32x4 w4 = *(const f32x4*)(W2 + (size_t)c * rd + j);
#pragma unroll
            for (int i = 0; i < SE_IPG; ++i)
                acc[i] = fmaf(w4[0], hs[i][j], fmaf(w4[1], hs[i][j + 1], fmaf(w4[2], hs[i][j + 2], fmaf(w4[3], hs[i][j + 3], acc[i]))));
        }
        for (int i = 0; i < nb; ++i) s[(size_t)(b0 + i) * C + c] = se_sigmoid(acc[i]);
    }
}

// per-image half of the gate's backward: ds, dh (SE), dz
__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const float* __restrict__ bnvec, const float* __restrict__ W1, const float* __restrict__ W2,
                                                          const float* __restrict__ s, const float* __restrict__ h, const float* __restrict__ A,
                                                          const float* __restrict__ B, float* __restrict__ ds, float* __restrict__ dh,
                                                          float* __restrict__ dz, int N, int C, int rd, int k) {
    __shared__ __attribute__((aligned(16))) float dss[SE_IPG][SE_MAX_C];
    __shared__ __attribute__((aligned(16))) float red[256 * 4 * SE_IPG];
    __shared__ float dhs[SE_IPG][SE_MAX_RD];
    const int b0 = blockIdx.x * SE_IPG, nb = min(SE_IPG, N - b0);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float sc = bnvec ? bnvec[c] : 1.f, sh = bnvec ? bnvec[C + c] : 0.f;
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) {
            float v = 0.f;
            if (i < nb) {
                const size_t o = (size_t)(b0 + i) * C + c;
                const float sv = s[o];
                v = fmaf(sc, B[o], sh * A[o]) * (sv * (1.f - sv));
                ds[o] = v;
            }
            dss[i][c] = v;
        }
    }
    __syncthreads();
    if (k > 0) {
        const int pad = (k - 1) / 2;
        float w[SE_MAX_K];
#pragma unroll
        for (int j = 0; j < SE_MAX_K; ++j) w[j] = j < k ? W1[j] : 0.f;
        for (int c = threadIdx.x; c < C; c += 256)
            for (int i = 0; i < nb; ++i) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < SE_MAX_K; ++j) {
                    const int cc = c - j + pad;
                    if (j < k && cc >= 0 && cc < C) a = fmaf(w[j], dss[i][cc], a);
                }
                dz[(size_t)(b0 + i) * C + c] = a;
            }
        return;
    }
    // dh[i][j] = (sum_c ds[i][c] W2[c][j]) [h > 0]: a thread owns four hidden units and every ncl-th channel; the ncl partial sums of a
    // unit are added in lane order through LDS
    const int q4 = rd / 4, ncl = 256 / q4;
    const int q = threadIdx.x % q4, cl = threadIdx.x / q4;
    if (cl < ncl) {
        float acc[SE_IPG][4];
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
#pragma unroll 4
        for (int c = cl; c < C; c += ncl) {
            const f32x4 w4 = *(const f32x4*)(W2 + (size_t)c * rd + q * 4);
#pragma unroll
            for (int i = 0; i < SE_IPG; ++i) {
                const float d = dss[i][c];
                acc[i][0] = fmaf(d, w4[0], acc[i][0]); acc[i][1] = fmaf(d, w4[1], acc[i][1]);
                acc[i][2] = fmaf(d, w4[2], acc[i][2]); acc[i][3] = fmaf(d, w4[3], acc[i][3]);
            }
        }
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(cl * SE_IPG + i) * rd + q * 4 + e] = acc[i][e];       // [ncl][SE_IPG][rd]: ncl * rd <= 256 * 4
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SE_IPG * rd; t += 256) {
        const int i = t / rd, j = t % rd;
        float a = 0.f;
        for (int l = 0; l < ncl; ++l) a += red[(l * SE_IPG + i) * rd + j];
        float v = 0.f;
        if (i < nb) {
            v = h[(size_t)(b0 + i) * rd + j] > 0.f ? a : 0.f;
            dh[(size_t)(b0 + i) * rd + j] = v;
        }
        dhs[i][j] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc[SE_IPG];
#pragma unroll
        for (int i = 0; i < SE_IPG; ++i) acc[i] = 0.f;
#pragma unroll 8
        for (int j = 0; j < rd; ++j) {
            const float w = W1[(size_t)j * C + c];
#pragma unroll
            for (int i = 0; i < SE_IPG; ++i) acc[i] = fmaf(dhs[i][j], w, acc[i]);
        }
        for (int i = 0; i < nb; ++i) dz[(size_t)(b0 + i) * C + c] = acc[i];
    }
}

// sum of the four image lanes of a channel, lanes in order; the caller has written red[lane * 64 + channel] and synchronised
__device__ __forceinline__ float se_lane4(const float* red, int t) { return ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t]; }

// cross-image half: S1, S2 (always), and the parameter gradients ("+=") of the 64 channels (x) the <= 32 hidden units of this workgroup
// (blockIdx.y walks the hidden units in slices of 32; slice 0 also owns S1, S2 and db2).  ECA: the workgroup leaves the tap sums of its 64
// channels in `part`, se_eca_dw_kernel adds the workgroups' rows in order
__global__ __launch_bounds__(256) void se_param_kernel(const float* __restrict__ bnvec, const float* __restrict__ cm, const float* __restrict__ s,
                                                       const float* __restrict__ h, const float* __restrict__ A, const float* __restrict__ B,
                                                       const float* __restrict__ ds, const float* __restrict__ dh, const float* __restrict__ dz,
                                                       float* __restrict__ S1, float* __restrict__ S2, float* __restrict__ dW1,
                                                       float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2,
                                                       float* __restrict__ part, int N, int C, int rd, int k) {
    __shared__ float red[3 * 256];
    __shared__ __attribute__((aligned(16))) float dsl[SE_PB][SE_CG], zl[SE_PB][SE_CG], hl[SE_PB][SE_JS], dhl[SE_PB][SE_JS];
    const int c0 = blockIdx.x * SE_CG;
    const int cl = threadIdx.x & 63, jq = threadIdx.x >> 6;
    if (blockIdx.y == 0) {
        const int c = c0 + cl;
        const float mean = bnvec ? bnvec[2 * C + c] : 0.f;
        float a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int b = jq; b < N; b += 4) {
            const size_t o = (size_t)b * C + c;
            const float sv = s[o], av = A[o], dzv = dz[o];
            a1 += fmaf(sv, av, dzv);
            a2 += fmaf(sv, B[o] - mean * av, dzv * (cm[o] - mean));
            a3 += ds[o];
        }
        red[threadIdx.x] = a1; red[256 + threadIdx.x] = a2; red[512 + threadIdx.x] = a3;
        __syncthreads();
        if (jq == 0) {
            S1[c] = se_lane4(red, threadIdx.x);
            S2[c] = se_lane4(red + 256, threadIdx.x);
            if (db2) db2[c] += se_lane4(red + 512, threadIdx.x);
        }
    }
    if (k > 0) {
        // ECA taps: sum_{b, ch in this workgroup} ds[b][ch] z[b][ch + j - pad]: a thread owns one channel and every fourth image
        if (!dW1) return;
        const int pad = (k - 1) / 2, c = c0 + cl;
        float acc[SE_MAX_K];
#pragma unroll
        for (int j = 0; j < SE_MAX_K; ++j) acc[j] = 0.f;
        for (int b = jq; b < N; b += 4) {
            const size_t row = (size_t)b * C;
            const float d = ds[row + c];
#pragma unroll
            for (int j = 0; j < SE_MAX_K; ++j) {
                const int cc = c + j - pad;
                if (j < k && cc >= 0 && cc < C) {
                    const float z = bnvec ? fmaf(bnvec[cc], cm[row + cc], bnvec[C + cc]) : cm[row + cc];
                    acc[j] = fmaf(d, z, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SE_MAX_K; ++j) {
            if (j < k) {                                        // (k is uniform: every thread meets the barriers)
                const float v = wave_sum(acc[j]);
                __syncthreads();
                if (cl == 0) red[jq] = v;
                __syncthreads();
                if (threadIdx.x == 0) part[blockIdx.x * SE_PART + j] = ((red[0] + red[1]) + red[2]) + red[3];
            }
        }
        return;
    }
    if (!dW2) return;
    // dW2[c][j] += sum_b ds[b][c] h[b][j] and dW1[j][c] += sum_b dh[b][j] z[b][c]: a thread owns one channel and njt = 2 .. 8 consecutive
    // hidden units of both tiles and walks the images in order, SE_PB of them staged in LDS at a time (its channel's ds and z: one
    // read each per image; the hidden units' h and dh: wave-uniform 8-byte reads)
    const int jb = blockIdx.y * SE_JS, njb = min(SE_JS, rd - jb), njt = njb / 4, j0 = jq * njt;
    float a2[SE_JS / 4], a1[SE_JS / 4];
#pragma unroll
    for (int e = 0; e < SE_JS / 4; ++e) a2[e] = a1[e] = 0.f;
    for (int bb = 0; bb < N; bb += SE_PB) {
        const int pb = min(SE_PB, N - bb);
        __syncthreads();
        for (int t = threadIdx.x; t < pb * SE_CG; t += 256) {
            const int i = t / SE_CG, c = t % SE_CG;
            const size_t o = (size_t)(bb + i) * C + c0 + c;
            dsl[i][c] = ds[o];
            zl[i][c] = bnvec ? fmaf(bnvec[c0 + c], cm[o], bnvec[C + c0 + c]) : cm[o];
        }
        for (int t = threadIdx.x; t < pb * njb; t += 256) {
            const int i = t / njb, j = t % njb;
            hl[i][j] = h[(size_t)(bb + i) * rd + jb + j];
            dhl[i][j] = dh[(size_t)(bb + i) * rd + jb + j];
        }
        __syncthreads();
        for (int i = 0; i < pb; ++i) {
            const float d = dsl[i][cl], zz = zl[i][cl];
#pragma unroll
            for (int e = 0; e < SE_JS / 4; e += 2) {
                if (e < njt) {
                    const nkb_f2 hv = *(const nkb_f2*)(&hl[i][j0 + e]), dv = *(const nkb_f2*)(&dhl[i][j0 + e]);
                    a2[e] = fmaf(d, hv[0], a2[e]); a2[e + 1] = fmaf(d, hv[1], a2[e + 1]);
                    a1[e] = fmaf(dv[0], zz, a1[e]); a1[e + 1] = fmaf(dv[1], zz, a1[e + 1]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < SE_JS / 4; ++e) {
        if (e < njt) {
            const int j = jb + j0 + e;
            dW2[(size_t)(c0 + cl) * rd + j] += a2[e];
            dW1[(size_t)j * C + c0 + cl] += a1[e];
        }
    }
    if (blockIdx.x == 0 && db1 && threadIdx.x < njb) {
        float a = 0.f;
        for (int b = 0; b < N; ++b) a += dh[(size_t)b * rd + jb + threadIdx.x];
        db1[jb + threadIdx.x] += a;
    }
}

// dw[j] += the workgroups' partial tap sums, in workgroup order
__global__ void se_eca_dw_kernel(const float* __restrict__ part, int nblk, int k, float* __restrict__ dw) {
    if ((int)threadIdx.x >= k) return;
    float a = 0.f;
    for (int i = 0; i < nblk; ++i) a += part[i * SE_PART + threadIdx.x];
    dw[threadIdx.x] += a;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void se_apply_kernel(const T* __restrict__ g, const T* __restrict__ c, const T* __restrict__ res,
                                                       const float* __restrict__ bnvec, const float* __restrict__ rvec,
                                                       const float* __restrict__ s, const float* __restrict__ dz, const float* __restrict__ S1,
                                                       const float* __restrict__ S2, unsigned char* __restrict__ bits,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, T* __restrict__ out, int HW, int C,
                                                       float inv_hw, float inv_m, int cpi, long long vpc) {
    constexpr int EPC = Chunk<T>::N;
    extern __shared__ __attribute__((aligned(16))) float se_tab[];     // 4 C floats, sized by the launch
    float* t0 = se_tab;             // forward: scale s      backward: k1 = scale s
    float* t1 = se_tab + C;         // forward: shift s      backward: k2 = -scale invstd^2 S2 / M
    float* t2 = se_tab + 2 * C;     // forward: rscale       backward: k3 = scale (dz / HW - S1 / M + mean invstd^2 S2 / M)
    float* t3 = se_tab + 3 * C;     // forward: rshift
    const int b = blockIdx.x / cpi, k = blockIdx.x % cpi;
    for (int ch = threadIdx.x; ch < C; ch += 256) {
        const float sc = bnvec ? bnvec[ch] : 1.f, sh = bnvec ? bnvec[C + ch] : 0.f;
        const float sv = s[(size_t)b * C + ch];
        if (BWD) {
            const float mean = bnvec[2 * C + ch], is = bnvec[3 * C + ch];
            const float q = is * is * S2[ch] * inv_m;
            t0[ch] = sc * sv;
            t1[ch] = -sc * q;
            t2[ch] = sc * (fmaf(dz[(size_t)b * C + ch], inv_hw, -S1[ch] * inv_m) + mean * q);
            if (blockIdx.x == 0) {                              // the BatchNorm's own parameter gradients ride along, once
                if (dgamma) dgamma[ch] += is * S2[ch];
                if (dbeta) dbeta[ch] += S1[ch];
            }
        } else {
            t0[ch] = sc * sv;
            t1[ch] = sh * sv;
            if (rvec) { t2[ch] = rvec[ch]; t3[ch] = rvec[C + ch]; }
        }
    }
    __syncthreads();
    const long long nv = (long long)HW * C / EPC;
    const long long v0 = k * vpc, v1 = min(nv, v0 + vpc);
    const size_t img = (size_t)b * HW * C;
    const int step = (256 * EPC) % C;
    int ch = (int)(((v0 + threadIdx.x) * EPC) % C);
#pragma unroll 2
    for (long long v = v0 + threadIdx.x; v < v1; v += 256) {
        const size_t off = img + (size_t)v * EPC;
        float cf[EPC], xf[EPC], of[EPC];
        Chunk<T>::load(c + off, cf);
        if (BWD) {
            Chunk<T>::load(g + off, xf);
            const unsigned m = bits[off / EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float gm = ((m >> e) & 1u) ? xf[e] : 0.f;
                of[e] = fmaf(t0[ch + e], gm, fmaf(t1[ch + e], cf[e], t2[ch + e]));
            }
        } else {
            Chunk<T>::load(res + off, xf);
            unsigned m = 0u;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float r = rvec ? DT<T>::rnd(fmaf(xf[e], t2[ch + e], t3[ch + e])) : xf[e];
                const float v2 = fmaxf(fmaf(cf[e], t0[ch + e], t1[ch + e]) + r, 0.f);
                of[e] = v2;
                m |= (DT<T>::rnd(v2) > 0.f ? 1u : 0u) << e;
            }
            if (bits) bits[off / EPC] = (unsigned char)m;
        }
        Chunk<T>::store(out + off, of);
        ch += step;
        if (ch >= C) ch -= C;
    }
}

// fp32 block of one closing stage (hip.se_workspace lays it out the same way): six [N][C] tables, two [C] vectors, C / 4 floats of partial
// tap sums (ECA), then two [N][rd] tables
struct SeWs {
    float *cm, *s, *A, *B, *dz, *ds, *S1, *S2, *part, *h, *dh;
};
static long long se_ws_floats(int N, int C, int rd) { return 6ll * N * C + 2ll * C + C / SE_CG * SE_PART + 2ll * N * rd; }
static SeWs se_ws(float* w, int N, int C, int rd) {
    const size_t nc = (size_t)N * C;
    SeWs r;
    r.cm = w; r.s = w + nc; r.A = w + 2 * nc; r.B = w + 3 * nc; r.dz = w + 4 * nc; r.ds = w + 5 * nc;
    r.S1 = w + 6 * nc; r.S2 = r.S1 + C; r.part = r.S2 + C; r.h = r.part + C / SE_CG * SE_PART; r.dh = r.h + (size_t)N * rd;
    return r;
}

// The channel-attention passes of nkb_avgpool (modes NKB_SE_*, include/nkbhip.h); every argument is checked before anything is launched.
int nkb_se(int dtype, int mode, const void* in, void* out, int N, int HW, int C, const void* in2, const float* weight, const float* bias,
           float* sumsq, float* dweight, float* dbias, const void* mul, float* workspace, long long workspace_floats, hipStream_t stream) {
    (void)mul;
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) { nkb_set_error("se: bad dtype %d", dtype); return 1; }
    if (C < SE_CG || C % SE_CG != 0 || C > SE_MAX_C) {
        nkb_set_error("se: C=%d must be a multiple of %d up to %d", C, SE_CG, SE_MAX_C);
        return 1;
    }
    const bool se_gate = mode == NKB_SE_GATE || mode == NKB_SE_BWD_GATE, eca_gate = mode == NKB_ECA_GATE || mode == NKB_ECA_BWD_GATE;
    const bool gate = se_gate || eca_gate;
    int rd = 0, k = 0;
    if (gate) {                                    // the gates act on [N][C]: the HW slot carries rd (SE) or k (ECA)
        if (N < 1) { nkb_set_error("se: N=%d must be positive", N); return 1; }
        if (se_gate) {
            rd = HW;
            if (rd < 8 || rd % 8 != 0 || rd > SE_MAX_RD) {
                nkb_set_error("se: rd=%d must be a multiple of 8 up to %d", rd, SE_MAX_RD);
                return 1;
            }
        } else {
            k = HW;
            if (k < 1 || k % 2 == 0 || k > SE_MAX_K) { nkb_set_error("se: k=%d must be odd, 1 .. %d", k, SE_MAX_K); return 1; }
        }
    } else if (N < 1 || HW < 1 || (long long)N * HW * C >= (1ll << 31)) {
        nkb_set_error("se: N=%d x HW=%d x C=%d outside 1 .. 2^31 elements", N, HW, C);
        return 1;
    }
    const long long need = se_ws_floats(N, C, rd);
    if (!workspace || workspace_floats < need) {
        nkb_set_error("se: mode %d: workspace of %lld floats given, %lld needed", mode, workspace ? workspace_floats : 0ll, need);
        return 1;
    }
    const SeWs w = se_ws(workspace, N, C, rd);
    const bool bf = dtype == NKB_DT_BF16;
    const double esz = bf ? 2.0 : 4.0, el = (double)N * HW * C, tab = 4.0 * N * C;
    if (mode == NKB_SE_POOL || mode == NKB_SE_BWD_REDUCE) {
        const bool bwd = mode == NKB_SE_BWD_REDUCE;
        if (!in) { nkb_set_error("se: mode %d needs its input tensor", mode); return 1; }
        if (bwd && (!in2 || !sumsq)) { nkb_set_error("se: the backward reduction needs c (in2) and the ReLU bits (sumsq slot)"); return 1; }
        const long long items = (long long)N * (C / SE_CG);
        const long long cap = (long long)nkb_cu_count() * 8;
        const unsigned grid = (unsigned)(items < cap ? items : cap);
        NkbProfScope prof(bwd ? NKB_K_BN_BWD_REDUCE : NKB_K_AVGPOOL, stream, (bwd ? 3.0 : 1.0) * el,
                          bwd ? 2.0 * esz * el + el / (bf ? 8 : 4) + 2.0 * tab : esz * el + tab);
#define SE_REDUCE(T) do { \
            if (bwd) hipLaunchKernelGGL((se_reduce_kernel<T, true>), dim3(grid), dim3(256), 0, stream, (const T*)in, (const T*)in2, \
                                        (const unsigned char*)sumsq, w.A, w.B, HW, C, items); \
            else hipLaunchKernelGGL((se_reduce_kernel<T, false>), dim3(grid), dim3(256), 0, stream, (const T*)nullptr, (const T*)in, \
                                    (const unsigned char*)nullptr, w.cm, (float*)nullptr, HW, C, items); \
        } while (0)
        if (bf) SE_REDUCE(bf16_t); else SE_REDUCE(float);
#undef SE_REDUCE
        return nkb_check_launch("se_reduce");
    }
    if (mode == NKB_SE_GATE || mode == NKB_ECA_GATE) {
        if (!in || (se_gate && (!in2 || !bias || !mul))) {
            nkb_set_error("se: mode %d needs %s", mode, se_gate ? "W1 (in), W2 (in2), b1 (bias) and b2 (mul)" : "the taps (in)");
            return 1;
        }
        NkbProfScope prof(NKB_K_MISC, stream, se_gate ? 4.0 * N * C * rd : 2.0 * N * C * k, 2.0 * tab);
        hipLaunchKernelGGL(se_gate_kernel, dim3((N + SE_IPG - 1) / SE_IPG), dim3(256), 0, stream, weight, (const float*)in, bias,
                           (const float*)in2, (const float*)mul, w.cm, w.s, w.h, N, C, rd, k);
        return nkb_check_launch("se_gate");
    }
    if (mode == NKB_SE_BWD_GATE || mode == NKB_ECA_BWD_GATE) {
        if (!in || (se_gate && !in2)) { nkb_set_error("se: mode %d needs %s", mode, se_gate ? "W1 (in) and W2 (in2)" : "the taps (in)"); return 1; }
        if (se_gate && (!out != !dweight)) { nkb_set_error("se: dW1 (out) and dW2 (dweight) come together or not at all"); return 1; }
        NkbProfScope prof(NKB_K_MISC, stream, se_gate ? 8.0 * N * C * rd : 4.0 * N * C * k, 8.0 * tab);
        hipLaunchKernelGGL(se_gate_bwd_kernel, dim3((N + SE_IPG - 1) / SE_IPG), dim3(256), 0, stream, weight, (const float*)in,
                           (const float*)in2, w.s, w.h, w.A, w.B, w.ds, w.dh, w.dz, N, C, rd, k);
        hipLaunchKernelGGL(se_param_kernel, dim3(C / SE_CG, se_gate ? (rd + SE_JS - 1) / SE_JS : 1), dim3(256), 0, stream, weight, w.cm, w.s,
                           w.h, w.A, w.B, w.ds, w.dh, w.dz, w.S1, w.S2, se_gate ? (float*)out : dweight, se_gate ? sumsq : (float*)nullptr,
                           se_gate ? dweight : (float*)nullptr, se_gate ? dbias : (float*)nullptr, w.part, N, C, rd, k);
        if (eca_gate && dweight) hipLaunchKernelGGL(se_eca_dw_kernel, dim3(1), dim3(64), 0, stream, w.part, C / SE_CG, k, dweight);
        return nkb_check_launch("se_gate_bwd");
    }
    if (mode == NKB_SE_FWD_APPLY || mode == NKB_SE_BWD_APPLY) {
        const bool bwd = mode == NKB_SE_BWD_APPLY;
        if (!in || !in2 || !out) { nkb_set_error("se: mode %d needs in, in2 and out", mode); return 1; }
        if (bwd && (!weight || !sumsq)) { nkb_set_error("se: the backward apply needs the BatchNorm vectors (weight) and the ReLU bits (sumsq slot)"); return 1; }
        const long long nv = (long long)HW * C / (bf ? 8 : 4);
        long long cpi = ((long long)nkb_cu_count() * 8 + N - 1) / N, most = (nv + 1023) / 1024;      // >= 4 chunks per thread where the image has them
        if (cpi > most) cpi = most;
        if (cpi < 1) cpi = 1;
        const long long vpc = (nv + cpi - 1) / cpi;
        cpi = (nv + vpc - 1) / vpc;
        const unsigned grid = (unsigned)(N * cpi);
        const size_t lds = 4 * sizeof(float) * (size_t)C;
        const float inv_hw = 1.f / (float)HW, inv_m = 1.f / ((float)N * (float)HW);
        NkbProfScope prof(bwd ? NKB_K_BN_BWD_APPLY : NKB_K_BN_APPLY, stream, 3.0 * el, 3.0 * esz * el + el / (bf ? 8 : 4) + tab);
#define SE_APPLY(T) do { \
            if (bwd) hipLaunchKernelGGL((se_apply_kernel<T, true>), dim3(grid), dim3(256), lds, stream, (const T*)in, (const T*)in2, (const T*)nullptr, \
                                        weight, (const float*)nullptr, w.s, w.dz, w.S1, w.S2, (unsigned char*)sumsq, dweight, dbias, (T*)out, HW, C, \
                                        inv_hw, inv_m, (int)cpi, vpc); \
            else hipLaunchKernelGGL((se_apply_kernel<T, false>), dim3(grid), dim3(256), lds, stream, (const T*)nullptr, (const T*)in, (const T*)in2, \
                                    weight, bias, w.s, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (unsigned char*)sumsq, \
                                    (float*)nullptr, (float*)nullptr, (T*)out, HW, C, inv_hw, inv_m, (int)cpi, vpc); \
        } while (0)
        if (bf) SE_APPLY(bf16_t); else SE_APPLY(float);
#undef SE_APPLY
        return nkb_check_launch("se_apply");
    }
    nkb_set_error("se: bad mode %d", mode);
    return 1;
}
