// Softmax cross-entropy / focal loss (forward + backward) and the logger's softmax+argmax,
// one wave per logits row, wave-shuffle reductions, fp32 throughout.
// Semantics follow torch's CrossEntropyLoss(weight) "mean" (weighted mean) and the reference's FocalLoss
// (/root/reference/nkb_classification/losses.py:59-94): rows whose label == ignore_index are dropped.
#include "common.h"

struct LossRow {
    float loss;   // per-row loss numerator (already multiplied by its class weight / focal term)
    float wsum;   // per-row contribution to the normaliser (class weight for CE, 1 for focal, 0 if ignored)
    float coef;   // d(row loss)/d(logit_j) = coef * (p_j - [j == y])   (before the 1/normaliser)
};

__device__ __forceinline__ bool argmax_takes(float v, int j, float mx, int am) {
    return v > mx || (v != v && mx == mx) || ((v == mx || (v != v && mx != mx)) && j < am);
}

// kind: 0 = CrossEntropy(weight), 1 = Focal(alpha, gamma); their mixed forms have a kernel of their own below
__global__ void loss_fwd_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target, int B,
                                int C, int kind, const float* __restrict__ cls_w, float gamma, long long ignore_index,
                                float* __restrict__ probs, int ldp, int* __restrict__ argmax, LossRow* __restrict__ rows) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* x = logits + (size_t)row * ld;
    float mx = -INFINITY;
    int am = 0x7fffffff;
    // torch.argmax: the first maximum, a NaN above every number and the first NaN among several.  Equal candidates (equal values,
    // or two NaNs) go to the smaller index, so a row of -inf ends at column 0 and a lane without a column (am = INT_MAX) never wins
    for (int j = lane; j < C; j += 64) {
        const float v = x[j];
        if (argmax_takes(v, j, mx, am)) { mx = v; am = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (argmax_takes(om, oa, mx, am)) { mx = om; am = oa; }
    }
    float se = 0.f;
    for (int j = lane; j < C; j += 64) se += expf(x[j] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    const float inv = 1.f / se;
    if (probs) for (int j = lane; j < C; j += 64) probs[(size_t)row * ldp + j] = expf(x[j] - mx) * inv;
    if (lane == 0) {
        if (argmax) argmax[row] = am;
        if (rows) {
            const long long y = target[row];
            LossRow r = {0.f, 0.f, 0.f};
            if (y != ignore_index && (y < 0 || y >= C)) {
                // label outside [0, C): torch's nll_loss raises a device-side assert here.  No assert channel exists in a
                // sync-free step, so the row poisons the loss with NaN instead of being dropped silently.
                r.loss = __builtin_nanf(""); r.wsum = 1.f; r.coef = __builtin_nanf("");
            } else if (y != ignore_index) {
                const float logpt = x[y] - lse;
                const float w = cls_w ? cls_w[y] : 1.f;
                if (kind == 0) {
                    r.loss = -w * logpt; r.wsum = w; r.coef = w;
                } else {
                    const float pt = expf(logpt);
                    const float om = 1.f - pt;
                    const float f = powf(om, gamma);
                    // d/dz of -w (1-pt)^g log pt  =  w * [(1-pt)^g - g pt log(pt) (1-pt)^(g-1)] * (p - onehot)
                    // (1-pt)^(g-1) * log(pt) -> 0 as pt -> 1 for every g > 0 (log pt ~ -(1-pt)); evaluated literally it is
                    // inf * 0 = NaN for 0 < g < 1 at pt == 1
                    const float fm1 = (gamma == 0.f || om <= 0.f) ? 0.f : gamma * powf(om, gamma - 1.f);
                    r.loss = -w * f * logpt; r.wsum = 1.f; r.coef = w * (f - fm1 * pt * logpt);
                }
            }
            rows[row] = r;
        }
    }
}

// ---- the mixed form (kind | NKB_LOSS_MIXED; contract and operation order in include/nkbhip.h) ------------------------------------
// Two labels and a weight per row (Mixup / CutMix) and, for cross entropy, label smoothing.  row_state = B of these records, then the
// C floats ew[j] = (eps / C) * w_j the backward pass subtracts (it gets neither the class weights nor eps).
struct LossRowMixed {
    float loss;   // per-row numerator
    float wsum;   // per-row contribution to the normaliser (0 for a dropped row)
    float A;      // sum of the row's target coefficients a_c
    float c1;     // coefficient on column y
    float c2;     // coefficient on column y2
    int sm;       // 1: the row takes the smoothing term ew (kept row, eps > 0)
    int pad[2];   // 0
};
static_assert(sizeof(LossRowMixed) == 32, "nkbhip.h documents 32 bytes per row");

// today's focal terms of one label: loss = (-w f) log pt, coef = w (f - (fm1 pt) log pt)
__device__ __forceinline__ void focal_label(float logpt, float w, float gamma, float& loss, float& coef) {
    const float pt = expf(logpt);
    const float om = 1.f - pt;
    const float f = powf(om, gamma);
    const float fm1 = (gamma == 0.f || om <= 0.f) ? 0.f : gamma * powf(om, gamma - 1.f);
    loss = -w * f * logpt;
    coef = w * (f - fm1 * pt * logpt);
}

// target: int64 [3][B] = y, y2, float64 bits of lam.  gamma: eps for kind 0, gamma for kind 1.  epsC = eps / C (0 for focal).
__global__ void loss_fwd_mixed_kernel(const float* __restrict__ logits, int ld, const long long* __restrict__ target, int B,
                                      int C, int kind, const float* __restrict__ cls_w, float gamma, float epsC,
                                      long long ignore_index, float* __restrict__ probs, int ldp, int* __restrict__ argmax,
                                      LossRowMixed* __restrict__ rows) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* x = logits + (size_t)row * ld;
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int j = lane; j < C; j += 64) {
        const float v = x[j];
        if (argmax_takes(v, j, mx, am)) { mx = v; am = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (argmax_takes(om, oa, mx, am)) { mx = om; am = oa; }
    }
    float se = 0.f;
    for (int j = lane; j < C; j += 64) se += expf(x[j] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    const float inv = 1.f / se;
    if (probs) for (int j = lane; j < C; j += 64) probs[(size_t)row * ldp + j] = expf(x[j] - mx) * inv;
    if (lane == 0 && argmax) argmax[row] = am;
    if (!rows) return;
    float* ew = (float*)(rows + B);
    if (row == 0) for (int j = lane; j < C; j += 64) ew[j] = cls_w ? epsC * cls_w[j] : epsC;
    const long long y = target[row], y2 = target[(size_t)B + row];
    const bool ign = y == ignore_index || y2 == ignore_index;
    const bool bad = !ign && (y < 0 || y >= C || y2 < 0 || y2 >= C);
    const bool smooth = kind == 0 && epsC > 0.f && !ign && !bad;
    // S = sum_j ew_j log p_j and SW = sum_j ew_j: each lane its columns in rising order, then the wave's butterfly
    float S = 0.f, SW = 0.f;
    if (smooth) {                                       // uniform over the wave: one row per wave
        for (int j = lane; j < C; j += 64) {
            const float e = cls_w ? epsC * cls_w[j] : epsC;
            S += e * (x[j] - lse);
            SW += e;
        }
        S = wave_sum(S);
        SW = wave_sum(SW);
    }
    if (lane != 0) return;
    LossRowMixed r = {0.f, 0.f, 0.f, 0.f, 0.f, 0, {0, 0}};
    if (bad) {
        r.loss = __builtin_nanf(""); r.wsum = 1.f; r.A = r.c1 = r.c2 = __builtin_nanf("");
    } else if (!ign) {
        const float lam = (float)__longlong_as_double(target[2 * (size_t)B + row]);
        const float oml = 1.f - lam;
        const float lp1 = x[y] - lse, lp2 = x[y2] - lse;
        const float w1 = cls_w ? cls_w[y] : 1.f, w2 = cls_w ? cls_w[y2] : 1.f;
        if (kind == 0) {
            const float keep = 1.f - gamma;             // 1 - eps
            r.c1 = lam * keep * w1;
            r.c2 = oml * keep * w2;
            const float hard = r.c1 * lp1 + r.c2 * lp2;
            r.loss = smooth ? -(hard + S) : -hard;
            r.A = smooth ? r.c1 + r.c2 + SW : r.c1 + r.c2;
            r.wsum = lam * w1 + oml * w2;
            r.sm = smooth ? 1 : 0;
        } else {
            float l1, l2, k1, k2;
            focal_label(lp1, w1, gamma, l1, k1);
            focal_label(lp2, w2, gamma, l2, k2);
            r.loss = lam * l1 + oml * l2;
            r.c1 = lam * k1;
            r.c2 = oml * k2;
            r.A = r.c1 + r.c2;
            r.wsum = 1.f;
        }
    }
    rows[row] = r;
}

// reduction 0 ("mean"): out[0] = sum(loss)/sum(wsum) (0 when every row is ignored), out[1] = 1/sum(wsum) (0 when empty)
// reduction 1 ("sum") / 2 ("none"): out[0] = sum(loss), out[1] = 1 — the per-row factor of the backward pass
// rows: records of `stride` floats (3: LossRow, 8: LossRowMixed) that begin with loss, wsum
__global__ void loss_reduce_kernel(const float* __restrict__ rows, int stride, int B, float* __restrict__ out, int reduction) {
    __shared__ float s0[4], s1[4];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) { a += rows[(size_t)i * stride]; b += rows[(size_t)i * stride + 1]; }
    a = wave_sum(a); b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { s0[threadIdx.x >> 6] = a; s1[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = s0[0] + s0[1] + s0[2] + s0[3];
        b = s1[0] + s1[1] + s1[2] + s1[3];
        if (reduction == 0) {
            out[0] = b > 0.f ? a / b : 0.f;
            out[1] = b > 0.f ? 1.f / b : 0.f;
        } else {
            out[0] = a;
            out[1] = 1.f;
        }
    }
}

// dlogits[i][j] = gout[i * gout_stride] * rows[i].coef * out[1] * (p_ij - [j == y_i])   (gout_stride 0: scalar loss)
__global__ void loss_bwd_kernel(const float* __restrict__ probs, int ldp, const long long* __restrict__ target,
                                const LossRow* __restrict__ rows, const float* __restrict__ red,
                                const float* __restrict__ gout, int gout_stride, int B, int C,
                                float* __restrict__ dlogits, int ldd) {
    const size_t total = (size_t)B * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % C), r = (int)(i / C);
        const float p = probs[(size_t)r * ldp + j];
        const float g = gout[(size_t)r * gout_stride] * red[1];
        dlogits[(size_t)r * ldd + j] = g * rows[r].coef * (p - (target[r] == j ? 1.f : 0.f));
    }
}

// dlogits[i][j] = g * (((A p_ij - c1 [j == y_i]) - c2 [j == y2_i]) - ew_j [sm_i]),  g = gout[i * gout_stride] * out[1]
__global__ void loss_bwd_mixed_kernel(const float* __restrict__ probs, int ldp, const long long* __restrict__ target,
                                      const LossRowMixed* __restrict__ rows, const float* __restrict__ red,
                                      const float* __restrict__ gout, int gout_stride, int B, int C,
                                      float* __restrict__ dlogits, int ldd) {
    const float* __restrict__ ew = (const float*)(rows + B);
    const size_t total = (size_t)B * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % C), r = (int)(i / C);
        const float p = probs[(size_t)r * ldp + j];
        const float g = gout[(size_t)r * gout_stride] * red[1];
        const LossRowMixed q = rows[r];
        float t = q.A * p;
        if (target[r] == j) t = t - q.c1;
        if (target[(size_t)B + r] == j) t = t - q.c2;
        if (q.sm) t = t - ew[j];
        dlogits[(size_t)r * ldd + j] = g * t;
    }
}

extern "C" int nkb_loss_forward(int kind, const float* logits, int ld, const long long* target, int B, int C,
                                const float* class_weight, float gamma, long long ignore_index, float* probs, int ldp,
                                int* argmax, void* row_state, float* out2, int reduction, hipStream_t stream) {
    if ((unsigned)reduction > 2u) { nkb_set_error("loss_forward: reduction %d (0 mean, 1 sum, 2 none)", reduction); return 1; }
    const bool mixed = kind == (NKB_LOSS_MIXED | 0) || kind == (NKB_LOSS_MIXED | 1);
    if ((unsigned)kind > 1u && !mixed) {
        nkb_set_error("loss_forward: kind %d (0 cross entropy, 1 focal, | %d the mixed form of either)", kind, NKB_LOSS_MIXED);
        return 1;
    }
    if (mixed && kind == NKB_LOSS_MIXED && !(gamma >= 0.f && gamma < 1.f)) {
        nkb_set_error("loss_forward: label smoothing %g outside [0, 1)", (double)gamma);
        return 1;
    }
    if (B < 0 || C < 0) { nkb_set_error("loss_forward: negative extent (B %d, C %d)", B, C); return 1; }
    if (row_state && !target) { nkb_set_error("loss_forward: row_state needs target"); return 1; }
    if (B == 0 || C == 0) return 0;
    NkbProfScope prof(NKB_K_LOSS, stream, 0);
    if (mixed) {
        const int base = kind & ~NKB_LOSS_MIXED;
        hipLaunchKernelGGL(loss_fwd_mixed_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, logits, ld, target, B, C, base,
                           class_weight, gamma, base == 0 ? gamma / (float)C : 0.f, ignore_index, probs, ldp, argmax,
                           (LossRowMixed*)row_state);
    } else {
        hipLaunchKernelGGL(loss_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, logits, ld, target, B, C, kind,
                           class_weight, gamma, ignore_index, probs, ldp, argmax, (LossRow*)row_state);
    }
    if (row_state && out2)
        hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, stream, (const float*)row_state,
                           (int)((mixed ? sizeof(LossRowMixed) : sizeof(LossRow)) / sizeof(float)), B, out2, reduction);
    return nkb_check_launch("loss_forward");
}
extern "C" size_t nkb_loss_row_state_bytes(int B) { return (size_t)B * sizeof(LossRow); }

extern "C" int nkb_loss_backward(const float* probs, int ldp, const long long* target, const void* row_state,
                                 const float* out2, const float* grad_out, int grad_out_per_row, int B, int C,
                                 float* dlogits, int ldd, hipStream_t stream) {
    if (B < 0 || C < 0) { nkb_set_error("loss_backward: negative extent (B %d, C %d)", B, C); return 1; }
    if ((unsigned)grad_out_per_row > 3u) {
        nkb_set_error("loss_backward: grad_out_per_row %d (bit 0 per-row grad_out, bit 1 mixed records)", grad_out_per_row);
        return 1;
    }
    if (B == 0 || C == 0) return 0;
    NkbProfScope prof(NKB_K_LOSS, stream, 0);
    size_t g = ((size_t)B * C + 255) / 256;
    if (g > 2048) g = 2048;
    if (grad_out_per_row & 2)
        hipLaunchKernelGGL(loss_bwd_mixed_kernel, dim3((unsigned)g), dim3(256), 0, stream, probs, ldp, target,
                           (const LossRowMixed*)row_state, out2, grad_out, grad_out_per_row & 1, B, C, dlogits, ldd);
    else
        hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)g), dim3(256), 0, stream, probs, ldp, target,
                           (const LossRow*)row_state, out2, grad_out, grad_out_per_row & 1, B, C, dlogits, ldd);
    return nkb_check_launch("loss_backward");
}
