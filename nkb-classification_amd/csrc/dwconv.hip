// Depthwise 7x7 convolution (stride 1, pad 3, NHWC) and the per-channel layer scale of the ConvNeXt block
// (timm.create_model("convnext_*") at nkb_classification/model.py:82 of the reference).
//
// A depthwise filter never mixes channels and NHWC puts the channels innermost, so LANES ARE CHANNELS: a wave owns 64 consecutive
// channels of a strip of DW_TW output columns of one image, over a chunk of output rows.  Every lane keeps its channel's 49 taps in
// registers for the whole launch.  The rows are walked once, input row by input row: the row that arrives (DW_TW + 6 values per lane,
// one coalesced 64-channel load each) is multiplied into the seven output rows it reaches, whose accumulators (7 x DW_TW) roll through
// registers; the row that became complete is stored and its slot restarts at the bias.  No LDS, no cross-lane traffic; the halo columns
// of the neighbouring strips are re-read through L2.  Registers per lane: 49 taps + 49 accumulators + 13 row values (+ addressing).
//
// The data gradient is the same kernel with the taps read back to front (w[6-r][6-s]) and no bias (+ add: the residual path's gradient).  The weight gradient walks the same
// way with the roles swapped: seven rows of the output gradient roll through registers (7 x DW_TW), the 49 (+1 for the bias)
// accumulators stay put, and each wave leaves its sums in a slab of its own; the slabs are added in split order by the common reducer
// (no float atomics: two launches give the same bits).
#include "common.h"

#define DW_R 7
#define DW_PAD 3
#define DW_TW 7                      // output columns per strip
#define DW_IN (DW_TW + DW_R - 1)     // input columns a strip reads
#define DW_ROWS 14                   // output rows per chunk (6 halo rows are re-read per chunk)
#define DW_WAVES 2048                // weight gradient: waves in flight (splits x channel groups)

struct DwGeom {
    int strips, chunks, rpc;
    long long items;                 // (image, row chunk, column strip) work items
};
static DwGeom dw_geom(int N, int H, int W) {
    DwGeom g;
    g.strips = (W + DW_TW - 1) / DW_TW;
    g.chunks = (H + DW_ROWS - 1) / DW_ROWS;
    g.rpc = (H + g.chunks - 1) / g.chunks;
    g.chunks = (H + g.rpc - 1) / g.rpc;          // (every chunk holds at least one row)
    g.items = (long long)N * g.chunks * g.strips;
    return g;
}

template <typename T>
__global__ __launch_bounds__(256) void dwconv_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     const T* __restrict__ add, T* __restrict__ y, int H, int W, int C, int ldx, int ldy, int strips, int chunks,
                                                     int rpc, int flip, long long units) {
    const int lane = threadIdx.x & 63;
    long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= units) return;                      // (no barrier below: a whole wave may leave)
    const int CG = C >> 6;
    const int cg = (int)(u % CG); u /= CG;
    const int strip = (int)(u % strips); u /= strips;
    const int chunk = (int)(u % chunks);
    const int n = (int)(u / chunks);
    const int c = cg * 64 + lane;
    float tap[DW_R * DW_R];
#pragma unroll
    for (int j = 0; j < DW_R * DW_R; ++j) tap[j] = w[(size_t)c * (DW_R * DW_R) + (flip ? DW_R * DW_R - 1 - j : j)];
    const float b = bias ? bias[c] : 0.f;
    const int p0 = chunk * rpc, rows = min(rpc, H - p0), q0 = strip * DW_TW;
    const T* xb = x + (size_t)n * H * W * ldx + c;
    T* yb = y + (size_t)n * H * W * ldy + c;
    const T* ab = add ? add + (size_t)n * H * W * ldy + c : nullptr;
    float acc[DW_R][DW_TW];
#pragma unroll
    for (int k = 0; k < DW_R; ++k)
#pragma unroll
        for (int q = 0; q < DW_TW; ++q) acc[k][q] = b;
    const int steps = rows + DW_R - 1;
    for (int i0 = 0; i0 < steps; i0 += DW_R) {
#pragma unroll
        for (int k = 0; k < DW_R; ++k) {          // output row o lives in slot o % 7 = (k - dr) % 7: static indices
            const int i = i0 + k;
            if (i < steps) {
                const int h = p0 - DW_PAD + i;
                if (h >= 0 && h < H) {
                    float xr[DW_IN];
#pragma unroll
                    for (int j = 0; j < DW_IN; ++j) {
                        const int col = q0 - DW_PAD + j;
                        xr[j] = (col >= 0 && col < W) ? DT<T>::ld(xb + ((size_t)h * W + col) * ldx) : 0.f;
                    }
#pragma unroll
                    for (int dr = 0; dr < DW_R; ++dr) {
                        const int o = i - dr;     // input row h is tap row dr of output row p0 + o
                        if (o >= 0 && o < rows) {
                            const int slot = (k - dr + DW_R) % DW_R;
#pragma unroll
                            for (int s = 0; s < DW_R; ++s)
#pragma unroll
                                for (int q = 0; q < DW_TW; ++q) acc[slot][q] = fmaf(tap[dr * DW_R + s], xr[q + s], acc[slot][q]);
                        }
                    }
                }
                const int o = i - (DW_R - 1);     // complete after this input row
                if (o >= 0) {
                    const int slot = (k + 1) % DW_R;
#pragma unroll
                    for (int q = 0; q < DW_TW; ++q) {
                        if (q0 + q < W) {
                            const size_t off = ((size_t)(p0 + o) * W + q0 + q) * ldy;
                            DT<T>::st(yb + off, ab ? acc[slot][q] + DT<T>::ld(ab + off) : acc[slot][q]);
                        }
                        acc[slot][q] = b;
                    }
                }
            }
        }
    }
}

// splits x (C / 64) waves; wave (split, cg) sums the work items split, split + splits, ... of its 64 channels
template <typename T>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const T* __restrict__ g, const T* __restrict__ x, float* __restrict__ part_w,
                                                           float* __restrict__ part_b, int H, int W, int C, int ldg, int ldx, int strips,
                                                           int chunks, int rpc, int splits, long long items) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int CG = C >> 6;
    if (wv >= (long long)splits * CG) return;
    const int cg = (int)(wv % CG), split = (int)(wv / CG);
    const int c = cg * 64 + lane;
    float acc[DW_R * DW_R];
    float accb = 0.f;
#pragma unroll
    for (int j = 0; j < DW_R * DW_R; ++j) acc[j] = 0.f;
    for (long long item = split; item < items; item += splits) {
        const int strip = (int)(item % strips);
        const int chunk = (int)((item / strips) % chunks);
        const int n = (int)(item / ((long long)strips * chunks));
        const int p0 = chunk * rpc, rows = min(rpc, H - p0), q0 = strip * DW_TW;
        const T* xb = x + (size_t)n * H * W * ldx + c;
        const T* gb = g + (size_t)n * H * W * ldg + c;
        float gr[DW_R][DW_TW];
#pragma unroll
        for (int k = 0; k < DW_R; ++k)
#pragma unroll
            for (int q = 0; q < DW_TW; ++q) gr[k][q] = 0.f;
        const int steps = rows + DW_R - 1;
        for (int i0 = 0; i0 < steps; i0 += DW_R) {
#pragma unroll
            for (int k = 0; k < DW_R; ++k) {
                const int i = i0 + k;
                if (i < steps) {
                    // gradient row o = i enters slot k (row i - 7, its previous tenant, was last read at step i - 1)
#pragma unroll
                    for (int q = 0; q < DW_TW; ++q) {
                        const float v = (i < rows && q0 + q < W) ? DT<T>::ld(gb + ((size_t)(p0 + i) * W + q0 + q) * ldg) : 0.f;
                        gr[k][q] = v;
                        accb += v;
                    }
                    const int h = p0 - DW_PAD + i;
                    if (h >= 0 && h < H) {
                        float xr[DW_IN];
#pragma unroll
                        for (int j = 0; j < DW_IN; ++j) {
                            const int col = q0 - DW_PAD + j;
                            xr[j] = (col >= 0 && col < W) ? DT<T>::ld(xb + ((size_t)h * W + col) * ldx) : 0.f;
                        }
#pragma unroll
                        for (int r = 0; r < DW_R; ++r) {
                            const int o = i - r;          // input row h is tap row r of gradient row p0 + o
                            if (o >= 0 && o < rows) {
                                const int slot = (k - r + DW_R) % DW_R;
#pragma unroll
                                for (int s = 0; s < DW_R; ++s)
#pragma unroll
                                    for (int q = 0; q < DW_TW; ++q) acc[r * DW_R + s] = fmaf(gr[slot][q], xr[q + s], acc[r * DW_R + s]);
                            }
                        }
                    }
                }
            }
        }
    }
    float* pw = part_w + (size_t)split * (DW_R * DW_R) * C + (size_t)c * (DW_R * DW_R);
#pragma unroll
    for (int j = 0; j < DW_R * DW_R; ++j) pw[j] = acc[j];
    part_b[(size_t)split * C + c] = accb;
}

static int dw_validate(const char* what, int dtype, int N, int H, int W, int C, int lda, int ldb, int R, int pad) {
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) { nkb_set_error("%s: bad dtype %d", what, dtype); return 1; }
    if (R != DW_R || pad != DW_PAD) {
        nkb_set_error("%s: the %dx%d filter with pad %d is the one instantiated (stride 1), got R=%d pad=%d", what, DW_R, DW_R, DW_PAD, R, pad);
        return 1;
    }
    if (C < 64 || C % 64 != 0) { nkb_set_error("%s: C=%d must be a multiple of 64 (lanes are channels)", what, C); return 1; }
    if (N < 1 || H < 1 || W < 1) { nkb_set_error("%s: empty tensor N=%d H=%d W=%d", what, N, H, W); return 1; }
    if (lda < C || ldb < C) { nkb_set_error("%s: row strides %d / %d must be >= C=%d", what, lda, ldb, C); return 1; }
    const long long px = (long long)N * H * W;
    if (px * lda >= (1ll << 31) || px * ldb >= (1ll << 31)) { nkb_set_error("%s: operand exceeds 2^31 elements", what); return 1; }
    return 0;
}

extern "C" int nkb_dwconv(int dtype, int dgrad, const void* x, const float* w, const float* bias, const void* add, void* y, int N, int H, int W, int C,
                          int ldx, int ldy, int R, int pad, hipStream_t stream) {
    if (dw_validate("dwconv", dtype, N, H, W, C, ldx, ldy, R, pad)) return 1;
    if (dgrad && bias) { nkb_set_error("dwconv: the data gradient takes no bias"); return 1; }
    const DwGeom g = dw_geom(N, H, W);
    const long long units = g.items * (C / 64);
    const long long blocks = (units + 3) / 4;
    if (blocks >= (1ll << 31)) { nkb_set_error("dwconv: grid too large"); return 1; }
    const double px = (double)N * H * W * C;
    NkbProfScope prof(dgrad ? NKB_K_DWCONV_DGRAD : NKB_K_DWCONV_FWD, stream, 2.0 * DW_R * DW_R * px,
                      (dtype == NKB_DT_BF16 ? 2.0 : 4.0) * (add ? 3.0 : 2.0) * px + 200.0 * C);
    if (dtype == NKB_DT_BF16)
        hipLaunchKernelGGL(dwconv_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)x, w, bias, (const bf16_t*)add, (bf16_t*)y, H, W, C,
                           ldx, ldy, g.strips, g.chunks, g.rpc, dgrad ? 1 : 0, units);
    else
        hipLaunchKernelGGL(dwconv_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)x, w, bias, (const float*)add, (float*)y, H, W, C,
                           ldx, ldy, g.strips, g.chunks, g.rpc, dgrad ? 1 : 0, units);
    nkb_count_launch(NKB_LAUNCH_DWCONV);
    return nkb_check_launch("dwconv");
}

static int dw_splits(const DwGeom& g, int C) {
    long long s = DW_WAVES / (C / 64);
    if (s < 1) s = 1;
    if (s > g.items) s = g.items;
    return (int)s;
}

extern "C" long long nkb_dwconv_wgrad_workspace_floats(int dtype, int N, int H, int W, int C, int R) {
    (void)dtype;
    if (N < 1 || H < 1 || W < 1 || C < 64 || C % 64 != 0 || R != DW_R) return 0;
    return (long long)dw_splits(dw_geom(N, H, W), C) * (DW_R * DW_R + 1) * C;
}

extern "C" int nkb_dwconv_wgrad(int dtype, const void* g, const void* x, float* dw, float* dbias, int N, int H, int W, int C, int ldg,
                                int ldx, int R, int pad, float* workspace, long long workspace_floats, hipStream_t stream) {
    if (dw_validate("dwconv_wgrad", dtype, N, H, W, C, ldg, ldx, R, pad)) return 1;
    const DwGeom gm = dw_geom(N, H, W);
    const int splits = dw_splits(gm, C);
    const long long need = (long long)splits * (DW_R * DW_R + 1) * C;
    if (!workspace || workspace_floats < need) {
        nkb_set_error("dwconv_wgrad: workspace of %lld floats given, %lld needed", workspace ? workspace_floats : 0ll, need);
        return 1;
    }
    float* part_b = workspace + (size_t)splits * (DW_R * DW_R) * C;
    const long long waves = (long long)splits * (C / 64);
    const double px = (double)N * H * W * C;
    int rc;
    {
        NkbProfScope prof(NKB_K_DWCONV_WGRAD, stream, 2.0 * (DW_R * DW_R + 0.5) * px, (dtype == NKB_DT_BF16 ? 4.0 : 8.0) * px + 4.0 * need);
        if (dtype == NKB_DT_BF16)
            hipLaunchKernelGGL(dwconv_wgrad_kernel<bf16_t>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)g,
                               (const bf16_t*)x, workspace, part_b, H, W, C, ldg, ldx, gm.strips, gm.chunks, gm.rpc, splits, gm.items);
        else
            hipLaunchKernelGGL(dwconv_wgrad_kernel<float>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, (const float*)g,
                               (const float*)x, workspace, part_b, H, W, C, ldg, ldx, gm.strips, gm.chunks, gm.rpc, splits, gm.items);
        rc = nkb_check_launch("dwconv_wgrad");
        nkb_count_launch(NKB_LAUNCH_DWCONV);
    }
    if (rc) return rc;
    NkbProfScope prof(NKB_K_WGRAD_REDUCE, stream, 0, 4.0 * ((double)splits + 2.0) * (DW_R * DW_R + 1) * C);
    const long long nw = (long long)(DW_R * DW_R) * C;
    if (!dbias) return nkb_launch_wgrad_reduce(workspace, nw, splits, dw, nw, /*assign=*/false, stream);
    return nkb_launch_wgrad_reduce2(workspace, nw, splits, dw, nw, part_b, C, dbias, C, /*assign=*/false, stream);
}

// ---------------------------------------------------------------------------------------------------
// Layer scale: forward out[m][c] = add[m][c] + gamma[c] * z[m][c]; backward out = gamma[c] * g[m][c] and
// dgamma[c] += sum_m g[m][c] * z[m][c] (per-block partial rows, then the ordered reducer).
template <typename T> struct V4;
template <> struct V4<float> {
    __device__ static __forceinline__ void ld(const float* p, float* f) { const f32x4 v = *(const f32x4*)p; f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; }
    __device__ static __forceinline__ void st(float* p, const float* f) { *(f32x4*)p = (f32x4){f[0], f[1], f[2], f[3]}; }
};
template <> struct V4<bf16_t> {
    __device__ static __forceinline__ void ld(const bf16_t* p, float* f) {
        const u32x2 v = *(const u32x2*)p;
        f[0] = __uint_as_float(v[0] << 16); f[1] = __uint_as_float(v[0] & 0xffff0000u);
        f[2] = __uint_as_float(v[1] << 16); f[3] = __uint_as_float(v[1] & 0xffff0000u);
    }
    __device__ static __forceinline__ void st(bf16_t* p, const float* f) { *(u32x2*)p = (u32x2){pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3])}; }
};

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void layer_scale_kernel(const T* __restrict__ z, const T* __restrict__ a, const float* __restrict__ gamma,
                                                          T* __restrict__ out, float* __restrict__ part, long long rows, int C, int bx, int by,
                                                          long long rpb) {
    __shared__ float red[256 * 4];
    const int V = C >> 2;
    const int tx = threadIdx.x % bx, ty = threadIdx.x / bx;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    for (int v0 = 0; v0 < V; v0 += bx) {
        const int v = v0 + tx;
        const bool active = v < V && ty < by;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (active) {
            const float gm[4] = {gamma[4 * v], gamma[4 * v + 1], gamma[4 * v + 2], gamma[4 * v + 3]};
            for (long long r = r0 + ty; r < r1; r += by) {
                const size_t off = (size_t)r * C + 4 * v;
                float zf[4], af[4] = {0.f, 0.f, 0.f, 0.f}, of[4];
                if (!BWD || part) V4<T>::ld(z + off, zf);
                if (a) V4<T>::ld(a + off, af);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (BWD) { of[e] = gm[e] * af[e]; if (part) acc[e] = fmaf(af[e], zf[e], acc[e]); }
                    else of[e] = fmaf(gm[e], zf[e], af[e]);
                }
                V4<T>::st(out + off, of);
            }
        }
        if (BWD && part) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) red[threadIdx.x * 4 + e] = acc[e];
            __syncthreads();
            if (active && ty == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = acc[e];
                    for (int yy = 1; yy < by; ++yy) s += red[(yy * bx + tx) * 4 + e];
                    part[(size_t)blockIdx.x * C + 4 * v + e] = s;
                }
            }
        }
    }
}

static void ls_geom(long long rows, int C, int* bx, int* by, int* blocks, long long* rpb) {
    const int V = C / 4;
    *bx = V < 256 ? V : 256;
    *by = 256 / *bx;
    long long nb = (rows + (long long)*by * 8 - 1) / ((long long)*by * 8);
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    *rpb = (rows + nb - 1) / nb;
    *blocks = (int)((rows + *rpb - 1) / *rpb);
}

extern "C" long long nkb_layer_scale_workspace_floats(long long rows, int C) {
    if (rows < 1 || C < 64 || C % 64 != 0) return 0;
    int bx, by, blocks; long long rpb;
    ls_geom(rows, C, &bx, &by, &blocks, &rpb);
    return (long long)blocks * C;
}

extern "C" int nkb_layer_scale(int dtype, int backward, const void* z, const void* a, const float* gamma, void* out, float* dgamma,
                               long long rows, int C, float* workspace, long long workspace_floats, hipStream_t stream) {
    if (dtype != NKB_DT_F32 && dtype != NKB_DT_BF16) { nkb_set_error("layer_scale: bad dtype %d", dtype); return 1; }
    if (C < 64 || C % 64 != 0) { nkb_set_error("layer_scale: C=%d must be a multiple of 64", C); return 1; }
    if (rows < 1 || rows * C >= (1ll << 31)) { nkb_set_error("layer_scale: rows=%lld x C=%d outside 1 .. 2^31 elements", rows, C); return 1; }
    if (backward && !a) { nkb_set_error("layer_scale: backward needs the incoming gradient"); return 1; }
    if (!backward && dgamma) { nkb_set_error("layer_scale: dgamma belongs to the backward pass"); return 1; }
    int bx, by, blocks; long long rpb;
    ls_geom(rows, C, &bx, &by, &blocks, &rpb);
    const long long need = (long long)blocks * C;
    if (dgamma && (!workspace || workspace_floats < need)) {
        nkb_set_error("layer_scale: workspace of %lld floats given, %lld needed", workspace ? workspace_floats : 0ll, need);
        return 1;
    }
    const double el = (double)rows * C, esz = dtype == NKB_DT_BF16 ? 2.0 : 4.0;
    float* part = dgamma ? workspace : nullptr;
    int rc;
    {
        NkbProfScope prof(NKB_K_LAYER_SCALE, stream, (backward && dgamma ? 3.0 : 2.0) * el, 3.0 * esz * el + (dgamma ? 4.0 * need : 0.0));
#define LS_LAUNCH(T, B) hipLaunchKernelGGL((layer_scale_kernel<T, B>), dim3(blocks), dim3(256), 0, stream, (const T*)z, (const T*)a, gamma, \
                                           (T*)out, part, rows, C, bx, by, rpb)
        if (dtype == NKB_DT_BF16) { if (backward) LS_LAUNCH(bf16_t, true); else LS_LAUNCH(bf16_t, false); }
        else { if (backward) LS_LAUNCH(float, true); else LS_LAUNCH(float, false); }
#undef LS_LAUNCH
        rc = nkb_check_launch("layer_scale");
        nkb_count_launch(NKB_LAUNCH_LAYER_SCALE);
    }
    if (rc || !dgamma) return rc;
    NkbProfScope prof(NKB_K_WGRAD_REDUCE, stream, 0, 4.0 * ((double)blocks + 2.0) * C);
    return nkb_launch_wgrad_reduce(workspace, C, blocks, dgamma, C, /*assign=*/false, stream);
}
