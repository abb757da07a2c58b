// Device side of the input pipeline: the tail of the reference's albumentations stack that is
// pure per-pixel arithmetic — PadIfNeeded(size, size, border_mode=CONSTANT, value=fill, centred) -> HorizontalFlip /
// VerticalFlip -> Normalize(mean, std, max_pixel_value=255) -> ToTensorV2 (HWC -> CHW), configs/singletask_config.py:
// 162-219 — run on the uint8 batch after the H2D copy, so the host hands over 1 byte per channel instead of 4
// (38 MB instead of 154 MB per 256 x 3 x 224 x 224 batch; engine.py:40 `img.to(device)` moves fp32).
//
//   out[b][c][y][x] = (P[b][yf][xf][c] - 255 mean[c]) * (1 / (255 std[c])),   yf / xf = y / x mirrored when flagged,
//   P = the (h_b x w_b) image centred in Ho x Wo (top = (Ho - h) / 2, left = (Wo - w) / 2, as PadIfNeeded) over `fill`.
//
// HBM-bound: 3 B read + 12 B written per output pixel.  One thread = 4 consecutive x of one row, all three channels:
// 12 source bytes (byte loads; neighbouring lanes cover neighbouring bytes) and three 16-byte stores, one per plane, where
// Wo % 4 == 0 and `out` is 16-byte aligned (every row of every plane then is); element stores otherwise.
//
// Flag bit 2 marks an image with an augmentation record behind the flag bytes (include/nkbhip.h): its pixels go through
// RandomBrightnessContrast -> HueSaturationValue -> CoarseDropout on uint8 levels between the load and the normalise step of
// the same thread, so the colour augmentations of the stack cost no HBM traffic of their own.
#include "common.h"

namespace {

// ---- augmentation records (flag bit 2; layout in include/nkbhip.h) ---------------------------------------------------------------
// RandomBrightnessContrast -> HueSaturationValue -> CoarseDropout of the reference stack on uint8 LEVELS of the padded, flipped
// canvas, every fp32 step its own operation (the build has -ffp-contract=off) so that tests/image_aug_reference.py reproduces
// the levels in numpy float32.  The HSV conversions restate OpenCV's 8-bit ones: integer forward conversion with the two
// 4096-scaled divisor tables, float inverse conversion.
constexpr int kRecWords = 64, kMaxHoles = 12;

// sdiv[v] = rint(255 * 4096 / v), hdiv[d] = rint(180 * 4096 / (6 d)), entry 0 = 0.  Neither quotient can end in .5 (that needs
// 2^13 | v), so the integer round-half-up is rint.  Constant memory rather than LDS: the plain path then pays nothing for them —
// no fill and no barrier in front of the first load; the 2 KB stay in the vector L1 for the lanes that index them.
struct DivTable { int v[256]; };
constexpr DivTable make_div_table(int num) {
    DivTable t{};
    for (int i = 1; i < 256; ++i) t.v[i] = (2 * num + i) / (2 * i);
    return t;
}
__constant__ DivTable kSdiv = make_div_table(255 * 4096), kHdiv = make_div_table(30 * 4096);

// albumentations' uint8 LUT: clip(level * alpha + beta * 255), truncated
__device__ __forceinline__ int aug_brightness_contrast(int P, float alpha, float offset) {
    float t = (float)P;
    if (alpha != 1.f) t = t * alpha;
    if (offset != 0.f) t = t + offset;
    return (int)fminf(fmaxf(t, 0.f), 255.f);
}

__device__ __forceinline__ int aug_level(float x) { return (int)fminf(fmaxf(rintf(x * 255.f), 0.f), 255.f); }

// r, g, b in 0..255 (so v and d index the 256-entry tables in range)
__device__ __forceinline__ void aug_hsv(int& r, int& g, int& b, float hue, float sat, float val) {
    const int v = max(r, max(g, b)), d = v - min(r, min(g, b));
    int s = (d * kSdiv.v[v] + 2048) >> 12;
    const int hraw = v == r ? g - b : v == g ? b - r + 2 * d : r - g + 4 * d;
    int h = (hraw * kHdiv.v[d] + 2048) >> 12;
    if (h < 0) h += 180;
    float m = fmodf((float)h + hue, 180.f);
    if (m < 0.f) m = m + 180.f;
    h = (int)m;
    if (h >= 180) h -= 180;
    s = (int)fminf(fmaxf((float)s + sat, 0.f), 255.f);
    const int v2 = (int)fminf(fmaxf((float)v + val, 0.f), 255.f);
    const float hf = (float)h * (6.f / 180.f), sf = (float)s * (1.f / 255.f), vf = (float)v2 * (1.f / 255.f);
    if (s == 0) {
        r = g = b = aug_level(vf);
        return;
    }
    const float fs = floorf(hf), f = hf - fs;
    const int sector = min(max((int)fs, 0), 5);
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
    float fb, fg, fr;        // (b, g, r) = tab[{{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}[sector]]
    switch (sector) {
        case 0: fb = t1; fg = t3; fr = t0; break;
        case 1: fb = t1; fg = t0; fr = t2; break;
        case 2: fb = t3; fg = t0; fr = t1; break;
        case 3: fb = t0; fg = t2; fr = t1; break;
        case 4: fb = t0; fg = t1; fr = t3; break;
        default: fb = t2; fg = t1; fr = t0; break;
    }
    r = aug_level(fr);
    g = aug_level(fg);
    b = aug_level(fb);
}

// One 4-pixel group of image k at output row y, groups gx: source bytes -> the value the un-mixed kernel writes there (plain(k) of
// include/nkbhip.h), from k's own sizes, pad, flips (fl bits 0, 1) and augmentation record (fl bit 2).  Bit 3 of fl is not looked at.
__device__ __forceinline__ void prep_group(const unsigned char* __restrict__ src, const int* __restrict__ sizes,
                                           const int* __restrict__ table, int k, unsigned fl, int y, int gx, int Hs, int Ws, int Ho,
                                           int Wo, float m0, float m1, float m2, float r0, float r1, float r2, float fill,
                                           float (&v)[3][4]) {
    const int h = sizes ? sizes[2 * k] : Hs, w = sizes ? sizes[2 * k + 1] : Ws;
    const int top = (Ho - h) / 2, left = (Wo - w) / 2;
    const int yf = (fl & 2u) ? Ho - 1 - y : y;
    const int sy = yf - top;
    const bool row_in = (unsigned)sy < (unsigned)h;
    const unsigned char* row = src + ((size_t)k * Hs + (row_in ? sy : 0)) * Ws * 3;
    // the 12 source bytes are loaded and turned into the plain path's values in straight-line code, exactly as without records;
    // lanes of an image with a record (per lane: a wave can straddle two images) then redo the arithmetic from the bytes
    int q[3][4];
    bool in[4];
    float p[3][4];                                  // the value Normalize sees: a level, or `fill` itself on the plain path
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = gx * 4 + j;
        const int xf = (fl & 1u) ? Wo - 1 - x : x;
        const int sx = xf - left;
        in[j] = row_in && (unsigned)sx < (unsigned)w && x < Wo;
        const unsigned char* px = row + (in[j] ? sx : 0) * 3;
        q[0][j] = px[0]; q[1][j] = px[1]; q[2][j] = px[2];
        p[0][j] = in[j] ? (float)q[0][j] : fill;
        p[1][j] = in[j] ? (float)q[1][j] : fill;
        p[2][j] = in[j] ? (float)q[2][j] : fill;
    }
    if (fl & 4u) {
        const int padlv = (int)fminf(fmaxf(fill, 0.f), 255.f);
        const int* __restrict__ rec = table + (size_t)kRecWords * k;
        const int mask = rec[0];
        const float alpha = __int_as_float(rec[1]), offset = __int_as_float(rec[2]);
        const float hue = __int_as_float(rec[3]), sat = __int_as_float(rec[4]), val = __int_as_float(rec[5]);
        const bool bc = mask & 1, hsv = (mask & 2) && (hue != 0.f || sat != 0.f || val != 0.f);
        int lv[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int cr = in[j] ? q[0][j] : padlv, cg = in[j] ? q[1][j] : padlv, cb = in[j] ? q[2][j] : padlv;
            if (bc) {
                cr = aug_brightness_contrast(cr, alpha, offset);
                cg = aug_brightness_contrast(cg, alpha, offset);
                cb = aug_brightness_contrast(cb, alpha, offset);
            }
            if (hsv) aug_hsv(cr, cg, cb, hue, sat, val);
            lv[0][j] = cr; lv[1][j] = cg; lv[2][j] = cb;
        }
        if (mask & 4) {                             // CoarseDropout: boxes in output-canvas coordinates, half-open
            const int n = min(max(rec[6], 0), kMaxHoles);
            const int f0 = rec[7], f1 = rec[8], f2 = rec[9];
            for (int t = 0; t < n; ++t) {
                const int y1 = rec[16 + 4 * t], x1 = rec[17 + 4 * t], y2 = rec[18 + 4 * t], x2 = rec[19 + 4 * t];
                if (y < y1 || y >= y2) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = gx * 4 + j;
                    if (x >= x1 && x < x2) { lv[0][j] = f0; lv[1][j] = f1; lv[2][j] = f2; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { p[0][j] = (float)lv[0][j]; p[1][j] = (float)lv[1][j]; p[2][j] = (float)lv[2][j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[0][j] = (p[0][j] - m0) * r0;
        v[1][j] = (p[1][j] - m1) * r1;
        v[2][j] = (p[2][j] - m2) * r2;
    }
}

__global__ __launch_bounds__(256) void image_prep_kernel(const unsigned char* __restrict__ src, const int* __restrict__ sizes,
                                                         const unsigned char* __restrict__ flags, float* __restrict__ out,
                                                         int B, int Hs, int Ws, int Ho, int Wo, float m0, float m1, float m2,
                                                         float r0, float r1, float r2, float fill, bool vec) {
    const int* __restrict__ table = (const int*)(flags + (((size_t)B + 15) & ~(size_t)15));     // dereferenced only behind bit 2 / 3
    const int xg = (Wo + 3) >> 2;                       // 4-pixel groups per row
    const long long total = (long long)B * Ho * xg;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int gx = (int)(i % xg);
        const int y = (int)((i / xg) % Ho);
        const int b = (int)(i / ((long long)xg * Ho));
        const unsigned fl = flags ? flags[b] : 0u;
        // flag bit 3: words 10..15 of record b mix image b with a partner.  take = the pixels of the group that come from the
        // partner (box), 0xF for a blend; an image is evaluated only where one of its pixels is used, so a box costs one evaluation
        // per pixel but in the groups its vertical edges cut.  A partner outside [0, B), the image itself or an unknown mode: no mix.
        int partner = b, mode = 0;
        unsigned take = 0u;
        float lam = 1.f, oml = 0.f;
        if (fl & 8u) {
            const int* __restrict__ rec = table + (size_t)kRecWords * b;
            const int p = rec[10], md = rec[11];
            if ((unsigned)p < (unsigned)B && p != b) {
                if (md == 1) {
                    partner = p; mode = 1; take = 0xFu;
                    lam = __int_as_float(rec[12]); oml = __int_as_float(rec[13]);
                } else if (md == 2) {
                    const int y1 = rec[12], x1 = rec[13], y2 = rec[14], x2 = rec[15];
                    if (y >= y1 && y < y2) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int x = gx * 4 + j;
                            if (x >= x1 && x < x2) take |= 1u << j;
                        }
                    }
                    if (take) { partner = p; mode = 2; }
                }
            }
        }
        float v[3][4];
        if (mode != 2 || take != 0xFu)
            prep_group(src, sizes, table, b, fl, y, gx, Hs, Ws, Ho, Wo, m0, m1, m2, r0, r1, r2, fill, v);
        if (mode) {
            float u[3][4];
            prep_group(src, sizes, table, partner, flags[partner], y, gx, Hs, Ws, Ho, Wo, m0, m1, m2, r0, r1, r2, fill, u);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (mode == 1) {
                        const float tb = lam * v[c][j], tp = oml * u[c][j];     // two multiplies and one add (no contraction)
                        v[c][j] = tb + tp;
                    } else if (take >> j & 1u) {
                        v[c][j] = u[c][j];
                    }
                }
        }
        const size_t plane = (size_t)Ho * Wo;
        float* o = out + (size_t)b * 3 * plane + (size_t)y * Wo + gx * 4;
        if (vec) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *(f32x4*)(o + c * plane) = (f32x4){v[c][0], v[c][1], v[c][2], v[c][3]};
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx * 4 + j < Wo) o[c * plane + j] = v[c][j];
        }
    }
}

}  // namespace

extern "C" int nkb_image_prep(const unsigned char* src, const int* sizes, const unsigned char* flags, float* out, int B,
                              int Hs, int Ws, int Ho, int Wo, const float* mean, const float* stdev, float fill,
                              hipStream_t stream) {
    if (B < 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || Hs > Ho || Ws > Wo) {
        nkb_set_error("image_prep: source %dx%d must fit the %dx%d output", Hs, Ws, Ho, Wo);
        return 1;
    }
    if (!mean || !stdev || stdev[0] == 0.f || stdev[1] == 0.f || stdev[2] == 0.f) { nkb_set_error("image_prep: bad mean / std"); return 1; }
    if (B == 0) return 0;
    NkbProfScope prof(NKB_K_MISC, stream, 0, (double)B * Ho * Wo * 15.0);
    // Normalize of the reference stack: img = (img - mean * 255) * (1 / (std * 255)) in float32
    const float m0 = mean[0] * 255.f, m1 = mean[1] * 255.f, m2 = mean[2] * 255.f;
    const float r0 = 1.f / (stdev[0] * 255.f), r1 = 1.f / (stdev[1] * 255.f), r2 = 1.f / (stdev[2] * 255.f);
    const long long total = (long long)B * Ho * ((Wo + 3) / 4);
    long long g = (total + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)g), dim3(256), 0, stream, src, sizes, flags, out, B, Hs, Ws, Ho, Wo,
                       m0, m1, m2, r0, r1, r2, fill, (Wo & 3) == 0 && ((uintptr_t)out & 15) == 0);
    return nkb_check_launch("image_prep");
}
