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
//
// Flag bit 4 marks an image with a geometry record in a second table behind the first: RandomResizedCrop (a crop box resampled onto
// the canvas by an integer bilinear filter), PadIfNeeded's BORDER_REFLECT_101 and MotionBlur (the mean over up to 16 taps) produce
// the canvas levels in place of the byte fetch, in front of the flips' successors: crop -> flips -> blur -> colour -> mix.  With
// flags the source canvas may be larger than the output, so that a crop cuts from more pixels than it writes.
//
// Grid: y walks the images, x the 4-pixel groups of one image, so everything that belongs to the image — sizes, flag byte, records,
// mixing partner — is uniform in a block and stays in scalar registers.
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

// ---- geometry records (flag bit 4; layout in include/nkbhip.h) ---------------------------------------------------------------------
// The canvas level of image k at (y, x) in front of the colour stages: stage canvas (integer bilinear resample of a crop box, or the
// centred pad stage with a constant or reflect-101 border) -> flips -> blur over the record's taps.  Integer arithmetic but for
// the three fp32 operations of a resample coordinate; every quotient of floats was divided on the host.  tests/image_geom_reference.py
// restates it.  The record and its taps are read from global memory where they are used: nothing here is indexed in registers.
constexpr int kGeomWords = 16, kMaxTaps = 16;

// i < 0 -> -i, i >= n -> 2 (n - 1) - i until in range; an extent below 2 has one index.  i stays within a canvas side + 127 of the
// range, so the loop ends after (that distance) / (n - 1) rounds, none or one for any image wider than its pad.
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n <= 1) return 0;
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// canvas coordinate X of one axis -> the two box indices and the 11-bit weight of the second; s = float32(n) / float32(N), host-divided
__device__ __forceinline__ void geom_axis(int X, float s, int n, int& i0, int& i1, int& c1) {
    const float f = ((float)X + 0.5f) * s - 0.5f;            // three operations (no contraction)
    const float fl = floorf(f);
    int i = (int)fl;
    float t = f - fl;
    if (i < 0) { i = 0; t = 0.f; }
    if (i >= n - 1) { i = n - 1; t = 0.f; }
    i0 = i;
    i1 = min(i + 1, n - 1);
    c1 = (int)rintf(t * 2048.f);
}

// step 1: C(yc, xc).  img = image k's Hs x Ws slot; every read is clamped into it, so a bad box or size reads wrong pixels, not
// outside the slot.
__device__ __forceinline__ void geom_stage(const unsigned char* __restrict__ img, const int* __restrict__ g, int gmask, int h, int w,
                                           int Hs, int Ws, int Ho, int Wo, int padlv, int yc, int xc, int (&lv)[3]) {
    if (gmask & 1) {
        const int y0 = g[1], x0 = g[2];
        int iy0, iy1, cy1, ix0, ix1, cx1;
        geom_axis(yc, __int_as_float(g[5]), g[3], iy0, iy1, cy1);
        geom_axis(xc, __int_as_float(g[6]), g[4], ix0, ix1, cx1);
        // the four corners one after the other (a rolled loop: one pixel's three bytes in flight at a time keeps the registers of
        // this path below what the record path needs); a corner of weight 0 — every second one of an axis that is copied — is skipped
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma nounroll
        for (int q = 0; q < 4; ++q) {
            const int wgt = ((q & 2) ? cy1 : 2048 - cy1) * ((q & 1) ? cx1 : 2048 - cx1);        // the four sum to 2^22
            if (wgt == 0) continue;
            const int r = min(max(y0 + ((q & 2) ? iy1 : iy0), 0), Hs - 1), cc = min(max(x0 + ((q & 1) ? ix1 : ix0), 0), Ws - 1);
            const unsigned char* px = img + (unsigned)((r * Ws + cc) * 3);
            a0 += wgt * px[0]; a1 += wgt * px[1]; a2 += wgt * px[2];
        }
        lv[0] = a0 >> 22; lv[1] = a1 >> 22; lv[2] = a2 >> 22;
    } else {
        int sy = yc - (Ho - h) / 2, sx = xc - (Wo - w) / 2;
        bool in = (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w;
        if (!in && (gmask & 4)) {
            sy = reflect101(sy, h);
            sx = reflect101(sx, w);
            in = true;
        }
        const unsigned char* px = img + ((size_t)min(max(sy, 0), Hs - 1) * Ws + min(max(sx, 0), Ws - 1)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) lv[c] = in ? (int)px[c] : padlv;
    }
}

// steps 2 and 3: flips, then the mean over the taps with reflect-101 at the canvas edge
__device__ __forceinline__ void geom_level(const unsigned char* __restrict__ img, const int* __restrict__ g, unsigned fl, int h, int w,
                                           int Hs, int Ws, int Ho, int Wo, int padlv, int y, int x, int (&lv)[3]) {
    const int gmask = g[0];
    if (gmask & 2) {
        const int n = min(max(g[7], 1), kMaxTaps);
        int acc0 = 0, acc1 = 0, acc2 = 0;
        for (int t = 0; t < n; ++t) {
            const int half = g[8 + (t >> 1)] >> ((t & 1) * 16);
            const int dy = (signed char)(half & 0xFF), dx = (signed char)((half >> 8) & 0xFF);
            const int yy = reflect101(y + dy, Ho), xx = reflect101(x + dx, Wo);
            int s[3];
            geom_stage(img, g, gmask, h, w, Hs, Ws, Ho, Wo, padlv, (fl & 2u) ? Ho - 1 - yy : yy, (fl & 1u) ? Wo - 1 - xx : xx, s);
            acc0 += s[0]; acc1 += s[1]; acc2 += s[2];
        }
        const unsigned d = 2u * (unsigned)n;                 // integer division: at most (2 * 16 * 255 + 16) / 2
        lv[0] = (int)((2u * (unsigned)acc0 + (unsigned)n) / d);
        lv[1] = (int)((2u * (unsigned)acc1 + (unsigned)n) / d);
        lv[2] = (int)((2u * (unsigned)acc2 + (unsigned)n) / d);
    } else {
        geom_stage(img, g, gmask, h, w, Hs, Ws, Ho, Wo, padlv, (fl & 2u) ? Ho - 1 - y : y, (fl & 1u) ? Wo - 1 - x : x, lv);
    }
}

// The canvas levels of the 4-pixel group gx of image k at row y, one pixel after the other through ONE copy of the level code; they
// come back as the bytes j of three registers (R, G, B), so the loop carries no more than those (shifts by j, nothing indexed at run
// time).  A pixel behind the row end repeats the last one; it is never stored.
__device__ __forceinline__ void geom_group(const unsigned char* __restrict__ src, const int* __restrict__ sizes,
                                           const int* __restrict__ table, int B, int k, unsigned fl, int y, int gx, int Hs, int Ws,
                                           int Ho, int Wo, float fill, unsigned& pk0, unsigned& pk1, unsigned& pk2) {
    const int h = sizes ? sizes[2 * k] : Hs, w = sizes ? sizes[2 * k + 1] : Ws;
    const int padlv = (int)fminf(fmaxf(fill, 0.f), 255.f);
    const int* __restrict__ g = table + (size_t)kRecWords * B + (size_t)kGeomWords * k;
    const unsigned char* img = src + (size_t)k * Hs * Ws * 3;
    pk0 = pk1 = pk2 = 0u;
#pragma nounroll
    for (int j = 0; j < 4; ++j) {
        int lv[3];
        geom_level(img, g, fl, h, w, Hs, Ws, Ho, Wo, padlv, y, min(gx * 4 + j, Wo - 1), lv);
        pk0 |= (unsigned)lv[0] << (8 * j); pk1 |= (unsigned)lv[1] << (8 * j); pk2 |= (unsigned)lv[2] << (8 * j);
    }
}

// One 4-pixel group of image k at output row y, groups gx: source bytes -> the value the un-mixed kernel writes there (plain(k) of
// include/nkbhip.h), from k's own sizes, pad, flips (fl bits 0, 1), augmentation record (fl bit 2) and, where fl has bit 4, the
// canvas levels pk0..2 that geom_group made of its geometry record.  Bit 3 of fl is not looked at.
__device__ __forceinline__ void prep_group(const unsigned char* __restrict__ src, const int* __restrict__ sizes,
                                           const int* __restrict__ table, int k, unsigned fl, unsigned pk0, unsigned pk1, unsigned pk2,
                                           int y, int gx, int Hs, int Ws, int Ho, int Wo, float m0, float m1, float m2, float r0,
                                           float r1, float r2, float fill, float (&v)[3][4]) {
    const int h = sizes ? sizes[2 * k] : Hs, w = sizes ? sizes[2 * k + 1] : Ws;
    int q[3][4];
    bool in[4];
    float p[3][4];                                  // the value Normalize sees: a level, or `fill` itself on the plain path
    if (fl & 16u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            in[j] = true;
            q[0][j] = (int)(pk0 >> (8 * j) & 255u); q[1][j] = (int)(pk1 >> (8 * j) & 255u); q[2][j] = (int)(pk2 >> (8 * j) & 255u);
            p[0][j] = (float)q[0][j]; p[1][j] = (float)q[1][j]; p[2][j] = (float)q[2][j];
        }
    } else {
        const int top = (Ho - h) / 2, left = (Wo - w) / 2;
        const int yf = (fl & 2u) ? Ho - 1 - y : y;
        const int sy = yf - top;
        const bool row_in = (unsigned)sy < (unsigned)h;
        const unsigned char* row = src + ((size_t)k * Hs + (row_in ? sy : 0)) * Ws * 3;
        // the 12 source bytes are loaded and turned into the plain path's values in straight-line code, exactly as without records;
        // an image with a record then redoes the arithmetic from the bytes
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

// waves_per_eu(8): the allocator is held to the 64 vector registers of eight waves per SIMD — what the kernel had before the geometry
// path — instead of trading occupancy for that path's comfort (61 VGPRs, no scratch; DESIGN.md 3.19 has the measurements)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void image_prep_kernel(const unsigned char* __restrict__ src, const int* __restrict__ sizes,
                                                         const unsigned char* __restrict__ flags, float* __restrict__ out,
                                                         int B, int Hs, int Ws, int Ho, int Wo, float m0, float m1, float m2,
                                                         float r0, float r1, float r2, float fill, bool vec) {
    const int* __restrict__ table = (const int*)(flags + (((size_t)B + 15) & ~(size_t)15));     // dereferenced only behind bit 2 / 3
    const int xg = (Wo + 3) >> 2;                       // 4-pixel groups per row
    const int per = Ho * xg;                            // groups per image (the host checked that it fits an int)
    // grid.y walks the images, grid.x the groups of one: a block works on ONE image, so its sizes, flag byte, records and mixing
    // partner are uniform and live in scalar registers — that is what leaves the vector registers to the geometry path
    for (int b = blockIdx.y; b < B; b += gridDim.y)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const int gx = i % xg;
        const int y = i / xg;
        const unsigned fl = flags ? flags[b] : 0u;
        // flag bit 3: words 10..15 of record b mix image b with a partner.  take = the pixels of the group that come from the
        // partner (box), 0xF for a blend; an image is evaluated only where one of its pixels is used, so a box costs one evaluation
        // per pixel but in the groups its vertical edges cut.  A partner outside [0, B), the image itself or an unknown mode: no mix.
        // b, and with it the flag byte, the partner and its flag byte, is the same for the whole block: they stay in scalar registers
        int partner = b, md = 0;
        if (fl & 8u) {
            const int* __restrict__ rec = table + (size_t)kRecWords * b;
            const int p = rec[10], m = rec[11];
            if ((unsigned)p < (unsigned)B && p != b && (m == 1 || m == 2)) { partner = p; md = m; }
        }
        int mode = md == 1 ? 1 : 0;
        unsigned take = md == 1 ? 0xFu : 0u;
        if (md == 2) {
            const int* __restrict__ rec = table + (size_t)kRecWords * b;
            const int y1 = rec[12], x1 = rec[13], y2 = rec[14], x2 = rec[15];
            if (y >= y1 && y < y2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = gx * 4 + j;
                    if (x >= x1 && x < x2) take |= 1u << j;
                }
            }
            if (take) mode = 2;
        }
        // flag bit 4: the geometry records are worked off first, while little else is live — image b's, then the partner's; each
        // leaves three registers of levels for prep_group
        const unsigned pfl = md ? flags[partner] : 0u;
        unsigned gb0 = 0u, gb1 = 0u, gb2 = 0u, gp0 = 0u, gp1 = 0u, gp2 = 0u;
        const bool own = mode != 2 || take != 0xFu;
        if (own && (fl & 16u)) geom_group(src, sizes, table, B, b, fl, y, gx, Hs, Ws, Ho, Wo, fill, gb0, gb1, gb2);
        if (mode && (pfl & 16u)) geom_group(src, sizes, table, B, partner, pfl, y, gx, Hs, Ws, Ho, Wo, fill, gp0, gp1, gp2);
        float v[3][4];
        if (own)
            prep_group(src, sizes, table, b, fl, gb0, gb1, gb2, y, gx, Hs, Ws, Ho, Wo, m0, m1, m2, r0, r1, r2, fill, v);
        if (mode) {
            float u[3][4];
            const int* __restrict__ rec = table + (size_t)kRecWords * b;
            const float lam = __int_as_float(rec[12]), oml = __int_as_float(rec[13]);
            prep_group(src, sizes, table, partner, pfl, gp0, gp1, gp2, y, gx, Hs, Ws, Ho, Wo, m0, m1, m2, r0, r1, r2, fill, u);
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
    // with flags the source canvas may be larger than the output (a resampled crop box cuts from more pixels than it writes; any
    // other image then shows its centred window); without flags nothing could ask for that
    if (B < 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || (!flags && (Hs > Ho || Ws > Wo))) {
        nkb_set_error("image_prep: source %dx%d must fit the %dx%d output", Hs, Ws, Ho, Wo);
        return 1;
    }
    if (!mean || !stdev || stdev[0] == 0.f || stdev[1] == 0.f || stdev[2] == 0.f) { nkb_set_error("image_prep: bad mean / std"); return 1; }
    if (B == 0) return 0;
    NkbProfScope prof(NKB_K_MISC, stream, 0, (double)B * Ho * Wo * 15.0);
    // Normalize of the reference stack: img = (img - mean * 255) * (1 / (std * 255)) in float32
    const float m0 = mean[0] * 255.f, m1 = mean[1] * 255.f, m2 = mean[2] * 255.f;
    const float r0 = 1.f / (stdev[0] * 255.f), r1 = 1.f / (stdev[1] * 255.f), r2 = 1.f / (stdev[2] * 255.f);
    const long long per = (long long)Ho * ((Wo + 3) / 4);                  // 4-pixel groups per image
    if (per > 0x7fffffffLL || (long long)Hs * Ws * 3 > 0x7fffffffLL) { nkb_set_error("image_prep: %dx%d -> %dx%d is too large", Hs, Ws, Ho, Wo); return 1; }
    long long g = (per + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)g, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, stream, src, sizes, flags, out, B, Hs, Ws, Ho, Wo,
                       m0, m1, m2, r0, r1, r2, fill, (Wo & 3) == 0 && ((uintptr_t)out & 15) == 0);
    return nkb_check_launch("image_prep");
}
