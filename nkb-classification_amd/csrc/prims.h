// Device primitives shared by the pipelined kernels (gfx950 / CDNA4 only): the LDS DMA, the raw barrier, the counted waits, the
// inline-assembly LDS reads, the DPP row sum and the LDS swizzles.  ONE definition each: a new pipelined kernel takes them from here
// instead of copying them (a slip in any of them is a silent race or a hang).  Everything is a macro or __forceinline__: no symbols.
#pragma once
#include "common.h"

// ---- global -> LDS DMA: 16 bytes per lane, the destination is wave-linear (dst of lane 0 + 16 * lane), so any swizzle goes on src ----
__device__ __forceinline__ void glds16(const unsigned char* src, unsigned char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// ---- raw s_barrier (no vmcnt drain, unlike __syncthreads) between two compiler-level memory barriers ----
#define NKB_BARRIER()                                \
    do {                                             \
        asm volatile("" ::: "memory");               \
        __builtin_amdgcn_s_barrier();                \
        asm volatile("" ::: "memory");               \
    } while (0)

// ---- counted waits: "all but the N youngest vector-memory operations have completed".  Two forms, kept apart because they emit
// different text: the template takes any constant expression, the macros paste a literal into the instruction ----
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
#define NKB_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define NKB_LGKM(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")

// ---- LDS fragment reads as inline assembly: a compiler-visible LDS read (the builtin or a plain load) behind an LDS DMA makes hipcc
// wait for vmcnt(0) first — the stages just requested.  The asm forms are ordered by the counted lgkmcnt waits of their callers ----
#define LDS_READ_TR16(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define LDS_READ128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
// all but the n youngest LDS reads have landed; ties the wait to the two registers f[0], f[1] of a transposed fragment
#define LDS_WAIT_PAIR(n, f) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f[0]), "+v"(f[1]) : "n"(n))
// the same tied to the four registers q[0..1][0..1] of a pair of ds_read_b128 fragments (n is pasted into the instruction: a literal)
#define LDS_WAIT_QUAD(n, q) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(q[0][0]), "+v"(q[0][1]), "+v"(q[1][0]), "+v"(q[1][1]))

// ---- sum over the 16 lanes of a DPP row (quad_perm xor 1, xor 2, row_half_mirror, row_mirror): every lane ends up with the total ----
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));
    return v;
}

// ---- LDS swizzles: byte offset of 16-byte chunk `ch` of row `row` ----
// 128-byte rows (ds_read_b128 fragments): chunk ^ (row & 7)
__device__ __forceinline__ int swz128(int row, int ch) { return row * 128 + ((ch ^ (row & 7)) << 4); }
// 256-byte rows (ds_read_b64_tr_b16 fragments of pixel-major operands): chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))
__device__ __forceinline__ int swz256(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
// 32-byte-block swizzle of pixel row px, for ds_read_b64_tr_b16 over DMA'd rows (XOR the block index of the source address with it):
// rows whose stride is a multiple of 256 bytes all start on bank 0, so the eight rows a 32-lane half reads (pixels 0-3 and 8-11 of a
// k-step, or 4-7 and 12-15) need eight different block positions: 3 bits from pixel bits 0, 1, 3.
// 128-byte rows alternate between the two halves of the bank row by themselves: 2 bits from pixel bits 1, 3.
__device__ __forceinline__ int swz_px8(int px) { return (px & 3) | (((px >> 3) & 1) << 2); }
__device__ __forceinline__ int swz_px4(int px) { return ((px >> 1) & 1) | (((px >> 3) & 1) << 1); }
// linear-address form for windows whose pixel stride is 48 .. 256 bytes (csrc/stem3.hip): 16-byte chunk index ^ address bits 8-10.  The
// sixteen pixels a quarter wave reads at one k-offset (stride 64 / 128 bytes) land on sixteen different 16-byte bank groups.
__device__ __forceinline__ int swz_lin(int byte_off) { return byte_off ^ (((byte_off >> 8) & 7) << 4); }
