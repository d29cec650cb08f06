// Device code shared by the two bodies of the bf16-storage GEMM core (kk_gemm16_body.h: gemm16_body; kk_gemm16x_body.h:
// g16x_body): the operand tile with its DMA issue, the fragment reads, the tile order, the counted DMA wait and the Delta dot
// product.  The LDS images are described at the top of kk_gemm16.hip.  The operand tile and the fragment addresses exist in two
// forms, Operand / FragAddr (general: the large-tile family) and Operand1 / FragAddr1 (one 32x32 accumulator per wave): they
// compute the same values, but the compiler emits other code for gemm16_body from the general form, and the remaining epilogue
// rows (GLU gate, write-through fp32 store, sum-of-squares record) change the kernels when moved into functions, so they stay
// written out in each body (docs/LAB_NOTES.md, "One device core for the bf16 GEMM families").
#pragma once
#include "kk_gemm16.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))

// One operand tile of ROWS x 64, issued by NT threads: DMA issue + the per-thread source offsets.  Rows [0, SPLIT) map to global
// rows r0.., rows [SPLIT, ROWS) to r1.. (the large-tile GLU forward's two panels of W1; SPLIT == ROWS otherwise).
template <int ROWS, bool KS, int NT, int SPLIT = ROWS, int AUX = 0> struct Operand {      // AUX: cache policy of the DMA loads (kk_gemm16.h: KK_A_AUX)
    static constexpr int BYTES = ROWS * BK * 2;
    static constexpr int NP = ROWS * 8 / NT;                    // 16-byte pieces per thread per tile
    static_assert(ROWS * 8 % NT == 0 && SPLIT % 8 == 0, "whole pieces per thread");
    static constexpr int PITCH = KS ? ROWS * 2 : BK * 2;        // bytes per LDS row
    static constexpr bool S4 = (PITCH % 256) == 0;              // k-strided image: four k-rows alias mod 256 bytes (else two)
    uint32_t voff[NP];                                          // per-thread byte offset of each piece (tile 0)
    uint32_t kstep;                                             // bytes to advance per k-tile
    __amdgpu_buffer_rsrc_t rsrc;

    __device__ __forceinline__ void init(const void *base, uint32_t bytes, int64_t ld, int r0, int r1, int t) {      // t: index among the NT issuing threads
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int p = t + NT * j;
            if constexpr (!KS) {
                const int row = p >> 3, c = (p & 7) ^ ((row >> 1) & 7);
                const int grow = row < SPLIT ? r0 + row : r1 + row - SPLIT;
                voff[j] = (uint32_t)(((int64_t)grow * ld + c * 8) * 2);
            } else {
                constexpr int PPR = ROWS / 8;                   // pieces per k-row
                const int k = p / PPR, q = p % PPR;
                const int s = S4 ? 2 * (k & 3) : 2 * ((k >> 1) & 1);
                const int col = ((((q >> 1) ^ s) << 1) | (q & 1)) * 8;
                const int gcol = col < SPLIT ? r0 + col : r1 + col - SPLIT;
                voff[j] = (uint32_t)(((int64_t)k * ld + gcol) * 2);
            }
        }
        kstep = KS ? (uint32_t)(ld * BK * 2) : (uint32_t)(BK * 2);
    }
    // start the DMA of k-tile `kt` (absolute tile index) into the LDS image at `dst`
    __device__ __forceinline__ void issue(char *dst, int kt, int wave) const {
        const uint32_t so = (uint32_t)kt * kstep;
#pragma unroll
        for (int j = 0; j < NP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, LDS_PTR(dst + (wave * 64 + NT * j) * 16), 16, voff[j], so, 0, AUX);
    }
};

struct Frag {
    bf16x8 v;            // k-contiguous operand
    s16x4 lo, hi;        // k-strided operand: k 0..3 and 4..7 of this lane's eight
};

// Fragment reads of NF 32-row blocks of an operand image; blk[f] = index of block f inside the image (wave-uniform).
template <int ROWS, bool KS, int NF> struct FragAddr {
    static constexpr int PITCH = KS ? ROWS * 2 : BK * 2;
    static constexpr bool S4 = (PITCH % 256) == 0;
    static constexpr int READS = KS ? 2 : 1;                    // LDS instructions per fragment
    uint32_t base;                                              // byte offset inside the image
    uint32_t x[KS ? NF : 4];                                    // KC: chunk offsets per ks;  KS: block offsets per 32-row block
    uint32_t boff[KS ? 1 : NF];
    __device__ __forceinline__ void init(int lane, const int (&blk)[NF]) {
        const int l31 = lane & 31, half = lane >> 5;
        if constexpr (!KS) {
            const int swz = (l31 >> 1) & 7;
            base = (uint32_t)(l31 * (BK * 2));
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) x[ks] = (uint32_t)(((2 * ks + half) ^ swz) * 16);
#pragma unroll
            for (int f = 0; f < NF; ++f) boff[f] = (uint32_t)(blk[f] * 32 * (BK * 2));
        } else {
            const int L = lane & 15, gi = (lane >> 4) & 1, kq = L >> 2;
            const int s = S4 ? 2 * (kq & 3) : 2 * ((kq >> 1) & 1);
            base = (uint32_t)((8 * half + kq) * PITCH + 8 * (L & 3));
#pragma unroll
            for (int f = 0; f < NF; ++f) x[f] = (uint32_t)(((2 * blk[f] + gi) ^ s) * 32);
        }
    }
    // Fragment of block f, k-slab ks (16 k): one ds_read_b128 (k-contiguous) or two transpose reads (k-strided).  All of them are
    // inline asm: the k-loop keeps the reads of the NEXT slabs in flight under the MFMAs of this one and retires them with counted
    // lgkmcnt waits, which only works when every LDS read of the loop is in program order under our control.  (Through the
    // builtin, hipcc also puts an s_waitcnt vmcnt(0) in front of every transpose read while a DMA is in flight.)
    __device__ __forceinline__ void load(Frag &fr, const char *img, int f, int ks) const {
        if constexpr (!KS) {
            const uint32_t addr = (uint32_t)(uintptr_t)LDS_PTR(img) + base + x[ks] + boff[f];
            asm volatile("ds_read_b128 %0, %1" : "=v"(fr.v) : "v"(addr));
        } else {
            const uint32_t addr = (uint32_t)(uintptr_t)LDS_PTR(img) + base + x[f] + ks * 16 * PITCH;
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fr.lo) : "v"(addr));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(fr.hi) : "v"(addr), "n"(4 * PITCH));
        }
    }
};

// Operand with SPLIT == ROWS issued by all NT threads of the workgroup, in the address arithmetic gemm16_body is compiled from.
template <int ROWS, bool KS, int NT = 256, int AUX = 0> struct Operand1 {      // AUX: cache policy of the DMA loads (kk_gemm16.h: KK_A_AUX)
    static constexpr int BYTES = ROWS * BK * 2;
    static constexpr int NP = ROWS * 8 / NT;                   // 16-byte pieces per thread per tile (NT threads)
    static constexpr int PITCH = KS ? ROWS * 2 : BK * 2;        // bytes per LDS row
    uint32_t voff[NP];                                          // per-thread byte offset of each piece (tile 0)
    uint32_t kstep;                                             // bytes to advance per k-tile
    __amdgpu_buffer_rsrc_t rsrc;

    __device__ __forceinline__ void init(const void *base, uint32_t bytes, int64_t ld, int r0) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int p = t + NT * j;
            if constexpr (!KS) {
                const int row = p >> 3, c = (p & 7) ^ ((row >> 1) & 7);
                voff[j] = (uint32_t)(((int64_t)(r0 + row) * ld + c * 8) * 2);
            } else {
                constexpr int PPR = ROWS / 8;                   // pieces per k-row
                const int k = p / PPR, q = p % PPR;
                const int s = ROWS == 128 ? 2 * (k & 3) : 2 * ((k >> 1) & 1);
                const int g = (((q >> 1) ^ s) << 1) | (q & 1);
                voff[j] = (uint32_t)(((int64_t)k * ld + r0 + g * 8) * 2);
            }
        }
        kstep = KS ? (uint32_t)(ld * BK * 2) : (uint32_t)(BK * 2);
    }
    // start the DMA of k-tile `kt` (absolute tile index) into the LDS image at `dst`
    __device__ __forceinline__ void issue(char *dst, int kt, int wave) const {
        const uint32_t so = (uint32_t)kt * kstep;
#pragma unroll
        for (int j = 0; j < NP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, LDS_PTR(dst + (wave * 64 + NT * j) * 16), 16, voff[j], so, 0, AUX);
    }
};

// FragAddr for the consecutive blocks from wave_row0 on (blk[f] = wave_row0 / 32 + f), block offsets folded into the instruction.
template <int ROWS, bool KS> struct FragAddr1 {
    uint32_t base;          // byte offset inside the image
    uint32_t x[4];          // KC: chunk offsets per ks;  KS: block offsets per 32-row block (ROWS/64 used... up to 4)
    __device__ __forceinline__ void init(int lane, int wave_row0) {
        const int l31 = lane & 31, half = lane >> 5;
        if constexpr (!KS) {
            const int swz = (l31 >> 1) & 7;
            base = (uint32_t)((wave_row0 + l31) * (BK * 2));
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) x[ks] = (uint32_t)(((2 * ks + half) ^ swz) * 16);
        } else {
            const int L = lane & 15, gi = (lane >> 4) & 1, kq = L >> 2;
            const int s = ROWS == 128 ? 2 * (kq & 3) : 2 * ((kq >> 1) & 1);
            base = (uint32_t)((8 * half + kq) * (ROWS * 2) + 8 * (L & 3));
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) x[rb] = (uint32_t)((((wave_row0 >> 4) + 2 * rb + gi) ^ s) * 32);
        }
    }
    // fragment of 32-row block rb (relative to the wave's first row), k-slab ks (see FragAddr::load)
    static constexpr int READS = KS ? 2 : 1;                    // LDS instructions per fragment
    __device__ __forceinline__ void load(Frag &f, const char *img, int rb, int ks) const {
        if constexpr (!KS) {
            const uint32_t addr = (uint32_t)(uintptr_t)LDS_PTR(img) + base + x[ks] + rb * 32 * (BK * 2);
            asm volatile("ds_read_b128 %0, %1" : "=v"(f.v) : "v"(addr));
        } else {
            const uint32_t addr = (uint32_t)(uintptr_t)LDS_PTR(img) + base + x[rb] + ks * 16 * (ROWS * 2);
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.lo) : "v"(addr));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.hi) : "v"(addr), "n"(4 * ROWS * 2));
        }
    }
};

__device__ __forceinline__ bf16x8 frag_value(const Frag &f, bool ks) {
    if (!ks) return f.v;
    s16x8 v;
    v[0] = f.lo[0]; v[1] = f.lo[1]; v[2] = f.lo[2]; v[3] = f.lo[3]; v[4] = f.hi[0]; v[5] = f.hi[1]; v[6] = f.hi[2]; v[7] = f.hi[3];
    return __builtin_bit_cast(bf16x8, v);
}
// Wait until at most PENDING younger LDS reads are outstanding (they return in order), then pin the slab's fragments
// behind the wait: the empty asm makes their registers data-dependent on this point, so no MFMA is scheduled above it.
template <int PENDING> __device__ __forceinline__ void wait_reads() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(PENDING) : "memory"); }
__device__ __forceinline__ void pin_frag(Frag &f, bool ks) {
    if (ks) asm volatile("" : "+v"(f.lo), "+v"(f.hi));
    else asm volatile("" : "+v"(f.v));
}

// Workgroup -> tile for the XCD-aware order: the dispatcher places workgroup i on XCD i % 8, and XCD x sweeps the x-th contiguous
// run of the n tiles (bijective for any tile count, see kk_gemm.hip).
__device__ __forceinline__ int g16_xcd_tile(int i, int n) {
    const int q = n >> 3, r = n & 7, xcd = i & 7, in = i >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + in;
}

// This wave's pieces of a k-tile have landed once at most the `younger` tiles' DMAs (NPT instructions per thread each) are
// outstanding: a COUNTED vmcnt, so the younger tiles stay in flight across the barrier.
template <int NS, int NPT> __device__ __forceinline__ void g16_wait_tile(int younger) {
    if (NS >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPT) : "memory");
    else if (NS >= 3 && younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Delta epilogue: dsum + sum over the 8 columns of dO * O, from the ROUNDED dO (what the attention kernels will read)
__device__ __forceinline__ float g16_delta_dot(float dsum, const bf16x8 &o, const __bf16 *op) {
    const bf16x8 ov = *reinterpret_cast<const bf16x8 *>(op);
#pragma unroll
    for (int e = 0; e < 8; ++e) dsum += (float)o[e] * (float)ov[e];
    return dsum;
}

}  // namespace
