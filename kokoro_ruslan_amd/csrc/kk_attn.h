// Attention, internal: the device code that more than one kernel family uses (kk_attn_fwd.hip, kk_attn_bwd.hip, kk_attn_fwd3.h and,
// through that body, kk_chain.hip).  Device code only; the host side the units share is declared in kk_attn_host.h.  Overview: kk_attn.hip.
#pragma once
#include "kk_common.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

namespace {

template <bool BF16> struct ACfg;
template <> struct ACfg<true> { typedef __bf16 elem; static constexpr int LR = 72; };    // 144-byte rows
template <> struct ACfg<false> { typedef float elem; static constexpr int LR = 65; };

struct AttnArgs {
    const void *Q, *K, *V, *O, *dO;      // fp32, or bf16 when the kernel is instantiated with ST16 (bf16 storage)
    const float *LSE, *Delta;
    void *Out, *Out2;
    float *LSEo;
    float *DeltaOut;                     // dQ kernel: when set (with O), compute Delta = rowsum(dO * O) here and store it
    const uint8_t *key_mask;
    int B, heads, Sq, Sk, causal;
    int64_t ldq, ldk, ldv, ldo, lddo, ldout, ldout2;
    float scale;
    // dropout on the attention probabilities (SDPA dropout_p, transformers.py:396): mask = f(seed, site, element)
    const uint32_t *seed;
    uint32_t site;
    float p_drop;
    int xcd_map;
    int wt;                              // write-through stores of the [rows, 64] outputs (kk_common.h: kk_write_through(B * S))
    int dbg;                             // timing probes (KK_ATTN_DBG; results are wrong when set)
    int short_first;                     // attn_bwd_pair3: the dK/dV half of a causal launch hands out its SHORT blocks first (see there)
    void *dS;                            // kk_attn_bwd_ws: bf16 dS tiles, written by the dK/dV kernel, read by the dQ pass (kk_attn_bwd_dkv3.inc)
    // Packed keep decisions of the probability dropout (kk_attn_fwd_kb / kk_attn_bwd_kb): one bit per score, written by the
    // third-generation forward as the 16 ballots of every 32 x 32 unit it computes, read by the third-generation backward instead of
    // re-hashing — the hash was ~40 % of the backward's vector instructions.  Unit (qu, ku) of (b, head): 128 bytes at
    // (((b * heads + head) * nQU + qu) * nKU + ku) * 128, nQU = ceil(Sq / 32), nKU = ceil(Sk / 32); dword 2 r + h of a unit = bits over
    // the unit's 32 queries (bit = query) for key frag_row(r, h): the forward's ballot of accumulator register r, half h.
    void *keep;
    // weight warming (kk_attn_warm_next): the third-generation forward touches one dword per 128-byte line of up to two matrices the NEXT
    // launches multiply with — each XCD's workgroups share the lines out — during its last tile step, when its own DMAs are over: the
    // forward is vector-bound and its CUs' request slots are idle, and an XCD's L2 keeps read-only lines across the kernel boundary
    // (profiles/r06_l2_retention_probe.txt), so the GEMM behind it finds its weights L2-hot instead of in HBM
    const void *warm[2];
    uint32_t warm_bytes[2];
    int keep_rd;                         // forward: 1 = READ the keep bits (written by kk_attn_keep_gen beside the encoder forward) instead of hashing + storing them
    // backward kernels: the gradient of the per-head RMSNorm (+ RoPE) that produced Q (dQ kernel) / K and V (dK/dV
    // kernel: hn[0], hn[1]) as the epilogue — Out / Out2 then receive the gradient of the RAW projection
    KkAttnHeadNorm hn[2];
};

// (ProbDrop, the dropout on the probabilities, is in kk_common.h: the persistent encoder launch uses it too)

// Edge sub-tiles without branches: bits 0 .. rel of a 32-bit word (rel < 0: none, rel >= 31: all).  A unit's visibility word is
// kk_low_bits(last visible element - first element of the unit) & ~(masked elements); a score is kept with v_bfe_i32 + v_and.
__device__ __forceinline__ uint32_t kk_low_bits(int rel) { return rel < 0 ? 0u : (rel >= 31 ? 0xFFFFFFFFu : (2u << rel) - 1u); }
// x with its bits ANDed by m (m = 0 or -1: v_bfe_i32 of a visibility / keep word).  Takes the value BY VALUE on purpose:
// __builtin_bit_cast applied directly to an element of an ext_vector (`bit_cast(int, acc[r])`) reads element 0 whatever r is (clang
// 19 / ROCm 7.2, seen in the disassembly: every select used the first accumulator register).
__device__ __forceinline__ float kk_andf(float x, int m) { return __builtin_bit_cast(float, __builtin_bit_cast(int, x) & m); }
__device__ __forceinline__ float kk_bfif(float x, int m, int other) { return __builtin_bit_cast(float, (__builtin_bit_cast(int, x) & m) | (~m & other)); }
typedef unsigned long long kk_u64x8 __attribute__((ext_vector_type(8)));
typedef const kk_u64x8 __attribute__((address_space(4))) kk_cu64x8;      // constant address space: a wave-uniform address gives s_load_dwordx16

// Workgroup -> (128-row block, batch*head).  The dispatcher places workgroup i (x fastest) on XCD i % 8, each with a private
// L2: in launch order the row blocks of one (batch, head) land on up to eight XCDs and every one of those L2s fetches that
// head's K and V (Q and dO in the dK/dV kernel) again.  With xcd_map set, the workgroups of XCD x are the blocks of the
// (batch, head) pairs = x (mod 8): a head's operands are fetched by one L2.  For causal launches the long blocks go first:
// per head (xcd_map = 1), or — xcd_map = 2, the causal pair launch of the backward — the longest blocks of ALL of an XCD's heads,
// then the second longest, ...: the dK/dV half of that launch is handed out as CUs finish their dQ block, and only in this order
// do the CUs that held the shortest dQ blocks receive the longest dK/dV blocks (5 block-units per CU instead of 7).
template <typename A> __device__ __forceinline__ void attn_block(A &a, int &bx, int &by, bool long_first_is_high) {
    bx = blockIdx.x; by = blockIdx.y;
    const int nx = gridDim.x, ny = gridDim.y;
    if (a.xcd_map && (ny & 7) == 0) {
        const int L = bx + nx * by, slot = L >> 3;
        if (a.xcd_map == 2) {                                  // block-major inside an XCD: ALL its longest blocks first (pair launch)
            const int per = ny >> 3;
            by = (L & 7) + 8 * (slot % per);
            bx = slot / per;
        } else {
            by = (L & 7) + 8 * (slot / nx);
            bx = slot % nx;
        }
    }
    if (a.causal && a.xcd_map) bx = long_first_is_high ? nx - 1 - bx : bx;
}

__device__ __forceinline__ float f4g(const float4 &v, int c) { return reinterpret_cast<const float *>(&v)[c]; }

// One row (this lane's row, lane&31) of a [32][64] fp32 matrix, held as an MFMA operand with k = d.
template <bool BF16> struct RowFrag;
template <> struct RowFrag<true> { bf16x8 v[4]; };    // v[ks][j] = X[row][16 ks + 8 half + j]
template <> struct RowFrag<false> { float v[32]; };   // v[ks]    = X[row][2 ks + half]

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <bool BF16>
__device__ __forceinline__ float rowfrag_dot(const RowFrag<BF16> &x, const RowFrag<BF16> &y) {   // this lane's 32 of the 64 d
    float s = 0.f;
    if constexpr (BF16) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (float)x.v[ks][j] * (float)y.v[ks][j];
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) s += x.v[j] * y.v[j];
    }
    return s;
}

template <bool BF16>
__device__ __forceinline__ void scale_rowfrag(RowFrag<BF16> &f, float k) {
    if constexpr (BF16) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) f.v[ks][j] = (__bf16)((float)f.v[ks][j] * k);
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) f.v[j] *= k;
    }
}

template <bool BF16, typename T>
__device__ __forceinline__ void load_rowfrag(RowFrag<BF16> &f, const T *rowptr, int half) {
    if constexpr (BF16 && sizeof(T) == 2) {            // bf16 storage: the fragment is a plain 16-byte load
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (rowptr) v = *reinterpret_cast<const u32x4 *>(rowptr + ks * 16 + half * 8);
            f.v[ks] = __builtin_bit_cast(bf16x8, v);
        }
    } else if constexpr (BF16) {
        const float *rp = reinterpret_cast<const float *>(rowptr);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (rp) { a = ld4(rp + ks * 16 + half * 8); b = ld4(rp + ks * 16 + half * 8 + 4); }
#pragma unroll
            for (int e = 0; e < 4; ++e) { f.v[ks][e] = (__bf16)f4g(a, e); f.v[ks][4 + e] = (__bf16)f4g(b, e); }
        }
    } else {
        const float *rp = reinterpret_cast<const float *>(rowptr);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rp) a = ld4(rp + 4 * j);
            f.v[2 * j] = half ? a.y : a.x;
            f.v[2 * j + 1] = half ? a.w : a.z;
        }
    }
}

// Staging of a [64][64] fp32 tile (row r at src + r*ld; rows >= nvalid read as zero) is split in two halves so the
// global loads of tile t+1 can be in flight while tile t is being multiplied: load_* fills 4 float4 registers,
// store_* converts and writes them to LDS.  "rows": LDS row-major S[64][LR];  "rows_T" (bf16 only): transposed
// St[d][row] (row contiguous), needed where the MFMA reduction runs over the tile's rows.
struct TileRegs { float4 r[4]; };

__device__ __forceinline__ void load_rows(TileRegs &t, const float *src, int64_t ld, int nvalid) {
    const int tl = threadIdx.x & 255, row = tl >> 2, seg = (tl & 3) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) t.r[i] = row < nvalid ? ld4(src + (int64_t)row * ld + seg + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <bool BF16>
__device__ __forceinline__ void store_rows(typename ACfg<BF16>::elem *S, const TileRegs &t) {
    constexpr int LR = ACfg<BF16>::LR;
    const int tl = threadIdx.x & 255, row = tl >> 2, seg = (tl & 3) * 16;
    if constexpr (BF16) {
        bf16x8 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = (__bf16)f4g(t.r[0], e); lo[4 + e] = (__bf16)f4g(t.r[1], e);
            hi[e] = (__bf16)f4g(t.r[2], e); hi[4 + e] = (__bf16)f4g(t.r[3], e);
        }
        *reinterpret_cast<bf16x8 *>(&S[row * LR + seg]) = lo;
        *reinterpret_cast<bf16x8 *>(&S[row * LR + seg + 8]) = hi;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) S[row * LR + seg + 4 * i + e] = f4g(t.r[i], e);
    }
}

__device__ __forceinline__ void load_rows_T(TileRegs &t, const float *src, int64_t ld, int nvalid) {
    const int tl = threadIdx.x & 255, rg = (tl & 15) * 4, dg = (tl >> 4) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) t.r[c] = (rg + c) < nvalid ? ld4(src + (int64_t)(rg + c) * ld + dg) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void store_rows_T(__bf16 *St, const TileRegs &t) {
    constexpr int LR = ACfg<true>::LR;
    const int tl = threadIdx.x & 255, rg = (tl & 15) * 4, dg = (tl >> 4) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bf16x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (__bf16)f4g(t.r[c], e);
        *reinterpret_cast<bf16x4 *>(&St[(dg + e) * LR + rg]) = v;
    }
}

// The same two staging patterns for tiles that are ALREADY bf16 in HBM (bf16 storage): no conversion, half the bytes.
struct TileRegs16 { u32x4 r[2]; };     // "rows" pattern: 16 contiguous bf16 of one row
struct TileRegs16T { u32x2 r[4]; };    // "rows_T" pattern: 4 rows x 4 contiguous bf16

__device__ __forceinline__ void load_rows(TileRegs16 &t, const __bf16 *src, int64_t ld, int nvalid) {
    const int tl = threadIdx.x & 255, row = tl >> 2, seg = (tl & 3) * 16;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 2; ++i) t.r[i] = row < nvalid ? *reinterpret_cast<const u32x4 *>(src + (int64_t)row * ld + seg + 8 * i) : z;
}
__device__ __forceinline__ void store_rows16(__bf16 *S, const TileRegs16 &t) {
    constexpr int LR = ACfg<true>::LR;
    const int tl = threadIdx.x & 255, row = tl >> 2, seg = (tl & 3) * 16;
    *reinterpret_cast<u32x4 *>(&S[row * LR + seg]) = t.r[0];
    *reinterpret_cast<u32x4 *>(&S[row * LR + seg + 8]) = t.r[1];
}
__device__ __forceinline__ void load_rows_T(TileRegs16T &t, const __bf16 *src, int64_t ld, int nvalid) {
    const int tl = threadIdx.x & 255, rg = (tl & 15) * 4, dg = (tl >> 4) * 4;
    const u32x2 z = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 4; ++c) t.r[c] = (rg + c) < nvalid ? *reinterpret_cast<const u32x2 *>(src + (int64_t)(rg + c) * ld + dg) : z;
}
__device__ __forceinline__ void store_rows_T16(__bf16 *St, const TileRegs16T &t) {
    constexpr int LR = ACfg<true>::LR;
    const int tl = threadIdx.x & 255, rg = (tl & 15) * 4, dg = (tl >> 4) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {        // element e of rows 0..3 -> 4 contiguous bf16 of transposed row dg+e
        const int w = e >> 1, sh = 16 * (e & 1);
        u32x2 v;
        v[0] = ((t.r[0][w] >> sh) & 0xFFFFu) | (((t.r[1][w] >> sh) & 0xFFFFu) << 16);
        v[1] = ((t.r[2][w] >> sh) & 0xFFFFu) | (((t.r[3][w] >> sh) & 0xFFFFu) << 16);
        *reinterpret_cast<u32x2 *>(&St[(dg + e) * LR + rg]) = v;
    }
}

// Uniform front end: Stage<BF16, ST16> picks the register type and the load/store pair for a tile.
template <bool BF16, bool ST16> struct Stage {
    typedef TileRegs R;
    typedef TileRegs RT;
    typedef float T;
    static __device__ __forceinline__ void st(typename ACfg<BF16>::elem *S, const R &r) { store_rows<BF16>(S, r); }
    static __device__ __forceinline__ void stT(__bf16 *S, const RT &r) { store_rows_T(S, r); }
};
template <> struct Stage<true, true> {
    typedef TileRegs16 R;
    typedef TileRegs16T RT;
    typedef __bf16 T;
    static __device__ __forceinline__ void st(__bf16 *S, const R &r) { store_rows16(S, r); }
    static __device__ __forceinline__ void stT(__bf16 *S, const RT &r) { store_rows_T16(S, r); }
};

// acc[row][col] += sum_d T[r0 + row][d] * F_col[d]: A operand = 32 rows of the LDS tile, B operand = RowFrag.
template <bool BF16>
__device__ __forceinline__ void mma_tile_x_frag(f32x16 &acc, const typename ACfg<BF16>::elem *T, int r0,
                                                const RowFrag<BF16> &f, int l31, int half) {
    constexpr int LR = ACfg<BF16>::LR;
    if constexpr (BF16) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&T[(r0 + l31) * LR + ks * 16 + half * 8]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, f.v[ks], acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < 32; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(T[(r0 + l31) * LR + 2 * ks + half], f.v[ks], acc, 0, 0, 0);
    }
}

// out[db][d_local][col] += sum_{rows of sub-tile} X[row][db*32 + d_local] * p[row][col], where p[16] are this
// lane's accumulator-layout values (row_local = frag_row(r, half), col = lane&31).  bf16: Tx is the TRANSPOSED
// tile [d][row]; fp32: Tx is the row-major tile [row][d].
template <bool BF16>
__device__ __forceinline__ void mma_T_x_p(f32x16 (&out)[2], const typename ACfg<BF16>::elem *Tx, int sub0,
                                          const float (&p)[16], int l31, int half) {
    constexpr int LR = ACfg<BF16>::LR;
    if constexpr (BF16) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 b;
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = (__bf16)p[8 * s2 + j];
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const __bf16 *base = &Tx[(db * 32 + l31) * LR + sub0 + 16 * s2 + 4 * half];
                const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(base);
                const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(base + 8);
                bf16x8 a;
#pragma unroll
                for (int e = 0; e < 4; ++e) { a[e] = lo[e]; a[4 + e] = hi[e]; }
                out[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, out[db], 0, 0, 0);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = sub0 + frag_row(r, half);
#pragma unroll
            for (int db = 0; db < 2; ++db)
                out[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(Tx[row * LR + db * 32 + l31], p[r], out[db], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ void zero_acc(f32x16 &a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// Store a transposed accumulator pair acc[db][r] (row = d, col = this lane's matrix row) to dst_row[0..63].
template <typename T>
__device__ __forceinline__ void store_row(T *dst_row, const f32x16 (&acc)[2], float mul, int half) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            stv4<T>(dst_row + db * 32 + 8 * g + 4 * half,
                make_float4(acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul, acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul));
}

// Epilogue of the backward kernels: gradient of y = RMSNorm64(x)*gain (+ RoPE) for the (row, head) vector this lane
// pair holds (same math as headnorm_rope_bwd_kernel, kk_norm.hip; acc*mul is first rounded to the storage type, as
// the unfused path's store does).  A lane has d = db*32 + 8g + 4*half + e, so rotate_half's partner d^32 is its own
// acc[db^1] element and the two row reductions are a local sum plus one xor-32 shuffle.  The gain gradient needs
// column sums over the workgroup's 128 rows: every lane drops dn*x*rstd into colred[row][65] and hn_colsum() adds
// the columns after a barrier.  Returns nothing; `valid` lanes store dx.
template <typename T>
__device__ __forceinline__ void hn_bwd_row(const f32x16 (&acc)[2], float mul, bool valid, const T *raw_row, T *out_row,
                                           const KkAttnHeadNorm &h, int pos, int half, float *colred_row) {
    float dn[32], v[32];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 x4 = valid ? ldv4<T>(raw_row + db * 32 + 8 * g + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[db * 16 + 4 * g] = x4.x; v[db * 16 + 4 * g + 1] = x4.y; v[db * 16 + 4 * g + 2] = x4.z; v[db * 16 + 4 * g + 3] = x4.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) dn[db * 16 + 4 * g + e] = valid ? (float)(T)(acc[db][4 * g + e] * mul) : 0.f;
        }
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) ssq += v[i] * v[i];
    ssq += __shfl_xor(ssq, 32, 64);
    const float rs = 1.f / sqrtf(ssq * (1.f / 64.f) + 1.1920928955078125e-7f);
    if (h.rope) {     // dn[d] = dy[d] cos[d] + (d < 32 ? dy[d+32] sin[d+32] : -dy[d-32] sin[d-32])
        const int64_t pr = valid ? pos : 0;                      // (rows past the end of the sequence have no table row)
        const float *cr = h.cos_t + pr * 64, *sr = h.sin_t + pr * 64;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 8 * g + 4 * half;
            const float4 c0 = ld4(cr + d), c1 = ld4(cr + 32 + d), s0 = ld4(sr + d), s1 = ld4(sr + 32 + d);
            const float cl[4] = {c0.x, c0.y, c0.z, c0.w}, ch[4] = {c1.x, c1.y, c1.z, c1.w};
            const float sl[4] = {s0.x, s0.y, s0.z, s0.w}, sh[4] = {s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = dn[4 * g + e], hi = dn[16 + 4 * g + e];
                dn[4 * g + e] = lo * cl[e] + hi * sh[e];
                dn[16 + 4 * g + e] = hi * ch[e] - lo * sl[e];
            }
        }
    }
    float kdot = 0.f;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 g4 = ld4(h.gain + db * 32 + 8 * g + 4 * half);
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = db * 16 + 4 * g + e;
                colred_row[db * 32 + 8 * g + 4 * half + e] = dn[i] * v[i] * rs;
                dn[i] *= gg[e];                                  // dg
                kdot += dn[i] * v[i];
            }
        }
    kdot += __shfl_xor(kdot, 32, 64);
    const float k = kdot * (1.f / 64.f) * rs * rs * rs;
    if (valid) {
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = db * 16 + 4 * g;
                stv4<T>(out_row + db * 32 + 8 * g + 4 * half,
                        make_float4(rs * dn[i] - v[i] * k, rs * dn[i + 1] - v[i + 1] * k, rs * dn[i + 2] - v[i + 2] * k, rs * dn[i + 3] - v[i + 3] * k));
            }
    }
}
// column sums of colred[128][65] -> partials[workgroup][64] (threads 0..63 of the workgroup; call between barriers)
__device__ __forceinline__ void hn_colsum(const float *colred, float *partials) {
    if (threadIdx.x < 64) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
        for (int r = 0; r < 128; r += 2) { s0 += colred[r * 65 + threadIdx.x]; s1 += colred[(r + 1) * 65 + threadIdx.x]; }
        partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 64 + threadIdx.x] = s0 + s1;
    }
}

// ------------------------------------------------------------------ helpers of the DMA-staged kernels (second generation and later)
typedef float f32x4_ __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define KK_LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))

__device__ __forceinline__ bf16x8 tr_pair(const s16x4 &lo, const s16x4 &hi) {
    s16x8 v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_bit_cast(bf16x8, v);
}

// value of the lane 32 away combined with the own one, by v_permlane32_swap (a VALU instruction; __shfl_xor(.., 32) is a
// ds_bpermute round trip through the LDS queue): the swap of v with itself returns {own, partner} in some order
// (inline asm: with this compiler __builtin_amdgcn_permlane32_swap hands back its FIRST result for both elements of the
// returned pair — `v_add_f32 v, v9, v9` after the swap; the s_nops cover the VALU-write -> swap -> VALU-read wait states)
__device__ __forceinline__ void xor32_pair(float v, float &lo, float &hi) {
    lo = v; hi = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi));
}
__device__ __forceinline__ float xor32_sum(float v) {
    float a, b;
    xor32_pair(v, a, b);
    return a + b;
}
__device__ __forceinline__ float xor32_max(float v) {
    float a, b;
    xor32_pair(v, a, b);
    return fmaxf(a, b);
}

// ---- coalesced prologue / epilogue pieces of the second-generation kernels.  A row-per-lane access (one 128-byte head row
// per lane: the RowFrag loads, store_row) touches 32 lines per wave instruction and is bound by requests, not bytes
// (4 us of a 13 us forward launch were the Q loads and the O stores).
// DMA of a [128 rows][64] bf16 head tile into a 16 KB LDS image with XOR-ed 16-byte chunks, by 512 threads (two pieces each).
template <int NT = 512>                 // threads of the workgroup (512: two pieces each, 256: four)
__device__ __forceinline__ void dma_rows128(const __bf16 *base, int64_t ld, int nrows, char *img, int wave8) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(base), 0, nrows > 0 ? (int)((((int64_t)nrows - 1) * ld + 64) * 2) : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < 1024 / NT; ++j) {
        const int p = threadIdx.x + NT * j, row = p >> 3, pc = p & 7;
        const uint32_t vo = (uint32_t)(((int64_t)row * ld + ((pc ^ ((row >> 1) & 7)) * 8)) * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, KK_LDS_PTR(img + wave8 * 1024 + j * (NT * 16)), 16, vo, 0, 0, 0);
    }
}
// this lane's row (row0 + lane&31, row0 a multiple of 16) of such an image as an MFMA operand with k = d (RowFrag layout)
__device__ __forceinline__ void rowfrag_from_image(RowFrag<true> &f, const char *img, int row0, int l31, int half) {
    const uint32_t base = (uint32_t)(uintptr_t)KK_LDS_PTR(img) + (uint32_t)((row0 + l31) * 128);
    const int swz = (l31 >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("ds_read_b128 %0, %1" : "=v"(f.v[ks]) : "v"(base + (uint32_t)(((2 * ks + half) ^ swz) * 16)));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(f.v[ks]));
}
// Store the wave's transposed accumulator pair (acc[db][r]: d = db*32 + 8(r>>2) + 4 half + (r&3), row = lane&31) times mul
// as 32 bf16 rows of 64 through a wave-private 4608-byte LDS tile: 16-byte global stores, eight lanes per 128-byte row.
__device__ __forceinline__ void store_rows_via_lds(__bf16 *dst_row0, int64_t ld, int nvalid, const f32x16 (&acc)[2], float mul,
                                                   char *tile, int lane, int wt) {
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (__bf16)(acc[db][4 * g + e] * mul);
            *reinterpret_cast<bf16x4 *>(tile + l31 * 144 + (db * 32 + 8 * g + 4 * half) * 2) = v;
        }
    __builtin_amdgcn_wave_barrier();                       // (one wave: its LDS operations complete in order)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (lane >> 3) + 8 * j, c = lane & 7;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(tile + row * 144 + c * 16);
        if (row < nvalid) kk_store16(dst_row0 + (int64_t)row * ld + c * 8, v, wt);
    }
}

#ifdef KK_TUNING_HOOKS
// Probe bit 4096 (tools): every workgroup of a launch leaves (first wave's entry, last wave's exit) in 10 ns ticks of the constant clock
// and its hardware id at stamp-buffer word 512 + 4 * linear workgroup index — the launch's dispatch ramp, the spread of workgroup
// durations and its tail, next to the rocprofv3 duration (tools/probes/attn_grid_timeline.py).
struct KkWgStamp {
    const AttnArgs &a;
    __device__ unsigned long long *slot() const {
        return reinterpret_cast<unsigned long long *>(a.DeltaOut) + 512 + 4 * (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
    }
    __device__ bool on() const { return KK_DBG(a, 4096) && a.DeltaOut != nullptr && (threadIdx.x & 63) == 0; }
    __device__ explicit KkWgStamp(const AttnArgs &a_) : a(a_) {
        if (on()) {
            atomicMin(slot(), (unsigned long long)__builtin_amdgcn_s_memrealtime());
            if (threadIdx.x == 0) slot()[2] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32 | __builtin_amdgcn_s_getreg((31 << 11) | 4);   // XCC_ID | HW_ID
        }
    }
    __device__ ~KkWgStamp() {
        if (on()) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            atomicMax(slot() + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
        }
    }
};
#define KK_WG_STAMP(args) KkWgStamp wg_stamp_(args)
#else
#define KK_WG_STAMP(args)
#endif

}  // namespace
