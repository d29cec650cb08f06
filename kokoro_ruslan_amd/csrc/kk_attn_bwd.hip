// Attention backward (overview, eligibility table and shared host side: kk_attn.hip): the first-generation dQ and dK/dV templates, the
// DMA-staged kernels built from kk_attn_bwd_dq2.inc / _dq3.inc / _dkv3.inc, the pair launch, the two passes, Delta, and the entry
// points that launch them.
#include "kk_attn_host.h"

using namespace kk_attn;

namespace {

// ------------------------------------------------------------------ backward: dQ
// Same decomposition as the forward: a lane owns a query, wave group g sweeps the key tiles g, g+G, ...; with G = 2
// group 1's partial dQ is added to group 0's through LDS at the end.  Two register sets (prefetch distance 2).
template <bool BF16, bool ST16, int G>
__global__ __launch_bounds__(256 * G) void attn_bwd_dq_kernel(AttnArgs a) {
    using elem = typename ACfg<BF16>::elem;
    using SG = Stage<BF16, ST16>;
    using T = typename SG::T;
    constexpr int LR = ACfg<BF16>::LR, TILE = 64 * LR, NT = BF16 ? 3 : 2;   // K, V (+ K transposed for bf16)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [buffer][group][NT tiles]
    elem *smem = reinterpret_cast<elem *>(smem_raw);
    int bx_, by_;
    attn_block(a, bx_, by_, true);                         // (causal: blocks near the end of the sequence see the most keys)
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int wave = wave8 & 3, grp = wave8 >> 2;
    const int q = qblk + wave * 32 + l31;
    const bool qvalid = q < a.Sq;
    RowFrag<BF16> qf, dof;
    load_rowfrag<BF16, T>(qf, qvalid ? static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + q) * a.ldq + hh * 64 : nullptr, half);
    load_rowfrag<BF16, T>(dof, qvalid ? static_cast<const T *>(a.dO) + ((int64_t)b * a.Sq + q) * a.lddo + hh * 64 : nullptr, half);
    float dlt;
    if (a.DeltaOut) {       // Delta[b,head,q] = sum_d dO*O from the two row fragments already at hand (saves kk_attn_delta)
        RowFrag<BF16> of;
        load_rowfrag<BF16, T>(of, qvalid ? static_cast<const T *>(a.O) + ((int64_t)b * a.Sq + q) * a.ldo + hh * 64 : nullptr, half);
        dlt = rowfrag_dot<BF16>(dof, of);
        dlt += __shfl_xor(dlt, 32, 64);
        if (qvalid && half == 0 && grp == 0) a.DeltaOut[((int64_t)b * a.heads + hh) * a.Sq + q] = dlt;
    } else {
        dlt = qvalid ? a.Delta[((int64_t)b * a.heads + hh) * a.Sq + q] : 0.f;
    }
    ProbDrop pd;
    pd.init(a, b, hh);
    if (pd.thr) scale_rowfrag<BF16>(dof, pd.inv_keep);     // dP of a kept element carries 1/(1-p): fold it into dO once
    const float c2 = a.scale * 1.4426950408889634f;
    const float lse2 = qvalid ? a.LSE[((int64_t)b * a.heads + hh) * a.Sq + q] * 1.4426950408889634f : INFINITY;   // log2 domain
    f32x16 dq[2];
    zero_acc(dq[0]); zero_acc(dq[1]);
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    const int qmin = qblk + wave * 32;
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.Sk * a.ldv + hh * 64;
    struct Regs {
        typename SG::R rk, rv;
        typename SG::RT rkt;
        uint32_t rkm;
    };
    Regs ra, rb;
    ra.rkm = rb.rkm = 0;
    auto issue = [&](Regs &t, int k0) {
        const int nvalid = a.Sk - k0 < 64 ? a.Sk - k0 : 64;
        load_rows(t.rk, Kb + (int64_t)k0 * a.ldk, a.ldk, nvalid);
        load_rows(t.rv, Vb + (int64_t)k0 * a.ldv, a.ldv, nvalid);
        if constexpr (BF16) load_rows_T(t.rkt, Kb + (int64_t)k0 * a.ldk, a.ldk, nvalid);
        t.rkm = km ? (lane < nvalid ? km[k0 + lane] : 0u) : 0u;
    };
    auto commit = [&](const Regs &t, int buf) {
        elem *dst = smem + (buf * G + grp) * NT * TILE;
        SG::st(dst, t.rk);
        SG::st(dst + TILE, t.rv);
        if constexpr (BF16) SG::stT(dst + 2 * TILE, t.rkt);
    };
    constexpr int STEP = 64 * G;
    const int kfirst = grp * 64;
    if (kfirst < kend) {
        issue(ra, kfirst);
        commit(ra, 0);
    }
    uint64_t kmbits = __ballot(ra.rkm != 0u), kmnext = 0;
    if (kfirst + STEP < kend) issue(ra, kfirst + STEP);
    if (kfirst + 2 * STEP < kend) issue(rb, kfirst + 2 * STEP);
    __syncthreads();
    int cur = 0;
    auto tile_step = [&](Regs &X, int kk0) {
        const int k0 = kk0 + kfirst;
        const elem *Ks = smem + (cur * G + grp) * NT * TILE, *Vs = Ks + TILE, *Kt = BF16 ? Ks + 2 * TILE : Ks;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= kend) continue;
            if (a.causal && kb > qmin + 31) continue;
            f32x16 s, dp;
            zero_acc(s); zero_acc(dp);
            mma_tile_x_frag<BF16>(s, Ks, sub * 32, qf, l31, half);
            mma_tile_x_frag<BF16>(dp, Vs, sub * 32, dof, l31, half);
            const uint32_t kmsub = (uint32_t)(kmbits >> (sub * 32));
            const bool edge = kb + 32 > a.Sk || (a.causal && kb + 31 > qmin) || kmsub != 0u;
            float pv[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) pv[r] = __builtin_amdgcn_exp2f(s[r] * c2 - lse2);
            if (edge) {
                const uint32_t kml = kmsub >> (4 * half);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kb + frag_row(r, half);
                    const bool ok = key < a.Sk && !(a.causal && key > q) && !((kml >> frag_row(r, 0)) & 1u);
                    pv[r] = ok ? pv[r] : 0.f;
                }
            }
            if (pd.thr) {
                const uint32_t xb = pd.row(q, kb + 4 * half);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const uint32_t hsh = pd.hash(xb + (uint32_t)(frag_row(r, 0) >> 1));
                    ds[r] = pv[r] * ((pd.keep_lo(hsh) ? dp[r] : 0.f) - dlt);
                    ds[r + 1] = pv[r + 1] * ((pd.keep_hi(hsh) ? dp[r + 1] : 0.f) - dlt);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] = pv[r] * (dp[r] - dlt);
            }
            mma_T_x_p<BF16>(dq, Kt, sub * 32, ds, l31, half);     // (the softmax scale is applied once, at the store)
        }
        kmnext = 0;
        if (k0 + STEP < kend) {
            commit(X, cur ^ 1);
            kmnext = __ballot(X.rkm != 0u);
            if (k0 + 3 * STEP < kend) issue(X, k0 + 3 * STEP);
        }
        kmbits = kmnext;
        __syncthreads();
        cur ^= 1;
    };
    for (int kk0 = 0; kk0 < (KK_DBG(a, 32) ? 0 : kend); kk0 += 2 * STEP) {      // the bound is the same for both groups (barriers)
        tile_step(ra, kk0);
        if (kk0 + STEP < kend) tile_step(rb, kk0 + STEP);
    }
    if constexpr (G == 2) {          // group 1's partial dQ -> LDS -> group 0
        float *mb = reinterpret_cast<float *>(smem_raw) + (wave * 64 + lane) * 33;
        if (grp == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { mb[r] = dq[0][r]; mb[16 + r] = dq[1][r]; }
        }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { dq[0][r] += mb[r]; dq[1][r] += mb[16 + r]; }
        }
    }
    T *out_row = static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + q) * a.ldout + hh * 64;
    if (a.hn[0].raw == nullptr) {
        if (qvalid && grp == 0) store_row<T>(out_row, dq, a.scale, half);
        return;
    }
    float *colred = reinterpret_cast<float *>(smem_raw);          // [128 rows][65]
    __syncthreads();                                              // the staging tiles / merge buffer are free
    if (grp == 0)
        hn_bwd_row<T>(dq, a.scale, qvalid, static_cast<const T *>(a.hn[0].raw) + ((int64_t)b * a.Sq + q) * a.hn[0].ldraw + hh * 64,
                      out_row, a.hn[0], q, half, colred + (wave * 32 + l31) * 65);
    __syncthreads();
    hn_colsum(colred, a.hn[0].partials);
}

// ------------------------------------------------------------------ backward, second generation: shared pieces
// XOR value (on the 32-byte block index of a 128-byte row) of an image that is read BOTH as row fragments (ds_read_b128, the
// lane's own row) and through ds_read_b64_tr_b16 (four consecutive rows per 16-lane group): rows r and r+2 of a transpose
// read must differ in bit 1 of the block index (conflict-free), and the four values spread the row-fragment reads (2-way).
__device__ __forceinline__ int kk_xb(int r) { return (((r >> 1) & 1) << 1) | ((r >> 2) & 1); }

// Head-norm (+ RoPE) backward of the (row, head) vector this lane pair holds — hn_bwd_row with every operand in LDS: the
// raw projection tile and the RoPE rows were DMA'd there while the main loop ran, so the epilogue has no exposed global
// latency and no row-per-lane requests.  rawimg: [128][64] bf16, cosimg / sinimg: columns 0..31 of the table rows as
// [128][32] fp32 (rotate-half RoPE tables have identical halves, positional_encoding.py:129-150), all with the chunk XOR
// of dma_rows128.  The gradient of the raw projection comes back in the accumulator layout (out), for store_rows_via_lds.
// (core: the per-column contributions to the gain gradient come back in cr[32], accumulator order, for a caller whose colred buffer
//  shares LDS with the images and can only be written behind a barrier)
// the lane's 32 gain values (its columns db * 32 + 8 g + 4 half + e), fetched EARLY by the third-generation epilogues: eight dependent
// global loads in the middle of the row arithmetic were ~1 us of each head-norm epilogue
struct HnGain { float4 g4[8]; };
__device__ __forceinline__ HnGain hn_load_gain(const float *gain, int half) {
    HnGain r;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) r.g4[db * 4 + g] = ld4(gain + db * 32 + 8 * g + 4 * half);
    return r;
}
// (round 6: written on PAIRS — v_pk_mul_f32 / v_pk_fma_f32 on adjacent accumulator elements, one v_cvt_pk_bf16_f32 per two values, the
//  row mask on the packed word.  The compiler's own version of the scalar source was 737 vector instructions per call, a third of them
//  v_mov / v_cndmask to marshal pairs it had picked across the two halves of a row; these launches are bound by instruction issue —
//  profiles/r06_attn_pair_balance.txt — so the epilogues cost what they count.  Sums are taken pairwise: (even elements) + (odd elements).)
#ifndef KK_HN_CORE_V1
typedef float f32x2_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_ kk_unpack_bf16x2(uint32_t w) { return f32x2_{__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u)}; }
__device__ __forceinline__ void hn_bwd_row2_core(const f32x16 (&acc)[2], float mul, bool valid, const char *rawimg, const char *cosimg,
                                                 const char *sinimg, int row, bool rope, const HnGain &gn, int half, float (&cr)[32],
                                                 f32x16 (&out)[2]) {
    f32x2_ dn[16], v[16];                  // pair 8 db + 2 g + e2 = elements 4 g + 2 e2, + 1 of accumulator block db
    asm volatile("" : "+v"(row));          // (or the image addresses below are computed in the prologue and spilled across the main loop)
    const int swz = (row >> 1) & 7;
    const uint32_t vm = valid ? 0xFFFFFFFFu : 0u;
    const f32x2_ mul2 = {mul, mul};
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const kk_u32x2 w = *reinterpret_cast<const kk_u32x2 *>(rawimg + row * 128 + (((4 * db + g) ^ swz) * 16) + half * 8);
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                v[db * 8 + 2 * g + e2] = kk_unpack_bf16x2(w[e2]);
                const f32x2_ a2 = f32x2_{acc[db][4 * g + 2 * e2], acc[db][4 * g + 2 * e2 + 1]} * mul2;
                const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(a2, bf16x2_)) & vm;      // the bf16 the consumer of this gradient sees
                dn[db * 8 + 2 * g + e2] = kk_unpack_bf16x2(pk);
            }
        }
    f32x2_ sq2 = v[0] * v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) sq2 = __builtin_elementwise_fma(v[i], v[i], sq2);
    const float ssq = xor32_sum(sq2[0] + sq2[1]);
    const float rs = 1.f / sqrtf(ssq * (1.f / 64.f) + 1.1920928955078125e-7f);
    if (rope) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4_ c4 = *reinterpret_cast<const f32x4_ *>(cosimg + row * 128 + (((2 * g + half) ^ swz) * 16));
            const f32x4_ s4 = *reinterpret_cast<const f32x4_ *>(sinimg + row * 128 + (((2 * g + half) ^ swz) * 16));
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const f32x2_ cc = {c4[2 * e2], c4[2 * e2 + 1]}, ss = {s4[2 * e2], s4[2 * e2 + 1]};
                const f32x2_ lo = dn[2 * g + e2], hi = dn[8 + 2 * g + e2];
                dn[2 * g + e2] = __builtin_elementwise_fma(lo, cc, hi * ss);
                dn[8 + 2 * g + e2] = __builtin_elementwise_fma(hi, cc, -(lo * ss));
            }
        }
    }
    const f32x2_ rs2 = {rs, rs};
    f32x2_ kd2 = {0.f, 0.f};
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 g4 = gn.g4[db * 4 + g];
            const f32x2_ gg[2] = {{g4.x, g4.y}, {g4.z, g4.w}};
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const int i = db * 8 + 2 * g + e2;
                const f32x2_ c2 = (dn[i] * v[i]) * rs2;
                cr[2 * i] = c2[0];
                cr[2 * i + 1] = c2[1];
                dn[i] *= gg[e2];
                kd2 = __builtin_elementwise_fma(dn[i], v[i], kd2);
            }
        }
    const float kdot = xor32_sum(kd2[0] + kd2[1]);
    const float k = kdot * (1.f / 64.f) * rs * rs * rs;
    const f32x2_ k2 = {k, k};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const f32x2_ o2 = __builtin_elementwise_fma(rs2, dn[i], -(v[i] * k2));
        out[i >> 3][2 * (i & 7)] = o2[0];
        out[i >> 3][2 * (i & 7) + 1] = o2[1];
    }
}
#else
__device__ __forceinline__ void hn_bwd_row2_core(const f32x16 (&acc)[2], float mul, bool valid, const char *rawimg, const char *cosimg,
                                                 const char *sinimg, int row, bool rope, const HnGain &gn, int half, float (&cr)[32],
                                                 f32x16 (&out)[2]) {
    float dn[32], v[32];
    asm volatile("" : "+v"(row));          // (or the image addresses below are computed in the prologue and spilled across the main loop)
    const int swz = (row >> 1) & 7;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bf16x4 x4 = *reinterpret_cast<const bf16x4 *>(rawimg + row * 128 + (((4 * db + g) ^ swz) * 16) + half * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[db * 16 + 4 * g + e] = (float)x4[e];
                dn[db * 16 + 4 * g + e] = valid ? (float)(__bf16)(acc[db][4 * g + e] * mul) : 0.f;
            }
        }
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) ssq += v[i] * v[i];
    ssq = xor32_sum(ssq);
    const float rs = 1.f / sqrtf(ssq * (1.f / 64.f) + 1.1920928955078125e-7f);
    if (rope) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 c4 = *reinterpret_cast<const float4 *>(cosimg + row * 128 + (((2 * g + half) ^ swz) * 16));
            const float4 s4 = *reinterpret_cast<const float4 *>(sinimg + row * 128 + (((2 * g + half) ^ swz) * 16));
            const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = dn[4 * g + e], hi = dn[16 + 4 * g + e];
                dn[4 * g + e] = lo * cc[e] + hi * ss[e];
                dn[16 + 4 * g + e] = hi * cc[e] - lo * ss[e];
            }
        }
    }
    float kdot = 0.f;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 g4 = gn.g4[db * 4 + g];
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = db * 16 + 4 * g + e;
                cr[i] = dn[i] * v[i] * rs;
                dn[i] *= gg[e];
                kdot += dn[i] * v[i];
            }
        }
    kdot = xor32_sum(kdot);
    const float k = kdot * (1.f / 64.f) * rs * rs * rs;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[db][r] = rs * dn[db * 16 + r] - v[db * 16 + r] * k;
}
#endif
__device__ __forceinline__ void hn_colred_store(const float (&cr)[32], int half, float *colred_row) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) colred_row[db * 32 + 8 * g + 4 * half + e] = cr[db * 16 + 4 * g + e];
}
// Column sums of cr over the 32 rows a half-wave holds (lane = row), in registers: a transposing butterfly — at the step with partner
// mask m a lane keeps the half of its live values whose index bit matches its own lane bit and hands the other half to its partner: 31
// exchange-adds.  The partner masks are taken in the order 8, 2, 1, 16, 4, so that the three big steps (16 + 8 + 4 exchanges) are DPP
// operand modifiers (row_ror:8, quad_perm) and only the last 2 + 1 are ds_bpermute round trips.  Afterwards lane l31 holds the sum over
// the 32 rows of cr[i], i = hn_colsum32_idx(l31): index bit 4 <- lane bit 3, 3 <- 1, 2 <- 0, 1 <- 4, 0 <- 2.
// Replaces, per head-norm epilogue, 32 LDS stores per lane into colred[128][65], two workgroup barriers and ONE wave adding up 128 rows.
template <int N, int MASK> __device__ __forceinline__ void hn_colsum_step(float (&v)[32], int l31) {      // N live values
    const bool up = (l31 & MASK) != 0;
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float keep = up ? v[j + N / 2] : v[j], send = up ? v[j] : v[j + N / 2];
        float got;
        if constexpr (MASK == 8) got = kk_dpp<0x128>(send);
        else if constexpr (MASK == 2) got = kk_dpp<0x4E>(send);
        else if constexpr (MASK == 1) got = kk_dpp<0xB1>(send);
        else got = __shfl_xor(send, MASK, 64);
        v[j] = keep + got;
    }
}
__device__ __forceinline__ float hn_colsum32(float (&v)[32], int l31) {
    hn_colsum_step<32, 8>(v, l31);
    hn_colsum_step<16, 2>(v, l31);
    hn_colsum_step<8, 1>(v, l31);
    hn_colsum_step<4, 16>(v, l31);
    hn_colsum_step<2, 4>(v, l31);
    return v[0];
}
__device__ __forceinline__ int hn_colsum32_col(int l31, int half) {
    const int i = ((l31 >> 3) & 1) << 4 | ((l31 >> 1) & 1) << 3 | (l31 & 1) << 2 | ((l31 >> 4) & 1) << 1 | ((l31 >> 2) & 1);
    return (i >> 4) * 32 + 8 * ((i >> 2) & 3) + 4 * half + (i & 3);
}
// store_rows_via_lds through a tile of 16 rows (2304 bytes), two halves one after the other: fits the wave's OWN 4 KB of a dead
// 128-row image, so no workgroup barrier stands between the head-norm arithmetic and the stores.
__device__ __forceinline__ void store_rows_via_lds16(__bf16 *dst_row0, int64_t ld, int nvalid, const f32x16 (&acc)[2], float mul,
                                                     char *tile, int lane, int wt) {
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if ((l31 >> 4) == h) {
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (__bf16)(acc[db][4 * g + e] * mul);
                    *reinterpret_cast<bf16x4 *>(tile + (l31 & 15) * 144 + (db * 32 + 8 * g + 4 * half) * 2) = v;
                }
        }
        __builtin_amdgcn_wave_barrier();                       // (one wave: its LDS operations complete in order)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = (lane >> 3) + 8 * j, c = lane & 7;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(tile + row * 144 + c * 16);
            if (16 * h + row < nvalid) kk_store16(dst_row0 + (int64_t)(16 * h + row) * ld + c * 8, v, wt);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
__device__ __forceinline__ void hn_bwd_row2(const f32x16 (&acc)[2], float mul, bool valid, const char *rawimg, const char *cosimg,
                                            const char *sinimg, int row, bool rope, const float *gain, int half, float *colred_row,
                                            f32x16 (&out)[2]) {
    float cr[32];
    hn_bwd_row2_core(acc, mul, valid, rawimg, cosimg, sinimg, row, rope, hn_load_gain(gain, half), half, cr, out);
    hn_colred_store(cr, half, colred_row);
}
// the three epilogue images of a 128-row block (rows row0 .. of a sequence of S rows, position = row): raw | cos | sin
template <int NT = 512, typename HN> __device__ __forceinline__ void hn_dma_inputs(HN &h, int64_t seq_row0, int pos0, int nrows, int hh, char *img, int wave8) {
    dma_rows128<NT>(static_cast<const __bf16 *>(h.raw) + seq_row0 * h.ldraw + hh * 64, h.ldraw, nrows, img, wave8);
    if (h.rope) {       // (fp32 rows of 64 = 128 bf16-sized elements; the first 128 bytes of each)
        dma_rows128<NT>(reinterpret_cast<const __bf16 *>(h.cos_t + (int64_t)pos0 * 64), 128, nrows, img + 16384, wave8);
        dma_rows128<NT>(reinterpret_cast<const __bf16 *>(h.sin_t + (int64_t)pos0 * 64), 128, nrows, img + 32768, wave8);
    }
}

// ------------------------------------------------------------------ backward: dQ, second generation (bf16 storage)
// attn_bwd_dq_kernel<true, true, 2>'s arithmetic in attn_fwd2_kernel's structure: K / V tiles by DMA (K once, in an image
// that serves both the row fragments of S = K.Q^T and the transpose reads of dQ^T += K^T.dS^T), Q / dO / O rows by DMA (Delta
// from the fragments), the scores and dP of unit u+1 issued before the exponentials of unit u, the head-norm epilogue's
// operands prefetched into the prologue's LDS while the loop runs, 16-byte coalesced stores.
// (body of the dQ kernel: kk_attn_bwd_dq2.inc, included into attn_bwd_dq2_kernel below; as one wave group: kk_attn_bwd_dq3.inc)

// ------------------------------------------------------------------ backward: dK, dV
// A lane owns a key; the workgroup sweeps the query tiles.  G = 2: two wave groups take alternate query tiles of the
// same 128 keys (2 waves per SIMD, see attn_fwd_kernel) and group 1's dK / dV partial sums are added to group 0's
// through LDS at the end.  Staging: with G = 1 two register sets alternate and a tile's loads have two tile-times to land;
// with G = 2 the 256-register budget of 8 waves leaves room for one set (distance 1) — the second wave hides the rest.
template <bool BF16, bool ST16, int G>
__global__ __launch_bounds__(256 * G) void attn_bwd_dkv_kernel(AttnArgs a) {
    using elem = typename ACfg<BF16>::elem;
    using SG = Stage<BF16, ST16>;
    using T = typename SG::T;
    constexpr int LR = ACfg<BF16>::LR, TILE = 64 * LR, NT = BF16 ? 4 : 2;   // Q, dO (+ both transposed for bf16)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [buffer][group][NT tiles], then lse/delta rows
    elem *smem = reinterpret_cast<elem *>(smem_raw);
    float *stat = reinterpret_cast<float *>(smem_raw + (size_t)2 * G * NT * TILE * sizeof(elem));   // [buffer][group][2][64]
    int bx_, by_;
    attn_block(a, bx_, by_, false);                        // (causal: the first key blocks see the most queries)
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int kblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int wave = wave8 & 3, grp = wave8 >> 2, tl = threadIdx.x & 255;
    const int key = kblk + wave * 32 + l31;
    const bool kvalid = key < a.Sk;
    const bool kalive = kvalid && !(a.key_mask && a.key_mask[(int64_t)b * a.Sk + key]);
    RowFrag<BF16> kf, vf;
    load_rowfrag<BF16, T>(kf, kvalid ? static_cast<const T *>(a.K) + ((int64_t)b * a.Sk + key) * a.ldk + hh * 64 : nullptr, half);
    load_rowfrag<BF16, T>(vf, kvalid ? static_cast<const T *>(a.V) + ((int64_t)b * a.Sk + key) * a.ldv + hh * 64 : nullptr, half);
    f32x16 dk[2], dv[2];
    zero_acc(dk[0]); zero_acc(dk[1]); zero_acc(dv[0]); zero_acc(dv[1]);
    ProbDrop pd;
    pd.init(a, b, hh);
    if (pd.thr) scale_rowfrag<BF16>(vf, pd.inv_keep);       // dP = dO.V of a kept element carries 1/(1-p)
    const float c2 = a.scale * 1.4426950408889634f;
    const int kmaxw = kblk + wave * 32 + 31;                           // largest key of this wave
    const bool anydead = __ballot(!kalive) != 0ull;                    // masked / out-of-range keys in this wave
    const int qstart = a.causal ? (kblk / 64) * 64 : 0;
    const T *Qb = static_cast<const T *>(a.Q) + (int64_t)b * a.Sq * a.ldq + hh * 64;
    const T *dOb = static_cast<const T *>(a.dO) + (int64_t)b * a.Sq * a.lddo + hh * 64;
    const float *LSEb = a.LSE + ((int64_t)b * a.heads + hh) * a.Sq, *DLb = a.Delta + ((int64_t)b * a.heads + hh) * a.Sq;
    struct Regs {
        typename SG::R rq, rdo;
        typename SG::RT rqt, rdot;
        float lse, dlt;
    };
    constexpr int DIST = G == 1 ? 2 : 1;                   // prefetch distance in tiles (= register sets)
    Regs ra;
    typename std::conditional<DIST == 2, Regs, int>::type rb_store;
    Regs &rb = [&]() -> Regs & { if constexpr (DIST == 2) return rb_store; else return ra; }();
    auto issue = [&](Regs &t, int q0) {
        const int nvalid = a.Sq - q0 < 64 ? a.Sq - q0 : 64;
        load_rows(t.rq, Qb + (int64_t)q0 * a.ldq, a.ldq, nvalid);
        load_rows(t.rdo, dOb + (int64_t)q0 * a.lddo, a.lddo, nvalid);
        if constexpr (BF16) {
            load_rows_T(t.rqt, Qb + (int64_t)q0 * a.ldq, a.ldq, nvalid);
            load_rows_T(t.rdot, dOb + (int64_t)q0 * a.lddo, a.lddo, nvalid);
        }
        if (tl < 64) {
            const int qq = q0 + tl;
            t.lse = qq < a.Sq ? LSEb[qq] * 1.4426950408889634f : INFINITY;      // log2 domain
            t.dlt = qq < a.Sq ? DLb[qq] : 0.f;
        }
    };
    auto commit = [&](const Regs &t, int buf) {
        elem *dst = smem + (buf * G + grp) * NT * TILE;
        SG::st(dst, t.rq);
        SG::st(dst + TILE, t.rdo);
        if constexpr (BF16) {
            SG::stT(dst + 2 * TILE, t.rqt);
            SG::stT(dst + 3 * TILE, t.rdot);
        }
        if (tl < 64) {
            float *st = stat + (buf * G + grp) * 128;
            st[tl] = t.lse;
            st[64 + tl] = t.dlt;
        }
    };
    constexpr int STEP = 64 * G;
    const int qfirst = qstart + grp * 64;
    if (qfirst < a.Sq) {
        issue(ra, qfirst);
        commit(ra, 0);
    }
    if (qfirst + STEP < a.Sq) issue(ra, qfirst + STEP);
    if (DIST == 2 && qfirst + 2 * STEP < a.Sq) issue(rb, qfirst + 2 * STEP);
    __syncthreads();
    int cur = 0;
    auto tile_step = [&](Regs &X, int qq0) {
        const int q0 = qq0 + grp * 64;
        const elem *Qs = smem + (cur * G + grp) * NT * TILE, *dOs = Qs + TILE;
        const elem *Qt = BF16 ? Qs + 2 * TILE : Qs, *dOt = BF16 ? Qs + 3 * TILE : dOs;
        const float *lse_t = stat + (cur * G + grp) * 128, *dlt_t = lse_t + 64;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int qb = q0 + sub * 32;
            if (qb >= a.Sq) continue;
            if (a.causal && qb + 31 < kblk + wave * 32) continue;
            f32x16 s, dp;
            zero_acc(s); zero_acc(dp);
            mma_tile_x_frag<BF16>(s, Qs, sub * 32, kf, l31, half);
            mma_tile_x_frag<BF16>(dp, dOs, sub * 32, vf, l31, half);
            const bool edge = anydead || qb + 32 > a.Sq || (a.causal && kmaxw > qb);
            float p[16], ds[16];
            const float *lse_r = lse_t + sub * 32 + 4 * half, *dlt_r = dlt_t + sub * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = __builtin_amdgcn_exp2f(s[r] * c2 - lse_r[frag_row(r, 0)]);
            if (edge) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qq = qb + frag_row(r, half);
                    const bool ok = kalive && qq < a.Sq && !(a.causal && key > qq);
                    p[r] = ok ? p[r] : 0.f;
                }
            }
            if (pd.thr) {
                const uint32_t xb = pd.row(qb + 4 * half, key);
                const bool odd = key & 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t hsh = pd.hash(xb + (uint32_t)frag_row(r, 0) * pd.sk2);
                    const bool keep = odd ? pd.keep_hi(hsh) : pd.keep_lo(hsh);
                    ds[r] = p[r] * ((keep ? dp[r] : 0.f) - dlt_r[frag_row(r, 0)]);
                    p[r] = keep ? p[r] : 0.f;                         // dropped probabilities feed dV (1/(1-p) at the store)
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] = p[r] * (dp[r] - dlt_r[frag_row(r, 0)]);
            }
            mma_T_x_p<BF16>(dv, dOt, sub * 32, p, l31, half);
            mma_T_x_p<BF16>(dk, Qt, sub * 32, ds, l31, half);
        }
        if (q0 + STEP < a.Sq) {
            commit(X, cur ^ 1);
            if (q0 + (DIST + 1) * STEP < a.Sq) issue(X, q0 + (DIST + 1) * STEP);
        }
        __syncthreads();
        cur ^= 1;
    };
    for (int qq0 = qstart; qq0 < (KK_DBG(a, 32) ? 0 : a.Sq); qq0 += 2 * STEP) {              // the bound is the same for both groups (barriers)
        tile_step(ra, qq0);
        if (qq0 + STEP < a.Sq) tile_step(rb, qq0 + STEP);
    }
    if constexpr (G == 2) {          // group 1's partial dK / dV -> LDS -> group 0
        float *mb = reinterpret_cast<float *>(smem_raw) + (wave * 64 + lane) * 65;      // 64 floats per lane (+1: bank spread)
        if (grp == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { mb[r] = dk[0][r]; mb[16 + r] = dk[1][r]; mb[32 + r] = dv[0][r]; mb[48 + r] = dv[1][r]; }
        }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[0][r] += mb[r]; dk[1][r] += mb[16 + r]; dv[0][r] += mb[32 + r]; dv[1][r] += mb[48 + r]; }
        }
    }
    T *dk_row = static_cast<T *>(a.Out) + ((int64_t)b * a.Sk + key) * a.ldout + hh * 64;
    T *dv_row = static_cast<T *>(a.Out2) + ((int64_t)b * a.Sk + key) * a.ldout2 + hh * 64;
    if (a.hn[0].raw == nullptr) {
        if (kvalid && grp == 0) {
            store_row<T>(dk_row, dk, a.scale, half);
            store_row<T>(dv_row, dv, pd.inv_keep, half);
        }
        return;
    }
    float *colred = reinterpret_cast<float *>(smem_raw);          // [128 rows][65]
    const int64_t rrow = (int64_t)b * a.Sk + key;
    __syncthreads();
    if (grp == 0)
        hn_bwd_row<T>(dk, a.scale, kvalid, static_cast<const T *>(a.hn[0].raw) + rrow * a.hn[0].ldraw + hh * 64, dk_row, a.hn[0], key,
                      half, colred + (wave * 32 + l31) * 65);
    __syncthreads();
    hn_colsum(colred, a.hn[0].partials);
    __syncthreads();
    if (grp == 0)
        hn_bwd_row<T>(dv, pd.inv_keep, kvalid, static_cast<const T *>(a.hn[1].raw) + rrow * a.hn[1].ldraw + hh * 64, dv_row, a.hn[1], key,
                      half, colred + (wave * 32 + l31) * 65);
    __syncthreads();
    hn_colsum(colred, a.hn[1].partials);
}

// ------------------------------------------------------------------ backward: the DMA-staged kernels (bf16 storage)
// The bodies live in .inc files because they must name a by-value KERNEL parameter: handed to a device function by reference
// (or read through a pointer to the kernarg segment) the same code spills 5-11 vector registers, and a spill is fatal beside
// LDS-DMA (scratch reloads queue behind the tile DMAs).
// Second generation, two wave groups: the dQ kernel that also writes Delta (kk_attn_bwd_dq given O).
__global__ __launch_bounds__(512) void attn_bwd_dq2_kernel(AttnArgs a) {
#include "kk_attn_bwd_dq2.inc"
}

// ------------------------------------------------------------------ backward, third generation: one wave group, two workgroups per CU
// The second-generation bodies as ONE 256-thread group each (kk_attn_bwd_dq3.inc / kk_attn_bwd_dkv3.inc): <= 70 KB of LDS, so two
// workgroups share a CU.  The dK/dV body is attn_bwd_dkv_kernel<true, true, 2>'s arithmetic; Q and dO tiles reach LDS once each by
// DMA, in the image that serves both the row fragments (S^T = Q.K^T, dP^T = dO.V^T) and the transpose reads (dV^T += dO^T.P,
// dK^T += Q^T.dS); lse / Delta rows by DMA; K and V rows, the head-norm epilogues' operands and the outputs as in the dQ body.  The waves per SIMD stay two (256 registers: the dK/dV half holds 64 accumulator registers per wave,
// DESIGN section 9) but they now belong to INDEPENDENT workgroups: no common barrier, one's prologue / epilogue under the other's
// loop, no merge of group partials, and the 2 x 256 workgroups of an 8 x 8 x 512^2 launch are resident at once (one round).  In the
// pair launch the dK/dV half of a causal launch hands out its SHORT blocks first: the i-th workgroup of each half land on the same
// CU, so every CU holds a long block of one kernel beside a short block of the other, concurrently.
__global__ __launch_bounds__(256, 2) void attn_bwd_dq3_kernel(AttnArgs a) {
#include "kk_attn_bwd_dq3.inc"
}
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv3_kernel(AttnArgs a) {
#include "kk_attn_bwd_dkv3.inc"
}
// dQ and dK/dV of one attention in ONE launch (grid z picks the half; Delta is an INPUT of both, see kk_gemm_dgrad_delta).  The two
// kernels are independent once Delta exists, and a causal launch is lopsided: dQ blocks near the end of the sequence see the most
// keys, dK/dV blocks near its start the most queries; a non-causal pair saves one launch's ramp and tail.
// Dispatch order: the dK/dV half (z = 0) goes out FIRST.  Its workgroups are the long ones (26.5 against 17.5 us at 512 x 512, four
// matmuls and two head-norm epilogues against three and one); dispatched last they are what a slot delayed by the side branch's
// workgroups finishes with.  Stand-alone the order makes no difference (32.5 us either way); inside the step it is -0.5 % at 8 x 512
// and -0.6 % at 8 x 1024 (interleaved, profiles/r05_attn_bwd_dispatch_order_ab.txt).  Probe bit 2048 restores dQ first.
__global__ __launch_bounds__(256, 2) void attn_bwd_pair3_kernel(AttnArgs a_dq, AttnArgs a_dkv) {
    KK_WG_STAMP(a_dq);
    if ((blockIdx.z == 1) != KK_DBG(a_dq, 2048)) {
#define a a_dq
#include "kk_attn_bwd_dq3.inc"
#undef a
    } else {
#define a a_dkv
#include "kk_attn_bwd_dkv3.inc"
#undef a
    }
}
// The pair launch that READS the dropout keep decisions the forward stored (AttnArgs::keep) instead of hashing them again: the same
// bodies compiled with KK_KEEP_BITS — same arithmetic on the same decisions, bit-identical outputs (tests), ~100 vector instructions
// per 32 x 32 unit less in each half.
#define KK_KEEP_BITS 1
__global__ __launch_bounds__(256, 2) void attn_bwd_pair3k_kernel(AttnArgs a_dq, AttnArgs a_dkv) {
    KK_WG_STAMP(a_dq);
    if ((blockIdx.z == 1) != KK_DBG(a_dq, 2048)) {             // (dK/dV first: see attn_bwd_pair3_kernel)
#define a a_dq
#include "kk_attn_bwd_dq3.inc"
#undef a
    } else {
#define a a_dkv
#include "kk_attn_bwd_dkv3.inc"
#undef a
    }
}
#undef KK_KEEP_BITS

// ------------------------------------------------------------------ backward in two passes (kk_attn_bwd_ws)
// The pair launch computes the scores, the exponentials, the dropout masks and dS TWICE (once per kernel: 7 S x S x 64 matmuls and
// ~560 vector instructions per 32 x 32 unit where the algorithm needs 5 and ~330), because dQ is a sum over keys and dK / dV sums
// over queries.  Here the dK/dV kernel — the same body — also stores dS as it feeds it to its dK MFMAs (bf16, [32 keys][32
// queries] tiles of 2 KB: 2 bytes per score, 32 MB per launch at 8 x 8 x 512^2, mostly served back by the Infinity Cache), and dQ =
// dS . K becomes a pass with NO vector work: four waves (one per 32 queries) stream K tiles and their dS tiles through a three-stage
// DMA ring and issue 4 MFMAs per unit, both operands by transpose reads (K^T as in the dQ kernel; dS^T [key][query] the same way: a
// 512-byte span of a tile per instruction, conflict free without a swizzle); the head-norm epilogue of the dQ kernel follows.
// dS is bit-identical to what the dQ kernel computes for itself (same MFMA sums, same rounding), so dQ differs from the pair
// launch's only by the order in which the key units are added (all of them in sequence here; two interleaved halves there).
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv3s_kernel(AttnArgs a) {      // (the one-group body: what kk_attn_bwd's dK/dV half runs)
#define KK_DKV_STORE_DS 1
#include "kk_attn_bwd_dkv3.inc"
#undef KK_DKV_STORE_DS
}

__global__ __launch_bounds__(256) void attn_bwd_dqpass_kernel(AttnArgs a) {
    typedef __bf16 T;
    constexpr int NS = 3, KIMG = 64 * 64 * 2, DIMG = 2 * 4 * 2048, STAGE = KIMG + DIMG, NPT = 6;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [stage][K image | 2 key units x 4 query units of dS]
    int bx_, by_;
    attn_block(a, bx_, by_, true);
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int qmin = qblk + 32 * wave;
    const bool qvalid = qmin + l31 < a.Sq;
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    int klim = kend;
    if (a.causal && qmin + 32 < klim) klim = qmin + 32;
    const int nt = (kend + 63) >> 6;
    const int nqu4 = ((a.Sq + 127) >> 7) << 2, nku = (a.Sk + 31) >> 5;
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const char *dsb = static_cast<const char *>(a.dS) + (int64_t)(b * a.heads + hh) * nku * nqu4 * 2048;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Kb), 0, (int)((((int64_t)a.Sk - 1) * a.ldk + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(dsb), 0, (int)((int64_t)nku * nqu4 * 2048), 0x00020000);
    uint32_t kvo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = threadIdx.x + 256 * j, row = p >> 3, pc = p & 7;
        kvo[j] = (uint32_t)(((int64_t)row * a.ldk + ((pc ^ (kk_xb(row) << 1)) * 8)) * 2);
    }
    const uint32_t ktile = (uint32_t)(64 * a.ldk * 2);
    const uint32_t drow = (uint32_t)(nqu4 * 2048), dq0 = (uint32_t)((qblk >> 5) * 2048 + threadIdx.x * 16);
    auto issue_tile = [&](int t, int st) {
        char *dst = smem_raw + st * STAGE + wave * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, KK_LDS_PTR(dst + j * 4096), 16, kvo[j] + (uint32_t)t * ktile, 0, 0, 0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j)           // the four query units' tiles of a key unit are one 8 KB run
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, KK_LDS_PTR(dst + KIMG + kk * 8192 + j * 4096), 16,
                                                         (uint32_t)(2 * t + kk) * drow + dq0 + (uint32_t)j * 4096, 0, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nt) issue_tile(t, t);
    const uint32_t sl = (uint32_t)(uintptr_t)KK_LDS_PTR(smem_raw);
    uint32_t ta[2], da;
    {
        const int L = lane & 15, kq = L >> 2, gi = (lane >> 4) & 1, xb = (((kq >> 1) & 1) << 1) | half;
#pragma unroll
        for (int db = 0; db < 2; ++db) ta[db] = (uint32_t)((4 * half + kq) * 128 + (((2 * db + gi) ^ xb) * 32) + 8 * (L & 3));
        da = (uint32_t)(KIMG + wave * 2048 + (4 * half + kq) * 64 + gi * 32 + 8 * (L & 3));
    }
    f32x16 dq[2];
    zero_acc(dq[0]); zero_acc(dq[1]);
    for (int t = 0; t < nt; ++t) {
        const int younger = min(nt - 1 - t, NS - 2);
        if (younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NS - 1 < nt) issue_tile(t + NS - 1, (t + NS - 1) % NS);
        const uint32_t stg = sl + (uint32_t)((t % NS) * STAGE);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (t * 64 + 32 * kk >= klim) continue;
            s16x4 tlo[4], thi[4], dlo[2], dhi[2];
            const uint32_t a0 = stg + kk * 4096 + ta[0], a1 = stg + kk * 4096 + ta[1], d0 = stg + kk * 8192 + da;
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dlo[0]) : "v"(d0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512" : "=v"(dhi[0]) : "v"(d0));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(tlo[0]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(thi[0]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(tlo[1]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(thi[1]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(dlo[1]) : "v"(d0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1536" : "=v"(dhi[1]) : "v"(d0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(tlo[2]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(thi[2]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(tlo[3]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(thi[3]) : "v"(a1));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(tlo[i]), "+v"(thi[i]));
#pragma unroll
            for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(dlo[i]), "+v"(dhi[i]));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(tlo[s2 * 2 + db], thi[s2 * 2 + db]), tr_pair(dlo[s2], dhi[s2]), dq[db], 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                           // the ring is free
    T *out0 = static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + qmin) * a.ldout + hh * 64;
    char *otile = smem_raw + 36864 + wave * 4608;
    if (a.hn[0].raw == nullptr) {
        store_rows_via_lds(out0, a.ldout, a.Sq - qmin, dq, a.scale, otile, lane, a.wt);
        return;
    }
    const int nrows = a.Sq - qblk < 128 ? a.Sq - qblk : 128;
    hn_dma_inputs<256>(a.hn[0], (int64_t)b * a.Sq + qblk, qblk, nrows, hh, smem_raw, wave);       // raw | cos | sin: 48 KB
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 dx[2];
    float cr[32];
    hn_bwd_row2_core(dq, a.scale, qvalid, smem_raw, smem_raw + 16384, smem_raw + 32768, wave * 32 + l31, a.hn[0].rope != 0, hn_load_gain(a.hn[0].gain, half), half, cr, dx);
    __syncthreads();                                           // every wave has read its image rows: colred and the store tiles lie over them
    float *colred = reinterpret_cast<float *>(smem_raw);       // [128 rows][65]
    hn_colred_store(cr, half, colred + (wave * 32 + l31) * 65);
    store_rows_via_lds(out0, a.ldout, a.Sq - qmin, dx, 1.f, otile, lane, a.wt);
    __syncthreads();
    hn_colsum(colred, a.hn[0].partials);
}

// Delta[b,h,q] = sum_d dO*O : one wave per (row, head).
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T *__restrict__ O, const T *__restrict__ dO,
                                                         float *__restrict__ Delta, int64_t npairs, int heads, int Sq,
                                                         int64_t ldo, int64_t lddo) {
    const int lane = threadIdx.x & 63;
    for (int64_t pr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pr < npairs; pr += (int64_t)gridDim.x * 4) {
        const int64_t row = pr / heads;
        const int hd = (int)(pr - row * heads);
        const float v = wave_sum((float)O[row * ldo + hd * 64 + lane] * (float)dO[row * lddo + hd * 64 + lane]);
        if (lane == 0) {
            const int64_t b = row / Sq, q = row - b * Sq;
            Delta[(b * heads + hd) * Sq + q] = v;
        }
    }
}

}  // namespace

// rows of the [workgroups][64] partial gain-gradient matrix a backward launch with a head-norm epilogue writes
extern "C" int kk_attn_bwd_blocks(int B, int heads, int S) { return kk_cdiv(S, 128) * B * heads; }

extern "C" int kk_attn_delta(const float *O, const float *dO, float *Delta, int B, int heads, int Sq, int64_t ldo,
                             int64_t lddo, int io_bf16, void *stream) {
    KK_REQUIRE(B > 0 && heads > 0 && Sq > 0, "kk_attn_delta: bad shape");
    const int64_t npairs = (int64_t)B * Sq * heads;
    int blocks = kk_cdiv(npairs, 4);
    if (blocks > 8192) blocks = 8192;
    if (io_bf16)
        hipLaunchKernelGGL(attn_delta_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const __bf16 *>(O),
                           reinterpret_cast<const __bf16 *>(dO), Delta, npairs, heads, Sq, ldo, lddo);
    else
        hipLaunchKernelGGL(attn_delta_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, O, dO, Delta, npairs, heads, Sq, ldo, lddo);
    KK_LAUNCH_CHECK("kk_attn_delta");
    return 0;
}

extern "C" int kk_attn_bwd_dq(const float *Q, const float *K, const float *V, const float *dO, const float *LSE,
                              float *Delta, float *dQ, int B, int heads, int Sq, int Sk, int64_t ldq,
                              int64_t ldk, int64_t ldv, int64_t lddo, int64_t lddq, const uint8_t *key_mask,
                              int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop, int math,
                              int io_bf16, const float *O, int64_t ldo, const KkAttnHeadNorm *hn, void *stream) {
    KK_REQUIRE(!io_bf16 || math == KK_MATH_BF16, "kk_attn_bwd_dq: bf16 storage needs KK_MATH_BF16");
    const int64_t lds[5] = {ldq, ldk, ldv, lddo, lddq};
    if (int rc = check_common("kk_attn_bwd_dq", B, heads, Sq, Sk, math, lds, 5)) return rc;
    AttnArgs a = attn_args(Q, K, V, B, heads, Sq, Sk, ldq, ldk, ldv, key_mask, causal, scale, seed, site, p_drop);
    a.dO = dO; a.LSE = LSE; a.Delta = Delta; a.lddo = lddo; a.Out = dQ; a.ldout = lddq;
    if (O) {                                  // Delta is an OUTPUT of this call (and still the input of kk_attn_bwd_dkv)
        KK_REQUIRE(ldo % 8 == 0 && ldo >= 64 * heads, "kk_attn_bwd_dq: row stride of O unsupported");
        a.O = O; a.ldo = ldo; a.DeltaOut = Delta;
    }
    if (hn) {
        if (int rc = check_headnorm("kk_attn_bwd_dq", hn, 1)) return rc;
        a.hn[0] = hn[0];
    }
    dim3 grid(kk_cdiv(Sq, 128), B * heads);
    const int G = (Sk > 64 && g_attn_groups == 2) ? 2 : 1;
    if (dma_storage(io_bf16, math, 2) && dma_tiles(Sk > 64, Sq, Sk) && Sk <= 4096 && al16_all({Q, K, V, dO, dQ, O}) && dma_hn_q(hn) &&
        dma_bytes(Sk, ldk, ldv)) {
        kk_note_kernel(!O ? "attn_bwd_dq3" : "attn_bwd_dq2");      // (the one-group kernel has no Delta output)
        int rc2 = !O ? launch_attn(attn_bwd_dq3_kernel, grid, 1, (size_t)3 * 16384 + 512 + 16384, (hipStream_t)stream, a)
                     : launch_attn(attn_bwd_dq2_kernel, grid, 2, (size_t)2 * 3 * 16384 + 512 + 3 * 16384, (hipStream_t)stream, a);
        if (rc2) return rc2;
        KK_LAUNCH_CHECK("kk_attn_bwd_dq");
        return 0;
    }
    kk_note_kernel("attn_bwd_dq");
    if (io_bf16) KK_ATTN_LAUNCH(attn_bwd_dq_kernel, true, true, G, 3);
    else if (math == KK_MATH_BF16) KK_ATTN_LAUNCH(attn_bwd_dq_kernel, true, false, G, 3);
    else KK_ATTN_LAUNCH(attn_bwd_dq_kernel, false, false, G, 2);
    KK_LAUNCH_CHECK("kk_attn_bwd_dq");
    return 0;
}

extern "C" int kk_attn_bwd_dkv(const float *Q, const float *K, const float *V, const float *dO, const float *LSE,
                               const float *Delta, float *dK, float *dV, int B, int heads, int Sq, int Sk,
                               int64_t ldq, int64_t ldk, int64_t ldv, int64_t lddo, int64_t lddk, int64_t lddv,
                               const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site,
                               float p_drop, int math, int io_bf16, const KkAttnHeadNorm *hn, void *stream) {
    KK_REQUIRE(!io_bf16 || math == KK_MATH_BF16, "kk_attn_bwd_dkv: bf16 storage needs KK_MATH_BF16");
    const int64_t lds[6] = {ldq, ldk, ldv, lddo, lddk, lddv};
    if (int rc = check_common("kk_attn_bwd_dkv", B, heads, Sq, Sk, math, lds, 6)) return rc;
    AttnArgs a = attn_args(Q, K, V, B, heads, Sq, Sk, ldq, ldk, ldv, key_mask, causal, scale, seed, site, p_drop);
    a.dO = dO; a.LSE = LSE; a.Delta = Delta; a.lddo = lddo; a.Out = dK; a.Out2 = dV; a.ldout = lddk; a.ldout2 = lddv;
    if (hn) {
        if (int rc = check_headnorm("kk_attn_bwd_dkv", hn, 2)) return rc;
        a.hn[0] = hn[0]; a.hn[1] = hn[1];
    }
    dim3 grid(kk_cdiv(Sk, 128), B * heads);
    const int G = (Sq > 64 && g_attn_groups == 2) ? 2 : 1;          // one query tile: nothing to split
    if (dma_storage(io_bf16, math, 4) && dma_tiles(Sq > 64, Sq, Sk) && al16_all({Q, K, V, dO, dK, dV}) && dma_hn_kv(hn) && dma_bytes(Sq, ldq, lddo)) {
        kk_note_kernel("attn_bwd_dkv3");
        if (int rc = launch_attn(attn_bwd_dkv3_kernel, grid, 1, (size_t)71680, (hipStream_t)stream, a)) return rc;
        KK_LAUNCH_CHECK("kk_attn_bwd_dkv");
        return 0;
    }
    kk_note_kernel("attn_bwd_dkv");
    if (io_bf16) KK_ATTN_LAUNCH_X(attn_bwd_dkv_kernel, true, true, G, 4, 2 * G * 128 * sizeof(float));
    else if (math == KK_MATH_BF16) KK_ATTN_LAUNCH_X(attn_bwd_dkv_kernel, true, false, 1, 4, 2 * 128 * sizeof(float));   // (G = 2 would spill)
    else KK_ATTN_LAUNCH_X(attn_bwd_dkv_kernel, false, false, G, 2, 2 * G * 128 * sizeof(float));
    KK_LAUNCH_CHECK("kk_attn_bwd_dkv");
    return 0;
}

// dQ, dK and dV in one launch (attn_bwd_pair3_kernel, or attn_bwd_pair3k_kernel reading keep bits) when both DMA-staged kernels
// apply; otherwise the two launches above, in order.  Delta[b, head, q] = sum_d dO * O is an INPUT here (kk_gemm_dgrad_delta writes it
// with dO, or kk_attn_delta).  hn_q / hn_kv: the head-norm backward epilogues of kk_attn_bwd_dq / kk_attn_bwd_dkv (both or neither).
static int attn_bwd_impl(const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Delta,
                         float *dQ, float *dK, float *dV, int B, int heads, int Sq, int Sk, int64_t ldq, int64_t ldk,
                         int64_t ldv, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, const uint8_t *key_mask,
                         int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop, int math, int io_bf16,
                         const KkAttnHeadNorm *hn_q, const KkAttnHeadNorm *hn_kv, const void *keep, void *stream) {
    KK_REQUIRE(Delta != nullptr, "kk_attn_bwd: Delta is an input of this call");
    KK_REQUIRE((hn_q == nullptr) == (hn_kv == nullptr), "kk_attn_bwd: head-norm epilogues for both kernels or for neither");
    const bool pair = dma_both(io_bf16, math, Sq, Sk, Q, K, V, dO, dQ, dK, dV, ldq, ldk, ldv, lddo, hn_q, hn_kv) && attn_pair() &&
                      dma_tiles(Sq > 64 && Sk > 64, Sq, Sk) && kk_cdiv(Sq, 128) == kk_cdiv(Sk, 128);
    if (!pair) {
        g_warm_bytes[0] = g_warm_bytes[1] = 0u;                 // (one-shot: a launch that cannot warm drops the request, it never waits for a later one)
        if (int rc = kk_attn_bwd_dq(Q, K, V, dO, LSE, const_cast<float *>(Delta), dQ, B, heads, Sq, Sk, ldq, ldk, ldv, lddo, lddq, key_mask,
                                    causal, scale, seed, site, p_drop, math, io_bf16, nullptr, 0, hn_q, stream))
            return rc;
        return kk_attn_bwd_dkv(Q, K, V, dO, LSE, Delta, dK, dV, B, heads, Sq, Sk, ldq, ldk, ldv, lddo, lddk, lddv, key_mask, causal,
                               scale, seed, site, p_drop, math, io_bf16, hn_kv, stream);
    }
    KK_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "kk_attn_bwd: dropout probability must be in [0,1)");
    const int64_t lds[7] = {ldq, ldk, ldv, lddo, lddq, lddk, lddv};
    if (int rc = check_common("kk_attn_bwd", B, heads, Sq, Sk, math, lds, 7)) return rc;
    AttnArgs a = attn_args(Q, K, V, B, heads, Sq, Sk, ldq, ldk, ldv, key_mask, causal, scale, seed, site, p_drop);
    a.dO = dO; a.LSE = LSE; a.Delta = Delta; a.lddo = lddo;
    if (a.xcd_map && causal) a.xcd_map = 2;                    // (the pair launch: always block-major when causal)
    AttnArgs a_dq = a, a_dkv = a;
    a_dq.Out = dQ; a_dq.ldout = lddq;
    a_dkv.Out = dK; a_dkv.Out2 = dV; a_dkv.ldout = lddk; a_dkv.ldout2 = lddv;
    a_dq.warm[0] = g_warm_ptr[0]; a_dq.warm[1] = g_warm_ptr[1];          // the dQ half warms the next GEMMs' weights
    a_dq.warm_bytes[0] = g_warm_bytes[0]; a_dq.warm_bytes[1] = g_warm_bytes[1];
    g_warm_bytes[0] = g_warm_bytes[1] = 0u;                     // (one-shot)
    if (hn_q) {
        if (int rc = check_headnorm("kk_attn_bwd", hn_q, 1)) return rc;
        if (int rc = check_headnorm("kk_attn_bwd", hn_kv, 2)) return rc;
        a_dq.hn[0] = hn_q[0];
        a_dkv.hn[0] = hn_kv[0]; a_dkv.hn[1] = hn_kv[1];
    }
    // (short blocks first only when both halves are resident at once — 2 workgroups per CU; with more rounds the longest-first
    //  order is the faster one: 8 x 8 x 1024^2 causal 79 against 96 us)
    a_dkv.short_first = (causal && attn_short_first() && (int64_t)kk_cdiv(Sq, 128) * B * heads <= g_attn_cus()) ? 1 : 0;
#ifdef KK_TUNING_HOOKS
    if (a.dbg & (256 | 4096)) { a_dq.DeltaOut = static_cast<float *>(g_attn_trace); a_dkv.DeltaOut = static_cast<float *>(g_attn_trace); }      // (stamp buffer: 8 rows x 64)
#endif
    const bool bits = keep != nullptr && p_drop > 0.f && Sk > 128 && kk_attn_keep_bytes(B, heads, Sq, Sk) > 0;      // (exactly the launches whose forward stored the bits)
    if (bits) a_dq.keep = a_dkv.keep = const_cast<void *>(keep);
    const auto kernel = bits ? attn_bwd_pair3k_kernel : attn_bwd_pair3_kernel;
    const size_t lds3 = 71680;                                 // one wave group per workgroup: two workgroups per CU
    if (int rc = attn_raise_lds((const void *)kernel, lds3, "kk_attn_bwd")) return rc;
    kk_note_kernel(bits ? "attn_bwd_pair3k" : "attn_bwd_pair3");
    hipLaunchKernelGGL(kernel, dim3(kk_cdiv(Sq, 128), B * heads, 2), dim3(256), lds3, (hipStream_t)stream, a_dq, a_dkv);
    KK_LAUNCH_CHECK("kk_attn_bwd");
    return 0;
}

extern "C" int kk_attn_bwd(const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Delta,
                           float *dQ, float *dK, float *dV, int B, int heads, int Sq, int Sk, int64_t ldq, int64_t ldk,
                           int64_t ldv, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, const uint8_t *key_mask,
                           int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop, int math, int io_bf16,
                           const KkAttnHeadNorm *hn_q, const KkAttnHeadNorm *hn_kv, void *stream) {
    return attn_bwd_impl(Q, K, V, dO, LSE, Delta, dQ, dK, dV, B, heads, Sq, Sk, ldq, ldk, ldv, lddo, lddq, lddk, lddv, key_mask, causal,
                         scale, seed, site, p_drop, math, io_bf16, hn_q, hn_kv, nullptr, stream);
}
// kk_attn_bwd reading the keep decisions kk_attn_fwd_kb stored for the SAME launch parameters (seed value, site, p_drop, shape): the
// pair launch then reads bits where it would hash (bit-identical results); every fall-back path ignores `keep` and hashes.
extern "C" int kk_attn_bwd_kb(const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Delta,
                              float *dQ, float *dK, float *dV, int B, int heads, int Sq, int Sk, int64_t ldq, int64_t ldk,
                              int64_t ldv, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, const uint8_t *key_mask,
                              int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop, int math, int io_bf16,
                              const KkAttnHeadNorm *hn_q, const KkAttnHeadNorm *hn_kv, const void *keep, void *stream) {
    KK_REQUIRE(keep == nullptr || al16(keep), "kk_attn_bwd_kb: unaligned keep buffer");
    return attn_bwd_impl(Q, K, V, dO, LSE, Delta, dQ, dK, dV, B, heads, Sq, Sk, ldq, ldk, ldv, lddo, lddq, lddk, lddv, key_mask, causal,
                         scale, seed, site, p_drop, math, io_bf16, hn_q, hn_kv, keep, stream);
}

// Backward in two passes through a caller-owned workspace (see attn_bwd_dkv3s_kernel): the same contract and fall-backs as
// kk_attn_bwd, which is what runs when ws is null / too small or the launch is not eligible for the two passes.
extern "C" int64_t kk_attn_bwd_ws_bytes(int B, int heads, int Sq, int Sk) {
    if (B <= 0 || heads <= 0 || Sq <= 0 || Sk <= 0) return 0;
    return (int64_t)B * heads * kk_cdiv(Sk, 32) * (kk_cdiv(Sq, 128) * 4) * 2048;
}
// Whether the two passes are the faster form for this shape (advice to the caller, who hands kk_attn_bwd_ws a workspace only then;
// the entry point itself takes the two passes whenever it gets an adequate workspace and the kernels serve the launch).  The dQ
// pass reads the dS tiles back from the Infinity Cache (~11 B/clk/CU with every CU streaming), 17 us of a 37-47 us launch at
// 8 x 8 x 512^2, so the two passes lose there; their best case is a long pair launch that is not lopsided, full attention at 1024^2,
// which they run in 128 us and the pair launch in 118 us.  So the advice is "never" (causal launches were the pair launch's already: its halves
// balance each other).  KK_ATTN_BWD_TWO_PASS=2 (tools): wherever the kernels serve the shape, 0: never.
static int attn_two_pass_mode() {
    static const int v = kk_tune_env("KK_ATTN_BWD_TWO_PASS", 1);
    return v;
}
extern "C" int kk_attn_bwd_two_pass(int B, int heads, int Sq, int Sk, int causal) {
    if (B <= 0 || heads <= 0 || Sq <= 64 || Sk <= 64 || Sk > 4096 || (causal && Sq != Sk)) return 0;
    return attn_two_pass_mode() == 2;
}

extern "C" int kk_attn_bwd_ws(const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Delta,
                              float *dQ, float *dK, float *dV, int B, int heads, int Sq, int Sk, int64_t ldq, int64_t ldk,
                              int64_t ldv, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, const uint8_t *key_mask,
                              int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop, int math, int io_bf16,
                              const KkAttnHeadNorm *hn_q, const KkAttnHeadNorm *hn_kv, void *ws, int64_t ws_bytes, void *stream) {
    KK_REQUIRE(Delta != nullptr, "kk_attn_bwd_ws: Delta is an input of this call");
    KK_REQUIRE((hn_q == nullptr) == (hn_kv == nullptr), "kk_attn_bwd_ws: head-norm epilogues for both kernels or for neither");
    const int two_pass = attn_two_pass_mode() != 0;             // (the shape policy is the caller's: kk_attn_bwd_two_pass)
    const int64_t per_head = (int64_t)kk_cdiv(Sk, 32) * (kk_cdiv(Sq, 128) * 4) * 2048;
    const bool ok = two_pass && ws && al16(ws) && ws_bytes >= kk_attn_bwd_ws_bytes(B, heads, Sq, Sk) && per_head < (1ll << 31) &&
                    dma_both(io_bf16, math, Sq, Sk, Q, K, V, dO, dQ, dK, dV, ldq, ldk, ldv, lddo, hn_q, hn_kv) &&
                    g_attn_groups == 2 && Sq > 64 && Sk > 64 && (!causal || Sq == Sk);
    if (!ok)
        return kk_attn_bwd(Q, K, V, dO, LSE, Delta, dQ, dK, dV, B, heads, Sq, Sk, ldq, ldk, ldv, lddo, lddq, lddk, lddv, key_mask, causal,
                           scale, seed, site, p_drop, math, io_bf16, hn_q, hn_kv, stream);
    KK_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "kk_attn_bwd_ws: dropout probability must be in [0,1)");
    const int64_t lds[7] = {ldq, ldk, ldv, lddo, lddq, lddk, lddv};
    if (int rc = check_common("kk_attn_bwd_ws", B, heads, Sq, Sk, math, lds, 7)) return rc;
    AttnArgs a = attn_args(Q, K, V, B, heads, Sq, Sk, ldq, ldk, ldv, key_mask, causal, scale, seed, site, p_drop);
    a.dO = dO; a.LSE = LSE; a.Delta = Delta; a.lddo = lddo; a.Out = dK; a.Out2 = dV; a.ldout = lddk; a.ldout2 = lddv;
    a.dS = ws;
    if (hn_q) {
        if (int rc = check_headnorm("kk_attn_bwd_ws", hn_q, 1)) return rc;
        if (int rc = check_headnorm("kk_attn_bwd_ws", hn_kv, 2)) return rc;
        a.hn[0] = hn_kv[0]; a.hn[1] = hn_kv[1];
    }
    if (int rc = launch_attn(attn_bwd_dkv3s_kernel, dim3(kk_cdiv(Sk, 128), B * heads), 1, (size_t)71680, (hipStream_t)stream, a)) return rc;
    KK_LAUNCH_CHECK("kk_attn_bwd_ws (dK, dV, dS)");
    a.Out = dQ; a.Out2 = nullptr; a.ldout = lddq; a.ldout2 = 0;
    a.hn[0] = KkAttnHeadNorm{}; a.hn[1] = KkAttnHeadNorm{};
    if (hn_q) a.hn[0] = hn_q[0];
    kk_note_kernel("attn_bwd_dkv3s+dqpass");
    if (int rc = launch_attn(attn_bwd_dqpass_kernel, dim3(kk_cdiv(Sq, 128), B * heads), 1, (size_t)3 * (8192 + 16384), (hipStream_t)stream, a))
        return rc;
    KK_LAUNCH_CHECK("kk_attn_bwd_ws (dQ pass)");
    return 0;
}
