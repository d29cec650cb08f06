// g16x_body: the large-tile family of the bf16-storage GEMM core (several accumulators per wave, optional loader waves).
// Kernels and entry points: kk_gemm16x.hip; kk_chain.hip runs the same body as a phase of its launch.
#pragma once
#include "kk_gemm16_dev.h"

namespace {

// EPI: 0 plain (bias, bf16 / fp32 C, optional Delta rows), 1 GLU backward on the linear2 dgrad, 2 GLU forward on linear1 (BN = the
// a-panel rows + the b-panel rows), 3 per-head RMSNorm (+ RoPE) on a q / k / v projection.  Same arithmetic, same bits as the
// epilogues of gemm16_body (kk_gemm16_body.h, which documents them).
template <bool TA, bool TB, int BM, int BN, int NS, int EPI, int WR, int WC, int LW>
__device__ __forceinline__ void g16x_body(const G16Args &a, const int wg, char *smem) {
    // WR x WC COMPUTE waves own the accumulators; LW LOADER waves (LW > 0) do nothing but issue the buffer-load-to-LDS DMA.
    // Why: a DMA instruction (1 KB per wave) costs its wave 70 - 140 clocks of issue when every wave of the CU issues its share
    // at the same point of the k-step (one address unit per CU), 350 - 700 clocks per k-step in which the wave's MFMAs wait behind
    // it (shader-clock stamps, tools/probes/g16x_trace.py: k-step 2100 clocks for 768 clocks of MFMA per SIMD; the DMA data had
    // always landed already).  With loader waves a SIMD holds one compute wave that never touches the address unit and one
    // loader wave that blocks there harmlessly.
    constexpr int CWV = WR * WC, WAVES = CWV + LW, NT = 64 * WAVES, LT = LW > 0 ? 64 * LW : NT;
    constexpr int BNH = EPI == 2 ? BN / 2 : BN;                 // output columns per workgroup (of ONE panel when EPI == 2)
    constexpr int MI = BM / (32 * WR);
    constexpr int NW = BNH / WC, NJ = NW / 32;                  // columns / 32-column blocks per wave (per panel)
    constexpr int NI = EPI == 2 ? 2 * NJ : NJ;
    static_assert(BM % (32 * WR) == 0 && BNH % (32 * WC) == 0, "whole 32x32 accumulators per wave");
    using OA = Operand<BM, TA, LT, BM, KK_A_AUX>;
    using OB = Operand<BN, TB, LT, BNH>;
    constexpr int STAGE = OA::BYTES + OB::BYTES;
    constexpr int NPT = OA::NP + OB::NP;

    // workgroup -> tile (same XCD-aware order as gemm16_body: an XCD sweeps a contiguous run of tiles)
    int tid_lin = wg;
    {   // (g16_xcd_tile written out: through the function, two tools-only kernels of this body come out with other code — docs/LAB_NOTES.md)
        const int ntiles = a.tiles_m * a.tiles_n;
        if (a.xcd_swizzle) {
            const int q = ntiles >> 3, r = ntiles & 7, xcd = tid_lin & 7, in = tid_lin >> 3;
            tid_lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + in;
        }
    }
    const int m0 = (a.m_fast ? tid_lin % a.tiles_m : tid_lin / a.tiles_n) * BM;
    const int n0 = (a.m_fast ? tid_lin / a.tiles_m : tid_lin % a.tiles_n) * BNH;
    const int nk = (a.K + BK - 1) / BK;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool loader = LW > 0 && wave >= CWV;
    const int wr = wave / WC, wc = wave % WC, half = lane >> 5, l31 = lane & 31;

    // probe (tools builds): shader-clock stamps of workgroup 0's waves, 4 per k-step, into the buffer at a.dl_out
    unsigned long long *trace = (KK_DBG(a, 32) && wg == 0 && lane == 0) ? reinterpret_cast<unsigned long long *>(a.dl_out) + wave * 64 : nullptr;
    auto stamp = [&](int kt, int which) {
        if (KK_DBG(a, 32) && trace != nullptr && kt < 16) trace[kt * 4 + which] = __builtin_amdgcn_s_memtime();
    };

    // the tile's bias row, read by phase A of the epilogues (24 dependent global loads there cost 3 us)
    float *bias_lds = reinterpret_cast<float *>(smem + NS * STAGE);
    if (EPI != 1 && !loader && threadIdx.x < BN) {
        const int tc = threadIdx.x, gc = (EPI == 2 && tc >= BNH) ? a.N + n0 + tc - BNH : n0 + tc;
        const int lim = EPI == 2 ? 2 * a.N : a.N;
        bias_lds[tc] = (a.bias != nullptr && gc < lim && (EPI != 2 || (tc < BNH ? gc < a.N : true))) ? a.bias[gc] : 0.f;
    }

    f32x16 acc[MI][NI];
    if (LW > 0 && loader) {
        // ---- loader waves: tile kt + NS - 1 goes out right behind the barrier that frees its stage
        OA oa;
        OB ob;
        const int lt = threadIdx.x - 64 * CWV, lw = wave - CWV;
        oa.init(a.A, a.a_bytes, a.lda, m0, m0, lt);
        ob.init(a.B, a.b_bytes, a.ldb, n0, EPI == 2 ? a.N + n0 : n0, lt);
#pragma unroll
        for (int p = 0; p < NS - 1; ++p)
            if (p < nk) {
                oa.issue(smem + p * STAGE, p, lw);
                ob.issue(smem + p * STAGE + OA::BYTES, p, lw);
            }
        int sn = NS - 1;
        for (int kt = 0; kt < nk; ++kt) {
            stamp(kt, 0);
            g16_wait_tile<NS, NPT>(min(nk - 1 - kt, NS - 2));
            stamp(kt, 1);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            stamp(kt, 2);
            if (kt + NS - 1 < nk) {
                oa.issue(smem + sn * STAGE, kt + NS - 1, lw);
                ob.issue(smem + sn * STAGE + OA::BYTES, kt + NS - 1, lw);
            }
            stamp(kt, 3);
            sn = sn + 1 == NS ? 0 : sn + 1;
        }
        stamp(min(nk, 15), 0);
    } else {
    OA oa;
    OB ob;
    if constexpr (LW == 0) {
        oa.init(a.A, a.a_bytes, a.lda, m0, m0, threadIdx.x);
        ob.init(a.B, a.b_bytes, a.ldb, n0, EPI == 2 ? a.N + n0 : n0, threadIdx.x);
    }
    int ablk[MI], bblk[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) ablk[i] = wr * MI + i;
#pragma unroll
    for (int j = 0; j < NI; ++j) bblk[j] = (EPI == 2 && j >= NJ) ? BNH / 32 + wc * NJ + (j - NJ) : wc * NJ + j;
    FragAddr<BM, TA, MI> fa;
    FragAddr<BN, TB, NI> fb;
    fa.init(lane, ablk);
    fb.init(lane, bblk);

#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if constexpr (LW == 0) {
#pragma unroll
        for (int p = 0; p < NS - 1; ++p)
            if (p < nk) {
                oa.issue(smem + p * STAGE, p, wave);
                ob.issue(smem + p * STAGE + OA::BYTES, p, wave);
            }
    }
    int sc = 0, sn = NS - 1;
    for (int kt = 0; kt < nk; ++kt) {
        stamp(kt, 0);
        if constexpr (LW == 0) g16_wait_tile<NS, NPT>(min(nk - 1 - kt, NS - 2));
        stamp(kt, 1);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        stamp(kt, 2);
        if constexpr (LW == 0) {
            if (kt + NS - 1 < nk) {
                oa.issue(smem + sn * STAGE, kt + NS - 1, wave);
                ob.issue(smem + sn * STAGE + OA::BYTES, kt + NS - 1, wave);
            }
        }
        stamp(kt, 3);
        const char *Ai = smem + sc * STAGE, *Bi = Ai + OA::BYTES;
        sn = sc;
        sc = sc + 1 == NS ? 0 : sc + 1;
        constexpr int RPS = MI * FragAddr<BM, TA, MI>::READS + NI * FragAddr<BN, TB, NI>::READS;
        static_assert(RPS <= 15, "a slab's reads must fit the lgkmcnt counter");
        constexpr int AHEAD = 3 * RPS <= 15 ? 2 : 1;            // slabs whose reads are in flight under the MFMAs of the current one
        Frag af[4][MI], bf[4][NI];
        auto read_slab = [&](int ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa.load(af[ks][i], Ai, i, ks);
#pragma unroll
            for (int j = 0; j < NI; ++j) fb.load(bf[ks][j], Bi, j, ks);
        };
        if (KK_DBG(a, 8)) continue;                             // probe: DMA + barriers only
#pragma unroll
        for (int ks = 0; ks < AHEAD; ++ks) read_slab(ks);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + AHEAD < 4) read_slab(ks + AHEAD);
            if (ks + AHEAD < 4) wait_reads<AHEAD * RPS>();
            else if (AHEAD == 2 && ks == 2) wait_reads<RPS>();
            else wait_reads<0>();
#pragma unroll
            for (int i = 0; i < MI; ++i) pin_frag(af[ks][i], TA);
#pragma unroll
            for (int j = 0; j < NI; ++j) pin_frag(bf[ks][j], TB);
            if (!KK_DBG(a, 4)) {                                // (probe: no MFMAs)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_value(bf[ks][j], TB), frag_value(af[ks][i], TA), acc[i][j], 0, 0, 0);      // (operands swapped: the block's transpose)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    stamp(min(nk, 15), 0);
    }
    if (nk <= 0) return;
    if (KK_DBG(a, 1)) {                                         // probe: no epilogue (one store keeps the accumulators alive)
        float t = 0.f;
        if (!loader) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) t += acc[i][j][r];
        }
        if (t == 1.2345f) static_cast<float *>(a.C)[0] = t;
        return;
    }

    // ---- epilogues.  The accumulators are TRANSPOSED blocks (the MFMAs run with their operands swapped): lane (l31, half) holds,
    // for row l31 of block (i, j), the columns 4 * half + 8 * g + e (g, e < 4) — four consecutive columns per register quad.  Phase A
    // (compute waves): the workgroup's tile goes to LDS with 8- / 16-byte stores.  Phase B (EVERY wave, loaders included): 32 x 32
    // blocks (32 x 64 for the plain epilogue: a head per block pair) are dealt out round robin; a lane works on 8 consecutive
    // columns of 2 rows with 16-byte global accesses, as the epilogues of gemm16_body do: same arithmetic, same bits.
    constexpr int TPF = BN + 4;                                 // floats per row of the fp32 tile (16-byte rows, 4-bank skew)
    constexpr int TPH = BN + 8;                                 // bf16 per row of the bf16 tile
    auto blockcol = [&](int j) { return (EPI == 2 && j >= NJ) ? BNH + wc * NW + (j - NJ) * 32 : wc * NW + j * 32; };      // tile-local first column of block j
    const int c8 = (lane & 3) * 8;
    __builtin_amdgcn_s_barrier();                               // every wave is done with the last stage
    stamp(9, 0);

    if constexpr (EPI == 1) {
        static_assert(EPI != 1 || NS * STAGE >= BM * TPF * 4, "the staging area holds the fp32 tile");
        const int F = a.N;
        const uint32_t thr = a.glu_seed ? kk_drop_threshold(a.glu_p) : 0u, seed = thr ? *a.glu_seed : 0u;
        const float ik = thr ? 1.f / (1.f - a.glu_p) : 1.f;
        float *tile = reinterpret_cast<float *>(smem);
        if (!loader) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        st4(tile + ((wr * MI + i) * 32 + l31) * TPF + blockcol(j) + 4 * half + 8 * g,
                            make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]));
        }
        stamp(9, 1);
        __syncthreads();
        stamp(9, 2);
        constexpr int NBR = BM / 32, NBC = BN / 32;
#pragma unroll 1
        for (int blk = wave; blk < NBR * NBC; blk += WAVES) {
            const int bi = blk / NBC, bj = blk % NBC;
            const int col = n0 + bj * 32 + c8;
            float sa[8], sb[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) sa[e] = sb[e] = 0.f;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int rl = it * 16 + (lane >> 2), row = m0 + bi * 32 + rl;
                if (row < a.M && col < F) {
                    const float *tp = tile + (bi * 32 + rl) * TPF + bj * 32 + c8;
                    const float4 d0 = ld4(tp), d1 = ld4(tp + 4);
                    const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
                    const int64_t o = (int64_t)row * 2 * F + col;
                    const bf16x8 av = *reinterpret_cast<const bf16x8 *>(a.glu_h + o), bv = *reinterpret_cast<const bf16x8 *>(a.glu_h + o + F);
                    float mk[8];
                    kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col, thr, ik, *reinterpret_cast<float(*)[4]>(mk));
                    kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col + 4, thr, ik, *reinterpret_cast<float(*)[4]>(mk + 4));
                    bf16x8 oa_, ob_;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float gv, gd;
                        kk_gelu_pair_fast((float)av[e], gv, gd);
                        const float dd = d[e] * mk[e];
                        const float da = dd * (float)bv[e] * gd, db = dd * gv;
                        oa_[e] = (__bf16)da;
                        ob_[e] = (__bf16)db;
                        sa[e] += da;
                        sb[e] += db;
                    }
                    kk_store16(a.glu_dh + o, __builtin_bit_cast(kk_u32x4, oa_), a.wt);
                    kk_store16(a.glu_dh + o + F, __builtin_bit_cast(kk_u32x4, ob_), a.wt);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                {   // lanes 4 and 8 away inside the 16-lane row by DPP rotations (only lanes 0..3 are read below: for them the same additions as
                // the xor butterfly), the rows 16 and 32 away by ds_bpermute
                sa[e] += kk_dpp<0x124>(sa[e]); sb[e] += kk_dpp<0x124>(sb[e]);
                sa[e] += kk_dpp<0x128>(sa[e]); sb[e] += kk_dpp<0x128>(sb[e]);
                sa[e] += __shfl_xor(sa[e], 16, 64); sb[e] += __shfl_xor(sb[e], 16, 64);
                sa[e] += __shfl_xor(sa[e], 32, 64); sb[e] += __shfl_xor(sb[e], 32, 64);
            }
            }
            const int prow = m0 / 32 + bi;                      // one partial row per 32 rows of dY (kk_gemm_dgrad_glu_blocks)
            if (lane < 4 && col < F && prow < 2 * ((a.M + 63) / 64)) {
                float *pr = a.glu_partials + (int64_t)prow * 2 * F;
                st4(pr + col, make_float4(sa[0], sa[1], sa[2], sa[3]));
                st4(pr + col + 4, make_float4(sa[4], sa[5], sa[6], sa[7]));
                st4(pr + F + col, make_float4(sb[0], sb[1], sb[2], sb[3]));
                st4(pr + F + col + 4, make_float4(sb[4], sb[5], sb[6], sb[7]));
            }
        }
        stamp(14, 0);
        if (KK_DBG(a, 32)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(14, 1); }
        return;
    }
    if constexpr (EPI == 2) {
        // (a | b) + bias, ROUNDED to bf16 — what h1 stores and the gate reads — is what the tile holds: [BM][a columns | b columns]
        static_assert(EPI != 2 || NS * STAGE >= BM * TPH * 2, "the staging area holds the bf16 tile");
        const int F = a.N;
        const uint32_t thr = a.glu_seed ? kk_drop_threshold(a.glu_p) : 0u, seed = thr ? *a.glu_seed : 0u;
        const float ik = thr ? 1.f / (1.f - a.glu_p) : 1.f;
        __bf16 *tile = reinterpret_cast<__bf16 *>(smem);
        if (!loader) {
#pragma unroll
            for (int j = 0; j < NI; ++j) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bq = ld4(bias_lds + blockcol(j) + 4 * half + 8 * g);
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        bf16x4 o;
                        o[0] = (__bf16)(acc[i][j][4 * g] + bq.x); o[1] = (__bf16)(acc[i][j][4 * g + 1] + bq.y);
                        o[2] = (__bf16)(acc[i][j][4 * g + 2] + bq.z); o[3] = (__bf16)(acc[i][j][4 * g + 3] + bq.w);
                        *reinterpret_cast<bf16x4 *>(tile + ((wr * MI + i) * 32 + l31) * TPH + blockcol(j) + 4 * half + 8 * g) = o;
                    }
                }
            }
        }
        stamp(9, 1);
        __syncthreads();
        stamp(9, 2);
        __bf16 *h = a.glu_dh, *gout = static_cast<__bf16 *>(a.C);
        constexpr int NBR = BM / 32, NBC = BNH / 32;
#pragma unroll 1
        for (int blk = wave; blk < NBR * NBC; blk += WAVES) {
            const int bi = blk / NBC, bj = blk % NBC;
            const int col = n0 + bj * 32 + c8;
            if (col >= F) continue;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int rl = it * 16 + (lane >> 2), row = m0 + bi * 32 + rl;
                if (row >= a.M) continue;
                const __bf16 *tp = tile + (bi * 32 + rl) * TPH + bj * 32 + c8;
                const bf16x8 oa_ = *reinterpret_cast<const bf16x8 *>(tp), ob_ = *reinterpret_cast<const bf16x8 *>(tp + BNH);
                float mk[8];
                kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col, thr, ik, *reinterpret_cast<float(*)[4]>(mk));
                kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col + 4, thr, ik, *reinterpret_cast<float(*)[4]>(mk + 4));
                bf16x8 og;
#pragma unroll
                for (int e = 0; e < 8; ++e) og[e] = (__bf16)(kk_gelu_fast((float)oa_[e]) * (float)ob_[e] * mk[e]);
                const int64_t o = (int64_t)row * 2 * F + col;
                kk_store16(h + o, __builtin_bit_cast(kk_u32x4, oa_), a.wt);
                kk_store16(h + o + F, __builtin_bit_cast(kk_u32x4, ob_), a.wt);
                kk_store16(gout + (int64_t)row * a.ldc + col, __builtin_bit_cast(kk_u32x4, og), a.wt);
            }
        }
        stamp(14, 0);
        if (KK_DBG(a, 32)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(14, 1); }
        return;
    }
    if constexpr (EPI == 3) {
        static_assert(EPI != 3 || BN % 64 == 0, "whole heads per workgroup tile");
        static_assert(EPI != 3 || NS * STAGE >= BM * TPH * 2, "the staging area holds the bf16 tile");
        constexpr int PITCH = TPH;
        __bf16 *tile = reinterpret_cast<__bf16 *>(smem);
        if (!loader) {
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int tc = blockcol(j) + 4 * half + 8 * g;
                    const float4 bq = ld4(bias_lds + tc);
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        bf16x4 o;
                        o[0] = (__bf16)(acc[i][j][4 * g] + bq.x); o[1] = (__bf16)(acc[i][j][4 * g + 1] + bq.y);
                        o[2] = (__bf16)(acc[i][j][4 * g + 2] + bq.z); o[3] = (__bf16)(acc[i][j][4 * g + 3] + bq.w);
                        *reinterpret_cast<bf16x4 *>(tile + ((wr * MI + i) * 32 + l31) * PITCH + tc) = o;
                    }
                }
        }
        stamp(9, 1);
        __syncthreads();
        stamp(9, 2);
        // Eight lanes per (row, head) vector, 8 consecutive columns (16 bytes) each: 16-byte LDS reads and 16-byte global stores (8-byte
        // write-through stores cost 2.7x per byte).  A head's column block is walked row by row, so the part, its gain and the RoPE
        // flag are uniform over a pass; rotate-half's partner columns (d +- 32) are a second 16-byte read of the tile, normalised
        // with the same rs: no cross-lane traffic but the three steps of the sum of squares.  Same arithmetic in the same order
        // as kk_headnorm_rope (16 lanes x 4 columns): the two give the same bits.
        __bf16 *raw = static_cast<__bf16 *>(a.C);
        constexpr int ET = BM % (NT / 8) == 0 ? NT : 64 * CWV;   // threads of the second phase (all of them when that gives whole passes)
        constexpr int HPR = BN / 64, GROUPS = ET / 8, PPH = BM / GROUPS;
        static_assert(BM % GROUPS == 0, "whole passes per head column block");
        if (ET < NT && threadIdx.x >= ET) return;
        const int u = threadIdx.x & 7, gidx = threadIdx.x >> 3, pu = u ^ 4;
        const int pos0 = m0 % a.hn_S;
#pragma unroll 1
        for (int hl = 0; hl < HPR; ++hl) {
            const int hc = n0 + hl * 64;
            if (hc >= a.N) break;
            stamp(10 + hl, 0);
            const int part = hc / a.hn_H;
            const bool rope = (a.hn_rope_mask >> part) & 1;
            const float *gp = a.hn_gain[part];
            const float4 g0 = ld4(gp + 8 * u), g1 = ld4(gp + 8 * u + 4);
            float4 q0 = g0, q1 = g1;
            if (rope) { q0 = ld4(gp + 8 * pu); q1 = ld4(gp + 8 * pu + 4); }
#pragma unroll
            for (int ps = 0; ps < PPH; ++ps) {
                const int rl = ps * GROUPS + gidx, row = m0 + rl;
                const bf16x8 r8 = *reinterpret_cast<const bf16x8 *>(tile + rl * PITCH + hl * 64 + 8 * u);
                const float4 va = make_float4((float)r8[0], (float)r8[1], (float)r8[2], (float)r8[3]);
                const float4 vb = make_float4((float)r8[4], (float)r8[5], (float)r8[6], (float)r8[7]);
                float ss = (va.x * va.x + va.y * va.y + va.z * va.z + va.w * va.w) + (vb.x * vb.x + vb.y * vb.y + vb.z * vb.z + vb.w * vb.w);
                ss += kk_dpp<0xB1>(ss); ss += kk_dpp<0x4E>(ss); ss += kk_dpp<0x141>(ss);       // (lanes 1, 2, 4 away: DPP, kk_common.h)
                const float rs = 1.f / sqrtf(ss * (1.f / 64.f) + 1.1920928955078125e-7f);
                float4 na = make_float4(va.x * rs * g0.x, va.y * rs * g0.y, va.z * rs * g0.z, va.w * rs * g0.w);
                float4 nb = make_float4(vb.x * rs * g1.x, vb.y * rs * g1.y, vb.z * rs * g1.z, vb.w * rs * g1.w);
                if (rope) {
                    int pos = pos0 + rl;
                    if (row >= a.M) pos = (a.M - 1) % a.hn_S;
                    else if (pos >= a.hn_S) pos %= a.hn_S;
                    const bf16x8 p8 = *reinterpret_cast<const bf16x8 *>(tile + rl * PITCH + hl * 64 + 8 * pu);
                    const float4 oa = make_float4((float)p8[0] * rs * q0.x, (float)p8[1] * rs * q0.y, (float)p8[2] * rs * q0.z, (float)p8[3] * rs * q0.w);
                    const float4 ob_ = make_float4((float)p8[4] * rs * q1.x, (float)p8[5] * rs * q1.y, (float)p8[6] * rs * q1.z, (float)p8[7] * rs * q1.w);
                    const float *cr = a.hn_cos + pos * 64 + 8 * u, *sr = a.hn_sin + pos * 64 + 8 * u;
                    const float4 c0 = ld4(cr), c1 = ld4(cr + 4), s0 = ld4(sr), s1 = ld4(sr + 4);
                    const float sg = u < 4 ? -1.f : 1.f;
                    na = make_float4(na.x * c0.x + sg * oa.x * s0.x, na.y * c0.y + sg * oa.y * s0.y, na.z * c0.z + sg * oa.z * s0.z, na.w * c0.w + sg * oa.w * s0.w);
                    nb = make_float4(nb.x * c1.x + sg * ob_.x * s1.x, nb.y * c1.y + sg * ob_.y * s1.y, nb.z * c1.z + sg * ob_.z * s1.z, nb.w * c1.w + sg * ob_.w * s1.w);
                }
                if (row < a.M) {
                    if (!KK_DBG(a, 64 | 128)) kk_store16(raw + (int64_t)row * a.ldc + hc + 8 * u, __builtin_bit_cast(kk_u32x4, r8), a.wt);      // (probe 128: the raw projection alone is not stored — the price of writing two tensors)
                    bf16x8 n8;
                    n8[0] = (__bf16)na.x; n8[1] = (__bf16)na.y; n8[2] = (__bf16)na.z; n8[3] = (__bf16)na.w;
                    n8[4] = (__bf16)nb.x; n8[5] = (__bf16)nb.y; n8[6] = (__bf16)nb.z; n8[7] = (__bf16)nb.w;
                    if (!KK_DBG(a, 64)) kk_store16(a.hn_y + (int64_t)row * a.hn_ldy + hc + 8 * u, __builtin_bit_cast(kk_u32x4, n8), a.wt);
                }
            }
        }
        stamp(14, 0);
        if (KK_DBG(a, 32)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(14, 1); }
        return;
    }
    // ---- EPI == 0
    constexpr int NBR0 = BM / 32, NBP = BN / 64;                // phase-B items: 32 rows x 64 columns (a head of the Delta epilogue)
    if (a.c_bf16 && a.residual == nullptr && (a.ldc & 7) == 0 && (a.N & 7) == 0 && (reinterpret_cast<uintptr_t>(a.C) & 15) == 0) {
        // bf16 C: the tile holds alpha * acc + bias, rounded
        __bf16 *tile = reinterpret_cast<__bf16 *>(smem);
        __bf16 *C = static_cast<__bf16 *>(a.C);
        if (!loader) {
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int tc = blockcol(j) + 4 * half + 8 * g;
                    const float4 bq = ld4(bias_lds + tc);
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        bf16x4 o;
                        o[0] = (__bf16)(a.alpha * acc[i][j][4 * g] + bq.x); o[1] = (__bf16)(a.alpha * acc[i][j][4 * g + 1] + bq.y);
                        o[2] = (__bf16)(a.alpha * acc[i][j][4 * g + 2] + bq.z); o[3] = (__bf16)(a.alpha * acc[i][j][4 * g + 3] + bq.w);
                        *reinterpret_cast<bf16x4 *>(tile + ((wr * MI + i) * 32 + l31) * TPH + tc) = o;
                    }
                }
        }
        __syncthreads();
#pragma unroll 1
        for (int blk = wave; blk < NBR0 * NBP; blk += WAVES) {
            const int bi = blk / NBP, bp = blk % NBP;
            float dsum[2] = {0.f, 0.f};
#pragma unroll
            for (int hj = 0; hj < 2; ++hj) {
                const int col = n0 + bp * 64 + hj * 32 + c8;
                if (col >= a.N) continue;
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int rl = it * 16 + (lane >> 2), row = m0 + bi * 32 + rl;
                    if (row >= a.M) continue;
                    const bf16x8 o = *reinterpret_cast<const bf16x8 *>(tile + (bi * 32 + rl) * TPH + bp * 64 + hj * 32 + c8);
                    kk_store16(C + (int64_t)row * a.ldc + col, __builtin_bit_cast(kk_u32x4, o), a.wt);
                    if (a.dl_out != nullptr) dsum[it] = g16_delta_dot(dsum[it], o, a.dl_o + (int64_t)row * a.dl_ldo + col);      // Delta rows
                }
            }
            if (a.dl_out != nullptr) {                          // the 4 lanes sharing lane >> 2 hold a row's 64 columns of this head
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    float t = dsum[it];
                    t += __shfl_xor(t, 1, 64);
                    t += __shfl_xor(t, 2, 64);
                    const int rl = it * 16 + (lane >> 2), row = m0 + bi * 32 + rl;
                    if ((lane & 3) == 0 && row < a.M && n0 + bp * 64 < a.N) {
                        const int bb = row / a.dl_S, q = row - bb * a.dl_S;
                        a.dl_out[((int64_t)bb * a.dl_heads + (n0 + bp * 64) / 64) * a.dl_S + q] = t;
                    }
                }
            }
        }
        return;
    }
    if (a.wt && !a.c_bf16 && !a.atomic && a.residual == nullptr && (a.ldc & 3) == 0 && (a.N & 7) == 0 &&
        (reinterpret_cast<uintptr_t>(a.C) & 15) == 0 && NS * STAGE >= BM * TPF * 4) {
        // fp32 C written (or accumulated into) exactly once per element — the weight gradients — as 16-byte write-through stores
        float *tile = reinterpret_cast<float *>(smem);
        float *C = static_cast<float *>(a.C);
        if (!loader) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        st4(tile + ((wr * MI + i) * 32 + l31) * TPF + blockcol(j) + 4 * half + 8 * g,
                            make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]));
        }
        __syncthreads();
        float ssq = 0.f;                                         // (ss_rec: this lane's share of the tile's sum of squares)
#pragma unroll 1
        for (int blk = wave; blk < NBR0 * (BN / 32); blk += WAVES) {
            const int bi = blk / (BN / 32), bj = blk % (BN / 32);
            const int col = n0 + bj * 32 + c8;
            if (col >= a.N) continue;
            float bv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) bv[e] = a.bias != nullptr ? a.bias[col + e] : 0.f;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int rl = it * 16 + (lane >> 2), row = m0 + bi * 32 + rl;
                if (row >= a.M) continue;
                float *dst = C + (int64_t)row * a.ldc + col;
                const float *tp = tile + (bi * 32 + rl) * TPF + bj * 32 + c8;
                const float4 v0 = ld4(tp), v1 = ld4(tp + 4);
                float4 o0 = make_float4(a.alpha * v0.x + bv[0], a.alpha * v0.y + bv[1], a.alpha * v0.z + bv[2], a.alpha * v0.w + bv[3]);
                float4 o1 = make_float4(a.alpha * v1.x + bv[4], a.alpha * v1.y + bv[5], a.alpha * v1.z + bv[6], a.alpha * v1.w + bv[7]);
                if (a.beta != 0.f) {
                    const float4 d0 = ld4(dst), d1 = ld4(dst + 4);
                    o0 = make_float4(o0.x + a.beta * d0.x, o0.y + a.beta * d0.y, o0.z + a.beta * d0.z, o0.w + a.beta * d0.w);
                    o1 = make_float4(o1.x + a.beta * d1.x, o1.y + a.beta * d1.y, o1.z + a.beta * d1.z, o1.w + a.beta * d1.w);
                }
                kk_st16_wt(dst, __builtin_bit_cast(kk_u32x4, o0));
                kk_st16_wt(dst + 4, __builtin_bit_cast(kk_u32x4, o1));
                ssq += (o0.x * o0.x + o0.y * o0.y) + (o0.z * o0.z + o0.w * o0.w) + (o1.x * o1.x + o1.y * o1.y) + (o1.z * o1.z + o1.w * o1.w);
            }
        }
        if constexpr (NS * STAGE >= BM * TPF * 4 + 8 * (WR * WC + LW)) {      // (room for the wave sums behind the fp32 tile)
        if (a.ss_rec != nullptr) {                              // (workgroup-uniform) wave sums in wave order: the same bits whatever the schedule
            double *wsum = reinterpret_cast<double *>(smem + BM * TPF * 4);
            const double wv = wave_sum_d((double)ssq);
            if (lane == 0) wsum[wave] = wv;
            __syncthreads();
            if (threadIdx.x == 0) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) t += wsum[w];
                a.ss_rec[wg] = KkSegRec{t, a.ss_seg + (a.ss_rows > 0 ? m0 / a.ss_rows : 0), 0};
            }
        }
        }
        return;
    }
    // general form (residual, unaligned C, accumulation without write-through): straight from the registers, 4 columns at a time
    if (loader) return;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int row = m0 + (wr * MI + i) * 32 + l31;
            if (row >= a.M) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = n0 + blockcol(j) + 4 * half + 8 * (r >> 2) + (r & 3);
                if (col >= a.N) continue;
                float v = a.alpha * acc[i][j][r] + (a.bias != nullptr ? a.bias[col] : 0.f);
                if (a.residual != nullptr) {
                    const int64_t rr = a.res_mod > 0 ? (int64_t)row % a.res_mod : (int64_t)row;
                    v += a.residual[rr * a.ldr + col];
                }
                if (a.c_bf16) {
                    static_cast<__bf16 *>(a.C)[(int64_t)row * a.ldc + col] = (__bf16)v;
                    continue;
                }
                float *dst = static_cast<float *>(a.C) + (int64_t)row * a.ldc + col;
                if (a.beta != 0.f) v += a.beta * (*dst);
                *dst = v;
            }
        }
}

}  // namespace
