// gemm16_body: the 64x64 / 128x64 tile family of the bf16-storage GEMM core (one 32x32 accumulator per wave, every wave loads
// and computes).  Kernels and entry points: kk_gemm16.hip; kk_chain.hip runs the same body as a phase of its launch.
#pragma once
#include "kk_gemm16_dev.h"

namespace {

// NS LDS stages: NS-1 k-tiles are in flight while one is multiplied.  The DMA of a tile is waited for with a COUNTED
// vmcnt (the younger tiles stay in flight across the barrier), and the barrier is a raw s_barrier: __syncthreads()
// would drain vmcnt(0) because an LDS-DMA is a pending LDS write.
// EPI = 1: the GEMM is dG = dY.W2 of a GLU feed-forward (N = F columns) and the epilogue is the gate's backward
// (transformers.py:107-108): with h1 = [a | b] saved by the forward and m the gate's dropout mask,
//   dh1[:, c] = dG*m * b * gelu'(a),   dh1[:, F + c] = dG*m * gelu(a)
// are written directly (dG never exists in HBM), and the column sums of dh1 — linear1's bias gradient — leave the
// workgroup as plain rows partials[2*tile_m + wave_row][2F] for kk_partials_reduce.  Replaces kk_glu_bwd + kk_colsum_acc.
// EPI = 3: the GEMM is a q / k / v projection whose heads are 64 wide, so a 64x64 tile holds whole (row, head) vectors:
// the epilogue writes the projection (saved for the backward) AND its per-head RMSNorm (+ RoPE) — the attention's
// operands — through an LDS transpose of the tile.  Replaces kk_headnorm_rope_fwd (same math, same bits).
// EPI = 2: the GEMM is h1 = x.W1^T + b1 of a GLU feed-forward; a workgroup owns output columns [n0, n0+64) AND
// [F+n0, F+n0+64) (two B panels, two accumulators, the A tile is read from LDS once for both), so its epilogue writes
// h1 = [a | b] (saved for the backward) and the gated product g = gelu(a)*b*mask in one go.  Replaces kk_glu_fwd.
template <bool TA, bool TB, int BM, int BN, int NS, int EPI, int WAVES = 4, int WC = 2>
__device__ __forceinline__ void gemm16_body(const G16Args &a, const int wg, char *smem) {
    constexpr int WR = WAVES / WC;                              // waves along M x waves along N
    constexpr int MI = BM / (32 * WR), NI = BN / (32 * WC);     // 32x32 MFMA tiles per wave (wave tile = BM/WR x BN/WC)
    static_assert(EPI == 0 || WAVES == 4 || (WAVES == 8 && BM == 128 && BN == 64),
                  "the epilogue variants are written for four waves and for the eight-wave 128x64 tile");
    using OA = Operand1<BM, TA, 64 * WAVES, KK_A_AUX>;
    using OB = Operand1<BN, TB, 64 * WAVES>;
    constexpr int NB = EPI == 2 ? 2 : 1;                        // EPI == 2 multiplies A with TWO 64-row panels of B (see below)
    constexpr int STAGE = OA::BYTES + NB * OB::BYTES;
    constexpr int NPT = OA::NP + NB * OB::NP;                   // DMA instructions per thread per k-tile

    // Workgroup -> (tile, k-slice).  The dispatcher places workgroup i on XCD i % 8 (private 4 MiB L2 each).
    //  tile-major (default): every XCD sweeps a contiguous run of tiles (n fastest), all k-slices of a tile together;
    //  split-major (option, split-K with a multiple of 8 slices): slice = i % splits, so XCD x owns the k-slices
    //    = x (mod 8) of every tile and reads its part of A and B from HBM exactly once.  It cuts FETCH_SIZE of the
    //    512x512x4096 weight gradients 4.5x, yet the train step is 2 % SLOWER with it (566K vs 579K frames/s): these
    //    launches are latency-bound, not HBM-bound, and a tile's atomics then come from eight XCDs.  Left off.
    int tid_lin, ksl;
    if (a.split_major) {
        ksl = wg % a.splits;
        tid_lin = wg / a.splits;
    } else {
        const int ntiles = a.tiles_m * a.tiles_n;
        tid_lin = wg % ntiles;
        ksl = wg / ntiles;
        if (a.xcd_swizzle) tid_lin = g16_xcd_tile(tid_lin, ntiles);
    }
    // An XCD's contiguous run of tiles covers a few rows of the tile grid in the FAST direction completely: it streams the whole
    // operand of that direction through its private L2 (all eight L2s do) and a slice of the other one.  n fastest: B re-read 8x,
    // A once; m fastest: the other way round.  The grouped weight gradients pick the direction that replicates the SMALLER
    // operand (linear2's dW is 512 x 1536: m fastest re-reads dY 8x = 32 MB instead of the gated activations 8x = 100 MB).
    const int m0 = (a.m_fast ? tid_lin % a.tiles_m : tid_lin / a.tiles_n) * BM;
    const int n0 = (a.m_fast ? tid_lin / a.tiles_m : tid_lin % a.tiles_n) * BN;
    const int kbeg = ksl * a.k_per_split;
    const int kend = min(a.K, kbeg + a.k_per_split);
    const int nk = (kend - kbeg + BK - 1) / BK, kt0 = kbeg / BK;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave / WC, wc = wave % WC, half = lane >> 5, l31 = lane & 31;

    OA oa;
    OB ob, ob2;
    oa.init(a.A, a.a_bytes, a.lda, m0);
    ob.init(a.B, a.b_bytes, a.ldb, n0);
    if constexpr (EPI == 2) ob2.init(a.B, a.b_bytes, a.ldb, n0 + a.N);
    FragAddr1<BM, TA> fa;
    FragAddr1<BN, TB> fb;
    fa.init(lane, wr * (BM / WR));
    fb.init(lane, wc * (BN / WC));

    f32x16 acc[MI][NI];
    f32x16 acc2;                                                // EPI == 2: the second B panel's accumulator (MI = NI = 1)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.f;

#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nk) {
            oa.issue(smem + p * STAGE, kt0 + p, wave);
            ob.issue(smem + p * STAGE + OA::BYTES, kt0 + p, wave);
            if constexpr (EPI == 2) ob2.issue(smem + p * STAGE + OA::BYTES + OB::BYTES, kt0 + p, wave);
        }
    int sc = 0, sn = NS - 1;                                    // stage being multiplied / stage being refilled
    for (int kt = 0; kt < nk; ++kt) {
        // this wave's pieces of tile kt have landed once at most the younger tiles' DMAs are outstanding
        g16_wait_tile<NS, NPT>(min(nk - 1 - kt, NS - 2));
        __builtin_amdgcn_s_barrier();                           // everyone's pieces landed; everyone finished reading stage sn
        asm volatile("" ::: "memory");
        if (kt + NS - 1 < nk) {
            oa.issue(smem + sn * STAGE, kt0 + kt + NS - 1, wave);
            ob.issue(smem + sn * STAGE + OA::BYTES, kt0 + kt + NS - 1, wave);
            if constexpr (EPI == 2) ob2.issue(smem + sn * STAGE + OA::BYTES + OB::BYTES, kt0 + kt + NS - 1, wave);
        }
        const char *cur = smem + sc * STAGE;
        sn = sc;
        sc = sc + 1 == NS ? 0 : sc + 1;
        const char *Ai = cur, *Bi = cur + OA::BYTES;
        // The four 16-k slabs of the tile, software-pipelined inside the wave: the LDS reads of slabs ks+1..ks+AHEAD
        // are in flight while slab ks is multiplied (the lgkmcnt counter holds 15, hence AHEAD by reads per slab).
        constexpr int RPS = MI * FragAddr1<BM, TA>::READS + (NI + (EPI == 2 ? 1 : 0)) * FragAddr1<BN, TB>::READS;
        constexpr int AHEAD = 3 * RPS <= 15 ? 2 : (2 * RPS <= 15 ? 1 : 0);
        Frag af[4][MI], bf[4][NI], bf2[4];
        auto read_slab = [&](int ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa.load(af[ks][i], Ai, i, ks);
#pragma unroll
            for (int j = 0; j < NI; ++j) fb.load(bf[ks][j], Bi, j, ks);
            if constexpr (EPI == 2) fb.load(bf2[ks], Bi + OB::BYTES, 0, ks);
        };
#pragma unroll
        for (int ks = 0; ks < AHEAD; ++ks) read_slab(ks);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + AHEAD < 4) read_slab(ks + AHEAD);
            if (ks + AHEAD < 4) wait_reads<AHEAD * RPS>();
            else if (ks + 1 < 4 && AHEAD == 2 && ks == 2) wait_reads<RPS>();
            else wait_reads<0>();
#pragma unroll
            for (int i = 0; i < MI; ++i) pin_frag(af[ks][i], TA);
#pragma unroll
            for (int j = 0; j < NI; ++j) pin_frag(bf[ks][j], TB);
            if constexpr (EPI == 2) pin_frag(bf2[ks], TB);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_value(af[ks][i], TA), frag_value(bf[ks][j], TB), acc[i][j], 0, 0, 0);
            if constexpr (EPI == 2)
                acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_value(af[ks][0], TA), frag_value(bf2[ks], TB), acc2, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                  // keep the slab's MFMAs here, between the waits
        }
    }
    if (nk <= 0) return;

    if constexpr (EPI == 1) {
        static_assert(EPI == 0 || (BM / WR == 32 && BN / WC == 32), "the GLU epilogues expect one 32x32 MFMA tile per wave");
        // The epilogue moves 8 bytes per output element (h1 = [a | b] in, dh1 out) — as much HBM traffic as the GEMM itself.
        // In the accumulator layout a lane owns ONE column of 16 rows: 64 two-byte accesses per lane, 64-byte segments.  So
        // the wave's 32x32 tile goes through LDS once and a lane works on 8 consecutive columns of 2 rows: 16-byte loads
        // and stores, eight of them per lane.
        const int F = a.N;
        const uint32_t thr = a.glu_seed ? kk_drop_threshold(a.glu_p) : 0u, seed = thr ? *a.glu_seed : 0u;
        const float ik = thr ? 1.f / (1.f - a.glu_p) : 1.f;
        constexpr int TP = 36;                                  // floats per tile row (16-byte aligned rows)
        __builtin_amdgcn_s_barrier();                           // every wave is done with the last stage
        float *tile = reinterpret_cast<float *>(smem) + wave * 32 * TP;
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[frag_row(r, half) * TP + l31] = acc[0][0][r];
        __builtin_amdgcn_wave_barrier();                        // (one wave: its LDS operations complete in order)
        const int c8 = (lane & 3) * 8, col = n0 + wc * 32 + c8;
        float sa[8], sb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sa[j] = sb[j] = 0.f;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int rl = it * 16 + (lane >> 2), row = m0 + wr * 32 + rl;
            if (row < a.M && col < F) {
                const float4 d0 = ld4(tile + rl * TP + c8), d1 = ld4(tile + rl * TP + c8 + 4);
                const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
                const int64_t o = (int64_t)row * 2 * F + col;
                const bf16x8 av = *reinterpret_cast<const bf16x8 *>(a.glu_h + o), bv = *reinterpret_cast<const bf16x8 *>(a.glu_h + o + F);
                float mk[8];
                kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col, thr, ik, *reinterpret_cast<float(*)[4]>(mk));
                kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col + 4, thr, ik, *reinterpret_cast<float(*)[4]>(mk + 4));
                bf16x8 oa, ob;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float gv, gd;
                    kk_gelu_pair_fast((float)av[j], gv, gd);
                    const float dd = d[j] * mk[j];
                    const float da = dd * (float)bv[j] * gd, db = dd * gv;
                    oa[j] = (__bf16)da;
                    ob[j] = (__bf16)db;
                    sa[j] += da;
                    sb[j] += db;
                }
                kk_store16(a.glu_dh + o, __builtin_bit_cast(kk_u32x4, oa), a.wt);
                kk_store16(a.glu_dh + o + F, __builtin_bit_cast(kk_u32x4, ob), a.wt);
            }
        }
        // column sums over the wave's 32 rows: the 16 lanes that share (lane & 3)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            {   // lanes 4 and 8 away inside the 16-lane row by DPP rotations (only lanes 0..3 are read below: for them the same additions as
                // the xor butterfly), the rows 16 and 32 away by ds_bpermute
                sa[j] += kk_dpp<0x124>(sa[j]); sb[j] += kk_dpp<0x124>(sb[j]);
                sa[j] += kk_dpp<0x128>(sa[j]); sb[j] += kk_dpp<0x128>(sb[j]);
                sa[j] += __shfl_xor(sa[j], 16, 64); sb[j] += __shfl_xor(sb[j], 16, 64);
                sa[j] += __shfl_xor(sa[j], 32, 64); sb[j] += __shfl_xor(sb[j], 32, 64);
            }
        }
        const int prow = (m0 + wr * 32) / 32;                   // one partial row per 32 rows of dY, kk_gemm_dgrad_glu_blocks(T) of them
        if (lane < 4 && col < F && prow < 2 * ((a.M + 63) / 64)) {
            float *pr = a.glu_partials + (int64_t)prow * 2 * F;
            st4(pr + col, make_float4(sa[0], sa[1], sa[2], sa[3]));
            st4(pr + col + 4, make_float4(sa[4], sa[5], sa[6], sa[7]));
            st4(pr + F + col, make_float4(sb[0], sb[1], sb[2], sb[3]));
            st4(pr + F + col + 4, make_float4(sb[4], sb[5], sb[6], sb[7]));
        }
        return;
    }
    if constexpr (EPI == 3) {
        static_assert(EPI != 3 || (BN == 64 && BM / WR == 32 && BN / WC == 32), "the head-norm epilogue expects one 32x32 MFMA tile per wave, 64 columns");
        constexpr int PITCH = 72;                               // bf16 per LDS row: 144 B, rows land on different banks
        __bf16 *tile = reinterpret_cast<__bf16 *>(smem);
        __builtin_amdgcn_s_barrier();                           // every wave is done with the last stage
        {
            const int col = wc * 32 + l31;
            const float bv = a.bias ? a.bias[n0 + col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) tile[(wr * 32 + frag_row(r, half)) * PITCH + col] = (__bf16)(acc[0][0][r] + bv);
        }
        __syncthreads();
        const int sub = threadIdx.x & 15, part = n0 / a.hn_H;
        const bool rope = (a.hn_rope_mask >> part) & 1;
        const float4 g = ld4(a.hn_gain[part] + sub * 4);
        __bf16 *raw = static_cast<__bf16 *>(a.C);
        constexpr int RPI = 4 * WAVES;                          // rows per pass: 16 threads per (row, head) vector
#pragma unroll
        for (int it = 0; it < BM / RPI; ++it) {
            const int rl = it * RPI + (threadIdx.x >> 4), row = m0 + rl;
            const bf16x4 r4 = *reinterpret_cast<const bf16x4 *>(tile + rl * PITCH + sub * 4);
            const float4 v = make_float4((float)r4[0], (float)r4[1], (float)r4[2], (float)r4[3]);
            const int pos = rope ? (row < a.M ? row : a.M - 1) % a.hn_S : 0;
            const float4 n = kk_headnorm_rope(v, g, rope, a.hn_cos + pos * 64, a.hn_sin + pos * 64, sub);
            if (row < a.M) {
                kk_store8(raw + (int64_t)row * a.ldc + n0 + sub * 4, __builtin_bit_cast(kk_u32x2, r4), a.wt);
                bf16x4 n4;
                n4[0] = (__bf16)n.x; n4[1] = (__bf16)n.y; n4[2] = (__bf16)n.z; n4[3] = (__bf16)n.w;
                kk_store8(a.hn_y + (int64_t)row * a.hn_ldy + n0 + sub * 4, __builtin_bit_cast(kk_u32x2, n4), a.wt);
            }
        }
        return;
    }
    if constexpr (EPI == 2) {
        // (same transposition as EPI == 1: both accumulators through LDS, a lane stores 8 consecutive columns of 2 rows)
        const int F = a.N;
        const uint32_t thr = a.glu_seed ? kk_drop_threshold(a.glu_p) : 0u, seed = thr ? *a.glu_seed : 0u;
        const float ik = thr ? 1.f / (1.f - a.glu_p) : 1.f;
        constexpr int TP = 36;
        __builtin_amdgcn_s_barrier();                           // every wave is done with the last stage
        float *ta_ = reinterpret_cast<float *>(smem) + wave * 2 * 32 * TP, *tb_ = ta_ + 32 * TP;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ta_[frag_row(r, half) * TP + l31] = acc[0][0][r];
            tb_[frag_row(r, half) * TP + l31] = acc2[r];
        }
        __builtin_amdgcn_wave_barrier();
        const int c8 = (lane & 3) * 8, col = n0 + wc * 32 + c8;
        if (col >= F) return;
        float ba[8], bb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { ba[j] = a.bias ? a.bias[col + j] : 0.f; bb[j] = a.bias ? a.bias[F + col + j] : 0.f; }
        __bf16 *h = a.glu_dh, *g = static_cast<__bf16 *>(a.C);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int rl = it * 16 + (lane >> 2), row = m0 + wr * 32 + rl;
            if (row >= a.M) continue;
            const float4 a0 = ld4(ta_ + rl * TP + c8), a1 = ld4(ta_ + rl * TP + c8 + 4);
            const float4 b0 = ld4(tb_ + rl * TP + c8), b1 = ld4(tb_ + rl * TP + c8 + 4);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float mk[8];
            kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col, thr, ik, *reinterpret_cast<float(*)[4]>(mk));
            kk_drop_mul4(seed, a.glu_site, (uint64_t)row * F + col + 4, thr, ik, *reinterpret_cast<float(*)[4]>(mk + 4));
            bf16x8 oa, ob, og;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                oa[j] = (__bf16)(av[j] + ba[j]);                 // what the backward will read
                ob[j] = (__bf16)(bv[j] + bb[j]);
                og[j] = (__bf16)(kk_gelu_fast((float)oa[j]) * (float)ob[j] * mk[j]);
            }
            const int64_t o = (int64_t)row * 2 * F + col;
            kk_store16(h + o, __builtin_bit_cast(kk_u32x4, oa), a.wt);
            kk_store16(h + o + F, __builtin_bit_cast(kk_u32x4, ob), a.wt);
            kk_store16(g + (int64_t)row * a.ldc + col, __builtin_bit_cast(kk_u32x4, og), a.wt);
        }
        return;
    }
    const bool lead = (ksl == 0);
    // bf16 C without accumulation or residual (most dgrads, linear2): the tile goes through LDS so that a lane stores 8
    // consecutive columns (16 bytes) of 2 rows instead of 16 two-byte values of one column
    constexpr bool WIDE_OK = NS * STAGE >= WAVES * 32 * 36 * 4 + 512;      // the staging area holds one 32x32 fp32 tile per wave (+ the Delta rows)
    constexpr bool DELTA_OK = EPI == 0 && WAVES == 8 && WC == 2 && BM == 128 && BN == 64;      // one 32x32 tile per wave, a head per workgroup
    if (WIDE_OK && a.c_bf16 && a.residual == nullptr && (a.ldc & 7) == 0 && (a.N & 7) == 0 && (reinterpret_cast<uintptr_t>(a.C) & 15) == 0) {
        constexpr int TP = 36;
        __builtin_amdgcn_s_barrier();                           // every wave is done with the last stage
        float *tile = reinterpret_cast<float *>(smem) + wave * 32 * TP;
        __bf16 *C = static_cast<__bf16 *>(a.C);
        const int c8 = (lane & 3) * 8;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) tile[frag_row(r, half) * TP + l31] = acc[i][j][r];
                __builtin_amdgcn_wave_barrier();
                const int col = n0 + wc * (BN / WC) + j * 32 + c8;
                float dsum[2] = {0.f, 0.f};                   // Delta epilogue: this lane's 8 columns of its 2 rows
                if (col < a.N) {
                    float bv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) bv[e] = (a.bias != nullptr && lead) ? a.bias[col + e] : 0.f;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int rl = it * 16 + (lane >> 2), row = m0 + wr * (BM / WR) + i * 32 + rl;
                        if (row >= a.M) continue;
                        const float4 v0 = ld4(tile + rl * TP + c8), v1 = ld4(tile + rl * TP + c8 + 4);
                        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                        bf16x8 o;
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[e] = (__bf16)(a.alpha * v[e] + bv[e]);
                        kk_store16(C + (int64_t)row * a.ldc + col, __builtin_bit_cast(kk_u32x4, o), a.wt);
                        if constexpr (DELTA_OK) {
                            if (a.dl_out != nullptr) {              // (from the ROUNDED dO: what the attention kernels will read)
                                dsum[it] = g16_delta_dot(dsum[it], o, a.dl_o + (int64_t)row * a.dl_ldo + col);
                            }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if constexpr (DELTA_OK) {
                    if (a.dl_out != nullptr) {                      // (workgroup-uniform; N % 64 == 0 is checked by the entry point)
                        // a row's 32 columns of this wave: the 4 lanes that share lane >> 2; its other 32 are in wave wc ^ 1
                        float *red = reinterpret_cast<float *>(smem + WAVES * 32 * TP * 4);      // [WR][32] row sums of the wc = 1 waves
#pragma unroll
                        for (int it = 0; it < 2; ++it) {
                            dsum[it] += __shfl_xor(dsum[it], 1, 64);
                            dsum[it] += __shfl_xor(dsum[it], 2, 64);
                        }
                        if (wc == 1 && (lane & 3) == 0) {
                            red[wr * 32 + (lane >> 2)] = dsum[0];
                            red[wr * 32 + 16 + (lane >> 2)] = dsum[1];
                        }
                        __syncthreads();
                        if (wc == 0 && (lane & 3) == 0) {
#pragma unroll
                            for (int it = 0; it < 2; ++it) {
                                const int rl = it * 16 + (lane >> 2), row = m0 + wr * 32 + rl;
                                if (row < a.M) {
                                    const int bb = row / a.dl_S, q = row - bb * a.dl_S;
                                    a.dl_out[((int64_t)bb * a.dl_heads + n0 / 64) * a.dl_S + q] = dsum[it] + red[wr * 32 + rl];
                                }
                            }
                        }
                    }
                }
            }
        return;
    }
    // fp32 C written (or accumulated into) exactly once per element — the weight gradients — in a write-through launch: the same
    // transposition, so that a lane stores 8 consecutive columns of 2 rows as 16-byte write-through stores (a launch leaves up to
    // 31 MB of dW behind; as plain 4-byte stores they sit dirty in the L2s until the kernel boundary writes them back)
    if (a.wt && WIDE_OK && !a.c_bf16 && !a.atomic && a.residual == nullptr && (a.ldc & 3) == 0 && (a.N & 7) == 0 &&
        (reinterpret_cast<uintptr_t>(a.C) & 15) == 0) {
        constexpr int TP = 36;
        __builtin_amdgcn_s_barrier();                           // every wave is done with the last stage
        float *tile = reinterpret_cast<float *>(smem) + wave * 32 * TP;
        float *C = static_cast<float *>(a.C);
        const int c8 = (lane & 3) * 8;
        float ssq = 0.f;                                         // (ss_rec: this lane's share of the tile's sum of squares)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) tile[frag_row(r, half) * TP + l31] = acc[i][j][r];
                __builtin_amdgcn_wave_barrier();
                const int col = n0 + wc * (BN / WC) + j * 32 + c8;
                if (col < a.N) {
                    float bv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) bv[e] = (a.bias != nullptr && lead) ? a.bias[col + e] : 0.f;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int rl = it * 16 + (lane >> 2), row = m0 + wr * (BM / WR) + i * 32 + rl;
                        if (row >= a.M) continue;
                        float *dst = C + (int64_t)row * a.ldc + col;
                        const float4 v0 = ld4(tile + rl * TP + c8), v1 = ld4(tile + rl * TP + c8 + 4);
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
                __builtin_amdgcn_wave_barrier();
            }
        if (a.ss_rec != nullptr) {                              // (workgroup-uniform; splits == 1 by the caller) wave sums added in wave order
            double *wsum = reinterpret_cast<double *>(smem + WAVES * 32 * TP * 4);
            const double wv = wave_sum_d((double)ssq);
            if (lane == 0) wsum[wave] = wv;
            __syncthreads();
            if (threadIdx.x == 0) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) t += wsum[w];
                a.ss_rec[tid_lin] = KkSegRec{t, a.ss_seg + (a.ss_rows > 0 ? m0 / a.ss_rows : 0), 0};
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = n0 + wc * (BN / WC) + j * 32 + l31;
            if (col >= a.N) continue;
            const float bv = (a.bias != nullptr && lead) ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * (BM / WR) + i * 32 + frag_row(r, half);
                if (row >= a.M) continue;
                float v = a.alpha * acc[i][j][r] + bv;
                if (a.residual != nullptr && lead) {
                    const int64_t rr = a.res_mod > 0 ? (int64_t)row % a.res_mod : (int64_t)row;
                    v += a.residual[rr * a.ldr + col];
                }
                if (a.c_bf16) {
                    static_cast<__bf16 *>(a.C)[(int64_t)row * a.ldc + col] = (__bf16)v;
                    continue;
                }
                float *dst = static_cast<float *>(a.C) + (int64_t)row * a.ldc + col;
                if (a.atomic) {
                    atomicAdd(dst, v);
                } else {
                    if (a.beta != 0.f) v += a.beta * (*dst);
                    *dst = v;
                }
            }
        }
}

}  // namespace
