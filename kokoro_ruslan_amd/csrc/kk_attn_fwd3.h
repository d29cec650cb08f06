// Attention, internal: the third-generation forward body.  Compiled into the four attn_fwd3_* kernels of kk_attn_fwd.hip and, as one
// phase of the persistent sub-layer launch, into kk_chain.hip (which sets KK_QKV_AUX).  Include kk_attn.h (or kk_attn_host.h) first.
#pragma once

namespace {

// ------------------------------------------------------------------ forward, third generation (bf16 storage): two workgroups per CU
// What the stamps of attn_fwd2 said (tools/probes/attn_trace.py): the loop is VALU-bound — a wave64 VALU instruction occupies its
// SIMD for 4 clocks, ~250 of them per 32 x 32 score unit against 8 MFMAs — and its two waves per SIMD, phase-locked by the per-tile
// barrier of the two key groups, keep the VALU ~60 % busy; one 112 KB workgroup fits a CU, so the 512 workgroups of a 1024-frame
// launch run as two rounds, each with its own prologue, group imbalance and merge.  Here a workgroup needs <= 74 KB of LDS and <= 128
// registers, so TWO are resident per CU (four waves per SIMD, from independent workgroups: no common barrier), and the work is dealt
// so that every wave does the same amount: the 8 waves are QW query waves x KG key slots over ONE shared K/V ring whose tile is
// KT = 32 KG keys — in a tile step wave (qw, kg) computes exactly one 32 x 32 unit (queries 32 qw.., keys 32 kg.. of the tile).  No
// software pipelining inside a wave (the other three waves of the SIMD are the overlap), Q fragments re-read from LDS per unit.
// Same arithmetic per unit as attn_fwd2 (softmax per 32-key unit, same dropout function): the results differ from it only by the
// order in which the key slots' partial softmaxes are merged.
#ifndef KK_QKV_AUX
#define KK_QKV_AUX 0            // cache policy of the Q / K / V DMA loads (kk_chain.hip: sc1 = L1 bypass for tensors written earlier in the launch)
#endif
// CHAIN (kk_chain.hip): the body as one phase of a persistent launch — block coordinates from the caller, every wave stays to the end
// (no early exit in front of a workgroup barrier) and leaves through a barrier that frees the LDS for the next unit.
// KRD (kk_attn_fwd_rb): the dropout keep decisions are READ — the unit's 16 lane masks by two scalar loads from the array that
// kk_attn_keep_gen filled beside the encoder forward — instead of hashed and stored: -9 vector instructions per two scores and the
// 32 v_writelane + the store of a unit.  Same bits, same arithmetic: the output equals the hashing launch's bit for bit.
template <int QW, int KG, int NS, bool CHAIN = false, bool KRD = false>
__device__ __forceinline__ void attn_fwd3_body(const AttnArgs &a, int chain_bx = 0, int chain_by = 0) {
    typedef __bf16 T;
    constexpr int QB = 32 * QW, KT = 32 * KG, KIMG = KT * 128, STAGE = 2 * KIMG, RING = NS * STAGE;
    constexpr int KP = KT / 64, NPT = 2 * KP;                 // 16-byte pieces per thread: per operand, per tile
    static_assert(QW * KG == 8 && (QB * 8) % 512 == 0, "eight waves; whole Q pieces per thread");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [stage][K image | V image] | key-mask words | Q image
    uint64_t *kmb = reinterpret_cast<uint64_t *>(smem_raw + RING);         // [64] one word per 64 keys
    char *qimg = smem_raw + RING + 512;                                    // [QB queries][64] image
    int bx_, by_;
    if constexpr (CHAIN) { bx_ = chain_bx; by_ = chain_by; }
    else attn_block(a, bx_, by_, true);
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * QB;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int qw = wave8 % QW, kg = wave8 / QW;
    const int qmin = qblk + 32 * qw, q = qmin + l31;
    const bool qvalid = q < a.Sq;
    int kend = a.Sk;
    if (a.causal && qblk + QB < kend) kend = qblk + QB;
    int klim = kend;                                           // this wave multiplies the keys [0, klim)
    if (a.causal && qmin + 32 < klim) klim = qmin + 32;
    const int nt = (kend + KT - 1) / KT;
    // ---- Q rows of the block (the oldest DMA: covered by every wait below)
    {
        const int nrows = a.Sq - qblk < QB ? a.Sq - qblk : QB;
        const T *qb = static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + qblk) * a.ldq + hh * 64;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(qb), 0, nrows > 0 ? (int)((((int64_t)nrows - 1) * a.ldq + 64) * 2) : 0, 0x00020000);
#pragma unroll
        for (int j = 0; j < QB * 8 / 512; ++j) {
            const int p = threadIdx.x + 512 * j, row = p >> 3, pc = p & 7;
            const uint32_t vo = (uint32_t)(((int64_t)row * a.ldq + ((pc ^ ((row >> 1) & 7)) * 8)) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r, KK_LDS_PTR(qimg + wave8 * 1024 + j * 8192), 16, vo, 0, 0, KK_QKV_AUX);
        }
    }
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    uint32_t kmv[8];
    if (km) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = (wave8 + 8 * i) * 64 + lane;
            kmv[i] = key < kend ? km[key] : 0u;
        }
    }
    // ---- K / V tiles: every thread issues KP pieces of each
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.Sk * a.ldv + hh * 64;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Kb), 0, (int)((((int64_t)a.Sk - 1) * a.ldk + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Vb), 0, (int)((((int64_t)a.Sk - 1) * a.ldv + 64) * 2), 0x00020000);
    uint32_t kvo[KP], vvo[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int p = threadIdx.x + 512 * j, row = p >> 3, pc = p & 7;
        kvo[j] = (uint32_t)(((int64_t)row * a.ldk + ((pc ^ ((row >> 1) & 7)) * 8)) * 2);
        const int sw = 2 * ((row >> 1) & 1), g = (((pc >> 1) ^ sw) << 1) | (pc & 1);
        vvo[j] = (uint32_t)(((int64_t)row * a.ldv + g * 8) * 2);
    }
    const uint32_t ktile = (uint32_t)(KT * a.ldk * 2), vtile = (uint32_t)(KT * a.ldv * 2);
    auto issue_tile = [&](int t, int st) {
        char *dst = smem_raw + st * STAGE + wave8 * 1024;
#pragma unroll
        for (int j = 0; j < KP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, KK_LDS_PTR(dst + j * 8192), 16, kvo[j] + (uint32_t)t * ktile, 0, 0, KK_QKV_AUX);
#pragma unroll
        for (int j = 0; j < KP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, KK_LDS_PTR(dst + KIMG + j * 8192), 16, vvo[j] + (uint32_t)t * vtile, 0, 0, KK_QKV_AUX);
    };
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nt) issue_tile(t, t);
    if (km) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t bits = __ballot(kmv[i] != 0u);
            if (lane == 0) kmb[wave8 + 8 * i] = bits;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the words are in LDS before this wave reaches the loop's raw s_barrier
    }
    // ---- fragment addresses (bytes inside an image)
    const uint32_t sl = (uint32_t)(uintptr_t)KK_LDS_PTR(smem_raw);
    const uint32_t ql = (uint32_t)(uintptr_t)KK_LDS_PTR(qimg) + (uint32_t)((32 * qw + l31) * 128);
    uint32_t ka[4], va[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ka[ks] = (uint32_t)(l31 * 128 + (((2 * ks + half) ^ ((l31 >> 1) & 7)) * 16));
    {
        const int L = lane & 15, kq = L >> 2, gi = (lane >> 4) & 1, sw = 2 * ((kq >> 1) & 1);
#pragma unroll
        for (int db = 0; db < 2; ++db) va[db] = (uint32_t)((4 * half + kq) * 128 + (((2 * db + gi) ^ sw) * 32) + 8 * (L & 3));
    }
    f32x16 o[2];
    zero_acc(o[0]); zero_acc(o[1]);
    float m = -1e30f, l = 0.f;
    const float c2 = a.scale * 1.4426950408889634f;
    const int klast = a.causal ? min(a.Sk - 1, q) : a.Sk - 1;  // the last key this lane's query sees
    ProbDrop pd;
    pd.init(a, b, hh);
    // keep bits (AttnArgs::keep): the unit's 32 ballot dwords are gathered into lanes 0..31 of ONE register (v_writelane) and stored
    // at the top of the NEXT tile step, BEFORE that step's tile DMAs are issued: the counted vmcnt waits above stay exact — the only
    // operations younger than the tile a step waits for are the DMAs of the tile after it (CDNA4 counts stores in vmcnt too).
    const int nKU = (a.Sk + 31) >> 5;
    uint32_t *kbh = (!KRD && a.keep != nullptr && pd.thr != 0u && qmin < a.Sq)         // (a wave whose 32 rows lie beyond Sq has no unit row in the array)
        ? reinterpret_cast<uint32_t *>(static_cast<char *>(a.keep) + ((int64_t)(b * a.heads + hh) * ((a.Sq + 31) >> 5) + (qmin >> 5)) * nKU * 128) : nullptr;
    // KRD: this wave's row of units (wave-uniform address: scalar loads); rows beyond Sq read any valid row (their output is not stored)
    const kk_cu64x8 *keep_row = KRD ? reinterpret_cast<const kk_cu64x8 *>(reinterpret_cast<uintptr_t>(
        static_cast<const char *>(a.keep) + ((int64_t)(b * a.heads + hh) * ((a.Sq + 31) >> 5) + (qmin < a.Sq ? qmin >> 5 : 0)) * nKU * 128)) : nullptr;
    uint32_t kw_pend = 0u;
    uint32_t warm_sink = 0u;                                   // destination of the weight-warming loads (never read)
    int kw_unit = -1;                                          // (wave-uniform) key unit whose words are pending in kw_pend
    auto flush_keep = [&]() {
        if (kw_unit >= 0) {
            if (lane < 32) {                                      // (write-through like the launch's other outputs: 2 - 8 MB of bits per launch)
                if (a.wt) kk_st4_wt(kbh + kw_unit * 32 + lane, kw_pend);
                else kbh[kw_unit * 32 + lane] = kw_pend;
            }
            kw_unit = -1;
        }
        asm volatile("" ::: "memory");
    };
    for (int t = 0; t < nt; ++t) {
        // tile t landed once at most the younger tiles' DMAs are outstanding (tile t + NS - 1 goes out behind this step's barrier)
        const int younger = min(nt - 1 - t, NS - 2);
        if (NS >= 3 && younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // ... for every wave, and every wave is done with tile t - 1
        asm volatile("" ::: "memory");
        flush_keep();
        if (t + NS - 1 < nt) issue_tile(t + NS - 1, (t + NS - 1) % NS);
        if (t == nt - 1 && a.warm_bytes[0] != 0u) {            // (no DMA is issued after this point: only the final vmcnt(0) waits for these)
            const uint32_t lin = blockIdx.x + gridDim.x * blockIdx.y, ngrp = max((gridDim.x * gridDim.y) >> 3, 1u), j = lin >> 3;    // (a launch of fewer than 8 workgroups: one group)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const uint32_t lines = a.warm_bytes[w] >> 7, per = (lines + ngrp - 1) / ngrp;                 // (lines == 0: per == 0, no trip)
                for (uint32_t i = wave8 * 64 + lane; i < per; i += 512) {
                    const uint32_t line = j * per + i;
                    if (line < lines) {
                        const char *ptr = static_cast<const char *>(a.warm[w]) + ((size_t)line << 7);
                        asm volatile("global_load_dword %0, %1, off" : "=v"(warm_sink) : "v"(ptr) : "memory");
                    }
                }
            }
        }
        const int k0 = t * KT + 32 * kg;
        if (k0 >= klim) continue;                             // (causal: nothing of this unit is visible to these queries)
        const uint32_t kimg = sl + (uint32_t)((t % NS) * STAGE + kg * 4096), vimg = kimg + KIMG;
        // S^T = K . Q^T
        bf16x8 kf[4], qf[4];
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[0]) : "v"(kimg + ka[0]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qf[0]) : "v"(ql + (ka[0] & 127)));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[1]) : "v"(kimg + ka[1]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qf[1]) : "v"(ql + (ka[1] & 127)));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[2]) : "v"(kimg + ka[2]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qf[2]) : "v"(ql + (ka[2] & 127)));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[3]) : "v"(kimg + ka[3]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qf[3]) : "v"(ql + (ka[3] & 127)));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(kf[ks]), "+v"(qf[ks]));
        f32x16 s;
        zero_acc(s);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // V^T fragments in flight under the softmax
        s16x4 vlo[4], vhi[4];
        {
            const uint32_t a0 = vimg + va[0], a1 = vimg + va[1];
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(vlo[0]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(vhi[0]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(vlo[1]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(vhi[1]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(vlo[2]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(vhi[2]) : "v"(a0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(vlo[3]) : "v"(a1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(vhi[3]) : "v"(a1));
        }
        // softmax (+ dropout) of the unit, in place: the arithmetic of attn_fwd2's softmax_unit
        const uint32_t kmsub = km ? (uint32_t)(kmb[k0 >> 6] >> (k0 & 32)) : 0u;
        const bool edge = k0 + 32 > a.Sk || (a.causal && k0 + 31 > qmin) || kmsub != 0u;
        if (edge) {                                            // bit c of the word = key c of the unit is visible: no branches (kk_low_bits)
            const uint32_t aw = (kk_low_bits(klast - k0) & ~kmsub) >> (4 * half);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = __builtin_amdgcn_sbfe((int)aw, frag_row(r, 0), 1);
                s[r] = kk_bfif(s[r], m, (int)0xff800000);     // (v_bfi_b32: s or -inf)
            }
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = xor32_max(mx) * c2;
        const float mn = fmaxf(m, mx);
        if (__ballot(mn > m) != 0ull) {
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
            m = mn;
        }
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -m)); rs += s[r]; }
        rs = xor32_sum(rs);
        l += rs;
        if constexpr (KRD) {
            if (pd.thr) {
                const kk_u64x8 mk0 = keep_row[(k0 >> 5) * 2], mk1 = keep_row[(k0 >> 5) * 2 + 1];
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_inverse_ballot_w64(r < 8 ? mk0[r & 7] : mk1[r & 7]) ? s[r] : 0.f;
            }
        } else if (pd.thr) {
            const uint32_t xb = pd.row(q, k0 + 4 * half);
            uint64_t mk[16];                                   // the comparisons' lane masks = the unit's ballots
            uint32_t hprev = 0u;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                // (probe 1024: one hash per FOUR scores — every second hash is a rotation of the one before: wrong masks, the instruction
                //  count of VERDICT r4 item 2b's 8-bit decisions)
                const uint32_t hsh = (KK_DBG(a, 1024) && (r & 2)) ? ((hprev >> 8) | (hprev << 24)) : pd.hash(xb + (uint32_t)(frag_row(r, 0) >> 1));
                hprev = hsh;
                mk[r] = __builtin_amdgcn_uicmp(hsh & 0xFFFFu, pd.thr, 35);          // >= : keep_lo
                mk[r + 1] = __builtin_amdgcn_uicmp(hsh >> 16, pd.thr, 35);          //      keep_hi
                s[r] = __builtin_amdgcn_inverse_ballot_w64(mk[r]) ? s[r] : 0.f;
                s[r + 1] = __builtin_amdgcn_inverse_ballot_w64(mk[r + 1]) ? s[r + 1] : 0.f;
            }
            if (kbh != nullptr) {
                uint32_t kw = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(kw) : "s"((uint32_t)mk[r]), "n"(2 * r));
                    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(kw) : "s"((uint32_t)(mk[r] >> 32)), "n"(2 * r + 1));
                }
                kw_pend = kw;
                kw_unit = __builtin_amdgcn_readfirstlane(k0 >> 5);
            }
        }
        bf16x8 pb[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 8; ++j) pb[s2][j] = (__bf16)s[8 * s2 + j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vlo[i]), "+v"(vhi[i]));
        // O^T += V^T . P^T
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < 2; ++db)
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(vlo[s2 * 2 + db], vhi[s2 * 2 + db]), pb[s2], o[db], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    flush_keep();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" :: "v"(warm_sink));
    __syncthreads();                                           // the ring is free: the key slots' partial softmaxes meet in it
    {
        float *mb = reinterpret_cast<float *>(smem_raw);       // [(kg - 1) * QW + qw][lane][34]
        if (kg > 0) {
            float *w = mb + (((kg - 1) * QW + qw) * 64 + lane) * 34;
            w[0] = m; w[1] = l;
#pragma unroll
            for (int r = 0; r < 16; ++r) { w[2 + r] = o[0][r]; w[18 + r] = o[1][r]; }
        }
        __syncthreads();
        if constexpr (!CHAIN) { if (kg > 0) return; }
        if (kg == 0) {
#pragma unroll
        for (int g = 1; g < KG; ++g) {
            const float *w = mb + (((g - 1) * QW + qw) * 64 + lane) * 34;
            const float m1 = w[0], l1 = w[1], mn = fmaxf(m, m1);
            const float a0 = __builtin_amdgcn_exp2f(m - mn), a1 = __builtin_amdgcn_exp2f(m1 - mn);
            l = l * a0 + l1 * a1;
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] = o[0][r] * a0 + w[2 + r] * a1; o[1][r] = o[1][r] * a0 + w[18 + r] * a1; }
        }
        }
    }
    __syncthreads();                                           // (the QW remaining waves: everyone has read the merge area — the store tiles reuse it)
    static_assert(RING >= (KG - 1) * QW * 64 * 34 * 4 && RING >= QW * 4608, "merge area / store tiles fit the ring");
    if (kg == 0) {
        const float inv = l > 0.f ? pd.inv_keep / l : 0.f;
        store_rows_via_lds(static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + qmin) * a.ldout + hh * 64, a.ldout, a.Sq - qmin, o, inv,
                           smem_raw + qw * 4608, lane, a.wt);
        if (qvalid && half == 0) a.LSEo[((int64_t)b * a.heads + hh) * a.Sq + q] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : INFINITY;
    }
    if constexpr (CHAIN) __syncthreads();                      // the next unit of this workgroup reuses the ring, the mask words and the Q image
}

}  // namespace
