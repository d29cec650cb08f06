// Body of attn_bwd_dq3_kernel (kk_attn_bwd.hip): the dQ kernel as ONE wave group — four waves, 66 KB of LDS, two workgroups per CU.
// `a` is the kernel's by-value AttnArgs parameter.  Differences from kk_attn_bwd_dq2.inc: every wave walks ALL key tiles (no merge of
// two groups' partial dQ); the Q / dO row images of the prologue lie in ring stage 2 and a 16 KB extra area (tile 2 is issued behind
// the first barrier of the loop, when every wave holds its row fragments); the head-norm epilogue's images are fetched after the
// loop into the free ring (the co-resident workgroup covers the latency) and colred / the store tiles lie over them behind a barrier.
// Delta is an input (no O rows).
// KK_KEEP_BITS (attn_bwd_dq3k_kernel / the dQ half of attn_bwd_pair3k_kernel): the dropout keep decisions are READ — the forward's
// ballots of the unit (AttnArgs::keep), 16 lane masks fetched by two scalar loads and used by the selects directly — instead of hashed.
    typedef __bf16 T;
    constexpr int NS = 3, KIMG = 64 * 64 * 2, STAGE = 2 * KIMG, GSZ = NS * STAGE, STEP = 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [stage][K | V] | mask words | dO rows (prologue)
    uint64_t *kmb = reinterpret_cast<uint64_t *>(smem_raw + GSZ);
    char *qrows = smem_raw + 2 * STAGE, *dorows = smem_raw + GSZ + 512;
    int bx_, by_;
    attn_block(a, bx_, by_, true);
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int tg = threadIdx.x;
    // probe (tools builds, KK_ATTN_DBG bit 256): shader-clock stamps of workgroup (0, 0)'s waves into the buffer at DeltaOut
    unsigned long long *trace_ = (KK_DBG(a, 256) && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && a.DeltaOut != nullptr)
        ? reinterpret_cast<unsigned long long *>(a.DeltaOut) + wave * 64 : nullptr;
    auto stamp_ = [&](int slot) { if (KK_DBG(a, 256) && trace_ != nullptr && slot < 64) trace_[slot] = __builtin_amdgcn_s_memtime(); };
    stamp_(0);
    const int q = qblk + wave * 32 + l31;
    const bool qvalid = q < a.Sq;
    const int qmin = qblk + wave * 32;
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    int klim = kend;
    if (a.causal && qmin + 32 < klim) klim = qmin + 32;
    const int nt = (kend + STEP - 1) / STEP;
    int nu = 0;
    if (klim > 0) {
        const int full = klim / STEP, rem = klim - full * STEP;
        nu = 2 * full + (rem > 32 ? 2 : (rem > 0 ? 1 : 0));
    }
    // every other global read is issued before the tile DMAs (the counted vmcnt waits assume the tiles are the youngest)
    const int64_t statrow = ((int64_t)b * a.heads + hh) * a.Sq + q;
    float lse2 = qvalid ? a.LSE[statrow] * 1.4426950408889634f : INFINITY;
    float dlt = qvalid ? a.Delta[statrow] : 0.f;
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    uint32_t kmv[16];
    if (km) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = (wave + 4 * i) * 64 + lane;
            kmv[i] = key < kend ? km[key] : 0u;
        }
    }
    const int nrows = a.Sq - qblk < 128 ? a.Sq - qblk : 128;
    dma_rows128<256>(static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + qblk) * a.ldq + hh * 64, a.ldq, nrows, qrows, wave);
    dma_rows128<256>(static_cast<const T *>(a.dO) + ((int64_t)b * a.Sq + qblk) * a.lddo + hh * 64, a.lddo, nrows, dorows, wave);
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.Sk * a.ldv + hh * 64;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Kb), 0, (int)((((int64_t)a.Sk - 1) * a.ldk + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Vb), 0, (int)((((int64_t)a.Sk - 1) * a.ldv + 64) * 2), 0x00020000);
    uint32_t kvo[2], vvo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = tg + 256 * j, row = p >> 3, pc = p & 7;
        kvo[j] = (uint32_t)(((int64_t)row * a.ldk + ((pc ^ (kk_xb(row) << 1)) * 8)) * 2);
        vvo[j] = (uint32_t)(((int64_t)row * a.ldv + ((pc ^ ((row >> 1) & 7)) * 8)) * 2);
    }
    char *gbase = smem_raw;
    const uint32_t ktile = (uint32_t)(STEP * a.ldk * 2), vtile = (uint32_t)(STEP * a.ldv * 2);
    auto issue_tile = [&](int t, int st) {
        char *dst = gbase + st * STAGE + wave * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, KK_LDS_PTR(dst + j * 4096), 16, kvo[j] + (uint32_t)t * ktile, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, KK_LDS_PTR(dst + KIMG + j * 4096), 16, vvo[j] + (uint32_t)t * vtile, 0, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)                       // (stage NS - 1 holds the Q rows until the loop's first barrier)
        if (t < nt) issue_tile(t, t);
    if (km) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint64_t bits = __ballot(kmv[i] != 0u);
            if (lane == 0) kmb[wave + 4 * i] = bits;
        }
    }
    // ---- fragment addresses (bytes inside a stage)
    const uint32_t gl = (uint32_t)(uintptr_t)KK_LDS_PTR(gbase);
    uint32_t ka[4], va[4], ta[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        ka[ks] = (uint32_t)(l31 * 128 + (((2 * ks + half) ^ (kk_xb(l31) << 1)) * 16));
        va[ks] = (uint32_t)(KIMG + l31 * 128 + (((2 * ks + half) ^ ((l31 >> 1) & 7)) * 16));
    }
    {
        const int L = lane & 15, kq = L >> 2, gi = (lane >> 4) & 1, xb = (((kq >> 1) & 1) << 1) | half;
#pragma unroll
        for (int db = 0; db < 2; ++db) ta[db] = (uint32_t)((4 * half + kq) * 128 + (((2 * db + gi) ^ xb) * 32) + 8 * (L & 3));
    }
    bf16x8 kf[4], vf[4];
    s16x4 tlo[4], thi[4];
    auto read_kv = [&](uint32_t img) {                     // row fragments of the unit's 32 keys (img = its first K row)
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[0]) : "v"(img + ka[0]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[1]) : "v"(img + ka[1]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[2]) : "v"(img + ka[2]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[3]) : "v"(img + ka[3]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(vf[0]) : "v"(img + va[0]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(vf[1]) : "v"(img + va[1]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(vf[2]) : "v"(img + va[2]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(vf[3]) : "v"(img + va[3]));
    };
    auto read_kt = [&](uint32_t img) {                     // K^T fragments of the same keys
        const uint32_t a0 = img + ta[0], a1 = img + ta[1];
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(tlo[0]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(thi[0]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(tlo[1]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(thi[1]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(tlo[2]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(thi[2]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(tlo[3]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(thi[3]) : "v"(a1));
    };
    auto wait_lds = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    RowFrag<true> qf, dof;
    auto scores = [&](f32x16 &s, f32x16 &dp) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(kf[ks]), "+v"(vf[ks]));
        zero_acc(s); zero_acc(dp);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf.v[ks], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks], dof.v[ks], dp, 0, 0, 0);
        }
    };
    f32x16 dq[2];
    zero_acc(dq[0]); zero_acc(dq[1]);
    const float c2 = a.scale * 1.4426950408889634f;
    ProbDrop pd;
    pd.init(a, b, hh);
#ifdef KK_KEEP_BITS
    // this wave's row of units in the keep-bit array (wave-uniform: scalar loads)
    const kk_cu64x8 *keep_row = reinterpret_cast<const kk_cu64x8 *>(reinterpret_cast<uintptr_t>(
        static_cast<const char *>(a.keep) + ((int64_t)(b * a.heads + hh) * ((a.Sq + 31) >> 5) + (qmin < a.Sq ? qmin >> 5 : 0)) * ((a.Sk + 31) >> 5) * 128));      // (rows beyond Sq: any valid row — their probabilities are 0)
#endif
    // the last key this lane's query sees, and the edge sub-tiles' masks without branches: bit c of a unit's word = key c is visible
    const int klast = a.causal ? min(a.Sk - 1, q) : a.Sk - 1;
    auto ds_unit = [&](const f32x16 &s, const f32x16 &dp, int kb, uint32_t kmsub, bf16x8 (&db8)[2]) {
        const bool edge = kb + 32 > a.Sk || (a.causal && kb + 31 > qmin) || kmsub != 0u;
        float pv[16], ds[16];
#ifdef KK_KEEP_BITS
        const kk_u64x8 mk0 = keep_row[(kb >> 5) * 2], mk1 = keep_row[(kb >> 5) * 2 + 1];      // (this variant is launched with dropout on only)
#endif
#pragma unroll
        for (int r = 0; r < 16; ++r) pv[r] = __builtin_amdgcn_exp2f(s[r] * c2 - lse2);
        if (edge) {
            const uint32_t aw = (kk_low_bits(klast - kb) & ~kmsub) >> (4 * half);
#pragma unroll
            for (int r = 0; r < 16; ++r) pv[r] = kk_andf(pv[r], __builtin_amdgcn_sbfe((int)aw, frag_row(r, 0), 1));
        }
#ifdef KK_KEEP_BITS
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool keep = __builtin_amdgcn_inverse_ballot_w64(r < 8 ? mk0[r & 7] : mk1[r & 7]);
            ds[r] = pv[r] * ((keep ? dp[r] : 0.f) - dlt);
        }
#else
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
#endif
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 8; ++j) db8[s2][j] = (__bf16)ds[8 * s2 + j];
    };
    auto dq_acc = [&](const bf16x8 (&db8)[2]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(tlo[i]), "+v"(thi[i]));
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < 2; ++db)
                dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(tlo[s2 * 2 + db], thi[s2 * 2 + db]), db8[s2], dq[db], 0, 0, 0);
    };
    // ---- prologue: the row images and tiles 0, 1 landed (the end of tile 0 already reads tile 1's fragments)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(lse2), "+v"(dlt));
    __syncthreads();
    rowfrag_from_image(qf, qrows, wave * 32, l31, half);
    rowfrag_from_image(dof, dorows, wave * 32, l31, half);
    if (pd.thr) scale_rowfrag<true>(dof, pd.inv_keep);
    stamp_(1);
    const bool has_hn = a.hn[0].raw != nullptr;
    f32x16 sa, dpa, sb, dpb;
    if (nu > 0) {
        read_kv(gl);
        wait_lds();
        scores(sa, dpa);
        if (nu > 1) read_kv(gl + 4096);
    }
    int st = 0;
    for (int t = 0; t < nt; ++t) {
        const int st1 = st + 1 == NS ? 0 : st + 1;
        stamp_(4 + 3 * t);
        if (t > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 (and whatever else was in flight) landed
        stamp_(5 + 3 * t);
        __builtin_amdgcn_s_barrier();                               // ... for every wave; every wave is done with tile t-1 (t = 0: with the Q rows)
        asm volatile("" ::: "memory");
        stamp_(6 + 3 * t);
        if (t + NS - 1 < nt) issue_tile(t + NS - 1, st == 0 ? NS - 1 : st - 1);
        const int u0 = 2 * t;
        if (u0 < nu) {
            const int k0 = t * STEP;
            const uint64_t kmbits = km ? kmb[k0 >> 6] : 0ull;
            const uint32_t cur = gl + st * STAGE, nxt = gl + st1 * STAGE;
            bf16x8 d8[2];
            if (u0 + 1 < nu) { wait_lds(); scores(sb, dpb); }
            __builtin_amdgcn_sched_barrier(0);
            read_kt(cur);
            ds_unit(sa, dpa, k0, (uint32_t)kmbits, d8);
            wait_lds();
            dq_acc(d8);
            __builtin_amdgcn_sched_barrier(0);
            if (u0 + 2 < nu) read_kv(nxt);
            if (u0 + 1 < nu) {
                if (u0 + 2 < nu) { wait_lds(); scores(sa, dpa); }
                __builtin_amdgcn_sched_barrier(0);
                read_kt(cur + 4096);
                ds_unit(sb, dpb, k0 + 32, (uint32_t)(kmbits >> 32), d8);
                wait_lds();
                dq_acc(d8);
                __builtin_amdgcn_sched_barrier(0);
                if (u0 + 3 < nu) read_kv(nxt + 4096);
            }
        }
        st = st1;
    }
    stamp_(58);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                              // the ring is free
    stamp_(59);
    T *out0 = static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + qmin) * a.ldout + hh * 64;
    char *otile = smem_raw + 36864 + wave * 4608;
    // Weight warming (AttnArgs::warm, kk_attn_warm_next): one dword per 128-byte line of the matrices the NEXT GEMMs multiply with, this
    // XCD's dQ workgroups sharing the lines out.  Last thing the dQ half does: it ends ~9 us before the dK/dV workgroup beside it
    // (profiles/r05_attn_bwd_pair_stamps.txt), so the round trips cost the launch nothing.
    auto warm_next = [&]() {
        if (a.warm_bytes[0] == 0u) return;
        const uint32_t lin = blockIdx.x + gridDim.x * blockIdx.y, ngrp = max((gridDim.x * gridDim.y) >> 3, 1u), j = lin >> 3;    // (a launch of fewer than 8 workgroups: one group)
        uint32_t sink = 0u;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const uint32_t lines = a.warm_bytes[w] >> 7, per = (lines + ngrp - 1) / ngrp;                 // (lines == 0: per == 0, no trip)
            for (uint32_t i = threadIdx.x; i < per; i += 256) {
                const uint32_t line = j * per + i;
                if (line < lines) {
                    const char *ptr = static_cast<const char *>(a.warm[w]) + ((size_t)line << 7);
                    asm volatile("global_load_dword %0, %1, off" : "=v"(sink) : "v"(ptr) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" :: "v"(sink));
    };
    if (!has_hn) {
        store_rows_via_lds(out0, a.ldout, a.Sq - qmin, dq, a.scale, otile, lane, a.wt);
        warm_next();
        return;
    }
    const HnGain gnq = hn_load_gain(a.hn[0].gain, half);                                           // (lands under the image DMAs below)
    hn_dma_inputs<256>(a.hn[0], (int64_t)b * a.Sq + qblk, qblk, nrows, hh, smem_raw, wave);       // raw | cos | sin: 48 KB
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp_(60);
    {
        f32x16 dx[2];
        float cr[32];
        hn_bwd_row2_core(dq, a.scale, qvalid, smem_raw, smem_raw + 16384, smem_raw + 32768, wave * 32 + l31, a.hn[0].rope != 0, gnq, half, cr, dx);
        // (as in the dK/dV body: column sums in registers, the store tile and the wave's 64 sums over its OWN dead image rows, one barrier)
        const float cq = hn_colsum32(cr, l31);
        store_rows_via_lds16(out0, a.ldout, a.Sq - qmin, dx, 1.f, smem_raw + wave * 4096, lane, a.wt);
        reinterpret_cast<float *>(smem_raw + 16384 + wave * 4096)[hn_colsum32_col(l31, half)] = cq;
        __syncthreads();
        if (threadIdx.x < 64) {
            const float *cp = reinterpret_cast<const float *>(smem_raw + 16384) + threadIdx.x;
            a.hn[0].partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 64 + threadIdx.x] = (cp[0] + cp[1024]) + (cp[2048] + cp[3072]);
        }
        if (KK_DBG(a, 256)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp_(61); }
    }
    warm_next();
