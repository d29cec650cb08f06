// Body of attn_bwd_dq2_kernel (kk_attn_bwd.hip); `a` is the kernel's by-value AttnArgs parameter.
    typedef __bf16 T;
    constexpr int NS = 3, KIMG = 64 * 64 * 2, STAGE = 2 * KIMG, GSZ = NS * STAGE, STEP = 128;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [group][stage][K | V], mask words, 3 x 16 KB images
    uint64_t *kmb = reinterpret_cast<uint64_t *>(smem_raw + 2 * GSZ);
    char *pro = smem_raw + 2 * GSZ + 512;                                  // Q | dO | O, later raw | cos | sin
    int bx_, by_;
    attn_block(a, bx_, by_, true);
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int wave = wave8 & 3, grp = wave8 >> 2, tg = threadIdx.x & 255;
    const int q = qblk + wave * 32 + l31;
    const bool qvalid = q < a.Sq;
    const int qmin = qblk + wave * 32;
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    int klim = kend;
    if (a.causal && qmin + 32 < klim) klim = qmin + 32;
    const int kfirst = grp * 64;
    const int nt = kfirst < kend ? (kend - kfirst + STEP - 1) / STEP : 0;
    const int nt0 = (kend + STEP - 1) / STEP;
    int nu = 0;
    if (klim > kfirst) {
        const int full = (klim - kfirst) / STEP, rem = (klim - kfirst) - full * STEP;
        nu = 2 * full + (rem > 32 ? 2 : (rem > 0 ? 1 : 0));
    }
    // every other global read is issued before the tile DMAs (the counted vmcnt waits assume the tiles are the youngest)
    const int64_t statrow = ((int64_t)b * a.heads + hh) * a.Sq + q;
    float lse2 = qvalid ? a.LSE[statrow] * 1.4426950408889634f : INFINITY;
    const bool want_delta = a.DeltaOut != nullptr;
    float dlt = (!want_delta && qvalid) ? a.Delta[statrow] : 0.f;
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    uint32_t kmv[8];
    if (km) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = (wave8 + 8 * i) * 64 + lane;
            kmv[i] = key < kend ? km[key] : 0u;
        }
    }
    const int nrows = a.Sq - qblk < 128 ? a.Sq - qblk : 128;
    dma_rows128(static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + qblk) * a.ldq + hh * 64, a.ldq, nrows, pro, wave8);
    dma_rows128(static_cast<const T *>(a.dO) + ((int64_t)b * a.Sq + qblk) * a.lddo + hh * 64, a.lddo, nrows, pro + 16384, wave8);
    if (want_delta) dma_rows128(static_cast<const T *>(a.O) + ((int64_t)b * a.Sq + qblk) * a.ldo + hh * 64, a.ldo, nrows, pro + 32768, wave8);
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
    char *gbase = smem_raw + grp * GSZ;
    const uint32_t ktile = (uint32_t)(STEP * a.ldk * 2), vtile = (uint32_t)(STEP * a.ldv * 2);
    const uint32_t kbeg = (uint32_t)(kfirst * a.ldk * 2), vbeg = (uint32_t)(kfirst * a.ldv * 2);
    auto issue_tile = [&](int t, int st) {
        char *dst = gbase + st * STAGE + wave * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, KK_LDS_PTR(dst + j * 4096), 16, kvo[j] + kbeg + (uint32_t)t * ktile, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, KK_LDS_PTR(dst + KIMG + j * 4096), 16, vvo[j] + vbeg + (uint32_t)t * vtile, 0, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (t < nt) issue_tile(t, t);
    if (km) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t bits = __ballot(kmv[i] != 0u);
            if (lane == 0) kmb[wave8 + 8 * i] = bits;
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
    auto ds_unit = [&](const f32x16 &s, const f32x16 &dp, int kb, uint32_t kmsub, bf16x8 (&db8)[2]) {
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
    // ---- prologue
    if (nt >= 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(lse2), "+v"(dlt));              // (their loads are older than the tiles: consumed here, not in the loop)
    __syncthreads();
    rowfrag_from_image(qf, pro, wave * 32, l31, half);
    rowfrag_from_image(dof, pro + 16384, wave * 32, l31, half);
    if (want_delta) {
        RowFrag<true> of;
        rowfrag_from_image(of, pro + 32768, wave * 32, l31, half);
        dlt = rowfrag_dot<true>(dof, of);
        dlt = xor32_sum(dlt);
        if (qvalid && half == 0 && grp == 0) a.DeltaOut[statrow] = dlt;
    }
    if (pd.thr) scale_rowfrag<true>(dof, pd.inv_keep);
    const bool has_hn = a.hn[0].raw != nullptr;
    bool hn_issued = false;
    f32x16 sa, dpa, sb, dpb;
    if (nu > 0) {
        read_kv(gl);
        wait_lds();
        scores(sa, dpa);
        if (nu > 1) read_kv(gl + 4096);
    }
    int st = 0;
    for (int t = 0; t < (KK_DBG(a, 32) ? 0 : nt0); ++t) {
        const int st1 = st + 1 == NS ? 0 : st + 1;
        if (t > 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // tile t+1 (and whatever else was in flight) landed
            __builtin_amdgcn_s_barrier();                           // ... for every wave; every wave is done with tile t-1
            asm volatile("" ::: "memory");
            if (t + NS - 1 < nt) issue_tile(t + NS - 1, st == 0 ? NS - 1 : st - 1);
            if (has_hn && !hn_issued) {                             // the prologue images are free since that barrier
                hn_dma_inputs(a.hn[0], (int64_t)b * a.Sq + qblk, qblk, nrows, hh, pro, wave8);
                hn_issued = true;
            }
        }
        const int u0 = 2 * t;
        if (u0 < nu) {
            const int k0 = kfirst + t * STEP;
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (has_hn && !hn_issued) hn_dma_inputs(a.hn[0], (int64_t)b * a.Sq + qblk, qblk, nrows, hh, pro, wave8);   // (single-tile launches)
    {                                // group 1's partial dQ -> LDS -> group 0
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
    T *out0 = static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + qmin) * a.ldout + hh * 64;
    char *otile = smem_raw + 36864 + wave * 4608;
    if (!has_hn) {
        if (grp == 0) store_rows_via_lds(out0, a.ldout, a.Sq - qmin, dq, a.scale, otile, lane, a.wt);
        return;
    }
    float *colred = reinterpret_cast<float *>(smem_raw);          // [128 rows][65]
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the epilogue images
    __syncthreads();                                              // ... for every wave; the merge buffer is free
    if (grp == 0) {
        f32x16 dx[2];
        hn_bwd_row2(dq, a.scale, qvalid, pro, pro + 16384, pro + 32768, wave * 32 + l31, a.hn[0].rope != 0, a.hn[0].gain, half,
                    colred + (wave * 32 + l31) * 65, dx);
        store_rows_via_lds(out0, a.ldout, a.Sq - qmin, dx, 1.f, otile, lane, a.wt);
    }
    __syncthreads();
    hn_colsum(colred, a.hn[0].partials);
