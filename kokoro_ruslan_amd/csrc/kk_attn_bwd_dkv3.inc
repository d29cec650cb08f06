// Body of attn_bwd_dkv3_kernel (kk_attn_bwd.hip): the dK/dV kernel as ONE wave group — four waves (32 keys each, every query tile),
// 70 KB of LDS, two workgroups per CU; no merge of two groups' partial dK / dV.  `a` is the kernel's by-value AttnArgs parameter.
// The K / V row images of the prologue lie in ring stage 2 and a 16 KB extra area (tile 2 is issued behind the loop's first barrier);
// the head-norm epilogues' images are fetched after the loop: raw K | cos | sin over the ring, raw V behind the store tiles.
// KK_KEEP_BITS (attn_bwd_dkv3k_kernel / the dK/dV half of attn_bwd_pair3k_kernel): the dropout keep decisions are READ.  A lane owns a
// key; the forward's ballot dword for that key holds its bits over the unit's 32 queries (AttnArgs::keep), so a lane needs ONE dword
// per unit: the 1 KB of a tile step's 2 x 4 units rides the stage's DMA (wave 2), each lane fetches its dword with the lse rows and
// a register's decision is v_bfe_i32 — 3 vector instructions per score where the hash took ~9.
    typedef __bf16 T;
    constexpr int NS = 3, IMG = 64 * 64 * 2, STAGE = 2 * IMG + 512 + 1024, GSZ = NS * STAGE, STEP = 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [stage][Q | dO | lse | delta | keep words] | V rows (prologue); 71680 bytes
    static_assert(GSZ + 16384 <= 71680 && 2 * STAGE + 16384 <= GSZ + 16384, "ring + prologue rows inside the launch's LDS");
    char *krows = smem_raw + 2 * STAGE, *vrows = smem_raw + GSZ;
    char *rawv_img = smem_raw + 55296;                                     // (behind the store tiles)
    int bx_, by_;
    attn_block(a, bx_, by_, a.short_first != 0);
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int kblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int tg = threadIdx.x;
    unsigned long long *trace_ = (KK_DBG(a, 256) && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && a.DeltaOut != nullptr)
        ? reinterpret_cast<unsigned long long *>(a.DeltaOut) + (4 + wave) * 64 : nullptr;      // (probe: rows 4..7 of the stamp buffer)
    auto stamp_ = [&](int slot) { if (KK_DBG(a, 256) && trace_ != nullptr && slot < 64) trace_[slot] = __builtin_amdgcn_s_memtime(); };
    stamp_(0);
    const int kmin = kblk + wave * 32, key = kmin + l31;
    const bool kvalid = key < a.Sk;
    const bool kalive = kvalid && !(a.key_mask && a.key_mask[(int64_t)b * a.Sk + key]);     // (older than every DMA)
    const int kmaxw = kmin + 31;
    const int qstart = a.causal ? (kblk / 64) * 64 : 0;
    const int qfirst = qstart;
    const int nt = qfirst < a.Sq ? (a.Sq - qfirst + STEP - 1) / STEP : 0;
    const int nrows = a.Sk - kblk < 128 ? a.Sk - kblk : 128;
    dma_rows128<256>(static_cast<const T *>(a.K) + ((int64_t)b * a.Sk + kblk) * a.ldk + hh * 64, a.ldk, nrows, krows, wave);
    dma_rows128<256>(static_cast<const T *>(a.V) + ((int64_t)b * a.Sk + kblk) * a.ldv + hh * 64, a.ldv, nrows, vrows, wave);
    const T *Qb = static_cast<const T *>(a.Q) + (int64_t)b * a.Sq * a.ldq + hh * 64;
    const T *dOb = static_cast<const T *>(a.dO) + (int64_t)b * a.Sq * a.lddo + hh * 64;
    const float *LSEb = a.LSE + ((int64_t)b * a.heads + hh) * a.Sq, *DLb = a.Delta + ((int64_t)b * a.heads + hh) * a.Sq;
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Qb), 0, (int)((((int64_t)a.Sq - 1) * a.ldq + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rdo = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(dOb), 0, (int)((((int64_t)a.Sq - 1) * a.lddo + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rst = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(wave == 0 ? LSEb : DLb), 0, a.Sq * 4, 0x00020000);
    uint32_t qvo[2], dvo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = tg + 256 * j, row = p >> 3, pc = p & 7, c = pc ^ (kk_xb(row) << 1);
        qvo[j] = (uint32_t)(((int64_t)row * a.ldq + c * 8) * 2);
        dvo[j] = (uint32_t)(((int64_t)row * a.lddo + c * 8) * 2);
    }
    char *gbase = smem_raw;
    const uint32_t qtile = (uint32_t)(STEP * a.ldq * 2), dtile = (uint32_t)(STEP * a.lddo * 2);
    const uint32_t qbeg = (uint32_t)(qfirst * a.ldq * 2), dbeg = (uint32_t)(qfirst * a.lddo * 2);
    const bool stat_lane = wave < 2 && lane < 16;          // wave 0: the tile's 64 lse values, wave 1: its 64 Delta values
#ifdef KK_KEEP_BITS
    // wave 2: the keep words of the tile step's 2 query units x this block's 4 key units (2 runs of 512 contiguous bytes), 16 bytes per lane
    const int nKU_ = (a.Sk + 31) >> 5, nQU_ = (a.Sq + 31) >> 5;
    const __amdgpu_buffer_rsrc_t rkb = __builtin_amdgcn_make_buffer_rsrc(
        static_cast<char *>(a.keep) + (int64_t)(b * a.heads + hh) * nQU_ * nKU_ * 128, 0, nQU_ * nKU_ * 128, 0x00020000);
    const uint32_t kb_vo = (uint32_t)((lane >> 5) * nKU_ * 128 + (kblk >> 5) * 128 + (lane & 31) * 16);
    const uint32_t kb_tile = (uint32_t)(2 * nKU_ * 128), kb_beg = (uint32_t)((qfirst >> 5) * nKU_ * 128);
#endif
    auto issue_tile = [&](int t, int st) {
        char *dst = gbase + st * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, KK_LDS_PTR(dst + wave * 1024 + j * 4096), 16, qvo[j] + qbeg + (uint32_t)t * qtile, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rdo, KK_LDS_PTR(dst + IMG + wave * 1024 + j * 4096), 16, dvo[j] + dbeg + (uint32_t)t * dtile, 0, 0, 0);
        if (stat_lane)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rst, KK_LDS_PTR(dst + 2 * IMG + wave * 256), 16, (uint32_t)((qfirst + t * STEP) * 4 + lane * 16), 0, 0, 0);
#ifdef KK_KEEP_BITS
        if (wave == 2)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rkb, KK_LDS_PTR(dst + 2 * IMG + 512), 16, kb_vo, kb_beg + (uint32_t)t * kb_tile, 0, 0);
#endif
    };
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)                       // (stage NS - 1 holds the K rows until the loop's first barrier)
        if (t < nt) issue_tile(t, t);
    // ---- fragment addresses (bytes inside a stage)
    const uint32_t gl = (uint32_t)(uintptr_t)KK_LDS_PTR(gbase);
    uint32_t ra_[4], ta[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ra_[ks] = (uint32_t)(l31 * 128 + (((2 * ks + half) ^ (kk_xb(l31) << 1)) * 16));
    {
        const int L = lane & 15, kq = L >> 2, gi = (lane >> 4) & 1, xb = (((kq >> 1) & 1) << 1) | half;
#pragma unroll
        for (int db = 0; db < 2; ++db) ta[db] = (uint32_t)((4 * half + kq) * 128 + (((2 * db + gi) ^ xb) * 32) + 8 * (L & 3));
    }
    bf16x8 qr[4], dr[4];
    s16x4 qlo[4], qhi[4], dlo[4], dhi[4];
    auto read_rows = [&](uint32_t img) {                   // row fragments of the unit's 32 queries (img = first Q row)
        asm volatile("ds_read_b128 %0, %1" : "=v"(qr[0]) : "v"(img + ra_[0]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qr[1]) : "v"(img + ra_[1]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qr[2]) : "v"(img + ra_[2]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(qr[3]) : "v"(img + ra_[3]));
        asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(dr[0]) : "v"(img + ra_[0]));
        asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(dr[1]) : "v"(img + ra_[1]));
        asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(dr[2]) : "v"(img + ra_[2]));
        asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(dr[3]) : "v"(img + ra_[3]));
    };
    auto wait_lds = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    RowFrag<true> kf, vf;
    f32x16 dk[2], dv[2];
    zero_acc(dk[0]); zero_acc(dk[1]); zero_acc(dv[0]); zero_acc(dv[1]);
    ProbDrop pd;
    pd.init(a, b, hh);
    const float c2 = a.scale * 1.4426950408889634f;
    const bool anydead = __ballot(!kalive) != 0ull;
#ifdef KK_DKV_STORE_DS
    // (attn_bwd_dkv3s_kernel) dS = P o (dP - Delta), rounded to bf16 exactly as the dK MFMA below consumes it, leaves the workgroup as
    // [32 keys][32 queries] tiles of 2 KB: tile (key unit, query unit) of this (batch, head) at ((ku * nqu4) + qu) * 2048 — the
    // operand of attn_bwd_dqpass_kernel, which then needs no scores, exponentials or masks of its own
    const int nqu4 = ((a.Sq + 127) >> 7) << 2;
    const bool ds_on = kmin < a.Sk;                        // (wave-uniform)
    // (buffer stores: descriptor and tile offset in scalar registers, one vector register for the lane's place in a tile — the
    //  kernel has no vector registers to spare, and a 64-bit address per lane cost 15 spilled ones)
    const __amdgpu_buffer_rsrc_t rds = __builtin_amdgcn_make_buffer_rsrc(
        static_cast<char *>(a.dS) + (int64_t)(b * a.heads + hh) * ((a.Sk + 31) >> 5) * nqu4 * 2048, 0, 0x7FFFFFFF, 0x00020000);
    const uint32_t ds_row = (uint32_t)((kmin >> 5) * nqu4) * 2048u;
#endif
    // ---- prologue: K, V rows and tiles 0, 1 landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rowfrag_from_image(kf, krows, wave * 32, l31, half);
    rowfrag_from_image(vf, vrows, wave * 32, l31, half);
    if (pd.thr) scale_rowfrag<true>(vf, pd.inv_keep);
    stamp_(1);
    const bool has_hn = a.hn[0].raw != nullptr;
    auto unit_live = [&](int qb) { return qb < a.Sq && !(a.causal && qb + 31 < kmin); };
    bool pref = false;                                     // (wave-uniform) the next live unit's row fragments are in flight
    int st = 0;
    for (int t = 0; t < nt; ++t) {
        const int st1 = st + 1 == NS ? 0 : st + 1;
        stamp_(4 + 3 * t);
        if (t > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp_(5 + 3 * t);
        __builtin_amdgcn_s_barrier();                      // (t = 0: every wave holds its K / V row fragments — stage 2 is free)
        asm volatile("" ::: "memory");
        stamp_(6 + 3 * t);
        if (t + NS - 1 < nt) issue_tile(t + NS - 1, st == 0 ? NS - 1 : st - 1);
        const int q0 = qfirst + t * STEP;
        const uint32_t cur = gl + st * STAGE, nxt = gl + st1 * STAGE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int qb = q0 + sub * 32;
            if (!unit_live(qb)) continue;
            f32x16 s, dp;
            if (!pref) read_rows(cur + sub * 4096);
            wait_lds();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qr[ks]), "+v"(dr[ks]));
            zero_acc(s); zero_acc(dp);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qr[ks], kf.v[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dr[ks], vf.v[ks], dp, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // Register diet (two waves per SIMD: 256 registers, and a spill is fatal here — scratch reloads queue behind the tile
            // DMAs): lse rows -> P -> Delta rows -> dS, the dO^T fragments fetched under the exponentials, the Q^T fragments under dS.
            const uint32_t tq0 = cur + sub * 4096 + ta[0], tq1 = cur + sub * 4096 + ta[1];
            const uint32_t sa_ = cur + 2 * IMG + (uint32_t)((sub * 32 + 4 * half) * 4);
            f32x4_ st4[4];
            asm volatile("ds_read_b128 %0, %1" : "=v"(st4[0]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(st4[1]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(st4[2]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:96" : "=v"(st4[3]) : "v"(sa_));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:8192" : "=v"(dlo[0]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:9216" : "=v"(dhi[0]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:8192" : "=v"(dlo[1]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:9216" : "=v"(dhi[1]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:10240" : "=v"(dlo[2]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:11264" : "=v"(dhi[2]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:10240" : "=v"(dlo[3]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:11264" : "=v"(dhi[3]) : "v"(tq1));
            asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");                      // the four lse reads
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(st4[g]));
            const bool edge = anydead || qb + 32 > a.Sq || (a.causal && kmaxw > qb);
            float p[16], ds[16];
#ifdef KK_KEEP_BITS
            uint32_t kwd = 0u;                                 // this key's keep bits over the unit's 32 queries
            {
                uint32_t ln = threadIdx.x & 31u;               // (recomputed per unit: a register kept across the loop is one too many here)
                asm volatile("" : "+v"(ln));
                const uint32_t wi = ((ln & 3u) << 3) + ((ln >> 3) << 5) + ((ln >> 2) & 1u) * 4u;      // 4 * (2 r_f + h_f): the forward's ballot of this key
                asm volatile("ds_read_b32 %0, %1" : "=v"(kwd) : "v"(cur + (uint32_t)(2 * IMG + 512) + (uint32_t)(sub * 512 + wave * 128) + wi));
            }
#endif
            // (ONE fma per score on lse rows scaled once per unit: written as two products, hipcc packs them into v_pk_mul_f32 with a
            //  v_mov per operand to pair them up — 3.5 vector instructions per score instead of 2)
#pragma unroll
            for (int g = 0; g < 4; ++g) st4[g] *= 1.4426950408889634f;
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -st4[r >> 2][r & 3]));
            if (edge) {
                // bit c of the word = query c of the unit is visible to this key: queries [key (causal), Sq) of a live key, no branches
                uint32_t aw = kk_low_bits(a.Sq - 1 - qb);
                if (a.causal) aw &= ~kk_low_bits(key - qb - 1);
                aw = kalive ? aw >> (4 * half) : 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] = kk_andf(p[r], __builtin_amdgcn_sbfe((int)aw, frag_row(r, 0), 1));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(p[r]));            // P exists: the lse registers are free
            asm volatile("ds_read_b128 %0, %1 offset:256" : "=v"(st4[0]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:288" : "=v"(st4[1]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:320" : "=v"(st4[2]) : "v"(sa_));
            asm volatile("ds_read_b128 %0, %1 offset:352" : "=v"(st4[3]) : "v"(sa_));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(st4[g]));
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(dlo[i]), "+v"(dhi[i]));
            bf16x8 p8[2], d8[2];
#ifdef KK_KEEP_BITS
            {                                                  // (this variant is launched with dropout on only: no branch, no second path)
                asm volatile("" : "+v"(kwd));                  // (landed: the lgkmcnt(0) above)
                const uint32_t kws = kwd >> (4 * half);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = __builtin_amdgcn_sbfe((int)kws, frag_row(r, 0), 1);
                    ds[r] = p[r] * (kk_andf(dp[r], m) - st4[r >> 2][r & 3]);
                    p[r] = kk_andf(p[r], m);
                }
            }
#else
            if (pd.thr) {
                // The keep decisions of (q, key) and (q, key ^ 1) are the two 16-bit fields of ONE hash (ProbDrop), and lanes l, l ^ 1
                // own such a key pair: the even lane hashes the even query rows of the accumulator, the odd lane the odd ones, each
                // keeps its own field and hands the other one to its neighbour through DPP — 8 hashes per unit instead of 16, the
                // same mask bit for bit.  Which of (own, received) belongs to a given register is a function of the lane parity:
                // resolved on the comparison masks (scalar xor / and), the selects read them directly.
                uint32_t sk2v = pd.sk2;
                asm volatile("" : "+s"(sk2v));             // (or the row offsets are hoisted out of the loop and spilled)
                const uint32_t par = (uint32_t)key & 1u, shm = 16u * par, shs = 16u - shm;
                const uint32_t xbp = pd.row(qb + 4 * half, key) + par * sk2v;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t hsh = pd.hash(xbp + (uint32_t)frag_row(2 * i, 0) * sk2v);
                    const uint32_t mine = (hsh >> shm) & 0xFFFFu, send = (hsh >> shs) & 0xFFFFu;
                    const uint32_t recv = (uint32_t)__builtin_amdgcn_mov_dpp((int)send, 0xB1, 0xF, 0xF, true);      // lane ^ 1
                    const uint64_t cm = __builtin_amdgcn_uicmp(mine, pd.thr, 35), cr = __builtin_amdgcn_uicmp(recv, pd.thr, 35);   // >=
                    const uint64_t u = (cm ^ cr) & 0xAAAAAAAAAAAAAAAAull;
                    const bool k0 = __builtin_amdgcn_inverse_ballot_w64(cm ^ u), k1 = __builtin_amdgcn_inverse_ballot_w64(cr ^ u);
                    const int r0 = 2 * i, r1 = 2 * i + 1;
                    ds[r0] = p[r0] * ((k0 ? dp[r0] : 0.f) - st4[r0 >> 2][r0 & 3]);
                    p[r0] = k0 ? p[r0] : 0.f;
                    ds[r1] = p[r1] * ((k1 ? dp[r1] : 0.f) - st4[r1 >> 2][r1 & 3]);
                    p[r1] = k1 ? p[r1] : 0.f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] = p[r] * (dp[r] - st4[r >> 2][r & 3]);
            }
#endif
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) p8[s2][j] = (__bf16)p[8 * s2 + j];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(dlo[s2 * 2 + db], dhi[s2 * 2 + db]), p8[s2], dv[db], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(qlo[0]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(qhi[0]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(qlo[1]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(qhi[1]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(qlo[2]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(qhi[2]) : "v"(tq0));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(qlo[3]) : "v"(tq1));
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(qhi[3]) : "v"(tq1));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) d8[s2][j] = (__bf16)ds[8 * s2 + j];
#ifdef KK_DKV_STORE_DS
            if (ds_on) {
                const uint32_t so = ds_row + (uint32_t)(qb >> 5) * 2048u;
                uint32_t ln = threadIdx.x;                 // the lane's place in a tile, recomputed per unit (two instructions): kept
                asm volatile("" : "+v"(ln));               // across the loop it was one more live register, spilled and reloaded in here
                const uint32_t ds_lane = ((ln & 31u) << 6) | ((ln & 32u) >> 2);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 v4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v4[e] = d8[g >> 1][4 * (g & 1) + e];
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(kk_u32x2, v4), rds, ds_lane, so + 16 * g, 0);   // (16 g on the scalar side: as lane offsets the four sums were hoisted and spilled)
                }
            }
#endif
            wait_lds();
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(qlo[i]), "+v"(qhi[i]));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(qlo[s2 * 2 + db], qhi[s2 * 2 + db]), d8[s2], dk[db], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // the next unit's row fragments (same tile, or the next tile: landed since this iteration's barrier)
            pref = sub == 0 ? unit_live(qb + 32) : (t + 1 < nt && unit_live(q0 + STEP));
            if (pref) read_rows(sub == 0 ? cur + 4096 : nxt);
        }
        st = st1;
    }
    stamp_(58);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                              // the ring is free
    stamp_(59);
    T *dk0 = static_cast<T *>(a.Out) + ((int64_t)b * a.Sk + kmin) * a.ldout + hh * 64;
    T *dv0 = static_cast<T *>(a.Out2) + ((int64_t)b * a.Sk + kmin) * a.ldout2 + hh * 64;
    char *otile = smem_raw + 36864 + wave * 4608;
    if (!has_hn) {
        store_rows_via_lds(dk0, a.ldout, a.Sk - kmin, dk, a.scale, otile, lane, a.wt);
        store_rows_via_lds(dv0, a.ldout2, a.Sk - kmin, dv, pd.inv_keep, otile, lane, a.wt);
        return;
    }
    const HnGain gnk = hn_load_gain(a.hn[0].gain, half);                                           // (lands under the image DMAs below)
    hn_dma_inputs<256>(a.hn[0], (int64_t)b * a.Sk + kblk, kblk, nrows, hh, smem_raw, wave);       // raw K | cos | sin: 48 KB
    dma_rows128<256>(static_cast<const T *>(a.hn[1].raw) + ((int64_t)b * a.Sk + kblk) * a.hn[1].ldraw + hh * 64, a.hn[1].ldraw, nrows, rawv_img, wave);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp_(60);
    // A wave reads only ITS 32 rows of every image, so what it writes afterwards goes over its own dead rows — the store tile over its
    // raw K / raw V rows, its column sums (hn_colsum32: in registers) over its cos rows — and the four waves meet ONCE, for the 4 x 64
    // partial gain-gradient sums.  (Before: colred[128][65] over everyone's images, four barriers, 128-row sums on one wave: the two
    // epilogues were 6.2 us of a 26.5 us workgroup at 512 x 512, profiles/r05_attn_bwd_pair_stamps.txt.)
    f32x16 dx[2];
    float cr[32];
    float *colpart = reinterpret_cast<float *>(smem_raw + 16384 + wave * 4096);      // [2][64]: this wave's column sums (K | V)
    const int ccol = hn_colsum32_col(l31, half);
    hn_bwd_row2_core(dk, a.scale, kvalid, smem_raw, smem_raw + 16384, smem_raw + 32768, wave * 32 + l31, a.hn[0].rope != 0, gnk, half, cr, dx);
    const HnGain gnv = hn_load_gain(a.hn[1].gain, half);          // (lands under the column sums and the stores of dK)
    const float ck = hn_colsum32(cr, l31);
    store_rows_via_lds16(dk0, a.ldout, a.Sk - kmin, dx, 1.f, smem_raw + wave * 4096, lane, a.wt);
    hn_bwd_row2_core(dv, pd.inv_keep, kvalid, rawv_img, nullptr, nullptr, wave * 32 + l31, false, gnv, half, cr, dx);
    const float cv = hn_colsum32(cr, l31);
    store_rows_via_lds16(dv0, a.ldout2, a.Sk - kmin, dx, 1.f, rawv_img + wave * 4096, lane, a.wt);
    colpart[ccol] = ck;
    colpart[64 + ccol] = cv;
    __syncthreads();
    if (threadIdx.x < 128) {                                      // (the dK/dV half's threads are numbered from 0 in this body)
        const int ps = threadIdx.x >> 6, col = threadIdx.x & 63;
        const float *cp = reinterpret_cast<const float *>(smem_raw + 16384) + ps * 64 + col;
        const float t = (cp[0] + cp[1024]) + (cp[2048] + cp[3072]);
        a.hn[ps].partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 64 + col] = t;
    }
    if (KK_DBG(a, 256)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp_(61); }
