// Attention forward (overview and shared host side: kk_attn.hip): the three generations of forward kernels, the keep-bit generator,
// the decode kernel, and the entry points that launch them.
#include "kk_attn_host.h"
#include "kk_attn_fwd3.h"

using namespace kk_attn;

namespace {

// ------------------------------------------------------------------ forward
// G = 1: 4 waves, every wave sees every key tile.  G = 2: 8 waves (2 per SIMD — the second wave's MFMAs and LDS
// latencies hide under the first one's softmax VALU work and vice versa); wave group g takes the key tiles
// g, g+2, g+4, ... of the same 128 queries with its own running (max, sum, O), and the two partial softmaxes are
// merged through LDS at the end.  Each group stages its own tiles with its own 256 threads.
template <bool BF16, bool ST16, int G>
__global__ __launch_bounds__(256 * G) void attn_fwd_kernel(AttnArgs a) {
    using elem = typename ACfg<BF16>::elem;
    using SG = Stage<BF16, ST16>;
    using T = typename SG::T;
    constexpr int LR = ACfg<BF16>::LR, TILE = 64 * LR;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [buffer][group][K | V]
    elem *smem = reinterpret_cast<elem *>(smem_raw);
    int bx_, by_;
    attn_block(a, bx_, by_, true);                         // (causal: blocks near the end of the sequence see the most keys)
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int wave = wave8 & 3, grp = wave8 >> 2;
    const int q = qblk + wave * 32 + l31;
    const bool qvalid = q < a.Sq;
    RowFrag<BF16> qf;
    load_rowfrag<BF16, T>(qf, qvalid ? static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + q) * a.ldq + hh * 64 : nullptr, half);
    f32x16 o[2];
    zero_acc(o[0]); zero_acc(o[1]);
    float m = -1e30f, l = 0.f;                            // running max in the log2 domain, running sum
    const float c2 = a.scale * 1.4426950408889634f;       // exp(x*scale) = exp2(x*c2)
    ProbDrop pd;
    pd.init(a, b, hh);
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    const int qmin = qblk + wave * 32;                    // smallest query of this wave
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.Sk * a.ldv + hh * 64;
    // Register staging with a prefetch distance of TWO tiles: the kernel is bound by the latency of the K/V loads, not by
    // bandwidth or math (19 us at S=512 with one tile ahead: four dependent ~2 us round trips), so two register sets
    // alternate and a tile's loads have two tile-times to land before they are written to LDS.
    struct Regs {
        typename SG::R rk;
        typename std::conditional<BF16, typename SG::RT, typename SG::R>::type rv;
        uint32_t rkm;                                     // key-mask byte of key (tile start + lane)
    };
    Regs ra, rb;
    ra.rkm = rb.rkm = 0;
    auto issue = [&](Regs &t, int k0) {
        const int nvalid = a.Sk - k0 < 64 ? a.Sk - k0 : 64;
        load_rows(t.rk, Kb + (int64_t)k0 * a.ldk, a.ldk, nvalid);
        if constexpr (BF16) load_rows_T(t.rv, Vb + (int64_t)k0 * a.ldv, a.ldv, nvalid);
        else load_rows(t.rv, Vb + (int64_t)k0 * a.ldv, a.ldv, nvalid);
        t.rkm = km ? (lane < nvalid ? km[k0 + lane] : 0u) : 0u;
    };
    auto commit = [&](const Regs &t, int buf) {
        elem *dst = smem + (buf * G + grp) * 2 * TILE;
        SG::st(dst, t.rk);
        if constexpr (BF16) SG::stT(dst + TILE, t.rv);
        else SG::st(dst + TILE, t.rv);
    };
    constexpr int STEP = 64 * G;                          // this group's tiles: grp*64, grp*64 + STEP, ...
    const int kfirst = grp * 64;
    if (kfirst < kend) {
        issue(ra, kfirst);
        commit(ra, 0);
    }
    uint64_t kmbits = __ballot(ra.rkm != 0u), kmnext = 0;  // bit j: key (tile start + j) is masked (wave-uniform)
    if (kfirst + STEP < kend) issue(ra, kfirst + STEP);         // tile 1 -> set a
    if (kfirst + 2 * STEP < kend) issue(rb, kfirst + 2 * STEP); // tile 2 -> set b
    __syncthreads();
    int cur = 0;
    // one tile: multiply tile k0 from LDS buffer `cur`, then write tile k0+STEP (register set X) to the other buffer and
    // reuse X for tile k0+3*STEP
    auto tile_step = [&](Regs &X, int kk0) {
        const int k0 = kk0 + kfirst;
        const elem *Ks = smem + (cur * G + grp) * 2 * TILE, *Vx = Ks + TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= kend) continue;
            if (a.causal && kb > qmin + 31) continue;
            f32x16 s;
            zero_acc(s);
            mma_tile_x_frag<BF16>(s, Ks, sub * 32, qf, l31, half);
            const uint32_t kmsub = (uint32_t)(kmbits >> (sub * 32));
            // masks are only evaluated on edge sub-tiles: ragged end, causal diagonal, or a masked key among the 32
            const bool edge = kb + 32 > a.Sk || (a.causal && kb + 31 > qmin) || kmsub != 0u;
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = s[r];
            if (edge) {
                const uint32_t kml = kmsub >> (4 * half);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kb + frag_row(r, half);
                    const bool ok = key < a.Sk && !(a.causal && key > q) && !((kml >> frag_row(r, 0)) & 1u);
                    p[r] = ok ? p[r] : -INFINITY;
                }
            }
            float mx = p[0];                               // max of the raw scores; the scale c2 > 0 commutes with max
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, p[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * c2;
            const float mn = fmaxf(m, mx);
            if (__ballot(mn > m) != 0ull) {               // rescale only when some row's maximum moved (wave-uniform)
                const float alpha = __builtin_amdgcn_exp2f(m - mn);
                l *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
                m = mn;
            }
            float rs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(fmaf(p[r], c2, -m)); rs += p[r]; }
            rs += __shfl_xor(rs, 32, 64);
            l += rs;
            if (pd.thr) {                // the row sum l stays un-dropped: softmax first, dropout after; 1/(1-p) at the store
                const uint32_t xb = pd.row(q, kb + 4 * half);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const uint32_t hsh = pd.hash(xb + (uint32_t)(frag_row(r, 0) >> 1));
                    p[r] = pd.keep_lo(hsh) ? p[r] : 0.f;
                    p[r + 1] = pd.keep_hi(hsh) ? p[r + 1] : 0.f;
                }
            }
            mma_T_x_p<BF16>(o, Vx, sub * 32, p, l31, half);
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
    if constexpr (G >= 2) {          // merge the key groups' partial softmaxes: groups 1 .. G-1 -> LDS -> group 0
        float *mb0 = reinterpret_cast<float *>(smem_raw) + (wave * 64 + lane) * 34;     // (the loop's last barrier is behind us)
        constexpr int GSTRIDE = 4 * 64 * 34;                                             // floats per group
        if (grp >= 1) {
            float *mb = mb0 + (grp - 1) * GSTRIDE;
            mb[0] = m; mb[1] = l;
#pragma unroll
            for (int r = 0; r < 16; ++r) { mb[2 + r] = o[0][r]; mb[18 + r] = o[1][r]; }
        }
        __syncthreads();
        if (grp >= 1) return;
#pragma unroll
        for (int g = 1; g < G; ++g) {
            const float *mb = mb0 + (g - 1) * GSTRIDE;
            const float m1 = mb[0], l1 = mb[1], mn = fmaxf(m, m1);
            const float a0 = __builtin_amdgcn_exp2f(m - mn), a1 = __builtin_amdgcn_exp2f(m1 - mn);
            l = l * a0 + l1 * a1;
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] = o[0][r] * a0 + mb[2 + r] * a1; o[1][r] = o[1][r] * a0 + mb[18 + r] * a1; }
        }
    }
    if (qvalid) {
        const float inv = l > 0.f ? pd.inv_keep / l : 0.f;
        store_row<T>(static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + q) * a.ldout + hh * 64, o, inv, half);
        if (half == 0) a.LSEo[((int64_t)b * a.heads + hh) * a.Sq + q] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : INFINITY;
    }
}

// ------------------------------------------------------------------ forward, second generation (bf16 storage)
// Same decomposition and the same arithmetic per score as attn_fwd_kernel<true, true, 2> (bit-identical dropout masks), but
//  * K and V tiles reach LDS by the buffer-load-to-LDS DMA (16 bytes per lane, no VGPR staging, no ds_write pass, no
//    software transpose): K as a [64 keys][64 d] image with XOR-ed 16-byte chunks (conflict-free ds_read_b128 fragments),
//    V exactly as it lies in memory with XOR-ed 32-byte blocks, its V^T fragments read by ds_read_b64_tr_b16 (the
//    hardware 4x16 transpose read) in the key order the accumulator registers hold the probabilities;
//  * NS stages per wave group, one raw s_barrier per 64-key tile, DMA waits by counted vmcnt;
//  * the wave is software-pipelined over 32-key units: the QK^T MFMAs of unit u+1 are issued BEFORE the softmax of
//    unit u, so the matrix pipe works under the VALU phase of the same wave (the first-generation kernel alternated
//    strictly: its phases add up).
template <int NS>
__global__ __launch_bounds__(512) void attn_fwd2_kernel(AttnArgs a) {
    typedef __bf16 T;
    constexpr int KIMG = 64 * 64 * 2, STAGE = 2 * KIMG, GSZ = NS * STAGE, STEP = 128;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];        // [group][stage][K image | V image], key-mask words
    uint64_t *kmb = reinterpret_cast<uint64_t *>(smem_raw + 2 * GSZ);       // [64] one word per 64-key tile
    int bx_, by_;
    attn_block(a, bx_, by_, true);                         // (causal: blocks near the end of the sequence see the most keys)
    const int b = by_ / a.heads, hh = by_ % a.heads;
    const int qblk = bx_ * 128;
    const int lane = threadIdx.x & 63, wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    const int wave = wave8 & 3, grp = wave8 >> 2, tg = threadIdx.x & 255;
    const int q = qblk + wave * 32 + l31;
    const bool qvalid = q < a.Sq;
    const int qmin = qblk + wave * 32;
    int kend = a.Sk;
    if (a.causal && qblk + 128 < kend) kend = qblk + 128;
    int klim = kend;                                       // this wave multiplies the keys [0, klim)
    if (a.causal && qmin + 32 < klim) klim = qmin + 32;
    const int kfirst = grp * 64;
    const int nt = kfirst < kend ? (kend - kfirst + STEP - 1) / STEP : 0;       // this group's tiles
    const int nt0 = (kend + STEP - 1) / STEP;                                   // group 0's: the loop bound (barriers)
    int nu = 0;                                            // this wave's 32-key units: a prefix of the group's
    if (klim > kfirst) {
        const int full = (klim - kfirst) / STEP, rem = (klim - kfirst) - full * STEP;
        nu = 2 * full + (rem > 32 ? 2 : (rem > 0 ? 1 : 0));
    }
    RowFrag<true> qf;
    if (KK_DBG(a, 64)) return;                                // (timing probe: the launch alone)
    // probe (tools builds, bit 256): shader-clock stamps of workgroup 0's waves into the buffer at a.DeltaOut
    unsigned long long *trace = (KK_DBG(a, 256) && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) ? reinterpret_cast<unsigned long long *>(a.DeltaOut) + wave8 * 64 : nullptr;
    auto stamp = [&](int slot) { if (KK_DBG(a, 256) && trace != nullptr && slot < 64) trace[slot] = __builtin_amdgcn_s_memtime(); };
    stamp(0);
    char *qimg = smem_raw + 2 * GSZ + 512;                 // [128 queries][64] image (the oldest DMA: covered by every wait below)
    dma_rows128(static_cast<const T *>(a.Q) + ((int64_t)b * a.Sq + qblk) * a.ldq + hh * 64, a.ldq, a.Sq - qblk < 128 ? a.Sq - qblk : 128, qimg, wave8);
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    uint32_t kmv[8];
    if (km) {                                              // tile T's mask word: wave T % 8 (issued before the DMAs)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = (wave8 + 8 * i) * 64 + lane;
            kmv[i] = key < kend ? km[key] : 0u;
        }
    }
    // ---- DMA
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.Sk * a.ldk + hh * 64;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.Sk * a.ldv + hh * 64;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Kb), 0, (int)((((int64_t)a.Sk - 1) * a.ldk + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Vb), 0, (int)((((int64_t)a.Sk - 1) * a.ldv + 64) * 2), 0x00020000);
    uint32_t kvo[2], vvo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = tg + 256 * j, row = p >> 3, pc = p & 7;
        kvo[j] = (uint32_t)(((int64_t)row * a.ldk + ((pc ^ ((row >> 1) & 7)) * 8)) * 2);
        const int sw = 2 * ((row >> 1) & 1), g = (((pc >> 1) ^ sw) << 1) | (pc & 1);
        vvo[j] = (uint32_t)(((int64_t)row * a.ldv + g * 8) * 2);
    }
    char *gbase = smem_raw + grp * GSZ;
    const uint32_t ktile = (uint32_t)(STEP * a.ldk * 2), vtile = (uint32_t)(STEP * a.ldv * 2);
    const uint32_t kbeg = (uint32_t)(kfirst * a.ldk * 2), vbeg = (uint32_t)(kfirst * a.ldv * 2);
    auto issue_tile = [&](int t, int st) {                 // (offsets in the VGPR: the range check then covers the tile's rows)
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
    uint32_t ka[4], va[2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ka[ks] = (uint32_t)(l31 * 128 + (((2 * ks + half) ^ ((l31 >> 1) & 7)) * 16));
    {
        const int L = lane & 15, kq = L >> 2, gi = (lane >> 4) & 1, sw = 2 * ((kq >> 1) & 1);
#pragma unroll
        for (int db = 0; db < 2; ++db) va[db] = (uint32_t)((4 * half + kq) * 128 + (((2 * db + gi) ^ sw) * 32) + 8 * (L & 3));
    }
    bf16x8 kf[4];
    s16x4 vlo[4], vhi[4];
    // (plain lambdas with literal offsets: inline-asm operands are not captured inside generic lambdas)
    auto read_k = [&](uint32_t img) {                      // img = LDS address of the unit's first K row
        if (KK_DBG(a, 16)) return;
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[0]) : "v"(img + ka[0]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[1]) : "v"(img + ka[1]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[2]) : "v"(img + ka[2]));
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[3]) : "v"(img + ka[3]));
    };
    auto read_v = [&](uint32_t img) {                      // img = LDS address of the unit's first V row
        if (KK_DBG(a, 16)) return;
        const uint32_t a0 = img + va[0], a1 = img + va[1];
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(vlo[0]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(vhi[0]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(vlo[1]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(vhi[1]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(vlo[2]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(vhi[2]) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(vlo[3]) : "v"(a1));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:3072" : "=v"(vhi[3]) : "v"(a1));
    };
    auto wait_lds = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    auto qk = [&](f32x16 &s) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(kf[ks]));
        zero_acc(s);
        if (KK_DBG(a, 4)) { s[0] = (float)kf[0][0] + (float)kf[1][1] + (float)kf[2][2] + (float)kf[3][3]; return; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf.v[ks], s, 0, 0, 0);
    };
    f32x16 o[2];
    zero_acc(o[0]); zero_acc(o[1]);
    float m = -1e30f, l = 0.f;
    const float c2 = a.scale * 1.4426950408889634f;
    ProbDrop pd;
    pd.init(a, b, hh);
    // softmax (+ dropout) of one unit: s -> two B operands of the PV MFMAs; the arithmetic of attn_fwd_kernel
    auto softmax_unit = [&](const f32x16 &s, int kb, uint32_t kmsub, bf16x8 (&pb)[2]) {
        if (KK_DBG(a, 2)) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[s2][j] = (__bf16)s[8 * s2 + j];
            return;
        }
        const bool edge = kb + 32 > a.Sk || (a.causal && kb + 31 > qmin) || kmsub != 0u;
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = s[r];
        if (edge) {
            const uint32_t kml = kmsub >> (4 * half);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb + frag_row(r, half);
                const bool ok = key < a.Sk && !(a.causal && key > q) && !((kml >> frag_row(r, 0)) & 1u);
                p[r] = ok ? p[r] : -INFINITY;
            }
        }
        float mx = p[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, p[r]);
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
        for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(fmaf(p[r], c2, -m)); rs += p[r]; }
        rs = xor32_sum(rs);
        l += rs;
        if (pd.thr) {
            const uint32_t xb = pd.row(q, kb + 4 * half);
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const uint32_t hsh = pd.hash(xb + (uint32_t)(frag_row(r, 0) >> 1));
                p[r] = pd.keep_lo(hsh) ? p[r] : 0.f;
                p[r + 1] = pd.keep_hi(hsh) ? p[r + 1] : 0.f;
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 8; ++j) pb[s2][j] = (__bf16)p[8 * s2 + j];
    };
    auto pv = [&](const bf16x8 (&pb)[2]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vlo[i]), "+v"(vhi[i]));
        if (KK_DBG(a, 4)) { o[0][0] += (float)pb[0][0] + (float)pb[1][0] + (float)vlo[0][0] + (float)vhi[3][0]; return; }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < 2; ++db)
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(vlo[s2 * 2 + db], vhi[s2 * 2 + db]), pb[s2], o[db], 0, 0, 0);
    };
    if (KK_DBG(a, 128)) return;                               // (timing probe: launch + DMA issue, nothing waited for)
    stamp(1);
    // ---- prologue: tiles 0 and 1 landed (tile 2 may stay in flight), unit 0's scores, unit 1's K fragments
    if (NS >= 4 && nt >= 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nt >= 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp(2);
    rowfrag_from_image(qf, qimg, wave * 32, l31, half);
    f32x16 sa, sb;
    if (nu > 0) {
        read_k(gl);
        wait_lds();
        qk(sa);
        if (nu > 1) read_k(gl + 4096);
    }
    stamp(3);
    int st = 0;
    for (int t = 0; t < (KK_DBG(a, 32) ? 0 : nt0); ++t) {
        const int st1 = st + 1 == NS ? 0 : st + 1;
        stamp(4 + 6 * t);
        if (t > 0) {
            // tile t+1 landed: the only DMA younger than it is tile t+2 when NS == 4
            if (NS >= 4 && t + 2 < nt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            stamp(5 + 6 * t);
            if (!KK_DBG(a, 8)) __builtin_amdgcn_s_barrier();                  // ... for every wave, and every wave is done with tile t-1
            asm volatile("" ::: "memory");
            stamp(6 + 6 * t);
            if (t + NS - 1 < nt && !KK_DBG(a, 1)) issue_tile(t + NS - 1, st == 0 ? NS - 1 : st - 1);
            stamp(7 + 6 * t);
        }
        const int u0 = 2 * t;
        if (u0 < nu) {
            const int k0 = kfirst + t * STEP;
            const uint64_t kmbits = km ? kmb[k0 >> 6] : 0ull;
            const uint32_t cur = gl + st * STAGE, nxt = gl + st1 * STAGE;
            bf16x8 pb[2];
            // unit (t, 0): scores in sa; next unit (t, 1) -> sb
            if (u0 + 1 < nu) { wait_lds(); qk(sb); }
            __builtin_amdgcn_sched_barrier(0);
            read_v(cur + KIMG);
            softmax_unit(sa, k0, (uint32_t)kmbits, pb);
            wait_lds();
            pv(pb);
            __builtin_amdgcn_sched_barrier(0);
            stamp(8 + 6 * t);
            if (u0 + 2 < nu) read_k(nxt);
            if (u0 + 1 < nu) {
                // unit (t, 1): scores in sb; next unit (t+1, 0) -> sa
                if (u0 + 2 < nu) { wait_lds(); qk(sa); }
                __builtin_amdgcn_sched_barrier(0);
                read_v(cur + KIMG + 4096);
                softmax_unit(sb, k0 + 32, (uint32_t)(kmbits >> 32), pb);
                wait_lds();
                pv(pb);
                __builtin_amdgcn_sched_barrier(0);
                stamp(9 + 6 * t);
                if (u0 + 3 < nu) read_k(nxt + 4096);
            }
        }
        st = st1;
    }
    stamp(58);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp(59);
    {                                // merge the two key groups' partial softmaxes: group 1 -> LDS -> group 0
        float *mb = reinterpret_cast<float *>(smem_raw) + (wave * 64 + lane) * 34;
        if (grp == 1) {
            mb[0] = m; mb[1] = l;
#pragma unroll
            for (int r = 0; r < 16; ++r) { mb[2 + r] = o[0][r]; mb[18 + r] = o[1][r]; }
        }
        __syncthreads();
        if (grp == 1) return;
        const float m1 = mb[0], l1 = mb[1], mn = fmaxf(m, m1);
        const float a0 = __builtin_amdgcn_exp2f(m - mn), a1 = __builtin_amdgcn_exp2f(m1 - mn);
        l = l * a0 + l1 * a1;
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] = o[0][r] * a0 + mb[2 + r] * a1; o[1][r] = o[1][r] * a0 + mb[18 + r] * a1; }
    }
    stamp(60);
    const float inv = l > 0.f ? pd.inv_keep / l : 0.f;
    store_rows_via_lds(static_cast<T *>(a.Out) + ((int64_t)b * a.Sq + qmin) * a.ldout + hh * 64, a.ldout, a.Sq - qmin, o, inv,
                       smem_raw + 36864 + wave * 4608, lane, a.wt);
    if (qvalid && half == 0) a.LSEo[((int64_t)b * a.heads + hh) * a.Sq + q] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : INFINITY;
    stamp(61);
}

// attn_fwd2_kernel is this unit's only caller of dma_rows128<512>, always with the same LDS image (its Q image).  The compiler propagates
// a lone call site's constant argument into the helper before it inlines it, and the kernel's other use of that address
// (rowfrag_from_image) is then left as a flat-to-LDS round trip: 7 more scalar instructions in the prologue, other operand orders
// behind them (docs/LAB_NOTES.md, "Cutting kk_attn.hip").  While the backward kernels shared the module the helper had several
// callers; this second call site, never executed, keeps the kernel's code what it was measured as.
__device__ __attribute__((used)) void attn_fwd2_dma_second_caller(const __bf16 *base, int64_t ld, int nrows, char *img, int wave8) {
    dma_rows128(base, ld, nrows, img, wave8);
}

// (plain kernels around the template body: hipcc's host pass did not emit the stub of the kernel TEMPLATE named in kk_attn_fwd, and
// rejected its explicit instantiation — the same host-pass trouble as g16x_group_kernel in kk_gemm16x.hip)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd3_q128_kernel(AttnArgs a) { KK_WG_STAMP(a); attn_fwd3_body<4, 2, 3>(a); }
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd3_q64_kernel(AttnArgs a) { KK_WG_STAMP(a); attn_fwd3_body<2, 4, 2>(a); }
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd3_q128r_kernel(AttnArgs a) { KK_WG_STAMP(a); attn_fwd3_body<4, 2, 3, false, true>(a); }
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd3_q64r_kernel(AttnArgs a) { KK_WG_STAMP(a); attn_fwd3_body<2, 4, 2, false, true>(a); }

// ------------------------------------------------------------------ keep-bit generator (kk_attn_keep_gen)
// The dropout keep decisions of up to 16 attention launches as ONE pure-vector launch (no LDS): per 32 x 32 unit the 512 hashes the
// forward evaluates for it, stored as the same 16 ballots in the same layout (AttnArgs::keep).
// Issued on the decoder-head stream beside the persistent encoder forward, which is latency-bound and leaves the vector ALUs idle.
struct KeepGenArgs {
    KkKeepSite s[16];
    int64_t start[17];               // first unit of each site in the flattened unit list
    int n;
    const uint32_t *seed;
    uint32_t seed_offset;            // the bits are those of seed value *seed + seed_offset (1: the NEXT micro-batch's, generated beside the optimizer pass)
};
// Lane-local on purpose: a lane owns one (unit, key pair) — 16 lanes per unit, four units per wave — walks the unit's 32 queries,
// and builds the two dwords of that key pair (even key, odd key) bit by bit: the same 512 hashes per unit the forward's 64 lanes
// evaluate, but no ballots, no v_writelane, nothing wave-wide.  (A first version mirrored the forward — compare masks moved into one
// register by v_writelane — and wrote stale words whenever it ran beside other kernels: the compares that produce those SGPRs sat
// right in front of the inline-asm v_writelanes, where the hazard recogniser does not look.)
__global__ __launch_bounds__(256) void attn_keep_gen_kernel(const KeepGenArgs g) {
    const int lane = threadIdx.x & 63, j = lane & 15, hbit = j & 1, rr = j >> 1;
    const int64_t nquads = (int64_t)gridDim.x * 4, total = g.start[g.n];
    const uint32_t seed = *g.seed + g.seed_offset;
    const int kp_off = ((rr & 1) + 4 * (rr >> 1));               // frag_row(2 rr, 0) >> 1: the key pair of accumulator registers 2 rr, 2 rr + 1
    for (int64_t u0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4; u0 < total; u0 += nquads * 4) {
        const int64_t u = u0 + (lane >> 4);
        if (u >= total) continue;
        int i = 0;
        while (i + 1 < g.n && u >= g.start[i + 1]) ++i;
        const KkKeepSite &st = g.s[i];
        const int nQU = (st.Sq + 31) >> 5, nKU = (st.Sk + 31) >> 5;
        const int64_t v = u - g.start[i];
        const int ku = (int)(v % nKU), qu = (int)((v / nKU) % nQU), bh = (int)(v / ((int64_t)nKU * nQU));
        if (st.causal && ku > qu) continue;                    // (the forward never visits a unit above the diagonal)
        uint32_t thr = (uint32_t)(st.p * 65536.f + 0.5f);
        thr = thr > 65535u ? 65535u : thr;
        const uint32_t key = kk_hash(seed, st.site, (uint64_t)bh), sk2 = (uint32_t)(st.Sk + 1) >> 1;
        // the forward's lane (l31 = query, half) hashes  q * sk2 + ((k0 + 4 half) >> 1) + (frag_row(r, 0) >> 1)  for r = 0, 2, ..., 14
        uint32_t x0 = (uint32_t)(qu * 32) * sk2 + ((uint32_t)(ku * 32 + 4 * hbit) >> 1) + (uint32_t)kp_off;
        uint32_t lo = 0u, hi = 0u;
// (unrolled by 2: 39 registers, so that TWO waves of this kernel fit a SIMD beside the persistent encoder's two 216-register waves — 432 + 2 x 40 = 512;
//  unrolled by 8 it held 60 and fit one: -0.2 % of the step at 8 x 512 and -0.7 % at 8 x 1024 for the same bits, profiles/r06_keep_bits_gen_ab.txt)
#ifndef KK_KEEPGEN_UNROLL
#define KK_KEEPGEN_UNROLL 2
#endif
#pragma unroll KK_KEEPGEN_UNROLL
        for (int q = 0; q < 32; ++q) {
            uint32_t x = x0 ^ key;
            x ^= x >> 16; x = __umul24(x, 0xb5352du); x ^= x >> 13; x = __umul24(x, 0xca68b5u); x ^= x >> 16;
            lo |= ((x & 0xFFFFu) >= thr ? 1u : 0u) << q;           // even key: register 2 rr
            hi |= ((x >> 16) >= thr ? 1u : 0u) << q;               // odd key:  register 2 rr + 1
            x0 += sk2;
        }
        uint32_t *unit = reinterpret_cast<uint32_t *>(static_cast<char *>(st.keep) + (((int64_t)bh * nQU + qu) * nKU + ku) * 128);
        unit[2 * (2 * rr) + hbit] = lo;                        // dword 2 r + half = the ballot half of register r
        unit[2 * (2 * rr + 1) + hbit] = hi;
    }
}

// ------------------------------------------------------------------ decode: one query per (row, head)
// Sq == 1 (the incremental path of transformers.py:237-253: a decoder step against the KV cache / against the memory), no dropout.
// The tiled kernels above would run one live row of a 128-row block; here a workgroup is one (row, head): 16 waves = 256 key groups
// x 4 lanes (16 of the 64 dims each), scores kept in LDS between the two passes (max, then exp / sum / P.V), fp32 throughout.
// Two callers: kk_attn_fwd at Sq = 1 (every row over all Sk keys, rows Sk * ld apart) and kk_attn_decode_rows (row b over its first
// klen[b] keys, explicit slot strides; nothing at or past klen[b] is loaded).  One kernel, so a key count and the equivalent key mask
// give the same bits.
constexpr int DECODE_MAX_KEYS = 8192;                                     // (the LDS score array holds Sk floats)
struct DecodeArgs {
    const void *Q, *K, *V;
    void *Out;
    float *LSEo;
    const int *klen;                                                      // keys of row b, clamped to [0, Sk]; nullptr: Sk for every row
    const uint8_t *key_mask;
    int heads, Sk;
    int64_t ldq, k_slot, ldk, v_slot, ldv, ldout;                         // row b of Q / K / V / Out at b * ldq / k_slot / v_slot / ldout
    float scale;
};

template <typename T>
__global__ __launch_bounds__(1024) void attn_decode_kernel(DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];          // [Sk] scores | [16 waves][64] partial outputs | [32] reductions
    float *sc = dsm, *part = dsm + ((a.Sk + 3) & ~3), *red = part + 16 * 64;
    const int b = blockIdx.x / a.heads, hh = blockIdx.x % a.heads;
    const int tid = threadIdx.x, kg = tid >> 2, dq = (tid & 3) * 16, lane = tid & 63, wave = tid >> 6;
    int n = a.Sk;                                                         // (the same in every lane of the workgroup)
    if (a.klen) {
        n = a.klen[b];
        n = n < 0 ? 0 : (n > a.Sk ? a.Sk : n);
    }
    const T *Q = static_cast<const T *>(a.Q) + (int64_t)b * a.ldq + hh * 64 + dq;
    const T *Kb = static_cast<const T *>(a.K) + (int64_t)b * a.k_slot + hh * 64 + dq;
    const T *Vb = static_cast<const T *>(a.V) + (int64_t)b * a.v_slot + hh * 64 + dq;
    const uint8_t *km = a.key_mask ? a.key_mask + (int64_t)b * a.Sk : nullptr;
    float qv[16];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
        const float4 t = ldv4<T>(Q + i);
        qv[i] = t.x; qv[i + 1] = t.y; qv[i + 2] = t.z; qv[i + 3] = t.w;
    }
    const float c2 = a.scale * 1.4426950408889634f;
    float mx = -INFINITY;
#pragma unroll 2
    for (int j = kg; j < n; j += 256) {                                   // 256 key groups x 4 lanes (16 of the 64 dims each)
        const bool masked = km && km[j];
        float d = 0.f;
        if (!masked) {
            const T *kr = Kb + (int64_t)j * a.ldk;
            float4 t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = ldv4<T>(kr + 4 * i);
#pragma unroll
            for (int i = 0; i < 4; ++i) d += qv[4 * i] * t[i].x + qv[4 * i + 1] * t[i].y + qv[4 * i + 2] * t[i].z + qv[4 * i + 3] * t[i].w;
        }
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d = masked ? -INFINITY : d * c2;
        if ((tid & 3) == 0) sc[j] = d;
        mx = fmaxf(mx, d);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    const float mm = fmaxf(m, -1e30f);
    float acc[16], l = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int j = kg; j < n; j += 256) {
        const float s = sc[j];
        if (s == -INFINITY) continue;
        const T *vr = Vb + (int64_t)j * a.ldv;
        float4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = ldv4<T>(vr + 4 * i);
        const float pj = __builtin_amdgcn_exp2f(s - mm);
        l += pj;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[4 * i] += pj * t[i].x; acc[4 * i + 1] += pj * t[i].y; acc[4 * i + 2] += pj * t[i].z; acc[4 * i + 3] += pj * t[i].w;
        }
    }
    // the 16 key groups of a wave (lanes with the same dims: lane ^ 4, 8, 16, 32), then the 16 waves through LDS
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) acc[i] += __shfl_xor(acc[i], o, 64);
    }
    if (lane < 4) {
#pragma unroll
        for (int i = 0; i < 16; ++i) part[wave * 64 + dq + i] = acc[i];
    }
    l = wave_sum(l) * 0.25f;                                              // (the 4 lanes of a key group hold the same p)
    if (lane == 0) red[16 + wave] = l;
    __syncthreads();
    if (tid < 64) {
        float lt = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) { lt += red[16 + w]; o += part[w * 64 + tid]; }
        o = lt > 0.f ? o / lt : 0.f;
        T *out = static_cast<T *>(a.Out) + (int64_t)b * a.ldout + hh * 64 + tid;
        *out = (T)o;
        if (tid == 0) a.LSEo[(int64_t)b * a.heads + hh] = lt > 0.f ? (mm + __builtin_amdgcn_logf(lt)) * 0.6931471805599453f : INFINITY;
    }
}

void launch_decode(const DecodeArgs &a, int rows, int bf16, hipStream_t s) {
    const size_t lds = (size_t)(((a.Sk + 3) & ~3) + 16 * 64 + 32) * sizeof(float);          // (as the kernel carves dsm)
    if (bf16) hipLaunchKernelGGL(attn_decode_kernel<__bf16>, dim3(rows * a.heads), dim3(1024), lds, s, a);
    else hipLaunchKernelGGL(attn_decode_kernel<float>, dim3(rows * a.heads), dim3(1024), lds, s, a);
}

}  // namespace

// Whether a forward launch of this shape stores keep bits (the third-generation kernels) and how many bytes they take; 0 = no.
extern "C" int64_t kk_attn_keep_bytes(int B, int heads, int Sq, int Sk) {
    if (B <= 0 || heads <= 0 || Sq <= 0 || Sk <= 128 || Sk > 4096 || g_attn_groups != 2 || !(attn_v2_mask() & 1)) return 0;
    const int64_t per_head = (int64_t)kk_cdiv(Sq, 32) * kk_cdiv(Sk, 32) * 128;
    return per_head < (1ll << 31) ? (int64_t)B * heads * per_head : 0;
}

// The NEXT third-generation forward launch of this thread also warms these (up to two) read-only matrices into every XCD's L2 (see
// AttnArgs::warm).  One-shot: consumed by that launch, dropped by any other forward launch.
extern "C" int kk_attn_warm_next(const void *w0, int64_t bytes0, const void *w1, int64_t bytes1) {
    g_warm_ptr[0] = w0; g_warm_bytes[0] = (w0 && bytes0 > 0 && bytes0 < (1ll << 31)) ? (uint32_t)bytes0 : 0u;
    g_warm_ptr[1] = w1; g_warm_bytes[1] = (w1 && bytes1 > 0 && bytes1 < (1ll << 31)) ? (uint32_t)bytes1 : 0u;
    if (g_warm_bytes[0] == 0u) { g_warm_ptr[0] = g_warm_ptr[1]; g_warm_bytes[0] = g_warm_bytes[1]; g_warm_bytes[1] = 0u; }
    return 0;
}

static int attn_fwd_impl(const float *Q, const float *K, const float *V, float *O, float *LSE, int B, int heads,
                         int Sq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                         const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site,
                         float p_drop, int math, int io_bf16, void *keep, void *stream, int keep_rd = 0) {
    KK_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "kk_attn_fwd: dropout probability must be in [0,1)");
    KK_REQUIRE(!io_bf16 || math == KK_MATH_BF16, "kk_attn_fwd: bf16 storage needs KK_MATH_BF16");
    const int64_t lds[4] = {ldq, ldk, ldv, ldo};
    if (int rc = check_common("kk_attn_fwd", B, heads, Sq, Sk, math, lds, 4)) return rc;
    AttnArgs a = attn_args(Q, K, V, B, heads, Sq, Sk, ldq, ldk, ldv, key_mask, causal, scale, seed, site, p_drop);
    a.Out = O; a.LSEo = LSE; a.ldout = ldo;
    a.keep = keep;
    a.keep_rd = (keep_rd && keep != nullptr && a.seed != nullptr) ? 1 : 0;
    a.warm[0] = g_warm_ptr[0]; a.warm[1] = g_warm_ptr[1];
    a.warm_bytes[0] = g_warm_bytes[0]; a.warm_bytes[1] = g_warm_bytes[1];
    g_warm_bytes[0] = g_warm_bytes[1] = 0u;                     // (one-shot)
#ifdef KK_TUNING_HOOKS
    if (a.dbg & (256 | 4096)) a.DeltaOut = static_cast<float *>(g_attn_trace);
#endif
    if (Sq == 1 && a.seed == nullptr && !causal && Sk <= DECODE_MAX_KEYS && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 &&
        (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) == 0) {  // a decoder step of the incremental path: one (batch, head) per workgroup
        DecodeArgs d;
        d.Q = Q; d.K = K; d.V = V; d.Out = O; d.LSEo = LSE; d.klen = nullptr; d.key_mask = key_mask;
        d.heads = heads; d.Sk = Sk; d.ldq = ldq; d.k_slot = (int64_t)Sk * ldk; d.ldk = ldk; d.v_slot = (int64_t)Sk * ldv; d.ldv = ldv;
        d.ldout = ldo; d.scale = scale;
        launch_decode(d, B, io_bf16, (hipStream_t)stream);
        KK_LAUNCH_CHECK("kk_attn_fwd");
        return 0;
    }
    dim3 grid(kk_cdiv(Sq, 128), B * heads);
    const int G = (Sk > 64 && g_attn_groups == 2) ? 2 : 1;          // one key tile: nothing to split
    // second-generation kernel (DMA-staged, software-pipelined): bf16 storage, two key groups, 16-byte aligned operands
    const int fwd_v2 = attn_v2_mask() & 1;
    if (io_bf16 && fwd_v2 && G == 2 && Sk <= 4096 && al16_all({Q, K, V, O}) && dma_bytes(Sk, ldk, ldv)) {
        // third generation: two 74 KB / 128-register workgroups per CU.  128-query blocks x 2 key slots when that gives two workgroups
        // per CU, else 64-query blocks x 4 key slots (a 512-frame launch: 512 workgroups instead of 256)
        static const int fwd3 = kk_tune_env("KK_ATTN_FWD3", 1);
        if (fwd3 && Sk > 128) {
            const bool q128 = (int64_t)kk_cdiv(Sq, 128) * B * heads >= 2 * g_attn_cus() || fwd3 == 2;    // (two workgroups per CU)
            const dim3 g128(kk_cdiv(Sq, 128), B * heads), g64(kk_cdiv(Sq, 64), B * heads);
            const size_t lds128 = (size_t)3 * 16384 + 512 + 16384, lds64 = (size_t)2 * 32768 + 512 + 8192;
            const struct { void (*kernel)(AttnArgs); const char *name; dim3 grid; size_t lds; } variant[2][2] = {      // [q128][keep_rd]
                {{attn_fwd3_q64_kernel, "attn_fwd3_q64", g64, lds64}, {attn_fwd3_q64r_kernel, "attn_fwd3_q64r", g64, lds64}},
                {{attn_fwd3_q128_kernel, "attn_fwd3_q128", g128, lds128}, {attn_fwd3_q128r_kernel, "attn_fwd3_q128r", g128, lds128}}};
            const auto &v = variant[q128][a.keep_rd];
            kk_note_kernel(v.name);
            if (!a.keep_rd && kk_capture(kk_last_kernel(), a, v.grid, 512, v.lds)) return 0;      // (kk_chain.hip has no phase that reads keep bits)
            if (int rc = launch_attn(v.kernel, v.grid, 2, v.lds, (hipStream_t)stream, a)) return rc;
            KK_LAUNCH_CHECK(a.keep_rd ? "kk_attn_fwd_rb" : "kk_attn_fwd");
            return 0;
        }
        KK_REQUIRE(keep == nullptr, "kk_attn_fwd_kb / _rb: only the third-generation forward stores or reads keep bits (ask kk_attn_keep_bytes)");
        static const int ns2 = kk_tune_env("KK_ATTN_NS", 3);
        kk_note_kernel("attn_fwd2");
#ifdef KK_TUNING_HOOKS
        int rc2 = ns2 == 4 ? launch_attn(attn_fwd2_kernel<4>, grid, 2, (size_t)2 * 4 * 16384 + 512 + 16384, (hipStream_t)stream, a)
                           : launch_attn(attn_fwd2_kernel<3>, grid, 2, (size_t)2 * 3 * 16384 + 512 + 16384, (hipStream_t)stream, a);
#else
        (void)ns2;
        int rc2 = launch_attn(attn_fwd2_kernel<3>, grid, 2, (size_t)2 * 3 * 16384 + 512 + 16384, (hipStream_t)stream, a);
#endif
        if (rc2) return rc2;
        KK_LAUNCH_CHECK("kk_attn_fwd");
        return 0;
    }
    KK_REQUIRE(keep == nullptr, "kk_attn_fwd_kb: this launch (storage, alignment or shape) does not take the third-generation forward, which alone stores keep bits");
    kk_note_kernel("attn_fwd");
    if (io_bf16) KK_ATTN_LAUNCH(attn_fwd_kernel, true, true, G, 2);
    else if (math == KK_MATH_BF16) KK_ATTN_LAUNCH(attn_fwd_kernel, true, false, G, 2);
    else KK_ATTN_LAUNCH(attn_fwd_kernel, false, false, G, 2);
    KK_LAUNCH_CHECK("kk_attn_fwd");
    return 0;
}

extern "C" int kk_attn_fwd(const float *Q, const float *K, const float *V, float *O, float *LSE, int B, int heads,
                           int Sq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                           const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site,
                           float p_drop, int math, int io_bf16, void *stream) {
    return attn_fwd_impl(Q, K, V, O, LSE, B, heads, Sq, Sk, ldq, ldk, ldv, ldo, key_mask, causal, scale, seed, site, p_drop, math, io_bf16,
                         nullptr, stream);
}
// kk_attn_fwd that also stores the dropout keep decisions (AttnArgs::keep; kk_attn_keep_bytes(B, heads, Sq, Sk) bytes, > 0 required)
extern "C" int kk_attn_fwd_kb(const float *Q, const float *K, const float *V, float *O, float *LSE, int B, int heads,
                              int Sq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                              const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site,
                              float p_drop, int math, int io_bf16, void *keep, void *stream) {
    KK_REQUIRE(keep == nullptr || (al16(keep) && kk_attn_keep_bytes(B, heads, Sq, Sk) > 0), "kk_attn_fwd_kb: no keep bits for this shape (kk_attn_keep_bytes) or unaligned buffer");
    return attn_fwd_impl(Q, K, V, O, LSE, B, heads, Sq, Sk, ldq, ldk, ldv, ldo, key_mask, causal, scale, seed, site, p_drop, math, io_bf16,
                         keep, stream);
}

// kk_attn_fwd whose dropout keep decisions are READ from `keep` (filled by kk_attn_keep_gen for the same seed value, site, p and shape):
// same output bits as kk_attn_fwd / kk_attn_fwd_kb
extern "C" int kk_attn_fwd_rb(const float *Q, const float *K, const float *V, float *O, float *LSE, int B, int heads,
                              int Sq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                              const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site,
                              float p_drop, int math, int io_bf16, const void *keep, void *stream) {
    KK_REQUIRE(keep != nullptr && al16(keep) && kk_attn_keep_bytes(B, heads, Sq, Sk) > 0 && p_drop > 0.f && seed != nullptr && io_bf16,
               "kk_attn_fwd_rb: needs dropout, bf16 storage and a keep-bit array of a shape that has one (kk_attn_keep_bytes)");
    return attn_fwd_impl(Q, K, V, O, LSE, B, heads, Sq, Sk, ldq, ldk, ldv, ldo, key_mask, causal, scale, seed, site, p_drop, math, io_bf16,
                         const_cast<void *>(keep), stream, 1);
}

// The decode kernel of kk_attn_fwd's Sq = 1 path with a key count per row and explicit slot strides (KokoroEngine.generate_stream: slot s
// of a pool at its own frame): q, out [S, heads * 64].
extern "C" int kk_attn_decode_rows(const void *q, const void *K, const void *V, void *out, float *lse, const int *klen,
                                   const uint8_t *key_mask, int S, int heads, int Sk, int64_t k_slot, int64_t ldk, int64_t v_slot,
                                   int64_t ldv, float scale, int bf16, void *stream) {
    static_assert(DECODE_MAX_KEYS == 8192, "the message below names the limit");
    KK_REQUIRE(q && K && V && out && lse && klen && S > 0 && heads > 0 && Sk > 0 && Sk <= DECODE_MAX_KEYS, "kk_attn_decode_rows: bad args (Sk <= 8192)");
    KK_REQUIRE(ldk % 4 == 0 && ldv % 4 == 0 && k_slot % 4 == 0 && v_slot % 4 == 0 && ldk >= (int64_t)heads * 64 && ldv >= (int64_t)heads * 64,
               "kk_attn_decode_rows: strides must be multiples of 4 elements and hold a frame");
    KK_REQUIRE((((uintptr_t)q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)out) & 15) == 0, "kk_attn_decode_rows: operands must be 16-byte aligned");
    DecodeArgs d;
    d.Q = q; d.K = K; d.V = V; d.Out = out; d.LSEo = lse; d.klen = klen; d.key_mask = key_mask;
    d.heads = heads; d.Sk = Sk; d.ldq = d.ldout = (int64_t)heads * 64; d.k_slot = k_slot; d.ldk = ldk; d.v_slot = v_slot; d.ldv = ldv;
    d.scale = scale;
    launch_decode(d, S, bf16, (hipStream_t)stream);
    KK_LAUNCH_CHECK("kk_attn_decode_rows");
    return 0;
}

// The keep bits of n <= 16 attention launches in one launch (see attn_keep_gen_kernel); sites: HOST array read during the call.
extern "C" int kk_attn_keep_gen(const KkKeepSite *sites, int n, const uint32_t *seed, int seed_offset, int max_workgroups, void *stream) {
    KK_REQUIRE(sites != nullptr && seed != nullptr && n > 0 && n <= 16, "kk_attn_keep_gen: 1..16 sites and the seed are required");
    KeepGenArgs g;
    g.n = n;
    g.seed = seed;
    g.seed_offset = (uint32_t)seed_offset;
    g.start[0] = 0;
    for (int i = 0; i < n; ++i) {
        const KkKeepSite &st = sites[i];
        KK_REQUIRE(st.keep != nullptr && al16(st.keep) && st.p > 0.f && st.p < 1.f && kk_attn_keep_bytes(st.B, st.heads, st.Sq, st.Sk) > 0,
                   "kk_attn_keep_gen: site %d has no keep-bit array (kk_attn_keep_bytes) or no dropout", i);
        g.s[i] = st;
        g.start[i + 1] = g.start[i] + (int64_t)st.B * st.heads * kk_cdiv(st.Sq, 32) * kk_cdiv(st.Sk, 32);
    }
    int64_t wgs = (g.start[n] + 15) / 16;                         // (a wave takes four units at a time)
    const int cap = max_workgroups > 0 ? max_workgroups : 2048;   // (thin: it runs beside another launch and must leave it its wave slots)
    if (wgs > cap) wgs = cap;
    kk_note_kernel("attn_keep_gen");
    hipLaunchKernelGGL(attn_keep_gen_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, g);
    KK_LAUNCH_CHECK("kk_attn_keep_gen");
    return 0;
}
