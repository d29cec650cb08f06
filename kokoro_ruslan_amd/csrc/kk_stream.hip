// Continuous batching of the autoregressive decode: KokoroEngine.generate_stream.  A pool of S slots of `cap` frames each; every slot
// carries its own frame index t_s, so a finished row's slot is refilled while the others go on, and the step's launches (their
// arguments depend on (S, cap) alone) are replayed from one captured hipGraph for the whole call.
//
//  attention, rows    one query per (slot, head) over the slot's first klen[s] keys                  transformers.py:237-253
//  prologue, rows     the step's input frame, positional row and RoPE rows of every slot at its t_s    model.py:541-545
//  cache append, rows row t_s of the slot-major K / V caches [S][cap][H]
//  epilogue, slots    frame and stop logit filed under t_s, the stop rule of ONE row                   model/generator.py:67-88
//  slot admit         cross-attention K|V, frame mask and counters of newly admitted rows
//
// State is int32 throughout (t_rows, done, frames, klen, the three bounds): the host reads done | frames in one copy.
#include "kk_common.h"
#include "kk_stop_rule.h"

namespace {

// ------------------------------------------------------------------ decode attention with a per-row key count
// attn_decode_kernel (kk_attn_fwd.hip) with the key loops bounded by klen[s] instead of Sk and explicit slot strides: 1024 threads, key j in
// group j % 256, 4 lanes x 16 dims, scores in LDS between the max pass and the exp / P.V pass, the same shuffle and LDS reduction
// order — so a row's bits are those of kk_attn_fwd at Sq = 1 over the same live keys.  Nothing at or past klen[s] is loaded.
struct RowsArgs {
    const void *Q, *K, *V;
    void *Out;
    float *LSEo;
    const int *klen;
    const uint8_t *key_mask;
    int heads, Sk;
    int64_t k_slot, ldk, v_slot, ldv;
    float scale;
};

template <typename T>
__global__ __launch_bounds__(1024) void attn_decode_rows_kernel(RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];          // [Sk] scores | [16 waves][64] partial outputs | [32] reductions
    float *sc = dsm, *part = dsm + ((a.Sk + 3) & ~3), *red = part + 16 * 64;
    const int b = blockIdx.x / a.heads, hh = blockIdx.x % a.heads;
    const int tid = threadIdx.x, kg = tid >> 2, dq = (tid & 3) * 16, lane = tid & 63, wave = tid >> 6;
    const int64_t H = (int64_t)a.heads * 64;
    int n = a.klen[b];
    n = n < 0 ? 0 : (n > a.Sk ? a.Sk : n);                                // (the LDS score array holds Sk entries)
    const T *Q = static_cast<const T *>(a.Q) + (int64_t)b * H + hh * 64 + dq;
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
        T *out = static_cast<T *>(a.Out) + (int64_t)b * H + hh * 64 + tid;
        *out = (T)o;
        if (tid == 0) a.LSEo[(int64_t)b * a.heads + hh] = lt > 0.f ? (mm + __builtin_amdgcn_logf(lt)) * 0.6931471805599453f : INFINITY;
    }
}

// ------------------------------------------------------------------ prologue: one workgroup per slot
// A finished (or idle) slot is fed position 0 and its own mel row 0, and gets klen = 0: its row of the step computes finite values
// that nothing reads.
__global__ __launch_bounds__(256) void decode_prologue_rows_kernel(
    const float *__restrict__ mel_all, float *__restrict__ frame_in, const float *__restrict__ pe, float *__restrict__ pe_rows,
    const float *__restrict__ cos_t, const float *__restrict__ sin_t, float *__restrict__ cos_rows, float *__restrict__ sin_rows,
    const int *__restrict__ t_rows, const int *__restrict__ done, int *__restrict__ klen, int L1, int M, int H, int n_pos) {
    const int s = blockIdx.x;
    int t = t_rows[s];
    const bool live = done[s] == 0 && t >= 0 && t + 1 < L1 && t < n_pos;
    if (!live) t = 0;
    for (int c = threadIdx.x; c < M; c += 256) frame_in[(int64_t)s * M + c] = mel_all[((int64_t)s * L1 + t) * M + c];
    for (int c = threadIdx.x; c < H; c += 256) pe_rows[(int64_t)s * H + c] = pe[(int64_t)t * H + c];
    for (int c = threadIdx.x; c < 64; c += 256) {
        cos_rows[s * 64 + c] = cos_t[(int64_t)t * 64 + c];
        sin_rows[s * 64 + c] = sin_t[(int64_t)t * 64 + c];
    }
    if (threadIdx.x == 0) klen[s] = live ? t + 1 : 0;
}

// the step's normalised q | k | v [S, 3H] -> q [S, H] and row t_s of slot s of the slot-major K and V caches [S][cap][H]
template <typename T>
__global__ __launch_bounds__(256) void decode_cache_append_rows_kernel(const T *__restrict__ nrm, T *__restrict__ q, T *__restrict__ kc,
                                                                       T *__restrict__ vc, const int *__restrict__ t_rows,
                                                                       const int *__restrict__ done, int S, int cap, int H) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < S * H; i += gridDim.x * 256) {
        const int s = i / H, c = i - s * H;
        const int t = t_rows[s];
        if (done[s] || t < 0 || t >= cap) continue;
        const T *src = nrm + (int64_t)s * 3 * H + c;
        const int64_t row = ((int64_t)s * cap + t) * H + c;
        q[i] = src[0];
        kc[row] = src[H];
        vc[row] = src[2 * H];
    }
}

// ------------------------------------------------------------------ epilogue: one wave per slot
// decode_epilogue_rows_kernel (kk_synth.hip) with a frame index per slot: the same decode_row_file_and_stop (kk_stop_rule.h) at t_s.
__global__ __launch_bounds__(64) void decode_epilogue_slots_kernel(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_all,
    int *__restrict__ t_rows, int *__restrict__ done, int *__restrict__ frames, int *__restrict__ live,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int L1, int M,
    float stop_threshold, float post_expected_stop_threshold) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (done[b]) return;
    const int t = t_rows[b];
    if (t < 0 || t + 1 >= L1) {                                           // no room for another frame: the row ends where it is
        if (lane == 0) { done[b] = 1; frames[b] = t < 0 ? 0 : t; atomicSub(live, 1); }
        return;
    }
    const bool fin = decode_row_file_and_stop(frame_out, stop, mel_all, stop_all + (int64_t)b * (L1 - 1) + t, min_b, expected_b, max_b,
                                              b, t, lane, L1, M, stop_threshold, post_expected_stop_threshold);
    if (lane == 0) {
        t_rows[b] = t + 1;
        if (fin) {
            done[b] = 1;
            frames[b] = t + 1;
            atomicSub(live, 1);
        }
    }
}

// ------------------------------------------------------------------ admission of n rows into their slots
// kv_src [n*T_adm, W16] (16-byte units per frame) -> rows [slot*cap, slot*cap + T_adm) of kv_pool; frame mask row; counters; mel row 0.
// The entries of slot_of must be distinct (two rows of one group in the same slot would race on its pool rows and counters); the
// caller admits into free slots only.  *live counts the occupied, unfinished slots for tools and tests; the engine reads done | frames.
__global__ __launch_bounds__(256) void slot_admit_kernel(const uint4 *__restrict__ kv_src, uint4 *__restrict__ kv_pool,
                                                         const uint8_t *__restrict__ fm_src, uint8_t *__restrict__ fm_pool,
                                                         const int *__restrict__ slot_of, const int *__restrict__ bounds,
                                                         int *__restrict__ t_rows, int *__restrict__ done, int *__restrict__ frames,
                                                         int *__restrict__ clen, int *__restrict__ min_b, int *__restrict__ expected_b,
                                                         int *__restrict__ max_b, float *__restrict__ mel_all, int *__restrict__ live,
                                                         int n, int T_adm, int S, int cap, int W16, int L1, int M) {
    const int64_t per_row = (int64_t)T_adm * W16, total = (int64_t)n * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / per_row);
        const int slot = slot_of[r];
        if (slot < 0 || slot >= S) continue;
        kv_pool[(int64_t)slot * cap * W16 + (i - (int64_t)r * per_row)] = kv_src[i];
    }
    if (blockIdx.x >= n) return;                                         // (the grid has at least n workgroups)
    const int r = blockIdx.x, slot = slot_of[r];
    if (slot < 0 || slot >= S) return;
    for (int j = threadIdx.x; j < cap; j += 256) fm_pool[(int64_t)slot * cap + j] = j < T_adm ? fm_src[(int64_t)r * T_adm + j] : (uint8_t)1;
    for (int c = threadIdx.x; c < M; c += 256) mel_all[(int64_t)slot * L1 * M + c] = 0.f;
    if (threadIdx.x == 0) {
        t_rows[slot] = 0;
        frames[slot] = 0;
        clen[slot] = T_adm;
        min_b[slot] = bounds[r];
        expected_b[slot] = bounds[n + r];
        max_b[slot] = bounds[2 * n + r];
        done[slot] = 0;
        atomicAdd(live, 1);
    }
}

}  // namespace

extern "C" int kk_attn_decode_rows(const void *q, const void *K, const void *V, void *out, float *lse, const int *klen,
                                   const uint8_t *key_mask, int S, int heads, int Sk, int64_t k_slot, int64_t ldk, int64_t v_slot,
                                   int64_t ldv, float scale, int bf16, void *stream) {
    KK_REQUIRE(q && K && V && out && lse && klen && S > 0 && heads > 0 && Sk > 0 && Sk <= 8192, "kk_attn_decode_rows: bad args (Sk <= 8192)");
    KK_REQUIRE(ldk % 4 == 0 && ldv % 4 == 0 && k_slot % 4 == 0 && v_slot % 4 == 0 && ldk >= (int64_t)heads * 64 && ldv >= (int64_t)heads * 64,
               "kk_attn_decode_rows: strides must be multiples of 4 elements and hold a frame");
    KK_REQUIRE((((uintptr_t)q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)out) & 15) == 0, "kk_attn_decode_rows: operands must be 16-byte aligned");
    RowsArgs a;
    a.Q = q; a.K = K; a.V = V; a.Out = out; a.LSEo = lse; a.klen = klen; a.key_mask = key_mask;
    a.heads = heads; a.Sk = Sk; a.k_slot = k_slot; a.ldk = ldk; a.v_slot = v_slot; a.ldv = ldv; a.scale = scale;
    const size_t lds = (size_t)(((Sk + 3) & ~3) + 16 * 64 + 32) * sizeof(float);
    if (bf16) hipLaunchKernelGGL(attn_decode_rows_kernel<__bf16>, dim3(S * heads), dim3(1024), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_decode_rows_kernel<float>, dim3(S * heads), dim3(1024), lds, (hipStream_t)stream, a);
    KK_LAUNCH_CHECK("kk_attn_decode_rows");
    return 0;
}

extern "C" int kk_decode_prologue_rows(const float *mel_all, float *frame_in, const float *pe, float *pe_rows, const float *cos_t,
                                       const float *sin_t, float *cos_rows, float *sin_rows, const int *t_rows, const int *done,
                                       int *klen, int S, int L1, int M, int H, int n_pos, void *stream) {
    KK_REQUIRE(mel_all && frame_in && pe && pe_rows && cos_t && sin_t && cos_rows && sin_rows && t_rows && done && klen && S > 0 &&
                   L1 > 1 && M > 0 && H > 0 && n_pos > 0,
               "kk_decode_prologue_rows: bad args");
    hipLaunchKernelGGL(decode_prologue_rows_kernel, dim3(S), dim3(256), 0, (hipStream_t)stream, mel_all, frame_in, pe, pe_rows, cos_t,
                       sin_t, cos_rows, sin_rows, t_rows, done, klen, L1, M, H, n_pos);
    KK_LAUNCH_CHECK("kk_decode_prologue_rows");
    return 0;
}

extern "C" int kk_decode_cache_append_rows(const void *nrm, void *q, void *kcache, void *vcache, const int *t_rows, const int *done,
                                           int S, int cap, int H, int bf16, void *stream) {
    KK_REQUIRE(nrm && q && kcache && vcache && t_rows && done && S > 0 && cap > 0 && H > 0 && (int64_t)S * H < (1ll << 31),
               "kk_decode_cache_append_rows: bad args");
    int blocks = kk_cdiv((int64_t)S * H, 256);
    if (blocks > 1024) blocks = 1024;
    if (bf16)
        hipLaunchKernelGGL(decode_cache_append_rows_kernel<uint16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const uint16_t *>(nrm), static_cast<uint16_t *>(q), static_cast<uint16_t *>(kcache),
                           static_cast<uint16_t *>(vcache), t_rows, done, S, cap, H);
    else
        hipLaunchKernelGGL(decode_cache_append_rows_kernel<uint32_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const uint32_t *>(nrm), static_cast<uint32_t *>(q), static_cast<uint32_t *>(kcache),
                           static_cast<uint32_t *>(vcache), t_rows, done, S, cap, H);
    KK_LAUNCH_CHECK("kk_decode_cache_append_rows");
    return 0;
}

extern "C" int kk_decode_epilogue_slots(const float *frame_out, const float *stop, float *mel_all, float *stop_all, int *t_rows,
                                        int *done, int *frames, int *live, const int *min_b, const int *expected_b, const int *max_b,
                                        int S, int L1, int M, float stop_threshold, float post_expected_stop_threshold, void *stream) {
    KK_REQUIRE(frame_out && stop && mel_all && stop_all && t_rows && done && frames && live && min_b && expected_b && max_b && S > 0 &&
                   L1 > 1 && M > 0,
               "kk_decode_epilogue_slots: bad args");
    hipLaunchKernelGGL(decode_epilogue_slots_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, frame_out, stop, mel_all, stop_all,
                       t_rows, done, frames, live, min_b, expected_b, max_b, L1, M, stop_threshold, post_expected_stop_threshold);
    KK_LAUNCH_CHECK("kk_decode_epilogue_slots");
    return 0;
}

extern "C" int kk_slot_admit(const void *kv_src, void *kv_pool, const uint8_t *fm_src, uint8_t *fm_pool, const int *slot_of,
                             const int *bounds, int *t_rows, int *done, int *frames, int *clen, int *min_b, int *expected_b, int *max_b,
                             float *mel_all, int *live, int n, int T_adm, int S, int cap, int64_t row_bytes, int L1, int M, void *stream) {
    KK_REQUIRE(kv_src && kv_pool && fm_src && fm_pool && slot_of && bounds && t_rows && done && frames && clen && min_b && expected_b &&
                   max_b && mel_all && live,
               "kk_slot_admit: null pointer");
    KK_REQUIRE(n > 0 && n <= S && T_adm > 0 && T_adm <= cap && L1 == cap + 1 && M > 0, "kk_slot_admit: bad shape (n <= S, T_adm <= cap, L1 = cap + 1)");
    KK_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && row_bytes / 16 < (1ll << 24) && (((uintptr_t)kv_src | (uintptr_t)kv_pool) & 15) == 0,
               "kk_slot_admit: K|V rows must be multiples of 16 bytes, 16-byte aligned");
    const int W16 = (int)(row_bytes / 16);
    int blocks = kk_cdiv((int64_t)n * T_adm * W16, 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < n) blocks = n;
    hipLaunchKernelGGL(slot_admit_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const uint4 *>(kv_src),
                       static_cast<uint4 *>(kv_pool), fm_src, fm_pool, slot_of, bounds, t_rows, done, frames, clen, min_b, expected_b,
                       max_b, mel_all, live, n, T_adm, S, cap, W16, L1, M);
    KK_LAUNCH_CHECK("kk_slot_admit");
    return 0;
}
