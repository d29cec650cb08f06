// The state kernels of the autoregressive decode step (model/generator.py:24-127, the KV-cache path of transformers.py:237-253), in
// both forms.  Lockstep (KokoroEngine.generate, generate_batch): every row of the batch is at the same frame t.  Per slot
// (KokoroEngine.generate_stream): a pool of S slots of `cap` frames each, every slot carries its own frame index t_s, so a finished row's
// slot is refilled while the others go on.
//
// The launches of one decoder step read the frame index from DEVICE memory (*t_dev, t_rows[s]), so that one captured hipGraph of the step
// is replayed for every frame (the step's ~100 launches are otherwise host-bound: ~1 ms per frame through eager launches); the per-slot
// launches' arguments depend on (S, cap) alone, so one graph serves a whole generate_stream call.
//
//  prologue       the step's input frame, positional row and RoPE rows into fixed buffers; key t becomes visible    model.py:541-545
//  cache append   the step's q | k | v: q to the query buffer, k and v to row t of the self-attention caches
//  epilogue       frame and stop logit filed under t, t += 1; rows / slots: the stop rule of ONE row         model/generator.py:67-88
//  slot admit     cross-attention K|V, frame mask and counters of newly admitted rows
//
// (The step's attention is attn_decode_kernel, kk_attn_fwd.hip.)  Per-slot state is int32 throughout (t_rows, done, frames, klen, the
// three bounds): the host reads done | frames in one copy.
#include "kk_common.h"

namespace {

// ------------------------------------------------------------------ prologue
// Lockstep, one workgroup: key t of the self-attention caches becomes visible (the attention runs over the whole cache with a key mask,
// so its arguments do not change with t).
__global__ __launch_bounds__(256) void decode_prologue_kernel(const float *__restrict__ mel_all, float *__restrict__ frame_in,
                                                              const float *__restrict__ pe, float *__restrict__ pe_row,
                                                              const float *__restrict__ cos_t, const float *__restrict__ sin_t,
                                                              float *__restrict__ cos_row, float *__restrict__ sin_row,
                                                              uint8_t *__restrict__ key_mask, const int *__restrict__ t_dev, int B, int L1,
                                                              int M, int H) {
    const int t = *t_dev;
    for (int i = threadIdx.x; i < B * M; i += 256) {
        const int b = i / M, c = i - b * M;
        frame_in[i] = mel_all[((int64_t)b * L1 + t) * M + c];
    }
    for (int i = threadIdx.x; i < H; i += 256) pe_row[i] = pe[(int64_t)t * H + i];
    for (int i = threadIdx.x; i < 64; i += 256) {
        cos_row[i] = cos_t[(int64_t)t * 64 + i];
        sin_row[i] = sin_t[(int64_t)t * 64 + i];
    }
    if (threadIdx.x == 0) key_mask[t] = 0;
}

// Per slot, one workgroup each: the attention gets a key count klen[s] instead of a mask.  A finished (or idle) slot is fed position 0
// and its own mel row 0, and gets klen = 0: its row of the step computes finite values that nothing reads.
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

// ------------------------------------------------------------------ cache append
// Lockstep: the step's normalised q | k | v [B, 3H] -> the query buffer [B*H] and row t of the time-major K and V caches [L][B*H]
template <typename T>
__global__ __launch_bounds__(256) void decode_cache_append_kernel(const T *__restrict__ nrm, T *__restrict__ q, T *__restrict__ kc,
                                                                  T *__restrict__ vc, const int *__restrict__ t_dev, int B, int H) {
    const int t = *t_dev;
    const int64_t row = (int64_t)t * B * H;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B * H; i += gridDim.x * 256) {
        const int b = i / H, c = i - b * H;
        const T *src = nrm + (int64_t)b * 3 * H + c;
        q[i] = src[0];
        kc[row + i] = src[H];
        vc[row + i] = src[2 * H];
    }
}

// Per slot: q | k | v [S, 3H] -> q [S, H] and row t_s of slot s of the slot-major K and V caches [S][cap][H]
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

// The elements are moved as 16- or 32-bit words: KERNEL<uint16_t> for bf16 storage, KERNEL<uint32_t> for fp32.
template <typename T, typename... A>
void launch_cache_append(void (*kernel)(const T *, T *, T *, T *, A...), int blocks, void *stream, const void *nrm, void *q, void *kc,
                         void *vc, A... rest) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const T *>(nrm), static_cast<T *>(q),
                       static_cast<T *>(kc), static_cast<T *>(vc), rest...);
}

// ------------------------------------------------------------------ epilogue
// Lockstep without a stop rule (generate: the host decides), one workgroup: the step's mel frame -> row t+1 of the output (= the next
// step's input), its stop logits -> row t; t += 1
__global__ __launch_bounds__(256) void decode_epilogue_kernel(const float *__restrict__ frame_out, const float *__restrict__ stop,
                                                              float *__restrict__ mel_all, float *__restrict__ stop_all,
                                                              int *__restrict__ t_dev, int B, int L1, int M) {
    const int t = *t_dev;
    for (int i = threadIdx.x; i < B * M; i += 256) {
        const int b = i / M, c = i - b * M;
        mel_all[((int64_t)b * L1 + t + 1) * M + c] = frame_out[i];
    }
    for (int i = threadIdx.x; i < B; i += 256) stop_all[(int64_t)t * B + i] = stop[i];
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = t + 1;
}

// Files the frame of row b and tells whether the row ends with it (defined below, with the stop rule).
__device__ __forceinline__ bool decode_row_file_and_stop(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_slot,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int b, int t, int lane, int L1,
    int M, float stop_threshold, float post_expected_stop_threshold);

// Lockstep with the stop rule of each row (generate_batch: row b of a padded batch must get what the reference's B = 1
// forward_inference gives utterance b alone).  One workgroup of 16 waves; wave w owns rows w, w + 16, ...  Everything a wave branches on
// (done flag, t, the row's bounds, its stop logit) is the same in all its lanes.
constexpr int EPI_WAVES = 16;

__global__ __launch_bounds__(64 * EPI_WAVES) void decode_epilogue_rows_kernel(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_all,
    int *__restrict__ t_dev, uint8_t *__restrict__ done, int *__restrict__ frames, int *__restrict__ live,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int B, int L1, int M,
    float stop_threshold, float post_expected_stop_threshold) {
    const int t = *t_dev;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (t + 1 < L1) {
        for (int b = wave; b < B; b += EPI_WAVES) {
            if (done[b]) continue;
            const bool fin = decode_row_file_and_stop(frame_out, stop, mel_all, stop_all + (int64_t)t * B + b, min_b, expected_b, max_b,
                                                      b, t, lane, L1, M, stop_threshold, post_expected_stop_threshold);
            if (fin && lane == 0) {
                done[b] = 1;
                frames[b] = t + 1;
                atomicSub(live, 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = t + 1;
}

// Per slot, one wave each: the same with a frame index per slot.
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

// ------------------------------------------------------------------ the stop rule of ONE row (model/generator.py:67-88)
// Called by one whole wave for row b at frame t (0 <= t < L1 - 1; what it branches on is the same in all lanes): files frame_out[b]
// under row t + 1 of the row's mel_all [L1][M] and the stop logit in *stop_slot (the caller's layout), and returns whether the row
// ends with this frame: its length bound, the stop head above the threshold of its side of `expected`, or the last 30 frames (rows
// t-28 .. t of earlier launches + this one) quiet in the mean, summed in fp64: lanes stride the frame, then the 29, then wave_sum_d.
__device__ __forceinline__ bool decode_row_file_and_stop(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_slot,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int b, int t, int lane, int L1,
    int M, float stop_threshold, float post_expected_stop_threshold) {
    const float *fo = frame_out + (int64_t)b * M;
    float *mrow = mel_all + (int64_t)b * L1 * M;
    double s = 0.0;
    for (int c = lane; c < M; c += 64) {
        const float v = fo[c];
        mrow[(int64_t)(t + 1) * M + c] = v;
        s += (double)v;
    }
    const float logit = stop[b];
    if (lane == 0) *stop_slot = logit;
    bool fin = t + 1 >= max_b[b];
    if (!fin && t >= min_b[b]) {
        const float thr = t < expected_b[b] ? stop_threshold : fminf(stop_threshold, post_expected_stop_threshold);
        const float prob = 1.f / (1.f + expf(-logit));
        if (prob > thr) {
            fin = true;
        } else if (t + 1 >= 30) {
            const float *tail = mrow + (int64_t)(t - 28) * M;             // 29 earlier frames, contiguous
            for (int i = lane; i < 29 * M; i += 64) s += (double)tail[i];
            s = wave_sum_d(s);
            fin = s / (30.0 * M) < -9.5;
        }
    }
    return fin;
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

extern "C" int kk_decode_prologue(const float *mel_all, float *frame_in, const float *pe, float *pe_row, const float *cos_t,
                                  const float *sin_t, float *cos_row, float *sin_row, uint8_t *key_mask, const int *t_dev, int B, int L1,
                                  int M, int H, void *stream) {
    KK_REQUIRE(mel_all && frame_in && pe && pe_row && cos_t && sin_t && cos_row && sin_row && key_mask && t_dev && B > 0 && L1 > 1 && M > 0 && H > 0,
               "kk_decode_prologue: bad args");
    hipLaunchKernelGGL(decode_prologue_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mel_all, frame_in, pe, pe_row, cos_t, sin_t,
                       cos_row, sin_row, key_mask, t_dev, B, L1, M, H);
    KK_LAUNCH_CHECK("kk_decode_prologue");
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

extern "C" int kk_decode_cache_append(const void *nrm, void *q, void *kcache, void *vcache, const int *t_dev, int B, int H, int bf16,
                                      void *stream) {
    KK_REQUIRE(nrm && q && kcache && vcache && t_dev && B > 0 && H > 0, "kk_decode_cache_append: bad args");
    int blocks = kk_cdiv((int64_t)B * H, 256);
    if (blocks > 64) blocks = 64;
    if (bf16) launch_cache_append(decode_cache_append_kernel<uint16_t>, blocks, stream, nrm, q, kcache, vcache, t_dev, B, H);
    else launch_cache_append(decode_cache_append_kernel<uint32_t>, blocks, stream, nrm, q, kcache, vcache, t_dev, B, H);
    KK_LAUNCH_CHECK("kk_decode_cache_append");
    return 0;
}

extern "C" int kk_decode_cache_append_rows(const void *nrm, void *q, void *kcache, void *vcache, const int *t_rows, const int *done,
                                           int S, int cap, int H, int bf16, void *stream) {
    KK_REQUIRE(nrm && q && kcache && vcache && t_rows && done && S > 0 && cap > 0 && H > 0 && (int64_t)S * H < (1ll << 31),
               "kk_decode_cache_append_rows: bad args");
    int blocks = kk_cdiv((int64_t)S * H, 256);
    if (blocks > 1024) blocks = 1024;
    if (bf16) launch_cache_append(decode_cache_append_rows_kernel<uint16_t>, blocks, stream, nrm, q, kcache, vcache, t_rows, done, S, cap, H);
    else launch_cache_append(decode_cache_append_rows_kernel<uint32_t>, blocks, stream, nrm, q, kcache, vcache, t_rows, done, S, cap, H);
    KK_LAUNCH_CHECK("kk_decode_cache_append_rows");
    return 0;
}

extern "C" int kk_decode_epilogue(const float *frame_out, const float *stop, float *mel_all, float *stop_all, int *t_dev, int B, int L1,
                                  int M, void *stream) {
    KK_REQUIRE(frame_out && stop && mel_all && stop_all && t_dev && B > 0 && L1 > 1 && M > 0, "kk_decode_epilogue: bad args");
    hipLaunchKernelGGL(decode_epilogue_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, frame_out, stop, mel_all, stop_all, t_dev, B, L1, M);
    KK_LAUNCH_CHECK("kk_decode_epilogue");
    return 0;
}

extern "C" int kk_decode_epilogue_rows(const float *frame_out, const float *stop, float *mel_all, float *stop_all, int *t_dev,
                                       uint8_t *done, int *frames, int *live, const int *min_b, const int *expected_b, const int *max_b,
                                       int B, int L1, int M, float stop_threshold, float post_expected_stop_threshold, void *stream) {
    KK_REQUIRE(frame_out && stop && mel_all && stop_all && t_dev && done && frames && live && min_b && expected_b && max_b && B > 0 &&
                   L1 > 1 && M > 0,
               "kk_decode_epilogue_rows: bad args");
    hipLaunchKernelGGL(decode_epilogue_rows_kernel, dim3(1), dim3(64 * EPI_WAVES), 0, (hipStream_t)stream, frame_out, stop, mel_all,
                       stop_all, t_dev, done, frames, live, min_b, expected_b, max_b, B, L1, M, stop_threshold,
                       post_expected_stop_threshold);
    KK_LAUNCH_CHECK("kk_decode_epilogue_rows");
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
