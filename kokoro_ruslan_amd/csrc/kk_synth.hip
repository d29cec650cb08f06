// Batched synthesis kernels: KokoroEngine.generate_batch, where row b of a padded batch must get what the reference's B = 1
// forward_inference gives utterance b alone.
//
//  row im2col3       conv1d(k=3, padding=1) operand with the row's own length as the sequence end  variance_predictor.py:47-52
//  row GroupNorm     GroupNorm(1, C) + ReLU with statistics over the row's valid frames of a chunk    variance_predictor.py:54-56,72-104
//  row mask          Linear(C->1) masked_fill: padding, frames past the row's length, <2-frame chunks   variance_predictor.py:94-115
//  row stop rule     the stop head / 30-frame energy rule / length bound of ONE row                     model/generator.py:67-88
//
// The per-row length lens[b] plays the part of the sequence length L at B = 1: a chunk is [512k, min(512(k+1), lens[b])), and
// everything at or past lens[b] is zero, as it would be outside the single-utterance tensor.
#include "kk_common.h"
#include "kk_stop_rule.h"

namespace {

// frames of row `len` inside the chunk that starts at cb (0 when the chunk lies past the row's end)
__device__ __forceinline__ int row_chunk_frames(int len, int cb, int chunk) {
    const int n = len - cb;
    return n <= 0 ? 0 : (n < chunk ? n : chunk);
}

// ------------------------------------------------------------------ conv k=3 as im2col, ends at the row's length
template <typename TO>
__global__ __launch_bounds__(256) void im2col3_rows_kernel(const float *__restrict__ x, TO *__restrict__ col, const int *__restrict__ lens,
                                                           int64_t total, int L, int C, int chunk) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t fr = i / C;
        const int c = (int)(i - fr * C);
        const int b = (int)(fr / L), l = (int)(fr - (int64_t)b * L);
        const int len = lens[b];
        const int cb = (l / chunk) * chunk;
        int ce = cb + chunk < L ? cb + chunk : L;
        if (len < ce) ce = len;
        TO *o = col + fr * 3 * C + c * 3;
        o[0] = (TO)((l - 1 >= cb && l - 1 < ce) ? x[i - C] : 0.f);
        o[1] = (TO)(l < ce ? x[i] : 0.f);
        o[2] = (TO)((l + 1 < ce) ? x[i + C] : 0.f);
    }
}

// ------------------------------------------------------------------ GroupNorm(1,C) per (row, 512-frame chunk) over the row's frames + ReLU
// Same fp64 partial -> finalize -> apply structure as kk_groupnorm_relu_fwd (kk_norm.hip); the element count of a (row, chunk) is its
// valid frames x C.
__global__ __launch_bounds__(256) void gn_rows_partial_kernel(const float *__restrict__ x, const int *__restrict__ lens,
                                                              double *__restrict__ scratch, int L, int C, int chunk, int nch, int slices) {
    __shared__ double red[4];
    const int bc = blockIdx.y, b = bc / nch, ci = bc % nch;
    const int64_t n = (int64_t)row_chunk_frames(lens[b], ci * chunk, chunk) * C;
    const float *base = x + ((int64_t)b * L + (int64_t)ci * chunk) * C;
    const int64_t per = ((n / 4 + slices - 1) / slices) * 4;
    const int64_t beg = (int64_t)blockIdx.x * per, end = beg + per < n ? beg + per : n;
    float s = 0.f, q = 0.f;
    for (int64_t i = beg + threadIdx.x * 4; i < end; i += 1024) {
        const float4 v = ld4(base + i);
        s += v.x + v.y + v.z + v.w;
        q += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    const double ds = block_sum_256_d((double)s, red);
    const double dq = block_sum_256_d((double)q, red);
    if (threadIdx.x == 0 && beg < end) {
        atomicAdd(&scratch[bc * 2], ds);
        atomicAdd(&scratch[bc * 2 + 1], dq);
    }
}

__global__ void gn_rows_finalize_kernel(const double *__restrict__ scratch, const int *__restrict__ lens, float *__restrict__ stats,
                                        int C, int chunk, int nch, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int frames = row_chunk_frames(lens[i / nch], (i % nch) * chunk, chunk);
    if (frames == 0) {                              // chunk past the row's end: never read (the apply writes zeros there)
        stats[i * 2] = 0.f;
        stats[i * 2 + 1] = 0.f;
        return;
    }
    const double n = (double)frames * C;
    const double mean = scratch[i * 2] / n;
    double var = scratch[i * 2 + 1] / n - mean * mean;
    if (var < 0) var = 0;
    stats[i * 2] = (float)mean;
    stats[i * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
}

__global__ __launch_bounds__(256) void gn_rows_apply_relu_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, const float *__restrict__ stats,
                                                                 const int *__restrict__ lens, float *__restrict__ y, int64_t total4,
                                                                 int L, int C, int chunk, int nch, const uint32_t *__restrict__ seedp,
                                                                 uint32_t site, float p) {
    const uint32_t thr = seedp ? kk_drop_threshold(p) : 0u, seed = thr ? *seedp : 0u;
    const float ik = thr ? 1.f / (1.f - p) : 1.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * 4;
        const int c = (int)(e % C);
        const int64_t fr = e / C;
        const int l = (int)(fr % L), b = (int)(fr / L), ci = l / chunk;
        const int len = lens[b];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l < len && row_chunk_frames(len, ci * chunk, chunk) >= 2) {
            const float mu = stats[(b * nch + ci) * 2], rs = stats[(b * nch + ci) * 2 + 1];
            const float4 v = ld4(x + e), g = ld4(gamma + c), bt = ld4(beta + c);
            o.x = fmaxf((v.x - mu) * rs * g.x + bt.x, 0.f);
            o.y = fmaxf((v.y - mu) * rs * g.y + bt.y, 0.f);
            o.z = fmaxf((v.z - mu) * rs * g.z + bt.z, 0.f);
            o.w = fmaxf((v.w - mu) * rs * g.w + bt.w, 0.f);
            if (thr) {
                float m[4];
                kk_drop_mul4(seed, site, (uint64_t)e, thr, ik, m);
                o.x *= m[0]; o.y *= m[1]; o.z *= m[2]; o.w *= m[3];
            }
        }
        st4(y + e, o);
    }
}

// ------------------------------------------------------------------ the predictors' output mask, per row
__global__ __launch_bounds__(256) void row_mask_kernel(const uint8_t *__restrict__ mask_in, const int *__restrict__ lens,
                                                       uint8_t *__restrict__ mask_out, int64_t total, int L, int chunk) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
        const int len = lens[b];
        const bool dead = (mask_in && mask_in[i]) || l >= len || row_chunk_frames(len, (l / chunk) * chunk, chunk) < 2;
        mask_out[i] = dead ? 1 : 0;
    }
}

// ------------------------------------------------------------------ decode epilogue with the stop rule of each row
// One workgroup of 16 waves; wave w owns rows w, w + 16, ...  Everything a wave branches on (done flag, t, the row's bounds, its stop
// logit) is the same in all its lanes.  Filing the frame and the stop rule of a row: decode_row_file_and_stop (kk_stop_rule.h).
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

inline int grid_cap(int64_t n, int cap) {
    int b = kk_cdiv(n, 256);
    return b > cap ? cap : (b < 1 ? 1 : b);
}

}  // namespace

extern "C" int kk_im2col3_rows_fwd(const float *x, float *col, const int *lens, int B, int L, int C, int chunk, int col_bf16, void *stream) {
    KK_REQUIRE(x && col && lens && B > 0 && L > 0 && C > 0 && chunk > 0, "kk_im2col3_rows_fwd: bad args");
    const int64_t total = (int64_t)B * L * C;
    if (col_bf16)
        hipLaunchKernelGGL(im2col3_rows_kernel<__bf16>, dim3(grid_cap(total, 1024)), dim3(256), 0, (hipStream_t)stream, x,
                           reinterpret_cast<__bf16 *>(col), lens, total, L, C, chunk);
    else
        hipLaunchKernelGGL(im2col3_rows_kernel<float>, dim3(grid_cap(total, 1024)), dim3(256), 0, (hipStream_t)stream, x, col, lens, total,
                           L, C, chunk);
    KK_LAUNCH_CHECK("kk_im2col3_rows_fwd");
    return 0;
}

extern "C" int kk_groupnorm_relu_rows_fwd(const float *x, const float *gamma, const float *beta, float *y, float *stats, double *scratch,
                                          const int *lens, int B, int L, int C, int chunk, const uint32_t *seed, uint32_t site, float p,
                                          void *stream) {
    KK_REQUIRE(x && gamma && beta && y && stats && scratch && lens && B > 0 && L > 0 && C > 0 && C % 4 == 0 && chunk > 0 && p >= 0.f && p < 1.f,
               "kk_groupnorm_relu_rows_fwd: bad args");
    hipStream_t s = (hipStream_t)stream;
    const int nch = kk_cdiv(L, chunk), total = B * nch;
    const int e = kk_zero_async(scratch, sizeof(double) * 2 * total, s);
    if (e != 0) return e;
    const int slices = 32;
    hipLaunchKernelGGL(gn_rows_partial_kernel, dim3(slices, total), dim3(256), 0, s, x, lens, scratch, L, C, chunk, nch, slices);
    hipLaunchKernelGGL(gn_rows_finalize_kernel, dim3(kk_cdiv(total, 64)), dim3(64), 0, s, scratch, lens, stats, C, chunk, nch, total);
    const int64_t total4 = (int64_t)B * L * C / 4;
    hipLaunchKernelGGL(gn_rows_apply_relu_kernel, dim3(grid_cap(total4, 1024)), dim3(256), 0, s, x, gamma, beta, stats, lens, y, total4, L,
                       C, chunk, nch, p > 0.f ? seed : nullptr, site, p);
    KK_LAUNCH_CHECK("kk_groupnorm_relu_rows_fwd");
    return 0;
}

extern "C" int kk_varpred_row_mask(const uint8_t *mask_in, const int *lens, uint8_t *mask_out, int B, int L, int chunk, void *stream) {
    KK_REQUIRE(lens && mask_out && B > 0 && L > 0 && chunk > 0, "kk_varpred_row_mask: bad args");
    const int64_t total = (int64_t)B * L;
    hipLaunchKernelGGL(row_mask_kernel, dim3(grid_cap(total, 256)), dim3(256), 0, (hipStream_t)stream, mask_in, lens, mask_out, total, L,
                       chunk);
    KK_LAUNCH_CHECK("kk_varpred_row_mask");
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
