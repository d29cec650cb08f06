// The last stretch of long-form synthesis on a ragged batch (kokoro_ruslan_amd/longform.py; the definitions and their fp64 restatement:
// kokoro_ruslan_amd/longform_torch.py).  Two kernels, one launch each:
//
//  mel_finish  one workgroup per mel [T, n_mels] of a batch packed back to back.  Health statistics of the RAW mel (NaN count, min and
//              max of the other values, mean and unbiased standard deviation: fp64 sums, every thread over its own positions in
//              ascending order, then the wave butterfly and the four waves in order; the deviations in a second pass about the mean, so
//              that a constant mel gives ~0 and not cancellation noise), the clamped mel, and the reference's trailing-silence trim: the
//              mean of every clamped frame (fp32: 16 lanes per frame, lane j sums channels j, j + 16, ... in ascending order, then the
//              16-lane butterfly), the 10 % and 20 % quantiles of the frame means by torch.quantile's linear definition (a bitonic sort
//              in LDS over the next power of two, padded with +inf), the threshold clipped to [thr_lo, thr_hi], the last frame above it
//              and from that the frame count to keep.  A mel that holds a NaN is not sorted: its threshold is thr_hi, as the host
//              function's max(lo, min(hi, nan)) gives, and a frame whose mean is NaN is not voiced.
//  wave_join   every output sample of all documents of a call: its chunk's sample (times the fade table inside the first and last
//              min(F, n / 2) samples of the chunk) or zero in a gap.  Four consecutive outputs per thread as one 16-byte store; the
//              load is 16 bytes wide too where the chunk's offset allows it.  Workgroups 0 .. C-1 do not copy: workgroup c takes
//              max |x| of chunk c (the order of a max does not matter).
//
// Nothing crosses a row: no atomics, no sum over the batch, so a row's outputs do not depend on what else is in the launch.
// Limits (the host refuses the rest): 1 <= T <= 4096 frames per mel (32 KB of LDS: the frame means and their sorted copy), 1 <= n_mels
// <= 128; every chunk >= 1 sample, dst ascending, fewer than 2^31 input and output samples.
#include "kk_common.h"

namespace {

constexpr int MF_THREADS = 256, MF_MAX_T = 4096;

__device__ __forceinline__ float block_max_256(float v, float *red) {      // as block_sum_256; NaN-free inputs
    v = wave_max(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// torch.quantile(..., interpolation="linear") on T ascending values
__device__ __forceinline__ double mf_quantile(const float *__restrict__ sorted, int T, double q) {
    const double pos = q * (double)(T - 1);
    const int i0 = (int)floor(pos), i1 = min(i0 + 1, T - 1);
    const double a = (double)sorted[i0], b = (double)sorted[i1];
    return a + (pos - (double)i0) * (b - a);
}

__global__ __launch_bounds__(MF_THREADS) void mel_finish_kernel(const float *__restrict__ mel, const int64_t *__restrict__ moff,
                                                               int64_t frames, int n_mels, float lo, float hi, double thr_lo,
                                                               double thr_hi, int margin, int min_keep, float *__restrict__ out,
                                                               int *__restrict__ ends, double *__restrict__ stats) {
    __shared__ float fm[MF_MAX_T], srt[MF_MAX_T];
    __shared__ double redd[4];
    __shared__ float redf[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = moff[b], Tl = moff[b + 1] - t0;
    if (t0 < 0 || Tl < 1 || Tl > MF_MAX_T || t0 + Tl > frames) {           // (the host never makes these: bounds only)
        if (tid == 0) {
            ends[2 * b] = 0;
            ends[2 * b + 1] = -1;
            for (int i = 0; i < 6; ++i) stats[6 * b + i] = __builtin_nan("");
        }
        return;
    }
    const int T = (int)Tl;
    const int64_t N = (int64_t)T * n_mels;
    const float *x = mel + t0 * n_mels;
    float *y = out + t0 * n_mels;

    // raw statistics, the clamp and the frame means: 16 lanes per frame, 16 frames per pass of the workgroup
    const int g = tid >> 4, j = tid & 15;
    double sum = 0.0, nnan = 0.0;
    float vmin = INFINITY, vmax = -INFINITY;
    for (int tb = 0; tb < T; tb += MF_THREADS / 16) {                      // (uniform trip count: the butterfly needs every lane)
        const int t = tb + g;
        float acc = 0.f;
        if (t < T) {
            const int64_t row = (int64_t)t * n_mels;
            for (int k = j; k < n_mels; k += 16) {
                const float v = x[row + k];
                sum += (double)v;
                if (v != v) nnan += 1.0;
                else { vmin = fminf(vmin, v); vmax = fmaxf(vmax, v); }
                const float c = v < lo ? lo : (v > hi ? hi : v);           // torch.clamp: a NaN stays a NaN
                y[row + k] = c;
                acc += c;
            }
        }
        acc = kk_row16_sum(acc);
        if (t < T && j == 0) fm[t] = acc / (float)n_mels;
    }
    sum = block_sum_256_d(sum, redd);
    nnan = block_sum_256_d(nnan, redd);
    vmax = block_max_256(vmax, redf);
    vmin = -block_max_256(-vmin, redf);
    const double mean = sum / (double)N;
    double dev = 0.0;
    for (int64_t i = tid; i < N; i += MF_THREADS) {
        const double d = (double)x[i] - mean;
        dev += d * d;
    }
    dev = block_sum_256_d(dev, redd);                                      // (its barriers also publish fm)
    const double sd = sqrt(dev / (double)(N - 1));                         // N = 1: NaN, as torch.std

    double thr = thr_hi;
    if (nnan == 0.0) {                                                      // workgroup-uniform
        int P = 1;
        while (P < T) P <<= 1;
        for (int i = tid; i < P; i += MF_THREADS) srt[i] = i < T ? fm[i] : INFINITY;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int i = tid; i < P; i += MF_THREADS) {
                    const int p = i ^ s;
                    if (p > i) {
                        const float a = srt[i], c = srt[p];
                        if ((a > c) == ((i & k) == 0)) { srt[i] = c; srt[p] = a; }
                    }
                }
                __syncthreads();
            }
        thr = fmax(thr_lo, fmin(thr_hi, 0.5 * (mf_quantile(srt, T, 0.10) + mf_quantile(srt, T, 0.20))));
    }
    float last = -1.f;                                                     // (frame numbers < 4096 are exact in fp32)
    for (int t = tid; t < T; t += MF_THREADS)
        if ((double)fm[t] > thr) last = (float)t;                          // ascending t: the thread's last one stays
    const int last_voiced = (int)block_max_256(last, redf);
    if (tid == 0) {
        ends[2 * b] = last_voiced < 0 ? T : min(T, max(min_keep, min(T, last_voiced + margin + 1)));
        ends[2 * b + 1] = last_voiced;
        double *st = stats + 6 * b;
        st[0] = thr; st[1] = (double)vmin; st[2] = (double)vmax; st[3] = mean; st[4] = sd; st[5] = nnan;
    }
}

constexpr int WJ_THREADS = 256, WJ_ITERS = 4;                              // 4 x 4 outputs per thread

// c with dst[c] <= i < dst[c + 1] (dst ascending), or -1 when i < dst[0]
__device__ __forceinline__ int wj_find(const int64_t *__restrict__ dst, int C, int64_t i) {
    if (i < dst[0]) return -1;
    int lo = 0, hi = C;                                                    // invariant: dst[lo] <= i, and i < dst[hi] where hi < C
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (dst[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float wj_sample(const float *__restrict__ wave, const float *__restrict__ fade, int64_t base, int64_t n,
                                           int64_t nf, int64_t jn) {
    if (jn >= n) return 0.f;                                               // the gap behind the chunk
    const float v = wave[base + jn];
    if (jn < nf) return v * fade[jn];
    if (jn >= n - nf) return v * fade[n - 1 - jn];
    return v;
}

__global__ __launch_bounds__(WJ_THREADS) void wave_join_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                              const int64_t *__restrict__ dst, int C, const float *__restrict__ fade,
                                                              int F, int64_t total, float *__restrict__ out, float *__restrict__ peak) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < C) {                                             // max |x| of chunk blockIdx.x
        const int64_t a = woff[blockIdx.x], e = woff[blockIdx.x + 1];
        const int64_t a4 = min(e, (a + 3) & ~(int64_t)3), e4 = a4 + ((e - a4) & ~(int64_t)3);
        float pk = 0.f;
        bool bad = false;
        auto take = [&](float v) { bad = bad || v != v; pk = fmaxf(pk, fabsf(v)); };
        if (a + tid < a4) take(wave[a + tid]);
        for (int64_t i = a4 + 4 * (int64_t)tid; i < e4; i += 4 * WJ_THREADS) {
            const float4 v = ld4(wave + i);
            take(v.x); take(v.y); take(v.z); take(v.w);
        }
        if (e4 + tid < e) take(wave[e4 + tid]);
        pk = block_max_256(pk, red);
        const float anynan = block_max_256(bad ? 1.f : 0.f, red);
        if (tid == 0) peak[blockIdx.x] = anynan != 0.f ? __builtin_nanf("") : pk;      // torch's max: a NaN wins
        return;
    }
    int64_t i0 = ((int64_t)(blockIdx.x - C) * (WJ_THREADS * WJ_ITERS) + tid) * 4;
    if (i0 >= total) return;
    int c = wj_find(dst, C, i0);
#pragma unroll
    for (int it = 0; it < WJ_ITERS; ++it, i0 += 4 * WJ_THREADS) {
        if (i0 >= total) return;
        while (c + 1 < C && dst[c + 1] <= i0) ++c;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        bool fast = false;
        if (c >= 0) {
            const int64_t base = woff[c], n = woff[c + 1] - base, jn = i0 - dst[c];
            const int64_t nf = min((int64_t)F, n / 2);
            fast = jn >= nf && jn + 3 < n - nf;                            // four samples of one chunk, outside its fades
            if (fast) {
                const float *src = wave + base + jn;
                if (((base + jn) & 3) == 0) {
                    const float4 q = ld4(src);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = src[k];
                }
            }
        }
        if (!fast) {                                                       // a chunk's edge, a fade or a gap: sample by sample
            int cc = c;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + k;
                while (cc + 1 < C && dst[cc + 1] <= i) ++cc;
                if (cc >= 0 && i < total) {
                    const int64_t base = woff[cc], n = woff[cc + 1] - base;
                    v[k] = wj_sample(wave, fade, base, n, min((int64_t)F, n / 2), i - dst[cc]);
                }
            }
        }
        if (i0 + 3 < total) st4(out + i0, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int k = 0; k < 4 && i0 + k < total; ++k) out[i0 + k] = v[k];
    }
}

}  // namespace

extern "C" int kk_mel_finish(const float *mel, const int64_t *moff, int B, int64_t frames, int n_mels, float lo, float hi, double thr_lo,
                             double thr_hi, int margin, int min_keep, float *out, int *ends, double *stats, void *stream) {
    KK_REQUIRE(mel && moff && out && ends && stats && out != mel && B > 0 && frames > 0, "kk_mel_finish: bad args");
    KK_REQUIRE(n_mels >= 1 && n_mels <= 128, "kk_mel_finish: n_mels %d, expected 1..128", n_mels);
    KK_REQUIRE(lo <= hi && thr_lo <= thr_hi && margin >= 0 && min_keep >= 0,
               "kk_mel_finish: clamp [%g, %g] and threshold [%g, %g] must be ordered, margin %d and min_keep %d >= 0", (double)lo,
               (double)hi, thr_lo, thr_hi, margin, min_keep);
    kk_note_kernel("mel_finish");
    hipLaunchKernelGGL(mel_finish_kernel, dim3(B), dim3(MF_THREADS), 0, (hipStream_t)stream, mel, moff, frames, n_mels, lo, hi, thr_lo,
                       thr_hi, margin, min_keep, out, ends, stats);
    KK_LAUNCH_CHECK("kk_mel_finish");
    return 0;
}

extern "C" int kk_wave_join(const float *wave, const int64_t *woff, const int64_t *dst, int C, const float *fade, int F, int64_t total,
                            float *out, float *peak, void *stream) {
    KK_REQUIRE(wave && woff && dst && out && peak && out != wave && C > 0 && F >= 0 && (fade || F == 0), "kk_wave_join: bad args");
    KK_REQUIRE(total > 0 && total < ((int64_t)1 << 31), "kk_wave_join: %lld output samples, expected 1 .. 2^31 - 1", (long long)total);
    KK_REQUIRE(((uintptr_t)wave & 15) == 0 && ((uintptr_t)out & 15) == 0, "kk_wave_join: wave and out must be 16-byte aligned");
    kk_note_kernel("wave_join");
    hipLaunchKernelGGL(wave_join_kernel, dim3(C + kk_cdiv(total, 4 * WJ_THREADS * WJ_ITERS)), dim3(WJ_THREADS), 0, (hipStream_t)stream,
                       wave, woff, dst, C, fade, F, total, out, peak);
    KK_LAUNCH_CHECK("kk_wave_join");
    return 0;
}
