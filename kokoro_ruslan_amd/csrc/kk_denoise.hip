// Spectral (bias) denoising of vocoded audio (kokoro_ruslan_amd/denoise.py): y = istft(G . stft(x)), G = max(1 - s b[k] / |X|, 0), with
// n_fft = win = 1024, hop = 256, periodic Hann window, center = True, reflect padding, onesided, torch.istft's window-square envelope.
//
//  denoise        one launch for a ragged batch of waveforms packed back to back (woff: sample offsets).  A tile is a run of DTF hops of
//                 ONE utterance: output samples [256 f0, 256 (f0 + DTF)) clipped to the utterance.  Sample j sits at position j + 512 of
//                 the padded signal, which frames j / 256 - 1 .. j / 256 + 2 cover, so the tile transforms frames f0 - 1 .. f0 + DTF + 1
//                 clipped to the utterance's 1 + N / 256 frames: DTF + 3 at most, the three extra ones being the halo its neighbours
//                 transform as well.  One wave per frame: forward frame, split step, gain, inverse pre-step and tail into LDS (all but
//                 the gain from kk_fft.h).  Then every thread sums the frames that cover its samples in ascending frame order, divides
//                 by the window-square envelope (stft_ola) and stores.  Nothing leaves the workgroup but its own samples: no atomics,
//                 and no sum whose order depends on the tile or on the rest of the batch.
//  stft_mag_mean  mean over frames [f_lo, f_hi) of |stft| of one waveform (the vocoder's bias): one workgroup, wave w sums frames
//                 f_lo + w, f_lo + w + 4, ... in registers, then the four partial sums are added in wave order.
//
// A lane computes bins k = lane + 64 j and 512 - k together (stft_split_pair: the split step has both operands at hand), so the gated
// spectrum never goes through LDS: the lane forms the inverse transform's input Z'[k] from Y[k] and Y[512 - k] directly.
// This file owns the tiles, the gate and the magnitude sum.
#include "kk_common.h"
#include "kk_fft.h"

namespace {

constexpr int DTF = 13, DHF = DTF + 3;                         // hops of one tile, frames it transforms at most (64 KiB of LDS)
constexpr int DTHREADS = 256, DWAVES = DTHREADS / 64;

__device__ __forceinline__ float2 dn_gate(float2 x, float sb) {   // x . max(1 - sb / |x|, 0), 0 at |x| = 0
    const float m = sqrtf(x.x * x.x + x.y * x.y);
    const float g = m > sb ? (m - sb) / m : 0.f;
    return make_float2(x.x * g, x.y * g);
}

__global__ __launch_bounds__(DTHREADS, 2) void denoise_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                           const int2 *__restrict__ tiles, const float *__restrict__ bias, float strength,
                                                           const float2 *__restrict__ twt, const float *__restrict__ win,
                                                           float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float frm[DHF][STFT_N]; // FFT slot of a frame, then its windowed inverse transform
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int2 tl = tiles[blockIdx.x];
    const int64_t base = woff[tl.x];
    const int64_t len = woff[tl.x + 1] - base;
    const int f0 = tl.y;
    if (len < STFT_N || len > 0x7fffffff - STFT_N || f0 < 0 || (int64_t)STFT_HOP * f0 >= len) return;      // (the host refuses these)
    const int N = (int)len, F = 1 + N / STFT_HOP;
    const int f1 = min(f0 + DTF, F), h0 = max(f0 - 1, 0), h1 = min(f1 + 2, F);
    const float *x = wave + base;

    StftTw tw;
    stft_twiddles(twt, lane, tw);

    // 1. every frame that covers the tile's samples: forward, gain, inverse, window
#pragma unroll 1
    for (int i = wv; i < h1 - h0; i += DWAVES) {
        float2 *sl = reinterpret_cast<float2 *>(frm[i]);
        float2 v[8];
        stft_frame_fwd([&](int j) { return x[j]; }, h0 + i, N, win, sl, tw, lane);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            float2 X, Xm;
            stft_split_pair(sl, tw.twk[m], lane + 64 * m, X, Xm);
            const float2 yk = dn_gate(X, strength * bias[lane + 64 * m]), ym = dn_gate(Xm, strength * bias[STFT_N / 2 - lane - 64 * m]);
            v[m] = stft_inv_pre(yk, ym, tw.twk[m]);
        }
        stft_inv_tail(v, sl, win, tw, lane);
    }
    __syncthreads();

    // 2. overlap-add in ascending frame order, envelope division, store: sample j is position p = j + 512 of the padded signal
    const int j1 = min(STFT_HOP * f1, N);
    for (int j = STFT_HOP * f0 + threadIdx.x; j < j1; j += DTHREADS) {
        const int p = j + STFT_N / 2;
        const int tlo = max(p >= STFT_N ? (p - STFT_N) / STFT_HOP + 1 : 0, h0), thi = min(p / STFT_HOP, h1 - 1);
        out[base + j] = stft_ola(frm, h0, tlo, thi, p, win);
    }
}

__global__ __launch_bounds__(DTHREADS) void stft_mag_mean_kernel(const float *__restrict__ x, int N, int f_lo, int f_hi,
                                                                 const float2 *__restrict__ twt, const float *__restrict__ win,
                                                                 float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float slot[DWAVES][STFT_N];
    __shared__ float part[DWAVES][STFT_BINS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    StftTw tw;
    stft_twiddles(twt, lane, tw);
    float acc[8], acc512 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll 1
    for (int t = f_lo + wv; t < f_hi; t += DWAVES) {
        const float2 *sl = reinterpret_cast<const float2 *>(slot[wv]);
        stft_frame_fwd([&](int j) { return x[j]; }, t, N, win, reinterpret_cast<float2 *>(slot[wv]), tw, lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float2 X, Xm;
            stft_split_pair(sl, tw.twk[j], lane + 64 * j, X, Xm);
            acc[j] += sqrtf(X.x * X.x + X.y * X.y);
            if (j == 0) acc512 += sqrtf(Xm.x * Xm.x + Xm.y * Xm.y);      // lane 0: bin 512
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wv][lane + 64 * j] = acc[j];
    if (lane == 0) part[wv][STFT_N / 2] = acc512;
    __syncthreads();
    const float inv = 1.f / (float)(f_hi - f_lo);
    for (int k = threadIdx.x; k < STFT_BINS; k += DTHREADS) out[k] = (((part[0][k] + part[1][k]) + part[2][k]) + part[3][k]) * inv;
}

}  // namespace

extern "C" int kk_denoise_tile_frames(void) { return DTF; }

extern "C" int kk_denoise(const float *wave, const int64_t *woff, const int *tiles, int ntiles, const float *bias, float strength,
                          const void *tw, const float *win, float *out, void *stream) {
    KK_REQUIRE(wave && woff && tiles && bias && tw && win && out && ntiles > 0 && out != wave && strength >= 0.f && strength < INFINITY,
               "kk_denoise: bad args (out != wave: a tile reads the samples of its neighbours; strength finite and >= 0)");
    kk_note_kernel("denoise");
    hipLaunchKernelGGL(denoise_kernel, dim3(ntiles), dim3(DTHREADS), 0, (hipStream_t)stream, wave, woff, (const int2 *)tiles, bias,
                       strength, (const float2 *)tw, win, out);
    KK_LAUNCH_CHECK("kk_denoise");
    return 0;
}

extern "C" int kk_stft_mag_mean(const float *wave, int64_t n, int f_lo, int f_hi, const void *tw, const float *win, float *out,
                                void *stream) {
    KK_REQUIRE(wave && tw && win && out, "kk_stft_mag_mean: bad args");
    KK_REQUIRE(n >= STFT_N && n <= 0x7fffffff - STFT_N, "kk_stft_mag_mean: %lld samples, need 1024 .. 2^31 - 1025", (long long)n);
    KK_REQUIRE(0 <= f_lo && f_lo < f_hi && f_hi <= 1 + n / STFT_HOP, "kk_stft_mag_mean: frames [%d, %d) of %lld", f_lo, f_hi,
               (long long)(1 + n / STFT_HOP));
    kk_note_kernel("stft_mag_mean");
    hipLaunchKernelGGL(stft_mag_mean_kernel, dim3(1), dim3(DTHREADS), 0, (hipStream_t)stream, wave, (int)n, f_lo, f_hi,
                       (const float2 *)tw, win, out);
    KK_LAUNCH_CHECK("kk_stft_mag_mean");
    return 0;
}
