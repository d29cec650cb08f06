// Audio feature extraction (kokoro_ruslan_amd/features.py): a batch of waveforms to log-mel, pitch and energy on the device, as the
// reference's dataset computes them per utterance (22050 Hz, n_fft = win = 1024, hop 256, 80 HTK mels, pitch window 2048, lags 27..441).
//
//  peak     per-utterance max|x| (an integer atomic max on the bits of |x|: exact in any order)
//  mel      per frame: x / (peak + 1e-9) on load, reflect padding by index, periodic Hann, real FFT of 1024, power, the sparse
//           80-column filterbank, log(. + 1e-9); and log1p(mean over mels) of the linear mel for the energy
//  pitch    per frame: normalise and pre-emphasise on load, reflect padding by index, periodic Hann of 2048, the linear autocorrelation
//           at lags 0..447 by direct sums, CMND, first dip below 0.15 (else the argmin) in lags 27..441, parabolic refinement
//  finish   per utterance: the order statistics (q05 / q95 of the energy, q25 of the largest autocorrelation, lower median of the mean
//           square) by rank counting, voicing, linear fill of gaps of <= 5 frames, 5-tap median filter, normalisation
//
// Layout: the waveforms of a batch are packed back to back (woff: sample offsets, B + 1), and so are the outputs: mel frames by moff
// (the frames kept after the cut to max_seq_length), pitch frames by poff (all of them: the pitch statistics run over every frame).
// Every sum runs in an order fixed by the frame's position in its own utterance, so an utterance's output does not depend on the batch.
//
// This file owns the sample load (x / (peak + 1e-9), zero past the samples given), the mel tile and the power / filterbank step per
// bin, and all of pitch and finish.  The frame transform, the split step and the reflect rule are kk_fft.h's.
#include "kk_common.h"
#include "kk_fft.h"

namespace {

constexpr int FMELS = 80;
constexpr int FTHREADS = 256, FWAVES = FTHREADS / 64;
constexpr int MTF = 16;                                       // mel frames per workgroup (64-byte runs of a [80, T] row)
constexpr int PW = 2048, PLAGS = 448, PLMIN = 27, PLMAX = 441;  // pitch window; lags computed (8 per lane group); the search range
constexpr int PGROUPS = PLAGS / 8;                            // 56 lane groups of 8 lags, one n-quarter of the window per wave
constexpr int PXS = PW + PLAGS + 8;                           // the frame, then zeros the largest lag reads
constexpr int PEAK_CHUNK = 4096;
constexpr float SR = 22050.f;

struct Utt {
    int64_t w0;      // first sample in the packed waveform
    int n_raw, n;    // samples given; samples after zero-padding to the window
    float d;         // peak + 1e-9
};

__device__ __forceinline__ Utt load_utt(const int64_t *woff, const float *peak, int b, int win) {
    Utt u;
    u.w0 = woff[b];
    u.n_raw = (int)(woff[b + 1] - u.w0);
    u.n = max(u.n_raw, win);
    u.d = peak[b] + 1e-9f;
    return u;
}

__global__ __launch_bounds__(FTHREADS) void feat_peak_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                             unsigned *__restrict__ peak_bits) {
    const int b = blockIdx.y;
    const int64_t w0 = woff[b], n = woff[b + 1] - w0;
    const int64_t i0 = (int64_t)blockIdx.x * PEAK_CHUNK;
    if (i0 >= n) return;
    const int64_t i1 = min(i0 + PEAK_CHUNK, n);
    float m = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += FTHREADS) m = fmaxf(m, fabsf(wave[w0 + i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(peak_bits + b, __float_as_uint(m));   // |x| >= 0: its bits order like the value
}

struct MelArgs {
    const float *wave;
    const int64_t *woff;
    const float *peak;
    const int *moff;       // first kept mel frame of each utterance in the packed outputs (B + 1)
    const int2 *tiles;     // {utterance, first frame of the tile}
    const float2 *tw;      // exp(-2 pi i j / 1024)
    const float *win;      // periodic Hann, 1024
    const float *fb;       // [513, 80]
    const int2 *span;      // per mel: bins [x, y) where its triangle is non-zero
    float *logmel;         // per utterance [80, T_b] at 80 moff[b]
    float *linmel;         // the same layout, or null
    float *eraw;           // log1p(mean over mels of the linear mel), per kept frame
};

__global__ __launch_bounds__(FTHREADS) void feat_mel_kernel(const MelArgs a) {
    __shared__ __attribute__((aligned(16))) float2 slot[FWAVES][STFT_N / 2];
    __shared__ float pw[FWAVES][STFT_BINS + 7];
    __shared__ float st[2][FMELS][MTF + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 tl = a.tiles[blockIdx.x];
    const int b = tl.x, f0 = tl.y;
    const Utt u = load_utt(a.woff, a.peak, b, STFT_N);
    const int m0 = a.moff[b], T = a.moff[b + 1] - m0, f1 = min(f0 + MTF, T);

    StftTw tw;
    stft_twiddles(a.tw, lane, tw);
    float2 *sl = slot[wave];
    float *p = pw[wave];

    for (int t = f0 + wave; t < f1; t += FWAVES) {
        stft_frame_fwd([&](int j) { return j < u.n_raw ? a.wave[u.w0 + j] / u.d : 0.f; }, t, u.n, a.win, sl, tw, lane);
#pragma unroll
        for (int j = 0; j <= 8; ++j) {
            if (j == 8 && lane != 0) break;
            const int k = j < 8 ? lane + 64 * j : STFT_N / 2;
            const float2 X = j < 8 ? stft_split(sl, tw.twk[j], k) : stft_bin512(sl);
            p[k] = X.x * X.x + X.y * X.y;
        }
        __syncwarp();
        float lin[2] = {0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = lane + 64 * h;
            if (m < FMELS) {
                const int2 sp = a.span[m];
                float acc = 0.f;
                for (int k = sp.x; k < sp.y; ++k) acc = fmaf(a.fb[k * FMELS + m], p[k], acc);
                lin[h] = acc;
                st[0][m][t - f0] = logf(acc + 1e-9f);
                st[1][m][t - f0] = acc;
            }
        }
        float sum = lin[0] + lin[1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) a.eraw[m0 + t] = log1pf(fmaxf(sum / FMELS, 0.f));
        __syncwarp();
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FMELS * MTF; i += FTHREADS) {
        const int m = i / MTF, f = i % MTF;
        if (f0 + f >= f1) continue;
        const int64_t o = (int64_t)FMELS * m0 + (int64_t)m * T + f0 + f;
        a.logmel[o] = st[0][m][f];
        if (a.linmel) a.linmel[o] = st[1][m][f];
    }
}

struct PitchArgs {
    const float *wave;
    const int64_t *woff;
    const float *peak;
    const int *poff;       // first pitch frame of each utterance in the packed outputs (B + 1)
    const int2 *frames;    // {utterance, frame}
    const float *win;      // periodic Hann, 2048
    float *cand;           // candidate frequency (Hz), per frame
    float *acmax;          // largest normalised autocorrelation over lags 27..441
    float *msq;            // mean square of the windowed frame
};

__global__ __launch_bounds__(FTHREADS) void feat_pitch_kernel(const PitchArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[PXS];
    __shared__ float part[FWAVES][PLAGS];
    __shared__ float cm[PLAGS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 fr = a.frames[blockIdx.x];
    const int b = fr.x, t = fr.y;
    const Utt u = load_utt(a.woff, a.peak, b, PW);

    for (int i = threadIdx.x; i < PXS; i += FTHREADS) {
        float s = 0.f;
        if (i < PW) {
            const int j = reflect(STFT_HOP * t - PW / 2 + i, u.n);
            const float x1 = j < u.n_raw ? a.wave[u.w0 + j] / u.d : 0.f;
            const float x0 = j > 0 && j - 1 < u.n_raw ? a.wave[u.w0 + j - 1] / u.d : 0.f;
            s = (j > 0 ? x1 - 0.97f * x0 : x1) * a.win[i];
        }
        xs[i] = s;
    }
    __syncthreads();

    // r[tau] = sum_n x[n] x[n + tau] (x = 0 past the window: the linear autocorrelation).  Wave q sums n in [512 q, 512 q + 512);
    // lane g < 56 holds lags 8 g .. 8 g + 7 and slides an 8 x 8 tile of products along n.
    if (lane < PGROUPS) {
        float acc[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[l] = 0.f;
        const int n0 = (PW / FWAVES) * wave, tau0 = 8 * lane;
        float4 lo0 = *reinterpret_cast<const float4 *>(xs + n0 + tau0), lo1 = *reinterpret_cast<const float4 *>(xs + n0 + tau0 + 4);
        for (int n = n0; n < n0 + PW / FWAVES; n += 8) {
            const float4 a0 = *reinterpret_cast<const float4 *>(xs + n), a1 = *reinterpret_cast<const float4 *>(xs + n + 4);
            const float4 hi0 = *reinterpret_cast<const float4 *>(xs + n + tau0 + 8), hi1 = *reinterpret_cast<const float4 *>(xs + n + tau0 + 12);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float bv[16] = {lo0.x, lo0.y, lo0.z, lo0.w, lo1.x, lo1.y, lo1.z, lo1.w, hi0.x, hi0.y, hi0.z, hi0.w, hi1.x, hi1.y, hi1.z, hi1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int l = 0; l < 8; ++l) acc[l] = fmaf(av[i], bv[i + l], acc[l]);
            lo0 = hi0;
            lo1 = hi1;
        }
#pragma unroll
        for (int l = 0; l < 8; ++l) part[wave][tau0 + l] = acc[l];
    }
    __syncthreads();
    if (wave != 0) return;

    // wave 0: lane holds lags 7 lane .. 7 lane + 6
    float r[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int tau = 7 * lane + i;
        r[i] = (part[0][tau] + part[1][tau]) + (part[2][tau] + part[3][tau]);
    }
    const float r0 = __shfl(r[0], 0);
    float d[7], run = 0.f, best_ac = -INFINITY;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int tau = 7 * lane + i;
        d[i] = tau >= 1 ? 2.f * r0 - 2.f * r[i] : 0.f;
        run += d[i];
        if (tau >= PLMIN && tau <= PLMAX) best_ac = fmaxf(best_ac, r[i] / fmaxf(r0, 1e-8f));
    }
    float incl = run;                                              // inclusive scan of the lanes' sums
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    float cum = incl - run;
    int dip = 1 << 20, amin = 1 << 20;
    float vmin = INFINITY;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int tau = 7 * lane + i;
        cum += d[i];
        const float c = tau >= 1 ? d[i] / (cum / (float)tau + 1e-8f) : 1.f;
        cm[tau] = c;
        if (tau >= PLMIN && tau <= PLMAX) {
            if (c < 0.15f && dip == (1 << 20)) dip = tau;
            if (c < vmin) { vmin = c; amin = tau; }                 // first minimum within the lane
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dip = min(dip, __shfl_xor(dip, o));
        best_ac = fmaxf(best_ac, __shfl_xor(best_ac, o));
        const float ov = __shfl_xor(vmin, o);
        const int oi = __shfl_xor(amin, o);
        if (ov < vmin || (ov == vmin && oi < amin)) { vmin = ov; amin = oi; }
    }
    __syncwarp();
    if (lane == 0) {
        const int best = dip != (1 << 20) ? dip : (amin != (1 << 20) ? amin : PLMIN);
        const float al = cm[max(best - 1, PLMIN)], be = cm[best], ga = cm[min(best + 1, PLMAX)];
        const float den = fmaxf(al - 2.f * be + ga, 1e-8f);
        const float off = fminf(fmaxf(0.5f * (al - ga) / den, -1.f), 1.f);
        const int o = a.poff[b] + t;
        a.cand[o] = SR / fmaxf((float)best + off, 1.f);
        a.acmax[o] = best_ac;
        a.msq[o] = r0 / PW;
    }
}

struct FinArgs {
    const int *moff, *poff;
    const float *eraw, *cand, *acmax, *msq;
    float *f0a, *f0b;      // scratch, per pitch frame
    float *pitch, *energy; // per kept mel frame
    int variance;
};

// sorted(v)[k] for 0 <= k < n by rank counting (ties by index), the same for any launch shape.  Every thread returns the value.
__device__ float kth(const float *v, int n, int k, float *sh) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += FTHREADS) {
        const float x = v[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float y = v[j];
            rank += (y < x) || (y == x && j < i);
        }
        if (rank == k) *sh = x;
    }
    __syncthreads();
    return *sh;
}

// torch.quantile(v, q) with linear interpolation, in fp32 as torch computes it
__device__ float quantile(const float *v, int n, float q, float *sh) {
    const float pos = q * (float)(n - 1);
    const int lo = (int)floorf(pos), hi = (int)ceilf(pos);
    const float w = pos - (float)lo;
    const float x = kth(v, n, lo, sh), y = kth(v, n, hi, sh);
    return w < 0.5f ? x + w * (y - x) : y - (y - x) * (1.f - w);
}

__device__ __forceinline__ void sort2(float &x, float &y) { const float lo = fminf(x, y), hi = fmaxf(x, y); x = lo; y = hi; }

__global__ __launch_bounds__(FTHREADS) void feat_finish_kernel(const FinArgs a) {
    __shared__ float sh;
    const int b = blockIdx.x;
    const int m0 = a.moff[b], T = a.moff[b + 1] - m0, p0 = a.poff[b], Tp = a.poff[b + 1] - p0;
    if (!a.variance) {
        for (int i = threadIdx.x; i < T; i += FTHREADS) a.pitch[m0 + i] = a.energy[m0 + i] = 0.f;
        return;
    }
    // energy: (e - q05) / max(q95 - q05, 1e-8) over the kept frames; min / max below 3 frames
    const float *e = a.eraw + m0;
    const float lo = T < 3 ? kth(e, T, 0, &sh) : quantile(e, T, 0.05f, &sh);
    const float hi = T < 3 ? kth(e, T, T - 1, &sh) : quantile(e, T, 0.95f, &sh);
    for (int i = threadIdx.x; i < T; i += FTHREADS)
        a.energy[m0 + i] = fminf(fmaxf((e[i] - lo) / fmaxf(hi - lo, 1e-8f), 0.f), 1.f);

    // voicing thresholds over all pitch frames
    const float vth = fminf(fmaxf(0.8f * quantile(a.acmax + p0, Tp, 0.25f, &sh), 0.15f), 0.35f);
    const float eth = fmaxf(0.05f * kth(a.msq + p0, Tp, (Tp - 1) / 2, &sh), 1e-9f);
    float *f = a.f0a + p0, *g = a.f0b + p0;
    for (int i = threadIdx.x; i < Tp; i += FTHREADS) {
        float x = a.cand[p0 + i];
        if (a.acmax[p0 + i] < vth || a.msq[p0 + i] < eth || x < 50.f || x > 800.f) x = 0.f;
        f[i] = x;
    }
    __syncthreads();
    // unvoiced gaps of <= 5 frames between voiced ones: both neighbours lie within 5 frames
    for (int i = threadIdx.x; i < Tp; i += FTHREADS) {
        float x = f[i];
        if (!(x > 0.f)) {
            int pi = -1, ni = -1;
            for (int k = 1; k <= 5 && pi < 0; ++k) if (i - k >= 0 && f[i - k] > 0.f) pi = i - k;
            for (int k = 1; k <= 5 && ni < 0; ++k) if (i + k < Tp && f[i + k] > 0.f) ni = i + k;
            if (pi >= 0 && ni >= 0 && ni - pi - 1 <= 5) {
                const float w = (float)(i - pi) / fmaxf((float)(ni - pi), 1.f);
                x = f[pi] * (1.f - w) + f[ni] * w;
            }
        }
        g[i] = x;
    }
    __syncthreads();
    // 5-tap median with reflect padding, normalisation with zeros kept; cut to the mel's frames
    for (int i = threadIdx.x; i < T; i += FTHREADS) {
        float out = 0.f;
        if (i < Tp) {
            float v[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = g[reflect(i + k - 2, Tp)];
            sort2(v[0], v[1]); sort2(v[3], v[4]); sort2(v[0], v[3]); sort2(v[1], v[4]);      // median of 5
            sort2(v[1], v[2]); sort2(v[2], v[3]); sort2(v[1], v[2]);
            const float med = v[2];
            out = med == 0.f ? 0.f : fminf(fmaxf((med - 50.f) / (750.f + 1e-8f), 0.f), 1.f);
        }
        a.pitch[m0 + i] = out;
    }
}

}  // namespace

extern "C" int kk_feat_mel_tile_frames(void) { return MTF; }

extern "C" int kk_feat_peak(const float *wave, const int64_t *woff, int B, int64_t max_samples, float *peak, void *stream) {
    KK_REQUIRE(wave && woff && peak && B > 0 && B <= 65535 && max_samples > 0, "kk_feat_peak: bad args");
    if (hipMemsetAsync(peak, 0, sizeof(float) * B, (hipStream_t)stream) != hipSuccess) return 1;
    kk_note_kernel("feat_peak");
    hipLaunchKernelGGL(feat_peak_kernel, dim3(kk_cdiv(max_samples, PEAK_CHUNK), B), dim3(FTHREADS), 0, (hipStream_t)stream, wave, woff,
                       (unsigned *)peak);
    KK_LAUNCH_CHECK("kk_feat_peak");
    return 0;
}

extern "C" int kk_feat_mel(const float *wave, const int64_t *woff, const float *peak, const int *moff, const int *tiles, int ntiles,
                           const void *tw, const float *win, const float *fb, const int *span, float *logmel, float *linmel, float *eraw,
                           void *stream) {
    KK_REQUIRE(wave && woff && peak && moff && tiles && tw && win && fb && span && logmel && eraw && ntiles > 0, "kk_feat_mel: bad args");
    MelArgs m{wave, woff, peak, moff, (const int2 *)tiles, (const float2 *)tw, win, fb, (const int2 *)span, logmel, linmel, eraw};
    kk_note_kernel("feat_mel");
    hipLaunchKernelGGL(feat_mel_kernel, dim3(ntiles), dim3(FTHREADS), 0, (hipStream_t)stream, m);
    KK_LAUNCH_CHECK("kk_feat_mel");
    return 0;
}

extern "C" int kk_feat_pitch(const float *wave, const int64_t *woff, const float *peak, const int *poff, const int *frames, int nframes,
                             const float *win, float *cand, float *acmax, float *msq, void *stream) {
    KK_REQUIRE(wave && woff && peak && poff && frames && win && cand && acmax && msq && nframes > 0, "kk_feat_pitch: bad args");
    PitchArgs p{wave, woff, peak, poff, (const int2 *)frames, win, cand, acmax, msq};
    kk_note_kernel("feat_pitch");
    hipLaunchKernelGGL(feat_pitch_kernel, dim3(nframes), dim3(FTHREADS), 0, (hipStream_t)stream, p);
    KK_LAUNCH_CHECK("kk_feat_pitch");
    return 0;
}

extern "C" int kk_feat_finish(const int *moff, const int *poff, int B, const float *eraw, const float *cand, const float *acmax,
                              const float *msq, float *scratch_a, float *scratch_b, float *pitch, float *energy, int variance,
                              void *stream) {
    KK_REQUIRE(moff && poff && B > 0 && eraw && pitch && energy, "kk_feat_finish: bad args");
    KK_REQUIRE(!variance || (cand && acmax && msq && scratch_a && scratch_b), "kk_feat_finish: variance needs the pitch kernel's outputs");
    FinArgs f{moff, poff, eraw, cand, acmax, msq, scratch_a, scratch_b, pitch, energy, variance};
    kk_note_kernel("feat_finish");
    hipLaunchKernelGGL(feat_finish_kernel, dim3(B), dim3(FTHREADS), 0, (hipStream_t)stream, f);
    KK_LAUNCH_CHECK("kk_feat_finish");
    return 0;
}
