// Griffin-Lim kernels (kokoro_ruslan_amd/griffinlim.py): a batch of log-mels to waveforms on the device, with n_fft = win = 1024,
// hop = 256, periodic Hann window, center = True, reflect padding, onesided (the reference's torchaudio GriffinLim settings).
//
//  init       S = sqrt(relu(pinv(fb^T) . exp(mel))) per frame (513 bins from 80 mels, fp32), Y = S . angles0, rebuilt = 0
//  iterate    one launch per Griffin-Lim iteration: x = istft(Y); X = stft(x); c = X - beta . rebuilt; rebuilt = X;
//             Y' = S . c / (|c| + 1e-16)
//  istft      the final waveform istft(Y) (the iterate kernel's first half)
//
// Layout: spectra are [frames, 513] complex (float2), S is [frames, 513] fp32.  The utterances of a batch are packed back to back
// along frames with no padding.  Work is split into tiles of GTF frames of ONE utterance (a host-built table of {start, frames,
// f0, wave offset}); a tile's inverse FFTs cover its frames and a halo of 3 frames on each side (n_fft / hop - 1), clipped to the
// utterance (4 on the left for a one-frame last tile), which is every frame that overlaps the samples the tile's forward frames
// read, reflect padding included.
//
// This file owns the tile and halo bookkeeping, the xs array the forward frames read, and the per-bin work: the k = 0 clearing of the
// imaginary parts on the way in, momentum and normalisation on the way out.  The transforms themselves (forward frame, split step with
// bin 512 on lane 0, inverse pre-step and tail, overlap-add of one position) are kk_fft.h's, one wave64 per frame.  Twiddles and the
// window come from host tables computed in fp64.
//
// Determinism: every sum runs in an order fixed by the frame's (or sample's) position in its own utterance: the overlap-add of a
// sample sums its frames in ascending order whichever tile computes it.  So a waveform's bits do not depend on the rest of the batch.
#include "kk_common.h"
#include "kk_fft.h"

namespace {

constexpr int GMELS = 80;
constexpr int GTF = 8, GHALO = 3, GHF = GTF + 2 * GHALO;     // tile frames, halo frames per side, inverse FFTs per tile (at most)
constexpr int GXS = GHF * STFT_HOP + STFT_N - STFT_HOP;      // samples the halo frames cover
constexpr int GTHREADS = 256, GWAVES = GTHREADS / 64;
constexpr int GINIT_F = 8;                                   // frames per init workgroup

struct GlIter {
    const float2 *yin;     // [frames, 513]
    float2 *yout;          // [frames, 513] (iterate) — ping-pong: neighbouring tiles read yin
    float2 *reb;           // [frames, 513] rebuilt of the previous iteration, overwritten with this one's (iterate)
    const float *S;        // [frames, 513] (iterate)
    const int4 *tiles;     // {utterance start frame, utterance frames, first frame of the tile, utterance's first wave sample}
    const float2 *tw;      // exp(-2 pi i j / 1024), j < 1024
    const float *win;      // periodic Hann, 1024
    float *wave;           // packed waveform, 256 (frames_b - 1) samples per utterance (istft)
    float beta;            // momentum / (1 + momentum); 0: no momentum term
    int final_istft;
};

__global__ __launch_bounds__(GTHREADS) void gl_init_kernel(const float *__restrict__ mel, int64_t frames, const float *__restrict__ pinv,
                                                           const float2 *__restrict__ ang, float *__restrict__ S, float2 *__restrict__ Y,
                                                           float2 *__restrict__ R) {
    __shared__ float e[GINIT_F][GMELS];
    const int64_t r0 = (int64_t)blockIdx.x * GINIT_F;
    for (int i = threadIdx.x; i < GINIT_F * GMELS; i += GTHREADS) {
        const int f = i / GMELS, m = i % GMELS;
        e[f][m] = r0 + f < frames ? expf(mel[(r0 + f) * GMELS + m]) : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < STFT_BINS; k += GTHREADS) {
        float acc[GINIT_F];
#pragma unroll
        for (int f = 0; f < GINIT_F; ++f) acc[f] = 0.f;
        const float *pr = pinv + k * GMELS;
        for (int m = 0; m < GMELS; ++m) {
            const float w = pr[m];
#pragma unroll
            for (int f = 0; f < GINIT_F; ++f) acc[f] = fmaf(w, e[f][m], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < GINIT_F; ++f) {
            const int64_t row = r0 + f;
            if (row >= frames) break;
            const int64_t i = row * STFT_BINS + k;
            const float s = sqrtf(fmaxf(acc[f], 0.f));
            const float2 a = ang ? ang[i] : make_float2(1.f, 0.f);
            S[i] = s;
            Y[i] = make_float2(s * a.x, s * a.y);
            R[i] = make_float2(0.f, 0.f);
        }
    }
}

__global__ __launch_bounds__(GTHREADS) void gl_iter_kernel(const GlIter a) {
    __shared__ __attribute__((aligned(16))) float frm[GHF][STFT_N]; // windowed inverse FFTs of the halo frames; then FFT slots
    __shared__ float xs[GXS];                                       // istft samples the tile reads, by overlap-add position
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int4 tl = a.tiles[blockIdx.x];
    const int start = tl.x, T = tl.y, f0 = tl.z;
    // the reflection at the end reads sample 256 (T - 1) - 1, which frames T - 5 .. T - 2 cover: a one-frame last tile reaches 4 back
    const int f1 = min(f0 + GTF, T), h0 = max(min(f0 - GHALO, T - 5), 0), h1 = min(f1 + GHALO, T);
    const int pbase = h0 * STFT_HOP, L = STFT_HOP * (T - 1);

    StftTw tw;
    stft_twiddles(a.tw, lane, tw);

    // 1. inverse real FFTs of the halo frames, windowed, into frm
    for (int i = wave; i < h1 - h0; i += GWAVES) {
        const float2 *yr = a.yin + (int64_t)(start + h0 + i) * STFT_BINS;
        float2 v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int k = lane + 64 * m;
            float2 xk = yr[k], xm = yr[STFT_N / 2 - k];
            if (k == 0) { xk.y = 0.f; xm.y = 0.f; }               // c2r ignores the imaginary parts of bins 0 and 512
            v[m] = stft_inv_pre(xk, xm, tw.twk[m]);
        }
        stft_inv_tail(v, reinterpret_cast<float2 *>(frm[i]), a.win, tw, lane);
    }
    __syncthreads();

    // 2. overlap-add / window-square envelope at every position the halo frames cover, inside the trimmed signal [512, 256 T + 256)
    const int nxs = (h1 - h0) * STFT_HOP + STFT_N - STFT_HOP;
    for (int idx = threadIdx.x; idx < nxs; idx += GTHREADS) {
        const int p = pbase + idx;
        if (p < STFT_N / 2 || p >= STFT_HOP * T + STFT_HOP) continue;
        const int tlo = max(p >= STFT_N ? (p - STFT_N) / STFT_HOP + 1 : 0, h0), thi = min(min(T - 1, p / STFT_HOP), h1 - 1);
        if (tlo > thi) continue;                                    // no halo frame here: never read
        xs[idx] = stft_ola(frm, h0, tlo, thi, p, a.win);
    }
    __syncthreads();

    if (a.final_istft) {                                            // 3'. the tile's own samples [256 f0, 256 f1) of the waveform
        const int j1 = min(STFT_HOP * f1, L);
        for (int j = STFT_HOP * f0 + threadIdx.x; j < j1; j += GTHREADS) a.wave[tl.w + j] = xs[j + STFT_N / 2 - pbase];
        return;
    }

    // 3. forward real FFTs of the tile's frames (reflect padding at the utterance's ends), momentum, normalisation
    float2 *sl = reinterpret_cast<float2 *>(frm[wave]);            // frm is free now: one exchange slot per wave
    for (int i = wave; i < f1 - f0; i += GWAVES) {
        const int t = f0 + i;
        stft_frame_fwd([&](int j) { return xs[j + STFT_N / 2 - pbase]; }, t, L, a.win, sl, tw, lane);
        const int64_t row = (int64_t)(start + t) * STFT_BINS;
#pragma unroll
        for (int j = 0; j <= 8; ++j) {
            if (j == 8 && lane != 0) break;
            const int k = j < 8 ? lane + 64 * j : STFT_N / 2;
            const float2 X = j < 8 ? stft_split(sl, tw.twk[j], k) : stft_bin512(sl);
            float2 c = X;
            if (a.beta != 0.f) {
                const float2 p = a.reb[row + k];
                c = make_float2(X.x - a.beta * p.x, X.y - a.beta * p.y);
            }
            a.reb[row + k] = X;
            const float d = sqrtf(c.x * c.x + c.y * c.y) + 1e-16f;
            const float s = a.S[row + k];
            a.yout[row + k] = make_float2(s * (c.x / d), s * (c.y / d));
        }
    }
}

int launch_iter(const GlIter &g, int ntiles, hipStream_t s, const char *name) {
    kk_note_kernel(g.final_istft ? "gl_istft" : "gl_iter");
    hipLaunchKernelGGL(gl_iter_kernel, dim3(ntiles), dim3(GTHREADS), 0, s, g);
    KK_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

extern "C" int kk_gl_tile_frames(void) { return GTF; }

extern "C" int kk_gl_init(const float *mel, int64_t frames, const float *pinv, const void *angles, float *S, void *Y, void *rebuilt,
                          void *stream) {
    KK_REQUIRE(mel && pinv && S && Y && rebuilt && frames > 0, "kk_gl_init: bad args");
    kk_note_kernel("gl_init");
    hipLaunchKernelGGL(gl_init_kernel, dim3(kk_cdiv(frames, GINIT_F)), dim3(GTHREADS), 0, (hipStream_t)stream, mel, frames, pinv,
                       (const float2 *)angles, S, (float2 *)Y, (float2 *)rebuilt);
    KK_LAUNCH_CHECK("kk_gl_init");
    return 0;
}

extern "C" int kk_gl_iter(const void *y_in, void *y_out, void *rebuilt, const float *S, const int *tiles, int ntiles, const void *tw,
                          const float *win, float beta, void *stream) {
    KK_REQUIRE(y_in && y_out && rebuilt && S && tiles && tw && win && ntiles > 0 && y_in != y_out,
               "kk_gl_iter: bad args (y_in != y_out: neighbouring tiles read the old spectrum)");
    GlIter g{(const float2 *)y_in, (float2 *)y_out, (float2 *)rebuilt, S, (const int4 *)tiles, (const float2 *)tw, win, nullptr, beta, 0};
    return launch_iter(g, ntiles, (hipStream_t)stream, "kk_gl_iter");
}

extern "C" int kk_gl_istft(const void *y, const int *tiles, int ntiles, const void *tw, const float *win, float *wave, void *stream) {
    KK_REQUIRE(y && tiles && tw && win && wave && ntiles > 0, "kk_gl_istft: bad args");
    GlIter g{(const float2 *)y, nullptr, nullptr, nullptr, (const int4 *)tiles, (const float2 *)tw, win, wave, 0.f, 1};
    return launch_iter(g, ntiles, (hipStream_t)stream, "kk_gl_istft");
}
