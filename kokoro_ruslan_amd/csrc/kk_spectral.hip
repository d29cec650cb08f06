// Spectral distance of two waveforms along a DTW path (kokoro_ruslan_amd/spectral.py): what the vocoded audio of an evaluation is
// judged by against the speaker's recording, along the alignment kk_dtw.hip found for the mels.
//
// A ragged batch of B pairs: side a (synthesized) and side b (the recording) are fp32 waveforms packed back to back (woffa / woffb:
// int64 sample offsets), each read as x / (peak + 1e-9), the feature extractor's scaling of audio (kk_features.hip).  The path of pair b is
// steps[b] entries (i, j) in mel frames from entry poff[b] of the packed path (kk_dtw_backtrack's layout); frame i is centred on sample
// 256 i, reflect padding by index (kk_fft.h).  A step is SKIPPED when i is outside [0, Ta), j outside [0, Tb) (aoff / boff: the mel
// frames of the pair) or a frame centre lies past its waveform (256 i > n): nothing is read for it.
//
// At a counted step and for each of three analysis windows (a periodic Hann of 256, 512, 1024 centred in the 1024-sample frame: one
// 1024-point transform serves all three, win: [3][1024]) with A = |STFT(a)|[i], B = |STFT(b)|[j] over the 513 bins:
//     sum A B,  sum A^2,  sum B^2,  sum d,  sum d^2,   d = 10 log10((A^2 + 1e-9) / (B^2 + 1e-9))
// Everything is fp64: the samples are read as (double) x / ((double) peak + 1e-9), the windows and twiddles come as fp64 tables, the
// transform is kk_fft.h's instantiated for double2 (one wave64 per frame: stft_frame_fwd and the split step) and so is every sum.
// The sums of d weigh every bin alike, so the quiet bins beside a loud harmonic decide them, and there an fp32 transform's rounding
// (relative to the loud bin) is 1e-4 of the bin itself; in fp64 the kernel computes what the definition says.
//
//  spectral        a workgroup owns SP_TILE consecutive steps of one pair (tiles: {pair, first step}, built by the host over the room
//                  each pair has in the packed path; a tile at or past steps[b] does nothing).  Wave w takes the tile's steps
//                  8 w .. 8 w + 7 in order; a side whose frame index repeats from the step before keeps its three power spectra
//                  (in LDS, each lane its own bins: neighbouring steps of a DTW path repeat i or j two times in three).  A lane sums its bins
//                  (lane + 64 m, m ascending; lane 0 then bin 512) over windows and steps in that order, the wave reduces its lanes
//                  as a fixed shuffle tree and thread q adds the four waves' sum q in wave order into part[tile][q].
//  finish          thread q of pair b's workgroup adds part[.][q] of the pair's tiles in ascending order into sums[q][b]; counts too.
// Which steps a tile, a wave and a lane take depends on the pair's own step count alone: a pair's outputs are bit for bit what it
// gives alone.  This file owns the tiles, the skip rule and the sums.
#include "kk_common.h"
#include "kk_fft.h"

namespace {

constexpr int SP_TILE = 32;                                   // path steps of one workgroup
constexpr int SP_THREADS = 256, SP_WAVES = SP_THREADS / 64, SP_CHUNK = SP_TILE / SP_WAVES;
constexpr int SP_WINDOWS = 3, SP_SUMS = 5 * SP_WINDOWS;
constexpr int SP_MAX_STEPS = 8191;                            // Ta + Tb - 1 of the longest pair the DP takes

struct SpecArgs {
    const float *wa, *wb;                     // packed waveforms
    const int64_t *woffa, *woffb;             // [B + 1] sample offsets
    const float *peaka, *peakb;               // [B] max |x|
    const int *aoff, *boff;                   // [B + 1] mel frame offsets: Ta, Tb
    const int *path;                          // [.][2]
    const int64_t *poff;                      // [B + 1] first path entry
    const int *steps;                         // [B]
    int B;
    const int2 *tiles;                        // {pair, first step}
    int ntiles;
    const int *toff;                          // [B + 1] first tile of each pair
    const double *win;                        // [3][1024]
    const double2 *tw;
    double *part;                             // [ntiles][15]
    int *pcnt;                                // [ntiles][2]
    double *sums;                             // [15][B]: window-major, {AB, AA, BB, d, d^2}
    int *counts;                              // [2][B]: counted steps, skipped steps
};

// steps of pair b that are walked: steps[b] held to the room the pair has in the packed path
__device__ __forceinline__ int spec_steps(const SpecArgs &a, int b) {
    const int64_t room = a.poff[b + 1] - a.poff[b];
    return (int)max((int64_t)0, min(min((int64_t)a.steps[b], room), (int64_t)SP_MAX_STEPS));
}

constexpr int SP_PROW = STFT_BINS + 7;                        // doubles of one power spectrum in LDS

// The three power spectra of frame t of x[0 .. n) / d into p[3][SP_PROW]; a lane writes the bins it later reads (lane + 64 m; lane 0
// also bin 512).  n >= 1024 and 256 t <= n (the caller's skip rule): stft_frame_fwd's domain.
__device__ __forceinline__ void spec_power(const float *__restrict__ x, double d, int t, int n, const double *__restrict__ win, double2 *sl,
                                           const StftTwT<double2> &tw, int lane, double *p) {
#pragma unroll 1
    for (int w = 0; w < SP_WINDOWS; ++w) {
        stft_frame_fwd([&](int j) { return (double)x[j] / d; }, t, n, win + w * STFT_N, sl, tw, lane);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const double2 X = stft_split(sl, tw.twk[m], lane + 64 * m);
            p[w * SP_PROW + lane + 64 * m] = X.x * X.x + X.y * X.y;
        }
        if (lane == 0) {
            const double2 N = stft_bin512(sl);
            p[w * SP_PROW + STFT_N / 2] = N.x * N.x + N.y * N.y;
        }
    }
}

__device__ __forceinline__ void spec_acc(double *s, double a2, double b2) {
    s[0] += sqrt(a2 * b2);                                    // A B (A^2 where the two are the same value: sqrt(x x) = x)
    s[1] += a2;
    s[2] += b2;
    const double d = 10.0 * log10((a2 + 1e-9) / (b2 + 1e-9));
    s[3] += d;
    s[4] += d * d;
}

__global__ __launch_bounds__(SP_THREADS) void dtw_spectral_kernel(const SpecArgs a) {
    __shared__ __attribute__((aligned(16))) double2 slot[SP_WAVES][STFT_N / 2];
    __shared__ double pw[SP_WAVES][2][SP_WINDOWS * SP_PROW];           // the power spectra of the wave's current frames of a and of b
    __shared__ double wsum[SP_WAVES][SP_SUMS];
    __shared__ int wcnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int2 tl = a.tiles[blockIdx.x];
    const int b = tl.x, s0 = tl.y;
    if ((unsigned)b >= (unsigned)a.B || s0 < 0) return;               // (uniform, before any barrier; the host builds the tiles)
    const int n = spec_steps(a, b);
    if (s0 >= n) return;                                              // (the finish pass reads the tiles below ceil(n / SP_TILE) only)
    const int Ta = a.aoff[b + 1] - a.aoff[b], Tb = a.boff[b + 1] - a.boff[b];
    const int64_t la = a.woffa[b + 1] - a.woffa[b], lb = a.woffb[b + 1] - a.woffb[b];
    const bool sides_ok = la >= STFT_N && la <= 0x7fffffff - STFT_N && lb >= STFT_N && lb <= 0x7fffffff - STFT_N;   // (the host refuses others)
    const int na = sides_ok ? (int)la : 0, nb = sides_ok ? (int)lb : 0;
    const float *xa = a.wa + a.woffa[b], *xb = a.wb + a.woffb[b];
    const double da = (double)a.peaka[b] + 1e-9, db = (double)a.peakb[b] + 1e-9;
    const int *path = a.path + 2 * a.poff[b];

    StftTwT<double2> tw;
    stft_twiddles(a.tw, lane, tw);
    double2 *sl = slot[wv];
    double acc[SP_SUMS];
#pragma unroll
    for (int q = 0; q < SP_SUMS; ++q) acc[q] = 0.0;
    int counted = 0, skipped = 0, ia = -1, jb = -1;
    double *pa = pw[wv][0], *pb = pw[wv][1];
    const int c0 = s0 + SP_CHUNK * wv, c1 = min(min(c0 + SP_CHUNK, s0 + SP_TILE), n);
#pragma unroll 1
    for (int s = c0; s < c1; ++s) {
        const int i = __builtin_amdgcn_readfirstlane(path[2 * s]), j = __builtin_amdgcn_readfirstlane(path[2 * s + 1]);
        // nothing is read for a step outside the pair: i < Ta, j < Tb, and the frame centres 256 i <= na, 256 j <= nb
        if (!sides_ok || (unsigned)i >= (unsigned)Ta || (unsigned)j >= (unsigned)Tb || i > na / STFT_HOP || j > nb / STFT_HOP) {
            ++skipped;
            continue;
        }
        if (i != ia) spec_power(xa, da, i, na, a.win, sl, tw, lane, pa), ia = i;
        if (j != jb) spec_power(xb, db, j, nb, a.win, sl, tw, lane, pb), jb = j;
        ++counted;
#pragma unroll
        for (int w = 0; w < SP_WINDOWS; ++w) {
            const int last = lane == 0 ? 8 : 7;                       // (lane 0: bin 512 after its eight)
#pragma unroll 1
            for (int m = 0; m <= last; ++m) spec_acc(acc + 5 * w, pa[w * SP_PROW + lane + 64 * m], pb[w * SP_PROW + lane + 64 * m]);
        }
    }
#pragma unroll
    for (int q = 0; q < SP_SUMS; ++q) {
        double v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);     // lane 0: a fixed tree over the wave
        if (lane == 0) wsum[wv][q] = v;
    }
    if (lane == 0) wcnt[wv][0] = counted, wcnt[wv][1] = skipped;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < SP_SUMS) a.part[(int64_t)blockIdx.x * SP_SUMS + t] = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
    else if (t < SP_SUMS + 2) {
        const int c = t - SP_SUMS;
        a.pcnt[2 * (int64_t)blockIdx.x + c] = ((wcnt[0][c] + wcnt[1][c]) + wcnt[2][c]) + wcnt[3][c];
    }
}

__global__ __launch_bounds__(64) void dtw_spectral_finish_kernel(const SpecArgs a) {
    const int b = blockIdx.x, q = threadIdx.x;
    const int n = spec_steps(a, b);
    const int t0 = a.toff[b];
    int nt = min((n + SP_TILE - 1) / SP_TILE, a.toff[b + 1] - t0);
    if (t0 < 0 || nt < 0 || t0 + nt > a.ntiles) nt = 0;               // (nothing is read outside the partial sums)
    if (q < SP_SUMS) {
        double s = 0.0;
        for (int t = 0; t < nt; ++t) s += a.part[(int64_t)(t0 + t) * SP_SUMS + q];
        a.sums[(int64_t)q * a.B + b] = s;
    } else if (q < SP_SUMS + 2) {
        int c = 0;
        for (int t = 0; t < nt; ++t) c += a.pcnt[2 * (int64_t)(t0 + t) + (q - SP_SUMS)];
        a.counts[(int64_t)(q - SP_SUMS) * a.B + b] = c;
    }
}

}  // namespace

extern "C" int kk_dtw_spectral_tile(void) { return SP_TILE; }

extern "C" int kk_dtw_spectral_stats(const float *wa, const int64_t *woffa, const float *peaka, const float *wb, const int64_t *woffb,
                                     const float *peakb, const int *aoff, const int *boff, const int *path, const int64_t *poff,
                                     const int *steps, int B, const int *tiles, int ntiles, const int *toff, const double *win,
                                     const void *tw, double *part, int *part_counts, double *sums, int *counts, void *stream) {
    KK_REQUIRE(wa && woffa && peaka && wb && woffb && peakb && aoff && boff && path && poff && steps && tiles && toff && win && tw && part &&
                   part_counts && sums && counts && B > 0 && ntiles > 0,
               "kk_dtw_spectral_stats: bad args");
    SpecArgs r{wa, wb, woffa, woffb, peaka, peakb, aoff, boff, path, poff, steps, B, (const int2 *)tiles, ntiles, toff, win,
               (const double2 *)tw, part, part_counts, sums, counts};
    kk_note_kernel("dtw_spectral");
    hipLaunchKernelGGL(dtw_spectral_kernel, dim3(ntiles), dim3(SP_THREADS), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_dtw_spectral_stats");
    hipLaunchKernelGGL(dtw_spectral_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_dtw_spectral_stats (finish)");
    return 0;
}
