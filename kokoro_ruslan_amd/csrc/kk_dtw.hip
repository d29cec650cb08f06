// Dynamic time warping of mel pairs (kokoro_ruslan_amd/dtw.py): the alignment behind MCD-DTW, the free-running evaluation's distance
// between a synthesized mel and its ground truth, which differ in length.
//
// A ragged batch of B pairs; side a (synthesized) and side b (ground truth) are packed back to back along time, aoff / boff (int32,
// B + 1) say where a pair's frames lie.  Four launches:
//   mcep        log-mel [T, M] -> cepstra c[k][t], k = 1..K: the orthonormal DCT-II without its 0th coefficient.  table[k - 1][m] =
//               fp32(sqrt(2 / M) cos(pi k (m + 0.5) / M)) comes from the host (fp64, rounded once); a frame's cepstrum is the fmaf
//               chain over ascending m of its own values, so identical frames give identical bits wherever they lie.  Laid out
//               [K][T_total]: the lanes of the DP walk a diagonal, consecutive i (and j) at consecutive addresses.
//   dtw         one workgroup per pair sweeps the anti-diagonals d = i + j of D(i, j) = dist(i, j) + min(D(i-1, j-1), D(i-1, j),
//               D(i, j-1)), dist = sqrt(sum_k (ca_k[i] - cb_k[j])^2).  The cells of a diagonal are independent; the last two diagonals
//               live in LDS indexed by i (three rotating rows of 4096 floats: the one written at d is read at d + 1 and d + 2 and
//               overwritten at d + 3, so one barrier per diagonal orders everything).  A diagonal wider than the workgroup is covered
//               in passes of DTW_W cells.  The predecessor chosen (0 diagonal, 1 (i-1, j), 2 (i, j-1); a later one only when strictly
//               smaller) goes out as 2 bits, 16 cells of a row per 32-bit word: the word of row i grows in LDS over 16 diagonals and is
//               stored when its last cell is done.
//   backtrack   one wave per pair: lane 0 walks the direction words from (Ta-1, Tb-1) to (0, 0) into LDS, then the wave writes the
//               path out in forward order.
//   path_stats  one workgroup per pair: thread t takes the steps t, t + 256, ... of the path and the workgroup reduces the partial
//               sums as a fixed tree.  These two sums are formed in fp64 from the fp32 cepstra / log-mels: a 13-term fp32 sum of
//               squares alone can miss the one-ulp-per-step accuracy asked of them on a one-step path, and the launch is O(steps).
//   track_stats the same walk over two scalar tracks per side (pitch and energy of the audio, kokoro.inference.evaluate): the voicing
//               counts, the gross pitch errors, the sums of the F0 difference in cents and of its square over the steps voiced on
//               both sides, the sum of |energy difference| over all steps.  Frequencies, differences and the comparisons are fp64
//               with every operation rounded on its own (no contraction into fma), so the counts are those of any IEEE evaluation of
//               the same expressions; only log2 is not correctly rounded, and it feeds the two cent sums alone.
// Nothing a pair computes depends on the other pairs: every output is bit for bit what the pair gives alone.
#include "kk_common.h"

namespace {

constexpr int DTW_W = 1024;                   // workgroup size of the DP = cells of a diagonal per pass
constexpr int DTW_MAX = 4096;                 // longest side (the positional table's order)
constexpr int MCEP_FRAMES = 64;               // frames per workgroup of mcep_kernel
constexpr int MCEP_THREADS = 256;
constexpr int MCEP_MAX_M = 128;
constexpr int STATS_THREADS = 256;

__global__ __launch_bounds__(MCEP_THREADS) void mcep_kernel(const float *__restrict__ mel, int64_t T, int M, int K,
                                                            const float *__restrict__ table, float *__restrict__ cep) {
    __shared__ float xs[MCEP_FRAMES * (MCEP_MAX_M + 1)];              // row stride M + 1: lanes of a wave read one column conflict-free
    const int64_t t0 = (int64_t)blockIdx.x * MCEP_FRAMES;
    const int nf = (int)min((int64_t)MCEP_FRAMES, T - t0);
    for (int e = threadIdx.x; e < nf * M; e += MCEP_THREADS) xs[(e / M) * (M + 1) + e % M] = mel[t0 * M + e];
    __syncthreads();
    const int f = threadIdx.x & 63, w = threadIdx.x >> 6;             // lane = frame, wave = coefficient (table reads are wave-uniform)
    if (f >= nf) return;
    const float *x = xs + f * (M + 1);
    for (int k = w; k < K; k += MCEP_THREADS / 64) {
        const float *c = table + k * M;
        float acc = 0.f;
        for (int m = 0; m < M; ++m) acc = fmaf(x[m], c[m], acc);
        cep[(int64_t)k * T + t0 + f] = acc;
    }
}

struct DtwArgs {
    const float *ca, *cb;                     // [K][Ta_total], [K][Tb_total]
    int64_t Ta_total, Tb_total;
    int K;
    const int *aoff, *boff;
    const int64_t *doff;                      // first direction word of each pair
    float *total;
    uint32_t *dir;
};

__device__ inline float dtw_dist(const float *__restrict__ pa, int64_t sa, const float *__restrict__ pb, int64_t sb, int K) {
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 8) {                               // eight coefficients' loads in flight, then the chain in order
        float x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = min(k0 + u, K - 1);
            x[u] = pa[k * sa], y[u] = pb[k * sb];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + u < K) {
                const float v = x[u] - y[u];
                acc = fmaf(v, v, acc);
            }
    }
    return sqrtf(acc);
}

__global__ __launch_bounds__(DTW_W) void dtw_kernel(const DtwArgs a) {
    __shared__ float diag[3][DTW_MAX];
    __shared__ uint32_t dirw[DTW_MAX];
    const int b = blockIdx.x;
    const int a0 = a.aoff[b], Ta = a.aoff[b + 1] - a0, b0 = a.boff[b], Tb = a.boff[b + 1] - b0;
    if (Ta < 1 || Tb < 1 || Ta > DTW_MAX || Tb > DTW_MAX) return;     // (the host checks; nothing is read or written past the LDS rows)
    const int wpr = (Tb + 15) >> 4;                                   // direction words per row
    uint32_t *dir = a.dir + a.doff[b];
    const float *ca = a.ca + a0, *cb = a.cb + b0;
    const float inf = __builtin_inff();
    float *cur = diag[0], *p1 = diag[1], *p2 = diag[2];               // this diagonal, the one before, the one before that
    for (int d = 0; d < Ta + Tb - 1; ++d) {
        const int lo = max(0, d - Tb + 1), hi = min(d, Ta - 1);
        for (int i = lo + (int)threadIdx.x; i <= hi; i += DTW_W) {
            const int j = d - i;
            const float dist = dtw_dist(ca + i, a.Ta_total, cb + j, a.Tb_total, a.K);
            float best = (i > 0 && j > 0) ? p2[i - 1] : inf;
            uint32_t code = 0;
            const float up = i > 0 ? p1[i - 1] : inf, left = j > 0 ? p1[i] : inf;
            if (up < best) best = up, code = 1;
            if (left < best) best = left, code = 2;
            const float D = d == 0 ? dist : dist + best;
            cur[i] = D;
            const int c = j & 15;
            const uint32_t w = (c ? dirw[i] : 0u) | (code << (2 * c));
            if (c == 15 || j == Tb - 1) dir[(int64_t)i * wpr + (j >> 4)] = w;
            else dirw[i] = w;
            if (d == Ta + Tb - 2) a.total[b] = D;
        }
        __syncthreads();
        float *t = p2;
        p2 = p1, p1 = cur, cur = t;
    }
}

__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const uint32_t *__restrict__ dirs, const int64_t *__restrict__ doff,
                                                           const int *__restrict__ aoff, const int *__restrict__ boff,
                                                           const int64_t *__restrict__ poff, int *__restrict__ path,
                                                           int *__restrict__ steps) {
    __shared__ uint32_t cells[2 * DTW_MAX];                           // i | j << 16, from the end of the path backwards
    __shared__ int count;
    const int b = blockIdx.x;
    const int Ta = aoff[b + 1] - aoff[b], Tb = boff[b + 1] - boff[b];
    if (Ta < 1 || Tb < 1 || Ta > DTW_MAX || Tb > DTW_MAX) return;
    if (threadIdx.x == 0) {
        const uint32_t *dir = dirs + doff[b];
        const int wpr = (Tb + 15) >> 4;
        int i = Ta - 1, j = Tb - 1, n = 0;
        int64_t have = -1;
        uint32_t w = 0;
        for (;;) {
            cells[n++] = (uint32_t)i | ((uint32_t)j << 16);
            if (i == 0 && j == 0) break;
            const int64_t at = (int64_t)i * wpr + (j >> 4);
            if (at != have) w = dir[at], have = at;
            uint32_t code = (w >> (2 * (j & 15))) & 3u;
            if (i == 0) code = 2;                                     // the edges have one way on, whatever the word says
            else if (j == 0) code = 1;
            if (code != 2) --i;
            if (code != 1) --j;
        }
        count = n;
    }
    __syncthreads();
    const int n = count;
    int *out = path + 2 * poff[b];
    for (int s = threadIdx.x; s < n; s += 64) {
        const uint32_t c = cells[n - 1 - s];
        out[2 * s] = (int)(c & 0xffffu);
        out[2 * s + 1] = (int)(c >> 16);
    }
    if (threadIdx.x == 0) steps[b] = n;
}

struct StatsArgs {
    const float *ca, *cb;
    int64_t Ta_total, Tb_total;
    int K;
    const float *xa, *xb;                     // log-mels [T_total, M]
    int M;
    const int *aoff, *boff;
    const int *path;
    const int64_t *poff;
    const int *steps;
    double *mcd_sum, *l1_sum;
};

__global__ __launch_bounds__(STATS_THREADS) void dtw_path_stats_kernel(const StatsArgs a) {
    __shared__ double red[2][STATS_THREADS];
    const int b = blockIdx.x, n = a.steps[b];
    const int a0 = a.aoff[b], b0 = a.boff[b];
    const int *path = a.path + 2 * a.poff[b];
    double mcd = 0.0, l1 = 0.0;
    for (int s = threadIdx.x; s < n; s += STATS_THREADS) {
        const int i = path[2 * s], j = path[2 * s + 1];
        double acc = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const double v = (double)a.ca[k * a.Ta_total + a0 + i] - (double)a.cb[k * a.Tb_total + b0 + j];
            acc += v * v;
        }
        mcd += sqrt(acc);
        const float *xa = a.xa + (int64_t)(a0 + i) * a.M, *xb = a.xb + (int64_t)(b0 + j) * a.M;
        double s1 = 0.0;
        for (int m = 0; m < a.M; ++m) s1 += fabs((double)xa[m] - (double)xb[m]);
        l1 += s1 / a.M;
    }
    red[0][threadIdx.x] = mcd, red[1][threadIdx.x] = l1;
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[0][threadIdx.x] += red[0][threadIdx.x + h], red[1][threadIdx.x] += red[1][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.mcd_sum[b] = red[0][0] * (10.0 / 2.302585092994045684 * 1.4142135623730950488);
        a.l1_sum[b] = red[1][0];
    }
}

struct TrackArgs {
    const float *pa, *ea, *pb, *eb;           // normalised pitch and energy, [Ta_total] and [Tb_total]
    const int *aoff, *boff;
    const int *path;
    const int64_t *poff;
    const int *steps;
    double f_lo, f_span, gpe_ratio;
    int *counts;                              // [5][B]: n_vv, n_vu, n_uv, n_uu, n_gpe
    double *sums;                             // [3][B]: sum c, sum c^2 (both voiced), sum |ea - eb| (all steps)
    int B;
};

__global__ __launch_bounds__(STATS_THREADS) void dtw_track_stats_kernel(const TrackArgs a) {
#pragma clang fp contract(off)                // f_lo + f_span p and gpe_ratio fb are a product rounded, then a sum / a comparison
    __shared__ double red[3][STATS_THREADS];
    __shared__ int cnt[5][STATS_THREADS];
    const int b = blockIdx.x, n = a.steps[b];
    const int a0 = a.aoff[b], Ta = a.aoff[b + 1] - a0, b0 = a.boff[b], Tb = a.boff[b + 1] - b0;
    if (Ta < 1 || Tb < 1 || Ta > DTW_MAX || Tb > DTW_MAX || n < 1 || n > Ta + Tb - 1) return;      // (uniform: before any barrier)
    const int *path = a.path + 2 * a.poff[b];
    double sc = 0.0, sc2 = 0.0, se = 0.0;
    int vv = 0, vu = 0, uv = 0, uu = 0, gpe = 0;
    for (int s = threadIdx.x; s < n; s += STATS_THREADS) {
        const int i = path[2 * s], j = path[2 * s + 1];
        if ((unsigned)i >= (unsigned)Ta || (unsigned)j >= (unsigned)Tb) continue;                  // (nothing is read outside the pair)
        const float p = a.pa[a0 + i], q = a.pb[b0 + j];
        se += fabs((double)a.ea[a0 + i] - (double)a.eb[b0 + j]);
        const bool va = p > 0.f, vb = q > 0.f;
        if (va && vb) {
            const double fa = a.f_lo + a.f_span * (double)p, fb = a.f_lo + a.f_span * (double)q;
            const double c = 1200.0 * log2(fa / fb);
            sc += c, sc2 += c * c;
            ++vv;
            if (fabs(fa - fb) > a.gpe_ratio * fb) ++gpe;
        } else if (va) ++vu;
        else if (vb) ++uv;
        else ++uu;
    }
    const int t = threadIdx.x;
    red[0][t] = sc, red[1][t] = sc2, red[2][t] = se;
    cnt[0][t] = vv, cnt[1][t] = vu, cnt[2][t] = uv, cnt[3][t] = uu, cnt[4][t] = gpe;
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int q = 0; q < 3; ++q) red[q][t] += red[q][t + h];
#pragma unroll
            for (int q = 0; q < 5; ++q) cnt[q][t] += cnt[q][t + h];
        }
        __syncthreads();
    }
    if (t < 3) a.sums[(int64_t)t * a.B + b] = red[t][0];
    if (t < 5) a.counts[(int64_t)t * a.B + b] = cnt[t][0];
}

}  // namespace

extern "C" int kk_dtw_tile(void) { return DTW_W; }

extern "C" int kk_mcep(const float *mel, int64_t T_total, int M, int K, const float *table, float *cep, void *stream) {
    KK_REQUIRE(mel && table && cep && T_total > 0 && T_total < ((int64_t)1 << 31), "kk_mcep: bad args");
    KK_REQUIRE(M >= 1 && M <= MCEP_MAX_M && K >= 1 && K <= 32, "kk_mcep: M = %d, K = %d; needs 1 <= M <= %d and 1 <= K <= 32", M, K,
               MCEP_MAX_M);
    kk_note_kernel("mcep");
    hipLaunchKernelGGL(mcep_kernel, dim3(kk_cdiv(T_total, MCEP_FRAMES)), dim3(MCEP_THREADS), 0, (hipStream_t)stream, mel, T_total, M, K,
                       table, cep);
    KK_LAUNCH_CHECK("kk_mcep");
    return 0;
}

extern "C" int kk_dtw(const float *ca, int64_t Ta_total, const float *cb, int64_t Tb_total, int K, const int *aoff, const int *boff,
                      const int64_t *doff, int B, float *total, uint32_t *dir, void *stream) {
    KK_REQUIRE(ca && cb && aoff && boff && doff && total && dir && B > 0 && Ta_total > 0 && Tb_total > 0 && K >= 1 && K <= 32,
               "kk_dtw: bad args");
    DtwArgs r{ca, cb, Ta_total, Tb_total, K, aoff, boff, doff, total, dir};
    kk_note_kernel("dtw");
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(DTW_W), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_dtw");
    return 0;
}

extern "C" int kk_dtw_backtrack(const uint32_t *dir, const int64_t *doff, const int *aoff, const int *boff, const int64_t *poff, int B,
                                int *path, int *steps, void *stream) {
    KK_REQUIRE(dir && doff && aoff && boff && poff && path && steps && B > 0, "kk_dtw_backtrack: bad args");
    kk_note_kernel("dtw_backtrack");
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, dir, doff, aoff, boff, poff, path, steps);
    KK_LAUNCH_CHECK("kk_dtw_backtrack");
    return 0;
}

extern "C" int kk_dtw_path_stats(const float *ca, int64_t Ta_total, const float *cb, int64_t Tb_total, int K, const float *xa,
                                 const float *xb, int M, const int *aoff, const int *boff, const int *path, const int64_t *poff,
                                 const int *steps, int B, double *mcd_sum, double *l1_sum, void *stream) {
    KK_REQUIRE(ca && cb && xa && xb && aoff && boff && path && poff && steps && mcd_sum && l1_sum && B > 0 && K >= 1 && K <= 32 && M >= 1,
               "kk_dtw_path_stats: bad args");
    StatsArgs r{ca, cb, Ta_total, Tb_total, K, xa, xb, M, aoff, boff, path, poff, steps, mcd_sum, l1_sum};
    kk_note_kernel("dtw_path_stats");
    hipLaunchKernelGGL(dtw_path_stats_kernel, dim3(B), dim3(STATS_THREADS), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_dtw_path_stats");
    return 0;
}

extern "C" int kk_dtw_track_stats(const float *pa, const float *ea, const float *pb, const float *eb, const int *aoff, const int *boff,
                                  const int *path, const int64_t *poff, const int *steps, int B, double f_lo, double f_span,
                                  double gpe_ratio, int *counts, double *sums, void *stream) {
    KK_REQUIRE(pa && ea && pb && eb && aoff && boff && path && poff && steps && counts && sums && B > 0, "kk_dtw_track_stats: bad args");
    KK_REQUIRE(f_span > 0.0 && f_lo > 0.0 && gpe_ratio >= 0.0, "kk_dtw_track_stats: f_lo = %g, f_span = %g, gpe_ratio = %g; needs f_lo, f_span > 0 and gpe_ratio >= 0",
               f_lo, f_span, gpe_ratio);
    TrackArgs r{pa, ea, pb, eb, aoff, boff, path, poff, steps, f_lo, f_span, gpe_ratio, counts, sums, B};
    kk_note_kernel("dtw_track_stats");
    hipLaunchKernelGGL(dtw_track_stats_kernel, dim3(B), dim3(STATS_THREADS), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_dtw_track_stats");
    return 0;
}
