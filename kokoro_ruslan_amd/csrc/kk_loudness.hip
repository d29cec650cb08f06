// Edge trimming, ITU-R BS.1770-4 integrated loudness and gain of a ragged batch of mono waveforms packed back to back
// (kokoro_ruslan_amd/loudness.py; the definitions and their fp64 restatement: kokoro_ruslan_amd/loudness_torch.py).  Five launches, no
// host read between them:
//
//  loud_hop_energy  sum of squares of every 256-sample hop of every utterance: one wave per hop, the lane's four samples summed in
//                   ascending order, then the wave butterfly.  fp64.
//  loud_edges       one workgroup per utterance: the energy of frame t (samples [256 t - 512, 256 t + 512), zeros outside) is the sum of
//                   hops t - 2 .. t + 1 in that order; the loudest frame, the first and the last frame above its energy less top_db, and
//                   from them {start, end} with the margin.  The max, min and max over frames do not depend on an order.
//  loud_kweight     one THREAD per step of S = round(0.1 fs) samples of the trimmed range, counted from `start`: it runs the two
//                   K-weighting biquads (transposed direct form II, fp64) from zero state 2 S samples early - or from `start` itself,
//                   where the state IS zero - and sums the squares of its own S outputs in sample order.  The high-pass poles have
//                   radius exp(-2 pi 38.1 / fs), so what a zero-state start forgets after 0.2 s is exp(-48) of the state, below fp64.
//                   It also keeps the peak |x| of its samples and, where N = round(0.4 fs) is not 4 S (N - 4 S = r, |r| <= 2), the
//                   squares of its first r (r > 0) or its last -r (r < 0) sample positions.
//  loud_gate        one wave per utterance: block j is steps j .. j + 3 (+ the first r samples of step j + 4, or less the last -r of
//                   step j + 3), summed in that order; lane l takes blocks l, l + 64, ..., the 64 partial sums go through the wave
//                   butterfly: an order fixed by the block count alone.  Both gates, L, the gain and the peak ceiling.
//  loud_apply       out[woff[b] + i] = x[woff[b] + start + i] g for i < end - start: the trimmed, scaled utterance left-aligned in
//                   its own slot of a buffer with the input's layout, so no scan over the trimmed lengths is needed.
//
// Nothing is accumulated across utterances and no atomics touch a float: an utterance's results do not depend on the batch.
// Limits (the host refuses the rest): fs in [8000, 48000]; every utterance >= 1 sample (below N samples: L = -inf, gain 1); fewer than
// 2^31 samples in the batch.
#include "kk_common.h"

namespace {

constexpr int LHOP = 256;                                          // the trim's frame is four hops: 1024
constexpr int LTHREADS = 256;
constexpr double L_OFFSET = -0.691, L_ABS_GATE = -70.0, L_REL_GATE = -10.0;

// b with off[b] <= i < off[b + 1] (off ascending, off[0] = 0, i < off[B]); an empty utterance's range is skipped
template <typename T> __device__ __forceinline__ int loud_find(const T *__restrict__ off, int B, int64_t i) {
    int lo = 0, hi = B;                                            // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LTHREADS) void loud_hop_energy_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                                   const int *__restrict__ hoff, int B, int nhops,
                                                                   double *__restrict__ hopsq) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * (LTHREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (h >= nhops) return;
    const int b = loud_find(hoff, B, h);
    const int64_t base = woff[b], n = woff[b + 1] - base;
    const int64_t j0 = (int64_t)LHOP * (h - hoff[b]);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < LHOP / 64; ++k) {
        const int64_t j = j0 + lane + 64 * k;
        const double v = j < n ? (double)wave[base + j] : 0.0;
        acc += v * v;
    }
    acc = wave_sum_d(acc);
    if (lane == 0) hopsq[h] = acc;
}

__global__ __launch_bounds__(LTHREADS) void loud_edges_kernel(const double *__restrict__ hopsq, const int64_t *__restrict__ woff,
                                                              const int *__restrict__ hoff, double top_db, int margin,
                                                              int *__restrict__ se) {
    __shared__ double red[LTHREADS];
    __shared__ int first_s, last_s;
    const int b = blockIdx.x;
    const int64_t n = woff[b + 1] - woff[b];
    const int nh = hoff[b + 1] - hoff[b], T = 1 + (int)(n / LHOP);
    const double *hs = hopsq + hoff[b];
    auto energy = [&](int t) {
        double e = 0.0;
#pragma unroll
        for (int d = -2; d <= 1; ++d) {
            const int h = t + d;
            e += (h >= 0 && h < nh) ? hs[h] : 0.0;
        }
        return e;
    };
    double top = 0.0;
    for (int t = threadIdx.x; t < T; t += LTHREADS) top = fmax(top, energy(t));
    red[threadIdx.x] = top;
    if (threadIdx.x == 0) { first_s = T; last_s = -1; }
    __syncthreads();
    for (int o = LTHREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    top = red[0];
    const double thr = top * pow(10.0, -top_db / 10.0);           // 20 log10(rms_t / rms_max) > -top_db
    int first = T, last = -1;
    for (int t = threadIdx.x; t < T; t += LTHREADS)
        if (energy(t) > thr) { first = min(first, t); last = max(last, t); }
    if (last >= 0) { atomicMin(&first_s, first); atomicMax(&last_s, last); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t start = 0, end = n;
        if (top > 0.0 && last_s >= 0) {
            start = max((int64_t)0, (int64_t)first_s * LHOP - margin);
            end = min(n, ((int64_t)last_s + 1) * LHOP + margin);
        }
        se[2 * b] = (int)start;
        se[2 * b + 1] = (int)end;
    }
}

struct Biquad { double b0, b1, b2, a1, a2; };

__device__ __forceinline__ double loud_kw(const Biquad &p, const Biquad &q, double x, double (&s)[4]) {
    const double y1 = p.b0 * x + s[0];
    s[0] = p.b1 * x - p.a1 * y1 + s[1];
    s[1] = p.b2 * x - p.a2 * y1;
    const double y2 = q.b0 * y1 + s[2];
    s[2] = q.b1 * y1 - q.a1 * y2 + s[3];
    s[3] = q.b2 * y1 - q.a2 * y2;
    return y2;
}

constexpr int LCH = 8;      // samples loaded ahead of the recursion

__global__ __launch_bounds__(64) void loud_kweight_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                          const int *__restrict__ se, const int *__restrict__ soff, int B, int nsteps,
                                                          int S, int r, const double *__restrict__ coef, double *__restrict__ stepsq,
                                                          double *__restrict__ stepex, float *__restrict__ steppk) {
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= nsteps) return;
    const int b = loud_find(soff, B, gid), k = gid - soff[b];
    const int64_t base = woff[b], n = woff[b + 1] - base;
    const int64_t start = se[2 * b], end = se[2 * b + 1];
    if (start < 0 || end > n || start > end) return;               // (loud_edges and the host never make these)
    const int64_t lo = start + (int64_t)k * S, hi = min(lo + S, end);
    if (lo >= end) return;                                         // a step of the untrimmed length that the trim removed
    const Biquad p{coef[0], coef[1], coef[2], coef[3], coef[4]}, q{coef[5], coef[6], coef[7], coef[8], coef[9]};
    const float *x = wave + base;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t i0 = max(start, lo - 2 * (int64_t)S);
    // positions of this step whose squares also go to stepex: [0, r) for r > 0, [S + r, S) for r < 0
    const int64_t e0 = lo + (r > 0 ? 0 : (r < 0 ? S + r : 0)), e1 = lo + (r > 0 ? r : (r < 0 ? S : 0));
    double acc = 0.0, ex = 0.0;
    float pk = 0.f;
    float cur[LCH], nxt[LCH];
#pragma unroll
    for (int c = 0; c < LCH; ++c) cur[c] = i0 + c < hi ? x[i0 + c] : 0.f;
    for (int64_t i = i0; i < hi; i += LCH) {
#pragma unroll
        for (int c = 0; c < LCH; ++c) nxt[c] = i + LCH + c < hi ? x[i + LCH + c] : 0.f;
#pragma unroll
        for (int c = 0; c < LCH; ++c) {
            const int64_t j = i + c;
            if (j < hi) {
                const double y = loud_kw(p, q, (double)cur[c], s);
                if (j >= lo) {
                    acc += y * y;
                    pk = fmaxf(pk, fabsf(cur[c]));
                    if (j >= e0 && j < e1) ex += y * y;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < LCH; ++c) cur[c] = nxt[c];
    }
    stepsq[gid] = acc;
    stepex[gid] = ex;
    steppk[gid] = pk;
}

__device__ __forceinline__ double loud_lufs(double z) { return L_OFFSET + 10.0 * log10(z); }      // -inf at z = 0

__global__ __launch_bounds__(64) void loud_gate_kernel(const double *__restrict__ stepsq, const double *__restrict__ stepex,
                                                       const float *__restrict__ steppk, const int *__restrict__ se,
                                                       const int *__restrict__ soff, int S, int N, double target, double ceiling,
                                                       double *__restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t len = (int64_t)se[2 * b + 1] - se[2 * b];
    const int cap = soff[b + 1] - soff[b];                         // steps of the untrimmed utterance: what the arrays hold
    const int K = (int)min((int64_t)cap, len > 0 ? (len + S - 1) / S : 0);
    const int r = N - 4 * S;
    int nb = len >= N ? (int)((len - N) / S) + 1 : 0;
    nb = max(0, min(nb, K - (r > 0 ? 4 : 3)));                     // (never lowers it for a consistent {start, end}: bounds only)
    const double *sq = stepsq + soff[b], *ex = stepex + soff[b];
    auto z = [&](int j) {
        double t = ((sq[j] + sq[j + 1]) + sq[j + 2]) + sq[j + 3];
        if (r > 0) t += ex[j + 4];
        if (r < 0) t -= ex[j + 3];
        return t / (double)N;
    };
    float pk = 0.f;
    for (int k = lane; k < K; k += 64) pk = fmaxf(pk, steppk[soff[b] + k]);
    pk = wave_max(pk);
    double sum = 0.0, cnt = 0.0;
    for (int j = lane; j < nb; j += 64) {
        const double zj = z(j);
        if (loud_lufs(zj) > L_ABS_GATE) { sum += zj; cnt += 1.0; }
    }
    sum = wave_sum_d(sum);
    cnt = wave_sum_d(cnt);
    double L = -INFINITY;
    if (cnt > 0.0) {                                               // wave-uniform: the sums are the same in every lane
        const double rel = loud_lufs(sum / cnt) + L_REL_GATE;
        double sum2 = 0.0, cnt2 = 0.0;
        for (int j = lane; j < nb; j += 64) {
            const double zj = z(j), lj = loud_lufs(zj);
            if (lj > L_ABS_GATE && lj > rel) { sum2 += zj; cnt2 += 1.0; }
        }
        sum2 = wave_sum_d(sum2);
        cnt2 = wave_sum_d(cnt2);
        if (cnt2 > 0.0) L = loud_lufs(sum2 / cnt2);
    }
    if (lane == 0) {
        double g = 1.0, limited = 0.0;
        if (L > -INFINITY) {
            g = pow(10.0, (target - L) / 20.0);
            if (g * (double)pk > ceiling) { g = ceiling / (double)pk; limited = 1.0; }
        }
        float g32 = (float)g;
        if (limited != 0.0 && (double)g32 * (double)pk > ceiling) g32 = nextafterf(g32, 0.f);      // the ceiling holds after rounding
        stats[4 * b] = L;
        stats[4 * b + 1] = (double)g32;
        stats[4 * b + 2] = limited;
        stats[4 * b + 3] = (double)pk;
    }
}

constexpr int LAPPLY = 4;      // samples per thread

__global__ __launch_bounds__(LTHREADS) void loud_apply_kernel(const float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                              const int *__restrict__ se, const double *__restrict__ stats, int B,
                                                              int64_t total, float *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * (LTHREADS * LAPPLY) + threadIdx.x;
    if (i >= total) return;
    int b = loud_find(woff, B, i);
#pragma unroll
    for (int c = 0; c < LAPPLY; ++c, i += LTHREADS) {
        if (i >= total) return;
        while (i >= woff[b + 1]) ++b;                              // (i < total = woff[B]: ends at b < B)
        const int64_t base = woff[b], start = se[2 * b], end = se[2 * b + 1];
        const int64_t j = i - base;                                // position in the output slot
        if (start >= 0 && start <= end && end <= woff[b + 1] - base && j < end - start)
            out[i] = wave[base + start + j] * (float)stats[4 * b + 1];
    }
}

}  // namespace

extern "C" int kk_loud_hop_energy(const float *wave, const int64_t *woff, const int *hoff, int B, int nhops, double *hopsq,
                                  void *stream) {
    KK_REQUIRE(wave && woff && hoff && hopsq && B > 0 && nhops > 0, "kk_loud_hop_energy: bad args");
    kk_note_kernel("loud_hop_energy");
    hipLaunchKernelGGL(loud_hop_energy_kernel, dim3(kk_cdiv(nhops, LTHREADS / 64)), dim3(LTHREADS), 0, (hipStream_t)stream, wave, woff,
                       hoff, B, nhops, hopsq);
    KK_LAUNCH_CHECK("kk_loud_hop_energy");
    return 0;
}

extern "C" int kk_loud_edges(const double *hopsq, const int64_t *woff, const int *hoff, int B, double top_db, int margin, int *se,
                             void *stream) {
    KK_REQUIRE(hopsq && woff && hoff && se && B > 0, "kk_loud_edges: bad args");
    KK_REQUIRE(top_db > 0.0 && top_db < INFINITY && margin >= 0, "kk_loud_edges: top_db %g must be finite and > 0, margin %d >= 0",
               top_db, margin);
    kk_note_kernel("loud_edges");
    hipLaunchKernelGGL(loud_edges_kernel, dim3(B), dim3(LTHREADS), 0, (hipStream_t)stream, hopsq, woff, hoff, top_db, margin, se);
    KK_LAUNCH_CHECK("kk_loud_edges");
    return 0;
}

extern "C" int kk_loud_kweight(const float *wave, const int64_t *woff, const int *se, const int *soff, int B, int nsteps, int S, int N,
                               const double *coef, double *stepsq, double *stepex, float *steppk, void *stream) {
    KK_REQUIRE(wave && woff && se && soff && coef && stepsq && stepex && steppk && B > 0 && nsteps > 0, "kk_loud_kweight: bad args");
    KK_REQUIRE(S >= 800 && S <= 4800 && N - 4 * S >= -2 && N - 4 * S <= 2,
               "kk_loud_kweight: step %d, block %d: expected round(0.1 fs) and round(0.4 fs) of fs in [8000, 48000]", S, N);
    kk_note_kernel("loud_kweight");
    hipLaunchKernelGGL(loud_kweight_kernel, dim3(kk_cdiv(nsteps, 64)), dim3(64), 0, (hipStream_t)stream, wave, woff, se, soff, B, nsteps,
                       S, N - 4 * S, coef, stepsq, stepex, steppk);
    KK_LAUNCH_CHECK("kk_loud_kweight");
    return 0;
}

extern "C" int kk_loud_gate(const double *stepsq, const double *stepex, const float *steppk, const int *se, const int *soff, int B, int S,
                            int N, double target, double ceiling, double *stats, void *stream) {
    KK_REQUIRE(stepsq && stepex && steppk && se && soff && stats && B > 0, "kk_loud_gate: bad args");
    KK_REQUIRE(S >= 800 && S <= 4800 && N - 4 * S >= -2 && N - 4 * S <= 2, "kk_loud_gate: step %d, block %d", S, N);
    KK_REQUIRE(target > -INFINITY && target < INFINITY && ceiling > 0.0 && ceiling <= 1.0,
               "kk_loud_gate: target %g must be finite, the peak ceiling %g in (0, 1]", target, ceiling);
    kk_note_kernel("loud_gate");
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, stepsq, stepex, steppk, se, soff, S, N, target,
                       ceiling, stats);
    KK_LAUNCH_CHECK("kk_loud_gate");
    return 0;
}

extern "C" int kk_loud_apply(const float *wave, const int64_t *woff, const int *se, const double *stats, int B, int64_t total,
                             float *out, void *stream) {
    KK_REQUIRE(wave && woff && se && stats && out && out != wave && B > 0 && total > 0 && total < ((int64_t)1 << 31),
               "kk_loud_apply: bad args (out != wave: a trimmed utterance moves to the front of its slot)");
    kk_note_kernel("loud_apply");
    hipLaunchKernelGGL(loud_apply_kernel, dim3(kk_cdiv(total, LTHREADS * LAPPLY)), dim3(LTHREADS), 0, (hipStream_t)stream, wave, woff,
                       se, stats, B, total, out);
    KK_LAUNCH_CHECK("kk_loud_apply");
    return 0;
}
