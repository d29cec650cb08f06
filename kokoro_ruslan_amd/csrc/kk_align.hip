// Flat-start forced alignment of phoneme tokens to mel frames (kokoro_ruslan_amd/align.py): the phoneme durations the length regulator
// and the duration loss train on, from one diagonal Gaussian per phoneme id and a few passes of Viterbi training.
//
// A ragged batch of B utterances packed as kk_dtw.hip packs pairs: frames back to back with foff (int32, B + 1), tokens back to back
// with poff (int32, B + 1).  Five launches:
//   feats       from kk_mcep's cepstra [K][T_total] and the packed log-mel: rows 0..K-1 c_1..c_K, row K c_0 (the frame's mean over
//               the mel channels), each minus the utterance's own mean over time, then rows K+1..2K+1 their first differences
//               (x(t+1) - x(t-1)) / 2 with the edge frames replicated.  One workgroup per (utterance, row); the mean is a fixed-order
//               sum (thread i takes the frames i, i + 256, ..., then a fixed tree), in fp64 from the fp32 values.
//   loglik      a class is a mixture of M = 1, 2 or 4 Gaussians, Gaussian c M + m component m of class c.  A component's value is
//               l_m = sum over ascending d of a[g][d] (x[d][t] - mu[g][d])^2 (one fmaf chain: mix_component()), plus k[g]: a = -1/2
//               / var, mu and k = ln w - 1/2 sum_d ln(2 pi var) come from the HOST (fp64, rounded once).  L[c][t] = mx + logf(sum
//               over ascending m of expf(l_m - mx)), mx = max_m l_m; M = 1 writes l_0 (no weight: k is the constant alone).  A
//               workgroup takes 256 frames and LL_GC Gaussians (LL_GC / M whole classes), whose parameters it stages in LDS (read
//               wave-uniformly); a thread holds its frame's features and its class's component values in registers.
//   viterbi     a phoneme is a left-to-right chain of NS states (1..3; align_torch.viterbi_states), class v NS + j for state j of
//               phoneme v.  One workgroup per utterance, thread p = token p, which keeps its NS scores in registers:
//               S(p, j, t) = L[ids[p] NS + j][t] + max(S(p, j, t-1), S(p, j-1, t-1)) for j > 0, and for j = 0 the maximum of
//               S(p, 0, t-1), S(p-1, NS-1, t-1) and, if token p-1 is optional, S(p-2, NS-1, t-1); a later candidate only when
//               strictly greater.  The states are updated in descending j, so S(p, j-1, t-1) is read before it is overwritten.  A
//               neighbour reads only the LAST state's score, and only of column t-1: two columns of it in LDS, two cells of -inf in
//               front of each so that p-1 and p-2 need no branch, one barrier per frame.  A thread loads its rows of L eight frames
//               ahead.  The candidate chosen (0 stay, 1 advance, 2 skip) goes out as 2 bits, 16 tokens per 32-bit word, straight
//               from the wave ballots: bits 0..15 of a word are the low bits of the 16 codes, bits 16..31 their high bits (zero
//               for j > 0); one row of W = ceil(P / 16) words per (frame, state): [T][NS][W].
//   backtrack   one wave per utterance: lane 0 walks (p, j) from (end, NS - 1) back to frame 0 along the code words; code 1 at j > 0
//               steps to the state before, code 1 at j = 0 to the last state of the token before, code 2 to the last state of the
//               token two before.  It counts the state durations in LDS and writes every frame's class ids[p] NS + j; the wave
//               writes the state durations and their row sums, the durations, out.  An infeasible utterance (no finite path) gets
//               durations 0 and labels -1.
//   accumulate  per class the count and, in fp64, sum x and sum x^2 over the frames labelled with it: one workgroup per (class, four
//               dimensions), thread i sums the frames i, i + 256, ... in order (acc_frame), then a fixed tree (acc_finish).  No
//               atomics: two runs give the same bits.
// Nothing an utterance computes in feats, viterbi or backtrack depends on the other utterances, and a frame's L on that frame alone.
// kk_align_scores (two more launches, described where they stand) turns L and an alignment into pronunciation scores.
// feats, loglik, accumulate and scores know nothing of states: they take V NS classes.
#include "kk_common.h"

namespace {

constexpr int AL_MAXP = 1024;                 // tokens of an utterance = threads of its workgroup
constexpr int AL_MAXT = 4096;                 // frames of an utterance (the positional table's order, as kk_dtw)
constexpr int AL_MAXS = 3;                    // states per phoneme
constexpr int AL_PRE = 8;                     // frames of L a state loads ahead
constexpr int AL_THREADS = 256;
constexpr int LL_GC = 16;                     // Gaussians per workgroup of loglik_kernel: 16 / M classes
constexpr int ACC_DG = 4;                     // dimensions per workgroup of accumulate_kernel and mix_sums_kernel
constexpr int MIX_MAXG = 1024;                // Gaussians of a model

// The fixed tree over a workgroup's N rows of fp64 partial sums, and over cnt beside them if given: the totals end in column 0.
template <int N>
__device__ __forceinline__ void al_tree(double (*red)[AL_THREADS], int *cnt) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int h = AL_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            double s[N];                                              // every row is read before any is written: paired LDS accesses
#pragma unroll
            for (int u = 0; u < N; ++u) s[u] = red[u][tid] + red[u][tid + h];
#pragma unroll
            for (int u = 0; u < N; ++u) red[u][tid] = s[u];
            if (cnt) cnt[tid] += cnt[tid + h];
        }
        __syncthreads();
    }
}

// The inclusive scan of one value per thread over a 256-thread workgroup (wave shuffles, then the waves' totals in LDS).
__device__ __forceinline__ int al_block_scan(int v, int *wave_sum, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) {
        const int up = __shfl_up(v, h);
        if (lane >= h) v += up;
    }
    __syncthreads();                                                  // (wave_sum of the call before has been read)
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < AL_THREADS / 64; ++w) {
        if (w < wave) v += wave_sum[w];
        total += wave_sum[w];
    }
    return v;
}

__global__ __launch_bounds__(AL_THREADS) void align_feats_kernel(const float *__restrict__ cep, const float *__restrict__ mel,
                                                                 int64_t T_total, int M, int K, const int *__restrict__ foff,
                                                                 float *__restrict__ feat) {
    __shared__ float row[AL_MAXT];
    __shared__ double red[1][AL_THREADS];
    const int b = blockIdx.x / (K + 1), r = blockIdx.x % (K + 1), tid = threadIdx.x;
    const int f0 = foff[b], T = foff[b + 1] - f0;
    if (T < 1 || T > AL_MAXT) return;                                 // (the host checks; nothing is written past the LDS row)
    double part = 0.0;
    for (int t = tid; t < T; t += AL_THREADS) {
        float v;
        if (r < K) v = cep[(int64_t)r * T_total + f0 + t];
        else {
            const float *x = mel + (int64_t)(f0 + t) * M;
            float acc = 0.f;
            for (int m = 0; m < M; ++m) acc += x[m];
            v = acc / (float)M;
        }
        row[t] = v;
        part += (double)v;
    }
    red[0][tid] = part;
    al_tree<1>(red, nullptr);
    const float mean = (float)(red[0][0] / (double)T);
    float *stat = feat + (int64_t)r * T_total + f0, *delta = feat + (int64_t)(K + 1 + r) * T_total + f0;
    for (int t = tid; t < T; t += AL_THREADS) {
        stat[t] = row[t] - mean;
        delta[t] = 0.5f * ((row[min(t + 1, T - 1)] - mean) - (row[max(t - 1, 0)] - mean));
    }
}

// One component's value at a frame: as, ms point at its D parameters (LDS or global), x holds the frame's features.
template <int DM>
__device__ __forceinline__ float mix_component(const float (&x)[DM], const float *as, const float *ms, float k, int D) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d)
        if (d < D) {
            const float diff = x[d] - ms[d];
            acc = fmaf(diff * diff, as[d], acc);
        }
    return acc + k;
}

template <int DM, int M>
__global__ __launch_bounds__(AL_THREADS) void align_loglik_kernel(const float *__restrict__ feat, int64_t T_total, int D, int C,
                                                                  const float *__restrict__ a, const float *__restrict__ mu,
                                                                  const float *__restrict__ k, float *__restrict__ L) {
    constexpr int CC = LL_GC / M;                                     // classes per workgroup
    __shared__ float as[LL_GC * DM], ms[LL_GC * DM], ks[LL_GC];
    const int tid = threadIdx.x, c0 = blockIdx.y * CC, nc = min(CC, C - c0), ng = nc * M, g0 = c0 * M;
    for (int e = tid; e < ng * D; e += AL_THREADS) {
        const int gg = e / D, d = e % D;
        as[gg * DM + d] = a[(int64_t)(g0 + gg) * D + d];
        ms[gg * DM + d] = mu[(int64_t)(g0 + gg) * D + d];
    }
    if (tid < ng) ks[tid] = k[g0 + tid];
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * AL_THREADS + tid;
    if (t >= T_total) return;
    float x[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) x[d] = feat[(int64_t)min(d, D - 1) * T_total + t];
    for (int cc = 0; cc < nc; ++cc) {
        if (M == 1) {
            // mix_component() written out with the class's index in the LDS subscripts: the same chain and the same bits, but through
            // the call the compiler unrolls this loop less (gfx950: 3022 against 4079 instructions at DM = 64) and the M = 1 launch was
            // 0.045 ms where this form takes 0.040 (59 classes x 38 400 frames, D = 28; docs/LAB_NOTES.md).
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < DM; ++d)
                if (d < D) {
                    const float diff = x[d] - ms[cc * DM + d];
                    acc = fmaf(diff * diff, as[cc * DM + d], acc);
                }
            L[(int64_t)(c0 + cc) * T_total + t] = acc + ks[cc];
            continue;
        }
        float l[M];
#pragma unroll
        for (int m = 0; m < M; ++m) l[m] = mix_component<DM>(x, as + (cc * M + m) * DM, ms + (cc * M + m) * DM, ks[cc * M + m], D);
        float out = l[0];
        if (M > 1) {
            float mx = l[0];
#pragma unroll
            for (int m = 1; m < M; ++m) mx = fmaxf(mx, l[m]);
            if (mx > -__builtin_inff()) {                             // (a class with no finite component stays -inf)
                float s = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) s += expf(l[m] - mx);
                out = mx + logf(s);
            } else out = mx;
        }
        L[(int64_t)(c0 + cc) * T_total + t] = out;
    }
}

struct VitArgs {
    const float *L;                           // [V NS][T_total]
    int64_t T_total;
    const int *ids;                           // [P_total]
    const unsigned char *opt;                 // [P_total]: 1 where the token may be skipped
    const int *foff, *poff;
    const int64_t *coff;                      // first code word of each utterance
    float *score;
    int *end;                                 // the end token, -1 when infeasible
    uint32_t *codes;
};

template <int NS>
__global__ __launch_bounds__(AL_MAXP) void align_viterbi_kernel(const VitArgs a) {
    __shared__ float S[2][AL_MAXP + 2];                               // the last state of token p at [p + 2]; [0] and [1] stay -inf
    const int b = blockIdx.x, p = threadIdx.x;
    const int f0 = a.foff[b], T = a.foff[b + 1] - f0, p0 = a.poff[b], P = a.poff[b + 1] - p0;
    if (P < 1 || P > (int)blockDim.x || T < 1 || T > AL_MAXT) return;  // (the host checks)
    const bool live = p < P, wave_live = (p & ~63) < P;
    const int W = (P + 15) >> 4;                                      // code words per (frame, state)
    uint32_t *codes = a.codes + a.coff[b];
    const float ninf = -__builtin_inff();
    const float *Lr = a.L + (int64_t)(live ? a.ids[p0 + p] : 0) * NS * a.T_total + f0;      // state j: Lr + j T_total
    const bool may_skip = live && p >= 2 && a.opt[p0 + p - 1];
    const bool starts = p == 0 || (p == 1 && a.opt[p0]);
    float sc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) sc[j] = ninf;
    if (p < 2) S[0][p] = S[1][p] = ninf;
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += AL_PRE) {
        float l[NS][AL_PRE];
        if (wave_live) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
#pragma unroll
                for (int u = 0; u < AL_PRE; ++u) l[j][u] = Lr[(int64_t)j * a.T_total + min(t0 + u, T - 1)];
        }
#pragma unroll
        for (int u = 0; u < AL_PRE; ++u) {
            const int t = t0 + u;
            if (t >= T) break;
            if (wave_live) {
                const float *prev = S[(t & 1) ^ 1];
                uint32_t code[NS];
#pragma unroll
                for (int j = 0; j < NS; ++j) code[j] = 0;
                if (t == 0) sc[0] = starts ? l[0][u] : ninf;          // (the other states stay -inf)
                else {
#pragma unroll
                    for (int j = NS - 1; j > 0; --j) {                // descending: sc[j - 1] still holds frame t - 1
                        float best = sc[j];
                        if (sc[j - 1] > best) best = sc[j - 1], code[j] = 1;
                        sc[j] = l[j][u] + best;
                    }
                    float best = sc[0];
                    const float adv = prev[p + 1], skip = may_skip ? prev[p] : ninf;
                    if (adv > best) best = adv, code[0] = 1;
                    if (skip > best) best = skip, code[0] = 2;
                    sc[0] = l[0][u] + best;
                }
                if (live) S[t & 1][p + 2] = sc[NS - 1];
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    if (!live) code[j] = 0;
                    const unsigned long long lo = __ballot(code[j] & 1u), hi = j == 0 ? __ballot(code[j] & 2u) : 0ull;
                    if (live && (p & 15) == 0) {
                        const int sh = p & 48;
                        codes[((int64_t)t * NS + j) * W + (p >> 4)] =
                            (uint32_t)((lo >> sh) & 0xffffull) | ((uint32_t)((hi >> sh) & 0xffffull) << 16);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (p == 0) {
        const float *last = S[(T - 1) & 1];
        int e = P - 1;
        float s = last[P + 1];
        if (P > 1 && a.opt[p0 + P - 1] && last[P] > s) e = P - 2, s = last[P];
        const bool ok = s > ninf;                                     // (false for a NaN too)
        a.score[b] = ok ? s : ninf;
        a.end[b] = ok ? e : -1;
    }
}

template <int NS>
__global__ __launch_bounds__(64) void align_backtrack_kernel(const uint32_t *__restrict__ codes, const int64_t *__restrict__ coff,
                                                             const int *__restrict__ foff, const int *__restrict__ poff,
                                                             const int *__restrict__ ids, const int *__restrict__ end,
                                                             int *__restrict__ state_durations,      // NULL: not wanted (NS = 1)
                                                             int *__restrict__ durations, int *__restrict__ label) {
    __shared__ int dur[AL_MAXP * NS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int f0 = foff[b], T = foff[b + 1] - f0, p0 = poff[b], P = poff[b + 1] - p0;
    if (P < 1 || P > AL_MAXP || T < 1 || T > AL_MAXT) return;
    for (int q = lane; q < P * NS; q += 64) dur[q] = 0;
    __syncthreads();
    const int e = end[b];
    if (e < 0 || e >= P) {
        for (int t = lane; t < T; t += 64) label[f0 + t] = -1;
    } else if (lane == 0) {
        const uint32_t *cod = codes + coff[b];
        const int W = (P + 15) >> 4;
        int p = e, j = NS - 1;
        for (int t = T - 1; t >= 0; --t) {
            ++dur[p * NS + j];
            label[f0 + t] = ids[p0 + p] * NS + j;
            if (t) {
                const uint32_t w = cod[((int64_t)t * NS + j) * W + (p >> 4)] >> (p & 15);
                const int c = (int)min((w & 1u) | ((w >> 15) & 2u), 2u);
                if (NS > 1 && c == 1 && j > 0) --j;
                else {                                                // (NS = 1: p - c alone, nothing to choose in the walk's chain)
                    p = max(p - c, 0);
                    if (NS > 1 && c) j = NS - 1;
                }
            }
        }
    }
    __syncthreads();
    if (state_durations)
        for (int q = lane; q < P * NS; q += 64) state_durations[(int64_t)p0 * NS + q] = dur[q];
    for (int q = lane; q < P; q += 64) {
        int d = 0;
#pragma unroll
        for (int j = 0; j < NS; ++j) d += dur[q * NS + j];
        durations[p0 + q] = d;
    }
}

// The one place that turns the run-time `states` into NS: launches align_viterbi_kernel<NS> or align_backtrack_kernel<NS>.
#define AL_LAUNCH_NS(kernel, states, ...)                                   \
    do {                                                                    \
        if ((states) == 1) hipLaunchKernelGGL(kernel<1>, __VA_ARGS__);      \
        else if ((states) == 2) hipLaunchKernelGGL(kernel<2>, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<3>, __VA_ARGS__);                    \
    } while (0)
static_assert(AL_MAXS == 3, "AL_LAUNCH_NS instantiates 1..3");

// The statistics of one Gaussian over the workgroup's ACC_DG dimensions from d0, shared by the dense path (accumulate_kernel: every
// frame whose label is the Gaussian) and the list path (mix_sums_kernel: the Gaussian's own list of frames).  acc_frame adds frame t
// to a thread's sums; acc_finish stages the threads' sums, reduces them (and cnt beside them if given) in the fixed tree and stores
// the Gaussian's row.  The two paths add a Gaussian's frames in different orders, so their sums may differ in the last bits.
__device__ __forceinline__ void acc_frame(const float *__restrict__ feat, int64_t T_total, int D, int d0, int64_t t,
                                          double (&s1)[ACC_DG], double (&s2)[ACC_DG]) {
#pragma unroll
    for (int u = 0; u < ACC_DG; ++u)
        if (d0 + u < D) {
            const double x = (double)feat[(int64_t)(d0 + u) * T_total + t];
            s1[u] += x;
            s2[u] += x * x;
        }
}

__device__ __forceinline__ void acc_finish(double (*red)[AL_THREADS], int *cnt, const double (&s1)[ACC_DG], const double (&s2)[ACC_DG],
                                           int g, int D, int d0, double *__restrict__ sum, double *__restrict__ sumsq) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < ACC_DG; ++u) red[u][tid] = s1[u], red[ACC_DG + u][tid] = s2[u];
    al_tree<2 * ACC_DG>(red, cnt);
    if (tid < ACC_DG && d0 + tid < D) {
        sum[(int64_t)g * D + d0 + tid] = red[tid][0];
        sumsq[(int64_t)g * D + d0 + tid] = red[ACC_DG + tid][0];
    }
}

__global__ __launch_bounds__(AL_THREADS) void align_accumulate_kernel(const float *__restrict__ feat, const int *__restrict__ label,
                                                                      int64_t T_total, int D, long long *__restrict__ count,
                                                                      double *__restrict__ sum, double *__restrict__ sumsq) {
    __shared__ double red[2 * ACC_DG][AL_THREADS];
    __shared__ int cnt[AL_THREADS];
    const int v = blockIdx.x, d0 = blockIdx.y * ACC_DG, tid = threadIdx.x;
    double s1[ACC_DG] = {}, s2[ACC_DG] = {};
    int n = 0;
    for (int64_t t = tid; t < T_total; t += AL_THREADS)
        if (label[t] == v) {
            ++n;
            acc_frame(feat, T_total, D, d0, t, s1, s2);
        }
    cnt[tid] = n;
    acc_finish(red, cnt, s1, s2, v, D, d0, sum, sumsq);
    if (tid == 0 && blockIdx.y == 0) count[v] = cnt[0];
}

// ---- Gaussian mixtures: training's two launches for M = 2 or 4 components per class (align_torch.mix_labels, accumulate) ------------
// G = C M Gaussians; a, mu [G][D] and k [G] as loglik takes them.
//   mix_labels      thread = frame: the M components of the frame's own class through loglik's mix_component(), read from global
//                   memory (a wave's frames are runs of few classes: the lines stay in L1/L2); the largest wins, the lowest m on a tie.
//   accumulate_mix  a stable counting sort of the frame indices by label, then one workgroup per (Gaussian, four dimensions) over
//                   its own list: hist counts the labels of every 256 frames per Gaussian (integer adds in LDS), scan turns every
//                   Gaussian's row of block counts into an exclusive prefix and its total, starts scans the totals, scatter gives
//                   frame t the slot start[g] + prefix[g][block] + (frames of the block before t with the same label): ascending t
//                   inside every list, whatever ran first.  sums is accumulate_kernel on a list: thread i takes the entries i, i +
//                   256, ... in order, then the fixed tree.  No floating-point atomics: two runs give the same bits.
template <int DM, int M>
__global__ __launch_bounds__(AL_THREADS) void align_mix_labels_kernel(const float *__restrict__ feat, int64_t T_total, int D, int C,
                                                                      const float *__restrict__ a, const float *__restrict__ mu,
                                                                      const float *__restrict__ k, const int *__restrict__ label,
                                                                      int *__restrict__ mixlabel) {
    const int64_t t = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (t >= T_total) return;
    const int c = label[t];
    if (c < 0 || c >= C) {
        mixlabel[t] = -1;
        return;
    }
    float x[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) x[d] = feat[(int64_t)min(d, D - 1) * T_total + t];
    int best = 0;
    float top = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int g = c * M + m;
        const float l = mix_component<DM>(x, a + (int64_t)g * D, mu + (int64_t)g * D, k[g], D);
        if (m == 0 || l > top) top = l, best = m;                     // ascending m, strictly greater: the lowest component wins a tie
    }
    mixlabel[t] = c * M + best;
}

// The workspace of accumulate_mix, in 32-bit words: prefix [G][NB] (hist's counts, then scan's exclusive prefixes), start [G], order
// [T_total]; NB = ceil(T_total / 256).
__global__ __launch_bounds__(AL_THREADS) void align_mix_hist_kernel(const int *__restrict__ label, int64_t T_total, int G, int NB,
                                                                    int *__restrict__ prefix) {
    __shared__ int h[MIX_MAXG];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int g = tid; g < G; g += AL_THREADS) h[g] = 0;
    __syncthreads();
    const int64_t t = (int64_t)b * AL_THREADS + tid;
    const int lab = t < T_total ? label[t] : -1;
    if (lab >= 0 && lab < G) atomicAdd(&h[lab], 1);                   // (integers: the count does not depend on the order)
    __syncthreads();
    for (int g = tid; g < G; g += AL_THREADS) prefix[(int64_t)g * NB + b] = h[g];
}

__global__ __launch_bounds__(AL_THREADS) void align_mix_scan_kernel(int *__restrict__ prefix, int NB, long long *__restrict__ count) {
    __shared__ int wave_sum[AL_THREADS / 64];
    int *row = prefix + (int64_t)blockIdx.x * NB;
    int carry = 0;
    for (int b0 = 0; b0 < NB; b0 += AL_THREADS) {
        const int b = b0 + threadIdx.x, v = b < NB ? row[b] : 0;
        int total;
        const int incl = al_block_scan(v, wave_sum, total);
        if (b < NB) row[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

__global__ __launch_bounds__(AL_THREADS) void align_mix_starts_kernel(const long long *__restrict__ count, int G, int *__restrict__ start) {
    __shared__ int wave_sum[AL_THREADS / 64];
    int carry = 0;
    for (int g0 = 0; g0 < G; g0 += AL_THREADS) {
        const int g = g0 + threadIdx.x, v = g < G ? (int)count[g] : 0;
        int total;
        const int incl = al_block_scan(v, wave_sum, total);
        if (g < G) start[g] = carry + incl - v;
        carry += total;
    }
}

__global__ __launch_bounds__(AL_THREADS) void align_mix_scatter_kernel(const int *__restrict__ label, int64_t T_total, int G, int NB,
                                                                       const int *__restrict__ prefix, const int *__restrict__ start,
                                                                       int *__restrict__ order) {
    __shared__ int lab[AL_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t t = (int64_t)b * AL_THREADS + tid;
    const int mine = t < T_total ? label[t] : -1;
    lab[tid] = mine;
    __syncthreads();
    if (mine < 0 || mine >= G) return;
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += lab[j] == mine;             // the frames of this block before t with its label
    order[start[mine] + prefix[(int64_t)mine * NB + b] + rank] = (int)t;           // (< count's total <= T_total: inside order)
}

__global__ __launch_bounds__(AL_THREADS) void align_mix_sums_kernel(const float *__restrict__ feat, int64_t T_total, int D,
                                                                    const long long *__restrict__ count, const int *__restrict__ start,
                                                                    const int *__restrict__ order, double *__restrict__ sum,
                                                                    double *__restrict__ sumsq) {
    __shared__ double red[2 * ACC_DG][AL_THREADS];
    const int g = blockIdx.x, d0 = blockIdx.y * ACC_DG, tid = threadIdx.x;
    const int n = (int)count[g];
    const int *list = order + start[g];
    double s1[ACC_DG] = {}, s2[ACC_DG] = {};
    for (int i = tid; i < n; i += AL_THREADS) acc_frame(feat, T_total, D, d0, list[i], s1, s2);
    acc_finish(red, nullptr, s1, s2, g, D, d0, sum, sumsq);
}

// ---- pronunciation scores of an alignment (align_torch.scores) ------------------------------------------------------------------------
// Two launches, nothing read by the host in between.
//   score_frames  thread = frame, so a wave reads 64 consecutive floats of every row of L [V][T_total]; L is read once.  SC_VC rows
//                 are loaded at a time (SC_VC loads in flight per lane).  The frame's maximum and the lowest class that attains it
//                 are exact; sum_v exp(L(v) - fmax) is an fp64 running sum that is rescaled by exp(old max - new max) at most once
//                 per SC_VC rows.  The value of the frame's own class (label[t]) is picked up as its row goes by.  Per frame:
//                 margin = L(label) - fmax and lpost = margin - log(sum), both fp64, and amax.  A frame without a class (label
//                 outside 0..V-1: the -1 of an infeasible utterance) gets 0 and 0.
//   score_tokens  one workgroup per utterance.  A thread owns SC_TPT consecutive tokens; an exclusive scan of the durations
//                 (al_block_scan) gives every token its first frame.  A token's sums run over its frames in
//                 ascending order from 0.0, its hits count amax == ids[p]; the utterance's totals run over the tokens' values (kept
//                 in LDS) in ascending token order, one lane per total.  An utterance outside the limits, or whose durations are not
//                 all in 0..T with the sum T (the zeros of an infeasible one), gets zeros everywhere: every output is written.
constexpr int SC_VC = 16;                     // rows of L a frame loads at a time
constexpr int SC_TPT = AL_MAXP / AL_THREADS;  // tokens a thread of score_tokens owns

__global__ __launch_bounds__(AL_THREADS) void align_score_frames_kernel(const float *__restrict__ L, int64_t T_total, int V,
                                                                        const int *__restrict__ label, double *__restrict__ margin,
                                                                        double *__restrict__ lpost, int *__restrict__ amax) {
    const int64_t t = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (t >= T_total) return;
    const int lab = label[t];
    const float ninf = -__builtin_inff();
    float m = ninf, own = 0.f;
    int am = 0;
    double s = 0.0;
    for (int v0 = 0; v0 < V; v0 += SC_VC) {
        float x[SC_VC];
#pragma unroll
        for (int u = 0; u < SC_VC; ++u) x[u] = v0 + u < V ? L[(int64_t)(v0 + u) * T_total + t] : ninf;
        const float before = m;
#pragma unroll
        for (int u = 0; u < SC_VC; ++u) {
            if (x[u] > m) m = x[u], am = v0 + u;                      // ascending v, strictly greater: the lowest class wins a tie
            if (v0 + u == lab) own = x[u];
        }
        if (v0 > 0 && m > before) s *= exp((double)before - (double)m);
#pragma unroll
        for (int u = 0; u < SC_VC; ++u)
            if (v0 + u < V) s += exp((double)x[u] - (double)m);
    }
    const bool has = lab >= 0 && lab < V;
    const double mg = has ? (double)own - (double)m : 0.0;
    margin[t] = mg;
    lpost[t] = has ? mg - log(s) : 0.0;
    amax[t] = am;
}

__global__ __launch_bounds__(AL_THREADS) void align_score_tokens_kernel(const double *__restrict__ margin,
                                                                        const double *__restrict__ lpost,
                                                                        const int *__restrict__ amax,
                                                                        const int *__restrict__ durations,
                                                                        const int *__restrict__ ids, const int *__restrict__ foff,
                                                                        const int *__restrict__ poff, double *__restrict__ gop_sum,
                                                                        double *__restrict__ lpost_sum, int *__restrict__ hits,
                                                                        double *__restrict__ utt_gop, double *__restrict__ utt_lpost,
                                                                        int *__restrict__ utt_hits) {
    __shared__ double tok[2][AL_MAXP];                                // the tokens' gop_sum and lpost_sum, for the totals
    __shared__ int wave_sum[AL_THREADS / 64], bad, hit_total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int f0 = foff[b], T = foff[b + 1] - f0, p0 = poff[b], P = poff[b + 1] - p0;
    if (P < 1 || P > AL_MAXP || T < 1 || T > AL_MAXT) {               // (the host checks) zeros, whatever its durations hold
        for (int q = tid; q < P; q += AL_THREADS) gop_sum[p0 + q] = 0.0, lpost_sum[p0 + q] = 0.0, hits[p0 + q] = 0;
        if (tid == 0) utt_gop[b] = 0.0, utt_lpost[b] = 0.0, utt_hits[b] = 0;
        return;
    }
    if (tid == 0) bad = 0, hit_total = 0;
    __syncthreads();
    int d[SC_TPT], mine = 0;
    bool wrong = false;
#pragma unroll
    for (int u = 0; u < SC_TPT; ++u) {
        const int q = tid * SC_TPT + u;
        d[u] = q < P ? durations[p0 + q] : 0;
        if (d[u] < 0 || d[u] > T) wrong = true, d[u] = 0;
        mine += d[u];                                                 // (at most AL_MAXP * AL_MAXT: no overflow)
    }
    if (wrong) bad = 1;
    int total, first = al_block_scan(mine, wave_sum, total) - mine;   // (its barriers also publish bad)
    const bool valid = !bad && total == T;                            // (so no span leaves the utterance's frames)
    int nh = 0;
#pragma unroll
    for (int u = 0; u < SC_TPT; ++u) {
        const int q = tid * SC_TPT + u;
        if (q >= P) break;
        double g = 0.0, l = 0.0;
        int h = 0;
        if (valid) {
            const int id = ids[p0 + q];
            const int64_t base = (int64_t)f0 + first;
#pragma unroll 4
            for (int k = 0; k < d[u]; ++k) {
                g += margin[base + k];
                l += lpost[base + k];
                h += amax[base + k] == id;
            }
            first += d[u];
        }
        gop_sum[p0 + q] = g, lpost_sum[p0 + q] = l, hits[p0 + q] = h;
        tok[0][q] = g, tok[1][q] = l;
        nh += h;
    }
    if (nh) atomicAdd(&hit_total, nh);
    __syncthreads();
    if (tid < 2) {                                                    // lane 0 the gop total, lane 1 the lpost total: the same loop
        const double *x = tok[tid];
        double acc = 0.0;
#pragma unroll 8
        for (int q = 0; q < P; ++q) acc += x[q];
        (tid == 0 ? utt_gop : utt_lpost)[b] = acc;
    }
    if (tid == 2) utt_hits[b] = hit_total;
}

}  // namespace

extern "C" int kk_align_max_tokens(void) { return AL_MAXP; }

extern "C" int kk_align_feats(const float *cep, const float *mel, int64_t T_total, int M, int K, const int *foff, int B, float *feat,
                              void *stream) {
    KK_REQUIRE(mel && foff && feat && B > 0 && T_total > 0 && T_total < ((int64_t)1 << 31), "kk_align_feats: bad args");
    KK_REQUIRE(M >= 1 && K >= 0 && K <= 31 && (cep || K == 0), "kk_align_feats: M = %d, K = %d; needs M >= 1 and 0 <= K <= 31", M, K);
    kk_note_kernel("align_feats");
    hipLaunchKernelGGL(align_feats_kernel, dim3((unsigned)B * (K + 1)), dim3(AL_THREADS), 0, (hipStream_t)stream, cep, mel, T_total, M, K,
                       foff, feat);
    KK_LAUNCH_CHECK("kk_align_feats");
    return 0;
}

extern "C" int kk_align_max_states(void) { return AL_MAXS; }

extern "C" int kk_align_viterbi(const float *L, int64_t T_total, const int *ids, const unsigned char *opt, const int *foff,
                                const int *poff, const int64_t *coff, int B, int threads, int states, float *score, int *end,
                                uint32_t *codes, void *stream) {
    KK_REQUIRE(L && ids && opt && foff && poff && coff && score && end && codes && B > 0 && T_total > 0, "kk_align_viterbi: bad args");
    KK_REQUIRE(threads >= 64 && threads <= AL_MAXP && threads % 64 == 0, "kk_align_viterbi: %d threads; needs a multiple of 64 in 64..%d",
               threads, AL_MAXP);
    KK_REQUIRE(states >= 1 && states <= AL_MAXS, "kk_align_viterbi: %d states; needs 1..%d", states, AL_MAXS);
    VitArgs r{L, T_total, ids, opt, foff, poff, coff, score, end, codes};
    kk_note_kernel("align_viterbi");
    AL_LAUNCH_NS(align_viterbi_kernel, states, dim3(B), dim3(threads), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_align_viterbi");
    return 0;
}

extern "C" int kk_align_backtrack(const uint32_t *codes, const int64_t *coff, const int *foff, const int *poff, const int *ids,
                                  const int *end, int B, int states, int *state_durations, int *durations, int *label, void *stream) {
    KK_REQUIRE(codes && coff && foff && poff && ids && end && durations && label && B > 0, "kk_align_backtrack: bad args");
    KK_REQUIRE(states >= 1 && states <= AL_MAXS, "kk_align_backtrack: %d states; needs 1..%d", states, AL_MAXS);
    KK_REQUIRE(state_durations || states == 1, "kk_align_backtrack: %d states need state_durations", states);
    kk_note_kernel("align_backtrack");
    AL_LAUNCH_NS(align_backtrack_kernel, states, dim3(B), dim3(64), 0, (hipStream_t)stream, codes, coff, foff, poff, ids, end,
                 state_durations, durations, label);
    KK_LAUNCH_CHECK("kk_align_backtrack");
    return 0;
}

extern "C" int kk_align_accumulate(const float *feat, const int *label, int64_t T_total, int D, int V, int64_t *count, double *sum,
                                   double *sumsq, void *stream) {
    KK_REQUIRE(feat && label && count && sum && sumsq && T_total > 0 && T_total < ((int64_t)1 << 31), "kk_align_accumulate: bad args");
    KK_REQUIRE(D >= 1 && D <= 64 && V >= 1 && V <= 256, "kk_align_accumulate: D = %d, V = %d; needs 1 <= D <= 64 and 1 <= V <= 256", D, V);
    kk_note_kernel("align_accumulate");
    hipLaunchKernelGGL(align_accumulate_kernel, dim3(V, kk_cdiv(D, ACC_DG)), dim3(AL_THREADS), 0, (hipStream_t)stream, feat, label, T_total,
                       D, (long long *)count, sum, sumsq);
    KK_LAUNCH_CHECK("kk_align_accumulate");
    return 0;
}

extern "C" int kk_align_mix_frames(void) { return AL_THREADS; }

// The one place that turns the run-time D and M into the template parameters of loglik_kernel and mix_labels_kernel.
#define AL_LAUNCH_MIX_D(kernel, D, MM, ...)                                              \
    do {                                                                                 \
        if ((D) <= 8) hipLaunchKernelGGL((kernel<8, MM>), __VA_ARGS__);                  \
        else if ((D) <= 32) hipLaunchKernelGGL((kernel<32, MM>), __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<64, MM>), __VA_ARGS__);                          \
    } while (0)
#define AL_LAUNCH_MIX(kernel, D, M, ...)                                \
    do {                                                                \
        if ((M) == 1) AL_LAUNCH_MIX_D(kernel, D, 1, __VA_ARGS__);       \
        else if ((M) == 2) AL_LAUNCH_MIX_D(kernel, D, 2, __VA_ARGS__);  \
        else AL_LAUNCH_MIX_D(kernel, D, 4, __VA_ARGS__);                \
    } while (0)

static bool mix_shape_ok(int D, int C, int M) {
    return D >= 1 && D <= 64 && (M == 1 || M == 2 || M == 4) && C >= 1 && (int64_t)C * M <= MIX_MAXG;
}

extern "C" int kk_align_loglik(const float *feat, int64_t T_total, int D, int C, int M, const float *a, const float *mu,
                                   const float *k, float *L, void *stream) {
    KK_REQUIRE(feat && a && mu && k && L && T_total > 0 && T_total < ((int64_t)1 << 31), "kk_align_loglik: bad args");
    KK_REQUIRE(mix_shape_ok(D, C, M), "kk_align_loglik: D = %d, C = %d, M = %d; needs 1 <= D <= 64, M in {1, 2, 4} and 1 <= C M <= %d",
               D, C, M, MIX_MAXG);
    const dim3 grid(kk_cdiv(T_total, AL_THREADS), kk_cdiv(C, LL_GC / M));
    kk_note_kernel("align_loglik");
    AL_LAUNCH_MIX(align_loglik_kernel, D, M, grid, dim3(AL_THREADS), 0, (hipStream_t)stream, feat, T_total, D, C, a, mu, k, L);
    KK_LAUNCH_CHECK("kk_align_loglik");
    return 0;
}

extern "C" int kk_align_mix_labels(const float *feat, int64_t T_total, int D, int C, int M, const float *a, const float *mu,
                                   const float *k, const int *label, int *mixlabel, void *stream) {
    KK_REQUIRE(feat && a && mu && k && label && mixlabel && T_total > 0 && T_total < ((int64_t)1 << 31), "kk_align_mix_labels: bad args");
    KK_REQUIRE(mix_shape_ok(D, C, M), "kk_align_mix_labels: D = %d, C = %d, M = %d; needs 1 <= D <= 64, M in {1, 2, 4} and 1 <= C M <= %d",
               D, C, M, MIX_MAXG);
    kk_note_kernel("align_mix_labels");
    AL_LAUNCH_MIX(align_mix_labels_kernel, D, M, dim3(kk_cdiv(T_total, AL_THREADS)), dim3(AL_THREADS), 0, (hipStream_t)stream, feat,
                  T_total, D, C, a, mu, k, label, mixlabel);
    KK_LAUNCH_CHECK("kk_align_mix_labels");
    return 0;
}

extern "C" int64_t kk_align_accumulate_mix_ws_bytes(int64_t T_total, int G) {
    if (T_total < 1 || T_total >= ((int64_t)1 << 31) || G < 1 || G > MIX_MAXG) return 0;
    return ((int64_t)G * kk_cdiv(T_total, AL_THREADS) + G + T_total) * (int64_t)sizeof(int);
}

extern "C" int kk_align_accumulate_mix(const float *feat, const int *mixlabel, int64_t T_total, int D, int G, int64_t *count,
                                       double *sum, double *sumsq, void *ws, int64_t ws_bytes, void *stream) {
    KK_REQUIRE(feat && mixlabel && count && sum && sumsq && ws && T_total > 0 && T_total < ((int64_t)1 << 31),
               "kk_align_accumulate_mix: bad args");
    KK_REQUIRE(D >= 1 && D <= 64 && G >= 1 && G <= MIX_MAXG, "kk_align_accumulate_mix: D = %d, G = %d; needs 1 <= D <= 64 and 1 <= G <= %d",
               D, G, MIX_MAXG);
    const int64_t need = kk_align_accumulate_mix_ws_bytes(T_total, G);
    KK_REQUIRE(ws_bytes >= need, "kk_align_accumulate_mix: a workspace of %lld bytes; needs %lld (kk_align_accumulate_mix_ws_bytes)",
               (long long)ws_bytes, (long long)need);
    const int NB = (int)kk_cdiv(T_total, AL_THREADS);
    int *prefix = (int *)ws, *start = prefix + (int64_t)G * NB, *order = start + G;
    hipStream_t s = (hipStream_t)stream;
    kk_note_kernel("align_accumulate_mix");
    hipLaunchKernelGGL(align_mix_hist_kernel, dim3(NB), dim3(AL_THREADS), 0, s, mixlabel, T_total, G, NB, prefix);
    KK_LAUNCH_CHECK("kk_align_accumulate_mix (hist)");
    hipLaunchKernelGGL(align_mix_scan_kernel, dim3(G), dim3(AL_THREADS), 0, s, prefix, NB, (long long *)count);
    KK_LAUNCH_CHECK("kk_align_accumulate_mix (scan)");
    hipLaunchKernelGGL(align_mix_starts_kernel, dim3(1), dim3(AL_THREADS), 0, s, (const long long *)count, G, start);
    KK_LAUNCH_CHECK("kk_align_accumulate_mix (starts)");
    hipLaunchKernelGGL(align_mix_scatter_kernel, dim3(NB), dim3(AL_THREADS), 0, s, mixlabel, T_total, G, NB, prefix, start, order);
    KK_LAUNCH_CHECK("kk_align_accumulate_mix (scatter)");
    hipLaunchKernelGGL(align_mix_sums_kernel, dim3(G, kk_cdiv(D, ACC_DG)), dim3(AL_THREADS), 0, s, feat, T_total, D,
                       (const long long *)count, start, order, sum, sumsq);
    KK_LAUNCH_CHECK("kk_align_accumulate_mix (sums)");
    return 0;
}

extern "C" int kk_align_scores(const float *L, int64_t T_total, int V, const int *label, const int *durations, const int *ids,
                               const int *foff, const int *poff, int B, double *margin, double *lpost, int *amax, double *gop_sum,
                               double *lpost_sum, int *hits, double *utt_gop, double *utt_lpost, int *utt_hits, void *stream) {
    KK_REQUIRE(L && label && durations && ids && foff && poff && margin && lpost && amax && gop_sum && lpost_sum && hits && utt_gop &&
                   utt_lpost && utt_hits && B > 0 && T_total > 0 && T_total < ((int64_t)1 << 31),
               "kk_align_scores: bad args");
    KK_REQUIRE(V >= 1 && V <= 256, "kk_align_scores: V = %d; needs 1 <= V <= 256", V);
    kk_note_kernel("align_score_frames");
    hipLaunchKernelGGL(align_score_frames_kernel, dim3(kk_cdiv(T_total, AL_THREADS)), dim3(AL_THREADS), 0, (hipStream_t)stream, L, T_total,
                       V, label, margin, lpost, amax);
    KK_LAUNCH_CHECK("kk_align_scores (frames)");
    kk_note_kernel("align_score_tokens");
    hipLaunchKernelGGL(align_score_tokens_kernel, dim3(B), dim3(AL_THREADS), 0, (hipStream_t)stream, margin, lpost, amax, durations, ids,
                       foff, poff, gop_sum, lpost_sum, hits, utt_gop, utt_lpost, utt_hits);
    KK_LAUNCH_CHECK("kk_align_scores (tokens)");
    return 0;
}
