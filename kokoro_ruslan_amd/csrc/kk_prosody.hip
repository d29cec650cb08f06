// Prosody control of the synthesis prefill (kokoro_ruslan_amd/prosody.py; the fp32 restatement: prosody_torch.py).
//
//  durations   frames per phoneme from the predictor's expm1(log_dur), a per-phoneme speed and forced values; the row sums
//  variance    per-frame pitch / energy from the predictors' outputs, per-phoneme scale + shift and forced values
//  contour     the same with a source track per row on top: every frame takes the centre-aligned nearest source frame of its phoneme
//
// All sit between the predictors and the length regulator / the bucket embeddings, twice per prefill and never in the decode loop:
// elementwise work on [B, Pn] and [B, T] plus one row sum, written for exactness against the torch restatement, not for speed.
#include "kk_common.h"

namespace {

// torch.clamp(x, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// One workgroup per row.  base = max(rint(d), 0); a phoneme with base > 0 keeps >= 1 frame at any speed; forced >= 0 wins.  The row sum
// is an integer sum (thread-strided partials, then an LDS tree): the same value in any order.
__global__ __launch_bounds__(256) void prosody_durations_kernel(const float *__restrict__ d, const float *__restrict__ speed,
                                                                const int *__restrict__ forced, const int *__restrict__ plens,
                                                                int64_t *__restrict__ dur_out, int64_t *__restrict__ sums_out, int Pn) {
    __shared__ int64_t red[256];
    const int b = blockIdx.x;
    const int len = plens ? (plens[b] < Pn ? plens[b] : Pn) : Pn;
    int64_t acc = 0;
    for (int p = threadIdx.x; p < Pn; p += 256) {
        const int64_t i = (int64_t)b * Pn + p;
        int64_t dur = 0;
        if (p < len) {
            const float x = d[i];
            const float r = rintf(x);                                    // half to even, as torch.round
            if (r > 0.f) {                                               // (false for NaN: base = 0)
                const float s = rintf(x / speed[i]);                     // IEEE fp32 division
                dur = (int64_t)(s > 1.f ? s : 1.f);
            }
            const int f = forced[i];
            if (f >= 0) dur = f;
        }
        dur_out[i] = dur;
        acc += dur;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums_out[b] = red[0];
}

// The multiply and the add round separately (no fma): the torch restatement does the same two fp32 operations.
__device__ __forceinline__ float scale_shift(float c, float s, float b) {
#pragma clang fp contract(off)
    const float m = c * s;
    return m + b;
}

// Today's rule of one frame of phoneme k = b * Pn + j, on the clamped predictions p, e: forced, else scaled and shifted.
__device__ __forceinline__ void phoneme_rule(float &p, float &e, int64_t k, const float *__restrict__ ps, const float *__restrict__ pb,
                                             const float *__restrict__ es, const float *__restrict__ eb, const float *__restrict__ fp,
                                             const float *__restrict__ fe) {
    const float f = fp[k], g = fe[k];
    if (f == f) p = f;                                                   // forced (not NaN)
    else if (p > 0.f) p = clamp01(scale_shift(p, ps[k], pb[k]));         // voiced; an unvoiced frame (0) stays unvoiced
    e = g == g ? g : clamp01(scale_shift(e, es[k], eb[k]));
}

__global__ __launch_bounds__(256) void prosody_variance_kernel(const float *__restrict__ pitch, const float *__restrict__ energy,
                                                               const int64_t *__restrict__ idx, const int64_t *__restrict__ lens,
                                                               const float *__restrict__ ps, const float *__restrict__ pb,
                                                               const float *__restrict__ es, const float *__restrict__ eb,
                                                               const float *__restrict__ fp, const float *__restrict__ fe,
                                                               float *__restrict__ pitch_out, float *__restrict__ energy_out,
                                                               int64_t total, int Pn, int T) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / T;
        const int t = (int)(i - b * T);
        float p = clamp01(pitch[i]), e = clamp01(energy[i]);
        const int64_t j = t < lens[b] ? idx[i] : -1;
        if (j >= 0 && j < Pn) phoneme_rule(p, e, b * Pn + j, ps, pb, es, eb, fp, fe);   // anything else keeps the clamped prediction
        pitch_out[i] = p;
        energy_out[i] = e;
    }
}

// Frame-level contours.  One workgroup per row.  Phase 1: the exclusive prefix sums of the row's dur and sd into two int32 LDS tables
// (a wave scan by __shfl_up, the waves' totals through LDS, a carry from chunk to chunk of 256 phonemes, as lr_index_kernel; sums are
// formed in int64 and saturate, and a frame only ever reads the entries below its own t).  Phase 2: frame t of phoneme j reads source
// frame s = cs_s[j] + floor((2k + 1) m / (2n)), k = t - cs_t[j]; a value that is there and not NaN wins over phoneme_rule.  A table
// that does not fit its row (k outside [0, n), s outside [0, Sn)) gives no contour value for that frame, never an access outside.
constexpr int PC_MAX = 4096;                                             // phonemes and source frames per row: 2 x 16 KB of LDS

__device__ __forceinline__ int sat_i32(int64_t v) { return v > 2147483647LL ? 2147483647 : (int)v; }

__global__ __launch_bounds__(256) void prosody_contour_kernel(const float *__restrict__ pitch, const float *__restrict__ energy,
                                                              const int64_t *__restrict__ idx, const int64_t *__restrict__ lens,
                                                              const float *__restrict__ ps, const float *__restrict__ pb,
                                                              const float *__restrict__ es, const float *__restrict__ eb,
                                                              const float *__restrict__ fp, const float *__restrict__ fe,
                                                              const int64_t *__restrict__ dur, const int *__restrict__ sd,
                                                              const float *__restrict__ pc, const float *__restrict__ ec,
                                                              float *__restrict__ pitch_out, float *__restrict__ energy_out, int Pn, int T,
                                                              int Sn) {
    __shared__ int cs_t[PC_MAX], cs_s[PC_MAX];
    __shared__ int64_t wtot[2][4];
    __shared__ int64_t carry[2];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float *prow = pitch + b * T, *erow = energy + b * T;
    float *po = pitch_out + b * T, *eo = energy_out + b * T;
    if (Pn > PC_MAX || Sn > PC_MAX) {                                    // beyond the tables: the clamped predictions (the host reports it)
        for (int t = tid; t < T; t += 256) { po[t] = clamp01(prow[t]); eo[t] = clamp01(erow[t]); }
        return;
    }
    const int64_t *drow = dur + b * Pn;
    const int *srow = sd + b * Pn;
    if (tid == 0) carry[0] = carry[1] = 0;
    __syncthreads();
    for (int base = 0; base < Pn; base += 256) {
        const int j = base + tid;
        int64_t n = 0, m = 0;
        if (j < Pn) { n = drow[j]; n = n > 0 ? n : 0; m = srow[j]; m = m > 0 ? m : 0; }
        int64_t vt = n, vs = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                               // wave inclusive scans
            const int64_t ut = __shfl_up(vt, o, 64), us = __shfl_up(vs, o, 64);
            if (lane >= o) { vt += ut; vs += us; }
        }
        if (lane == 63) { wtot[0][w] = vt; wtot[1][w] = vs; }
        __syncthreads();
        int64_t ot = carry[0], os = carry[1];
        for (int k = 0; k < w; ++k) { ot += wtot[0][k]; os += wtot[1][k]; }
        if (j < Pn) { cs_t[j] = sat_i32(vt - n + ot); cs_s[j] = sat_i32(vs - m + os); }      // exclusive
        __syncthreads();
        if (tid == 0) {
            carry[0] += wtot[0][0] + wtot[0][1] + wtot[0][2] + wtot[0][3];
            carry[1] += wtot[1][0] + wtot[1][1] + wtot[1][2] + wtot[1][3];
        }
        __syncthreads();
    }
    const int64_t len = lens[b];
    const float *pcr = pc ? pc + b * Sn : nullptr, *ecr = ec ? ec + b * Sn : nullptr;
    for (int t = tid; t < T; t += 256) {
        float p = clamp01(prow[t]), e = clamp01(erow[t]);
        const int64_t j = t < len ? idx[b * T + t] : -1;
        if (j >= 0 && j < Pn) {
            const int64_t k = b * Pn + j;
            phoneme_rule(p, e, k, ps, pb, es, eb, fp, fe);
            const int64_t n = drow[j], m = srow[j], kt = (int64_t)t - cs_t[j];
            if (m > 0 && n > 0 && kt >= 0 && kt < n) {
                const int64_t s = (int64_t)cs_s[j] + ((2 * kt + 1) * m) / (2 * n);
                if (s >= 0 && s < Sn) {
                    if (pcr) {
                        const float v = pcr[s];
                        if (v == v) p = v > 0.f ? clamp01(scale_shift(v, ps[k], pb[k])) : v;   // an unvoiced source frame stays unvoiced
                    }
                    if (ecr) {
                        const float v = ecr[s];
                        if (v == v) e = clamp01(scale_shift(v, es[k], eb[k]));
                    }
                }
            }
        }
        po[t] = p;
        eo[t] = e;
    }
}

}  // namespace

extern "C" int kk_prosody_durations(const float *d, const float *speed, const int *forced, const int *plens, int64_t *dur_out,
                                    int64_t *sums_out, int B, int Pn, void *stream) {
    KK_REQUIRE(d && speed && forced && dur_out && sums_out && B > 0 && Pn > 0, "kk_prosody_durations: bad args");
    hipLaunchKernelGGL(prosody_durations_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, d, speed, forced, plens, dur_out, sums_out, Pn);
    KK_LAUNCH_CHECK("kk_prosody_durations");
    return 0;
}

extern "C" int kk_prosody_variance(const float *pitch, const float *energy, const int64_t *idx, const int64_t *lens, const float *ps,
                                   const float *pb, const float *es, const float *eb, const float *fp, const float *fe, float *pitch_out,
                                   float *energy_out, int B, int Pn, int T, void *stream) {
    KK_REQUIRE(pitch && energy && idx && lens && ps && pb && es && eb && fp && fe && pitch_out && energy_out && B > 0 && Pn > 0 && T > 0,
               "kk_prosody_variance: bad args");
    const int64_t total = (int64_t)B * T;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(prosody_variance_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, pitch,
                       energy, idx, lens, ps, pb, es, eb, fp, fe, pitch_out, energy_out, total, Pn, T);
    KK_LAUNCH_CHECK("kk_prosody_variance");
    return 0;
}

extern "C" int kk_prosody_contour(const float *pitch, const float *energy, const int64_t *idx, const int64_t *lens, const float *ps,
                                  const float *pb, const float *es, const float *eb, const float *fp, const float *fe, const int64_t *dur,
                                  const int *sd, const float *pc, const float *ec, float *pitch_out, float *energy_out, int B, int Pn,
                                  int T, int Sn, void *stream) {
    KK_REQUIRE(pitch && energy && idx && lens && ps && pb && es && eb && fp && fe && dur && sd && pitch_out && energy_out && B > 0 &&
                   Pn > 0 && T > 0 && Sn >= 0 && (Sn > 0 || (!pc && !ec)),
               "kk_prosody_contour: bad args");
    hipLaunchKernelGGL(prosody_contour_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pitch, energy, idx, lens, ps, pb, es, eb, fp, fe,
                       dur, sd, pc, ec, pitch_out, energy_out, Pn, T, Sn);
    KK_LAUNCH_CHECK("kk_prosody_contour");
    if (Pn > PC_MAX || Sn > PC_MAX)                                      // (the rows hold the clamped predictions)
        return kk_fail(KK_EINVAL, "kk_prosody_contour: Pn = %d or Sn = %d exceeds the %d-entry tables", Pn, Sn, PC_MAX);
    return 0;
}
