// Prosody control of the synthesis prefill (kokoro_ruslan_amd/prosody.py; the fp32 restatement: prosody_torch.py).
//
//  durations   frames per phoneme from the predictor's expm1(log_dur), a per-phoneme speed and forced values; the row sums
//  variance    per-frame pitch / energy from the predictors' outputs, per-phoneme scale + shift and forced values
//
// Both sit between the predictors and the length regulator / the bucket embeddings, twice per prefill and never in the decode loop:
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
        if (j >= 0 && j < Pn) {                                          // a frame of phoneme j; anything else keeps the clamped prediction
            const int64_t k = b * Pn + j;
            const float f = fp[k], g = fe[k];
            if (f == f) p = f;                                           // forced (not NaN)
            else if (p > 0.f) p = clamp01(scale_shift(p, ps[k], pb[k])); // voiced; an unvoiced frame (0) stays unvoiced
            e = g == g ? g : clamp01(scale_shift(e, es[k], eb[k]));
        }
        pitch_out[i] = p;
        energy_out[i] = e;
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
