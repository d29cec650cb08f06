// Band-limited resampling (kokoro_ruslan_amd/resample.py): a batch of waveforms, each with its own rate pair, by windowed-sinc
// interpolation: torchaudio's sinc_interp_hann with lowpass_filter_width = 6 and rolloff = 0.99, the resampler behind the reference's
// train-time speed perturbation (data/dataset.py:674-684) and its corpus resampling (:662-665).
//
// With the rates reduced by their gcd to o (in) and n (out), base = 0.99 min(o, n), width = ceil(6 o / base), output sample
// j = q n + p (0 <= p < n) is
//     y[j] = sum over m = c - width .. c + width, c = floor(p o / n), of x[q o + m] h(t),      x = 0 outside the utterance
//     t    = base (m n - p o) / (o n) clamped to [-6, 6],   h(t) = (base / o) sinc(pi t) cos(pi t / 12)^2
// The clamp puts every tap past the window on its zero, so the fixed 2 width + 1 taps are the whole filter.  torchaudio tabulates h
// for every phase p (a [n, 2 width + o] matrix of which ~13 taps per row are non-zero: 1.85 GB for 22050 -> 20947) and convolves;
// here every tap is evaluated where it is used.  The phase numerator m n - p o is an INTEGER (below 2^24 wherever the tap is
// non-zero): it is formed in integers and scaled once by the fp32 rounding of the fp64 constant base / (o n), and sin / cos take
// their argument in half-turns (sinpif / cospif: exact range reduction), so the tap carries a few ulp of error whatever the rates;
// forming p / n and m / o separately in fp32, as torchaudio does, loses 4e-4 of the signal for coprime rates.
//
// Layout: waveforms packed back to back, in by woff_in and out by woff_out (int64, B + 1); the output length of an utterance is what
// woff_out says (the host's ceil(n L / o)).  A workgroup owns RS_TILE consecutive outputs of one utterance: it stages the input span
// they read into LDS with coalesced loads (x / (peak + 1e-9) on load when peak is given, zeros outside the utterance), then every
// lane sums its outputs over ascending m with fp32 FMAs.  An output's sum depends on its own utterance alone: bit for bit the same
// alone, in any batch, in any order.
#include "kk_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;                 // outputs per workgroup
constexpr int RS_SPAN = 4096;                 // staged input samples (16 KB of LDS): RS_TILE outputs at o / n <= 3.9, else fewer per pass

struct RsRate {                               // one per utterance (int32 x 8 on the host side)
    int o, n, width;                          // reduced rates; taps on each side of the centre (0 with o = n = 1: a copy)
    float scale;                              // fp32(base / (o n))
    float gain;                               // fp32(base / o)
    int pad[3];
};

struct RsArgs {
    const float *wave;
    const int64_t *woff_in;
    const float *peak;                        // or null
    const RsRate *rate;
    const int2 *tiles;                        // {utterance, first output sample of the tile}
    const int64_t *woff_out;
    float *out;
};

// `outputs` consecutive outputs read at most this many input samples
__host__ __device__ inline int64_t rs_span_bound(int64_t outputs, int o, int n, int width) { return (outputs * o) / n + 2 * (int64_t)width + 2; }

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsArgs a) {
    __shared__ float xs[RS_SPAN];
    const int2 tl = a.tiles[blockIdx.x];
    const int b = tl.x;
    const RsRate r = a.rate[b];
    const int64_t w0 = a.woff_in[b], L = a.woff_in[b + 1] - w0;
    const int64_t y0 = a.woff_out[b], Lout = a.woff_out[b + 1] - y0;
    const float d = a.peak ? a.peak[b] + 1e-9f : 1.f;
    const int64_t j_end = min((int64_t)tl.y + RS_TILE, Lout);
    int per_pass = RS_TILE;                                           // the host has checked that RS_THREADS outputs fit
    while (per_pass > RS_THREADS && rs_span_bound(per_pass, r.o, r.n, r.width) > RS_SPAN) per_pass >>= 1;

    for (int64_t j0 = tl.y; j0 < j_end; j0 += per_pass) {
        const int64_t j1 = min(j0 + per_pass, j_end);
        const int64_t s0 = (j0 * r.o) / r.n - r.width;                // first and last input sample the outputs [j0, j1) read
        const int span = (int)(((j1 - 1) * r.o) / r.n + r.width - s0) + 1;
        __syncthreads();                                              // (the previous pass has read xs)
        for (int i = threadIdx.x; i < min(span, RS_SPAN); i += RS_THREADS) {
            const int64_t s = s0 + i;
            float v = 0.f;
            if (s >= 0 && s < L) {
                v = a.wave[w0 + s];
                if (a.peak) v = v / d;
            }
            xs[i] = v;
        }
        __syncthreads();
        for (int64_t j = j0 + threadIdx.x; j < j1; j += RS_THREADS) {
            const int64_t q = j / r.n;
            const int64_t po = (j - q * r.n) * r.o;                   // p o  (< o n)
            const int64_t c = po / r.n;
            const float *x = xs + (q * r.o + c - r.width - s0);       // x[q o + m] for m = c - width
            int num = (int)(c * r.n - po) - r.width * r.n;            // m n - p o: |.| <= (width + 1) n < 2^31 (kk_resample_supported)
            float acc = 0.f;
            for (int k = 0; k <= 2 * r.width; ++k, num += r.n) {
                const float t = fminf(fmaxf((float)num * r.scale, -6.f), 6.f);
                const float c12 = cospif(t * (1.f / 12.f));
                const float sinc = t == 0.f ? 1.f : sinpif(t) / (3.14159265358979323846f * t);
                acc = fmaf(x[k], r.gain * sinc * (c12 * c12), acc);
            }
            a.out[y0 + j] = acc;
        }
    }
}

// x /= peak + 1e-9 in place: the second normalisation of the reference's normalise -> resample -> normalise
__global__ __launch_bounds__(RS_THREADS) void resample_normalise_kernel(float *__restrict__ wave, const int64_t *__restrict__ woff,
                                                                        const float *__restrict__ peak) {
    const int b = blockIdx.y;
    const int64_t w0 = woff[b], n = woff[b + 1] - w0;
    const float d = peak[b] + 1e-9f;
    const int64_t i = ((int64_t)blockIdx.x * RS_THREADS + threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) wave[w0 + i + k] = wave[w0 + i + k] / d;
}

}  // namespace

extern "C" int kk_resample_tile(void) { return RS_TILE; }

extern "C" int kk_resample_supported(int o, int n, int width) {
    return o >= 1 && n >= 1 && width >= 0 && rs_span_bound(RS_THREADS, o, n, width) <= RS_SPAN &&
                   ((int64_t)width + 1) * (o > n ? o : n) < ((int64_t)1 << 31)
               ? 1
               : 0;
}

extern "C" int kk_resample(const float *wave, const int64_t *woff_in, const float *peak, const int *rate, const int *tiles, int ntiles,
                           const int64_t *woff_out, float *out, void *stream) {
    KK_REQUIRE(wave && woff_in && rate && tiles && woff_out && out && ntiles > 0, "kk_resample: bad args");
    static_assert(sizeof(RsRate) == 32, "RsRate is int32 x 8 on the host side");
    RsArgs r{wave, woff_in, peak, (const RsRate *)rate, (const int2 *)tiles, woff_out, out};
    kk_note_kernel("resample");
    hipLaunchKernelGGL(resample_kernel, dim3(ntiles), dim3(RS_THREADS), 0, (hipStream_t)stream, r);
    KK_LAUNCH_CHECK("kk_resample");
    return 0;
}

extern "C" int kk_resample_normalise(float *wave, const int64_t *woff, int B, int64_t max_samples, const float *peak, void *stream) {
    KK_REQUIRE(wave && woff && peak && B > 0 && B <= 65535 && max_samples > 0, "kk_resample_normalise: bad args");
    kk_note_kernel("resample_normalise");
    hipLaunchKernelGGL(resample_normalise_kernel, dim3(kk_cdiv(max_samples, 4 * RS_THREADS), B), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       wave, woff, peak);
    KK_LAUNCH_CHECK("kk_resample_normalise");
    return 0;
}
