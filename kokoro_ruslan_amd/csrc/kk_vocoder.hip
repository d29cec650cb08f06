// HiFi-GAN generator kernels (kokoro_ruslan_amd/vocoder.py): a batch of mels to waveforms on the device.
//
//  implicit-GEMM conv   Conv1d(Cin, Cout, k, dilation d, padding (k-1)d/2) and the polyphase ConvTranspose1d on one MFMA core
//  post                 leaky_relu(., 0.01) -> Conv1d(C, 1, k, padding (k-1)/2) -> tanh, a per-sample reduction
//
// Layout: activations are channels-last fp32 [rows, C].  The utterances of a batch are packed back to back along time; seg[0..nseg]
// holds their start rows (seg[0] = 0, seg[nseg] = rows) in the row units of the layer's INPUT.  A tap reading row r + off is live only
// when that row lies in r's own utterance: every conv zero-pads at its own utterance's ends, as on a single-utterance tensor.
//
// Determinism: an output element's reduction runs over (tap, 32-channel chunk, MFMA k-step) in an order fixed by the layer shape; one
// tile shape, no split-K, no atomics.  So a sample's bits do not depend on the other utterances of the batch or on its position.
#include "kk_common.h"

namespace {

constexpr int VBM = 128, VBN = 64, VKC = 32;       // rows x output channels per workgroup (4 waves of 32 rows x 64), K chunk

struct VocConv {
    const float *x;        // [rows_in, cin]
    const void *w;         // [taps][npad][kpad] of T (tap-major, K contiguous, zero padded)
    const float *bias;     // [bias_mod] (index n % bias_mod) or null
    const float *res;      // [rows, n] residual added after the bias, or null (may alias y)
    const float *mrf;      // [rows, n] multi-receptive-field sum the result is added to, or null (may alias y)
    float *y;              // [rows, n]
    const int *seg;        // [nseg + 1] utterance starts in input rows
    int64_t rows;          // output rows (= input rows: the polyphase form writes u*Cout channels per input row)
    int cin, kpad, n, npad, bias_mod, taps, off0, dil, nseg, mrf_div;
    float slope;           // leaky_relu slope applied to the operand on load (1 = identity)
};

__device__ __forceinline__ void find_seg(const int *__restrict__ seg, int nseg, int64_t r, int &lo_row, int &hi_row) {
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= r) lo = mid;
        else hi = mid;
    }
    lo_row = seg[lo];
    hi_row = seg[lo + 1];
}

__device__ __forceinline__ float lrelu(float v, float s) { return v >= 0.f ? v : v * s; }

template <typename T>
__global__ __launch_bounds__(256) void voc_conv_kernel(const VocConv a) {
    constexpr bool BF = sizeof(T) == 2;
    constexpr int KP = VKC + (BF ? 8 : 4);                        // LDS row pitch: 80 / 144 bytes, rows stay 16-byte aligned
    __shared__ __attribute__((aligned(16))) T As[VBM * KP];
    __shared__ __attribute__((aligned(16))) T Bs[VBN * KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * VBM;
    const int col0 = blockIdx.y * VBN;

    // operand rows of this thread: tid / 8 + 32 i (i < 4), channels (tid % 8) * 4 .. + 3 of each K chunk
    const int c4 = (tid & 7) * 4, ar = tid >> 3;
    int64_t arow[4];
    int slo[4], shi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        arow[i] = row0 + ar + 32 * i;
        slo[i] = shi[i] = 0;                                      // rows past the end: no live tap
        if (arow[i] < a.rows) find_seg(a.seg, a.nseg, arow[i], slo[i], shi[i]);
    }

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

    const T *W = reinterpret_cast<const T *>(a.w);
    for (int j = 0; j < a.taps; ++j) {
        const int off = a.off0 + j * a.dil;
        for (int k0 = 0; k0 < a.kpad; k0 += VKC) {
            const int c = k0 + c4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t src = arow[i] + off;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < a.cin && src >= slo[i] && src < shi[i]) v = ld4(a.x + src * a.cin + c);
                T *d = As + (ar + 32 * i) * KP + c4;
                d[0] = (T)lrelu(v.x, a.slope);
                d[1] = (T)lrelu(v.y, a.slope);
                d[2] = (T)lrelu(v.z, a.slope);
                d[3] = (T)lrelu(v.w, a.slope);
            }
            const T *wt = W + ((int64_t)j * a.npad + col0) * a.kpad + k0;
            if constexpr (BF) {                                   // 64 x 32 bf16: one 16-byte load per thread
                const int bc = tid >> 2, bk = (tid & 3) * 8;
                *reinterpret_cast<bf16x8 *>(Bs + bc * KP + bk) = *reinterpret_cast<const bf16x8 *>(wt + (int64_t)bc * a.kpad + bk);
            } else {                                              // 64 x 32 f32: two
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int idx = tid + 256 * i, bc = idx >> 3, bk = (idx & 7) * 4;
                    st4(reinterpret_cast<float *>(Bs + bc * KP + bk), ld4(reinterpret_cast<const float *>(wt + (int64_t)bc * a.kpad + bk)));
                }
            }
            __syncthreads();
            const T *Aw = As + (wave * 32 + l31) * KP;
            const T *B0 = Bs + l31 * KP, *B1 = Bs + (32 + l31) * KP;
            if constexpr (BF) {
#pragma unroll
                for (int kk = 0; kk < VKC; kk += 16) {
                    const bf16x8 av = *reinterpret_cast<const bf16x8 *>(Aw + kk + half * 8);
                    const bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(B0 + kk + half * 8);
                    const bf16x8 b1 = *reinterpret_cast<const bf16x8 *>(B1 + kk + half * 8);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b1, acc1, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < VKC / 2; ++ks) {
                    const int k = 2 * ks + half;
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32((float)Aw[k], (float)B0[k], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32((float)Aw[k], (float)B1[k], acc1, 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }

    // epilogue: bias, residual, multi-receptive-field sum (first / accumulate / last with the division), fp32 store
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = col0 + 32 * h + l31;
        if (n >= a.n) continue;
        const float b = a.bias ? a.bias[n % a.bias_mod] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + wave * 32 + frag_row(r, half);
            if (row >= a.rows) continue;
            const int64_t idx = row * a.n + n;
            float v = (h == 0 ? acc0[r] : acc1[r]) + b;
            if (a.res) v = v + a.res[idx];
            if (a.mrf) v = a.mrf[idx] + v;
            if (a.mrf_div) v = v / (float)a.mrf_div;
            a.y[idx] = v;
        }
    }
}

// conv_post: y[r] = tanh(bias + sum_{j, c} w[j][c] * leaky_relu(x[r + j - (k-1)/2][c], slope)), taps masked to r's utterance.
// One thread per sample; taps then channels in order (fp32).
__global__ __launch_bounds__(256) void voc_post_kernel(const float *__restrict__ x, int64_t rows, int cin, const float *__restrict__ w,
                                                       const float *__restrict__ bias, float *__restrict__ y, int k, float slope,
                                                       const int *__restrict__ seg, int nseg) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int lo, hi;
    find_seg(seg, nseg, r, lo, hi);
    float acc = 0.f;
    for (int j = 0; j < k; ++j) {
        const int64_t src = r + j - (k - 1) / 2;
        if (src < lo || src >= hi) continue;
        const float *xr = x + src * cin, *wr = w + (int64_t)j * cin;
        for (int c = 0; c < cin; c += 4) {
            const float4 v = ld4(xr + c), g = ld4(wr + c);
            acc += g.x * lrelu(v.x, slope);
            acc += g.y * lrelu(v.y, slope);
            acc += g.z * lrelu(v.z, slope);
            acc += g.w * lrelu(v.w, slope);
        }
    }
    y[r] = tanhf(acc + (bias ? bias[0] : 0.f));
}

int launch_conv(VocConv &a, int w_bf16, hipStream_t s, const char *name) {
    const dim3 grid(kk_cdiv(a.rows, VBM), a.npad / VBN);
    if (w_bf16) {
        kk_note_kernel("voc_conv_bf16");
        hipLaunchKernelGGL(voc_conv_kernel<__bf16>, grid, dim3(256), 0, s, a);
    } else {
        kk_note_kernel("voc_conv_f32");
        hipLaunchKernelGGL(voc_conv_kernel<float>, grid, dim3(256), 0, s, a);
    }
    KK_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

extern "C" int kk_voc_convt_taps(int k, int stride, int *off0) {
    if (stride < 1 || k < stride || (k - stride) % 2 != 0) return 0;
    const int p = (k - stride) / 2;
    const int amin = p / stride, amax = (p + stride - 1) / stride, mmax = (k + stride - 1) / stride - 1;
    if (off0) *off0 = amin - mmax;
    return amax - (amin - mmax) + 1;
}

extern "C" int kk_voc_conv1d(const float *x, int64_t rows, int cin, const void *w, int kpad, int npad, const float *bias, float *y, int cout,
                             int k, int dilation, float slope, const int *seg, int nseg, const float *res, const float *mrf, int mrf_div,
                             int w_bf16, void *stream) {
    KK_REQUIRE(x && w && y && seg && rows > 0 && nseg > 0 && cin > 0 && cin % 4 == 0 && kpad >= cin && kpad % VKC == 0 && cout > 0 &&
                   npad >= cout && npad % VBN == 0 && k > 0 && k % 2 == 1 && dilation > 0 && mrf_div >= 0 && (void *)x != (void *)y,
               "kk_voc_conv1d: bad args (cin %% 4 == 0, kpad %% 32 == 0, npad %% 64 == 0, odd k, x != y)");
    VocConv a{x, w, bias, res, mrf, y, seg, rows, cin, kpad, cout, npad, cout, k, -(k - 1) / 2 * dilation, dilation, nseg, mrf_div, slope};
    return launch_conv(a, w_bf16, (hipStream_t)stream, "kk_voc_conv1d");
}

extern "C" int kk_voc_convt1d(const float *x, int64_t rows, int cin, const void *w, int kpad, int npad, const float *bias, float *y,
                              int cout, int k, int stride, float slope, const int *seg, int nseg, int w_bf16, void *stream) {
    int off0 = 0;
    const int taps = kk_voc_convt_taps(k, stride, &off0);
    KK_REQUIRE(taps > 0, "kk_voc_convt1d: ConvTranspose1d(k=%d, stride=%d, padding (k-stride)/2) needs k >= stride and k - stride even", k,
               stride);
    KK_REQUIRE(x && w && y && seg && rows > 0 && nseg > 0 && cin > 0 && cin % 4 == 0 && kpad >= cin && kpad % VKC == 0 && cout > 0 &&
                   npad >= cout * stride && npad % VBN == 0 && (void *)x != (void *)y,
               "kk_voc_convt1d: bad args (cin %% 4 == 0, kpad %% 32 == 0, npad %% 64 == 0 and >= stride * cout, x != y)");
    VocConv a{x, w, bias, nullptr, nullptr, y, seg, rows, cin, kpad, cout * stride, npad, cout, taps, off0, 1, nseg, 0, slope};
    return launch_conv(a, w_bf16, (hipStream_t)stream, "kk_voc_convt1d");
}

extern "C" int kk_voc_post(const float *x, int64_t rows, int cin, const float *w, const float *bias, float *y, int k, float slope,
                           const int *seg, int nseg, void *stream) {
    KK_REQUIRE(x && w && y && seg && rows > 0 && nseg > 0 && cin > 0 && cin % 4 == 0 && k > 0 && k % 2 == 1,
               "kk_voc_post: bad args (cin %% 4 == 0, odd k)");
    kk_note_kernel("voc_post");
    hipLaunchKernelGGL(voc_post_kernel, dim3(kk_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, x, rows, cin, w, bias, y, k, slope, seg,
                       nseg);
    KK_LAUNCH_CHECK("kk_voc_post");
    return 0;
}
