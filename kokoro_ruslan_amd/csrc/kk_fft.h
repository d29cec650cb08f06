// The wave64 FFT the Griffin-Lim (kk_griffinlim.hip) and feature-extraction (kk_features.hip) kernels share: a 512-point complex
// transform per wave, 8 points per lane, three radix-8 passes in registers with two LDS exchanges (XOR-swizzled so each b64 access is
// conflict-free within its lane group).  A 1024-point real transform is this plus the split step at the call site.
#pragma once
#include "kk_common.h"

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int SIGN> __device__ __forceinline__ float2 dirw(float2 w) { return SIGN < 0 ? w : make_float2(w.x, -w.y); }
template <int SIGN> __device__ __forceinline__ float2 mul_i(float2 a) {      // a . (SIGN i)
    return SIGN < 0 ? make_float2(a.y, -a.x) : make_float2(-a.y, a.x);
}

// In-place 8-point DFT, natural order in and out: X[k] = sum_n v[n] exp(SIGN 2 pi i n k / 8).
template <int SIGN> __device__ __forceinline__ void dft8(float2 *v) {
    constexpr float R = 0.70710678118654752f;
    float2 e[4], o[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                            // DFT4 of the even (h = 0) and odd (h = 1) samples
        const float2 a = v[h], b = v[h + 2], c = v[h + 4], d = v[h + 6];
        const float2 s0 = make_float2(a.x + c.x, a.y + c.y), s1 = make_float2(a.x - c.x, a.y - c.y);
        const float2 s2 = make_float2(b.x + d.x, b.y + d.y), s3 = mul_i<SIGN>(make_float2(b.x - d.x, b.y - d.y));
        float2 *y = h ? o : e;
        y[0] = make_float2(s0.x + s2.x, s0.y + s2.y);
        y[2] = make_float2(s0.x - s2.x, s0.y - s2.y);
        y[1] = make_float2(s1.x + s3.x, s1.y + s3.y);
        y[3] = make_float2(s1.x - s3.x, s1.y - s3.y);
    }
    o[1] = cmul(o[1], make_float2(R, SIGN * R));
    o[2] = mul_i<SIGN>(o[2]);
    o[3] = cmul(o[3], make_float2(-R, SIGN * R));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = make_float2(e[k].x + o[k].x, e[k].y + o[k].y);
        v[k + 4] = make_float2(e[k].x - o[k].x, e[k].y - o[k].y);
    }
}

// 512-point complex DFT of one wave: lane l holds v[m] = z[l + 64 m]; on return lane q holds v[k2] = Z[(q >> 3) + 8 (q & 7) + 64 k2].
// Z[k0 + 8 k1 + 64 k2] = sum_{l0} w8^(l0 k2) w64^(l0 k1) sum_{l1} w8^(l1 k1) w512^(l k0) sum_m w8^(m k0) z[l + 64 m], l = l0 + 8 l1.
// sl: this wave's 512-float2 LDS exchange slot.  tw1[j] = w512^(lane j), tw2[j] = w512^(8 (lane & 7) j) (forward sign).
template <int SIGN> __device__ __forceinline__ void fft512(float2 *v, float2 *sl, const float2 *tw1, const float2 *tw2, int lane) {
    dft8<SIGN>(v);
#pragma unroll
    for (int j = 1; j < 8; ++j) v[j] = cmul(v[j], dirw<SIGN>(tw1[j]));
    const int a = lane >> 3, b = lane & 7;
    __syncwarp();                                            // the slot's previous readers are done
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) sl[k0 * 64 + 8 * (a ^ k0) + b] = v[k0];          // element (k0, l = b + 8 a)
    __syncwarp();
#pragma unroll
    for (int l1 = 0; l1 < 8; ++l1) v[l1] = sl[a * 64 + 8 * (l1 ^ a) + b];           // lane (k0 = a, l0 = b)
    dft8<SIGN>(v);
#pragma unroll
    for (int j = 1; j < 8; ++j) v[j] = cmul(v[j], dirw<SIGN>(tw2[j]));
    __syncwarp();
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) sl[a * 64 + 8 * (k1 ^ a) + (b ^ k1)] = v[k1];    // element (k0 = a, k1, l0 = b)
    __syncwarp();
#pragma unroll
    for (int l0 = 0; l0 < 8; ++l0) v[l0] = sl[a * 64 + 8 * (b ^ a) + (l0 ^ b)];     // lane (k0 = a, k1 = b)
    dft8<SIGN>(v);
}

}  // namespace
