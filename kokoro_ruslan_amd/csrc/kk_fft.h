// The 1024-point real STFT of one wave64, the single copy that feature extraction (kk_features.hip), Griffin-Lim (kk_griffinlim.hip) and
// spectral denoising (kk_denoise.hip) share: n_fft = win = 1024, hop 256, 513 bins, center = True with reflect padding by index.
//
//  fft512       a 512-point complex transform per wave, 8 points per lane, three radix-8 passes in registers with two LDS exchanges
//               (XOR-swizzled so each b64 access is conflict-free within its lane group)
//  forward      stft_frame_fwd (reflected index, the caller's sample load, window, fft512<-1>, Z in natural order in the wave's slot), then
//               the split step per bin: stft_split_pair (bins k and 512 - k from one pair of loads; bin 512 from the k = 0 pair) or
//               stft_split (bin k alone) with stft_bin512.  The two forms may differ in the last bit or the sign of a zero on bin 512:
//               a kernel keeps the one it has.
//  inverse      stft_inv_pre (Z'[k] from Y[k] and Y[512 - k]), stft_inv_tail (fft512<1>, 1 / 1024, window, into the frame's LDS row),
//               stft_ola (one padded position: the frames that cover it summed in ascending order, over the window-square envelope)
//
// Where a sample comes from, which frames a tile owns and what is done to a bin stay with each kernel.  Everything here inlines.
// The forward half is written for a complex type C: those three kernels use float2, the spectral distance (kk_spectral.hip) double2.
#pragma once
#include "kk_common.h"

namespace {

// The transform is written once for a complex type C: float2 (every kernel but one) or double2 (kk_spectral.hip, whose sums are held
// to fp64).  cx(x, y) makes a C from two scalars of its precision.
__device__ __forceinline__ float2 cx(float x, float y) { return make_float2(x, y); }
__device__ __forceinline__ double2 cx(double x, double y) { return make_double2(x, y); }

template <class C> __device__ __forceinline__ C cmul(C a, C b) { return cx(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int SIGN, class C> __device__ __forceinline__ C dirw(C w) { return SIGN < 0 ? w : cx(w.x, -w.y); }
template <int SIGN, class C> __device__ __forceinline__ C mul_i(C a) {      // a . (SIGN i)
    return SIGN < 0 ? cx(a.y, -a.x) : cx(-a.y, a.x);
}

// In-place 8-point DFT, natural order in and out: X[k] = sum_n v[n] exp(SIGN 2 pi i n k / 8).
template <int SIGN, class C> __device__ __forceinline__ void dft8(C *v) {
    using S = decltype(v[0].x);
    constexpr S R = (S)0.70710678118654752440;
    C e[4], o[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                            // DFT4 of the even (h = 0) and odd (h = 1) samples
        const C a = v[h], b = v[h + 2], c = v[h + 4], d = v[h + 6];
        const C s0 = cx(a.x + c.x, a.y + c.y), s1 = cx(a.x - c.x, a.y - c.y);
        const C s2 = cx(b.x + d.x, b.y + d.y), s3 = mul_i<SIGN>(cx(b.x - d.x, b.y - d.y));
        C *y = h ? o : e;
        y[0] = cx(s0.x + s2.x, s0.y + s2.y);
        y[2] = cx(s0.x - s2.x, s0.y - s2.y);
        y[1] = cx(s1.x + s3.x, s1.y + s3.y);
        y[3] = cx(s1.x - s3.x, s1.y - s3.y);
    }
    o[1] = cmul(o[1], cx(R, SIGN * R));
    o[2] = mul_i<SIGN>(o[2]);
    o[3] = cmul(o[3], cx(-R, SIGN * R));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = cx(e[k].x + o[k].x, e[k].y + o[k].y);
        v[k + 4] = cx(e[k].x - o[k].x, e[k].y - o[k].y);
    }
}

// 512-point complex DFT of one wave: lane l holds v[m] = z[l + 64 m]; on return lane q holds v[k2] = Z[(q >> 3) + 8 (q & 7) + 64 k2].
// Z[k0 + 8 k1 + 64 k2] = sum_{l0} w8^(l0 k2) w64^(l0 k1) sum_{l1} w8^(l1 k1) w512^(l k0) sum_m w8^(m k0) z[l + 64 m], l = l0 + 8 l1.
// sl: this wave's 512-element LDS exchange slot.  tw1[j] = w512^(lane j), tw2[j] = w512^(8 (lane & 7) j) (forward sign).
template <int SIGN, class C> __device__ __forceinline__ void fft512(C *v, C *sl, const C *tw1, const C *tw2, int lane) {
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

constexpr int STFT_N = 1024, STFT_HOP = 256, STFT_BINS = STFT_N / 2 + 1;

template <class C> struct StftTwT { C tw1[8], tw2[8], twk[8]; };   // of one lane, from the table tw[j] = exp(-2 pi i j / 1024)
using StftTw = StftTwT<float2>;

template <class C> __device__ __forceinline__ void stft_twiddles(const C *tw, int lane, StftTwT<C> &t) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        t.tw1[j] = tw[(2 * lane * j) & (STFT_N - 1)];
        t.tw2[j] = tw[(16 * (lane & 7) * j) & (STFT_N - 1)];
        t.twk[j] = tw[lane + 64 * j];                          // w1024^k of bin k = lane + 64 j (the split step)
    }
}

// Index j of a signal of n samples under reflect padding.  One reflection: -n < j < 2 n - 1.  No overflow for n < 2^31.
__device__ __forceinline__ int reflect(int j, int n) { return j < 0 ? -j : (j >= n ? (n - 1) - (j - (n - 1)) : j); }

// fft512's output lane holds, in v[k2], the element of this natural-order index.
__device__ __forceinline__ int stft_nat(int lane, int k2) { return (lane >> 3) + 8 * (lane & 7) + 64 * k2; }

// Frame t of a signal of n samples (n > 512, t <= n / 256), windowed, through the 512-point complex transform: Z in natural order in the
// wave's slot sl.  load(j): sample j, 0 <= j < n, in the window's precision S.
template <class Load, class S, class C> __device__ __forceinline__ void stft_frame_fwd(Load load, int t, int n, const S *__restrict__ win,
                                                                                      C *sl, const StftTwT<C> &tw, int lane) {
    C v[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = lane + 64 * m;
        S s[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) s[h] = load(reflect(STFT_HOP * t - STFT_N / 2 + 2 * i + h, n));
        const C w = *reinterpret_cast<const C *>(win + 2 * i);
        v[m] = cx(s[0] * w.x, s[1] * w.y);
    }
    fft512<-1>(v, sl, tw.tw1, tw.tw2, lane);
    __syncwarp();
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) sl[stft_nat(lane, k2)] = v[k2];
    __syncwarp();
}

// The split step for bin k < 512 from Z in sl: X[k] = fe + c, X[512 - k] = conj(fe - c), with c = w^k fo,
// fe = (Z[k] + conj Z[512-k]) / 2, fo = (Z[k] - conj Z[512-k]) / 2i.
template <class C> __device__ __forceinline__ void stft_split_parts(const C *sl, C twk, int k, C &fe, C &c) {
    using S = decltype(twk.x);
    const C zk = sl[k], zm = sl[(STFT_N / 2 - k) & (STFT_N / 2 - 1)];
    fe = cx((zk.x + zm.x) * (S)0.5, (zk.y - zm.y) * (S)0.5);
    const C fo = cx((zk.y + zm.y) * (S)0.5, (zm.x - zk.x) * (S)0.5);
    c = cmul(twk, fo);
}

// X = bin k, Xm = bin 512 - k (k = 0: bins 0 and 512).
template <class C> __device__ __forceinline__ void stft_split_pair(const C *sl, C twk, int k, C &X, C &Xm) {
    C fe, c;
    stft_split_parts(sl, twk, k, fe, c);
    X = cx(fe.x + c.x, fe.y + c.y);
    Xm = cx(fe.x - c.x, c.y - fe.y);
}

// Bin k alone; bin 512 is then stft_bin512 on lane 0: even sum minus odd sum.
template <class C> __device__ __forceinline__ C stft_split(const C *sl, C twk, int k) {
    C fe, c;
    stft_split_parts(sl, twk, k, fe, c);
    return cx(fe.x + c.x, fe.y + c.y);
}
template <class C> __device__ __forceinline__ C stft_bin512(const C *sl) {
    const C z0 = sl[0];
    return cx(z0.x - z0.y, (decltype(z0.x))0);
}

// The inverse transform's input: Z'[k] = Y[k] + conj Y[512-k] + i w^-k (Y[k] - conj Y[512-k]), yk = Y[k], ym = Y[512 - k].
__device__ __forceinline__ float2 stft_inv_pre(float2 yk, float2 ym, float2 twk) {
    const float2 A = make_float2(yk.x + ym.x, yk.y - ym.y);
    const float2 C = cmul(make_float2(yk.x - ym.x, yk.y + ym.y), make_float2(twk.x, -twk.y));
    return make_float2(A.x - C.y, A.y + C.x);
}

// v = Z' of one frame (lane's v[m]: k = lane + 64 m) to its 1024 samples, scaled by 1 / 1024 and windowed, in the LDS row sl.
__device__ __forceinline__ void stft_inv_tail(float2 (&v)[8], float2 *sl, const float *__restrict__ win, const StftTw &tw, int lane) {
    fft512<1>(v, sl, tw.tw1, tw.tw2, lane);
    __syncwarp();
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
        const int i = stft_nat(lane, k2);
        const float2 w = *reinterpret_cast<const float2 *>(win + 2 * i);
        sl[i] = make_float2(v[k2].x * (1.f / STFT_N) * w.x, v[k2].y * (1.f / STFT_N) * w.y);
    }
}

// Overlap-add at position p of the padded signal: frames tlo .. thi (rows tlo - h0 .. of frm, stft_inv_tail's output) in ascending
// order, over the window-square envelope of the same frames.
__device__ __forceinline__ float stft_ola(const float (*frm)[STFT_N], int h0, int tlo, int thi, int p, const float *__restrict__ win) {
    float acc = 0.f, env = 0.f;
    for (int t = tlo; t <= thi; ++t) {
        const int o = p - STFT_HOP * t;
        const float w = win[o];
        acc += frm[t - h0][o];
        env += w * w;
    }
    return acc / env;
}

}  // namespace
