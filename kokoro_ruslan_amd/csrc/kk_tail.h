// The forward sub-layer tail:  x_out = res + dropout(s) * DropPath * [RMSNorm(H)](y);  n = LayerNorm(x_out), statistics saved.
// Its arguments and its row body, for sublayer_out_fwd_kernel (kk_dropout.hip) and the persistent chain (kk_chain.hip).  The fused
// Linear + tail (kk_dropout.hip) and the encoder stack (kk_encstack.hip: tail_row) keep written-out mirrors of sublayer_out_row, see
// the notes there; all of them must agree to the bit, because kk_sublayer_in_bwd regenerates the masks and reads the saved statistics
// (tests/golden/tail_parent_digests.json and encstack_parent_digests.json pin the bits).  Device code only.
//   residual dropout + DropPath   model/transformers.py:16-40 (drop_path), :482-487, :569-581: x + dropout(drop_path(y))
//   FFN output dropout            transformers.py:111 (a second dropout in front of the residual one)
#pragma once
#include "kk_common.h"
#include <float.h>

namespace {

struct DropArgs {
    const uint32_t *seed;
    uint32_t site1, site2, site_dp;
    float p1, p2, dp_rate;
    int S;   // rows per sample (DropPath is per sample)
};

__device__ __forceinline__ float row_scale(const DropArgs &d, uint32_t seed, int64_t row) {
    if (d.dp_rate <= 0.f) return 1.f;
    return kk_drop_mul(seed, d.site_dp, (uint64_t)(row / d.S), kk_drop_threshold(d.dp_rate), 1.f / (1.f - d.dp_rate));
}

// ---- fused sub-layer tail (forward): [RMSNorm(H)] -> dropout(s) -> DropPath -> + residual -> [LayerNorm of the sum] ----
// One wave per row, the row in registers: replaces kk_rmsnorm_fwd + kk_dropout_fwd + kk_layernorm_fwd (three launches
// and two extra round trips of the [rows, H] tensor) at the end of every attention / feed-forward sub-layer.  The
// masks are the same functions of (seed, site, element) as dropout_kernel's, so kk_dropout_bwd regenerates them.
struct SubOutArgs {
    const void *y;                 // sub-layer result (TY): output projection (fp32) or FFN linear2 output (bf16 / fp32)
    const float *gain;             // optional RMSNorm(H) gain (GLU output_norm, transformers.py:109-110) ...
    float *rstd_f;                 // ... and where its 1/rms goes (saved for backward)
    const float *res;              // residual stream in
    float *x_out;                  // residual stream out = res + masks * norm(y)
    const float *ln_gamma, *ln_beta;   // optional LayerNorm of x_out (the next sub-layer's pre-norm / the stack's final norm)
    void *n;                       // its output (TN)
    float *mean, *rstd;
    int64_t rows;
    int H;
    int wt;                        // write-through output stores (kk_write_through(rows))
    DropArgs d;
};

// one row, one wave (every lane active); called by sublayer_out_fwd_kernel (kk_dropout.hip) and by the persistent chain (kk_chain.hip)
template <typename TY, typename TN, int NV>
__device__ __forceinline__ void sublayer_out_row(const SubOutArgs &a, const int64_t row) {
    const int lane = threadIdx.x & 63, H = a.H;
    const uint32_t seed = *a.d.seed;
    const uint32_t t1 = kk_drop_threshold(a.d.p1), t2 = kk_drop_threshold(a.d.p2);
    const float k1 = a.d.p1 > 0.f ? 1.f / (1.f - a.d.p1) : 1.f, k2 = a.d.p2 > 0.f ? 1.f / (1.f - a.d.p2) : 1.f;
    const TY *yr = static_cast<const TY *>(a.y) + row * H;
    // every global load of the row is issued here, before the first reduction: the kernel is three dependent phases
    // (RMS statistic -> residual add -> LayerNorm) and was paying one memory latency per phase
    float4 v[NV], rres[NV], gg[NV], lg[NV], lb[NV];
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        v[i] = c < H ? ldv4<TY>(yr + c) : z;
        rres[i] = c < H ? ld4(a.res + row * H + c) : z;
        gg[i] = (a.gain && c < H) ? ld4(a.gain + c) : z;
        lg[i] = (a.ln_gamma && c < H) ? ld4(a.ln_gamma + c) : z;
        lb[i] = (a.ln_gamma && c < H) ? ld4(a.ln_beta + c) : z;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) q += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    float rs = 1.f;
    if (a.gain) {
        rs = 1.f / sqrtf(wave_sum(q) / (float)H + FLT_EPSILON);
        if (lane == 0) a.rstd_f[row] = rs;
    }
    const float dp = row_scale(a.d, seed, row);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < H) {
            float o[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            if (a.gain) {
                const float4 g = gg[i];
                o[0] = o[0] * rs * g.x; o[1] = o[1] * rs * g.y; o[2] = o[2] * rs * g.z; o[3] = o[3] * rs * g.w;
            }
            const float4 r = rres[i];
            const float rr[4] = {r.x, r.y, r.z, r.w};
            float m1[4], m2[4];
            kk_drop_mul4(seed, a.d.site1, (uint64_t)row * H + c, t1, k1, m1);
            kk_drop_mul4(seed, a.d.site2, (uint64_t)row * H + c, t2, k2, m2);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = o[e] * (dp * m1[e] * m2[e]) + rr[e];
            v[i] = make_float4(o[0], o[1], o[2], o[3]);
            st4_out(a.x_out + row * H + c, v[i], a.wt);
            s += o[0] + o[1] + o[2] + o[3];
        }
    }
    if (!a.ln_gamma) return;
    const float mean = wave_sum(s) / (float)H;
    float qq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane * 4 + 256 * i < H) {
            const float e0 = v[i].x - mean, e1 = v[i].y - mean, e2 = v[i].z - mean, e3 = v[i].w - mean;
            qq += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(qq) / (float)H + 1e-5f);
    TN *nr = static_cast<TN *>(a.n) + row * H;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < H) {
            const float4 g = lg[i], b = lb[i];
            stv4_out<TN>(nr + c, make_float4((v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y,
                                         (v[i].z - mean) * rstd * g.z + b.z, (v[i].w - mean) * rstd * g.w + b.w), a.wt);
        }
    }
    if (lane == 0) {
        a.mean[row] = mean;
        a.rstd[row] = rstd;
    }
}

}  // namespace
