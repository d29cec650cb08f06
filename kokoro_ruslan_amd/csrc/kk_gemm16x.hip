// Large-tile family of the bf16-storage MFMA GEMM core (gfx950).
//
// Why it exists.  A compute unit pulls ~20 B/clk from L2 into LDS whatever the staging depth, so a GEMM
// launch cannot finish before   max over CUs of  sum over its workgroups of (BM + BN) * K * 2 bytes  have gone through a CU.
// kk_gemm16.hip's tiles (64x64, 128x64: ONE 32x32 accumulator per wave) sit on that floor for the model's big launches.
// The tiles here hold 2 - 6 accumulators per wave on 128x128 .. 256x192 workgroup tiles: 1.5 - 1.8x fewer bytes through the
// busiest CU for the q|k|v projections, linear1 + GLU, the linear2 dgrad + GLU', and the grouped weight gradients, and half
// the LDS fragment reads per MFMA.  One workgroup (eight waves, two per SIMD) per CU; tile chosen per launch by that byte count
// (the entry points of kk_gemm16.hip, by g16_cost).
//
// Same operand images as kk_gemm16.hip (see its header): LDS filled by buffer-load-to-LDS DMA, 16 bytes per lane;
//   k-contiguous operand: [rows][64] bf16, 16-byte chunk index XOR (row >> 1) & 7 applied on the global address;
//   k-strided operand: [64 k][rows] as it lies in memory, 32-byte blocks XOR-ed by a function of k, fragments by
//     ds_read_b64_tr_b16 (the XOR class follows the row pitch mod 256 bytes: 192- and 64-row images share one, 128 / 256 the other).
// Counted vmcnt + raw s_barrier keep NS - 1 k-tiles in flight across the barrier; LDS reads of the next 16-k slab(s) are in flight
// under the MFMAs of the current one (inline asm, counted lgkmcnt).
#include "kk_gemm16x_body.h"

namespace {

template <bool TA, bool TB, int BM, int BN, int NS, int EPI, int WR, int WC, int LW>
__global__ __launch_bounds__(64 * (WR * WC + LW)) void g16x_kernel(G16Args a) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (BM + BN) * BK * 2 + BN * 4];      // (static: up to 145 KB, one workgroup per CU; the tail: the tile's bias row)
    g16x_body<TA, TB, BM, BN, NS, EPI, WR, WC, LW>(a, blockIdx.x, smem);
}
template <bool TA, bool TB, int BM, int BN, int NS, int WR, int WC, int LW>
__global__ __launch_bounds__(64 * (WR * WC + LW)) void g16x_group_kernel(G16Group g) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (BM + BN) * BK * 2 + BN * 4];
    // Which tiles share an XCD's L2.  The dispatcher places workgroup w on XCD w % 8; with xcd_chunks set, XCD x works on the x-th
    // contiguous eighth of the concatenation of ALL problems' tile lists (each in its own sweep order), not on an eighth of every
    // problem: the 30 tiles it runs side by side then come from one or two problems and share operand panels — 115 instead of 188
    // panel fetches per decoder-layer launch from the Infinity Cache into the eight L2s (these launches are bound by the latency of
    // the L2 misses: ~64 requests in flight per CU).
    int w = (int)blockIdx.x;
    if (g.xcd_chunks) w = g16_xcd_tile(w, g.start[g.n]);
    int i = 0;
    while (i + 1 < g.n && w >= g.start[i + 1]) ++i;
    // (hipcc's host pass rejects a g16x_body specialization named by two kernels when TA = TB = true: the weight-gradient layout is
    // instantiated here only; single weight-gradient GEMMs are groups of one)
    g16x_body<TA, TB, BM, BN, NS, 0, WR, WC, LW>(g.p[i], w - g.start[i], smem);
}

#ifdef KK_TUNING_HOOKS
int g16x_probe_bits = 0;                                        // tools: probe bits for every launch of the family, and the stamp buffer of bit 32
void *g16x_probe_buf = nullptr;
#endif
template <bool TA, bool TB, int BM, int BN, int NS, int EPI, int WR, int WC, int LW>
int launch_x(const G16Args &a0, const char *name, hipStream_t s) {
#ifdef KK_TUNING_HOOKS
    G16Args a = a0;
    a.dbg |= g16x_probe_bits;
    if ((a.dbg & 32) && EPI != 0) a.dl_out = static_cast<float *>(g16x_probe_buf);
#else
    const G16Args &a = a0;
#endif
    kk_note_kernelf("g16x<%d,%d,%d,%d,%d,%d,%d,%d,%d>", (int)TA, (int)TB, BM, BN, NS, EPI, WR, WC, LW);
    if (kk_capture(kk_last_kernel(), a, dim3(a.tiles_m * a.tiles_n), 64 * (WR * WC + LW), 0)) return 0;
    hipLaunchKernelGGL((g16x_kernel<TA, TB, BM, BN, NS, EPI, WR, WC, LW>), dim3(a.tiles_m * a.tiles_n), dim3(64 * (WR * WC + LW)), 0, s, a);
    KK_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

#ifdef KK_TUNING_HOOKS
void kk_g16x_probe(int bits, void *buf) { g16x_probe_bits = bits; g16x_probe_buf = buf; }
#endif
// Loader-wave form of every launch: 1 = four compute + four loader waves (the product), 0 = every wave loads and computes (the form
// of gemm16_body), 2 = eight compute + four loader waves.  0 and 2 are A/B arms: they are instantiated in the TOOLS flavour only
// (KK_TUNING_HOOKS, KK_G16X_LW); the product build folds the choice to 1 and carries one kernel per tile and layout.
#ifdef KK_TUNING_HOOKS
int g16x_lw = kk_tune_env("KK_G16X_LW", 1);
int g16x_ns4 = kk_tune_env("KK_G16X_NS4", 0);          // tools: four stages (three k-tiles in flight) on the 128 x 128 tile
#define G16X_LW(lw1, lw0) (g16x_lw ? (lw1) : (lw0))
#else
#define G16X_LW(lw1, lw0) (lw1)
#endif

void kk_g16x_tile(int cfg, int *bm, int *bn) {
    static const int t[G16X_NCFG][2] = {{128, 128}, {256, 128}, {128, 192}, {256, 192}};
    *bm = t[cfg][0];
    *bn = t[cfg][1];
}

int kk_g16x_plain(int cfg, int ta, int tb, const G16Args &a, hipStream_t s) {
    const int lay = (ta ? 2 : 0) | (tb ? 1 : 0);
    if (cfg == G16X_128x128) {
#ifdef KK_TUNING_HOOKS
        if (g16x_ns4 && lay == 0) return launch_x<false, false, 128, 128, 4, 0, 2, 2, 4>(a, "kk_gemm", s);
        if (g16x_ns4 && lay == 1) return launch_x<false, true, 128, 128, 4, 0, 2, 2, 4>(a, "kk_gemm", s);
#endif
        if (lay == 0) return G16X_LW((launch_x<false, false, 128, 128, 3, 0, 2, 2, 4>(a, "kk_gemm", s)), (launch_x<false, false, 128, 128, 3, 0, 4, 2, 0>(a, "kk_gemm", s)));
        if (lay == 1) return G16X_LW((launch_x<false, true, 128, 128, 3, 0, 2, 2, 4>(a, "kk_gemm", s)), (launch_x<false, true, 128, 128, 3, 0, 4, 2, 0>(a, "kk_gemm", s)));
    } else if (cfg == G16X_256x128) {
        if (lay == 0) return G16X_LW((launch_x<false, false, 256, 128, 3, 0, 2, 2, 4>(a, "kk_gemm", s)), (launch_x<false, false, 256, 128, 3, 0, 4, 2, 0>(a, "kk_gemm", s)));
        if (lay == 1) return G16X_LW((launch_x<false, true, 256, 128, 3, 0, 2, 2, 4>(a, "kk_gemm", s)), (launch_x<false, true, 256, 128, 3, 0, 4, 2, 0>(a, "kk_gemm", s)));
    }
    return kk_fail(KK_EINVAL, "kk_g16x_plain: no kernel for tile %d, layout %d", cfg, lay);
}
int kk_g16x_headnorm(int cfg, const G16Args &a, hipStream_t s) {
#ifdef KK_TUNING_HOOKS
    if (cfg == G16X_128x192 && g16x_lw == 2) return launch_x<false, false, 128, 192, 3, 3, 4, 2, 4>(a, "kk_gemm_qkv_headnorm", s);
#endif
    if (cfg == G16X_128x192) return G16X_LW((launch_x<false, false, 128, 192, 3, 3, 2, 2, 4>(a, "kk_gemm_qkv_headnorm", s)), (launch_x<false, false, 128, 192, 3, 3, 4, 2, 0>(a, "kk_gemm_qkv_headnorm", s)));
    if (cfg == G16X_256x192) return launch_x<false, false, 256, 192, 2, 3, 4, 2, 0>(a, "kk_gemm_qkv_headnorm", s);
    if (cfg == G16X_128x128) return G16X_LW((launch_x<false, false, 128, 128, 3, 3, 2, 2, 4>(a, "kk_gemm_qkv_headnorm", s)), (launch_x<false, false, 128, 128, 3, 3, 4, 2, 0>(a, "kk_gemm_qkv_headnorm", s)));
    if (cfg == G16X_256x128) return G16X_LW((launch_x<false, false, 256, 128, 3, 3, 2, 2, 4>(a, "kk_gemm_qkv_headnorm", s)), (launch_x<false, false, 256, 128, 3, 3, 4, 2, 0>(a, "kk_gemm_qkv_headnorm", s)));
    return kk_fail(KK_EINVAL, "kk_g16x_headnorm: no kernel for tile %d", cfg);
}
int kk_g16x_glu_fwd(const G16Args &a0, hipStream_t s) {
    G16Args a = a0;
    a.tiles_n = kk_cdiv(a.N, 96);
#ifdef KK_TUNING_HOOKS
    if (g16x_lw == 2) {                                         // (tools: 128 rows x (96 + 96) columns, four compute waves of 32 x 192 + four loaders: 2 rounds at 4096 rows, slower)
        a.tiles_m = kk_cdiv(a.M, 128);
        return launch_x<false, false, 128, 192, 3, 2, 4, 1, 4>(a, "kk_gemm_linear_glu", s);
    }
#endif
    a.tiles_m = kk_cdiv(a.M, 256);
    // (eight compute waves of 32 x 192 + four loaders, 3 waves per SIMD at 166 registers, measured level: 24.2 against 25.3 us at 4096
    // rows, 51.9 against 50.6 at 8192 — the epilogue's 38 MB of stores is most of this launch; not instantiated)
    return launch_x<false, false, 256, 192, 2, 2, 8, 1, 0>(a, "kk_gemm_linear_glu", s);
}
int kk_g16x_glu_bwd(const G16Args &a, hipStream_t s) {
    return G16X_LW((launch_x<false, true, 128, 192, 3, 1, 2, 2, 4>(a, "kk_gemm_dgrad_glu", s)), (launch_x<false, true, 128, 192, 3, 1, 4, 2, 0>(a, "kk_gemm_dgrad_glu", s)));
}
int kk_g16x_group(const G16Group &g, int grid, hipStream_t s) {
#ifdef KK_TUNING_HOOKS
    kk_note_kernelf("g16x_group<1,1,128,128,3,lw%d>", g16x_lw);
    if (g16x_ns4) hipLaunchKernelGGL((g16x_group_kernel<true, true, 128, 128, 4, 2, 2, 4>), dim3(grid), dim3(512), 0, s, g);
    else if (g16x_lw == 2) hipLaunchKernelGGL((g16x_group_kernel<true, true, 128, 128, 3, 4, 2, 4>), dim3(grid), dim3(768), 0, s, g);
    else if (g16x_lw) hipLaunchKernelGGL((g16x_group_kernel<true, true, 128, 128, 3, 2, 2, 4>), dim3(grid), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((g16x_group_kernel<true, true, 128, 128, 3, 4, 2, 0>), dim3(grid), dim3(512), 0, s, g);
#else
    kk_note_kernel("g16x_group<1,1,128,128,3,lw1>");
    hipLaunchKernelGGL((g16x_group_kernel<true, true, 128, 128, 3, 2, 2, 4>), dim3(grid), dim3(512), 0, s, g);
#endif
    KK_LAUNCH_CHECK("kk_gemm_wgrad_group");
    return 0;
}
