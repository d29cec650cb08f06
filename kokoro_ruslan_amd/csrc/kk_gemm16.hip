// bf16-storage MFMA GEMM core for gfx950: operands already bf16 in HBM, fp32 accumulate, LDS filled by the
// buffer-load-to-LDS DMA (16 bytes per lane, no VGPR staging, no ds_write pass).
//
// kk_gemm (kk_gemm.hip) routes to this core when both operands are stored as bf16 and the alignment rules below
// hold; it serves the same three Linear layouts (reference call sites listed at the top of kk_gemm.hip):
//   forward  Y = X.W^T        A k-contiguous, B k-contiguous
//   dgrad    dX = dY.W        A k-contiguous, B k-strided
//   wgrad    dW = dY^T.X      A k-strided,    B k-strided
//
// LDS images (BK = 64 reduction elements per stage, two stages):
//   k-contiguous operand: [rows][64] bf16, 128-byte rows, 16-byte chunk index XOR-ed with (row>>1)&7.  The DMA
//     writes LDS lane-linearly, so the XOR is applied to the GLOBAL source address (a permutation inside one
//     128-byte line: still fully coalesced); MFMA fragments are conflict-free ds_read_b128.
//   k-strided operand: [64 k][rows] bf16 exactly as it lies in memory (rows*2 bytes per k), 32-byte blocks XOR-ed
//     with a function of k; fragments (8 consecutive k per lane) come from two ds_read_b64_tr_b16 — the hardware
//     4x16 transpose read — so no software transpose exists anywhere.
// Out-of-range rows (tile edges, the K tail of a k-strided operand) are zero-filled by the buffer bounds check.
#include "kk_gemm16_body.h"
#include <algorithm>
#include <stdlib.h>

namespace {

// ---- policy: every knob of the host dispatch below, one instance ---------------------------------------------------------------
// Small tiles (by tile count): with four waves per workgroup the 64x64 tile wins on every shape of this model measured inside the
// train step (the launches are latency-bound: more, smaller workgroups keep more DMAs in flight); with EIGHT waves the 128x64 tile is
// level or better from 128 tiles on (the decoder's 4096-row GEMMs: +0.8 % on the 8x512 step, +2.2 % at 8x1024, interleaved A/B), so
// those take it and the encoder's 512-row GEMMs stay on 64x64.
// Split-K target: a small-tile launch with fewer than target / 2 tiles splits its reduction until it has ~target workgroups.  384 (fill
// the chip 1.5 x) was chosen stand-alone in round 1; INSIDE the step the launches it applies to are the side branch's (the text
// encoder's 512-row GEMMs), where more workgroups + a zero-fill launch + fp32 atomics per launch cost the critical chain beside them more
// than the shorter launch returns: 128 is -0.9 % on the 8 x 512 step (3.722 -> 3.690 ms interleaved), level at 8 x 1024
// (profiles/r05_splitk_target_ab.txt).
// Large tiles (kk_gemm16x.hip): a CU's L2 -> LDS stream runs at ~20 B/clk whatever a kernel does, so a launch's floor
// is the bytes that pass through its BUSIEST CU: rounds of workgroups x (BM + BN) x K x 2.  Every candidate tile is priced by that number
// (g16_cost, in units of K x 2 bytes) and the cheapest one runs; ties go to the small tile (more workgroups in flight, shorter
// prologue / epilogue).
// Set ONCE when the library is loaded: from KK_GEMM16_TUNE="thr128,thr12864,code" (code = flags*100000 + stages*10000 + split target, as
// tools/ encode it) and, in a tools build, from the KK_G16X* variables; afterwards only the tools hooks at the end of this section write it.
struct G16Policy {
    int thr128 = 4096, thr12864 = 128;                          // tiles from which 128x128 (four waves) / 128x64 (eight waves) run
    int split_target = 128, stages = 3, split_major = 0;
    int on = kk_tune_env("KK_G16X", 15);                        // large tiles: bit 0 plain, 1 head-norm, 2 GLU forward / backward, 3 grouped weight gradients
    int min_k_plain = kk_tune_env("KK_G16X_PLAIN_MIN_K", 1024);
    int min_k_group = kk_tune_env("KK_G16X_GROUP_MIN_K", 1024);
    int min_n_hn = kk_tune_env("KK_G16X_HN_MIN_N", 1024);
    int group_chunks = kk_tune_env("KK_G16X_GROUP_CHUNKS", 1);  // grouped launches: an XCD takes a contiguous eighth of ALL tiles (0: of every problem)
    int force = kk_tune_env("KK_G16X_FORCE", -1);               // tools: forced large tile (-1 = by cost)
    int dbg = kk_tune_env("KK_G16X_DBG", 0);                    // tools: probe bits of g16x_body (1 no epilogue, 4 no MFMAs, 8 DMA + barriers only)
    void small_tiles(int t128, int t12864, int code) {
        thr128 = t128;
        thr12864 = t12864;
        stages = (code / 10000) % 10 ? (code / 10000) % 10 : 3;
        split_major = code / 100000 ? 1 : 0;                    // 1xxxxx: split-major split-K (A/B comparison)
        split_target = code % 10000;
    }
    G16Policy() {
        const char *e = getenv("KK_GEMM16_TUNE");
        int a = 0, b = 0, c = 0;
        if (e && sscanf(e, "%d,%d,%d", &a, &b, &c) == 3 && a > 0) small_tiles(a, b, c);
    }
} g16;

int g16_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) return v;
        return 256;
    }();
    return n;
}
long g16_cost(int64_t tiles, int bm, int bn) { return (long)((tiles + g16_cus() - 1) / g16_cus()) * (bm + bn); }

// ---- the tile choice: one function, one row of data per route --------------------------------------------------------------------
struct G16Tile { int bm, bn; };                                 // (bn: columns of ONE B panel)
enum { FORCE_NONE, FORCE_CANDIDATE, FORCE_ANY };
struct G16Route {
    // small tiles
    bool thr128;                                                // 128x128 from policy.thr128 tiles on
    int w8_ktiles;                                              // eight waves on 128x64 from policy.thr12864 tiles and this many k-tiles on; 0: never, -1: always
    int ns;                                                     // stages of a reduction of >= 3 k-tiles (0: policy.stages)
    int panels;                                                 // B panels per workgroup (linear1 + GLU: 2, its tile's width counts twice)
    // large tiles
    int on_bit, min_ktiles;                                     // gate: this bit of policy.on, this many k-tiles ...
    bool min_k, min_n;                                          // ... K >= policy.min_k_plain, N >= policy.min_n_hn
    G16Tile base;                                               // the tile whose cost a candidate must beat ({0, 0}: the small tile that would run)
    int force;                                                  // policy.force: ignored | taken when it is a candidate | taken when >= 0
    int ncand, cand[G16X_NCFG];                                 // candidates, in order (the first of equal cost wins)
};
const G16Route R_PLAIN    = {true,  1, 0, 1,   1, 0, true,  false, {0, 0},    FORCE_CANDIDATE, 2, {G16X_128x128, G16X_256x128}};
const G16Route R_DELTA    = {false, -1, 0, 1,  1, 0, true,  false, {0, 0},    FORCE_NONE,      1, {G16X_128x128}};
const G16Route R_GLU_BWD  = {false, 3, 3, 1,   4, 3, false, false, {128, 64}, FORCE_NONE,      1, {G16X_128x192}};      // (priced against 128x64 whether or not it would run)
const G16Route R_GLU_FWD  = {false, 0, 2, 2,   4, 3, false, false, {64, 64},  FORCE_NONE,      1, {G16X_256x192}};      // 256 rows x (96 + 96) columns against 64 x (64 + 64)
const G16Route R_HEADNORM = {false, 3, 3, 1,   2, 3, false, true,  {0, 0},    FORCE_ANY,       4, {G16X_128x128, G16X_128x192, G16X_256x128, G16X_256x192}};

struct G16Choice {
    int cfg;                                                    // large-tile family: its tile; -1: the small-tile family
    G16Tile tile;
    int waves;
};
// `large_ok`: what the caller alone knows about the large tiles' gate (one k-slice, the operand layout, the alignment of the epilogue's stores)
G16Choice g16_choose(const G16Route &r, int64_t M, int64_t N, int64_t K, bool large_ok) {
    const int ktiles = kk_cdiv(K, BK);
    auto tiles = [&](G16Tile t) { return (int64_t)kk_cdiv(M, t.bm) * kk_cdiv(N, t.bn); };
    auto cost = [&](G16Tile t) { return g16_cost(tiles(t), t.bm, t.bn * r.panels); };
    G16Choice c = {-1, {64, 64}, 4};
    if (r.thr128 && tiles({128, 128}) >= g16.thr128) c.tile = {128, 128};
    else if (r.w8_ktiles < 0 || (r.w8_ktiles > 0 && ktiles >= r.w8_ktiles && tiles({128, 64}) >= g16.thr12864)) c = {-1, {128, 64}, 8};
    if (!large_ok || !(g16.on & r.on_bit) || ktiles < r.min_ktiles || (r.min_k && K < g16.min_k_plain) || (r.min_n && N < g16.min_n_hn)) return c;
    auto large = [&](int cfg) { G16Tile t; kk_g16x_tile(cfg, &t.bm, &t.bn); t.bn /= r.panels; return t; };
    int best = -1;
    long best_cost = cost(r.base.bm ? r.base : c.tile);
    for (int i = 0; i < r.ncand; ++i) {
        const long cc = cost(large(r.cand[i]));
        if (cc < best_cost) { best = r.cand[i]; best_cost = cc; }
    }
    if (r.force == FORCE_ANY && g16.force >= 0) best = g16.force;
    if (r.force == FORCE_CANDIDATE && std::find(r.cand, r.cand + r.ncand, g16.force) != r.cand + r.ncand) best = g16.force;
    if (best >= 0) c = {best, large(best), 8};
    return c;
}
// LDS stages of a small-tile launch whose k-slices hold `ktiles` k-tiles (a short reduction gains nothing from depth)
int g16_ns(const G16Route &r, const G16Choice &c, int ktiles) {
    if (c.tile.bn == 128 || ktiles < 3) return 2;
    return std::min(std::max(r.ns ? r.ns : g16.stages, 2), c.waves == 8 ? 3 : 4);
}

// ---- split-K -------------------------------------------------------------------------------------------------------------------
struct G16Split { int splits, k_per_split, split_major; };
G16Split g16_split_plain(int tiles, int ktiles, int64_t N, int64_t K, float beta, int64_t ldc, int c_bf16, int split_k) {
    int splits = split_k;
    if (splits <= 0) {
        splits = 1;
        if (tiles * 2 <= g16.split_target) {
            splits = kk_cdiv(g16.split_target, tiles);
            const int cap = ktiles / 2 > 0 ? ktiles / 2 : 1;
            if (splits > cap) splits = cap;
        }
    }
    // beta == 0 with k-slices needs C zero-filled first: one more node in front of a GEMM that is latency-bound anyway
    // (the encoder's 1000-row projections), so short reductions are not sliced then
    // (+1 % on the train step)
    if (split_k <= 0 && beta == 0.f && ktiles < 32) splits = 1;
    if (splits > ktiles) splits = ktiles;
    if (splits > 1 && (c_bf16 || !(beta == 1.f || (beta == 0.f && ldc == N)))) splits = 1;
    if (split_k <= 0 && splits >= 6 && g16.split_major) {       // a multiple of 8 slices: one XCD per slice residue class
        int s8 = ((splits + 4) / 8) * 8;
        while (s8 > 8 && ktiles / s8 < 2) s8 -= 8;
        if (ktiles / s8 >= 1) splits = s8;
    }
    int k_per_split = kk_cdiv(ktiles, splits) * BK;
    splits = kk_cdiv(K, k_per_split);
    const int split_major = (g16.split_major && splits > 1 && splits % 8 == 0) ? 1 : 0;
    return {splits, k_per_split, split_major};
}
// grouped launch: the k-slices that `splits` asks for leave problem i (reduction T) with `sp` slices of `kps`
G16Split g16_split_group(int64_t T, int splits) {
    const int ktiles = kk_cdiv(T, BK);
    int sp = std::min(splits, std::max(ktiles / 2, 1));
    const int kps = kk_cdiv(ktiles, sp) * BK;
    sp = kk_cdiv(T, kps);
    return {sp, kps, 0};
}

// ---- kernels: explicit instantiations of exactly what the launch helpers and entry points below name -----------------------------
template <bool TA, bool TB, int BM, int BN, int NS, int EPI = 0>
__global__ __launch_bounds__(256) void gemm16_kernel(G16Args a) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (BM + (EPI == 2 ? 2 : 1) * BN) * BK * 2];
    gemm16_body<TA, TB, BM, BN, NS, EPI>(a, blockIdx.x, smem);
}
// The same body run by EIGHT waves on the 128x64 tile (a 4x2 wave grid, one 32x32 MFMA chain per wave): twice the waves per
// byte of LDS, which is what these latency-bound launches respond to (see the grouped weight gradients below).
template <bool TA, bool TB, int NS>
__global__ __launch_bounds__(512) void gemm16_kernel_w8(G16Args a) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (128 + 64) * BK * 2];
    gemm16_body<TA, TB, 128, 64, NS, 0, 8, 2>(a, blockIdx.x, smem);
}
// ... with the GLU backward epilogue (linear2 dgrad + gate backward: +0.3 % on the step) ...
template <bool TB, int NS, int EPI>
__global__ __launch_bounds__(512) void gemm16_kernel_w8_glu(G16Args a) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (128 + (EPI == 2 ? 2 : 1) * 64) * BK * 2];
    gemm16_body<false, TB, 128, 64, NS, EPI, 8, 2>(a, blockIdx.x, smem);
}
// ... and with the head-norm epilogue (+0.8 % on the step)
template <int NS>
__global__ __launch_bounds__(512) void gemm16_kernel_w8_hn(G16Args a) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (128 + 64) * BK * 2];
    gemm16_body<false, false, 128, 64, NS, 3, 8, 2>(a, blockIdx.x, smem);
}
// Several independent GEMMs of one operand layout in ONE launch (a layer's weight gradients: they have no consumer
// before the optimizer, so they wait until the layer's backward is through and then fill the chip together: full reduction
// lengths, no split-K atomics, one launch instead of four to six).  Eight waves on 128x64 tiles: +1 % on the step over 64x64.
template <bool TA, bool TB, int BM, int BN, int NS, int WAVES = 4, int WC = 2>
__global__ __launch_bounds__(64 * WAVES) void gemm16_group_kernel(G16Group g) {
    __shared__ __attribute__((aligned(16))) char smem[NS * (BM + BN) * BK * 2];
    int i = 0;
    while (i + 1 < g.n && (int)blockIdx.x >= g.start[i + 1]) ++i;
    gemm16_body<TA, TB, BM, BN, NS, 0, WAVES, WC>(g.p[i], (int)blockIdx.x - g.start[i], smem);
}
// (explicit, in this order: the host stubs of kernels only named inside an if/else chain of a launch helper were not emitted, and the
// compiler's register allocation of a kernel is not independent of the instantiations before it)
#define G16_LAYOUTS(K, ...) \
    template __global__ void K<false, false, __VA_ARGS__>(G16Args); template __global__ void K<false, true, __VA_ARGS__>(G16Args); \
    template __global__ void K<true, false, __VA_ARGS__>(G16Args);  template __global__ void K<true, true, __VA_ARGS__>(G16Args);
G16_LAYOUTS(gemm16_kernel_w8, 2)
G16_LAYOUTS(gemm16_kernel_w8, 3)
template __global__ void gemm16_kernel_w8_hn<3>(G16Args);
template __global__ void gemm16_kernel_w8_glu<true, 3, 1>(G16Args);
template __global__ void gemm16_group_kernel<true, true, 128, 64, 2, 8>(G16Group);
G16_LAYOUTS(gemm16_kernel, 128, 128, 2)
G16_LAYOUTS(gemm16_kernel, 64, 64, 2)
G16_LAYOUTS(gemm16_kernel, 64, 64, 3)
G16_LAYOUTS(gemm16_kernel, 64, 64, 4)
#undef G16_LAYOUTS
template __global__ void gemm16_kernel<false, false, 64, 64, 2, 2>(G16Args);
template __global__ void gemm16_kernel<false, false, 64, 64, 2, 3>(G16Args);
template __global__ void gemm16_kernel<false, false, 64, 64, 3, 3>(G16Args);
template __global__ void gemm16_kernel<false, true, 64, 64, 2, 1>(G16Args);
template __global__ void gemm16_kernel<false, true, 64, 64, 3, 1>(G16Args);

template <int BM, int BN, int NS>
void launch_tile(int ta, int tb, const G16Args &a, dim3 grid, hipStream_t s) {
    kk_note_kernelf("gemm16<%d,%d,%d,%d,%d>", ta, tb, BM, BN, NS);
    if (!ta && !tb) hipLaunchKernelGGL((gemm16_kernel<false, false, BM, BN, NS>), grid, dim3(256), 0, s, a);
    else if (!ta && tb) hipLaunchKernelGGL((gemm16_kernel<false, true, BM, BN, NS>), grid, dim3(256), 0, s, a);
    else if (ta && !tb) hipLaunchKernelGGL((gemm16_kernel<true, false, BM, BN, NS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gemm16_kernel<true, true, BM, BN, NS>), grid, dim3(256), 0, s, a);
}
template <int NS>
void launch_w8(int ta, int tb, const G16Args &a, dim3 grid, hipStream_t s) {
    kk_note_kernelf("gemm16_w8<%d,%d,%d>", ta, tb, NS);
    if (kk_capture(kk_last_kernel(), a, grid, 512, 0)) return;
    if (!ta && !tb) hipLaunchKernelGGL((gemm16_kernel_w8<false, false, NS>), grid, dim3(512), 0, s, a);
    else if (!ta && tb) hipLaunchKernelGGL((gemm16_kernel_w8<false, true, NS>), grid, dim3(512), 0, s, a);
    else if (ta && !tb) hipLaunchKernelGGL((gemm16_kernel_w8<true, false, NS>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((gemm16_kernel_w8<true, true, NS>), grid, dim3(512), 0, s, a);
}

// C[M, N] = A.B over the whole reduction K in one k-slice, on BM x BN tiles: what every launch derives the same way (alpha = 1, beta = 0,
// fp32 C; write-through by the launch length: a weight gradient's — ta — is its reduction).  The entry points add their epilogue's fields.
G16Args g16_args(int ta, int tb, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc,
                 int BM, int BN, int xcd_swizzle) {
    G16Args a = {};
    a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.wt = kk_write_through(ta ? K : M);
    a.alpha = 1.f; a.A = A; a.B = B; a.C = C; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.k_per_split = kk_cdiv(K, BK) * BK; a.splits = 1;
    a.tiles_m = kk_cdiv(M, BM); a.tiles_n = kk_cdiv(N, BN); a.xcd_swizzle = xcd_swizzle;
    a.a_bytes = (uint32_t)(((ta ? (K - 1) * lda + M : (M - 1) * lda + K)) * 2);
    a.b_bytes = (uint32_t)(((tb ? (K - 1) * ldb + N : (N - 1) * ldb + K)) * 2);
    return a;
}

// ss_rec / ss_seg of a grouped launch: when every problem is written exactly once per element by one workgroup (no k-slices; the
// conditions of the write-through fp32 epilogue, which both bodies have; a tile inside ONE segment), its tiles leave the sums of squares of
// what they stored as records [*ss_count ..) of ss_rec and *ss_count is advanced; otherwise *ss_count stays and the caller's norm pass
// reads those tensors itself
void g16_group_ss(G16Group &g, KkSegRec *rec, const int32_t *ss_seg, int32_t *ss_count) {
    bool all_wt = rec != nullptr && ss_seg != nullptr && ss_count != nullptr;
    for (int i = 0; i < g.n && all_wt; ++i)
        all_wt = (ss_seg[2 * i + 1] == 0 || ss_seg[2 * i + 1] % 128 == 0) && g.p[i].splits == 1 && g.p[i].wt && (g.p[i].ldc & 3) == 0 && (g.p[i].N & 7) == 0 && (reinterpret_cast<uintptr_t>(g.p[i].C) & 15) == 0;
    if (!all_wt) return;
    for (int i = 0; i < g.n; ++i) {
        g.p[i].ss_rec = rec + *ss_count + g.start[i];
        g.p[i].ss_seg = ss_seg[2 * i];
        g.p[i].ss_rows = ss_seg[2 * i + 1];
    }
    *ss_count += g.start[g.n];
}

}  // namespace

#ifdef KK_TUNING_HOOKS
// Tuning hooks used by tools/ (not part of the C ABI): the small tiles' thresholds; the large-tile family's on/off bits, forced tile
// (-1 = by cost) and probe bits
void kk_gemm16_tune(int thr128, int thr12864, int split_target) { g16.small_tiles(thr128, thr12864, split_target); }
extern int g16x_lw;
extern "C" int kk_gemm_tune16x(int on, int force, int dbg) { g16.on = on & 255; g16x_lw = (on >> 8) & 1 ? 0 : ((on >> 9) & 1 ? 2 : 1); g16.group_chunks = (on >> 10) & 1 ? 0 : 1; g16.force = force; g16.dbg = dbg; return 0; }
void kk_g16x_probe(int bits, void *buf);
extern "C" int kk_gemm_trace16x(void *buf) { kk_g16x_probe(g16.dbg, buf); return 0; }      // probe bit 32: 8 waves x 64 stamps (uint64) of workgroup 0
#endif

// True when this core can run the problem (both operands bf16 assumed by the caller).
bool kk_gemm16_eligible(int ta, int tb, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B, int64_t ldb) {
    if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || lda % 8 || ldb % 8) return false;
    if ((!ta || !tb) && K % BK) return false;                 // a k-contiguous operand has no zero-filled K tail
    const int64_t a_el = ta ? (K - 1) * lda + M : (M - 1) * lda + K, b_el = tb ? (K - 1) * ldb + N : (N - 1) * ldb + K;
    return a_el * 2 < (1ll << 31) && b_el * 2 < (1ll << 31);
}

int kk_gemm16_launch(int ta, int tb, int64_t M, int64_t N, int64_t K, float alpha, const void *A, int64_t lda, const void *B,
                     int64_t ldb, float beta, void *C, int64_t ldc, int c_bf16, const float *bias, const float *residual,
                     int64_t ldr, int64_t res_mod, int split_k, int xcd_swizzle, hipStream_t s) {
    const G16Tile t = g16_choose(R_PLAIN, M, N, K, false).tile;      // (the k-slices are counted for the small tile)
    const int ktiles = kk_cdiv(K, BK);
    const G16Split sp = g16_split_plain(kk_cdiv(M, t.bm) * kk_cdiv(N, t.bn), ktiles, N, K, beta, ldc, c_bf16, split_k);
    // (long reductions only: at K = 512 a one-workgroup-per-CU launch shows its whole prologue and epilogue, two 128x64 workgroups per CU
    // hide each other's — measured 9.5 against 10.3 us at 8192 x 512 x 512, 46 against 37 us at K = 3072; weight-gradient layouts: grouped launches only)
    const G16Choice c = g16_choose(R_PLAIN, M, N, K, sp.splits == 1 && !ta);
    G16Args a = g16_args(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, c.tile.bm, c.tile.bn, xcd_swizzle);
    a.alpha = alpha; a.beta = beta; a.bias = bias; a.residual = residual; a.c_bf16 = c_bf16; a.ldr = ldr; a.res_mod = res_mod;
    a.k_per_split = sp.k_per_split; a.atomic = sp.splits > 1 ? 1 : 0; a.splits = sp.splits; a.split_major = sp.split_major;
    if (c.cfg >= 0) {
        a.dbg = g16.dbg;
        return kk_g16x_plain(c.cfg, ta, tb, a, s);
    }
    if (sp.splits > 1 && beta == 0.f) {
        const int e = kk_zero_async(C, (size_t)M * N * sizeof(float), s);
        if (e != 0) return e;
    }
    dim3 grid(a.tiles_m * a.tiles_n * sp.splits);
    const int ns = g16_ns(R_PLAIN, c, ktiles / sp.splits);
    if (c.tile.bn == 128) launch_tile<128, 128, 2>(ta, tb, a, grid, s);
    else if (c.waves == 8) { if (ns == 3) launch_w8<3>(ta, tb, a, grid, s); else launch_w8<2>(ta, tb, a, grid, s); }
    else if (ns == 4) launch_tile<64, 64, 4>(ta, tb, a, grid, s);
    else if (ns == 3) launch_tile<64, 64, 3>(ta, tb, a, grid, s);
    else launch_tile<64, 64, 2>(ta, tb, a, grid, s);
    KK_LAUNCH_CHECK("kk_gemm");
    return 0;
}

// dX[M, N] = dY[M, K] . W[K, N] (bf16 everywhere) with Delta[b, head, q] = sum_d dX * O as the epilogue: the dgrad of an attention
// output projection on the eight-wave 128x64 tile (a tile's 64 columns = one head).  `supported`: the shapes the epilogue is written
// for.  The decoder's 4096-row launches take that tile anyway; the text encoder's 512-row ones (32 tiles, a 64x64 launch otherwise)
// take it FOR the epilogue: Delta is what lets the attention backward run as one launch (kk_attn_bwd).
bool kk_gemm16_dgrad_delta_supported(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && N % 64 == 0 && K % BK == 0 && kk_cdiv(M, 128) * kk_cdiv(N, 128) < g16.thr128;
}
int kk_gemm16_dgrad_delta(int64_t M, int64_t N, int64_t K, const void *dy, int64_t lddy, const void *W, int64_t ldw, void *dx,
                          int64_t lddx, const void *O, int64_t ldo, float *delta, int S, int heads, int xcd_swizzle, hipStream_t s) {
    const G16Choice c = g16_choose(R_DELTA, M, N, K, true);
    G16Args a = g16_args(0, 1, M, N, K, dy, lddy, W, ldw, dx, lddx, c.tile.bm, c.tile.bn, xcd_swizzle);
    a.c_bf16 = 1;
    a.dl_o = static_cast<const __bf16 *>(O); a.dl_out = delta; a.dl_ldo = ldo; a.dl_S = S; a.dl_heads = heads;
    if (c.cfg >= 0) return kk_g16x_plain(c.cfg, 0, 1, a, s);
    dim3 grid(a.tiles_m * a.tiles_n);
    if (g16_ns(R_DELTA, c, kk_cdiv(K, BK)) == 3) launch_w8<3>(0, 1, a, grid, s);
    else launch_w8<2>(0, 1, a, grid, s);
    KK_LAUNCH_CHECK("kk_gemm_dgrad_delta");
    return 0;
}

int kk_gemm16_dgrad_glu(int64_t T, int64_t F, int64_t H, const void *dy, int64_t lddy, const void *W, const void *h1, void *dh1,
                        float *partials, const uint32_t *seed, uint32_t site, float p, int xcd_swizzle, hipStream_t s) {
    const G16Choice c = g16_choose(R_GLU_BWD, T, F, H, true);
    G16Args a = g16_args(0, 1, T, F, H, dy, lddy, W, F, nullptr, 0, c.tile.bm, c.tile.bn, xcd_swizzle);      // (C is not written: the epilogue stores dh1)
    a.glu_h = static_cast<const __bf16 *>(h1); a.glu_dh = static_cast<__bf16 *>(dh1); a.glu_partials = partials;
    a.glu_seed = p > 0.f ? seed : nullptr; a.glu_site = site; a.glu_p = p;
    if (c.cfg >= 0) return kk_g16x_glu_bwd(a, s);
    dim3 grid(a.tiles_m * a.tiles_n);
    if (c.waves == 8) {                                         // eight waves on 128x64 tiles, like the plain GEMMs
        kk_note_kernel("gemm16_w8_glu<1,3,1>");
        hipLaunchKernelGGL((gemm16_kernel_w8_glu<true, 3, 1>), grid, dim3(512), 0, s, a);
    } else {
        kk_note_kernel("gemm16<0,1,64,64,*,1>");
        if (g16_ns(R_GLU_BWD, c, kk_cdiv(H, BK)) == 2) hipLaunchKernelGGL((gemm16_kernel<false, true, 64, 64, 2, 1>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gemm16_kernel<false, true, 64, 64, 3, 1>), grid, dim3(256), 0, s, a);
    }
    KK_LAUNCH_CHECK("kk_gemm_dgrad_glu");
    return 0;
}

int kk_gemm16_linear_glu(int64_t T, int64_t F, int64_t K, const void *x, int64_t ldx, const void *W, const float *bias, void *h1,
                         void *g, int64_t ldg, const uint32_t *seed, uint32_t site, float p, int xcd_swizzle, hipStream_t s) {
    const G16Choice c = g16_choose(R_GLU_FWD, T, F, K, true);
    G16Args a = g16_args(0, 0, T, F, K, x, ldx, W, K, g, ldg, c.tile.bm, c.tile.bn, xcd_swizzle);      // N = F: a workgroup covers columns n and F + n of the [T, 2F] product
    a.bias = bias; a.c_bf16 = 1;
    a.b_bytes = (uint32_t)(((2 * F - 1) * K + K) * 2);     // (both panels of W1)
    a.glu_dh = static_cast<__bf16 *>(h1);
    a.glu_seed = p > 0.f ? seed : nullptr; a.glu_site = site; a.glu_p = p;
    if (c.cfg >= 0) return kk_g16x_glu_fwd(a, s);
    kk_note_kernel("gemm16<0,0,64,64,2,2>");
    hipLaunchKernelGGL((gemm16_kernel<false, false, 64, 64, 2, 2>), dim3(a.tiles_m * a.tiles_n), dim3(256), 0, s, a);
    KK_LAUNCH_CHECK("kk_gemm_linear_glu");
    return 0;
}

int kk_gemm16_qkv_headnorm(int64_t T, int parts, int heads, int64_t K, const void *x, int64_t ldx, const void *W, const float *bias,
                           void *raw, int64_t ldraw, void *y, int64_t ldy, int S, const float *const *gains, int rope_mask,
                           const float *cos_t, const float *sin_t, int xcd_swizzle, hipStream_t s) {
    const int64_t N = (int64_t)parts * heads * 64;
    const bool stores16 = ldraw % 8 == 0 && ldy % 8 == 0 && (((uintptr_t)raw | (uintptr_t)y) & 15) == 0;      // (the large tiles' 16-byte stores)
    const G16Choice c = g16_choose(R_HEADNORM, T, N, K, stores16);
    G16Args a = g16_args(0, 0, T, N, K, x, ldx, W, K, raw, ldraw, c.tile.bm, c.tile.bn, xcd_swizzle);
    a.bias = bias; a.c_bf16 = 1;
    for (int i = 0; i < parts; ++i) a.hn_gain[i] = gains[i];
    a.hn_cos = cos_t; a.hn_sin = sin_t; a.hn_y = static_cast<__bf16 *>(y); a.hn_ldy = ldy;
    a.hn_S = S; a.hn_H = heads * 64; a.hn_rope_mask = rope_mask;
    if (c.cfg >= 0) {
        a.dbg = g16.dbg;
        return kk_g16x_headnorm(c.cfg, a, s);
    }
    dim3 grid(a.tiles_m * a.tiles_n);
    if (c.waves == 8) {                                         // eight waves on 128x64 tiles, like the plain GEMMs
        kk_note_kernel("gemm16_w8_hn<3>");
        hipLaunchKernelGGL((gemm16_kernel_w8_hn<3>), grid, dim3(512), 0, s, a);
    } else {
        kk_note_kernel("gemm16<0,0,64,64,*,3>");
        if (g16_ns(R_HEADNORM, c, kk_cdiv(K, BK)) == 2) hipLaunchKernelGGL((gemm16_kernel<false, false, 64, 64, 2, 3>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gemm16_kernel<false, false, 64, 64, 3, 3>), grid, dim3(256), 0, s, a);
    }
    KK_LAUNCH_CHECK("kk_gemm_qkv_headnorm");
    return 0;
}

// dW_i[M_i, N_i] += dY_i[T_i, M_i]^T . X_i[T_i, N_i] for i < n, one launch (see gemm16_group_kernel): eight waves on 128x64 tiles, or
// the large-tile family's 128x128 — full reductions only, long ones (short launches sit on the side branch, where a 96 KB workgroup
// keeps the main chain's workgroups waiting)
int kk_gemm16_wgrad_group(const KkWgradDesc *d, int n, int split_k, int overwrite, int xcd_swizzle, hipStream_t s, void *ss_rec,
                          const int32_t *ss_seg, int32_t *ss_count) {
    if (n < 1 || n > GROUP_MAX) return kk_fail(KK_EINVAL, "kk_gemm_wgrad_group: 1..%d problems per launch, got %d", GROUP_MAX, n);
    int total = 0, total_x = 0;
    int64_t kmin = 1ll << 40;
    for (int i = 0; i < n; ++i) {
        if (d[i].M <= 0 || d[i].N <= 0 || d[i].T <= 0 || !d[i].dy || !d[i].x || !d[i].dw)
            return kk_fail(KK_EINVAL, "kk_gemm_wgrad_group: bad problem %d", i);
        if (!kk_gemm16_eligible(1, 1, d[i].M, d[i].N, d[i].T, d[i].dy, d[i].lddy, d[i].x, d[i].ldx))
            return kk_fail(KK_EINVAL, "kk_gemm_wgrad_group: problem %d needs 16-byte aligned bf16 operands with row strides %% 8 == 0", i);
        total += kk_cdiv(d[i].M, 128) * kk_cdiv(d[i].N, 64);
        total_x += kk_cdiv(d[i].M, 128) * kk_cdiv(d[i].N, 128);
        kmin = std::min<int64_t>(kmin, d[i].T);
    }
    const bool by_target = total * 2 <= g16.split_target;      // (k-slices accumulate with atomics: they need the old value, so never with overwrite)
    const bool sliced = split_k > 1 || (split_k <= 0 && !overwrite && by_target);
    const bool large = (g16.on & 8) && !sliced && kmin >= g16.min_k_group && g16_cost(total_x, 128, 128) < g16_cost(total, 128, 64);
    const int splits = overwrite ? 1 : split_k > 0 ? split_k : by_target ? kk_cdiv(g16.split_target, total) : 1;      // the caller's k-slice count (0 = by the split target)
    G16Group g = {};
    g.n = n;
    g.xcd_chunks = (large && xcd_swizzle && g16.group_chunks) ? 1 : 0;
    for (int i = 0; i < n; ++i) {
        const G16Split sp = g16_split_group(d[i].T, splits);
        G16Args &a = g.p[i];
        a = g16_args(1, 1, d[i].M, d[i].N, d[i].T, d[i].dy, d[i].lddy, d[i].x, d[i].ldx, d[i].dw, d[i].lddw, 128, large ? 128 : 64, g.xcd_chunks ? 0 : xcd_swizzle);
        a.beta = overwrite ? 0.f : 1.f;
        a.k_per_split = sp.k_per_split; a.splits = sp.splits; a.atomic = sp.splits > 1 ? 1 : 0;
        a.m_fast = (xcd_swizzle && d[i].M < d[i].N) ? 1 : 0;    // sweep direction by operand size
        if (large) a.dbg = g16.dbg;
        g.start[i + 1] = g.start[i] + a.tiles_m * a.tiles_n * sp.splits;
    }
    g16_group_ss(g, static_cast<KkSegRec *>(ss_rec), ss_seg, ss_count);
    if (large) return kk_g16x_group(g, g.start[n], s);
    kk_note_kernel("gemm16_group<128,64,w8>");
    hipLaunchKernelGGL((gemm16_group_kernel<true, true, 128, 64, 2, 8>), dim3(g.start[n]), dim3(512), 0, s, g);
    KK_LAUNCH_CHECK("kk_gemm_wgrad_group");
    return 0;
}
