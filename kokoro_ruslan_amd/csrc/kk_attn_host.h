// Attention, internal: the host side that kk_attn_fwd.hip and kk_attn_bwd.hip share, defined once in kk_attn.hip.
// Ordinary functions and variables of the library, not of its ABI: namespace kk_attn, hidden from the dynamic symbol table.  AttnArgs
// stays in the anonymous namespace (it is part of every kernel's name) and therefore never appears in a signature here: attn_args()
// and launch_attn() below, which do name it, are compiled into each unit on top of these.
#pragma once
#include "kk_attn.h"
#include <initializer_list>

#define KK_ATTN_LOCAL __attribute__((visibility("hidden")))
namespace kk_attn {
KK_ATTN_LOCAL extern int g_attn_groups;
KK_ATTN_LOCAL int attn_v2_mask();
KK_ATTN_LOCAL int attn_dbg();
KK_ATTN_LOCAL int attn_pair();
KK_ATTN_LOCAL bool attn_short_first();
KK_ATTN_LOCAL int g_attn_cus();
KK_ATTN_LOCAL int attn_xcd_map(int causal = 0);
KK_ATTN_LOCAL bool al16(const void *p);
KK_ATTN_LOCAL bool al16_all(std::initializer_list<const void *> ps);
KK_ATTN_LOCAL bool dma_storage(int io_bf16, int math, int v2_bits);
KK_ATTN_LOCAL bool dma_tiles(bool more_than_one, int Sq, int Sk);
KK_ATTN_LOCAL bool dma_hn_q(const KkAttnHeadNorm *hn);
KK_ATTN_LOCAL bool dma_hn_kv(const KkAttnHeadNorm *hn);
KK_ATTN_LOCAL bool dma_bytes(int S, int64_t ld0, int64_t ld1);
KK_ATTN_LOCAL bool dma_both(int io_bf16, int math, int Sq, int Sk, const void *Q, const void *K, const void *V, const void *dO, const void *dQ,
                            const void *dK, const void *dV, int64_t ldq, int64_t ldk, int64_t ldv, int64_t lddo, const KkAttnHeadNorm *hn_q,
                            const KkAttnHeadNorm *hn_kv);
KK_ATTN_LOCAL int attn_raise_lds(const void *kernel, size_t lds, const char *who);
KK_ATTN_LOCAL int check_common(const char *name, int B, int heads, int Sq, int Sk, int math, const int64_t *lds, int nld);
KK_ATTN_LOCAL int check_headnorm(const char *name, const KkAttnHeadNorm *hn, int n);
// (__thread, not thread_local: constant-initialised storage with no initialisation wrapper to call from another unit)
KK_ATTN_LOCAL extern __thread const void *g_warm_ptr[2];
KK_ATTN_LOCAL extern __thread uint32_t g_warm_bytes[2];
#ifdef KK_TUNING_HOOKS
KK_ATTN_LOCAL extern void *g_attn_trace;      // destination of the stamps of probe bits 256 / 4096 (kk_attn_trace)
#endif
}  // namespace kk_attn

namespace {

// What every launch of one attention has in common.  An entry point adds what is its own: outputs, dO / LSE / Delta, head-norm
// descriptors, keep, warm, dS, short_first.
AttnArgs attn_args(const float *Q, const float *K, const float *V, int B, int heads, int Sq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv,
                   const uint8_t *key_mask, int causal, float scale, const uint32_t *seed, uint32_t site, float p_drop) {
    AttnArgs a = {};
    a.Q = Q; a.K = K; a.V = V; a.key_mask = key_mask;
    a.B = B; a.heads = heads; a.Sq = Sq; a.Sk = Sk; a.causal = causal;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.scale = scale;
    a.seed = p_drop > 0.f ? seed : nullptr; a.site = site; a.p_drop = p_drop;
    a.xcd_map = kk_attn::attn_xcd_map(causal); a.dbg = kk_attn::attn_dbg(); a.wt = kk_write_through((int64_t)B * std::max(Sq, Sk));
    return a;
}

// Launch KERNEL<BF16, ST16, G> with G*256 threads and its dynamic LDS (buffers x groups x NT tiles).
template <typename K>
int launch_attn(K kernel, dim3 grid, int G, size_t lds, hipStream_t s, const AttnArgs &a) {
    if (int rc = kk_attn::attn_raise_lds((const void *)kernel, lds, "attention")) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256 * G), lds, s, a);
    return 0;
}
#define KK_ATTN_LDS(BF16, G, NT, EXTRA) ((size_t)2 * (G) * (NT) * 64 * ACfg<BF16>::LR * sizeof(typename ACfg<BF16>::elem) + (EXTRA))
#define KK_ATTN_LAUNCH_X(KERNEL, BF16, ST16, G, NT, EXTRA)                                                                         \
    do {                                                                                                                           \
        int rc__ = (G) == 2 ? launch_attn(KERNEL<BF16, ST16, 2>, grid, 2, KK_ATTN_LDS(BF16, 2, NT, EXTRA), (hipStream_t)stream, a) \
                            : launch_attn(KERNEL<BF16, ST16, 1>, grid, 1, KK_ATTN_LDS(BF16, 1, NT, EXTRA), (hipStream_t)stream, a); \
        if (rc__) return rc__;                                                                                                     \
    } while (0)
#define KK_ATTN_LAUNCH(KERNEL, BF16, ST16, G, NT) KK_ATTN_LAUNCH_X(KERNEL, BF16, ST16, G, NT, 0)

}  // namespace
