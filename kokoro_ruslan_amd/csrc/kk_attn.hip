// Fused (flash-style) multi-head attention, forward and backward, head_dim 64, for gfx950.
//
// Replaces F.scaled_dot_product_attention(Q,K,V, attn_mask=additive -inf bias) and its autograd backward
// (reference model/transformers.py:393-398; masks built at :299-316; causal mask model/model.py:434-437).
// The reference's SDPA math path materialises [B,h,Sq,Sk] scores/probabilities (268 MB per tensor at 8x1024);
// here nothing of size Sq x Sk ever leaves the CU.
//
// Work decomposition: one 256-thread workgroup per (batch, head, 128-row block); each of its 4 waves owns
// 32 rows.  K/V (or Q/dO in the dK/dV kernel) stream through LDS in 64-row tiles shared by the 4 waves.
//
// MFMA orientation ("swapped QK^T"): scores are computed TRANSPOSED, S^T[key][q] = K.Q^T, with the 32x32
// MFMA (C/D map: col = lane&31, row = (r&3)+8(r>>2)+4(lane>>5)).  A lane then owns one query column and 16 of
// the 32 keys of a sub-tile, so the softmax row reduction is 16 in-lane operations + one lane^32 exchange,
// and the probabilities are already laid out as the B operand of the second MFMA (O^T[d][q] = V^T.P^T) with
// no cross-lane traffic: the k-slots of that MFMA are bound to keys in the order the accumulator registers
// hold them, and the A operand (V^T) is read from a transposed LDS tile in that same order.
//
// KK_MATH_F32 runs the identical structure on v_mfma_f32_32x32x2_f32 (exact fp32) — the parity mode;
// KK_MATH_BF16 rounds Q/K/V/P/dS/dO to bf16 for the MFMAs and keeps scores, softmax and accumulators in fp32.
//
// Where things are.  kk_attn.h: the device code more than one kernel family uses; kk_attn_host.h: the declarations of what this file defines;
// kk_attn_fwd3.h: the third-generation forward body (also a phase of kk_chain.hip); kk_attn_fwd.hip / kk_attn_bwd.hip: the forward /
// backward kernels with their entry points.  This file is the host side the two share: the switches, the eligibility predicates of
// the dispatch, the argument checks and the per-thread state.  Everything here has ONE definition, reached by both units (a switch
// is read once, the raised-LDS table and the warm request exist once per thread); nothing here is exported (namespace kk_attn, KK_ATTN_LOCAL).
#include "kk_attn_host.h"

namespace kk_attn {

int g_attn_groups = 2;
int attn_v2_mask() {              // bit 0: forward, bit 1: dQ, bit 2: dK/dV DMA-staged kernels (second generation and later)
    static const int v = kk_tune_env("KK_ATTN_V2", 7);
    return v;
}
#ifdef KK_TUNING_HOOKS
void *g_attn_trace = nullptr;
extern "C" int kk_attn_trace(void *buf) { g_attn_trace = buf; return 0; }      // tools: destination of the stamps of probe bit 256
#endif
int attn_dbg() {                  // timing probes of tools/probes (tools build only: results are wrong when set)
    static const int v = kk_tune_env("KK_ATTN_DBG", 0);
    return v;
}
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// The second-generation BACKWARD kernels also take sequences of ONE 64-row tile (33..64 queries and keys: the text encoder): wave
// group 1 then has no tile and only joins the barriers and the merge, but the DMA prologue, the LDS-transposed epilogues and the
// one-launch form (kk_attn_bwd) beat the first generation's 13 + 17 us there (KK_ATTN_V2_SMALL=0 in the tools build: old dispatch)
static bool attn_v2_small(int Sq, int Sk) {
    static const int v = kk_tune_env("KK_ATTN_V2_SMALL", 1);
    return v != 0 && Sq > 32 && Sk > 32;
}
int attn_pair() {                 // KK_ATTN_PAIR=0: kk_attn_bwd issues the dQ and the dK/dV kernel as two launches
    static const int v = kk_tune_env("KK_ATTN_PAIR", 1);
    return v;
}
// KK_ATTN_BWD3 (tools) bit 1: the dK/dV half of a causal pair launch hands out its short blocks first (default).  Bit 0 is ignored.
bool attn_short_first() {
    static const int v = kk_tune_env("KK_ATTN_BWD3", 3);
    return (v & 2) != 0;
}
int g_attn_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) return v;
        return 256;
    }();
    return n;
}
static int attn_xcd_env() {
    static const int v = kk_tune_env("KK_ATTN_XCD", 2);
    return v;
}
// AttnArgs::xcd_map of a launch: 0 = launch order, 1 = a head's blocks on one XCD, 2 (default for causal launches) = that, with the
// blocks of an XCD's heads longest first (attn_block).  KK_ATTN_XCD=1 keeps 1 for the single-kernel causal launches.
int attn_xcd_map(int causal) {
    const int v = attn_xcd_env();
    return v == 2 ? (causal ? 2 : 1) : v;
}

// Which backward launches take the DMA-staged bf16 kernels (dq2 / dq3, dkv3, pair3 / pair3k, dkv3s + dqpass); everything else runs the
// first-generation templates.  One row per route, one column per condition; "-" = the route does not ask.
//
//                  KK_ATTN_V2  more than one 64-row  Sk <=  16-byte aligned   head-norm    32-bit byte     the route's own
//                  bits        tile of ...           4096                     descriptors  offsets of
//   kk_attn_bwd_dq      2      keys, or small        yes    Q K V dO dQ (O)   q            K / V           -
//   kk_attn_bwd_dkv     4      queries, or small     -      Q K V dO dK dV    kv           Q / dO          -
//   kk_attn_bwd (pair)  2 | 4  both, or small        yes    all seven         q and kv     both            KK_ATTN_PAIR, cdiv(Sq, 128) == cdiv(Sk, 128)
//   kk_attn_bwd_ws      2 | 4  both (small: no)      yes    all seven         q and kv     both            workspace, !causal || Sq == Sk
//
// All four: bf16 storage with bf16 math, g_attn_groups == 2.  "small" = attn_v2_small (33..64 rows: one tile, second wave group idle).
// The dK/dV kernels address K, V and their outputs block by block through 64-bit pointers and loop over queries, which is why that
// route alone has no Sk cap and bounds Q / dO instead.
bool dma_storage(int io_bf16, int math, int v2_bits) { return io_bf16 && math == KK_MATH_BF16 && (attn_v2_mask() & v2_bits) == v2_bits; }
bool dma_tiles(bool more_than_one, int Sq, int Sk) { return g_attn_groups == 2 && (more_than_one || attn_v2_small(Sq, Sk)); }
bool al16_all(std::initializer_list<const void *> ps) {              // (a null pointer counts as aligned: the optional O)
    for (const void *p : ps)
        if (!al16(p)) return false;
    return true;
}
bool dma_hn_q(const KkAttnHeadNorm *hn) { return !hn || (al16(hn->raw) && (!hn->rope || (al16(hn->cos_t) && al16(hn->sin_t)))); }
bool dma_hn_kv(const KkAttnHeadNorm *hn) { return !hn || (dma_hn_q(&hn[0]) && al16(hn[1].raw) && !hn[1].rope); }      // (no rope on V)
bool dma_bytes(int S, int64_t ld0, int64_t ld1) { return (int64_t)S * std::max(ld0, ld1) * 2 < (1ll << 31); }
// (what the pair launch and the two passes share: both kernels' conditions apart from the tile gate)
bool dma_both(int io_bf16, int math, int Sq, int Sk, const void *Q, const void *K, const void *V, const void *dO, const void *dQ, const void *dK,
                     const void *dV, int64_t ldq, int64_t ldk, int64_t ldv, int64_t lddo, const KkAttnHeadNorm *hn_q, const KkAttnHeadNorm *hn_kv) {
    return dma_storage(io_bf16, math, 6) && Sk <= 4096 && al16_all({Q, K, V, dO, dQ, dK, dV}) && dma_hn_q(hn_q) && dma_hn_kv(hn_kv) &&
           dma_bytes(Sk, ldk, ldv) && dma_bytes(Sq, ldq, lddo);
}

// Above 64 KB of dynamic LDS a kernel's attribute has to be raised, once per kernel and thread.
// (one table: 64 slots for the ~20 kernels with more than 64 KB of dynamic LDS; a full table is an error, not a silent
//  hipFuncSetAttribute per launch — ADVICE r4)
int attn_raise_lds(const void *kernel, size_t lds, const char *who) {
    if (lds <= 64 * 1024) return 0;
    static thread_local const void *raised[64];
    for (const void *p : raised)
        if (p == kernel) return 0;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return kk_fail((int)e, "%s: cannot reserve %zu bytes of LDS: %s", who, lds, hipGetErrorString(e));
    for (auto &p : raised)
        if (!p) { p = kernel; return 0; }
    return kk_fail(KK_EINVAL, "%s: the table of kernels with raised LDS limits is full", who);
}

int check_common(const char *name, int B, int heads, int Sq, int Sk, int math, const int64_t *lds, int nld) {
    KK_REQUIRE(B > 0 && heads > 0 && Sq > 0 && Sk > 0, "%s: bad shape B=%d heads=%d Sq=%d Sk=%d", name, B, heads, Sq, Sk);
    KK_REQUIRE(math == KK_MATH_F32 || math == KK_MATH_BF16, "%s: bad math mode", name);
    for (int i = 0; i < nld; ++i) KK_REQUIRE(lds[i] % 8 == 0 && lds[i] >= 64 * heads, "%s: row stride %ld unsupported", name, (long)lds[i]);
    KK_REQUIRE((int64_t)B * heads < 65536, "%s: B*heads too large", name);
    return 0;
}

int check_headnorm(const char *name, const KkAttnHeadNorm *hn, int n) {
    for (int i = 0; i < n; ++i) {
        KK_REQUIRE(hn[i].raw && hn[i].gain && hn[i].partials && hn[i].ldraw % 8 == 0, "%s: head-norm epilogue %d needs raw, gain, partials", name, i);
        KK_REQUIRE(!hn[i].rope || (hn[i].cos_t && hn[i].sin_t), "%s: head-norm epilogue %d: RoPE needs cos/sin tables", name, i);
    }
    return 0;
}

// The one-shot warm request (AttnArgs::warm): written by kk_attn_warm_next, consumed by the next forward or pair launch of the thread.
__thread const void *g_warm_ptr[2] = {nullptr, nullptr};
__thread uint32_t g_warm_bytes[2] = {0u, 0u};

}  // namespace kk_attn
