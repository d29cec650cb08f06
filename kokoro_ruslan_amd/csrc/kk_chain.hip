// One XCD per batch item: a decoder sub-layer as ONE persistent launch (round 6, VERDICT r5 item 1, Stage 0).
//
// What it is.  The decoder's self-attention sub-layer forward (transformers.py:543-560: pre-LN -> q|k|v + per-head RMSNorm + RoPE ->
// causal attention with dropout -> w_o + dropout tail + next LayerNorm) is four dependent launches today.  Every one of them is
// row-local to a batch item, a fixed batch of 8 items is one item per XCD (the dispatcher places workgroup w on XCD w % 8), and an
// XCD's 32 CUs share a 4 MB L2 that holds an item's tensors (0.5 - 1.5 MB each at 512 - 1024 frames).  Here the four kernels run as
// the PHASES of one launch of 256 workgroups: workgroups x, x + 8, x + 16, ... (XCD x) carry item x through all of them and meet at a
// GROUP barrier between phases (one counter per group, never a grid barrier).  Hand-over inside the XCD: PLAIN stores (the lines stay
// in the XCD's L2), sc1 loads on the reading side (L1 bypass, served by that L2) — no write-through round trip, no fence.
//
// How it is built.  The phases ARE the library's kernels: their bodies (g16x_body, attn_fwd3_body, gemm16_body, sublayer_out_row)
// are compiled into this translation unit from the same device headers (the GEMM and attention bodies from theirs, the tail's row
// from kk_tail.h; KK_A_AUX / KK_QKV_AUX set the cache policy of the activation loads), and their
// ARGUMENT BLOCKS are the ones the library's own entry points build: between
// kk_chain_begin() and kk_chain_launch() the entry points record the launch they would have made instead of making it (kk_common.h:
// kk_capture).  Same tile policy, same arguments, same arithmetic in the same order — the chained launch stores the bits the four
// launches store (tests/test_chain_gpu.py), and anything it does not recognise is refused (the caller then launches as before).
//
// Placement is an observation, not a contract (MICROARCH "Workgroup dispatch"): every workgroup reads HW_REG_XCC_ID and reports a
// mismatch in the sync words; the results stay correct under any placement only with KK_CHAIN_SAFE loads / stores (sc1 both sides),
// which kk_chain_launch selects when asked to (flags bit 0) — the probe measures both.
#ifdef KK_CHAIN_PLAIN           // (A/B flavour: plain loads behind an agent-scope acquire — buffer_inv sc1 — after every group barrier)
#define KK_A_AUX 0
#define KK_QKV_AUX 0
#else
#define KK_A_AUX 16             // sc1: the activation operand was written earlier in this launch by another CU of the XCD
#define KK_QKV_AUX 16
#endif
#include "kk_gemm16.h"
#include "kk_group_sync.h"
#include "kk_tail.h"
#include <algorithm>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <type_traits>

namespace chain_g {
#include "kk_gemm16_dev.h"
#include "kk_gemm16x_body.h"
#include "kk_gemm16_body.h"
}
namespace chain_a {
#include "kk_attn.h"
#include "kk_attn_fwd3.h"
}

KkLaunchCapture *kk_capture_begin();
KkLaunchCapture *kk_capture_end();

namespace {

using chain_a::AttnArgs;

// group barrier (sync words: kk_group_sync.h): XCD-local atomics unless the launch asks for agent scope; the A/B flavour with plain
// loads takes the acquire fence behind every barrier
#ifdef KK_CHAIN_PLAIN
struct ChainSyncPolicy { static constexpr bool XCD_LOCAL = true, ACQUIRE = true, SPLIT = false; };
#else
struct ChainSyncPolicy { static constexpr bool XCD_LOCAL = true, ACQUIRE = false, SPLIT = false; };
#endif

struct ChainSA {
    G16Args qkv;                 // phase 1: q|k|v projection + head norm (+ RoPE)
    AttnArgs attn;               // phase 2: causal attention
    G16Args wo;                  // phase 3: output projection
    SubOutArgs tail;             // phase 4: dropout tail + next LayerNorm
    unsigned *sync;
    unsigned long long *trace;   // tools: per workgroup 8 clock stamps (100 MHz) + its XCC id, or null
    int S, nqb, local_sync, wo_rounds;
};

constexpr int CHAIN_LDS = 124 * 1024;

// FORM 0: the kernels an 8 x 512 step takes (g16x 128x192 loader-wave tile, 64-query attention blocks);
// FORM 1: 8 x 1024 (256x192 tile, 128-query blocks).  Both: gemm16 128x64 eight-wave tile for w_o, two 256-column vectors per row.
template <int FORM>
__global__ __launch_bounds__(512) void chain_sa_fwd_kernel(const ChainSA c) {
    extern __shared__ __attribute__((aligned(16))) char chain_smem[];
    const int wg = blockIdx.x, item = wg & 7, member = wg >> 3, members = gridDim.x >> 3;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long *tr = (c.trace && threadIdx.x == 0) ? c.trace + (size_t)wg * 16 : nullptr;
    auto stamp = [&](int i) { if (tr) tr[i] = wall_clock64(); };
    stamp(0);
    if (threadIdx.x == 0) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;         // HW_REG_XCC_ID[3:0]
        if (tr) tr[15] = xcc;
        if ((int)xcc != item) __hip_atomic_fetch_add(c.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    GroupSync<ChainSyncPolicy> sy;
    sy.init(c.sync, item, members, c.local_sync != 0);

    // ---- phase 1: the item's q|k|v tiles (the XCD sweep of g16x_body IS the item: 256 tiles, 32 per XCD, n fastest)
    if constexpr (FORM == 0) chain_g::g16x_body<false, false, 128, 192, 3, 3, 2, 2, 4>(c.qkv, wg, chain_smem);
    else chain_g::g16x_body<false, false, 256, 192, 2, 3, 4, 2, 0>(c.qkv, wg, chain_smem);
    stamp(1);
    sy.barrier();
    stamp(2);

    // ---- phase 2: 8 heads x nqb query blocks of the item = 2 units per member, a long and a short causal block together
    {
        const int units = c.attn.heads * c.nqb;
        for (int k = 0; k < 2; ++k) {
            const int u = k == 0 ? units - 1 - member : member;                       // (the long one first)
            const int hh = u % c.attn.heads, qb = u / c.attn.heads;
            if constexpr (FORM == 0) chain_a::attn_fwd3_body<2, 4, 2, true>(c.attn, qb, item * c.attn.heads + hh);
            else chain_a::attn_fwd3_body<4, 2, 3, true>(c.attn, qb, item * c.attn.heads + hh);
        }
    }
    stamp(3);
    sy.barrier();
    stamp(4);

    // ---- phase 3: the item's output-projection tiles (same sweep)
    for (int r = 0; r < c.wo_rounds; ++r) {                                            // (tiles [32 x rounds .. ) of XCD x: rows of item x)
        if (r) __syncthreads();
        chain_g::gemm16_body<false, false, 128, 64, 3, 0, 8, 2>(c.wo, wg + 256 * r, chain_smem);
    }
    stamp(5);
    sy.barrier();
    stamp(6);

    // ---- phase 4: the item's rows, a wave per row
    {
        const int per = c.S / members;                                                // rows of the item per member
        for (int r = wave; r < per; r += 8) {
            const int64_t row = (int64_t)item * c.S + member * per + r;
            if (c.tail.n != nullptr) sublayer_out_row<__bf16, __bf16, 2>(c.tail, row);
        }
    }
    stamp(7);
    sy.exit();
}

}  // namespace

extern "C" int kk_chain_begin(void *stream) {
    (void)stream;
    kk_capture_begin();
    return 0;
}

// kind 0: decoder self-attention sub-layer forward.  flags bit 0: agent-scope barrier atomics (else XCD-local).
// Returns KK_ENOTSUP (and launches nothing) when the recorded sequence is not one this launch carries.
extern "C" int kk_chain_launch(int kind, uint32_t *sync, uint64_t *trace, int flags, void *stream) {
    KkLaunchCapture *cap = kk_capture_end();
    KK_REQUIRE(kind == 0, "kk_chain_launch: unknown kind %d", kind);
    KK_REQUIRE(sync != nullptr, "kk_chain_launch: sync words required");
    if (cap->overflow || cap->n != 4) return kk_fail(KK_ENOTSUP, "kk_chain_launch: %d launches recorded (want 4)", cap->n);
    const KkCapturedLaunch &l0 = cap->e[0], &l1 = cap->e[1], &l2 = cap->e[2], &l3 = cap->e[3];
    int form = -1;
    if (!strcmp(l0.kernel, "g16x<0,0,128,192,3,3,2,2,4>") && !strcmp(l1.kernel, "attn_fwd3_q64")) form = 0;
    if (!strcmp(l0.kernel, "g16x<0,0,256,192,2,3,4,2,0>") && !strcmp(l1.kernel, "attn_fwd3_q128")) form = 1;
    if (form < 0 || strcmp(l2.kernel, "gemm16_w8<0,0,3>") || strcmp(l3.kernel, "sublayer_out_fwd<2,2,2>"))
        return kk_fail(KK_ENOTSUP, "kk_chain_launch: sequence [%s | %s | %s | %s] is not a chain this launch carries", l0.kernel, l1.kernel,
                       l2.kernel, l3.kernel);
    static_assert(sizeof(ChainSA) <= 4096, "kernel arguments");
    ChainSA c;
    KK_REQUIRE(l0.bytes == sizeof(G16Args) && l1.bytes == sizeof(AttnArgs) && l2.bytes == sizeof(G16Args) && l3.bytes == sizeof(SubOutArgs),
               "kk_chain_launch: argument block sizes differ from this translation unit's");
    memcpy(&c.qkv, l0.args, sizeof(G16Args));
    memcpy(&c.attn, l1.args, sizeof(AttnArgs));
    memcpy(&c.wo, l2.args, sizeof(G16Args));
    memcpy(&c.tail, l3.args, sizeof(SubOutArgs));
    const int B = c.attn.B, S = c.attn.Sq, QB = form == 0 ? 64 : 128;
    const bool ok = B == 8 && c.attn.Sk == S && c.attn.causal && c.attn.heads == 8 && S % QB == 0 && (S / QB) * 8 == 64 && S % 32 == 0 &&
                    c.qkv.M == (int64_t)B * S && c.qkv.tiles_m * c.qkv.tiles_n == 256 && c.qkv.tiles_m == 32 && c.qkv.splits <= 1 &&
                    c.wo.M == (int64_t)B * S && (c.wo.tiles_m * c.wo.tiles_n) % 256 == 0 && c.wo.tiles_m * 128 == B * S && c.wo.splits <= 1 && !c.wo.atomic &&
                    c.tail.rows == (int64_t)B * S && c.tail.H == 512 && c.tail.n != nullptr && c.attn.key_mask == nullptr;
    if (!ok) return kk_fail(KK_ENOTSUP, "kk_chain_launch: shape B=%d S=%d tiles %dx%d / %dx%d is not one item per XCD", B, S, c.qkv.tiles_m,
                            c.qkv.tiles_n, c.wo.tiles_m, c.wo.tiles_n);
    // the XCD sweep of the GEMM bodies, n fastest: XCD x runs tiles [32 x, 32 x + 32) = the 4 row tiles of item x (any order gives the
    // same bits: a tile's arithmetic does not depend on who runs it); plain stores: the consumers sit on the same XCD
    c.qkv.xcd_swizzle = c.wo.xcd_swizzle = 1;
    c.qkv.m_fast = c.wo.m_fast = 0;
    c.qkv.wt = c.wo.wt = c.attn.wt = c.tail.wt = 0;
    c.sync = sync;
    c.trace = reinterpret_cast<unsigned long long *>(trace);
    c.S = S;
    c.nqb = S / QB;
    c.local_sync = (flags & 1) ? 0 : 1;
    c.wo_rounds = c.wo.tiles_m * c.wo.tiles_n / 256;
    static bool raised[2] = {false, false};
    const void *fn = form == 0 ? (const void *)chain_sa_fwd_kernel<0> : (const void *)chain_sa_fwd_kernel<1>;
    if (!raised[form]) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CHAIN_LDS);
        if (e != hipSuccess) return kk_fail((int)e, "kk_chain_launch: cannot reserve %d bytes of LDS: %s", CHAIN_LDS, hipGetErrorString(e));
        raised[form] = true;
    }
    kk_note_kernelf("chain_sa_fwd<%d>", form);
    if (form == 0) hipLaunchKernelGGL(chain_sa_fwd_kernel<0>, dim3(256), dim3(512), CHAIN_LDS, (hipStream_t)stream, c);
    else hipLaunchKernelGGL(chain_sa_fwd_kernel<1>, dim3(256), dim3(512), CHAIN_LDS, (hipStream_t)stream, c);
    KK_LAUNCH_CHECK("kk_chain_launch");
    return 0;
}

// the recorded launches of the open capture are dropped (an error path of the caller)
extern "C" int kk_chain_abort(void *stream) {
    (void)stream;
    kk_capture_end();
    return 0;
}
