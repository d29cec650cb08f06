"""MI355X engine for the Kokoro acoustic-model train step.

Host side of the hot path: owns a flat fp32 parameter arena (params, grads, Adam m/v, EMA as contiguous
HBM slabs with a segment table), per-shape activation workspaces, and the explicit forward / backward /
optimizer kernel sequences.  Autograd is not used: the model is a fixed DAG, so the backward is a
hand-written reverse sequence of the same C-ABI kernels (kokoro_ruslan_amd.lib → libkokoro_hip.so).
Nothing in a step synchronises with the host, so a whole step can be captured in one hipGraph.

What it restates (reference file:line, relative to /root/reference/src/kokoro):
  forward        model/model.py:565-673 (forward_training) with encode_text :358-388, VarianceAdaptor.forward
                 model/variance_predictor.py:286-439, decoder model/transformers.py:543-583,622-662
  losses         training/losses.py:9-216
  step driver    training/trainer.py:2218-2242,2346-2477 + runtime_policies.py:14-87 (see csrc/kk_optim.hip)
Quirks kept on purpose: the length-regulated memory is detached (no gradient from the decoder into
the text encoder, facts 5); key padding = (phoneme id == 0) (fact 6); GroupNorm(1,C) statistics per 512-frame
chunk including padding (fact 7); stop head sees a detached decoder output (model.py:562).
Expanded length T' = max_b Σdur != mel length T (model/model.py:607-628): see forward_backward(expanded_len=...).
Activation memory: one workspace sized for the largest batch seen (see _buf), whatever the number of batch shapes.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading
from collections import OrderedDict
from functools import lru_cache
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import lib as kk
from . import spec
from .prosody import as_list as prosody_list
from .prosody import pack as pack_prosody
from .prosody import pack_contours
from .spec import VA, ModelDims, StepHyper

CHUNK = 512   # variance_predictor.py:77
_ITEMSIZE = {torch.float32: 4, torch.bfloat16: 2, torch.float64: 8, torch.int64: 8, torch.int32: 4, torch.uint8: 1}


def _b16(t) -> int:
    """1 when the tensor is stored as bf16 (the C ABI's *_bf16 flags are derived from the tensors themselves)."""
    return 1 if t is not None and t.dtype == torch.bfloat16 else 0


class LayerNames(NamedTuple):
    """What the launches of one transformer layer are addressed by.  site / next_ln are per sub-layer: "sa", "ff" and, in the
    decoder, "ca".  A site seeds the sub-layer's dropout masks (its kernels add small fixed offsets), so the forward and the
    backward of a layer must take it from here; next_ln = (workspace key, parameter prefix, dtype) of the LayerNorm that reads
    the sub-layer's output, which its fused tail computes.  (The two functions below cache what they return: read only.)"""
    prefix: str                                     # parameters: "transformer_encoder_layers.<i>" / "decoder.layers.<i>"
    key: str                                        # workspace buffers: "<ns>enc<i>" / "<ns>dec<i>"
    site: Dict[str, int]
    next_ln: Dict[str, Tuple[str, str, torch.dtype]]


_SUBLAYER = {"sa": ".self_attn", "ca": ".cross_attn", "ff": ".ff"}     # parameter prefix of a sub-layer within its layer


@lru_cache(maxsize=None)
def encoder_layer_names(i: int, n_layers: int, dtype: torch.dtype, ns: str = "") -> LayerNames:
    """Text-encoder layer i of n_layers with activations stored as `dtype`, workspace keys under the namespace `ns`
    (inference: "syn." ...).  The stack ends in encoder_norm, whose output is fp32."""
    pf, key, site = f"transformer_encoder_layers.{i}", f"{ns}enc{i}", 1000 + 32 * i
    after = ((f"{ns}enc{i + 1}.ln1", f"transformer_encoder_layers.{i + 1}.norm1", dtype) if i + 1 < n_layers
             else (f"{ns}enc.norm", "encoder_norm", torch.float32))
    return LayerNames(pf, key, {"sa": site, "ff": site + 8}, {"sa": (key + ".ln2", pf + ".norm2", dtype), "ff": after})


@lru_cache(maxsize=None)
def decoder_layer_names(i: int, n_layers: int, dtype: torch.dtype, ns: str = "") -> LayerNames:
    """Decoder layer i of n_layers (self-attention, cross-attention, feed-forward); the stack ends in decoder.norm."""
    pf, key, site = f"decoder.layers.{i}", f"{ns}dec{i}", 2000 + 32 * i
    after = ((f"{ns}dec{i + 1}.ln1", f"decoder.layers.{i + 1}.norm1", dtype) if i + 1 < n_layers
             else (f"{ns}dec.norm", "decoder.norm", dtype))
    return LayerNames(pf, key, {"sa": site, "ca": site + 8, "ff": site + 16},
                      {"sa": (key + ".ln2", pf + ".norm2", dtype), "ca": (key + ".ln3", pf + ".norm3", dtype), "ff": after})


class _Step:
    """What the stages of one training micro-batch share (KokoroEngine._fb_launches).  _step_setup makes it with every decision
    taken; what a later stage fills in is None (deferred0: []) until then, so no stage reads a name that nothing has bound."""
    __slots__ = (
        "batch", "backward", "zero_grads",
        "B", "Pn", "T", "Tp", "Ne", "Nd", "Np",           # Tp: frames the durations expand to (>= T); rows B * Pn, B * T, B * Tp
        "p_din", "pe_drop", "p_enc", "p_dec", "p_var",    # dropout rates (0 with train_dropout off)
        "stack",                                          # text encoder as one persistent launch (_encoder_stack_ok)
        "gen_keep", "gen_layers",                         # attention keep bits generated beside it, for so many decoder layers
        "spec_aug",
        "sort_buckets",                                   # bucket-embedding gradients as the sorted segmented sum (embed_bwd_sorted)
        "tail_mode",                                      # where the backward's memory tail runs (tail_aside, resolved)
        "lcfg", "largs",                                  # kk.KkLossCfg; the loss kernels' common arguments (_fb_losses)
        "fork",                                           # events: behind the loss gradients (_fb_loss_grads),
        "tail_fork",                                      # behind the last cross-attention dK / dV (tail_mode 1, 3, 4; 2: the decoder backward),
        "wgrad0_fork", "deferred0",                       # behind decoder layer 0's backward when its grouped weight gradients wait: those
        # workspace views that cross stages, set by the stage that first writes them:
        "text_mask",                                                                  # _step_setup
        "shifted", "dec_head",                                                        # _fb_decoder_head: (x0, dec0.xa, dec0.ln2.y)
        "enc_last", "enc",                                                            # _fb_encoder_fwd: last stream, encoder_norm of it
        "dur_pred", "col_e", "col_f", "idx", "lens", "memory", "fmask", "pidx", "eidx", "pitch_pred", "energy_pred",   # _fb_variance_adaptor
        "xf_p", "fmask_p", "pitch_l", "energy_l",         # (the predictors' Tp-frame views, what the losses read; the T-frame ones when Tp == T)
        "be_order", "be_items",                                                       # _fb_predictors_fwd, with sort_buckets
        "dec_last", "dec_out", "mel_pred", "stop",                                    # _fb_decoder_fwd
        "dmel", "ddur", "dstop", "dpitch", "denergy",                                 # _fb_loss_grads
        "dy", "dmem")                                                                 # _fb_decoder_bwd: gradients of the decoder stream, the memory

    def __init__(self, **decided):
        for name in self.__slots__:
            setattr(self, name, decided.pop(name, None))
        assert not decided, decided
        self.deferred0 = []


class _Micro(NamedTuple):
    """The decisions of one micro-batch of an accumulation cycle, taken once (KokoroEngine._micro) however the step is run."""
    first: bool                                     # opens the cycle: the gradient arena is zeroed for it
    boundary: bool                                  # closes it: the only micro-batch that talks to the other ranks; finish_cycle follows
    div: int                                        # the accumulation divisor
    scale: float                                    # dp_loss_scale / div: the seed of the backward
    mel_length: int                                 # canonical_mel_length: what the optimizer boundary and the graph keys take
    external_sync: bool                             # the caller reduces arena.g itself at the boundary (grad_sync): no tile norms


class _FbKey(NamedTuple):
    """What a captured forward/backward graph depends on besides the batch shape (KokoroEngine._fb_graph)."""
    div: int
    first: bool
    train_dropout: bool
    spec_augment: bool
    math: int
    exchange: bool                                  # the in-step bucket exchange runs in this micro-batch (the boundary's, with dp_comm)
    # kk_losses_finalize takes the GLOBAL mel length by value, so a graph captured under one value must not be replayed under another
    # (ADVICE r3); canonical_mel_length keeps that to one capture per local shape up to 1400 frames.  0 without a loss exchange.
    mel_length: int
    loss_sync: bool                                 # a loss exchange is captured
    self_cleaning_acc: bool
    attn_keep_gen: Tuple[bool, float]               # (switch, rate): how many layers' keep bits are generated aside
    tile_norms: bool                                # the grouped weight-gradient launches leave tile-norm records


class _AttnOps(NamedTuple):
    """The workspace views of one attention sub-layer (KokoroEngine._attn_ops): what its forward and its backward both address,
    named once.  q / k / v are column slices of the containers below them.  A field the caller did not ask for is None (the
    decode step names the first five alone)."""
    q_n: torch.Tensor                               # per-head normalised (+ RoPE) q, k, v: what the attention kernels read
    k_n: torch.Tensor
    v_n: torch.Tensor
    ctx: torch.Tensor
    lse: torch.Tensor
    q_raw: Optional[torch.Tensor] = None            # the projections before the head norm
    k_raw: Optional[torch.Tensor] = None
    v_raw: Optional[torch.Tensor] = None
    gains: Optional[Tuple] = None                   # the (q, k, v) head-norm gains
    raw: Optional[torch.Tensor] = None              # the sub-layer's own projection: q|k|v fused [Nq, 3H] (self), q alone (cross)
    nrm: Optional[torch.Tensor] = None
    kv_raw: Optional[torch.Tensor] = None           # cross-attention: this layer's K|V slice [Nk, 2H] of the all-layer buffers
    # with grads:
    dgains: Optional[Tuple] = None                  # the gains' gradient vectors
    d_out: Optional[torch.Tensor] = None            # masked gradient of the output projection's result (_tail_bwd wrote it)
    dctx: Optional[torch.Tensor] = None
    delta: Optional[torch.Tensor] = None
    dn: Optional[torch.Tensor] = None               # gradient containers shaped like nrm / raw
    draw: Optional[torch.Tensor] = None
    dq_n: Optional[torch.Tensor] = None
    dk_n: Optional[torch.Tensor] = None
    dv_n: Optional[torch.Tensor] = None
    dq_raw: Optional[torch.Tensor] = None
    dk_raw: Optional[torch.Tensor] = None
    dv_raw: Optional[torch.Tensor] = None
    dkv_n: Optional[torch.Tensor] = None            # cross-attention with a K/V branch: the layer's slices of the all-layer gradients
    dkv_raw: Optional[torch.Tensor] = None


class Arena:
    """Flat fp32 slabs p / g / m / v / ema with one 1024-aligned, zero-padded segment per tensor."""

    def __init__(self, dims: ModelDims, hp: StepHyper, device: torch.device, shadow_bf16: bool = False):
        self.dims, self.device = dims, device
        self.param_names = list(spec.param_shapes(dims).keys())
        # physical order (spec.arena_layout): the K and V projections of all decoder cross-attention layers first and
        # contiguous, so the memory is projected for every layer by ONE GEMM against a [layers*2H, H] matrix (and its two
        # gradients likewise); everything else in state-dict order.  Names, not offsets, are the interface.
        assert spec.SEG_ALIGN == kk.KK_SEG_ALIGN
        self.names, self.shapes, self.offset, off = spec.arena_layout(dims)
        segs = [(n, self.shapes[n]) for n in self.names]
        self.total = off
        self.nblocks = off // kk.KK_SEG_ALIGN
        self.nseg = len(segs)
        z = lambda: torch.zeros(off, dtype=torch.float32, device=device)
        self.p, self.g, self.m, self.v = z(), z(), z(), z()
        self.ema = z() if hp.use_ema else None
        # bf16 mode: a bf16 copy of p at the same element offsets, rewritten by the optimizer kernels; the GEMMs read
        # weights from it (half the bytes, no conversion in the k-loop).  fp32 p stays the master copy.
        self.p16 = torch.zeros(off, dtype=torch.bfloat16, device=device) if shadow_bf16 else None
        block_seg = torch.empty(self.nblocks, dtype=torch.int32)
        preclip, lr_mult, wd, flags = [], [], [], []
        table = spec.group_lr_mult_wd(hp)
        for i, (n, s) in enumerate(segs):
            b0 = self.offset[n] // kk.KK_SEG_ALIGN
            block_seg[b0:b0 + -(-math.prod(s) // kk.KK_SEG_ALIGN)] = i
            if n in spec.param_shapes(dims):
                mx = spec.preclip_max_norm(n, hp)
                preclip.append(mx if mx is not None else 0.0)
                mult, w = table[spec.param_group_of(n)]
                lr_mult.append(mult), wd.append(w)
                flags.append(1 | 2 | (4 if spec.is_weight_norm_target(n) else 0))
            else:                                   # persistent buffer: EMA-tracked only (trainer.py:1504-1517)
                preclip.append(0.0), lr_mult.append(0.0), wd.append(0.0), flags.append(2)
        self.block_seg = block_seg.to(device)
        self.seg_preclip = torch.tensor(preclip, dtype=torch.float32, device=device)
        self.seg_lr_mult = torch.tensor(lr_mult, dtype=torch.float32, device=device)
        self.seg_wd = torch.tensor(wd, dtype=torch.float32, device=device)
        self.seg_flags = torch.tensor(flags, dtype=torch.int32, device=device)
        self.P = {n: self.view(self.p, n) for n in self.names}
        self.G = {n: self.view(self.g, n) for n in self.names}
        self.E = {n: self.view(self.ema, n) for n in self.names} if hp.use_ema else {}
        self.P16 = {n: self.view(self.p16, n) for n in self.names} if shadow_bf16 else {}

    def view(self, slab: torch.Tensor, name: str) -> torch.Tensor:
        o, s = self.offset[name], self.shapes[name]
        return slab[o:o + math.prod(s)].view(s)

    def fused(self, slab: torch.Tensor, first: str, count: int) -> torch.Tensor:
        """[count*H, H] view over `count` consecutive square projection weights (w_q|w_k|w_v are adjacent)."""
        H = self.dims.hidden
        assert (H * H) % kk.KK_SEG_ALIGN == 0
        o = self.offset[first]
        return slab[o:o + count * H * H].view(count * H, H)


def canonical_mel_length(global_mel_length, local_T: int) -> int:
    """The mel length the step's kernels take BY VALUE (kk_losses_finalize, kk_opt_prepare: the batch-shape heuristics of
    trainer.py:2218-2242), canonicalised for the graph keys: both kernels use it only as max(T / 1400, max_dur / 150) > 1, so every
    length up to 1400 frames gives the result of 1400 exactly (T / 1400 <= 1 never decides the max when the max exceeds 1).  Keying the
    step graphs on the raw global length made every (local shape, global T) pair of a ragged data-parallel run a new capture
    (VERDICT r4); with this value a shape is captured once for all global lengths <= 1400 and once per longer length."""
    return max(int(global_mel_length or local_T), 1400)


class KokoroEngine:
    def __init__(self, dims: Optional[ModelDims] = None, hyper: Optional[StepHyper] = None, device="cuda",
                 math_mode: str = "f32", total_steps: int = 20000, seed: int = 0, init: bool = True,
                 storage: str = "auto"):
        kk.load()                                   # fails loudly when libkokoro_hip.so is missing
        if not torch.cuda.is_available():
            raise RuntimeError("KokoroEngine needs an MI355X (no CPU fallback in the product path)")
        self.dims = dims or ModelDims()
        self.dims.validate()
        self.hp = hyper or StepHyper()
        self.device = torch.device(device)
        self.math = {"f32": kk.KK_MATH_F32, "bf16": kk.KK_MATH_BF16}[math_mode]
        self.math_mode = math_mode
        # activation / weight-operand storage: "f32" everywhere (always in the parity mode), or bf16 for the GEMM and
        # attention operands of the bf16 mode ("bf16": both stacks, "bf16-dec": decoder stack only).
        if storage == "auto":
            storage = "bf16" if math_mode == "bf16" else "f32"
        if storage not in ("f32", "bf16", "bf16-dec") or (storage != "f32" and math_mode != "bf16"):
            raise ValueError(f"storage={storage!r} is not available with math_mode={math_mode!r}")
        if storage != "f32" and any(v % 8 for v in (self.dims.enc_ff, self.dims.dec_ff, self.dims.var_filter)):
            raise ValueError("bf16 storage needs enc_ff, dec_ff and var_filter to be multiples of 8")
        self.storage = storage
        self.enc_dt = torch.bfloat16 if storage == "bf16" else torch.float32
        self.dec_dt = torch.bfloat16 if storage in ("bf16", "bf16-dec") else torch.float32
        self.arena = Arena(self.dims, self.hp, self.device, shadow_bf16=storage != "f32")
        self.use_shadow = storage != "f32"
        self.total_steps = total_steps
        # Workspace: ONE flat buffer per name, grown to the largest request ever made under that name, and handed out as
        # views — so a run over ever-changing batch shapes (dynamic batching: B in [4, 32], T up to 1800) holds one
        # activation set sized for the largest batch instead of one per shape.  Growing a buffer moves it, so everything
        # that baked its address in (captured graphs, descriptor tables) is dropped with it (_invalidate).
        self._ws: Dict[str, torch.Tensor] = {}
        self._views: Dict[Tuple, torch.Tensor] = {}
        self._ops: Dict[Tuple, _AttnOps] = {}          # attention operand records by shape (_attn_ops): views, dropped with them
        self.ws_generation = 0
        self.ws_bytes = 0
        self.max_graphs = int(os.environ.get("KK_MAX_GRAPHS", "24"))     # LRU bound of captured batch shapes
        self.max_tables = 8192                                           # descriptor tables (all kinds together)
        self._graphs: "OrderedDict[Tuple, Dict]" = OrderedDict()
        self._tables: "OrderedDict[Tuple, object]" = OrderedDict()
        self._shape_seen: "OrderedDict[Tuple, int]" = OrderedDict()
        # Held while a hipGraph capture is in progress.  Other host threads that talk to the HIP runtime (the trainer's
        # batch prefetcher: event waits, pinned allocations, H2D copies) take it around those calls: on this runtime a
        # concurrent call from another thread invalidates the capture (hipErrorStreamCaptureInvalidated), thread_local
        # capture mode notwithstanding.
        self.capture_lock = threading.Lock()
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._reduce_lists = {"": [], "side.": [], "kv.": []}   # per stream namespace
        self.opt_state = torch.zeros(kk.OS["SIZE"], dtype=torch.float64, device=self.device)
        ns = self.arena.nseg
        f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
        self.seg_gscale, self.seg_decay, self.seg_stepsize = f32(ns), f32(ns), f32(ns)
        self.step_consts = f32(4)
        self.grad_sumsq = torch.zeros(ns, dtype=torch.float64, device=self.device)
        # (Q34.30 fixed-point sums: integer adds commute, so the weight-norm projection decides the same on every replica)
        self.p_sumsq = torch.zeros(ns, dtype=torch.int64, device=self.device)
        # record workspace of kk_seg_sumsq: workgroup partials merged in arena order by a fixed tree (no atomics, no zero-fill)
        self.sumsq_ws = torch.zeros(kk.load().kk_seg_sumsq_ws_bytes(self.arena.nblocks), dtype=torch.uint8, device=self.device)
        self.max_dur = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.loss_acc = torch.zeros(12, dtype=torch.float64, device=self.device)    # 5 sums, 5 counts, non-finite outputs, spare
        self.losses = f32(6)
        self.loss_coef = f32(5)
        self.micro_in_cycle = 0
        self._last_micro: Optional[_Micro] = None   # the record of the micro-batch last run: what finish_cycle closes the cycle by
        self.dp_loss_scale = 1.0                    # 1/world in data-parallel runs (dp.GradSync.loss_scale)
        # Data parallel with ragged shards: an object with .loss_sync(acc[12] f64, max_dur[1] i64) that SUM / MAX all-reduces
        # them in place between the loss forward and the loss backward; the losses are then re-finalised with the global
        # valid-element counts and dp_loss_scale stays 1.  dp.BucketedExchange over RCCL issues the two collectives through
        # the C ABI (kk_comm_loss_sync) on the stream of the step, so they are captured with it: ONE communicator per step,
        # graph replay for ragged shards too.  dp.LossSync (torch.distributed; the gloo tests) is eager only.
        # None = per-rank normalisers (exact for equal shards).
        self.loss_sync = None
        # Data-parallel exchange INSIDE the step (dp.BucketedExchange over the C ABI's kk_comm_*): every bucket of the
        # gradient arena is all-reduced on the exchange's stream as soon as the backward has finished it — after each
        # decoder / encoder layer's grouped weight gradients, the rest after the last launch — and the optimizer waits for
        # that stream.  The collectives are captured with the step, so they are one more branch of its hipGraph (no graph
        # split, nothing between the backward graph and the optimizer graph).  With gradient accumulation only the
        # boundary micro-batch exchanges (_exchange_now: written by _micro_flags alone, True between steps).
        self.dp_comm = None
        self._comm_events = {}
        self._exchange_now = True
        self.global_mel_length = None               # batch-max T over all ranks (adaptive loss scale / clip heuristics)
        # dropout / DropPath / SpecAugment: off = the parity configuration (reference with p = 0)
        self.train_dropout = False
        # Second HIP stream: the parts of a step that do not depend on the decoder (pitch/energy predictors; after the
        # loss, the predictors' and the whole text encoder's backward — the length-regulated memory is detached) run
        # beside the decoder kernels instead of after them; they are small launches that cannot fill 256 CUs alone.
        self.overlap = True
        self._side = torch.cuda.Stream(device=self.device)
        self._tmp_ns = ""
        # Third stream: the decoder's input projection and layer-0 self-attention run beside the text encoder (they do not
        # need its output); one fork, one join before the first cross-attention.  Forks are not free in a hipGraph:
        # measured at 8x512, the long independent encoder/predictor branch pays (470K -> 548K frames/s) and so does this
        # one (630K -> 638K), but a per-layer fork for the cross-attention K/V backward lost 9 %, a stream per
        # weight-gradient GEMM 19 %, and moving the duration predictor's forward aside 2 %.
        self._kv = torch.cuda.Stream(device=self.device)
        self.dec_head_aside = True
        # Where the backward's memory tail (all layers' cross-attention K/V weight gradient, the memory gradient, the two
        # bucket-embedding gradients: needs only the cross-attention dK / dV) runs.  0: at the end of the main chain; 3: on the side
        # stream behind the encoder's backward; 4: like 3 with the K/V weight gradient as a member of decoder layer 0's grouped launch;
        # -1: 4 up to 4096 decoder rows, 3 above (measured: profiles/r05_memory_tail_aside_ab.txt).  1 / 2 (a THIRD branch) serialise
        # the side branch behind the main chain in the replayed graph (+21 %): kept for the record of that measurement.
        self.tail_aside = -1
        # bucket-embedding gradients as a segmented sum over frames sorted by bin (kk_bucket_sort beside the predictors' forward)
        self.embed_bwd_sorted = True
        # decoder layer 0's grouped weight-gradient launch on the side stream's idle end instead of the main chain: 1 always, 0 never,
        # -1 where the memory tail is in mode 3 (> 4096 rows: -0.5 ... -1.1 %; at 4096 rows +0.3 ... +1.4 %)
        self.wgrad0_aside = -1
        # legacy schedule (hp.use_onecycle_lr = False): scheduler steps taken so far = epochs completed; the trainer advances it
        self.lr_epoch = 0
        # Fusion switches: plain attributes (tests and tools/probes set them on the object for A/B runs; nothing reads the
        # environment).  Each fused form is tested against the unfused one it replaces.
        self.fuse_glu_fwd = True
        self.group_wgrads = True
        self.fuse_headnorm = True
        self.fuse_headnorm_bwd = True
        # attention backward as ONE launch (kk_attn_bwd: the dQ and the dK/dV kernel as the two halves of a grid), Delta from the
        # epilogue of the w_o dgrad GEMM (kk_gemm_dgrad_delta) — bf16 storage, shapes that take the eight-wave GEMM tile
        self.attn_bwd_pair = True
        # ... or, where the library prices it cheaper (kk_attn_bwd_two_pass: nowhere, 128 against the pair launch's 118 us at full 1024 x 1024), as the dK/dV
        # kernel that also stores dS + a dQ pass without softmax work (kk_attn_bwd_ws; workspace of 2 bytes per score per stream)
        self.attn_two_pass = True
        # the attention forward stores its dropout keep decisions as packed bits (kk_attn_fwd_kb) and the backward's pair launch reads
        # them (kk_attn_bwd_kb) instead of hashing them again: ~40 % of the backward kernels' vector instructions (round 5)
        self.attn_keep_bits = True
        # ... and, where the persistent encoder launch gives it a place to hide, the bits of ALL the decoder's attention launches come
        # from ONE pure-vector launch beside the encoder forward (kk_attn_keep_gen, on the decoder-head stream) and the forward READS
        # them too (kk_attn_fwd_rb): -3 us per forward launch at 512 frames, -6.4 ... -8.6 us at 1024 (round 6; same bits either way)
        self.attn_keep_gen = True
        # How many decoder layers' bits the generator writes: what fits beside the persistent encoder.  The generator of ALL twelve launches of an
        # 8 x 1024 step outlasts the encoder and delays the decoder head; four layers' worth is the measured optimum there, all six at 8 x 512
        # (profiles/r06_keep_bits_gen_ab.txt; the generator holds 40 registers so that TWO of its waves fit a SIMD beside the encoder's two).
        # Budget = attn_keep_gen_rate 32 x 32 units per microsecond of encoder time (~160 + 2 P us for P phonemes); the later layers' forwards hash and
        # store as before (same bits either way).  0 = never generate.
        self.attn_keep_gen_rate = 1100.0
        # One GPU: the per-segment gradient norms of the weight matrices come from the epilogue of the grouped weight-gradient launches
        # (a record per tile of the FINAL values it stored) instead of from the optimizer's pass over the 199 MB gradient arena, which then
        # reads only what no such launch wrote (embeddings, biases, norms, predictors).  Data parallel keeps the full pass: the norm that
        # clips is the REDUCED gradient's.  _ss_step: the book-keeping of the micro-batch in flight; _ss_ready: what the optimizer boundary
        # behind it may rely on (consumed by optimizer_step; None = full pass).
        self.grad_norm_from_wgrads = True
        self._ss_step = None
        self._ss_ready = None
        self._ss_masks: Dict[frozenset, torch.Tensor] = {}
        self._external_sync = False
        self._seg_of_ptr = {self.arena.G[n].data_ptr(): i for i, n in enumerate(self.arena.names)}
        # Weight warming (kk_attn_warm_next; profiles/r06_l2_retention_probe.txt): an XCD's L2 keeps read-only lines across a kernel
        # boundary, and the attention launches are vector-bound with idle request slots — so the decoder's attention forward touches
        # the lines of the output projection behind it (bit 0) and the dQ half of the backward's pair launch, which ends ~9 us before
        # its dK/dV half, those of the q | k | v (or q) projection whose dgrad follows (bit 2): the GEMMs find their weights L2-hot
        # instead of in HBM.  Interleaved: -0.2 ... -0.6 % at 8 x 512, -0.4 ... -0.7 % at 8 x 1024, level under dynamic batching; bit 1
        # (+ the next sub-layer's first matrix, 0.5 - 3 MB, from the forward) and bit 3 (+ the next output projection from the backward)
        # measured level or worse (profiles/r06_weight_warming_ab.txt).
        self.attn_warm = 5
        self._keep_ready = set()                    # sub-layer keys whose bits kk_attn_keep_gen has written in this step
        # (one-tile sequences — the text encoder's <= 64 phonemes, on the side branch — take the two thinner launches: re-measured INSIDE
        #  the step in round 5, 3.6215 -> 3.608 ms at 8 x 512 (4 of 4 interleaved rounds); 65..128 phonemes keep the pair launch: two launches
        #  there are +0.3 % at 8 x 1024.  profiles/r05_encoder_attn_pair_ab.txt)
        self.attn_pair_min_seq = 64
        self.attn_proj_bf16 = True                 # decoder w_o output stored as bf16 (bf16 mode)
        # the decoder's attention output projection and the sub-layer tail behind it as ONE row-owner launch (kk_linear_tail_fwd) where
        # the library measured it faster (kk_linear_tail_pays: whole rounds of workgroups at >= ~6 K rows); bit-identical results
        self.fuse_linear_tail = True
        # the step's small fp64 accumulators (loss sums, per-segment gradient / parameter norms) are kept zero by their last readers
        # instead of a zero-fill launch in front of every writer (three dependent launches of the critical chain)
        # _acc_clean: host-side record of the invariant "the accumulators are zero between steps".  It is dropped while a writer ..
        # cleaner sequence is in flight and restored only when the sequence has been issued completely (_acc_guard): a step that
        # aborts in between (a collective or a launch raising), or a flip of the switch on a live engine, costs one zero-fill
        # instead of silently adding onto stale sums.
        self._acc_clean = True
        self._acc_depth = 0
        self._self_cleaning_acc = True
        # key-padding mask + embedding (+ PE, dropout) + the first encoder layer's pre-LayerNorm as one launch (kk_embed_ln_fwd): the
        # head of the critical path in front of the encoder forward is 3 dependent launches instead of 5
        self.fuse_enc_prologue = True
        # kk_rowdot_bwd (the predictors' / stop head's Linear(C -> 1) backward) leaves its weight-gradient sums as one plain row per
        # workgroup for the backward's single kk_partials_reduce instead of 256 workgroups' atomics on the same C + 1 addresses
        self.rowdot_partials = True
        # length-regulator gather + pitch / energy embedding adds + SpecAugment of the memory as one launch (kk_regulate_embed_fwd)
        self.fuse_memory_fwd = True
        # The zero-fill at the start of an accumulation cycle skips what the cycle's first grouped weight-gradient launches
        # overwrite (89 % of the arena at default dims; the fill runs beside the latency-bound encoder launch: 20 us of the step).
        # Which tensors those are is RECORDED from the launches of a step (per precision mode), never assumed, and a step that
        # zeroed by the record checks at its end that it overwrote exactly that set (_zero_grad_step / _grouped_wgrads).
        self.zero_skip_overwritten = True
        self._ow_sets: Dict[Tuple, frozenset] = {}
        self._ow_seen: Optional[set] = None
        self._ow_expect: Optional[frozenset] = None
        self._wgrad_queue = {}
        self._defer_wgrads = None                   # a list while a caller collects grouped weight-gradient launches for later
        # The gradient arena was zeroed for THIS micro-batch (first of an accumulation cycle): a layer's grouped weight
        # gradients are each written exactly once per micro-batch, so they overwrite instead of read-modify-write (dW is
        # 31 MB per decoder layer: a sixth of the grouped launch's traffic).  _first_micro, _external_sync: written by _micro_flags alone.
        self._grads_fresh = False
        self._first_micro = False
        # Text-encoder forward as one persistent launch (kk_encoder_stack_fwd): bf16 mode, phoneme sequences <= 128;
        # otherwise (and with KK_ENC_FUSED=0) the per-kernel sequence.  _enc_sync: its group-barrier words (word 0 != 0
        # = a barrier timed out; encoder_stack_error() reads it).
        self.enc_fused = True
        self.enc_fused_max_batch = 8                # one item per workgroup group (see _encoder_stack_ok)
        self.zero_late = True                       # gradient zero-fill after the decoder head's first launches
        self.enc_placement = 0                      # (tests force the groups across XCDs with 1)
        self._enc_sync = torch.zeros(512, dtype=torch.int32, device=self.device)
        self.enc_trace, self.enc_trace_wg = None, 0      # tools/probes/enc_stack_phases.py: per-phase clock stamps of one workgroup
        self.spec_augment_active = True             # the trainer clears it for epochs < spec_augment_start_epoch
        # KK_TRACE=1: one-thread time-stamp launches at the marks of a step (also inside the captured graphs), read back by
        # timeline() — the real overlap of the graph's branches, which rocprofv3 cannot show (it serialises them)
        self.trace = os.environ.get("KK_TRACE", "0") == "1"
        self._marks: Dict[str, int] = {}
        self._mark_buf = torch.zeros(512, dtype=torch.int64, device=self.device) if self.trace else None
        self.rng = torch.full((1,), int(seed) & 0x7FFFFFFF, dtype=torch.int32, device=self.device)   # step seed, read on device
        for n, b in spec.make_buffers(self.dims).items():
            self.arena.P[n].copy_(b)
        if init:
            self.load_params(spec.init_params(self.dims, seed))
        elif self.arena.ema is not None:
            self.arena.ema.copy_(self.arena.p)
        self.sync_shadow()

    @property
    def self_cleaning_acc(self) -> bool:
        return self._self_cleaning_acc

    @self_cleaning_acc.setter
    def self_cleaning_acc(self, on) -> None:
        if bool(on) != self._self_cleaning_acc:     # (the other mode's last reader did not leave the sums as this mode expects them)
            self._acc_clean = False
        self._self_cleaning_acc = bool(on)

    @contextlib.contextmanager
    def _acc_guard(self):
        """Around every sequence that writes and then cleans the handed-round accumulators (loss_acc in _fb; p_sumsq in
        optimizer_step; a graph capture / replay of either): restores the zero state first when an earlier sequence did not complete."""
        if self._acc_depth == 0:
            if not self._acc_clean:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the step's accumulators are not in their zero state inside a graph capture")
                self.loss_acc.zero_()
                self.grad_sumsq.zero_()
                self.p_sumsq.zero_()
            self._acc_clean = False
        self._acc_depth += 1
        try:
            yield
        except BaseException:
            self._acc_depth -= 1
            raise
        self._acc_depth -= 1
        if self._acc_depth == 0:
            self._acc_clean = True

    # ------------------------------------------------------------------ state
    def load_params(self, params: Dict[str, torch.Tensor], reset_ema: bool = True) -> None:
        for n in self.arena.param_names:
            self.arena.P[n].copy_(params[n].to(self.device, torch.float32).view(self.arena.shapes[n]))
        if reset_ema and self.arena.ema is not None:
            self.arena.ema.copy_(self.arena.p)      # EMA starts as a deep copy of the model (trainer.py:835)
        self.sync_shadow()

    @contextlib.contextmanager
    def fp32_math(self):
        """Run the enclosed calls in the fp32 parity mode (fp32 MFMA, fp32 storage, master weights) whatever the
        engine's training precision is — the reference validates without autocast (trainer.py:1821-1834)."""
        saved = (self.math, self.enc_dt, self.dec_dt, self.use_shadow)
        self.math, self.enc_dt, self.dec_dt, self.use_shadow = kk.KK_MATH_F32, torch.float32, torch.float32, False
        try:
            yield self
        finally:
            self.math, self.enc_dt, self.dec_dt, self.use_shadow = saved

    @contextlib.contextmanager
    def _no_dropout(self):
        """Run the enclosed launches with every dropout and stochastic-depth rate at 0 (_p, _dpr): the generate* methods."""
        saved, self.train_dropout = self.train_dropout, False
        try:
            yield self
        finally:
            self.train_dropout = saved

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the enclosed forward passes on the EMA replica (reference validation, trainer.py:1771-1790) by pointing the
        parameter views at the EMA slab — no copy, and nothing but two references to restore if the block raises.  Only
        meaningful without the bf16 weight shadow (combine with fp32_math())."""
        a = self.arena
        if a.ema is None:
            yield self
            return
        if self.use_shadow:
            raise RuntimeError("ema_weights(): the bf16 shadow holds the live weights; use it inside fp32_math()")
        saved = (a.P, a.p)
        a.P, a.p = a.E, a.ema
        try:
            yield self
        finally:
            a.P, a.p = saved

    def sync_shadow(self) -> None:
        """Rebuild the bf16 weight shadow from the fp32 master arena (after any write to arena.p from outside the
        optimizer kernels)."""
        if self.arena.p16 is not None:
            kk.call("kk_cast_f32_bf16", self.arena.p, self.arena.p16, self.arena.total)

    def state_dict(self, ema: bool = False) -> "OrderedDict[str, torch.Tensor]":
        """311 reference-named tensors (views of the arena; clone before mutating)."""
        src = self.arena.E if ema else self.arena.P
        return OrderedDict((n, src[n]) for n in spec.state_dict_order(self.dims))

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> None:
        want = set(spec.state_dict_order(self.dims))
        missing, unexpected = want - set(sd), set(sd) - want
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing={sorted(missing)} unexpected={sorted(unexpected)}")
        for n in want & set(sd):
            if tuple(sd[n].shape) != tuple(self.arena.shapes[n]):
                raise RuntimeError(f"size mismatch for {n}: {tuple(sd[n].shape)} vs {self.arena.shapes[n]}")
            self.arena.P[n].copy_(sd[n].to(self.device, torch.float32))
        self.sync_shadow()

    def grads(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((n, self.arena.G[n]) for n in self.arena.param_names)

    # ------------------------------------------------------------------ helpers
    @contextlib.contextmanager
    def _on_stream(self, stream, ns, enable=True, after=None):
        """Run the enclosed launches on `stream`, after everything already queued on the current stream (or, with
        `after`, after that earlier point of it: an event from _fork_point); the caller joins with _join(stream).
        Scratch ("tmp.*") buffers get the namespace `ns` so that streams never share one.
        With overlap off this is a no-op (same stream, same order).

        Under rocprofv3 the branch captured FIRST after a fork runs first and the other one starts late (the decoder
        backward appeared 1.1 ms after the losses when the encoder backward was captured before it), so the
        critical-path branch is captured first and the side branch afterwards, forked from an event recorded at the
        fork point.  Unprofiled, the step time is the same either way."""
        if not (self.overlap and enable):
            yield
            return
        saved, self._tmp_ns = self._tmp_ns, ns
        try:
            if after is not None:
                stream.wait_event(after)
            else:
                stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                yield
        finally:
            self._tmp_ns = saved

    def _on_side_stream(self, after=None):
        return self._on_stream(self._side, "side.", after=after)

    def _fork_point(self):
        """An event on the current stream that a later _on_stream(..., after=event) forks from."""
        if not self.overlap:
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def _comm_bucket(self, tag: str) -> None:
        """The gradients of bucket `tag` are final on the current stream from here on: exchange them on the comm stream."""
        c = self.dp_comm
        if c is None or not self._exchange_now:
            return
        # buckets travel in GROUPS (dp.BucketedExchange.groups): the bucket's event is recorded where it becomes final; when the last
        # bucket of a group has arrived the communication branch waits for all of the group's events and carries ONE exchange
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._comm_events.setdefault(c._group_of[tag], []).append(ev)
        tags = c.arrive(tag)
        if tags is None:
            return
        events = self._comm_events.pop(c._group_of[tag])
        for e in events:
            c.stream.wait_event(e)
        with torch.cuda.stream(c.stream):
            c.reduce_tags(self.arena.g, tags)

    def _comm_join(self) -> None:
        c = self.dp_comm
        if c is not None and self._exchange_now:
            torch.cuda.current_stream().wait_stream(c.stream)

    def _mark(self, name: str) -> None:
        if self.trace:
            idx = self._marks.setdefault(name, len(self._marks))
            kk.call("kk_timestamp", self._mark_buf[idx:])

    def timeline(self):
        """[(microseconds since the step's first mark, name)] of the last executed step (KK_TRACE=1), sorted by time."""
        if not self.trace:
            raise RuntimeError("timeline(): set KK_TRACE=1 before constructing the engine")
        t = self._mark_buf.cpu().tolist()
        rows = sorted((t[i], n) for n, i in self._marks.items() if t[i])
        return [((v - rows[0][0]) / 100.0, n) for v, n in rows]          # 100 MHz ticks

    def _join(self, stream) -> None:
        if self.overlap:
            torch.cuda.current_stream().wait_stream(stream)

    def _join_side(self) -> None:
        self._join(self._side)

    def _buf(self, key, *shape, dtype=torch.float32) -> torch.Tensor:
        """A [shape] view of the workspace buffer `key` (scratch names "tmp.*" are private to the current stream)."""
        if key.startswith("tmp."):
            key = self._tmp_ns + key
        vk = (key, shape, dtype)
        v = self._views.get(vk)
        if v is not None:
            return v
        need = math.prod(shape) * _ITEMSIZE[dtype]
        t = self._ws.get(key)
        if t is None or t.numel() < need:
            t = self._grow(key, need)
        v = t[:need].view(dtype).view(shape)
        if len(self._views) > 32768:
            self._views.clear()
        self._views[vk] = v
        return v

    def _grow(self, key: str, need: int) -> torch.Tensor:
        old = self._ws.get(key)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"workspace '{key}' would be allocated inside a graph capture (run the shape eagerly first)")
        if old is not None:
            # the old block may still be in use by queued kernels of any stream, and captured graphs / tables hold its
            # address: drain, drop them, then let it go.  12.5 % headroom so that slowly creeping shapes do not regrow
            # every step.
            torch.cuda.synchronize(self.device)
            self._invalidate()
            self.ws_bytes -= old.numel()
            need = need + need // 8
        need = (need + 255) // 256 * 256
        t = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._ws[key] = t
        self.ws_bytes += need
        return t

    def _invalidate(self) -> None:
        """Forget everything that holds workspace addresses: views, descriptor tables, captured graphs."""
        self._views.clear()
        self._ops.clear()
        self._tables.clear()
        self._graphs.clear()
        self.ws_generation += 1

    def _table(self, key: Tuple, build):
        """Descriptor table cache (pointer / weight-gradient / head-norm / reduction tables), LRU-bounded.  A captured graph
        reads device-resident tables when it replays, so evicting tables also drops the graphs."""
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) >= self.max_tables:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("descriptor-table cache overflow inside a graph capture")
                torch.cuda.synchronize(self.device)
                self._graphs.clear()
                self.ws_generation += 1                    # (a graph held outside _graphs checks this: generate_stream)
                for _ in range(self.max_tables // 4):
                    self._tables.popitem(last=False)
            t = self._tables[key] = build()
        else:
            self._tables.move_to_end(key)
        return t

    def workspace_bytes(self) -> int:
        """Bytes held by the activation workspace (bounded by the largest batch seen, not by the number of shapes)."""
        return self.ws_bytes

    def _rope_tables(self, S: int):
        """cos / sin tables for positions [0, S): prefixes of one pair built once for the longest supported sequence
        (2 x max_len x 64 floats), so their addresses never change under captured graphs."""
        if not self._rope:
            c, s = spec.rope_tables(self.dims.max_len, 64)
            self._rope[0] = (c.to(self.device), s.to(self.device))
        if S > self.dims.max_len:
            raise ValueError(f"sequence of {S} positions exceeds the positional table ({self.dims.max_len})")
        c, s = self._rope[0]
        return c[:S], s[:S]

    def _W(self, name: str) -> torch.Tensor:
        """GEMM weight operand: the bf16 shadow when there is one, else the fp32 master."""
        if self.use_shadow and self.arena.shapes[name][-1] % 8 == 0:      # bf16 rows are fetched 8 elements at a time
            return self.arena.P16[name]
        return self.arena.P[name]

    def _Wconv(self, name: str, rows: int, cols: int) -> torch.Tensor:
        """Conv1d(k=3) weight [C_out, C_in, 3] as the [C_out, 3*C_in] operand of the unfolded GEMM: the bf16 shadow when the
        row length allows 16-byte fetches (the shape's last dim is 3, so _W would fall back to the fp32 master)."""
        if self.use_shadow and cols % 8 == 0:
            return self.arena.P16[name].view(rows, cols)
        return self.arena.P[name].view(rows, cols)

    def _Wf(self, first: str, count: int) -> torch.Tensor:
        a = self.arena
        return a.fused(a.p16 if self.use_shadow else a.p, first, count)

    def _linear(self, x, W, b, out, res=None, res_mod=0, split_k=0):
        N, K = x.shape
        M = W.shape[0]
        # split_k = 0: kk_gemm splits K (fp32 atomics) by itself when the tile grid is too small to fill the chip
        # (split_k = 1, _stream_step: one slice, no atomics, so that a replayed step repeats its bits)
        kk.call("kk_gemm", 0, 0, N, M, K, 1.0, x, x.stride(0), W, K, 0.0, out, out.stride(0), b, res,
                res.stride(0) if res is not None else 0, res_mod, split_k, self.math, _b16(x) | _b16(W) << 1 | _b16(out) << 2)

    def _dgrad(self, dy, W, dx, beta=0.0):
        N, M = dy.shape
        K = W.shape[1]
        kk.call("kk_gemm", 0, 1, N, K, M, 1.0, dy, dy.stride(0), W, K, beta, dx, dx.stride(0), None, None, 0, 0, 0, self.math,
                _b16(dy) | _b16(W) << 1 | _b16(dx) << 2)

    def _wgrad(self, dy, x, dW, db=None):
        N, M = dy.shape
        K = x.shape[1]
        q = self._wgrad_queue.get(self._tmp_ns)
        if q is not None and db is None and _b16(dy) and _b16(x) and self.math == kk.KK_MATH_BF16:
            q.append((dy, x, dW))                        # issued with the rest of the layer's weight gradients
            return
        kk.call("kk_gemm", 1, 1, M, K, N, 1.0, dy, dy.stride(0), x, x.stride(0), 1.0, dW, K, None, None, 0, 0, 0, self.math,
                _b16(dy) | _b16(x) << 1)
        if db is not None:
            kk.call("kk_colsum_acc", dy, dy.stride(0), N, M, db, _b16(dy))

    @contextlib.contextmanager
    def _grouped_wgrads(self):
        """Weight-gradient GEMMs issued inside the block (one layer's backward) are queued and run as ONE grouped launch
        at its end: nothing reads a weight gradient before the optimizer, and together they fill the chip with
        full-length reductions (no split-K atomics).  Their operands — the saved activations and the layer's own
        gradient buffers — are not rewritten before the next layer's backward starts."""
        ns = self._tmp_ns
        if not self.group_wgrads or ns in self._wgrad_queue:
            yield
            return
        q = self._wgrad_queue[ns] = []
        try:
            yield
        finally:
            del self._wgrad_queue[ns]
        if self._defer_wgrads is not None:               # (the caller issues this group later, elsewhere: _issue_wgrad_group)
            self._defer_wgrads.append(q)
            return
        self._issue_wgrad_group(q)

    def _issue_wgrad_group(self, q) -> None:
        for i in range(0, len(q), 8):
            part = q[i:i + 8]
            sig = ("wg",) + tuple((dy.data_ptr(), x.data_ptr(), dw.data_ptr(), tuple(dy.shape), tuple(x.shape)) for dy, x, dw in part)
            table = self._table(sig, lambda: kk.wgrad_table(part))
            st = self._ss_step
            if st is None:
                kk.call("kk_gemm_wgrad_group", table, len(part), 0, 1 if self._grads_fresh else 0, None, None, None)
            else:
                # (one GPU) the tiles of a launch that writes every element once also leave the sums of squares of what they stored as
                # records of kk_seg_sumsq's workspace: the optimizer's norm pass then skips those tensors (the library decides per launch
                # and says so by advancing the count)
                segs, flat = [], []
                for _, _, dw in part:
                    si = self._seg_of_ptr.get(dw.data_ptr())
                    if si is None:
                        segs = None
                        break
                    rows = self.arena.shapes[self.arena.names[si]][0]
                    cnt = dw.shape[0] // rows                  # (fused q|k|v / k|v views: `cnt` adjacent segments of `rows` rows each)
                    if dw.shape[0] % rows or any(self.arena.shapes[self.arena.names[si + c]] != self.arena.shapes[self.arena.names[si]] for c in range(cnt)):
                        segs = None
                        break
                    segs.extend(range(si, si + cnt))
                    flat.extend((si, rows if cnt > 1 else 0))
                n0 = st["count"].value
                if segs is None or n0 + 1024 > st["cap"]:
                    kk.call("kk_gemm_wgrad_group", table, len(part), 0, 1 if self._grads_fresh else 0, None, None, None)
                else:
                    seg_arr = (kk.C.c_int32 * len(flat))(*flat)
                    kk.call("kk_gemm_wgrad_group", table, len(part), 0, 1 if self._grads_fresh else 0, st["rec"], seg_arr, kk.C.byref(st["count"]))
                    if st["count"].value != n0:
                        st["covered"].update(segs)
            if self._grads_fresh and self._ow_seen is not None:
                self._ow_seen.update((dw.data_ptr(), dw.numel()) for _, _, dw in part)

    def _ln_out(self, ln, rows, H):
        """(gamma, beta, y, mean, rstd) of the LayerNorm ln = (workspace key, parameter prefix, dtype of y) over [rows, H]: the one
        place that spells the ".y" / ".mean" / ".rstd" keys.  None gives five Nones (a sub-layer tail that no LayerNorm follows); a
        bare key gives the saved statistics alone (the backward, which holds the parameters and the input itself)."""
        if ln is None:
            return None, None, None, None, None
        if isinstance(ln, str):
            return None, None, None, self._buf(ln + ".mean", rows), self._buf(ln + ".rstd", rows)
        key, prefix, dtype = ln
        P = self.arena.P
        return (P[prefix + ".weight"], P[prefix + ".bias"], self._buf(key + ".y", rows, H, dtype=dtype), self._buf(key + ".mean", rows),
                self._buf(key + ".rstd", rows))

    def _ln_fwd(self, key, x, prefix, dtype=torch.float32):
        rows, H = x.shape
        g, b, y, mean, rstd = self._ln_out((key, prefix, dtype), rows, H)
        kk.call("kk_layernorm_fwd", x, g, b, y, mean, rstd, rows, H, _b16(y))
        return y

    def _partials(self, key, rows, H, ncols, dst0, dst1, split):
        """Per-workgroup column partial sums of a norm backward, summed into the gradient vectors by the single
        kk_partials_reduce launch at the end of the backward pass (instead of device-scope atomics per workgroup)."""
        nb = kk.load().kk_norm_bwd_blocks(rows, H)
        part = self._buf(key + ".part", nb, ncols)
        self._reduce_lists[self._tmp_ns].append((part, dst0, dst1, nb, ncols, split))
        return part

    def _rowdot_partials(self, key, rows, C, dw, db):
        """[blocks][C + 4] partial (dw | db) rows of one kk_rowdot_bwd launch, summed by the backward's kk_partials_reduce — or None
        (same-address atomics inside the launch) when C is not a multiple of 4."""
        if C % 4 or not self.rowdot_partials:
            return None
        nb = kk.load().kk_rowdot_bwd_blocks(rows)
        part = self._buf(key + ".rdpart", nb, C + 4)
        self._reduce_lists[self._tmp_ns].append((part, dw.view(-1), db.view(-1), nb, C + 1, C, C + 4))
        return part

    def _headnorm_partials(self, key, rows, dgains):
        """[parts][blocks][64] partial gain gradients of one head-norm backward launch, one reduce descriptor per part."""
        nb = kk.load().kk_headnorm_bwd_blocks(rows, self.dims.heads)
        part = self._buf(key + ".hpart", len(dgains), nb, 64)
        for j, dg in enumerate(dgains):
            self._reduce_lists[self._tmp_ns].append((part[j], dg, None, nb, 64, 64))
        return part

    def _ln_bwd(self, key, dy, x, prefix, dx, accumulate):
        P, G = self.arena.P, self.arena.G
        rows, H = x.shape
        part = self._partials(key, rows, H, 2 * H, G[prefix + ".weight"], G[prefix + ".bias"], H)
        *_, mean, rstd = self._ln_out(key, rows, H)
        kk.call("kk_layernorm_bwd", dy, x, P[prefix + ".weight"], mean, rstd, dx, 1 if accumulate else 0, G[prefix + ".weight"],
                G[prefix + ".bias"], part, rows, H, _b16(dy))

    def _tail_bwd(self, key, dn, x, prefix, dres, accumulate, head) -> None:
        """Backward of LayerNorm `key` (input x = the residual stream after the sub-layer `head`), fused — when that
        sub-layer ran its dropout tail — with the head of the sub-layer's own backward (kk_sublayer_in_bwd): masks,
        RMSNorm backward for an FFN, bias column sums.  head = (kind, ffn_key, prefix, S, site, p, dpr, dtype).
        The sub-layer's backward then starts from the prepared buffers (tmp.df2 / tmp.d_attn_proj)."""
        kind, hkey, hprefix, S, site, p, dpr, dt = head
        P, G = self.arena.P, self.arena.G
        rows, H = x.shape
        nb = kk.load().kk_sublayer_in_bwd_blocks(rows)
        part = self._buf(key + ".tpart", nb, 4 * H)
        self._reduce_lists[self._tmp_ns].append((part, G[prefix + ".weight"], G[prefix + ".bias"], nb, 2 * H, H, 4 * H))
        if kind == "ffn":
            f2, gain = self._buf(hkey + ".f2", rows, H, dtype=dt), P[hprefix + ".output_norm.weight"]
            rstd_f, dy = self._buf(hkey + ".rstd_f", rows), self._buf("tmp.df2", rows, H, dtype=dt)
            self._reduce_lists[self._tmp_ns].append((part[:, 2 * H:], G[hprefix + ".linear2.bias"], G[hprefix + ".output_norm.weight"], nb, 2 * H, H, 4 * H))
            p2 = p
        else:
            f2 = gain = rstd_f = None
            dy = self._buf("tmp.d_attn_proj" + (".x" if hprefix.endswith(".cross_attn") else ""), rows, H, dtype=dt)
            self._reduce_lists[self._tmp_ns].append((part[:, 2 * H:], G[hprefix + ".w_o.bias"], None, nb, H, H, 4 * H))
            p2 = 0.0
        *_, mean, rstd = self._ln_out(key, rows, H)
        kk.call("kk_sublayer_in_bwd", dn, _b16(dn), x, P[prefix + ".weight"], mean, rstd, dres, 1 if accumulate else 0, f2, gain, rstd_f,
                dy, _b16(dy), part, rows, H, S, self.rng, site, p, site + 1, p2, site + 2, dpr)

    def _reduce_partials(self, shape_key) -> None:
        """One launch that adds the column sums of every partial matrix written so far (by streams already joined into
        the current one) to its gradient vectors."""
        todo = [e for ns in ("side.", "kv.", "") for e in self._reduce_lists[ns]]
        for ns in self._reduce_lists:
            self._reduce_lists[ns] = []
        if not todo:
            return
        tkey = ("red", shape_key, tuple((e[0].data_ptr(), e[3]) for e in todo))      # which partial matrices this pass wrote
        # workspace addresses are stable while no buffer grows: the table is built once per batch shape
        ent = self._table(tkey, lambda: (kk.reduce_table(todo, self.device), len(todo), max(e[4] for e in todo)))
        kk.call("kk_partials_reduce", ent[0], ent[1], ent[2])

    # ------------------------------------------------------------------ dropout plumbing
    def _p(self, rate: float) -> float:
        return float(rate) if self.train_dropout else 0.0

    def _dpr(self, i: int, n: int) -> float:
        """Stochastic-depth rate of layer i of n (model.py:100-107)."""
        if not (self.train_dropout and self.hp.use_stochastic_depth):
            return 0.0
        return (i / max(n - 1, 1)) * self.hp.stochastic_depth_rate

    def _sublayer_tail(self, y, x_res, x_out, S, site, p, dpr, p2, gain, rstd_f, next_ln):
        """Fused tail of a sub-layer on the dropout path (kk_sublayer_out_fwd): x_out = x_res + masks * [RMSNorm](y), and
        the LayerNorm `next_ln = (key, prefix, dtype)` of x_out when the caller names one; returns that LayerNorm's
        output (else None)."""
        rows, H = y.shape
        g, b, n, mean, rstd = self._ln_out(next_ln, rows, H)
        kk.call("kk_sublayer_out_fwd", y, _b16(y), gain, rstd_f, x_res, x_out, g, b, n, _b16(n), mean, rstd, rows, H, S, self.rng,
                site, p, site + 1, p2, site + 2, dpr)
        return n

    # ------------------------------------------------------------------ attention sub-layer
    def _attn_fwd(self, key, prefix, xq, xkv, B, Sq, Sk, rope, causal, key_mask, x_res, x_out, site=0, p=0.0, dpr=0.0, next_ln=None,
                  layer=0):
        """x_out = x_res + w_o(attention(...)) + b_o.  xq [B*Sq,H] (post-LN), xkv [B*Sk,H] (None = self-attention).
        Returns LayerNorm_next_ln(x_out) when the fused dropout tail computed it, else None."""
        h, own_kv = self.dims.heads, xkv is None      # own_kv: q|k|v from one fused projection; RoPE on q and k only
        i16 = _b16(xq)
        cos, sin = self._rope_tables(max(Sq, Sk)) if rope and own_kv else (None, None)
        o = self._attn_ops(key, prefix, xq, xkv, B, Sq, Sk, layer)
        # (cross-attention: the K|V slices were filled by _cross_kv_fwd_all)
        self._proj_headnorm(xq, self._attn_wq(prefix, xkv), o.raw, o.nrm, Sq, o.gains[:3 if own_kv else 1],
                            3 if cos is not None else 0, cos, sin)
        keep = self._attn_keep(key, B, Sq, Sk, p, i16)
        if (self.attn_warm & 3) and i16 and key.startswith("dec") and self.use_shadow:
            # the forward warms the weights of the GEMMs behind it into every XCD's L2 (kk_attn_warm_next): its own output projection, and
            # (bit 1) the next sub-layer's first matrix (cross-attention: w_q; feed-forward: linear1)
            base = prefix.rsplit(".", 1)[0]                # "decoder.layers.<i>"
            nxt = base + (".cross_attn.w_q.weight" if own_kv else ".ff.linear1.weight")
            self._attn_warm(self._W(prefix + ".w_o.weight"), self._W(nxt), bool(self.attn_warm & 2))
        # with keep bits the forward stores the dropout keep decisions (1 bit per score) for the backward's pair launch (_kb), or reads
        # them where kk_attn_keep_gen has written them already (_rb)
        name = "kk_attn_fwd" if keep is None else "kk_attn_fwd_rb" if key in self._keep_ready else "kk_attn_fwd_kb"
        self._attn_launch(name, o, B, h, Sq, Sk, key_mask, causal, site + 3, p, own=() if keep is None else (keep,))
        return self._attn_out(key, prefix, o.ctx, B * Sq, Sq, x_res, x_out, site, p, dpr, next_ln)

    def _attn_ops(self, key, prefix, xq, xkv, B, Sq, Sk, layer=0, grads=False, kv_grads=True) -> _AttnOps:
        """The operand views of attention sub-layer `key` (self-attention: xkv None; cross-attention: decoder layer `layer`), with
        grads also those of its backward — dK / dV of cross-attention only with kv_grads (the K/V branch: _cross_kv_bwd_all)."""
        dt = xq.dtype                                   # storage of every activation of the sub-layer
        # built once per shape and stream namespace (the "tmp." keys): the views stay what they are until a workspace buffer moves
        # (_invalidate drops the records with the views), and slicing them anew per call was most of a launch's host time
        memo = (self._tmp_ns, key, prefix, dt, xkv is None, B, Sq, Sk, layer, grads, kv_grads)
        o = self._ops.get(memo)
        if o is not None:
            return o
        P, G, H, h = self.arena.P, self.arena.G, self.dims.hidden, self.dims.heads
        Nq, Nk = B * Sq, B * Sk
        norms = [f"{prefix}.{c}_norm.weight" for c in "qkv"]
        if xkv is None:
            raw, nrm = self._buf(key + ".qkv_raw", Nq, 3 * H, dtype=dt), self._buf(key + ".qkv_n", Nq, 3 * H, dtype=dt)
            kv_raw, k_raw, v_raw, k_n, v_n = None, raw[:, H:], raw[:, 2 * H:], nrm[:, H:], nrm[:, 2 * H:]
        else:
            raw, nrm = self._buf(key + ".q_raw", Nq, H, dtype=dt), self._buf(key + ".q_n", Nq, H, dtype=dt)
            kv_raw, kv_n = self._cross_kv(layer, Nk, dt)
            k_raw, v_raw, k_n, v_n = kv_raw, kv_raw[:, H:], kv_n, kv_n[:, H:]
        o = _AttnOps(nrm, k_n, v_n, self._buf(key + ".ctx", Nq, H, dtype=dt), self._buf(key + ".lse", B, h, Sq),
                     q_raw=raw, k_raw=k_raw, v_raw=v_raw, gains=tuple(P[n] for n in norms), raw=raw, nrm=nrm, kv_raw=kv_raw)
        if grads:
            # cross-attention: dctx / delta are read by the K/V branch on its own stream, so each layer keeps its own
            ck = "tmp" if xkv is None else key
            dk_n = dv_n = dk_raw = dv_raw = dkv_n = dkv_raw = None
            if xkv is None:
                dn, draw = self._buf("tmp.dqkv_n", Nq, 3 * H, dtype=dt), self._buf("tmp.dqkv_raw", Nq, 3 * H, dtype=dt)
                dk_n, dv_n, dk_raw, dv_raw = dn[:, H:], dn[:, 2 * H:], draw[:, H:], draw[:, 2 * H:]
            else:
                dn, draw = self._buf("tmp.dq_n", Nq, H, dtype=dt), self._buf("tmp.dq_raw", Nq, H, dtype=dt)
                if kv_grads:
                    dkv_raw, dkv_n = self._cross_kv(layer, Nk, dt, "d")
                    dk_n, dv_n, dk_raw, dv_raw = dkv_n, dkv_n[:, H:], dkv_raw, dkv_raw[:, H:]
            o = o._replace(dgains=tuple(G[n] for n in norms), dctx=self._buf(ck + ".dctx", Nq, H, dtype=dt),
                           d_out=self._buf("tmp.d_attn_proj" + ("" if xkv is None else ".x"), Nq, H, dtype=dt),
                           delta=self._buf(ck + ".delta", B, h, Sq), dn=dn, draw=draw, dq_n=dn, dk_n=dk_n, dv_n=dv_n,
                           dq_raw=draw, dk_raw=dk_raw, dv_raw=dv_raw, dkv_n=dkv_n, dkv_raw=dkv_raw)
        if len(self._ops) >= 4096:                      # (dynamic batching: every new shape adds its records)
            self._ops.clear()
        self._ops[memo] = o
        return o

    def _attn_wq(self, prefix, xkv):
        """Weight operand of the sub-layer's own projection: q|k|v fused (self-attention) or q alone."""
        return self._Wf(prefix + ".w_q.weight", 3) if xkv is None else self._W(prefix + ".w_q.weight")

    def _attn_launch(self, name, o, B, h, Sq, Sk, key_mask, causal, site, p, outs=(), own=()):
        """Every kk_attn_* launch of the engine, their positional order written once: the operands of `o`, the problem, the row strides,
        the mask ... storage tail.  The forward entry points (no outs) write o.ctx and o.lse; the backward ones read o.dctx, o.lse
        and o.delta and write `outs` (dQ | dK, dV | all three).  own: what only this entry point takes, in its order — keep bits;
        the head-norm tables; ctx and its stride (kk_attn_bwd_dq); the dS workspace and its size (kk_attn_bwd_ws).  B, h: the
        decode step passes 1 and B * heads over its time-major caches."""
        mid = (o.dctx, o.lse, o.delta, *outs) if outs else (o.ctx, o.lse)
        kk.call(name, o.q_n, o.k_n, o.v_n, *mid, B, h, Sq, Sk, o.q_n.stride(0), o.k_n.stride(0), o.v_n.stride(0), mid[0].stride(0),
                *[t.stride(0) for t in outs], key_mask, 1 if causal else 0, 0.125, self.rng, site, p, self.math, _b16(o.q_n), *own)

    def _attn_warm(self, w0, w1=None, second=True):
        """kk_attn_warm_next: the next attention forward or pair launch of this thread touches the lines of w0 (and w1) so that the
        GEMMs behind it find them in L2.  second=False names w1 by its size alone, which the library reads as "w0 only"."""
        kk.load().kk_attn_warm_next(w0.data_ptr(), w0.numel() * w0.element_size(), w1.data_ptr() if w1 is not None and second else None,
                                    w1.numel() * w1.element_size() if w1 is not None else 0)

    def _attn_out(self, key, prefix, ctx, Nq, Sq, x_res, x_out, site, p, dpr, next_ln, split_k=0):
        """The output projection and residual tail of an attention sub-layer: x_out = x_res + w_o(ctx) + b_o, and LayerNorm_next_ln."""
        P, H = self.arena.P, self.dims.hidden
        dt, i16 = ctx.dtype, _b16(ctx)
        # the projection output lives only until the tail two launches later: in the decoder's bf16 mode it is stored like every
        # other GEMM result there (what autocast gives the reference's nn.Linear); the text encoder keeps fp32 (its persistent
        # launch hands the tile over in fp32, and the per-kernel path must match it)
        Wo = self._W(prefix + ".w_o.weight")
        p16 = self.attn_proj_bf16 and i16 and key.startswith("dec")
        if (p16 and self.fuse_linear_tail and _b16(Wo) and self.math == kk.KK_MATH_BF16 and kk.load().kk_linear_tail_pays(Nq, H, H)):
            # projection + tail as ONE row-owner launch (kk_linear_tail_fwd: same bits as the two launches below)
            g, b, n, mean, rstd = self._ln_out(next_ln, Nq, H)
            kk.call("kk_linear_tail_fwd", ctx, ctx.stride(0), Wo, P[prefix + ".w_o.bias"], H, None, 1, None, None, x_res, x_out, g, b, n,
                    _b16(n), mean, rstd, Nq, H, Sq, self.rng, site, p, site + 1, 0.0, site + 2, dpr)
            return n
        proj = self._buf("tmp.attn_proj16" if p16 else "tmp.attn_proj", Nq, H, dtype=dt if p16 else torch.float32)
        self._linear(ctx, Wo, P[prefix + ".w_o.bias"], proj, split_k=split_k)
        return self._sublayer_tail(proj, x_res, x_out, Sq, site, p, dpr, 0.0, None, None, next_ln)   # (p = 0: masks are all ones)

    def _attn_keep(self, key, B, Sq, Sk, p, i16):
        """Buffer of the attention sub-layer's packed dropout keep decisions (kk_attn_fwd_kb writes, kk_attn_bwd_kb reads: the backward
        then spends no vector instructions on the mask hash), or None where the library stores none (short sequences, fp32 storage,
        no dropout) or the switch is off."""
        if not (self.attn_keep_bits and i16 and p > 0.0):
            return None
        n = kk.load().kk_attn_keep_bytes(B, self.dims.heads, Sq, Sk)
        return self._buf(key + ".keep", n, dtype=torch.uint8) if n > 0 else None

    def _keep_gen_launch(self, B, T, p_dec, seed_offset=0, mark_ready=True, max_wgs=0, layers=None) -> bool:
        """kk_attn_keep_gen for every decoder attention launch of a (B, T) step; False when that shape has no keep-bit arrays."""
        d, ents = self.dims, []
        for li in range(d.dec_layers if layers is None else min(layers, d.dec_layers)):
            lay = self._dec_layer(li)
            for sub, cz in (("sa", True), ("ca", False)):
                kb = self._attn_keep(f"{lay.key}.{sub}", B, T, T, p_dec, 1)
                if kb is not None:
                    ents.append((kb, lay.site[sub] + 3, p_dec, B, d.heads, T, T, cz))      # (+ 3: the attention kernels' own offset)
                    if mark_ready:
                        self._keep_ready.add(f"{lay.key}.{sub}")
        for c0 in range(0, len(ents), 16):
            part = ents[c0:c0 + 16]
            table = self._table(("keepgen",) + tuple((e[0].data_ptr(), e[1], e[2], B, T) for e in part), lambda part=part: kk.keep_sites(part))
            kk.call("kk_attn_keep_gen", table, len(part), self.rng, seed_offset, max_wgs)
        return bool(ents)

    def _cross_kv(self, layer, Nk, dt, which="", ns=""):
        """(raw, normed) K|V of cross-attention layer `layer`: column slices [.., 2H] of the all-layer buffers (row stride
        layers*2H); which = "d" for their gradients; ns = a key prefix of the buffers (generate_batch: its own)."""
        H = self.dims.hidden
        raw, nrm = self._cross_kv_all(Nk, dt, which, ns)
        return raw[:, 2 * H * layer:2 * H * (layer + 1)], nrm[:, 2 * H * layer:2 * H * (layer + 1)]

    def _cross_kv_all(self, Nk, dt, which="", ns=""):
        """The all-layer buffers themselves: (raw, normed) K|V of every cross-attention layer, [Nk, layers * 2H]."""
        W = 2 * self.dims.hidden * self.dims.dec_layers
        return self._buf(f"{ns}dec.ca.{which}kv_raw_all", Nk, W, dtype=dt), self._buf(f"{ns}dec.ca.{which}kv_n_all", Nk, W, dtype=dt)

    def _proj_headnorm(self, x, W, raw, nrm, S, gains, rope_mask, cos, sin, split_k=0):
        """raw = x.W^T (an attention projection of len(gains) parts x heads x 64 columns, no bias: transformers.py:131-136)
        and nrm = its per-head RMSNorm (+ RoPE): in bf16 mode one GEMM whose epilogue normalises, else GEMM + norm launches."""
        H, h = self.dims.hidden, self.dims.heads
        rows, parts = x.shape[0], len(gains)
        if self.fuse_headnorm and _b16(x) and _b16(W) and _b16(raw) and parts <= 12 and x.shape[1] % 64 == 0:
            table = self._table(("ptr",) + tuple(g.data_ptr() for g in gains), lambda: kk.pointer_table(gains))
            kk.call("kk_gemm_qkv_headnorm", rows, parts, h, x.shape[1], x, x.stride(0), W, None, raw, raw.stride(0), nrm,
                    nrm.stride(0), S, table, rope_mask, cos, sin)
            return
        self._linear(x, W, None, raw, split_k=split_k)
        for p0 in range(0, parts, 3):                      # the norm kernel takes up to three parts per launch
            g = list(gains[p0:p0 + 3]) + [None] * 3
            n = min(3, parts - p0)
            kk.call("kk_headnorm_rope_fwd", raw[:, p0 * H:], raw.stride(0), nrm[:, p0 * H:], nrm.stride(0), rows, h, S, n,
                    g[0], g[1], g[2], (rope_mask >> p0) & 7, cos, sin, _b16(raw))

    def _cross_kv_fwd_all(self, xkv, Nk, Sk, dt, first=0, last=None, ns=""):
        """K/V projections of ALL decoder cross-attention layers in one GEMM (they depend on the memory alone and their
        weights are contiguous in the arena), then the per-head RMSNorm of each layer's slice (no RoPE:
        transformers.py:268-277 applies it to self-attention only)."""
        P, H, h, L = self.arena.P, self.dims.hidden, self.dims.heads, self.dims.dec_layers
        raw_all, nrm_all = self._cross_kv_all(Nk, dt, ns=ns)
        last = L if last is None else last                 # layers [first, last): a column slice of the all-layer buffers
        gains = [P[f"decoder.layers.{l}.cross_attn.{kv}_norm.weight"] for l in range(first, last) for kv in ("k", "v")]
        c0, c1 = 2 * H * first, 2 * H * last
        self._proj_headnorm(xkv, self._Wf(f"decoder.layers.{first}.cross_attn.w_k.weight", 2 * (last - first)), raw_all[:, c0:c1],
                            nrm_all[:, c0:c1], Sk, gains, 0, None, None)

    def _cross_kv_bwd_all(self, xkv, Nk, dt, d_xkv, wgrad=True, dgrad=True):
        """Weight gradient of all layers' K/V projections and the memory gradient: two GEMMs over the all-layer buffer."""
        a, L = self.arena, self.dims.dec_layers
        draw_all, _ = self._cross_kv_all(Nk, dt, "d")     # (what every layer's _attn_bwd wrote its slice of)
        if wgrad:
            with self._grouped_wgrads():                # (a group of one — the 128x64-tile, full-reduction launch — or a member of the
                self._wgrad(draw_all, xkv, a.fused(a.g, "decoder.layers.0.cross_attn.w_k.weight", 2 * L))   # caller's open group)
        if dgrad:
            self._dgrad(draw_all, self._Wf("decoder.layers.0.cross_attn.w_k.weight", 2 * L), d_xkv)

    def _attn_bwd(self, key, prefix, d_out, xq, xkv, B, Sq, Sk, rope, causal, key_mask, d_xq, d_xkv, d_xkv_beta,
                  site=0, p=0.0, dpr=0.0, layer=0):
        """Given d_out = dL/d(sub-layer output, pre-residual), accumulate parameter grads, write d_xq (dL/d xq) and,
        for cross-attention, d_xkv (+= when d_xkv_beta == 1)."""
        a, G, H, h, own_kv = self.arena, self.arena.G, self.dims.hidden, self.dims.heads, xkv is None
        Nq, Nk, i16 = B * Sq, B * Sk, _b16(xq)
        kv_branch = own_kv or d_xkv is not None           # (cross-attention: its two GEMMs run once for all layers, _cross_kv_bwd_all)
        cos, sin = self._rope_tables(max(Sq, Sk)) if rope and own_kv else (None, None)
        o = self._attn_ops(key, prefix, xq, xkv, B, Sq, Sk, layer, grads=True, kv_grads=kv_branch)
        # _tail_bwd (the fused LayerNorm backward before this call) already wrote the masked gradient of the projection
        # output and the column sums for w_o.bias
        d_out = o.d_out
        self._wgrad(d_out, o.ctx, G[prefix + ".w_o.weight"], None)
        Wo = self._W(prefix + ".w_o.weight")
        # Delta = rowsum(dctx * ctx): from the epilogue of this GEMM when the pair launch below takes it as an input, else computed
        # by the dQ kernel from fragments it holds anyway (and read by the dK/dV kernel launched after it)
        pair = bool(self.attn_bwd_pair and self.fuse_headnorm_bwd and i16 and _b16(d_out) and _b16(Wo) and kv_branch
                    and min(Sq, Sk) > self.attn_pair_min_seq and kk.load().kk_gemm_dgrad_delta_supported(Nq, H, H))
        if pair:
            kk.call("kk_gemm_dgrad_delta", Nq, H, H, d_out, d_out.stride(0), Wo, Wo.shape[1], o.dctx, o.dctx.stride(0), o.ctx,
                    o.ctx.stride(0), o.delta, Sq, h)
        else:
            self._dgrad(d_out, Wo, o.dctx)
        # where dQ, dK and dV land: the raw projections' gradients, the head norms' backward being the epilogue of the attention
        # backward kernels (their tables: RoPE on q and k of self-attention), or the normed ones, with kk_headnorm_rope_bwd behind
        epi = pair or self.fuse_headnorm_bwd
        (gq, gk, gv), (dgq, dgk, dgv) = o.gains, o.dgains
        dq, dk, dv = (o.dq_raw, o.dk_raw, o.dv_raw) if epi else (o.dq_n, o.dk_n, o.dv_n)
        hq = self._hn_table(key, "q", B, Sq, [(o.q_raw, gq, dgq, cos, sin)]) if epi else None
        hkv = None
        if epi and kv_branch:      # (built before the dQ launch also where dK / dV have a launch of their own: same table, same order)
            hkv = self._hn_table(key, "kv", B, Sk, [(o.k_raw, gk, dgk, cos, sin), (o.v_raw, gv, dgv, None, None)])
        launch = (o, B, h, Sq, Sk, key_mask, causal, site + 3, p)
        if pair and self.attn_two_pass and kk.load().kk_attn_bwd_two_pass(B, h, Sq, Sk, 1 if causal else 0):
            # where the library says the shape pays (no shape at present, see there): the dK/dV kernel also stores dS, and a dQ pass
            # without softmax work reads it from this stream's workspace (2 bytes per score; "tmp.": private to the stream)
            need = kk.load().kk_attn_bwd_ws_bytes(B, h, Sq, Sk)
            self._attn_launch("kk_attn_bwd_ws", *launch, (dq, dk, dv), (hq, hkv, self._buf("tmp.attn_dS", need, dtype=torch.uint8), need))
        elif pair:         # dQ | dK, dV in one launch
            keep = self._attn_keep(key, B, Sq, Sk, p, i16)          # (the buffer the forward of this sub-layer filled)
            if (self.attn_warm & 12) and i16 and key.startswith("dec") and self.use_shadow:
                # the dQ half of the pair launch warms the weights of the dgrad GEMM(s) behind it, and (bit 3, from the cross-attention)
                # the self-attention's output projection, whose dgrad comes after the tail behind that
                w1 = self._W(prefix.rsplit(".", 1)[0] + ".self_attn.w_o.weight") if self.attn_warm & 8 and not own_kv else None
                self._attn_warm(self._attn_wq(prefix, xkv), w1)
            self._attn_launch("kk_attn_bwd" if keep is None else "kk_attn_bwd_kb", *launch, (dq, dk, dv),
                              (hq, hkv) if keep is None else (hq, hkv, keep))
        else:
            self._attn_launch("kk_attn_bwd_dq", *launch, (dq,), (o.ctx, o.ctx.stride(0), hq))      # also writes delta
            if kv_branch:
                self._attn_launch("kk_attn_bwd_dkv", *launch, (dk, dv), (hkv,))
        if not epi:        # self-attention: one 3-part launch; cross-attention: K|V (if that branch runs), then q
            if kv_branch and not own_kv:
                self._headnorm_bwd(key + ".kv", o.dkv_n, o.kv_raw, o.dkv_raw, Nk, Sk, (gk, gv), (dgk, dgv), 0, None, None)
            n = 3 if own_kv else 1
            self._headnorm_bwd(key if own_kv else key + ".q", o.dn, o.raw, o.draw, Nq, Sq, o.gains[:n], o.dgains[:n],
                               3 if cos is not None else 0, cos, sin)
        self._wgrad(o.draw, xq, a.fused(a.g, prefix + ".w_q.weight", 3) if own_kv else G[prefix + ".w_q.weight"])
        self._dgrad(o.draw, self._attn_wq(prefix, xkv), d_xq)

    def _hn_table(self, key, tag, B, S, entries):
        """KkAttnHeadNorm descriptors of one attention backward launch of sub-layer `key` (cached: every pointer is a persistent
        buffer) with their partial gain-gradient rows registered for the reduction at the end of the backward.
        entries = [(raw projection, gain, gain gradient, cos | None, sin | None)]."""
        nb = kk.load().kk_attn_bwd_blocks(B, self.dims.heads, S)
        part = self._buf(f"{key}.hnpart.{tag}", len(entries), nb, 64)
        tk = ("hn", self._tmp_ns, key, tag, B, S, part.data_ptr()) + tuple(
            (r.data_ptr(), r.stride(0), g_.data_ptr(), c_.data_ptr() if c_ is not None else 0) for r, g_, _, c_, _ in entries)
        table = self._table(tk, lambda: kk.attn_headnorm([(r, g_, part[j], c_, s_) for j, (r, g_, _, c_, s_) in enumerate(entries)]))
        for j, (_, _, dg_, _, _) in enumerate(entries):
            self._reduce_lists[self._tmp_ns].append((part[j], dg_, None, nb, 64, 64))
        return table

    def _headnorm_bwd(self, pkey, dn, raw, draw, rows, S, gains, dgains, rope_mask, cos, sin):
        """The per-head RMSNorm (+ RoPE) backward of len(gains) <= 3 parts as its own launch (the unfused arm): draw from dn and raw,
        the gain gradients as partial rows under `pkey`."""
        pad = (None,) * (3 - len(gains))
        kk.call("kk_headnorm_rope_bwd", dn, dn.stride(0), raw, raw.stride(0), draw, draw.stride(0), rows, self.dims.heads, S, len(gains),
                *gains, *pad, *dgains, *pad, self._headnorm_partials(pkey, rows, dgains), rope_mask, cos, sin, _b16(dn))

    # ------------------------------------------------------------------ text encoder: all layers in one launch
    def _encoder_stack_ok(self, B: int, Pn: int) -> bool:
        """The persistent launch carries batch item b on workgroup group b % 8: up to 8 items it is one pass (265-290 us against 545 us
        as 48 launches at 8 x 64 phonemes); a group walks further items one after the other, and from two passes on the 48 launches —
        whose kernels grow with the batch instead — are level or faster (dynamic batching, B up to 32: 9.50 against 9.69 ms per
        step on the configs[2] workload), so larger batches take the per-kernel sequence."""
        d = self.dims
        return bool(self.enc_fused and B <= self.enc_fused_max_batch and self.enc_dt == torch.bfloat16 and self.use_shadow and self.math == kk.KK_MATH_BF16 and
                    kk.load().kk_encoder_stack_supported(B, Pn, d.hidden, d.enc_ff, d.heads, d.enc_layers))

    def _encoder_stack_fwd(self, x0, B, Pn, text_mask, p_enc):
        """Forward of every encoder layer by kk_encoder_stack_fwd: same buffers, same masks as the per-kernel sequence
        (_attn_fwd / _ffn_fwd / _sublayer_tail), so the backward does not know the difference.  Returns (stream after the
        last layer, encoder_norm output)."""
        d, P, H, F, h, L = self.dims, self.arena.P, self.dims.hidden, self.dims.enc_ff, self.dims.heads, self.dims.enc_layers
        Ne, edt = B * Pn, self.enc_dt
        cos, sin = self._rope_tables(Pn)
        layers = []
        for i in range(L):
            lay = self._enc_layer(i)
            pf, key, ndt = lay.prefix, lay.key, lay.next_ln["ff"][2]
            sa, ff = key + ".sa", key + ".ff"
            ln2_g, ln2_b, y2, mean2, rstd2 = self._ln_out(lay.next_ln["sa"], Ne, H)
            next_g, next_b, next_y, next_mean, next_rstd = self._ln_out(lay.next_ln["ff"], Ne, H)
            layers.append(dict(
                w_qkv=self._Wf(pf + ".self_attn.w_q.weight", 3), g_q=P[pf + ".self_attn.q_norm.weight"],
                g_k=P[pf + ".self_attn.k_norm.weight"], g_v=P[pf + ".self_attn.v_norm.weight"],
                w_o=self._W(pf + ".self_attn.w_o.weight"), b_o=P[pf + ".self_attn.w_o.bias"],
                ln2_g=ln2_g, ln2_b=ln2_b,
                w1=self._W(pf + ".ff.linear1.weight"), b1=P[pf + ".ff.linear1.bias"],
                w2=self._W(pf + ".ff.linear2.weight"), b2=P[pf + ".ff.linear2.bias"], ffn_gain=P[pf + ".ff.output_norm.weight"],
                next_g=next_g, next_b=next_b,
                y1=self._buf(key + ".ln1.y", Ne, H, dtype=edt),
                qkv_raw=self._buf(sa + ".qkv_raw", Ne, 3 * H, dtype=edt), qkv_n=self._buf(sa + ".qkv_n", Ne, 3 * H, dtype=edt),
                ctx=self._buf(sa + ".ctx", Ne, H, dtype=edt), lse=self._buf(sa + ".lse", B, h, Pn),
                proj=self._buf(sa + ".proj", Ne, H),
                x_in=x0 if i == 0 else self._buf(f"enc{i - 1}.xo", Ne, H), xm=self._buf(key + ".xm", Ne, H),
                y2=y2, mean2=mean2, rstd2=rstd2,
                h1=self._buf(ff + ".h1", Ne, 2 * F, dtype=edt), g=self._buf(ff + ".g", Ne, F, dtype=edt),
                f2=self._buf(ff + ".f2", Ne, H, dtype=edt), rstd_f=self._buf(ff + ".rstd_f", Ne),
                xo=self._buf(key + ".xo", Ne, H), next_y=next_y,
                next_mean=next_mean, next_rstd=next_rstd,
                next_y_bf16=1 if ndt == torch.bfloat16 else 0, site=lay.site["sa"], p=float(p_enc), dpr=float(self._dpr(i, L))))
        sig = ("encstack", B, Pn, float(p_enc), self.train_dropout, self.enc_placement) + tuple(v.data_ptr() for v in layers[0].values() if hasattr(v, "data_ptr"))
        desc = self._table(sig, lambda: kk.enc_stack(B, Pn, H, F, h, text_mask, cos, sin, self.rng, self._enc_sync, layers, self.enc_placement,
                                                     self.enc_trace, self.enc_trace_wg))
        kk.call("kk_encoder_stack_fwd", desc)
        return self._buf(f"enc{L - 1}.xo", Ne, H), self._buf("enc.norm.y", Ne, H)

    # ------------------------------------------------------------------ GLU feed-forward sub-layer
    def _ffn_fwd(self, key, prefix, y, x_res, x_out, Fd, S=1, site=0, p=0.0, dpr=0.0, next_ln=None, split_k=0):
        P = self.arena.P
        N, H = y.shape
        dt, i16 = y.dtype, _b16(y)
        h1, g, f2 = (self._buf(key + ".h1", N, 2 * Fd, dtype=dt), self._buf(key + ".g", N, Fd, dtype=dt),
                     self._buf(key + ".f2", N, H, dtype=dt))
        W1 = self._W(prefix + ".linear1.weight")
        if i16 and _b16(W1) and H % 64 == 0 and self.fuse_glu_fwd:             # bf16 mode: the gate is the epilogue of the linear1 GEMM
            kk.call("kk_gemm_linear_glu", N, Fd, H, y, y.stride(0), W1, P[prefix + ".linear1.bias"], h1, g, Fd, self.rng, site + 4, p)
        else:
            self._linear(y, W1, P[prefix + ".linear1.bias"], h1, split_k=split_k)
            kk.call("kk_glu_fwd", h1, g, N, Fd, self.rng, site + 4, p, i16)
        self._linear(g, self._W(prefix + ".linear2.weight"), P[prefix + ".linear2.bias"], f2, split_k=split_k)
        # rmsnorm -> FFN dropout (:111) -> drop_path -> residual dropout (+ the next LayerNorm), one launch
        return self._sublayer_tail(f2, x_res, x_out, S, site, p, dpr, p, P[prefix + ".output_norm.weight"],
                                   self._buf(key + ".rstd_f", N), next_ln)

    def _ffn_bwd(self, key, prefix, d_out, y, d_y, Fd, S=1, site=0, p=0.0, dpr=0.0):
        P, G = self.arena.P, self.arena.G
        N, H = y.shape
        dt, i16 = y.dtype, _b16(y)
        h1, g, f2 = (self._buf(key + ".h1", N, 2 * Fd, dtype=dt), self._buf(key + ".g", N, Fd, dtype=dt),
                     self._buf(key + ".f2", N, H, dtype=dt))
        df2, dg, dh1 = (self._buf("tmp.df2", N, H, dtype=dt), self._buf("tmp.dg", N, Fd, dtype=dt),
                        self._buf("tmp.dh1", N, 2 * Fd, dtype=dt))
        # _tail_bwd already produced df2 (masks + RMSNorm backward) and the column sums for linear2.bias / output_norm
        self._wgrad(df2, g, G[prefix + ".linear2.weight"], None)
        W2 = self._W(prefix + ".linear2.weight")
        if i16 and _b16(W2) and H % 64 == 0:             # bf16 mode: the gate's backward is the epilogue of the linear2 dgrad
            nb = kk.load().kk_gemm_dgrad_glu_blocks(N)
            part = self._buf(key + ".glupart", nb, 2 * Fd)
            self._reduce_lists[self._tmp_ns].append((part, G[prefix + ".linear1.bias"], None, nb, 2 * Fd, 2 * Fd))
            kk.call("kk_gemm_dgrad_glu", N, Fd, H, df2, df2.stride(0), W2, h1, dh1, part, self.rng, site + 4, p)
            self._wgrad(dh1, y, G[prefix + ".linear1.weight"], None)
        else:
            self._dgrad(df2, W2, dg)
            kk.call("kk_glu_bwd", dg, h1, dh1, N, Fd, self.rng, site + 4, p, i16)
            self._wgrad(dh1, y, G[prefix + ".linear1.weight"], G[prefix + ".linear1.bias"])
        self._dgrad(dh1, self._W(prefix + ".linear1.weight"), d_y)

    # ------------------------------------------------------------------ variance predictor
    def _varpred_fwd(self, key, prefix, x, col1, B, L, mask, out, site=0, p=0.0, lens=None):
        """x [B*L, H]; col1 = im2col3(x) (shared by pitch & energy predictors); out [B*L].
        lens (int32 [B], or None: every row is L long): row b is a sequence of lens[b] positions, as the B = 1 predictor sees it; the
        three kernels take it as it is.  Then col1 = kk_im2col3_fwd(x, lens) too, and mask is the plain padding mask."""
        P, Fv = self.arena.P, self.dims.var_filter
        rows, nch = B * L, -(-L // CHUNK)
        scratch = self._buf("tmp.gn_scratch", 2 * B * nch, dtype=torch.float64)
        inp_col, cin = col1, x.shape[1]
        for li in range(2):
            c, y = self._buf(f"{key}.c{li}", rows, Fv), self._buf(f"{key}.y{li}", rows, Fv)
            stats = self._buf(f"{key}.st{li}", B * nch, 2)
            self._linear(inp_col, self._Wconv(f"{prefix}.conv_layers.{li}.weight", Fv, 3 * cin), P[f"{prefix}.conv_layers.{li}.bias"], c)
            gw, gb = P[f"{prefix}.norms.{li}.weight"], P[f"{prefix}.norms.{li}.bias"]
            kk.call("kk_groupnorm_relu_fwd", c, gw, gb, y, stats, scratch, lens, B, L, Fv, CHUNK, self.rng, site + li, p)
            if li == 0:
                inp_col, cin = self._buf(f"{key}.col2", rows, 3 * Fv, dtype=col1.dtype), Fv
                kk.call("kk_im2col3_fwd", y, inp_col, lens, B, L, Fv, CHUNK, _b16(inp_col))
        kk.call("kk_rowdot_fwd", y, P[f"{prefix}.linear.weight"], P[f"{prefix}.linear.bias"], mask, lens, out, rows, Fv, L, CHUNK, 0)

    def _varpred_bwd(self, key, prefix, dout, x, col1, B, L, mask, dx, p=0.0):
        """Accumulate the predictor's parameter grads; write dx (dL/dx) when dx is not None."""
        P, G, Fv = self.arena.P, self.arena.G, self.dims.var_filter
        rows, nch, H = B * L, -(-L // CHUNK), x.shape[1]
        scratch = self._buf("tmp.gn_scratch", 2 * B * nch, dtype=torch.float64)
        # bf16 mode: the conv gradients' GEMM operand is stored as bf16 like every other dY of the step (DMA GEMM core)
        dc_dt = col1.dtype
        dy, dc = self._buf("tmp.vp_dy", rows, Fv), self._buf("tmp.vp_dc", rows, Fv, dtype=dc_dt)
        y1 = self._buf(f"{key}.y1", rows, Fv)
        kk.call("kk_rowdot_bwd", dout, y1, P[f"{prefix}.linear.weight"], mask, dy, G[f"{prefix}.linear.weight"],
                G[f"{prefix}.linear.bias"], rows, Fv, L, CHUNK, 0,
                self._rowdot_partials(key, rows, Fv, G[f"{prefix}.linear.weight"], G[f"{prefix}.linear.bias"]))
        for li in (1, 0):
            c, y, stats = self._buf(f"{key}.c{li}", rows, Fv), self._buf(f"{key}.y{li}", rows, Fv), self._buf(f"{key}.st{li}", B * nch, 2)
            cin = Fv if li == 1 else H
            col = self._buf(f"{key}.col2", rows, 3 * Fv, dtype=col1.dtype) if li == 1 else col1
            kk.call("kk_groupnorm_relu_bwd", dy, c, y, P[f"{prefix}.norms.{li}.weight"], stats, dc, G[f"{prefix}.norms.{li}.weight"],
                    G[f"{prefix}.norms.{li}.bias"], scratch, B, L, Fv, CHUNK, p, _b16(dc))
            W, dW = self._Wconv(f"{prefix}.conv_layers.{li}.weight", Fv, 3 * cin), G[f"{prefix}.conv_layers.{li}.weight"].view(Fv, 3 * cin)
            self._wgrad(dc, col, dW, G[f"{prefix}.conv_layers.{li}.bias"])
            if li == 1 or dx is not None:
                dcol = self._buf(f"tmp.vp_dcol{li}", rows, 3 * cin, dtype=col1.dtype)
                self._dgrad(dc, W, dcol)
                kk.call("kk_im2col3_bwd", dcol, dy if li == 1 else dx, B, L, cin, CHUNK, _b16(dcol))

    # ------------------------------------------------------------------ forward + losses + backward
    def forward_backward(self, batch: Dict[str, torch.Tensor], loss_scale: float = 1.0, adaptive: bool = False,
                         backward: bool = True, zero_grads: bool = False, expanded_len: Optional[int] = None
                         ) -> Dict[str, torch.Tensor]:
        """One micro-batch: forward, the 6 losses, and (optionally) the full backward into the gradient arena
        (which accumulates; zero_grads=True clears it first, overlapped with the forward).  `batch` follows the
        reference collate contract (data/dataset.py:871-921), tensors on the device.  Returns device tensors (no sync):
        losses[6] = (total, mel, dur, stop, pitch, energy) and outputs.

        expanded_len = max_b sum(phoneme_durations[b]), the frame count T' the durations expand to, as a host integer
        (the caller has the durations on the host before the copy; nothing in a step synchronises).  None means T' = T,
        which holds for the reference's datasets unless an utterance was clipped (data/dataset.py:769-776).  T' > T:
        the pitch / energy predictors run on all T' frames and their outputs are [B, T'] like the reference's, the
        decoder memory is the first T frames (model/model.py:607-613), the losses read the first T columns
        (losses.py:111,137).  T' < T: the reference fails in the pitch loss with a size-mismatch RuntimeError
        (losses.py:126: [B, T'] predictions against [B, T] targets) — the same error is raised here, before any launch."""
        return self._fb(batch, loss_scale, adaptive, backward, zero_grads, expanded_len)

    def _fb(self, batch, loss_scale, adaptive, backward, zero_grads=False, expanded_len=None):
        """The launch sequence of forward_backward (also what train_step_graphed captures)."""
        self._defer_wgrads = None                     # (a list only while layer 0's grouped launch is being collected: ADVICE r5)
        self._ss_step = None
        try:
            with self._acc_guard():
                return self._fb_launches(batch, loss_scale, adaptive, backward, zero_grads, expanded_len)
        finally:
            self._defer_wgrads = None
            self._ss_step = None
            self._wgrad_queue.clear()

    def _fb_launches(self, batch, loss_scale, adaptive, backward, zero_grads=False, expanded_len=None):
        """The stages of one micro-batch in launch order.  Streams: the decoder head runs on _kv beside the encoder, the predictors'
        forward and (forked from st.fork) the side backward on _side; the decoder chain, captured first, stays on this one."""
        st = self._step_setup(batch, loss_scale, adaptive, backward, zero_grads, expanded_len)
        self._fb_decoder_head(st)
        self._fb_encoder_fwd(st)
        self._fb_variance_adaptor(st)
        # ---- decoder (model.py:519-531; transformers.py:543-583,660) ----
        self._mark("memory ready")
        self._cross_kv_fwd_all(st.memory, st.Nd, st.T, self.dec_dt)        # every layer's cross-attention K/V in one GEMM
        self._mark("cross K/V fwd done")
        self._fb_predictors_fwd(st)
        self._fb_decoder_fwd(st)
        out = self._fb_losses(st)
        if not st.backward:
            return out
        # =========================== backward ===========================
        self._fb_loss_grads(st)
        # The decoder backward is the critical path, so it is captured first and the predictors' + encoder's backward
        # after it, forked from the point right after the loss gradients (see _on_stream).
        self._fb_decoder_bwd(st)
        # the memory tail needs the cross-attention dK / dV of all layers and nothing else of the decoder backward: it runs on the
        # third stream beside layer 0's self-attention backward (1) or beside the input projection's backward (2), or on the side
        # stream behind the encoder's backward (3, 4: _fb_side_bwd), or at the end of the main chain (0)
        if st.tail_mode == 2:
            st.tail_fork = self._fork_point()
        self._fb_input_projection_bwd(st)
        if st.tail_mode in (1, 2):
            with self._on_stream(self._kv, "kv.", after=st.tail_fork):
                self._fb_memory_tail(st)
            self._join(self._kv)
        elif st.tail_mode == 0:
            self._fb_memory_tail(st)
        self._mark("main: backward tail done")
        self._fb_side_bwd(st)
        self._fb_finish(st)
        return out

    # ---- the stages: each takes the step's record; the views it leaves for later stages are listed in _Step ----
    def _enc_layer(self, i, ns="") -> LayerNames:
        return encoder_layer_names(i, self.dims.enc_layers, self.enc_dt, ns)

    def _dec_layer(self, i, ns="") -> LayerNames:
        return decoder_layer_names(i, self.dims.dec_layers, self.dec_dt, ns)

    def _step_setup(self, batch, loss_scale, adaptive, backward, zero_grads, expanded_len) -> _Step:
        """Validate the batch, take every decision of the step, issue the launches in front of the first fork."""
        d, hp = self.dims, self.hp
        self._grads_fresh = bool(zero_grads) or self._first_micro
        self._ow_seen = set() if (self._grads_fresh and backward) else None
        self._ow_expect = None
        B, Pn = batch["phoneme_indices"].shape
        T = batch["mel_specs"].shape[1]
        Tp = T if expanded_len is None else max(int(expanded_len), 3)     # variance_predictor.py:358-360 (at least 3 frames)
        if Tp < T:
            raise RuntimeError(f"The size of tensor a ({Tp}) must match the size of tensor b ({T}) at non-singleton dimension 1 "
                               f"(durations expand to {Tp} frames, the batch has {T} mel frames: losses.py:126)")
        if max(T, Tp) > d.max_len or Pn > d.max_len:
            raise ValueError(f"sequence longer than the positional table ({d.max_len})")
        if self.tail_aside not in (-1, 0, 1, 2, 3, 4):
            raise ValueError(f"tail_aside = {self.tail_aside!r}: -1 or one of the modes 0 ... 4")
        p_dec = self._p(hp.decoder_dropout)
        stack = self._encoder_stack_ok(B, Pn)
        # beside the persistent encoder forward, where that pays (measured: -0.4 % at 8 x 512, +1.6 % at 8 x 1024, where the generator
        # outlasts the encoder and delays the decoder head; profiles/r06_keep_bits_gen_ab.txt)
        gen_keep = bool(self.attn_keep_gen and self.attn_keep_bits and self.train_dropout and p_dec > 0.0 and self.dec_dt == torch.bfloat16 and
                        self.overlap and stack and self.dec_head_aside)
        gen_layers = 0
        if gen_keep:
            units = B * d.heads * ((T + 31) // 32) ** 2 * 1.5          # a layer: the causal self-attention (half) + the cross-attention
            gen_layers = min(d.dec_layers, int(self.attn_keep_gen_rate * (160.0 + 2.0 * Pn) / units))
            gen_keep = gen_layers > 0
        tail_mode = (4 if B * T <= 4096 else 3) if self.tail_aside < 0 else self.tail_aside
        st = _Step(batch=batch, backward=bool(backward), zero_grads=bool(zero_grads), B=B, Pn=Pn, T=T, Tp=Tp, Ne=B * Pn, Nd=B * T, Np=B * Tp,
                   p_din=self._p(hp.decoder_input_dropout), pe_drop=self._p(hp.encoder_dropout), p_enc=self._p(hp.encoder_dropout),
                   p_dec=p_dec, p_var=self._p(hp.variance_dropout), stack=stack, gen_keep=gen_keep, gen_layers=gen_layers,
                   spec_aug=bool(self.train_dropout and hp.use_spec_augment and self.spec_augment_active),
                   sort_buckets=bool(backward and self.embed_bwd_sorted and d.var_bins <= 1024),
                   tail_mode=tail_mode if self.overlap else 0,
                   lcfg=kk.KkLossCfg(hp.duration_loss_weight, hp.stop_token_loss_weight, hp.pitch_loss_weight, hp.energy_loss_weight,
                                     hp.duration_huber_delta, hp.pitch_huber_delta, hp.energy_huber_delta, hp.stop_token_pos_weight,
                                     float(loss_scale), 1 if adaptive else 0))
        self._keep_ready = set()
        st.text_mask = self._buf("text_mask", B, Pn, dtype=torch.uint8)
        if not self.fuse_enc_prologue:
            kk.call("kk_ids_eq_zero", batch["phoneme_indices"], st.text_mask, st.Ne)
        if self.train_dropout:
            self.rng.add_(1)                              # fresh masks every micro-batch (captured in the hipGraph)
        self._mark("step.start")
        return st

    def _dec_self_attn_fwd(self, st, i, y_in, n1_in):
        """Self-attention sub-layer of decoder layer i: (stream behind it, its norm2 output)."""
        lay = self._dec_layer(i)
        ya = self._buf(lay.key + ".xa", st.Nd, self.dims.hidden)
        n2 = self._attn_fwd(lay.key + ".sa", lay.prefix + ".self_attn", n1_in, None, st.B, st.T, st.T, True, True, None, y_in, ya,
                            lay.site["sa"], st.p_dec, self._dpr(i, self.dims.dec_layers), next_ln=lay.next_ln["sa"])
        return ya, n2

    def _fb_decoder_head(self, st) -> None:
        """---- decoder head: mel input projection + layer-0 self-attention need no encoder output (model.py:519-531) ----
        On the _kv stream beside the encoder; joined before the first cross-attention (_fb_decoder_fwd)."""
        P, H, M, B, T, Nd = self.arena.P, self.dims.hidden, self.dims.mel, st.B, st.T, st.Nd
        pe = P["positional_encoding.pe"].view(self.dims.max_len, H)
        st.shifted = shifted = self._buf("dec.shifted", Nd, M)
        with self._on_stream(self._kv, "kv.", self.dec_head_aside):
            if st.zero_grads and not self.zero_late:
                self._zero_grad_step()
            kk.call("kk_max_i64", st.batch["phoneme_durations"], st.Ne, self.max_dur)  # (read by the losses only: not in front of the encoder)
            kk.call("kk_shift_right", st.batch["mel_specs"], shifted, B, T, M)
            y0 = self._buf("dec.x0", Nd, H)
            if self.train_dropout and (st.p_din > 0.0 or st.pe_drop > 0.0):    # dropout(proj) + pe, then the PE module's dropout
                lin, t1 = self._buf("tmp.dec_lin", Nd, H), self._buf("tmp.dec_t1", Nd, H)
                self._linear(shifted, self._W("mel_projection_in.weight"), P["mel_projection_in.bias"], lin)
                kk.call("kk_dropout_fwd", lin, pe, T, t1, Nd, H, T, self.rng, 30, st.p_din, 0, 0.0, 0, 0.0)
                kk.call("kk_dropout_fwd", t1, None, 0, y0, Nd, H, T, self.rng, 31, st.pe_drop, 0, 0.0, 0, 0.0)
            else:
                self._linear(shifted, self._W("mel_projection_in.weight"), P["mel_projection_in.bias"], y0, res=pe, res_mod=T)
            n10 = self._ln_fwd("dec0.ln1", y0, "decoder.layers.0.norm1", self.dec_dt)
            # The 200 MB gradient zero-fill goes HERE: the launches above are in flight before the persistent encoder
            # kernel (which takes every CU's LDS) starts; the fill needs no LDS and runs beside it, while the GEMMs and
            # the attention below cannot and follow the encoder — with the fill in front of the whole head, none of the
            # head ran early and it ended 46 us after the cross-attention K/V GEMM, on the critical path.
            if st.zero_grads and self.zero_late:
                self._zero_grad_step()
            self._mark("kv: zero_grad done")
            if st.gen_keep:
                # the keep bits of every decoder attention launch of this step, HERE: this stream idles until the persistent encoder
                # launch (which holds every CU's LDS) has ended, and the generator needs no LDS — it runs beside the encoder
                self._keep_gen_launch(B, T, st.p_dec, 0, True, layers=st.gen_layers)
                self._mark("kv: keep bits generated")
            st.dec_head = (y0,) + self._dec_self_attn_fwd(st, 0, y0, n10)
            self._mark("kv: decoder head done")

    def _encoder_layers_fwd(self, ns, first, x, y1, B, Pn, text_mask, p=0.0, train=False):
        """Encoder layers [first, enc_layers) as one launch sequence per layer, on the workspace keys `ns` + "enc<i>...": x = the
        stream entering layer `first`, y1 = its norm1 output.  train: RNG sites, drop-path and the step's marks apply (the inference
        callers run with dropout off and the kernels' default site).  Returns (stream behind the last layer, encoder_norm output)."""
        d, H, Ne = self.dims, self.dims.hidden, B * Pn
        for i in range(first, d.enc_layers):
            lay = self._enc_layer(i, ns)
            dpr = self._dpr(i, d.enc_layers) if train else 0.0
            xm, xo = self._buf(lay.key + ".xm", Ne, H), self._buf(lay.key + ".xo", Ne, H)
            y2 = self._attn_fwd(lay.key + ".sa", lay.prefix + ".self_attn", y1, None, B, Pn, Pn, True, False, text_mask, x, xm,
                                lay.site["sa"] if train else 0, p, dpr, next_ln=lay.next_ln["sa"])
            y1 = self._ffn_fwd(lay.key + ".ff", lay.prefix + ".ff", y2, xm, xo, d.enc_ff, Pn, lay.site["ff"] if train else 0, p, dpr,
                               next_ln=lay.next_ln["ff"])
            x = xo
            if train:
                self._mark(f"enc{i} fwd done")
        return x, y1

    def _fb_encoder_fwd(self, st) -> None:
        """---- encoder (model.py:375-388) ----"""
        d, P, H, edt, B, Pn, Ne = self.dims, self.arena.P, self.dims.hidden, self.enc_dt, st.B, st.Pn, st.Ne
        ids, stress = st.batch["phoneme_indices"], st.batch.get("stress_indices")
        pe = P["positional_encoding.pe"].view(d.max_len, H)
        x, lay0 = self._buf("enc.x0", Ne, H), self._enc_layer(0)
        # LayerNorm outputs come from the previous sub-layer's fused tail; layer 0's from the prologue
        if self.fuse_enc_prologue:                        # key mask + embedding + layer 0's pre-norm: ONE launch in front of the encoder
            y1, m1, r1 = self._buf("enc0.ln1.y", Ne, H, dtype=edt), self._buf("enc0.ln1.mean", Ne), self._buf("enc0.ln1.rstd", Ne)
            kk.call("kk_embed_ln_fwd", ids, stress, P["text_embedding.weight"], P["stress_embedding.weight"] if stress is not None else None,
                    pe, x, B, Pn, H, float(H ** 0.5), self.rng, 1, st.pe_drop, st.text_mask, P[lay0.prefix + ".norm1.weight"],
                    P[lay0.prefix + ".norm1.bias"], y1, _b16(y1), m1, r1)
        else:
            kk.call("kk_embed_fwd", ids, stress, P["text_embedding.weight"], P["stress_embedding.weight"] if stress is not None else None,
                    pe, x, B, Pn, H, float(H ** 0.5), self.rng, 1, st.pe_drop)
            y1 = self._ln_fwd(lay0.key + ".ln1", x, lay0.prefix + ".norm1", edt)
        if st.stack:                                      # all layers in ONE persistent launch (csrc/kk_encstack.hip)
            x, y1 = self._encoder_stack_fwd(x, B, Pn, st.text_mask, st.p_enc)
            self._mark(f"enc{d.enc_layers - 1} fwd done")
        st.enc_last, st.enc = self._encoder_layers_fwd("", d.enc_layers if st.stack else 0, x, y1, B, Pn, st.text_mask, st.p_enc, train=True)

    def _fb_variance_adaptor(self, st) -> None:
        """---- variance adaptor (variance_predictor.py:338-439) ----"""
        d, P, H, hp, edt, ddt = self.dims, self.arena.P, self.dims.hidden, self.hp, self.enc_dt, self.dec_dt
        batch, B, Pn, T, Tp, Ne, Nd, Np = st.batch, st.B, st.Pn, st.T, st.Tp, st.Ne, st.Nd, st.Np
        st.dur_pred = self._buf("out.log_dur", B, Pn)
        st.col_e = self._buf("vp.col_enc", Ne, 3 * H, dtype=edt)      # (both conv unfolds are the predictors' inputs only: side stream)
        # (teacher forcing: the regulator and the embeddings below use the batch's durations / pitch / energy, so the three
        #  predictors feed only the losses and run on the side stream — see _fb_predictors_fwd)
        st.idx, st.lens, tot = (self._buf("lr.idx", B, T, dtype=torch.int64), self._buf("lr.lens", B, dtype=torch.int64),
                                self._buf("lr.total", B, dtype=torch.int64))
        kk.call("kk_length_regulate_index", batch["phoneme_durations"], st.idx, st.lens, tot, B, Pn, T)
        xf = self._buf("va.xf", Nd, H)
        st.memory, st.fmask = memory, fmask = self._buf("va.memory", Nd, H, dtype=ddt), self._buf("va.fmask", B, T, dtype=torch.uint8)
        st.pidx, st.eidx = pidx, eidx = self._buf("va.pidx", B, T, dtype=torch.int32), self._buf("va.eidx", B, T, dtype=torch.int32)
        if self.fuse_memory_fwd:     # gather + embedding adds + SpecAugment: ONE launch between the encoder and the cross-attention K/V GEMM
            kk.call("kk_regulate_embed_fwd", st.enc, st.idx, batch["pitches"], batch["energies"], P[f"{VA}.pitch_bins"], P[f"{VA}.energy_bins"],
                    P[f"{VA}.pitch_embedding.weight"], P[f"{VA}.energy_embedding.weight"], st.lens, xf, memory, pidx, eidx, fmask, B, Pn, T, H,
                    d.var_bins, _b16(memory), self.rng if st.spec_aug else None, 20, hp.spec_augment_time_mask_max,
                    hp.spec_augment_freq_mask_max, hp.spec_augment_num_time_masks, hp.spec_augment_num_freq_masks)
        else:
            kk.call("kk_length_regulate_gather", st.enc, st.idx, xf, B, Pn, T, H)       # detached by construction
            kk.call("kk_bucket_embed_add_fwd", xf, batch["pitches"], batch["energies"], P[f"{VA}.pitch_bins"], P[f"{VA}.energy_bins"],
                    P[f"{VA}.pitch_embedding.weight"], P[f"{VA}.energy_embedding.weight"], st.lens, memory, pidx, eidx, fmask, B, T, H,
                    d.var_bins, _b16(memory))
        st.pitch_pred, st.energy_pred = self._buf("out.pitch", B, Tp), self._buf("out.energy", B, Tp)
        st.col_f = self._buf("vp.col_frames", Np, 3 * H, dtype=ddt)
        if Tp != T:      # the predictors' own T'-frame view of the expansion; the losses read the first T columns
            st.xf_p, st.fmask_p = self._buf("va.xf_p", Np, H), self._buf("va.fmask_p", B, Tp, dtype=torch.uint8)
            st.pitch_l, st.energy_l = self._buf("out.pitch_T", B, T), self._buf("out.energy_T", B, T)
        else:
            st.xf_p, st.fmask_p, st.pitch_l, st.energy_l = xf, fmask, st.pitch_pred, st.energy_pred
        if st.spec_aug and not self.fuse_memory_fwd:         # on the cross-attention memory only (model.py:636-639)
            kk.call("kk_specaug", memory, B, T, H, self.rng, 20, hp.spec_augment_time_mask_max, hp.spec_augment_freq_mask_max,
                    hp.spec_augment_num_time_masks, hp.spec_augment_num_freq_masks, _b16(memory))

    def _fb_predictors_fwd(self, st) -> None:
        """The three variance predictors (and the bucket sort the backward wants) on the side stream; joined before the losses."""
        d, H, B, Pn, T, Tp, Nd = self.dims, self.dims.hidden, st.B, st.Pn, st.T, st.Tp, st.Nd
        dur = st.batch["phoneme_durations"]
        # Forked only here, after the K/V GEMM: started earlier (right after im2col3) the predictors' fp32 GEMMs compete
        # with the critical path into the decoder; 2.8 % of the step (729K -> 749K frames/s).
        with self._on_side_stream():                      # joined before the losses
            self._mark("side: predictors fwd start")
            if st.sort_buckets:
                n_items = kk.load().kk_bucket_sort_items(Nd, d.var_bins)
                st.be_order, st.be_items = (self._buf("va.be_order", 2, Nd, dtype=torch.int32),
                                            self._buf("va.be_items", 2, n_items, 4, dtype=torch.int32))
                kk.call("kk_bucket_sort", st.pidx, st.eidx, st.fmask, Nd, d.var_bins, st.be_order, st.be_items)
            kk.call("kk_im2col3_fwd", st.enc, st.col_e, None, B, Pn, H, CHUNK, _b16(st.col_e))
            if Tp != T:
                idx_p, lens_p = self._buf("lr.idx_p", B, Tp, dtype=torch.int64), self._buf("lr.lens_p", B, dtype=torch.int64)
                kk.call("kk_length_regulate_index", dur, idx_p, lens_p, self._buf("lr.total_p", B, dtype=torch.int64), B, Pn, Tp)
                kk.call("kk_length_regulate_gather", st.enc, idx_p, st.xf_p, B, Pn, Tp, H)
                kk.call("kk_frame_mask", lens_p, st.fmask_p, B, Tp)
            kk.call("kk_im2col3_fwd", st.xf_p, st.col_f, None, B, Tp, H, CHUNK, _b16(st.col_f))
            self._varpred_fwd("vp.dur", f"{VA}.duration_predictor", st.enc, st.col_e, B, Pn, st.text_mask, st.dur_pred, 10, st.p_var)
            self._varpred_fwd("vp.pitch", f"{VA}.pitch_predictor", st.xf_p, st.col_f, B, Tp, st.fmask_p, st.pitch_pred, 12, st.p_var)
            self._varpred_fwd("vp.energy", f"{VA}.energy_predictor", st.xf_p, st.col_f, B, Tp, st.fmask_p, st.energy_pred, 14, st.p_var)
            if Tp != T:
                kk.call("kk_pad2d_f32", st.pitch_pred, Tp, Tp, st.pitch_l, T, T, B)
                kk.call("kk_pad2d_f32", st.energy_pred, Tp, Tp, st.energy_l, T, T, B)
            self._mark("side: predictors fwd done")

    def _fb_decoder_fwd(self, st) -> None:
        """The decoder layers behind the head (cross-attention and feed-forward of layer 0, then layers 1 ...) and the two output heads."""
        d, P, H, M, B, T, Nd = self.dims, self.arena.P, self.dims.hidden, self.dims.mel, st.B, st.T, st.Nd
        self._join(self._kv)                             # input projection + layer-0 self-attention ran beside the encoder
        y, ya, n2 = st.dec_head
        for i in range(d.dec_layers):
            lay, dpr = self._dec_layer(i), self._dpr(i, d.dec_layers)
            if i > 0:
                ya, n2 = self._dec_self_attn_fwd(st, i, y, n1)
            yc, yo = self._buf(lay.key + ".xc", Nd, H), self._buf(lay.key + ".xo", Nd, H)
            n3 = self._attn_fwd(lay.key + ".ca", lay.prefix + ".cross_attn", n2, st.memory, B, T, T, False, False, st.fmask, ya, yc,
                                lay.site["ca"], st.p_dec, dpr, next_ln=lay.next_ln["ca"], layer=i)
            n1 = self._ffn_fwd(lay.key + ".ff", lay.prefix + ".ff", n3, yc, yo, d.dec_ff, T, lay.site["ff"], st.p_dec, dpr,
                               next_ln=lay.next_ln["ff"])
            y = yo
            self._mark(f"dec{i} fwd done")
        st.dec_last, st.dec_out = y, n1                   # (n1: decoder.norm of the last stream, from the last feed-forward's tail)
        st.mel_pred, st.stop = self._buf("out.mel", B, T, M), self._buf("out.stop", B, T)
        self._linear(st.dec_out, self._W("mel_projection_out.weight"), P["mel_projection_out.bias"], st.mel_pred.view(Nd, M))
        kk.call("kk_rowdot_fwd", st.dec_out, P["stop_token_predictor.weight"], P["stop_token_predictor.bias"], None, None, st.stop, Nd, H, T, 0,
                _b16(st.dec_out))

    def _fb_losses(self, st) -> Dict[str, torch.Tensor]:
        """---- losses (losses.py) ----  Returns forward_backward's result."""
        batch, B, T = st.batch, st.B, st.T
        self._join_side()
        st.largs = (st.mel_pred, batch["mel_specs"], st.dur_pred, batch["phoneme_durations"], st.stop, batch["stop_token_targets"],
                    st.pitch_l, batch["pitches"], st.energy_l, batch["energies"], batch["mel_lengths"], batch["phoneme_lengths"],
                    B, T, st.Pn, self.dims.mel, st.lcfg)
        # per-micro-batch finite-output / finite-loss guard (trainer.py:3233-3296), device side: a flagged micro-batch
        # back-propagates nothing and its accumulation cycle takes no optimizer step; forward-only calls (validation) do
        # not touch the training cycle's flag
        guard = self.opt_state[kk.OS["MICRO_BAD"]:] if st.backward else None
        # (loss_acc is handed round zero: allocated zero, cleared by its last reader — no zero-fill launch on the critical chain)
        sc = 1 if self.self_cleaning_acc else 0
        kk.call("kk_losses_fwd", *st.largs, self.max_dur, self.loss_acc, self.losses, self.loss_coef,
                guard if self.loss_sync is None else None, sc * (1 if self.loss_sync is not None else 3))
        if self.loss_sync is not None:                    # global normalisers for ragged shards (one more collective of the step)
            self.loss_sync.loss_sync(self.loss_acc, self.max_dur)
            kk.call("kk_losses_finalize", self.loss_acc, st.lcfg, self.max_dur, canonical_mel_length(self.global_mel_length, T), self.losses,
                    self.loss_coef, guard, sc)
        return {"losses": self.losses, "mel": st.mel_pred, "log_dur": st.dur_pred, "stop": st.stop, "pitch": st.pitch_pred,
                "energy": st.energy_pred, "lr_idx": st.idx, "lr_lens": st.lens, "memory": st.memory.view(B, T, self.dims.hidden)}

    def _fb_loss_grads(self, st) -> None:
        """The backward's book-keeping and the loss gradients; st.fork = the point the side backward forks from."""
        B, T = st.B, st.T
        self._ss_ready = None
        if self.grad_norm_from_wgrads and self.dp_comm is None and not self._external_sync and self.group_wgrads:
            self._ss_step = dict(rec=kk.C.c_void_p(self.sumsq_ws.data_ptr() + int(kk.load().kk_seg_sumsq_rec_offset())), count=kk.C.c_int32(0),
                                 cap=int(kk.load().kk_seg_sumsq_rec_capacity()), covered=set())
        for ns in self._reduce_lists:
            self._reduce_lists[ns] = []
        if self.dp_comm is not None and self._exchange_now:
            self.dp_comm.begin_step()
            self._comm_events = {}
        st.dmel, st.ddur = self._buf("g.mel", B, T, self.dims.mel), self._buf("g.dur", B, st.Pn)
        st.dstop, st.dpitch, st.denergy = self._buf("g.stop", B, T), self._buf("g.pitch", B, T), self._buf("g.energy", B, T)
        kk.call("kk_losses_bwd", *st.largs, self.loss_coef, st.dmel, st.ddur, st.dstop, st.dpitch, st.denergy)
        self._mark("losses + loss gradients done")
        st.fork = self._fork_point()

    def _enc_bwd_head(self, st, i, sub):
        """_tail_bwd's `head` for sub-layer `sub` of encoder layer i (every LayerNorm's backward is fused with the head of the
        backward of the sub-layer that produced its input): (kind, ffn buffer key, parameter prefix, S, site, p, drop-path, dtype)."""
        lay = self._enc_layer(i)
        return ("ffn" if sub == "ff" else "attn", lay.key + ".ff", lay.prefix + _SUBLAYER[sub], st.Pn, lay.site[sub], st.p_enc,
                self._dpr(i, self.dims.enc_layers), self.enc_dt)

    def _dec_bwd_head(self, st, i, sub):
        """The same for sub-layer `sub` of decoder layer i."""
        lay = self._dec_layer(i)
        return ("ffn" if sub == "ff" else "attn", lay.key + ".ff", lay.prefix + _SUBLAYER[sub], st.T, lay.site[sub], st.p_dec,
                self._dpr(i, self.dims.dec_layers), self.dec_dt)

    def _fb_decoder_bwd(self, st) -> None:
        """The mel head's input gradient and the decoder layers, last to first, on the main chain.  Leaves st.tail_fork where the
        memory tail may start, and layer 0's grouped weight gradients in st.deferred0 (behind st.wgrad0_fork) when they wait."""
        d, H, M, ddt, B, T, Nd = self.dims, self.dims.hidden, self.dims.mel, self.dec_dt, st.B, st.T, st.Nd
        # heads: only the mel projection's input gradient continues down the decoder (the two heads' weight gradients are
        # on the side branch, see _fb_side_bwd)
        d_dec_out = self._buf("tmp.d_dec_out", Nd, H, dtype=ddt)
        self._dgrad(st.dmel.view(Nd, M), self._W("mel_projection_out.weight"), d_dec_out)
        st.dy = dy = self._buf("g.dec_stream", Nd, H)          # gradient of the decoder residual stream, updated in place
        self._tail_bwd("dec.norm", d_dec_out, st.dec_last, "decoder.norm", dy, False, self._dec_bwd_head(st, d.dec_layers - 1, "ff"))
        st.dmem = dmem = self._buf("g.memory", Nd, H)
        dn = self._buf("tmp.dn", Nd, H, dtype=ddt)
        for i in reversed(range(d.dec_layers)):
            lay, dpr = self._dec_layer(i), self._dpr(i, d.dec_layers)
            pf, key = lay.prefix, lay.key
            x_in = self._buf(f"dec{i - 1}.xo", Nd, H) if i > 0 else self._buf("dec.x0", Nd, H)
            ya, yc = self._buf(key + ".xa", Nd, H), self._buf(key + ".xc", Nd, H)
            n1, n2, n3 = (self._buf(f"{key}.ln{j}.y", Nd, H, dtype=ddt) for j in (1, 2, 3))
            # layer 0's grouped weight gradients: nothing on the main chain overwrites their operands any more (the layer-norm backward and
            # the input projection below use their own buffers), so the launch can wait for the side stream's idle end (wgrad0_aside)
            defer0 = i == 0 and st.tail_mode in (3, 4) and self.group_wgrads and self.dp_comm is None and \
                (self.wgrad0_aside > 0 or (self.wgrad0_aside < 0 and st.tail_mode == 3))
            if defer0:
                self._defer_wgrads = st.deferred0           # (reset by _fb whatever happens in between)
            with self._grouped_wgrads():
                self._ffn_bwd(key + ".ff", pf + ".ff", dy, n3, dn, d.dec_ff, T, lay.site["ff"], st.p_dec, dpr)
                self._tail_bwd(key + ".ln3", dn, yc, pf + ".norm3", dy, True, self._dec_bwd_head(st, i, "ca"))
                self._attn_bwd(key + ".ca", pf + ".cross_attn", dy, n2, st.memory, B, T, T, False, False, st.fmask, dn, dmem,
                               0.0, lay.site["ca"], st.p_dec, dpr, layer=i)
                if i == 0 and st.tail_mode in (1, 3, 4):  # every layer's cross-attention dK / dV is written: the memory tail may start
                    st.tail_fork = self._fork_point()
                    if st.tail_mode == 4:            # (4: the K/V weight gradient as one more member of layer 0's grouped launch)
                        self._cross_kv_bwd_all(st.memory, Nd, ddt, dmem, dgrad=False)
                self._tail_bwd(key + ".ln2", dn, ya, pf + ".norm2", dy, True, self._dec_bwd_head(st, i, "sa"))
                self._attn_bwd(key + ".sa", pf + ".self_attn", dy, n1, None, B, T, T, True, True, None, dn, None, 0.0, lay.site["sa"],
                               st.p_dec, dpr)
            if defer0:
                self._defer_wgrads = None
                st.wgrad0_fork = self._fork_point()
            self._comm_bucket(f"dec{i}")                    # the layer's weight matrices are final: exchange beside the rest
            if i > 0:
                self._tail_bwd(key + ".ln1", dn, x_in, pf + ".norm1", dy, True, self._dec_bwd_head(st, i - 1, "ff"))
            else:
                self._ln_bwd(key + ".ln1", dn, x_in, pf + ".norm1", dy, accumulate=True)
            self._mark(f"dec{i} bwd done")

    def _fb_input_projection_bwd(self, st) -> None:
        """(the PE add and the shift are parameter-free; mel is data)"""
        G, H, T, Nd = self.arena.G, self.dims.hidden, st.T, st.Nd
        if self.train_dropout and (st.p_din > 0.0 or st.pe_drop > 0.0):
            t1, dlin = self._buf("tmp.d_dec_t1", Nd, H), self._buf("tmp.d_dec_lin", Nd, H)
            kk.call("kk_dropout_bwd", st.dy, t1, Nd, H, T, self.rng, 31, st.pe_drop, 0, 0.0, 0, 0.0, 0)
            kk.call("kk_dropout_bwd", t1, dlin, Nd, H, T, self.rng, 30, st.p_din, 0, 0.0, 0, 0.0, 0)
            self._wgrad(dlin, st.shifted, G["mel_projection_in.weight"], G["mel_projection_in.bias"])
        else:
            self._wgrad(st.dy, st.shifted, G["mel_projection_in.weight"], G["mel_projection_in.bias"])
        self._mark("decoder input projection bwd done")

    def _fb_memory_tail(self, st) -> None:
        """variance adaptor: memory gradient feeds only the two embedding tables (xf is detached, lengths.py:30)"""
        d, G, hp, H, B, T, Nd = self.dims, self.arena.G, self.hp, self.dims.hidden, st.B, st.T, st.Nd
        self._cross_kv_bwd_all(st.memory, Nd, self.dec_dt, st.dmem, wgrad=st.tail_mode != 4)   # K/V weight gradients and the memory gradient, all layers at once
        self._mark("cross K/V bwd (all layers) done")
        if st.spec_aug:
            kk.call("kk_specaug", st.dmem, B, T, H, self.rng, 20, hp.spec_augment_time_mask_max, hp.spec_augment_freq_mask_max,
                    hp.spec_augment_num_time_masks, hp.spec_augment_num_freq_masks, 0)
        if st.sort_buckets:
            kk.call("kk_bucket_embed_add_bwd_sorted", st.dmem, st.be_order, st.be_items, G[f"{VA}.pitch_embedding.weight"],
                    G[f"{VA}.energy_embedding.weight"], Nd, H, d.var_bins)
        else:
            kk.call("kk_bucket_embed_add_bwd", st.dmem, st.pidx, st.eidx, st.fmask, G[f"{VA}.pitch_embedding.weight"],
                    G[f"{VA}.energy_embedding.weight"], B, T, H, d.var_bins)

    def _fb_side_bwd(self, st) -> None:
        """On the side stream, forked from st.fork: the output heads' weight gradients, the three predictors, the text encoder and
        the embedding — independent of the decoder backward (disjoint gradient segments) — and, in tail modes 3 / 4, the memory
        tail and decoder layer 0's deferred weight gradients behind them."""
        d, P, G, H, M, edt = self.dims, self.arena.P, self.arena.G, self.dims.hidden, self.dims.mel, self.enc_dt
        B, Pn, T, Tp, Ne, Nd = st.B, st.Pn, st.T, st.Tp, st.Ne, st.Nd
        ids, stress = st.batch["phoneme_indices"], st.batch.get("stress_indices")
        with self._on_side_stream(after=st.fork):
            self._mark("side: backward start")
            # the output heads' weight gradients have no consumer on the decoder chain (the stop head's input is
            # detached, model.py:561-562): 50 us off the critical path
            kk.call("kk_rowdot_bwd", st.dstop, st.dec_out, P["stop_token_predictor.weight"], None, None, G["stop_token_predictor.weight"],
                    G["stop_token_predictor.bias"], Nd, H, T, 0, _b16(st.dec_out),
                    self._rowdot_partials("stop", Nd, H, G["stop_token_predictor.weight"], G["stop_token_predictor.bias"]))
            self._wgrad(st.dmel.view(Nd, M), st.dec_out, G["mel_projection_out.weight"], G["mel_projection_out.bias"])
            dpitch_p, denergy_p = st.dpitch, st.denergy
            if Tp != T:                               # frames past T carry no loss: zero gradient there
                dpitch_p, denergy_p = self._buf("g.pitch_p", B, Tp), self._buf("g.energy_p", B, Tp)
                kk.call("kk_pad2d_f32", st.dpitch, T, T, dpitch_p, Tp, Tp, B)
                kk.call("kk_pad2d_f32", st.denergy, T, T, denergy_p, Tp, Tp, B)
            self._varpred_bwd("vp.pitch", f"{VA}.pitch_predictor", dpitch_p, st.xf_p, st.col_f, B, Tp, st.fmask_p, None, st.p_var)
            self._varpred_bwd("vp.energy", f"{VA}.energy_predictor", denergy_p, st.xf_p, st.col_f, B, Tp, st.fmask_p, None, st.p_var)
            d_enc = self._buf("g.enc_out", Ne, H)
            self._varpred_bwd("vp.dur", f"{VA}.duration_predictor", st.ddur, st.enc, st.col_e, B, Pn, st.text_mask, d_enc, st.p_var)
            self._mark("side: predictors bwd done")
            dx = self._buf("g.enc_stream", Ne, H)
            self._tail_bwd("enc.norm", d_enc, st.enc_last, "encoder_norm", dx, False, self._enc_bwd_head(st, d.enc_layers - 1, "ff"))
            dne = self._buf("tmp.dne", Ne, H, dtype=edt)
            for i in reversed(range(d.enc_layers)):
                lay, dpr = self._enc_layer(i), self._dpr(i, d.enc_layers)
                pf, key = lay.prefix, lay.key
                x_in = self._buf(f"enc{i - 1}.xo", Ne, H) if i > 0 else self._buf("enc.x0", Ne, H)
                xm = self._buf(key + ".xm", Ne, H)
                y1, y2 = self._buf(key + ".ln1.y", Ne, H, dtype=edt), self._buf(key + ".ln2.y", Ne, H, dtype=edt)
                with self._grouped_wgrads():
                    self._ffn_bwd(key + ".ff", pf + ".ff", dx, y2, dne, d.enc_ff, Pn, lay.site["ff"], st.p_enc, dpr)
                    self._tail_bwd(key + ".ln2", dne, xm, pf + ".norm2", dx, True, self._enc_bwd_head(st, i, "sa"))
                    self._attn_bwd(key + ".sa", pf + ".self_attn", dx, y1, None, B, Pn, Pn, True, False, st.text_mask, dne, None, 0.0,
                                   lay.site["sa"], st.p_enc, dpr)
                self._comm_bucket(f"enc{i}")            # (the grouped weight-gradient launch is behind us)
                if i > 0:
                    self._tail_bwd(key + ".ln1", dne, x_in, pf + ".norm1", dx, True, self._enc_bwd_head(st, i - 1, "ff"))
                else:
                    self._ln_bwd(key + ".ln1", dne, x_in, pf + ".norm1", dx, accumulate=True)
                self._mark(f"side: enc{i} bwd done")
            kk.call("kk_embed_bwd", ids, stress, dx, G["text_embedding.weight"],
                    G["stress_embedding.weight"] if stress is not None else None, B, Pn, H, float(H ** 0.5), self.rng, 1, st.pe_drop)
            self._mark("side: backward done")
            if st.tail_mode in (3, 4):                   # the memory tail behind the encoder's backward (no third branch)
                torch.cuda.current_stream().wait_event(st.tail_fork)
                self._fb_memory_tail(st)
                if st.deferred0:
                    torch.cuda.current_stream().wait_event(st.wgrad0_fork)
                    for q in st.deferred0:
                        self._issue_wgrad_group(q)

    def _fb_finish(self, st) -> None:
        """Join the branches, reduce the partial sums, hand the tail bucket to the exchange, close the step's records."""
        self._join(self._side)
        self._reduce_partials((st.B, st.T, st.Pn, st.Tp))
        self._comm_bucket("tail")                       # everything that was not a layer's weight matrix
        self._comm_join()
        self._mark("backward joined, partials reduced")
        if self._ss_step is not None:                   # the tile records of this micro-batch: what an optimizer boundary right behind it may use
            if self._ss_step["covered"]:
                self._ss_ready = (frozenset(self._ss_step["covered"]), int(self._ss_step["count"].value))
            self._ss_step = None
        if self._ow_seen is not None:                   # what this cycle's first micro-batch overwrote (see _zero_grad_step)
            seen = frozenset(self._ow_seen)
            if self._ow_expect is not None and seen != self._ow_expect:
                raise RuntimeError("the step zero-filled the gradient arena by a stale overwrite record: "
                                   f"{len(self._ow_expect - seen)} tensors were skipped but not overwritten")
            self._ow_sets[self._ow_key()] = seen
            self._ow_seen = None

    # ------------------------------------------------------------------ inference
    def _decoder_step(self, ns, rows, pe_res, res_mod, cos, sin, S, split_k, self_attn, cross_attn):
        """The decoder at Sq = 1 for `rows` rows on the workspace keys `ns`.*, from the mel input projection of frame_in (written, like
        the positional operands, by the caller's prologue kernel) to (frame_out [rows, mel], stop_now [rows]) for its epilogue kernel.
        The callers (_decode_step: every row at one frame; _stream_step: each at its own) differ in the positional rows pe_res /
        cos / sin (one for all: res_mod = 1, S = 1; one per row: res_mod = 0, S = rows), in split_k of the step's GEMMs, and in
        self_attn(i, key, nrm [rows, 3H]) (append q|k|v to layer i's cache, attend over it) and cross_attn(i, key, q_n [rows, H])
        (attend over layer i's K|V of the expanded memory), which return ctx [rows, H]."""
        d, P, H, M, ddt = self.dims, self.arena.P, self.dims.hidden, self.dims.mel, self.dec_dt
        frame_in, y = self._buf(f"{ns}.frame_in", rows, M), self._buf(f"{ns}.y", rows, H)
        frame_out, stop_now = self._buf(f"{ns}.frame_out", rows, M), self._buf(f"{ns}.stop_now", rows)
        # mel_projection_in + positional encoding at the row's frame (model.py:541-545)
        self._linear(frame_in, self._W("mel_projection_in.weight"), P["mel_projection_in.bias"], y, res=pe_res, res_mod=res_mod, split_k=split_k)
        n1 = self._ln_fwd(f"{ns}.dec0.ln1", y, "decoder.layers.0.norm1", ddt)
        yl = y
        for i in range(d.dec_layers):
            lay = self._dec_layer(i, ns + ".")
            pf, key = lay.prefix, lay.key
            sp, cp = pf + ".self_attn", pf + ".cross_attn"
            raw, nrm = self._buf(key + ".qkv_raw", rows, 3 * H, dtype=ddt), self._buf(key + ".qkv_n", rows, 3 * H, dtype=ddt)
            # K alone is rotated, by the row's absolute position; the single query by position 0, i.e. not at all (generate)
            self._proj_headnorm(n1, self._Wf(sp + ".w_q.weight", 3), raw, nrm, S,
                                (P[sp + ".q_norm.weight"], P[sp + ".k_norm.weight"], P[sp + ".v_norm.weight"]), 2, cos, sin, split_k=split_k)
            ctx = self_attn(i, key, nrm)
            proj = self._buf("str.proj" if ns == "str" else f"tmp.{ns}_proj", rows, H)
            self._linear(ctx, self._W(sp + ".w_o.weight"), P[sp + ".w_o.bias"], proj, split_k=split_k)
            ya = self._buf(key + ".xa", rows, H)
            n2 = self._sublayer_tail(proj, yl, ya, 1, 0, 0.0, 0.0, 0.0, None, None, lay.next_ln["sa"])
            # cross-attention: _attn_fwd's launches without dropout, with the caller's attention kernel
            q_raw, q_n = self._buf(key + ".ca.q_raw", rows, H, dtype=ddt), self._buf(key + ".ca.q_n", rows, H, dtype=ddt)
            self._proj_headnorm(n2, self._W(cp + ".w_q.weight"), q_raw, q_n, 1, (P[cp + ".q_norm.weight"],), 0, None, None, split_k=split_k)
            ctx = cross_attn(i, key, q_n)
            yc = self._buf(key + ".xc", rows, H)
            n3 = self._attn_out(key + ".ca", cp, ctx, rows, 1, ya, yc, 0, 0.0, 0.0, lay.next_ln["ca"], split_k=split_k)
            yo = self._buf(key + ".xo", rows, H)
            n1 = self._ffn_fwd(key + ".ff", pf + ".ff", n3, yc, yo, d.dec_ff, 1, next_ln=lay.next_ln["ff"], split_k=split_k)
            yl = yo
        self._linear(n1, self._W("mel_projection_out.weight"), P["mel_projection_out.bias"], frame_out, split_k=split_k)
        kk.call("kk_rowdot_fwd", n1, P["stop_token_predictor.weight"], P["stop_token_predictor.bias"], None, None, stop_now, rows, H, 1, 0, _b16(n1))
        return frame_out, stop_now

    def _decode_step(self, ns, B, T, max_expected, fm2):
        """One decoder step of generate / generate_batch, all B rows at the frame of one device counter: kk_decode_prologue, then
        _decoder_step; returns its (frame_out [B, mel], stop_now [B]), which the caller's epilogue files under frame t.  The state is
        the workspace entries under `ns` ("gen" / "syn") that _decode_state_init reset.  Self-attention: one kk_attn_fwd with B*heads
        "heads" over the time-major caches [t][B*H]; cross-attention over the K|V of _expand_fwd ("" for "gen", else `ns` + ".")."""
        d, P, H, M, h, ddt = self.dims, self.arena.P, self.dims.hidden, self.dims.mel, self.dims.heads, self.dec_dt
        BH, L1, kv_ns = B * H, max_expected + 1, "" if ns == "gen" else ns + "."
        pe, (cos, sin) = P["positional_encoding.pe"].view(d.max_len, H), self._rope_tables(d.max_len)
        mel_out, frame_in = self._buf(f"{ns}.mel", B, L1, M), self._buf(f"{ns}.frame_in", B, M)
        t_dev, kmask = self._buf(f"{ns}.t", 1, dtype=torch.int32), self._buf(f"{ns}.kmask", 1, max_expected, dtype=torch.uint8)
        pe_row, cos_row, sin_row = self._buf(f"{ns}.pe_row", 1, H), self._buf(f"{ns}.cos_row", 1, 64), self._buf(f"{ns}.sin_row", 1, 64)
        kk.call("kk_decode_prologue", mel_out, frame_in, pe, pe_row, cos, sin, cos_row, sin_row, kmask, t_dev, B, L1, M, H)

        def self_attn(i, key, nrm):
            Kc, Vc = self._buf(key + ".kcache", max_expected, BH, dtype=ddt), self._buf(key + ".vcache", max_expected, BH, dtype=ddt)
            qb = self._buf(key + ".q", 1, BH, dtype=ddt)
            kk.call("kk_decode_cache_append", nrm, qb, Kc, Vc, t_dev, B, H, _b16(nrm))
            ctx, lse = self._buf(key + ".ctx", 1, BH, dtype=ddt), self._buf(key + ".lse", 1, B * h, 1)
            self._attn_launch("kk_attn_fwd", _AttnOps(qb, Kc, Vc, ctx, lse), 1, B * h, 1, max_expected, kmask, False, 0, 0.0)
            return ctx.view(B, H)

        def cross_attn(i, key, q_n):
            _, kv_n = self._cross_kv(i, B * T, ddt, ns=kv_ns)              # filled by _cross_kv_fwd_all
            ctx, lse = self._buf(key + ".ca.ctx", B, H, dtype=ddt), self._buf(key + ".ca.lse", B, h, 1)
            self._attn_launch("kk_attn_fwd", _AttnOps(q_n, kv_n, kv_n[:, H:], ctx, lse), B, h, 1, T, fm2, False, 3, 0.0)
            return ctx

        return self._decoder_step(ns, B, pe_row, 1, cos_row, sin_row, 1, 0, self_attn, cross_attn)

    def _encode_text_fwd(self, ns, ids, stress, B, Pn, text_mask):
        """encode_text (model.py:375-388) with dropout off: embedding, the encoder layers under the key mask `text_mask`
        (= ids == 0, written here) and encoder_norm.  Workspace keys `ns` + "enc...".  Returns the encoder output [B*Pn, H]."""
        d, P, H, edt = self.dims, self.arena.P, self.dims.hidden, self.enc_dt
        Ne = B * Pn
        kk.call("kk_ids_eq_zero", ids, text_mask, Ne)
        x = self._buf(ns + "enc.x0", Ne, H)
        kk.call("kk_embed_fwd", ids, stress, P["text_embedding.weight"], P["stress_embedding.weight"] if stress is not None else None,
                P["positional_encoding.pe"].view(d.max_len, H), x, B, Pn, H, float(H ** 0.5), self.rng, 1, 0.0)
        lay0 = self._enc_layer(0, ns)
        y1 = self._ln_fwd(lay0.key + ".ln1", x, lay0.prefix + ".norm1", edt)
        return self._encoder_layers_fwd(ns, 0, x, y1, B, Pn, text_mask)[1]

    def _expand_fwd(self, ns, enc, dur, B, Pn, T, flens=None, controls=None, contours=None):
        """The variance adaptor behind the durations, without targets (variance_predictor.py:338-439): repeat phoneme p of
        each row dur[b, p] times up to T frames, predict pitch and energy, add the bucket embeddings of the clamped predictions,
        and project the result to the cross-attention K|V of every decoder layer (_cross_kv_fwd_all under `ns`).  flens (int32
        [B]) makes the predictors see row b as a sequence of flens[b] frames; None = the padded batch as one.  Workspace keys
        `ns` + "lr.* / va.* / vp.* / out.*".  controls (prosody.PackedProsody, or None: none): kk_prosody_variance puts the
        per-phoneme pitch / energy controls on the clamped predictions in front of the bucket embeddings.  contours
        (prosody.PackedContours, or None: no row has one; needs controls): kk_prosody_contour in its place, which also puts the rows'
        frame-level source tracks on the frames that `dur` gave their phonemes.
        Returns (memory [B*T, H], fm2 = the frame mask [B, T])."""
        d, P, H, ddt = self.dims, self.arena.P, self.dims.hidden, self.dec_dt
        Nd = B * T
        idx, lens, tot = (self._buf(ns + "lr.idx", B, T, dtype=torch.int64), self._buf(ns + "lr.lens", B, dtype=torch.int64),
                          self._buf(ns + "lr.total", B, dtype=torch.int64))
        kk.call("kk_length_regulate_index", dur, idx, lens, tot, B, Pn, T)
        xf = self._buf(ns + "va.xf", Nd, H)
        kk.call("kk_length_regulate_gather", enc, idx, xf, B, Pn, T, H)
        fmask = (torch.arange(T, device=self.device)[None, :] >= lens[:, None]).to(torch.uint8).contiguous()
        col_f = self._buf(ns + "vp.col_frames", Nd, 3 * H, dtype=ddt)
        kk.call("kk_im2col3_fwd", xf, col_f, flens, B, T, H, CHUNK, _b16(col_f))
        pitch, energy = self._buf(ns + "out.pitch", B, T), self._buf(ns + "out.energy", B, T)
        self._varpred_fwd(ns + "vp.pitch", f"{VA}.pitch_predictor", xf, col_f, B, T, fmask, pitch, lens=flens)
        self._varpred_fwd(ns + "vp.energy", f"{VA}.energy_predictor", xf, col_f, B, T, fmask, energy, lens=flens)
        memory, fm2 = self._buf(ns + "va.memory", Nd, H, dtype=ddt), self._buf(ns + "va.fmask", B, T, dtype=torch.uint8)
        pidx, eidx = self._buf(ns + "va.pidx", B, T, dtype=torch.int32), self._buf(ns + "va.eidx", B, T, dtype=torch.int32)
        if controls is None:
            kk.call("kk_bucket_embed_add_fwd", xf, pitch.clamp(0.0, 1.0), energy.clamp(0.0, 1.0), P[f"{VA}.pitch_bins"],
                    P[f"{VA}.energy_bins"], P[f"{VA}.pitch_embedding.weight"], P[f"{VA}.energy_embedding.weight"], lens, memory,
                    pidx, eidx, fm2, B, T, H, d.var_bins, _b16(memory))
        else:
            c, pc, ec = controls, torch.empty_like(pitch), torch.empty_like(energy)
            if contours is None:
                kk.call("kk_prosody_variance", pitch, energy, idx, lens, c.pitch_ss[0], c.pitch_ss[1], c.energy_ss[0], c.energy_ss[1],
                        c.pitch, c.energy, pc, ec, B, Pn, T)
            else:
                src = contours.pitch if contours.pitch is not None else contours.energy
                kk.call("kk_prosody_contour", pitch, energy, idx, lens, c.pitch_ss[0], c.pitch_ss[1], c.energy_ss[0], c.energy_ss[1],
                        c.pitch, c.energy, dur, contours.src_dur, contours.pitch, contours.energy, pc, ec, B, Pn, T, src.shape[1])
            kk.call("kk_bucket_embed_add_fwd", xf, pc, ec, P[f"{VA}.pitch_bins"],
                    P[f"{VA}.energy_bins"], P[f"{VA}.pitch_embedding.weight"], P[f"{VA}.energy_embedding.weight"], lens, memory,
                    pidx, eidx, fm2, B, T, H, d.var_bins, _b16(memory))
        self._cross_kv_fwd_all(memory, Nd, T, ddt, ns=ns)          # cross-attention K|V of every layer, normalised
        return memory, fm2

    def _controlled_durations(self, log_dur, controls, plens, B, Pn):
        """Durations under prosody controls (kk_prosody_durations on torch's expm1(log_dur), so that neutral controls give the bits
        of the torch line they replace).  Returns (dur int64 [B, Pn], row sums int64 [B])."""
        dur = torch.empty(B, Pn, dtype=torch.int64, device=self.device)
        sums = torch.empty(B, dtype=torch.int64, device=self.device)
        kk.call("kk_prosody_durations", torch.expm1(log_dur).contiguous(), controls.speed, controls.durations, plens, dur, sums, B, Pn)
        return dur, sums

    def _generation_bounds(self, expected, max_len, min_len_ratio, min_len_floor, max_len_ratio, max_len_cap, who=""):
        """(min, expected, max) frames of an utterance of `expected` predicted frames (model.py:741-750); `who` opens the message
        of the error."""
        lo = max(min_len_floor, int(expected * min_len_ratio))
        hi = min(max_len, max(expected + 80, int(expected * max_len_ratio)), max_len_cap)
        if hi <= lo:
            hi = min(max_len, lo + 1)
        if hi > self.dims.max_len:
            raise ValueError(f"{who}generation bound {hi} exceeds the positional table ({self.dims.max_len})")
        return lo, expected, hi

    def _decode_state_init(self, ns, B, max_expected):
        """Reset what _decode_step(ns, ...) carries from frame to frame: empty K / V caches, the all-zero first input frame,
        frame counter 0, every cache key masked.  Returns (mel_out [B, max_expected + 1, mel], stop_logit [max_expected, B], t_dev)."""
        d, ddt = self.dims, self.dec_dt
        for i in range(d.dec_layers):                              # (rows >= t are masked, but 0 * garbage must stay 0)
            self._buf(f"{ns}.dec{i}.kcache", max_expected, B * d.hidden, dtype=ddt).zero_()
            self._buf(f"{ns}.dec{i}.vcache", max_expected, B * d.hidden, dtype=ddt).zero_()
        mel_out = self._buf(f"{ns}.mel", B, max_expected + 1, d.mel)           # row 0 = the all-zero first input
        mel_out.zero_()
        t_dev = self._buf(f"{ns}.t", 1, dtype=torch.int32)
        t_dev.zero_()
        self._buf(f"{ns}.kmask", 1, max_expected, dtype=torch.uint8).fill_(1)
        return mel_out, self._buf(f"{ns}.stop", max_expected, B), t_dev

    def _capture(self, launches, *args) -> "torch.cuda.CUDAGraph":
        """One hipGraph of launches(*args): a decode step, a training micro-batch or the optimizer boundary that has run eagerly before."""
        with self.capture_lock:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # thread_local: with an RCCL process group alive, its watchdog thread polls events while we capture; only
            # this thread's calls must be capture-safe
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                launches(*args)
        return g

    def _decode_loop(self, step, stop, max_expected, check_every, decode_graph):
        """Run step() for up to max_expected frames; every `check_every` frames and after the last the host asks stop(t), t = the
        frame just decoded (a host sync), and leaves when it says so.  The step's launches take the frame index from device
        memory (kk_decode_*): their arguments are the same for every frame, so with decode_graph ONE captured hipGraph of the
        step serves the whole utterance (~100 launches per frame are host-bound when issued one by one)."""
        step_graph = None
        for t in range(max_expected):
            if step_graph is not None:
                step_graph.replay()
            else:
                step()                                     # frame 0 eagerly: it sizes the workspaces a capture may not allocate
                if decode_graph and max_expected > 1:
                    step_graph = self._capture(step)
            if ((t + 1) % check_every == 0 or t + 1 == max_expected) and stop(t):
                break

    @torch.no_grad()
    def generate(self, ids: torch.Tensor, stress: Optional[torch.Tensor] = None, max_len: int = 4000,
                 stop_threshold: float = 0.5, min_len_ratio: float = 0.7, min_len_floor: int = 12,
                 max_len_ratio: float = 3.0, max_len_cap: int = 1600, post_expected_stop_threshold: float = 0.2,
                 check_every: int = 16, decode_graph: bool = True, prosody=None) -> torch.Tensor:
        """KokoroModel.forward_inference (model/model.py:676-790) + KokoroGenerator.generate (model/generator.py:24-127):
        encode, expand by the model's own durations, pick the pitch / energy embeddings from its own (clamped)
        predictions (variance_predictor.py:338-439 without targets), then decode one mel frame at a time against a KV
        cache until the stop head fires, the output goes quiet or the length bound is reached.  Returns [B, frames, mel]
        clamped to [-11.5, 2] like the reference.  Weights: the engine's current parameters, dropout off.

        Decoder step = the training kernels at Sq = 1: the self-attention cache holds the NORMALISED (and, for K,
        rotated by the absolute position) heads time-major as [t][B*H], so one attention launch with B*heads "heads"
        serves the whole batch; the cross-attention K|V of all layers come from one GEMM (_cross_kv_fwd_all).  Like
        the reference, the single query of a step is rotated by position 0 (RoPE offsets default to 0 in its
        incremental path, transformers.py:276).  The stop decision needs the host; the reference syncs every frame,
        here the frames of `check_every` steps are decoded before the host looks (frames past the stop are dropped, so
        the result is the same).  decode_graph: frames 1.. are replays of ONE hipGraph of the step, captured after frame 0 ran
        eagerly (_decode_loop); False issues the same launches one by one.

        The stages are generate_batch's (_encode_text_fwd, _varpred_fwd, _expand_fwd, _generation_bounds, _decode_state_init,
        _decode_step, _decode_loop).  Up to the decode state they run on the train step's workspace keys (no prefix), so an
        engine that trains and synthesises shares those buffers; the decode state is under "gen.".

        prosody: a prosody.Prosody for every row, or a list of B (None entries: neutral), each over the Pn positions of the padded
        batch; None: the model's own durations, pitch and energy, by the launches issued without this argument."""
        d, H, M = self.dims, self.dims.hidden, self.dims.mel
        ids = ids.to(self.device, torch.int64).contiguous()
        stress = stress.to(self.device, torch.int64).contiguous() if stress is not None else None
        B, Pn = ids.shape
        prosody = prosody_list(prosody, B, "rows")
        controls = None if prosody is None else pack_prosody(prosody, [Pn] * B, Pn, self.device)
        contours = pack_contours(prosody, [Pn] * B, Pn, self.device)
        with self._no_dropout():
            text_mask = self._buf("gen.text_mask", B, Pn, dtype=torch.uint8)
            enc = self._encode_text_fwd("", ids, stress, B, Pn, text_mask)
            # ---- duration predictor ----
            log_dur = self._buf("out.log_dur", B, Pn)
            col_e = self._buf("vp.col_enc", B * Pn, 3 * H, dtype=self.enc_dt)
            kk.call("kk_im2col3_fwd", enc, col_e, None, B, Pn, H, CHUNK, _b16(col_e))
            self._varpred_fwd("vp.dur", f"{VA}.duration_predictor", enc, col_e, B, Pn, text_mask, log_dur)
            if controls is None:
                dur = torch.clamp(torch.round(torch.expm1(log_dur)), min=0).to(torch.int64)
                sums = dur.sum(dim=1)
            else:                                                  # (no row lengths: the reference's pads keep their durations)
                dur, sums = self._controlled_durations(log_dur, controls, None, B, Pn)
            expected = T = max(int(sums.max()), 3)                 # (host sync: the expanded length sizes everything below)
            if T > d.max_len:
                raise ValueError(f"predicted length {T} exceeds the positional table ({d.max_len})")
            memory, fm2 = self._expand_fwd("", enc, dur, B, Pn, T, controls=controls, contours=contours)
            min_expected, _, max_expected = self._generation_bounds(expected, max_len, min_len_ratio, min_len_floor, max_len_ratio,
                                                                    max_len_cap)
            mel_out, stop_logit, t_dev = self._decode_state_init("gen", B, max_expected)

            def step():
                frame_out, stop_now = self._decode_step("gen", B, T, max_expected, fm2)
                kk.call("kk_decode_epilogue", frame_out, stop_now, mel_out, stop_logit, t_dev, B, max_expected + 1, M)

            frames, done = max_expected, 0

            def stop(t):                                   # generator.py:67-88 over the frames [done, t] the host has not seen yet
                nonlocal frames, done
                sp = torch.sigmoid(stop_logit[done:t + 1]).mean(dim=1).cpu().tolist()
                mel_host = mel_out[:, 1:t + 2].float().cpu() if t + 1 >= 30 else None
                first, done = done, t + 1
                for tt in range(first, t + 1):
                    if tt < min_expected:
                        continue
                    thr = stop_threshold if tt < expected else min(stop_threshold, post_expected_stop_threshold)
                    if sp[tt - first] > thr or (tt + 1 >= 30 and float(mel_host[:, tt - 29:tt + 1].mean()) < -9.5):
                        frames = tt + 1
                        return True
                return False

            self._decode_loop(step, stop, max_expected, check_every, decode_graph)
            return mel_out[:, 1:frames + 1].clamp(min=-11.5, max=2.0).clone()

    def _check_utterances(self, utterances, stress):
        """The argument checks of generate_batch / generate_stream; returns (stress or None, phonemes per utterance)."""
        B = len(utterances)
        if stress is not None and len(stress) != B:
            raise ValueError(f"stress: {len(stress)} vectors for {B} utterances")
        if stress is not None and any(s is None for s in stress):
            if not all(s is None for s in stress):
                raise ValueError("stress must be given for every utterance or for none")
            stress = None
        lens_p = [int(u.numel()) for u in utterances]
        if min(lens_p) < 1:
            raise ValueError("empty utterance")
        if stress is not None and [int(s.numel()) for s in stress] != lens_p:
            raise ValueError("stress and phoneme vectors differ in length")
        if max(lens_p) > self.dims.max_len:
            raise ValueError(f"utterance of {max(lens_p)} phonemes exceeds the positional table ({self.dims.max_len})")
        return stress, lens_p

    def _prefill_rows(self, ns, utterances, stress, lens_p, first=0, frame_limit=None, prosody=None):
        """Everything of a ragged batch in front of the decode loop, on the workspace keys under `ns`: pad, encode, the duration
        predictor over each row's own phonemes, the expansion with each row's own frame count (_expand_fwd(flens=...)).  Error
        messages name utterance `first` + row; frame_limit: a row predicted longer raises before anything is expanded.
        prosody: one Prosody or None per row, or None for no controls at all (then no prosody kernel is launched); a row's
        frame-level contour is packed with the rows it is prefilled with (pack_contours) and so goes wherever the row goes.
        Returns (dur [B, Pn], T_b, T = max(T_b), memory, fm2)."""
        d, H = self.dims, self.dims.hidden
        B, Pn = len(utterances), max(lens_p)
        controls = None if prosody is None else pack_prosody(prosody, lens_p, Pn, self.device)
        contours = pack_contours(prosody, lens_p, Pn, self.device)       # (None unless a row carries a frame-level contour)
        ids_h = torch.zeros(B, Pn, dtype=torch.int64)
        st_h = torch.zeros(B, Pn, dtype=torch.int64) if stress is not None else None
        for b, u in enumerate(utterances):
            ids_h[b, :lens_p[b]] = u.reshape(-1).to("cpu", torch.int64)
            if st_h is not None:
                st_h[b, :lens_p[b]] = stress[b].reshape(-1).to("cpu", torch.int64)
        ids = ids_h.to(self.device)
        st = st_h.to(self.device) if st_h is not None else None
        text_mask = self._buf(ns + "text_mask", B, Pn, dtype=torch.uint8)
        enc = self._encode_text_fwd(ns, ids, st, B, Pn, text_mask)
        # ---- duration predictor, each row over its own P_b phonemes ----
        plens = torch.tensor(lens_p, dtype=torch.int32).to(self.device)
        log_dur = self._buf(ns + "out.log_dur", B, Pn)
        col_e = self._buf(ns + "vp.col_enc", B * Pn, 3 * H, dtype=self.enc_dt)
        kk.call("kk_im2col3_fwd", enc, col_e, plens, B, Pn, H, CHUNK, _b16(col_e))
        self._varpred_fwd(ns + "vp.dur", f"{VA}.duration_predictor", enc, col_e, B, Pn, text_mask, log_dur, lens=plens)
        if controls is None:
            dur = torch.clamp(torch.round(torch.expm1(log_dur)), min=0).to(torch.int64)
            sums = dur.sum(dim=1).cpu().tolist()               # (host sync: the row lengths size everything below)
        else:
            dur, sums = self._controlled_durations(log_dur, controls, plens, B, Pn)
            sums = sums.cpu().tolist()
        Tb = [max(int(s_), 3) for s_ in sums]
        for b, tb in enumerate(Tb):
            if tb > d.max_len:
                raise ValueError(f"utterance {first + b}: predicted length {tb} exceeds the positional table ({d.max_len})")
            if frame_limit is not None and tb > frame_limit:
                raise ValueError(f"utterance {first + b}: predicted length {tb} exceeds slot_frames ({frame_limit})")
        T = max(Tb)
        memory, fm2 = self._expand_fwd(ns, enc, dur, B, Pn, T, flens=torch.tensor(Tb, dtype=torch.int32).to(self.device),
                                       controls=controls, contours=contours)
        return dur, Tb, T, memory, fm2

    @torch.no_grad()
    def generate_batch(self, utterances: Sequence[torch.Tensor], stress: Optional[Sequence[torch.Tensor]] = None, *, max_len: int = 4000,
                       stop_threshold: float = 0.5, min_len_ratio: float = 0.7, min_len_floor: int = 12, max_len_ratio: float = 3.0,
                       max_len_cap: int = 1600, post_expected_stop_threshold: float = 0.2, check_every: int = 16,
                       decode_graph: bool = True, want_info: bool = False, prosody=None):
        """Synthesise a batch of utterances of different lengths; row b of the result equals generate() on utterance b alone (the
        reference's B = 1 forward_inference), not generate() on the padded batch, whose stop rule and predictors see the whole batch.

        utterances: phoneme-id vectors [P_b]; stress: one vector per utterance, or None.  Returns [mel_b [frames_b, mel]] in input
        order, clamped to [-11.5, 2]; with want_info also a dict of per-row "durations" [P_b], "T" (= T_b) and "bounds" (min_b,
        expected_b, max_b).

        Row lengths are those of the single-utterance call: L_b = P_b phonemes, T_b = max(sum(dur_b), 3) frames (frames in
        [sum(dur_b), T_b) are zero inputs that count in the predictors' convolutions and GroupNorms, as at B = 1).  The stages are
        generate's, on workspace keys of their own ("syn."): the duration, pitch and energy predictors are given the row lengths,
        which their kernels take as `lens` (_varpred_fwd(lens=...), _expand_fwd(flens=...)); the encoder (key mask), length regulator,
        bucket embeddings and cross-attention (frame mask) are row-independent already.  Each row has its own bounds
        (_generation_bounds) and its own stop rule, applied on the device by kk_decode_epilogue_rows inside the replayed step; the
        host reads only the count of live rows, every `check_every` frames.

        prosody: one prosody.Prosody for every utterance or one per utterance (None entries: neutral); None: no controls, the
        launches issued without this argument.  The controls act in the prefill only (durations, then pitch / energy per frame), so a row still equals what it
        gets alone under the same controls, and "durations" of want_info are the ones used.  A Prosody with a frame-level contour
        (pitch_contour / energy_contour) makes the prefill launch kk_prosody_contour in place of kk_prosody_variance; without one in
        the batch the launches are those of per-phoneme controls."""
        d, H, M = self.dims, self.dims.hidden, self.dims.mel
        B = len(utterances)
        if B == 0:
            return ([], {"durations": [], "T": [], "bounds": []}) if want_info else []
        stress, lens_p = self._check_utterances(utterances, stress)
        prosody = prosody_list(prosody, B)
        with self._no_dropout():
            dur, Tb, T, memory, fm2 = self._prefill_rows("syn.", utterances, stress, lens_p, prosody=prosody)
            bounds = []
            for b, expected in enumerate(Tb):
                bounds.append(self._generation_bounds(expected, max_len, min_len_ratio, min_len_floor, max_len_ratio, max_len_cap,
                                                      who=f"utterance {b}: "))
                if bounds[b][2] < 1:       # (max_len < 1; generate returns an empty mel there)
                    raise ValueError(f"utterance {b}: generation bound {bounds[b][2]} leaves no frame")
            max_expected = max(hi for _, _, hi in bounds)
            rb = torch.tensor([[r[k] for r in bounds] for k in range(3)], dtype=torch.int32).to(self.device)   # [3, B]: min | expected | max
            mel_out, stop_logit, t_dev = self._decode_state_init("syn", B, max_expected)
            done, frames_d = self._buf("syn.done", B, dtype=torch.uint8), self._buf("syn.frames", B, dtype=torch.int32)
            live = self._buf("syn.live", 1, dtype=torch.int32)
            done.zero_()
            frames_d.zero_()
            live.fill_(B)

            def step():
                frame_out, stop_now = self._decode_step("syn", B, T, max_expected, fm2)
                kk.call("kk_decode_epilogue_rows", frame_out, stop_now, mel_out, stop_logit, t_dev, done, frames_d, live, rb[0], rb[1],
                        rb[2], B, max_expected + 1, M, float(stop_threshold), float(post_expected_stop_threshold))

            self._decode_loop(step, lambda t: int(live.item()) == 0, max_expected, check_every, decode_graph)
            nf = frames_d.cpu().tolist()
            mels = [mel_out[b, 1:nf[b] + 1].clamp(min=-11.5, max=2.0).clone() for b in range(B)]
            if want_info:
                return mels, {"durations": [dur[b, :lens_p[b]].clone() for b in range(B)], "T": Tb, "bounds": bounds}
            return mels

    # ------------------------------------------------------------------ continuous batching
    def _stream_state(self, S, cap):
        """The slot pool's int32 state, one buffer [8, S] (+ the live count): t | done | frames | klen | clen | min | expected | max."""
        st = self._buf("str.state", 8, S, dtype=torch.int32)
        return {"all": st, "t": st[0], "done": st[1], "frames": st[2], "klen": st[3], "clen": st[4], "min": st[5], "exp": st[6],
                "max": st[7], "live": self._buf("str.live", 1, dtype=torch.int32)}

    def _stream_step(self, S, cap, stop_threshold, post_expected_stop_threshold):
        """One decoder step of a pool of S slots of `cap` frames, slot s at its own frame t_s: kk_decode_prologue_rows, _decoder_step
        with the row kernels of kk_decode.hip, kk_decode_epilogue_slots.  Self-attention: kk_attn_decode_rows over the slot-major
        caches [S][cap][H] with klen[s] = t_s + 1 keys (0 for a finished slot), no mask and no zero-filled cache.  Cross-attention:
        the same kernel over the slot's rows of the K|V pool [S*cap, 2H*layers] with clen[s] = the admitted group's frame count and
        the slot frame mask [S, cap].  The plain GEMMs are one k-slice each (split_k = 1: no fp32 atomics), so a replayed step
        repeats the bits of the eager one; at a few rows that gives up the k-split's extra workgroups."""
        d, P, H, M, h = self.dims, self.arena.P, self.dims.hidden, self.dims.mel, self.dims.heads
        ddt, L1, W = self.dec_dt, cap + 1, 2 * self.dims.hidden * self.dims.dec_layers
        st = self._stream_state(S, cap)
        pe, (cos, sin) = P["positional_encoding.pe"].view(d.max_len, H), self._rope_tables(d.max_len)
        mel_all, stop_all, frame_in = self._buf("str.mel", S, L1, M), self._buf("str.stop", S, cap), self._buf("str.frame_in", S, M)
        pool, fmask = self._buf("str.dec.ca.kv_n_pool", S * cap, W, dtype=ddt), self._buf("str.fmask", S, cap, dtype=torch.uint8)
        pe_rows, cos_rows, sin_rows = self._buf("str.pe_rows", S, H), self._buf("str.cos_rows", S, 64), self._buf("str.sin_rows", S, 64)
        kk.call("kk_decode_prologue_rows", mel_all, frame_in, pe, pe_rows, cos, sin, cos_rows, sin_rows, st["t"], st["done"], st["klen"],
                S, L1, M, H, d.max_len)

        def self_attn(i, key, nrm):
            qb = self._buf(key + ".q", S, H, dtype=ddt)
            Kc, Vc = self._buf(key + ".kcache", S, cap, H, dtype=ddt), self._buf(key + ".vcache", S, cap, H, dtype=ddt)
            kk.call("kk_decode_cache_append_rows", nrm, qb, Kc, Vc, st["t"], st["done"], S, cap, H, _b16(nrm))
            ctx, lse = self._buf(key + ".ctx", S, H, dtype=ddt), self._buf(key + ".lse", S, h)
            kk.call("kk_attn_decode_rows", qb, Kc, Vc, ctx, lse, st["klen"], None, S, h, cap, cap * H, H, cap * H, H, 0.125, _b16(qb))
            return ctx

        def cross_attn(i, key, q_n):
            k_n, v_n = pool[:, 2 * H * i:], pool[:, 2 * H * i + H:]
            ctx, lse = self._buf(key + ".ca.ctx", S, H, dtype=ddt), self._buf(key + ".ca.lse", S, h)
            kk.call("kk_attn_decode_rows", q_n, k_n, v_n, ctx, lse, st["clen"], fmask, S, h, cap, cap * W, W, cap * W, W, 0.125, _b16(q_n))
            return ctx

        frame_out, stop_now = self._decoder_step("str", S, pe_rows, 0, cos_rows, sin_rows, S, 1, self_attn, cross_attn)
        kk.call("kk_decode_epilogue_slots", frame_out, stop_now, mel_all, stop_all, st["t"], st["done"], st["frames"], st["live"],
                st["min"], st["exp"], st["max"], S, L1, M, float(stop_threshold), float(post_expected_stop_threshold))

    @torch.no_grad()
    def generate_stream(self, utterances: Sequence[torch.Tensor], stress: Optional[Sequence[torch.Tensor]] = None, *, slots: int = 32,
                        slot_frames: Optional[int] = None, max_len: int = 4000, stop_threshold: float = 0.5, min_len_ratio: float = 0.7,
                        min_len_floor: int = 12, max_len_ratio: float = 3.0, max_len_cap: int = 1600,
                        post_expected_stop_threshold: float = 0.2, check_every: int = 16, decode_graph: bool = True,
                        want_info: bool = False, prosody=None):
        """generate_batch with continuous batching: the utterances are decoded in a pool of `slots` slots of `slot_frames` frames and
        a finished row's slot is refilled with the next utterance, so the decode steps are spent on live rows instead of lasting as
        long as the longest row of a fixed batch.  Arguments, results (in input order) and the want_info dict are generate_batch's.
        Every mel is what generate_batch([u]) gives for that utterance alone (within 1e-4 in fp32) as long as slot_frames does not
        cut the row's bound: slot_frames (default min(max_len_cap, the positional table)) bounds both T_b and the generation bound
        of a row, which is computed with max_len_cap = min(max_len_cap, slot_frames).  An utterance predicted longer than
        slot_frames raises ValueError naming its index before anything of it is decoded.

        Admission: whenever slots are free and utterances remain, generate_batch's prefill stages (_prefill_rows, the same
        launches) run on the next group on workspace keys "str.adm.", with their host sync for the row lengths; then kk_slot_admit
        files the group's cross-attention K|V, frame mask and bounds under its slots.  A refill group is often one utterance.
        Step: _stream_step; its buffers depend on (slots, slot_frames) alone, so one captured hipGraph serves the call unless an
        admission regrows a workspace (which drops every graph of the engine, _invalidate): then the next step runs eagerly and
        is captured again.  Workspaces only grow, so that dies out after the first few admissions of an engine's life.
        Harvest: every `check_every` frames the host reads done | frames in one copy, clones the finished slots' mels and admits
        into them; the steps of a block behind the last finished row run with every slot done.  Idle slots have done = 1 and
        klen = 0.
        prosody: as in generate_batch; an utterance's controls go with it into whichever admission group prefills it."""
        d, H, M = self.dims, self.dims.hidden, self.dims.mel
        N = len(utterances)
        if N == 0:
            return ([], {"durations": [], "T": [], "bounds": []}) if want_info else []
        S = int(slots)
        cap = int(min(max_len_cap, d.max_len) if slot_frames is None else slot_frames)    # (no row outgrows the positional table)
        if S < 1 or cap < 1 or check_every < 1:
            raise ValueError("slots, slot_frames and check_every must be positive")
        if cap > d.max_len:
            raise ValueError(f"slot_frames {cap} exceeds the positional table ({d.max_len})")
        if cap > 8192:
            raise ValueError(f"slot_frames {cap} exceeds the decode attention's 8192 keys")
        stress, lens_p = self._check_utterances(utterances, stress)
        prosody = prosody_list(prosody, N)
        for i, pr in enumerate(prosody or ()):                     # (before anything is decoded, not at the utterance's admission)
            if pr is not None:
                try:
                    pr.validate(lens_p[i])
                except ValueError as e:
                    raise ValueError(f"utterance {i}: {e}") from None
        with self._no_dropout():
            ddt, L1, W = self.dec_dt, cap + 1, 2 * H * d.dec_layers
            st = self._stream_state(S, cap)
            mel_all = self._buf("str.mel", S, L1, M)
            pool, fmask = self._buf("str.dec.ca.kv_n_pool", S * cap, W, dtype=ddt), self._buf("str.fmask", S, cap, dtype=torch.uint8)
            st["all"].zero_()
            st["done"].fill_(1)                            # every slot idle: klen = 0, nothing of it is read or written
            st["live"].zero_()
            mel_all[:, 0].zero_()
            fmask.fill_(1)
            mels, durs, Ts, bounds = [None] * N, [None] * N, [None] * N, [None] * N
            owner = [-1] * S                               # utterance in each slot
            nxt = 0

            def admit():
                nonlocal nxt
                free = [s for s in range(S) if owner[s] < 0]
                n = min(len(free), N - nxt)
                if n == 0:
                    return
                grp = list(range(nxt, nxt + n))
                dur, Tb, T, memory, fm2 = self._prefill_rows("str.adm.", [utterances[i] for i in grp],
                                                             [stress[i] for i in grp] if stress is not None else None,
                                                             [lens_p[i] for i in grp], first=nxt, frame_limit=cap,
                                                             prosody=[prosody[i] for i in grp] if prosody is not None else None)
                rb = []
                for r, i in enumerate(grp):
                    b3 = self._generation_bounds(Tb[r], max_len, min_len_ratio, min_len_floor, max_len_ratio, min(max_len_cap, cap),
                                                 who=f"utterance {i}: ")
                    if b3[2] < 1:
                        raise ValueError(f"utterance {i}: generation bound {b3[2]} leaves no frame")
                    if b3[2] > cap:
                        raise ValueError(f"utterance {i}: generation bound {b3[2]} exceeds slot_frames ({cap})")
                    rb.append(b3)
                    durs[i], Ts[i], bounds[i] = dur[r, :lens_p[i]].clone(), Tb[r], b3
                kv_n = self._buf("str.adm.dec.ca.kv_n_all", n * T, W, dtype=ddt)      # (_expand_fwd -> _cross_kv_fwd_all wrote it)
                dev = torch.tensor([free[:n]] + [[r[k] for r in rb] for k in range(3)], dtype=torch.int32).to(self.device)   # slots | bounds [3, n]
                kk.call("kk_slot_admit", kv_n, pool, fm2, fmask, dev[0], dev[1:], st["t"], st["done"], st["frames"], st["clen"], st["min"],
                        st["exp"], st["max"], mel_all, st["live"], n, T, S, cap, W * kv_n.element_size(), L1, M)
                for r, i in enumerate(grp):
                    owner[free[r]] = i
                nxt += n

            step = lambda: self._stream_step(S, cap, stop_threshold, post_expected_stop_threshold)
            admit()
            graph, graph_at = None, None
            while any(o >= 0 for o in owner):
                for _ in range(check_every):
                    if graph is not None and self.ws_generation == graph_at:
                        graph.replay()
                        continue
                    # no graph yet, or an admission regrew a workspace or evicted tables and its addresses are stale: this step
                    step()                                 # eagerly (it sizes the workspaces a capture may not allocate)
                    if decode_graph:
                        graph, graph_at = self._capture(step), self.ws_generation
                host = st["all"][1:3].cpu().tolist()       # done | frames: the one copy of a harvest
                for s in range(S):
                    if owner[s] >= 0 and host[0][s]:
                        mels[owner[s]] = mel_all[s, 1:host[1][s] + 1].clamp(min=-11.5, max=2.0).clone()
                        owner[s] = -1
                admit()
            if want_info:
                return mels, {"durations": durs, "T": Ts, "bounds": bounds}
            return mels

    # ------------------------------------------------------------------ optimizer boundary
    def _opt_cfg(self, mel_length: int) -> kk.KkOptCfg:
        hp = self.hp
        c = spec.lr_schedule_consts(hp, self.total_steps)
        return kk.KkOptCfg(c["learning_rate"], c["max_lr"], c["warmup_start_lr"], c["warmup_target_lr"], c["pct_start"],
                           c["div_factor"], c["final_div_factor"], c["warmup_steps"], c["onecycle_steps"], c["use_warmup"],
                           hp.adam_betas[0], hp.adam_betas[1], hp.adam_eps, hp.max_grad_norm, mel_length,
                           hp.grad_explosion_ema_alpha, hp.grad_explosion_abs_floor, hp.grad_explosion_multiplier,
                           hp.grad_explosion_warmup_floor, hp.grad_explosion_warmup_steps, hp.grad_explosion_min_ema_steps,
                           hp.ema_decay, hp.dec_ffn_max_weight_norm, max(1, int(hp.ema_update_every)),
                           0 if hp.use_onecycle_lr else 1,
                           0.0 if hp.use_onecycle_lr else spec.cosine_restart_factor(self.lr_epoch, hp.lr_T_0, hp.lr_T_mult),
                           hp.lr_eta_min)

    def zero_grad(self) -> None:
        self.arena.g.zero_()

    def _ow_key(self) -> Tuple:
        return (self.math, self.enc_dt, self.dec_dt, self.use_shadow, self.group_wgrads)

    def _zero_grad_step(self) -> None:
        """The zero-fill inside a step (forward_backward(zero_grads=True)): everything, or — once a step of this precision mode
        has been seen — everything but the tensors its grouped weight-gradient launches overwrite, as ONE kk_zero_many launch."""
        a = self.arena
        rec = self._ow_sets.get(self._ow_key()) if self.zero_skip_overwritten else None
        if not rec:
            self._ow_expect = None
            self.zero_grad()
            return
        self._ow_expect = rec

        def build():
            base, spans, pos = a.g.data_ptr(), [], 0
            for ptr, n in sorted(rec):
                b = (ptr - base) // 4
                if b < pos or b % 4 or n % 4:
                    raise RuntimeError("overlapping or misaligned weight-gradient tensors in the overwrite record")
                if b > pos:
                    spans.append(a.g[pos:b])
                pos = b + n
            if pos < a.total:
                spans.append(a.g[pos:a.total])
            return [kk.zero_table(spans[i:i + 160]) for i in range(0, len(spans), 160)]
        for dst, nbytes, n in self._table(("zero", a.g.data_ptr(), rec), build):
            kk.call("kk_zero_many", dst, nbytes, n)

    def optimizer_step(self, mel_length: int, tile_norms=None) -> None:
        """Pre-clip → total norm → non-finite skip / explosion tracker / adaptive + global clip → fused AdamW+EMA →
        FFN weight-norm projection.  All decisions on the device (see csrc/kk_optim.hip).
        tile_norms = (segments, records) from the micro-batch right in front (finish_cycle passes _ss_ready; see grad_norm_from_wgrads):
        the norm pass skips those segments — only for callers that have not touched the gradient arena in between."""
        a, hp = self.arena, self.hp
        cfg = self._opt_cfg(mel_length)
        self._mark("optimizer start")
        skip, extra = None, 0
        if tile_norms is not None and tile_norms[1] > 0:
            skip = self._ss_masks.get(tile_norms[0])
            if skip is None and not torch.cuda.is_current_stream_capturing():
                m = torch.zeros(a.nseg, dtype=torch.int32)
                m[sorted(tile_norms[0])] = 1
                skip = self._ss_masks[tile_norms[0]] = m.to(self.device)
            extra = tile_norms[1] if skip is not None else 0
        # grad_sumsq: every segment stored once per call by kk_seg_sumsq (records merged in a fixed order: replicas agree bit for bit).
        # p_sumsq (fixed-point atomics) is private to this sequence: kk_opt_prepare, the one-workgroup launch in front of its writer,
        # leaves it zero — no zero-fill launch on the optimizer's chain.
        with self._acc_guard():
            sc = 1 if self.self_cleaning_acc else 0
            kk.call("kk_seg_sumsq", a.g, a.block_seg, a.nblocks, self.grad_sumsq, a.nseg, self.sumsq_ws, skip, extra)
            kk.call("kk_opt_prepare", self.grad_sumsq, a.seg_preclip, a.seg_lr_mult, a.seg_wd, a.nseg, self.max_dur, cfg,
                    self.opt_state, self.seg_gscale, self.seg_decay, self.seg_stepsize, self.step_consts,
                    None, self.p_sumsq if sc else None)
            kk.call("kk_adamw_ema", a.p, a.g, a.m, a.v, a.ema, a.block_seg, a.nblocks, self.seg_gscale, self.seg_decay,
                    self.seg_stepsize, a.seg_flags, self.step_consts, hp.adam_betas[0], hp.adam_betas[1], hp.ema_decay,
                    self.p_sumsq, a.nseg, a.p16, sc)
            kk.call("kk_weight_norm_project", a.p, a.block_seg, a.nblocks, self.p_sumsq, a.seg_flags, self.step_consts,
                    float(hp.dec_ffn_max_weight_norm), a.p16)
        self._mark("optimizer done")

    def train_step(self, batch: Dict[str, torch.Tensor], accumulation_divisor: Optional[int] = None,
                   boundary: Optional[bool] = None, grad_sync=None, expanded_len: Optional[int] = None) -> torch.Tensor:
        """One micro-batch of training in the reference's order (trainer.py:2257-2477): zero grads at the start of an
        accumulation cycle, forward+backward with loss_scale = adaptive/divisor, optimizer boundary when the cycle
        completes.  Returns the device tensor of 6 losses (no host sync).  The cycle itself is micro_batch + finish_cycle."""
        losses = self.micro_batch(batch, accumulation_divisor, boundary, grad_sync, expanded_len)
        if self._last_micro.boundary:
            self.finish_cycle(grad_sync)
        return losses

    # ------------------------------------------------------------------ the accumulation cycle
    def _micro(self, T: int, accumulation_divisor, boundary, grad_sync) -> _Micro:
        """Where the next micro-batch (T mel frames) stands in its accumulation cycle: the only copy of the defaults."""
        G = max(1, int(self.hp.gradient_accumulation_steps))
        div = int(accumulation_divisor) if accumulation_divisor is not None else G
        return _Micro(first=self.micro_in_cycle == 0, boundary=bool(boundary) if boundary is not None else self.micro_in_cycle + 1 >= G,
                      div=div, scale=self.dp_loss_scale / div, mel_length=canonical_mel_length(self.global_mel_length, T),
                      external_sync=grad_sync is not None)

    @contextlib.contextmanager
    def _micro_flags(self, m: _Micro):
        """Around the launch sequence of a micro-batch, run or captured: the only writer of _exchange_now, _first_micro and
        _external_sync besides __init__.  A sequence that raises leaves them as they are between steps too."""
        self._exchange_now, self._first_micro, self._external_sync = m.boundary, m.first, m.external_sync
        try:
            yield
        finally:
            self._exchange_now, self._first_micro, self._external_sync = True, False, False

    def micro_batch(self, batch: Dict[str, torch.Tensor], accumulation_divisor: Optional[int] = None, boundary: Optional[bool] = None,
                    grad_sync=None, expanded_len: Optional[int] = None, _zero_in_step: bool = False, _graphs: Optional[Dict] = None) -> torch.Tensor:
        """One micro-batch of an accumulation cycle.  Returns the 6 losses; at the boundary (_last_micro) the caller runs finish_cycle
        with the same grad_sync.  For train_step_graphed: _zero_in_step = the fill of forward_backward(zero_grads=True) instead of
        zero_grad() in front; _graphs = a shape's entry of the graph cache: the launches are replayed from it instead of issued."""
        m = self._micro(batch["mel_specs"].shape[1], accumulation_divisor, boundary, grad_sync)
        if _graphs is not None:
            self._stage(_graphs["static"], batch)
            with self._acc_guard():                    # (a replayed graph assumes the accumulators' zero state like an eager step)
                graph, tile_norms = self._fb_graph(_graphs, m, expanded_len)
                graph.replay()
                self._ss_ready = tile_norms
        else:
            if m.first and not _zero_in_step:
                self.zero_grad()
            with self._micro_flags(m):
                self._fb(batch, m.scale, True, True, m.first and _zero_in_step, expanded_len)
        self.micro_in_cycle += 1
        self._last_micro = m
        return self.losses

    def finish_cycle(self, grad_sync=None, _graphs: Optional[Dict] = None) -> None:
        """The boundary of an accumulation cycle: grad_sync(arena.g) if given (data parallel: SUM over ranks, dp.GradSync), the
        optimizer pass (replayed from _graphs like micro_batch's launches) and the reset."""
        m = self._last_micro
        if m is None or m.external_sync != (grad_sync is not None):
            raise RuntimeError("finish_cycle: no micro_batch since the last boundary, or not the grad_sync that micro_batch was given")
        if grad_sync is not None:
            grad_sync(self.arena.g)
        tile_norms = None if m.external_sync else self._ss_ready       # (records of the unreduced gradient say nothing of the reduced one)
        if _graphs is None:
            self.optimizer_step(m.mel_length, tile_norms)
        else:
            with self._acc_guard():
                self._opt_graph(_graphs, m.mel_length, tile_norms).replay()
        self._ss_ready, self._last_micro, self.micro_in_cycle = None, None, 0

    def drop_cycle(self) -> None:
        """Give up the accumulation cycle in flight (the trainer's strict guard, on a flagged micro-batch): the next micro-batch opens a new one."""
        self.opt_state[kk.OS["MICRO_BAD"]].zero_()
        self.zero_grad()
        self._ss_ready, self._last_micro, self.micro_in_cycle = None, None, 0

    def train_step_auto(self, batch: Dict[str, torch.Tensor], accumulation_divisor: Optional[int] = None,
                        boundary: Optional[bool] = None, grad_sync=None, expanded_len: Optional[int] = None) -> torch.Tensor:
        """train_step for a stream of batches whose shapes may or may not repeat (the trainer's entry point): a shape that
        comes back is replayed from hipGraphs (train_step_graphed: ~0.2 ms of host time instead of ~2.5 ms for ~700
        launches), a shape seen for the first time runs eagerly.  Large dynamic batches (max_frames 16384: 15-20 ms of
        GPU time per step) hide the eager launches anyway; small fixed shapes are where the graphs pay.  At most
        max_graphs shapes are kept (least recently used first out)."""
        key = self._shape_key(batch, expanded_len)
        if self._loss_sync_capturable():               # (a torch.distributed loss exchange is eager)
            if key in self._graphs:
                return self.train_step_graphed(batch, grad_sync, accumulation_divisor, boundary, expanded_len)
            n = self._shape_seen.get(key, 0) + 1
            self._shape_seen[key] = n
            self._shape_seen.move_to_end(key)
            if len(self._shape_seen) > 4096:
                self._shape_seen.popitem(last=False)
            if n >= 2:
                return self.train_step_graphed(batch, grad_sync, accumulation_divisor, boundary, expanded_len)
        return self.train_step(batch, accumulation_divisor, boundary, grad_sync, expanded_len)

    # ------------------------------------------------------------------ hipGraph replay of a whole step
    @staticmethod
    def _shape_key(batch, expanded_len) -> Tuple[int, int, int, int]:
        """What the graph cache and train_step_auto's first-sight count know a batch shape by: (B, T, phonemes, T')."""
        B, T = batch["mel_specs"].shape[:2]
        return (B, T, batch["phoneme_indices"].shape[1], T if expanded_len is None else int(expanded_len))

    def _loss_sync_capturable(self) -> bool:
        return self.loss_sync is None or getattr(self.loss_sync, "capturable", False)

    def _stage(self, static: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        """Copy a batch into the static tensors that the graphs of its shape read."""
        moved = []
        for k, v in batch.items():
            d = static[k]
            if v.data_ptr() == d.data_ptr():
                continue
            if v.shape == d.shape and v.dtype == d.dtype and v.device == d.device and v.is_contiguous() and d.is_contiguous():
                moved.append((d, v))
            else:
                d.copy_(v, non_blocking=True)
        if moved:
            kk.copy_many(moved)                        # one launch for the whole batch

    def _fb_graph(self, ent: Dict, m: _Micro, expanded_len) -> Tuple["torch.cuda.CUDAGraph", Optional[Tuple]]:
        """(graph, tile-norm records its launches leave: the same at every replay) of micro-batch m for the shape's cache entry ent."""
        key = _FbKey(m.div, m.first, self.train_dropout, self.spec_augment_active, self.math, self.dp_comm is not None and m.boundary,
                     m.mel_length if self.loss_sync is not None else 0, self.loss_sync is not None, self.self_cleaning_acc,
                     (self.attn_keep_gen, self.attn_keep_gen_rate), self.grad_norm_from_wgrads and not m.external_sync)
        fbe = ent["fb"].get(key)
        if fbe is None:
            with self._micro_flags(m):
                g = self._capture(self._fb, ent["static"], m.scale, True, True, m.first, expanded_len)
            fbe = ent["fb"][key] = (g, self._ss_ready)
        return fbe

    def _opt_graph(self, ent: Dict, mel_length: int, tile_norms) -> "torch.cuda.CUDAGraph":
        """The optimizer-boundary graph for the shape whose cache entry is ent, captured at first use."""
        # (KkOptCfg travels by value: the legacy schedule's factor changes once per epoch -> one re-capture per epoch; the graphs of
        #  earlier epochs are dropped then — they can never be replayed again and would otherwise pile up, epochs x shapes: ADVICE r5)
        epoch = 0 if self.hp.use_onecycle_lr else self.lr_epoch
        for k in [k for k in ent["opt"] if k[1] != epoch]:
            torch.cuda.synchronize(self.device)       # (a graph about to be destroyed may still be running)
            del ent["opt"][k]
        if tile_norms is not None and tile_norms[0] not in self._ss_masks:       # (its skip table is built by an eager boundary only: no copies under capture)
            tile_norms = None
        key = (mel_length, epoch, self.self_cleaning_acc, tile_norms)
        if key not in ent["opt"]:
            ent["opt"][key] = self._capture(self.optimizer_step, mel_length, tile_norms)
        return ent["opt"][key]

    def train_step_graphed(self, batch: Dict[str, torch.Tensor], grad_sync=None, accumulation_divisor: Optional[int] = None,
                           boundary: Optional[bool] = None, expanded_len: Optional[int] = None) -> torch.Tensor:
        """Same semantics as train_step (gradient accumulation included), but the kernel sequence of a micro-batch is
        captured once per (batch shape, accumulation divisor, first-of-cycle) into hipGraphs and replayed (a step is ~700
        launches; eager launch overhead would dominate), and the optimizer boundary once per (shape, mel length).
        `grad_sync` (data parallel) runs between the backward graph and the optimizer graph.  The first call with a new
        shape runs eagerly: it sizes the workspace and builds the descriptor tables, neither of which may happen inside
        a capture: micro_batch + finish_cycle like train_step.  A replay takes the same _micro record and the same finish_cycle."""
        if not self._loss_sync_capturable():
            raise RuntimeError("train_step_graphed: this loss_sync exchanges the loss counts through torch.distributed between "
                               "kernels of the step, which a hipGraph cannot hold; use train_step, or the RCCL exchange "
                               "(dp.BucketedExchange, backend 'rccl'), whose collectives are captured with the step")
        key = self._shape_key(batch, expanded_len)
        ent = self._graphs.get(key)
        if ent is None:                               # first sight of a shape: eager (allocates the workspaces and the
            static = {k: v.clone() for k, v in batch.items()}      # reduction tables — host-to-device copies, illegal in a capture)
            self.micro_batch(static, accumulation_divisor, boundary, grad_sync, expanded_len, _zero_in_step=True)
            # (registered only now: growing a buffer during the eager pass drops every graph entry)
            if len(self._graphs) >= self.max_graphs:
                torch.cuda.synchronize(self.device)   # a graph about to be destroyed may still be running
                self._graphs.popitem(last=False)
            self._graphs[key] = {"static": static, "fb": {}, "opt": {}}
        else:
            self._graphs.move_to_end(key)
            self.micro_batch(batch, accumulation_divisor, boundary, grad_sync, expanded_len, _graphs=ent)
        if self._last_micro.boundary:
            self.finish_cycle(grad_sync, _graphs=ent)      # (ent is None on first sight: the boundary runs eagerly too)
        return self.losses

    def encoder_stack_error(self) -> int:
        """Non-zero when a group barrier of kk_encoder_stack_fwd has timed out since the last reset (host read: synchronises)."""
        return int(self._enc_sync[0].item())

    def check_encoder_stack(self) -> None:
        """Raise if a group barrier of the persistent encoder launch has timed out.  kk_encoder_stack_fwd is a plain launch whose
        256 workgroups must be co-resident; every spin is bounded, and a workgroup that gives up sets word 0 of the sync buffer
        and carries on with stale activations — the step (and every later one: the word makes later barriers fall through) is
        then garbage that no finite-value guard sees.  The trainer calls this wherever it synchronises anyway (end of an epoch,
        before validation, before a checkpoint is written).  Handling it = clear the word (so later launches wait again), fall
        back to the per-kernel encoder for the rest of the run, drop the graphs that hold the launch, and fail the caller: the
        weights since the last check cannot be trusted."""
        # data parallel: the ranks decide TOGETHER — a rank that raised alone would leave the others waiting in the next
        # collective.  The check sits at the trainer's sync points (epoch end, validation, checkpoint), which every rank reaches, and
        # EVERY rank enters the all-reduce — also one whose own fused launch is already off (it contributes 0; ADVICE r4: returning
        # early there left the other ranks alone in the collective).
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if not self.enc_fused and not multi:
            return
        code = self.encoder_stack_error() if self.enc_fused else 0
        if multi:
            word = torch.tensor([code], dtype=torch.int64, device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(word, op=dist.ReduceOp.MAX)
            code = int(word.item())
        if code:
            self._enc_sync.zero_()
            if self.enc_fused:
                self.enc_fused = False
                self._graphs.clear()
            raise RuntimeError(f"kk_encoder_stack_fwd: a group barrier timed out (code {code}); the activations of at least one "
                               "step were stale.  The fused encoder launch is now off for this engine (per-kernel sequence); "
                               "reload the last checkpoint before continuing.")

    def opt_stats(self) -> Dict[str, float]:
        """Host read-back of the device optimizer state (synchronises; for logging/tests only)."""
        s = self.opt_state.cpu().tolist()
        return {k.lower(): s[v] for k, v in kk.OS.items() if k != "SIZE"}
