"""Shared by test_engine_launches_gpu.py and tools/record_engine_launches.py: a recorder of the launches one engine call issues, in a
form that holds no raw address, and the cases both files run.  Not a test.

What is recorded.  For the duration of one engine call the recorder stands in for kk.call, for kk_attn_warm_next on the loaded library
object and for kk.reduce_table.  Per launch it keeps [entry-point name, stream namespace, canonical arguments]:
  scalars         as they are (floats by repr);
  tensors         ["T", owner, byte offset within the owner, dtype, shape, strides]; the owner is the workspace name (engine._ws),
                  the arena slab, "batch.<key>" or the engine attribute whose storage contains the address;
  ctypes values   structures field by field, arrays element by element, pointers (c_void_p fields and elements, and integers that
                  lie inside an owner) as [owner, byte offset];
  reduce table    the device-resident KkReduceDesc array, as the host entries kk.reduce_table built it from.
A buffer that moves, or is first requested in another order, therefore records the same; a wrong stride, a wrong buffer, a missing or
reordered launch does not.

The descriptor tables are dropped (engine._invalidate) before the recorded call, so that every table of the call, the reduce table
among them, is built inside it; and each training case runs once unrecorded first, so that the record is the steady state of its
configuration whatever ran on the engine before."""
import bisect
import contextlib
import ctypes as C
import hashlib
import json

import torch

from kokoro_ruslan_amd import lib as kk

_SKIP_ATTRS = {"_ws", "_views", "_tables", "_graphs", "arena"}


def _walk(prefix, v, depth, out):
    """(name, tensor) for every tensor reachable from v through dicts, lists and tuples, in a fixed order."""
    if torch.is_tensor(v):
        out.append((prefix, v))
    elif depth > 0 and isinstance(v, dict):
        for i, (k, x) in enumerate(v.items()):
            _walk(f"{prefix}[{k}]" if isinstance(k, (str, int)) else f"{prefix}[#{i}]", x, depth - 1, out)
    elif depth > 0 and isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _walk(f"{prefix}[{i}]", x, depth - 1, out)


class LaunchRecorder:
    def __init__(self, eng, batch=None):
        self.eng, self.batch = eng, batch or {}
        self.launches = []                              # [name, stream namespace, canonical arguments]
        self.unowned = 0                                # tensors and pointers no owner contains (temporaries of torch's allocator)
        self._reduce = {}                               # data_ptr of a device reduce table -> its canonical host entries
        self._starts, self._spans, self._stamp = [], [], None

    # ---- owners -------------------------------------------------------------------------------------------------------------------
    def _owners(self):
        named = [("ws." + k, t) for k, t in self.eng._ws.items()]
        named += [("arena." + n, t) for n, t in sorted(vars(self.eng.arena).items()) if torch.is_tensor(t)]
        named += [("batch." + k, t) for k, t in self.batch.items() if torch.is_tensor(t)]
        for n, v in sorted(vars(self.eng).items()):
            if n not in _SKIP_ATTRS:
                _walk("eng." + n, v, 3, named)
        spans, seen = [], set()
        for name, t in named:
            if not t.is_cuda:
                continue
            s = t.untyped_storage()
            if s.data_ptr() and s.data_ptr() not in seen:          # (views share a storage: the first name in the order above owns it)
                seen.add(s.data_ptr())
                spans.append((s.data_ptr(), s.data_ptr() + s.nbytes(), name))
        spans.sort()
        self._spans, self._starts = spans, [s[0] for s in spans]

    def _lookup(self, addr):
        i = bisect.bisect_right(self._starts, addr) - 1
        if i >= 0 and addr < self._spans[i][1]:
            return [self._spans[i][2], addr - self._spans[i][0]]
        return None

    def _addr(self, addr, strict=True):
        """[owner, byte offset] of a device address; strict=False: None for what no owner contains (an integer that is no address)."""
        if not addr:
            return None
        stamp = (len(self.eng._ws), self.eng.ws_bytes, self.eng.ws_generation)
        if stamp != self._stamp:
            self._owners()
            self._stamp = stamp
        hit = self._lookup(addr)
        if hit is None:
            self._owners()                              # (an attribute the call made meanwhile: the positional tables, ...)
            hit = self._lookup(addr)
        if hit is None and strict:
            self.unowned += 1
            return ["unowned", 0]
        return hit

    # ---- canonical form -------------------------------------------------------------------------------------------------------------
    def canon(self, a):
        if a is None or isinstance(a, str):
            return a
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, int):
            hit = self._addr(a, strict=False) if a >= 1 << 32 else None
            return a if hit is None else ["P"] + hit
        if isinstance(a, float):
            return repr(a)
        if torch.is_tensor(a):
            if a.data_ptr() in self._reduce:
                return ["reduce_table", self._reduce[a.data_ptr()]]
            own = self._addr(a.data_ptr()) if a.is_cuda else ["host", 0]
            return ["T"] + (own or ["null", 0]) + [str(a.dtype), list(a.shape), list(a.stride())]
        if isinstance(a, C.Structure):
            return {"struct": type(a).__name__,
                    "fields": [[n, self._field(getattr(a, n), t)] for n, t, *_ in a._fields_]}
        if isinstance(a, C.Array):
            return [self._field(x, a._type_) for x in a]
        if hasattr(a, "_obj"):                          # ctypes.byref(x)
            return ["byref", self.canon(a._obj)]
        if hasattr(a, "value"):                         # a ctypes scalar
            return self._field(a.value, type(a))
        if isinstance(a, (list, tuple)):
            return [self.canon(x) for x in a]
        raise TypeError(f"launch argument of type {type(a).__name__} has no canonical form")

    def _field(self, v, ctype):
        if ctype is C.c_void_p:
            return None if not v else ["P"] + self._addr(v)
        if isinstance(v, (C.Structure, C.Array)):
            return self.canon(v)
        return repr(v) if isinstance(v, float) else v

    # ---- the three wrappers -----------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def recording(self):
        lib = kk.load()
        real_call, real_warm, real_reduce = kk.call, lib.kk_attn_warm_next, kk.reduce_table

        def call(name, *args):
            self.launches.append([name, self.eng._tmp_ns, [self.canon(a) for a in args]])
            real_call(name, *args)

        def warm(*args):
            self.launches.append(["kk_attn_warm_next", self.eng._tmp_ns, [self.canon(a) for a in args]])
            return real_warm(*args)

        def reduce_table(entries, device):
            t = real_reduce(entries, device)
            self._reduce[t.data_ptr()] = [self.canon(e) for e in entries]
            return t

        self.eng._invalidate()
        kk.call, lib.kk_attn_warm_next, kk.reduce_table = call, warm, reduce_table
        try:
            yield self
        finally:
            kk.call, lib.kk_attn_warm_next, kk.reduce_table = real_call, real_warm, real_reduce

    def digest(self):
        """[[name, first 16 hex digits of the SHA-256 of the canonical arguments]] of every recorded launch."""
        return [[name, hashlib.sha256(json.dumps([ns, args], sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:16]]
                for name, ns, args in self.launches]


# ------------------------------------------------------------------------------------------------------------------ the cases
# engines: name -> (math_mode, storage); default ModelDims, gradient_accumulation_steps = 1, weights of init_params(seed 0)
ENGINES = {"bf16": ("bf16", "auto"), "f32": ("f32", "auto"), "bf16-dec": ("bf16", "bf16-dec")}

# training cases: id -> (engine, (B, T, Pn), engine attributes set for the call, forward_backward keywords); dropout is on unless
# the case turns it off.  The shapes are the smallest on each side of each gate of the Python dispatch: keep bits above 128 keys,
# the pair launch above attn_pair_min_seq = 64 positions, the encoder's pair launch above 64 phonemes, kk_linear_tail_pays at 6400 rows.
_BASE = (2, 160, 40)
TRAIN_CASES = {
    "base": ("bf16", _BASE, {}, {}),
    "base-pn72": ("bf16", (2, 160, 72), {}, {}),
    "base-t100": ("bf16", (2, 100, 40), {}, {}),
    "base-t60": ("bf16", (2, 60, 40), {}, {}),
    "dropout-off": ("bf16", _BASE, {"train_dropout": False}, {}),
    "attn_keep_gen-off": ("bf16", _BASE, {"attn_keep_gen": False}, {}),
    "attn_keep_bits-off": ("bf16", _BASE, {"attn_keep_bits": False}, {}),
    "attn_bwd_pair-off": ("bf16", _BASE, {"attn_bwd_pair": False}, {}),
    "fuse_headnorm_bwd-off": ("bf16", _BASE, {"fuse_headnorm_bwd": False}, {}),
    "fuse_headnorm-off": ("bf16", _BASE, {"fuse_headnorm": False}, {}),
    "attn_warm-0": ("bf16", _BASE, {"attn_warm": 0}, {}),
    "attn_warm-15": ("bf16", _BASE, {"attn_warm": 15}, {}),
    "attn_proj_bf16-off": ("bf16", _BASE, {"attn_proj_bf16": False}, {}),
    "overlap-off": ("bf16", _BASE, {"overlap": False}, {}),
    "backward-off": ("bf16", _BASE, {}, {"backward": False}),
    "f32": ("f32", _BASE, {}, {}),
    "bf16-dec": ("bf16-dec", _BASE, {}, {}),
    "linear-tail": ("bf16", (8, 800, 64), {}, {}),
    "linear-tail-unfused": ("bf16", (8, 800, 64), {"fuse_linear_tail": False}, {}),
}
# inference cases: id -> engine; one generate() of 2 x 24 phonemes whose length cap (max_len = 3) ends it after three eager steps
INFER_CASES = {"generate-bf16": "bf16", "generate-f32": "f32"}
CASES = list(TRAIN_CASES) + list(INFER_CASES)
# Arguments that no owner contains, as counted when the golden was recorded: none in a training step (every buffer is a workspace
# entry, an arena slab, a batch tensor or an engine attribute); in generate() the five tensors torch itself allocates in front of the
# decode loop (the rounded durations, the frame mask of the pitch and of the energy predictor's last dot product, the clamped pitch
# and energy predictions).  They
# are recorded by dtype, shape and strides alone, so the count is pinned: no other argument may lose its owner unnoticed.
UNOWNED = {"generate-bf16": 5, "generate-f32": 5}

# what the trace of a case must (True) or must not (False) contain for the case to be on the route it is there for
ROUTES = {
    "base": {"kk_attn_bwd_kb": True, "kk_attn_keep_gen": True, "kk_attn_fwd_rb": True, "kk_encoder_stack_fwd": True,
             "kk_attn_bwd_dq": True, "kk_attn_warm_next": True},
    "base-pn72": {"kk_attn_bwd": True},
    "base-t100": {"kk_attn_bwd": True, "kk_attn_bwd_kb": False, "kk_attn_fwd_kb": False, "kk_attn_fwd_rb": False},
    "base-t60": {"kk_attn_bwd": False, "kk_attn_bwd_kb": False, "kk_attn_bwd_dkv": True},
    "dropout-off": {"kk_attn_bwd": True, "kk_attn_bwd_kb": False},
    "attn_keep_gen-off": {"kk_attn_keep_gen": False, "kk_attn_fwd_kb": True, "kk_attn_bwd_kb": True},
    "attn_keep_bits-off": {"kk_attn_fwd_kb": False, "kk_attn_bwd_kb": False, "kk_attn_bwd": True},
    "attn_bwd_pair-off": {"kk_attn_bwd": False, "kk_attn_bwd_kb": False, "kk_headnorm_rope_bwd": False},
    "fuse_headnorm_bwd-off": {"kk_headnorm_rope_bwd": True, "kk_attn_bwd_kb": False},
    "fuse_headnorm-off": {"kk_headnorm_rope_fwd": True},
    "attn_warm-0": {"kk_attn_warm_next": False},
    "attn_warm-15": {"kk_attn_warm_next": True},
    "overlap-off": {"kk_attn_keep_gen": False},
    "backward-off": {"kk_attn_bwd_kb": False, "kk_attn_bwd_dq": False},
    "f32": {"kk_headnorm_rope_fwd": True, "kk_attn_bwd": False, "kk_attn_bwd_dq": True},
    "bf16-dec": {"kk_encoder_stack_fwd": False, "kk_attn_bwd_kb": True},
    "linear-tail": {"kk_linear_tail_fwd": True},
    "linear-tail-unfused": {"kk_linear_tail_fwd": False},
    "generate-bf16": {"kk_attn_fwd": True, "kk_decode_cache_append": True, "kk_sublayer_out_fwd": True},
    "generate-f32": {"kk_attn_fwd": True, "kk_decode_cache_append": True, "kk_sublayer_out_fwd": True},
}


def make_engine(name):
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    math_mode, storage = ENGINES[name]
    return KokoroEngine(ModelDims(), StepHyper(gradient_accumulation_steps=1), math_mode=math_mode, storage=storage)


def ragged_batch(B, T, Pn, device="cuda"):
    """synthetic_batch padded to T x Pn: row 0 full, the others 55-100 % of it."""
    from kokoro_ruslan_amd.synthetic import synthetic_batch
    g = torch.Generator().manual_seed(9)
    mel = (T * (0.55 + 0.45 * torch.rand(B, generator=g))).long().clamp(min=8)
    ph = (Pn * (0.55 + 0.45 * torch.rand(B, generator=g))).long().clamp(min=4)
    mel[0], ph[0] = T, Pn
    return {k: v.to(device) for k, v in synthetic_batch(B, T, Pn, seed=77, lengths=(mel, ph)).items()}


def record_case(case, engines):
    """Run `case` on its engine (made on first use and kept in `engines`); returns the LaunchRecorder of the call."""
    name = TRAIN_CASES[case][0] if case in TRAIN_CASES else INFER_CASES[case]
    eng = engines.get(name)
    if eng is None:
        eng = engines[name] = make_engine(name)
    if case in INFER_CASES:
        g = torch.Generator().manual_seed(5)
        ids = torch.randint(1, eng.dims.vocab, (2, 24), generator=g)
        ids[1, 17:] = 0                                  # ragged: row 1 is padded
        ids = ids.to(eng.device)
        rec = LaunchRecorder(eng, {"ids": ids})
        with rec.recording():
            eng.generate(ids, max_len=3, decode_graph=False)
        torch.cuda.synchronize()
        return rec
    _, (B, T, Pn), switches, kw = TRAIN_CASES[case]
    switches = {"train_dropout": True, **switches}
    saved = {k: getattr(eng, k) for k in switches}
    batch = ragged_batch(B, T, Pn, eng.device)
    rec = LaunchRecorder(eng, batch)
    try:
        for k, v in switches.items():
            setattr(eng, k, v)
        eng.zero_grad()
        eng.forward_backward(batch, **kw)                # unrecorded: sizes the workspace, settles what the engine remembers of a shape
        with rec.recording():
            eng.forward_backward(batch, **kw)
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(eng, k, v)
    return rec


def check_routes(case, rec):
    names = {l[0] for l in rec.launches}
    for entry, want in ROUTES.get(case, {}).items():
        assert (entry in names) == want, f"case {case}: {entry} {'missing from' if want else 'present in'} the trace"
