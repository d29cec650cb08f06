"""GPU suite, kernel level: every kernel of kk_optim.hip against float64, called through the C ABI (kokoro_ruslan_amd.lib.call) on
small arenas — no engine, no graphs.  One concern per test, so that a failure names the kernel and the output that moved.

Values (kk_adamw_ema, the composed step): kernel error <= 4 E_ref + 2^-22 per segment and output (tests/fp64_bounds.py), E_ref being
the error of the fp32 restatement in tests/optim_reference.py; test_optim_reference_cpu.py shows that eleven one-line mistakes miss
this bound on these inputs by more than 100x.  Sums (kk_seg_sumsq, p_sumsq): dyadic data whose squares and partial sums are exact in
fp32 and fp64, so the comparison is equality.  Every buffer a kernel writes lies between guards that are checked afterwards.
Each check prints its figures (pytest -s)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_bounds as FB  # noqa: E402
import optim_reference as R  # noqa: E402
from fp64_bounds import FLT_EPS, NAN, SENT  # noqa: E402

pytestmark = pytest.mark.gpu

bounded = functools.partial(FB.bounded, tag="optim-fp64")
BLK, OS = R.BLK, R.OS
GUARD = 4096                                   # guard elements on either side of a flat buffer (a multiple of 16 bytes in every dtype)
INF = float("inf")


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def dev(t):
    return t.cuda().contiguous()


def call(kk, name, *args):
    """kk.call, after making sure every tensor is a contiguous device tensor (a host pointer would fault in the kernel)."""
    for a in args:
        if torch.is_tensor(a):
            assert a.is_cuda and a.is_contiguous(), f"{name}: host or strided tensor"
    kk.call(name, *args)


class Flat:
    """A flat device buffer t of n elements between two guards of GUARD elements."""

    def __init__(self, src=None, n=None, dtype=torch.float32, fill=None):
        if src is not None:
            src = torch.as_tensor(src)
            n, dtype = src.numel(), src.dtype
        self.n = n
        self.sent = 0xAB if dtype == torch.uint8 else SENT
        self.buf = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if src is not None:
            self.t.copy_(src.reshape(-1))
        elif fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.n:] == self.sent).all())

    def cpu(self):
        return self.t.cpu()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ================================================================================================ kk_adamw_ema: values
@pytest.mark.parametrize("variant", ["ema_shadow", "ema", "shadow"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("regime", ["sharp", "realistic"])
def test_adamw_ema_values(kk, regime, mode, variant):
    """m, v, p and ema of every segment against float64 at flags [3, 1, 2, 0, 7, 4, 6, 5, 3] and modes 0 / 1 / 2, with and without
    the EMA buffer and the bf16 shadow; what the flags and the mode leave unwritten is bit-identical, the zero padding stays zero,
    the shadow is bfloat16(p) bit for bit where bit 0 is set."""
    c = R.adamw_case(regime)
    with_ema, with_shadow = variant != "shadow", variant != "ema"
    inp = dict(p=c["p"], g=c["g"], m=c["m"], v=c["v"], ema=c["ema"])
    buf = {k: Flat(t) for k, t in inp.items() if k != "ema" or with_ema}
    shadow0 = c["p"].bfloat16()
    sh = Flat(shadow0) if with_shadow else None
    consts = c["consts"].clone()
    consts[0] = float(mode)
    call(kk, "kk_adamw_ema", buf["p"].t, buf["g"].t, buf["m"].t, buf["v"].t, buf["ema"].t if with_ema else None, dev(c["block_seg"]),
         c["nblocks"], dev(c["gscale"]), dev(c["decay"]), dev(c["stepsize"]), dev(c["flags"]), dev(consts), c["beta1"], c["beta2"],
         c["ema_decay"], None, c["nseg"], sh.t if with_shadow else None, 0)
    torch.cuda.synchronize()
    got = {k: b.cpu() for k, b in buf.items()}
    ref64 = dict(zip("p m v ema".split(), R.adamw_refs(regime, mode, with_ema)))
    ref32 = dict(zip("p m v ema".split(), R.adamw_refs(regime, mode, with_ema, dtype=torch.float32)))
    for k, b in buf.items():
        assert b.intact(), f"{k}: guard overwritten"
    assert same_bits(got["g"], inp["g"]), "the gradient is an input"
    got16 = sh.cpu() if with_shadow else None
    assert sh is None or sh.intact()
    for si, (sl, flags, nb, r) in enumerate(zip(c["slices"], R.ADAMW_FLAGS, R.ADAMW_LENS, R.ADAMW_RAGGED)):
        pad = slice(sl.start + (nb - 1) * BLK + r, sl.stop)
        for what in ("m", "v", "p", "ema"):
            if what == "ema" and not with_ema:
                continue
            tag = f"{regime} mode {mode} {variant} seg {si} (flags {flags}) {what}"
            if R.written(flags, mode, what, with_ema):
                bounded(tag, got[what][sl], ref32[what][sl], ref64[what][sl])
            else:
                assert same_bits(got[what][sl], inp[what][sl]), f"{tag}: must not be written"
            assert not bool(got[what][pad].any()), f"{tag}: zero padding"
        if with_shadow:
            if R.written(flags, mode, "p"):
                assert same_bits(got16[sl], got["p"][sl].bfloat16()), f"seg {si}: shadow != bfloat16(p)"
            else:
                assert same_bits(got16[sl], shadow0[sl]), f"seg {si}: shadow must not be written"
            assert not bool(got16[pad].any()), f"seg {si}: shadow zero padding"


# ================================================================================================ kk_adamw_ema: p_sumsq
DYADIC = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])


@functools.lru_cache(maxsize=None)
def _dyadic(nblocks, seed=7):
    """Values from {0, +-0.5, +-1, +-2}: squares are multiples of 1/4 up to 4, so every sum over up to 2^24 of them is exact in fp32
    (and far below 2^53 / 4 in fp64) whatever the order of the additions."""
    g = torch.Generator().manual_seed(seed)
    return DYADIC[torch.randint(0, len(DYADIC), (nblocks * BLK,), generator=g)]


PS_LENS, PS_FLAGS = [3, 1, 2, 1, 1, 1, 5], [4, 4, 0, 4, 4, 4, 4]


def _psumsq_case():
    p = _dyadic(sum(PS_LENS)).clone()
    sl = R.seg_slices(PS_LENS)
    p[sl[3]] = 128.0                                     # one block of 1024 x 2^14 = 2^24 >= 2^22: the clamp
    p[sl[4].start + 77] = NAN                            # a NaN block counts as the clamp
    p[sl[5]] = 0.0
    p[sl[5].start + 1000] = 2.0 ** -16                   # sum 2^-32 < 2^-31: rounds to 0
    block_seg, _ = R.seg_layout(PS_LENS)
    return p, block_seg, torch.tensor(PS_FLAGS, dtype=torch.int32)


def _adamw_psumsq(kk, p, block_seg, flags, mode, psq, zeroed, g=None, m=None, v=None, tables=None):
    n, nseg = p.numel(), len(flags)
    z = torch.zeros(n)
    P, M, V = Flat(p), Flat(z if m is None else m), Flat(z if v is None else v)
    one = torch.ones(nseg, device="cuda")
    gs, dec, stp = tables if tables is not None else (one, one, torch.zeros(nseg, device="cuda"))
    consts = torch.tensor([float(mode), 0.5, 1e-8, 0.0], device="cuda")
    call(kk, "kk_adamw_ema", P.t, dev(z if g is None else g), M.t, V.t, None, dev(block_seg), len(block_seg), gs, dec, stp, dev(flags),
         consts, 0.9, 0.999, 0.999, psq.t, nseg, None, zeroed)
    torch.cuda.synchronize()
    assert P.intact() and M.intact() and V.intact() and psq.intact()
    return P.cpu()


@pytest.mark.parametrize("zeroed", [0, 1])
def test_adamw_p_sumsq_exact(kk, zeroed):
    """Flags 4 (and one 0): p is untouched and p_sumsq EQUALS the Q34.30 reference — over garbage with zeroed = 0 (the call
    zero-fills), over zeros with zeroed = 1.  A block summing to >= 2^22 and a block holding a NaN contribute 2^52 each, a block
    summing to less than 2^-31 contributes nothing, an unflagged segment gets nothing."""
    p, block_seg, flags = _psumsq_case()
    want = R.p_sumsq_ref(p, block_seg, flags.tolist(), len(flags))
    assert want.tolist()[3:6] == [2 ** 52, 2 ** 52, 0] and int(want[2]) == 0 and int(want[0]) > 0
    psq = Flat(n=len(flags), dtype=torch.int64, fill=0 if zeroed else 0x123456789)
    got_p = _adamw_psumsq(kk, p, block_seg, flags, 0, psq, zeroed)
    print(f"[optim-exact] p_sumsq zeroed={zeroed}: {psq.cpu().tolist()}")
    assert torch.equal(psq.cpu(), want)
    assert same_bits(got_p, p), "flags 4: p is read only"


def test_adamw_p_sumsq_mode1_contract(kk):
    """Mode 1 (no step).  The contract the engine relies on, as the code stands: with zeroed = 1 the accumulator is not touched
    (kk_opt_prepare cleared it and kk_weight_norm_project does not read it in mode 1); with zeroed = 0 the call still zero-fills it
    and then adds nothing."""
    p, block_seg, flags = _psumsq_case()
    psq = Flat(n=len(flags), dtype=torch.int64, fill=77)
    _adamw_psumsq(kk, p, block_seg, flags, 1, psq, 1)
    assert psq.cpu().tolist() == [77] * len(flags)
    _adamw_psumsq(kk, p, block_seg, flags, 1, psq, 0)
    assert psq.cpu().tolist() == [0] * len(flags)


def test_adamw_p_sumsq_of_the_stored_weights(kk):
    """Bits 0 and 2 on random data: p_sumsq / 2^30 is the float64 sum of squares of the weights the step STORED (1e-6, as
    test_kernels_gpu.py::test_optimizer_accumulators_handed_round_zero holds it)."""
    c = R.adamw_case("realistic")
    flags = torch.full((c["nseg"],), 5, dtype=torch.int32)
    psq = Flat(n=c["nseg"], dtype=torch.int64, fill=-5)
    got_p = _adamw_psumsq(kk, c["p"], c["block_seg"], flags, 0, psq, 0, c["g"], c["m"], c["v"],
                          (dev(c["gscale"]), dev(c["decay"]), dev(c["stepsize"])))
    assert not same_bits(got_p, c["p"])
    want, _ = R.seg_sumsq_ref(got_p, c["block_seg"], c["nseg"])
    got = psq.cpu().double() / R.Q30
    # 1e-6 relative for the fp32 block sums, plus what the format itself drops: each block's share is rounded to a multiple of 2^-30
    # (half a unit per block; the one-element segments here sum to ~1e-6, where that is 1e-4 relative).  Tighter than the 1e-6
    # absolute allowance of the older test.
    quantum = torch.tensor(R.ADAMW_LENS, dtype=torch.float64) * 2.0 ** -31
    err = (got - want).abs()
    print(f"[optim-fp64] p_sumsq of stored weights: max err / (1e-6 want + blocks 2^-31) = {float((err / (1e-6 * want + quantum)).max()):.3f}")
    assert bool((err <= 1e-6 * want + quantum).all()), (got, want)


# ================================================================================================ kk_weight_norm_project
WN_LENS = [3, 2, 2, 4, 6, 3, 1]                # 21 blocks: groups of 8 are blocks 0-7, 8-15 and the tail 16-20
WN_FLAGS = [4, 4, 3, 4, 7, 0, 4]               # group 0 holds seg 0 (over), seg 1 (under), seg 2 (unflagged) and the head of seg 3
WN_MAX = 2.0
WN_PSUMSQ = [int(9.7 * 2 ** 30) + 12345,       # norm 3.11: over
             int(3.9 * 2 ** 30),               # under
             2 ** 60,                          # unflagged: whatever the accumulator says
             4 * 2 ** 30,                      # norm == max_norm exactly: the kernel tests strict >, must not move
             10 ** 4 * 2 ** 30 + 7,            # norm 100 (straddles groups 1 and 2)
             2 ** 60,                          # unflagged
             4 * 2 ** 30 + 1]                  # norm 2 + 2^-32 > 2: rewritten with scale float32(1 - 2^-33) = 1


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("mode,max_norm", [(0, WN_MAX), (2, WN_MAX), (1, WN_MAX), (0, 0.0), (0, -1.0)])
def test_weight_norm_project(kk, mode, max_norm, with_shadow):
    """Only the blocks of a flag-bit-2 segment whose norm is STRICTLY above the ceiling are rewritten, to p float32(max_norm / norm)
    within 2 eps32 |p| (one double division and square root rounded once to fp32; device and host square roots may differ in the last
    double bit: at most one fp32 ulp of scale, plus the product's rounding), their shadow to bfloat16 of the stored value; everything
    else is bit-identical in fp32 and in the shadow.  Mode 1 and max_norm <= 0 change nothing."""
    g = torch.Generator().manual_seed(21)
    nblocks = sum(WN_LENS)
    p = torch.randn(nblocks * BLK, generator=g)
    block_seg, _ = R.seg_layout(WN_LENS)
    if mode == 1 or max_norm <= 0:
        psq = [2 ** 60] * len(WN_LENS)                  # every accumulator far over the ceiling
    else:
        psq = WN_PSUMSQ
        assert math.sqrt(psq[3] / R.Q30) == max_norm and math.sqrt(psq[6] / R.Q30) > max_norm
    P = Flat(p)
    shadow0 = torch.full((nblocks * BLK,), 3.0).bfloat16()
    S = Flat(shadow0) if with_shadow else None
    call(kk, "kk_weight_norm_project", P.t, dev(block_seg), nblocks, dev(torch.tensor(psq, dtype=torch.int64)),
         dev(torch.tensor(WN_FLAGS, dtype=torch.int32)), torch.tensor([float(mode), 0.5, 1e-8, 0.0], device="cuda"), float(max_norm),
         S.t if with_shadow else None)
    torch.cuda.synchronize()
    assert P.intact() and (S is None or S.intact())
    want, moved = R.project_ref(p, block_seg, psq, WN_FLAGS, mode, max_norm)
    if mode != 1 and max_norm > 0:
        assert moved.tolist() == [s in (0, 4, 6) for s in block_seg.tolist()]
    else:
        assert not bool(moved.any())
    got, got16 = P.cpu(), (S.cpu() if with_shadow else None)
    worst = 0.0
    for b in range(nblocks):
        sl = slice(b * BLK, (b + 1) * BLK)
        if moved[b]:
            err = (got[sl].double() - want[sl]).abs() / p[sl].double().abs()
            worst = max(worst, float(err.max()) / FLT_EPS)
            assert float(err.max()) <= 2.0 * FLT_EPS, f"block {b}: {float(err.max()) / FLT_EPS:.2f} eps32"
            assert got16 is None or same_bits(got16[sl], got[sl].bfloat16()), f"block {b}: shadow != bfloat16(stored)"
        else:
            assert same_bits(got[sl], p[sl]), f"block {b} (segment {int(block_seg[b])}) must not move"
            assert got16 is None or same_bits(got16[sl], shadow0[sl]), f"block {b}: shadow must not move"
    print(f"[optim-fp64] weight_norm_project mode {mode} max_norm {max_norm}: worst rewritten error {worst:.2f} eps32")


# ================================================================================================ kk_seg_sumsq: exact sums
def _mixed_lens(nblocks, seed):
    g = torch.Generator().manual_seed(seed)
    choice, lens, left = [1, 1, 2, 3, 5, 17, 64, 130], [], nblocks
    while left > 0:
        n = min(left, choice[int(torch.randint(0, len(choice), (1,), generator=g))])
        lens.append(n)
        left -= n
    return lens


def _range_lens(shift):
    """6144 blocks at per = 3: segments of 15, 16, 17, 255, 256 and 257 whole workgroup ranges, every boundary at block `shift` of a
    range (0: its first block, 1: the middle, 2: the last), one-block segments behind them."""
    lens = ([shift] if shift else []) + [3 * r for r in (15, 16, 17, 255, 256, 257)]
    return lens + [1] * (6144 - sum(lens))


SEG_LAYOUTS = {                                          # name -> segment lengths in blocks; per = ceil(nblocks / 2048)
    "n1": [1], "n9": [2, 1, 3, 1, 2], "n2047": _mixed_lens(2047, 1), "n2048": _mixed_lens(2048, 2), "n2049": _mixed_lens(2049, 3),
    "n4097": _mixed_lens(4097, 4), "n6144": _mixed_lens(6144, 5),
    "ones_per2": [1] * 2049,                             # per = 2: lead and trail records only
    "ones_per3": [1] * 4097,                             # per = 3: interior stores too
    "whole": [6144],                                     # 2048 records of one id through all four merge levels
    "ranges0": _range_lens(0), "ranges1": _range_lens(1), "ranges2": _range_lens(2),
}


def _seg_ids(lens):
    """block_seg with ids 0, 2, 3, ...: id 1 and the last id (nseg - 1) own no block."""
    ids = torch.arange(len(lens), dtype=torch.int32)
    ids[1:] += 1
    return torch.repeat_interleave(ids, torch.tensor(lens)), len(lens) + 2


def _seg_sumsq(kk, buf, block_seg, nseg, fill, skip=None, extra=0, records=None):
    lib = kk.load()
    nblocks = len(block_seg)
    ws = Flat(n=int(lib.kk_seg_sumsq_ws_bytes(nblocks)), dtype=torch.uint8)
    ws.t.random_(0, 256)                                 # the record workspace needs no initial state
    if records is not None:
        raw = torch.from_numpy(records.view(np.uint8).copy())
        off = int(lib.kk_seg_sumsq_rec_offset())
        assert off + raw.numel() <= ws.n
        ws.t[off:off + raw.numel()] = raw.cuda()
    out = Flat(n=nseg, dtype=torch.float64, fill=fill)
    call(kk, "kk_seg_sumsq", dev(buf), dev(block_seg), nblocks, out.t, nseg, ws.t, None if skip is None else dev(skip), extra)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return out.cpu()


@pytest.mark.parametrize("name", list(SEG_LAYOUTS))
def test_seg_sumsq_exact(kk, name):
    """Dyadic gradients: every segment's sum of squares EQUALS the float64 reference at the edges of the fixed 2048-workgroup walk
    (see SEG_LAYOUTS), over an output pre-filled with NaN and a workspace of random bytes.  Contract: a segment id that owns no
    block is not stored — its NaN stays; the engine's arena has no such id."""
    lens = SEG_LAYOUTS[name]
    nblocks = sum(lens)
    buf = _dyadic(6144)[:nblocks * BLK]
    block_seg, nseg = _seg_ids(lens)
    want, owned = R.seg_sumsq_ref(buf, block_seg, nseg)
    assert owned.tolist() == [i not in (1, nseg - 1) for i in range(nseg)]
    got = _seg_sumsq(kk, buf, block_seg, nseg, NAN)
    bad = int((got[owned] != want[owned]).sum())
    print(f"[optim-exact] seg_sumsq {name}: {nblocks} blocks, {len(lens)} segments, {bad} wrong")
    assert torch.equal(got[owned], want[owned])
    assert bool(torch.isnan(got[~owned]).all()), "an id without a block must be left alone"


def test_seg_sumsq_inf_poisons_its_own_segment(kk):
    lens = SEG_LAYOUTS["n2049"]
    buf = _dyadic(6144)[:sum(lens) * BLK].clone()
    block_seg, nseg = _seg_ids(lens)
    want, owned = R.seg_sumsq_ref(buf, block_seg, nseg)
    victim_block = 1000
    victim = int(block_seg[victim_block])
    buf[victim_block * BLK + 5] = INF
    got = _seg_sumsq(kk, buf, block_seg, nseg, NAN)
    others = owned.clone()
    others[victim] = False
    assert float(got[victim]) == INF and torch.equal(got[others], want[others])


# ================================================================================================ kk_seg_sumsq: skip table, tile records
SEG_REC = np.dtype([("v", "<f8"), ("seg", "<i4"), ("pad", "<i4")])           # KkSegRec


@pytest.mark.parametrize("fill_capacity", [False, True])
def test_seg_sumsq_skip_table_and_tile_records(kk, fill_capacity):
    """Segments marked in the skip table are never loaded (NaN lies under them) and take the sum of their tile records — 1, 17 and
    300 adjacent records for the arena's first segment, one straddling a workgroup-range boundary (per = 3: blocks 4-8 cross block 6)
    and the arena's last; a skipped segment without a record and an id without a block stay as they were; all others are exact.
    With fill_capacity the record count is kk_seg_sumsq_rec_capacity(), the rest being empty records (seg = -1)."""
    lens = [2, 2, 5] + _mixed_lens(4097 - 2 - 2 - 5 - 2 - 3, 9) + [2, 3]
    assert sum(lens) == 4097
    block_seg, nseg = _seg_ids(lens)
    nl = len(lens)
    sid = lambda i: i if i == 0 else i + 1                                    # noqa: E731  (segment index -> id, see _seg_ids)
    first, straddle, norec, last = sid(0), sid(2), sid(nl - 2), sid(nl - 1)
    buf = _dyadic(6144)[:4097 * BLK].clone()
    skip = torch.zeros(nseg, dtype=torch.int32)
    for s in (first, straddle, norec, last):
        skip[s] = 1
        buf[(block_seg == s).repeat_interleave(BLK)] = NAN
    g = np.random.RandomState(4)
    recs, sums = [], {}
    for s, cnt in ((straddle, 17), (last, 300), (first, 1)):                  # (launch order, not arena order: only adjacency matters)
        vals = g.randint(0, 4096, cnt) / 4.0
        sums[s] = float(vals.sum())
        recs += [(float(x), s, 0) for x in vals]
    extra = len(recs)
    if fill_capacity:
        extra = int(kk.load().kk_seg_sumsq_rec_capacity())
        recs += [(NAN, -1, 0)] * (extra - len(recs))
    want, owned = R.seg_sumsq_ref(buf.nan_to_num(0.0), block_seg, nseg)
    got = _seg_sumsq(kk, buf, block_seg, nseg, -3.0, skip, extra, np.array(recs, dtype=SEG_REC))
    for s, v in sums.items():
        assert float(got[s]) == v, (s, float(got[s]), v)
    assert float(got[norec]) == -3.0 and float(got[1]) == -3.0 and float(got[nseg - 1]) == -3.0
    rest = owned & (skip == 0)
    assert torch.equal(got[rest], want[rest])


def test_seg_sumsq_refuses_bad_record_counts(kk):
    """More records than the workspace holds, or records without a skip table: refused by the argument check in front of the launch
    (KK_REQUIRE in kk_seg_sumsq); the buffers are correctly sized anyway."""
    lib = kk.load()
    buf, block_seg = dev(_dyadic(6144)[:9 * BLK]), dev(torch.zeros(9, dtype=torch.int32))
    ws = torch.zeros(int(lib.kk_seg_sumsq_ws_bytes(9)), dtype=torch.uint8, device="cuda")
    out, skip = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="tile records"):
        call(kk, "kk_seg_sumsq", buf, block_seg, 9, out, 1, ws, skip, int(lib.kk_seg_sumsq_rec_capacity()) + 1)
    with pytest.raises(RuntimeError, match="tile records"):
        call(kk, "kk_seg_sumsq", buf, block_seg, 9, out, 1, ws, None, 1)
    call(kk, "kk_seg_sumsq", buf, block_seg, 9, out, 1, ws, skip, 0)
    torch.cuda.synchronize()
    assert float(out[0]) == float(R.seg_sumsq_ref(buf.cpu(), block_seg.cpu(), 1)[0][0])


# ================================================================================================ kk_opt_prepare
REL_F32 = 2.0 ** -22           # a double rounded to fp32 once (gscale: twice) is within 2^-23; two ulps allowed
STATE_DOUBLES = ("LAST_GRAD_NORM", "LAST_CLIP_COEF", "LAST_BASE_LR", "LAST_CLIP_NORM", "EXPL_EMA")
STATE_COUNTERS = ("SKIPPED", "ATTEMPT", "EXPL_EMA_STEPS", "EXPL_STREAK", "EXPL_EMA_VALID", "LAST_SKIP", "MICRO_BAD", "BAD_COUNT",
                  "BAD_ATTEMPT", "MICRO_BAD_TOTAL")


def _prepare_inputs(nseg):
    """Random positive sums, lr_mult and wd; pre-clip by i % 4: disabled (0) | a ceiling above the norm | below it | ss = 0.25 under
    a ceiling of exactly 0.5 = sqrt(ss), which must not scale."""
    g = np.random.RandomState(nseg)
    ss = g.uniform(0.01, 4.0, nseg)
    mult = g.uniform(0.5, 2.0, nseg).astype(np.float32)
    wd = g.uniform(0.0, 0.1, nseg).astype(np.float32)
    pre = np.zeros(nseg, dtype=np.float32)
    i = np.arange(nseg)
    pre[i % 4 == 1] = (2.0 * np.sqrt(ss[i % 4 == 1])).astype(np.float32)
    pre[i % 4 == 2] = (0.5 * np.sqrt(ss[i % 4 == 2])).astype(np.float32)
    ss[i % 4 == 3] = 0.25
    pre[i % 4 == 3] = 0.5
    return ss, pre, mult, wd


def _state(**over):
    st = np.zeros(OS["SIZE"])
    st[OS["ATTEMPT"]], st[OS["SKIPPED"]] = 10.0, 3.0                          # k = 7
    st[OS["EXPL_EMA"]], st[OS["EXPL_EMA_VALID"]], st[OS["EXPL_EMA_STEPS"]], st[OS["EXPL_STREAK"]] = 0.7, 1.0, 6.0, 2.0
    st[OS["BAD_SEG"]], st[OS["BAD_COUNT"]], st[OS["BAD_ATTEMPT"]] = 41.0, 1.0, 2.0
    for k, v in over.items():
        st[OS[k]] = v
    return st


def _prepare(kk, ss, pre, mult, wd, cfg, st, clear="b"):
    nseg = len(ss)
    S = Flat(torch.from_numpy(np.asarray(st, dtype=np.float64)))
    out = {k: Flat(n=nseg, fill=NAN) for k in ("gscale", "decay", "stepsize")}
    consts = Flat(n=4, fill=NAN)
    dss = Flat(torch.from_numpy(np.asarray(ss, dtype=np.float64)))
    cb = Flat(n=nseg, dtype=torch.int64, fill=99)
    call(kk, "kk_opt_prepare", dss.t, dev(torch.from_numpy(pre)), dev(torch.from_numpy(mult)), dev(torch.from_numpy(wd)), nseg, None,
         cfg, S.t, out["gscale"].t, out["decay"].t, out["stepsize"].t, consts.t, dss.t if clear == "ab" else None, cb.t)
    torch.cuda.synchronize()
    for f in (S, consts, dss, cb, *out.values()):
        assert f.intact()
    assert cb.cpu().tolist() == [0] * nseg, "clear_b"
    if clear == "ab":
        assert not bool(dss.cpu().any()), "clear_a (the sums are read before they are cleared)"
    else:
        assert same_bits(dss.cpu(), torch.from_numpy(np.asarray(ss, dtype=np.float64)))
    return dict(st=S.cpu().numpy(), consts=consts.cpu().numpy(), **{k: v.cpu().numpy() for k, v in out.items()})


def _check_prepare(tag, got, ref, segments=True):
    for name in STATE_DOUBLES:
        g_, r_ = got["st"][OS[name]], ref["st"][OS[name]]
        assert abs(g_ - r_) <= 1e-12 * abs(r_), (tag, name, g_, r_)
    for name in STATE_COUNTERS:
        assert got["st"][OS[name]] == ref["st"][OS[name]], (tag, name, got["st"][OS[name]], ref["st"][OS[name]])
    assert got["consts"][0] == ref["consts"][0], (tag, got["consts"], ref["consts"])
    worst = {}
    for name in ("consts",) + (("gscale", "decay", "stepsize") if segments else ()):
        g_, r_ = got[name].astype(np.float64), ref[name].astype(np.float64)
        if name == "consts":
            g_, r_ = g_[1:], r_[1:]
        assert np.isfinite(g_).all(), (tag, name)
        err = np.abs(g_ - r_)
        worst[name] = float((err / np.maximum(np.abs(r_), 1e-300)).max()) / 2.0 ** -23
        assert (err <= REL_F32 * np.abs(r_)).all(), (tag, name, worst[name])
    print(f"[optim-fp64] opt_prepare {tag}: worst fp32 output error in units of 2^-23: "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


PREPARE_CFGS = {
    "plain": dict(),
    "warmup_explosion": dict(use_warmup=1, warmup_steps=10, onecycle_steps=990, expl_abs_floor=0.5, expl_warmup_floor=2.0,
                             expl_warmup_steps=20, div_factor=3.0),
    "legacy": dict(legacy_schedule=1, legacy_cos=0.3141592653589793, learning_rate=2e-3),
    "past_warmup": dict(use_warmup=1, warmup_steps=4, onecycle_steps=20, pct_start=0.3, max_grad_norm=0.05),
}


@pytest.mark.parametrize("variant", list(PREPARE_CFGS))
@pytest.mark.parametrize("nseg", [1, 255, 256, 257, 700])
def test_opt_prepare_outputs(kk, nseg, variant):
    """State, step constants and the per-segment gscale / decay / stepsize against the float64 replay at k = attempt - skipped = 7,
    from one segment up to three passes of the 256-thread loops: state doubles to 1e-12 (double arithmetic and libm), counters
    exactly, fp32 outputs to 2^-22 relative."""
    ss, pre, mult, wd = _prepare_inputs(nseg)
    cfg = R.make_cfg(**PREPARE_CFGS[variant])
    st = _state()
    ref = R.opt_prepare_ref(ss, pre, mult, wd, cfg, st)
    assert ref["st"][OS["ATTEMPT"]] == 11.0 and ref["st"][OS["SKIPPED"]] == 3.0 and ref["consts"][0] == 0.0
    if nseg >= 4:
        assert ref["gscale"][3] == np.float32(ref["st"][OS["LAST_CLIP_COEF"]]), "ss = pre^2: the pre-clip does not scale"
        assert ref["gscale"][2] < 0.51 * ref["gscale"][3]
    got = _prepare(kk, ss, pre, mult, wd, cfg, st, clear="ab" if variant == "plain" else "b")
    _check_prepare(f"nseg {nseg} {variant}", got, ref)
    for name in ("BAD_SEG", "BAD_COUNT", "BAD_ATTEMPT"):
        assert got["st"][OS[name]] == st[OS[name]], "the diagnostics of an earlier skip stay"


@pytest.mark.parametrize("nseg", [1, 257])
def test_opt_prepare_ema_update_every(kk, nseg):
    """ema_update_every = 4: successful step k = 7 steps without the EMA (consts[0] = 2), k = 8 with it (0)."""
    ss, pre, mult, wd = _prepare_inputs(nseg)
    cfg = R.make_cfg(ema_update_every=4)
    st = _state()
    for k, mode in ((7, 2.0), (8, 0.0)):
        ref = R.opt_prepare_ref(ss, pre, mult, wd, cfg, st)
        got = _prepare(kk, ss, pre, mult, wd, cfg, st)
        assert ref["consts"][0] == mode and got["consts"][0] == mode, (k, got["consts"])
        _check_prepare(f"nseg {nseg} ema_update_every k {k}", got, ref)
        st = got["st"]


def test_opt_prepare_nonfinite_sums_skip(kk):
    """A NaN in segment 5 and an inf in segment 300 of 700: no step, the first bad segment (1-based), their count and the attempt are
    recorded.  gscale / the clip coefficient of a skipped boundary are consumed by nothing and not asserted."""
    ss, pre, mult, wd = _prepare_inputs(700)
    ss[5], ss[300] = NAN, INF
    st = _state(MICRO_BAD=1.0)
    got = _prepare(kk, ss, pre, mult, wd, R.make_cfg(), st)
    s = got["st"]
    assert got["consts"][0] == 1.0 and s[OS["LAST_SKIP"]] == 1.0
    assert s[OS["BAD_SEG"]] == 6.0 and s[OS["BAD_COUNT"]] == 2.0 and s[OS["BAD_ATTEMPT"]] == 10.0
    assert s[OS["SKIPPED"]] == 4.0 and s[OS["ATTEMPT"]] == 11.0 and s[OS["MICRO_BAD"]] == 0.0
    ref = R.opt_prepare_ref(ss, pre, mult, wd, R.make_cfg(), st)
    for name in ("BAD_SEG", "BAD_COUNT", "BAD_ATTEMPT", "SKIPPED", "ATTEMPT", "MICRO_BAD", "LAST_SKIP", "EXPL_EMA_STEPS"):
        assert ref["st"][OS[name]] == s[OS[name]], name
    assert ref["consts"][0] == 1.0


def test_opt_prepare_bad_micro_batch_skips(kk):
    """MICRO_BAD = 1 with finite sums also skips the step (and is cleared); the finite outputs still match the replay."""
    ss, pre, mult, wd = _prepare_inputs(257)
    st = _state(MICRO_BAD=1.0)
    ref = R.opt_prepare_ref(ss, pre, mult, wd, R.make_cfg(), st)
    got = _prepare(kk, ss, pre, mult, wd, R.make_cfg(), st)
    s = got["st"]
    assert got["consts"][0] == 1.0 and s[OS["SKIPPED"]] == 4.0 and s[OS["ATTEMPT"]] == 11.0 and s[OS["MICRO_BAD"]] == 0.0
    assert s[OS["BAD_COUNT"]] == 0.0 and s[OS["BAD_ATTEMPT"]] == 10.0
    _check_prepare("bad micro-batch", got, ref, segments=False)


# ================================================================================================ kk_cast_f32_bf16
def _f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


CAST_EDGES = _f32_from_bits([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties: to even downwards, to even upwards, and their negatives
    0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,      # one fp32 ulp off a tie
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,      # +-0, +-inf
    0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F7FFFFF,      # NaNs (one whose payload is in the dropped bits only), FLT_MAX -> inf
    0x7F7F7FFF, 0x7F7F8000, 0xFF7FFFFF, 0x00800000])     # just below the last tie (finite), the last tie (-> inf), -FLT_MAX, FLT_MIN


@pytest.mark.parametrize("n", [4, 1028, 4 * 256 * 4096 + 4])
def test_cast_f32_bf16(kk, n):
    """Bit-exact against torch's bfloat16 (round to nearest even; NaN stays NaN, whatever its payload) at 4 elements, a ragged
    second workgroup and the first size whose grid-stride loop takes a second trip (4096 workgroups x 256 x 4 elements, + 4).
    fp32 denormals are left out: bf16 keeps them as denormals in torch, and whether the hardware conversion does is the float mode's
    business, not this kernel's."""
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g) * 10.0 ** torch.randint(-20, 20, (n,), generator=g).float()
    k = len(CAST_EDGES)
    if n == 4:
        src = _f32_from_bits([0x3F808000, 0x3F818000, 0x7F800001, 0x7F7FFFFF])
    else:
        src[:k], src[n // 2:n // 2 + k], src[n - k:] = CAST_EDGES, CAST_EDGES, CAST_EDGES
        src[n - 4:] = _f32_from_bits([0xBF818000, 0x7F7F8000, 0xFFC12345, 0x3F808000])        # the + 4 tail
    den = (src != 0) & (src.abs() < 2.0 ** -126)
    src[den] = 1.0
    dst = Flat(n=n, dtype=torch.bfloat16, fill=5.0)
    call(kk, "kk_cast_f32_bf16", dev(src), dst.t, n)
    torch.cuda.synchronize()
    assert dst.intact()
    got, want = dst.cpu(), src.bfloat16()
    nan = torch.isnan(src)
    assert bool(torch.isnan(got[nan]).all()) and bool(torch.isnan(want[nan]).all())
    wrong = bits(got)[~nan] != bits(want)[~nan]
    print(f"[optim-exact] cast n={n}: {int(wrong.sum())} of {int((~nan).sum())} differ")
    assert not bool(wrong.any())


def test_cast_f32_bf16_refuses_ragged_length(kk):
    src, dst = torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        call(kk, "kk_cast_f32_bf16", src, dst, 6)


# ================================================================================================ one composed step
def _composed_ref(dtype, c, cfg, base_lr):
    """Pre-clip, clip_grad_norm_, torch.optim.AdamW, EMA and the weight-norm projection on the logical tensors, in `dtype` on the CPU
    (on clones: in float32 .to() would hand out views of the inputs)."""
    P = [torch.nn.Parameter(c["p"][sl].to(dtype).clone()) for sl in c["views"]]
    G = [c["g"][sl].to(dtype).clone() for sl in c["views"]]
    for g_, pre in zip(G, c["preclip"]):
        nr = float(g_.norm(2))
        if pre > 0 and nr > pre:
            g_.mul_(pre / (nr + 1e-12))
    for q, g_ in zip(P, G):
        q.grad = g_
    torch.nn.utils.clip_grad_norm_(P, cfg.max_grad_norm)
    opt = torch.optim.AdamW([dict(params=[q], lr=base_lr * R.f32(mu), weight_decay=R.f32(w)) for q, mu, w in zip(P, c["mult"], c["wd"])],
                            betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    for q, sl in zip(P, c["views"]):
        opt.state[q] = dict(step=torch.tensor(float(c["k"])), exp_avg=c["m"][sl].to(dtype).clone(), exp_avg_sq=c["v"][sl].to(dtype).clone())
    opt.step()
    out = dict(p=[], m=[], v=[], ema=[])
    with torch.no_grad():
        for q, sl, fl in zip(P, c["views"], c["flags"]):
            e = c["ema"][sl].to(dtype).clone()
            if fl & 2:
                e = e * c["ema_decay"] + q * (1.0 - c["ema_decay"])
            if fl & 4:
                nr = float(q.norm(2))
                if nr > c["max_norm"]:
                    q.mul_(c["max_norm"] / nr)
            out["p"].append(q.detach()), out["m"].append(opt.state[q]["exp_avg"]), out["v"].append(opt.state[q]["exp_avg_sq"])
            out["ema"].append(e)
    return out


def test_composed_step(kk):
    """kk_seg_sumsq -> kk_opt_prepare(clear_b = p_sumsq) -> kk_adamw_ema(zeroed = 1) -> kk_weight_norm_project on 12 blocks and 4
    tensors — one over its pre-clip ceiling, one over the weight-norm ceiling, the global clip active — against pre-clip,
    clip_grad_norm_, torch.optim.AdamW, the EMA and the projection in float64 on the CPU.  The only test that chains kernels: it
    catches a disagreement between what one writes and the next reads."""
    gen = torch.Generator().manual_seed(12)
    lens, sizes, flags = [3, 4, 1, 4], [2500, 4096, 300, 3073], [3, 7, 3, 5]
    block_seg, first = R.seg_layout(lens)
    n, nseg = sum(lens) * BLK, len(lens)
    views = [slice(f * BLK, f * BLK + s) for f, s in zip(first, sizes)]
    live = torch.zeros(n, dtype=torch.bool)
    for sl in views:
        live[sl] = True
    rn = lambda: torch.randn(n, generator=gen) * live                         # noqa: E731
    p, g = 0.04 * rn(), 0.01 * rn()
    p[views[3]] *= 0.2                                                        # seg 1: norm ~ 2.6 > 2; seg 3: ~ 0.44 < 2
    m, v, ema = 0.01 * rn(), (0.01 * rn()) ** 2 + 1e-6 * live, p + 1e-3 * rn()
    c = dict(p=p, g=g, m=m, v=v, ema=ema, views=views, flags=flags, k=7, preclip=[0.0, 0.0, 0.05, 10.0], mult=[1.0, 0.5, 2.0, 1.0],
             wd=[0.01, 0.0, 0.1, 0.05], ema_decay=R.f32(0.999), max_norm=2.0)
    assert float(g[views[2]].norm()) > 0.05 and float(p[views[1]].norm()) > 2.2 and float(p[views[3]].norm()) < 1.0
    cfg = R.make_cfg(max_grad_norm=0.5, beta1=R.f32(0.9), beta2=R.f32(0.999), eps=R.f32(1e-8), max_weight_norm=2.0)
    st = _state()
    base_lr = R.base_lr_ref(cfg, c["k"])
    ref64, ref32 = _composed_ref(torch.float64, c, cfg, base_lr), _composed_ref(torch.float32, c, cfg, base_lr)
    assert float(ref64["p"][1].norm()) == pytest.approx(2.0, rel=1e-12) and not torch.equal(ref64["p"][3], p[views[3]].double())

    lib = kk.load()
    B = {k: Flat(t) for k, t in dict(p=p, g=g, m=m, v=v, ema=ema).items()}
    S = Flat(p.bfloat16())
    ws = Flat(n=int(lib.kk_seg_sumsq_ws_bytes(len(block_seg))), dtype=torch.uint8)
    ss = Flat(n=nseg, dtype=torch.float64, fill=NAN)
    psq = Flat(n=nseg, dtype=torch.int64, fill=0x7777)
    S_ = Flat(torch.from_numpy(st))
    gs, dec, stp, consts = (Flat(n=k_, fill=NAN) for k_ in (nseg, nseg, nseg, 4))
    bseg, dflags = dev(block_seg), dev(torch.tensor(flags, dtype=torch.int32))
    t32 = lambda x: dev(torch.tensor(x, dtype=torch.float32))                 # noqa: E731
    call(kk, "kk_seg_sumsq", B["g"].t, bseg, len(block_seg), ss.t, nseg, ws.t, None, 0)
    call(kk, "kk_opt_prepare", ss.t, t32(c["preclip"]), t32(c["mult"]), t32(c["wd"]), nseg, None, cfg, S_.t, gs.t, dec.t, stp.t, consts.t,
         None, psq.t)
    call(kk, "kk_adamw_ema", B["p"].t, B["g"].t, B["m"].t, B["v"].t, B["ema"].t, bseg, len(block_seg), gs.t, dec.t, stp.t, dflags,
         consts.t, cfg.beta1, cfg.beta2, c["ema_decay"], psq.t, nseg, S.t, 1)
    call(kk, "kk_weight_norm_project", B["p"].t, bseg, len(block_seg), psq.t, dflags, consts.t, c["max_norm"], S.t)
    torch.cuda.synchronize()
    for f in (*B.values(), S, ws, ss, psq, S_, gs, dec, stp, consts):
        assert f.intact()
    state = S_.cpu().numpy()
    assert state[OS["LAST_SKIP"]] == 0.0 and state[OS["LAST_CLIP_COEF"]] < 1.0 and float(consts.cpu()[0]) == 0.0
    assert float(gs.cpu()[2]) < 0.9 * float(gs.cpu()[0]), "segment 2 was over its pre-clip ceiling"
    got = {k: b.cpu() for k, b in B.items()}
    for what in ("m", "v", "p", "ema"):
        for si, sl in enumerate(views):
            bounded(f"composed step seg {si} (flags {flags[si]}) {what}", got[what][sl], ref32[what][si], ref64[what][si])
        assert not bool(got[what][~live].any()), f"{what}: zero padding"
    assert same_bits(S.cpu(), got["p"].bfloat16()), "the shadow is bfloat16 of the stored weights, projection included"
