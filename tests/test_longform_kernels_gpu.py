"""kk_mel_finish and kk_wave_join on the device (kokoro_ruslan_amd/longform.py) against the fp64 oracle and against torch on the device:
the case table of test_longform_cpu.py, batch independence bit for bit, the limits, and the join's copy, fades and peaks."""
import os
import sys

import pytest
import torch

from kokoro_ruslan_amd.longform_torch import fade_table, finish_reference

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def _table(n_mels):
    """(cases, the oracle's result per case, the device result of all cases finished in one batch): computed once per n_mels"""
    from kokoro_ruslan_amd.longform import MelFinisher
    if n_mels not in _cache:
        cases = LC.finish_cases(n_mels)
        fin = MelFinisher(n_mels=n_mels)
        _cache[n_mels] = (cases, [finish_reference(m) for _, m, _ in cases], fin.finish([m.cuda() for _, m, _ in cases]), fin)
    return _cache[n_mels]


def _check(name, mel, ref, trimmed, info):
    clamped, t_end, last, thr, st = ref
    assert st["frame_margin"] >= 1e-3 and st["branch_margin"] >= 1e-3, name
    print(f"{name}: kept {info['kept']} / {t_end}, last_voiced {info['last_voiced']} / {last}, threshold error "
          f"{abs(info['threshold'] - thr):.3g}, mean error {abs(info['mean'] - st['mean']):.3g}, std error {abs(info['std'] - st['std']):.3g}")
    assert (info["frames"], info["kept"], info["last_voiced"]) == (mel.shape[0], t_end, last), name
    assert trimmed.is_cuda and trimmed.dtype == torch.float32 and trimmed.shape == (t_end, mel.shape[1])
    assert torch.equal(_bits(trimmed.cpu()), _bits(clamped[:t_end])), name
    assert abs(info["threshold"] - thr) <= 1e-4, name
    assert (info["min"], info["max"], info["nan"]) == (st["min"], st["max"], st["nan"]), name
    assert info["flat"] is False
    if st["std"] >= 1e-3:
        assert abs(info["mean"] - st["mean"]) <= 1e-9 * abs(st["mean"]) and abs(info["std"] - st["std"]) <= 1e-9 * st["std"], name
    else:
        assert st["nan"] and info["mean"] != info["mean"] and info["std"] != info["std"], name      # a NaN in: NaN out, as torch


@pytest.mark.parametrize("n_mels", [80, 8])
def test_mel_finish_against_the_oracle(n_mels):
    _need_gpu()
    cases, refs, (trimmed, info), _ = _table(n_mels)
    assert len(trimmed) == len(info) == len(cases)
    for (name, mel, _), ref, t, i in zip(cases, refs, trimmed, info):
        _check(name, mel, ref, t, i)
    # the whole clamped mel, not only the kept frames: the views share one buffer in input order
    base = trimmed[0]
    full = torch.cat([m for _, m, _ in cases]).clamp(min=-11.5, max=2.0)
    buf = torch.as_strided(base, (full.shape[0], n_mels), (n_mels, 1))
    assert torch.equal(_bits(buf.cpu()), _bits(full))


@pytest.mark.parametrize("n_mels", [80, 8])
def test_mel_finish_does_not_depend_on_the_batch(n_mels):
    _need_gpu()
    cases, _, (trimmed, info), fin = _table(n_mels)
    for (name, mel, _), t, i in zip(cases, trimmed, info):
        (t1,), (i1,) = fin.finish([mel.cuda()])
        assert torch.equal(_bits(t1), _bits(t)), name
        assert {k: v for k, v in i1.items() if v == v} == {k: v for k, v in i.items() if v == v}, name
        assert [k for k, v in i1.items() if v != v] == [k for k, v in i.items() if v != v], name


def test_mel_finish_flat_limits_and_arguments():
    _need_gpu()
    from kokoro_ruslan_amd.longform import MelFinisher
    fin = MelFinisher()
    (t,), (i,) = fin.finish([torch.full((70, 80), -3.3).cuda()])
    assert i["flat"] is True and i["std"] < 1e-5 and abs(i["mean"] + 3.3) < 1e-6 and i["min"] == i["max"] and i["kept"] == 70
    (t,), (i,) = fin.finish([torch.full((4096, 80), -10.9).cuda()])                    # the largest mel; nothing voiced: nothing cut
    assert i["flat"] and i["last_voiced"] == -1 and i["kept"] == 4096 and i["threshold"] == -9.8
    with pytest.raises(ValueError, match="4097 frames, the limit is 4096"):
        fin.finish([torch.zeros(10, 80).cuda(), torch.zeros(4097, 80).cuda()])
    with pytest.raises(ValueError, match="mel 1: shape"):
        fin.finish([torch.zeros(10, 80).cuda(), torch.zeros(10, 79).cuda()])
    with pytest.raises(ValueError, match="frames >= 1"):
        fin.finish([torch.zeros(0, 80).cuda()])
    assert fin.finish([]) == ([], [])
    for kw, match in (({"n_mels": 129}, "n_mels 129"), ({"clamp": (2.0, -11.5)}, "clamp"), ({"threshold": (float("nan"), 0)}, "threshold"),
                      ({"margin": -1}, "margin"), ({"min_keep": 1.5}, "min_keep")):
        with pytest.raises(ValueError, match=match):
            MelFinisher(**kw)
    # other parameters than the reference's: against the oracle at the same ones
    name, mel, _ = LC.finish_cases()[7]
    kw = dict(clamp=(-8.0, -4.0), threshold=(-7.5, -7.0), margin=3, min_keep=10)
    ref = finish_reference(mel, **kw)
    assert ref[4]["frame_margin"] >= 1e-3 and ref[4]["branch_margin"] >= 1e-3
    (t,), (i,) = MelFinisher(**kw).finish([mel.cuda()])
    assert (i["kept"], i["last_voiced"]) == (ref[1], ref[2]) and abs(i["threshold"] - ref[3]) <= 1e-4
    assert torch.equal(_bits(t.cpu()), _bits(ref[0][:ref[1]]))


def _join(chunks, documents, gap, fade):
    """join() into a buffer that holds NaNs: none may be left, so every sample is written"""
    from kokoro_ruslan_amd.longform import join
    n = sum(int(chunks[c].numel()) for d in documents for c in d) + gap * sum(len(d) - 1 for d in documents)
    out = torch.full((n,), float("nan"), device="cuda")
    docs, peaks = join(chunks, documents, gap, fade, out=out)
    assert docs[0].data_ptr() == out.data_ptr() and sum(int(d.numel()) for d in docs) == n
    assert not bool(torch.isnan(out).any())
    return docs, peaks


@pytest.mark.parametrize("gap", LC.GAPS)
def test_wave_join_is_torch_cat(gap):
    _need_gpu()
    chunks = [c.cuda() for c in LC.join_chunks_input()]
    docs, peaks = _join(chunks, LC.DOCUMENTS, gap, 0)
    for d, want in zip(docs, LC.cat_documents(chunks, LC.DOCUMENTS, gap)):
        assert d.is_cuda and d.dtype == torch.float32 and torch.equal(_bits(d), _bits(want))
    assert torch.equal(_bits(peaks), _bits(torch.stack([c.abs().max() for c in chunks])))
    single = [[i] for i in range(len(chunks))]
    docs, peaks1 = _join(chunks, single, gap, 0)
    assert all(torch.equal(d, c) for d, c in zip(docs, chunks)) and torch.equal(peaks1, peaks)


@pytest.mark.parametrize("gap", LC.GAPS)
def test_wave_join_fades(gap):
    _need_gpu()
    F = 64
    chunks = [c.cuda() for c in LC.join_chunks_input()] + [torch.rand(100, generator=torch.Generator().manual_seed(9)).cuda() + 0.5]
    documents = list(LC.DOCUMENTS) + [[6]]
    table = fade_table(F).cuda()
    faded = []
    for c in chunks:
        nf = min(F, c.numel() // 2)
        x = c.clone()
        x[:nf] = c[:nf] * table[:nf]
        x[c.numel() - nf:] = c[c.numel() - nf:] * table[:nf].flip(0)
        faded.append(x)
    assert min(F, 100 // 2) == 50 and not torch.equal(faded[6], chunks[6])
    docs, peaks = _join(chunks, documents, gap, F)
    for d, want in zip(docs, LC.cat_documents(faded, documents, gap)):
        assert torch.equal(_bits(d), _bits(want))
    assert torch.equal(_bits(peaks), _bits(torch.stack([c.abs().max() for c in chunks])))      # before the fade


def test_wave_join_unaligned_offsets_and_arguments():
    _need_gpu()
    from kokoro_ruslan_amd.longform import join
    g = torch.Generator().manual_seed(21)
    lengths = [3, 4099, 1, 1027, 13, 2050]                                 # woff: 0, 3, 4102, 4103, 5130, 5143: odd from the second on
    chunks = [(torch.rand(n, generator=g) - 0.5).cuda() for n in lengths]
    chunks[3][5] = -3.0
    chunks[1][7] = -0.0
    documents = [[0, 1, 2], [3, 4, 5]]
    docs, peaks = _join(chunks, documents, 5, 0)                           # dst: 0, 8, 4112 | 4113, 5145, 5163: odd ones among them
    for d, want in zip(docs, LC.cat_documents(chunks, documents, 5)):
        assert torch.equal(_bits(d), _bits(want))
    assert float(peaks[3]) == 3.0 and torch.equal(_bits(peaks), _bits(torch.stack([c.abs().max() for c in chunks])))
    with pytest.raises(ValueError, match=r"documents\[1\] is empty"):
        join(chunks[:2], [[0, 1], []], 5)
    with pytest.raises(ValueError, match="exactly once"):
        join(chunks[:3], [[0, 1]], 5)
    with pytest.raises(ValueError, match="gap must be an integer >= 0, not -1"):
        join(chunks[:1], [[0]], -1)
    with pytest.raises(ValueError, match="fade must be an integer >= 0, not 2.5"):
        join(chunks[:1], [[0]], 0, 2.5)
    with pytest.raises(ValueError, match="waveform 1: shape"):
        join([chunks[0], torch.zeros(0).cuda()], [[0, 1]], 0)


def test_public_wrappers():
    _need_gpu()
    from kokoro.inference.audio import finish_mels, join_chunks
    cases, refs, (trimmed, info), fin = _table(80)
    t, i = finish_mels(fin, [cases[7][1].cuda(), cases[3][1].cuda()])
    assert torch.equal(t[0], trimmed[7]) and torch.equal(t[1], trimmed[3]) and i == [info[7], info[3]]
    chunks = [c.cuda() for c in LC.join_chunks_input()]
    docs, peaks = join_chunks(chunks, LC.DOCUMENTS, 22050)                 # int(22050 * 0.15) = 3307
    for d, want in zip(docs, LC.cat_documents(chunks, LC.DOCUMENTS, 3307)):
        assert torch.equal(d, want)
    docs, _ = join_chunks(chunks, LC.DOCUMENTS, 22050, gap_ms=0.0, fade_ms=64000 / 22050 + 1e-6)
    assert docs[1].numel() == 1 + 3307 + 255 and not torch.equal(docs[1][-255:], chunks[1])
    with pytest.raises(ValueError, match="gap_ms must be finite and >= 0, not -1"):
        join_chunks(chunks, LC.DOCUMENTS, 22050, gap_ms=-1)
