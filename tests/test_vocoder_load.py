"""HiFi-GAN vocoder on the CPU: weight-norm folding from the three checkpoint key forms, strict loading, checkpoint / config
resolution, the polyphase ConvTranspose1d packing, the packed-batch orchestration (kernel entry points emulated in torch), write_wav."""
import json

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kokoro_ruslan_amd import vocoder as V
from kokoro_ruslan_amd import vocoder_torch as VT

SMALL = {"upsample_rates": [4, 2], "upsample_kernel_sizes": [8, 4], "upsample_initial_channel": 32, "resblock_kernel_sizes": [3, 5],
         "resblock_dilation_sizes": [[1, 3], [1, 2]]}


def _torch_wn(module, new_style):
    if new_style:
        return nn.utils.parametrizations.weight_norm(module)
    return nn.utils.weight_norm(module)


@pytest.mark.parametrize("new_style", [False, True])
def test_weight_norm_folding_matches_torch(new_style):
    torch.manual_seed(0)
    for m in (nn.Conv1d(6, 5, 7, padding=3), nn.ConvTranspose1d(6, 4, 16, 8, padding=4)):
        with torch.no_grad():
            m.weight.normal_()
        m = _torch_wn(m, new_style)
        with torch.no_grad():
            if new_style:
                m.parametrizations.weight.original0.uniform_(0.5, 2.0)
            else:
                m.weight_g.uniform_(0.5, 2.0)
        with torch.no_grad():
            m(torch.zeros(1, 6, 20))                  # the old-style hook recomputes .weight before each forward
        sd = m.state_dict()
        g = sd["parametrizations.weight.original0" if new_style else "weight_g"]
        v = sd["parametrizations.weight.original1" if new_style else "weight_v"]
        assert g.shape == (v.shape[0], 1, 1)         # ConvTranspose1d: dim 0 is Cin
        torch.testing.assert_close(V.fold_weight_norm(g, v), m.weight.detach(), rtol=1e-6, atol=1e-7)


def test_convtranspose_folds_over_cin():
    v = torch.randn(6, 4, 8)
    g = torch.rand(6, 1, 1) + 0.5
    w = V.fold_weight_norm(g, v)
    torch.testing.assert_close(w.flatten(1).norm(dim=1), g.flatten(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("form", ["weight_norm", "parametrizations", "plain"])
def test_load_state_dict_three_forms_agree(form):
    ref = V.HifiganVocoder(SMALL, device="cpu", math_mode="f32")
    ref.load_state_dict(VT.random_state_dict(SMALL, seed=3, form="weight_norm"))
    voc = V.HifiganVocoder(SMALL, device="cpu", math_mode="f32")
    voc.load_state_dict(VT.random_state_dict(SMALL, seed=3, form=form))
    assert set(voc.weights) == set(ref.weights) == set(V.layer_shapes(voc.config))
    for n in ref.weights:
        torch.testing.assert_close(voc.weights[n], ref.weights[n], rtol=1e-6, atol=1e-7)
        assert torch.equal(voc.biases[n], ref.biases[n])


def test_load_state_dict_is_strict():
    sd = VT.random_state_dict(SMALL, seed=1)
    voc = V.HifiganVocoder(SMALL, device="cpu")
    bad = dict(sd)
    del bad["resblocks.1.convs2.0.weight_v"]
    with pytest.raises(KeyError, match="missing"):
        voc.load_state_dict(bad)
    bad = dict(sd)
    del bad["conv_post.bias"]
    with pytest.raises(KeyError, match="conv_post.bias"):
        voc.load_state_dict(bad)
    bad = dict(sd, **{"resblocks.9.convs1.0.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="unexpected"):
        voc.load_state_dict(bad)
    bad = dict(sd, **{"ups.0.weight_v": torch.randn(32, 16, 4)})
    with pytest.raises(ValueError, match="shape"):
        voc.load_state_dict(bad)


def test_config_validation():
    with pytest.raises(ValueError, match="k - stride even"):
        V.HifiganVocoder(dict(SMALL, upsample_kernel_sizes=[7, 4]), device="cpu")
    with pytest.raises(ValueError, match="k >= stride"):
        V.HifiganVocoder(dict(SMALL, upsample_kernel_sizes=[2, 4]), device="cpu")
    with pytest.raises(ValueError, match="resblock"):
        V.HifiganVocoder(dict(SMALL, resblock="2"), device="cpu")
    with pytest.raises(ValueError, match="num_mels"):
        V.HifiganVocoder(dict(SMALL, num_mels=100), device="cpu")
    d = V.HifiganVocoder(device="cpu")
    assert (d.rates, d.up_kernels, d.c0, d.res_kernels, d.hop, d.sampling_rate) == ([8, 8, 2, 2], [16, 16, 4, 4], 512, [3, 7, 11], 256, 22050)
    assert V.convt_taps(16, 8) == (-1, 3) and V.convt_taps(4, 2) == (-1, 3) and V.convt_taps(8, 4) == (-1, 3)
    assert V.convt_taps(2, 2) == (0, 1) and V.convt_taps(5, 1) == (-2, 5)


@pytest.mark.parametrize("k,u", [(16, 8), (4, 2), (8, 4), (2, 2), (7, 3), (5, 1), (12, 4)])
def test_polyphase_packing_is_conv_transpose(k, u):
    torch.manual_seed(k * 10 + u)
    cin, cout, L = 5, 3, 9
    w, x = torch.randn(cin, cout, k, dtype=torch.float64), torch.randn(1, cin, L, dtype=torch.float64)
    ref = F.conv_transpose1d(x, w, stride=u, padding=(k - u) // 2)[0].t()          # [L * u, cout]
    assert ref.shape[0] == L * u
    off0, taps = V.convt_taps(k, u)
    P = V.pack_convt(w, u, torch.float64)
    xr = x[0].t()
    y = torch.zeros(L, u * cout, dtype=torch.float64)
    for t in range(taps):
        for q in range(L):
            s = q + off0 + t
            if 0 <= s < L:
                y[q] += P[t, :u * cout, :cin] @ xr[s]
    torch.testing.assert_close(y.reshape(L * u, cout), ref)


# ---- the kernel entry points restated in torch (fp64), to run HifiganVocoder's packed orchestration on the CPU
def _emulate(name, *a):
    def conv(x, rows, cin, w, taps, off0, dil, n, bias, bmod, slope, seg, nseg, bf):
        x = x[:rows * cin].view(rows, cin).double()
        x = F.leaky_relu(x, slope) if slope != 1.0 else x
        if bf:
            x = x.to(torch.bfloat16).double()
        W = w[:, :n, :cin].double()
        out = torch.zeros(rows, n, dtype=torch.float64)
        s = seg[:nseg + 1].tolist()
        for b in range(nseg):
            lo, hi = s[b], s[b + 1]
            for j in range(taps):
                o = off0 + j * dil
                for r in range(lo, hi):
                    if lo <= r + o < hi:
                        out[r] += W[j] @ x[r + o]
        return out + bias.double()[torch.arange(n) % bmod]

    if name == "kk_voc_conv1d":
        x, rows, cin, w, kpad, npad, b, y, cout, k, d, slope, seg, nseg, res, mrf, div, bf = a
        v = conv(x, rows, cin, w, k, -(k - 1) // 2 * d, d, cout, b, cout, slope, seg, nseg, bf)
        yv = y[:rows * cout].view(rows, cout)
        if res is not None:
            v = v + res[:rows * cout].view(rows, cout).double()
        if mrf is not None:
            v = mrf[:rows * cout].view(rows, cout).double() + v
        if div:
            v = v / div
        yv.copy_(v.float())
    elif name == "kk_voc_convt1d":
        x, rows, cin, w, kpad, npad, b, y, cout, k, u, slope, seg, nseg, bf = a
        off0, taps = V.convt_taps(k, u)
        v = conv(x, rows, cin, w, taps, off0, 1, u * cout, b, cout, slope, seg, nseg, bf)
        y[:rows * u * cout].view(rows, u * cout).copy_(v.float())
    elif name == "kk_voc_post":
        x, rows, cin, w, b, y, k, slope, seg, nseg = a
        P = w.t()[None].double()                            # [1, cin, k]
        s = seg[:nseg + 1].tolist()
        xv = F.leaky_relu(x[:rows * cin].view(rows, cin).double(), slope)
        for i in range(nseg):
            y[s[i]:s[i + 1]] = torch.tanh(F.conv1d(xv[s[i]:s[i + 1]].t()[None], P, b.double(), padding=(k - 1) // 2))[0, 0].float()
    else:
        raise AssertionError(name)


TINY = {"upsample_rates": [2, 2], "upsample_kernel_sizes": [4, 4], "upsample_initial_channel": 16, "resblock_kernel_sizes": [3, 5],
        "resblock_dilation_sizes": [[1, 3], [1, 2]]}


def test_packed_orchestration_matches_restatement(monkeypatch):
    """vocode() on a ragged batch, its kernel calls emulated: the packing, the tap offsets, the residual / MRF wiring, the stage
    segment tables and the grouping give the torch restatement of each utterance alone."""
    monkeypatch.setattr(V.kk, "call", _emulate)
    sd = VT.random_state_dict(TINY, seed=4)
    voc = V.HifiganVocoder(TINY, device="cpu", math_mode="f32")
    voc.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    mels = [torch.randn(f, 80, generator=g) for f in (1, 3, 2, 5)]
    outs = voc.vocode(mels)
    outs2 = voc.vocode(mels, max_samples=6 * voc.hop)                  # several groups
    W = {n: w.double() for n, w in voc.weights.items()}
    for m, o, o2 in zip(mels, outs, outs2):
        ref = VT.forward(W, voc.biases, TINY, m.double())
        assert o.shape == (m.shape[0] * 4,) and float(ref.std()) > 0.05
        torch.testing.assert_close(o.double(), ref, rtol=0, atol=2e-5)
        assert torch.equal(o, o2)


def test_checkpoint_resolution(tmp_path):
    sd = VT.random_state_dict(SMALL, seed=2)
    d = tmp_path / "voc"
    d.mkdir()
    torch.save({"generator": sd}, d / "generator.pth")
    (d / "config.json").write_text(json.dumps(SMALL))
    assert V.resolve_checkpoint(str(d)) == (str(d / "generator.pth"), str(d / "config.json"))
    assert V.resolve_checkpoint(str(d / "generator.pth")) == (str(d / "generator.pth"), str(d / "config.json"))
    v = V.HifiganVocoder.from_checkpoint(str(d), device="cpu", math_mode="f32")
    assert v.rates == [4, 2] and v.c0 == 32
    # a file without a sibling config, or a config path that does not exist: the defaults
    lone = tmp_path / "lone"
    lone.mkdir()
    torch.save(VT.random_state_dict(None, seed=0, form="plain"), lone / "g.pt")
    assert V.resolve_checkpoint(str(lone / "g.pt")) == (str(lone / "g.pt"), None)
    assert V.resolve_checkpoint(str(lone / "g.pt"), str(lone / "nope.json")) == (str(lone / "g.pt"), None)
    assert V.HifiganVocoder.from_checkpoint(str(lone / "g.pt"), device="cpu").c0 == 512
    # an explicit config wins over the sibling; a bare state dict (no 'generator' key) loads too
    torch.save(sd, lone / "bare.pth")
    cfg = tmp_path / "c.json"
    cfg.write_text(json.dumps(SMALL))
    assert V.HifiganVocoder.from_checkpoint(str(lone / "bare.pth"), str(cfg), device="cpu").rates == [4, 2]
    with pytest.raises(FileNotFoundError):
        V.resolve_checkpoint(str(tmp_path / "missing"))


def test_write_wav_round_trip(tmp_path):
    from scipy.io import wavfile
    from kokoro.inference import write_wav
    a = torch.tensor([0.0, 0.25, -0.5, 0.1])
    p = tmp_path / "a.wav"
    write_wav(str(p), a, 22050)
    sr, data = wavfile.read(str(p))
    assert sr == 22050 and data.dtype == np.int16
    np.testing.assert_array_equal(data, (np.array([0.0, 0.5, -1.0, 0.2], dtype=np.float32) * 32767).astype(np.int16))
    write_wav(str(p), torch.full((3,), 1e-9), 16000)                # below the peak floor: not normalised
    sr, data = wavfile.read(str(p))
    assert sr == 16000 and data.tolist() == [0, 0, 0]


def test_vocode_clamps_before_the_vocoder():
    from kokoro.inference import vocode
    seen = []

    class Fake:
        def vocode(self, mels, **kw):
            seen.extend(mels)
            return [m[:, 0] for m in mels]

    m = torch.tensor([[5.0] * 80, [-20.0] * 80])
    vocode(Fake(), [m])
    assert seen[0].max() == 2.0 and seen[0].min() == -11.5
    vocode(Fake(), [m], clamp=False)
    assert torch.equal(seen[1], m)


def test_synth_parser_vocoder_flags():
    from kokoro.cli import synth as cli
    a = cli.build_parser().parse_args(["--checkpoint", "c", "--ids", "x", "--output", "o"])
    assert (a.vocoder, a.vocoder_config, a.vocoder_math) == (None, None, "bf16")
    a = cli.build_parser().parse_args(["--checkpoint", "c", "--ids", "x", "--output", "o", "--vocoder", "v", "--vocoder-config", "c.json",
                                       "--vocoder-math", "f32"])
    assert (a.vocoder, a.vocoder_config, a.vocoder_math) == ("v", "c.json", "f32")
