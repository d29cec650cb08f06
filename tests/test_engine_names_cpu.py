"""The one place that names a transformer layer's parameters, workspace buffers and RNG sites (engine.encoder_layer_names /
decoder_layer_names), pinned to the literals the launch sequences used to spell out at every call site: a site that drifts changes
the dropout masks between a layer's forward and its backward, and a key that drifts moves a buffer that tests, probes and captured
graphs address by name.  No GPU: the helpers are plain functions."""
import torch

from kokoro_ruslan_amd.engine import LayerNames, decoder_layer_names, encoder_layer_names
from kokoro_ruslan_amd.spec import ModelDims

D = ModelDims()
BF, F32 = torch.bfloat16, torch.float32


def test_default_dims_are_the_ones_the_literals_below_assume():
    assert (D.enc_layers, D.dec_layers) == (6, 6)


def test_encoder_first_layer():
    lay = encoder_layer_names(0, D.enc_layers, BF)
    assert isinstance(lay, LayerNames)
    assert lay.prefix == "transformer_encoder_layers.0" and lay.key == "enc0"
    assert lay.site == {"sa": 1000, "ff": 1008}
    assert lay.next_ln == {"sa": ("enc0.ln2", "transformer_encoder_layers.0.norm2", BF),
                           "ff": ("enc1.ln1", "transformer_encoder_layers.1.norm1", BF)}


def test_encoder_last_layer_ends_in_the_fp32_encoder_norm():
    lay = encoder_layer_names(5, D.enc_layers, BF)
    assert lay.prefix == "transformer_encoder_layers.5" and lay.key == "enc5"
    assert lay.site == {"sa": 1160, "ff": 1168}
    assert lay.next_ln["sa"] == ("enc5.ln2", "transformer_encoder_layers.5.norm2", BF)
    assert lay.next_ln["ff"] == ("enc.norm", "encoder_norm", torch.float32)
    assert encoder_layer_names(5, D.enc_layers, F32).next_ln["ff"] == ("enc.norm", "encoder_norm", torch.float32)


def test_decoder_first_layer():
    lay = decoder_layer_names(0, D.dec_layers, BF)
    assert lay.prefix == "decoder.layers.0" and lay.key == "dec0"
    assert lay.site == {"sa": 2000, "ca": 2008, "ff": 2016}
    assert lay.next_ln == {"sa": ("dec0.ln2", "decoder.layers.0.norm2", BF), "ca": ("dec0.ln3", "decoder.layers.0.norm3", BF),
                           "ff": ("dec1.ln1", "decoder.layers.1.norm1", BF)}


def test_decoder_last_layer_ends_in_decoder_norm_of_the_decoder_dtype():
    for dt in (BF, F32):
        lay = decoder_layer_names(5, D.dec_layers, dt)
        assert lay.prefix == "decoder.layers.5" and lay.key == "dec5"
        assert lay.site == {"sa": 2160, "ca": 2168, "ff": 2176}
        assert lay.next_ln["sa"] == ("dec5.ln2", "decoder.layers.5.norm2", dt)
        assert lay.next_ln["ca"] == ("dec5.ln3", "decoder.layers.5.norm3", dt)
        assert lay.next_ln["ff"] == ("dec.norm", "decoder.norm", dt)


def test_sites_of_every_layer_are_distinct_and_32_apart():
    enc = [encoder_layer_names(i, D.enc_layers, BF).site for i in range(D.enc_layers)]
    dec = [decoder_layer_names(i, D.dec_layers, BF).site for i in range(D.dec_layers)]
    assert [s["sa"] for s in enc] == [1000, 1032, 1064, 1096, 1128, 1160]
    assert [s["sa"] for s in dec] == [2000, 2032, 2064, 2096, 2128, 2160]
    every = [v for s in enc + dec for v in s.values()]
    assert len(set(every)) == len(every) == 2 * 6 + 3 * 6


def test_namespaced_keys_of_the_inference_paths():
    """generate_batch encodes under "syn.", the decode steps run under "gen." / "syn." / "str.": the namespace is in every workspace
    key and in no parameter prefix, and the sites do not depend on it."""
    lay = encoder_layer_names(5, D.enc_layers, BF, "syn.")
    assert lay.prefix == "transformer_encoder_layers.5" and lay.key == "syn.enc5" and lay.site == {"sa": 1160, "ff": 1168}
    assert lay.next_ln == {"sa": ("syn.enc5.ln2", "transformer_encoder_layers.5.norm2", BF), "ff": ("syn.enc.norm", "encoder_norm", F32)}
    assert encoder_layer_names(0, D.enc_layers, BF, "syn.").next_ln["ff"] == ("syn.enc1.ln1", "transformer_encoder_layers.1.norm1", BF)
    lay = decoder_layer_names(4, D.dec_layers, BF, "gen.")
    assert lay.prefix == "decoder.layers.4" and lay.key == "gen.dec4" and lay.site == {"sa": 2128, "ca": 2136, "ff": 2144}
    assert lay.next_ln == {"sa": ("gen.dec4.ln2", "decoder.layers.4.norm2", BF), "ca": ("gen.dec4.ln3", "decoder.layers.4.norm3", BF),
                           "ff": ("gen.dec5.ln1", "decoder.layers.5.norm1", BF)}
    assert decoder_layer_names(5, D.dec_layers, BF, "str.").next_ln["ff"] == ("str.dec.norm", "decoder.norm", BF)
