"""Inference surface: batched mel synthesis from a trained checkpoint (see synth.py) and HiFi-GAN vocoding (see audio.py)."""
from kokoro.inference.audio import vocode, write_wav  # noqa: F401
from kokoro.inference.synth import (InferenceControls, load_for_inference, resolve_controls, synthesize,  # noqa: F401
                                    trim_trailing_silence)
