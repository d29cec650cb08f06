"""Inference surface: batched mel synthesis from a trained checkpoint (see synth.py) HiFi-GAN / Griffin-Lim vocoding and spectral denoising (see audio.py)."""
from kokoro.inference.audio import denoise, vocode, write_wav  # noqa: F401
from kokoro.inference.synth import (InferenceControls, load_for_inference, resolve_controls, synthesize,  # noqa: F401
                                    trim_trailing_silence)
