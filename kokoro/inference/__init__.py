"""Inference surface: batched mel synthesis from a trained checkpoint (see synth.py) HiFi-GAN / Griffin-Lim vocoding, spectral denoising, loudness normalisation and the two ends of long-form synthesis (see audio.py)."""
from kokoro.inference.audio import denoise, finish_mels, join_chunks, normalise_loudness, vocode, write_wav  # noqa: F401
from kokoro.inference.synth import (InferenceControls, load_for_inference, resolve_controls, synthesize,  # noqa: F401
                                    trim_trailing_silence)
