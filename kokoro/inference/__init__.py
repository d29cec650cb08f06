"""Inference surface: batched mel synthesis from a trained checkpoint (see synth.py)."""
from kokoro.inference.synth import (InferenceControls, load_for_inference, resolve_controls, synthesize,  # noqa: F401
                                    trim_trailing_silence)
