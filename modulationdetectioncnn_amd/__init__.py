"""MI355X-native inference path for the VT-CNN2-family modulation classifiers of
peteroh23/ModulationDetectionCNN.  Product code: formats + host surface +
libmdc.so (HIP).  The CPU oracle lives in /oracle and is never imported from here."""
from .topology import Topology, synthetic_weights, synthetic_frames  # noqa: F401
from .model import VTCNN2, Model, NonFiniteInputError  # noqa: F401
from .frontend import frames_from_iq_u8, normalized_frames_from_iq_u8, window_stats_iq_u8, window_power_dbfs  # noqa: F401
from .frontend import frames_from_iq, normalized_frames_from_iq, window_stats_iq  # noqa: F401
from .frontend import ddc, design_lowpass, phase_step  # noqa: F401
from .frontend import design_resampler, resample, resample_ratio  # noqa: F401
from .frontend import cf32_histogram, design_cf32_gain, quantize_cf32  # noqa: F401
from .frontend import RML2016_MODS, SynthRecipe, SynthFading, synth_recipe, synth_fading, synth_frames, synth_dataset  # noqa: F401
from .frontend import SynthScene, synth_scene, synth_capture, scene_truth, score_detections  # noqa: F401
from . import callbacks  # noqa: F401

__all__ = ["Topology", "VTCNN2", "Model", "callbacks", "synthetic_weights", "synthetic_frames", "frames_from_iq_u8", "NonFiniteInputError"]
