"""ctypes binding of libmdc.so (include/mdc.h).  This is the stub INTEGRATION.md shows.

The product path has no CPU fallback: if the shared library is missing, cannot be
loaded, or reports no gfx950 device, the calls below raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdc.so")
# "alternates" = the -DMDC_ALTERNATES test build (build.py): the product kernels plus the measured-slower alternates the
# GPU suite holds them against.  Tests ask for it by name; nothing in the package does.
LIB_PATHS = {"product": LIB_PATH, "alternates": os.path.join(_HERE, "libmdc_alt.so")}

KIND_DEPLOYED, KIND_VTCNN2, KIND_CNNPY = 1, 2, 3
F32, BF16, FP8, F16 = 0, 1, 2, 3
TAP_NONE, TAP_CONV, TAP_FLAT, TAP_DENSE, TAP_HIDDEN = 0, 1, 2, 3, 4

EXPORTS = [
    "mdc_abi_version", "mdc_create", "mdc_num_layers", "mdc_layer_sizes", "mdc_set_weights",
    "mdc_finalize", "mdc_workspace_bytes", "mdc_forward", "mdc_set_profiling", "mdc_profile_slots",
    "mdc_profile_name", "mdc_profile_read", "mdc_profile_reset", "mdc_last_error", "mdc_destroy",
    "mdc_forward_q612", "mdc_confusion", "mdc_iq_u8_to_frames", "mdc_set_fp8_input_absmax",
    "mdc_forward_iq_u8", "mdc_confusion_binned", "mdc_iq_u8_windows", "mdc_predict_host", "mdc_predict_host_iq_u8",
    "mdc_crossentropy", "mdc_set_fp8_feature_absmax",
    "mdc_trainer_create", "mdc_trainer_num_layers", "mdc_trainer_layer_sizes", "mdc_trainer_set_adam", "mdc_trainer_set_dropout", "mdc_trainer_set_tensor",
    "mdc_trainer_get_tensor", "mdc_trainer_set_iterations", "mdc_train_batch", "mdc_trainer_evaluate", "mdc_trainer_read",
    "mdc_trainer_destroy",
    "mdc_head_trainer_create", "mdc_head_trainer_set_adam", "mdc_head_trainer_set_dropout", "mdc_head_trainer_set_tensor", "mdc_head_trainer_get_tensor",
    "mdc_head_trainer_set_iterations", "mdc_head_train_batch", "mdc_head_trainer_evaluate", "mdc_head_trainer_read", "mdc_head_trainer_destroy",
    "mdc_forward_checked", "mdc_predict_host_checked",
    "mdc_iq_u8_windows_norm", "mdc_predict_host_iq_u8_norm",
    "mdc_iq_windows", "mdc_iq_windows_norm", "mdc_predict_host_iq", "mdc_predict_host_iq_norm",
    "mdc_iq_ddc", "mdc_iq_ddc_out_count", "mdc_iq_ddc_nco_table",
    "mdc_iq_resample", "mdc_iq_resample_out_count",
    "mdc_iq_extract", "mdc_iq_extract_plan", "mdc_iq_extract_plan_bytes",
    "mdc_iq_spectrogram", "mdc_iq_spectrogram_rows", "mdc_iq_line_spectrum",
    "mdc_iq_channelizer", "mdc_iq_channelizer_out_count",
    "mdc_iq_spectrum_quantiles",
    "mdc_iq_spectrogram_components", "mdc_iq_spectrogram_components_workspace",
    "mdc_iq_spectrogram_cfar",
    "mdc_iq_line_spectra", "mdc_iq_line_spectra_rows", "mdc_iq_find_lines",
    "mdc_iq_balance", "mdc_iq_balance_stats", "mdc_iq_balance_blocks",
    "mdc_iq_cf32_histogram", "mdc_iq_cf32_quantize",
    "mdc_iq_synth_plan_bytes", "mdc_iq_synth_plan", "mdc_iq_synth_frames", "mdc_iq_synth_frames_faded",
    "mdc_iq_synth_scene_bytes", "mdc_iq_synth_scene", "mdc_iq_synth_scene_hops", "mdc_iq_synth_capture_workspace_bytes", "mdc_iq_synth_capture",
]
ABI_VERSION = 5
TRAIN_WEIGHTS, TRAIN_ADAM_M, TRAIN_ADAM_V, TRAIN_GRADIENT = 0, 1, 2, 3
MDC_OPT_FP8_BF16_FEATURES = 1      # include/mdc.h: option bit in mdc_topology.reserved[0]
HOP_FRAME = 128
NONFINITE_REPORT, NONFINITE_PROPAGATE = 0, 1     # include/mdc.h: policies of mdc_forward_checked / mdc_predict_host_checked
IQ_REMOVE_DC = 1                                 # include/mdc.h: flag of mdc_iq_u8_windows_norm / mdc_predict_host_iq_u8_norm
# mdc_iq_window_stats (16 B): one record per window, exact integers (s = 2*byte - 255)
IQ_WINDOW_STATS = np.dtype([("sum_i", np.int32), ("sum_q", np.int32), ("sum_sq", np.uint32), ("energy", np.uint32)])
# sample formats of mdc_iq_windows / mdc_iq_windows_norm / mdc_predict_host_iq(_norm): MDC_IQ_*, bytes per (I,Q) pair, numpy dtype
IQ_CU8, IQ_CI8, IQ_CI16 = 0, 1, 2
IQ_PAIR_BYTES = {IQ_CU8: 2, IQ_CI8: 2, IQ_CI16: 4}
IQ_SAMPLE_DTYPE = {IQ_CU8: np.dtype(np.uint8), IQ_CI8: np.dtype(np.int8), IQ_CI16: np.dtype("<i2")}
# mdc_iq_window_stats64 (32 B): the same four exact integers for any format (s: include/mdc.h)
IQ_WINDOW_STATS64 = np.dtype([("sum_i", np.int64), ("sum_q", np.int64), ("sum_sq", np.uint64), ("energy", np.uint64)])


class IqWindowEntries(NamedTuple):
    """What differs between the two families of window entries: the names, whether they take an MDC_IQ_* format, and the record"""
    frames: str
    frames_norm: str
    host: str
    host_norm: str
    takes_format: bool
    stats: np.dtype


# unsigned bytes through their own kernels and the 16-byte record; any format (unsigned bytes too) through the 32-byte record's
IQ_U8_ENTRIES = IqWindowEntries("mdc_iq_u8_windows", "mdc_iq_u8_windows_norm", "mdc_predict_host_iq_u8", "mdc_predict_host_iq_u8_norm", False,
                                IQ_WINDOW_STATS)
IQ_ENTRIES = IqWindowEntries("mdc_iq_windows", "mdc_iq_windows_norm", "mdc_predict_host_iq", "mdc_predict_host_iq_norm", True, IQ_WINDOW_STATS64)
# mdc_iq_ddc: limits of include/mdc.h, and the kernel's tiling (csrc/iq_ddc.hip: kDdcTilePairs, kDdcGridCap) for tests and tools
DDC_MAX_DECIMATE, DDC_MAX_TAPS, DDC_MAX_TAPS_ABS_SUM, DDC_NCO_ENTRIES = 256, 1024, 65535, 4096
DDC_TILE_PAIRS, DDC_GRID_CAP = 8192, 1024
# mdc_iq_balance_stats / mdc_iq_balance: limits of include/mdc.h, the coefficient record (mdc_iq_balance_coeffs, 24 B), and the
# kernels' grids (csrc/iq_balance.hip: kBalStatsGridCap blocks in flight; kBalGridCap work-groups of BALANCE_GROUP_PAIRS pairs)
BALANCE_MIN_BLOCK, BALANCE_MAX_BLOCK = 64, 1 << 20
BALANCE_MAX_DC, BALANCE_MAX_ROW_ABS_SUM, BALANCE_ONE = 32768, 32767, 16384
BALANCE_STATS_GRID_CAP, BALANCE_GRID_CAP, BALANCE_GROUP_PAIRS = 2048, 2048, 1024
IQ_BALANCE_COEFFS = np.dtype([("dc_i", np.int32), ("dc_q", np.int32), ("m00", np.int32), ("m01", np.int32), ("m10", np.int32), ("m11", np.int32)])
# mdc_iq_cf32_histogram / mdc_iq_cf32_quantize: limits of include/mdc.h (the gain's range, pairs per call), and the kernels' grid
# (csrc/iq_cf32.hip: at most kCfGridCap work-groups, each taking CF32_GROUP_PAIRS pairs per stride step)
CF32_MIN_GAIN, CF32_MAX_GAIN, CF32_MAX_PAIRS = 2.0 ** -126, 2.0 ** 125, 1 << 40
CF32_GRID_CAP, CF32_GROUP_PAIRS = 1024, 1024
# mdc_iq_synth_plan / mdc_iq_synth_frames: the class record of include/mdc.h (mdc_iq_synth_class, 40 B), its limits, and the kernel's
# walk (csrc/iq_synth.hip: kSynGridCap work-groups of SYNTH_GROUP_FRAMES waves, one frame per wave; more frames are walked in passes)
SYNTH_ALPHABET, SYNTH_GAUSS, SYNTH_LINEAR, SYNTH_PHASE = 0, 1, 0, 1
IQ_SYNTH_CLASS = np.dtype([("source", np.int32), ("points", np.int32), ("first_point", np.int32), ("sps", np.int32), ("span", np.int32),
                           ("first_tap", np.int32), ("mode", np.int32), ("phase_factor", np.int32), ("amplitude", np.int16),
                           ("add_re", np.int16), ("add_im", np.int16), ("reserved", np.int16)])
SYNTH_MAX_CLASSES, SYNTH_MAX_SNRS, SYNTH_MAX_POINTS, SYNTH_MAX_SPS, SYNTH_MAX_SPAN, SYNTH_MAX_TAPS = 64, 64, 64, 16, 16, 128
SYNTH_GAUSS_MAX, SYNTH_MAX_STEP, SYNTH_MAX_Q, SYNTH_MAX_FRAMES = 262140, 1 << 30, 40, 1 << 30
SYNTH_GRID_CAP, SYNTH_GROUP_FRAMES = 2048, 4
# mdc_iq_synth_frames_faded: the fading record of include/mdc.h (mdc_iq_synth_path, 48 B; mdc_iq_synth_fading, 208 B) and its limits;
# delay taps are Q14 (SYNTH_FADING_TAP_ONE), path gains Q13 (SYNTH_FADING_GAIN_ONE)
IQ_SYNTH_PATH = np.dtype([("delay_taps", np.int16, (16,)), ("los_re", np.int16), ("los_im", np.int16), ("scatter", np.int32),
                          ("reserved", np.int32, (2,))])
IQ_SYNTH_FADING = np.dtype([("paths", np.int32), ("taps", np.int32), ("max_doppler_step", np.uint32), ("reserved", np.int32),
                            ("path", IQ_SYNTH_PATH, (4,))])
SYNTH_MAX_PATHS, SYNTH_MAX_DELAY_TAPS, SYNTH_MAX_DOPPLER_STEP = 4, 16, 1 << 30
SYNTH_FADING_TAP_ONE, SYNTH_FADING_GAIN_ONE, SYNTH_FADING_MAX_ABS_SUM = 16384, 8192, 32767
# mdc_iq_synth_scene / mdc_iq_synth_capture: the emitter record of include/mdc.h (mdc_iq_synth_emitter, 96 B), its limits, and the
# kernel's walk (csrc/iq_synth_capture.hip: one work-group per tile of SYNTH_CAPTURE_TILE pairs, at most SYNTH_CAPTURE_GRID_CAP)
IQ_SYNTH_EMITTER = np.dtype([("cls", np.int32), ("interpolate", np.int32), ("decimate", np.int32), ("first_tap", np.int32), ("ntaps", np.int32),
                             ("gain", np.int32), ("phase0", np.uint32), ("hops", np.int32), ("phase_step", np.uint32, (8,)), ("start", np.int64),
                             ("on", np.int64), ("period", np.int64), ("reserved", np.int32, (2,))])
SYNTH_SCENE_MAX_EMITTERS, SYNTH_SCENE_MAX_INTERPOLATE, SYNTH_SCENE_MAX_TAPS, SYNTH_SCENE_MAX_BRANCH_TAPS = 32, 32, 1024, 64
SYNTH_SCENE_MAX_BRANCH_ABS_SUM, SYNTH_SCENE_MAX_HOPS, SYNTH_SCENE_MAX_TIME, SYNTH_CAPTURE_MAX_PAIRS = 65535, 8, 1 << 52, 1 << 34
SYNTH_CAPTURE_TILE, SYNTH_CAPTURE_GRID_CAP = 1024, 4096
# mdc_iq_resample: limits of include/mdc.h (taps and decimation as the DDC's; the sum |h| bound holds per BRANCH), and the kernel's
# tiling (csrc/iq_resample.hip): a tile is ((RESAMPLE_TILE_PAIRS - ceil(T / L)) // D) * L outputs, RESAMPLE_GRID_CAP work-groups
RESAMPLE_MAX_INTERPOLATE, RESAMPLE_MAX_DECIMATE, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_BRANCH_ABS_SUM = 32, 256, 1024, 65535
RESAMPLE_TILE_PAIRS, RESAMPLE_GRID_CAP = 8192, 1024
# mdc_iq_extract: the records of include/mdc.h (mdc_iq_extract_filter, 16 B; mdc_iq_extract_job, 48 B).  Limits and tiling are the
# resampler's, per filter; the kernel strides over the plan's (job, tile) list with at most RESAMPLE_GRID_CAP work-groups
IQ_EXTRACT_FILTER = np.dtype([("interpolate", np.int32), ("decimate", np.int32), ("ntaps", np.int32), ("first_tap", np.int32)])
IQ_EXTRACT_JOB = np.dtype([("first_pair", np.int64), ("pairs", np.int64), ("out_first", np.int64), ("n_out", np.int64),
                           ("phase0", np.uint32), ("phase_step", np.uint32), ("filter", np.int32), ("reserved", np.int32)])
# mdc_iq_spectrogram: limits of include/mdc.h, and the kernel's grid (csrc/iq_spectrogram.hip: kSpecGridCap): one work-group per
# row, at most SPECTROGRAM_GRID_CAP of them; more rows are walked in passes
SPECTROGRAM_MIN_NFFT, SPECTROGRAM_MAX_NFFT, SPECTROGRAM_MAX_AVG = 64, 4096, 4096
SPECTROGRAM_GRID_CAP = 2048
# mdc_iq_line_spectrum: the same kernel and limits; `order` is 0 (MDC_IQ_LINE_ENVELOPE: I^2 + Q^2), 1 (the spectrogram), 2 or 4
IQ_LINE_ENVELOPE = 0
LINE_SPECTRUM_ORDERS = (0, 1, 2, 4)
# mdc_iq_line_spectra: the job record of include/mdc.h (mdc_iq_line_job, 32 B), up to LINE_SPECTRA_MAX_ORDERS distinct orders per
# call; the row kernel is the spectrogram's (one work-group per (order, row), SPECTROGRAM_GRID_CAP of them at most)
IQ_LINE_JOB = np.dtype([("first_pair", np.int64), ("pairs", np.int64), ("first_row", np.int64), ("rows", np.int64)])
LINE_SPECTRA_MAX_ORDERS = 4
# mdc_iq_find_lines: the band and the record of include/mdc.h (mdc_iq_line_band, 24 B; mdc_iq_line_record, 48 B)
IQ_LINE_BAND = np.dtype([("lo", np.float64), ("hi", np.float64), ("two_sided", np.int32), ("reserved", np.int32)])
IQ_LINE_RECORD = np.dtype([("bin", np.int32), ("count", np.int32), ("peak", np.float64), ("left", np.float64), ("right", np.float64),
                           ("median_lo", np.float64), ("median_hi", np.float64)])
# mdc_iq_spectrum_quantiles: limits of include/mdc.h, and the kernel's tile (csrc/iq_quantiles.hip: kQuantTile): one work-group
# per QUANTILES_TILE adjacent columns
QUANTILES_MAX_RANKS, QUANTILES_MAX_ROWS = 8, 2 ** 31 - 1
QUANTILES_TILE = 16
# mdc_iq_spectrogram_components: limits of include/mdc.h, the record (mdc_iq_component, 32 B), and the kernels' decomposition
# (csrc/iq_components.hip: kTileRows x kTileCols cells are labelled in LDS; the workspace holds one counter per COMPONENTS_CHUNK cells)
COMPONENTS_MAX_REACH, COMPONENTS_MAX_CELLS = 4, 2 ** 31 - 1
COMPONENTS_TILE_ROWS, COMPONENTS_TILE_COLS, COMPONENTS_CHUNK = 32, 64, 1024
IQ_COMPONENT = np.dtype([("row_first", np.int32), ("row_stop", np.int32), ("bin_first", np.int32), ("bin_stop", np.int32),
                         ("cells", np.int32), ("peak", np.float32), ("peak_row", np.int32), ("peak_bin", np.int32)])
# mdc_iq_spectrogram_cfar: limits of include/mdc.h, and the kernel's tile (csrc/iq_cfar.hip: kCfarTileRows x kCfarTileCols cells per
# work-group, CFAR_LANE_CELLS consecutive rows of a column per lane)
CFAR_MAX_TRAIN_ROWS, CFAR_MAX_TRAIN_BINS = 16, 128
CFAR_TILE_ROWS, CFAR_TILE_COLS, CFAR_LANE_CELLS = 16, 64, 4
# mdc_iq_channelizer: limits of include/mdc.h (channels a power of two in MIN..MAX, decimate <= channels, ntaps <= 16 per channel,
# per-residue sum |h| <= 65535), and the kernel's tiling (csrc/iq_channelizer.hip: kChanGridCap, chan_tile_steps): a work-group
# owns channelizer_tile_steps(channels) consecutive output steps, at most CHANNELIZER_GRID_CAP work-groups; more tiles are
# walked in passes
CHANNELIZER_MIN_CHANNELS, CHANNELIZER_MAX_CHANNELS, CHANNELIZER_MAX_TAPS_PER_CHANNEL, CHANNELIZER_MAX_TAP_SHIFT = 8, 1024, 16, 15
CHANNELIZER_MAX_BRANCH_ABS_SUM = 65535
CHANNELIZER_GRID_CAP = 2048


def channelizer_tile_steps(channels: int) -> int:
    """Output steps one work-group of mdc_iq_channelizer owns at a time: max(16, 1024 / channels)."""
    return max(16, 1024 // int(channels))
# mdc_forward_q612: the kernel's walk (csrc/deployed_q612.hip: kQGridCap, kQBlockFrames) for tests and tools -- at most Q612_GRID_CAP
# work-groups of 4 waves, each wave taking Q612_BLOCK_FRAMES frames at a time; more frames than that product are walked in passes
Q612_GRID_CAP, Q612_BLOCK_FRAMES = 2048, 64


class MdcTopology(C.Structure):
    _fields_ = [("kind", C.c_int32), ("filters", C.c_int32), ("hidden", C.c_int32),
                ("classes", C.c_int32), ("reserved", C.c_int32 * 4)]


class MdcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmdc error {code}: {msg}")
        self.code = code


_libs: dict = {}


def lib(variant: str = "product") -> C.CDLL:
    """Load libmdc.so (once).  Raises if the HIP extension has not been built."""
    if variant in _libs:
        return _libs[variant]
    path = LIB_PATHS[variant]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m modulationdetectioncnn_amd.build` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    # torch FIRST: its wheel bundles its own libamdhip64.so, libmdc.so names the system's as DT_NEEDED, and whichever HIP runtime a
    # process loads first serves both (same soname).  Loaded the other way round the process ends up with TWO runtimes, and
    # the one under libmdc.so then finds no device (`mdc_create`: MDC_ENODEV) -- measured on the GPU box, round 5.  The Python
    # mirror hands torch tensors to the library anyway; a caller without torch (examples/c_client.c) has one runtime by construction.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    L.mdc_abi_version.restype = i32
    L.mdc_create.argtypes = [C.POINTER(MdcTopology), i32, C.POINTER(vp)]
    L.mdc_num_layers.argtypes = [vp]
    L.mdc_layer_sizes.argtypes = [vp, i32, C.POINTER(sz), C.POINTER(sz)]
    L.mdc_set_weights.argtypes = [vp, i32, C.POINTER(C.c_float), sz, C.POINTER(C.c_float), sz]
    L.mdc_finalize.argtypes = [vp, i32]
    L.mdc_workspace_bytes.argtypes = [vp, i64]
    L.mdc_workspace_bytes.restype = sz
    L.mdc_forward.argtypes = [vp, vp, i64, vp, vp, vp, i32, vp, sz, vp]
    L.mdc_set_profiling.argtypes = [vp, i32]
    L.mdc_profile_slots.argtypes = [vp]
    L.mdc_profile_name.argtypes = [vp, i32]
    L.mdc_profile_name.restype = C.c_char_p
    L.mdc_profile_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i64)]
    L.mdc_profile_reset.argtypes = [vp]
    L.mdc_last_error.restype = C.c_char_p
    L.mdc_destroy.argtypes = [vp]
    L.mdc_destroy.restype = None
    L.mdc_forward_q612.argtypes = [vp, vp, i32, i64, vp, vp, vp]
    L.mdc_confusion.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.mdc_iq_u8_to_frames.argtypes = [vp, i64, C.c_float, vp, vp]
    L.mdc_set_fp8_input_absmax.argtypes = [vp, C.c_float]
    L.mdc_set_fp8_feature_absmax.argtypes = [vp, C.c_float]
    L.mdc_forward_iq_u8.argtypes = [vp, vp, i64, i64, C.c_float, vp, vp, vp, sz, vp]
    L.mdc_confusion_binned.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp]
    L.mdc_iq_u8_windows.argtypes = [vp, i64, i64, C.c_float, vp, vp]
    L.mdc_predict_host.argtypes = [vp, vp, i64, vp, vp, i64]
    L.mdc_predict_host_iq_u8.argtypes = [vp, vp, i64, i64, C.c_float, vp, vp, i64]
    L.mdc_crossentropy.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    # (getattr with a default: tools/ab_libs.py loads builds from before these entries; tests/test_nonfinite_abi.py holds
    # both libraries of this tree to exporting them)
    for name, args in (("mdc_forward_checked", [vp, vp, i64, vp, vp, vp, sz, vp, vp, i32, vp]),
                       ("mdc_predict_host_checked", [vp, vp, i64, vp, vp, vp, vp, i32, i64]),
                       ("mdc_iq_u8_windows_norm", [vp, i64, i64, C.c_float, i32, vp, vp, vp]),
                       ("mdc_predict_host_iq_u8_norm", [vp, vp, i64, i64, C.c_float, i32, vp, vp, vp, i64]),
                       ("mdc_iq_windows", [vp, i32, i64, i64, C.c_float, vp, vp]),
                       ("mdc_iq_windows_norm", [vp, i32, i64, i64, C.c_float, i32, vp, vp, vp]),
                       ("mdc_predict_host_iq", [vp, vp, i32, i64, i64, C.c_float, vp, vp, i64]),
                       ("mdc_predict_host_iq_norm", [vp, vp, i32, i64, i64, C.c_float, i32, vp, vp, vp, i64]),
                       ("mdc_iq_ddc_nco_table", [vp]),
                       ("mdc_iq_ddc", [vp, i32, i64, C.c_uint32, C.c_uint32, i32, vp, i32, vp, i64, vp]),
                       ("mdc_iq_resample", [vp, i32, i64, C.c_uint32, C.c_uint32, i32, i32, vp, i32, vp, i64, vp]),
                       ("mdc_iq_extract_plan", [i32, i64, vp, i64, vp, C.c_int32, vp, i64, i64, vp, i64]),
                       ("mdc_iq_extract", [vp, i32, i64, vp, vp, i64, vp, i64, vp]),
                       ("mdc_iq_spectrogram", [vp, i32, i64, i32, i64, i32, vp, C.c_float, vp, i64, vp]),
                       ("mdc_iq_line_spectrum", [vp, i32, i64, i32, i32, i64, i32, vp, C.c_float, vp, i64, vp]),
                       ("mdc_iq_channelizer", [vp, i32, i64, i64, i32, i32, vp, i32, i32, vp, i64, vp]),
                       ("mdc_iq_spectrum_quantiles", [vp, i64, i32, vp, i32, vp, vp]),
                       ("mdc_iq_spectrogram_components", [vp, i64, i32, vp, i32, i32, vp, vp, i64, vp, vp, vp]),
                       ("mdc_iq_spectrogram_cfar", [vp, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
                       ("mdc_iq_line_spectra", [vp, i32, i64, vp, vp, i64, vp, i32, i32, i64, i32, vp, C.c_float, vp, i64, vp, vp]),
                       ("mdc_iq_find_lines", [vp, i64, i32, vp, vp, vp, vp]),
                       ("mdc_iq_balance_stats", [vp, i32, i64, i64, vp, i64, vp]),
                       ("mdc_iq_balance", [vp, i32, i64, vp, vp, vp]),
                       ("mdc_iq_cf32_histogram", [vp, i64, vp, vp]),
                       ("mdc_iq_cf32_quantize", [vp, i64, C.c_float, vp, vp, vp]),
                       ("mdc_iq_synth_plan", [vp, C.c_int32, vp, i64, vp, i64, vp, i64, vp, C.c_int32, C.c_uint32, C.c_int32, vp, i64]),
                       ("mdc_iq_synth_frames", [vp, vp, i64, C.c_uint64, C.c_uint64, i64, vp, vp, vp, vp, vp]),
                       ("mdc_iq_synth_frames_faded", [vp, vp, i64, C.c_uint64, C.c_uint64, i64, vp, vp, vp, vp, vp, vp]),
                       ("mdc_iq_synth_scene", [vp, i64, vp, C.c_int32, vp, i64, C.c_int32, C.c_int32, C.c_int16, C.c_int16, vp, i64]),
                       ("mdc_iq_synth_scene_hops", [vp, i64, C.c_uint64, C.c_int32, i64, i64, vp]),
                       ("mdc_iq_synth_capture", [vp, vp, i64, vp, vp, i64, C.c_uint64, i64, vp, vp, vp, i64, vp])):
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, i32
    if getattr(L, "mdc_iq_ddc_out_count", None) is not None:
        L.mdc_iq_ddc_out_count.argtypes, L.mdc_iq_ddc_out_count.restype = [i64, i32, i32], i64
    if getattr(L, "mdc_iq_balance_blocks", None) is not None:
        L.mdc_iq_balance_blocks.argtypes, L.mdc_iq_balance_blocks.restype = [i64, i64], i64
    if getattr(L, "mdc_iq_resample_out_count", None) is not None:
        L.mdc_iq_resample_out_count.argtypes, L.mdc_iq_resample_out_count.restype = [i64, i32, i32, i32], i64
    if getattr(L, "mdc_iq_extract_plan_bytes", None) is not None:
        L.mdc_iq_extract_plan_bytes.argtypes, L.mdc_iq_extract_plan_bytes.restype = [i64, C.c_int32, vp, vp], i64
    if getattr(L, "mdc_iq_synth_plan_bytes", None) is not None:
        L.mdc_iq_synth_plan_bytes.argtypes, L.mdc_iq_synth_plan_bytes.restype = [C.c_int32, C.c_int32, vp], i64
    if getattr(L, "mdc_iq_synth_scene_bytes", None) is not None:
        L.mdc_iq_synth_scene_bytes.argtypes, L.mdc_iq_synth_scene_bytes.restype = [C.c_int32, i64], i64
    if getattr(L, "mdc_iq_synth_capture_workspace_bytes", None) is not None:
        L.mdc_iq_synth_capture_workspace_bytes.argtypes, L.mdc_iq_synth_capture_workspace_bytes.restype = [vp, i64, i64], i64
    if getattr(L, "mdc_iq_spectrogram_rows", None) is not None:
        L.mdc_iq_spectrogram_rows.argtypes, L.mdc_iq_spectrogram_rows.restype = [i64, i32, i64, i32], i64
    if getattr(L, "mdc_iq_line_spectra_rows", None) is not None:
        L.mdc_iq_line_spectra_rows.argtypes, L.mdc_iq_line_spectra_rows.restype = [vp, i64, i64, i32, i64, i32], i64
    if getattr(L, "mdc_iq_channelizer_out_count", None) is not None:
        L.mdc_iq_channelizer_out_count.argtypes, L.mdc_iq_channelizer_out_count.restype = [i64, i32, i32, i32], i64
    if getattr(L, "mdc_iq_spectrogram_components_workspace", None) is not None:
        L.mdc_iq_spectrogram_components_workspace.argtypes, L.mdc_iq_spectrogram_components_workspace.restype = [i64, i32], i64
    fp = C.POINTER(C.c_float)
    L.mdc_trainer_create.argtypes = [C.POINTER(MdcTopology), i32, C.POINTER(vp)]
    L.mdc_trainer_num_layers.argtypes = [vp]
    L.mdc_trainer_layer_sizes.argtypes = [vp, i32, C.POINTER(sz), C.POINTER(sz)]
    L.mdc_trainer_set_adam.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
    L.mdc_trainer_set_dropout.argtypes = [vp, C.c_float, C.c_uint32]
    L.mdc_trainer_set_tensor.argtypes = [vp, i32, i32, fp, sz, fp, sz, vp]
    L.mdc_trainer_get_tensor.argtypes = [vp, i32, i32, fp, sz, fp, sz, vp]
    L.mdc_trainer_set_iterations.argtypes = [vp, i64, vp]
    L.mdc_train_batch.argtypes = [vp, vp, vp, i64, vp, i64, i64, i32, vp]
    L.mdc_trainer_evaluate.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp]
    L.mdc_trainer_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64), vp]
    L.mdc_trainer_destroy.argtypes = [vp]
    L.mdc_trainer_destroy.restype = None
    # head training (getattr with a default, as above: tools/ab_libs.py loads builds from before these entries)
    dp = C.POINTER(C.c_double)
    for name, args in (("mdc_head_trainer_create", [i32, i32, i32, i64, i32, C.POINTER(vp)]),
                       ("mdc_head_trainer_set_adam", [vp, C.c_float, C.c_float, C.c_float, C.c_float]),
                       ("mdc_head_trainer_set_dropout", [vp, C.c_float, C.c_float, C.c_uint32]),
                       ("mdc_head_trainer_set_tensor", [vp, i32, i32, fp, sz, fp, sz, vp]),
                       ("mdc_head_trainer_get_tensor", [vp, i32, i32, fp, sz, fp, sz, vp]),
                       ("mdc_head_trainer_set_iterations", [vp, i64, vp]),
                       ("mdc_head_train_batch", [vp, vp, vp, i64, vp, i64, i64, i32, vp]),
                       ("mdc_head_trainer_evaluate", [vp, vp, vp, i64, vp, i64, i64, vp]),
                       ("mdc_head_trainer_read", [vp, i32, dp, C.POINTER(i64), dp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp])):
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, i32
    if getattr(L, "mdc_head_trainer_destroy", None) is not None:
        L.mdc_head_trainer_destroy.argtypes, L.mdc_head_trainer_destroy.restype = [vp], None
    for name in ("mdc_create", "mdc_num_layers", "mdc_layer_sizes", "mdc_set_weights", "mdc_finalize",
                 "mdc_forward", "mdc_set_profiling", "mdc_profile_slots", "mdc_profile_read", "mdc_profile_reset",
                 "mdc_forward_q612", "mdc_confusion", "mdc_iq_u8_to_frames", "mdc_set_fp8_input_absmax", "mdc_forward_iq_u8",
                 "mdc_confusion_binned", "mdc_iq_u8_windows", "mdc_predict_host", "mdc_predict_host_iq_u8", "mdc_crossentropy", "mdc_set_fp8_feature_absmax",
                 "mdc_trainer_create", "mdc_trainer_num_layers", "mdc_trainer_layer_sizes", "mdc_trainer_set_adam", "mdc_trainer_set_dropout", "mdc_trainer_set_tensor",
                 "mdc_trainer_get_tensor", "mdc_trainer_set_iterations", "mdc_train_batch", "mdc_trainer_evaluate", "mdc_trainer_read"):
        getattr(L, name).restype = i32
    if L.mdc_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{os.path.basename(path)} ABI version {L.mdc_abi_version()} != {ABI_VERSION}; rebuild it")
    _libs[variant] = L
    return L


def check(rc: int, variant: str = "product") -> int:
    if rc < 0:
        raise MdcError(rc, lib(variant).mdc_last_error().decode("utf-8", "replace"))
    return rc
