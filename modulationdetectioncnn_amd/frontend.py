"""Raw SDR samples -> frames (the RTL-SDR/HPS glue of the reference's README.md:5).

An RTL-SDR delivers unsigned 8-bit interleaved (I, Q) samples; a frame of the classifier is 128 such pairs
(256 bytes).  `frames_from_iq_u8` turns a device-resident byte buffer into the (n,2,128) float32 tensor every
`predict` entry point takes, on the device (mdc_iq_u8_to_frames), so the host never touches the samples.
"""
from __future__ import annotations

import numpy as np

from . import _cabi

DEFAULT_SCALE = 1.0 / 127.5
HOP_FRAME = 128


def window_count(nbytes: int, hop: int = HOP_FRAME) -> int:
    """Windows of 128 (I,Q) pairs, `hop` pairs apart, that fit a capture of nbytes bytes.  hop = 128 (disjoint frames)
    keeps the strict rule of the frame format: a trailing partial frame is an error."""
    if hop < 1:
        raise ValueError("hop must be >= 1 sample pair")
    if hop == HOP_FRAME:
        if nbytes % 256:
            raise ValueError(f"{nbytes} bytes is not a whole number of 256-byte frames")
        return nbytes // 256
    if nbytes % 2:
        raise ValueError(f"{nbytes} bytes is not a whole number of (I,Q) pairs")
    pairs = nbytes // 2
    return 0 if pairs < 128 else (pairs - 128) // hop + 1


def frames_from_iq_u8(iq, scale: float = DEFAULT_SCALE, device=None, hop: int = HOP_FRAME):
    """iq: uint8 tensor/array of interleaved bytes (I0,Q0,I1,Q1,...).  Returns float32 (n,2,128) on the device:
    row 0 = (I - 127.5)*scale, row 1 = (Q - 127.5)*scale; window i starts at pair i*hop (hop = 128: disjoint
    256-byte frames, a trailing partial frame is an error; smaller hops: overlapping windows, mdc_iq_u8_windows)."""
    import torch
    t = iq if isinstance(iq, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(iq, dtype=np.uint8)))
    if t.dtype != torch.uint8:
        raise TypeError(f"iq must be uint8, got {t.dtype}")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous().view(-1)
    if t.data_ptr() % 2:
        t = t.clone()       # a view starting at an odd byte of a larger buffer: the ABI wants whole (I,Q) pairs
    n = window_count(t.numel(), hop)
    x = torch.empty((n, 2, 128), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_u8_windows(t.data_ptr() if n else None, n, int(hop), float(scale), x.data_ptr() if n else None,
                                                  torch.cuda.current_stream(t.device).cuda_stream))
    return x


# ---- level-normalised windows (mdc_iq_u8_windows_norm): DC removal, fixed complex rms, per-window power ------------------
DEFAULT_LEVEL = 7.8e-3      # the complex rms of the bundled frames, and of RadioML2016.10a's energy-normalised vectors
FULL_SCALE_ENERGY = float((128 * 255) ** 2)      # E of a full-scale constant-envelope window: 0 dBFS


def _device_bytes(iq, device=None):
    import torch
    t = iq if isinstance(iq, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(iq, dtype=np.uint8)))
    if t.dtype != torch.uint8:
        raise TypeError(f"iq must be uint8, got {t.dtype}")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous().view(-1)
    if t.data_ptr() % 2:
        t = t.clone()       # a view starting at an odd byte of a larger buffer: the ABI wants whole (I,Q) pairs
    return t


def stats_tensor_to_numpy(stats):
    """The (n,4) int32 device tensor the calls below fill -> a numpy array of _cabi.IQ_WINDOW_STATS records."""
    return stats.cpu().numpy().view(_cabi.IQ_WINDOW_STATS).reshape(-1)


def normalized_frames_from_iq_u8(iq, level: float = DEFAULT_LEVEL, remove_dc: bool = True, hop: int = HOP_FRAME, device=None,
                                 return_stats: bool = False):
    """frames_from_iq_u8 with a scale per window: every window leaves with complex rms sqrt(mean(I^2 + Q^2)) == level, after
    removing each channel's mean if remove_dc (include/mdc.h, mdc_iq_u8_windows_norm).  A constant window becomes all zeros.
    Returns float32 (n,2,128) on the device; with return_stats also the windows' statistics as an (n,4) int32 device tensor
    (columns sum_i, sum_q, sum_sq, energy -- the last two are unsigned 32-bit values; stats_tensor_to_numpy names them)."""
    import torch
    t = _device_bytes(iq, device)
    n = window_count(t.numel(), hop)
    x = torch.empty((n, 2, 128), dtype=torch.float32, device=t.device)
    stats = torch.empty((n, 4), dtype=torch.int32, device=t.device) if return_stats else None
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_u8_windows_norm(t.data_ptr() if n else None, n, int(hop), float(level),
                                                       _cabi.IQ_REMOVE_DC if remove_dc else 0, x.data_ptr() if n else None,
                                                       stats.data_ptr() if return_stats and n else None,
                                                       torch.cuda.current_stream(t.device).cuda_stream))
    return (x, stats) if return_stats else x


def window_stats_iq_u8(iq, hop: int = HOP_FRAME, remove_dc: bool = True, device=None):
    """The statistics alone (no frames are written): a numpy array of _cabi.IQ_WINDOW_STATS records, one per window."""
    import torch
    t = _device_bytes(iq, device)
    n = window_count(t.numel(), hop)
    stats = torch.empty((n, 4), dtype=torch.int32, device=t.device)
    if n:
        with torch.cuda.device(t.device):
            _cabi.check(_cabi.lib().mdc_iq_u8_windows_norm(t.data_ptr(), n, int(hop), 1.0, _cabi.IQ_REMOVE_DC if remove_dc else 0, None,
                                                           stats.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream))
    return stats_tensor_to_numpy(stats)


def window_power_dbfs(stats) -> np.ndarray:
    """10*log10(E / (128*255)^2) per window: 0 dBFS is a full-scale constant-envelope window, -inf stands for E == 0.
    stats: IQ_WINDOW_STATS records, or an (n,4) integer array / tensor whose last column is the energy."""
    if hasattr(stats, "cpu"):
        stats = stats.cpu().numpy()
    a = np.asarray(stats)
    e = (a["energy"] if a.dtype.names else a[..., 3].astype(np.int64) & 0xFFFFFFFF).astype(np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(e / FULL_SCALE_ENERGY)


def squelch_energy_threshold(squelch_dbfs: float) -> int:
    """The smallest energy E whose window_power_dbfs is >= squelch_dbfs: `E < threshold` is the squelch test, in integers, and
    agrees with comparing the dBFS values themselves (the power is monotone in E; found by bisection on that very formula)."""
    sq = float(squelch_dbfs)
    if np.isnan(sq):
        raise ValueError("squelch_dbfs is NaN")
    lo, hi = 0, 1 << 31      # power(hi) is above every window's; the answer lies in [lo, hi]
    if not (10.0 * np.log10(hi / FULL_SCALE_ENERGY) >= sq):
        return hi
    while lo < hi:
        mid = (lo + hi) // 2
        with np.errstate(divide="ignore"):
            ok = 10.0 * np.log10(np.float64(mid) / FULL_SCALE_ENERGY) >= sq
        lo, hi = (lo, mid) if ok else (mid + 1, hi)
    return lo
