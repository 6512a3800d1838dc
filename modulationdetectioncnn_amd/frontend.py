"""Raw SDR samples -> frames (the RTL-SDR/HPS glue of the reference's README.md:5).

An RTL-SDR delivers unsigned 8-bit interleaved (I, Q) samples; a frame of the classifier is 128 such pairs
(256 bytes).  `frames_from_iq_u8` turns a device-resident byte buffer into the (n,2,128) float32 tensor every
`predict` entry point takes, on the device (mdc_iq_u8_to_frames), so the host never touches the samples.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _cabi

DEFAULT_SCALE = 1.0 / 127.5
HOP_FRAME = 128


def window_count(nbytes: int, hop: int = HOP_FRAME, pair_bytes: int = 2) -> int:
    """Windows of 128 (I,Q) pairs, `hop` pairs apart, that fit a capture of nbytes bytes (pair_bytes per pair: 2 for the 8-bit
    formats, 4 for 16-bit samples).  hop = 128 (disjoint frames) keeps the strict rule of the frame format: a trailing
    partial frame is an error."""
    if hop < 1:
        raise ValueError("hop must be >= 1 sample pair")
    frame = 128 * pair_bytes
    if hop == HOP_FRAME:
        if nbytes % frame:
            raise ValueError(f"{nbytes} bytes is not a whole number of {frame}-byte frames")
        return nbytes // frame
    if nbytes % pair_bytes:
        raise ValueError(f"{nbytes} bytes is not a whole number of (I,Q) pairs")
    pairs = nbytes // pair_bytes
    return 0 if pairs < 128 else (pairs - 128) // hop + 1


def frames_from_iq_u8(iq, scale: float = DEFAULT_SCALE, device=None, hop: int = HOP_FRAME):
    """iq: uint8 tensor/array of interleaved bytes (I0,Q0,I1,Q1,...).  Returns float32 (n,2,128) on the device:
    row 0 = (I - 127.5)*scale, row 1 = (Q - 127.5)*scale; window i starts at pair i*hop (hop = 128: disjoint
    256-byte frames, a trailing partial frame is an error; smaller hops: overlapping windows, mdc_iq_u8_windows)."""
    return _windows(_as_bytes(iq), _cabi.IQ_U8_ENTRIES, _cabi.IQ_CU8, hop, scale, None, True, False, device)[0]


# ---- level-normalised windows (mdc_iq_u8_windows_norm): DC removal, fixed complex rms, per-window power ------------------
DEFAULT_LEVEL = 7.8e-3      # the complex rms of the bundled frames, and of RadioML2016.10a's energy-normalised vectors
FULL_SCALE_ENERGY = float((128 * 255) ** 2)      # E of a full-scale constant-envelope window: 0 dBFS


def _as_bytes(iq):
    """what the _u8 names take: a uint8 tensor as it is, anything else (a list, a wider integer array) as numpy makes it uint8"""
    import torch
    return iq if isinstance(iq, torch.Tensor) else np.asarray(iq, dtype=np.uint8)


def stats_tensor_to_numpy(stats):
    """The (n,4) int32 device tensor the calls below fill -> a numpy array of _cabi.IQ_WINDOW_STATS records."""
    return stats.cpu().numpy().view(_cabi.IQ_WINDOW_STATS).reshape(-1)


def normalized_frames_from_iq_u8(iq, level: float = DEFAULT_LEVEL, remove_dc: bool = True, hop: int = HOP_FRAME, device=None,
                                 return_stats: bool = False):
    """frames_from_iq_u8 with a scale per window: every window leaves with complex rms sqrt(mean(I^2 + Q^2)) == level, after
    removing each channel's mean if remove_dc (include/mdc.h, mdc_iq_u8_windows_norm).  A constant window becomes all zeros.
    Returns float32 (n,2,128) on the device; with return_stats also the windows' statistics as an (n,4) int32 device tensor
    (columns sum_i, sum_q, sum_sq, energy -- the last two are unsigned 32-bit values; stats_tensor_to_numpy names them)."""
    flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
    x, stats = _windows(_as_bytes(iq), _cabi.IQ_U8_ENTRIES, _cabi.IQ_CU8, hop, level, flags, True, return_stats, device)
    return (x, stats) if return_stats else x


def window_stats_iq_u8(iq, hop: int = HOP_FRAME, remove_dc: bool = True, device=None):
    """The statistics alone (no frames are written): a numpy array of _cabi.IQ_WINDOW_STATS records, one per window."""
    flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
    return stats_tensor_to_numpy(_windows(_as_bytes(iq), _cabi.IQ_U8_ENTRIES, _cabi.IQ_CU8, hop, 1.0, flags, False, True, device)[1])


def window_power_dbfs(stats, sample_format="cu8") -> np.ndarray:
    """10*log10(E / (128*A)^2) per window (A: the format's full-scale amplitude, 255 for "cu8"): 0 dBFS is a full-scale
    constant-envelope window, -inf stands for E == 0.  stats: IQ_WINDOW_STATS / IQ_WINDOW_STATS64 records, or an (n,4) integer
    array / tensor whose last column is the energy (int32 columns hold the 32-bit record's unsigned values)."""
    if hasattr(stats, "cpu"):
        stats = stats.cpu().numpy()
    a = np.asarray(stats)
    if a.dtype.names:
        e = a["energy"].astype(np.float64)
    elif a.dtype.itemsize <= 4:
        e = (a[..., 3].astype(np.int64) & 0xFFFFFFFF).astype(np.float64)
    else:
        e = a[..., 3].astype(np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(e / full_scale_energy(sample_format))


def squelch_energy_threshold(squelch_dbfs: float, sample_format="cu8") -> int:
    """The smallest energy E whose window_power_dbfs is >= squelch_dbfs: `E < threshold` is the squelch test, in integers, and
    agrees with comparing the dBFS values themselves (the power is monotone in E; found by bisection on that very formula,
    over the format's energy range)."""
    sq = float(squelch_dbfs)
    if np.isnan(sq):
        raise ValueError("squelch_dbfs is NaN")
    fmt = sample_format_id(sample_format)
    full = full_scale_energy(fmt)
    lo, hi = 0, _ENERGY_CEILING[fmt]      # power(hi) is above every window's; the answer lies in [lo, hi]
    if not (10.0 * np.log10(hi / full) >= sq):
        return hi
    while lo < hi:
        mid = (lo + hi) // 2
        with np.errstate(divide="ignore"):
            ok = 10.0 * np.log10(np.float64(mid) / full) >= sq
        lo, hi = (lo, mid) if ok else (mid + 1, hi)
    return lo


# ---- any integer sample format (mdc_iq_windows / mdc_iq_windows_norm): unsigned 8-bit, signed 8-bit, signed 16-bit LE ------
SAMPLE_FORMATS = {"cu8": _cabi.IQ_CU8, "ci8": _cabi.IQ_CI8, "ci16": _cabi.IQ_CI16, "ci16_le": _cabi.IQ_CI16,
                  "u8": _cabi.IQ_CU8, "i8": _cabi.IQ_CI8, "sc8": _cabi.IQ_CI8, "sc16": _cabi.IQ_CI16, "i16": _cabi.IQ_CI16}
FULL_SCALE_AMPLITUDE = {_cabi.IQ_CU8: 255, _cabi.IQ_CI8: 128, _cabi.IQ_CI16: 32768}
DEFAULT_SCALES = {_cabi.IQ_CU8: DEFAULT_SCALE, _cabi.IQ_CI8: 1.0 / 128.0, _cabi.IQ_CI16: 1.0 / 32768.0}
_ENERGY_CEILING = {_cabi.IQ_CU8: 1 << 31, _cabi.IQ_CI8: 1 << 30, _cabi.IQ_CI16: 1 << 46}      # above 128 * max(sum_sq) of the format


def sample_format_id(sample_format) -> int:
    """"cu8" / "ci8" / "ci16" (SigMF's "ci16_le", UHD's "sc16", ... are aliases), or an MDC_IQ_* value -> the MDC_IQ_* value."""
    if isinstance(sample_format, str):
        key = sample_format.lower()
        if key not in SAMPLE_FORMATS:
            raise ValueError(f"sample_format must be one of 'cu8', 'ci8', 'ci16' (got {sample_format!r})")
        return SAMPLE_FORMATS[key]
    if sample_format in FULL_SCALE_AMPLITUDE:
        return int(sample_format)
    raise ValueError(f"unknown sample format {sample_format!r}")


def full_scale_energy(sample_format) -> float:
    """E of a full-scale constant-envelope window: (128*A)^2, the 0 dBFS reference of the format."""
    return float((128 * FULL_SCALE_AMPLITUDE[sample_format_id(sample_format)]) ** 2)


def host_samples(iq, fmt: int) -> np.ndarray:
    """A numpy capture, flat interleaved or (..., 2), as a flat contiguous array of the format's dtype.  Only the byte order
    is ever converted (big-endian int16 -> '<i2'); any other dtype is a TypeError."""
    a = np.asarray(iq)
    want = _cabi.IQ_SAMPLE_DTYPE[fmt]
    if a.dtype.kind != want.kind or a.dtype.itemsize != want.itemsize:
        raise TypeError(f"iq must be {want.name} for this sample format, got {a.dtype}")
    return np.ascontiguousarray(a.astype(want, copy=False)).reshape(-1)


def _device_samples(iq, fmt: int, device=None):
    import torch
    want = {_cabi.IQ_CU8: torch.uint8, _cabi.IQ_CI8: torch.int8, _cabi.IQ_CI16: torch.int16}[fmt]
    t = iq if isinstance(iq, torch.Tensor) else torch.from_numpy(host_samples(iq, fmt))
    if t.dtype != want:
        raise TypeError(f"iq must be {want} for this sample format, got {t.dtype}")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous().view(-1)
    if t.data_ptr() % _cabi.IQ_PAIR_BYTES[fmt]:
        t = t.clone()       # a view starting inside a pair of a larger buffer: the ABI wants whole (I,Q) pairs
    return t


def _pair_count(t, fmt: int) -> int:
    """(I,Q) pairs of the flat device capture t"""
    nbytes = t.numel() * t.element_size()
    if nbytes % _cabi.IQ_PAIR_BYTES[fmt]:
        raise ValueError("the capture is not a whole number of (I,Q) pairs")
    return nbytes // _cabi.IQ_PAIR_BYTES[fmt]


def _windows(iq, entries, fmt: int, hop, gain, flags, want_frames: bool, want_stats: bool, device):
    """The six functions of this file that cut a capture into windows: (frames or None, statistics or None) through one row of
    _cabi's entry table.  flags None: the plain entry, gain is the scale; else the normalising one, gain is the level.  The
    statistics are the (n,4) device tensor of the row's record, int32 or int64 columns."""
    import torch
    t = _device_samples(iq, fmt, device)
    n = window_count(t.numel() * t.element_size(), hop, _cabi.IQ_PAIR_BYTES[fmt])
    x = torch.empty((n, 2, 128), dtype=torch.float32, device=t.device) if want_frames else None
    stats = torch.empty((n, 4), dtype=torch.int32 if entries.stats.itemsize == 16 else torch.int64, device=t.device) if want_stats else None
    head = (t.data_ptr() if n else None,) + ((fmt,) if entries.takes_format else ())
    if n or want_frames:      # (the statistics alone of no window: nothing is asked of the library)
        with torch.cuda.device(t.device):
            stream = torch.cuda.current_stream(t.device).cuda_stream
            if flags is None:
                _cabi.check(getattr(_cabi.lib(), entries.frames)(*head, n, int(hop), float(gain), x.data_ptr() if n else None, stream))
            else:
                _cabi.check(getattr(_cabi.lib(), entries.frames_norm)(*head, n, int(hop), float(gain), flags, x.data_ptr() if want_frames and n else None,
                                                                      stats.data_ptr() if want_stats and n else None, stream))
    return x, stats


def stats64_tensor_to_numpy(stats):
    """The (n,4) int64 device tensor the calls below fill -> a numpy array of _cabi.IQ_WINDOW_STATS64 records."""
    return stats.cpu().numpy().view(_cabi.IQ_WINDOW_STATS64).reshape(-1)


def frames_from_iq(iq, sample_format, scale=None, device=None, hop: int = HOP_FRAME):
    """frames_from_iq_u8 for any sample format: iq holds interleaved samples of the format's dtype (uint8 / int8 / int16).
    Returns float32 (n,2,128) on the device, sample * scale ("cu8": (byte - 127.5) * scale); default scale 1/127.5, 1/128,
    1/32768 (mdc_iq_windows)."""
    fmt = sample_format_id(sample_format)
    return _windows(iq, _cabi.IQ_ENTRIES, fmt, hop, DEFAULT_SCALES[fmt] if scale is None else scale, None, True, False, device)[0]


def normalized_frames_from_iq(iq, sample_format, level: float = DEFAULT_LEVEL, remove_dc: bool = True, hop: int = HOP_FRAME, device=None,
                              return_stats: bool = False):
    """normalized_frames_from_iq_u8 for any sample format (mdc_iq_windows_norm).  With return_stats also the windows' statistics
    as an (n,4) int64 device tensor (columns sum_i, sum_q, sum_sq, energy; stats64_tensor_to_numpy names them)."""
    flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
    x, stats = _windows(iq, _cabi.IQ_ENTRIES, sample_format_id(sample_format), hop, level, flags, True, return_stats, device)
    return (x, stats) if return_stats else x


def window_stats_iq(iq, sample_format, hop: int = HOP_FRAME, remove_dc: bool = True, device=None):
    """The statistics alone (no frames are written): a numpy array of _cabi.IQ_WINDOW_STATS64 records, one per window."""
    flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
    return stats64_tensor_to_numpy(_windows(iq, _cabi.IQ_ENTRIES, sample_format_id(sample_format), hop, 1.0, flags, False, True, device)[1])


# ---- float captures (mdc_iq_cf32_histogram / mdc_iq_cf32_quantize): complex float32 -> an ordinary "ci16" stream, once, at the door ----
def _device_cf32(iq, device=None):
    """A complex float32 capture -- complex64 (n,), float32 (2n,) interleaved or float32 (n, 2); numpy or torch, host or device --
    as a flat float32 device tensor I0 Q0 I1 Q1 ... starting on a whole pair.  Big-endian numpy input is byte-swapped on the host
    (as host_samples does); any other dtype is a TypeError, any other shape a ValueError."""
    import torch
    if isinstance(iq, torch.Tensor):
        t = iq
        if t.dtype not in (torch.complex64, torch.float32):
            raise TypeError(f"a cf32 capture must be complex64 or float32, got {t.dtype}")
    else:
        a = np.asarray(iq)
        if not ((a.dtype.kind == "c" and a.dtype.itemsize == 8) or (a.dtype.kind == "f" and a.dtype.itemsize == 4)):
            raise TypeError(f"a cf32 capture must be complex64 or float32, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(a.dtype.newbyteorder("<"), copy=False)))
    if t.dtype == torch.complex64:
        if t.dim() != 1:
            raise ValueError(f"a complex64 capture must have shape (n,), got {tuple(t.shape)}")
    elif not ((t.dim() == 1 and t.numel() % 2 == 0) or (t.dim() == 2 and t.shape[1] == 2)):
        raise ValueError(f"a float32 capture must have shape (2n,) or (n, 2), got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous()
    t = (torch.view_as_real(t) if t.dtype == torch.complex64 else t).reshape(-1)
    if t.data_ptr() % 8:
        t = t.clone()       # a view starting inside a pair of a larger buffer: the ABI wants whole (I,Q) pairs
    return t


def _cf32_histogram_into(t, hist):
    """mdc_iq_cf32_histogram of the flat float32 device tensor t, added into the uint64[256] device tensor hist"""
    import torch
    pairs = t.numel() // 2
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_cf32_histogram(t.data_ptr() if pairs else None, pairs, hist.data_ptr(),
                                                      torch.cuda.current_stream(t.device).cuda_stream))
    return hist


def cf32_histogram(iq, hist=None, device=None):
    """The exact statistics of a complex float32 capture (mdc_iq_cf32_histogram, include/mdc.h): the uint64[256] device tensor
    of how many components carry each biased exponent byte -- bin 0 zeros and denormals, bin e the normal numbers with
    2^(e-127) <= |x| < 2^(e-126), bin 255 NaN and +-Inf.  iq: complex64 (n,), float32 (2n,) or (n, 2), numpy or torch.  hist: a
    tensor an earlier call returned; this capture's counts are ADDED to it (a file read in chunks) and it is returned.  Integer
    counts: bit-identical on every run.  Enqueues on torch's current stream without synchronising."""
    import torch
    t = _device_cf32(iq, device)
    if hist is None:
        hist = torch.zeros(256, dtype=torch.int64, device=t.device).view(torch.uint64)
    elif not (isinstance(hist, torch.Tensor) and hist.dtype == torch.uint64 and hist.shape == (256,) and hist.is_contiguous()
              and hist.device == t.device):
        raise ValueError("hist must be the contiguous uint64[256] tensor of an earlier call, on the capture's device")
    return _cf32_histogram_into(t, hist)


def _host_histogram(hist) -> np.ndarray:
    h = hist.cpu().numpy() if hasattr(hist, "cpu") else np.asarray(hist)
    if h.dtype.kind not in "iu" or h.shape != (256,):
        raise ValueError("hist must hold 256 integer counts")
    return h.astype(np.uint64, copy=False)


def design_cf32_gain(hist, clip_fraction: float = 0.0) -> float:
    """The power-of-two gain of quantize_cf32 from a capture's exponent histogram (cf32_histogram's tensor, or 256 integers).
    Walk down from bin 254 while the components in the bins above stay within floor(clip_fraction * finite components): the
    bin the walk stops at is the top kept bin e -- with clip_fraction 0 the highest occupied one -- and every kept component
    has |x| < 2^(e-126).  gain = 2^clamp(140 - e, -126, 125): every kept component then has |x * gain| < 2^14, so nothing kept
    can clip and the largest kept ones use 13 to 14 bits (the clamp keeps the gain inside mdc_iq_cf32_quantize's range; only its
    upper end can bind, for a capture whose top bin is below 15: |x| < 2^-111).  clip_fraction > 0 gives up that share of the components to a few glitch
    samples, which then clip (and are counted) instead of costing everyone else their resolution.  No normal component at all
    (an empty, all-zero or denormal-only capture): 1.0."""
    p = float(clip_fraction)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"clip_fraction must be in [0, 1) (got {clip_fraction!r})")
    h = [int(v) for v in _host_histogram(hist)]
    budget = int(p * sum(h[:255]))      # floor: both factors are non-negative
    above, e = 0, 254
    while e >= 1 and above + h[e] <= budget:
        above += h[e]
        e -= 1
    if e < 1:
        return 1.0
    return float(2.0 ** min(max(140 - e, -126), 125))


def quantize_cf32(iq, full_scale=None, clip_fraction: float = 0.0, nonfinite: str = "zero", device=None, return_report: bool = False):
    """A complex float32 capture (GNU Radio's file sink, UHD's fc32, SigMF's cf32_le) as an ordinary "ci16" capture: the flat
    int16 device tensor I0 Q0 I1 Q1 ... of mdc_iq_cf32_quantize (include/mdc.h) -- per component ONE correctly rounded
    multiplication by the gain, ONE rounding to nearest (ties to even), saturation to -32768 .. 32767.  iq: complex64 (n,),
    float32 (2n,) or (n, 2); numpy or torch, host or device.
    full_scale: the float amplitude that becomes 32768 (UHD and GNU Radio write +-1.0 as ADC full scale): gain =
    float32(32768 / full_scale).  None measures instead: cf32_histogram, then design_cf32_gain(hist, clip_fraction) -- a power of
    two, so the multiplication is exact, with the capture's peak in [2^13, 2^14).
    nonfinite: a pair with a NaN or +-Inf component becomes (0, 0) and is counted ("zero"), or the call raises
    NonFiniteInputError with the number of such components, taken from the histogram's bin 255 before anything is written
    ("raise": one extra histogram pass when full_scale is given).
    return_report=True returns (tensor, report): gain, full_scale = 32768 / gain (the float amplitude that 0 dBFS of every
    later record refers to), nonfinite_pairs, clipped (components that saturated) and pairs.  The report, the measurement and
    nonfinite="raise" read counts back and synchronise; with a given full_scale and neither of the others the call only
    enqueues on torch's current stream."""
    import torch
    if nonfinite not in ("zero", "raise"):
        raise ValueError(f"nonfinite must be 'zero' or 'raise'; got {nonfinite!r}")
    if not 0.0 <= float(clip_fraction) < 1.0:
        raise ValueError(f"clip_fraction must be in [0, 1) (got {clip_fraction!r})")
    if full_scale is not None:
        fs = float(full_scale)
        # (a NaN fails every comparison; the range's ends are float32 values, so rounding to float32 cannot leave it)
        if not (0.0 < fs < float("inf") and _cabi.CF32_MIN_GAIN <= 32768.0 / fs <= _cabi.CF32_MAX_GAIN):
            raise ValueError(f"full_scale must be a positive float with 32768 / full_scale in 2^-126 .. 2^125 (got {full_scale!r})")
        gain = float(np.float32(32768.0 / fs))
    t = _device_cf32(iq, device)
    pairs = t.numel() // 2
    if full_scale is None or nonfinite == "raise":
        hist = _cf32_histogram_into(t, torch.zeros(256, dtype=torch.int64, device=t.device).view(torch.uint64)).cpu().numpy()
        if nonfinite == "raise" and int(hist[255]):
            from .model import NonFiniteInputError
            raise NonFiniteInputError([], count=int(hist[255]),
                                      message=f"{int(hist[255])} component(s) of the cf32 capture are NaN or +-Inf")
        if full_scale is None:
            gain = design_cf32_gain(hist, clip_fraction)
    out = torch.empty(2 * pairs, dtype=torch.int16, device=t.device)
    counts = torch.zeros(2, dtype=torch.int64, device=t.device) if return_report else None
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_cf32_quantize(t.data_ptr() if pairs else None, pairs, gain, out.data_ptr() if pairs else None,
                                                     counts.data_ptr() if counts is not None else None,
                                                     torch.cuda.current_stream(t.device).cuda_stream))
    if not return_report:
        return out
    c = counts.cpu().numpy()
    return out, dict(gain=gain, full_scale=32768.0 / gain, nonfinite_pairs=int(c[0]), clipped=int(c[1]), pairs=pairs)


# ---- I/Q balance (mdc_iq_balance_stats / mdc_iq_balance): gain / phase imbalance and DC offset -- exact integers, on the device ----
class BalanceCoeffs(NamedTuple):
    """The six integers of mdc_iq_balance (include/mdc.h): the DC offsets in widened units and the Q14 matrix.  scale is what
    design_balance multiplied the matrix by to keep a row's |m_i0| + |m_i1| <= 32767 (1.0: nothing; it is no argument of the
    correction)."""
    dc_i: int
    dc_q: int
    m00: int
    m01: int
    m10: int
    m11: int
    scale: float = 1.0


BALANCE_IDENTITY = BalanceCoeffs(0, 0, _cabi.BALANCE_ONE, 0, 0, _cabi.BALANCE_ONE)
BALANCE_SWAP = BalanceCoeffs(0, 0, 0, _cabi.BALANCE_ONE, _cabi.BALANCE_ONE, 0)            # I <-> Q: spectrum inversion of a wrongly wired capture
BALANCE_CONJUGATE = BalanceCoeffs(0, 0, _cabi.BALANCE_ONE, 0, 0, -_cabi.BALANCE_ONE)      # Q -> -Q (-32768 clamps to 32767)


def balance_blocks(pairs_in: int, block_pairs: int = 65536) -> int:
    """mdc_iq_balance_blocks: ceil(pairs_in / block_pairs), the rows of balance_stats (needs no GPU)."""
    return _cabi.check(_cabi.lib().mdc_iq_balance_blocks(int(pairs_in), int(block_pairs)))


def balance_stats(iq, sample_format, block_pairs: int = 65536, device=None):
    """The capture's exact second-order statistics per block of block_pairs pairs (mdc_iq_balance_stats, include/mdc.h): the
    (nblocks, 5) int64 device tensor of sum x, sum y, sum x^2, sum y^2, sum x y over each block's widened samples.  The tensor
    carries the capture's pair count and the block size as attributes `pairs` and `block_pairs` for design_balance and
    image_rejection_db (a slice or copy of it does not: pass pairs= there).  Enqueues on torch's current stream without
    synchronising."""
    import torch
    fmt = sample_format_id(sample_format)
    t = _device_samples(iq, fmt, device)
    pairs, B = _pair_count(t, fmt), int(block_pairs)
    L = _cabi.lib()
    nblocks = _cabi.check(L.mdc_iq_balance_blocks(pairs, B))
    sums = torch.empty((nblocks, 5), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(L.mdc_iq_balance_stats(t.data_ptr() if pairs else None, fmt, pairs, B, sums.data_ptr() if nblocks else None, nblocks,
                                           torch.cuda.current_stream(t.device).cuda_stream))
    sums.pairs, sums.block_pairs = pairs, B
    return sums


def _total_sums(sums, pairs):
    """(n, Sx, Sy, Sxx, Syy, Sxy) as Python integers from balance_stats' tensor, a numpy array of block rows or one summed row"""
    if pairs is None:
        pairs = getattr(sums, "pairs", None)
    if pairs is None:
        raise ValueError("pairs= is needed: only the tensor balance_stats returned knows how many pairs its sums cover")
    rows = sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums)
    if rows.dtype.kind not in "iu" and rows.dtype != object:
        raise TypeError(f"the sums must be integers (got {rows.dtype})")
    rows = rows.reshape(-1, 5)
    return (int(pairs),) + tuple(sum(int(v) for v in rows[:, k]) for k in range(5))


def _central_moments(sums, pairs):
    """n and the exact integers n^2 times the (co)variances: cxx = n Sxx - Sx^2, cyy, cxy = n Sxy - Sx Sy"""
    n, Sx, Sy, Sxx, Syy, Sxy = _total_sums(sums, pairs)
    return n, Sx, Sy, n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy


def design_balance(sums, pairs=None) -> BalanceCoeffs:
    """The coefficients of mdc_iq_balance from a capture's statistics (include/mdc.h, "design").  sums: balance_stats' tensor
    (it knows its pair count), or a numpy array of block rows or one summed row (sum x, sum y, sum x^2, sum y^2, sum x y) with
    pairs= the number of pairs they cover -- a caller who leaves blocks out passes the rows kept and their pairs.  dc = (2 S + n)
    // (2 n): the mean, round half up, exact.  M = sqrt(tr C / 2) C^(-1/2) in float64 from the exact integer central moments --
    the symmetric whitening matrix: it equalises the rails, makes them orthogonal, keeps the total power and does not rotate --,
    m_ij = rint(16384 M_ij).  If a row's |m_i0| + |m_i1| exceeds 32767 (an imbalance near 6 dB: no real receiver) M is scaled
    down until both rows hold, and the result's `scale` says by how much.  No pairs, or a capture without variance on a rail or
    with fully correlated rails (nothing to estimate): the identity matrix, the DC alone.  The estimate is blind: it takes the
    capture as a whole to be proper (include/mdc.h says when that fails)."""
    import math
    n, Sx, Sy, cxx, cyy, cxy = _central_moments(sums, pairs)
    if n <= 0:
        return BALANCE_IDENTITY
    dc_i, dc_q = (2 * Sx + n) // (2 * n), (2 * Sy + n) // (2 * n)
    det = cxx * cyy - cxy * cxy
    if cxx <= 0 or cyy <= 0 or det <= 0:
        return BALANCE_IDENTITY._replace(dc_i=dc_i, dc_q=dc_q)
    n2 = float(n) * float(n)
    a, b, d = cxx / n2, cxy / n2, cyy / n2
    s = math.sqrt(a * d - b * b) if a * d - b * b > 0.0 else math.sqrt(det) / n2
    # C^(1/2) = (C + s I) / t, t = sqrt(tr C + 2 s), s = sqrt(det C) (Cayley-Hamilton for 2 x 2); its inverse, times sqrt(tr C / 2)
    t = math.sqrt(a + d + 2.0 * s)
    g = math.sqrt((a + d) / 2.0) * t / ((a + s) * (d + s) - b * b)
    M = (g * (d + s), -g * b, -g * b, g * (a + s))
    scale = 1.0
    while True:
        m = [int(np.rint(_cabi.BALANCE_ONE * scale * v)) for v in M]
        worst = max(abs(m[0]) + abs(m[1]), abs(m[2]) + abs(m[3]))
        if worst <= _cabi.BALANCE_MAX_ROW_ABS_SUM:
            return BalanceCoeffs(dc_i, dc_q, *m, scale=scale)
        scale *= (_cabi.BALANCE_MAX_ROW_ABS_SUM - 0.5) / worst


def image_rejection_db(sums, pairs=None) -> float:
    """The capture's own image rejection ratio in dB from its statistics (sums, pairs: as design_balance), before any
    correction: with the exact integer central moments cxx, cyy, cxy, rho = hypot(cxx - cyy, 2 cxy) / (cxx + cyy) = |E[z^2]| /
    E[|z|^2], r = (1 - sqrt(1 - rho^2)) / rho the image's amplitude relative to the signal's, IRR = -20 log10 r; inf when rho
    is 0 (or there is nothing to measure).  1 dB and 5 degrees give 22.83 dB.  On a balanced capture the estimate's own noise
    ends it near 90 dB for 2^18 pairs."""
    import math
    n, _, _, cxx, cyy, cxy = _central_moments(sums, pairs)
    if n <= 0 or cxx + cyy <= 0:
        return math.inf
    num2 = (cxx - cyy) ** 2 + 4 * cxy * cxy      # exact
    if num2 == 0:
        return math.inf
    rho = min(math.sqrt(num2) / (cxx + cyy), 1.0)
    r = (1.0 - math.sqrt(1.0 - rho * rho)) / rho
    if r <= 0.0:      # rho below float64's resolution of 1 - rho^2: r = rho / 2 to first order
        r = rho / 2.0
    return -20.0 * math.log10(r)


def _balance_record(coeffs):
    """The six integers of `coeffs` (a BalanceCoeffs, or any sequence of at least six integers) as the 24-byte record"""
    c = tuple(coeffs)[:6]
    if len(c) != 6:
        raise ValueError("coeffs must hold dc_i, dc_q, m00, m01, m10, m11")
    rec = np.zeros((), _cabi.IQ_BALANCE_COEFFS)
    for name, v in zip(_cabi.IQ_BALANCE_COEFFS.names, c):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"coeffs.{name} must be a 32-bit integer (got {v!r})")
        rec[name] = int(v)
    return rec


def balance(iq, sample_format, coeffs=None, block_pairs: int = 65536, device=None, return_coeffs: bool = False):
    """Remove a capture's DC offset and I/Q imbalance on the device (mdc_iq_balance, include/mdc.h: exact integer arithmetic).
    Returns the (n, 2) int16 device tensor of corrected pairs: an ordinary "ci16" capture for every other function here.
    coeffs=None estimates from this capture -- one balance_stats launch, one transfer of 40 bytes per block, design_balance,
    one correction launch; passing a BalanceCoeffs (or any six integers dc_i, dc_q, m00, m01, m10, m11) skips the first two:
    the normal use for a receiver calibrated once per tuning and gain.  BALANCE_SWAP exchanges I and Q, BALANCE_CONJUGATE
    negates Q; BALANCE_IDENTITY only widens.  return_coeffs=True returns (tensor, the BalanceCoeffs applied, the capture's
    image_rejection_db before correction -- None when coefficients were passed).  With given coefficients the call enqueues on
    torch's current stream without synchronising."""
    import torch
    fmt = sample_format_id(sample_format)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    irr = None
    if coeffs is None:
        sums = balance_stats(t, fmt, block_pairs)
        host = sums.cpu().numpy()
        coeffs, irr = design_balance(host, pairs), image_rejection_db(host, pairs)
    elif not isinstance(coeffs, BalanceCoeffs):
        coeffs = BalanceCoeffs(*(int(v) for v in tuple(coeffs)[:6]))
    rec = _balance_record(coeffs)
    out = torch.empty((pairs, 2), dtype=torch.int16, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_balance(t.data_ptr() if pairs else None, fmt, pairs, rec.ctypes.data, out.data_ptr() if pairs else None,
                                               torch.cuda.current_stream(t.device).cuda_stream))
    return (out, coeffs, irr) if return_coeffs else out


def balanced_capture(iq, sample_format, balance_arg, device=None):
    """The `balance=` keyword of predict_iq / scan_iq / detect_iq / predict_channels: (capture, format id, image_rejection_db or
    None).  balance_arg True: estimated from the capture; a coefficients tuple: applied as given.  The capture comes back flat,
    as "ci16", on the device."""
    out, _, irr = balance(iq, sample_format, None if balance_arg is True else balance_arg, device=device, return_coeffs=True)
    return out.view(-1), _cabi.IQ_CI16, irr


# ---- digital down-converter (mdc_iq_ddc): frequency shift, low-pass, decimate -- exact integers, on the device -------------
def phase_step(shift: float) -> int:
    """shift: the frequency ADDED to every component of the capture, in cycles per input sample, in [-0.5, 0.5] (a signal at
    +f0 comes to 0 with shift = -f0).  Returns the oscillator's 32-bit step, round(shift * 2^32) mod 2^32."""
    shift = float(shift)
    if not -0.5 <= shift <= 0.5:
        raise ValueError(f"shift must lie in [-0.5, 0.5] cycles per sample (got {shift!r})")
    return int(round(shift * 2.0 ** 32)) % (1 << 32)


def design_lowpass(decimate: int, ntaps=None, cutoff=None, beta: float = 8.0) -> np.ndarray:
    """The anti-alias filter in front of a decimation by `decimate` >= 2, as int16 Q15 taps for mdc_iq_ddc: a Kaiser-windowed
    sinc of ntaps taps (default 8 * decimate) whose -6 dB point lies at `cutoff` cycles per input sample (default 0.4 / decimate),
    normalised to unit sum, rounded to Q15, the centre tap(s) then adjusted so that the taps sum to exactly 32768 (DC gain 1;
    the taps stay symmetric).  With the defaults, for decimate in {2, 3, 4, 8, 12, 16, 32, 64}: sum |h| <= 40,712 (mdc_iq_ddc
    wants <= 65,535), droop <= 0.95 dB over |f| <= 0.25 / decimate, and >= 63 dB attenuation for |f| >= 0.75 / decimate --
    everything that aliases onto |f| <= 0.25 / decimate.  (A signal of 8 samples per symbol AFTER decimation with a root
    raised cosine pulse occupies |f| <= 0.085 / decimate.)  Group delay: (ntaps - 1) / 2 input samples."""
    D = int(decimate)
    if D < 2:
        raise ValueError("design_lowpass needs decimate >= 2 (a decimation by 1 has nothing to reject: pass explicit taps)")
    T = 8 * D if ntaps is None else int(ntaps)
    if not 1 <= T <= _cabi.DDC_MAX_TAPS:
        raise ValueError(f"ntaps must be in 1..{_cabi.DDC_MAX_TAPS} (got {T})")
    fc = 0.4 / D if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError(f"cutoff must lie in (0, 0.5] cycles per sample (got {fc!r})")
    k = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(T, float(beta))
    q = np.rint(h / h.sum() * 32768.0).astype(np.int64)
    rest = 32768 - int(q.sum())
    if T % 2:
        q[T // 2] += rest
    else:      # symmetric taps of even length sum to an even number: both centre taps take half of what is missing
        q[T // 2 - 1] += rest // 2
        q[T // 2] += rest - rest // 2
    if np.abs(q).max() > 32767 or int(np.abs(q).sum()) > _cabi.DDC_MAX_TAPS_ABS_SUM:
        raise ValueError("these parameters give taps outside int16 Q15 / the sum |h| <= 65535 of mdc_iq_ddc")
    return q.astype(np.int16)


def ddc_out_count(pairs_in: int, ntaps: int, decimate: int) -> int:
    """mdc_iq_ddc_out_count: output pairs of a capture of pairs_in pairs (a "valid" convolution)."""
    return _cabi.check(_cabi.lib().mdc_iq_ddc_out_count(int(pairs_in), int(ntaps), int(decimate)))


def nco_table() -> np.ndarray:
    """The (4096, 2) int16 (cos, sin) table the device oscillator uses (mdc_iq_ddc_nco_table; needs no GPU)."""
    t = np.empty((_cabi.DDC_NCO_ENTRIES, 2), np.int16)
    _cabi.check(_cabi.lib().mdc_iq_ddc_nco_table(t.ctypes.data))
    return t


def _int16_taps(taps) -> np.ndarray:
    h = np.asarray(taps)
    if h.dtype.kind != "i" or h.ndim != 1:
        raise TypeError("taps must be a one-dimensional integer array (int16)")
    if h.size and (h.min() < -32768 or h.max() > 32767):
        raise ValueError("taps must fit int16")
    return np.ascontiguousarray(h.astype(np.int16))


def ddc(iq, sample_format, shift: float = 0.0, decimate: int = 1, taps=None, phase0: int = 0, device=None):
    """Tune, low-pass and decimate a capture on the device (mdc_iq_ddc, include/mdc.h: exact integer arithmetic).  iq: as
    frames_from_iq; shift: the frequency added to the capture, cycles per input sample (phase_step); taps: int16 Q15, applied as
    written, None = design_lowpass(decimate) -- decimate == 1 needs explicit taps; phase0: the oscillator's 32-bit phase at the
    capture's first pair.  Returns the (n_out, 2) int16 device tensor of (I, Q) pairs, n_out = (pairs - ntaps) // decimate + 1: an
    ordinary "ci16" capture for frames_from_iq / normalized_frames_from_iq / VTCNN2.predict_iq.  Enqueues on torch's current
    stream without synchronising."""
    import torch
    fmt = sample_format_id(sample_format)
    D, step = int(decimate), phase_step(shift)
    if taps is None:
        if D == 1:
            raise ValueError("decimate == 1 needs explicit taps (design_lowpass designs anti-alias filters for decimate >= 2)")
        taps = design_lowpass(D)
    h = _int16_taps(taps)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    L = _cabi.lib()
    n_out = _cabi.check(L.mdc_iq_ddc_out_count(pairs, h.size, D))
    out = torch.empty((n_out, 2), dtype=torch.int16, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(L.mdc_iq_ddc(t.data_ptr() if pairs else None, fmt, pairs, int(phase0) % (1 << 32), step, D, h.ctypes.data, h.size,
                                 out.data_ptr() if n_out else None, n_out, torch.cuda.current_stream(t.device).cuda_stream))
    return out


# ---- rational resampler (mdc_iq_resample): frequency shift, low-pass, resample by L/D -- exact integers, on the device ------
def resample_out_count(pairs_in: int, ntaps: int, interpolate: int, decimate: int) -> int:
    """mdc_iq_resample_out_count: output pairs of a capture of pairs_in pairs, ((pairs_in - 1) L + 1 - ntaps) // D + 1 or 0."""
    return _cabi.check(_cabi.lib().mdc_iq_resample_out_count(int(pairs_in), int(ntaps), int(interpolate), int(decimate)))


def _check_resample_factors(interpolate, decimate):
    L, D = int(interpolate), int(decimate)
    if not 1 <= L <= _cabi.RESAMPLE_MAX_INTERPOLATE:
        raise ValueError(f"interpolate must be in 1..{_cabi.RESAMPLE_MAX_INTERPOLATE} (got {L})")
    if not 1 <= D <= _cabi.RESAMPLE_MAX_DECIMATE:
        raise ValueError(f"decimate must be in 1..{_cabi.RESAMPLE_MAX_DECIMATE} (got {D})")
    return L, D


def design_resampler(interpolate: int, decimate: int, ntaps=None, cutoff=None, beta: float = 8.0) -> np.ndarray:
    """The prototype low-pass of a resampling by interpolate / decimate = L / D, as int16 taps for mdc_iq_resample: a Kaiser-windowed
    sinc at the INTERPOLATED rate of ntaps taps (default 8 M, M = max(L, D); beyond 1024 taps ntaps must be given) whose -6 dB
    point lies at `cutoff` cycles per interpolated sample (default 0.4 / M), scaled to sum 32768 L and rounded; then, in each of
    the L polyphase branches h[r::L], what is missing to 32768 goes to the branch's largest tap, so that EVERY branch has DC gain
    exactly 1 (no output phase is louder than its neighbour at DC; the prototype's symmetry may be off by those few LSB).  With
    the defaults: droop <= 0.95 dB over |f| <= 0.25 / M, >= 63 dB attenuation for |f| >= 0.75 / M -- design_lowpass's figures, at
    the interpolated rate -- and every branch's sum |h| far below the 65,535 mdc_iq_resample wants.  L == 1 returns
    design_lowpass(D, ntaps, cutoff, beta) unchanged.  Group delay: (ntaps - 1) / 2 interpolated samples."""
    L, D = _check_resample_factors(interpolate, decimate)
    if L == 1:
        return design_lowpass(D, ntaps, cutoff, beta)
    M = max(L, D)
    if ntaps is None:
        T = 8 * M
        if T > _cabi.RESAMPLE_MAX_TAPS:
            raise ValueError(f"the default of 8 * max(L, D) = {T} taps exceeds {_cabi.RESAMPLE_MAX_TAPS}: pass ntaps explicitly")
    else:
        T = int(ntaps)
    if not 1 <= T <= _cabi.RESAMPLE_MAX_TAPS:
        raise ValueError(f"ntaps must be in 1..{_cabi.RESAMPLE_MAX_TAPS} (got {T})")
    fc = 0.4 / M if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError(f"cutoff must lie in (0, 0.5] cycles per interpolated sample (got {fc!r})")
    k = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(T, float(beta))
    q = np.rint(h / h.sum() * (32768.0 * L)).astype(np.int64)
    for r in range(min(L, T)):
        branch = q[r::L]                                    # a view: the correction lands in q
        branch[int(np.argmax(branch))] += 32768 - int(branch.sum())
    if q.min() < -32768 or q.max() > 32767 or max(int(np.abs(q[r::L]).sum()) for r in range(min(L, T))) > _cabi.RESAMPLE_MAX_BRANCH_ABS_SUM:
        raise ValueError("these parameters give taps outside int16 / a branch beyond the sum |h| <= 65535 of mdc_iq_resample")
    return q.astype(np.int16)


def _closest_ratio(target, Lmax: int, Dmax: int):
    """(|L/D - target|, L/D) as Fractions: the rational with L <= Lmax, D <= Dmax closest to target > 0 (ties: the smaller L)."""
    from fractions import Fraction
    best = None
    for L in range(1, Lmax + 1):
        d = Fraction(L) / target
        for D in {max(1, min(Dmax, d.__floor__())), max(1, min(Dmax, d.__ceil__()))}:
            err = abs(Fraction(L, D) - target)
            if best is None or err < best[0]:
                best = (err, Fraction(L, D))
    return best


def resample_ratio(rate: float, symbol_rate: float, samples_per_symbol: float = 8, max_interpolate: int = _cabi.RESAMPLE_MAX_INTERPOLATE,
                   max_decimate: int = _cabi.RESAMPLE_MAX_DECIMATE):
    """(L, D, achieved samples per symbol) for a capture at `rate` Hz of a signal of `symbol_rate` symbols per second: L / D in
    lowest terms is the rational number with L <= max_interpolate and D <= max_decimate closest to
    samples_per_symbol * symbol_rate / rate (ties: the smaller L); the stream after mdc_iq_resample then has rate * L / D /
    symbol_rate samples per symbol.  ValueError when nothing within the limits comes within 1 % of the target.  (The only
    place Hz appear: everything else counts in samples.)"""
    from fractions import Fraction
    rate, symbol_rate, sps = float(rate), float(symbol_rate), float(samples_per_symbol)
    if not (np.isfinite(rate) and np.isfinite(symbol_rate) and np.isfinite(sps) and rate > 0 and symbol_rate > 0 and sps > 0):
        raise ValueError("rate, symbol_rate and samples_per_symbol must be finite and > 0")
    Lmax, Dmax = _check_resample_factors(max_interpolate, max_decimate)
    target = Fraction(sps) * Fraction(symbol_rate) / Fraction(rate)
    err, f = _closest_ratio(target, Lmax, Dmax)
    if err > target / 100:
        raise ValueError(f"no L / D with L <= {Lmax}, D <= {Dmax} comes within 1 % of {float(target):.6g} "
                         f"({sps:g} samples per symbol at {symbol_rate:g} sym/s from {rate:g} S/s); closest {f.numerator}/{f.denominator}")
    return f.numerator, f.denominator, rate * f.numerator / f.denominator / symbol_rate


def resample(iq, sample_format, shift: float = 0.0, interpolate: int = 1, decimate: int = 1, taps=None, phase0: int = 0, device=None):
    """Tune, low-pass and resample a capture by interpolate / decimate on the device (mdc_iq_resample, include/mdc.h: exact
    integer arithmetic; interpolate == 1 is ddc, bit for bit).  iq, shift, phase0: as ddc (shift in cycles per INPUT sample).
    taps: the int16 prototype at the interpolated rate, applied as written; None = design_resampler(L, D) of the factors reduced
    by their gcd -- interpolate == decimate needs explicit taps.  With explicit taps the factors are used as given.  Returns the
    (n_out, 2) int16 device tensor, n_out = resample_out_count(pairs, ntaps, L, D): an ordinary "ci16" capture.  Enqueues on
    torch's current stream without synchronising."""
    import math
    import torch
    fmt = sample_format_id(sample_format)
    (L, D), step = _check_resample_factors(interpolate, decimate), phase_step(shift)
    if taps is None:
        g = math.gcd(L, D)
        L, D = L // g, D // g
        if L == 1 and D == 1:
            raise ValueError("interpolate == decimate needs explicit taps (design_resampler designs filters for a change of rate)")
        taps = design_resampler(L, D)
    h = _int16_taps(taps)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    lib = _cabi.lib()
    n_out = _cabi.check(lib.mdc_iq_resample_out_count(pairs, h.size, L, D))
    out = torch.empty((n_out, 2), dtype=torch.int16, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(lib.mdc_iq_resample(t.data_ptr() if pairs else None, fmt, pairs, int(phase0) % (1 << 32), step, L, D, h.ctypes.data, h.size,
                                        out.data_ptr() if n_out else None, n_out, torch.cuda.current_stream(t.device).cuda_stream))
    return out


# ---- batched extraction (mdc_iq_extract): K stretches of a capture, each through the resampler's chain, in one launch ---------
def extract_plan(jobs, filters, sample_format, pairs_in: int, out_pairs=None):
    """The plan of one mdc_iq_extract launch (include/mdc.h, "batched extraction"; host code, no GPU).  filters: a sequence of
    (interpolate, decimate, taps); equal ones -- the same L, D and tap bytes -- are stored once.  jobs: a numpy array of
    _cabi.IQ_EXTRACT_JOB records whose `filter` indexes `filters` and whose out_first / n_out are used as given (out_pairs: the
    output's length, default the end of the last range), or a sequence of (first_pair, pairs, phase0, phase_step, filter, n_out),
    which are packed back to back in the order given.  Returns (blob, out_pairs): the plan as a numpy uint8 array -- the same
    inputs give the same bytes -- and the output's length in pairs.  Everything mdc_iq_extract_plan rejects is a _cabi.MdcError
    that names the job."""
    fmt = sample_format_id(sample_format)
    unique, index, taps_all, recs = {}, [], [], []
    for L, D, taps in filters:
        h = _int16_taps(taps)
        key = (int(L), int(D), h.tobytes())
        if key not in unique:
            unique[key] = len(recs)
            recs.append((int(L), int(D), h.size, sum(t.size for t in taps_all)))
            taps_all.append(h)
        index.append(unique[key])
    frec = np.array(recs, dtype=_cabi.IQ_EXTRACT_FILTER).reshape(-1)
    h_all = np.ascontiguousarray(np.concatenate(taps_all)) if taps_all else np.zeros(0, np.int16)
    if isinstance(jobs, np.ndarray) and jobs.dtype == _cabi.IQ_EXTRACT_JOB:
        jrec = np.ascontiguousarray(jobs).reshape(-1).copy()
        if out_pairs is None:
            out_pairs = int((jrec["out_first"] + jrec["n_out"]).max()) if jrec.size else 0
    else:
        rows = [tuple(int(v) for v in j) for j in jobs]
        jrec = np.zeros(len(rows), _cabi.IQ_EXTRACT_JOB)
        at = 0
        for k, (first, pairs, phase0, step, f, n_out) in enumerate(rows):
            jrec[k] = (first, pairs, at, n_out, phase0 % (1 << 32), step % (1 << 32), f, 0)
            at += max(n_out, 0)
        if out_pairs is None:
            out_pairs = at
    known = (jrec["filter"] >= 0) & (jrec["filter"] < len(index))      # an unknown index stays one: the planner names the job
    jrec["filter"][known] = np.asarray(index, np.int32)[jrec["filter"][known]] if len(index) else 0
    jrec["filter"][~known] = -1
    lib = _cabi.lib()
    nbytes = _cabi.check(lib.mdc_iq_extract_plan_bytes(jrec.size, frec.size, jrec.ctypes.data, frec.ctypes.data))
    blob = np.empty(nbytes, np.uint8)
    _cabi.check(lib.mdc_iq_extract_plan(fmt, int(pairs_in), jrec.ctypes.data, jrec.size, frec.ctypes.data, frec.size, h_all.ctypes.data, h_all.size,
                                        int(out_pairs), blob.ctypes.data, nbytes))
    return blob, int(out_pairs)


def extract_run(iq, sample_format, blob, out_pairs: int, out=None, device=None):
    """One mdc_iq_extract launch of a plan of extract_plan on a capture (iq: as frames_from_iq).  Returns the (out_pairs, 2)
    int16 device tensor; `out`, a tensor of that shape, is filled instead of a new one (pairs that no job names keep what they
    held; a new tensor holds zeros there).  Enqueues on torch's current stream; the plan's device copy is an ordinary torch
    transfer."""
    import torch
    fmt = sample_format_id(sample_format)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if out is None:
        out = torch.zeros((int(out_pairs), 2), dtype=torch.int16, device=t.device)
    elif out.dtype != torch.int16 or tuple(out.shape) != (int(out_pairs), 2) or not out.is_contiguous() or out.device != t.device:
        raise ValueError(f"out must be a contiguous ({int(out_pairs)}, 2) int16 tensor on the capture's device")
    plan_dev = torch.from_numpy(blob).to(t.device)
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_extract(t.data_ptr() if pairs else None, fmt, pairs, blob.ctypes.data, plan_dev.data_ptr(), blob.size,
                                               out.data_ptr() if out_pairs else None, int(out_pairs), torch.cuda.current_stream(t.device).cuda_stream))
    return out


def extract(iq, sample_format, stretches, device=None, whole_frames: bool = True):
    """Tune, low-pass and resample K stretches of one capture in ONE launch (mdc_iq_extract).  stretches: a sequence of
    (first_pair, stop_pair, shift, interpolate, decimate, taps); stretch k gives what resample(iq[first_pair:stop_pair], ...,
    shift, interpolate, decimate, taps) gives (for interpolate == 1: ddc), bit for bit -- the oscillator starts at phase 0 on
    the stretch's first pair.  Returns (block, offsets): the (N, 2) int16 device tensor of all stretches' outputs back to back
    and an int64 numpy array of K + 1 offsets, stretch k being block[offsets[k]:offsets[k + 1]].  whole_frames: every stretch
    is trimmed to a multiple of 128 outputs, so that the block is whole frames and no window of predict_iq(block, "ci16")
    straddles two stretches (a stretch of fewer than 128 outputs is empty)."""
    import torch
    fmt = sample_format_id(sample_format)
    t = _device_samples(iq, fmt, device)
    pairs_in = t.numel() * t.element_size() // _cabi.IQ_PAIR_BYTES[fmt]
    lib = _cabi.lib()
    jobs, filters, slot = [], [], {}
    for first, stop, shift, L, D, taps in stretches:
        (L, D), h = _check_resample_factors(L, D), np.asarray(taps)
        key = (L, D, id(taps))      # the same array object again: no need to compare its bytes (extract_plan dedupes the rest)
        if key not in slot:
            slot[key] = len(filters)
            filters.append((L, D, taps))
        first, stop = int(first), int(stop)
        if not 0 <= first <= stop <= pairs_in:
            raise ValueError(f"stretch [{first}, {stop}) does not lie inside the capture's {pairs_in} pairs")
        n = _cabi.check(lib.mdc_iq_resample_out_count(stop - first, h.size, L, D))
        jobs.append((first, stop - first, 0, phase_step(shift), slot[key], n // HOP_FRAME * HOP_FRAME if whole_frames else n))
    blob, out_pairs = extract_plan(jobs, filters, fmt, pairs_in)
    offsets = np.zeros(len(jobs) + 1, np.int64)
    np.cumsum([j[5] for j in jobs], out=offsets[1:])
    block = torch.empty((out_pairs, 2), dtype=torch.int16, device=t.device)      # packed back to back: every pair is written
    return extract_run(t, fmt, blob, out_pairs, out=block), offsets


def segment_votes(labels, offsets, classes: int):
    """Per segment k = labels[offsets[k]:offsets[k + 1]] the most frequent label among those >= 0 (the smallest on a tie; -1 when
    there is none): VTCNN2.scan_iq's rule for all segments at once.  labels: an integer tensor of class indices < classes, -1
    for "no label" (a squelched window); offsets: K + 1 non-decreasing window offsets, offsets[-1] <= len(labels).  Returns a (K,)
    int64 tensor on labels' device; torch operations only, nothing synchronises."""
    import torch
    C = int(classes)
    off = torch.as_tensor(np.asarray(offsets, np.int64) if not isinstance(offsets, torch.Tensor) else offsets, dtype=torch.int64).to(labels.device)
    K = off.numel() - 1
    if K < 0:
        raise ValueError("offsets must hold at least one value")
    lab = labels.reshape(-1).to(torch.int64)
    at = torch.arange(lab.numel(), dtype=torch.int64, device=lab.device)
    seg = torch.bucketize(at, off[1:], right=True)      # the segment of window i: how many segments end at or before it
    counted = (lab >= 0) & (lab < C) & (at >= off[0]) & (seg < K)
    counts = torch.zeros(max(K, 1) * C, dtype=torch.int64, device=lab.device)
    counts.scatter_add_(0, torch.where(counted, seg * C + lab, torch.zeros_like(lab)), counted.to(torch.int64))
    counts = counts.view(max(K, 1), C)[:K]
    # the largest count, and among equals the smallest class: one key per class, no two equal
    key = counts * C + torch.arange(C - 1, -1, -1, dtype=torch.int64, device=lab.device)
    return torch.where(counts.sum(1) > 0, key.argmax(1), torch.full((K,), -1, dtype=torch.int64, device=lab.device))


# ---- power spectrogram (mdc_iq_spectrogram) and the emitter scan: where the signals are, and how wide ------------------------
def spectrogram_rows(pairs: int, nfft: int, hop: int, avg: int) -> int:
    """mdc_iq_spectrogram_rows: rows of a capture of `pairs` pairs -- ((pairs - nfft) // hop + 1) // avg, or 0 when pairs < nfft;
    trailing segments that do not fill a row of `avg` are dropped."""
    return _cabi.check(_cabi.lib().mdc_iq_spectrogram_rows(int(pairs), int(nfft), int(hop), int(avg)))


def design_window(nfft: int, kind: str = "hann", beta: float = 8.0) -> np.ndarray:
    """An int16 analysis window for mdc_iq_spectrogram: rint(32767 w), w the PERIODIC Hann window 0.5 - 0.5 cos(2 pi n / nfft)
    (kind="hann") or numpy's Kaiser window of shape `beta` (kind="kaiser")."""
    n = int(nfft)
    if n < 1:
        raise ValueError("nfft must be >= 1")
    if kind == "hann":
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)
    elif kind == "kaiser":
        w = np.kaiser(n, float(beta))
    else:
        raise ValueError(f"kind must be 'hann' or 'kaiser' (got {kind!r})")
    return np.rint(32767.0 * w).astype(np.int16)


def _window_sums(window):
    w = np.asarray(window.cpu().numpy() if hasattr(window, "cpu") else window)
    if w.ndim != 1 or w.dtype.kind not in "iu":
        raise TypeError("window must be a one-dimensional integer array (int16)")
    w = w.astype(np.int64)
    return w.size, int(w.sum()), int((w * w).sum())


def window_scale(window) -> float:
    """The `scale` of mdc_iq_spectrogram with which a full-scale "ci16" tone (amplitude 32768) on a bin reads 1.0, 0 dBFS:
    1 / (32768 sum(w))^2.  ValueError unless sum(w) > 0."""
    _, s1, _ = _window_sums(window)
    if s1 <= 0:
        raise ValueError(f"the window's values must sum to more than 0 (got {s1})")
    return 1.0 / (32768.0 * s1) ** 2


def window_enbw(window) -> float:
    """Equivalent noise bandwidth in bins, nfft sum(w^2) / sum(w)^2: the factor by which the SUM of a noise-like signal's bins
    overstates its power (1.5 for Hann).  ValueError unless sum(w) > 0."""
    n, s1, s2 = _window_sums(window)
    if s1 <= 0:
        raise ValueError(f"the window's values must sum to more than 0 (got {s1})")
    return n * s2 / float(s1) ** 2


_default_windows: dict = {}      # (nfft, device) -> (int16 device tensor, scale)


def _default_window(nfft: int, device):
    import torch
    key = (int(nfft), str(device))
    if key not in _default_windows:
        w = design_window(nfft)
        _default_windows[key] = (torch.from_numpy(w).to(device), window_scale(w))
    return _default_windows[key]


def _spectra(order, iq, sample_format, nfft, hop, avg, window, device, scale):
    """spectrogram (order None: mdc_iq_spectrogram) and line_spectrum (mdc_iq_line_spectrum) share everything but the call"""
    import torch
    fmt = sample_format_id(sample_format)
    N = int(nfft)
    H = N // 2 if hop is None else int(hop)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    lib = _cabi.lib()
    rows = _cabi.check(lib.mdc_iq_spectrogram_rows(pairs, N, H, int(avg)))
    w, default_scale = _window_tensor(window, N, t.device)
    k = float(scale) if scale is not None else default_scale if default_scale is not None else window_scale(window)
    out = torch.empty((rows, N), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        tail = (N, H, int(avg), w.data_ptr(), k, out.data_ptr() if rows else None, rows, torch.cuda.current_stream(t.device).cuda_stream)
        if order is None:
            _cabi.check(lib.mdc_iq_spectrogram(t.data_ptr() if pairs else None, fmt, pairs, *tail))
        else:
            _cabi.check(lib.mdc_iq_line_spectrum(t.data_ptr() if pairs else None, fmt, pairs, order, *tail))
    return out


def spectrogram(iq, sample_format, nfft: int = 1024, hop=None, avg: int = 1, window=None, device=None, scale=None):
    """Averaged power spectra of a capture on the device (mdc_iq_spectrogram, include/mdc.h).  iq: as frames_from_iq.  Segments of
    nfft pairs every `hop` pairs (default nfft // 2; hop > nfft skips pairs), each multiplied by the int16 `window` and
    transformed; row r is the mean of segments r*avg .. r*avg + avg-1.  Returns the (rows, nfft) float32 device tensor in natural
    DFT order (spectrum_freqs), rows = spectrogram_rows(pairs, nfft, hop, avg).  window: None = design_window(nfft), built once
    per (nfft, device) and kept on the device; a numpy array (uploaded on every call); or an int16 device tensor, used where it
    lies.  scale: None = window_scale(window) -- 1.0 is a full-scale "ci16" tone on a bin; for an explicit DEVICE window that
    reads the window back (a synchronisation): pass scale to avoid it.  Otherwise the call enqueues on torch's current stream
    without synchronising."""
    return _spectra(None, iq, sample_format, nfft, hop, avg, window, device, scale)


def line_spectrum(iq, sample_format, order: int, nfft: int = 1024, hop=None, avg: int = 1, window=None, device=None, scale=None):
    """Averaged power spectra of a pointwise power of the capture on the device (mdc_iq_line_spectrum, include/mdc.h): spectrogram,
    argument for argument, of y = I^2 + Q^2 (order 0, IQ_LINE_ENVELOPE: a line at the symbol rate of a pulse-shaped linear
    modulation), of the capture itself (order 1: spectrogram's bits), of its square (order 2: a line at twice the carrier offset
    of BPSK and PAM) or of its fourth power (order 4: at four times the offset of QPSK and QAM), formed in exact integers from the
    samples at 16-bit full scale and scaled by 2^-16 (orders 0, 2) or 2^-48 (order 4).  The default window is spectrogram's cached
    one, scale=None is window_scale(window): the absolute level of a line spectrum carries no unit anyone needs -- find_line
    works with ratios.  ValueError for any other order."""
    if isinstance(order, bool) or order not in _cabi.LINE_SPECTRUM_ORDERS:
        raise ValueError(f"order must be one of {_cabi.LINE_SPECTRUM_ORDERS} (got {order!r})")
    return _spectra(int(order), iq, sample_format, nfft, hop, avg, window, device, scale)


def find_line(psd, lo: float, hi: float, two_sided: bool = False):
    """(frequency, prominence_db) of the strongest spectral line of ONE power spectrum of nfft bins in natural DFT order within a
    band; host numpy, float64.  Searched are the bins with lo <= f <= hi (two_sided: lo <= |f| <= hi), f = spectrum_freqs(nfft) in
    cycles per sample.  prominence_db is the strongest of them over the MEDIAN of the searched bins, in dB (inf over a median of
    0).  The frequency is refined by the parabola through the natural logarithms a, b, c of the bin before, the bin and the bin
    after (circular neighbours): delta = (a - c) / (2 (a - 2b + c)) bins -- exact for a Gaussian main lobe, within 0.016
    bin for a Hann window's --; delta = 0 when one of the three is <= 0 or the parabola has no maximum
    (a - 2b + c >= 0).  ValueError if no bin falls in the band or the spectrum holds a non-finite value."""
    p = np.array(psd.cpu().numpy() if hasattr(psd, "cpu") else psd, dtype=np.float64).reshape(-1)
    n = p.size
    if n < 2 or not np.all(np.isfinite(p)):
        raise ValueError("psd must hold at least two finite bins")
    lo, hi = float(lo), float(hi)
    f = np.fft.fftfreq(n)
    g = np.abs(f) if two_sided else f
    band = np.flatnonzero((g >= lo) & (g <= hi))
    if band.size == 0:
        raise ValueError(f"no bin of the {n} lies in the band {lo:g} .. {hi:g} cycles per sample")
    k = int(band[np.argmax(p[band])])
    return _line_from_search(n, k, float(p[k]), float(p[(k - 1) % n]), float(p[(k + 1) % n]), float(np.median(p[band])))


def _line_from_search(n: int, k: int, peak: float, left: float, right: float, floor: float):
    """find_line and find_lines behind their searches: (frequency, prominence_db) from the strongest searched bin k of n, its
    value, its circular neighbours' values and the median of the searched bins -- Python floats, float64 arithmetic"""
    prominence = 10.0 * np.log10(peak / floor) if floor > 0.0 and peak > 0.0 else (np.inf if peak > 0.0 else 0.0)
    delta = 0.0
    if left > 0.0 and peak > 0.0 and right > 0.0:
        a, b, c = np.log(left), np.log(peak), np.log(right)
        den = a - 2.0 * b + c
        if den < 0.0:
            delta = 0.5 * (a - c) / den
    return float(np.fft.fftfreq(n)[k] + delta / n), float(prominence)


def _window_tensor(window, N: int, device):
    """(int16 device tensor of N values, its default scale or None): spectrogram's rules for `window`"""
    import torch
    if window is None:
        return _default_window(N, device)
    if isinstance(window, torch.Tensor):
        if window.dtype != torch.int16:
            raise TypeError(f"window must be int16, got {window.dtype}")
        w = window.to(device).contiguous().view(-1)
    else:
        h = np.asarray(window)
        if h.dtype.kind not in "iu" or h.ndim != 1:
            raise TypeError("window must be a one-dimensional integer array (int16)")
        if h.size and (h.min() < -32768 or h.max() > 32767):
            raise ValueError("window must fit int16")
        w = torch.from_numpy(np.ascontiguousarray(h.astype(np.int16))).to(device)
    if w.numel() != N:
        raise ValueError(f"the window has {w.numel()} values, nfft is {N}")
    return w, None


def line_spectra(iq, sample_format, jobs, orders=(0, 2, 4), nfft: int = 1024, hop=None, avg: int = 8, window=None, device=None, scale=None,
                 return_rows: bool = False):
    """The line spectra of K stretches of one capture at several orders, and their means over the rows, in one call
    (mdc_iq_line_spectra, include/mdc.h: one launch per order and one for the means, whatever K).  iq: as frames_from_iq -- in
    practice the "ci16" block of extract(..., whole_frames=False).  jobs: a sequence of (first_pair, stop_pair), or a
    one-dimensional integer array of K + 1 non-decreasing offsets as extract returns them (job k is offsets[k]:offsets[k + 1]);
    jobs may overlap, be empty and start on any pair.  orders: 1 to 4 distinct values of 0, 1, 2, 4.  nfft, hop, avg, window,
    scale: as line_spectrum.  Returns (means, rows): the (K, len(orders), nfft) float64 device tensor -- means[k, i] is the
    float64 mean, row by row from the first, of line_spectrum(iq[first:stop], ..., orders[i], nfft, hop, avg), bit for bit;
    all zeros for a job too short for a row -- and an int64 numpy array of each job's row count.  With return_rows also the
    (len(orders), total rows, nfft) float32 device tensor of the rows themselves and the int64 numpy array of K + 1 first rows
    (job k owns rows first[k]:first[k + 1] of every plane).  Enqueues on torch's current stream; the job table goes to the
    device as an ordinary torch transfer."""
    import torch
    fmt = sample_format_id(sample_format)
    N = int(nfft)
    H = N // 2 if hop is None else int(hop)
    ords = [o for o in orders]
    if not 1 <= len(ords) <= _cabi.LINE_SPECTRA_MAX_ORDERS or len(set(ords)) != len(ords) or \
            any(isinstance(o, bool) or o not in _cabi.LINE_SPECTRUM_ORDERS for o in ords):
        raise ValueError(f"orders must be 1..{_cabi.LINE_SPECTRA_MAX_ORDERS} distinct values of {_cabi.LINE_SPECTRUM_ORDERS} (got {orders!r})")
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    if isinstance(jobs, np.ndarray) and jobs.ndim == 1:
        if jobs.size < 1 or jobs.dtype.kind not in "iu":
            raise ValueError("offsets must be a one-dimensional integer array of at least one value")
        off = jobs.astype(np.int64)
        spans = list(zip(off[:-1].tolist(), off[1:].tolist()))
    else:
        spans = [(int(a), int(z)) for a, z in jobs]
    rec = np.zeros(len(spans), _cabi.IQ_LINE_JOB)
    for k, (a, z) in enumerate(spans):
        if not 0 <= a <= z <= pairs:
            raise ValueError(f"job {k}: [{a}, {z}) does not lie inside the capture's {pairs} pairs")
        rec[k] = (a, z - a, 0, 0)
    lib = _cabi.lib()
    total = _cabi.check(lib.mdc_iq_line_spectra_rows(rec.ctypes.data, rec.size, pairs, N, H, int(avg)))
    w, default_scale = _window_tensor(window, N, t.device)
    k = float(scale) if scale is not None else default_scale if default_scale is not None else window_scale(window)
    K, no = rec.size, len(ords)
    rows = torch.empty((no, total, N), dtype=torch.float32, device=t.device)
    means = torch.empty((K, no, N), dtype=torch.float64, device=t.device)
    if K:
        jobs_dev = torch.from_numpy(rec.view(np.int64).reshape(K, 4)).to(t.device)
        o = (C.c_int * no)(*[int(v) for v in ords])
        with torch.cuda.device(t.device):
            _cabi.check(lib.mdc_iq_line_spectra(t.data_ptr() if pairs else None, fmt, pairs, rec.ctypes.data, jobs_dev.data_ptr(), K, o, no, N, H, int(avg),
                                                w.data_ptr(), k, rows.data_ptr() if total else None, total, means.data_ptr(),
                                                torch.cuda.current_stream(t.device).cuda_stream))
    counts = rec["rows"].astype(np.int64)
    if return_rows:
        return means, counts, rows, np.concatenate([rec["first_row"].astype(np.int64), np.array([total], np.int64)])
    return means, counts


def line_records(spectra, bands):
    """mdc_iq_find_lines on S spectra (include/mdc.h, "line search"): spectra, an (S, nfft) float64 tensor (a host tensor or
    array is moved to the device); bands, S tuples (lo, hi, two_sided).  Returns the S records as a numpy array of
    _cabi.IQ_LINE_RECORD -- one transfer of 48 bytes per spectrum, which synchronises.  A band without a bin is a ValueError that
    names the spectrum, before anything is launched."""
    import torch
    t = spectra if isinstance(spectra, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(spectra, dtype=np.float64)))
    if t.dtype != torch.float64 or t.dim() != 2:
        raise TypeError(f"spectra must be a two-dimensional float64 tensor, got {t.dtype} with {t.dim()} dimensions")
    if not t.is_cuda:
        t = t.to("cuda:0")
    t = t.contiguous()
    S, N = int(t.shape[0]), int(t.shape[1])
    rec = np.zeros(S, _cabi.IQ_LINE_BAND)
    bands = list(bands)
    if len(bands) != S:
        raise ValueError(f"{S} spectra, {len(bands)} bands")
    for i, (lo, hi, two) in enumerate(bands):
        rec[i] = (float(lo), float(hi), 1 if two else 0, 0)
    out = torch.zeros((S, _cabi.IQ_LINE_RECORD.itemsize), dtype=torch.uint8, device=t.device)
    if S:
        bands_dev = torch.from_numpy(rec.view(np.uint8).reshape(S, -1)).to(t.device)
        with torch.cuda.device(t.device):
            rc = _cabi.lib().mdc_iq_find_lines(t.data_ptr(), S, N, rec.ctypes.data, bands_dev.data_ptr(), out.data_ptr(),
                                               torch.cuda.current_stream(t.device).cuda_stream)
        if rc == -22:
            raise ValueError(_cabi.lib().mdc_last_error().decode("utf-8", "replace"))
        _cabi.check(rc)
    return out.cpu().numpy().view(_cabi.IQ_LINE_RECORD).reshape(-1)


def find_lines(spectra, bands):
    """find_line for S spectra at once, searched on the device (mdc_iq_find_lines): spectra, an (S, nfft) float64 tensor, nfft a
    power of two in 64..4096; bands, S tuples (lo, hi, two_sided).  Returns a list of S (frequency, prominence_db), each equal
    to find_line(spectra[s], lo, hi, two_sided) to the bit: the device finds the strongest searched bin, its neighbours and the
    two middle order statistics of the band, the arithmetic after the search is find_line's own.  ValueError if a band holds no
    bin or a spectrum holds a non-finite or negative value."""
    rec = line_records(spectra, bands)
    n = int(spectra.shape[1])
    out = []
    for s, r in enumerate(rec):
        if r["count"] < 0:
            raise ValueError(f"spectrum {s} holds a non-finite or negative value")
        floor = float(r["median_lo"]) if r["count"] % 2 else float(np.median(np.array([r["median_lo"], r["median_hi"]], np.float64)))
        out.append(_line_from_search(n, int(r["bin"]), float(r["peak"]), float(r["left"]), float(r["right"]), floor))
    return out


def _line_psd(iq, sample_format, order: int, nfft: int, avg: int):
    """the rows of line_spectrum(order) averaged in float64 on the host, as VTCNN2.scan_iq averages its spectrogram; None when
    the capture is too short for one row"""
    import torch
    spec = line_spectrum(iq, sample_format, order, nfft=nfft, avg=avg)
    if spec.shape[0] == 0:
        return None
    return spec.to(torch.float64).mean(0).cpu().numpy()


def estimate_symbol_rate(iq, sample_format, lo: float, hi: float, nfft: int = 1024, avg: int = 8, min_line_db: float = 8.0):
    """(rate, line_db): the symbol rate of a pulse-shaped linear modulation, in cycles per sample of iq, from the line of its
    envelope's spectrum -- line_spectrum(order 0, nfft, hop nfft // 2, avg), all rows averaged in float64, then
    find_line(psd, lo, hi).  rate is None when the line stays below min_line_db (line_db is returned either way).  A capture
    too short for one row of avg segments gives (None, -inf), not an error.

    min_line_db is a parameter, not a measurement.  What it rests on: the largest of about nfft noise-only bins of a spectrum
    averaged over K segments sat 1.4 - 2.5 dB over the median at K about 60, 5 dB at K = 30 and 8 dB at K = 6 in a float64
    prototype, while the lines of BPSK, QPSK, PAM4, QAM16 and QAM64 at 10 and 20 dB SNR stood 10 - 44 dB above it: 8 dB keeps
    noise out from a few dozen segments on, and with fewer a caller should raise it."""
    if not (0.0 < float(lo) <= float(hi) <= 0.5):
        raise ValueError(f"the band must satisfy 0 < lo <= hi <= 0.5 cycles per sample (got {lo!r} .. {hi!r})")
    psd = _line_psd(iq, sample_format, _cabi.IQ_LINE_ENVELOPE, nfft, avg)
    if psd is None:
        return None, float("-inf")
    rate, db = find_line(psd, lo, hi)
    return (rate if db >= float(min_line_db) else None), db


def estimate_carrier_offset(iq, sample_format, max_offset: float, nfft: int = 1024, avg: int = 8, min_line_db: float = 8.0):
    """(offset, order, line_db): the residual carrier offset of a linear modulation within +-max_offset cycles per sample of iq,
    from the line its square or fourth power shows.  Order 2 first (BPSK, PAM): find_line(psd of line_spectrum(order 2), 0,
    2 max_offset, two_sided=True); if that line reaches min_line_db, offset = f / 2.  Else order 4 (QPSK, QAM) with
    4 max_offset, offset = f / 4.  Else (0.0, 0, the better of the two prominences): keep the coarse estimate.  8PSK, analogue
    and frequency-shift signals show no line at these orders, and end there.  max_offset must keep 4 max_offset < 0.5.  A
    capture too short for one row gives (0.0, 0, -inf).  min_line_db: see estimate_symbol_rate."""
    m = float(max_offset)
    if not (np.isfinite(m) and m > 0.0 and 4.0 * m < 0.5):
        raise ValueError(f"max_offset must be > 0 and keep 4 * max_offset < 0.5 cycles per sample (got {max_offset!r})")
    best = float("-inf")
    for order in (2, 4):
        psd = _line_psd(iq, sample_format, order, nfft, avg)
        if psd is None:
            break
        f, db = find_line(psd, 0.0, order * m, two_sided=True)
        if db >= float(min_line_db):
            return f / order, order, db
        best = max(best, db)
    return 0.0, 0, best


def spectrum_freqs(nfft: int) -> np.ndarray:
    """The bins' frequencies in cycles per sample, in the natural order of spectrogram's columns: 0, 1/nfft, ... up to
    0.5 - 1/nfft, then -0.5 ... -1/nfft.  All in [-0.5, 0.5)."""
    return np.fft.fftfreq(int(nfft))


def find_emitters(psd, threshold_db: float = 6.0, min_bins: int = 3, merge_bins: int = 2, dc_guard: int = 1, window=None):
    """(centre, bandwidth, power_dbfs, snr_db) of every emitter in ONE power spectrum of nfft bins in natural order, for example
    spectrogram(...).mean(0).cpu(); host numpy, float64.  The noise floor is the median bin.  Bins within dc_guard of bin 0
    (both sides; dc_guard < 0: none) are set to the floor first: a tuner's DC spike is no emitter.  In centred order
    (-0.5 .. 0.5) an emitter is a run of adjacent bins above floor * 10^(threshold_db / 10); runs separated by at most
    merge_bins bins at or below the threshold are joined (the bins between them then belong to the run), and runs of fewer than
    min_bins bins are dropped.  Per run: centre, the centroid of the power above the floor (bins below the floor count as 0), in
    cycles per sample; bandwidth, the run's width in bins / nfft; power_dbfs, 10 log10 of the summed power above the floor,
    divided by window_enbw(window) when the window is given (the bins of a noise-like signal overstate its power by that
    factor); snr_db, the largest bin over the floor.  Returned in order of centre.  The spectrum is NOT treated as circular: a
    signal straddling +-0.5 comes out as two emitters, one at each edge."""
    from collections import namedtuple
    Emitter = namedtuple("Emitter", "centre bandwidth power_dbfs snr_db")
    p = np.array(psd.cpu().numpy() if hasattr(psd, "cpu") else psd, dtype=np.float64).reshape(-1)
    n = p.size
    if n < 2 or not np.all(np.isfinite(p)):
        raise ValueError("psd must hold at least two finite bins")
    floor = float(np.median(p))
    if not floor > 0.0:
        return []
    if dc_guard >= 0:
        p[np.arange(-int(dc_guard), int(dc_guard) + 1) % n] = floor
    p = np.fft.fftshift(p)
    f = np.fft.fftshift(np.fft.fftfreq(n))
    above = np.flatnonzero(p > floor * 10.0 ** (float(threshold_db) / 10.0))
    if above.size == 0:
        return []
    cut = np.flatnonzero(np.diff(above) > int(merge_bins) + 1)      # a gap of g bins is a difference of g + 1
    first, last = above[np.r_[0, cut + 1]], above[np.r_[cut, above.size - 1]]
    enbw = window_enbw(window) if window is not None else 1.0
    found = []
    for a, b in zip(first, last):
        if b - a + 1 < int(min_bins):
            continue
        excess = np.maximum(p[a:b + 1] - floor, 0.0)
        total = float(excess.sum())
        found.append(Emitter(float((excess * f[a:b + 1]).sum() / total), float(b - a + 1) / n, 10.0 * np.log10(total / enbw),
                             10.0 * np.log10(float(p[a:b + 1].max()) / floor)))
    return found


# ---- intermittent emitters: quantile spectra along time (mdc_iq_spectrum_quantiles), band power per row, bursts ---------------
def _quantile_ranks(q, rows: int):
    """(ranks, scalar): floor(q * (rows - 1)) per value of q, in Python floats; ValueError for what spectrum_quantiles refuses"""
    import math
    scalar = isinstance(q, (int, float, np.floating, np.integer)) and not isinstance(q, bool)
    qs = [q] if scalar else list(q)
    if len(qs) > _cabi.QUANTILES_MAX_RANKS:
        raise ValueError(f"at most {_cabi.QUANTILES_MAX_RANKS} quantiles per call (got {len(qs)})")
    if rows < 1:
        raise ValueError("the spectrogram has no rows")
    ranks = []
    for v in qs:
        v = float(v)
        if not 0.0 <= v <= 1.0:      # (a NaN fails both comparisons)
            raise ValueError(f"q must lie in [0, 1] (got {v!r})")
        ranks.append(math.floor(v * (rows - 1)))
    return ranks, scalar


def spectrum_quantiles(spec, q, device=None):
    """Order statistics of a spectrogram along time, per bin, on the device (mdc_iq_spectrum_quantiles, include/mdc.h).  spec: the
    (rows, nfft) float32 tensor of spectrogram / line_spectrum (a host tensor or array is moved to the device); q: a float or
    up to 8 floats in [0, 1].  Row i of the result is, for every bin, the element at position floor(q[i] * (rows - 1)) of the
    bin's values sorted ascending: an element of the column, never an interpolation -- q = 0.5 is the (lower) median over time,
    a noise floor that bursts do not lift; q = 0.98 the level a bin reaches in its top 2 % of rows, which shows an intermittent
    emitter at full strength.  Returns (len(q), nfft) float32 on the device, (nfft,) for a scalar q.  ValueError -- before
    anything touches a device -- for q outside [0, 1], more than 8 values, a spectrogram without rows, or a shape that is not
    (rows, nfft) with nfft a power of two in 64..4096.  Enqueues on torch's current stream without synchronising."""
    import torch
    shape = tuple(spec.shape) if hasattr(spec, "shape") else ()
    if len(shape) != 2 or not (_cabi.SPECTROGRAM_MIN_NFFT <= shape[1] <= _cabi.SPECTROGRAM_MAX_NFFT and shape[1] & (shape[1] - 1) == 0):
        raise ValueError(f"spec must be a (rows, nfft) spectrogram, nfft a power of two in {_cabi.SPECTROGRAM_MIN_NFFT}.."
                         f"{_cabi.SPECTROGRAM_MAX_NFFT} (got shape {shape})")
    rows, nfft = int(shape[0]), int(shape[1])
    ranks, scalar = _quantile_ranks(q, rows)
    if rows > _cabi.QUANTILES_MAX_ROWS:
        raise ValueError(f"at most {_cabi.QUANTILES_MAX_ROWS} rows (got {rows})")
    t = spec if isinstance(spec, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(spec)))
    if t.dtype != torch.float32:
        raise TypeError(f"spec must be float32, got {t.dtype}")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous()
    out = torch.empty((len(ranks), nfft), dtype=torch.float32, device=t.device)
    r = np.asarray(ranks, np.int64)
    if len(ranks):
        with torch.cuda.device(t.device):
            _cabi.check(_cabi.lib().mdc_iq_spectrum_quantiles(t.data_ptr(), rows, nfft, r.ctypes.data, len(ranks), out.data_ptr(),
                                                              torch.cuda.current_stream(t.device).cuda_stream))
    return out[0] if scalar else out


def emitter_bins(emitter, nfft: int):
    """(first, count): the bins of an emitter of find_emitters in natural DFT order -- its width placed around its centroid.
    count = max(1, round(bandwidth * nfft)); first = round(centre * nfft - (count - 1) / 2) mod nfft; the bins are
    (first + i) mod nfft, i < count (an emitter around 0 wraps from the last bins to the first)."""
    n = int(nfft)
    count = max(1, int(round(float(emitter.bandwidth) * n)))
    first = int(round(float(emitter.centre) * n - (count - 1) / 2.0)) % n
    return first, count


def band_power(spec, first: int, count: int):
    """(rows,) float64 device tensor: per row the sum of spec[:, (first + i) mod nfft], i < count, taken in float64 -- the power
    in an emitter's bins (emitter_bins) row by row, which against count times the noise floor per bin gives its bursts
    (find_bursts)."""
    import torch
    nfft = spec.shape[1]
    cols = (int(first) + torch.arange(int(count), device=spec.device)) % nfft
    return spec[:, cols].to(torch.float64).sum(1)


def find_bursts(band, floor: float, threshold_db: float = 3.0, min_rows: int = 1, merge_rows: int = 1):
    """Half-open (first_row, stop_row) of every burst in one band-power series, in order; host numpy.  Row r is on when
    band[r] > floor * 10^(threshold_db / 10); runs of on-rows separated by at most merge_rows off-rows are joined (the rows
    between them then belong to the run), and runs of fewer than min_rows rows are dropped: find_emitters' run logic, along
    time."""
    b = np.array(band.cpu().numpy() if hasattr(band, "cpu") else band, dtype=np.float64).reshape(-1)
    on = np.flatnonzero(b > float(floor) * 10.0 ** (float(threshold_db) / 10.0))
    if on.size == 0:
        return []
    cut = np.flatnonzero(np.diff(on) > int(merge_rows) + 1)      # a gap of g rows is a difference of g + 1
    first, last = on[np.r_[0, cut + 1]], on[np.r_[cut, on.size - 1]]
    return [(int(a), int(z) + 1) for a, z in zip(first, last) if z - a + 1 >= int(min_rows)]


def burst_pairs(first_row: int, stop_row: int, nfft: int, hop: int, avg: int):
    """Half-open interval of input pairs that rows first_row .. stop_row - 1 of a spectrogram read: row r averages segments
    r*avg .. r*avg + avg-1, segment s holds pairs s*hop .. s*hop + nfft-1."""
    return int(first_row) * int(avg) * int(hop), ((int(stop_row) - 1) * int(avg) + int(avg) - 1) * int(hop) + int(nfft)


def window_support(w: int, hop: int, ntaps: int, interpolate: int, decimate: int):
    """Inclusive (first, last) input pair read by window w -- outputs w*hop .. w*hop + 127 -- of a stream of mdc_iq_ddc /
    mdc_iq_resample with ntaps taps and the factors L / D (include/mdc.h): output j reads the pairs n with
    j D <= n L <= j D + ntaps - 1, that is ceil(j D / L) .. floor((j D + ntaps - 1) / L); for L = 1, j D .. j D + ntaps - 1.
    An output whose stretch of the zero-stuffed stream holds no input pair (possible only with ntaps < L) reads nothing and
    counts for nothing; among 128 consecutive outputs at least one reads a pair (L <= 32)."""
    first, last = _window_supports([int(w)], hop, ntaps, interpolate, decimate)
    return int(first[0]), int(last[0])


def _window_supports(windows, hop, ntaps, interpolate, decimate):
    """window_support for an array of window indices: (first, last), int64 arrays"""
    L, D, T = int(interpolate), int(decimate), int(ntaps)
    j = np.asarray(windows, np.int64).reshape(-1, 1) * int(hop) + np.arange(HOP_FRAME, dtype=np.int64)[None, :]
    lo, hi = -((-j * D) // L), (j * D + T - 1) // L
    reads = hi >= lo
    return np.where(reads, lo, np.iinfo(np.int64).max).min(axis=1), np.where(reads, hi, -1).max(axis=1)


DEFAULT_FILL = 1.35 / 8      # occupied fraction of the output rate: a root-raised-cosine signal, beta 0.35, at 8 samples per symbol


def channel_plan(centre: float, bandwidth: float, fill: float = DEFAULT_FILL, max_interpolate: int = _cabi.RESAMPLE_MAX_INTERPOLATE,
                 max_decimate: int = _cabi.RESAMPLE_MAX_DECIMATE):
    """(shift, L, D, fill_achieved) for an emitter of find_emitters: shift = -centre brings it to 0, and L / D in lowest terms is
    the rational with L <= max_interpolate, D <= max_decimate closest to bandwidth / fill (resample_ratio's search): resampling by
    L / D stretches every width by D / L, after which the emitter occupies fill_achieved = bandwidth * D / L of the output rate.  The default fill is what a root-raised-cosine
    signal with beta = 0.35 occupies at the nets' 8 samples per symbol.  ValueError when nothing within the limits comes within
    1 % of bandwidth / fill."""
    from fractions import Fraction
    centre, bandwidth, fill = float(centre), float(bandwidth), float(fill)
    if not (np.isfinite(centre) and -0.5 <= centre <= 0.5):
        raise ValueError(f"centre must lie in [-0.5, 0.5] cycles per sample (got {centre!r})")
    if not (np.isfinite(bandwidth) and np.isfinite(fill) and bandwidth > 0 and fill > 0):
        raise ValueError("bandwidth and fill must be finite and > 0")
    Lmax, Dmax = _check_resample_factors(max_interpolate, max_decimate)
    target = Fraction(bandwidth) / Fraction(fill)
    err, f = _closest_ratio(target, Lmax, Dmax)
    if err > target / 100:
        raise ValueError(f"no L / D with L <= {Lmax}, D <= {Dmax} comes within 1 % of {float(target):.6g} "
                         f"(fill {fill:g} of the output rate for a bandwidth of {bandwidth:g}); closest {f.numerator}/{f.denominator}")
    return -centre, f.numerator, f.denominator, bandwidth * f.denominator / f.numerator


def channel_plans(emitters, fill: float = DEFAULT_FILL):
    """channel_plan(centre, bandwidth, fill) for a sequence of (centre, bandwidth): the same tuples, with the search for L / D made
    once per distinct bandwidth -- the boxes of a spectrogram have few widths (a number of bins over nfft), and the search, exact
    rationals over every L, is most of what a plan costs."""
    ratios, out = {}, []
    for centre, bandwidth in emitters:
        centre, bandwidth = float(centre), float(bandwidth)
        if bandwidth not in ratios:
            ratios[bandwidth] = channel_plan(centre, bandwidth, fill)[1:]
        elif not (np.isfinite(centre) and -0.5 <= centre <= 0.5):
            raise ValueError(f"centre must lie in [-0.5, 0.5] cycles per sample (got {centre!r})")
        out.append((-centre,) + ratios[bandwidth])
    return out


def plan_taps(interpolate: int, decimate: int) -> np.ndarray:
    """The filter VTCNN2.scan_iq puts behind a channel_plan: design_resampler(L, D) (for L == 1: design_lowpass(D)) with its default
    8 max(L, D) taps where mdc_iq_resample's limit of 1024 taps allows them, else the same design cut to 1024 taps (max(L, D) > 128:
    the transition band widens in proportion); L == D == 1, nothing to reject: one tap of (all but) unit gain."""
    L, D = _check_resample_factors(interpolate, decimate)
    if L == 1 and D == 1:
        return np.array([32767], np.int16)
    return design_resampler(L, D, ntaps=min(8 * max(L, D), _cabi.RESAMPLE_MAX_TAPS))


# ---- channelizer (mdc_iq_channelizer): all M evenly spaced channels of a capture in one pass -- a polyphase filter bank ------
def _check_channels(channels) -> int:
    M = int(channels)
    if not (_cabi.CHANNELIZER_MIN_CHANNELS <= M <= _cabi.CHANNELIZER_MAX_CHANNELS and M & (M - 1) == 0):
        raise ValueError(f"channels must be a power of two in {_cabi.CHANNELIZER_MIN_CHANNELS}..{_cabi.CHANNELIZER_MAX_CHANNELS} (got {channels!r})")
    return M


def _check_channelizer_taps(h, M: int) -> np.ndarray:
    """host taps for mdc_iq_channelizer -> contiguous int16, or TypeError / ValueError: the checks the library cannot make of a
    device buffer without a synchronisation"""
    h = np.asarray(h)
    if h.dtype.kind not in "iu" or h.ndim != 1:
        raise TypeError("taps must be a one-dimensional integer array (int16)")
    if not 1 <= h.size <= _cabi.CHANNELIZER_MAX_TAPS_PER_CHANNEL * M:
        raise ValueError(f"ntaps must be in 1..{_cabi.CHANNELIZER_MAX_TAPS_PER_CHANNEL * M} for {M} channels (got {h.size})")
    if h.min() < -32768 or h.max() > 32767:
        raise ValueError("taps must fit int16")
    a = np.abs(h.astype(np.int64))
    for r in range(min(M, h.size)):
        total = int(a[r::M].sum())
        if total > _cabi.CHANNELIZER_MAX_BRANCH_ABS_SUM:
            raise ValueError(f"residue {r} of the taps has sum |h| = {total}: mdc_iq_channelizer wants <= {_cabi.CHANNELIZER_MAX_BRANCH_ABS_SUM} "
                             f"per residue mod {M}")
    return np.ascontiguousarray(h.astype(np.int16))


def design_channelizer(channels: int, taps_per_channel: int = 8, cutoff=None, beta: float = 8.0):
    """(taps int16, tap_shift): the prototype low-pass of an M = channels channel filter bank for mdc_iq_channelizer.  A
    Kaiser-windowed sinc of taps_per_channel * M taps whose -6 dB point lies at `cutoff` cycles per input sample (default 0.5 / M,
    the channel edge: neighbouring channels cross at -6 dB), in Q(15 + tap_shift) with tap_shift = log2(M) - 1: scaled to sum
    exactly 32768 * 2^tap_shift (DC gain 1), rounded, the centre tap(s) taking what is missing so that the taps stay symmetric.
    ValueError if a tap leaves int16 or a residue's sum |h| exceeds 65535.

    With the defaults, for M in {8, 16, 64, 256, 1024} (from the taps themselves, dense FFT): droop <= 0.1 dB over |f| <= 0.25 / M
    (0.068 .. 0.078 dB), -6.0 +- 0.1 dB at 0.5 / M, >= 75 dB attenuation for |f| >= 0.85 / M (76.1 .. 80.7 dB); the largest tap
    is about 16,380 and the largest residue's sum |h| about 24,600.  (A plain Q15 unit sum would leave the largest tap near 100 at
    M = 1024: the shift is what keeps the stop band.)

    Aliasing: a decimation by D folds the frequency f (relative to the channel's centre) onto f - m / D.  With D = M / 2 the output
    rate is 2 / M and its band |f'| <= 1 / M; whatever folds INTO that band comes from |f| >= 2 / M - 1 / M = 1 / M, which lies in
    the stop band: over the whole output band every alias is >= 75 dB down, and the transition band 0.5 / M .. 0.85 / M, where
    the neighbours leak in, stays where it is, outside the channel.  With D = M (critically sampled) the output band is
    |f'| <= 0.5 / M and the transition band folds back onto 0.15 / M .. 0.5 / M: only |f'| <= 0.15 / M is alias-free to 75 dB.
    Group delay: (ntaps - 1) / 2 input samples."""
    M = _check_channels(channels)
    tpc = int(taps_per_channel)
    if not 1 <= tpc <= _cabi.CHANNELIZER_MAX_TAPS_PER_CHANNEL:
        raise ValueError(f"taps_per_channel must be in 1..{_cabi.CHANNELIZER_MAX_TAPS_PER_CHANNEL} (got {taps_per_channel!r})")
    fc = 0.5 / M if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError(f"cutoff must lie in (0, 0.5] cycles per sample (got {fc!r})")
    T, shift = tpc * M, M.bit_length() - 2
    total = 32768 << shift
    k = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(T, float(beta))
    q = np.rint(h / h.sum() * float(total)).astype(np.int64)
    rest = total - int(q.sum())      # T is even: symmetric taps sum to an even number, both centre taps take half of what is missing
    q[T // 2 - 1] += rest // 2
    q[T // 2] += rest - rest // 2
    if q.min() < -32768 or q.max() > 32767 or max(int(np.abs(q[r::M]).sum()) for r in range(M)) > _cabi.CHANNELIZER_MAX_BRANCH_ABS_SUM:
        raise ValueError("these parameters give taps outside int16 / a residue beyond the sum |h| <= 65535 of mdc_iq_channelizer")
    return q.astype(np.int16), shift


def channelizer_out_count(pairs_in: int, channels: int, ntaps: int, decimate: int) -> int:
    """mdc_iq_channelizer_out_count: output pairs PER CHANNEL of a capture of pairs_in pairs, (pairs_in - ntaps) // decimate + 1 or
    0 (a "valid" convolution)."""
    return _cabi.check(_cabi.lib().mdc_iq_channelizer_out_count(int(pairs_in), int(channels), int(ntaps), int(decimate)))


def channel_freqs(channels: int) -> np.ndarray:
    """The channels' centres in cycles per input sample, in the order of channelize's rows: k / M folded into [-0.5, 0.5) --
    0, 1/M, ... up to 0.5 - 1/M, then -0.5 ... -1/M."""
    return np.fft.fftfreq(_check_channels(channels))


_default_channelizers: dict = {}      # (channels, device) -> (int16 device tensor, tap_shift)


def _default_channelizer(channels: int, device):
    import torch
    key = (int(channels), str(device))
    if key not in _default_channelizers:
        h, shift = design_channelizer(channels)
        _default_channelizers[key] = (torch.from_numpy(h).to(device), shift)
    return _default_channelizers[key]


def channelize(iq, sample_format, channels: int, decimate=None, taps=None, tap_shift=None, first_index: int = 0, whole_frames: bool = False,
               device=None):
    """Split a capture into M = channels evenly spaced channels in one pass on the device (mdc_iq_channelizer, include/mdc.h: exact
    integer branch sums, one float32 M-point transform per output step).  iq: as frames_from_iq.  Returns the (M, n_out, 2) int16
    device tensor: row k is the capture shifted by -k / M cycles per sample (channel_freqs; the phase referenced to absolute sample
    first_index at iq's first pair), low-passed by the taps and decimated by `decimate` -- an ordinary "ci16" capture for
    frames_from_iq / normalized_frames_from_iq / VTCNN2.predict_iq; n_out = channelizer_out_count(pairs, M, ntaps, decimate).

    decimate: None = M / 2.  The channels are then 2 x oversampled: the output rate 2 / M is twice the channel spacing, so the
    filter's transition band beyond the channel edge 0.5 / M stays inside the output band instead of folding back onto the
    channel -- nothing aliases onto a channel that the prototype has not taken down to its stop band (design_channelizer).  M
    (critically sampled) halves the output but folds each channel's edges onto itself.
    taps: None = design_channelizer(M), built once per (M, device) and kept on the device; a numpy array, int16 in Q(15 + tap_shift),
    validated (int16, per-residue sum |h| <= 65535) and uploaded on every call; or an int16 device tensor, used where it lies and
    NOT validated -- the precondition is then the caller's.  tap_shift: required with explicit taps.
    whole_frames: use only as many input pairs as give the largest n_out that is a multiple of 128 (hop == 128 windows then never
    straddle two channels of the flat block).  Enqueues on torch's current stream without synchronising."""
    import torch
    fmt = sample_format_id(sample_format)
    M = _check_channels(channels)
    D = M // 2 if decimate is None else int(decimate)
    t = _device_samples(iq, fmt, device)
    pairs = _pair_count(t, fmt)
    if int(first_index) < 0:
        raise ValueError("first_index must be >= 0")
    if taps is None:
        if tap_shift is not None:
            raise ValueError("tap_shift belongs to explicit taps (the default design brings its own)")
        h, shift = _default_channelizer(M, t.device)
    else:
        if tap_shift is None:
            raise ValueError("explicit taps need their tap_shift (the taps are Q(15 + tap_shift))")
        shift = int(tap_shift)
        if isinstance(taps, torch.Tensor):
            if taps.dtype != torch.int16:
                raise TypeError(f"taps must be int16, got {taps.dtype}")
            h = taps.to(t.device).contiguous().view(-1)
        else:
            h = torch.from_numpy(_check_channelizer_taps(taps, M)).to(t.device)
    if not 0 <= shift <= _cabi.CHANNELIZER_MAX_TAP_SHIFT:
        raise ValueError(f"tap_shift must be in 0..{_cabi.CHANNELIZER_MAX_TAP_SHIFT} (got {shift})")
    T = h.numel()
    lib = _cabi.lib()
    n_out = _cabi.check(lib.mdc_iq_channelizer_out_count(pairs, M, T, D))
    if whole_frames:
        n_out = n_out // HOP_FRAME * HOP_FRAME
        pairs = (n_out - 1) * D + T if n_out else 0
    out = torch.empty((M, n_out, 2), dtype=torch.int16, device=t.device)
    with torch.cuda.device(t.device):
        _cabi.check(lib.mdc_iq_channelizer(t.data_ptr() if pairs else None, fmt, pairs, int(first_index), M, D, h.data_ptr(), T, shift,
                                           out.data_ptr() if n_out else None, n_out, torch.cuda.current_stream(t.device).cuda_stream))
    return out


# ---- time-frequency detection (mdc_iq_spectrogram_components): hoppers, overlapping bursts, single packets -------------------------
def _check_spectrogram_shape(spec):
    shape = tuple(spec.shape) if hasattr(spec, "shape") else ()
    if len(shape) != 2 or not (_cabi.SPECTROGRAM_MIN_NFFT <= shape[1] <= _cabi.SPECTROGRAM_MAX_NFFT and shape[1] & (shape[1] - 1) == 0):
        raise ValueError(f"spec must be a (rows, nfft) spectrogram, nfft a power of two in {_cabi.SPECTROGRAM_MIN_NFFT}.."
                         f"{_cabi.SPECTROGRAM_MAX_NFFT} (got shape {shape})")
    return int(shape[0]), int(shape[1])


def _float32_tensor(x, what: str):
    """x as a float32 torch tensor where it lies (TypeError for another dtype): nothing is moved yet"""
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    return t


def components_workspace(rows: int, nfft: int) -> int:
    """mdc_iq_spectrogram_components_workspace: bytes of scratch the labelling of a (rows, nfft) spectrogram needs (no GPU)."""
    return _cabi.check(_cabi.lib().mdc_iq_spectrogram_components_workspace(int(rows), int(nfft)))


def spectrogram_components(spec, thresh, reach_rows: int = 1, reach_bins: int = 1, capacity: int = 65536, device=None):
    """Connected components of a thresholded spectrogram on the device (mdc_iq_spectrogram_components, include/mdc.h).  spec: the
    (rows, nfft) float32 tensor of spectrogram (a host tensor or array is moved to the device); thresh: nfft float32 values in
    natural DFT order (detection_threshold).  Cell (r, k) is on iff spec[r, k] > thresh[k]; on-cells at most reach_rows rows and
    reach_bins CENTRED columns apart are linked (centred column c = (k + nfft/2) mod nfft: the band is not circular at +-0.5,
    and natural bins nfft-1 and 0 are neighbours); a component is a connected set, numbered by its first cell in (row, centred
    column) order.  Returns (labels, records, count): labels, the (rows, nfft) int32 device tensor of component numbers in natural
    positions, -1 where off; records, a numpy array of _cabi.IQ_COMPONENT (box in rows and centred columns, half-open; cells;
    peak and where it is) trimmed to min(count, capacity); count, the number of components, which may exceed capacity -- the
    labels are complete regardless.  Reading count and the records back is the call's one synchronisation; the workspace is
    allocated here.  ValueError / TypeError -- before anything touches a device -- for a shape that is not (rows, nfft) with
    nfft a power of two in 64..4096, no rows, more than 2^31 - 1 cells, a thresh that does not hold nfft values, a reach
    outside 0..4, or a negative capacity."""
    import torch
    rows, nfft = _check_spectrogram_shape(spec)
    if rows < 1:
        raise ValueError("the spectrogram has no rows")
    if rows * nfft > _cabi.COMPONENTS_MAX_CELLS:
        raise ValueError(f"at most {_cabi.COMPONENTS_MAX_CELLS} cells (got {rows} x {nfft})")
    tshape = tuple(thresh.shape) if hasattr(thresh, "shape") else (len(thresh),)
    if tshape != (nfft,):
        raise ValueError(f"thresh must hold nfft = {nfft} values (got shape {tshape})")
    a, b, cap = int(reach_rows), int(reach_bins), int(capacity)
    if not (0 <= a <= _cabi.COMPONENTS_MAX_REACH and 0 <= b <= _cabi.COMPONENTS_MAX_REACH):
        raise ValueError(f"reach_rows and reach_bins must be in 0..{_cabi.COMPONENTS_MAX_REACH} (got {reach_rows!r}, {reach_bins!r})")
    if cap < 0:
        raise ValueError(f"capacity must be >= 0 (got {capacity!r})")
    t, th = _float32_tensor(spec, "spec"), _float32_tensor(thresh, "thresh")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t, th = t.contiguous(), th.to(t.device).contiguous()
    lib = _cabi.lib()
    labels = torch.empty((rows, nfft), dtype=torch.int32, device=t.device)
    comps = torch.empty((cap, 4), dtype=torch.int64, device=t.device)      # 32-byte records, 8-byte aligned
    count = torch.empty((1,), dtype=torch.int64, device=t.device)
    work = torch.empty((_cabi.check(lib.mdc_iq_spectrogram_components_workspace(rows, nfft)) // 8 + 2,), dtype=torch.int64, device=t.device)
    ws = work.data_ptr() + (-work.data_ptr()) % 16
    with torch.cuda.device(t.device):
        _cabi.check(lib.mdc_iq_spectrogram_components(t.data_ptr(), rows, nfft, th.data_ptr(), a, b, labels.data_ptr(),
                                                      comps.data_ptr() if cap else None, cap, count.data_ptr(), ws,
                                                      torch.cuda.current_stream(t.device).cuda_stream))
    n = int(count.item())
    records = comps[:min(n, cap)].cpu().numpy().view(_cabi.IQ_COMPONENT).reshape(-1)
    return labels, records, n


def detection_threshold(spec, threshold_db: float = 6.0, dc_guard: int = 1, floor: str = "flat"):
    """The per-bin threshold of a time-frequency detection: an (nfft,) float32 device tensor in natural DFT order.  Q0 =
    spectrum_quantiles(spec, 0.5) is every bin's median over time, which bursts do not lift.  floor="flat": the median over the
    bins of Q0, one level for the whole band -- an element of Q0, the LOWER median sort(Q0)[(nfft - 1) // 2], taken on the device in
    float32; scan_iq(bursts=True)'s noise is numpy's float64 median of the same Q0, the mean of the two middle values, so the
    two agree to within the spacing of Q0's middle values, not bit for bit; "per-bin": Q0
    itself, for a coloured front-end -- whatever is on in more than half the rows is then floor, not signal.  The floor times
    10^(threshold_db / 10), in float32; bins within dc_guard of bin 0 (both sides; dc_guard < 0: none) are +inf, which switches
    them off.  A floor that is not > 0 gives +inf (nothing is detected there; "flat": anywhere)."""
    import torch
    if floor not in ("flat", "per-bin"):
        raise ValueError(f"floor must be 'flat' or 'per-bin' (got {floor!r})")
    factor = float(np.float32(10.0 ** (float(threshold_db) / 10.0)))
    if not np.isfinite(factor):
        raise ValueError(f"threshold_db must be finite (got {threshold_db!r})")
    q0 = spectrum_quantiles(spec, 0.5)
    nfft = q0.shape[0]
    level = q0 if floor == "per-bin" else torch.sort(q0).values[(nfft - 1) // 2].expand(nfft)
    inf = torch.full((nfft,), float("inf"), dtype=torch.float32, device=q0.device)
    thresh = torch.where(level > 0, level * factor, inf)
    if int(dc_guard) >= 0:
        thresh[torch.arange(-int(dc_guard), int(dc_guard) + 1, device=q0.device) % nfft] = float("inf")
    return thresh


# ---- a local noise floor (mdc_iq_spectrogram_cfar): 2-D order-statistic CFAR, for a floor that moves in time and in frequency ------
CFAR_DEFAULTS = dict(train_rows=8, train_bins=32, guard_rows=2, guard_bins=8, rank=0.5)


def cfar_parameters(cfar=None):
    """detect_iq's cfar= as the tuple (train_rows, train_bins, guard_rows, guard_bins, rank): None gives CFAR_DEFAULTS, a dict
    overrides them by key (ValueError for an unknown key), a sequence must hold all five in that order."""
    if cfar is None:
        cfar = {}
    if isinstance(cfar, dict):
        unknown = sorted(set(cfar) - set(CFAR_DEFAULTS))
        if unknown:
            raise ValueError(f"cfar: unknown key(s) {unknown}; the keys are {list(CFAR_DEFAULTS)}")
        values = [cfar.get(k, v) for k, v in CFAR_DEFAULTS.items()]
    else:
        values = list(cfar)
        if len(values) != 5:
            raise ValueError(f"cfar must hold (train_rows, train_bins, guard_rows, guard_bins, rank) (got {len(values)} values)")
    return int(values[0]), int(values[1]), int(values[2]), int(values[3]), float(values[4])


def cfar_floor(spec, train_rows: int = 8, train_bins: int = 32, guard_rows: int = 2, guard_bins: int = 8, rank: float = 0.5,
               return_ratio: bool = False, device=None):
    """A local noise floor for every cell of a spectrogram, on the device (mdc_iq_spectrogram_cfar, include/mdc.h: 2-D
    order-statistic CFAR).  spec: the (rows, nfft) float32 tensor of spectrogram (a host tensor or array is moved to the device).
    The training set of a cell is the rectangle of +-train_rows rows and +-train_bins CENTRED columns around it, cut off at the
    spectrogram's borders (the band is not circular), minus the guard rectangle of +-guard_rows and +-guard_bins, which holds
    the cell itself and keeps an emitter's own skirt out of its floor; the floor is the training set's element at position
    floor((n - 1) * rank_permille / 1000) of its ascending order, rank_permille = round(1000 * rank) -- rank 0.5 the lower
    median --, an element of the spectrogram, never an interpolation; +inf where the training set is empty.  Returns the (rows,
    nfft) float32 floor in natural positions, or with return_ratio (floor, ratio), ratio = spec / floor in one float32 division (0/0 and inf/inf: NaN, stored as
    0x7FC00000, which find_detections reads as off; x/0: +inf, on; x/inf: 0, off):
    the spectrogram in units of its local floor, which find_detections takes with cfar_threshold's plain factor.  Known limit
    (self-masking): an emitter that fills more than the share 1 - rank of its own training window lifts its own floor; at the
    defaults that is one wider than about 40 bins and on in every row of the window.  ValueError / TypeError -- before anything
    touches a device -- for a shape that is not (rows, nfft) with nfft a power of two in 64..4096, no rows, more than 2^31 - 1
    cells, parameters outside 0 <= guard_rows <= train_rows <= 16 and 0 <= guard_bins <= train_bins <= 128, a guard that is the
    whole window, or a rank outside [0, 1].  Enqueues on torch's current stream without synchronising."""
    import torch
    rows, nfft = _check_spectrogram_shape(spec)
    if rows < 1:
        raise ValueError("the spectrogram has no rows")
    if rows * nfft > _cabi.COMPONENTS_MAX_CELLS:
        raise ValueError(f"at most {_cabi.COMPONENTS_MAX_CELLS} cells (got {rows} x {nfft})")
    tr, tb, gr, gb = int(train_rows), int(train_bins), int(guard_rows), int(guard_bins)
    if not (0 <= gr <= tr <= _cabi.CFAR_MAX_TRAIN_ROWS and 0 <= gb <= tb <= _cabi.CFAR_MAX_TRAIN_BINS):
        raise ValueError(f"0 <= guard_rows <= train_rows <= {_cabi.CFAR_MAX_TRAIN_ROWS} and 0 <= guard_bins <= train_bins <= "
                         f"{_cabi.CFAR_MAX_TRAIN_BINS} (got train ({train_rows!r}, {train_bins!r}), guard ({guard_rows!r}, {guard_bins!r}))")
    if (tr, tb) == (gr, gb):
        raise ValueError(f"the guard ({gr}, {gb}) is the whole training window: no training cells")
    if not 0.0 <= float(rank) <= 1.0:      # (a NaN fails both comparisons)
        raise ValueError(f"rank must lie in [0, 1] (got {rank!r})")
    permille = int(round(1000.0 * float(rank)))
    t = _float32_tensor(spec, "spec")
    if not t.is_cuda:
        t = t.to(device if device is not None else "cuda:0")
    t = t.contiguous()
    floor = torch.empty((rows, nfft), dtype=torch.float32, device=t.device)
    ratio = torch.empty((rows, nfft), dtype=torch.float32, device=t.device) if return_ratio else None
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().mdc_iq_spectrogram_cfar(t.data_ptr(), rows, nfft, tr, tb, gr, gb, permille, floor.data_ptr(),
                                                        ratio.data_ptr() if return_ratio else None,
                                                        torch.cuda.current_stream(t.device).cuda_stream))
    return (floor, ratio) if return_ratio else floor


def cfar_threshold(nfft: int, threshold_db: float = 6.0, dc_guard: int = 1, device=None):
    """The threshold that goes with cfar_floor's ratio: an (nfft,) float32 device tensor in natural DFT order that holds
    10^(threshold_db / 10), detection_threshold's float32 factor, and +inf in the bins within dc_guard of bin 0 (both sides;
    dc_guard < 0: none), detection_threshold's rule."""
    import torch
    nfft = int(nfft)
    if not (_cabi.SPECTROGRAM_MIN_NFFT <= nfft <= _cabi.SPECTROGRAM_MAX_NFFT and nfft & (nfft - 1) == 0):
        raise ValueError(f"nfft must be a power of two in {_cabi.SPECTROGRAM_MIN_NFFT}..{_cabi.SPECTROGRAM_MAX_NFFT} (got {nfft})")
    factor = float(np.float32(10.0 ** (float(threshold_db) / 10.0)))
    if not np.isfinite(factor):
        raise ValueError(f"threshold_db must be finite (got {threshold_db!r})")
    dev = device if device is not None else "cuda:0"
    thresh = torch.full((nfft,), factor, dtype=torch.float32, device=dev)
    if int(dc_guard) >= 0:
        thresh[torch.arange(-int(dc_guard), int(dc_guard) + 1, device=dev) % nfft] = float("inf")
    return thresh


def detections_from_components(spec, thresh, records, count: int, min_rows: int = 3, min_bins: int = 3, nfft_hop=None, avg: int = 1):
    """The host half of find_detections: spectrogram_components' records -> a list of Detection(first_row, stop_row, first_bin,
    stop_bin, cells, centre, bandwidth, peak_db, snr_db, first_pair, stop_pair), ordered by (first_pair, centre); float64.
    Components whose box spans fewer than min_rows rows or min_bins bins are dropped.  first_bin / stop_bin are the box's CENTRED
    columns (half-open; column c is the frequency (c - nfft/2) / nfft), bandwidth its width / nfft.  centre: the box's columns
    are averaged over the box's rows, every column's mean is taken above thresh at that bin (below it: 0; the threshold is the
    floor of a detection) and centre is the centroid of that excess in cycles per sample -- find_emitters' centroid on the box;
    a box without excess gets its middle.  peak_db = 10 log10(peak); snr_db, the peak over the threshold AT ITS BIN in dB (add
    threshold_db for the ratio to the noise floor).  first_pair / stop_pair: burst_pairs(first_row, stop_row, nfft, nfft_hop, avg)
    -- nfft_hop (default nfft // 2) and avg are the spectrogram's.  spec, thresh: device or host; only the boxes are read."""
    from collections import namedtuple
    Detection = namedtuple("Detection", "first_row stop_row first_bin stop_bin cells centre bandwidth peak_db snr_db first_pair stop_pair")
    rows, nfft = _check_spectrogram_shape(spec)
    hop = nfft // 2 if nfft_hop is None else int(nfft_hop)
    th = np.asarray(thresh.cpu().numpy() if hasattr(thresh, "cpu") else thresh, dtype=np.float64).reshape(-1)
    if th.size != nfft:
        raise ValueError(f"thresh must hold nfft = {nfft} values (got {th.size})")
    found = []
    for rec in records[:min(int(count), len(records))]:
        r0, r1, c0, c1 = int(rec["row_first"]), int(rec["row_stop"]), int(rec["bin_first"]), int(rec["bin_stop"])
        if r1 - r0 < int(min_rows) or c1 - c0 < int(min_bins):
            continue
        cols = (np.arange(c0, c1) + nfft // 2) % nfft
        box = spec[r0:r1]
        box = box[:, cols] if not hasattr(box, "cpu") else box[:, cols.tolist()].cpu().numpy()
        mean = np.asarray(box, np.float64).mean(axis=0)
        with np.errstate(invalid="ignore"):
            excess = np.where(mean > th[cols], mean - th[cols], 0.0)
        f = (np.arange(c0, c1) - nfft // 2) / float(nfft)
        total = float(excess.sum())
        centre = float((excess * f).sum() / total) if total > 0.0 else float(f[0] + f[-1]) / 2.0
        peak = float(rec["peak"])
        at = th[(int(rec["peak_bin"]) + nfft // 2) % nfft]
        a, z = burst_pairs(r0, r1, nfft, hop, avg)
        with np.errstate(divide="ignore"):
            found.append(Detection(r0, r1, c0, c1, int(rec["cells"]), centre, float(c1 - c0) / nfft, float(10.0 * np.log10(peak)),
                                   float(10.0 * np.log10(peak / at)), a, z))
    found.sort(key=lambda d: (d.first_pair, d.centre))
    return found


def find_detections(spec, thresh, reach_rows: int = 2, reach_bins: int = 3, min_rows: int = 3, min_bins: int = 3, capacity: int = 65536,
                    nfft_hop=None, avg: int = 1):
    """Every emitter's every appearance in a spectrogram, as boxes in time and frequency: spectrogram_components(spec, thresh,
    reach_rows, reach_bins, capacity) on the device, then detections_from_components(spec, thresh, records, count, min_rows,
    min_bins, nfft_hop, avg) on the host.  A reach of g + 1 joins on-cells across g off cells, as merge_bins / merge_rows do in
    one dimension.  A hopper gives one Detection per dwell, two emitters that share bins at different times stay two, a single
    packet is one box.  ValueError if the spectrogram holds more components than capacity (both numbers are named): raise
    capacity, or the threshold."""
    _, records, count = spectrogram_components(spec, thresh, reach_rows, reach_bins, capacity)
    if count > int(capacity):
        raise ValueError(f"the spectrogram holds {count} components, capacity is {int(capacity)}: raise capacity or the threshold")
    return detections_from_components(spec, thresh, records, count, min_rows, min_bins, nfft_hop, avg)


# ---- frame synthesis (mdc_iq_synth_plan / mdc_iq_synth_frames): labelled frames of a balanced (modulation x SNR) grid ----------
RML2016_MODS = ("8PSK", "AM-DSB", "AM-SSB", "BPSK", "CPFSK", "GFSK", "PAM4", "QAM16", "QAM64", "QPSK", "WBFM")      # the dataset's order
SYNTH_NOISE_VARIANCE = 8.0 * (2 ** 32 - 1) / 12.0      # of the sum of eight uniform 16-bit integers (include/mdc.h: exact)
_SYNTH_Q = 20
_SYNTH_PEAK = 16384          # the largest component of an alphabet, and the PHASE classes' amplitude


class SynthRecipe(NamedTuple):
    """What synth_recipe designs: the tables as mdc_iq_synth_plan takes them, the plan blob, and what the design knows.
    power[k]: the exact expected |m|^2 (both components, after the mixer, before the gains) of class k; snr_exact_db[k, s]: the
    SNR the integer gains give, 10 log10 of gain_sig^2 power / (gain_noise^2 2 var(w))."""
    mods: tuple
    snrs_db: tuple
    classes: np.ndarray
    points: np.ndarray
    taps: np.ndarray
    gain_sig: np.ndarray
    gain_noise: np.ndarray
    max_step: int
    q: int
    blob: np.ndarray
    power: np.ndarray
    snr_exact_db: np.ndarray
    fading: Optional["SynthFading"] = None      # synth_fading's design: frames go through mdc_iq_synth_frames_faded


class SynthFading(NamedTuple):
    """What synth_fading designs: `record`, one _cabi.IQ_SYNTH_FADING as mdc_iq_synth_frames_faded takes it, and what the design
    knows.  path_power[p]: the exact E|g_p|^2 of path p's gain in the integer definition, in units of one (8192^2); power_sum:
    their sum, the channel's mean power gain for a signal inside `band`; delay_deviation[p]: the worst | |D_p(f)|^2 - 1 | of path
    p's quantised delay filter over |f| <= band cycles per sample."""
    record: np.ndarray
    delays: tuple
    mags: tuple
    rician_k: float
    max_doppler: float
    band: float
    path_power: tuple
    power_sum: float
    delay_deviation: tuple


def _rrc_pulse(sps: int, span: int, beta: float) -> np.ndarray:
    """Root-raised-cosine pulse, sps * span taps, unit energy."""
    n = sps * span
    t = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) / sps
    h = np.empty(n)
    for i, x in enumerate(t):
        if abs(x) < 1e-12:
            h[i] = 1.0 - beta + 4.0 * beta / np.pi
        elif beta > 0 and abs(abs(4.0 * beta * x) - 1.0) < 1e-9:
            h[i] = beta / np.sqrt(2.0) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
        else:
            h[i] = (np.sin(np.pi * x * (1 - beta)) + 4 * beta * x * np.cos(np.pi * x * (1 + beta))) / (np.pi * x * (1 - (4 * beta * x) ** 2))
    return h / np.sqrt(np.sum(h * h))


def _lowpass_pulse(sps: int, span: int, cutoff: float, kaiser_beta: float = 6.0) -> np.ndarray:
    """Kaiser-windowed sinc, sps * span taps, cutoff in cycles per sample."""
    n = sps * span
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    return 2.0 * cutoff * np.sinc(2.0 * cutoff * t) * np.kaiser(n, kaiser_beta)


def _gaussian_frequency_pulse(sps: int, span: int, bt: float) -> np.ndarray:
    """A rectangle of one symbol through a Gaussian filter of bandwidth-time product bt, sps * span taps, unit sum."""
    n = sps * span
    t = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) / sps
    sigma = np.sqrt(np.log(2.0)) / (2.0 * np.pi * bt)
    from math import erf
    g = np.array([0.5 * (erf((x + 0.5) / (np.sqrt(2.0) * sigma)) - erf((x - 0.5) / (np.sqrt(2.0) * sigma))) for x in t])
    return g / g.sum()


def _branch_abs_sum(h: np.ndarray, sps: int) -> int:
    a = np.abs(h[:, 0].astype(np.int64)) + np.abs(h[:, 1].astype(np.int64))
    return int(max(a[b::sps].sum() for b in range(sps)))


def _quantise_pulse(h, sps: int, branch_limit: float) -> np.ndarray:
    """Complex float taps -> (n, 2) int16, scaled so that the largest branch's sum of |re| + |im| is 90 % of branch_limit."""
    h = np.asarray(h, dtype=np.complex128)
    a = np.abs(h.real) + np.abs(h.imag)
    worst = max(a[b::sps].sum() for b in range(sps))
    scaled = h * (0.9 * branch_limit / worst)
    q = np.stack([np.rint(scaled.real), np.rint(scaled.imag)], axis=1)
    if np.abs(q).max() > 32767:
        q *= 32767.0 / np.abs(q).max()
        q = np.rint(q)
    return q.astype(np.int16)


def _alphabet(name: str) -> np.ndarray:
    """(M, 2) int16: the constellation at a peak component of at most _SYNTH_PEAK"""
    P = float(_SYNTH_PEAK)
    if name in ("BPSK", "CPFSK", "GFSK"):
        pts = np.array([-1.0, 1.0], np.complex128) * P
    elif name == "PAM4":
        pts = np.array([-3.0, -1.0, 1.0, 3.0], np.complex128) * (P / 3.0)
    elif name == "QPSK":
        pts = P * np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    elif name == "8PSK":
        pts = P * np.exp(1j * np.pi / 4 * np.arange(8))
    else:
        side = {"QAM16": 4, "QAM64": 8}[name]
        lv = (2.0 * np.arange(side) - (side - 1)) * (P / (side - 1))
        pts = (lv[:, None] + 1j * lv[None, :]).reshape(-1)
    return np.stack([np.rint(pts.real), np.rint(pts.imag)], axis=1).astype(np.int16)


def synth_expected_power(cls, points, taps, table=None) -> float:
    """The exact expected |m|^2 (I^2 + Q^2 after the mixer, before the gains) of one class record over the generator's draws:
    independent symbols, a uniform timing offset, uniform oscillator phases; each rounding adds 1/12 per component."""
    T = (nco_table() if table is None else np.asarray(table)).astype(np.float64)
    T2 = float(np.mean(T[:, 0] ** 2 + T[:, 1] ** 2))
    add = complex(int(cls["add_re"]), int(cls["add_im"]))
    sps, span = int(cls["sps"]), int(cls["span"])
    if int(cls["mode"]) == _cabi.SYNTH_PHASE:
        pz = float(int(cls["amplitude"])) ** 2 * T2 / 2.0 ** 30 + 1.0 / 6.0 + abs(add) ** 2
    else:
        h = np.asarray(taps, np.float64).reshape(-1, 2)[int(cls["first_tap"]):int(cls["first_tap"]) + sps * span]
        h = h[:, 0] + 1j * h[:, 1]
        if int(cls["source"]) == _cabi.SYNTH_GAUSS:
            mu, e2 = 0.0, SYNTH_NOISE_VARIANCE
        else:
            p = np.asarray(points, np.float64).reshape(-1, 2)[int(cls["first_point"]):int(cls["first_point"]) + int(cls["points"])]
            p = p[:, 0] + 1j * p[:, 1]
            mu, e2 = p.mean(), float(np.mean(np.abs(p) ** 2))
        pz = 0.0
        for b in range(sps):
            hb = h[b::sps]
            pz += (e2 - abs(mu) ** 2) * float(np.sum(np.abs(hb) ** 2)) / 2.0 ** 30 + abs(mu * hb.sum() / 2.0 ** 15 + add) ** 2
        pz = pz / sps + 1.0 / 6.0
    return pz * T2 / 2.0 ** 32 + 1.0 / 6.0


def synth_plan(classes, points, taps, gain_sig, gain_noise, max_step: int, q: int) -> np.ndarray:
    """mdc_iq_synth_plan (host code, no GPU): the plan blob of a recipe given as tables -- classes: _cabi.IQ_SYNTH_CLASS records;
    points, taps: (N, 2) int16; gain_sig: (C, S) int32; gain_noise: (S) int32.  Every refusal is a _cabi.MdcError."""
    classes = np.ascontiguousarray(classes, dtype=_cabi.IQ_SYNTH_CLASS).reshape(-1)
    points = np.ascontiguousarray(points, dtype=np.int16).reshape(-1, 2)
    taps = np.ascontiguousarray(taps, dtype=np.int16).reshape(-1, 2)
    gain_sig = np.ascontiguousarray(gain_sig, dtype=np.int32)
    gain_noise = np.ascontiguousarray(gain_noise, dtype=np.int32).reshape(-1)
    lib = _cabi.lib()
    nbytes = _cabi.check(lib.mdc_iq_synth_plan_bytes(classes.size, gain_noise.size, classes.ctypes.data))
    blob = np.empty(nbytes, np.uint8)
    _cabi.check(lib.mdc_iq_synth_plan(classes.ctypes.data, classes.size, points.ctypes.data, points.shape[0], taps.ctypes.data, taps.shape[0],
                                      gain_sig.ctypes.data, gain_sig.size, gain_noise.ctypes.data, gain_noise.size, int(max_step), int(q),
                                      blob.ctypes.data, nbytes))
    return blob


_irwin_hall = None


def _irwin_hall_pmf() -> np.ndarray:
    """P(G = v - 262140), v = 0 .. 524280: the sum of eight uniform integers on 0 .. 65535, by seven sliding-window sums."""
    global _irwin_hall
    if _irwin_hall is None:
        p = np.full(65536, 1.0 / 65536.0)
        for _ in range(7):
            c = np.concatenate([[0.0], np.cumsum(np.concatenate([p, np.zeros(65535)]))])
            p = (c[1:] - np.concatenate([np.zeros(65536), c[1:-65536]])) / 65536.0
        _irwin_hall = p
    return _irwin_hall


def synth_scatter_moments(scatter: int):
    """(E X, E X^2) of one drawn gain component X = (G scatter + 2^17) >> 18 of mdc_iq_synth_frames_faded, G the sum of eight
    uniform 16-bit integers minus 262140: summed over G's whole distribution, so the rounding shift is in it."""
    pmf = _irwin_hall_pmf()
    x = ((np.arange(pmf.size, dtype=np.int64) - _cabi.SYNTH_GAUSS_MAX) * int(scatter) + (1 << 17)) >> 18
    return float(pmf @ x), float(pmf @ (x * x).astype(np.float64))


def synth_path_power(los_re: int, los_im: int, scatter: int) -> float:
    """The exact E|g|^2 of a path's gain g = los + X (two independent components), in integer units (8192^2 is a power of one)."""
    m1, m2 = synth_scatter_moments(scatter)
    return float(los_re) ** 2 + float(los_im) ** 2 + 2.0 * m1 * (float(los_re) + float(los_im)) + 2.0 * m2


def synth_fading(delays=(0.0, 0.9, 1.7), mags=(1.0, 0.8, 0.3), rician_k: float = 4.0, ntaps: int = 8, max_doppler: float = 0.0,
                 band: float = 0.25, kaiser_beta: float = 4.0) -> SynthFading:
    """Design a frequency-selective Rician channel for mdc_iq_synth_frames_faded (include/mdc.h; numpy on the host, no GPU).
    delays: each path's delay in samples (fractions allowed, 0 <= delay <= (ntaps - 1) / 2), 1..4 paths; mags: the paths' relative
    amplitudes; rician_k: path 0's line-of-sight power over its scattered power (the other paths are all scattered: Rayleigh);
    ntaps: taps of every path's delay filter, 1..16 -- a Kaiser-windowed sinc centred at delay + (ntaps - 1) / 2, unit gain at
    DC, in Q14; max_doppler: every path's frequency offset is drawn per frame, uniformly in +-max_doppler cycles per sample (at
    most 0.25; 0: gains constant over a frame, no oscillator read).  The defaults are the delay profile of the RML2016.10a
    generator's channel.  The path powers are mags^2 scaled to sum to one; what the integers then give is reported (path_power,
    power_sum), as is each delay filter's worst deviation from unit power gain over |f| <= band (delay_deviation).  Bad
    arguments are refused by name (ValueError)."""
    delays, mags = tuple(float(d) for d in delays), tuple(float(m) for m in mags)
    P, T = len(delays), int(ntaps)
    if not 1 <= P <= _cabi.SYNTH_MAX_PATHS:
        raise ValueError(f"delays: synth_fading takes 1..{_cabi.SYNTH_MAX_PATHS} paths (got {P})")
    if len(mags) != P:
        raise ValueError(f"mags: {len(mags)} magnitudes for {P} delays")
    if not 1 <= T <= _cabi.SYNTH_MAX_DELAY_TAPS:
        raise ValueError(f"ntaps must be in 1..{_cabi.SYNTH_MAX_DELAY_TAPS} (got {ntaps})")
    for d in delays:
        if not 0.0 <= d <= (T - 1) / 2.0:
            raise ValueError(f"delays: {d} is outside 0..{(T - 1) / 2.0}, what {T} taps can centre")
    for m in mags:
        if not (np.isfinite(m) and m > 0.0):
            raise ValueError(f"mags: every magnitude must be positive and finite (got {m})")
    if not (np.isfinite(rician_k) and rician_k >= 0.0):
        raise ValueError(f"rician_k must be >= 0 and finite (got {rician_k})")
    if not 0.0 <= max_doppler <= 0.25:
        raise ValueError(f"max_doppler must be in 0..0.25 cycles per sample (got {max_doppler})")
    if not 0.0 < band <= 0.5:
        raise ValueError(f"band must be in (0, 0.5] cycles per sample (got {band})")
    rec = np.zeros(1, _cabi.IQ_SYNTH_FADING)
    rec["paths"], rec["taps"], rec["max_doppler_step"] = P, T, int(round(max_doppler * 2.0 ** 32))
    share = np.asarray(mags) ** 2 / np.sum(np.asarray(mags) ** 2)
    one, sigma_g = float(_cabi.SYNTH_FADING_GAIN_ONE), np.sqrt(SYNTH_NOISE_VARIANCE)
    f = np.linspace(-band, band, 257)
    k = np.arange(T, dtype=np.float64)
    powers, deviations = [], []
    for p in range(P):
        path = rec["path"][0][p]
        h = np.sinc(k - (T - 1) / 2.0 - delays[p]) * np.kaiser(T, kaiser_beta) if T > 1 else np.ones(1)
        d = np.rint(h / h.sum() * _cabi.SYNTH_FADING_TAP_ONE).astype(np.int64)
        if np.abs(d).sum() > _cabi.SYNTH_FADING_MAX_ABS_SUM:
            raise ValueError(f"delays: path {p}'s delay filter sums to {int(np.abs(d).sum())} in absolute value, more than "
                             f"{_cabi.SYNTH_FADING_MAX_ABS_SUM}: use fewer taps or a larger kaiser_beta")
        path["delay_taps"][:T] = d
        gain = np.abs(np.exp(-2j * np.pi * f[:, None] * k[None, :]) @ (d / float(_cabi.SYNTH_FADING_TAP_ONE))) ** 2
        deviations.append(float(np.abs(gain - 1.0).max()))
        los_power = share[p] * rician_k / (rician_k + 1.0) if p == 0 else 0.0
        los = int(round(one * np.sqrt(los_power)))
        scatter = int(round(one * np.sqrt((share[p] - los_power) / 2.0) * 2.0 ** 18 / sigma_g))
        if los + scatter > 32767:
            raise ValueError(f"mags: path {p}'s gain needs |los| + scatter = {los} + {scatter}, more than 32767")
        path["los_re"], path["scatter"] = los, scatter
        powers.append(synth_path_power(los, 0, scatter) / one ** 2)
    return SynthFading(rec, delays, mags, float(rician_k), float(max_doppler), float(band), tuple(powers), float(sum(powers)), tuple(deviations))


def synth_recipe(mods=RML2016_MODS, snrs_db=range(-20, 20, 2), sps: int = 8, beta: float = 0.35, span: int = 8, rms: float = 2048.0,
                 max_cfo: float = 0.01, fsk_index: float = 0.5, gfsk_bt: float = 0.35, fm_deviation: float = 0.08,
                 am_carrier: int = 12000, fading: Optional[SynthFading] = None) -> SynthRecipe:
    """Design the recipe of a balanced (modulation x SNR) grid of synthesised frames (include/mdc.h, "frame synthesis"; numpy on the
    host, no GPU).  mods: names out of RML2016_MODS, an unknown one is refused by name; snrs_db: the grid's SNR values; sps: samples
    per symbol (for the analogue classes: per source sample); beta, span: the root-raised-cosine pulse of the linear classes (the
    low-passes and the Gaussian frequency pulse are span symbols long too; CPFSK's rectangle is one); rms: the complex rms of
    signal PLUS noise at every SNR, in int16 units (2048: -24 dBFS, the noise's 4.9 sigma far below the rails); max_cfo: the carrier
    offset is drawn uniformly in +-max_cfo cycles per sample; fsk_index: modulation index of CPFSK / GFSK; gfsk_bt: GFSK's
    bandwidth-time product; fm_deviation: WBFM's rms frequency deviation, cycles per sample; am_carrier: AM-DSB's carrier against
    a message of 4.9 sigma <= 32767 - am_carrier.  Gains are designed from each class's exact expected power (synth_expected_power),
    so 10 log10(P_sig / P_noise) is the nominal SNR up to the gains' rounding (SynthRecipe.snr_exact_db).  fading: a SynthFading
    of synth_fading, or None: with one, synth_frames and synth_dataset send every frame through that channel
    (mdc_iq_synth_frames_faded) between the mixer and the gains; the tables and the plan blob are the same either way, and the
    nominal SNR is then the average over the fading (the channel's mean power gain is fading.power_sum, one by design)."""
    if fading is not None and not isinstance(fading, SynthFading):
        raise TypeError("fading must be a SynthFading (synth_fading) or None")
    mods = tuple(mods)
    snrs = tuple(snrs_db)
    for m in mods:
        if m not in RML2016_MODS:
            raise ValueError(f"unknown modulation {m!r}: synth_recipe designs {', '.join(RML2016_MODS)}")
    if not mods or not snrs:
        raise ValueError("synth_recipe needs at least one modulation and one SNR")
    sps, span = int(sps), int(span)
    if not 0.0 <= max_cfo <= 0.25:
        raise ValueError("max_cfo must be in 0..0.25 cycles per sample")
    G = _cabi.SYNTH_GAUSS_MAX
    classes = np.zeros(len(mods), _cabi.IQ_SYNTH_CLASS)
    points, taps = [], []
    npoints = ntaps = 0
    for k, m in enumerate(mods):
        c = classes[k]
        c["sps"], c["span"], c["first_point"], c["first_tap"] = sps, span, npoints, ntaps
        if m in ("AM-DSB", "AM-SSB", "WBFM"):
            c["source"], c["points"] = _cabi.SYNTH_GAUSS, 0
            add = int(am_carrier) if m == "AM-DSB" else 0
            limit = (32767 - add) * 32768.0 / G
            cutoff = 0.4 / sps
            h = _lowpass_pulse(sps, span, cutoff).astype(np.complex128)
            if m == "AM-SSB":      # the analytic low-pass: the pass band moved to 0 .. 2 cutoff (the upper sideband)
                h = h * np.exp(2j * np.pi * cutoff * (np.arange(h.size) - (h.size - 1) / 2.0))
            hq = _quantise_pulse(h, sps, limit)
            if m == "WBFM":
                c["mode"], c["amplitude"] = _cabi.SYNTH_PHASE, _SYNTH_PEAK
                hf = hq[:, 0].astype(np.float64)
                y_rms = np.sqrt(SYNTH_NOISE_VARIANCE * np.mean([np.sum(hf[b::sps] ** 2) for b in range(sps)])) / 32768.0
                c["phase_factor"] = int(round(fm_deviation * 2.0 ** 32 / y_rms))
            else:
                c["mode"], c["add_re"] = _cabi.SYNTH_LINEAR, add
        else:
            a = _alphabet(m)
            c["source"], c["points"] = _cabi.SYNTH_ALPHABET, a.shape[0]
            points.append(a)
            npoints += a.shape[0]
            amax = int(np.abs(a.astype(np.int64)).max())
            if m in ("CPFSK", "GFSK"):
                # y = +-amax / 2 while the pulse is a rectangle: pi fsk_index per symbol is an increment of fsk_index 2^31 / sps per sample
                c["mode"], c["amplitude"] = _cabi.SYNTH_PHASE, _SYNTH_PEAK
                if m == "CPFSK":
                    c["span"] = 1
                    hq = np.stack([np.full(sps, 16384, np.int16), np.zeros(sps, np.int16)], axis=1)
                else:
                    g = _gaussian_frequency_pulse(sps, span, gfsk_bt) * (sps * 16384.0)
                    hq = np.stack([np.rint(g), np.zeros(g.size)], axis=1).astype(np.int16)
                c["phase_factor"] = int(round(fsk_index * 2.0 ** 31 / sps / (amax / 2.0)))
            else:
                c["mode"] = _cabi.SYNTH_LINEAR
                hq = _quantise_pulse(_rrc_pulse(sps, span, beta), sps, 32767 * 32768.0 / amax)
        taps.append(hq)
        ntaps += hq.shape[0]
    points_a = np.concatenate(points) if points else np.zeros((0, 2), np.int16)
    taps_a = np.concatenate(taps)
    table = nco_table()
    power = np.array([synth_expected_power(classes[k], points_a, taps_a, table) for k in range(len(mods))])
    q = _SYNTH_Q
    lin = 10.0 ** (np.asarray(snrs, np.float64) / 10.0)
    p_sig, p_noise = float(rms) ** 2 * lin / (1.0 + lin), float(rms) ** 2 / (1.0 + lin)
    gs = np.rint(2.0 ** q * np.sqrt(p_sig[None, :] / power[:, None]))
    gn = np.rint(2.0 ** q * np.sqrt(p_noise / (2.0 * SYNTH_NOISE_VARIANCE)))
    if gs.max() > 2 ** 31 - 1 or gn.max() > 2 ** 31 - 1:
        raise ValueError("rms is too large for the gains' int32")
    gain_sig, gain_noise = gs.astype(np.int32), gn.astype(np.int32)
    max_step = int(round(max_cfo * 2.0 ** 32))
    blob = synth_plan(classes, points_a, taps_a, gain_sig, gain_noise, max_step, q)
    with np.errstate(divide="ignore"):
        exact = 10.0 * np.log10(gs ** 2 * power[:, None] / (gn[None, :] ** 2 * 2.0 * SYNTH_NOISE_VARIANCE))
    return SynthRecipe(mods, snrs, classes, points_a, taps_a, gain_sig, gain_noise, max_step, q, blob, power, exact, fading)


def _synth_blob(recipe) -> np.ndarray:
    return np.ascontiguousarray(recipe.blob if isinstance(recipe, SynthRecipe) else recipe, dtype=np.uint8)


def synth_frames(n: int, recipe, seed: int = 2016, first_frame: int = 0, device=None, return_saturated: bool = False):
    """n labelled frames of a recipe of synth_recipe, made on the device in one launch (mdc_iq_synth_frames, or
    mdc_iq_synth_frames_faded when the recipe carries a fading design): frame i is the grid's
    frame first_frame + i -- a function of (recipe, seed, that index) alone, so calls can be split, repeated and resumed bit for
    bit; class = index mod C, SNR entry = (index / C) mod S.  Returns (iq, labels, snr_db): the (n, 256) int16 device tensor of
    interleaved (I, Q) samples -- reshape(-1) is an ordinary "ci16" capture --, the int32 class indices and each frame's SNR
    value (int32 when the recipe's SNRs are whole numbers, else float32); with return_saturated also the number of components the
    final clamp changed (one synchronising read).  Enqueues on torch's current stream."""
    import torch
    if not isinstance(recipe, SynthRecipe):
        raise TypeError("recipe must be a SynthRecipe (synth_recipe)")
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    blob = _synth_blob(recipe)
    iq = torch.empty((n, 2 * HOP_FRAME), dtype=torch.int16, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    snr_index = torch.empty((n,), dtype=torch.int32, device=dev)
    sat = torch.zeros((1,), dtype=torch.int64, device=dev) if return_saturated else None
    plan_dev = torch.from_numpy(blob).to(dev)
    args = (blob.ctypes.data, plan_dev.data_ptr(), blob.size, int(seed) % (1 << 64), int(first_frame) % (1 << 64), n, iq.data_ptr() if n else None,
            labels.data_ptr() if n else None, snr_index.data_ptr() if n else None, sat.data_ptr() if sat is not None else None)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if recipe.fading is None:
            _cabi.check(_cabi.lib().mdc_iq_synth_frames(*args, stream))
        else:
            record = np.ascontiguousarray(recipe.fading.record, dtype=_cabi.IQ_SYNTH_FADING)
            _cabi.check(_cabi.lib().mdc_iq_synth_frames_faded(*args, record.ctypes.data, stream))
    whole = all(float(s) == int(s) for s in recipe.snrs_db)
    values = torch.tensor([int(s) if whole else float(s) for s in recipe.snrs_db], dtype=torch.int32 if whole else torch.float32, device=dev)
    snr_db = values[snr_index.long()]
    return (iq, labels, snr_db, int(sat.item())) if return_saturated else (iq, labels, snr_db)


def synth_dataset(n: int, recipe, seed: int = 2016, level: float = DEFAULT_LEVEL, first_frame: int = 0, device=None):
    """synth_frames through the library's normaliser (normalized_frames_from_iq at hop 128: DC removal, complex rms `level`):
    (X float32 (n, 2, 128), labels int32, snr_db) on the device, ready for VTCNN2.fit / evaluate / confusion / accuracy_by_snr --
    what cnn.py:42-82 selects from RML2016.10a_dict.pkl, whose vectors are energy-normalised too."""
    iq, labels, snr_db = synth_frames(n, recipe, seed=seed, first_frame=first_frame, device=device)
    if int(n) == 0:
        import torch
        return torch.empty((0, 2, HOP_FRAME), dtype=torch.float32, device=iq.device), labels, snr_db
    return normalized_frames_from_iq(iq.reshape(-1), "ci16", level=level, hop=HOP_FRAME), labels, snr_db


# ---- capture synthesis (mdc_iq_synth_scene / mdc_iq_synth_capture): a scene of emitters rendered into one wideband capture ------
class SynthScene(NamedTuple):
    """What synth_scene designs: the emitter records and the tap array as mdc_iq_synth_scene takes them, the scene blob, and what
    the design knows.  Per emitter: mods (the class's name), centres (a tuple of up to 8, cycles per capture sample), bandwidth
    (cycles per capture sample), rms (the exact expected complex rms while on, from the integer gain and the recipe's exact
    power), level_db (that rms against the noise inside the bandwidth; +inf without noise), passband_deviation (the worst
    | |H(f)|^2 - 1 | of the interpolation filter over the class's band).  noise_rms: what the integer gain_noise gives."""
    recipe: "SynthRecipe"
    emitters: np.ndarray
    taps: np.ndarray
    gain_noise: int
    q: int
    dc: tuple
    blob: np.ndarray
    mods: tuple
    centres: tuple
    bandwidth: tuple
    rms: tuple
    level_db: tuple
    passband_deviation: tuple
    noise_rms: float


SCENE_TRUTH = np.dtype([("emitter", np.int32), ("mod", "U16"), ("label", np.int32), ("dwell", np.int64), ("first_pair", np.int64),
                        ("stop_pair", np.int64), ("centre", np.float64), ("bandwidth", np.float64), ("level_db", np.float64),
                        ("whole", np.bool_)])


def synth_class_bandwidth(recipe, k: int) -> float:
    """The occupied (two-sided) bandwidth of class k of a recipe, in cycles per BASEBAND sample.  LINEAR classes: the band around
    the pulse's spectral centroid that holds 99 % of the pulse's energy (a root-raised-cosine of roll-off beta gives about (1 +
    beta / 2) / sps).  PHASE classes: Carson's rule, 2 (deviation + the pulse's own 99 % half band), the deviation being
    phase_factor times the largest |y| an alphabet gives (two standard deviations of y for a Gaussian source)."""
    c = recipe.classes[k]
    sps, span = int(c["sps"]), int(c["span"])
    h = recipe.taps[int(c["first_tap"]):int(c["first_tap"]) + sps * span].astype(np.float64)
    h = h[:, 0] + 1j * h[:, 1]
    N = 4096
    p = np.abs(np.fft.fftshift(np.fft.fft(h, N))) ** 2
    f = (np.arange(N) - N // 2) / float(N)
    centroid = int(np.clip(round(float(np.sum(f * p) / p.sum()) * N) + N // 2, 0, N - 1))
    half = 0
    while half < N // 2 and p[max(centroid - half, 0):centroid + half + 1].sum() < 0.99 * p.sum():
        half += 1
    own = (2 * half + 1) / float(N)
    if int(c["mode"]) != _cabi.SYNTH_PHASE:
        return min(own, 1.0)
    branch = max(float(np.abs(h[b::sps]).sum()) for b in range(sps)) / 32768.0
    if int(c["source"]) == _cabi.SYNTH_GAUSS:
        y = 2.0 * np.sqrt(SYNTH_NOISE_VARIANCE * np.mean([np.sum(np.abs(h[b::sps]) ** 2) for b in range(sps)])) / 32768.0
    else:
        pts = recipe.points[int(c["first_point"]):int(c["first_point"]) + int(c["points"])].astype(np.float64)
        y = float(np.abs(pts[:, 0]).max()) * branch
    return min(2.0 * (abs(int(c["phase_factor"])) * y / 2.0 ** 32 + own / 2.0), 1.0)


def _scene_ratio(target: float):
    """(L, D) with 1 <= D <= L <= 32 closest to target = L / D (ties: the smaller L)"""
    best = None
    for L in range(1, _cabi.SYNTH_SCENE_MAX_INTERPOLATE + 1):
        for D in range(1, L + 1):
            if np.gcd(L, D) == 1:
                err = abs(L / D - target)
                if best is None or err < best[0] - 1e-15:
                    best = (err, L, D)
    return best[1], best[2]


def synth_scene(recipe, emitters, noise_rms: float, q: int = _SYNTH_Q, dc=(0, 0)) -> SynthScene:
    """Design a scene for synth_capture (include/mdc.h, "capture synthesis"; numpy on the host, no GPU).  recipe: a SynthRecipe;
    emitters: up to 32 mappings with
      mod                 a name in recipe.mods
      samples_per_symbol  capture samples per symbol (>= the recipe's sps), met by the closest L / D with D <= L <= 32 -- or
      interpolate, decimate   L and D themselves (capture samples per symbol = sps L / D)
      centre              cycles per capture sample in [-0.5, 0.5], or a sequence of up to 8 for a hopper (needs period)
      level_db            the emitter's power while on against the scene's noise INSIDE the emitter's bandwidth, in dB -- or
      rms                 its complex rms while on, in int16 units
      start, on, period   the burst schedule in CAPTURE samples (default 0, 0, 0: always on), each converted to baseband samples
                          by D / L and rounded to the nearest (an on > 0 stays >= 1)
      phase0              the carrier's 32-bit phase at capture sample 0 (default 0)
    noise_rms: the complex rms of the scene's noise in int16 units (0: none; level_db then needs rms instead).  Filters are
    design_resampler(L, D) (L == 1: the single tap 32767); equal ones are stored once.  Gains come from recipe.power[class], the
    exact expectation; the scene reports what the rounded integers give.  Bad arguments are refused by name (ValueError)."""
    if not isinstance(recipe, SynthRecipe):
        raise TypeError("recipe must be a SynthRecipe (synth_recipe)")
    emitters = list(emitters)
    if len(emitters) > _cabi.SYNTH_SCENE_MAX_EMITTERS:
        raise ValueError(f"emitters: a scene holds at most {_cabi.SYNTH_SCENE_MAX_EMITTERS} (got {len(emitters)})")
    noise_rms, q = float(noise_rms), int(q)
    if not (np.isfinite(noise_rms) and noise_rms >= 0.0):
        raise ValueError(f"noise_rms must be >= 0 and finite (got {noise_rms})")
    if not 1 <= q <= _cabi.SYNTH_MAX_Q:
        raise ValueError(f"q must be in 1..{_cabi.SYNTH_MAX_Q} (got {q})")
    dc = (int(dc[0]), int(dc[1]))
    if not all(-32768 <= v <= 32767 for v in dc):
        raise ValueError(f"dc must fit int16 (got {dc})")
    gn = int(round(2.0 ** q * noise_rms / np.sqrt(2.0 * SYNTH_NOISE_VARIANCE)))
    if gn > 2 ** 31 - 1:
        raise ValueError("noise_rms is too large for the gain's int32 at this q")
    noise_exact = gn * np.sqrt(2.0 * SYNTH_NOISE_VARIANCE) / 2.0 ** q
    rec = np.zeros(len(emitters), _cabi.IQ_SYNTH_EMITTER)
    filters, taps, ntaps = {}, [], 0
    mods, centres, bws, rmss, levels, devs = [], [], [], [], [], []
    known = {"mod", "samples_per_symbol", "interpolate", "decimate", "centre", "level_db", "rms", "start", "on", "period", "phase0"}
    for k, em in enumerate(emitters):
        who = f"emitter {k}"
        unknown = set(em) - known
        if unknown:
            raise ValueError(f"{who}: unknown key(s) {sorted(unknown)}")
        if em.get("mod") not in recipe.mods:
            raise ValueError(f"{who}: mod {em.get('mod')!r} is not in the recipe ({', '.join(recipe.mods)})")
        cls = recipe.mods.index(em["mod"])
        sps = int(recipe.classes[cls]["sps"])
        if "samples_per_symbol" in em:
            if "interpolate" in em or "decimate" in em:
                raise ValueError(f"{who}: give samples_per_symbol or (interpolate, decimate), not both")
            target = float(em["samples_per_symbol"]) / sps
            if not 1.0 <= target <= _cabi.SYNTH_SCENE_MAX_INTERPOLATE:
                raise ValueError(f"{who}: samples_per_symbol must be in {sps}..{sps * _cabi.SYNTH_SCENE_MAX_INTERPOLATE} (got {em['samples_per_symbol']})")
            L, D = _scene_ratio(target)
        else:
            L, D = int(em.get("interpolate", 1)), int(em.get("decimate", 1))
            if not 1 <= L <= _cabi.SYNTH_SCENE_MAX_INTERPOLATE:
                raise ValueError(f"{who}: interpolate must be in 1..{_cabi.SYNTH_SCENE_MAX_INTERPOLATE} (got {L})")
            if not 1 <= D <= L:
                raise ValueError(f"{who}: decimate must be in 1..interpolate = {L} (got {D})")
        if (L, D) not in filters:
            h = np.array([32767], np.int16) if L == 1 else design_resampler(L, D)
            filters[L, D] = (ntaps, h)
            taps.append(h)
            ntaps += h.size
        first_tap, h = filters[L, D]
        cs = em.get("centre", 0.0)
        cs = tuple(float(c) for c in (cs if isinstance(cs, (tuple, list, np.ndarray)) else (cs,)))
        if not 1 <= len(cs) <= _cabi.SYNTH_SCENE_MAX_HOPS:
            raise ValueError(f"{who}: centre takes 1..{_cabi.SYNTH_SCENE_MAX_HOPS} carriers (got {len(cs)})")
        for c in cs:
            if not -0.5 <= c <= 0.5:
                raise ValueError(f"{who}: centre {c} is outside [-0.5, 0.5] cycles per sample")
        sched = []
        for name in ("start", "on", "period"):
            v = float(em.get(name, 0))
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{who}: {name} must be >= 0 (got {em.get(name)})")
            b = int(round(v * D / L))
            sched.append(max(b, 1) if v > 0 and name != "start" else b)
        if len(cs) > 1 and sched[2] == 0:
            raise ValueError(f"{who}: a hopper ({len(cs)} centres) needs a period > 0: a dwell is one period")
        bw = synth_class_bandwidth(recipe, cls) * D / L
        power = float(recipe.power[cls])
        if ("level_db" in em) == ("rms" in em):
            raise ValueError(f"{who}: give level_db or rms (one of them)")
        if "rms" in em:
            rms = float(em["rms"])
        else:
            if gn == 0:
                raise ValueError(f"{who}: level_db is relative to the scene's noise, which is 0: give rms")
            rms = noise_exact * np.sqrt(min(bw, 1.0) * 10.0 ** (float(em["level_db"]) / 10.0))
        if not (np.isfinite(rms) and rms >= 0):
            raise ValueError(f"{who}: rms must be >= 0 and finite (got {rms})")
        gain = int(round(2.0 ** q * rms / np.sqrt(power)))
        if gain > 2 ** 31 - 1:
            raise ValueError(f"{who}: the level needs a gain beyond int32 at q = {q}")
        r = rec[k]
        r["cls"], r["interpolate"], r["decimate"], r["first_tap"], r["ntaps"], r["gain"] = cls, L, D, first_tap, h.size, gain
        r["phase0"], r["hops"] = int(em.get("phase0", 0)) % (1 << 32), len(cs)
        r["phase_step"][:len(cs)] = [phase_step(c) for c in cs]
        r["start"], r["on"], r["period"] = sched
        exact = gain * np.sqrt(power) / 2.0 ** q
        f = np.linspace(-0.5, 0.5, 129) * synth_class_bandwidth(recipe, cls) / L      # the class's band at the interpolated rate
        H = np.exp(-2j * np.pi * f[:, None] * np.arange(h.size)[None, :]) @ (h.astype(np.float64) / (32768.0 * L))
        mods.append(em["mod"])
        centres.append(cs)
        bws.append(bw)
        rmss.append(exact)
        with np.errstate(divide="ignore"):
            levels.append(float(10.0 * np.log10(exact ** 2 / (noise_exact ** 2 * min(bw, 1.0)))) if gn and exact > 0 else float("inf") if exact > 0 else float("-inf"))
        devs.append(float(np.abs(np.abs(H) ** 2 - 1.0).max()))
    taps_a = np.concatenate(taps) if taps else np.zeros(0, np.int16)
    blob = synth_scene_blob(recipe.blob, rec, taps_a, gn, q, dc)
    return SynthScene(recipe, rec, taps_a, gn, q, dc, blob, tuple(mods), tuple(centres), tuple(bws), tuple(rmss), tuple(levels), tuple(devs),
                      float(noise_exact))


def synth_scene_blob(plan_blob, emitters, taps, gain_noise: int, q: int, dc=(0, 0)) -> np.ndarray:
    """mdc_iq_synth_scene (host code, no GPU): the scene blob of emitter records (_cabi.IQ_SYNTH_EMITTER) and an int16 tap array,
    validated against the plan blob they index.  Every refusal is a _cabi.MdcError that names the emitter."""
    plan_blob = np.ascontiguousarray(plan_blob, dtype=np.uint8)
    emitters = np.ascontiguousarray(emitters, dtype=_cabi.IQ_SYNTH_EMITTER).reshape(-1)
    taps = np.ascontiguousarray(taps, dtype=np.int16).reshape(-1)
    lib = _cabi.lib()
    nbytes = max(_cabi.check(lib.mdc_iq_synth_scene_bytes(min(emitters.size, _cabi.SYNTH_SCENE_MAX_EMITTERS), taps.size)), 0)
    blob = np.empty(nbytes, np.uint8)
    _cabi.check(lib.mdc_iq_synth_scene(plan_blob.ctypes.data, plan_blob.size, emitters.ctypes.data, emitters.size, taps.ctypes.data, taps.size,
                                       int(gain_noise), int(q), int(dc[0]), int(dc[1]), blob.ctypes.data, nbytes))
    return blob


def synth_scene_hops(scene, seed: int, emitter: int, first_dwell: int, n: int) -> np.ndarray:
    """mdc_iq_synth_scene_hops (host code, no GPU): the hop indices of dwells first_dwell .. first_dwell + n - 1 of an emitter."""
    blob = np.ascontiguousarray(scene.blob if isinstance(scene, SynthScene) else scene, dtype=np.uint8)
    out = np.empty(int(n), np.int32)
    _cabi.check(_cabi.lib().mdc_iq_synth_scene_hops(blob.ctypes.data, blob.size, int(seed) % (1 << 64), int(emitter), int(first_dwell), int(n),
                                                    out.ctypes.data))
    return out


def synth_capture(n_pairs: int, scene, seed: int = 2016, device=None, return_saturated: bool = False):
    """The first n_pairs pairs of a scene of synth_scene, rendered on the device (mdc_iq_synth_capture): a flat int16 device tensor
    of 2 n_pairs interleaved (I, Q) samples, an ordinary "ci16" capture for scan_iq / detect_iq / spectrogram.  A function of
    (scene, seed) alone; a shorter capture is a prefix of a longer one, bit for bit.  With return_saturated also the number of
    components a clamp changed (one synchronising read).  Enqueues on torch's current stream."""
    import torch
    if not isinstance(scene, SynthScene):
        raise TypeError("scene must be a SynthScene (synth_scene)")
    n = int(n_pairs)
    if n < 0:
        raise ValueError("n_pairs must be >= 0")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    blob, plan = np.ascontiguousarray(scene.blob, dtype=np.uint8), _synth_blob(scene.recipe)
    lib = _cabi.lib()
    wbytes = _cabi.check(lib.mdc_iq_synth_capture_workspace_bytes(blob.ctypes.data, blob.size, n))
    out = torch.empty((2 * n,), dtype=torch.int16, device=dev)
    work = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=dev)
    sat = torch.zeros((1,), dtype=torch.int64, device=dev) if return_saturated else None
    scene_dev, plan_dev = torch.from_numpy(blob).to(dev), torch.from_numpy(plan).to(dev)
    with torch.cuda.device(dev):
        _cabi.check(lib.mdc_iq_synth_capture(blob.ctypes.data, scene_dev.data_ptr(), blob.size, plan.ctypes.data, plan_dev.data_ptr(), plan.size,
                                             int(seed) % (1 << 64), n, out.data_ptr() if n else None, sat.data_ptr() if sat is not None else None,
                                             work.data_ptr(), wbytes, torch.cuda.current_stream(dev).cuda_stream))
    return (out, int(sat.item())) if return_saturated else out


def scene_pair(i, interpolate: int, decimate: int, ntaps: int):
    """The capture pair on which baseband sample i of an emitter is centred (include/mdc.h: the interpolation filter's centre,
    (ntaps - 1) / 2 interpolated samples): floor((2 i L - (T - 1) + D) / (2 D)), rounded half up, clamped at 0."""
    i = np.asarray(i, np.int64)
    return np.maximum((2 * i * int(interpolate) - (int(ntaps) - 1) + int(decimate)) // (2 * int(decimate)), 0)


def scene_truth(scene, n_pairs: int, seed: int = 2016) -> np.ndarray:
    """What a capture of synth_capture(n_pairs, scene, seed) holds (host only, no GPU): one SCENE_TRUTH record per (emitter, dwell)
    whose on-time meets the capture -- emitter, mod, label (the class index), dwell, [first_pair, stop_pair) (clipped to the
    capture), centre (the dwell's carrier: the hop draws are mdc_iq_synth_scene_hops'), bandwidth (cycles per capture sample,
    synth_class_bandwidth at the emitter's rate), level_db, and whole: the dwell's on-time ends inside the capture.  An emitter
    without a period has one record.  Baseband indices become capture pairs by scene_pair: a burst is on from the pair its
    first baseband sample is centred on up to (not including) the pair its first off sample is centred on; the filter's and the
    pulse's tails reach further on both sides."""
    if not isinstance(scene, SynthScene):
        raise TypeError("scene must be a SynthScene (synth_scene)")
    n = int(n_pairs)
    rows = []
    for k, em in enumerate(scene.emitters):
        L, D, T = int(em["interpolate"]), int(em["decimate"]), int(em["ntaps"])
        start, on, period = int(em["start"]), int(em["on"]), int(em["period"])
        count = ((n - 1) * D + T - 1) // L + 1 if n > 0 else 0          # baseband samples the capture reads
        if count <= start:
            continue
        if period == 0:
            dwells, first, stop = np.zeros(1, np.int64), np.array([start], np.int64), np.array([start + on if on else -1], np.int64)
        else:
            if on == 0:
                continue
            dwells = np.arange((count - 1 - start) // period + 1, dtype=np.int64)
            first = start + dwells * period
            stop = first + min(on, period)
        first_pair = scene_pair(first, L, D, T)
        stop_pair = np.where(stop < 0, n + 1, scene_pair(np.maximum(stop, 0), L, D, T))
        whole = stop_pair <= n
        keep = (first_pair < n) & (np.minimum(stop_pair, n) > first_pair)
        hops = synth_scene_hops(scene, seed, k, 0, dwells.size) if int(em["hops"]) > 1 else np.zeros(dwells.size, np.int32)
        for j in np.flatnonzero(keep):
            rows.append((k, scene.mods[k], int(em["cls"]), int(dwells[j]), int(first_pair[j]), int(min(stop_pair[j], n)),
                         scene.centres[k][int(hops[j])], scene.bandwidth[k], scene.level_db[k], bool(whole[j])))
    return np.array(rows, dtype=SCENE_TRUTH)


def score_detections(records, truth, min_overlap: float = 0.5, classes=None):
    """Score detect_iq's records against scene_truth's (host code, numpy only).  A truth dwell is FOUND when some detection's
    [first_pair, stop_pair) covers at least min_overlap of the dwell's pairs and the detection's centre lies inside the dwell's
    band, |centre - truth centre| <= bandwidth / 2 (frequencies compared modulo one cycle per sample).  A detection that finds no
    dwell is FALSE.  Returns a dict: found (pairs (truth index, detection index): per dwell the matching detection with the
    largest overlap), missed (truth indices), false (detection indices), and confusion, an integer matrix [truth label, detected
    label] over the found pairs whose detection has a label >= 0 (classes rows and columns; default: the largest label + 1),
    with accuracy, its trace over its sum (nan when empty)."""
    truth = np.asarray(truth, dtype=SCENE_TRUTH)
    recs = list(records)
    if not 0.0 < float(min_overlap) <= 1.0:
        raise ValueError(f"min_overlap must be in (0, 1] (got {min_overlap})")
    d_first = np.array([int(r["first_pair"]) for r in recs], np.int64)
    d_stop = np.array([int(r["stop_pair"]) for r in recs], np.int64)
    d_centre = np.array([float(r["centre"]) for r in recs], np.float64)
    d_label = np.array([int(r.get("label", -1)) for r in recs], np.int64)
    found, missed, matched = [], [], np.zeros(len(recs), bool)
    for t, row in enumerate(truth):
        length = int(row["stop_pair"] - row["first_pair"])
        overlap = np.minimum(d_stop, row["stop_pair"]) - np.maximum(d_first, row["first_pair"])
        df = np.abs((d_centre - row["centre"] + 0.5) % 1.0 - 0.5)
        ok = (overlap >= min_overlap * length) & (overlap > 0) & (df <= row["bandwidth"] / 2.0)
        matched |= ok
        if ok.any():
            found.append((t, int(np.flatnonzero(ok)[np.argmax(overlap[ok])])))
        else:
            missed.append(t)
    labels = [int(truth["label"][t]) for t, d in found] + [int(d_label[d]) for t, d in found]
    C = int(classes) if classes is not None else (max(labels) + 1 if labels else 0)
    confusion = np.zeros((C, C), np.int64)
    for t, d in found:
        if 0 <= d_label[d] < C and 0 <= truth["label"][t] < C:
            confusion[int(truth["label"][t]), int(d_label[d])] += 1
    total = int(confusion.sum())
    return dict(found=found, missed=missed, false=[int(i) for i in np.flatnonzero(~matched)], confusion=confusion,
                accuracy=float(np.trace(confusion)) / total if total else float("nan"))
