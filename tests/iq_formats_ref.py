"""numpy restatement of mdc_iq_windows / mdc_iq_windows_norm (include/mdc.h) for the three integer sample formats: the
definition the tests hold the kernels to.  Statistics in int64 (exact: E <= 2^45), frames in float64 from the header's
formula; nothing of the package is imported.

    format   integer sample s        full-scale amplitude A     dtype
    "cu8"    2*byte - 255            255                        uint8
    "ci8"    the int8 value          128                        int8
    "ci16"   the int16 value         32768                      int16 (little-endian)
    sum_i, sum_q = sum of s over the window's I / Q samples;  sum_sq = sum of s_I^2 + s_Q^2
    E = 128*sum_sq - sum_i^2 - sum_q^2 (remove_dc)  |  128*sum_sq
    a = s - sum/128 (remove_dc)  |  s;      x = a * (128*level / sqrt(E)),   all zeros where E == 0
    plain conversion: s * scale ("cu8": (byte - 127.5) * scale), in float32
"""
import numpy as np

FORMATS = {"cu8": 0, "ci8": 1, "ci16": 2}
DTYPE = {"cu8": np.dtype(np.uint8), "ci8": np.dtype(np.int8), "ci16": np.dtype("<i2")}
PAIR_BYTES = {"cu8": 2, "ci8": 2, "ci16": 4}
AMPLITUDE = {"cu8": 255, "ci8": 128, "ci16": 32768}
SAMPLE_MIN = {"cu8": 0, "ci8": -128, "ci16": -32768}          # of the stored value
SAMPLE_MAX = {"cu8": 255, "ci8": 127, "ci16": 32767}
STATS64_DTYPE = np.dtype([("sum_i", np.int64), ("sum_q", np.int64), ("sum_sq", np.uint64), ("energy", np.uint64)])
# the header's bounds: |sum|, sum_sq, E
BOUNDS = {"cu8": (32640, 16646400, 2130739200), "ci8": (1 << 14, 1 << 22, 1 << 29), "ci16": (1 << 22, 1 << 38, 1 << 45)}


def full_scale_energy(fmt):
    return (128 * AMPLITUDE[fmt]) ** 2


def window_count(nsamples, hop):
    pairs = nsamples // 2
    return 0 if pairs < 128 else (pairs - 128) // hop + 1


def windows(iq, fmt, hop, n=None):
    """(n, 128, 2) int64 array of s: window i = pairs [i*hop, i*hop + 128)."""
    v = np.asarray(iq).reshape(-1)
    assert v.dtype == DTYPE[fmt], (v.dtype, fmt)
    if n is None:
        n = window_count(v.size, hop)
    pairs = v[:2 * (hop * (n - 1) + 128)].reshape(-1, 2) if n else v[:0].reshape(0, 2)
    idx = (np.arange(n)[:, None] * hop + np.arange(128)[None, :]) if n else np.zeros((0, 128), np.int64)
    s = pairs[idx].astype(np.int64)
    return 2 * s - 255 if fmt == "cu8" else s


def stats(iq, fmt, hop=128, remove_dc=True, n=None):
    """The four exact integers per window, as int64 columns of a dict."""
    s = windows(iq, fmt, hop, n)
    sum_i, sum_q = s[:, :, 0].sum(axis=1), s[:, :, 1].sum(axis=1)
    sum_sq = (s * s).sum(axis=(1, 2))
    energy = 128 * sum_sq - (sum_i * sum_i + sum_q * sum_q if remove_dc else 0)
    return {"sum_i": sum_i, "sum_q": sum_q, "sum_sq": sum_sq, "energy": energy}


def stats_records(iq, fmt, hop=128, remove_dc=True, n=None):
    st = stats(iq, fmt, hop, remove_dc, n)
    assert (st["energy"] >= 0).all() and (st["sum_sq"] >= 0).all()
    out = np.empty(st["energy"].shape, STATS64_DTYPE)
    for k in STATS64_DTYPE.names:
        out[k] = st[k]
    return out


def centred(iq, fmt, hop=128, remove_dc=True, n=None):
    """a, (n, 2, 128) float64: exact (s is an integer below 2^16, the mean a multiple of 1/128)."""
    s = windows(iq, fmt, hop, n)
    a = s.astype(np.float64)
    if remove_dc:
        a = a - s.sum(axis=1, keepdims=True).astype(np.float64) / 128.0
    return np.ascontiguousarray(a.transpose(0, 2, 1))


def frames(iq, fmt, level=7.8e-3, hop=128, remove_dc=True, n=None):
    """(n, 2, 128) float64 normalised frames: row 0 = I, row 1 = Q."""
    a = centred(iq, fmt, hop, remove_dc, n)
    e = stats(iq, fmt, hop, remove_dc, n)["energy"].astype(np.float64)      # E <= 2^45: exact in f64
    g = np.divide(128.0 * float(level), np.sqrt(e), out=np.zeros_like(e), where=e > 0)
    return a * g[:, None, None]


def plain_frames(iq, fmt, scale, hop=128, n=None):
    """mdc_iq_windows in float32, operation for operation: (float)s * scale ("cu8": ((float)byte - 127.5f) * scale)."""
    s = windows(iq, fmt, hop, n)
    v = ((s + 255) // 2).astype(np.float32) - np.float32(127.5) if fmt == "cu8" else s.astype(np.float32)
    return np.ascontiguousarray((v * np.float32(scale)).transpose(0, 2, 1))


def power_dbfs(energy, fmt):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(energy, np.float64) / float(full_scale_energy(fmt)))


def quantise_frames(x, fmt, peak_lsb, dc=(0, 0)):
    """float frames (n, 2, 128) -> interleaved samples (n*256,) as a signed-sample receiver would deliver them: the whole batch
    scaled so that its largest |sample| is `peak_lsb` LSB, plus a DC offset (dc_i, dc_q) in LSB, rounded."""
    assert fmt in ("ci8", "ci16")
    x = np.asarray(x, np.float64)
    k = float(peak_lsb) / np.abs(x).max()
    q = np.rint(x * k + np.asarray(dc, np.float64)[None, :, None])
    assert q.min() >= SAMPLE_MIN[fmt] and q.max() <= SAMPLE_MAX[fmt]
    return np.ascontiguousarray(q.astype(DTYPE[fmt]).transpose(0, 2, 1)).reshape(-1)


def emulate_f32_chain(iq, fmt, level, hop=128, remove_dc=True, n=None):
    """The header's normative chain in float32, operation by operation (numpy's f32 sqrt, division and multiplication are
    correctly rounded; int64 -> f32 is one correctly rounded conversion): what a conforming kernel returns bit for bit."""
    s = windows(iq, fmt, hop, n)
    st = stats(iq, fmt, hop, remove_dc, n)
    c = np.stack([st["sum_i"], st["sum_q"]], axis=1)[:, None, :] if remove_dc else 0
    num = 128 * s - c
    assert (np.abs(num) < 1 << 24).all()
    e = st["energy"]
    with np.errstate(divide="ignore"):
        g = np.where(e > 0, np.float32(level) / np.sqrt(e.astype(np.float32)), np.float32(0)).astype(np.float32)
    return np.ascontiguousarray((num.astype(np.float32) * g[:, None, None]).transpose(0, 2, 1))
