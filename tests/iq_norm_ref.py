"""numpy restatement of mdc_iq_u8_windows_norm (include/mdc.h): the definition the tests hold the kernel to.

Statistics in int64 (exact), frames in float64 from the header's formula; nothing of the package's kernels is imported.

    s = 2*byte - 255
    sum_i, sum_q = sum of s over the window's I / Q bytes;  sum_sq = sum of s_I^2 + s_Q^2
    E = 128*sum_sq - sum_i^2 - sum_q^2 (remove_dc)  |  128*sum_sq
    a = s - sum/128 (remove_dc)  |  s;      x = a * (128*level / sqrt(E)),   all zeros where E == 0
"""
import numpy as np

STATS_DTYPE = np.dtype([("sum_i", np.int32), ("sum_q", np.int32), ("sum_sq", np.uint32), ("energy", np.uint32)])
FULL_SCALE_ENERGY = (128 * 255) ** 2


def window_count(nbytes, hop):
    pairs = nbytes // 2
    return 0 if pairs < 128 else (pairs - 128) // hop + 1


def windows(iq, hop, n=None):
    """(n, 128, 2) int64 view of s = 2*byte - 255: window i = pairs [i*hop, i*hop + 128)."""
    b = np.asarray(iq, np.uint8).reshape(-1)
    if n is None:
        n = window_count(b.size, hop)
    pairs = b[:2 * (hop * (n - 1) + 128)].reshape(-1, 2) if n else b[:0].reshape(0, 2)
    idx = (np.arange(n)[:, None] * hop + np.arange(128)[None, :]) if n else np.zeros((0, 128), np.int64)
    return 2 * pairs[idx].astype(np.int64) - 255


def stats(iq, hop=128, remove_dc=True, n=None):
    """The four exact integers per window, as int64 columns of a dict."""
    s = windows(iq, hop, n)
    sum_i, sum_q = s[:, :, 0].sum(axis=1), s[:, :, 1].sum(axis=1)
    sum_sq = (s * s).sum(axis=(1, 2))
    energy = 128 * sum_sq - (sum_i * sum_i + sum_q * sum_q if remove_dc else 0)
    return {"sum_i": sum_i, "sum_q": sum_q, "sum_sq": sum_sq, "energy": energy}


def stats_records(iq, hop=128, remove_dc=True, n=None):
    st = stats(iq, hop, remove_dc, n)
    out = np.empty(st["energy"].shape, STATS_DTYPE)
    for k in STATS_DTYPE.names:
        assert (st[k] >= np.iinfo(STATS_DTYPE[k]).min).all() and (st[k] <= np.iinfo(STATS_DTYPE[k]).max).all()
        out[k] = st[k]
    return out


def centred(iq, hop=128, remove_dc=True, n=None):
    """a, (n, 2, 128) float64: exact (s is an integer, the mean a multiple of 1/128)."""
    s = windows(iq, hop, n)
    a = s.astype(np.float64)
    if remove_dc:
        a = a - s.sum(axis=1, keepdims=True).astype(np.float64) / 128.0
    return np.ascontiguousarray(a.transpose(0, 2, 1))


def frames(iq, level=7.8e-3, hop=128, remove_dc=True, n=None):
    """(n, 2, 128) float64 normalised frames: row 0 = I, row 1 = Q."""
    a = centred(iq, hop, remove_dc, n)
    e = stats(iq, hop, remove_dc, n)["energy"].astype(np.float64)
    g = np.divide(128.0 * float(level), np.sqrt(e), out=np.zeros_like(e), where=e > 0)
    return a * g[:, None, None]


def power_dbfs(energy):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(energy, np.float64) / float(FULL_SCALE_ENERGY))


def quantise_frames(x, peak_lsb, dc=(0, 0)):
    """float frames (n, 2, 128) -> interleaved bytes (n*256,) as an 8-bit tuner would deliver them: the whole batch scaled so
    that its largest |sample| is `peak_lsb` LSB, plus a DC offset (dc_i, dc_q) in LSB, rounded, around the byte midpoint."""
    x = np.asarray(x, np.float64)
    k = float(peak_lsb) / np.abs(x).max()
    q = np.rint(127.5 + x * k + np.asarray(dc, np.float64)[None, :, None])
    assert q.min() >= 0 and q.max() <= 255
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 1)).reshape(-1)
