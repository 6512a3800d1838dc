"""The numpy restatement of mdc_iq_cf32_histogram / mdc_iq_cf32_quantize and of frontend.design_cf32_gain, written from
include/mdc.h ("float captures").  numpy's float32 multiplication and rint are IEEE-754 single operations with round to nearest,
ties to even: the products and roundings below are the header's, bit for bit (numpy keeps denormals; the header says why that
cannot matter for a gain in range)."""
import numpy as np

MIN_GAIN, MAX_GAIN = 2.0 ** -126, 2.0 ** 125


def flat(x):
    """complex64 (n,), float32 (2n,) or float32 (n, 2) -> the flat little-endian float32 array I0 Q0 I1 Q1 ..."""
    a = np.asarray(x)
    if a.dtype.kind == "c":
        a = a.astype("<c8", copy=False).view("<f4")
    return np.ascontiguousarray(a.astype("<f4", copy=False)).reshape(-1)


def histogram(x):
    """256 uint64 counts of the biased exponent byte of every component"""
    return np.bincount((flat(x).view(np.uint32) >> 23) & 0xFF, minlength=256).astype(np.uint64)


def quantize(x, gain):
    """-> (int16 flat, non-finite pairs, clipped components)"""
    f = flat(x)
    g = np.float32(gain)
    assert MIN_GAIN <= float(g) <= MAX_GAIN
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r = np.rint((f * g).astype(np.float32))
    bad = ~np.isfinite(f).reshape(-1, 2).all(axis=1)
    bad2 = np.repeat(bad, 2)
    over = ((r > 32767) | (r < -32768)) & ~bad2
    out = np.where(bad2, np.float32(0), np.clip(r, -32768, 32767))
    return out.astype(np.int16), int(bad.sum()), int(over.sum())


def design_gain(hist, clip_fraction=0.0):
    """frontend.design_cf32_gain, in Python integers"""
    h = [int(v) for v in np.asarray(hist).reshape(256)]
    budget = int(float(clip_fraction) * sum(h[:255]))
    above = 0
    for e in range(254, 0, -1):
        if above + h[e] > budget:
            return float(2.0 ** min(max(140 - e, -126), 125))
        above += h[e]
    return 1.0


# gain 32768: ties at +-0.5, 1.5 and 2.5 LSB (to even: 0, 2, 2), the two ends of the int16 range, full scale, values whose
# product overflows to +-Inf, and a denormal
EDGE_GAIN = 32768.0
EDGES = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 32767.5, -32768.5, 1.0, -1.0, 3e38, -3e38, 1e-45, 0.0], np.float64) / \
    np.array([32768] * 8 + [1] * 6, np.float64)
EDGES = EDGES.astype(np.float32)
EDGES_OUT = np.array([0, 0, 2, -2, 2, -2, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0], np.int16)
EDGES_CLIPPED = 4      # 32767.5 / 32768 rounds to 32768; +1.0 is 32768; +-3e38 overflow.  -32768.5 / 32768 rounds to -32768: inside
