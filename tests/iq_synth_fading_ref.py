"""numpy int64 restatement of mdc_iq_synth_frames_faded (include/mdc.h, "frame synthesis through a frequency-selective Rician
channel"): the definition the tests hold the kernel to, bit for bit.  Written from the header's text: the class chain is restated
here over 128 + H samples (only the generator and the label raster are shared with iq_synth_ref), every intermediate is an int64
(or uint64) array, and the bounds the header proves -- |m| <= 32768, |u| <= 65537, |r| < 46341, |y| < 2^22, the gain stage below
2^62, and the 32-bit ranges the device arithmetic relies on -- are asserted on every call."""
import numpy as np

from iq_ddc_ref import nco_table
from iq_synth_ref import draw, fmix32, frame_keys, gauss, labels_of  # noqa: F401  (fmix32: the generator's one primitive)

ALPHABET, GAUSS, LINEAR, PHASE = 0, 1, 0, 1
DRAW_SYMBOLS, DRAW_PATHS, DRAW_NOISE = 16, 768, 1024
FRAME = 128
MAX_PATHS, MAX_TAPS = 4, 16

_TABLE = nco_table().astype(np.int64)
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def _amax(*arrays):
    return max(int(np.abs(a).max(initial=0)) for a in arrays)


def fading_record(paths, taps, max_doppler_step=0):
    """a fading record as plain Python: paths = [(delay_taps (<= 16 ints), los_re, los_im, scatter), ...]"""
    return dict(taps=int(taps), max_doppler_step=int(max_doppler_step),
                paths=[dict(d=[int(v) for v in d], los=(int(lr), int(li)), scatter=int(sc)) for d, lr, li, sc in paths])


def record_of(rec):
    """the same from one _cabi.IQ_SYNTH_FADING record (a numpy structured scalar or 1-element array)"""
    rec = np.asarray(rec).reshape(-1)[0]
    P, T = int(rec["paths"]), int(rec["taps"])
    return fading_record([(rec["path"][p]["delay_taps"][:T].tolist(), rec["path"][p]["los_re"], rec["path"][p]["los_im"], rec["path"][p]["scatter"])
                          for p in range(P)], T, int(rec["max_doppler_step"]))


def _step(d, max_step):
    """((d * (2 max + 1)) >> 32) - max, mod 2^32"""
    return (((d * _U(2 * max_step + 1)) >> _U(32)) + _U((1 << 32) - max_step)) & _M32


def _class_stream(c, points, taps, key, max_step, N):
    """one class: m_{n'} for n' = 0 .. N - 1 of the frames with the keys `key` -> (re, im) int64 (n, N)"""
    n = key.size
    sps, span = int(c["sps"]), int(c["span"])
    h = taps[int(c["first_tap"]):int(c["first_tap"]) + sps * span].astype(np.int64)
    assert h.shape == (sps * span, 2)
    nsym = (N - 1 + sps - 1) // sps + span
    assert nsym <= 159
    k = np.arange(nsym, dtype=np.uint64)[None, :]
    j = _U(DRAW_SYMBOLS) + _U(4) * k
    assert int(j.max()) + 3 <= 651 < DRAW_PATHS
    if int(c["source"]) == GAUSS:
        a_re, a_im = gauss(key[:, None], j), np.zeros((n, nsym), np.int64)
    else:
        M = int(c["points"])
        assert M >= 1 and M & (M - 1) == 0 and M <= 64
        idx = ((draw(key[:, None], j) * _U(M)) >> _U(32)).astype(np.int64)
        pts = points[int(c["first_point"]):int(c["first_point"]) + M].astype(np.int64)
        a_re, a_im = pts[idx, 0], pts[idx, 1]
    tau = ((draw(key, 0) * _U(sps)) >> _U(32)).astype(np.int64)
    assert tau.min(initial=0) >= 0 and tau.max(initial=0) < sps
    p = np.arange(N, dtype=np.int64)[None, :] + tau[:, None]
    m, b = p // sps, p % sps
    acc_re, acc_im = np.zeros((n, N), np.int64), np.zeros((n, N), np.int64)
    for i in range(span):
        s = m + span - 1 - i
        assert s.min(initial=0) >= 0 and s.max(initial=0) < nsym
        x_re, x_im = np.take_along_axis(a_re, s, 1), np.take_along_axis(a_im, s, 1)
        h_re, h_im = h[b + i * sps, 0], h[b + i * sps, 1]
        acc_re += x_re * h_re - x_im * h_im
        acc_im += x_re * h_im + x_im * h_re
        assert _amax(acc_re, acc_im) < 2 ** 31
    y_re, y_im = (acc_re + 16384) >> 15, (acc_im + 16384) >> 15
    add_re, add_im = int(c["add_re"]), int(c["add_im"])
    if int(c["mode"]) == PHASE:
        inc = (y_re * int(c["phase_factor"])).astype(np.uint64) & _M32
        theta = (draw(key, 3)[:, None] + np.cumsum(inc, axis=1, dtype=np.uint64)) & _M32
        e = (theta >> _U(20)).astype(np.int64)
        amp = int(c["amplitude"])
        z_re, z_im = ((_TABLE[e, 0] * amp + 16384) >> 15) + add_re, ((_TABLE[e, 1] * amp + 16384) >> 15) + add_im
    else:
        z_re, z_im = y_re + add_re, y_im + add_im
    assert _amax(z_re, z_im) <= 32767
    phi = (draw(key, 1)[:, None] + (np.arange(N, dtype=np.uint64)[None, :] * _step(draw(key, 2), max_step)[:, None] & _M32)) & _M32
    e = (phi >> _U(20)).astype(np.int64)
    cs, sn = _TABLE[e, 0], _TABLE[e, 1]
    pre_re, pre_im = z_re * cs - z_im * sn + 32768, z_re * sn + z_im * cs + 32768
    assert _amax(pre_re, pre_im) < 2 ** 31
    return pre_re >> 16, pre_im >> 16


def path_gains(fading, key):
    """g_p of the frames with the keys `key`: (re, im) int64 (n, P)"""
    n, P = key.size, len(fading["paths"])
    g_re, g_im = np.zeros((n, P), np.int64), np.zeros((n, P), np.int64)
    for p, path in enumerate(fading["paths"]):
        los, sc = path["los"], path["scatter"]
        assert sc >= 0 and max(abs(los[0]), abs(los[1])) + sc <= 32767
        j = DRAW_PATHS + 16 * p
        g_re[:, p] = los[0] + ((gauss(key, _U(j)) * sc + (1 << 17)) >> 18)
        g_im[:, p] = los[1] + ((gauss(key, _U(j + 4)) * sc + (1 << 17)) >> 18)
    assert _amax(g_re, g_im) <= 32767
    return g_re, g_im


def fade(fading, key, m_re, m_im):
    """y_n, n = 0 .. 127, from the head-extended stream m (n, 128 + H): (re, im) int64 (n, 128)"""
    T, P = fading["taps"], len(fading["paths"])
    H = T - 1
    assert 1 <= P <= MAX_PATHS and 1 <= T <= MAX_TAPS and m_re.shape[1] == FRAME + H and 0 <= fading["max_doppler_step"] <= 1 << 30
    assert _amax(m_re, m_im) <= 32768
    g_re, g_im = path_gains(fading, key)
    nn = np.arange(FRAME, dtype=np.uint64)[None, :]
    y_re, y_im = np.zeros((key.size, FRAME), np.int64), np.zeros((key.size, FRAME), np.int64)
    for p, path in enumerate(fading["paths"]):
        d = list(path["d"]) + [0] * (MAX_TAPS - len(path["d"]))
        assert all(v == 0 for v in d[T:]) and sum(abs(v) for v in d) <= 32767
        a_re, a_im = np.zeros_like(y_re), np.zeros_like(y_im)
        for k in range(T):
            a_re += d[k] * m_re[:, H - k:H - k + FRAME]
            a_im += d[k] * m_im[:, H - k:H - k + FRAME]
        assert _amax(a_re, a_im) + 8192 < 2 ** 31
        u_re, u_im = (a_re + 8192) >> 14, (a_im + 8192) >> 14
        assert _amax(u_re, u_im) <= 65537
        if fading["max_doppler_step"] > 0:
            j = DRAW_PATHS + 16 * p
            psi, nu = draw(key, j + 8), _step(draw(key, j + 9), fading["max_doppler_step"])
            e = (((psi[:, None] + (nn * nu[:, None] & _M32)) & _M32) >> _U(20)).astype(np.int64)
            c, s = _TABLE[e, 0], _TABLE[e, 1]
            pre_re, pre_im = g_re[:, p, None] * c - g_im[:, p, None] * s + 16384, g_re[:, p, None] * s + g_im[:, p, None] * c + 16384
            assert _amax(pre_re, pre_im) < 2 ** 31
            r_re, r_im = pre_re >> 15, pre_im >> 15
        else:
            r_re, r_im = np.broadcast_to(g_re[:, p, None], y_re.shape), np.broadcast_to(g_im[:, p, None], y_re.shape)
        assert _amax(r_re, r_im) < 46341
        y_re += r_re * u_re - r_im * u_im
        y_im += r_re * u_im + r_im * u_re
    y_re, y_im = (y_re + 4096) >> 13, (y_im + 4096) >> 13
    assert _amax(y_re, y_im) < 2 ** 22
    return y_re, y_im


def synth(classes, points, taps, gain_sig, gain_noise, max_step, q, seed, first_frame, n, fading, stage="out"):
    """The frames first_frame .. first_frame + n - 1 of mdc_iq_synth_frames_faded: the tables as iq_synth_ref.synth takes them and
    a fading record (fading_record / record_of).  Returns (iq int16 (n, 256), labels, snr_index, saturated); stage "m": the
    head-extended mixed stream (n, 128 + H, 2) int64 in place of iq; stage "y": the faded samples (n, 128, 2) before the gains."""
    C, S = len(classes), len(gain_noise)
    gain_sig = np.asarray(gain_sig, np.int64).reshape(C, S)
    gain_noise = np.asarray(gain_noise, np.int64)
    points = np.asarray(points, np.int16).reshape(-1, 2)
    taps = np.asarray(taps, np.int16).reshape(-1, 2)
    assert 0 <= max_step <= 1 << 30 and 1 <= q <= 40
    H = fading["taps"] - 1
    f = np.arange(n, dtype=np.uint64) + _U(int(first_frame) % (1 << 64))
    labels, snr = labels_of(first_frame, n, C, S)
    key = frame_keys(seed, f)
    m = np.zeros((n, FRAME + H, 2), np.int64)
    for k in range(C):
        sel = np.flatnonzero(labels == k)
        if sel.size:
            m[sel, :, 0], m[sel, :, 1] = _class_stream(classes[k], points, taps, key[sel], int(max_step), FRAME + H)
    if stage == "m":
        return m, labels, snr, 0
    y = np.stack(fade(fading, key, m[:, :, 0], m[:, :, 1]), axis=2)
    if stage == "y":
        return y, labels, snr, 0
    j = _U(DRAW_NOISE) + _U(8) * np.arange(FRAME, dtype=np.uint64)[None, :, None] + _U(4) * np.arange(2, dtype=np.uint64)[None, None, :]
    w = gauss(key[:, None, None], j)
    v = y * gain_sig[labels, snr][:, None, None] + w * gain_noise[snr][:, None, None] + (1 << (q - 1))
    assert np.abs(v).max(initial=0) < 2 ** 62
    v >>= q
    out = np.clip(v, -32768, 32767)
    return out.astype(np.int16).reshape(n, 2 * FRAME), labels, snr, int((out != v).sum())
