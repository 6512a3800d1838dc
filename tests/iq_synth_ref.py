"""numpy int64 restatement of mdc_iq_synth_frames (include/mdc.h, "frame synthesis"): the definition the tests hold the kernel
to, bit for bit.  Written from the header's text, not from the kernel: taps are used in the NATURAL order the recipe gives them
(the plan's branch-major image is the kernel's business), every intermediate is an int64 (or uint64) array, the ranges the 32-bit
device arithmetic relies on are asserted on every call, and everything is vectorised over the frames of a class."""
import numpy as np

from iq_ddc_ref import nco_table

ALPHABET, GAUSS, LINEAR, PHASE = 0, 1, 0, 1
GAUSS_MAX = 262140
NOISE_VARIANCE = (8 * (2 ** 32 - 1), 12)          # the exact rational: eight uniform integers on 0 .. 65535
DRAW_STRIDE, DRAW_SYMBOLS, DRAW_NOISE = 0xC2B2AE35, 16, 1024
FRAME = 128

_TABLE = nco_table().astype(np.int64)
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> _U(16))
    h = (h * _U(0x85EBCA6B)) & _M32
    h = h ^ (h >> _U(13))
    h = (h * _U(0xC2B2AE35)) & _M32
    return h ^ (h >> _U(16))


def seed_key(seed):
    seed = int(seed) % (1 << 64)
    return fmix32(fmix32(_U(((seed & 0xFFFFFFFF) + 0x9E3779B9) & 0xFFFFFFFF)) ^ _U(seed >> 32))


def frame_keys(seed, f):
    """key_f of the frames f (a uint64 array)"""
    f = np.asarray(f, dtype=np.uint64)
    lo, hi = f & _M32, f >> _U(32)
    inner = fmix32(seed_key(seed) ^ ((lo * _U(0x85EBCA6B)) & _M32))
    return fmix32(inner ^ ((hi * _U(0x85EBCA6B) + _U(1)) & _M32))


def draw(key, j):
    """d(j) = fmix32(key_f + j * 0xC2B2AE35); key and j broadcast"""
    return fmix32((np.asarray(key, np.uint64) + (np.asarray(j, np.uint64) * _U(DRAW_STRIDE) & _M32)) & _M32)


def gauss(key, j):
    """g(d(j) .. d(j + 3)): int64, |g| <= 262140"""
    g = np.full(np.broadcast(key, j).shape, -GAUSS_MAX, np.int64)
    for e in range(4):
        d = draw(key, np.asarray(j, np.uint64) + _U(e))
        g += (d & _U(0xFFFF)).astype(np.int64) + (d >> _U(16)).astype(np.int64)
    assert np.abs(g).max(initial=0) <= GAUSS_MAX
    return g


def frame_indices(first_frame, n):
    return (np.arange(n, dtype=np.uint64) + _U(int(first_frame) % (1 << 64)))          # wraps mod 2^64


def labels_of(first_frame, n, C, S):
    cell = (frame_indices(first_frame, n) % _U(C * S)).astype(np.int64)
    return (cell % C).astype(np.int32), (cell // C).astype(np.int32)


def timing_offsets(seed, f, sps):
    return ((draw(frame_keys(seed, f), 0) * _U(sps)) >> _U(32)).astype(np.int64)


def carrier_steps(seed, f, max_step):
    """the drawn step as a signed integer in -max_step .. max_step"""
    return ((draw(frame_keys(seed, f), 2) * _U(2 * max_step + 1)) >> _U(32)).astype(np.int64) - max_step


def _class_frames(c, points, taps, key, max_step, want):
    """one class: the frames of the keys `key`.  want: "z" (before the channel), "m" (after the mixer) -> (re, im) int64 (n, 128)"""
    n = key.size
    sps, span = int(c["sps"]), int(c["span"])
    h = taps[int(c["first_tap"]):int(c["first_tap"]) + sps * span].astype(np.int64)
    assert h.shape == (sps * span, 2)
    nsym = (FRAME - 1 + sps - 1) // sps + span
    assert nsym <= 144
    k = np.arange(nsym, dtype=np.uint64)[None, :]
    if int(c["source"]) == GAUSS:
        a_re, a_im = gauss(key[:, None], _U(DRAW_SYMBOLS) + _U(4) * k), np.zeros((n, nsym), np.int64)
    else:
        M = int(c["points"])
        assert M >= 1 and M & (M - 1) == 0 and M <= 64
        idx = ((draw(key[:, None], _U(DRAW_SYMBOLS) + _U(4) * k) * _U(M)) >> _U(32)).astype(np.int64)
        assert idx.min() >= 0 and idx.max() < M
        pts = points[int(c["first_point"]):int(c["first_point"]) + M].astype(np.int64)
        a_re, a_im = pts[idx, 0], pts[idx, 1]
    tau = ((draw(key, 0) * _U(sps)) >> _U(32)).astype(np.int64)
    assert tau.min(initial=0) >= 0 and tau.max(initial=0) < sps
    p = np.arange(FRAME, dtype=np.int64)[None, :] + tau[:, None]
    m, b = p // sps, p % sps
    acc_re, acc_im = np.zeros((n, FRAME), np.int64), np.zeros((n, FRAME), np.int64)
    for i in range(span):
        s = m + span - 1 - i
        assert s.min(initial=0) >= 0 and s.max(initial=0) < nsym
        x_re, x_im = np.take_along_axis(a_re, s, 1), np.take_along_axis(a_im, s, 1)
        h_re, h_im = h[b + i * sps, 0], h[b + i * sps, 1]
        acc_re += x_re * h_re - x_im * h_im
        acc_im += x_re * h_im + x_im * h_re
        assert max(np.abs(acc_re).max(initial=0), np.abs(acc_im).max(initial=0)) < 2 ** 31          # the plan's branch bound
    y_re, y_im = (acc_re + 16384) >> 15, (acc_im + 16384) >> 15
    add_re, add_im = int(c["add_re"]), int(c["add_im"])
    if int(c["mode"]) == PHASE:
        inc = (y_re * int(c["phase_factor"])).astype(np.uint64) & _M32          # two's complement: the low 32 bits
        theta = (draw(key, 3)[:, None] + np.cumsum(inc, axis=1, dtype=np.uint64)) & _M32
        e = (theta >> _U(20)).astype(np.int64)
        amp = int(c["amplitude"])
        z_re, z_im = ((_TABLE[e, 0] * amp + 16384) >> 15) + add_re, ((_TABLE[e, 1] * amp + 16384) >> 15) + add_im
    else:
        z_re, z_im = y_re + add_re, y_im + add_im
    assert max(np.abs(z_re).max(initial=0), np.abs(z_im).max(initial=0)) <= 32767
    if want == "z":
        return z_re, z_im
    step = (((draw(key, 2) * _U(2 * max_step + 1)) >> _U(32)) + _U((1 << 32) - max_step)) & _M32
    phi = (draw(key, 1)[:, None] + (np.arange(FRAME, dtype=np.uint64)[None, :] * step[:, None] & _M32)) & _M32
    e = (phi >> _U(20)).astype(np.int64)
    cs, sn = _TABLE[e, 0], _TABLE[e, 1]
    pre_re, pre_im = z_re * cs - z_im * sn + 32768, z_re * sn + z_im * cs + 32768
    assert max(np.abs(pre_re).max(initial=0), np.abs(pre_im).max(initial=0)) < 2 ** 31
    return pre_re >> 16, pre_im >> 16


def synth(classes, points, taps, gain_sig, gain_noise, max_step, q, seed, first_frame, n, stage="out"):
    """The frames first_frame .. first_frame + n - 1 of a recipe given as mdc_iq_synth_plan takes it (classes: records with the
    fields of mdc_iq_synth_class; points, taps: (N, 2) int16; gain_sig (C, S), gain_noise (S) int32).  Returns (iq int16 (n, 256),
    labels int32, snr_index int32, saturated); stage "z" / "m": the (n, 128, 2) int64 values before the channel / after the mixer
    in place of iq."""
    C, S = len(classes), len(gain_noise)
    gain_sig = np.asarray(gain_sig, np.int64).reshape(C, S)
    gain_noise = np.asarray(gain_noise, np.int64)
    points = np.asarray(points, np.int16).reshape(-1, 2)
    taps = np.asarray(taps, np.int16).reshape(-1, 2)
    assert 0 <= max_step <= 1 << 30 and 1 <= q <= 40
    f = frame_indices(first_frame, n)
    labels, snr = labels_of(first_frame, n, C, S)
    key = frame_keys(seed, f)
    val = np.zeros((n, FRAME, 2), np.int64)
    for k in range(C):
        sel = np.flatnonzero(labels == k)
        if sel.size:
            re, im = _class_frames(classes[k], points, taps, key[sel], int(max_step), "z" if stage == "z" else "m")
            val[sel, :, 0], val[sel, :, 1] = re, im
    if stage != "out":
        return val, labels, snr, 0
    assert np.abs(val).max(initial=0) <= 32768
    j = _U(DRAW_NOISE) + _U(8) * np.arange(FRAME, dtype=np.uint64)[None, :, None] + _U(4) * np.arange(2, dtype=np.uint64)[None, None, :]
    w = gauss(key[:, None, None], j)
    v = (val * gain_sig[labels, snr][:, None, None] + w * gain_noise[snr][:, None, None] + (1 << (q - 1)))
    assert np.abs(v).max(initial=0) < 2 ** 62
    v >>= q
    out = np.clip(v, -32768, 32767)
    return out.astype(np.int16).reshape(n, 2 * FRAME), labels, snr, int((out != v).sum())
