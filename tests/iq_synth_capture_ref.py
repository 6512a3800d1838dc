"""numpy int64 restatement of mdc_iq_synth_capture (include/mdc.h, "capture synthesis"): the definition the tests hold the kernel
to, bit for bit.  Written from the header's text, not from the kernel: every emitter's baseband stream is computed whole, from
sample 0 (PHASE: one cumulative sum over the whole stream), taps in the natural order, every intermediate an int64 (or uint64)
array, the draws those of tests/iq_synth_ref.py, and every bound the header proves is asserted on every call."""
import numpy as np

from iq_synth_ref import ALPHABET, GAUSS, LINEAR, PHASE, GAUSS_MAX, DRAW_SYMBOLS, DRAW_NOISE, _TABLE, _M32, _U, draw, frame_keys, gauss  # noqa: F401

FIELD_SYMBOLS, FIELD_CONSTANTS, FIELD_DWELL, FIELD_NOISE = 0, 1, 2, 3
MAX_EMITTERS, MAX_L, MAX_TAPS, MAX_BRANCH, MAX_BRANCH_ABS_SUM, MAX_HOPS = 32, 32, 1024, 64, 65535, 8


def _f(e_plus_1, field, low=0):
    low = np.asarray(low, dtype=np.uint64)
    assert low.max(initial=0) < (1 << 52)
    return _U((e_plus_1 << 56) + (field << 52)) + low


def hop_indices(seed, e, dwells, hops):
    """hop index of the dwells `dwells` of emitter e: (d(0) * hops) >> 32 under f = (e+1) 2^56 + 2 2^52 + w"""
    d = draw(frame_keys(seed, _f(e + 1, FIELD_DWELL, dwells)), 0)
    idx = ((d * _U(int(hops))) >> _U(32)).astype(np.int64)
    assert idx.min(initial=0) >= 0 and idx.max(initial=0) < hops
    return idx


def gate(i, start, on, period):
    """(is the emitter on at the baseband samples i, their dwells w(i))"""
    i = np.asarray(i, np.int64)
    started = i >= start
    x = np.where(started, i - start, 0)
    if period == 0:
        return started & ((on == 0) | (x < on)), np.zeros(i.shape, np.int64)
    return started & (x % period < on), np.where(started, x // period, 0)


def baseband(e, c, points, taps, seed, count):
    """z_0 .. z_{count-1} of emitter e of class record c: (re, im) int64"""
    sps, span = int(c["sps"]), int(c["span"])
    h = np.asarray(taps, np.int16).reshape(-1, 2)[int(c["first_tap"]):int(c["first_tap"]) + sps * span].astype(np.int64)
    assert h.shape == (sps * span, 2)
    ckey = frame_keys(seed, _f(e + 1, FIELD_CONSTANTS))
    tau = int((draw(ckey, 0) * _U(sps)) >> _U(32))
    assert 0 <= tau < sps
    p = np.arange(count, dtype=np.int64) + tau
    m, b = p // sps, p % sps
    nsym = int(m.max(initial=0)) + span
    k = np.arange(nsym, dtype=np.uint64)
    key = frame_keys(seed, _f(e + 1, FIELD_SYMBOLS, k >> _U(7)))
    j = _U(DRAW_SYMBOLS) + _U(4) * (k & _U(127))
    if int(c["source"]) == GAUSS:
        a_re, a_im = gauss(key, j), np.zeros(nsym, np.int64)
    else:
        M = int(c["points"])
        assert M >= 1 and M & (M - 1) == 0 and M <= 64
        idx = ((draw(key, j) * _U(M)) >> _U(32)).astype(np.int64)
        pts = np.asarray(points, np.int16).reshape(-1, 2)[int(c["first_point"]):int(c["first_point"]) + M].astype(np.int64)
        a_re, a_im = pts[idx, 0], pts[idx, 1]
    acc_re, acc_im = np.zeros(count, np.int64), np.zeros(count, np.int64)
    for t in range(span):
        s = m + span - 1 - t
        assert s.min(initial=0) >= 0 and s.max(initial=0) < nsym
        h_re, h_im = h[b + t * sps, 0], h[b + t * sps, 1]
        acc_re += a_re[s] * h_re - a_im[s] * h_im
        acc_im += a_re[s] * h_im + a_im[s] * h_re
        assert max(np.abs(acc_re).max(initial=0), np.abs(acc_im).max(initial=0)) < 2 ** 31
    y_re, y_im = (acc_re + 16384) >> 15, (acc_im + 16384) >> 15
    add_re, add_im = int(c["add_re"]), int(c["add_im"])
    if int(c["mode"]) == PHASE:
        inc = (y_re * int(c["phase_factor"])).astype(np.uint64) & _M32
        theta = (draw(ckey, 3) + np.cumsum(inc, dtype=np.uint64)) & _M32          # uint64 wraps mod 2^64: the low 32 bits are exact
        t = (theta >> _U(20)).astype(np.int64)
        amp = int(c["amplitude"])
        z_re, z_im = ((_TABLE[t, 0] * amp + 16384) >> 15) + add_re, ((_TABLE[t, 1] * amp + 16384) >> 15) + add_im
    else:
        z_re, z_im = y_re + add_re, y_im + add_im
    assert max(np.abs(z_re).max(initial=0), np.abs(z_im).max(initial=0)) <= 32767
    return z_re, z_im


def emitter_mixed(e, em, classes, points, taps, scene_taps, seed, n_pairs):
    """m_{e,n}, n < n_pairs: (re, im) int64, the number of components the interpolation clamp changed, and the gate (on, dwell)
    of every baseband sample the capture reads"""
    L, D, T = int(em["interpolate"]), int(em["decimate"]), int(em["ntaps"])
    assert 1 <= D <= L <= MAX_L and 1 <= T <= MAX_TAPS
    K = (T + L - 1) // L
    assert K <= MAX_BRANCH
    h = np.asarray(scene_taps, np.int16).reshape(-1)[int(em["first_tap"]):int(em["first_tap"]) + T].astype(np.int64)
    assert h.size == T
    for r in range(L):
        assert np.abs(h[r::L]).sum() <= MAX_BRANCH_ABS_SUM
    n = np.arange(n_pairs, dtype=np.int64)
    P = n * D + T - 1
    m, r = P // L, P % L
    count = int(m.max(initial=-1)) + 1
    z_re, z_im = baseband(e, classes[int(em["cls"])], points, taps, seed, count)
    start, on, period, hops = int(em["start"]), int(em["on"]), int(em["period"]), int(em["hops"])
    assert start >= 0 and on >= 0 and period >= 0 and 1 <= hops <= MAX_HOPS and (hops == 1 or period > 0)
    is_on, dwell = gate(np.arange(count, dtype=np.int64), start, on, period)
    zg_re, zg_im = np.where(is_on, z_re, 0), np.where(is_on, z_im, 0)
    acc_re, acc_im = np.zeros(n_pairs, np.int64), np.zeros(n_pairs, np.int64)
    for i in range(K):
        t = r + i * L
        valid = t < T
        src = m - i
        assert src[valid].min(initial=0) >= 0          # no start-up ramp
        hh = np.where(valid, h[np.minimum(t, T - 1)], 0)
        src = np.maximum(src, 0)
        acc_re += hh * zg_re[src]
        acc_im += hh * zg_im[src]
    assert max(np.abs(acc_re).max(initial=0), np.abs(acc_im).max(initial=0)) < 2 ** 31
    v_re, v_im = (acc_re + 16384) >> 15, (acc_im + 16384) >> 15
    u_re, u_im = np.clip(v_re, -32768, 32767), np.clip(v_im, -32768, 32767)
    clamped = int((u_re != v_re).sum() + (u_im != v_im).sum())
    steps = np.asarray(em["phase_step"], np.uint64).reshape(-1)
    if hops > 1:
        w = dwell[m]
        uniq, inv = np.unique(w, return_inverse=True)
        step = steps[hop_indices(seed, e, uniq, hops)[inv]]
    else:
        step = np.full(n_pairs, steps[0], np.uint64)
    phi = (_U(int(em["phase0"])) + ((n.astype(np.uint64) & _M32) * step & _M32)) & _M32
    t = (phi >> _U(20)).astype(np.int64)
    cs, sn = _TABLE[t, 0], _TABLE[t, 1]
    pre_re, pre_im = u_re * cs - u_im * sn + 32768, u_re * sn + u_im * cs + 32768
    assert max(np.abs(pre_re).max(initial=0), np.abs(pre_im).max(initial=0)) < 2 ** 31
    m_re, m_im = pre_re >> 16, pre_im >> 16
    assert max(np.abs(m_re).max(initial=0), np.abs(m_im).max(initial=0)) <= 32768
    return m_re, m_im, clamped, (is_on, dwell)


def noise(seed, n_pairs):
    """w_n: (n_pairs, 2) int64"""
    n = np.arange(n_pairs, dtype=np.uint64)
    key = frame_keys(seed, _f(0, FIELD_NOISE, n >> _U(7)))
    j = _U(DRAW_NOISE) + _U(8) * (n & _U(127))
    return np.stack([gauss(key, j), gauss(key, j + _U(4))], axis=1)


def capture(classes, points, taps, emitters, scene_taps, gain_noise, q, dc, seed, n_pairs, stage="out"):
    """The first n_pairs pairs of a scene given as mdc_iq_synth_scene takes it (classes, points, taps: the plan's recipe tables;
    emitters: records with the fields of mdc_iq_synth_emitter; scene_taps: int16).  Returns (iq int16 (n_pairs, 2), saturated);
    stage "m": the (E, n_pairs, 2) int64 values after the mixer, before the gains, in place of iq."""
    E = len(emitters)
    assert 0 <= E <= MAX_EMITTERS and gain_noise >= 0 and 1 <= q <= 40
    mixed = np.zeros((E, n_pairs, 2), np.int64)
    saturated = 0
    for e in range(E):
        mixed[e, :, 0], mixed[e, :, 1], clamped, _ = emitter_mixed(e, emitters[e], classes, points, taps, scene_taps, seed, n_pairs)
        saturated += clamped
    if stage == "m":
        return mixed, saturated
    gains = np.array([int(em["gain"]) for em in emitters], np.int64).reshape(E, 1, 1)
    v = (mixed * gains).sum(axis=0)
    if gain_noise:
        v = v + noise(seed, n_pairs) * int(gain_noise)
    v = v + (1 << (q - 1))
    assert np.abs(v).max(initial=0) < 2 ** 62
    v = (v >> q) + np.array([int(dc[0]), int(dc[1])], np.int64)[None, :]
    out = np.clip(v, -32768, 32767)
    return out.astype(np.int16), saturated + int((out != v).sum())


def scene_capture(scene, seed, n_pairs, stage="out"):
    """capture() of a frontend.SynthScene"""
    r = scene.recipe
    return capture(r.classes, r.points, r.taps, scene.emitters, scene.taps, scene.gain_noise, scene.q, scene.dc, seed, n_pairs, stage)
