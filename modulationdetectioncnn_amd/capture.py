"""The capture pipelines scan_iq, detect_iq and predict_channels as functions of a model: they use its predict_iq, device_index
and topology.classes, the rest is the frontend's pieces in order.  VTCNN2 binds the three as methods, hence `self`.  torch and
the frontend are imported at the first call, not with the package."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _cabi


def _tuned(dev, fmt, shift, L, D, taps, hop):
    """One stretch of a capture at the nets' rate, as a (n, 2) "ci16" tensor: frontend.ddc when L == 1, else frontend.resample;
    hop == 128: trimmed to whole frames"""
    from . import frontend as F
    if L == 1:
        down = F.ddc(dev, fmt, shift=shift, decimate=D, taps=taps)
    else:
        down = F.resample(dev, fmt, shift=shift, interpolate=L, decimate=D, taps=taps)
    return down[:down.shape[0] // 128 * 128] if hop == 128 else down


def _capture(iq, fmt, balance, device):
    """scan_iq's and detect_iq's capture on the device: (flat tensor, format id, the records' extra keys).  balance False: as it
    came, no key; True or a coefficients tuple: through frontend.balance first, then "ci16", and image_rejection_db -- the
    capture's estimate before correction, None for given coefficients"""
    from . import frontend as F
    if balance is False or balance is None:
        return F._device_samples(iq, fmt, device), fmt, {}
    dev, fmt, irr = F.balanced_capture(iq, fmt, balance, device)
    return dev, fmt, dict(image_rejection_db=irr)


def _no_windows(classes, device):
    """predict_iq(..., return_power=True)'s three results for a stretch without a window"""
    import torch
    return (torch.empty((0, classes), dtype=torch.float32, device=device), torch.empty((0,), dtype=torch.int32, device=device),
            torch.empty((0,), dtype=torch.float64, device=device))


def _vote(labels) -> int:
    """The most frequent label among the windows with label >= 0 (the smallest on a tie; -1 if there are none)"""
    import torch
    open_ = labels[labels >= 0]
    return int(torch.bincount(open_).argmax()) if open_.numel() else -1


def _line_bands(bandwidth, line_nfft):
    """detect_iq(refine=True): (D0, bands) of a detection of that bandwidth -- the isolating decimation and the three bands of
    frontend.find_lines (envelope, square, fourth power) at its isolated rate; bands is None when the envelope's band holds
    no bin of line_nfft"""
    D0 = min(max(int(1.0 / (4.0 * bandwidth)), 1), 256)
    b = bandwidth * D0
    lo, hi = b / 2.5, min(0.45, 1.25 * b)
    f = np.fft.fftfreq(int(line_nfft))
    if not np.any((f >= lo) & (f <= hi)):
        return D0, None
    m = min(b / 8.0, 0.12)
    return D0, [(lo, hi, False), (0.0, 2.0 * m, True), (0.0, 4.0 * m, True)]


def _apply_estimate(centre, D0, plan, rate, rate_db, offset, order, offset_db):
    """refine=True: ((shift, L, D), the record's five extra keys) from the estimates made on an emitter isolated at decimation D0
    -- rate (None: no symbol line), offset and order as frontend.estimate_symbol_rate / estimate_carrier_offset give them.  The
    carrier moves the shift; the symbol rate replaces the plan's ratio where one within its 1 % exists."""
    from . import frontend as F
    _, L, D = plan
    shift = -(centre + offset / D0)
    if abs(shift) > 0.5:      # at the band's edge: the same frequency, one turn on
        shift -= round(shift)
    if rate is not None:
        try:
            L, D, _ = F.resample_ratio(1.0, rate / D0, 8)
        except ValueError:      # nothing within 1 %: the plan's ratio stands
            pass
    return (shift, L, D), dict(symbol_rate=None if rate is None else rate / D0, symbol_line_db=rate_db, carrier_offset=offset / D0,
                               carrier_order=order, carrier_line_db=offset_db)


def _refined_plan(centre, D0, plan, lines, min_line_db):
    """detect_iq(refine=True): ((shift, L, D), the record's five extra keys) from find_lines' three results at orders 0, 2, 4
    of the detection isolated at decimation D0 (lines None: no spectrum, the plan stands) -- the decisions of
    frontend.estimate_symbol_rate and frontend.estimate_carrier_offset, and scan_iq(refine=True)'s use of them"""
    if lines is None:
        return plan, dict(symbol_rate=None, symbol_line_db=float("-inf"), carrier_offset=0.0, carrier_order=0, carrier_line_db=float("-inf"))
    (rate, rate_db), (f2, db2), (f4, db4) = lines
    if rate_db < float(min_line_db):
        rate = None
    if db2 >= float(min_line_db):
        offset, order, offset_db = f2 / 2, 2, db2
    elif db4 >= float(min_line_db):
        offset, order, offset_db = f4 / 4, 4, db4
    else:
        offset, order, offset_db = 0.0, 0, max(db2, db4)
    return _apply_estimate(centre, D0, plan, rate, rate_db, offset, order, offset_db)


def scan_iq(self, iq, sample_format, nfft: int = 1024, avg: int = 8, threshold_db: float = 6.0, hop: int = 128, level: float = 7.8e-3,
            squelch_dbfs: Optional[float] = None, refine: bool = False, min_line_db: float = 8.0, bursts: bool = False, hold: float = 0.98,
            burst_threshold_db: float = 3.0, min_rows: int = 1, merge_rows: int = 1, balance=False, **find_kw):
    """A wideband capture in, "what is transmitting where, and what modulation" out.  The capture's power spectrogram
    (frontend.spectrogram: nfft bins, Hann window, segments nfft // 2 apart, `avg` of them per row, on the device) is averaged
    over its rows into one spectrum; frontend.find_emitters(spectrum, threshold_db, window=the Hann window, **find_kw) lists
    the emitters; each one is brought to 0 Hz and to the nets' rate by frontend.channel_plan's (shift, L, D) -- through
    frontend.ddc when L == 1, else frontend.resample, with frontend.plan_taps(L, D) as the filter --, cut into windows `hop` output pairs apart
    (hop == 128: the stream is trimmed to whole frames) and classified with predict_iq(..., "ci16", normalize="rms", level=,
    squelch_dbfs=, return_power=True).  Returns one dict per emitter, in order of centre: centre, bandwidth (cycles per input
    sample), power_dbfs, snr_db, shift, interpolate, decimate, probs, labels, window_dbfs (predict_iq's three results: device
    tensors, or numpy arrays for a numpy capture) and label, the most frequent label among the windows the squelch let through
    (the smallest on a tie; -1 if there are none).

    refine=True replaces the plan's two guesses -- a symbol rate from the thresholded width, a carrier from the centroid -- by
    the emitter's spectral lines.  Per emitter: (1) isolate it at about four times its width, D0 = clamp(floor(1 / (4
    bandwidth)), 1, 256), iso = frontend.ddc(capture, shift=-centre, decimate=D0, taps=frontend.plan_taps(1, D0)); b =
    bandwidth D0 is its width there.  (2) frontend.estimate_symbol_rate(iso, "ci16", lo=b / 2.5, hi=min(0.45, 1.25 b),
    min_line_db=): a linear modulation's symbol rate is b / (1 + beta), beta in 0..1, and a thresholded width may be 25 % off;
    the band also keeps the line's harmonics out.  symbol_rate = rate / D0 (None without a line).  (3)
    frontend.estimate_carrier_offset(iso, "ci16", max_offset=b / 8, min_line_db=) (at most 0.12: an emitter filling the whole
    band); carrier_offset = offset / D0, and shift = -(centre + carrier_offset), folded into [-0.5, 0.5].  (4) (L, D) = frontend.resample_ratio(1.0, symbol_rate, 8) when the symbol line was found and
    a ratio within its 1 % exists, else channel_plan's.  (5) The ORIGINAL capture is resampled with that shift and ratio and
    plan_taps(L, D), and classified as above.  The record gains symbol_rate (cycles per input sample, or None),
    symbol_line_db, carrier_offset, carrier_order (2, 4, or 0: no line -- 8PSK, analogue and frequency-shift signals show
    none -- and the centroid stands) and carrier_line_db; centre stays the centroid.  refine=False is the plan alone, and its
    record has none of the five.

    bursts=True is the scan for INTERMITTENT emitters -- push-to-talk, telemetry bursts, packet traffic --, which the mean over
    the rows dilutes (on 3 % of the time: by 15 dB) until they are missed or found in fragments.  The spectrogram is then looked
    at along time per bin: Q = frontend.spectrum_quantiles(spec, (0.5, hold)), one call on the device.  The emitters are
    find_emitters(Q[1], threshold_db, ...): the spectrum each bin reaches in its top 1 - hold of the rows, whose own median bin
    is find_emitters' floor, so that the noise's high quantile cancels.  The noise per bin is the median over the bins of
    Q[0], the median over time, which bursts do not lift.  Per emitter, (first, count) = frontend.emitter_bins(e, nfft), band =
    frontend.band_power(spec, first, count), and frontend.find_bursts(band, count * noise, burst_threshold_db, min_rows,
    merge_rows) gives the rows it was on.  The record gains bursts, a list of half-open intervals of INPUT pairs
    (frontend.burst_pairs), and duty, on-rows / rows.  Plan, refine, tuning, resampling and predict_iq run on the whole
    capture as without bursts; then every window whose frontend.window_support (the input pairs its 128 outputs read through
    the filter) is not wholly inside one burst gets label -1, as the squelch does, and label is the majority among the
    windows still open; probs and window_dbfs are untouched.  A spectrogram's rows drop trailing segments that do not fill a
    row (and a window's support is wider than the window): the last windows of a capture can therefore be gated even for an
    emitter that never pauses.  An emitter must revisit its bins in at least 1 - hold of the rows to be seen.  bursts=False
    (the default) is the mean spectrum, and its record has neither key.

    balance=True first removes the receiver's DC offset and I/Q imbalance, estimated from the capture itself
    (frontend.balance), and carries on with the corrected "ci16" stream: an uncalibrated zero-IF receiver mirrors every emitter
    at +f to -f, 20 .. 40 dB down, and a strong one's image is otherwise listed -- and classified -- as an emitter.  A
    coefficients tuple (frontend.BalanceCoeffs) is applied as given.  The records gain image_rejection_db, the capture's estimate
    before correction (None for given coefficients).  balance=False (the default) changes nothing and adds no key."""
    import torch
    from . import frontend as F
    fmt = F.sample_format_id(sample_format)
    as_numpy = not isinstance(iq, torch.Tensor)
    dev, fmt, balanced = _capture(iq, fmt, balance, f"cuda:{self.device_index}")
    window = F.design_window(nfft)
    spec = F.spectrogram(dev, fmt, nfft=nfft, avg=avg)
    if spec.shape[0] == 0:
        raise ValueError(f"the capture is too short for one row of {avg} segments of {nfft} pairs")
    if bursts:
        quant = F.spectrum_quantiles(spec, (0.5, float(hold))).to(torch.float64).cpu().numpy()
        psd, noise = quant[1], float(np.median(quant[0]))
    else:
        psd = spec.to(torch.float64).mean(0).cpu().numpy()
    out = []
    for e in F.find_emitters(psd, threshold_db=threshold_db, window=window, **find_kw):
        shift, L, D, _ = F.channel_plan(e.centre, e.bandwidth)
        extra = {}
        if refine:
            D0 = min(max(int(1.0 / (4.0 * e.bandwidth)), 1), 256)
            iso = F.ddc(dev, fmt, shift=-e.centre, decimate=D0, taps=F.plan_taps(1, D0)).reshape(-1)
            b = e.bandwidth * D0
            rate, rate_db = F.estimate_symbol_rate(iso, _cabi.IQ_CI16, lo=b / 2.5, hi=min(0.45, 1.25 * b), min_line_db=min_line_db)
            offset, order, offset_db = F.estimate_carrier_offset(iso, _cabi.IQ_CI16, max_offset=min(b / 8.0, 0.12), min_line_db=min_line_db)
            (shift, L, D), extra = _apply_estimate(e.centre, D0, (shift, L, D), rate, rate_db, offset, order, offset_db)
        taps = F.plan_taps(L, D)
        probs, labels, dbfs = self.predict_iq(_tuned(dev, fmt, shift, L, D, taps, hop).reshape(-1), _cabi.IQ_CI16, hop=hop, normalize="rms",
                                              level=level, squelch_dbfs=squelch_dbfs, return_power=True)
        if bursts:
            first_bin, count = F.emitter_bins(e, nfft)
            rows_on = F.find_bursts(F.band_power(spec, first_bin, count).cpu(), count * noise, burst_threshold_db, min_rows, merge_rows)
            on = [F.burst_pairs(a, z, nfft, nfft // 2, avg) for a, z in rows_on]
            extra.update(bursts=on, duty=sum(z - a for a, z in rows_on) / spec.shape[0])
            lo, hi = F._window_supports(np.arange(labels.shape[0]), hop, taps.size, L, D)
            inside = np.zeros(labels.shape[0], bool)
            for a, z in on:
                inside |= (lo >= a) & (hi < z)
            labels.masked_fill_(torch.from_numpy(~inside).to(labels.device), -1)
        label = _vote(labels)
        if as_numpy:
            probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
        out.append(dict(centre=e.centre, bandwidth=e.bandwidth, power_dbfs=e.power_dbfs, snr_db=e.snr_db, shift=shift, interpolate=L, decimate=D,
                        labels=labels, probs=probs, window_dbfs=dbfs, label=label, **extra, **balanced))
    return out


def detect_iq(self, iq, sample_format, nfft: int = 1024, avg: int = 8, threshold_db: float = 6.0, floor: str = "flat", reach_rows: int = 2,
              reach_bins: int = 3, min_rows: int = 3, min_bins: int = 3, hop: int = 128, level: float = 7.8e-3,
              squelch_dbfs: Optional[float] = None, dc_guard: int = 1, batched: bool = False, refine: bool = False, min_line_db: float = 8.0,
              line_nfft: int = 1024, line_avg: int = 8, balance=False, cfar=None):
    """A wideband capture in, "what transmitted when, where, and what modulation" out: the scan in two dimensions, for
    frequency hoppers, emitters that share bins at different times and single packets, which scan_iq's one-dimensional
    searches miss or mangle.  The capture's spectrogram (frontend.spectrogram, as scan_iq builds it: nfft bins, segments nfft //
    2 apart, `avg` per row) is thresholded per cell at frontend.detection_threshold(spec, threshold_db, dc_guard, floor) and
    frontend.find_detections(spec, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg) joins the on-cells into boxes
    in time and frequency, all on the device.  Per detection, frontend.channel_plan(centre, bandwidth) and frontend.plan_taps
    give (shift, L, D) and the filter, and ONLY the pairs [first_pair, stop_pair) of the capture go through frontend.ddc (L ==
    1) or frontend.resample; the result is cut into windows `hop` output pairs apart (hop == 128: trimmed to whole frames)
    and classified with predict_iq(..., "ci16", normalize="rms", level=, squelch_dbfs=, return_power=True).  Returns one dict
    per detection, ordered by (first_pair, centre): the Detection's fields (first_row, stop_row, first_bin, stop_bin, cells,
    centre, bandwidth, peak_db, snr_db, first_pair, stop_pair) plus shift, interpolate, decimate, probs, labels, window_dbfs
    (device tensors, or numpy arrays for a numpy capture), windows, their number, and label, the most frequent label among the
    windows the squelch let through (the smallest on a tie; -1 if there are none).  A detection whose pairs are too few for
    one window gives windows = 0, label = -1 and empty results.  The default dc_guard of 1 switches bins -1, 0, +1 off, a gap
    of three that reach_bins = 3 does not bridge: an emitter ON bin 0 comes out as two boxes, one each side of the guard.  A
    capture without a DC spike takes dc_guard=0 (only bin 0 off) and gets it as one.
    batched=True gives the same records, key for key and bit for bit, without the loop over detections: one
    frontend.extract launch tunes, filters and resamples every detection's pairs into one block of whole frames, one
    predict_iq classifies the block, frontend.segment_votes takes every detection's vote on the device, and the labels come to
    the host in one transfer; probs, labels and window_dbfs are then slices of the block's results.  It needs hop == 128 (with
    another hop windows would straddle detections: ValueError).
    refine=True replaces the plan's two guesses per detection -- a symbol rate from the box's width, a carrier from its
    centroid -- by the detection's spectral lines, scan_iq(refine=True)'s recipe on the detection's own pairs: D0 = clamp(floor(1
    / (4 bandwidth)), 1, 256); iso = the pairs [first_pair, stop_pair) through frontend.ddc(shift=-centre, decimate=D0,
    taps=frontend.plan_taps(1, D0)); b = bandwidth D0.  frontend.line_spectra(iso, "ci16", orders (0, 2, 4), nfft=line_nfft,
    avg=line_avg) gives the three mean spectra, frontend.find_lines searches the envelope's in [b / 2.5, min(0.45, 1.25 b)] and,
    with m = min(b / 8, 0.12), the square's in |f| <= 2 m and the fourth power's in |f| <= 4 m.  The symbol line counts from
    min_line_db on (frontend.estimate_symbol_rate's rule); the carrier is order 2's line if it reaches min_line_db, else order
    4's, else none (frontend.estimate_carrier_offset's rule).  shift = -(centre + offset / D0), folded into [-0.5, 0.5]; (L, D) =
    frontend.resample_ratio(1.0, rate / D0, 8) when the symbol line was found and a ratio within its 1 % exists, else the plan's.
    The record gains symbol_rate (cycles per input sample, or None), symbol_line_db, carrier_offset, carrier_order (2, 4, or 0)
    and carrier_line_db; centre stays the centroid.  A detection too short for one row of line_avg segments of line_nfft
    isolated pairs, or whose symbol band holds no bin at line_nfft, keeps the plan: symbol_rate None, symbol_line_db -inf,
    carrier_offset 0.0, carrier_order 0, carrier_line_db -inf.  The loop does ddc, line_spectra (one job) and find_lines (three
    bands) per detection; batched=True does ONE frontend.extract(..., whole_frames=False) for all isolations, ONE line_spectra
    over the block, ONE find_lines whose 3 K records come to the host in one transfer, and then the extraction above with the
    refined shifts and ratios: the same spectra from the same entries, so both forms agree bit for bit.  refine=False is the
    plan alone, and its record has none of the five keys.
    balance: as scan_iq's -- True, or a coefficients tuple, corrects the capture's DC offset and I/Q imbalance first
    (frontend.balance) and the records gain image_rejection_db; False (the default) changes nothing and adds no key.
    floor="cfar" detects against a LOCAL noise floor instead of one number per bin for the whole capture: ratio =
    frontend.cfar_floor(spec, *cfar, return_ratio=True)[1] divides every cell by an order statistic of the cells around it
    (mdc_iq_spectrogram_cfar, include/mdc.h), thresh = frontend.cfar_threshold(nfft, threshold_db, dc_guard) is the plain factor
    10^(threshold_db / 10) with the DC guard, and found = frontend.find_detections(ratio, thresh, ...); everything behind
    `found` is the code above, loop or batched, with or without refine.  It follows a coloured front-end AND a floor that moves
    in time (a gain step, a pulsed wideband interferer), and a continuous emitter does not become its own floor as under
    "per-bin".  cfar: the five parameters (train_rows, train_bins, guard_rows, guard_bins, rank) as a tuple or a dict with
    those keys (missing ones take the defaults); None: frontend.cfar_floor's defaults (8, 32, 2, 8, 0.5).  The record changes
    its meaning in three places: peak_db is dB above the LOCAL floor at the peak, snr_db = peak_db - threshold_db, and centre is
    the centroid of the ratio's excess over the factor.  The method's known limit is self-masking: an emitter that fills more
    than the share 1 - rank of its own training window lifts its own floor -- at the defaults one wider than about 40 bins
    that is on in every row of the window; such an emitter needs a wider train_bins, or "flat".  cfar= with another floor is a
    ValueError; "flat" and "per-bin" run exactly as before."""
    import torch
    from . import frontend as F
    fmt = F.sample_format_id(sample_format)
    if batched and hop != 128:
        raise ValueError(f"batched=True needs hop == 128 (got {hop}): windows at another hop would straddle two detections")
    if cfar is not None and floor != "cfar":
        raise ValueError(f"cfar= goes with floor='cfar' (got floor={floor!r})")
    cfar_args = F.cfar_parameters(cfar) if floor == "cfar" else None
    as_numpy = not isinstance(iq, torch.Tensor)
    dev, fmt, balanced = _capture(iq, fmt, balance, f"cuda:{self.device_index}")
    spec = F.spectrogram(dev, fmt, nfft=nfft, avg=avg)
    if spec.shape[0] == 0:
        raise ValueError(f"the capture is too short for one row of {avg} segments of {nfft} pairs")
    if floor == "cfar":
        ratio = F.cfar_floor(spec, *cfar_args, return_ratio=True)[1]
        thresh = F.cfar_threshold(nfft, threshold_db, dc_guard, device=ratio.device)
        found = F.find_detections(ratio, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg)
    else:
        thresh = F.detection_threshold(spec, threshold_db, dc_guard, floor)
        found = F.find_detections(spec, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg)
    if batched:
        plans, extras = [p[:3] for p in F.channel_plans([(d.centre, d.bandwidth) for d in found])], None
        if refine and found:
            plans, extras = _refine_detections(dev, fmt, found, plans, min_line_db, line_nfft, line_avg)
        return [dict(r, **balanced) for r in _classify_detections(self, dev, fmt, found, plans, extras, level, squelch_dbfs, as_numpy)]
    per_pair = _cabi.IQ_PAIR_BYTES[fmt] // dev.element_size()      # elements of `dev` per (I,Q) pair
    out = []
    for d in found:
        shift, L, D, _ = F.channel_plan(d.centre, d.bandwidth)
        part, pairs = dev[d.first_pair * per_pair:d.stop_pair * per_pair], d.stop_pair - d.first_pair
        extra = {}
        if refine:
            D0, bands = _line_bands(d.bandwidth, line_nfft)
            lines = None
            if bands is not None:
                iso = F.ddc(part, fmt, shift=-d.centre, decimate=D0, taps=F.plan_taps(1, D0))
                means, rows = F.line_spectra(iso.reshape(-1), _cabi.IQ_CI16, [(0, iso.shape[0])], orders=(0, 2, 4), nfft=line_nfft, avg=line_avg)
                if rows[0] > 0:
                    lines = F.find_lines(means[0], bands)
            (shift, L, D), extra = _refined_plan(d.centre, D0, (shift, L, D), lines, min_line_db)
        taps = F.plan_taps(L, D)
        if (F.ddc_out_count(pairs, taps.size, D) if L == 1 else F.resample_out_count(pairs, taps.size, L, D)) < 128:
            probs, labels, dbfs = _no_windows(self.topology.classes, dev.device)
        else:
            probs, labels, dbfs = self.predict_iq(_tuned(part, fmt, shift, L, D, taps, hop).reshape(-1), _cabi.IQ_CI16, hop=hop, normalize="rms",
                                                  level=level, squelch_dbfs=squelch_dbfs, return_power=True)
        label, windows = _vote(labels), int(labels.shape[0])
        if as_numpy:
            probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
        out.append(dict(d._asdict(), shift=shift, interpolate=L, decimate=D, probs=probs, labels=labels, window_dbfs=dbfs, windows=windows,
                        label=label, **extra, **balanced))
    return out


def _refine_detections(dev, fmt, found, plans, min_line_db, line_nfft, line_avg):
    """detect_iq(batched=True, refine=True) before the extraction: (plans, extras) of all detections (at least one) from one
    frontend.extract of their isolations, one frontend.line_spectra over that block and one frontend.find_lines"""
    import torch
    from . import frontend as F
    geo = [_line_bands(d.bandwidth, line_nfft) for d in found]
    taps = {}
    for D0, _ in geo:
        if D0 not in taps:
            taps[D0] = F.plan_taps(1, D0)
    block, offsets = F.extract(dev, fmt, [(d.first_pair, d.stop_pair, -d.centre, 1, D0, taps[D0]) for d, (D0, _) in zip(found, geo)],
                               whole_frames=False)
    means, rows = F.line_spectra(block.reshape(-1), _cabi.IQ_CI16, offsets, orders=(0, 2, 4), nfft=line_nfft, avg=line_avg)
    live = [k for k, (_, bands) in enumerate(geo) if bands is not None and rows[k] > 0]
    lines = {}
    if live:
        at = torch.as_tensor(live, dtype=torch.int64, device=means.device)
        got = F.find_lines(means[at].reshape(-1, means.shape[2]), [band for k in live for band in geo[k][1]])
        lines = {k: got[3 * i:3 * i + 3] for i, k in enumerate(live)}
    out = [_refined_plan(d.centre, D0, plan, lines.get(k), min_line_db) for k, (d, (D0, _), plan) in enumerate(zip(found, geo, plans))]
    return [p for p, _ in out], [e for _, e in out]


def _classify_detections(self, dev, fmt, found, plans, extras, level, squelch_dbfs, as_numpy):
    """detect_iq(batched=True) behind the search: the records of `found` (frontend.find_detections) on the device capture dev;
    plans: (shift, L, D) per detection; extras: per detection, further keys of its record, or None"""
    from . import frontend as F
    if not found:
        return []
    Cn = self.topology.classes
    taps = {}
    for _, L, D in plans:
        if (L, D) not in taps:
            taps[L, D] = F.plan_taps(L, D)
    block, offsets = F.extract(dev, fmt, [(d.first_pair, d.stop_pair, shift, L, D, taps[L, D]) for d, (shift, L, D) in zip(found, plans)],
                               whole_frames=True)
    first = (offsets // 128).tolist()      # in windows
    if block.shape[0]:
        probs, labels, dbfs = self.predict_iq(block.reshape(-1), _cabi.IQ_CI16, normalize="rms", level=level, squelch_dbfs=squelch_dbfs,
                                              return_power=True)
    else:
        probs, labels, dbfs = _no_windows(Cn, dev.device)
    label = F.segment_votes(labels, offsets // 128, Cn).cpu().tolist()      # the one transfer of the K labels
    if as_numpy:
        probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
    out = []
    for k, (d, (shift, L, D)) in enumerate(zip(found, plans)):
        a, z = first[k], first[k + 1]
        out.append(dict(d._asdict(), shift=shift, interpolate=L, decimate=D, probs=probs[a:z], labels=labels[a:z], window_dbfs=dbfs[a:z],
                        windows=z - a, label=label[k], **(extras[k] if extras else {})))
    return out


def predict_channels(self, iq, sample_format, channels: int, decimate: Optional[int] = None, taps=None, tap_shift: Optional[int] = None,
                     hop: int = 128, level: float = 7.8e-3, squelch_dbfs: Optional[float] = None, batch_size: int = 0, balance=False):
    """A band with a channel raster in, "what is on every channel" out.  The capture is split into M = channels evenly spaced
    channels in one pass (frontend.channelize(iq, sample_format, channels, decimate, taps, tap_shift, whole_frames=True):
    decimate=None is M / 2, taps=None frontend.design_channelizer(M)), and every channel's stream is cut into windows `hop`
    output pairs apart and classified with predict_iq(..., "ci16", normalize="rms", level=, squelch_dbfs=, return_power=True).
    With hop == 128 that is ONE predict_iq call over the flat (M * n_out) block: the rows are whole frames, so no window
    straddles two channels; other hops go channel by channel.  Returns probs (M, W, C), labels (M, W), window_dbfs (M, W) and
    label (M,), int64: per channel the most frequent label among the windows the squelch let through (the smallest on a tie;
    -1 if there are none) -- scan_iq's rule.  Row k is the channel centred at frontend.channel_freqs(M)[k].  Device tensors
    for a device capture, numpy arrays for a numpy capture.  balance=True, or a coefficients tuple, corrects the capture's DC
    offset and I/Q imbalance first (frontend.balance); False (the default) changes nothing."""
    import torch
    from . import frontend as F
    fmt = F.sample_format_id(sample_format)
    as_numpy = not isinstance(iq, torch.Tensor)
    if balance is not False and balance is not None:
        iq, fmt, _ = F.balanced_capture(iq, fmt, balance, f"cuda:{self.device_index}")
    down = F.channelize(iq, fmt, channels, decimate=decimate, taps=taps, tap_shift=tap_shift, whole_frames=True,
                        device=f"cuda:{self.device_index}")
    M, n_out = down.shape[0], down.shape[1]
    kw = dict(batch_size=batch_size, hop=hop, normalize="rms", level=level, squelch_dbfs=squelch_dbfs, return_power=True)
    if hop == 128:
        probs, labels, dbfs = self.predict_iq(down.view(-1), _cabi.IQ_CI16, **kw)
        W = n_out // 128
        probs, labels, dbfs = probs.view(M, W, self.topology.classes), labels.view(M, W), dbfs.view(M, W)
    else:
        per = [self.predict_iq(down[k].reshape(-1), _cabi.IQ_CI16, **kw) for k in range(M)]
        probs, labels, dbfs = (torch.stack([p[i] for p in per]) for i in range(3))
    classes = torch.arange(self.topology.classes, dtype=labels.dtype, device=labels.device)
    counts = (labels[:, :, None] == classes).sum(1)      # (M, C): squelched windows (-1) count for no class
    label = torch.where(counts.sum(1) > 0, counts.argmax(1), torch.full((M,), -1, dtype=torch.int64, device=labels.device))
    if as_numpy:
        return probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy(), label.cpu().numpy()
    return probs, labels, dbfs, label
