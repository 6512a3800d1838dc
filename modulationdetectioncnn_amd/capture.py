"""The capture pipelines scan_iq, detect_iq and predict_channels as functions of a model: they use its predict_iq, device_index
and topology.classes, the rest is the frontend's pieces in order.  VTCNN2 binds the three as methods, hence `self`.  torch and
the frontend are imported at the first call, not with the package.  detect_stream, bound the same way, is detect_iq for a capture
that arrives in chunks: DetectStream runs the same pieces per chunk, _StreamCore keeps the books."""
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


# ---- detect_iq on a capture that arrives in chunks: the bookkeeping (no arithmetic), and the stream that runs it on the device ----
class _StreamCore:
    """detect_stream's bookkeeping: which spectrogram rows exist, which ratio rows are final, which components are closed, which
    were emitted, from which row on anything is still needed -- and nothing else.  It owns three sequences it only slices and
    joins (the raw components, 2 per pair; the spectrogram's rows; the ratio's rows) and calls five injected functions for all
    arithmetic: spectrogram(pairs) -> the rows of a stretch that starts on a row boundary; ratio(spec) -> the CFAR ratio of a
    slab of rows; components(ratio) -> records with row_first, row_stop, bin_first, bin_stop (frontend.spectrogram_components');
    classify(ratio, pairs, records) -> the records' dicts, rows and pairs counted from the window's first row; cat(a, b) -> a
    followed by b (a is None at the start).  DetectStream injects the device functions, tests/test_capture_stream.py the numpy
    restatements.  Rows are global (from the stream's start) throughout:
      S     spectrogram rows that exist: row r reads pairs [r R, r R + R + nfft/2), R = avg nfft / 2 (frontend.burst_pairs)
      F     ratio rows that are final: F = S - train_rows while the stream is open (the CFAR window of row r reads rows r -
            train_rows .. r + train_rows, cut off only at the slab's borders), F = S once it is closed
      t0    the first row anything still depends on: raw pairs from t0 R on and ratio rows [t0, F) are held
      mark  the F (or the forced cut) of the previous round: a component with row_stop + reach_rows <= mark was emitted then or
            earlier, whole or as part of a larger one, and is skipped -- the emit-once rule
    A component is closed when row_stop + reach_rows <= F: an on-cell links to rows at most reach_rows away (include/mdc.h,
    "spectrogram components"), the component's last row is row_stop - 1, so the last row that could still join it is row_stop
    - 1 + reach_rows, and that row is final iff it is < F.  A closed component lies whole inside [t0, F) -- it was open from its
    first row on, and t0 never passes an open component's first row -- so its record is the whole capture's."""

    def __init__(self, nfft, avg, train_rows, reach_rows, min_rows, min_bins, max_rows, spectrogram, ratio, components, classify, cat):
        self.nfft, self.avg, self.hop, self.R = int(nfft), int(avg), int(nfft) // 2, int(avg) * (int(nfft) // 2)
        self.train_rows, self.reach_rows, self.min_rows, self.min_bins, self.max_rows = int(train_rows), int(reach_rows), int(min_rows), int(min_bins), int(max_rows)
        if self.max_rows < 1:
            raise ValueError(f"max_rows must be >= 1 (got {max_rows!r})")
        self._spectrogram, self._ratio, self._components, self._classify, self._cat = spectrogram, ratio, components, classify, cat
        self.pairs_seen = self.S = self.F = self.t0 = self.mark = 0
        self.pair0 = self.spec0 = 0      # the first pair of self.pairs, the first row of self.spec; self.ratio starts at t0
        self.pairs = self.spec = self.ratio = None
        self.closed = False

    @property
    def pairs_held(self):
        return self.pairs_seen - self.pair0

    @property
    def pairs_bound(self):
        """pairs_held never exceeds this after a push: F - t0 <= max_rows, S - F <= train_rows, and fewer than R + nfft/2 pairs
        wait for their row"""
        return (self.max_rows + self.train_rows + 1) * self.R + self.hop - 1

    def rows_of(self, pairs):
        """frontend.spectrogram_rows(pairs, nfft, nfft // 2, avg)"""
        return 0 if pairs < self.nfft else ((pairs - self.nfft) // self.hop + 1) // self.avg

    def push(self, chunk, pairs):
        """chunk: `pairs` more pairs (2 * pairs components, in the sequence type the injected functions take)"""
        if self.closed:
            raise ValueError("push after close: the stream has ended")
        if pairs:
            self.pairs = self._cat(self.pairs, chunk)
            self.pairs_seen += int(pairs)
        return self._advance()

    def close(self):
        if self.closed:
            return []
        self.closed = True
        out = self._advance()
        self.abandon()
        return out

    def abandon(self):
        """closed, and nothing held"""
        self.closed = True
        self.pairs = self.spec = self.ratio = None
        self.pair0 = self.pairs_seen

    def _advance(self):
        R, T = self.R, self.train_rows
        S = self.rows_of(self.pairs_seen)
        if S > self.S:      # rows [self.S, S): from a slice that starts on a row boundary and holds exactly their pairs
            new = self._spectrogram(self.pairs[2 * (self.S * R - self.pair0):2 * (S * R + self.hop - self.pair0)])
            if len(new) != S - self.S:
                raise RuntimeError(f"the spectrogram of rows [{self.S}, {S}) came back with {len(new)} rows")
            self.spec, self.S = self._cat(self.spec, new), S
        F = self.S if self.closed else max(self.S - T, 0)
        if F > self.F:      # rows [self.F, F) of the ratio: the interior of a slab that reaches train_rows rows back and ahead
            lo, hi = max(self.F - T, 0), min(F + T, self.S)
            slab = self._ratio(self.spec[lo - self.spec0:hi - self.spec0])
            self.ratio, self.F = self._cat(self.ratio, slab[self.F - lo:F - lo]), F
            keep = max(F - T, 0)
            self.spec, self.spec0 = self.spec[keep - self.spec0:], keep
        out = self._emit()
        self.pairs, self.pair0 = (None, self.pairs_seen) if self.pairs is None else (self.pairs[2 * (self.t0 * R - self.pair0):], self.t0 * R)
        out.sort(key=lambda r: (r["first_pair"], r["centre"]))
        return out

    def _emit(self):
        """The rounds of one advance.  A round looks at the window [t0, E), E = min(F, t0 + max_rows): a larger step is taken in
        pieces, so that closing, t0 and the forced cuts depend on the rows alone and not on how they arrived."""
        out, M, reach = [], self.max_rows, self.reach_rows
        while self.ratio is not None:
            t0, E = self.t0, min(self.F, self.t0 + M)
            if E <= t0 or (E == self.mark and E == self.F and not self.closed):
                break      # no rows, or nothing new since the last round
            last = self.closed and E == self.F
            window = self.ratio[:E - t0]
            recs = self._components(window)
            first, stop = np.asarray(recs["row_first"], np.int64) + t0, np.asarray(recs["row_stop"], np.int64) + t0
            fresh = stop + reach > self.mark
            shut = fresh & (np.full(stop.shape, last) | (stop + reach <= E))
            open_ = fresh & ~shut
            t0_next = int(first[open_].min()) if open_.any() else E
            # forced cut: an open component holds all max_rows rows of the window (t0 cannot move) and rows beyond it are final
            forced = not last and E < self.F and t0_next + M <= E
            big = (stop - first >= self.min_rows) & (np.asarray(recs["bin_stop"], np.int64) - np.asarray(recs["bin_first"], np.int64) >= self.min_bins)
            for sel, cut in ((shut & big, False), (open_ & big, True)) if forced else ((shut & big, False),):
                if sel.any():
                    for r in self._classify(window, self.pairs[2 * (t0 * self.R - self.pair0):], recs[sel]):
                        out.append(dict(r, first_row=r["first_row"] + t0, stop_row=r["stop_row"] + t0, first_pair=r["first_pair"] + t0 * self.R,
                                        stop_pair=r["stop_pair"] + t0 * self.R, cut=cut))
            if forced:
                t0_next = E
            self.mark = E
            self.ratio, self.t0 = self.ratio[t0_next - t0:], t0_next
            if E == self.F:
                break
        if self.ratio is not None and len(self.ratio) == 0:
            self.ratio = None
        return out


class DetectStream:
    """detect_iq(floor="cfar", batched=True) on a capture that arrives in chunks (VTCNN2.detect_stream makes one).  push(chunk)
    takes any number of pairs -- a fraction of a spectrogram row, none, many rows -- as a numpy array or a device tensor in the
    stream's sample format and returns the records of every detection that CLOSED with this chunk; close() treats the end of
    the stream as the end of the capture and returns the rest (a second close() returns []; leaving the `with` block closes the
    stream and drops what it holds, so call close() yourself for its records); push after close is a ValueError.  The records
    of all calls together are detect_iq's of the concatenated capture, key for key and bit for bit, however the capture was
    cut into chunks -- first_row, stop_row, first_pair and stop_pair count from the stream's start; probs, labels and
    window_dbfs are numpy arrays when the chunk of the call that returns them was one -- plus one key, cut (below).  Two
    differences: a stream that ends before its first row gives [] where detect_iq raises, and max_rows.
    Why chunks can be exact: a spectrogram row reads only its own pairs, so new rows come from a slice that
    starts on a row boundary; the CFAR window is cut off only at the borders of what it is given, so a ratio row is final once
    train_rows rows after it exist, computed from a slab that reaches train_rows rows back; a component cannot grow once
    row_stop + reach_rows <= the final rows, is emitted in the round in which that first holds, and components smaller than
    min_rows / min_bins are dropped only then; extraction and refinement start their oscillators at each detection's first
    pair, so they run on the retained pairs with rebased offsets.  Per push: one spectrogram over the new rows, one CFAR over
    them plus 2 train_rows, one labelling of the retained rows (its count read back: the one synchronisation) and, when
    something closed, detect_iq's batched extraction and forward.
    pairs_seen: pairs pushed so far; rows_final: ratio rows that can no longer change; pairs_held: raw pairs retained on the
    device -- from the first row of the oldest detection still open.  max_rows bounds it against an emitter that never
    pauses: when more than max_rows rows from that row on are final, those max_rows rows are closed as if the capture ended
    there, every detection in them is emitted -- cut=True for one that touches their last reach_rows rows, the ones the cut
    goes through; cut=False for every other record -- and what follows becomes a new detection.  This is the one departure
    from the whole capture's records, and it depends on the rows alone, not on the chunking.  After every call pairs_held <=
    pairs_bound = (max_rows + train_rows + 1) * avg * nfft / 2 + nfft / 2 - 1: at most max_rows final rows are held, train_rows
    rows wait for rows after them, and fewer than one row's avg * nfft / 2 + nfft / 2 pairs wait for the rest of their row;
    during a push the chunk comes on top, and the joined buffer is a copy, so the peak is twice that."""

    def __init__(self, model, sample_format, nfft: int = 1024, avg: int = 8, threshold_db: float = 6.0, floor: str = "cfar", reach_rows: int = 2,
                 reach_bins: int = 3, min_rows: int = 3, min_bins: int = 3, level: float = 7.8e-3, squelch_dbfs: Optional[float] = None,
                 dc_guard: int = 1, refine: bool = False, min_line_db: float = 8.0, line_nfft: int = 1024, line_avg: int = 8, balance=False,
                 cfar=None, max_rows: int = 4096):
        from . import frontend as F
        if floor != "cfar":
            raise ValueError(f"a stream takes floor='cfar' only (got {floor!r}): the 'flat' and 'per-bin' floors are quantiles over the whole "
                             "capture, which no chunked run can reproduce")
        if balance is True:
            raise ValueError("balance=True estimates the coefficients from the whole capture, which a stream never holds: estimate them on "
                             "a first stretch (frontend.balance_stats, frontend.design_balance) and pass the coefficients tuple")
        self._fmt = F.sample_format_id(sample_format)      # "cu8", "ci8", "ci16": a cf32 chunk goes through frontend.quantize_cf32 first
        self._cfar = F.cfar_parameters(cfar)
        if not 0 <= self._cfar[0] <= _cabi.CFAR_MAX_TRAIN_ROWS:
            raise ValueError(f"train_rows must be in 0..{_cabi.CFAR_MAX_TRAIN_ROWS} (got {self._cfar[0]})")
        if not 0 <= int(reach_rows) <= _cabi.COMPONENTS_MAX_REACH:
            raise ValueError(f"reach_rows must be in 0..{_cabi.COMPONENTS_MAX_REACH} (got {reach_rows!r})")
        F.spectrogram_rows(0, nfft, int(nfft) // 2, avg)      # nfft and avg are checked here, before any chunk
        self._model, self._device = model, f"cuda:{model.device_index}"
        self._coeffs = None if balance is False or balance is None else balance
        self._dev_fmt = self._fmt if self._coeffs is None else _cabi.IQ_CI16
        self._balanced = {} if self._coeffs is None else dict(image_rejection_db=None)
        self._nfft, self._avg, self._reach, self._thresh_args, self._thresh = int(nfft), int(avg), (int(reach_rows), int(reach_bins)), (threshold_db, dc_guard), None
        self._level, self._squelch, self._refine, self._line = level, squelch_dbfs, bool(refine), (min_line_db, line_nfft, line_avg)
        self._as_numpy, self._ratios = False, {}      # _ratios: bandwidth -> (L, D) of frontend.channel_plan (a box has one of nfft widths)
        self._core =_StreamCore(nfft, avg, self._cfar[0], reach_rows, min_rows, min_bins, max_rows, self._spectrogram, self._ratio,
                                 self._components, self._classify, self._cat)

    pairs_seen = property(lambda self: self._core.pairs_seen)
    pairs_held = property(lambda self: self._core.pairs_held)
    pairs_bound = property(lambda self: self._core.pairs_bound)
    rows_final = property(lambda self: self._core.F)

    # the five functions of _StreamCore, on the device
    @staticmethod
    def _cat(a, b):
        import torch
        return b.clone() if a is None else torch.cat((a, b))      # (a clone: the first chunk may be the caller's own tensor)

    def _spectrogram(self, pairs):
        from . import frontend as F
        return F.spectrogram(pairs, self._dev_fmt, nfft=self._nfft, avg=self._avg)

    def _ratio(self, spec):
        from . import frontend as F
        return F.cfar_floor(spec, *self._cfar, return_ratio=True)[1]

    def _threshold(self, device):
        from . import frontend as F
        if self._thresh is None:
            self._thresh = F.cfar_threshold(self._nfft, *self._thresh_args, device=device)
        return self._thresh

    def _components(self, ratio, capacity: int = 65536):
        from . import frontend as F
        _, records, count = F.spectrogram_components(ratio, self._threshold(ratio.device), *self._reach, capacity)
        if count > capacity:
            raise ValueError(f"the retained rows hold {count} components, capacity is {capacity}: raise the threshold")
        return records

    def _classify(self, ratio, pairs, records):
        from . import frontend as F
        found = F.detections_from_components(ratio, self._threshold(ratio.device), records, len(records), 1, 1, None, self._avg)
        for d in found:      # frontend.channel_plans, with its search per distinct bandwidth made once per stream, not once per push
            if d.bandwidth not in self._ratios:
                self._ratios[d.bandwidth] = F.channel_plans([(d.centre, d.bandwidth)])[0][1:3]
        plans, extras = [(-float(d.centre),) + self._ratios[d.bandwidth] for d in found], None
        if self._refine and found:
            plans, extras = _refine_detections(pairs, self._dev_fmt, found, plans, *self._line)
        return [dict(r, **self._balanced) for r in _classify_detections(self._model, pairs, self._dev_fmt, found, plans, extras, self._level,
                                                                        self._squelch, self._as_numpy)]

    def push(self, chunk):
        import torch
        from . import frontend as F
        if self._core.closed:
            raise ValueError("push after close: the stream has ended")
        self._as_numpy = not isinstance(chunk, torch.Tensor)
        n = int(chunk.numel()) if isinstance(chunk, torch.Tensor) else int(np.asarray(chunk).size)
        if n % 2:
            raise ValueError(f"a chunk holds whole (I,Q) pairs: {n} components is an odd number")
        if n == 0:
            return self._core.push(None, 0)
        dev = F._device_samples(chunk, self._fmt, self._device)
        if self._coeffs is not None:
            dev = F.balance(dev, self._fmt, self._coeffs).view(-1)
        return self._core.push(dev, n // 2)

    def close(self):
        return self._core.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        else:      # the block failed: no more device work, only let go of what is held
            self._core.abandon()
        return False


def detect_stream(self, sample_format, **kw):
    """detect_iq for a capture that does not fit on the device, or never ends: a DetectStream (which see) that takes the
    capture a chunk at a time -- push(chunk) returns the detections that closed with it, close() the rest -- and gives, all
    calls together, the records of detect_iq(whole capture, sample_format, floor="cfar", batched=True, ...), bit for bit, for
    any chunking.  Keywords: detect_iq's nfft, avg, threshold_db, cfar, reach_rows, reach_bins, min_rows, min_bins, level,
    squelch_dbfs, dc_guard, refine, min_line_db, line_nfft, line_avg, and balance (False, or a coefficients tuple; True would
    estimate from the whole capture: ValueError); max_rows (default 4096) bounds what the stream holds against an emitter that
    never pauses.  A floor= other than "cfar" is a ValueError: "flat" and "per-bin" are quantiles over the whole capture.
    "cf32" chunks go through frontend.quantize_cf32(chunk, full_scale=...) first, which is stateless per chunk."""
    return DetectStream(self, sample_format, **kw)
