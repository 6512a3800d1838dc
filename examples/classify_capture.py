#!/usr/bin/env python3
"""An SDR capture (interleaved I,Q samples: unsigned bytes of an RTL-SDR -- the front-end of the reference's README.md:5 --,
signed bytes of a HackRF, or signed 16-bit little-endian samples of a USRP / SDRplay / bladeRF / Airspy) -> one label per
window, whatever the gain and DC offset of the capture: each window is brought to the level the nets were trained at
(predict_iq(normalize="rms")), and windows whose power lies below the squelch get label -1.

    python examples/classify_capture.py capture.bin --weights tests/golden/weights/convmodrecnets_CNN2_0.5.npz --hop 64 --squelch -35
A wideband capture -- the signal away from the tuner's centre, the sample rate above the nets' 8 samples per symbol -- is tuned,
low-pass filtered and decimated on the device first (frontend.ddc, exact integer arithmetic); hop, level and squelch then apply
to the decimated stream:

    python examples/classify_capture.py capture.bin --format cu8 --rate 2.4e6 --shift-hz -480e3 --decimate 12

A rate that no integer brings to 8 samples per symbol is resampled by a rational factor instead (frontend.resample, the same
exact arithmetic): give the factor as --interpolate L --decimate D, or let --symbol-rate choose it from --rate -- 2.4 MS/s on a
250 ksym/s signal is 9.6 samples per symbol, and 5/6 makes that 8:

    python examples/classify_capture.py capture.bin --rate 2.4e6 --symbol-rate 250e3 --shift-hz -480e3

When it is not known where in the band the signals are, --scan finds out: the capture's power spectrum (frontend.spectrogram, on
the device) is searched for emitters, each one is tuned, resampled and classified (VTCNN2.scan_iq), and one line per emitter
comes out -- in Hz when --rate is given, else in cycles per sample:

    python examples/classify_capture.py capture.bin --format ci16 --rate 2.4e6 --scan --nfft 1024 --threshold 6

With --refine the scan takes each emitter's symbol rate and carrier from its spectral lines instead of its width and centroid
(frontend.estimate_symbol_rate, estimate_carrier_offset: the spectra of |x|^2 and of x^2 / x^4, on the device) and prints them
as two more columns.

With --bursts the scan also finds emitters that are on only now and then -- push-to-talk, telemetry, packet traffic --, which the
spectrum averaged over the whole capture dilutes: the emitters are searched in the level each bin reaches in its top 1 - HOLD of
the spectrogram's rows (--hold, default 0.98; frontend.spectrum_quantiles, on the device), each emitter's bursts are cut out of
its band power over time, only windows inside a burst are classified, and two more columns give the number of bursts and the
share of the time the emitter was on:

    python examples/classify_capture.py capture.bin --format ci16 --scan --bursts --hold 0.98

With --detections the band is searched in two dimensions instead (VTCNN2.detect_iq): the spectrogram is thresholded cell by cell,
neighbouring cells are joined into boxes in time and frequency on the device (frontend.find_detections), and only the pairs inside
a box are tuned, resampled and classified -- one line per box.  That finds what both scans above miss: a frequency hopper (one
line per dwell), two emitters that use the same bins at different times (two lines), a single short packet:

    python examples/classify_capture.py capture.bin --format ci16 --detections --threshold 6

Add --batched for a busy band: all boxes are then extracted in one launch and classified in one forward (the same lines, bit for
bit; frontend.extract, detect_iq(batched=True)) instead of a few launches and one synchronisation per box.  Add --refine to
take each box's symbol rate and carrier from its spectral lines instead of its width and centroid (detect_iq(refine=True);
with --batched all boxes' line spectra come from one frontend.line_spectra and one frontend.find_lines); two more columns, as
with --scan --refine.  Add --floor cfar where the noise floor is neither flat nor still -- a coloured front-end, an AGC or gain
step, a neighbour keying up: every cell is then held against an order statistic of the cells AROUND it (frontend.cfar_floor,
2-D order-statistic CFAR on the device; --cfar TR,TB,GR,GB,RANK sets the training window, the guard and the rank) instead of one
level per bin for the whole capture:

    python examples/classify_capture.py capture.bin --format ci16 --detections --floor cfar --cfar 8,32,2,8,0.5

A recording that does not fit on the device -- minutes of a wideband receiver -- takes --stream CHUNK_PAIRS on top of that: the file
is read CHUNK_PAIRS pairs at a time (never more than one chunk on the host), every chunk is pushed into VTCNN2.detect_stream, and
each box is printed when it has closed.  The boxes are those of the run without --stream, bit for bit, whatever the chunk size;
only the local floor allows that, so --stream is an error without --detections --floor cfar.  --max-rows bounds what is held for
an emitter that never pauses (its box is then cut, and the line says so):

    python examples/classify_capture.py long.bin --format ci16 --detections --floor cfar --stream 1048576

A band with a channel raster -- PMR / LMR, GSM, FM broadcast, ISM sub-bands -- is split into all its M evenly spaced channels in
one pass instead (frontend.channelize, a polyphase filter bank on the device; VTCNN2.predict_channels), one line per channel:

    python examples/classify_capture.py capture.bin --format ci16 --rate 2.4e6 --channels 16

An uncalibrated zero-IF receiver (HackRF, bladeRF, USRP, an RTL-SDR with a direct-conversion tuner) mirrors every emitter at +f
to -f, 20 .. 40 dB down, and --scan, --detections and --channels then list a strong emitter's image as an emitter.  --balance
removes the receiver's DC offset and I/Q imbalance first, estimated from the capture itself (frontend.balance, exact integers on
the device), and --scan prints the image rejection it found:

    python examples/classify_capture.py capture.bin --format ci8 --scan --balance
    python examples/classify_capture.py --format ci16 --scan --imbalance [--balance]      # the synthetic band 1 dB / 5 degrees off: 4 lines, 3 with --balance

A float capture -- GNU Radio's file sink, UHD's fc32, SigMF's cf32_le: interleaved complex float32 -- is turned into 16-bit
integers once, on the device, in front of every mode above (frontend.quantize_cf32: one exact rounding per sample, a pair with a
NaN or Inf becomes (0, 0) and is counted).  --full-scale F says which float amplitude is the ADC's full scale (UHD and GNU Radio
write +-1.0); without it the gain is the power of two that puts the capture's peak into 13 to 14 bits, found from a histogram
of the samples' exponents, and --clip-fraction P gives up that share of the samples to glitches.  One line reports the gain and
the counts:

    python examples/classify_capture.py capture.cf32 --format cf32 --full-scale 1.0 --rate 2.4e6 --scan

Without a capture file it classifies a synthetic one (--format cf32: the float copy, / 32768, of the "ci16" one): bursts of tones at three gains with silence between them (--scan: a
band of three QPSK emitters of different widths over noise and a DC offset, with --bursts a fourth that is on 4.5 % of the time; --detections: a QPSK hopper of six dwells and a second emitter on an
earlier dwell's bins; --channels: QPSK on two channels of the raster)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulationdetectioncnn_amd import VTCNN2      # noqa: E402


DTYPES = {"cu8": np.uint8, "ci8": np.int8, "ci16": "<i2"}


def quantize(x, full_scale=None, clip_fraction=0.0):
    """--format cf32: the float capture x (interleaved float32) as a "ci16" one (frontend.quantize_cf32), and one line about it.
    Returns (int16 array, "ci16") for the functions below; a pipeline would keep the device tensor."""
    from modulationdetectioncnn_amd import frontend
    out, r = frontend.quantize_cf32(x[:x.size // 2 * 2], full_scale=full_scale, clip_fraction=clip_fraction, return_report=True)
    print(f"cf32: {r['pairs']} pairs, gain {r['gain']:g} (0 dBFS is the float amplitude {r['full_scale']:g}), "
          f"{r['nonfinite_pairs']} non-finite pairs zeroed, {r['clipped']} components clipped")
    return out.cpu().numpy(), "ci16"


def load(a, synthetic):
    """(samples, format) of the capture file, or of synthetic(format) without one; --format cf32 goes through quantize"""
    if a.format != "cf32":
        return (np.fromfile(a.capture, DTYPES[a.format]) if a.capture else synthetic(a.format)), a.format
    x = np.fromfile(a.capture, "<f4") if a.capture else synthetic("ci16").astype(np.float32) / np.float32(32768.0)
    return quantize(x, a.full_scale, a.clip_fraction)


def synthetic_capture(fmt="cu8", seed=1):
    rng = np.random.default_rng(seed)
    parts = []
    for gain in (4.0, 30.0, 110.0):
        t = np.arange(128 * 40)
        burst = gain * np.exp(2j * np.pi * (0.07 * t + rng.uniform()))
        quiet = np.zeros(128 * 20, complex)
        z = np.concatenate([burst, quiet]) + 0.4 * (rng.standard_normal(128 * 60) + 1j * rng.standard_normal(128 * 60))
        parts.append(z)
    z = np.concatenate(parts)
    if fmt == "cu8":
        iq = np.stack([z.real + 129.3, z.imag + 126.1], axis=1)      # a tuner's DC offset: the midpoint is not 127.5
        return np.clip(np.rint(iq), 0, 255).astype(np.uint8).reshape(-1)
    k = 1.0 if fmt == "ci8" else 256.0                                 # the same signal in the wider format's LSBs
    iq = np.stack([k * (z.real + 1.8), k * (z.imag - 1.4)], axis=1)
    lo, hi = (-128, 127) if fmt == "ci8" else (-32768, 32767)
    return np.clip(np.rint(iq), lo, hi).astype(DTYPES[fmt]).reshape(-1)


BAND_EMITTERS = ((96, -0.31, 0.02), (48, 0.12, 0.05), (20, 0.36, 0.01))      # samples per symbol, centre, rms of full scale
# the band as an uncalibrated zero-IF receiver delivers it (--imbalance): the Q rail 1 dB up and 5 degrees off, which mirrors every
# emitter 22.8 dB down.  The emitter at -0.31 is weaker here, so that only the strong one's image, at -0.12, clears the threshold
IMBALANCED_EMITTERS = ((96, -0.31, 0.004), (48, 0.12, 0.05), (20, 0.36, 0.01))
IMBALANCE = (1.0, 5.0)


def synthetic_band(fmt="ci16", seed=1, pairs=1 << 18, bursty=False, emitters=BAND_EMITTERS, imbalance=None):
    """Three QPSK emitters with a root-raised-cosine pulse (beta 0.35) at 96 / 48 / 20 samples per symbol, centred at -0.31 / +0.12 /
    +0.36 cycles per sample with rms 0.02 / 0.05 / 0.01 of full scale, over noise of rms 0.002 and a tuner's DC offset.  bursty: a
    fourth one at 32 samples per symbol, centred at -0.08 with rms 0.003, that is on only during [0.40, 0.43) and [0.80, 0.815)
    of the capture.  emitters: other (samples per symbol, centre, rms) triples; imbalance: (gain in dB, phase in degrees) of the
    receiver's Q rail against its I rail, applied to signals and noise before the DC offset and the quantiser."""
    rng = np.random.default_rng(seed)
    beta, n, z = 0.35, np.arange(pairs), np.zeros(pairs, complex)

    def emitter(rng, sps, fc, amp, on=None):
        t = np.arange(-12 * sps, 12 * sps + 1) / sps + 1e-9          # (off the pulse's removable singularities)
        h = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
        sym = rng.choice([-1.0, 1.0], pairs // sps + 2) + 1j * rng.choice([-1.0, 1.0], pairs // sps + 2)
        up = np.zeros(sym.size * sps, complex)
        up[::sps] = sym
        base = np.convolve(up, h, mode="same")[:pairs]
        base = amp / np.sqrt(np.mean(np.abs(base) ** 2)) * base
        if on is not None:
            gate = np.zeros(pairs)
            for a, b in on:
                gate[int(a * pairs):int(b * pairs)] = 1.0
            base = base * gate
        return base * np.exp(2j * np.pi * fc * n)

    for sps, fc, amp in emitters:
        z += emitter(rng, sps, fc, amp)
    if bursty:      # symbols from a stream of its own: the draws of everything else stay what they are
        z += emitter(np.random.default_rng(seed + 100), 32, -0.08, 0.003, on=((0.40, 0.43), (0.80, 0.815)))
    z += 0.002 / np.sqrt(2) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    if imbalance is not None:      # I = Re z, Q = g Im(e^{-j phi} z)
        g, phi = 10.0 ** (imbalance[0] / 20.0), np.radians(imbalance[1])
        z = z.real + 1j * g * (z.imag * np.cos(phi) - z.real * np.sin(phi))
    z += 0.01 - 0.02j
    if fmt == "cu8":
        return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    full, lo, hi = (128.0, -128, 127) if fmt == "ci8" else (32768.0, -32768, 32767)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * full), lo, hi).astype(DTYPES[fmt]).reshape(-1)


def scan(model, iq, fmt, nfft=1024, threshold_db=6.0, rate=None, hop=128, level=7.8e-3, squelch=-60.0, refine=False, bursts=False, hold=0.98,
         balance=False):
    """Print one line per emitter of the capture (VTCNN2.scan_iq) and return the records.  rate: Hz columns instead of cycles per sample.
    refine: symbol rate and carrier from the emitter's spectral lines (scan_iq's refine=True), as two more columns -- the symbol
    rate ("-" where no line was found) and the refined centre.  bursts: the scan for intermittent emitters (scan_iq's bursts=True
    on the `hold` quantile spectrum, spectrogram rows of 2 segments), as two more columns -- the number of bursts and the share of
    the rows the emitter was on.  balance: correct the receiver's DC offset and I/Q imbalance first (scan_iq's balance=True), and
    print the capture's image rejection before the correction."""
    more = dict(bursts=True, hold=hold, avg=2) if bursts else {}
    if balance:
        more["balance"] = True
    found = model.scan_iq(iq[:iq.size // 2 * 2], fmt, nfft=nfft, threshold_db=threshold_db, hop=hop, level=level, squelch_dbfs=squelch,
                          refine=refine, **more)
    k, unit = (rate, "Hz") if rate else (1.0, "cyc/sample")
    print(f"{len(found)} emitters ({unit})" + (f", image rejection before correction {found[0]['image_rejection_db']:.1f} dB" if balance and found else ""))
    print(f"{'centre':>12s} {'bandwidth':>12s} {'dBFS':>7s} {'SNR dB':>7s} {'L/D':>7s} {'windows':>8s} {'open':>6s} {'label':>6s}"
          + (f" {'symbol rate':>12s} {'refined':>12s}" if refine else "") + (f" {'bursts':>7s} {'duty':>6s}" if bursts else ""))
    for e in found:
        labels = np.asarray(e["labels"])
        more = ""
        if refine:
            symbol = "-" if e["symbol_rate"] is None else f"{e['symbol_rate'] * k:.6g}"
            more = f" {symbol:>12s} {(e['centre'] + e['carrier_offset']) * k:12.8g}"
        if bursts:
            more += f" {len(e['bursts']):7d} {e['duty']:6.3f}"
        print(f"{e['centre'] * k:12.6g} {e['bandwidth'] * k:12.6g} {e['power_dbfs']:7.1f} {e['snr_db']:7.1f} "
              f"{str(e['interpolate']) + '/' + str(e['decimate']):>7s} {labels.size:8d} {int((labels >= 0).sum()):6d} {e['label']:6d}{more}")
    return found


def synthetic_hopper(fmt="ci16", seed=1, pairs=1 << 19):
    """A frequency hopper over noise of rms 0.002: six QPSK dwells (root-raised-cosine, 32 samples per symbol, rms 0.002 of full scale:
    about 14 dB per bin of 1024) of 65,536 pairs, 8,192 pairs apart, centred at -0.475 / +0.21 / +0.02 / -0.18 / +0.475 / +0.33 cycles per sample, and a second emitter
    of the same kind on the second dwell's bins during the last dwell: seven boxes in time and frequency."""
    rng = np.random.default_rng(seed)
    beta, sps, n = 0.35, 32, np.arange(pairs)
    z = 0.002 / np.sqrt(2) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    centres = (-0.475, 0.21, 20 / 1024, -0.18, 0.475, 0.33)
    spans = [((1 << 14) + i * ((1 << 16) + (1 << 13)), (1 << 14) + i * ((1 << 16) + (1 << 13)) + (1 << 16)) for i in range(6)]
    t = np.arange(-12 * sps, 12 * sps + 1) / sps + 1e-9          # (off the pulse's removable singularities)
    h = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
    for (a, b), fc in list(zip(spans, centres)) + [(spans[5], centres[1])]:
        sym = rng.choice([-1.0, 1.0], (b - a) // sps + 2) + 1j * rng.choice([-1.0, 1.0], (b - a) // sps + 2)
        up = np.zeros(sym.size * sps, complex)
        up[::sps] = sym
        base = np.convolve(up, h, mode="same")[:b - a]
        z[a:b] += 0.002 / np.sqrt(np.mean(np.abs(base) ** 2)) * base * np.exp(2j * np.pi * fc * n[a:b])
    if fmt == "cu8":
        return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    full, lo, hi = (128.0, -128, 127) if fmt == "ci8" else (32768.0, -32768, 32767)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * full), lo, hi).astype(DTYPES[fmt]).reshape(-1)


def detections(model, iq, fmt, nfft=1024, threshold_db=6.0, rate=None, hop=128, level=7.8e-3, squelch=-60.0, batched=False, refine=False,
               balance=False, floor="flat", cfar=None):
    """Print one line per detection of the capture (VTCNN2.detect_iq: boxes in time and frequency) and return the records: the
    box's span in input pairs, centre and width (Hz with rate, else cycles per sample), the peak over the threshold, the plan and
    the label.  batched: all boxes in one extraction launch and one forward (needs hop == 128); the same records.  refine: symbol
    rate and carrier from each box's spectral lines (detect_iq's refine=True), as two more columns -- the symbol rate ("-" where no
    line was found) and the refined centre.  balance: correct the receiver's DC offset and I/Q imbalance first (detect_iq's
    balance=True).  floor: detect_iq's noise floor -- "flat", "per-bin" or "cfar", the local order-statistic floor per cell, with
    cfar = (train_rows, train_bins, guard_rows, guard_bins, rank) or None for the defaults; the peak column is then dB above the
    local floor's threshold."""
    more = dict(refine=True) if refine else {}
    if balance:
        more["balance"] = True
    if floor != "flat":
        more["floor"] = floor
    if cfar is not None:
        more["cfar"] = cfar
    found = model.detect_iq(iq[:iq.size // 2 * 2], fmt, nfft=nfft, threshold_db=threshold_db, hop=hop, level=level, squelch_dbfs=squelch,
                            batched=batched, **more)
    k, unit = (rate, "Hz") if rate else (1.0, "cyc/sample")
    print(f"{len(found)} detections ({unit})")
    print(f"{'first pair':>12s} {'stop pair':>12s} {'centre':>12s} {'bandwidth':>12s} {'peak dB':>8s} {'L/D':>7s} {'windows':>8s} {'open':>6s} {'label':>6s}"
          + (f" {'symbol rate':>12s} {'refined':>12s}" if refine else ""))
    for d in found:
        labels = np.asarray(d["labels"])
        more = ""
        if refine:
            symbol = "-" if d["symbol_rate"] is None else f"{d['symbol_rate'] * k:.6g}"
            more = f" {symbol:>12s} {(d['centre'] + d['carrier_offset']) * k:12.8g}"
        print(f"{d['first_pair']:12d} {d['stop_pair']:12d} {d['centre'] * k:12.6g} {d['bandwidth'] * k:12.6g} {d['snr_db']:8.1f} "
              f"{str(d['interpolate']) + '/' + str(d['decimate']):>7s} {d['windows']:8d} {int((labels >= 0).sum()):6d} {d['label']:6d}{more}")
    return found


def file_chunks(path, fmt, chunk_pairs, full_scale=None):
    """--stream: the capture file, chunk_pairs pairs at a time -- never more than one chunk on the host.  "cf32" chunks are
    quantised on the device with the fixed --full-scale (frontend.quantize_cf32 is stateless per chunk with one)."""
    dtype = np.dtype("<f4") if fmt == "cf32" else np.dtype(DTYPES[fmt])
    with open(path, "rb") as f:
        while True:
            x = np.fromfile(f, dtype, 2 * chunk_pairs)
            if x.size < 2:
                return
            x = x[:x.size // 2 * 2]
            if fmt == "cf32":
                from modulationdetectioncnn_amd import frontend
                x = frontend.quantize_cf32(x, full_scale=full_scale).reshape(-1)
            yield x


def stream_detections(model, chunks, fmt, nfft=1024, threshold_db=6.0, rate=None, level=7.8e-3, squelch=-60.0, refine=False, cfar=None,
                      max_rows=4096):
    """detections(..., batched=True, floor="cfar") for a capture that arrives as an iterable of chunks (VTCNN2.detect_stream):
    the same lines, each printed when its box has closed -- in order of closing, not of first pair -- and the count at the end.
    A box that max_rows cut short (an emitter that never pauses) is marked with a trailing `cut`."""
    k, unit = (rate, "Hz") if rate else (1.0, "cyc/sample")
    print(f"{'first pair':>12s} {'stop pair':>12s} {'centre':>12s} {'bandwidth':>12s} {'peak dB':>8s} {'L/D':>7s} {'windows':>8s} {'open':>6s} {'label':>6s}"
          + (f" {'symbol rate':>12s} {'refined':>12s}" if refine else ""))
    found, held = [], 0

    def show(records):
        for d in records:
            labels = np.asarray(d["labels"].cpu() if hasattr(d["labels"], "cpu") else d["labels"])
            more = ""
            if refine:
                symbol = "-" if d["symbol_rate"] is None else f"{d['symbol_rate'] * k:.6g}"
                more = f" {symbol:>12s} {(d['centre'] + d['carrier_offset']) * k:12.8g}"
            print(f"{d['first_pair']:12d} {d['stop_pair']:12d} {d['centre'] * k:12.6g} {d['bandwidth'] * k:12.6g} {d['snr_db']:8.1f} "
                  f"{str(d['interpolate']) + '/' + str(d['decimate']):>7s} {d['windows']:8d} {int((labels >= 0).sum()):6d} {d['label']:6d}{more}"
                  + (" cut" if d["cut"] else ""), flush=True)
            found.append(d)

    fmt = "ci16" if fmt == "cf32" else fmt
    with model.detect_stream(fmt, nfft=nfft, threshold_db=threshold_db, level=level, squelch_dbfs=squelch, refine=refine, cfar=cfar, max_rows=max_rows) as s:
        for chunk in chunks:
            show(s.push(chunk))
            held = max(held, s.pairs_held)
        show(s.close())
    print(f"{len(found)} detections ({unit}) in {s.pairs_seen} pairs; at most {held} pairs held between chunks")
    return found


def synthetic_raster(fmt="ci16", channels=16, seed=1, pairs=1 << 16):
    """QPSK with a root-raised-cosine pulse (beta 0.35), 8 samples per symbol at the channelizer's default output rate 2 / M, on the
    raster's channels 3 and M - 5, rms 0.05 of full scale each, over noise of rms 0.002."""
    rng = np.random.default_rng(seed)
    M, sps, beta, n, z = int(channels), 4 * int(channels), 0.35, np.arange(pairs), np.zeros(pairs, complex)
    for k in (3, M - 5):
        t = np.arange(-12 * sps, 12 * sps + 1) / sps + 1e-9          # (off the pulse's removable singularities)
        h = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
        sym = rng.choice([-1.0, 1.0], pairs // sps + 2) + 1j * rng.choice([-1.0, 1.0], pairs // sps + 2)
        up = np.zeros(sym.size * sps, complex)
        up[::sps] = sym
        base = np.convolve(up, h, mode="same")[:pairs]
        z += 0.05 / np.sqrt(np.mean(np.abs(base) ** 2)) * base * np.exp(2j * np.pi * k / M * n)
    z += 0.002 / np.sqrt(2) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    if fmt == "cu8":
        return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    full, lo, hi = (128.0, -128, 127) if fmt == "ci8" else (32768.0, -32768, 32767)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * full), lo, hi).astype(DTYPES[fmt]).reshape(-1)


def channels(model, iq, fmt, nchannels, rate=None, hop=128, level=7.8e-3, squelch=-60.0, balance=False):
    """Print one line per channel of the raster (VTCNN2.predict_channels: M = nchannels channels, each 2 x oversampled) and return
    (labels, window dBFS, label per channel).  rate: the centres in Hz instead of cycles per sample.  balance: correct the
    receiver's DC offset and I/Q imbalance first (predict_channels' balance=True)."""
    from modulationdetectioncnn_amd import frontend
    more = dict(balance=True) if balance else {}
    _, labels, dbfs, label = model.predict_channels(iq[:iq.size // 2 * 2], fmt, nchannels, hop=hop, level=level, squelch_dbfs=squelch, **more)
    k, unit = (rate, "Hz") if rate else (1.0, "cyc/sample")
    print(f"{nchannels} channels ({unit}), {labels.shape[1]} windows each")
    print(f"{'centre':>12s} {'median dBFS':>12s} {'open':>6s} {'label':>6s}")
    for fc, l, d, verdict in zip(frontend.channel_freqs(nchannels), labels, dbfs, label):
        median = float(np.median(d)) if d.size else float("nan")
        print(f"{fc * k:12.6g} {median:12.1f} {int((l >= 0).sum()):6d} {int(verdict):6d}")
    return labels, dbfs, label


def classify(model, iq, fmt, hop=128, level=7.8e-3, squelch=-35.0, shift=0.0, decimate=1, interpolate=1):
    """(probs, labels, dBFS) per window.  shift (cycles per sample, ADDED to the capture) / decimate: the capture is tuned,
    low-pass filtered (frontend.design_lowpass) and decimated on the device first, and the windows are cut from that stream.
    interpolate != 1: resampled by interpolate / decimate instead (frontend.resample with frontend.design_resampler's taps)."""
    ddc = {}
    if interpolate != 1:
        import math
        from modulationdetectioncnn_amd import frontend
        g = math.gcd(interpolate, decimate)
        L, D = interpolate // g, decimate // g
        if L == 1:                  # an integer decimation after all
            return classify(model, iq, fmt, hop, level, squelch, shift, D)
        taps = frontend.design_resampler(L, D)
        iq = iq[:iq.size // 2 * 2]
        down = frontend.resample(iq, fmt, shift=shift, interpolate=L, decimate=D, taps=taps, device=f"cuda:{model.device_index}")
        if hop == 128:              # disjoint frames want whole frames of the RESAMPLED stream
            down = down[:frontend.resample_out_count(iq.size // 2, taps.size, L, D) // 128 * 128]
        res = model.predict_iq(down.reshape(-1), "ci16", hop=hop, normalize="rms", level=level, squelch_dbfs=squelch, return_power=True)
        return tuple(r.cpu().numpy() for r in res)
    if shift != 0.0 or decimate != 1:
        from modulationdetectioncnn_amd import frontend
        ddc = dict(shift=shift, decimate=decimate)
        ntaps = 8 * decimate        # frontend.design_lowpass's default
        if decimate == 1:           # a pure frequency shift: one tap of (all but) unit gain
            ddc["taps"], ntaps = np.array([32767], np.int16), 1
        if hop == 128:              # disjoint frames want whole frames of the DECIMATED stream: trim the input to what gives them
            keep = frontend.ddc_out_count(iq.size // 2, ntaps, decimate) // 128 * 128
            iq = iq[:2 * ((keep - 1) * decimate + ntaps)] if keep else iq[:0]
        else:
            iq = iq[:iq.size // 2 * 2]
    else:
        iq = iq[:iq.size // 256 * 256] if hop == 128 else iq[:iq.size // 2 * 2]
    return model.predict_iq(iq, fmt, hop=hop, normalize="rms", level=level, squelch_dbfs=squelch, return_power=True, **ddc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("capture", nargs="?", help="file of interleaved samples I0 Q0 I1 Q1 ... in --format")
    ap.add_argument("--format", choices=["cu8", "ci8", "ci16", "cf32"], default="cu8",
                    help="sample format: unsigned bytes (RTL-SDR), signed bytes (HackRF), signed 16-bit little-endian (USRP sc16, ...), "
                         "complex float32 (GNU Radio, UHD fc32, SigMF cf32_le)")
    ap.add_argument("--full-scale", type=float, default=None,
                    help="with --format cf32: the float amplitude of the ADC's full scale (UHD, GNU Radio: 1.0); default: measured")
    ap.add_argument("--clip-fraction", type=float, default=0.0,
                    help="with --format cf32 and a measured gain: the share of the samples that may clip (glitches)")
    ap.add_argument("--weights", default=None, help=".h5 / .npz of a deployed net (default: synthetic weights)")
    ap.add_argument("--hop", type=int, default=128, help="sample pairs between windows (128: disjoint frames)")
    ap.add_argument("--level", type=float, default=7.8e-3, help="complex rms every window is normalised to")
    ap.add_argument("--squelch", type=float, default=-35.0, help="dBFS below which a window gets label -1")
    ap.add_argument("--rate", type=float, default=1.0, help="sample rate of the capture in Hz (only scales --shift-hz)")
    ap.add_argument("--shift-hz", type=float, default=0.0,
                    help="frequency ADDED to the capture before filtering, in Hz at --rate: a signal at +f0 from the tuner's centre wants -f0")
    ap.add_argument("--decimate", type=int, default=1, help="keep one sample in this many after the anti-alias low-pass (1..256)")
    ap.add_argument("--interpolate", type=int, default=1, help="with --decimate D: resample by this L over D (1..32)")
    ap.add_argument("--symbol-rate", type=float, default=None,
                    help="symbols per second of the signal: picks --interpolate / --decimate so that --rate becomes 8 samples per symbol")
    ap.add_argument("--scan", action="store_true", help="find the emitters in the band first and classify each one (ignores --shift-hz, --decimate, ...)")
    ap.add_argument("--nfft", type=int, default=1024, help="with --scan: bins of the spectrum (a power of two in 64..4096)")
    ap.add_argument("--threshold", type=float, default=6.0, help="with --scan: dB above the noise floor at which a bin belongs to an emitter")
    ap.add_argument("--refine", action="store_true",
                    help="with --scan or --detections: symbol rate and carrier of each emitter from its spectral lines; two more columns")
    ap.add_argument("--bursts", action="store_true",
                    help="with --scan: find intermittent emitters too and classify only inside their bursts; two more columns")
    ap.add_argument("--hold", type=float, default=0.98, help="with --bursts: the quantile over time of each bin that the emitters are searched in")
    ap.add_argument("--channels", type=int, default=0,
                    help="split the band into this many evenly spaced channels (a power of two in 8..1024) and classify every one")
    ap.add_argument("--detections", action="store_true",
                    help="search the spectrogram in two dimensions (hoppers, emitters sharing bins, single packets): one line per box in "
                         "time and frequency; uses --nfft and --threshold")
    ap.add_argument("--batched", action="store_true",
                    help="with --detections: extract all boxes in one launch and classify them in one forward (the same lines; needs --hop 128)")
    ap.add_argument("--floor", choices=["flat", "per-bin", "cfar"], default="flat",
                    help="with --detections: the noise floor -- one level for the band, every bin's median over time, or a local "
                         "order-statistic floor per cell (follows a coloured front-end and a gain step)")
    ap.add_argument("--cfar", default=None, metavar="TR,TB,GR,GB,RANK",
                    help="with --floor cfar: training rows and bins, guard rows and bins, rank in [0, 1] (default 8,32,2,8,0.5)")
    ap.add_argument("--balance", action="store_true",
                    help="with --scan, --detections or --channels: remove the receiver's DC offset and I/Q imbalance, estimated from the "
                         "capture, first (an uncalibrated zero-IF receiver lists every strong emitter's mirror image as an emitter)")
    ap.add_argument("--imbalance", action="store_true",
                    help="with --scan and no capture file: the synthetic band as a receiver 1 dB / 5 degrees out of balance delivers it")
    ap.add_argument("--stream", type=int, default=0, metavar="CHUNK_PAIRS",
                    help="with --detections --floor cfar: read the capture this many pairs at a time and print every box when it has closed "
                         "(VTCNN2.detect_stream: the same boxes, for a recording that does not fit on the device, or a receiver)")
    ap.add_argument("--max-rows", type=int, default=4096,
                    help="with --stream: spectrogram rows after which a box that is still open is cut (an emitter that never pauses)")
    a = ap.parse_args()
    if a.stream:
        if a.stream < 0 or not a.detections or a.floor != "cfar":
            ap.error("--stream CHUNK_PAIRS goes with --detections --floor cfar: only the local floor can be computed a chunk at a time "
                     "(the 'flat' and 'per-bin' floors are quantiles over the whole capture)")
        if a.balance:
            ap.error("--stream cannot take --balance: the coefficients would be estimated from the whole capture")
        if a.hop != 128:
            ap.error("--stream needs --hop 128, as --batched does")
        if a.format == "cf32" and a.full_scale is None:
            ap.error("--stream with --format cf32 needs --full-scale: a gain measured per chunk would change from chunk to chunk")
    if a.detections and a.stream:
        if a.capture:
            chunks = file_chunks(a.capture, a.format, a.stream, a.full_scale)
        else:
            iq, a.format = load(a, synthetic_hopper)
            chunks = (iq[at:at + 2 * a.stream] for at in range(0, iq.size // 2 * 2, 2 * a.stream))
        if a.weights is None:
            model = VTCNN2.synthetic("deployed3")
        else:
            model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
        stream_detections(model, chunks, a.format, nfft=a.nfft, threshold_db=a.threshold, rate=a.rate if a.rate != 1.0 else None, level=a.level,
                          squelch=a.squelch, refine=a.refine, cfar=None if a.cfar is None else tuple(float(v) for v in a.cfar.split(",")),
                          max_rows=a.max_rows)
        return
    if a.detections:
        iq, a.format = load(a, synthetic_hopper)
        if a.weights is None:
            model = VTCNN2.synthetic("deployed3")
        else:
            model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
        detections(model, iq, a.format, nfft=a.nfft, threshold_db=a.threshold, rate=a.rate if a.rate != 1.0 else None, hop=a.hop, level=a.level,
                   squelch=a.squelch, batched=a.batched, refine=a.refine, balance=a.balance, floor=a.floor,
                   cfar=None if a.cfar is None else tuple(float(v) for v in a.cfar.split(",")))
        return
    if a.channels:
        iq, a.format = load(a, lambda fmt: synthetic_raster(fmt, a.channels))
        if a.weights is None:
            model = VTCNN2.synthetic("deployed3")
        else:
            model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
        channels(model, iq, a.format, a.channels, rate=a.rate if a.rate != 1.0 else None, hop=a.hop, level=a.level, squelch=a.squelch,
                 balance=a.balance)
        return
    if a.scan:
        iq, a.format = load(a, lambda fmt: synthetic_band(fmt, bursty=a.bursts, emitters=IMBALANCED_EMITTERS, imbalance=IMBALANCE) if a.imbalance
                            else synthetic_band(fmt, bursty=a.bursts))
        if a.weights is None:
            model = VTCNN2.synthetic("deployed3")
        else:
            model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
        scan(model, iq, a.format, nfft=a.nfft, threshold_db=a.threshold, rate=a.rate if a.rate != 1.0 else None, hop=a.hop, level=a.level,
             squelch=a.squelch, refine=a.refine, bursts=a.bursts, hold=a.hold, balance=a.balance)
        return
    if a.symbol_rate is not None:
        from modulationdetectioncnn_amd import frontend
        a.interpolate, a.decimate, sps = frontend.resample_ratio(a.rate, a.symbol_rate)
        print(f"{a.rate:g} S/s at {a.symbol_rate:g} sym/s is {a.rate / a.symbol_rate:g} samples per symbol: "
              f"resampling by {a.interpolate}/{a.decimate} gives {sps:g}")
    iq, a.format = load(a, synthetic_capture)
    if a.weights is None:
        model = VTCNN2.synthetic("deployed3")
    else:
        model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
    probs, labels, dbfs = classify(model, iq, a.format, hop=a.hop, level=a.level, squelch=a.squelch, shift=a.shift_hz / a.rate, decimate=a.decimate,
                                   interpolate=a.interpolate)
    print(f"{labels.size} windows, {int((labels < 0).sum())} below {a.squelch} dBFS")
    for k in np.unique(labels):
        sel = labels == k
        print(f"  label {int(k):2d}: {int(sel.sum()):6d} windows, power {dbfs[sel].min():7.1f} .. {dbfs[sel].max():6.1f} dBFS")


if __name__ == "__main__":
    main()
