"""The window classifier behind VTCNN2.predict_iq_u8 / predict_iq on the MI355X, in the cells of (format x scaling x input x kind of
net) that no other test reaches: "ci8" with normalize="rms" on a deployed net and on cnn.py's net, and "cu8" on cnn.py's net in
chunks (tests/test_iq_norm_gpu.py, test_iq_formats_gpu.py, test_eval_ops_gpu.py and test_deployed_gpu.py hold the others; "ci8" with
normalize="rms" meets only the trained VT-CNN2 there).  The shape is the smallest at which the shared chunk loop can go wrong: 5
windows at hop 128 and 48 with batch_size=2 -- three chunks, a ragged last one, non-zero offsets into the samples, the
probabilities, the labels and the statistics of either record width --, a squelch that closes two of the five windows, and
return_power=True.  Everything the kernels compute is an identity between two runs of the same kernels and is held exactly; the one
float64 logarithm that torch takes on the device for "cu8" is held to its rounding (the last test says how)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulationdetectioncnn_amd import VTCNN2, frontend                                  # noqa: E402

WINDOWS, CHUNK = 5, 2
CELLS = [("ci8", "deployed3"), ("ci8", "cnnpy"), ("cu8", "cnnpy")]
HOPS = [128, 48]
DTYPE = {"cu8": np.uint8, "ci8": np.int8}


@functools.lru_cache(maxsize=None)
def _net(name):
    return VTCNN2.synthetic(name)      # shared: the tests only forward


@functools.lru_cache(maxsize=None)
def _capture(fmt, hop):
    """(samples, statistics, dBFS, squelch): WINDOWS windows whose powers lie tens of dB apart around a small DC offset, what
    window_stats_iq(_u8) and window_power_dbfs say of them, and a squelch half way between the second and third weakest.  Computed
    once per (fmt, hop); nobody writes to it."""
    rng = np.random.default_rng(1000 + hop)
    pairs = hop * (WINDOWS - 1) + 128
    amp = np.repeat(rng.permutation([2.0, 9.0, 38.0, 5.5, 76.0]), -(-pairs // WINDOWS))[:pairs]
    v = np.rint(amp[:, None] * rng.standard_normal((pairs, 2)) / 3 + 3) + (127.5 if fmt == "cu8" else 0)
    iq = np.clip(v, 0 if fmt == "cu8" else -128, 255 if fmt == "cu8" else 127).astype(DTYPE[fmt]).reshape(-1)
    stats = frontend.window_stats_iq_u8(iq, hop=hop) if fmt == "cu8" else frontend.window_stats_iq(iq, fmt, hop=hop)
    dbfs = frontend.window_power_dbfs(stats, fmt)
    squelch = float(np.sort(dbfs)[1:3].mean())
    assert stats.shape == (WINDOWS,) and (dbfs < squelch).sum() == 2
    return iq, stats, dbfs, squelch


def _bytes(results):
    return [(r.cpu().numpy() if isinstance(r, torch.Tensor) else r).tobytes() for r in results]


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("fmt,net", CELLS)
def test_chunks_inputs_and_entries_agree_exactly(fmt, net, hop):
    """The chunked call is the call in one chunk (all three results, bit for bit), the numpy call is the device call (probabilities
    and labels: the dBFS vector is the next test's), predict_iq(..., "cu8") is predict_iq_u8, and the squelch closes the windows that the integer statistics say."""
    m = _net(net)
    iq, stats, dbfs, squelch = _capture(fmt, hop)
    dev = torch.from_numpy(iq).cuda()
    for kw in (dict(normalize="rms", squelch_dbfs=squelch, return_power=True), dict(normalize="rms", remove_dc=False), dict(scale=0.02 / 127.5)):
        whole = m.predict_iq(dev, fmt, hop=hop, **kw)
        assert whole[0].shape == (WINDOWS, m.topology.classes) and whole[1].shape == (WINDOWS,) and all(r.is_cuda for r in whole)
        chunked = m.predict_iq(dev, fmt, hop=hop, batch_size=CHUNK, **kw)
        assert len(chunked) == len(whole) and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(chunked, whole)), kw
        for bs in (0, CHUNK):
            host = m.predict_iq(iq, fmt, hop=hop, batch_size=bs, **kw)
            assert len(host) == len(whole) and all(isinstance(r, np.ndarray) for r in host)
            assert _bytes(host[:2]) == _bytes(whole[:2]), (kw, bs)
        if fmt == "cu8":
            for src in (dev, iq):
                for bs in (0, CHUNK):
                    old, new = m.predict_iq_u8(src, hop=hop, batch_size=bs, **kw), m.predict_iq(src, "cu8", hop=hop, batch_size=bs, **kw)
                    assert len(old) == len(new) and _bytes(old) == _bytes(new) and all(type(a) is type(b) for a, b in zip(old, new)), (kw, bs)
    # the squelch against the integer statistics; the probabilities and the open windows' labels are the unsquelched call's
    closed = stats["energy"] < frontend.squelch_energy_threshold(squelch, fmt)
    np.testing.assert_array_equal(closed, dbfs < squelch)
    free = m.predict_iq(dev, fmt, hop=hop, normalize="rms")
    for src in (dev, iq):
        for bs in (0, CHUNK):
            p, l, _ = m.predict_iq(src, fmt, hop=hop, batch_size=bs, normalize="rms", squelch_dbfs=squelch, return_power=True)
            assert _bytes([p]) == _bytes(free[:1])
            np.testing.assert_array_equal(np.asarray(l.cpu() if isinstance(l, torch.Tensor) else l), np.where(closed, -1, free[1].cpu().numpy()))


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("fmt,net", CELLS)
def test_power_is_window_power_dbfs_of_the_statistics(fmt, net, hop):
    """The dBFS vector of return_power=True against window_power_dbfs(window_stats_iq(_u8)) on the same windows, and the numpy call's
    against the device call's.  The numpy call's vector IS that function's: bit for bit, every cell.  The device call's is torch's
    float64 10 log10(E / full scale) on the GPU of the same integer energies.  In the "ci8" cells, the ones no other test reaches, it
    is held bit for bit as well: full scale is 2^28 there, the quotient is exact, and the two log10 agree on these windows.  For
    "cu8" (a cell tests/test_iq_norm_gpu.py holds already, to 1e-9 dB; it is here for the 16-byte record under the chunk loop) full
    scale is (128 * 255)^2 and the two chains round differently in the last place on some windows -- measured on the MI355X, with
    the window classifiers separate and merged alike: -17.15707545012062 on the device, -17.157075450120622 on the host.  The bar
    there comes from the arithmetic, not from that figure: each side is a division (0.5 ulp, worth less than 0.25 ulp of the result
    after the logarithm, whose value is beyond 1.1 in size), a log10 (at most 2 ulp in the device's library, less on the host) and
    a product (0.5 ulp): under 3 ulp a side, 6 ulp of the reference between the two."""
    m = _net(net)
    iq, stats, dbfs, squelch = _capture(fmt, hop)
    dev = torch.from_numpy(iq).cuda()
    for bs in (0, CHUNK):
        on_host = m.predict_iq(iq, fmt, hop=hop, batch_size=bs, normalize="rms", squelch_dbfs=squelch, return_power=True)[2]
        on_device = m.predict_iq(dev, fmt, hop=hop, batch_size=bs, normalize="rms", squelch_dbfs=squelch, return_power=True)[2]
        assert on_device.dtype == torch.float64 and on_host.dtype == np.float64
        got = on_device.cpu().numpy()
        print(f"{fmt} {net} hop {hop} batch_size {bs}: window_power_dbfs {dbfs.tolist()}, numpy call {on_host.tolist()}, "
              f"device call {got.tolist()}, device - reference in ulp {((got - dbfs) / np.spacing(np.abs(dbfs))).tolist()}")
        assert on_host.tobytes() == dbfs.tobytes()
        if fmt == "cu8":
            assert got.shape == dbfs.shape and (np.abs(got - dbfs) <= 6 * np.spacing(np.abs(dbfs))).all()
        else:
            assert got.tobytes() == dbfs.tobytes()
