"""mdc_iq_synth_frames_faded on the MI355X against the numpy restatement (tests/iq_synth_fading_ref.py), bit for bit: frames,
labels, SNR indices and the saturation count, on the smallest shapes that take another path -- partial work-groups, a first
frame that is no multiple of anything, the high word of the frame index, the stride beyond the grid cap, one and four paths, one
and sixteen taps (no head, and a head that needs the third sample per lane), records at their preconditions' bounds, the longest
symbol head, the PHASE scan past the lane pairs, Doppler off and at its largest step, both rails of the clamp, absent outputs --
then a graph capture and the Python layer."""
import functools

import numpy as np
import pytest

import iq_synth_fading_ref as fref
import iq_synth_ref as ref
from modulationdetectioncnn_amd import _cabi, frontend

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 2016
POISON = -21846          # 0xAAAA


@functools.lru_cache(maxsize=None)
def grid_recipe():
    """all eleven classes at the lowest and the highest SNR of the default grid, through the default channel"""
    return frontend.synth_recipe(snrs_db=(-20, 18), fading=frontend.synth_fading())


def tables_of(r):
    return dict(classes=r.classes, points=r.points, taps=r.taps, gain_sig=r.gain_sig, gain_noise=r.gain_noise, max_step=r.max_step, q=r.q)


@functools.lru_cache(maxsize=None)
def grid_reference(first, n):
    r = grid_recipe()
    return fref.synth(seed=SEED, first_frame=first, n=n, fading=fref.record_of(r.fading.record), **tables_of(r))


def launch(blob, record, first, n, seed=SEED, want_labels=True, want_snr=True, want_sat=True, plan_dev=None, out=None):
    """one raw call; returns (iq (n + 1, 256) with a poisoned guard row, labels, snr_index, saturated tensor) -- absent ones None"""
    blob = np.ascontiguousarray(blob, np.uint8)
    record = np.ascontiguousarray(record, _cabi.IQ_SYNTH_FADING)
    plan_dev = torch.from_numpy(blob).cuda() if plan_dev is None else plan_dev
    iq, labels, snr, sat = out if out is not None else (
        torch.full((n + 1, 256), POISON, dtype=torch.int16, device="cuda"),
        torch.full((n + 1,), -7, dtype=torch.int32, device="cuda") if want_labels else None,
        torch.full((n + 1,), -7, dtype=torch.int32, device="cuda") if want_snr else None,
        torch.zeros((1,), dtype=torch.int64, device="cuda") if want_sat else None)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _cabi.check(_cabi.lib().mdc_iq_synth_frames_faded(blob.ctypes.data, plan_dev.data_ptr(), blob.size, seed, first, n, ptr(iq), ptr(labels), ptr(snr),
                                                      ptr(sat), record.ctypes.data, torch.cuda.current_stream().cuda_stream))
    return iq, labels, snr, sat


def check_against(got, want, n):
    iq, labels, snr, sat = got
    w_iq, w_lab, w_snr, w_sat = want
    torch.cuda.synchronize()
    assert np.array_equal(iq[:n].cpu().numpy(), w_iq)
    assert (iq[n] == POISON).all()                                        # nothing behind the last frame
    if labels is not None:
        assert np.array_equal(labels[:n].cpu().numpy(), w_lab) and int(labels[n]) == -7
    if snr is not None:
        assert np.array_equal(snr[:n].cpu().numpy(), w_snr) and int(snr[n]) == -7
    if sat is not None:
        assert int(sat.item()) == w_sat


# ------------------------------------------------------------------------------------------------ 1. the grid, call shapes
@pytest.mark.parametrize("first,n", [(0, 1), (0, 5), (0, 67), (13, 54), ((1 << 32) + 3, 23)])
def test_grid_frames_match_the_restatement(first, n):
    r = grid_recipe()
    check_against(launch(r.blob, r.fading.record, first, n), grid_reference(first, n), n)


def test_the_channel_changes_the_frames_and_nothing_else():
    r = grid_recipe()
    faded = launch(r.blob, r.fading.record, 13, 54)
    plain = ref.synth(seed=SEED, first_frame=13, n=54, **tables_of(r))
    torch.cuda.synchronize()
    assert np.array_equal(faded[1][:54].cpu().numpy(), plain[1]) and np.array_equal(faded[2][:54].cpu().numpy(), plain[2])
    assert (faded[0][:54].cpu().numpy() != plain[0]).mean() > 0.9


def test_one_call_beyond_the_grid_cap():
    r = grid_recipe()
    n = _cabi.SYNTH_GRID_CAP * _cabi.SYNTH_GROUP_FRAMES + 5
    check_against(launch(r.blob, r.fading.record, 5, n), grid_reference(5, n), n)


@pytest.mark.parametrize("absent", ["labels", "snr", "sat", "all"])
def test_absent_outputs(absent):
    r = grid_recipe()
    got = launch(r.blob, r.fading.record, 0, 67, want_labels=absent not in ("labels", "all"), want_snr=absent not in ("snr", "all"),
                 want_sat=absent not in ("sat", "all"))
    assert sum(t is None for t in got) == (3 if absent == "all" else 1)
    check_against(got, grid_reference(0, 67), 67)


# ------------------------------------------------------------------------------------------------ 2. records and classes at their edges
def random_record(seed, P, T, max_doppler_step):
    """P paths of T random taps that sum to exactly 32767 in absolute value, gains with max|los| + scatter = 32767 exactly"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(1, _cabi.IQ_SYNTH_FADING)
    rec["paths"], rec["taps"], rec["max_doppler_step"] = P, T, max_doppler_step
    for p in range(P):
        path = rec["path"][0][p]
        raw = rng.standard_normal(T)
        d = np.trunc(raw * (32767 / np.abs(raw).sum())).astype(np.int64)
        i = int(np.argmax(np.abs(d)))
        d[i] += (1 if d[i] >= 0 else -1) * (32767 - int(np.abs(d).sum()))
        assert int(np.abs(d).sum()) == 32767
        path["delay_taps"][:T] = d
        scatter = int(rng.integers(0, 20000))
        top = 32767 - scatter
        los = (top if rng.random() < 0.5 else -top, int(rng.integers(-top, top + 1)))
        path["los_re"], path["los_im"] = los if p % 2 == 0 else los[::-1]
        path["scatter"] = scatter
    return rec


@functools.lru_cache(maxsize=None)
def quiet_grid():
    """the grid's tables with the signal gains divided by 16: gains of up to four per path times tap sums of two stay off the rails"""
    t = tables_of(grid_recipe())
    t["gain_sig"] = t["gain_sig"] // 16
    return t, frontend.synth_plan(**t)


@pytest.mark.parametrize("P,T,step", [(1, 1, 0), (1, 16, 1 << 30), (4, 1, 1 << 30), (4, 16, 0), (4, 16, 1 << 30), (2, 2, 1), (3, 9, 1 << 20)])
def test_path_and_tap_extremes_with_doppler_off_and_at_its_largest(P, T, step):
    t, blob = quiet_grid()
    rec = random_record(100 * P + T, P, T, step)
    first, n = (1 << 40) + 1, 45                       # two full grids of 22 cells and one frame: every class at both SNRs, a partial group
    want = fref.synth(seed=SEED, first_frame=first, n=n, fading=fref.record_of(rec), **t)
    check_against(launch(blob, rec, first, n), want, n)
    assert np.abs(want[0]).max() > 1000 and want[3] < want[0].size // 100


def class_tables(seed, source, sps, span, mode, phase_factor=0, amplitude=0, add=(0, 0), gain=None, q=12):
    """three copies of one class with random complex taps scaled to the plan's branch bound (the waves of a work-group then differ
    in nothing but the frame), two SNR entries"""
    rng = np.random.default_rng(seed)
    cl = np.zeros(3, _cabi.IQ_SYNTH_CLASS)
    amax = ref.GAUSS_MAX if source == ref.GAUSS else 12000
    pts = np.zeros((0, 2), np.int16)
    if source == ref.ALPHABET:
        pts = rng.integers(-amax, amax + 1, (4, 2)).astype(np.int16)
        pts[0] = (amax, -amax)
    limit = (32767 - max(abs(add[0]), abs(add[1])) - 1) * 32768 // amax
    raw = rng.standard_normal((sps * span, 2))
    taps = np.zeros((sps * span, 2), np.int16)
    for b in range(sps):
        br = raw[b::sps]
        taps[b::sps] = np.trunc(br * (limit / np.abs(br).sum())).astype(np.int16)
    for c in cl:
        c["source"], c["points"], c["sps"], c["span"], c["mode"] = source, 4 if source == ref.ALPHABET else 0, sps, span, mode
        c["phase_factor"], c["amplitude"], c["add_re"], c["add_im"] = phase_factor, amplitude, add[0], add[1]
    gs = np.full((3, 2), (1 << q) // 16 if gain is None else gain, np.int32)
    return dict(classes=cl, points=pts, taps=taps, gain_sig=gs, gain_noise=np.full(2, 1 << (q - 6), np.int32), max_step=1 << 26, q=q)


def run_tables(t, rec, n=23, first=(1 << 40) + 1):
    want = fref.synth(seed=SEED, first_frame=first, n=n, fading=fref.record_of(rec), **t)
    check_against(launch(frontend.synth_plan(**t), rec, first, n), want, n)
    return want


def test_head_symbols_at_their_maximum():
    """sps = 1, span = 16 at T = 16: 158 symbols per frame, the last of them read by the head's last sample only"""
    rec = random_record(7, 2, 16, 0)
    run_tables(class_tables(1, ref.ALPHABET, 1, 16, ref.LINEAR), rec)
    run_tables(class_tables(2, ref.GAUSS, 1, 16, ref.LINEAR, add=(900, -700)), rec)
    run_tables(class_tables(3, ref.ALPHABET, 16, 1, ref.LINEAR), rec)


@pytest.mark.parametrize("T", [2, 15, 16])
def test_phase_class_whose_scan_runs_past_the_lane_pairs(T):
    """PHASE's running sum over 128 + H samples, with increments that wrap the phase many times per frame: a wrong total at the
    128th sample, or a wrong order among the H behind it, turns every later carrier sample"""
    rec = random_record(8 + T, 3, T, 1 << 22)
    t = class_tables(4, ref.ALPHABET, 8, 4, ref.PHASE, phase_factor=-(1 << 21) - 12345, amplitude=-30000, add=(1500, -2000))
    m = fref.synth(seed=SEED, first_frame=0, n=4, fading=fref.record_of(rec), stage="m", **t)[0]
    assert m.shape[1] == 128 + T - 1 and np.abs(m[:, 128:]).max() > 5000
    run_tables(t, rec)
    run_tables(class_tables(5, ref.GAUSS, 8, 8, ref.PHASE, phase_factor=77777, amplitude=32767), rec)


def test_both_rails_saturate_and_are_counted():
    rec = random_record(9, 4, 16, 1 << 30)
    iq, _, _, sat = run_tables(class_tables(6, ref.ALPHABET, 8, 8, ref.LINEAR, gain=40 << 12), rec, n=67)
    assert iq.min() == -32768 and iq.max() == 32767 and sat > 100


# ------------------------------------------------------------------------------------------------ 3. capture, and the Python layer
def test_capturable_and_the_replay_gives_the_same_bits():
    r = grid_recipe()
    blob = np.ascontiguousarray(r.blob)
    plan_dev = torch.from_numpy(blob).cuda()
    n = 67
    eager = launch(blob, r.fading.record, 13, n, plan_dev=plan_dev)
    torch.cuda.synchronize()
    out = tuple(torch.zeros_like(t) for t in eager)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(blob, r.fading.record, 13, n, plan_dev=plan_dev, out=out)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager[:3], out[:3]):
        assert torch.equal(a[:n], b[:n])
    assert int(out[3]) == int(eager[3])
    assert np.array_equal(out[0][:n].cpu().numpy(), fref.synth(seed=SEED, first_frame=13, n=n, fading=fref.record_of(r.fading.record), **tables_of(r))[0])


def test_frontend_takes_the_faded_entry_only_for_a_fading_recipe():
    r = grid_recipe()
    iq, labels, snr_db, sat = frontend.synth_frames(67, r, seed=SEED, return_saturated=True)
    w_iq, w_lab, w_snr, w_sat = grid_reference(0, 67)
    assert iq.dtype == torch.int16 and tuple(iq.shape) == (67, 256)
    assert np.array_equal(iq.cpu().numpy(), w_iq) and np.array_equal(labels.cpu().numpy(), w_lab) and sat == w_sat
    assert np.array_equal(snr_db.cpu().numpy(), np.array(r.snrs_db)[w_snr])
    assert frontend.synth_frames(0, r)[0].shape == (0, 256)
    # a recipe without fading: the bits of mdc_iq_synth_frames, as before
    plain = r._replace(fading=None)
    iq, labels, _ = frontend.synth_frames(67, plain, seed=SEED)
    blob = np.ascontiguousarray(plain.blob)
    plan_dev = torch.from_numpy(blob).cuda()
    raw = torch.empty((67, 256), dtype=torch.int16, device="cuda")
    _cabi.check(_cabi.lib().mdc_iq_synth_frames(blob.ctypes.data, plan_dev.data_ptr(), blob.size, SEED, 0, 67, raw.data_ptr(), None, None, None,
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(iq, raw) and np.array_equal(iq.cpu().numpy(), ref.synth(seed=SEED, first_frame=0, n=67, **tables_of(plain))[0])


def test_faded_dataset_feeds_the_per_snr_evaluation():
    from modulationdetectioncnn_amd import VTCNN2, Topology
    r = frontend.synth_recipe(mods=("BPSK", "WBFM", "QAM16"), snrs_db=range(-4, 20, 4), fading=frontend.synth_fading(max_doppler=0.001))
    S = len(r.snrs_db)
    n = 3 * S * 64
    X, labels, snr_db = frontend.synth_dataset(n, r, seed=11)
    assert X.dtype == torch.float32 and tuple(X.shape) == (n, 2, 128) and bool(torch.isfinite(X).all())
    iq = frontend.synth_frames(n, r, seed=11)[0]
    assert torch.equal(X, frontend.normalized_frames_from_iq(iq.reshape(-1), "ci16", level=frontend.DEFAULT_LEVEL))
    assert not torch.equal(iq, frontend.synth_frames(n, r._replace(fading=None), seed=11)[0])
    model = VTCNN2.synthetic(Topology.deployed(3, 3), seed=1)
    acc, conf = model.accuracy_by_snr(X, labels, snr_db)
    assert sorted(acc) == sorted(r.snrs_db)
    assert all(int(conf[s].sum()) == n // S for s in r.snrs_db)                  # exactly n / S frames per bin
    assert all((conf[s].sum(axis=1) == n // S // 3).all() for s in r.snrs_db)


def test_training_example_takes_fading(tmp_path, capsys):
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("train_like_cnn_py", os.path.join(ROOT, "examples", "train_like_cnn_py.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    _, _, score, (x_test, idx_test) = example.main([str(tmp_path / "w.h5"), "--synth", "BPSK,GFSK,QAM64", "--frames", "2700", "--epochs", "1", "--fading"])
    assert np.isfinite(score) and len(x_test) == len(idx_test) == 2700 - int(2700 * 0.7)
    assert capsys.readouterr().out.rstrip().endswith(repr(score))
    with pytest.raises(SystemExit):
        example.main([str(tmp_path / "w.h5"), "--fading", "2.5"])          # --fading belongs to --synth
