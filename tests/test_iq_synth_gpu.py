"""mdc_iq_synth_frames on the MI355X against the numpy restatement (tests/iq_synth_ref.py), bit for bit: frames, labels, SNR
indices and the saturation count, at every shape where the kernel takes another path -- partial work-groups, a first frame
that is no multiple of anything, the high word of the frame index, the stride beyond the grid cap, the shortest and the longest
pulses, both sources, both modes, both rails of the clamp, absent outputs -- then a graph capture, and the frames on their way
through the normaliser into fit() and the per-SNR evaluation."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import iq_synth_ref as ref
from conftest import ROOT
from modulationdetectioncnn_amd import _cabi, frontend

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 2016
POISON = -21846          # 0xAAAA


@functools.lru_cache(maxsize=None)
def grid_recipe():
    """all eleven classes at the lowest and the highest SNR of the default grid"""
    return frontend.synth_recipe(snrs_db=(-20, 18))


def tables_of(r):
    return dict(classes=r.classes, points=r.points, taps=r.taps, gain_sig=r.gain_sig, gain_noise=r.gain_noise, max_step=r.max_step, q=r.q)


@functools.lru_cache(maxsize=None)
def grid_reference(first, n):
    return ref.synth(seed=SEED, first_frame=first, n=n, **tables_of(grid_recipe()))


def launch(blob, first, n, seed=SEED, want_labels=True, want_snr=True, want_sat=True, plan_dev=None, out=None):
    """one raw call; returns (iq (n + 1, 256) with a poisoned guard row, labels, snr_index, saturated tensor) -- absent ones None"""
    blob = np.ascontiguousarray(blob, np.uint8)
    plan_dev = torch.from_numpy(blob).cuda() if plan_dev is None else plan_dev
    iq, labels, snr, sat = out if out is not None else (
        torch.full((n + 1, 256), POISON, dtype=torch.int16, device="cuda"),
        torch.full((n + 1,), -7, dtype=torch.int32, device="cuda") if want_labels else None,
        torch.full((n + 1,), -7, dtype=torch.int32, device="cuda") if want_snr else None,
        torch.zeros((1,), dtype=torch.int64, device="cuda") if want_sat else None)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _cabi.check(_cabi.lib().mdc_iq_synth_frames(blob.ctypes.data, plan_dev.data_ptr(), blob.size, seed, first, n, ptr(iq), ptr(labels), ptr(snr), ptr(sat),
                                                torch.cuda.current_stream().cuda_stream))
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
    check_against(launch(grid_recipe().blob, first, n), grid_reference(first, n), n)


def test_a_call_equals_its_two_halves():
    blob = grid_recipe().blob
    whole, a, b = launch(blob, 0, 67), launch(blob, 0, 13), launch(blob, 13, 54)
    torch.cuda.synchronize()
    for t in range(3):
        assert torch.equal(whole[t][:67], torch.cat([a[t][:13], b[t][:54]]))
    assert int(whole[3]) == int(a[3]) + int(b[3])


def test_the_high_word_of_the_frame_index_enters_the_key():
    blob = grid_recipe().blob
    hi, lo = launch(blob, (1 << 32) + 3, 1), launch(blob, 3, 1)
    torch.cuda.synchronize()
    assert not torch.equal(hi[0][0], lo[0][0])
    assert not np.array_equal(grid_reference((1 << 32) + 3, 23)[0][0], ref.synth(seed=SEED, first_frame=3, n=1, **tables_of(grid_recipe()))[0][0])


def test_one_call_beyond_the_grid_cap():
    r = grid_recipe()
    n = _cabi.SYNTH_GRID_CAP * _cabi.SYNTH_GROUP_FRAMES + 7
    iq, labels, snr, _ = launch(r.blob, 5, n)
    torch.cuda.synchronize()
    w_lab, w_snr = ref.labels_of(5, n, len(r.mods), len(r.snrs_db))
    assert np.array_equal(labels[:n].cpu().numpy(), w_lab) and np.array_equal(snr[:n].cpu().numpy(), w_snr)
    assert (iq[n] == POISON).all() and int(labels[n]) == -7
    picks = sorted({0, n - 1, *np.random.default_rng(3).integers(0, n, 64).tolist()})
    got = iq[torch.tensor(picks, device="cuda")].cpu().numpy()
    for row, i in zip(got, picks):
        assert np.array_equal(row, ref.synth(seed=SEED, first_frame=5 + i, n=1, **tables_of(r))[0][0]), i


def test_two_runs_give_identical_bits():
    blob = grid_recipe().blob
    a, b = launch(blob, 7, 67), launch(blob, 7, 67)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_zero_frames_is_ok_without_a_launch():
    blob = np.ascontiguousarray(grid_recipe().blob)
    assert _cabi.lib().mdc_iq_synth_frames(blob.ctypes.data, None, blob.size, SEED, 0, 0, None, None, None, None, None) == 0


@pytest.mark.parametrize("absent", ["labels", "snr", "sat", "all"])
def test_absent_outputs(absent):
    got = launch(grid_recipe().blob, 0, 67, want_labels=absent not in ("labels", "all"), want_snr=absent not in ("snr", "all"),
                 want_sat=absent not in ("sat", "all"))
    assert sum(t is None for t in got) == (3 if absent == "all" else 1)
    check_against(got, grid_reference(0, 67), 67)


# ------------------------------------------------------------------------------------------------ 2. classes at their edges
def random_tables(seed, source, M, sps, span, mode, S=2, phase_factor=0, amplitude=0, add=(0, 0), gain_sig=None, gain_noise=None, max_step=1 << 26,
                  q=12):
    """one class with random complex taps and a random alphabet, scaled to the plan's branch bound; three copies of it as classes
    (so that the waves of a work-group differ in nothing but the frame), S SNR entries"""
    rng = np.random.default_rng(seed)
    C = 3
    cl = np.zeros(C, _cabi.IQ_SYNTH_CLASS)
    amax = ref.GAUSS_MAX if source == ref.GAUSS else 12000
    pts = rng.integers(-amax, amax + 1, (max(M, 1), 2)).astype(np.int16) if source == ref.ALPHABET else np.zeros((0, 2), np.int16)
    if source == ref.ALPHABET:
        pts[0] = (amax, -amax)
    limit = (32767 - max(abs(add[0]), abs(add[1])) - 1) * 32768 // amax            # a branch's sum of |re| + |im|
    raw = rng.standard_normal((sps * span, 2))
    taps = np.zeros((sps * span, 2), np.int16)
    for b in range(sps):
        br = raw[b::sps]
        taps[b::sps] = np.trunc(br * (limit / np.abs(br).sum())).astype(np.int16)
    for c in cl:
        c["source"], c["points"], c["sps"], c["span"], c["mode"] = source, M if source == ref.ALPHABET else 0, sps, span, mode
        c["phase_factor"], c["amplitude"], c["add_re"], c["add_im"] = phase_factor, amplitude, add[0], add[1]
    gs = np.full((C, S), 1 << q, np.int32) if gain_sig is None else np.asarray(gain_sig, np.int32).reshape(C, S)
    gn = np.full(S, 1 << (q - 6), np.int32) if gain_noise is None else np.asarray(gain_noise, np.int32)
    return dict(classes=cl, points=pts, taps=taps, gain_sig=gs, gain_noise=gn, max_step=max_step, q=q)


def run_tables(t, n=23, first=(1 << 40) + 1):
    want = ref.synth(seed=SEED, first_frame=first, n=n, **t)
    check_against(launch(frontend.synth_plan(**t), first, n), want, n)
    return want


@pytest.mark.parametrize("sps,span", [(4, 16), (16, 8), (1, 16), (3, 5), (16, 1)])
def test_shortest_and_longest_pulses(sps, span):
    run_tables(random_tables(1, ref.ALPHABET, 4, sps, span, ref.LINEAR))
    run_tables(random_tables(2, ref.GAUSS, 0, sps, span, ref.LINEAR, add=(900, -700)))


@pytest.mark.parametrize("M", [1, 2, 64])
def test_alphabet_sizes(M):
    run_tables(random_tables(3, ref.ALPHABET, M, 8, 8, ref.LINEAR))


def test_phase_class_that_wraps_the_phase_many_times_per_frame():
    t = random_tables(4, ref.ALPHABET, 2, 8, 4, ref.PHASE, phase_factor=-(1 << 21) - 12345, amplitude=-30000, add=(1500, -2000))
    z = ref.synth(seed=SEED, first_frame=0, n=4, stage="z", **t)[0]
    assert np.abs(z).max() > 25000                        # a carrier, and large increments: |y| is in the thousands, x 2^21 > 2^32
    run_tables(t)
    run_tables(random_tables(5, ref.GAUSS, 0, 8, 8, ref.PHASE, phase_factor=77777, amplitude=32767))


def test_both_rails_saturate_and_are_counted():
    t = random_tables(6, ref.ALPHABET, 4, 8, 8, ref.LINEAR, gain_sig=np.full((3, 2), 40 << 12, np.int32), gain_noise=[1 << 10, 1 << 12])
    iq, _, _, sat = run_tables(t, n=67)
    assert iq.min() == -32768 and iq.max() == 32767 and sat > 100


def test_noise_alone_and_signal_alone():
    t = random_tables(7, ref.ALPHABET, 8, 8, 8, ref.LINEAR, gain_sig=np.zeros((3, 2), np.int32))
    assert np.abs(run_tables(t)[0]).max() > 1000
    t = random_tables(7, ref.ALPHABET, 8, 8, 8, ref.LINEAR, gain_noise=[0, 0])
    assert np.abs(run_tables(t)[0]).max() > 1000


# ------------------------------------------------------------------------------------------------ 3. capture, and downstream
def test_capturable_and_the_replay_gives_the_same_bits():
    blob = np.ascontiguousarray(grid_recipe().blob)
    plan_dev = torch.from_numpy(blob).cuda()
    n = 67
    eager = launch(blob, 13, n, plan_dev=plan_dev)
    torch.cuda.synchronize()
    out = tuple(torch.zeros_like(t) for t in eager)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(blob, 13, n, plan_dev=plan_dev, out=out)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager[:3], out[:3]):
        assert torch.equal(a[:n], b[:n])
    assert int(out[3]) == int(eager[3])


def test_frontend_returns_the_same_frames_and_snr_values():
    r = grid_recipe()
    iq, labels, snr_db, sat = frontend.synth_frames(67, r, seed=SEED, return_saturated=True)
    w_iq, w_lab, w_snr, w_sat = grid_reference(0, 67)
    assert iq.dtype == torch.int16 and tuple(iq.shape) == (67, 256) and labels.dtype == torch.int32
    assert np.array_equal(iq.cpu().numpy(), w_iq) and np.array_equal(labels.cpu().numpy(), w_lab) and sat == w_sat
    assert np.array_equal(snr_db.cpu().numpy(), np.array(r.snrs_db)[w_snr])
    assert frontend.synth_frames(0, r)[0].shape == (0, 256)


def test_dataset_feeds_fit_and_the_per_snr_evaluation():
    from modulationdetectioncnn_amd import VTCNN2, Topology
    r = frontend.synth_recipe(mods=("BPSK", "WBFM", "QAM16"), snrs_db=range(-4, 20, 4))
    S = len(r.snrs_db)
    n = 3 * S * 64
    X, labels, snr_db = frontend.synth_dataset(n, r, seed=11)
    assert X.dtype == torch.float32 and tuple(X.shape) == (n, 2, 128) and bool(torch.isfinite(X).all())
    iq = frontend.synth_frames(n, r, seed=11)[0]
    assert torch.equal(X, frontend.normalized_frames_from_iq(iq.reshape(-1), "ci16", level=frontend.DEFAULT_LEVEL))      # the one normaliser
    model = VTCNN2.synthetic(Topology.deployed(3, 3), seed=1)
    model.compile(loss="categorical_crossentropy", optimizer="adam")
    hist = model.fit(X, labels.long(), batch_size=256, epochs=1, seed=1)
    assert len(hist.history["loss"]) == 1 and np.isfinite(hist.history["loss"][0])
    assert np.isfinite(model.evaluate(X, labels.long()))
    assert model.confusion(X, labels, normalize=False).sum() == n
    acc, conf = model.accuracy_by_snr(X, labels, snr_db)
    assert sorted(acc) == sorted(r.snrs_db)
    assert all(int(conf[s].sum()) == n // S for s in r.snrs_db)                  # an exactly balanced grid
    assert all((conf[s].sum(axis=1) == n // S // 3).all() for s in r.snrs_db)     # ... in both directions


def test_training_example_runs_on_synthesised_frames(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("train_like_cnn_py", os.path.join(ROOT, "examples", "train_like_cnn_py.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    model, history, score, (x_test, idx_test) = example.main([str(tmp_path / "w.h5"), "--synth", "BPSK,GFSK,QAM64", "--frames", "5400", "--epochs", "2"])
    assert np.isfinite(score) and len(x_test) == len(idx_test) == 5400 - int(5400 * 0.7)
    assert capsys.readouterr().out.rstrip().endswith(repr(score))
