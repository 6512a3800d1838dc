"""The exact-integer fixtures (tests/exact_fixtures.py) at the smallest batch that reaches each launch form, each round of a
persistent kernel's walk and each raw-byte entry -- every frame against the f64 oracle BIT FOR BIT.

tests/test_exact_fixtures_gpu.py stops at 2,304 frames (VT-CNN2) and 1,000 (deployed nets), where every persistent work-group
still owns one group.  The sizes below are thresholds read from the launch code (paths below modulationdetectioncnn_amd/csrc/):
  VT-CNN2   1,025                 bf16 / fp8 conv: batch form, one past the range form (vtcnn2_sched_common.h:21,
                                  vtcnn2_bf16_sched.hip:474, vtcnn2_fp8_conv.hip:576); 65 groups, the last holds one frame
            4,117 = 4,096+16+5    min(ngroups, 256) work-groups (vtcnn2_bf16_sched.hip:466-467, vtcnn2_fp8_conv.hip:566-567):
                                  work-groups 0 and 1 take a second group from the other image buffer (staged in iterations
                                  5..9, :346-348 / :357-358), work-group 1's is ragged, 2..255 have none
            8,213 = 8,192+16+5    a third group, staged into image buffer 0 again; f32: the conv's loop form (vtcnn2.hip:598-613)
            16,517 = 16,384+128+5 f32 dense1 on 128-row tiles, head fused and unfused, ragged last tile (vtcnn2.hip:644-649)
            32,821                the head dense_chain<1,1>: 512 work-groups x 4 waves x 16 rows, then a second tile
                                  (dense_chain.hip:224-226); with a dense tap the TAPS instantiation, with a hidden tap the other
  deployed  32,789 = 32,768+16+5  bf16 / f16 / fp8: 256 work-groups x 8 waves x 16 frames (deployed_bf16.hip:161-192, :573-574),
                                  then a wave's second group (ragged for wave 1): row buffer 0 refilled under row 1
            131,093               raw bytes: round 4, the four-slot ring read after its first refill (:186, :197-202)
            524,392 = 524,288+64+40   f32: 2,048 work-groups x 4 waves x 64 frames (deployed.hip:598-599), then a wave's second
                                  block (has_next, :325) and the tail kernel (:649-666)
Every batch is a seeded arrangement of the fixture's 64 frames (raw bytes: of 64 raw frames, or a periodic stream with 128
distinct windows), gathered on the device; so is the expectation, from the oracle's 64 (128) rows.  Every call is ONE launch
of n frames (batch_size=n).  Taps and labels are compared with ==; the only numeric bar is the project's f32 softmax bar, 2e-6,
against the oracle's probabilities."""
import numpy as np
import pytest
import torch

import exact_fixtures as X
from modulationdetectioncnn_amd import VTCNN2, Topology, frames_from_iq_u8

pytestmark = pytest.mark.gpu

SOFTMAX_BAR = 2e-6
RAW_SEED = 0                     # tests/test_exact_fixtures.py proves the preconditions on this seed's raw frames (and they are re-checked here)
VT_IDS = ["f32", "bf16", "fp8", "fp8-bf16feat"]
# (frames per unit of work, units per round of the walk): where a differing frame sits in its kernel's walk
CONV16 = (16, 256)               # bf16 / fp8 conv: 16-frame groups, 256 work-groups (the f32 conv: 64-frame groups, no walk below 8,192)
DEP16 = (16, 256 * 8)            # deployed bf16 / f16 / fp8: one 16-frame group per wave, 8 waves, 256 work-groups
DEP32 = (64, 2048 * 4)           # deployed f32: one 64-frame block per wave, 4 waves, 2,048 work-groups
CHAIN = (16, 512 * 4)            # dense_chain: one 16-row tile per wave, 4 waves, 512 work-groups

_fixtures = {}
_models = {}
_wants = {}


def _fixture(kind, shape, flavour):
    key = (kind, shape, flavour)
    if key not in _fixtures:
        _fixtures[key] = X.vtcnn2_fixture(shape, flavour) if kind == "vtcnn2" else X.deployed_fixture(shape, flavour)
    return _fixtures[key]


def _model(fx, mode, bf16feat=False):
    """One engine per (fixture, mode) for the whole file: the walks reuse its workspace, largest batch last or not."""
    key = (fx.kind, fx.shape, fx.flavour, mode, bf16feat)
    if key not in _models:
        kw = {}
        if mode == "fp8":
            kw["fp8_input_absmax"] = fx.fp8_input_absmax
            if fx.kind == "vtcnn2":
                kw["fp8_bf16_features"] = bf16feat
                if not bf16feat:
                    kw["fp8_feature_absmax"] = fx.fp8_feature_absmax
        topo = Topology.vtcnn2(fx.shape[0]) if fx.kind == "vtcnn2" else Topology.deployed(fx.shape[0])
        m = VTCNN2(topo, dtype=mode, **kw)
        m.set_weights(fx.weights)
        _models[key] = m
    return _models[key]


def _want(fx, mode, bf16feat=False, hop=None):
    """The oracle's rows on the device, computed once per (fixture, mode, frames): hop None = the fixture's own 64 frames,
    128 / 64 / 3 = the distinct windows of that raw-byte layout.  Preconditions first: an AssertionError here is a broken
    fixture, a test error, never a skip.  Taps as f32 (they are f32 numbers: precondition 3), probabilities as f64."""
    key = (fx.kind, fx.shape, fx.flavour, mode, bf16feat, hop)
    if key not in _wants:
        frames = None if hop is None else X.raw_oracle_frames(fx.kind, hop, RAW_SEED)
        out = X.checked_expected(fx, mode, bf16feat, frames=frames)
        w = {k: torch.from_numpy(np.ascontiguousarray(out[k], np.float32)).cuda() for k in ("conv", "flat", "hidden", "dense") if k in out}
        w["probs"] = torch.from_numpy(np.ascontiguousarray(out["probs"], np.float64)).cuda()
        w["labels"] = torch.from_numpy(np.ascontiguousarray(out["labels"], np.int64)).cuda()
        w["frames"] = torch.from_numpy(np.ascontiguousarray(fx.frames if frames is None else frames, np.float32)).cuda()
        _wants[key] = w
    return _wants[key]


def _where(i, walk):
    per, units = walk
    return f"frame {i}: round {i // (per * units)} of the walk, unit {(i // per) % units}, slot {i % per} of its {per}"


def _equal(got, want_rows, idx, what, walk):
    """got == want_rows[idx], every element (gathered and compared on the device); the first differing frame with its place."""
    want = want_rows[idx].reshape(got.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(got.shape[0], -1)
    rows = torch.nonzero(bad.any(dim=1)).flatten()
    i = int(rows[0])
    j = int(torch.nonzero(bad[i]).flatten()[0])
    raise AssertionError(f"{what}: {len(rows)} of {got.shape[0]} frames differ ({int(bad.sum())} elements); first at {_where(i, walk)}, "
                         f"fixture row {int(idx[i])}, element {j}: got {got.reshape(got.shape[0], -1)[i, j].item()!r}, "
                         f"oracle {want.reshape(got.shape[0], -1)[i, j].item()!r}")


def _probs_labels(probs, labels, w, idx, what, walk):
    err = (probs.double() - w["probs"][idx]).abs().amax(dim=1)
    worst = float(err.max())
    if not worst <= SOFTMAX_BAR:                       # (a NaN fails too)
        i = int(torch.nonzero(~(err <= SOFTMAX_BAR)).flatten()[0])
        raise AssertionError(f"{what} probs: max |p - oracle| = {worst:.3g} > {SOFTMAX_BAR}; first at {_where(i, walk)}, fixture row {int(idx[i])}")
    _equal(labels.long(), w["labels"], idx, what + " labels", walk)


def _indices(n, seed_extra=0):
    return torch.from_numpy(X.batch_indices(n, 64, seed=n + seed_extra)).cuda()


def _forward(m, x, n, tap=None):
    assert x.shape[0] == n
    return m.forward_device(x, tap=tap, batch_size=n)      # batch_size=n: one launch of n frames, whatever the default chunk


# ---------------------------------------------------------------------------------------------------------------
# VT-CNN2: the conv walks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode,bf16feat", X.VT_MODES, ids=VT_IDS)
def test_vtcnn2_conv_walk_rounds_equal_the_oracle(mode, bf16feat, flavour):
    """1,025 / 4,117 / 8,213 frames: the batch form's first, second and third round (f32: three of its four conv forms and,
    above 2,048, dense1's 64-row tiles).  All four taps, probabilities, labels; the tapped and the untapped path agree."""
    fx = _fixture("vtcnn2", 11, flavour)
    w = _want(fx, mode, bf16feat)
    m = _model(fx, mode, bf16feat)
    for n in (1025, 4117, 8213):
        idx = _indices(n)
        x = w["frames"][idx].contiguous()
        tag = f"vtcnn2 C=11 {flavour} {mode}{'+bf16feat' if bf16feat else ''} n={n}"
        p0, l0, _ = _forward(m, x, n)                              # no tap: above 2,048 frames the head fused into dense1's epilogue
        for tap in ("flat", "conv", "hidden", "dense"):            # (layer by layer: a failure names the first layer that differs)
            p, l, t = _forward(m, x, n, tap)
            _equal(t, w[tap], idx, f"{tag} {tap}", CONV16)
            _probs_labels(p, l, w, idx, f"{tag} (tap={tap})", CONV16)
            assert torch.equal(p, p0) and torch.equal(l, l0), f"{tag}: tap={tap} and the untapped path disagree"
            del t
        _probs_labels(p0, l0, w, idx, tag, CONV16)


@pytest.mark.parametrize("flavour", ["dense", "sparse"])
def test_vtcnn2_f32_dense1_on_128_row_tiles_equals_the_oracle(flavour):
    """16,517 frames, f32: 130 tiles of 128 rows, the last with 5; head fused (no tap) and unfused (hidden / dense tap)."""
    fx = _fixture("vtcnn2", 11, flavour)
    w = _want(fx, "f32")
    m = _model(fx, "f32")
    n = 16384 + 128 + 5
    idx = _indices(n)
    x = w["frames"][idx].contiguous()
    tag = f"vtcnn2 C=11 {flavour} f32 n={n}"
    tiles = (128, 1 << 30)
    p0, l0, _ = _forward(m, x, n)
    _probs_labels(p0, l0, w, idx, tag + " fused head", tiles)
    for tap in ("hidden", "dense"):
        p, l, t = _forward(m, x, n, tap)
        _equal(t, w[tap], idx, f"{tag} {tap}", tiles)
        _probs_labels(p, l, w, idx, f"{tag} (tap={tap})", tiles)
        assert torch.equal(p, p0) and torch.equal(l, l0), f"{tag}: tap={tap} and the fused head disagree"


@pytest.mark.parametrize("flavour", ["dense", "sparse"])
def test_vtcnn2_bf16_head_walks_to_a_second_tile(flavour):
    """32,821 frames, bf16: the head as its own launch, dense_chain<1,1>, walks on to a second tile -- the TAPS instantiation
    under a dense tap, the other one under a hidden tap (the product build reaches both; untapped, the head is fused)."""
    fx = _fixture("vtcnn2", 11, flavour)
    w = _want(fx, "bf16")
    m = _model(fx, "bf16")
    n = 32768 + 53
    idx = _indices(n)
    x = w["frames"][idx].contiguous()
    tag = f"vtcnn2 C=11 {flavour} bf16 n={n}"
    p0, l0, _ = _forward(m, x, n)
    _probs_labels(p0, l0, w, idx, tag + " fused head", CHAIN)
    for tap in ("dense", "hidden"):
        p, l, t = _forward(m, x, n, tap)
        _equal(t, w[tap], idx, f"{tag} {tap}", CHAIN)
        _probs_labels(p, l, w, idx, f"{tag} (tap={tap})", CHAIN)
        assert torch.equal(p, p0) and torch.equal(l, l0), f"{tag}: tap={tap} and the fused head disagree"


# ---------------------------------------------------------------------------------------------------------------
# deployed nets: a wave's second group / block
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode", ["bf16", "f16", "fp8"])
def test_deployed_second_group_of_a_wave_equals_the_oracle(mode, flavour, filters):
    fx = _fixture("deployed", filters, flavour)
    w = _want(fx, mode)
    m = _model(fx, mode)
    n = 32768 + 16 + 5
    idx = _indices(n)
    p, l, _ = _forward(m, w["frames"][idx].contiguous(), n)
    _probs_labels(p, l, w, idx, f"deployed F={filters} {flavour} {mode} n={n}", DEP16)


@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
def test_deployed_f32_second_block_of_a_wave_equals_the_oracle(flavour, filters):
    """524,392 frames (537 MB, gathered on the device): has_next is taken, then the 40-frame tail kernel."""
    fx = _fixture("deployed", filters, flavour)
    w = _want(fx, "f32")
    m = _model(fx, "f32")
    n = 524288 + 64 + 40
    idx = _indices(n)
    x = w["frames"][idx].contiguous()
    tag = f"deployed F={filters} {flavour} f32 n={n}"
    p0, l0, _ = _forward(m, x, n)
    _probs_labels(p0, l0, w, idx, tag, DEP32)
    p, l, t = _forward(m, x, n, "dense")
    _equal(t, w["dense"], idx, tag + " dense", DEP32)
    _probs_labels(p, l, w, idx, tag + " (tap=dense)", DEP32)
    assert torch.equal(p, p0) and torch.equal(l, l0), tag


# ---------------------------------------------------------------------------------------------------------------
# raw bytes on the same walks
# ---------------------------------------------------------------------------------------------------------------
def _raw(m, w, stream, hop, n, idx, tag, walk):
    """predict_iq_u8 on the stream, one launch: against the exact oracle expectation, and bit for bit against
    convert-then-forward; the converted frames themselves are the oracle's, exactly."""
    p, l = m.predict_iq_u8(stream, scale=2 ** -6, batch_size=n, hop=hop)
    assert p.shape[0] == n, (tag, p.shape)
    _probs_labels(p, l, w, idx, tag, walk)
    x = frames_from_iq_u8(stream, 2 ** -6, hop=hop)
    _equal(x, w["frames"], idx, tag + " converted frames", walk)
    p2, l2, _ = m.forward_device(x, batch_size=n)
    assert torch.equal(p, p2), f"{tag}: raw bytes and convert-then-forward differ in {int((p != p2).any(dim=1).sum())} rows of probabilities"
    assert torch.equal(l, l2), f"{tag}: raw bytes and convert-then-forward differ in {int((l != l2).sum())} labels"


def _raw_frames_dev(kind):
    return torch.from_numpy(X.raw_fixture_frames(kind, RAW_SEED)).cuda()


@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode,bf16feat", X.VT_MODES, ids=VT_IDS)
def test_vtcnn2_raw_bytes_on_every_conv_form_equal_the_oracle(mode, bf16feat, flavour):
    """hop 128 at 17 / 257 / 1,025 / 4,117 / 8,213 windows: f32 crosses its four conv forms (<= 128, <= 2,048, <= 8,192, loop),
    bf16 / fp8 the range form and rounds 1-3 of the batch form (the fp8 batch kernel's U8 instantiations, both feature formats)."""
    fx = _fixture("vtcnn2", 11, flavour)
    w = _want(fx, mode, bf16feat, hop=128)
    m = _model(fx, mode, bf16feat)
    raw = _raw_frames_dev("vtcnn2")
    for n in (17, 257, 1025, 4117, 8213):
        idx = _indices(n, seed_extra=1)
        stream = raw[idx].reshape(-1)                              # window i = raw fixture frame idx[i] (X.raw_capture's hop-128 layout)
        _raw(m, w, stream, 128, n, idx, f"vtcnn2 raw hop=128 {flavour} {mode}{'+bf16feat' if bf16feat else ''} n={n}", CONV16)


@pytest.mark.parametrize("hop", [64, 3])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode,bf16feat", X.VT_MODES, ids=VT_IDS)
def test_vtcnn2_raw_bytes_overlapping_and_odd_hops_equal_the_oracle(mode, bf16feat, flavour, hop):
    """4,117 windows of a periodic stream: overlapping windows (hop 64) and windows that are only 2-byte aligned (hop 3)."""
    fx = _fixture("vtcnn2", 11, flavour)
    w = _want(fx, mode, bf16feat, hop=hop)
    m = _model(fx, mode, bf16feat)
    n = 4096 + 16 + 5
    stream = torch.from_numpy(X.raw_capture("vtcnn2", hop, RAW_SEED, windows=n)).cuda()
    idx = torch.arange(n, device="cuda") % X.raw_period_windows(hop)
    _raw(m, w, stream, hop, n, idx, f"vtcnn2 raw hop={hop} {flavour} {mode}{'+bf16feat' if bf16feat else ''} n={n}", CONV16)


@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode", ["bf16", "f16", "fp8"])
def test_deployed_raw_bytes_round_four_of_the_ring_equals_the_oracle(mode, flavour, filters):
    """hop 128 at 131,093 windows: every wave's fourth group re-reads ring slot 0 after its first refill, wave 1's is ragged."""
    fx = _fixture("deployed", filters, flavour)
    w = _want(fx, mode, hop=128)
    m = _model(fx, mode)
    n = 131072 + 16 + 5
    idx = _indices(n, seed_extra=1)
    stream = _raw_frames_dev("deployed")[idx].reshape(-1)
    _raw(m, w, stream, 128, n, idx, f"deployed raw hop=128 F={filters} {flavour} {mode} n={n}", DEP16)


@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode", ["bf16", "f16", "fp8"])
def test_deployed_raw_bytes_odd_hop_second_group_equals_the_oracle(mode, flavour, filters):
    """hop 3 at 32,789 windows: a wave's second group out of a stream whose windows are only 2-byte aligned."""
    fx = _fixture("deployed", filters, flavour)
    w = _want(fx, mode, hop=3)
    m = _model(fx, mode)
    n = 32768 + 16 + 5
    stream = torch.from_numpy(X.raw_capture("deployed", 3, RAW_SEED, windows=n)).cuda()
    idx = torch.arange(n, device="cuda") % X.raw_period_windows(3)
    _raw(m, w, stream, 3, n, idx, f"deployed raw hop=3 F={filters} {flavour} {mode} n={n}", DEP16)


@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
def test_deployed_f32_raw_bytes_second_block_equals_the_oracle(flavour, filters):
    """hop 128 at 524,392 windows: 134 MB of bytes, gathered on the device."""
    fx = _fixture("deployed", filters, flavour)
    w = _want(fx, "f32", hop=128)
    m = _model(fx, "f32")
    n = 524288 + 64 + 40
    idx = _indices(n, seed_extra=1)
    stream = _raw_frames_dev("deployed")[idx].reshape(-1)
    _raw(m, w, stream, 128, n, idx, f"deployed raw hop=128 F={filters} {flavour} f32 n={n}", DEP32)
