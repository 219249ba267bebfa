"""GPU: the host-pointer calls against copy-pool stragglers (option debug.copy_stall_ms).

A fill of a pinned piece by the copy pool (csrc/context.hip: CopyPool::run with a token) is a set of idempotent
block copies: once nothing is left to draw, the caller copies the blocks a descheduled worker still holds and
returns without waiting for it, and that worker writes the same day bytes into the piece later.  Nothing may write
into the piece before such a straggler is done: not the next fill, not a plain memcpy, not the D2H of results that
come down through the same pieces (bpmf_mf_run's CC matrix, staged_download's beams).  On an idle box a worker
finishes within microseconds and no straggler outlives a fill.  Option debug.copy_stall_ms = k makes one on every
fill: the worker that draws block 0 sleeps k ms before its copy.

Every case makes its call with the option on and compares it bit for bit with the oracle and with the same call
without the stall (under mf.split16 with the unstalled call only); bpmf_host_call_stats must have counted a
straggler, i.e. the hook really fired (a page-locked day fills no piece: none there).  Sizes: a fill reaches the pool only from 4 MB (rows x piece), hence days
of 8 channels x 1.6 M samples; every batch of CC output spans at least two pinned pieces (mf.host_piece_kb = 8 MB),
so whichever piece holds a straggler gets a D2H.  Every stalled call starts from released pinned pieces, so their
size follows that call alone.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STALL_MS = 200
PIECE_KB = 8 << 10          # mf.host_piece_kb: the CC matrix comes down in pieces of 8 MB


def _assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want                               # (a NaN of the poisoned output counts as a difference)
    if bad.any():
        first = np.argwhere(bad)[0].tolist()
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ, the first at {first} "
                    f"({got[tuple(first)]!r} instead of {want[tuple(first)]!r})")


def _stalled(hip_opts, call, stragglers=True):
    """call() under option debug.copy_stall_ms, from released pinned pieces; skips in a process whose copy pool
    has no worker (no fill can leave a straggler there)."""
    from seismic_bpmf_amd import _lib
    _lib.release_device_memory()
    hip_opts("debug.copy_stall_ms", STALL_MS)
    try:
        out = call()
        st = _lib.host_call_stats()
    finally:
        hip_opts.reset("debug.copy_stall_ms")
    if st["fill_threads"] <= 1:
        pytest.skip("the copy pool of this process has no worker thread (one usable CPU): no fill leaves a straggler")
    if stragglers:
        assert st["stragglers"] >= 1, f"no straggler was left, the hook did not fire: {st}"
    else:
        assert st["stragglers"] == 0, st
    return out


@pytest.fixture(scope="module")
def day(oracle_lib):
    rng = np.random.default_rng(6060)
    T, S, C, L, N = 8, 4, 2, 64, 1_600_000
    tp = rng.standard_normal((T, S, C, L)).astype(np.float32)
    mv = rng.integers(-50, 2500, (T, S, C)).astype(np.int32)
    w = (0.25 + rng.random((T, S, C))).astype(np.float32)      # every channel weighted: equal shares per device
    d = rng.standard_normal((S, C, N)).astype(np.float32)
    return {"tp": tp, "mv": mv, "w": w, "d": d, "want": oracle_lib.matched_filter(tp, mv, w, d, 1)}


def _mf(tp, mv, w, d, network_sum=True, device=0):
    from seismic_bpmf_amd import matched_filter
    return matched_filter(tp, mv, w, d, 1, arch="gpu", device=device, network_sum=network_sum, check_zeros=False)


@pytest.mark.parametrize("piece_lags", [None, 0], ids=["streamed", "one_upload"])
@pytest.mark.parametrize("network_sum", [True, False])
def test_mf_cc_survives_a_straggler_of_the_days_last_fill(oracle_lib, hip_opts, day, network_sum, piece_lags):
    """bpmf_mf_run: the CC matrix comes down through the pieces the day went up through; a straggler of the day's
    last fills must be done before the first D2H lands there."""
    T = 4 if network_sum else 2
    tp, mv, w, d = day["tp"][:T], day["mv"][:T], day["w"][:T], day["d"]
    want = day["want"][:T] if network_sum else oracle_lib.matched_filter(tp, mv, w, d, 1, network_sum=False)
    row_kb = want[0].nbytes // 1024 + 1
    hip_opts("mf.host_piece_kb", PIECE_KB)
    hip_opts("mf.host_batch_kb", (2 if network_sum else 1) * row_kb)     # two batches of 12.8 / 51 MB of output
    if piece_lags is not None:
        hip_opts("mf.host_piece_lags", piece_lags)
    calm = _mf(tp, mv, w, d, network_sum)
    _assert_same(calm, want, "without a straggler")
    got = _stalled(hip_opts, lambda: _mf(tp, mv, w, d, network_sum))
    _assert_same(got, want, f"with a {STALL_MS} ms straggler")
    _assert_same(got, calm, "stalled against calm")


def test_mf_split16_survives_a_straggler(hip_opts, day):
    """mf.split16 = 2 (one upload of the day: no streamed pieces under it): the stalled call equals the unstalled."""
    tp, mv, w, d = day["tp"][:4], day["mv"][:4], day["w"][:4], day["d"]
    hip_opts("mf.split16", 2)
    hip_opts("mf.host_piece_kb", PIECE_KB)
    hip_opts("mf.host_batch_kb", 2 * (day["want"][0].nbytes // 1024 + 1))
    calm = _mf(tp, mv, w, d)
    got = _stalled(hip_opts, lambda: _mf(tp, mv, w, d))
    _assert_same(got, calm, "mf.split16, stalled against calm")


@pytest.mark.parametrize("fail_peer_copy", [0, 1], ids=["peer_fanout", "host_uploads"])
@pytest.mark.parametrize("k", [2, 4])
def test_mf_multi_survives_a_straggler(hip_opts, day, k, fail_peer_copy):
    """bpmf_mf_run_multi on k logical devices: the first device uploads the day and the others copy it device to
    device, or (debug.fail_peer_copy) every device uploads it through its own pieces.  The stats are the calling
    thread's, i.e. the first device's block."""
    tp, mv, w, d = day["tp"], day["mv"], day["w"], day["d"]
    hip_opts("debug.virtual_devices", k)
    hip_opts("mf.host_piece_kb", PIECE_KB)
    hip_opts("debug.fail_peer_copy", fail_peer_copy)
    devices = list(range(k))
    calm = _mf(tp, mv, w, d, device=devices)
    _assert_same(calm, day["want"], f"{k} devices without a straggler")
    got = _stalled(hip_opts, lambda: _mf(tp, mv, w, d, device=devices))
    _assert_same(got, day["want"], f"{k} devices with a {STALL_MS} ms straggler")
    _assert_same(got, calm, "stalled against calm")


@pytest.fixture(scope="module")
def features():
    rng = np.random.default_rng(6161)
    S, C, N, K = 8, 2, 600_000, 40
    f = np.abs(rng.standard_normal((S, C, N))).astype(np.float32)
    tau = rng.integers(0, 400, (K, S, 2)).astype(np.int32)
    wp = np.zeros((S, C, 2), np.float32)
    wp[:, 0, 0] = 1.0
    wp[:, 1, 1] = 1.0
    ws = (rng.random((K, S)) < 0.7).astype(np.float32)
    return f, tau, wp, ws


@pytest.mark.parametrize("devices", [1, 2])
@pytest.mark.parametrize("reduce", ["max", "none"])
@pytest.mark.parametrize("oob", ["strict", "flexible"])
def test_bp_survives_a_straggler(oracle_lib, hip_opts, features, oob, reduce, devices):
    """bpmf_bp_run / bpmf_bp_run_multi: the day of features goes up in pool fills and the beams come down through
    the same pieces (staged_download); with reduce="none" they span several pieces."""
    from seismic_bpmf_amd import beamform
    f, tau, wp, ws = features
    if devices > 1:
        hip_opts("debug.virtual_devices", devices)
    ids = list(range(devices))
    want = oracle_lib.beamform(f, tau, wp, ws, oob, reduce)
    want = (want,) if reduce == "none" else want

    def call():
        got = beamform(f, tau, wp, ws, device="gpu", reduce=reduce, out_of_bounds=oob, device_id=ids)
        return (got,) if reduce == "none" else got

    for g, w_ in zip(call(), want):
        _assert_same(g, w_, "without a straggler")
    for g, w_ in zip(_stalled(hip_opts, call), want):
        _assert_same(g, w_, f"with a {STALL_MS} ms straggler")


def test_a_page_locked_day_fills_no_piece(oracle_lib, hip_opts, day):
    """A day that is already page-locked (a torch pinned tensor seen through NumPy) goes to the device where it lies:
    no fill of a pinned piece, so no straggler even with the option on, and the same CC sums."""
    import torch
    tp, mv, w = day["tp"][:4], day["mv"][:4], day["w"][:4]
    d_pin = torch.empty(day["d"].shape, dtype=torch.float32).pin_memory()
    d_pin.copy_(torch.from_numpy(day["d"]))
    hip_opts("mf.host_piece_kb", PIECE_KB)
    hip_opts("mf.host_batch_kb", 2 * (day["want"][0].nbytes // 1024 + 1))
    got = _stalled(hip_opts, lambda: _mf(tp, mv, w, d_pin.numpy()), stragglers=False)
    _assert_same(got, day["want"][:4], "page-locked day")
