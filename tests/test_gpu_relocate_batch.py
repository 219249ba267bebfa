"""GPU: workflow.relocate_events -- a batch of events relocated in shared launches (csrc/bp_relocate.hip) --
against the CPU oracle's beam volumes and against the per-event path on the device.  Every comparison is
np.array_equal: both sides are the same float32 fmaf chains."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def small_setup(n_closest):
    from seismic_bpmf_amd import synthetic as syn
    geo = syn.make_bp_geometry((12, 12, 6), 9, 2, 50.0, n_closest=n_closest)
    return geo["moveouts"], geo["weights_sources"], syn.phase_weights(9, 3, 2)


def make_events(tau, n, seed, n_events=7):
    """(E, S, 3, n): two events of rounded features (many exact ties), an all-zero one, a planted arrival, and
    half-normal noise for the rest."""
    rng = np.random.default_rng(seed)
    S = tau.shape[1]
    f = np.abs(rng.standard_normal((n_events, S, 3, n))).astype(np.float32)
    f[0] = np.round(f[0])
    f[1] = np.round(2.0 * f[1])
    f[2] = 0.0
    src, t0 = tau.shape[0] // 3, n // 2
    f[3] *= 0.25
    for s in range(S):
        f[3, s, 0, min(n - 1, t0 + tau[src, s, 0])] += 6.0
        f[3, s, 1:, min(n - 1, t0 + tau[src, s, 1])] += 6.0
    return f


def check_against_oracle(oracle_lib, res, f, tau, wp, ws, oob, what):
    from seismic_bpmf_amd import postprocess as pp
    like = res["likelihood"].cpu().numpy()
    cols = res["columns"].cpu().numpy()
    for e in range(f.shape[0]):
        vol = oracle_lib.beamform(f[e], tau, wp, ws, oob, "none")
        k, t = np.unravel_index(vol.argmax(), vol.shape)
        assert (res["src_idx"][e], res["time_idx"][e]) == (k, t), (what, e)
        assert res["max_beam"][e] == vol.max(), (what, e)
        assert np.array_equal(cols[e], vol[:, t]), (what, e)
        with np.errstate(invalid="ignore"):
            want = pp.likelihood(vol[:, t])
        assert np.array_equal(like[e], want, equal_nan=True), (what, e)
        if not vol.any():
            assert np.isnan(like[e]).all(), (what, e)                 # 0 / 0 as NumPy gives it


@pytest.mark.parametrize("n_closest", [5, 9])
def test_relocate_events_equals_numpy_on_the_oracle_volumes(oracle_lib, n_closest):
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp = small_setup(n_closest)
    bf = BeamformerGPU(tau, ws)
    try:
        for n in (700, 1500, 3000):
            f = make_events(tau, n, seed=n + n_closest)
            assert not f[2].any() and np.array_equal(f[0], np.round(f[0])) and np.array_equal(f[1], np.round(f[1]))
            for oob in ("flexible", "strict"):
                res = relocate_events(bf, f, wp, "spatial", oob, columns=True)
                assert res["src_idx"].dtype == np.int64 and res["time_idx"].dtype == np.int64
                assert res["max_beam"].dtype == np.float32 and res["likelihood"].is_cuda
                check_against_oracle(oracle_lib, res, f, tau, wp, ws, oob, (n, oob))
                tmp = relocate_events(bf, f, wp, "temporal", oob)
                for e in range(f.shape[0]):
                    mb, ma = oracle_lib.beamform(f[e], tau, wp, ws, oob, "max")
                    assert np.array_equal(tmp["maxbeam"][e].cpu().numpy(), mb), (n, oob, e)
                    assert np.array_equal(tmp["maxbeam_sources"][e].cpu().numpy(), ma), (n, oob, e)
                    assert tmp["time_idx"][e] == mb.argmax() and tmp["src_idx"][e] == ma[mb.argmax()]
                    assert tmp["max_beam"][e] == mb.max()
    finally:
        bf.close()


@pytest.mark.parametrize("P,S,n_closest", [(1, 9, 5), (3, 20, 12), (6, 9, 5)])
def test_relocate_events_on_the_other_general_kernels(oracle_lib, P, S, n_closest):
    """Grids that are not two-phase run the per-term-table kernel (<= 32 terms per source) or the readlane kernel
    over the event dimension; more than four phases take the one-thread-per-phase prestack."""
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    from seismic_bpmf_amd.workflow import relocate_events
    geo = syn.make_bp_geometry((10, 10, 5), S, P, 50.0, n_closest=n_closest)
    tau, ws = geo["moveouts"], geo["weights_sources"]
    wp = np.random.default_rng(P).random((S, 3, P)).astype(np.float32)
    bf = BeamformerGPU(tau, ws)
    try:
        assert bf.plan_info()["stations_max"] == 0                      # not the packed two-phase kernel
        rng = np.random.default_rng(S)
        f = np.abs(rng.standard_normal((5, S, 3, 1300))).astype(np.float32)
        f[1] = np.round(f[1])
        f[2] = 0.0
        for oob in ("flexible", "strict"):
            res = relocate_events(bf, f, wp, "spatial", oob, columns=True)
            check_against_oracle(oracle_lib, res, f, tau, wp, ws, oob, (P, oob))
    finally:
        bf.close()


def test_group_range_split_of_a_batch_changes_nothing(hip_opts):
    """A small batch splits the plan's groups over several workgroups per tile and folds the partial rows per
    event; a batch that fills the chip does not (option bp.split forces either)."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp = small_setup(9)
    f = make_events(tau, 1500, seed=13)
    bf = BeamformerGPU(tau, ws)
    try:
        for method in ("spatial", "temporal"):
            auto = relocate_events(bf, f, wp, method)
            for split in (1, 3):
                hip_opts("bp.split", split)
                got = relocate_events(bf, f, wp, method)
                hip_opts.reset("bp.split")
                assert all(same_event(auto, e, got, e) for e in range(f.shape[0])), (method, split)
    finally:
        bf.close()


def test_relocate_events_on_a_plan_without_lds_windows(oracle_lib, hip_opts):
    """Plans that take the global-memory kernel of bp_direct.hip: the events' max-beams run one after the other
    inside the call, focus / column / likelihood stay batched."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    hip_opts("bp.direct", 1)
    tau, ws, wp = small_setup(5)
    bf = BeamformerGPU(tau, ws)
    try:
        assert bf.plan_info()["n_groups"] == 0                          # no LDS plan
        f = make_events(tau, 1500, seed=77)
        for oob in ("flexible", "strict"):
            res = relocate_events(bf, f, wp, "spatial", oob, columns=True)
            check_against_oracle(oracle_lib, res, f, tau, wp, ws, oob, ("direct", oob))
    finally:
        bf.close()


def same_event(a, i, b, j):
    ok = a["src_idx"][i] == b["src_idx"][j] and a["time_idx"][i] == b["time_idx"][j]
    ok = ok and a["max_beam"][i] == b["max_beam"][j]
    for key in ("likelihood", "columns", "maxbeam", "maxbeam_sources"):
        if key in a:
            ok = ok and np.array_equal(a[key][i].cpu().numpy(), b[key][j].cpu().numpy(), equal_nan=True)
    return bool(ok)


@pytest.mark.parametrize("method", ["spatial", "temporal"])
def test_an_event_never_reads_its_neighbours(method):
    """Flexible bounds skip what lies outside a window: a kernel that read across the event boundary instead
    would still return finite beams.  Reordering the batch, or replacing one event by huge values, must leave
    every other event's results as they were."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp = small_setup(5)
    bf = BeamformerGPU(tau, ws)
    try:
        f = make_events(tau, 1500, seed=5)
        E = f.shape[0]
        kw = dict(uncertainty_method=method, columns=True) if method == "spatial" else dict(uncertainty_method=method)
        for oob in ("flexible", "strict"):
            base = relocate_events(bf, f, wp, out_of_bounds=oob, **kw)
            rev = relocate_events(bf, f[::-1].copy(), wp, out_of_bounds=oob, **kw)
            assert all(same_event(base, e, rev, E - 1 - e) for e in range(E)), oob
            loud = f.copy()
            loud[4] = 1.0e6
            got = relocate_events(bf, loud, wp, out_of_bounds=oob, **kw)
            assert all(same_event(base, e, got, e) for e in range(E) if e != 4), oob
            assert not same_event(base, 4, got, 4)
    finally:
        bf.close()


def test_windows_of_a_resident_day_equal_the_sliced_batch():
    """The `starts` form: windows that abut, overlap and touch both ends of the day, read where the day lies."""
    import torch
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp = small_setup(5)
    n, n_day = 1500, 20_000
    day = syn.make_bp_features(tau, 9, 3, n_day, n_events=12)[0]
    starts = np.array([0, 1500, 3000, 3700, 3701, 9000, n_day - n, 9000], dtype=np.int64)   # abut, overlap, repeat
    batch = np.stack([day[:, :, s:s + n] for s in starts])
    bf = BeamformerGPU(tau, ws)
    try:
        day_dev = torch.as_tensor(day, device="cuda")
        for method in ("spatial", "temporal"):
            for oob in ("flexible", "strict"):
                want = relocate_events(bf, batch, wp, method, oob)
                for d in (day, day_dev):
                    got = relocate_events(bf, d, wp, method, oob, starts=starts, n_samples=n)
                    assert all(same_event(want, e, got, e) for e in range(len(starts))), (method, oob)
                got = relocate_events(bf, day_dev, wp, method, oob, starts=starts, n_samples=n, _chunk=3)
                assert all(same_event(want, e, got, e) for e in range(len(starts))), (method, oob)
        with pytest.raises(ValueError, match="leaves the day"):
            relocate_events(bf, day_dev, wp, starts=[n_day - n + 1], n_samples=n)
    finally:
        bf.close()


def duplicate_pairs(K):
    """200 pairs (a, b) of distinct sources: b becomes a copy of a."""
    src = np.random.default_rng(11).choice(K, 400, replace=False)
    return list(zip(src[:200].tolist(), src[200:].tolist()))


@pytest.fixture(scope="module")
def mid_plan():
    """Grid (40, 40, 10), 20 stations, 10 closest weighted, with duplicated sources: identical moveout rows and
    weights at different ids, so that wherever one of them holds the maximum the lowest id must win."""
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    geo = syn.make_bp_geometry((40, 40, 10), 20, 2, 50.0, n_closest=10)
    tau, ws = geo["moveouts"].copy(), geo["weights_sources"].copy()
    for a, b in duplicate_pairs(tau.shape[0]):
        tau[b], ws[b] = tau[a], ws[a]
    wp = syn.phase_weights(20, 3, 2)
    bf = BeamformerGPU(tau, ws)
    yield bf, tau, ws, wp
    bf.close()


def mid_events(tau, E, n=3000, seed=21, negative=True):
    rng = np.random.default_rng(seed)
    S = tau.shape[1]
    f = np.abs(rng.standard_normal((E, S, 3, n))).astype(np.float32)
    f[1] = np.round(f[1])
    f[2] = 0.0
    # arrivals planted on ordinary sources and (events 3 and 4) on the HIGHER id of a duplicated pair
    pairs = duplicate_pairs(tau.shape[0])
    for e in range(3, E):
        src, t0 = int(rng.integers(tau.shape[0])), int(rng.integers(200, n - 800))
        if e < 5:
            src = max(pairs[e])
        for s in range(S):
            f[e, s, 0, min(n - 1, t0 + tau[src, s, 0])] += 8.0
            f[e, s, 1:, min(n - 1, t0 + tau[src, s, 1])] += 8.0
    if negative and E > 6:
        f[5] = -f[5]                                                 # every beam <= 0: redone on its volume
        f[6] = rng.standard_normal(f[6].shape).astype(np.float32)    # mixed signs, positive maximum
    return f


def test_relocate_events_equals_the_per_event_path(mid_plan):
    from seismic_bpmf_amd.workflow import relocate_events, relocation_focus, relocation_likelihood
    bf, tau, ws, wp = mid_plan
    f = mid_events(tau, 33)
    for oob in ("flexible", "strict"):
        res = relocate_events(bf, f, wp, "spatial", oob, columns=True)
        tmp = relocate_events(bf, f, wp, "temporal", oob)
        like, cols = res["likelihood"].cpu().numpy(), res["columns"].cpu().numpy()
        for e in range(f.shape[0]):
            k, t, want_like = relocation_likelihood(bf, f[e], wp, oob)
            assert (res["src_idx"][e], res["time_idx"][e]) == (k, t), (oob, e)
            assert np.array_equal(like[e], want_like, equal_nan=True), (oob, e)
            k2, t2, col = relocation_focus(bf, f[e], wp, "spatial", oob)
            assert (k2, t2) == (k, t) and np.array_equal(cols[e], col), (oob, e)
            assert res["max_beam"][e] == col[k], (oob, e)
            ks, ts, maxbeam = relocation_focus(bf, f[e], wp, "temporal", oob)
            assert (tmp["src_idx"][e], tmp["time_idx"][e]) == (ks, ts), (oob, e)
            assert np.array_equal(tmp["maxbeam"][e].cpu().numpy(), maxbeam), (oob, e)
        assert res["max_beam"][5] <= 0 and res["max_beam"][6] > 0       # the fallback was exercised, and was not
        pairs = duplicate_pairs(tau.shape[0])
        for e in (3, 4):                                                # the copy was planted, the lower id wins
            assert res["src_idx"][e] == min(pairs[e]) and tmp["src_idx"][e] == min(pairs[e]), (oob, e)


def test_results_do_not_depend_on_the_event_chunk(mid_plan):
    from seismic_bpmf_amd.workflow import relocate_events
    bf, tau, ws, wp = mid_plan
    f = mid_events(tau, 12, seed=3)
    for method in ("spatial", "temporal"):
        whole = relocate_events(bf, f, wp, method)
        for chunk in (1, 5):
            got = relocate_events(bf, f, wp, method, _chunk=chunk)
            assert all(same_event(whole, e, got, e) for e in range(f.shape[0])), (method, chunk)
        one = relocate_events(bf, f[7:8], wp, method)                  # E = 1
        assert one["src_idx"].shape == (1,) and same_event(whole, 7, one, 0)
        none = relocate_events(bf, f[:0], wp, method)                  # E = 0
        assert none["src_idx"].shape == (0,) and none["time_idx"].shape == (0,)


def test_the_volume_is_never_allocated(mid_plan):
    """33 events at K = 16 000, N = 3 000: inputs, prestacks, partial rows and outputs of ALL of them stay below
    the K N 4 bytes of ONE event's volume (the library allocates nothing itself: workspace and outputs are
    torch tensors)."""
    import torch
    from seismic_bpmf_amd.workflow import relocate_events
    bf, tau, ws, wp = mid_plan
    f = mid_events(tau, 33, negative=False)
    relocate_events(bf, f[:2], wp)                                     # (the plan's dense tables are resident now)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = relocate_events(bf, f, wp, "spatial", columns=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    one_volume = bf.K * 3000 * 4
    assert one_volume == 192_000_000
    assert (res["max_beam"][[0, 1] + list(range(3, 33))] > 0).all()    # nobody took the per-event path
    assert peak < one_volume, (peak, one_volume)
    assert bf.relocation_workspace_bytes(33, 3000, 3) < one_volume // 4


def test_every_output_element_is_written(mid_plan):
    """Outputs handed in full of junk come back fully written (and debug.poison_output is on for the session: an
    element no kernel writes would come back as NaN / -1)."""
    import torch
    from seismic_bpmf_amd.workflow import relocate_events
    bf, tau, ws, wp = mid_plan
    f = mid_events(tau, 6, n=1700, seed=9, negative=False)
    E, N, K = 6, 1700, bf.K
    dev = bf.device
    fd, wpd = torch.as_tensor(f, device=dev), torch.as_tensor(wp, device=dev)
    ws_bytes = torch.empty(bf.relocation_workspace_bytes(E, N, 3), dtype=torch.uint8, device=dev)

    def junk(shape, dtype):
        return torch.full(shape, 12345, dtype=dtype, device=dev)

    for method in ("spatial", "temporal"):
        want = relocate_events(bf, f, wp, method, columns=True) if method == "spatial" else relocate_events(bf, f, wp, method)
        ti, si, mx = junk((E,), torch.int32), junk((E,), torch.int32), junk((E,), torch.float32)
        out = dict(likelihood=junk((E, K), torch.float32), columns=junk((E, K), torch.float32)) if method == "spatial" \
            else dict(maxbeam=junk((E, N), torch.float32), maxbeam_sources=junk((E, N), torch.int32))
        bf.relocate_batch(fd, 20 * 3 * N, N, None, wpd, E, N, 3, "flexible", method, ws_bytes, ti, si, mx, **out)
        assert np.array_equal(ti.cpu().numpy(), want["time_idx"]) and np.array_equal(si.cpu().numpy(), want["src_idx"])
        assert np.array_equal(mx.cpu().numpy(), want["max_beam"])
        for key, val in out.items():
            got = val.cpu().numpy()
            assert np.array_equal(got, want[key].cpu().numpy(), equal_nan=True), (method, key)
            assert not (got == 12345).any(), (method, key)
        assert np.isnan(out["likelihood"][2].cpu().numpy()).all() if method == "spatial" else True


def test_the_c_entry_point_checks_its_arguments(mid_plan, hip_opts):
    import torch
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd.workflow import relocate_events
    bf, tau, ws, wp = mid_plan
    f = mid_events(tau, 3, n=1700, negative=False)
    lib = _lib.lib()
    assert lib.bpmf_bp_relocate_workspace_bytes(None, 4, 800, 3) == 0
    dev = bf.device
    x = torch.zeros(16, device=dev)
    small = torch.empty(256, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.BpmfHipError, match="workspace too small"):
        bf.relocate_batch(torch.as_tensor(f, device=dev), 20 * 3 * 1700, 1700, None, torch.as_tensor(wp, device=dev), 3,
                          1700, 3, "flexible", "temporal", small, x.int(), x.int(), x,
                          maxbeam=torch.empty((3, 1700), device=dev),
                          maxbeam_sources=torch.empty((3, 1700), dtype=torch.int32, device=dev))
    rc = lib.bpmf_bp_relocate_batch_dev(bf._plan, None, 0, 0, None, None, None, None, 3, 1700, 3, 1, 0, None, 0,
                                        C.c_void_p(0), None, None, None, None, None, None, None)
    assert rc == -1
    # the alternative conventions are refused, not ignored
    hip_opts("bp.compat_first_computed", 1)
    with pytest.raises(_lib.BpmfHipError, match="compat"):
        relocate_events(bf, f, wp)
