"""GPU: workflow.relocate_events(uncertainties=True) -- the location uncertainties of a batch of relocated events
on the device (csrc/bp_uncertainty.hip) -- against workflow.location_uncertainties_host, the per-event host loop,
run on the likelihood rows / max-beams the device itself returned: only this stage is under test.

Tolerances (derived, not tuned).  vunc has no transcendental: two sums of at most K non-negative float64 terms in
different orders, relative 4 K 2^-53.  hunc: the same relative term plus 1e-9 km absolute -- two correct Vincenty
iterations that stop at |d lambda| < 1e-12 differ by at most about tol f / (1 - f) = 3.4e-15 rad, 2e-11 km on the
ellipsoid; 1e-9 km is fifty times that and one micrometre on the ground.  Temporal: the float32 Gibbs weights of
device and host may differ in the last place (expf), so the test requires of its INPUTS that no sample's weight
lies within 1e-5 relative of the cut-off (asserted, no event left out); then the masks are equal and weights
within 2 ulp of float32 move a weighted mean of non-negative terms by at most about 4 2^-23 = 5e-7: relative 1e-6.
Domain masks, n_domain and the coordinates are exact.
(The host divides by np.sum of float32 weights, a float32 sum about 1e-7 from the exact one: the spatial tolerances
hold because the device takes that denominator in NumPy's own order, bit for bit, and only the float64
numerators are summed in another order.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORIGINS = [(30.0, 40.0), (-71.5, -33.0)]                 # mid-latitude, and the southern hemisphere


def small_setup(n_closest=5, origin=ORIGINS[0]):
    from seismic_bpmf_amd import synthetic as syn
    geo = syn.make_bp_geometry((12, 12, 6), 9, 2, 50.0, n_closest=n_closest)
    return geo["moveouts"], geo["weights_sources"], syn.phase_weights(9, 3, 2), \
        syn.geographic_coordinates(geo["sources"], origin)


def make_events(tau, n, seed, n_events=7):
    """(E, S, 3, n): two events of rounded features (many exact ties), an all-zero one, a planted arrival, and
    half-normal noise for the rest.  (The generator of tests/test_gpu_relocate_batch.py.)"""
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


def close(got, want, rel, absolute=0.0):
    """|got - want| <= rel |want| + absolute element by element, NaN where (and only where) want is NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool((np.abs(got[~nan] - want[~nan]) <= rel * np.abs(want[~nan]) + absolute).all())


def check_spatial(res, coords, side, K, what, offset=0):
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    lon, lat, dep = coords
    host = location_uncertainties_host(res, lon, lat, dep, "spatial", restricted_domain_side_km=side)
    rel = 4 * K * 2.0 ** -53
    print(what, "side", side, "n_domain", res["n_domain"].tolist(),
          "max |dhunc|", np.nanmax(np.abs(res["hunc"] - host["hunc"]), initial=0.0),
          "max |dvunc|", np.nanmax(np.abs(res["vunc"] - host["vunc"]), initial=0.0))
    assert res["n_domain"].dtype == np.int64 and res["hunc"].dtype == np.float64 and res["vunc"].dtype == np.float64
    assert np.array_equal(res["n_domain"], host["n_domain"]), what
    if "domain" in res:
        assert res["domain"].is_cuda and res["domain"].dtype.is_floating_point is False
        assert np.array_equal(res["domain"].cpu().numpy(), host["domain"]), what
    rows = res["src_idx"]
    assert np.array_equal(res["longitude"], lon[rows]) and np.array_equal(res["latitude"], lat[rows]), what
    assert np.array_equal(res["depth"], dep[rows]), what
    assert close(res["vunc"], host["vunc"], rel), (what, res["vunc"], host["vunc"])
    assert close(res["hunc"], host["hunc"], rel, 1e-9), (what, res["hunc"], host["hunc"])
    return host


def no_sample_near_the_cutoff(maxbeam, effective_kT, gibbs_cutoff):
    from seismic_bpmf_amd import postprocess as pp
    for e in range(maxbeam.shape[0]):
        w = pp.gibbs_weights(maxbeam[e], effective_kT).astype(np.float64)
        if (np.abs(w - gibbs_cutoff) <= 1e-5 * gibbs_cutoff).any():
            return False
    return True


def check_temporal(res, coords, K, what, offset=0, effective_kT=0.33, gibbs_cutoff=0.25):
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    lon, lat, dep = coords
    maxbeam = res["maxbeam"].cpu().numpy()
    assert no_sample_near_the_cutoff(maxbeam, effective_kT, gibbs_cutoff), what     # a condition on the inputs
    host = location_uncertainties_host(res, lon, lat, dep, "temporal", source_id_offset=offset,
                                       effective_kT=effective_kT, gibbs_cutoff=gibbs_cutoff)
    print(what, "n_domain", res["n_domain"].tolist(),
          "max rel dhunc", np.nanmax(np.abs(res["hunc"] - host["hunc"]) / np.maximum(host["hunc"], 1e-300), initial=0.0),
          "max rel dvunc", np.nanmax(np.abs(res["vunc"] - host["vunc"]) / np.maximum(host["vunc"], 1e-300), initial=0.0))
    assert np.array_equal(res["n_domain"], host["n_domain"]), what
    assert (res["n_domain"] >= 1).all(), what                                       # the maximum itself has weight 1
    rows = res["src_idx"] - offset
    assert np.array_equal(res["longitude"], lon[rows]) and np.array_equal(res["latitude"], lat[rows]), what
    assert np.array_equal(res["depth"], dep[rows]), what
    assert close(res["vunc"], host["vunc"], 1e-6), (what, res["vunc"], host["vunc"])
    assert close(res["hunc"], host["hunc"], 1e-6), (what, res["hunc"], host["hunc"])
    return host


def boundary_side(coords, k0, j):
    """The side that puts the longitude column of source j exactly on the boundary of the domain around k0."""
    from seismic_bpmf_amd import postprocess as pp
    return float(2.0 * (np.abs(coords[0][j] - coords[0][k0]) * pp.domain_scale_per_longitude()))


@pytest.mark.parametrize("origin", ORIGINS)
def test_spatial_uncertainties_equal_the_host_loop(origin):
    from seismic_bpmf_amd import BeamformerGPU, postprocess as pp
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5, origin)
    K = tau.shape[0]
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        f = make_events(tau, 1500, seed=41)
        for oob in ("flexible", "strict"):
            plain = relocate_events(bf, f, wp, "spatial", oob)
            k0 = int(plain["src_idx"][3])                       # the planted event; a column two steps east of it
            j = k0 + 2 * 12 * 6 if k0 + 2 * 12 * 6 < K else k0 - 2 * 12 * 6
            on = boundary_side(coords, k0, j)
            assert 10.0 < on < 100.0
            sizes = []
            for side in (100.0, 20.0, 5.0, on, float(np.nextafter(on, np.inf))):
                res = relocate_events(bf, f, wp, "spatial", oob, uncertainties=True, domain_mask=True,
                                      restricted_domain_side_km=side)
                assert np.array_equal(res["src_idx"], plain["src_idx"])
                check_spatial(res, coords, side, K, (origin, oob))
                # the all-zero event: a NaN likelihood row, not a number on both sides; the others are numbers
                assert np.isnan(res["hunc"][2]) and np.isnan(res["vunc"][2]) and res["n_domain"][2] > 0
                ok = np.arange(7) != 2
                assert np.isfinite(res["hunc"][ok]).all() and np.isfinite(res["vunc"][ok]).all()
                sizes.append(int(res["n_domain"][3]))
            # the column on the boundary is outside at `on` (strict <) and inside one ulp further
            assert sizes[4] > sizes[3] and sizes[0] > sizes[1] > sizes[2] >= 6, sizes
            assert not pp.rectangular_domain(coords[0][k0], coords[1][k0], coords[0], coords[1], side_km=on)[j]
    finally:
        bf.close()


@pytest.mark.parametrize("origin", ORIGINS)
def test_temporal_uncertainties_equal_the_host_loop(origin):
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5, origin)
    K = tau.shape[0]
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        for n, seed in ((1500, 41), (700, 42)):
            f = make_events(tau, n, seed=seed)
            for oob in ("flexible", "strict"):
                for kT, cut in ((0.33, 0.25), (1.0, 0.5)):
                    res = relocate_events(bf, f, wp, "temporal", oob, uncertainties=True, effective_kT=kT,
                                          gibbs_cutoff=cut)
                    assert "domain" not in res
                    check_temporal(res, coords, K, (origin, n, oob, kT), effective_kT=kT, gibbs_cutoff=cut)
                    assert res["n_domain"][2] == n                 # the all-zero event: every sample has weight 1
                    assert np.isfinite(res["hunc"]).all() and np.isfinite(res["vunc"]).all()
    finally:
        bf.close()


def same_uncertainties(a, b, keys=("hunc", "vunc", "n_domain", "longitude", "latitude", "depth")):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("method", ["spatial", "temporal"])
def test_bits_do_not_depend_on_the_batch(method):
    """Chunks of 1, 3 and E, a second run of the same call, and the `starts` form against the explicit batch:
    the same hunc, vunc and n_domain, bit for bit."""
    import torch
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5)
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        f = make_events(tau, 1500, seed=5)
        E = f.shape[0]
        whole = relocate_events(bf, f, wp, method, uncertainties=True, _chunk=E)
        assert np.isfinite(whole["hunc"]).sum() >= E - 1
        for chunk in (1, 3, None):
            got = relocate_events(bf, f, wp, method, uncertainties=True, _chunk=chunk)
            assert same_uncertainties(whole, got), (method, chunk)
        rev = relocate_events(bf, f[::-1].copy(), wp, method, uncertainties=True)
        assert all(np.array_equal(whole[k], rev[k][::-1], equal_nan=True) for k in ("hunc", "vunc", "n_domain"))
        n, n_day = 1500, 20_000
        day = syn.make_bp_features(tau, 9, 3, n_day, n_events=12)[0]
        starts = np.array([0, 1500, 3000, 3700, 3701, 9000, n_day - n, 9000], dtype=np.int64)
        batch = np.stack([day[:, :, s:s + n] for s in starts])
        want = relocate_events(bf, batch, wp, method, uncertainties=True)
        assert np.isfinite(want["hunc"]).all() and (want["hunc"] >= 0).all() and (want["hunc"] > 0).any()
        for d in (day, torch.as_tensor(day, device="cuda")):
            for chunk in (None, 3):
                got = relocate_events(bf, d, wp, method, starts=starts, n_samples=n, uncertainties=True, _chunk=chunk)
                assert same_uncertainties(want, got), (method, chunk)
        assert want["hunc"][5] == want["hunc"][7] and want["vunc"][5] == want["vunc"][7]      # the repeated window
    finally:
        bf.close()


def test_a_shard_with_a_source_id_offset_equals_the_same_rows_without():
    """One shard of a grid: rows [lo, hi) under source_id_offset = lo.  The coordinates are those of the shard's
    rows; maxbeam_sources and the temporal src_idx keep global ids and the kernel indexes its tables with
    id - offset.  Every output equals that of the same rows in a plan with offset 0."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5, ORIGINS[1])
    lo, hi = 300, 800
    shard = tuple(c[lo:hi] for c in coords)
    a = BeamformerGPU(tau[lo:hi], ws[lo:hi], source_id_offset=lo)
    b = BeamformerGPU(tau[lo:hi], ws[lo:hi])
    try:
        a.set_source_coordinates(*shard)
        b.set_source_coordinates(*shard)
        f = make_events(tau[lo:hi], 1500, seed=41)
        for oob in ("flexible", "strict"):
            ra = relocate_events(a, f, wp, "spatial", oob, uncertainties=True, domain_mask=True, restricted_domain_side_km=30.0)
            rb = relocate_events(b, f, wp, "spatial", oob, uncertainties=True, domain_mask=True, restricted_domain_side_km=30.0)
            assert same_uncertainties(ra, rb) and np.array_equal(ra["src_idx"], rb["src_idx"])
            assert np.array_equal(ra["domain"].cpu().numpy(), rb["domain"].cpu().numpy())
            check_spatial(ra, shard, 30.0, hi - lo, ("shard", oob))
            ta = relocate_events(a, f, wp, "temporal", oob, uncertainties=True)
            tb = relocate_events(b, f, wp, "temporal", oob, uncertainties=True)
            assert np.array_equal(ta["src_idx"], tb["src_idx"] + lo)
            assert np.array_equal(ta["maxbeam_sources"].cpu().numpy(), tb["maxbeam_sources"].cpu().numpy() + lo)
            assert same_uncertainties(ta, tb)
            check_temporal(ta, shard, hi - lo, ("shard", oob), offset=lo)
    finally:
        a.close()
        b.close()


def test_fallback_events_get_the_uncertainties_of_their_corrected_row():
    """Negative features: the maximum is not > 0, the event is redone on its volume, and its uncertainties are
    recomputed from the corrected row and likelihood."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events, relocation_likelihood
    tau, ws, wp, coords = small_setup(5)
    K = tau.shape[0]
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        f = make_events(tau, 1500, seed=8)
        f[4] = -f[4]                                                     # every beam <= 0
        f[5] = -np.round(f[5])                                           # ... with ties
        for oob in ("flexible", "strict"):
            res = relocate_events(bf, f, wp, "spatial", oob, uncertainties=True, domain_mask=True,
                                  restricted_domain_side_km=40.0)
            assert res["max_beam"][4] <= 0 and res["max_beam"][5] <= 0 and res["max_beam"][3] > 0
            for e in (4, 5):
                k, _, like = relocation_likelihood(bf, f[e], wp, oob)
                assert res["src_idx"][e] == k
                assert np.array_equal(res["likelihood"][e].cpu().numpy(), like, equal_nan=True)
            check_spatial(res, coords, 40.0, K, ("fallback", oob))
            assert np.isfinite(res["hunc"][[4, 5]]).all()
    finally:
        bf.close()


def test_full_size_grid_of_cfg3():
    """K = 50 000 on the 50 x 50 x 20 lattice over 100 km x 100 km, 64 windows of a resident day, side 100 km."""
    import torch
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    from seismic_bpmf_amd.workflow import relocate_events
    cfg = syn.BP_CONFIGS["cfg3"]
    geo = syn.make_bp_geometry(cfg["grid"], cfg["S"], cfg["P"], cfg["sr"])
    tau, ws = geo["moveouts"], geo["weights_sources"]
    K = tau.shape[0]
    assert K == 50_000
    coords = syn.geographic_coordinates(geo["sources"], ORIGINS[0])
    wp = syn.phase_weights(cfg["S"], cfg["C"], cfg["P"])
    n, n_day, E = 1500, 120_000, 64
    day = torch.as_tensor(syn.make_bp_features(tau, cfg["S"], cfg["C"], n_day, sr=cfg["sr"], n_events=40)[0], device="cuda")
    starts = np.sort(np.random.default_rng(64).integers(0, n_day - n, E))
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        res = relocate_events(bf, day, wp, starts=starts, n_samples=n, uncertainties=True)
        assert "domain" not in res
        check_spatial(res, coords, 100.0, K, "cfg3")
        assert (res["n_domain"] >= 20 * 25 * 25).all() and (res["n_domain"] < K).all()
        assert np.isfinite(res["hunc"]).all() and (res["hunc"] > 1.0).all() and (res["vunc"] > 0.1).all()
    finally:
        bf.close()


def test_without_uncertainties_nothing_changes():
    """uncertainties=False (the default) returns exactly the keys the call returned before, and the keys the two
    forms share hold the same bits."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5)
    bf = BeamformerGPU(tau, ws)
    try:
        f = make_events(tau, 1500, seed=41)
        with pytest.raises(ValueError, match="set_source_coordinates"):
            relocate_events(bf, f, wp, uncertainties=True)
        bf.set_source_coordinates(*coords)
        for method, keys in (("spatial", {"src_idx", "time_idx", "max_beam", "likelihood", "columns"}),
                             ("temporal", {"src_idx", "time_idx", "max_beam", "maxbeam", "maxbeam_sources"})):
            kw = dict(columns=True) if method == "spatial" else {}
            off = relocate_events(bf, f, wp, method, uncertainties=False, **kw)
            dflt = relocate_events(bf, f, wp, method, **kw)
            on = relocate_events(bf, f, wp, method, uncertainties=True, **kw)
            assert set(off) == keys and set(dflt) == keys
            assert set(on) == keys | {"longitude", "latitude", "depth", "hunc", "vunc", "n_domain"}
            for k in keys:
                for other in (dflt, on):
                    x, y = off[k], other[k]
                    x, y = (x.cpu().numpy(), y.cpu().numpy()) if hasattr(x, "cpu") else (x, y)
                    assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (method, k)
    finally:
        bf.close()


def test_every_output_is_written_and_the_entry_point_checks_its_arguments():
    """Outputs handed in full of junk come back written (debug.poison_output is on for the session), and bad
    arguments are refused before any launch."""
    import ctypes as C
    import torch
    from seismic_bpmf_amd import BeamformerGPU, _lib
    from seismic_bpmf_amd.workflow import relocate_events
    tau, ws, wp, coords = small_setup(5)
    K = tau.shape[0]
    bf = BeamformerGPU(tau, ws)
    try:
        bf.set_source_coordinates(*coords)
        f = make_events(tau, 700, seed=9)
        E, dev = f.shape[0], bf.device
        want = relocate_events(bf, f, wp, uncertainties=True, domain_mask=True)
        src = torch.as_tensor(want["src_idx"].astype(np.int32), device=dev)
        out = torch.full((5, E), 12345.0, dtype=torch.float64, device=dev)
        n_dom = torch.full((E,), 12345, dtype=torch.int32, device=dev)
        mask = torch.full((E, K), 7, dtype=torch.uint8, device=dev)
        work = torch.empty(bf.uncertainty_workspace_bytes(E, K), dtype=torch.uint8, device=dev)
        bf.location_uncertainty("spatial", E, 700, src, work, out, n_dom, likelihood=want["likelihood"], domain_mask=mask)
        got = out.cpu().numpy()
        for i, k in enumerate(("hunc", "vunc", "longitude", "latitude", "depth")):
            assert np.array_equal(got[i], want[k], equal_nan=True) and not (got[i] == 12345.0).any(), k
        assert np.array_equal(n_dom.cpu().numpy(), want["n_domain"])
        assert np.array_equal(mask.cpu().numpy(), want["domain"].cpu().numpy().astype(np.uint8))
        # a source id that is not of the plan: NaN and -1, nothing read outside the tables
        bad = src.clone()
        bad[1], bad[4] = K, -3
        bf.location_uncertainty("spatial", E, 700, bad, work, out, n_dom, likelihood=want["likelihood"])
        got, n_got = out.cpu().numpy(), n_dom.cpu().numpy()
        assert np.isnan(got[:, [1, 4]]).all() and (n_got[[1, 4]] == -1).all()
        keep = [0, 3, 5, 6]
        assert np.array_equal(got[0, keep], want["hunc"][keep]) and np.array_equal(n_got[keep], want["n_domain"][keep])
        lib = _lib.lib()
        assert lib.bpmf_bp_location_uncertainty_workspace_bytes(0, K) == 0
        with pytest.raises(_lib.BpmfHipError, match="workspace too small"):
            bf.location_uncertainty("spatial", E, 700, src, work[:64], out, n_dom, likelihood=want["likelihood"])
        with pytest.raises(_lib.BpmfHipError, match="null pointer"):
            bf.location_uncertainty("spatial", E, 700, src, work, out, n_dom)
        with pytest.raises(_lib.BpmfHipError, match="null pointer"):
            bf.location_uncertainty("temporal", E, 700, src, work, out, n_dom, likelihood=want["likelihood"])
        with pytest.raises(_lib.BpmfHipError, match="bad argument"):
            bf.location_uncertainty("spatial", E, 700, src, work, out, n_dom, likelihood=want["likelihood"], side_km=-1.0)
        rc = lib.bpmf_bp_location_uncertainty_dev(bf._plan, 5, E, 700, None, None, None, None, None, None, 1.0, 1.0, 1.0,
                                                  1.0, None, 0, C.c_void_p(0), None, None, None, None, None, None, None)
        assert rc == -1 and "method" in _lib.last_error()
    finally:
        bf.close()
