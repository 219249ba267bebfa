"""CPU: host-side callers of the hot paths against golden vectors from the reference's own Python
(tests/golden/make_goldens.py).  Integer outputs must match exactly."""
import os

import numpy as np
import pytest

import golden_npz
from seismic_bpmf_amd import postprocess as pp
from seismic_bpmf_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return golden_npz.load(os.path.join(GOLD, name))


def test_sec_to_samp():
    g = load("host_helpers.npz")
    for sr in (25, 50, 100):
        got = pp.sec_to_samp(g["t"], float(sr))
        assert got.dtype == np.int64 and np.array_equal(got, g[f"sr_{sr}"])
        assert np.array_equal(syn.sec_to_samp(g["t"], float(sr)), g[f"sr_{sr}"])
    assert pp.sec_to_samp(7.96, 25.0) == 199 and pp.sec_to_samp(-0.04, 25.0) == -1


def test_detect_peaks():
    g = load("host_helpers.npz")
    assert list(pp.detect_peaks([0, 1, 0, 2, 0, 3, 0, 2, 0, 1, 0], mpd=2)) == [1, 5, 9]
    for j in range(int(g["n_series"])):
        for mpd in (1, 2, 25, 300):
            got = pp.detect_peaks(g[f"x_{j}"], mpd=mpd)
            assert np.array_equal(got, g[f"ind_{j}_{mpd}"]), (j, mpd)


def test_find_beam_detections():
    g = load("bp_find_detections.npz")
    for j in range(int(g["n_cases"])):
        peaks, src = pp.find_beam_detections(g[f"maxbeam_{j}"], g[f"sources_{j}"], g[f"thr_{j}"],
                                             int(g[f"mpd_{j}"]))
        assert np.array_equal(peaks, g[f"peaks_{j}"]), j
        assert np.array_equal(src, g[f"peak_sources_{j}"]), j
        assert peaks.size >= 3


def test_select_cc_indexes_python_variant():
    g = load("select_cc_indexes_py.npz")
    for j in range(int(g["n_cases"])):
        idx = pp.select_cc_indexes(
            g[f"x_{j}"], g[f"thr_{j}"], int(g[f"win_{j}"]), step=int(g[f"step_{j}"]), sr=float(g["sr"]),
            data_duration_sec=float(g["duration"]), n_dev_threshold=float(g["n_dev"]),
            min_freq_hz=float(g["min_freq_hz"]), data_buffer_sec=float(g["data_buffer_sec"]),
            remove_edges=bool(g[f"remove_edges_{j}"]),
            anomalous_cdf_at_mean_plus_1sig=float(g[f"acdf_{j}"]))
        assert np.array_equal(idx, g[f"idx_{j}"]), (j, idx, g[f"idx_{j}"])


def test_time_dependent_threshold_mad():
    g = load("tdt_mad.npz")
    thr = pp.time_dependent_threshold_mad(g["x"], int(g["window"]), float(g["n_dev"]),
                                          overlap=float(g["overlap"]), white_noise=g["white_noise"])
    assert thr.shape == g["thr"].shape and np.array_equal(thr, g["thr"])


def test_conditioning_helpers():
    rng = np.random.default_rng(0)
    d = rng.standard_normal((3, 2, 500)).astype(np.float32) * 7
    d[1, 1] = 0
    n = pp.normalize_data(d)
    assert np.allclose(n[0, 0].std(), 1.0, atol=1e-5) and not n[1, 1].any()
    w = pp.normalize_weights(rng.random((4, 3, 2)))
    assert np.allclose(w.sum(axis=(1, 2)), 1.0, atol=1e-6)
    tau = rng.integers(0, 200, (10, 6, 2))
    ws = pp.weights_sources_closest(tau, 3)
    assert (ws.sum(axis=1) >= 3).all() and set(np.unique(ws)) <= {0.0, 1.0}
    mv, first = pp.moveouts_to_samples(rng.uniform(1, 30, (5, 4, 2)), 50.0)
    assert mv.dtype == np.int32 and mv.min(axis=(1, 2)).max() == 0 and (first > 0).all()


def test_synthetic_generators_are_seeded_and_conditioned():
    a = syn.make_mf_inputs(3, 4, 3, 64, 20000, seed=5)
    b = syn.make_mf_inputs(3, 4, 3, 64, 20000, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in ("templates", "moveouts", "weights", "data"))
    assert np.allclose(a["data"].std(axis=-1), 1.0, atol=1e-4)
    assert np.allclose(a["templates"].std(axis=-1), 1.0, atol=1e-4)
    assert np.allclose(a["weights"].sum(axis=(1, 2)), 1.0, atol=1e-6)
    assert (a["moveouts"][:, :, 1] == a["moveouts"][:, :, 2]).all() and a["moveouts"].min() >= 0
    geo = syn.make_bp_geometry((5, 4, 3), 6, 2, 25.0)
    assert geo["moveouts"].shape == (60, 6, 2) and geo["moveouts"].min(axis=(1, 2)).max() == 0
    assert np.allclose(geo["weights_sources"].sum(axis=1), 1.0, atol=1e-6)


def test_bp_time_dependent_threshold():
    """Same windows / medians / MADs as the reference, and the linear interpolation in SciPy's own
    operation order (postprocess.interp_threshold): bit-identical to the reference's output."""
    g = load("bp_threshold.npz")
    thr = pp.bp_time_dependent_threshold(g["maxbeam"], int(g["window"]), float(g["n_dev"]),
                                         float(g["overlap"]))
    assert thr.shape == g["thr"].shape
    assert thr.dtype == g["thr"].dtype and np.array_equal(thr, g["thr"])
    # and the detections it leads to are identical
    a = pp.find_beam_detections(g["maxbeam"], np.arange(g["maxbeam"].size), thr, 200)[0]
    b = pp.find_beam_detections(g["maxbeam"], np.arange(g["maxbeam"].size), g["thr"], 200)[0]
    assert np.array_equal(a, b) and a.size > 0


def test_candidate_merge_equals_reference_selection_on_the_full_series():
    """workflow.merge_candidates on the sparse candidate list == the reference's select_cc_indexes
    loop on the whole series (golden), for every golden case without edge removal/validation."""
    from seismic_bpmf_amd.workflow import merge_candidates, search_window
    g = load("select_cc_indexes_py.npz")
    for j in (0, 3):
        x, thr, win = g[f"x_{j}"], g[f"thr_{j}"], int(g[f"win_{j}"])
        cand = np.flatnonzero(x > thr)
        got = merge_candidates(cand, x[cand], win)
        want = pp.select_cc_indexes(x, thr, win, step=1, sr=25.0, data_duration_sec=1e9,
                                    n_dev_threshold=8.0, min_freq_hz=2.0, data_buffer_sec=0.0,
                                    remove_edges=False, anomalous_cdf_at_mean_plus_1sig=0.0)
        assert np.array_equal(got, want)
    mv = np.array([[0, 40, 40], [10, 90, 90], [5, 25, 25]])
    assert search_window(mv, 100, 1) == 100 and search_window(mv, 10, 2) == 20.5


def test_numpy_order_sum_matches_numpy_bit_for_bit():
    """workflow.numpy_order_sum (element-wise torch adds) == np.sum over the last two axes of a
    contiguous float32 array, the reduction of dataset.py:4828-4830."""
    import torch
    from seismic_bpmf_amd.workflow import numpy_order_sum
    rng = np.random.default_rng(11)
    for S, C in [(1, 1), (2, 3), (3, 2), (4, 3), (8, 1), (20, 3), (40, 3), (43, 3), (50, 3), (100, 3), (200, 3)]:
        x = (rng.standard_normal((37, S, C)) * rng.random((37, S, C)) * 10.0 ** rng.integers(-3, 4, (37, S, C))).astype(np.float32)
        want = np.sum(x, axis=(-1, -2))
        got = numpy_order_sum(torch.as_tensor(x).reshape(37, S * C)).numpy()
        assert np.array_equal(got, want), (S, C)


def _suppress_reference_loop(ind, rank, mpd):
    """Restatement of the O(peaks^2) loop of BPMF/utils.py:2334-2345 (pins postprocess._suppress)."""
    order = ind[rank]
    dropped = np.zeros(order.size, dtype=bool)
    for q in range(order.size):
        if dropped[q]:
            continue
        near = (order >= order[q] - mpd) & (order <= order[q] + mpd)
        dropped |= near
        dropped[q] = False
    keep = np.zeros(ind.size, dtype=bool)
    keep[rank[~dropped]] = True
    return keep


def test_fast_peak_suppression_equals_the_reference_loop():
    """bpmf_suppress_peaks (host routine of the library) against the restated NumPy loop of
    BPMF/utils.py:2334-2345, ties and fractional mpd included."""
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(21)
    for trial in range(30):
        n = int(rng.integers(50, 4000))
        x = rng.integers(0, 12, n).astype(np.float64) if trial % 3 == 0 else rng.standard_normal(n)
        mpd = [2, 3, 7.5, 25, 100, 2.0001][trial % 6]
        dx = np.diff(x)
        ind = np.flatnonzero((np.append(dx, 0.0) <= 0) & (np.insert(dx, 0, 0.0) > 0))
        ind = ind[(ind > 0) & (ind < n - 1)]
        rank = np.argsort(x[ind])[::-1]
        want = _suppress_reference_loop(ind.astype(np.int64), rank.astype(np.int64), mpd)
        got = pp._suppress(ind, rank, mpd)
        assert np.array_equal(got, want), (trial, n, mpd)
        assert np.array_equal(pp.detect_peaks(x, mpd=mpd), ind[want])


# ------------------------------------------------------------------ BP-4 / MF-6 weight builders ---
def _kwargs(g, prefix, j):
    pre = f"{prefix}_kw_{j}_"
    return {k[len(pre):]: g[k].item() for k in g.files if k.startswith(pre)}


def test_weights_sources_match_reference():
    """Beamformer.set_weights_sources and its two builders (template_search.py:779-895), with and
    without offline stations, ties at the cut-off, n_min_stations, density weights, normalisation."""
    g = load("weights.npz")
    mv, online, dist = g["bp_moveouts"], g["bp_online"], g["bp_dist"]
    for j in range(int(g["bp_n_cases"])):
        kw = _kwargs(g, "bp", j)
        dens = None
        if kw.pop("weight_station_density", False):
            dens = pp.station_density_weights(dist, kw.pop("cutoff_dist", None),
                                              kw.pop("lower_percentile", 0.0),
                                              kw.pop("upper_percentile", 100.0))
        w = pp.set_weights_sources(mv, online=online if bool(g[f"bp_avail_{j}"]) else None,
                                   density_weights=dens, **kw)
        assert w.dtype == np.float32 and np.array_equal(w, g[f"bp_w_{j}"]), (j, kw)
    assert np.array_equal(pp.station_density_weights(dist), g["bp_density_default"])
    # the cut-off is taken over the operational stations only (template_search.py:786-795)
    w = pp.weights_sources_closest(mv, 4, online)
    assert (w[:, ~online] == 0).all() and (w.sum(axis=1) >= 4).all()


def test_weights_channels_match_reference():
    """MatchedFilter.set_weights_channels and its three builders (similarity_search.py:288-474)."""
    g = load("weights.npz")
    wav, mv, avail, dist = g["mf_waveforms"], g["mf_moveouts"], g["mf_availability"], g["mf_dist"]
    present = pp.network_to_template_map(wav)
    common = dict(present=present, moveouts=mv, availability=avail, sr=float(g["mf_sr"]),
                  min_channels=int(g["mf_min_channels"]), min_stations=int(g["mf_min_stations"]))
    for j in range(int(g["mf_n_cases"])):
        kw = _kwargs(g, "mf", j)
        dens = None
        if kw.pop("weight_station_density", False):
            dens = pp.station_density_weights(dist, kw.pop("cutoff_dist", None),
                                              kw.pop("lower_percentile", 0.0),
                                              kw.pop("upper_percentile", 100.0))
        w = pp.set_weights_channels(density_weights=dens, **common, **kw)
        assert w.dtype == np.float32 and np.array_equal(w, g[f"mf_w_{j}"]), (j, kw)
    if "mf_w_cha" in g.files:
        w = pp.set_weights_channels(method="closest_stations", num_closest_stations=4,
                                    data_channels_ok=g["mf_cha_ok"], **common)
        assert np.array_equal(w, g["mf_w_cha"])


def test_input_conditioning_matches_reference():
    """MatchedFilter.set_data (similarity_search.py:181-185) and TemplateGroup.normalize
    (dataset.py:4152-4166)."""
    g = load("weights.npz")
    assert np.array_equal(pp.normalize_data(g["sd_data"]), g["sd_data_arr"])
    for method in ("rms", "max"):
        assert np.array_equal(pp.normalize_templates(g["mf_waveforms"], method), g[f"tg_norm_{method}"])


def test_candidate_based_beam_detections_equal_the_full_series_logic():
    """Host half of the device detection stage (workflow.beam_detections_device): given only the
    rising-edge local maxima above a floor that no threshold value undercuts -- what
    csrc/bp_detect.hip compacts -- and window medians / MADs, the detections equal the ones of
    find_beam_detections on the whole series: the reference's goldens and time-dependent thresholds,
    plateaus, exact ties."""
    def local_maxima_above(x, floor):
        idx = np.flatnonzero((x[1:-1] > x[:-2]) & (x[2:] <= x[1:-1]) & (x[1:-1].astype(np.float64) > floor)) + 1
        return idx, x[idx]

    g = load("bp_find_detections.npz")
    for j in range(int(g["n_cases"])):
        mb, src, thr, mpd = g[f"maxbeam_{j}"], g[f"sources_{j}"], g[f"thr_{j}"], int(g[f"mpd_{j}"])
        idx, h = local_maxima_above(mb, float(thr[0]))
        peaks = pp.find_beam_detections_from_candidates(idx, h, lambda s: np.full(len(s), float(thr[0])), mpd,
                                                        mb.size, lambda i0, i1: mb[i0:i1])
        assert np.array_equal(peaks, g[f"peaks_{j}"]) and np.array_equal(src[peaks], g[f"peak_sources_{j}"])
    rng = np.random.default_rng(12)
    for n, window, mpd, gain in [(120_000, 9_000, 40, 4.0), (60_000, 6_000, 1, 1.0), (80_000, 8_000, 501, 2.5)]:
        x = np.abs(rng.standard_normal(n)).astype(np.float32)
        x[n // 2:] *= np.float32(gain)
        for p in rng.integers(1000, n - 1000, 40):
            x[p - 3:p + 4] += np.float32(rng.uniform(3, 30)) * np.array([.2, .6, .9, 1, .9, .6, .2], np.float32)
        x = np.round(x, 2)
        overlap, n_dev = 0.75, 8.0
        shift = int((1.0 - overlap) * window)
        nw = int((n - window) // shift) + 1
        med, mad = np.zeros(nw + 2, np.float32), np.zeros(nw + 2, np.float32)
        for q in range(1, nw + 1):
            seg = x[q * shift:min(n, q * shift + window)]
            med[q] = np.median(seg)
            mad[q] = np.median(np.abs(seg - med[q]))
        centre, nodes = pp.bp_threshold_nodes(n, window, overlap, med, mad, n_dev)
        full_thr = pp.bp_time_dependent_threshold(x, window, n_dev, overlap)
        assert np.array_equal(pp.interp_threshold(np.arange(n), centre, nodes), full_thr)
        want, _ = pp.find_beam_detections(x, np.zeros(n, np.int32), full_thr, mpd)
        idx, h = local_maxima_above(x, float(np.nextafter(np.float32(nodes.min()), np.float32(-np.inf))))
        got = pp.find_beam_detections_from_candidates(idx, h, lambda s: pp.interp_threshold(s, centre, nodes), mpd, n,
                                                      lambda i0, i1: x[i0:i1])
        assert np.array_equal(got, want) and want.size >= 5 and idx.size < n // 4


def test_has_close_ties():
    """Equal heights matter only within mpd of each other (postprocess.has_close_ties decides
    whether the device path needs the full list of local maxima)."""
    idx = np.array([10, 50, 400, 900])
    assert not pp.has_close_ties(idx, np.array([1.0, 2.0, 3.0, 4.0]), 100)
    assert pp.has_close_ties(idx, np.array([2.0, 2.0, 3.0, 4.0]), 40)
    assert not pp.has_close_ties(idx, np.array([2.0, 2.0, 3.0, 4.0]), 39)
    assert not pp.has_close_ties(idx, np.array([2.0, 5.0, 2.0, 2.0]), 300)      # equal, but far apart
    assert pp.has_close_ties(idx, np.array([2.0, 5.0, 2.0, 2.0]), 500)
    assert not pp.has_close_ties(idx[:1], np.array([2.0]), 500)


def test_relocation_likelihood_and_uncertainty_match_reference():
    """Beamformer._likelihood, the weighted means of _compute_location_uncertainty and the Gibbs weights
    of relocate_beam (BPMF/template_search.py:498-506, 1269-1333; dataset.py:2224-2231) against vectors
    produced by the reference's own methods (tests/golden/make_goldens.py: relocation_goldens)."""
    g = load("relocation.npz")
    for j in range(int(g["n_cases"])):
        like = pp.likelihood(g[f"column_{j}"])
        assert like.dtype == g[f"likelihood_{j}"].dtype and np.array_equal(like, g[f"likelihood_{j}"]), j
        hunc, vunc = pp.location_uncertainty(like[g[f"domain_{j}"]], g[f"distances_km_{j}"], g[f"depth_diff_{j}"])
        assert hunc == g[f"hunc_{j}"] and vunc == g[f"vunc_{j}"], j
        assert np.array_equal(pp.gibbs_weights(g[f"maxbeam_{j}"], float(g["effective_kT"])), g[f"gibbs_{j}"]), j


def test_geodesic_distance_known_answers_and_location_uncertainty():
    """postprocess.geodesic_distance_m stands in for cartopy's Geodesic().inverse(...)[:, 0] in
    Beamformer._compute_location_uncertainty (BPMF/template_search.py:1310-1320; cartopy is not in this image,
    so the reference's method cannot run here).  Pinned instead to published lengths on the same ellipsoid:
    the WGS84 quarter meridian (10 001 965.729 m), an arc of the equator (a x dlambda exactly), Geoscience
    Australia's Flinders Peak - Buninyong line (54 972.271 m; GRS80, whose flattening differs from WGS84's
    in the 11th digit) and GeographicLib's JFK - LHR example (5 551 759.400 m).  Tolerance: 1 mm -- the
    reference divides by 1000 and averages distances of kilometres."""
    d = pp.geodesic_distance_m
    assert abs(d(0.0, 0.0, 0.0, 90.0)[0] - 10_001_965.729) < 1e-3
    assert abs(d(12.0, -90.0, 77.0, 0.0)[0] - 10_001_965.729) < 1e-3          # from the pole, any longitude
    assert abs(d(0.0, 0.0, 10.0, 0.0)[0] - pp.WGS84_A * np.deg2rad(10.0)) < 1e-6
    assert abs(d(175.0, 0.0, -175.0, 0.0)[0] - pp.WGS84_A * np.deg2rad(10.0)) < 1e-6   # across the date line
    flinders = (144 + 25 / 60 + 29.52440 / 3600, -(37 + 57 / 60 + 3.72030 / 3600))
    buninyong = (143 + 55 / 60 + 35.38390 / 3600, -(37 + 39 / 60 + 10.15610 / 3600))
    assert abs(d(*flinders, *buninyong)[0] - 54_972.271) < 1e-3
    assert abs(d(*buninyong, *flinders)[0] - 54_972.271) < 1e-3               # symmetric
    assert abs(d(-73.8, 40.6, -0.5, 51.6)[0] - 5_551_759.400) < 1e-3
    # a regional grid around an event: vectorised call == one call per source; zero at the event itself;
    # close to the local flat-earth figure the reference's own _rectangular_domain uses (6371 km sphere)
    rng = np.random.default_rng(3)
    lon0, lat0 = 30.4, 40.7
    lons = lon0 + rng.uniform(-0.5, 0.5, 200)
    lats = lat0 + rng.uniform(-0.4, 0.4, 200)
    lons[0], lats[0] = lon0, lat0
    dist = d(lon0, lat0, lons, lats)
    assert dist[0] == 0.0 and np.all(np.isfinite(dist)) and np.all(dist[1:] > 0)
    assert np.array_equal(dist, np.concatenate([d(lon0, lat0, lons[i], lats[i]) for i in range(200)]))
    flat = 6371.0e3 * np.hypot(np.deg2rad(lats - lat0), np.deg2rad(lons - lon0) * np.cos(np.deg2rad(lat0)))
    assert np.all(np.abs(dist - flat) <= 0.006 * flat + 1.0)
    depth = rng.uniform(0.0, 30.0, 200)
    like = rng.random(200)
    hunc, vunc = pp.compute_location_uncertainty(lon0, lat0, 12.5, like, lons, lats, depth)
    assert hunc == np.sum(like * dist / 1000.0) / np.sum(like)
    assert vunc == np.sum(like * np.abs(12.5 - depth)) / np.sum(like)
    with pytest.raises(ValueError):
        d(0.0, 0.0, 179.9, 0.05)                                              # nearly antipodal: no silent wrong answer


def test_geodesic_distance_properties():
    """Symmetry, the triangle inequality and agreement with the meridian / equator closed forms over random
    regional point sets (the geometry a source grid has: points within a few degrees of one another)."""
    rng = np.random.default_rng(11)
    d = pp.geodesic_distance_m
    for _ in range(20):
        lon_c, lat_c = rng.uniform(-180, 180), rng.uniform(-70, 70)
        lon = lon_c + rng.uniform(-3, 3, 30)
        lat = lat_c + rng.uniform(-3, 3, 30)
        ab = d(lon[0], lat[0], lon[1:], lat[1:])
        ba = np.concatenate([d(lon[i], lat[i], lon[0], lat[0]) for i in range(1, 30)])
        assert np.all(np.abs(ab - ba) < 1e-6)
        bc = d(lon[1], lat[1], lon[2:], lat[2:])
        assert np.all(ab[1:] <= ab[0] + bc + 1e-6)
        # same meridian: the length is the difference of two meridian arcs from the equator
        m = d(lon_c, 0.0, [lon_c, lon_c], [lat_c, lat_c + 1.0])
        signed = np.sign([lat_c, lat_c + 1.0]) * m           # (arcs south of the equator count negative)
        assert abs(d(lon_c, lat_c, lon_c, lat_c + 1.0)[0] - abs(signed[1] - signed[0])) < 1e-5


def test_geodesic_antipodal_fallback_keeps_every_other_distance_exact():
    """geodesic_distance_m(nonconverged="antipodal"): the pairs Vincenty's iteration cannot finish get
    pi (a + b) / 2 (within 17 km of any geodesic between nearly antipodal points), every other pair keeps its
    exact length, and compute_location_uncertainty no longer fails on such a source
    (BPMF/template_search.py:1269-1333 calls cartopy, which always returns a length)."""
    import pytest
    from seismic_bpmf_amd import postprocess as pp
    lon = np.array([10.0, 179.9, -30.0])
    lat = np.array([5.0, 0.05, 40.0])
    with pytest.raises(ValueError):
        pp.geodesic_distance_m(0.0, 0.0, lon, lat)
    d = pp.geodesic_distance_m(0.0, 0.0, lon, lat, nonconverged="antipodal")
    exact = pp.geodesic_distance_m(0.0, 0.0, lon[[0, 2]], lat[[0, 2]])
    assert np.array_equal(d[[0, 2]], exact)
    assert abs(d[1] - np.pi * (pp.WGS84_A + (1 - pp.WGS84_F) * pp.WGS84_A) / 2) < 1e-6
    assert 20_003_900 < d[1] < 20_037_600
    hunc, vunc = pp.compute_location_uncertainty(0.0, 0.0, 5.0, np.array([1.0, 1e-9, 1.0]), lon, lat, np.array([4.0, 9.0, 8.0]))
    assert np.isfinite(hunc) and np.isfinite(vunc)


def test_excess_kurtosis_mirror_is_scipy_on_one_series():
    """postprocess.excess_kurtosis_f32 == np.float32(scipy.stats.kurtosis(series)) for ONE float32 series at a time
    (BPMF/similarity_search.py:640) -- on the row of tests/golden/kurtosis_scalar_pow_row.npz as well, whose m2 the C
    library's powf (what a NumPy scalar `**` calls) does not square like an array `**` does."""
    import os
    from scipy.stats import kurtosis
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(5)
    series = [np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kurtosis_scalar_pow_row.npz"))["row"]]
    for n in (1, 2, 9, 1000, 8193, 70_001):
        series.append((rng.standard_normal(n) * rng.uniform(0.01, 3)).astype(np.float32))
        series.append(np.full(n, 0.5, np.float32))
    for x in series:
        with np.errstate(all="ignore"):
            want = np.float32(kurtosis(x))
            got = pp.excess_kurtosis_f32(x)
        assert np.array_equal(got, want, equal_nan=True), x.size
        if x.size > 8:                      # and from the moments, as the device path finishes it
            m = np.mean(x, keepdims=True)
            s2 = (x - m) ** 2
            with np.errstate(all="ignore"):
                assert np.array_equal(pp.kurtosis_from_moments_f32(m[0], np.mean(s2), np.mean(s2 ** 2)), want, equal_nan=True)
