"""CPU: the conditions on the inputs of tests/test_gpu_location_uncertainty_edges.py and the sensitivity of its
checks (the cases are those of tests/uncertainty_cases.py, the same objects the GPU file runs).

A / B.  The domain of every call holds exactly the n rows of lowest rank; every weighted |dz| is exactly 2, so the
float64 numerator of vunc is exact in any order and vunc is the exact numerator over the float32 denominator.
np.sum of the float32 weights is the chunk-of-8192 pairwise order the kernel implements, at every size of the
sweep; a running sum (n >= 15) and a pairwise sum that ignores the chunks (n > 8192) give another float32 for at
least one of the rows of every such size, and that moves vunc off the host's bits: the bit-equality of the GPU file
rejects both orders.  (One size is exempt by construction, not by luck: at n = 16 384 the root of the pairwise tree
splits into the two chunks, so the order without chunks IS NumPy's; the test asserts that identity instead.)

C.  Every pair of a convergent class converges on the host within 20 iterations and its length moves by less than
1e-10 km when the four table entries and the longitude move by one ulp; every pair of the non-convergent class
still fails at 2000 iterations; nothing lies in between.  The host's lengths are anchored to Vincenty's inverse in
50-digit arithmetic within 1e-9 km: the stop at |d lambda| < 1e-12 is worth about 2e-11 km (header of
tests/test_gpu_location_uncertainty.py) and some twenty float64 roundings at 2e4 km about 4e-11 km."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uncertainty_cases as uc  # noqa: E402


def test_the_sweep_holds_the_sizes_where_the_tree_changes_shape():
    need = {1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 135, 136, 137, 143, 144, 255, 256, 257, 1023, 1024,
            1025, 4095, 4096, 4097, 8191, 8192, 8193, 8199, 8200, 8320, 8321, 12345, 16383, 16384, 16385, 16391,
            16392, 24576, 24577, 24583, 24713, 24800}
    assert need <= set(uc.SWEEP_SIZES) and uc.SWEEP_K == 24_800 and uc.SWEEP_E == 4
    assert (uc.SWEEP_K + 255) // 256 == 97
    for K, blocks, seg in uc.LONG_GRIDS:
        assert (K + 255) // 256 == blocks and (blocks + 255) // 256 == seg and K > 65_536
        assert seg * 255 >= blocks              # the scan's last threads start beyond the counts: j0 = j1 = n_blocks
    assert 547 % 3 != 0                         # ... and at 547 one thread's segment is cut short by the clamp of j1


def check_domains(plan, like, sizes):
    """Per size: the host's domain is the n rows of lowest rank, vunc is the exact numerator over np.sum, and np.sum
    is sum_numpy_order.  Returns {n: (host result, float32 weights of the domain (E, n))}."""
    out = {}
    for n in sizes:
        host = uc.spatial_host(plan, like, uc.side_for(plan, n))
        want = np.zeros(plan["lon"].shape[0], bool)
        want[plan["members"][:n]] = True
        assert (host["n_domain"] == n).all() and (host["domain"] == want).all(), n
        w = like[:, want]                                     # (E, n) in row order: what the boolean index makes
        den = np.array([np.sum(like[e][want]) for e in range(like.shape[0])])
        assert den.dtype == np.float32
        assert np.array_equal(den, uc.sum_numpy_order(w)), n
        dz = np.abs(plan["dep"][plan["event"]] - plan["dep"][want])
        weighted = w > 0
        assert ((dz == 2.0) | ~weighted).all() and weighted.sum() == like.shape[0] * (n - 1)
        scaled = w.astype(np.float64) * 2.0 ** 24                  # integers: the weights are multiples of 2^-24
        exact = scaled.astype(np.int64).sum(axis=1)
        assert (scaled == np.floor(scaled)).all() and (exact < 2 ** 52).all()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(host["vunc"], exact * 2.0 ** -23 / den.astype(np.float64), equal_nan=True), n
        out[n] = (host, w)
    return out


def test_sweep_domains_are_exact_and_the_bit_equality_rejects_wrong_summation_orders():
    plan, like = uc.sweep_case()
    K = plan["lon"].shape[0]
    assert K == uc.SWEEP_K and like.shape == (uc.SWEEP_E, K) and like.dtype == np.float32
    assert plan["dep"][plan["event"]] == 10.0 and set(np.delete(plan["dep"], plan["event"])) == {8.0, 12.0}
    assert (like[:, plan["event"]] == 0).all()
    rest = np.delete(like, plan["event"], axis=1)
    assert (rest >= 0.5).all() and (rest < 1.0).all()
    # members of small domains lie scattered over the workgroups of 256 rows; most workgroups are empty
    assert len(set(plan["members"][:64] // 256)) >= 40 and len(set(plan["members"][:4097] // 256)) == 97
    from seismic_bpmf_amd import postprocess as pp
    far = np.abs(plan["lon"][plan["members"][-1]] - plan["lon"][plan["event"]]) * pp.domain_scale_per_longitude()
    assert abs(far - uc.FAR_KM) < 1e-6
    done = check_domains(plan, like, uc.SWEEP_SIZES)
    rejected = {"running": [], "pairwise without chunks": []}
    for n in uc.SWEEP_SIZES:
        host, w = done[n]
        good = uc.sum_numpy_order(w)
        for name, wrong, applies in (("running", uc.sum_running(w), n >= 15),
                                     ("pairwise without chunks", uc.sum_pairwise_without_chunks(w),
                                      n > 8192 and n != 16_384)):
            differs = wrong != good
            if name != "running" and (n <= 8192 or n == 16_384):
                assert not differs.any(), n                     # the same tree: nothing to tell apart
            if applies:
                assert differs.any(), (name, n)                 # a condition on the generator: change the seed
                rejected[name].append((n, int(differs.sum())))
            num = host["vunc"][differs] * good[differs].astype(np.float64)
            assert (num / wrong[differs].astype(np.float64) != host["vunc"][differs]).all(), (name, n)
    for name, rows in rejected.items():
        print(f"{name}: rejected at {len(rows)} sizes, rows that differ (of {uc.SWEEP_E}) per size:", rows)
    assert len(rejected["running"]) == sum(n >= 15 for n in uc.SWEEP_SIZES)
    assert len(rejected["pairwise without chunks"]) == sum(n > 8192 for n in uc.SWEEP_SIZES) - 1


def test_long_grid_domains_are_exact():
    for K, blocks, _ in uc.LONG_GRIDS:
        plan = uc.parallel_plan(K, uc.LONG_SEED)
        like = uc.likelihood_rows(plan, uc.LONG_E, uc.LONG_SEED + 100)
        check_domains(plan, like, (1, 300, 65_537, K))
        assert len(set(plan["members"][:300] // 256)) > 100
        ends = uc.parallel_plan(K, uc.LONG_SEED + 1, first_and_last=True)
        like = uc.likelihood_rows(ends, uc.LONG_E, uc.LONG_SEED + 101)
        n = ends["n_ends"]
        assert 256 < n < 512 and ends["event"] == K - 1
        host, _ = check_domains(ends, like, (n,))[n]
        inside = np.flatnonzero(host["domain"][0]) // 256
        assert set(inside) == {0, blocks - 1} and (inside == 0).sum() == 256 and K % 256 != 0


# ---------------------------------------------------------------- C ---
@pytest.fixture(scope="module")
def geo():
    from seismic_bpmf_amd import postprocess as pp
    case = uc.geodesic_case()
    su, cu = pp.reduced_latitude_sin_cos(case["lat"])
    s, d = case["src"], case["dst"]
    case["tables"] = (case["lon"][s], su[s], cu[s], case["lon"][d], su[d], cu[d])
    case["convergent"] = case["cls"] != uc.NOT_CONVERGENT
    return case


def test_every_class_of_the_geodesic_has_its_pairs_in_both_directions(geo):
    names, counts = np.unique(geo["cls"], return_counts=True)
    assert set(names) >= {"coincident", "equator_short", "equator_170", "date_line_equator", "date_line_mid_latitude",
                          "meridian_short", "meridian_70", "pole", "near_pole", "straddle_equator", "nano_degree",
                          "regional", "intercontinental", "near_antipodal_3deg", uc.NOT_CONVERGENT}
    assert (counts >= 16).all(), dict(zip(names, counts))                       # 8 pairs, both directions
    assert np.array_equal(geo["src"][0::2], geo["dst"][1::2]) and np.array_equal(geo["src"][1::2], geo["dst"][0::2])
    assert 200 <= geo["lon"].shape[0] <= 600 and (geo["likelihood"].sum(axis=1) == 1.0).all()
    lon, lat, s, d = geo["lon"], geo["lat"], geo["src"], geo["dst"]
    is_ = lambda name: geo["cls"] == name                                       # noqa: E731
    assert ((lon[s] == lon[d]) & (lat[s] == lat[d]))[is_("coincident")].all()
    for name in ("equator_short", "equator_170", "date_line_equator"):
        assert (lat[s][is_(name)] == 0).all() and (lat[d][is_(name)] == 0).all()
    for name in ("date_line_equator", "date_line_mid_latitude"):
        assert (np.abs(lon[s] - lon[d])[is_(name)] > 350).all()
    assert (lon[s] == lon[d])[is_("meridian_short") | is_("meridian_70")].all()
    assert (np.maximum(np.abs(lat[s]), np.abs(lat[d])) == 90)[is_("pole")].all()
    assert (np.minimum(np.abs(lat[s]), np.abs(lat[d])) >= 89.9)[is_("near_pole")].all()
    assert (lat[s] * lat[d] < 0)[is_("straddle_equator")].all()
    from seismic_bpmf_amd import postprocess as pp
    km = np.array([pp.geodesic_distance_m(lon[a], lat[a], lon[b], lat[b], nonconverged="antipodal")[0]
                   for a, b in zip(s, d)]) / 1000.0
    assert (km[is_("intercontinental")] > 5000).all() and (km[is_("intercontinental")] < 19_000).all()
    assert km[is_("intercontinental")].min() < 6000 and km[is_("intercontinental")].max() > 18_000
    assert (km[is_("near_antipodal_3deg")] > 19_500).all() and (km[is_("nano_degree")] < 2e-7).all()
    assert (km[is_("meridian_70")] > 7000).all() and (km[is_("equator_170")] > 18_000).all()


def test_the_table_form_is_the_host_function_and_the_pairs_are_convergent_or_hopeless(geo):
    from seismic_bpmf_amd import postprocess as pp
    lon, lat, s, d = geo["lon"], geo["lat"], geo["src"], geo["dst"]
    got, iters, done = uc.vincenty_from_tables(*geo["tables"])
    host = np.array([pp.geodesic_distance_m(lon[a], lat[a], lon[b], lat[b], nonconverged="antipodal")[0]
                     for a, b in zip(s, d)])
    assert np.array_equal(got, host)                                    # bit for bit: the same function
    conv = geo["convergent"]
    assert done[conv].all() and (iters[conv] <= 20).all() and (iters[conv] >= 1).all()
    print("iterations of the convergent classes: at most", int(iters[conv].max()))
    _, iters2k, done2k = uc.vincenty_from_tables(*geo["tables"], max_iter=2000)
    assert not done2k[~conv].any() and (got[~conv] == uc.FALLBACK_M).all()
    assert not ((iters2k > 20) & done2k).any()                          # nobody needs 21 .. 2000 iterations
    for a, b in zip(s[~conv], d[~conv]):
        with pytest.raises(ValueError, match="no convergence"):
            pp.geodesic_distance_m(lon[a], lat[a], lon[b], lat[b], max_iter=2000)
    # one ulp in each of the five inputs the device takes from its tables, either way
    worst = 0.0
    base = geo["tables"]
    for k in (1, 2, 3, 4, 5):                                           # su1, cu1, lon, su2, cu2
        for toward in (-np.inf, np.inf):
            moved = list(base)
            moved[k] = np.nextafter(base[k], toward)
            km = uc.vincenty_from_tables(*moved)[0] / 1000.0
            worst = max(worst, float(np.abs(km - got / 1000.0)[conv].max()))
    print("worst move of a convergent length under one ulp of an input:", worst, "km")
    assert worst < 1e-10
    assert uc.FALLBACK_M == np.pi * (pp.WGS84_A + (1.0 - pp.WGS84_F) * pp.WGS84_A) / 2.0
    assert abs(uc.FALLBACK_M / 1000.0 - 20_003.917) < 1e-3
    # the figures of geodesic_distance_m's docstring: half a meridian (pole to pole) is 14 m longer than the fallback
    half_meridian = pp.geodesic_distance_m(0.0, 90.0, 0.0, -90.0)[0]
    assert abs(half_meridian / 1000.0 - 20_003.931) < 1e-3 and 14.0 < half_meridian - uc.FALLBACK_M < 14.2
    assert abs(np.pi * (1.0 - pp.WGS84_F) * pp.WGS84_A / 1e3 - 19_970.3) < 0.05
    assert abs(np.pi * pp.WGS84_A / 1e3 - 20_037.5) < 0.05


def test_host_lengths_equal_vincenty_in_50_digit_arithmetic(geo):
    pytest.importorskip("mpmath")
    from seismic_bpmf_amd import postprocess as pp
    lon, lat, s, d = geo["lon"], geo["lat"], geo["src"], geo["dst"]
    worst, where, n = 0.0, None, 0
    for e in np.flatnonzero(geo["convergent"]):
        a, b = s[e], d[e]
        exact = uc.vincenty_mpmath(lon[a], lat[a], lon[b], lat[b])
        assert exact is not None, (geo["cls"][e], e)
        host = pp.geodesic_distance_m(lon[a], lat[a], lon[b], lat[b])[0]
        dev = abs(float(exact - host)) / 1000.0
        n += 1
        if dev > worst:
            worst, where = dev, (geo["cls"][e], (lon[a], lat[a]), (lon[b], lat[b]))
    print(f"{n} convergent pairs: worst |host - 50-digit Vincenty| = {worst:.3e} km at", where)
    assert n == int(geo["convergent"].sum()) and worst <= 1e-9
    for e in np.flatnonzero(~geo["convergent"])[:4]:
        assert uc.vincenty_mpmath(lon[s[e]], lat[s[e]], lon[d[e]], lat[d[e]], max_iter=500) is None


def test_the_geodesic_events_read_one_length_each(geo):
    """The one-hot likelihood rows on a side of 1e6 km: the host loop returns hunc = d(src, dst) / 1000 and
    vunc = |dz| exactly, with every source in the domain."""
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    host = location_uncertainties_host({"src_idx": geo["src"], "likelihood": geo["likelihood"]}, geo["lon"],
                                       geo["lat"], geo["dep"], "spatial", restricted_domain_side_km=1e6)
    K = geo["lon"].shape[0]
    assert (host["n_domain"] == K).all() and host["domain"].all()
    d = uc.vincenty_from_tables(*geo["tables"])[0]
    assert np.array_equal(host["hunc"], d / 1000.0)
    assert np.array_equal(host["vunc"], np.abs(geo["dep"][geo["src"]] - geo["dep"][geo["dst"]]))
    assert (host["hunc"][~geo["convergent"]] == uc.FALLBACK_M / 1000.0).all()


# ---------------------------------------------------------------- B / D: temporal streams ---
@pytest.mark.parametrize("N, kT, cutoff, share", [(70_001, 1.0, 0.25, 1.0), (70_001, 0.33, 0.97, 0.01),
                                                  (1500, 0.33, 0.25, None)])
def test_temporal_streams_keep_clear_of_the_cutoff(N, kT, cutoff, share):
    from seismic_bpmf_amd import postprocess as pp
    K, off, E = 864, 300, 3
    mb, ids, src = uc.temporal_stream(E, N, K, off, 23, kT, cutoff)
    assert mb.dtype == np.float32 and ids.dtype == np.int32 and ids.min() >= off and ids.max() < off + K
    assert len(np.unique(ids)) > 0.95 * K
    for e in range(E):
        w = pp.gibbs_weights(mb[e], kT)
        assert w.dtype == np.float32
        assert not (np.abs(w.astype(np.float64) - cutoff) <= 1e-5 * cutoff).any()
        admitted = (w > np.float32(cutoff)).sum() / N
        if share is not None:
            assert 0.7 * share <= admitted <= min(1.0, 1.3 * share), admitted
        assert src[e] == ids[e, mb[e].argmax()]
