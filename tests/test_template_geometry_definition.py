"""CPU: the host definitions of the pair geometry (postprocess.compute_distances_host, mercator_xy,
template_geometry_host, intertemplate_pair_mask, intertemplate_station_weights) against the reference's own output
(tests/golden/template_geometry.npz, written by tests/golden/make_template_geometry_golden.py from the real
BPMF methods with cartopy's two calls stubbed by the definitions), Snyder's worked example for the projection, the
sharpness of the checks the GPU file applies (tests/geometry_cases.py: every planted variant fails), the conditions on
the inputs that the GPU file's tolerances rest on, and the refusals of the device entry points that need no device.

The Mercator projection is restated from the documentation of PROJ and is NOT verified against cartopy here
(tests/test_template_geometry_cartopy_live.py does that where cartopy is installed)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import geometry_cases as gc  # noqa: E402
import uncertainty_cases as uc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402
from seismic_bpmf_amd import workflow  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "template_geometry.npz")) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------------- the reference's output ---
def test_distances_equal_the_reference_bit_for_bit(golden):
    for g in range(int(golden["n_groups"])):
        hypo, epi = pp.compute_distances_host(golden[f"longitude_{g}"], golden[f"latitude_{g}"], golden[f"depth_{g}"],
                                              golden[f"station_longitude_{g}"], golden[f"station_latitude_{g}"],
                                              golden[f"station_depth_{g}"], return_epicentral_distances=True)
        assert hypo.dtype == epi.dtype == np.float32
        assert np.array_equal(bits(hypo), bits(golden[f"source_receiver_dist_{g}"])), g
        assert np.array_equal(bits(epi), bits(golden[f"source_receiver_epicentral_{g}"])), g


def test_template_geometry_equals_the_reference(golden):
    """intertemplate_dist bit for bit (all-float32 depths); dir_errors within 1 float32 ulp (the reference's BLAS dot
    leaves the order of its three-term sums open); ellipsoid_dist the float32 (dist - err) - err.T."""
    for g in range(int(golden["n_groups"])):
        got = pp.template_geometry_host(golden[f"longitude_{g}"], golden[f"latitude_{g}"], golden[f"depth_{g}"],
                                        golden[f"cov_mat_{g}"], golden[f"has_cov_{g}"])
        dist, err, ell = (golden[f"{k}_{g}"] for k in ("intertemplate_dist", "dir_errors", "ellipsoid_dist"))
        assert np.array_equal(bits(got["intertemplate_dist"]), bits(dist)), g
        assert gc.ulps_apart(got["dir_errors"], err).max() <= 1, g
        assert (got["dir_errors"][~golden[f"has_cov_{g}"]] == 15.0).all()
        assert np.array_equal(bits(ell), bits((dist - err) - err.T)), g
        assert np.array_equal(bits(got["ellipsoid_dist"]),
                              bits((got["intertemplate_dist"] - got["dir_errors"]) - got["dir_errors"].T)), g
        assert (np.diagonal(got["intertemplate_dist"]) == 0.0).all()


def test_masks_and_weights_equal_the_reference_bit_for_bit(golden):
    """weights[t, u] of the reference = the station weights of t where not (ellipsoid_dist[u, t] > threshold), else 0."""
    checked = 0
    for g in range(int(golden["n_groups"])):
        base = pp.intertemplate_station_weights(golden[f"source_receiver_dist_{g}"], golden[f"availability_{g}"],
                                                golden[f"availability_per_cha_{g}"], int(golden[f"n_stations_{g}"]))
        assert base.dtype == np.float32
        ell = golden[f"ellipsoid_dist_{g}"]
        for j, threshold in enumerate(golden["distance_thresholds"]):
            mask = pp.intertemplate_pair_mask(ell, float(threshold))
            assert mask.dtype == bool
            want = golden[f"weights_{j}_{g}"]
            full = base[:, None, :, :] * mask[:, :, None, None]
            assert np.array_equal(bits(full), bits(want)), (g, j)
            checked += int(mask.sum() not in (0, mask.size))
            if not np.array_equal(mask, mask.T):
                checked += 100
    assert checked >= 1                                     # some threshold keeps part of the pairs


def test_station_weights_ties_and_missing_distances():
    dist = np.array([[3.0, 1.0, 1.0, np.nan, 2.0]])
    per_cha = np.ones((1, 5, 2), bool)
    w = pp.intertemplate_station_weights(dist, np.ones((1, 5), bool), per_cha, 2)
    assert np.array_equal(w[0, :, 0] > 0, [False, True, True, False, False])          # the tie: station order
    w = pp.intertemplate_station_weights(dist, np.array([[True, False, False, True, False]]), per_cha, 3)
    assert np.array_equal(w[0, :, 0] > 0, [True, True, False, True, False])           # NaN last; filled with the closest
    assert w.dtype == np.float32 and w.sum() == np.float32(1.0)
    with pytest.raises(ValueError):
        pp.intertemplate_station_weights(dist, np.ones((1, 4), bool), per_cha, 2)


# --------------------------------------------------------------------------------------------- the projection ---
def test_mercator_reproduces_snyders_worked_example():
    """Snyder (1987), Map Projections -- A Working Manual, p. 267: Clarke 1866, phi = 35 N, lambda = 75 W, lambda_0 =
    180 W gives x = 11 688 673.7 m, y = 4 139 145.6 m."""
    a, e2 = 6378206.4, 0.00676866
    f = 1.0 - np.sqrt(1.0 - e2)
    x, y = pp.mercator_xy(-75.0, 35.0, -180.0, a=a, f=f)
    assert abs(float(x) - 11688673.7) < 0.06 and abs(float(y) - 4139145.6) < 0.06, (float(x), float(y))


def test_mercator_is_odd_and_has_the_documented_scale():
    lat = np.linspace(-85.0, 85.0, 341)
    x, y = pp.mercator_xy(np.zeros_like(lat), lat, 0.0)
    assert (x == 0.0).all() and y[170] == 0.0
    assert np.array_equal(y, -y[::-1])
    e2 = pp.WGS84_F * (2.0 - pp.WGS84_F)
    phi = np.deg2rad(lat)
    h = 1e-6
    dy = (pp.mercator_xy(0.0, np.rad2deg(phi + h), 0.0)[1] - pp.mercator_xy(0.0, np.rad2deg(phi - h), 0.0)[1]) / (2 * h)
    want = pp.WGS84_A * (1.0 - e2) / ((1.0 - e2 * np.sin(phi) ** 2) * np.cos(phi))
    assert np.allclose(dy, want, rtol=1e-8, atol=0.0)
    # longitudes wrap about the central one
    x, _ = pp.mercator_xy(np.array([179.0, -179.0, 170.0]), np.zeros(3), 175.0)
    assert np.allclose(x, pp.WGS84_A * np.deg2rad([4.0, 6.0, -5.0]), rtol=1e-14)


# ------------------------------------------------------------------------- the checks of the GPU file are sharp ---
def test_the_definitions_pass_every_check_of_the_gpu_file():
    gc.run_all_checks(gc.HostStandIn())


def _variant_checks(variant):
    """The part of run_all_checks a planted variant must fail."""
    b = gc.HostStandIn(variant)
    if variant in ("root_dtype",):
        return lambda: [gc.check_distances(b, n, s, r) for n, s, r in gc.shape_cases(np.float32)]
    if variant == "swapped_roles":
        return lambda: [gc.check_distances(b, n, s, r) for n, s, r in gc.class_cases() if n == "regional"]
    if variant in ("mask_row_for_column", "less_equal"):
        return lambda: gc.check_masks(b, "synthetic", *gc.synthetic_mask_case())
    return lambda: [gc.check_geometry(b, c) for c in gc.template_cases() if c["name"] in ("T65_reference", "T3_reference")]


@pytest.mark.parametrize("variant", gc.VARIANTS)
def test_every_planted_variant_fails_the_checks(variant):
    with pytest.raises(AssertionError):
        _variant_checks(variant)()


# -------------------------------------------------------------------- what the GPU file's tolerances rest on ---
def test_input_conditions_of_the_gpu_comparison():
    for dtype in (np.float32, np.float64):
        name, src, rcv = gc.regional_case(dtype)
        metres, iters, done = gc.host_metres(src, rcv)
        assert done.all() and metres.min() >= 1000.0 and metres.max() <= 300000.0, (metres.min(), metres.max())
        hypo, epi = pp.hypocentral_from_metres(metres, src[2], rcv[2])
        for shift in (-1e-6, 1e-6):
            h2, e2 = pp.hypocentral_from_metres(metres + shift, src[2], rcv[2])
            assert (bits(e2) != bits(epi)).mean() < 0.02 and (bits(h2) != bits(hypo)).mean() < 0.02
    # the named classes: what the names promise, and no pair that converges only near the iteration limit
    for name, src, rcv in gc.class_cases():
        _, iters, done = gc.host_metres(src, rcv)
        assert (np.diagonal(done) == (name != uc.NOT_CONVERGENT)).all(), name
        assert iters[done].max() < 150, (name, iters[done].max())
    # no ellipsoid_dist of the mask cases within 2 ulp of a criterion (the synthetic case holds criteria EXACTLY)
    for case in gc.template_cases():
        if case["name"] in ("T65_reference", "T3_reference"):
            ell = gc.geometry_definition(case)["ellipsoid_dist"]
            for values in gc.MASK_CRITERIA:
                for v in (values[0], values[2]):
                    assert gc.ulps_apart(ell, np.full_like(ell, np.float32(v)))[np.sign(ell) == np.sign(v)].min() > 2


# ------------------------------------------------------------------------------ refusals that need no device ---
def test_refusals_before_any_device_call():
    lon, lat, dep = np.array([10.0, 11.0]), np.array([45.0, 46.0]), np.array([5.0, 6.0])
    cov = np.tile(np.eye(3), (2, 1, 1))
    with pytest.raises(ValueError, match="no CPU implementation"):
        workflow.compute_distances(lon, lat, dep, lon, lat, dep, device="cpu")
    with pytest.raises(ValueError, match="no CPU implementation"):
        workflow.template_geometry(lon, lat, dep, cov, device="cpu")
    with pytest.raises(ValueError, match="no CPU implementation"):
        workflow.template_pair_masks(np.zeros((2, 2), np.float32), distance_criterion=1.0, device="cpu")
    for bad in (np.array([10.0, np.nan]), np.array([10.0, np.inf])):
        with pytest.raises(ValueError, match="finite"):
            workflow.compute_distances(bad, lat, dep, lon, lat, dep)
        with pytest.raises(ValueError, match="finite"):
            workflow.template_geometry(lon, lat, bad, cov)
    for bad in (np.array([45.0, 90.5]), np.array([-91.0, 0.0])):
        with pytest.raises(ValueError, match="latitudes"):
            workflow.compute_distances(lon, lat, dep, lon, bad, dep)
        with pytest.raises(ValueError, match="latitudes"):
            workflow.template_geometry(lon, bad, dep, cov)
    with pytest.raises(ValueError, match="one length"):
        workflow.compute_distances(lon, lat[:1], dep, lon, lat, dep)
    with pytest.raises(ValueError, match="cov_mat"):
        workflow.template_geometry(lon, lat, dep, np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="has_cov"):
        workflow.template_geometry(lon, lat, dep, cov, has_cov=np.ones(3, bool))
    with pytest.raises(ValueError, match="depth_unit"):
        workflow.template_geometry(lon, lat, dep, cov, depth_unit="km")
    with pytest.raises(ValueError, match="nonconverged"):
        workflow.compute_distances(lon, lat, dep, lon, lat, dep, nonconverged="ignore")
    with pytest.raises(ValueError):
        workflow.template_pair_masks(np.zeros((2, 2), np.float32))                       # no criterion at all
    with pytest.raises(ValueError, match="float32"):
        workflow.template_pair_masks(np.zeros((2, 3), np.float32), distance_criterion=1.0)
    with pytest.raises(ValueError, match="float32"):
        workflow.template_pair_masks(np.zeros((2, 2)), distance_threshold=1.0)
    with pytest.raises(ValueError, match="intertemplate_cc"):
        workflow.template_pair_masks(np.zeros((2, 2), np.float32), distance_criterion=1.0, similarity_criterion=0.5)


def test_host_antipodal_pairs_raise_or_fall_back():
    with pytest.raises(ValueError, match="convergence"):
        pp.compute_distances_host([0.0], [0.0], [0.0], [180.0], [0.0], [0.0])
    d = pp.compute_distances_host([0.0], [0.0], [0.0], [180.0], [0.0], [0.0], nonconverged="antipodal")
    assert d[0, 0] == np.float32(uc.FALLBACK_M / 1000.0)
