"""The cases and the checks of the pair geometry (postprocess.compute_distances_host, template_geometry_host,
multiples_pair_mask, intertemplate_pair_mask; workflow.compute_distances, template_geometry, template_pair_masks),
shared by the host and the GPU tests.

A BACKEND is what is under test: an object with
    distances(src, rcv)                -> hypocentral, epicentral (K, R) float32, metres (K, R) float64, count int
    geometry(case)                     -> {"intertemplate_dist", "dir_errors", "ellipsoid_dist"}: (T, T) float32
    masks(ellipsoid, criterion, cc, similarity, threshold) -> pair_ok, pair_mask (T, T) bool
all NumPy.  tests/test_gpu_template_geometry.py wraps the device entry points into one; `HostStandIn` is the host
definitions with one switch per way of getting them wrong (VARIANTS), and tests/test_template_geometry_definition.py
checks that the checks below are SHARP: every planted variant fails at least one of them.

Tolerances (derived, none measured).
  metres: |device - host| <= 1e-9 km + 8 * 2^-53 d against uncertainty_cases.vincenty_from_tables, the same operations
    in NumPy on the same tables -- the limit of tests/test_gpu_location_uncertainty_edges.py with its summation factor
    (4 K, from a sum over K terms) replaced by a constant: a single geodesic is a few dozen roundings behind the last
    iteration, each at most 2^-53 relative.
  float32 outputs: bit for bit the definition's two rounding steps (postprocess.hypocentral_from_metres) applied to the
    backend's OWN metres -- IEEE divide, multiply, add and square root only.
  against the whole definition, regional case: float64 metres that differ by at most 1e-9 km + 8 * 2^-53 * 300 km
    < 1.1e-9 km land on different float32 kilometres only when a rounding boundary lies between them.  The float32
    spacing at 1 km is 1.2e-7 km, so that happens for at most about 1 % of the elements at 1 km and fewer beyond, and
    then by exactly one ulp: never more than 1 ulp apart, at most 2 % of the elements different.  The host test checks
    that condition on the inputs themselves (regional distances in 1 .. 300 km; moving the metres by +- 1e-6 m changes
    fewer than 2 % of the float32 kilometres).
  dir_errors: bit for bit -- float64 subtract, multiply, add, divide, sqrt of the SAME uploaded coordinates.
  ellipsoid_dist: bit for bit (dist - dir_errors) - dir_errors.T of the backend's own matrices, in float32.
  masks: bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uncertainty_cases as uc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

VARIANTS = ("no_abs", "dir_transposed", "chi2_90", "nan_kept", "depth_metres_under_reference", "float64_subtraction",
            "subtraction_order", "mask_row_for_column", "less_equal", "root_dtype", "swapped_roles")
TEMPLATE_SIZES = (1, 2, 3, 65, 257)
REL = 8 * 2.0 ** -53
ABS_KM = 1e-9


# ------------------------------------------------------------------------------------------------ cases ---
def _points(lon, lat, dep, dtype):
    return (np.asarray(lon, np.float64), np.asarray(lat, np.float64), np.asarray(dep, dtype))


def regional_case(dtype=np.float32, seed=20261021):
    """300 sources x 7 receivers in a 2 x 2 degree box around (-119, 36): every pair distance in 1 .. 300 km."""
    rng = np.random.default_rng(seed)
    rlon, rlat = rng.uniform(-120.0, -118.0, 7), rng.uniform(35.0, 37.0, 7)
    slon, slat = np.zeros(0), np.zeros(0)
    while slon.size < 300:                                   # keep the sources at least ~2 km from every receiver
        lon, lat = rng.uniform(-120.0, -118.0, 300), rng.uniform(35.0, 37.0, 300)
        far = (np.hypot((lon[:, None] - rlon) * 90.0, (lat[:, None] - rlat) * 111.0) > 2.0).all(axis=1)
        slon, slat = np.concatenate([slon, lon[far]])[:300], np.concatenate([slat, lat[far]])[:300]
    return ("regional", _points(slon, slat, rng.uniform(0.0, 30.0, 300), dtype),
            _points(rlon, rlat, rng.uniform(-3.0, 0.0, 7), dtype))


def shape_cases(dtype):
    """K x R = 1 x 1, 1 x 300, 300 x 7 (the regional case) and 257 x 3 (one lane past a workgroup)."""
    rng = np.random.default_rng(5)
    name, src, rcv = regional_case(dtype)
    one = tuple(x[:1] for x in src)
    lon, lat = rng.uniform(-125.0, -113.0, 300), rng.uniform(30.0, 42.0, 300)
    many = _points(lon, lat, rng.uniform(-3.0, 0.0, 300), dtype)
    src257 = _points(rng.uniform(-120.0, -118.0, 257), rng.uniform(35.0, 37.0, 257), rng.uniform(0.0, 30.0, 257), dtype)
    return [("1x1", one, tuple(x[:1] for x in rcv)), ("1x300", one, many), (name, src, rcv),
            ("257x3", src257, tuple(x[:3] for x in rcv))]


def class_cases(dtype=np.float64):
    """One case per named class of uncertainty_cases.geodesic_pairs: the first points are the sources, the second
    points the receivers, so that the class's pairs are the diagonal and every other element is a pair of the
    same region of the geodesic's branches."""
    rng = np.random.default_rng(uc.GEODESIC_SEED + 7)
    pairs = uc.geodesic_pairs()
    out = []
    for name in sorted({p[0] for p in pairs}):
        a = np.array([p[1] for p in pairs if p[0] == name])
        b = np.array([p[2] for p in pairs if p[0] == name])
        n = a.shape[0]
        out.append((name, _points(a[:, 0], a[:, 1], rng.integers(0, 160, n) * 0.25, dtype),
                    _points(b[:, 0], b[:, 1], rng.integers(-12, 1, n) * 0.25, dtype)))
    return out


def tables(points):
    su, cu = pp.reduced_latitude_sin_cos(points[1])
    return points[0], su, cu


def host_metres(src, rcv):
    """(metres (K, R), iterations, converged) of uncertainty_cases.vincenty_from_tables: receiver first."""
    slon, ssu, scu = tables(src)
    rlon, rsu, rcu = tables(rcv)
    K, R = slon.size, rlon.size
    g = lambda x, axis: np.broadcast_to(x[:, None] if axis == 0 else x[None, :], (K, R)).ravel()
    m, it, done = uc.vincenty_from_tables(g(rlon, 1), g(rsu, 1), g(rcu, 1), g(slon, 0), g(ssu, 0), g(scu, 0))
    return m.reshape(K, R), it.reshape(K, R), done.reshape(K, R)


def template_case(T, seed=None, depth_unit="reference"):
    """T templates in a 1 x 1 degree region, float64 coordinates as a catalogue holds them.  From T = 3 on: template 1
    lies AT template 0 (0 / 0 gives direction 0), template 2 under template 0 (the same epicentre, another depth).
    has_cov is mixed at T = 2 and from T = 4 on (at T = 3 the three special templates all carry one); among the
    covariances one is zero and one is negative definite (|.| matters), from T = 65 on one is indefinite as well."""
    rng = np.random.default_rng(1000 + T if seed is None else seed)
    lon, lat = rng.uniform(-119.5, -118.5, T), rng.uniform(35.5, 36.5, T)
    dep = rng.uniform(1.0, 25.0, T)
    if T >= 3:
        lon[1], lat[1], dep[1] = lon[0], lat[0], dep[0]
        lon[2], lat[2], dep[2] = lon[0], lat[0], dep[0] + 7.25
    a = rng.normal(0.0, 1.5, (T, 3, 3))
    cov = a @ a.transpose(0, 2, 1)
    has = np.ones(T, bool)
    if T >= 2:
        has[rng.random(T) < 0.3] = False
        has[0], has[T - 1] = True, False
    if T >= 3:
        has[1] = has[2] = True
        cov[1] = 0.0
        cov[2] = -cov[2]
    if T >= 65:
        has[5:9] = True
        cov[5] = 0.0
        cov[6] = -cov[6]
        cov[7] = np.diag([4.0, -9.0, 1.0])
    return {"name": f"T{T}_{depth_unit}", "longitude": lon, "latitude": lat, "depth": dep, "cov_mat": cov,
            "has_cov": has, "depth_unit": depth_unit}


def template_cases():
    cases = [template_case(T) for T in TEMPLATE_SIZES]
    cases += [template_case(T, depth_unit="metres") for T in (3, 65)]
    two = template_case(2, seed=77)                         # T = 2 with the two templates at one point
    two.update(name="T2_coincident", longitude=two["longitude"][[0, 0]], latitude=two["latitude"][[0, 0]],
               depth=two["depth"][[0, 0]], has_cov=np.array([True, True]))
    none = template_case(3, seed=78)                        # no covariance at all: every error 15.0
    none.update(name="T3_no_cov", cov_mat=None, has_cov=None)
    return cases + [two, none]


# (distance_criterion, similarity_criterion, distance_threshold): Python numbers compare as float32 (NumPy's weak
# scalars), NumPy float64 scalars as float64 -- 0.1 is not a float32, so the two differ at an element that holds it
MASK_CRITERIA = ((1.0, -1.0, 5.0), (15.0, 0.1, 1.0), (15.0, 0.5, 15.0), (0.1, -1.0, 0.1),
                 (np.float64(0.1), 0.5, np.float64(0.1)))


def synthetic_mask_case(T=65, seed=3):
    """A float32 matrix that is NOT symmetric, with NaN on one side of the diagonal only and elements exactly at every
    criterion of MASK_CRITERIA (as float32 rounds it), and a float32 similarity matrix with elements at 0.1 and 0.5."""
    rng = np.random.default_rng(seed)
    ell = rng.uniform(-30.0, 30.0, (T, T)).astype(np.float32)
    cc = rng.uniform(-0.2, 1.0, (T, T)).astype(np.float32)
    at = rng.permutation(T * T)
    for k, value in enumerate((1.0, 5.0, 15.0, 0.1)):
        for j in at[8 * k:8 * k + 8]:
            ell[j // T, j % T] = np.float32(value)
    for k, value in enumerate((0.1, 0.5)):
        for j in at[100 + 8 * k:108 + 8 * k]:
            cc[j // T, j % T] = np.float32(value)
    iu = np.triu_indices(T, 1)
    pick = rng.permutation(iu[0].size)[:40]
    ell[iu[0][pick], iu[1][pick]] = np.nan
    cc[iu[1][pick[:10]], iu[0][pick[:10]]] = np.nan
    return ell, cc


# ---------------------------------------------------------------------------------------------- backends ---
class HostStandIn:
    """The host definitions in the place of the device; `variant` plants one deviation (VARIANTS)."""

    def __init__(self, variant=None):
        assert variant is None or variant in VARIANTS
        self.variant = variant

    def distances(self, src, rcv):
        metres, _, done = host_metres(src, rcv)
        if self.variant == "swapped_roles" and metres.shape[0] == metres.shape[1]:
            metres = np.ascontiguousarray(host_metres(rcv, src)[0])          # element [k, r] is pair (r, k)
        sdep, rdep = src[2], rcv[2]
        if self.variant == "root_dtype":
            other = np.float64 if sdep.dtype == np.float32 else np.float32
            sdep, rdep = sdep.astype(other), rdep.astype(other)
        hypo, epi = pp.hypocentral_from_metres(metres, sdep, rdep)
        return hypo, epi, metres, int((~done).sum())

    def geometry(self, case):
        v = self.variant
        unit = "metres" if v == "depth_metres_under_reference" and case["depth_unit"] == "reference" else case["depth_unit"]
        lon, lat, dep, xyz, cov, has = pp.template_geometry_arguments(case["longitude"], case["latitude"], case["depth"],
                                                                      case["cov_mat"], case["has_cov"], unit)
        dist = pp.compute_distances_host(lon, lat, dep, lon, lat, dep, nonconverged="antipodal")
        T = lon.size
        err = np.zeros((T, T), np.float32)
        for t in range(T):
            if not has[t]:
                err[t] = 15.0
                continue
            d = xyz - xyz[t]
            n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            with np.errstate(all="ignore"):
                u = d / n[:, None]
            if v != "nan_kept":
                u[np.isnan(u)] = 0.0
            rows = [(cov[t, i, 0] * u[:, 0] + cov[t, i, 1] * u[:, 1]) + cov[t, i, 2] * u[:, 2] for i in range(3)]
            q = (rows[0] * u[:, 0] + rows[1] * u[:, 1]) + rows[2] * u[:, 2]
            with np.errstate(all="ignore"):
                err[t] = np.sqrt((6.251 if v == "chi2_90" else 3.52) * (q if v == "no_abs" else np.abs(q)))
        if v == "dir_transposed":
            err = np.ascontiguousarray(err.T)
        if v == "float64_subtraction":
            ell = (dist.astype(np.float64) - err - err.T).astype(np.float32)
        elif v == "subtraction_order":
            ell = (dist - err.T) - err
        else:
            ell = (dist - err) - err.T
        return {"intertemplate_dist": dist, "dir_errors": err, "ellipsoid_dist": ell}

    def masks(self, ellipsoid, criterion, cc, similarity, threshold):
        if self.variant == "less_equal":
            ok = ellipsoid <= criterion
            if similarity > -1.0:
                ok = ok & (cc >= similarity)
        else:
            ok = pp.multiples_pair_mask(ellipsoid, criterion, cc, similarity)
        if self.variant == "mask_row_for_column":
            return ok, ~(ellipsoid > threshold)
        return ok, pp.intertemplate_pair_mask(ellipsoid, threshold)


# ------------------------------------------------------------------------------------------------ checks ---
def ulps_apart(a, b):
    """Distance in float32 ulps of two float32 arrays of finite values of one sign or zero."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def check_distances(backend, name, src, rcv):
    """The metres against the host's operations on the same tables, the float32 outputs against the two rounding steps
    on the backend's own metres, the pairs that do not converge and their count.  Returns the figures."""
    hypo, epi, metres, count = backend.distances(src, rcv)
    K, R = src[0].size, rcv[0].size
    assert hypo.shape == epi.shape == metres.shape == (K, R), (name, hypo.shape)
    assert hypo.dtype == epi.dtype == np.float32 and metres.dtype == np.float64, name
    ref, _, done = host_metres(src, rcv)
    err_km = np.abs(metres - ref) / 1000.0
    bound = ABS_KM + REL * ref / 1000.0
    worst = float((err_km / bound)[done].max()) if done.any() else 0.0
    print(f"{name}: {K} x {R}, {int((~done).sum())} not convergent, lengths {ref.min() / 1e3:.6g} .. "
          f"{ref.max() / 1e3:.6g} km, worst |d metres| = {float(err_km[done].max()) if done.any() else 0.0:.3e} km "
          f"({worst:.3g} of the bound)")
    assert (err_km <= bound)[done].all(), (name, "metres", worst)
    assert (metres[~done] == uc.FALLBACK_M).all(), (name, "fallback", metres[~done])
    assert count == int((~done).sum()), (name, "count", count, int((~done).sum()))
    want_hypo, want_epi = pp.hypocentral_from_metres(metres, src[2], rcv[2])
    assert np.array_equal(epi.view(np.int32), want_epi.view(np.int32)), (name, "epicentral")
    assert np.array_equal(hypo.view(np.int32), want_hypo.view(np.int32)), (name, "hypocentral")
    return {"worst_of_bound": worst}


def check_against_definition(name, got, want, cap=0.02):
    """float32 kilometres against the whole definition: never more than 1 ulp apart, at most `cap` of them different."""
    apart = ulps_apart(got, want)
    frac = float((apart > 0).mean())
    print(f"{name}: {apart.size} elements, {frac:.4%} differ from the definition, at most {int(apart.max())} ulp")
    assert apart.max() <= 1, (name, int(apart.max()))
    if cap is not None:
        assert frac <= cap, (name, frac)
    return frac


def check_regional(backend, dtype):
    name, src, rcv = regional_case(dtype)
    hypo, epi, _, count = backend.distances(src, rcv)
    want_hypo, want_epi = pp.compute_distances_host(*src, *rcv, return_epicentral_distances=True)
    assert count == 0
    check_against_definition(f"{name} {np.dtype(dtype).name} epicentral", epi, want_epi)
    check_against_definition(f"{name} {np.dtype(dtype).name} hypocentral", hypo, want_hypo)


def check_geometry(backend, case, definition=None):
    """One template case.  `definition`: template_geometry_host of the case (computed here if not given)."""
    name = case["name"]
    T = case["longitude"].size
    got = backend.geometry(case)
    want = definition if definition is not None else geometry_definition(case)
    for key in ("intertemplate_dist", "dir_errors", "ellipsoid_dist"):
        assert got[key].shape == (T, T) and got[key].dtype == np.float32, (name, key)
    dist, err, ell = got["intertemplate_dist"], got["dir_errors"], got["ellipsoid_dist"]
    # (the 2 % cap is a statement about many elements: below 65 templates only the 1-ulp limit is checked)
    check_against_definition(f"{name} intertemplate_dist", dist, want["intertemplate_dist"], cap=0.02 if T >= 65 else None)
    assert (np.diagonal(dist) == 0.0).all() and not np.signbit(np.diagonal(dist)).any(), (name, "diagonal of dist")
    assert np.array_equal(err.view(np.int32), want["dir_errors"].view(np.int32)), \
        (name, "dir_errors", int((err.view(np.int32) != want["dir_errors"].view(np.int32)).sum()))
    has = np.ones(T, bool) if case["has_cov"] is None and case["cov_mat"] is not None else \
        np.zeros(T, bool) if case["has_cov"] is None else np.asarray(case["has_cov"], bool)
    assert (np.diagonal(err)[has] == 0.0).all() and (err[~has] == 15.0).all(), (name, "diagonal / default of dir_errors")
    own = (dist - err) - err.T
    assert own.dtype == np.float32
    assert np.array_equal(ell.view(np.int32), own.view(np.int32)), \
        (name, "ellipsoid_dist", int((ell.view(np.int32) != own.view(np.int32)).sum()))
    return got


def geometry_definition(case):
    return pp.template_geometry_host(case["longitude"], case["latitude"], case["depth"], case["cov_mat"], case["has_cov"],
                                     case["depth_unit"])


def check_masks(backend, name, ellipsoid, cc):
    """Both modes against the definitions for every criterion of MASK_CRITERIA."""
    for criterion, similarity, threshold in MASK_CRITERIA:
        ok, mask = backend.masks(ellipsoid, criterion, cc, similarity, threshold)
        want_ok = pp.multiples_pair_mask(ellipsoid, criterion, cc, similarity)
        want_mask = pp.intertemplate_pair_mask(ellipsoid, threshold)
        assert ok.dtype == mask.dtype == bool and ok.shape == mask.shape == ellipsoid.shape
        assert np.array_equal(ok, want_ok), (name, "pair_ok", criterion, similarity, int((ok != want_ok).sum()))
        assert np.array_equal(mask, want_mask), (name, "pair_mask", threshold, int((mask != want_mask).sum()))


def mask_inputs(ellipsoid, seed=11):
    """A geometry's ellipsoid_dist with NaN planted on one side of the diagonal, and a similarity matrix for it."""
    rng = np.random.default_rng(seed)
    T = ellipsoid.shape[0]
    ell = ellipsoid.copy()
    cc = rng.uniform(-0.2, 1.0, (T, T)).astype(np.float32)
    if T > 1:
        iu = np.triu_indices(T, 1)
        pick = rng.permutation(iu[0].size)[:max(1, iu[0].size // 50)]
        ell[iu[0][pick], iu[1][pick]] = np.nan
    return ell, cc


def run_all_checks(backend, definitions=None):
    """Every check of the GPU file on `backend` (what the planted variants must fail)."""
    for dtype in (np.float32, np.float64):
        for name, src, rcv in shape_cases(dtype):
            check_distances(backend, f"{name} {np.dtype(dtype).name}", src, rcv)
        check_regional(backend, dtype)
    for name, src, rcv in class_cases():
        check_distances(backend, name, src, rcv)
    for k, case in enumerate(template_cases()):
        got = check_geometry(backend, case, None if definitions is None else definitions[k])
        if case["name"] in ("T65_reference", "T3_reference"):
            check_masks(backend, case["name"], *mask_inputs(got["ellipsoid_dist"]))
    check_masks(backend, "synthetic", *synthetic_mask_case())
