"""Seeded inputs for the edge tests of the location uncertainties (CPU and GPU): source rows on one parallel whose
domain holds exactly the n rows of lowest rank, likelihood rows that make the float64 numerator of vunc exact,
the float32 summation orders that are and are not NumPy's, named pairs of points for every branch of the geodesic,
postprocess.geodesic_distance_m with the reduced latitudes handed in (as the device reads them from its tables),
and Vincenty's inverse in 50-digit arithmetic.  Not a test module."""
import numpy as np

# ---------------------------------------------------------------- A / B: sources on one parallel ---
PARALLEL_LAT, PARALLEL_LON0, FAR_KM = 35.0, 30.0, 40.0
SWEEP_K, SWEEP_E, SWEEP_SEED = 24_800, 4, 50
SWEEP_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 135, 136, 137, 143, 144, 255, 256, 257, 1023,
               1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 8199, 8200, 8320, 8321, 12345, 16383, 16384, 16385,
               16391, 16392, 24576, 24577, 24583, 24713, SWEEP_K)
LONG_GRIDS = ((70_001, 274, 2), (140_003, 547, 3))          # K, workgroups of 256, counts per thread of the scan
LONG_E, LONG_SEED = 3, 21


def parallel_plan(K, seed, first_and_last=False):
    """K source rows on the parallel of 35 degrees, longitudes lon0 + j delta for the RANK j = 0 .. K-1 of a row;
    the ranks are a seeded permutation of the rows, so the n rows of lowest rank lie scattered over all workgroups
    of 256 rows.  delta puts rank K-1 at 40 km from rank 0 by the domain's own scale (km per degree of a great
    circle).  The event is the row of rank 0, 10 km deep; every other row is 12 or 8 km deep by a seeded coin.
    first_and_last: the rows of the first and of the last (partly filled) workgroup take the lowest ranks, the
    event is the last row.  Returns dict(lon, lat, dep, rank, event, members) -- members: the rows ordered by rank."""
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    delta = FAR_KM / ((K - 1) * pp.domain_scale_per_longitude())
    if first_and_last:
        ends = np.concatenate([np.arange(256), np.arange((K - 1) // 256 * 256, K)])
        rest = np.setdiff1d(np.arange(K), ends)
        members = np.concatenate([[K - 1], rng.permutation(ends[:-1]), rng.permutation(rest)])
    else:
        members = rng.permutation(K)
    rank = np.empty(K, np.int64)
    rank[members] = np.arange(K)
    lon = PARALLEL_LON0 + rank * delta
    dep = np.where(rng.random(K) < 0.5, 12.0, 8.0)
    dep[members[0]] = 10.0
    return dict(lon=lon, lat=np.full(K, PARALLEL_LAT), dep=dep, rank=rank, event=int(members[0]), members=members,
                n_ends=(256 + K - (K - 1) // 256 * 256) if first_and_last else None)


def side_for(plan, n):
    """A side (km) whose half lies halfway between the scaled longitude differences of rank n-1 and rank n: exactly
    the n rows of lowest rank pass the strict `<` of the domain."""
    from seismic_bpmf_amd import postprocess as pp
    K = plan["lon"].shape[0]
    dx = np.sort(np.abs(plan["lon"] - plan["lon"][plan["event"]]) * pp.domain_scale_per_longitude())
    assert 1 <= n <= K
    half = 0.5 * (dx[n - 1] + dx[n]) if n < K else dx[K - 1] + 0.5 * (dx[K - 1] - dx[K - 2])
    return 2.0 * float(half)


def likelihood_rows(plan, E, seed):
    """(E, K) float32 weights uniform in [0.5, 1), the event's own 0.  With every |dz| of a weighted row exactly
    2 km the float64 numerator of vunc, sum w 2, is exact in any order: fewer than 2^17 multiples of 2^-23 below
    2, and 17 + 1 + 24 bits < 53."""
    rng = np.random.default_rng(seed)
    K = plan["lon"].shape[0]
    like = (0.5 + 0.5 * rng.random((E, K), dtype=np.float32)).astype(np.float32)
    like = np.minimum(like, np.nextafter(np.float32(1.0), np.float32(0.0)))
    like[:, plan["event"]] = 0.0
    return like


def sweep_case():
    plan = parallel_plan(SWEEP_K, SWEEP_SEED)
    return plan, likelihood_rows(plan, SWEEP_E, SWEEP_SEED + 100)


def spatial_host(plan, like, side):
    """workflow.location_uncertainties_host on the arrays of a plan: the yardstick."""
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    E = like.shape[0]
    res = {"src_idx": np.full(E, plan["event"], np.int64), "likelihood": like}
    return location_uncertainties_host(res, plan["lon"], plan["lat"], plan["dep"], "spatial",
                                       restricted_domain_side_km=side)


# ---------------------------------------------------------------- float32 summation orders ---
def _pairwise_f32(x):
    """NumPy's pairwise sum over the last axis of a float32 array: a running sum below 8 elements, up to 128 eight
    strided running sums combined as a tree plus the tail, above that halves cut at a multiple of 8."""
    n = x.shape[-1]
    if n < 8:
        res = np.zeros(x.shape[:-1], np.float32)
        for i in range(n):
            res = res + x[..., i]
        return res
    if n <= 128:
        r = [x[..., j] for j in range(8)]
        m = n - n % 8
        for i in range(8, m, 8):
            r = [r[j] + x[..., i + j] for j in range(8)]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(m, n):
            res = res + x[..., i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise_f32(x[..., :n2]) + _pairwise_f32(x[..., n2:])


def sum_numpy_order(x):
    """np.sum of float32 over the last axis as csrc/bp_uncertainty.hip takes it: chunks of 8192 added one after the
    other to a float32 zero, each chunk summed pairwise."""
    x = np.asarray(x, np.float32)
    res = np.zeros(x.shape[:-1], np.float32)
    for c in range(0, x.shape[-1], 8192):
        res = res + _pairwise_f32(x[..., c:c + 8192])
    return res


def sum_pairwise_without_chunks(x):
    """A wrong order: the pairwise recursion over the whole vector.  (At n = 16 384 it is the right one: the halves
    of the root are the two chunks, (0 + P(8192)) + P(8192).  Up to 8192 there is one chunk and no difference.)"""
    return _pairwise_f32(np.asarray(x, np.float32))


def sum_running(x):
    """A wrong order: one float32 running sum."""
    x = np.asarray(x, np.float32)
    return np.add.accumulate(x, axis=-1, dtype=np.float32)[..., -1]


# ---------------------------------------------------------------- C: named pairs for the geodesic ---
NOT_CONVERGENT = "not_convergent"
GEODESIC_SEED = 22


def _antipode(lon, lat):
    return (lon - 180.0 if lon > 0 else lon + 180.0), -lat


def _offset(lon, lat, dist_deg, azimuth_deg):
    """The point `dist_deg` of arc from (lon, lat) at an azimuth, on a sphere (the classes need only about that)."""
    p, l, d, z = np.deg2rad([lat, lon, dist_deg, azimuth_deg])
    lat2 = np.arcsin(np.clip(np.sin(p) * np.cos(d) + np.cos(p) * np.sin(d) * np.cos(z), -1.0, 1.0))
    lon2 = l + np.arctan2(np.sin(z) * np.sin(d) * np.cos(p), np.cos(d) - np.sin(p) * np.sin(lat2))
    return float((np.rad2deg(lon2) + 180.0) % 360.0 - 180.0), float(np.rad2deg(lat2))


def geodesic_pairs(seed=GEODESIC_SEED):
    """[(class, (lon, lat), (lon, lat))]: at least 8 pairs of every class of the geodesic's branches."""
    rng = np.random.default_rng(seed)
    u = rng.uniform
    out = []

    def add(name, p, q):
        out.append((name, (float(p[0]), float(p[1])), (float(q[0]), float(q[1]))))

    for p in ((0.0, 0.0), (12.5, 47.25), (-70.0, -33.0), (180.0, 10.0), (-180.0, -60.0), (33.0, 90.0), (5.0, -90.0),
              (100.0, 0.0), (u(-180, 180), u(-89, 89))):
        add("coincident", p, p)
    for _ in range(8):
        lon = u(-170, 0)
        add("equator_short", (lon, 0.0), (lon + u(1e-3, 2.0), 0.0))
        lon = u(-175, 0)
        add("equator_170", (lon, 0.0), (lon + 170.0, 0.0))
        add("date_line_equator", (180.0 - u(1e-3, 2.0), 0.0), (-180.0 + u(1e-3, 2.0), 0.0))
        lat = u(20, 60) * rng.choice([-1.0, 1.0])
        add("date_line_mid_latitude", (180.0 - u(1e-3, 2.0), lat), (-180.0 + u(1e-3, 2.0), lat + u(-1, 1)))
        lon, lat = u(-180, 180), u(-60, 60)
        add("meridian_short", (lon, lat), (lon, lat + u(1e-3, 1.0)))
        lon, lat = u(-180, 180), u(-80, 10)
        add("meridian_70", (lon, lat), (lon, lat + 70.0))
    add("date_line_equator", (180.0, 0.0), (-180.0, 0.0))                  # the same point under two longitudes
    add("date_line_mid_latitude", (180.0, 40.0), (-179.5, 40.0))
    for s in (1.0, -1.0):
        add("pole", (u(-180, 180), 0.0), (u(-180, 180), 90.0 * s))
        add("pole", (0.0, 0.0), (0.0, 90.0 * s))
        add("pole", (u(-180, 180), 90.0 * s), (u(-180, 180), u(-89, 89)))
        add("pole", (0.0, 90.0 * s), (u(-180, 180), 45.0))
        add("pole", (u(-180, 180), 90.0 * s), (u(-180, 180), -89.5 * s))
        add("pole", (0.0, 90.0 * s), (0.0, -90.0 * s))
        add("pole", (10.0, 90.0 * s), (95.0, -90.0 * s))
        add("pole", (u(-180, 180), 90.0 * s), (u(-180, 180), (90.0 - 1e-6) * s))
        for _ in range(4):
            add("near_pole", (u(-180, 180), s * (90.0 - u(0, 0.1))), (u(-180, 180), s * (90.0 - u(0, 0.1))))
    for dlon in (0.0, 0.0, 1e-9, 1e-3, 0.5, 3.0, 40.0, 120.0):
        lon = u(-180, 50)
        add("straddle_equator", (lon, 1e-9), (lon + dlon, -1e-9))
    for lat in (0.0, 45.0, 80.0, -33.0):
        lon = u(-179, 179)
        add("nano_degree", (lon, lat), (lon + 1e-9, lat))
        add("nano_degree", (lon, lat), (lon, lat + 1e-9))
        add("nano_degree", (lon, lat), (lon - 1e-9, lat - 1e-9))
    for lat in (0.0, 45.0, -45.0, 80.0, -80.0):
        for _ in range(2):
            lon = u(-170, 170)
            add("regional", (lon + u(-3, 3), lat + u(-3, 3)), (lon + u(-3, 3), lat + u(-3, 3)))
    for k in range(10):
        p = (u(-180, 180), u(-70, 70))
        add("intercontinental", p, _offset(*p, 45.5 + 124.0 * k / 9.0, u(0, 360)))      # 5 000 to 19 000 km
        add("near_antipodal_3deg", p, _offset(*_antipode(*p), 3.0, u(0, 360)))
    for lon, lat in ((0.0, 0.0), (-120.0, 0.0), (77.5, 0.0), (180.0, 0.0), (10.0, 30.0), (-60.0, -45.0), (150.0, 5.0),
                     (-33.0, 80.0)):
        add(NOT_CONVERGENT, (lon, lat), _antipode(lon, lat))
    add(NOT_CONVERGENT, (0.0, 0.0), (179.9, 0.05))
    add(NOT_CONVERGENT, (0.0, 0.0), (179.5, 0.2))
    return out


def geodesic_case(seed=GEODESIC_SEED):
    """The plan of the named points and one event per direction of every pair: dict(lon, lat, dep (K,), src, dst
    (E,) rows, cls (E,) class names, likelihood (E, K) float32 -- 1 at dst[e], 0 elsewhere, so that
    hunc[e] = d(src[e], dst[e]) and vunc[e] = |dep[src[e]] - dep[dst[e]]|)."""
    pairs = geodesic_pairs(seed)
    rng = np.random.default_rng(seed + 1)
    pts = np.array([p for _, a, b in pairs for p in (a, b)])
    K = pts.shape[0]
    src = np.array([r for i in range(len(pairs)) for r in (2 * i, 2 * i + 1)])
    dst = np.array([r for i in range(len(pairs)) for r in (2 * i + 1, 2 * i)])
    cls = np.array([name for name, _, _ in pairs for _ in (0, 1)])
    like = np.zeros((src.shape[0], K), np.float32)
    like[np.arange(src.shape[0]), dst] = 1.0
    return dict(lon=pts[:, 0].copy(), lat=pts[:, 1].copy(), dep=rng.integers(0, 160, K) * 0.25, src=src, dst=dst,
                cls=cls, likelihood=like)


FALLBACK_M = np.pi * (6378137.0 + (1.0 - 1.0 / 298.257223563) * 6378137.0) / 2.0


def vincenty_from_tables(lon0, su1, cu1, lon, su2, cu2, max_iter=200, tol=1e-12):
    """postprocess.geodesic_distance_m, operation for operation, on arrays of pairs with the sines and cosines of
    the reduced latitudes handed in -- what the device reads from its tables.  Returns (metres, iteration at which
    each pair converged or 0, converged)."""
    from seismic_bpmf_amd import postprocess as pp
    f, a = pp.WGS84_F, pp.WGS84_A
    b = (1.0 - f) * a
    lon0, su1, cu1, lon, su2, cu2 = (np.asarray(x, np.float64) for x in (lon0, su1, cu1, lon, su2, cu2))
    big_l = np.deg2rad((lon - lon0 + 180.0) % 360.0 - 180.0)

    def at(lam):
        sl, cl = np.sin(lam), np.cos(lam)
        sin_sig = np.hypot(cu2 * sl, cu1 * su2 - su1 * cu2 * cl)
        cos_sig = su1 * su2 + cu1 * cu2 * cl
        sig = np.arctan2(sin_sig, cos_sig)
        sin_al = np.where(sin_sig > 0.0, cu1 * cu2 * sl / np.where(sin_sig > 0.0, sin_sig, 1.0), 0.0)
        cos2_al = 1.0 - sin_al * sin_al
        cos_2sm = np.where(cos2_al > 0.0, cos_sig - 2.0 * su1 * su2 / np.where(cos2_al > 0.0, cos2_al, 1.0), 0.0)
        return sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm

    lam = big_l.copy()
    done = np.zeros(lam.shape, dtype=bool)
    iters = np.zeros(lam.shape, dtype=np.int64)
    for it in range(max_iter):
        sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
        c = f / 16.0 * cos2_al * (4.0 + f * (4.0 - 3.0 * cos2_al))
        new = big_l + (1.0 - c) * f * sin_al * (
            sig + c * sin_sig * (cos_2sm + c * cos_sig * (-1.0 + 2.0 * cos_2sm * cos_2sm)))
        conv = np.abs(new - lam) < tol
        lam = np.where(done, lam, new)
        iters[conv & ~done] = it + 1
        done = done | conv
        if done.all():
            break
    sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
    usq = cos2_al * (a * a - b * b) / (b * b)
    big_a = 1.0 + usq / 16384.0 * (4096.0 + usq * (-768.0 + usq * (320.0 - 175.0 * usq)))
    big_b = usq / 1024.0 * (256.0 + usq * (-128.0 + usq * (74.0 - 47.0 * usq)))
    d_sig = big_b * sin_sig * (cos_2sm + big_b / 4.0 * (
        cos_sig * (-1.0 + 2.0 * cos_2sm * cos_2sm)
        - big_b / 6.0 * cos_2sm * (-3.0 + 4.0 * sin_sig * sin_sig) * (-3.0 + 4.0 * cos_2sm * cos_2sm)))
    return np.where(done, b * big_a * (sig - d_sig), np.pi * (a + b) / 2.0), iters, done


def vincenty_mpmath(lon0, lat0, lon, lat, digits=50, tol="1e-30", max_iter=20_000):
    """Vincenty's inverse for one pair in `digits`-digit arithmetic, iterated to |d lambda| < tol: metres, or None
    where the iteration does not converge.  The same ellipsoid constants as postprocess (their float64 values)."""
    import mpmath as mp
    from seismic_bpmf_amd import postprocess as pp
    with mp.workdps(digits):
        f, a = mp.mpf(pp.WGS84_F), mp.mpf(pp.WGS84_A)
        b = (1 - f) * a
        u1 = mp.atan((1 - f) * mp.tan(mp.radians(mp.mpf(float(lat0)))))
        u2 = mp.atan((1 - f) * mp.tan(mp.radians(mp.mpf(float(lat)))))
        su1, cu1, su2, cu2 = mp.sin(u1), mp.cos(u1), mp.sin(u2), mp.cos(u2)
        dl = mp.mpf(float(lon)) - mp.mpf(float(lon0)) + 180
        big_l = mp.radians(dl - 360 * mp.floor(dl / 360) - 180)

        def at(lam):
            sl, cl = mp.sin(lam), mp.cos(lam)
            sin_sig = mp.hypot(cu2 * sl, cu1 * su2 - su1 * cu2 * cl)
            cos_sig = su1 * su2 + cu1 * cu2 * cl
            sig = mp.atan2(sin_sig, cos_sig)
            sin_al = cu1 * cu2 * sl / sin_sig if sin_sig > 0 else mp.mpf(0)
            cos2_al = 1 - sin_al * sin_al
            cos_2sm = cos_sig - 2 * su1 * su2 / cos2_al if cos2_al > 0 else mp.mpf(0)
            return sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm

        lam, done = big_l, False
        for _ in range(max_iter):
            sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
            c = f / 16 * cos2_al * (4 + f * (4 - 3 * cos2_al))
            new = big_l + (1 - c) * f * sin_al * (
                sig + c * sin_sig * (cos_2sm + c * cos_sig * (-1 + 2 * cos_2sm * cos_2sm)))
            done = abs(new - lam) < mp.mpf(tol)
            lam = new
            if done:
                break
        if not done:
            return None
        sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
        usq = cos2_al * (a * a - b * b) / (b * b)
        big_a = 1 + usq / 16384 * (4096 + usq * (-768 + usq * (320 - 175 * usq)))
        big_b = usq / 1024 * (256 + usq * (-128 + usq * (74 - 47 * usq)))
        d_sig = big_b * sin_sig * (cos_2sm + big_b / 4 * (
            cos_sig * (-1 + 2 * cos_2sm * cos_2sm)
            - big_b / 6 * cos_2sm * (-3 + 4 * sin_sig * sin_sig) * (-3 + 4 * cos_2sm * cos_2sm)))
        return b * big_a * (sig - d_sig)


# ---------------------------------------------------------------- B / D: temporal streams ---
def temporal_stream(E, N, K, offset, seed, kT, cutoff, clear=1e-4):
    """(maxbeam (E, N) float32 in [1, 2), maxbeam_sources (E, N) int32 in [offset, offset + K), src_idx (E,) the id
    at each row's maximum).  A sample whose float32 Gibbs weight lies within `clear` relative of the cut-off is
    set to 1.0 (far below it), so that the last place of expf cannot move a sample across."""
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    mb = (1.0 + rng.random((E, N), dtype=np.float32)).astype(np.float32)
    for e in range(E):
        top = int(mb[e].argmax())
        w = pp.gibbs_weights(mb[e], kT).astype(np.float64)
        near = np.abs(w - cutoff) <= clear * cutoff
        near[top] = False
        mb[e, near] = 1.0
    ids = (offset + rng.integers(0, K, (E, N))).astype(np.int32)
    src = np.array([ids[e, mb[e].argmax()] for e in range(E)], dtype=np.int64)
    return mb, ids, src
