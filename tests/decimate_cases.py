"""The grid decimation (decimate.find_similar_sources, csrc/decimate.hip) stated in NumPy, the ways a faster kernel
could get it wrong, and the inputs that tell them apart.  Shared by tests/test_decimate_definition.py (CPU),
tests/test_gpu_decimate.py (device) and tests/golden/make_similar_sources_edges_golden.py (the reference's answers).

`definition` restates BPMF/libc.c:find_similar_moveouts (:55-223, "smallest") and find_similar_moveouts2 (:225-387,
"closest") operation for operation:

  * the moveout difference is a float32 subtraction, its square is taken in float64 (`pow(float, 2)`; the square of a
    float32 is exact in float64);
  * "closest": a float32 accumulator, `acc = float32(float64(acc) + d*d)`, over the n_diff first stations of the
    EARLIER source's ranking -- the selection sort of libc.c:389-410 on indexes (first minimum wins, swap-based, so
    not stable: [1, 1, 0] ranks as [2, 1, 0]);
  * "smallest": every square rounded to float32, the n_diff smallest added in ascending order in float32;
  * thr2 = float32(float64(float32(n_diff)) * float64(float32(threshold))**2), the comparison is a strict `<`;
  * a source is in cell (i, j) unless `lon < v_i or lon >= v_{i+1} or lat < w_j or lat >= w_{j+1}`: half-open cells,
    and a NaN coordinate is a member of every cell;
  * first the cells in (i, j) order, each greedy in ascending source index among its members, then all sources;
  * a source already redundant never makes another one redundant.

One earlier source against all its later ones is one vector operation (they are independent); only a row of squares
that holds a NaN is sorted by the reference's own loop, because NumPy orders NaN differently.

`DEFECTS` plants one change each.  `named_cases()` gives every case with the defects it exists to reject;
`random_cases()` is the seeded sweep.  Everything comes from fixed seeds; the few two-source cases that separate two
roundings are found by seeded searches that run at import (`_search`).
"""
import numpy as np

FS_BATCH = 256                                   # csrc/decimate.hip: kept candidates resolved per batch
METHODS = ("closest", "smallest")
DEFECTS = ("no_cell_pass", "closed_upper_edge", "cells_transposed", "le_threshold", "f32_square", "f64_accumulate",
           "thr2_in_float", "ranking_of_later_source", "stable_argsort", "smallest_in_station_order",
           "redundant_knocks_out")
# cases that are degenerate on purpose: the 5 % .. 95 % condition on the redundant share does not apply
DEGENERATE = ("thr0", "thr_big", "nan_threshold", "K1", "K2_redundant", "K2_kept", "rounding_closest_f32_square",
              "rounding_closest_f64_acc", "rounding_smallest_f64_acc", "thr2_rounding", "smallest_add_order")
SEARCH_LIMIT = 100_000
# the method a defect can touch at all (the others leave it bit for bit alone)
DEFECT_METHODS = {d: METHODS for d in DEFECTS}
DEFECT_METHODS.update(f32_square=("closest",), ranking_of_later_source=("closest",), stable_argsort=("closest",),
                      smallest_in_station_order=("smallest",))

# the names of named_cases(), in order: tests parametrise over this without building a case at collection
NAMED = ("rounding_closest_f32_square", "rounding_closest_f64_acc", "rounding_smallest_f64_acc", "thr2_rounding",
         "smallest_add_order", "tie_at_threshold", "tied_ranking", "ranking_asymmetric", "chain_in_batch",
         "chain_across_batches", "chain_shuffled", "chain_in_one_cell", "batch_exact_256", "batch_257",
         "batch_exact_in_cell", "thr0", "thr_big", "cells_change_answer", "on_vertices", "outside_cells",
         "nan_coordinates", "descending_vertices", "one_cell", "many_empty_cells", "S1", "K1", "K2_redundant", "K2_kept",
         "S256_all", "S256_some", "S80", "n_diff_1", "nan_moveouts", "negative_threshold", "nan_threshold",
         "large_offsets", "denormal_differences")

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------- the definition
def selection_argsort(v):
    """libc.c:389-410 on one row: positions swapped, the first minimum wins."""
    idx = list(range(len(v)))
    for i in range(len(v) - 1):
        mn = i
        for j in range(i + 1, len(v)):
            if v[idx[j]] < v[idx[mn]]:
                mn = j
        idx[mn], idx[i] = idx[i], idx[mn]
    return idx


def selection_sort(v):
    """libc.c:421-439 on one row of values (NaN never compares smaller, and nothing is smaller than it)."""
    v = list(v)
    for i in range(len(v) - 1):
        mn = i
        for j in range(i + 1, len(v)):
            if v[j] < v[mn]:
                mn = j
        v[mn], v[i] = v[i], v[mn]
    return v


def rankings(mv, stable=False):
    """(K, S) station ranking of every source: the selection sort, all rows at once (np.argmin takes the first
    minimum, as the loop does); rows with a NaN go through the loop."""
    K, S = mv.shape
    if stable:
        return np.argsort(mv, axis=1, kind="stable")
    idx = np.tile(np.arange(S), (K, 1))
    rows = np.arange(K)
    for i in range(S - 1):
        mn = i + np.argmin(np.take_along_axis(mv, idx[:, i:], axis=1), axis=1)
        tmp = idx[rows, mn].copy()
        idx[rows, mn] = idx[:, i]
        idx[:, i] = tmp
    for k in np.flatnonzero(np.isnan(mv).any(axis=1)):
        idx[k] = selection_argsort(mv[k])
    return idx


def threshold2(threshold, n_diff, defect=None):
    t = f32(threshold)
    if defect == "thr2_in_float":
        return f32(f32(f32(n_diff) * t) * t)
    return f32(f64(f32(n_diff)) * (f64(t) * f64(t)))


def _sums(ma, mb, rank_a, rank_b, n_diff, method, defect):
    """Summed squared difference of one earlier row `ma` against the later rows `mb` (B, S): float32 (B,), or float64
    under the f64_accumulate defect."""
    with np.errstate(all="ignore"):
        if method == "closest":
            if defect == "ranking_of_later_source":
                st = rank_b[:, :n_diff]
                d = ma[st] - np.take_along_axis(mb, st, axis=1)
            else:
                st = rank_a[:n_diff]
                d = ma[st][None, :] - mb[:, st]
            sq = np.ascontiguousarray((d.astype(f64) * d.astype(f64)).T)             # (n_diff, B): rows are stations
            if defect == "f32_square":
                sq = sq.astype(f32).astype(f64)
            if defect == "f64_accumulate":
                acc = np.zeros(len(mb), f64)
                for s in range(n_diff):
                    acc = acc + sq[s]
                return acc
            acc = np.zeros(len(mb), f32)
            for s in range(n_diff):
                acc = (acc.astype(f64) + sq[s]).astype(f32)
            return acc
        d = ma[None, :] - mb
        sq = (d.astype(f64) * d.astype(f64)).astype(f32)
        if defect == "smallest_in_station_order":
            pick = np.sort(np.argsort(sq, axis=1, kind="stable")[:, :n_diff], axis=1)
            use = np.take_along_axis(sq, pick, axis=1)
        else:
            use = np.sort(sq, axis=1)[:, :n_diff]
            for r in np.flatnonzero(np.isnan(sq).any(axis=1)):
                use[r] = selection_sort(sq[r])[:n_diff]
        use = np.ascontiguousarray(use.T)
        acc = np.zeros(len(mb), f64 if defect == "f64_accumulate" else f32)
        for s in range(n_diff):
            acc = acc + use[s]                                     # float32 + float32, or float64 + float32
        return acc


def _greedy(members, mv, rank, red, n_diff, thr2, method, defect):
    for pos, a in enumerate(members[:-1]):
        if red[a] and defect != "redundant_knocks_out":
            continue
        later = members[pos + 1:]
        later = later[~red[later]]
        if later.size == 0:
            continue
        s = _sums(mv[a], mv[later], rank[a] if rank is not None else None,
                  rank[later] if rank is not None else None, n_diff, method, defect)
        with np.errstate(invalid="ignore"):
            close = (s <= thr2) if defect == "le_threshold" else (s < thr2)
        red[later[close]] = True


def definition(moveouts, lon, lat, cell_lon, cell_lat, threshold, n_diff, method, defect=None, global_pass=True):
    """Boolean (K,): the reference's single-threaded answer; `defect` plants one of DEFECTS.  `global_pass=False` stops
    behind the cells (what the second pass starts from)."""
    assert method in METHODS and (defect is None or defect in DEFECTS)
    mv = np.ascontiguousarray(moveouts, dtype=f32)
    K, S = mv.shape
    lon, lat = np.asarray(lon, f32), np.asarray(lat, f32)
    clon, clat = np.asarray(cell_lon, f32), np.asarray(cell_lat, f32)
    n_diff = S if n_diff is None else int(n_diff)
    assert 1 <= n_diff <= S and lon.shape == (K,) and lat.shape == (K,)
    thr2 = threshold2(threshold, n_diff, defect)
    red = np.zeros(K, bool)
    if K < 2:
        return red
    rank = rankings(mv, stable=defect == "stable_argsort") if method == "closest" else None
    if defect != "no_cell_pass":
        n_i, n_j = len(clon) - 1, len(clat) - 1
        if defect == "cells_transposed":
            n_i, n_j = n_j, n_i
        with np.errstate(invalid="ignore"):
            for i in range(min(n_i, len(clon) - 1)):               # a transposed count is cut at the array's end
                for j in range(min(n_j, len(clat) - 1)):
                    if defect == "closed_upper_edge":
                        out = (lon < clon[i]) | (lon > clon[i + 1]) | (lat < clat[j]) | (lat > clat[j + 1])
                    else:
                        out = (lon < clon[i]) | (lon >= clon[i + 1]) | (lat < clat[j]) | (lat >= clat[j + 1])
                    members = np.flatnonzero(~out)
                    if members.size >= 2:
                        _greedy(members, mv, rank, red, n_diff, thr2, method, defect)
    if global_pass:
        _greedy(np.arange(K), mv, rank, red, n_diff, thr2, method, defect)
    return red


# ---------------------------------------------------------------------------------------------------- the cases
NO_CELLS = (np.array([5.0, 6.0, 8.0], f32), np.array([5.0, 7.0], f32))       # no source of [0, 1]^2 lies in one
LON_V = np.array([-0.01, 0.2, 0.5, 1.01], f32)                               # 3 x 5 cells, unequal everywhere
LAT_V = np.array([-0.01, 0.3, 0.4, 0.7, 0.9, 1.01], f32)


def _case(name, reason, mv, lon, lat, clon, clat, thr, n_diff, why=""):
    """`reason`: the defects the case exists to reject.  `why`: one line for a case that is there for the device's own
    seams (batches, sizes, values), which no defect of the definition models; such a case may name no defect."""
    return dict(name=name, reason=tuple(reason), why=why, moveouts=np.ascontiguousarray(mv, dtype=f32),
                lon=np.asarray(lon, f32), lat=np.asarray(lat, f32), cell_lon=np.asarray(clon, f32),
                cell_lat=np.asarray(clat, f32), threshold=float(thr), n_diff=int(n_diff))


def args_of(case):
    return (case["moveouts"], case["lon"], case["lat"], case["cell_lon"], case["cell_lat"], case["threshold"],
            case["n_diff"])


def _ulp_neighbours(t, reach=6):
    t = f32(t)
    out, lo, hi = [t], t, t
    for _ in range(reach):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return out


def _search(seed, defect, method, S, n_diff, scale=3.0):
    """A two-source table and a threshold on which `defect` decides the pair differently: random pairs, and for each
    the float32 thresholds within 6 ulp of sqrt(sum / n_diff).  None when SEARCH_LIMIT candidates hold none."""
    rng = np.random.default_rng(seed)
    tried = 0
    while tried < SEARCH_LIMIT:
        mv = (rng.uniform(0.0, scale, (2, S))).astype(f32)
        rank = rankings(mv) if method == "closest" else None
        ra, rb = (rank[0], rank[1:]) if rank is not None else (None, None)
        good = _sums(mv[0], mv[1:], ra, rb, n_diff, method, None)[0]
        bad = _sums(mv[0], mv[1:], ra, rb, n_diff, method, defect)[0]
        for t in _ulp_neighbours(np.sqrt(f64(good) / n_diff)):
            tried += 1
            if (good < threshold2(t, n_diff)) != (bad < threshold2(t, n_diff, defect)):
                return mv, float(t)
    return None


def _pair_case(name, defect, method, seed, S, n_diff):
    found = _search(seed, defect, method, S, n_diff)
    if found is None:
        return None
    mv, t = found
    return _case(name, [defect], mv, [0.1, 0.2], [0.1, 0.2], LON_V, LAT_V, t, n_diff)


def _hypot_grid(rng, K, S, snap=None, scale=20.0):
    """A smooth travel-time table of K sources in the unit square.  With `snap` the COORDINATES go onto that grid
    (so they meet vertices exactly); the moveouts keep the unsnapped positions, so that sources of one grid point
    are not one clique and the order of the passes still matters."""
    x, y = rng.uniform(0, 1, K), rng.uniform(0, 1, K)
    sta = rng.uniform(0, 1, (S, 2))
    mv = np.hypot(x[:, None] - sta[None, :, 0], y[:, None] - sta[None, :, 1]) * scale
    if snap:
        x, y = np.round(x / snap) * snap, np.round(y / snap) * snap
    return mv.astype(f32), x.astype(f32), y.astype(f32)


def _chain(n, S, thr, order=None):
    """Sources on a line, 0.6 x the distance the threshold allows apart: every station sees the same distance, so a
    source is close to its neighbour (0.6) and not to the one after (1.2), and the greedy answer alternates."""
    pos = np.arange(n, dtype=f64) * 0.6 * thr
    if order is not None:
        pos = pos[order]
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    mv = pos[:, None] * sign[None, :] + np.linspace(0.0, 3.0, S)[None, :]
    return mv.astype(f32)


def _clustered(rng, n_distinct, S, twins):
    """Rows far apart (uniform on [0, 10]^S) and twins: for every (original, after, tag) a copy of distinct row
    `original` plus 1e-3 -- far inside a threshold of 0.05 -- is inserted behind distinct row `after` >= original.
    Returns the rows in final order and the tag of each (None for a distinct row)."""
    base = rng.uniform(0.0, 10.0, (n_distinct, S))
    rows, tags = [], []
    for k in range(n_distinct):
        rows.append(base[k])
        tags.append(None)
        for orig, after, tag in twins:
            if after == k:
                assert orig <= after
                rows.append(base[orig] + 1e-3 * rng.uniform(-1, 1, S))
                tags.append(tag)
    return np.array(rows).astype(f32), tags


def _batch_seam(rng, n_kept_at_global, n_cell_twins, n_far_twins, S=6, last_is_twin=False):
    """The global pass starts with exactly `n_kept_at_global` candidates, the last of them the last source.  "near"
    twins lie in their original's cell (lon 0.1) and are gone after the cell pass; "far" twins lie in another cell
    (lon 0.8) and fall in the global pass, inside the batch.  `last_is_twin`: the last source is a far twin, alone in
    the second batch, of a survivor of the first."""
    n_distinct = n_kept_at_global - n_far_twins - (1 if last_is_twin else 0)
    after = rng.choice(np.arange(1, n_distinct - 1), n_cell_twins + n_far_twins, replace=False)
    twins = [(int(rng.integers(0, k + 1)), int(k), "near") for k in after[:n_cell_twins]]
    far_of = rng.choice(np.arange(4, n_distinct // 2), n_far_twins, replace=False)     # one far twin per original
    twins += [(int(o), int(max(o, k)), "far") for o, k in zip(far_of, after[n_cell_twins:])]
    if last_is_twin:
        twins.append((3, n_distinct - 1, "far"))
    mv, tags = _clustered(rng, n_distinct, S, twins)
    lon = np.array([0.8 if t == "far" else 0.1 for t in tags], f32)
    return mv, lon, np.full(len(mv), 0.5, f32)


_CACHE = {}


def named_cases():
    """Every named case: a dict with name, reason (the defects it exists to reject), moveouts, lon, lat, cell_lon,
    cell_lat, threshold, n_diff.  Built once; treat the arrays as read-only."""
    if "named" in _CACHE:
        return _CACHE["named"]
    cases = []

    def add(*a, **kw):
        cases.append(_case(*a, **kw))

    # ---- roundings: two sources, a threshold between the two candidate sums
    for c in (_pair_case("rounding_closest_f32_square", "f32_square", "closest", 101, 7, 7),
              _pair_case("rounding_closest_f64_acc", "f64_accumulate", "closest", 102, 9, 9),
              _pair_case("rounding_smallest_f64_acc", "f64_accumulate", "smallest", 103, 9, 6),
              _pair_case("thr2_rounding", "thr2_in_float", "closest", 104, 5, 3),
              _pair_case("smallest_add_order", "smallest_in_station_order", "smallest", 105, 8, 5)):
        if c is not None:
            cases.append(c)

    # ---- exactly at the threshold: multiples of 0.5, thr2 = 4 * 0.25 = 1.0; sums of 1.0 stay, 0.75 goes
    rng = np.random.default_rng(201)
    mv = rng.integers(0, 4, (200, 4)) * 0.5
    add("tie_at_threshold", ["le_threshold"], mv, rng.uniform(0, 1, 200), rng.uniform(0, 1, 200), LON_V, LAT_V, 0.5, 4)

    # ---- rankings: ties of the earlier source across rank n_diff; the later source ranks differently
    rng = np.random.default_rng(202)
    mv = rng.integers(0, 3, (150, 6)).astype(f64) + np.where(rng.random((150, 6)) < 0.5, 0.0, 0.6)
    mv[::2] = np.floor(mv[::2])                                              # every other source: ties only
    add("tied_ranking", ["stable_argsort"], mv, rng.uniform(0, 1, 150), rng.uniform(0, 1, 150), LON_V, LAT_V,
        0.55, 3)
    rng = np.random.default_rng(203)
    mv, lon, lat = _hypot_grid(rng, 300, 10)
    add("ranking_asymmetric", ["ranking_of_later_source"], mv, lon, lat, LON_V, LAT_V, 0.35, 4)

    # ---- chains: the answer of a source depends on the whole sequence before it
    thr = 0.25
    in_cell = (np.array([-1.0, 0.5, 2.0], f32), np.array([-1.0, 0.25, 0.5, 2.0], f32))
    add("chain_in_batch", ["redundant_knocks_out"], _chain(200, 5, thr), np.full(200, 0.5), np.full(200, 0.5),
        *NO_CELLS, thr, 5)
    add("chain_across_batches", ["redundant_knocks_out"], _chain(1200, 5, thr), np.full(1200, 0.5),
        np.full(1200, 0.5), *NO_CELLS, thr, 5)
    rng = np.random.default_rng(204)
    add("chain_shuffled", ["redundant_knocks_out"], _chain(1200, 5, thr, rng.permutation(1200)), np.full(1200, 0.5),
        np.full(1200, 0.5), *NO_CELLS, thr, 5)
    # one cell holds the chain (every third source lies outside it, far away in moveout): `sub` is not the identity
    n = 900
    outside = np.arange(n) % 3 == 1
    mv = np.zeros((n, 5), f32)
    mv[~outside] = _chain(int((~outside).sum()), 5, thr)
    mv[outside] = f32(1000.0) + np.arange(outside.sum(), dtype=f32)[:, None] * f32(7.0)
    add("chain_in_one_cell", ["redundant_knocks_out"], mv, np.where(outside, 5.0, 0.0), np.full(n, 0.3), *in_cell,
        thr, 5)

    # ---- batch seams: the first batch of FS_BATCH candidates ends exactly at the last source, or one before it
    rng = np.random.default_rng(205)
    seam_cells = (np.array([0.0, 0.5, 1.0], f32), np.array([0.0, 0.2, 0.6, 1.0], f32))
    mv, lon, lat = _batch_seam(rng, FS_BATCH, 60, 40)
    add("batch_exact_256", [], mv, lon, lat, *seam_cells, 0.05, 6,
        why="device: the first batch of candidates ends exactly at the last source")
    mv, lon, lat = _batch_seam(rng, FS_BATCH + 1, 60, 40, last_is_twin=True)
    add("batch_257", [], mv, lon, lat, *seam_cells, 0.05, 6,
        why="device: one candidate is left for the second batch, a twin of a survivor of the first")
    # inside a cell subset: the cell at lon 0.1 holds FS_BATCH members (twins among them), the rest lies elsewhere
    mv, _ = _clustered(rng, 300, 6, [(int(rng.integers(0, k + 1)), int(k), "twin") for k in
                                      rng.choice(np.arange(1, 299), 100, replace=False)])
    lon = np.full(len(mv), 0.8, f32)
    lon[np.sort(rng.choice(len(mv) - 1, FS_BATCH - 1, replace=False))] = 0.1
    lon[-1] = 0.1
    add("batch_exact_in_cell", [], mv, lon, np.full(len(mv), 0.5), *seam_cells, 0.05, 6,
        why="device: a cell's subset fills exactly one batch, ending at its last member")
    rng = np.random.default_rng(206)
    mv, lon, lat = _hypot_grid(rng, 600, 7)
    mv[1::2] = mv[0::2]                                                      # identical rows: a sum of exactly 0
    add("thr0", ["le_threshold"], mv, lon, lat, LON_V, LAT_V, 0.0, 7)
    add("thr_big", [], mv, lon, lat, LON_V, LAT_V, 1.0e6, 7,
        why="device: source 0 knocks out everything, every later batch is spent")

    # ---- cells: vertex arrays of different length and spacing, on grids dense enough for the cell pass to matter
    rng = np.random.default_rng(207)
    mv, lon, lat = _hypot_grid(rng, 400, 6)
    add("cells_change_answer", ["no_cell_pass", "cells_transposed"], mv, lon, lat, LON_V, LAT_V, 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 400, 6, snap=0.1)
    add("on_vertices", ["closed_upper_edge", "no_cell_pass", "cells_transposed"], mv, lon, lat, np.array([0.0, 0.2, 0.5, 1.0], f32),
        np.array([0.0, 0.3, 0.4, 0.7, 0.9, 1.0], f32), 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 400, 6)
    add("outside_cells", ["no_cell_pass"], mv, lon, lat, np.array([0.2, 0.4, 0.7], f32),
        np.array([0.3, 0.4, 0.55, 0.8], f32), 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 300, 6)
    lon[rng.choice(300, 25, replace=False)] = np.nan
    lat[rng.choice(300, 25, replace=False)] = np.nan
    add("nan_coordinates", ["no_cell_pass", "cells_transposed"], mv, lon, lat, LON_V, LAT_V, 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 400, 6)
    add("descending_vertices", ["no_cell_pass", "cells_transposed"], mv, lon, lat, np.array([0.0, 0.5, 0.3, 1.0], f32),
        np.array([1.0, 0.6, 0.2, 0.5, 0.9], f32), 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 300, 6)
    add("one_cell", ["no_cell_pass"], mv, lon, lat, np.array([0.25, 0.75], f32), np.array([0.1, 0.9], f32), 1.0, 6)
    mv, lon, lat = _hypot_grid(rng, 160, 6)
    add("many_empty_cells", ["no_cell_pass", "cells_transposed"], mv, lon, lat, np.linspace(0.0, 1.0, 13) ** 1.5,
        np.linspace(0.0, 1.0, 10) ** 0.7, 1.0, 6)

    # ---- sizes
    rng = np.random.default_rng(208)
    add("S1", [], rng.uniform(0, 100, (200, 1)), rng.uniform(0, 1, 200), rng.uniform(0, 1, 200), LON_V, LAT_V, 0.2, 1,
        why="one station")
    add("K1", [], rng.uniform(0, 5, (1, 5)), [0.5], [0.5], LON_V, LAT_V, 1.0, 3,
        why="one source: nothing to compare")
    two = rng.uniform(0, 5, (2, 5))
    add("K2_redundant", [], two, [0.3, 0.3], [0.5, 0.5], LON_V, LAT_V, 10.0, 3,
        why="the smallest grid with a pair, close")
    add("K2_kept", [], two, [0.3, 0.3], [0.5, 0.5], LON_V, LAT_V, 0.01, 3,
        why="the smallest grid with a pair, apart")
    mv, lon, lat = _hypot_grid(rng, 300, 256)
    add("S256_all", [], mv, lon, lat, LON_V, LAT_V, 0.6, 256,
        why="the largest station count, all of them summed")
    add("S256_some", ["ranking_of_later_source"], mv, lon, lat, LON_V, LAT_V, 0.3, 17)
    mv, lon, lat = _hypot_grid(rng, 350, 40)                                  # 40 stations x 2 phases
    add("S80", [], np.concatenate([mv, mv * f32(1.73)], axis=1), lon, lat, LON_V, LAT_V, 0.7, 80,
        why="40 stations x 2 phases, the shape of the largest benchmark configuration")
    mv, lon, lat = _hypot_grid(rng, 300, 9)
    add("n_diff_1", ["ranking_of_later_source"], mv, lon, lat, LON_V, LAT_V, 0.15, 1)

    # ---- values
    rng = np.random.default_rng(209)
    mv, lon, lat = _hypot_grid(rng, 300, 6)
    mv[17, 2] = np.nan
    mv[40, :] = np.nan
    mv[5, 4] = np.inf
    mv[90, 1] = np.inf
    mv[91, 1] = np.inf
    mv[120, 0] = -np.inf
    add("nan_moveouts", [], mv, lon, lat, LON_V, LAT_V, 0.45, 4,
        why="NaN and Inf moveouts: a NaN sum is never below the threshold")
    mv, lon, lat = _hypot_grid(rng, 300, 6)
    add("negative_threshold", [], mv, lon, lat, LON_V, LAT_V, -0.45, 6,
        why="the threshold is squared: equals the case at its absolute value")
    add("nan_threshold", [], mv, lon, lat, LON_V, LAT_V, np.nan, 6,
        why="a NaN threshold: nothing is redundant")
    mv, lon, lat = _hypot_grid(rng, 300, 6, scale=2.0)
    add("large_offsets", [], mv.astype(f64) + 1.0e4, lon, lat, LON_V, LAT_V, 0.045, 6,
        why="moveouts near 1e4 s, where the float32 table itself is coarse (1e-3 s)")
    mv, lon, lat = _hypot_grid(rng, 300, 6, scale=2.0)
    add("denormal_differences", [], mv.astype(f64) * 1.0e-20, lon, lat, LON_V, LAT_V, 0.045e-20, 6,
        why="squares near 1e-40: denormal float32 squares, sums and thr2")
    names = [c["name"] for c in cases]
    assert tuple(names) == NAMED, names
    _CACHE["named"] = cases
    return cases


def named_case(name):
    return next(c for c in named_cases() if c["name"] == name)


def big_grid():
    """K = 3000, S = 40 under a threshold that keeps nearly everything: twelve batches, most of them full.  Not a case
    of its own (no recorded answer): the call that leaves a device's working set full of another grid's values."""
    mv, lon, lat = _hypot_grid(np.random.default_rng(31), 3000, 40)
    return _case("big_grid", [], mv, lon, lat, LON_V, LAT_V, 0.08, 10, why="stale working set")


def random_cases(count=60):
    """Seeded grids, K <= 700, S <= 40: independent vertex arrays per axis, coordinates on a 0.1 grid (vertices
    included) on every other one, moveouts rounded on every third one."""
    if ("random", count) in _CACHE:
        return _CACHE[("random", count)]
    cases = []
    for seed in range(count):
        rng = np.random.default_rng(77_000 + seed)
        K = int(rng.choice([2, 3, 40, 255, 256, 257, 300, 511, 513, 700]))
        S = int(rng.integers(1, 41))
        mv, lon, lat = _hypot_grid(rng, K, S, snap=0.1 if seed % 2 else None)
        if seed % 3 == 0:
            mv = np.round(mv * 4) / 4
        clon = np.sort(np.round(rng.uniform(-0.1, 1.1, int(rng.integers(2, 7))), 1))
        clat = np.sort(np.round(rng.uniform(-0.1, 1.1, int(rng.integers(2, 9))), 1))
        nd = int(rng.integers(1, S + 1))
        thr = float(f32(rng.uniform(0.1, 0.9) * (0.25 + 0.75 * nd / S)))
        cases.append(_case(f"random_{seed}", [], mv, lon, lat, clon, clat, thr, nd))
    _CACHE[("random", count)] = cases
    return cases
