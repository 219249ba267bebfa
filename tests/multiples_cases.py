"""The cases of the multiples flagging (postprocess.flag_multiples, workflow.flag_multiples) shared by the host and
the GPU tests, and `definition`: the definition restated with one switch per way of getting it wrong.  Every case is
(name, origin_time_sec, template_rows, cc, pair_ok, dt_criterion); test_multiples_host.py checks that the named cases
are SHARP -- each planted variant changes the result of at least one of them."""
import numpy as np

VARIANTS = ("direct_difference", "less_equal", "last_maximum", "reversed_ties", "visit_flagged", "keep_flagged",
            "transposed", "no_keeper", "window_64")


def definition(t, rows, cc, pair_ok, dt, variant=None):
    """The issue's definition, line by line; `variant` plants one deviation (VARIANTS)."""
    t, rows, cc = np.asarray(t, np.float64), np.asarray(rows), np.asarray(cc, np.float32)
    n = len(t)
    if variant == "reversed_ties":
        order = (n - 1 - np.argsort(t[::-1], kind="stable"))          # stable, but LAST of the equals first
    else:
        order = np.argsort(t, kind="stable")
    ts, r, c = t[order], rows[order], cc[order]
    ie = np.zeros(n)
    ie[1:] = ts[1:] - ts[:-1]
    unique = np.ones(n, bool)
    for n1 in range(n):
        if not unique[n1] and variant != "visit_flagged":
            continue
        neighbours, acc, n2 = [n1], 0.0, n1 + 1
        while n2 < n:
            acc = acc + ie[n2] if n2 > n1 + 1 else ie[n2]
            span = ts[n2] - ts[n1] if variant == "direct_difference" else acc
            if not (span <= dt if variant == "less_equal" else span < dt):
                break
            neighbours.append(n2)
            n2 += 1
        if variant == "window_64":
            neighbours = neighbours[:64]
        candidates = [m for m in neighbours if unique[m] or variant == "keep_flagged"]
        if variant == "transposed":
            multiples = [m for m in candidates if pair_ok[r[m], r[n1]]]
        else:
            multiples = [m for m in candidates if pair_ok[r[n1], r[m]]]
        if len(multiples) >= 2:
            unique[multiples] = False
            values = c[multiples]
            best = len(values) - 1 - int(np.argmax(values[::-1])) if variant == "last_maximum" else int(np.argmax(values))
            if variant != "no_keeper":
                unique[multiples[best]] = True
    out = np.empty(n, bool)
    out[order] = unique
    return out


def _all_ok(T):
    return np.ones((T, T), bool)


def _case(name, t, rows, cc, pair_ok, dt):
    return (name, np.asarray(t, np.float64), np.asarray(rows, np.int64), np.asarray(cc, np.float32),
            np.asarray(pair_ok, bool), float(dt))


# Two triples found by a CPU search (test_multiples_host.py repeats the check): with ie = differences of neighbours,
# ie[1] + ie[2] and t[2] - t[0] are different float64 numbers and dt_criterion is the larger of the two, so that one of
# them is < dt_criterion and the other is not.
def split_triples(count=2, seed=7):
    """[(t (3,), dt, sum_is_smaller)]: one triple where the accumulated sum is the smaller number, one where the direct
    difference is."""
    rng = np.random.default_rng(seed)
    found = {}
    for _ in range(10000):
        t = np.cumsum(rng.uniform(0.1, 2.0, 3))
        acc, direct = (t[1] - t[0]) + (t[2] - t[1]), t[2] - t[0]
        if acc != direct and (acc < direct) not in found:
            found[acc < direct] = (t, max(acc, direct), bool(acc < direct))
        if len(found) == count:
            return [found[True], found[False]]
    raise AssertionError("no triple found")


def named_cases():
    rng = np.random.default_rng(20261018)
    cases = [_case("n0", [], [], [], _all_ok(2), 4.0),
             _case("n1", [5.0], [1], [0.5], _all_ok(2), 4.0),
             _case("n2_multiples", [5.0, 6.0], [0, 1], [0.5, 0.7], _all_ok(2), 4.0),
             _case("n2_apart", [5.0, 9.5], [0, 1], [0.5, 0.7], _all_ok(2), 4.0)]
    # all events in one segment (gaps of 1 s, dt 4 s), input order shuffled
    n = 300
    cases.append(_case("one_segment", rng.permutation(np.arange(n) * 1.0 + 0.25 * rng.random(n)), rng.integers(0, 6, n),
                       rng.random(n), rng.random((6, 6)) < 0.6, 4.0))
    # every event its own segment
    cases.append(_case("own_segments", rng.permutation(np.arange(200) * 4.0), rng.integers(0, 3, 200), rng.random(200),
                       _all_ok(3), 4.0))
    # windows of exactly 63, 64, 65 and 130 neighbours (n1 included) behind a first event, every event a multiple of
    # it, twice: the keeper is the first event (a window cut short leaves the events behind the cut unique), then the
    # last one
    for k in (63, 64, 65, 130):
        t = np.concatenate([np.linspace(0.0, 3.9, k), 100.0 + np.linspace(0.0, 3.9, k)])
        cc = np.concatenate([np.linspace(0.9, 0.1, k), np.linspace(0.1, 0.9, k)])
        cases.append(_case(f"neighbours_{k}", t, np.zeros(2 * k, int), cc, _all_ok(1), 4.0))
    # a sliding chain: A flags B; B is then skipped as n1 (visited, it would make multiples of C and D, which are none
    # for each other) and X, between them, must not see B among its candidates (B would win against X)
    ok = np.eye(6, dtype=bool)
    for a, b in ((0, 2), (2, 3), (2, 4), (1, 2)):
        ok[a, b] = ok[b, a] = True
    cases.append(_case("sliding_chain", [0.0, 1.0, 3.0, 5.0, 6.5], [0, 1, 2, 3, 4], [0.9, 0.2, 0.8, 0.5, 0.4], ok, 4.0))
    # time ties: multiples of 0.5 s, three templates that are not transitive (0~1, 1~2, not 0~2), input order random
    ok3 = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]], bool)
    n = 240
    cases.append(_case("time_ties", rng.integers(0, 160, n) * 0.5, rng.integers(0, 3, n), rng.random(n), ok3, 1.0))
    cases.append(_case("time_ties_minimal", [1.0, 1.0, 1.0], [0, 1, 2], [0.5, 0.6, 0.7], ok3, 1.0))
    # cc ties: few distinct values, among them -0.0 and 0.0
    n = 200
    cases.append(_case("cc_ties", np.sort(rng.random(n) * 150.0), rng.integers(0, 4, n),
                       rng.choice(np.array([-0.0, 0.0, 0.25, 0.5], np.float32), n), rng.random((4, 4)) < 0.7, 4.0))
    cases.append(_case("cc_ties_minimal", [0.0, 1.0, 2.0], [0, 0, 0], [0.5, 0.5, 0.5], _all_ok(1), 4.0))
    # a keeper that is not n1
    cases.append(_case("keeper_not_n1", [0.0, 1.0, 2.0, 10.0], [0, 1, 0, 1], [0.3, 0.9, 0.5, 0.1], _all_ok(2), 4.0))
    # a window that closes exactly at dt_criterion: times in exact halves, dt 4.0 -- 4.0 < 4.0 is False
    cases.append(_case("closes_at_dt", [0.0, 2.5, 4.0, 8.0, 12.0, 15.5], [0, 0, 0, 0, 0, 0],
                       [0.1, 0.2, 0.9, 0.3, 0.4, 0.5], _all_ok(1), 4.0))
    # accumulated sum and direct difference on opposite sides of dt_criterion
    for t, dt, sum_smaller in split_triples():
        cases.append(_case(f"split_triple_sum_{'smaller' if sum_smaller else 'larger'}", t, [0, 0, 0], [0.9, 0.5, 0.2],
                           _all_ok(1), dt))
    # an asymmetric pair_ok: the row is the template of n1
    ok = np.array([[1, 1], [0, 1]], bool)
    cases.append(_case("asymmetric", [0.0, 1.0, 10.0, 11.0], [0, 1, 1, 0], [0.9, 0.5, 0.9, 0.5], ok, 4.0))
    # a diagonal that is False: n1 itself is no multiple, two others are
    ok = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], bool)
    cases.append(_case("false_diagonal", [0.0, 1.0, 2.0, 20.0, 21.0], [0, 1, 2, 0, 0], [0.9, 0.5, 0.7, 0.5, 0.6], ok, 4.0))
    # T = 1
    cases.append(_case("one_template", np.sort(rng.random(50) * 60.0), np.zeros(50, int), rng.random(50), _all_ok(1), 4.0))
    return cases


def random_cases(count=200, seed=20261019):
    """Seeded random catalogs, n <= 2000 and T <= 40, clustered times (some on a 0.5 s lattice: ties), pair_ok from
    random matrices through postprocess.multiples_pair_mask with every criterion of the reference fixtures."""
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    cases = []
    for j in range(count):
        n = int(rng.choice([rng.integers(2, 40), rng.integers(40, 400), rng.integers(400, 2001)]))
        T = int(rng.integers(1, 41))
        dt = float(rng.choice([0.5, 4.0, 9.0]))
        dist = np.where(rng.random((T, T)) < 0.4, rng.uniform(0.0, 1.0, (T, T)), rng.uniform(1.0, 30.0, (T, T)))
        sim = rng.uniform(-0.2, 1.0, (T, T))
        ok = pp.multiples_pair_mask(dist, float(rng.choice([1.0, 15.0])), sim, float(rng.choice([-1.0, 0.1, 0.5])))
        n_clusters = max(1, n // int(rng.choice([3, 10, 80])))
        centres = rng.uniform(0.0, 15.0 * n_clusters, n_clusters)
        t = centres[rng.integers(0, n_clusters, n)] + rng.exponential(0.7 * dt, n)
        if j % 4 == 0:
            t = np.round(t * 2.0) / 2.0
        cc = rng.random(n).astype(np.float32)
        if j % 5 == 0:
            cc = np.round(cc, 1)
        cases.append(_case(f"random_{j}", t, rng.integers(0, T, n), cc, ok, dt))
    return cases
