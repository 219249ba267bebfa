#!/usr/bin/env python3
"""Generate tests/golden/multiples.npz from the REAL reference's TemplateGroup.remove_multiples
(BPMF/dataset.py:5130-5295); runs only where the reference tree is (make_goldens.py:import_reference).

The method is called unbound on a namespace object that carries what it reads: `catalog.catalog` (a DataFrame with
origin_time, tid, cc), `ellipsoid_dist`, `intertemplate_cc` / `_intertemplate_cc` (DataFrames indexed by template id),
`tids`, `tindexes` and `templates[k].catalog.catalog`.  The cases (reference_cases) cover every combination of
similarity_criterion in {-1, 0.1, 0.5}, distance_criterion in {1, 15} and dt_criterion in {0.5, 4, 9}, twice: template
ids that are not contiguous, matrices that are not symmetric, origin times in clusters and PAIRWISE DISTINCT at the
millisecond the reference rounds them to (on equal times the reference's own answer depends on the platform's
quicksort).  Only arrays are stored: the inputs of every case and the reference's `unique_event` in input order.

Usage: python tests/golden/make_multiples_golden.py
"""
import importlib.util
import itertools
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "multiples.npz")
EPOCH_MS = 1343260800000          # 2012-07-26T00:00:00 in ms: seconds near 1.3e9, where 1 ms is not a float64
CRITERIA = list(itertools.product((-1.0, 0.1, 0.5), (1.0, 15.0), (0.5, 4.0, 9.0)))


def reference_case(rng, n, n_templates, similarity_criterion, distance_criterion, dt_criterion):
    """One case as a dict of arrays -- pure NumPy, the same wherever it runs."""
    tids = np.sort(rng.choice(np.arange(3, 400), size=n_templates, replace=False)).astype(np.int64)
    # distances: a third of the pairs under 1 km, a third under 15 km, the rest beyond; nothing symmetric
    dist = np.where(rng.random((n_templates, n_templates)) < 0.35, rng.uniform(0.0, 1.0, (n_templates, n_templates)),
                    rng.uniform(1.0, 30.0, (n_templates, n_templates)))
    sim = rng.uniform(-0.2, 1.0, (n_templates, n_templates))
    np.fill_diagonal(dist, 0.0)
    np.fill_diagonal(sim, 1.0)
    # clustered origin times, pairwise distinct milliseconds: a cluster every ~20 s, events within ~dt of its centre
    n_clusters = max(1, n // 6)
    centres = rng.uniform(0.0, 20.0 * n_clusters, n_clusters)
    ms = set()
    while len(ms) < n:
        t = centres[rng.integers(n_clusters)] + rng.exponential(0.6 * dt_criterion)
        ms.add(int(round(1000.0 * t)))
    ms = rng.permutation(np.array(sorted(ms), dtype=np.int64)) + EPOCH_MS          # input order is not time order
    return {"origin_time_ms": ms, "event_tids": tids[rng.integers(0, n_templates, n)],
            "cc": rng.uniform(0.1, 1.0, n).astype(np.float32), "tids": tids, "ellipsoid_dist": dist,
            "intertemplate_cc": sim, "similarity_criterion": np.float64(similarity_criterion),
            "distance_criterion": np.float64(distance_criterion), "dt_criterion": np.float64(dt_criterion)}


def reference_cases(seed=20261018, repeats=2, n_max=400):
    """The cases of the file: every combination of the criteria `repeats` times, one small and one large catalog."""
    rng = np.random.default_rng(seed)
    cases = []
    for rep in range(repeats):
        for sim_c, dist_c, dt_c in CRITERIA:
            n = int(rng.integers(2, 60)) if rep == 0 else int(rng.integers(150, n_max + 1))
            cases.append(reference_case(rng, n, int(rng.integers(2, 12)), sim_c, dist_c, dt_c))
    return cases


def origin_time_sec(case):
    """The float64 seconds the reference derives from its datetime64[ms] origin times (BPMF/dataset.py:5179-5184)."""
    return case["origin_time_ms"].astype("datetime64[ms]").astype("float64") / 1000.0


def mirror_arguments(case, pp):
    """(origin_time_sec, template_rows, cc, pair_ok, dt_criterion) of postprocess.flag_multiples for a case."""
    pair_ok = pp.multiples_pair_mask(case["ellipsoid_dist"], float(case["distance_criterion"]),
                                     case["intertemplate_cc"], float(case["similarity_criterion"]))
    return (origin_time_sec(case), np.searchsorted(case["tids"], case["event_tids"]), case["cc"], pair_ok,
            float(case["dt_criterion"]))


def reference_unique_event(dataset, case):
    """The reference's own answer to a case, in input order; also checks what it writes into the templates' catalogs."""
    import contextlib
    import io
    import pandas as pd
    tids = case["tids"]
    n = len(case["cc"])
    catalog = pd.DataFrame({"origin_time": case["origin_time_ms"].astype("datetime64[ms]"), "tid": case["event_tids"],
                            "cc": case["cc"]}, index=np.arange(n))
    templates = [types.SimpleNamespace(catalog=types.SimpleNamespace(catalog=catalog[catalog["tid"] == tid].copy()))
                 for tid in tids]
    sim = pd.DataFrame(case["intertemplate_cc"], index=tids, columns=tids)
    group = types.SimpleNamespace(catalog=types.SimpleNamespace(catalog=catalog), tids=tids, templates=templates,
                                  tindexes=pd.Series(index=tids, data=np.arange(len(tids))),
                                  ellipsoid_dist=pd.DataFrame(case["ellipsoid_dist"], index=tids, columns=tids),
                                  intertemplate_cc=sim, _intertemplate_cc=sim)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset.TemplateGroup.remove_multiples(group, dt_criterion=float(case["dt_criterion"]),
                                               distance_criterion=float(case["distance_criterion"]),
                                               similarity_criterion=float(case["similarity_criterion"]))
    unique = group.catalog.catalog["unique_event"].sort_index().values.astype(bool)
    for tid, tp in zip(tids, templates):
        assert np.array_equal(tp.catalog.catalog["unique_event"].values.astype(bool), unique[case["event_tids"] == tid])
    return unique


def main():
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF import dataset
    cases = reference_cases()
    out, flagged = {"n_cases": len(cases)}, 0
    for j, case in enumerate(cases):
        unique = reference_unique_event(dataset, case)
        assert (~unique).sum() >= 1, f"case {j} flags nothing"
        assert len(np.unique(case["origin_time_ms"])) == len(unique)
        flagged += int((~unique).sum())
        out.update({f"{k}_{j}": v for k, v in case.items()})
        out[f"unique_event_{j}"] = np.packbits(unique)
    assert flagged >= 1000, flagged
    assert {(float(c["similarity_criterion"]), float(c["distance_criterion"]), float(c["dt_criterion"]))
            for c in cases} == set(CRITERIA)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} cases, {sum(len(c['cc']) for c in cases)} events, {flagged} flagged, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
