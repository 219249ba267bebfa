#!/usr/bin/env python3
"""Generate tests/golden/template_geometry.npz from the REAL reference's utils.compute_distances,
TemplateGroup.compute_intertemplate_dist, compute_dir_errors, compute_ellipsoid_dist and the weight loop of
compute_intertemplate_cc (BPMF/utils.py:1419-1498, BPMF/dataset.py:4568-4688, :4787-4816); runs only where the
reference tree is (make_goldens.py:import_reference).

The methods are called unbound on namespace objects that carry what they read.  cartopy is not installed where this
runs: sys.modules carries stubs for `cartopy.geodesic` and `cartopy.crs` backed by the package's own two definitions
(postprocess.geodesic_distance_m and postprocess.mercator_xy), and one for `fast_matched_filter` that records the
weights it is handed.  The fixture therefore pins everything of the reference EXCEPT the two cartopy calls: pandas'
indexing, the column-versus-row read of ellipsoid_dist, BLAS's dot, every rounding and dtype.  Only arrays are stored.

Three groups of 2 .. 12 templates with template ids that are not contiguous, mixed cov_mat, and station distances
without ties (on equal distances the reference's answer depends on the platform's quicksort).

Usage: python tests/golden/make_template_geometry_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "template_geometry.npz")
GROUPS = ((2, 5, 3, 3), (7, 9, 3, 4), (12, 14, 3, 10))      # templates, stations, channels, n_stations
DISTANCE_THRESHOLDS = (-20.0, 5.0)                           # for the weight loop (ellipsoid_dist is mostly negative)


def group_case(rng, T, S, C):
    """One group as a dict of arrays -- pure NumPy, the same wherever it runs."""
    tids = np.sort(rng.choice(np.arange(3, 400), size=T, replace=False)).astype(np.int64)
    a = rng.normal(0.0, 1.5, (T, 3, 3))
    has_cov = rng.random(T) < 0.7
    has_cov[0], has_cov[-1] = True, False
    avail_cha = rng.random((T, S, C)) < 0.8
    avail = avail_cha.any(axis=2) & (rng.random((T, S)) < 0.8)
    avail[0] = False                                         # fewer available stations than n_stations: filled up
    avail[0, :2] = True
    return {"tids": tids, "longitude": rng.uniform(-119.5, -118.5, T), "latitude": rng.uniform(35.5, 36.5, T),
            "depth": rng.uniform(1.0, 25.0, T), "cov_mat": a @ a.transpose(0, 2, 1), "has_cov": has_cov,
            "station_longitude": rng.uniform(-120.0, -118.0, S), "station_latitude": rng.uniform(35.0, 37.0, S),
            "station_depth": rng.uniform(-3.0, 0.0, S), "availability": avail, "availability_per_cha": avail_cha}


def cases(seed=20261021):
    rng = np.random.default_rng(seed)
    return [group_case(rng, T, S, C) for T, S, C, _ in GROUPS]


def install_stubs(pp):
    """cartopy.geodesic / cartopy.crs backed by the two definitions; fast_matched_filter as a recorder."""
    class Geodesic:
        def inverse(self, points, endpoints):
            points, endpoints = np.asarray(points, np.float64), np.asarray(endpoints, np.float64)
            d = pp.geodesic_distance_m(points[0, 0], points[0, 1], endpoints[:, 0], endpoints[:, 1])
            return np.stack([d, np.zeros_like(d), np.zeros_like(d)], axis=1)

    class PlateCarree:
        pass

    class Mercator:
        def __init__(self, central_longitude=0.0, min_latitude=-80.0, max_latitude=84.0):
            self.central_longitude = central_longitude

        def transform_points(self, src_crs, x, y):
            X, Y = pp.mercator_xy(x, y, self.central_longitude)
            return np.stack([X, Y, np.zeros_like(X)], axis=1)

    recorded = []

    def matched_filter(templates, moveouts, weights, data, step, **kwargs):
        recorded.append((templates[:, 0, 0, 0].astype(np.int64), np.array(weights, copy=True)))
        return np.zeros((templates.shape[0], 3) + templates.shape[1:3], np.float32)

    cartopy = types.ModuleType("cartopy")
    cartopy.geodesic = types.ModuleType("cartopy.geodesic")
    cartopy.geodesic.Geodesic = Geodesic
    cartopy.crs = types.ModuleType("cartopy.crs")
    cartopy.crs.PlateCarree, cartopy.crs.Mercator = PlateCarree, Mercator
    fmf = types.ModuleType("fast_matched_filter")
    fmf.matched_filter = matched_filter
    sys.modules.update({"cartopy": cartopy, "cartopy.geodesic": cartopy.geodesic, "cartopy.crs": cartopy.crs,
                        "fast_matched_filter": fmf})
    return recorded


def reference_group(dataset, utils, case, n_stations, recorded):
    import pandas as pd
    T, S, C = case["availability_per_cha"].shape
    stations = np.array([f"ST{k:02d}" for k in range(S)])
    # source-receiver distances of every template, float64 depths as a network file holds them
    srd, srd_epi = utils.compute_distances(case["longitude"], case["latitude"], case["depth"], case["station_longitude"],
                                           case["station_latitude"], case["station_depth"],
                                           return_epicentral_distances=True)
    templates = []
    for t in range(T):
        tp = types.SimpleNamespace(longitude=case["longitude"][t], latitude=case["latitude"][t], depth=case["depth"][t],
                                   where="nowhere/template.h5", network_stations=stations,
                                   availability=pd.Series(case["availability"][t], index=stations),
                                   source_receiver_dist=pd.Series(srd[t], index=stations),
                                   availability_per_cha=pd.DataFrame(case["availability_per_cha"][t], index=stations))
        if case["has_cov"][t]:
            tp.cov_mat = case["cov_mat"][t]
        templates.append(tp)
    group = types.SimpleNamespace(templates=templates, tids=case["tids"], n_templates=T)
    out = {"source_receiver_dist": srd, "source_receiver_epicentral": srd_epi}
    with contextlib.redirect_stdout(io.StringIO()):
        dataset.TemplateGroup.compute_intertemplate_dist(group)
        group.intertemplate_dist = group._intertemplate_dist
        dataset.TemplateGroup.compute_dir_errors(group)
        group.dir_errors = group._dir_errors
        dataset.TemplateGroup.compute_ellipsoid_dist(group)
        group.ellipsoid_dist = group._ellipsoid_dist
        for key in ("intertemplate_dist", "dir_errors", "ellipsoid_dist"):
            out[key] = getattr(group, key).values
            assert out[key].dtype == np.float32, (key, out[key].dtype)
        # waveforms whose first sample names the template: the recorder learns which rows `keep` kept
        group.waveforms_arr = np.broadcast_to(np.arange(T, dtype=np.float32)[:, None, None, None], (T, S, C, 8)).copy()
        for j, threshold in enumerate(DISTANCE_THRESHOLDS):
            del recorded[:]
            dataset.TemplateGroup.compute_intertemplate_cc(group, distance_threshold=threshold, n_stations=n_stations,
                                                           max_lag=2, compute_from_scratch=True)
            assert len(recorded) == T
            weights = np.zeros((T, T, S, C), np.float32)
            for t, (kept, w) in enumerate(recorded):
                weights[t, kept] = w
            out[f"weights_{j}"] = weights
    return out


def main():
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    sys.path.insert(0, mg.ROOT)
    from seismic_bpmf_amd import postprocess as pp
    recorded = install_stubs(pp)
    mg.import_reference()
    from BPMF import dataset, utils
    out = {"n_groups": len(GROUPS), "distance_thresholds": np.array(DISTANCE_THRESHOLDS)}
    for g, (case, (_, _, _, n_stations)) in enumerate(zip(cases(), GROUPS)):
        ref = reference_group(dataset, utils, case, n_stations, recorded)
        d = ref["source_receiver_dist"]
        assert all(len(np.unique(row)) == len(row) for row in d), "tied station distances"
        assert any((ref[f"weights_{j}"] != 0).reshape(len(d), len(d), -1).any(axis=2).sum() not in (0, len(d) ** 2)
                   for j in range(len(DISTANCE_THRESHOLDS))), "every threshold keeps all pairs or none"
        out.update({f"{k}_{g}": v for k, v in case.items()})
        out.update({f"{k}_{g}": v for k, v in ref.items()})
        out[f"n_stations_{g}"] = n_stations
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(GROUPS)} groups, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
