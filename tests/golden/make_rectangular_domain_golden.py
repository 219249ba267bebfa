#!/usr/bin/env python3
"""Generate tests/golden/rectangular_domain.npz from the REAL reference's Beamformer._rectangular_domain
(BPMF/template_search.py:1232-1267); runs only where the reference tree is (make_goldens.py:import_reference).

The cases (rectangular_domain_cases) are lattices at several latitudes -- mid-latitude, equatorial, southern,
near-polar -- with several `side_km`, among them sides built so that a lattice column or row lands EXACTLY on
the boundary: side = 2 * (|lon[j] - lon0| * dist_per_lon) makes column j fail the strict `<`, and
np.nextafter(side, inf) makes it pass.  Only arrays are stored: the grids, the centre and side of every case and
the reference's mask (bit-packed).

Usage: python tests/golden/make_rectangular_domain_golden.py
"""
import importlib.util
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rectangular_domain.npz")


def lattice(lon_c, lat_c, n_lon, n_lat, n_dep, span_lon, span_lat):
    """(K,) longitudes and latitudes of a regular lattice, depth fastest (every epicentre repeats n_dep times)."""
    lon = np.linspace(lon_c - span_lon / 2.0, lon_c + span_lon / 2.0, n_lon)
    lat = np.linspace(lat_c - span_lat / 2.0, lat_c + span_lat / 2.0, n_lat)
    LON, LAT, _ = np.meshgrid(lon, lat, np.arange(n_dep), indexing="ij")
    return LON.ravel(), LAT.ravel()


def rectangular_domain_grids():
    """The grids of the cases: a list of (longitudes, latitudes)."""
    rng = np.random.default_rng(20261015)
    grids = [lattice(30.3, 40.7, 21, 17, 3, 1.4, 1.1),           # mid-latitude, northern
             lattice(-70.6, -33.4, 19, 23, 2, 1.2, 1.3),         # southern hemisphere, western longitudes
             lattice(101.0, 0.0, 15, 15, 2, 1.0, 1.0),           # astride the equator
             lattice(15.0, 84.5, 25, 13, 2, 9.0, 1.0),           # near-polar: a degree along the parallel is short
             lattice(-140.0, -78.25, 17, 11, 2, 6.0, 1.2)]       # near-polar, southern
    return grids + [(rng.uniform(29.0, 31.0, 4000), rng.uniform(39.5, 41.5, 4000))]     # and a scattered one


def rectangular_domain_cases(grids):
    """Yield (grid index, lon0, lat0, side_km) -- pure NumPy, the same list wherever it runs."""
    rng = np.random.default_rng(20261016)
    for g, (lon, lat) in enumerate(grids):
        K = lon.shape[0]
        centres = [K // 2, 0, K - 1] + rng.integers(0, K, 3).tolist()
        for k0 in centres:
            lon0, lat0 = lon[k0], lat[k0]
            for side in (100.0, 20.0, 5.0, 37.5, 1.0e-3, 1.0e4):
                yield g, lon0, lat0, side
        # sides that put a lattice column (longitude) or row (latitude) exactly on the boundary, and one ulp beyond
        k0 = centres[0]
        lon0, lat0 = lon[k0], lat[k0]
        dist_per_lon = 2.0 * np.pi * (1.0 / 360.0) * 6371.0
        dist_per_lat = 2.0 * np.pi * (1.0 / 360.0) * (6371.0 * np.sin(np.deg2rad(90.0 - lat0)))
        for j in rng.integers(0, K, 6).tolist():
            for side in (2.0 * (np.abs(lon[j] - lon0) * dist_per_lon), 2.0 * (np.abs(lat[j] - lat0) * dist_per_lat)):
                if side > 0.0:
                    yield g, lon0, lat0, float(side)
                    yield g, lon0, lat0, float(np.nextafter(side, np.inf))


def reference_masks(template_search):
    """The reference's own answer to every case."""
    import pandas as pd
    masks = []
    grids = rectangular_domain_grids()
    for g, lon0, lat0, side in rectangular_domain_cases(grids):
        lon, lat = grids[g]
        fake = types.SimpleNamespace(source_coordinates=pd.DataFrame({"longitude": lon, "latitude": lat}))
        masks.append(np.asarray(template_search.Beamformer._rectangular_domain(fake, lon0, lat0, side_km=side)))
    return masks


def main():
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF import template_search
    grids = rectangular_domain_grids()
    out = {}
    for g, (lon, lat) in enumerate(grids):
        out.update({f"longitudes_{g}": lon, f"latitudes_{g}": lat})
    cases = list(rectangular_domain_cases(grids))
    for j, mask in enumerate(reference_masks(template_search)):
        out[f"mask_{j}"] = np.packbits(mask)
    np.savez_compressed(OUT, n_grids=len(grids), grid=np.array([c[0] for c in cases], dtype=np.int64),
                        lon0=np.array([c[1] for c in cases]), lat0=np.array([c[2] for c in cases]),
                        side_km=np.array([c[3] for c in cases]), **out)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
