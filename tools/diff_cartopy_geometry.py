#!/usr/bin/env python3
"""First contact with cartopy: compare the package's two restated definitions with the calls the reference makes.

  postprocess.geodesic_distance_m  against  cartopy.geodesic.Geodesic().inverse(...)[:, 0]     (utils.compute_distances)
  postprocess.mercator_xy          against  cartopy.crs.Mercator(central_longitude, min_latitude, max_latitude)
                                            .transform_points(PlateCarree(), lon, lat)       (compute_dir_errors)

on seeded regional and global points.  Neither comparison has ever been run where the package was written (cartopy is
not installed there): mercator_xy is restated from PROJ's documentation and checked against Snyder's worked example
only.  Prints the largest differences and exits 1 if the geodesic differs by more than 1 mm on pairs that are not nearly
antipodal, or the projection by more than 1e-9 relative + 1 micrometre.

Usage: python tools/diff_cartopy_geometry.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEODESIC_LIMIT_M = 1e-3
MERCATOR_REL, MERCATOR_ABS_M = 1e-9, 1e-6


def points(n, regional, seed):
    rng = np.random.default_rng(seed)
    if regional:
        return rng.uniform(-120.0, -118.0, n), rng.uniform(35.0, 37.0, n)
    return rng.uniform(-180.0, 180.0, n), rng.uniform(-80.0, 80.0, n)


def geodesic_difference(n=2000, seed=1):
    """Largest |definition - cartopy| in metres over regional and global pairs further than 1 degree from antipodal."""
    from cartopy.geodesic import Geodesic
    from seismic_bpmf_amd import postprocess as pp
    worst = 0.0
    for regional in (True, False):
        lon, lat = points(n, regional, seed)
        lon0, lat0 = float(lon[0]), float(lat[0])
        want = np.asarray(Geodesic().inverse(np.array([[lon0, lat0]]), np.stack([lon, lat], axis=1)))[:, 0]
        got = pp.geodesic_distance_m(lon0, lat0, lon, lat, nonconverged="antipodal")
        keep = want < 19.8e6
        worst = max(worst, float(np.abs(got - want)[keep].max()))
    return worst


def mercator_difference(n=2000, seed=2):
    """Largest |definition - cartopy| / (1e-9 |value| + 1 micrometre) over regional and global points."""
    from cartopy import crs
    from seismic_bpmf_amd import postprocess as pp
    worst = 0.0
    for regional in (True, False):
        lon, lat = points(n, regional, seed)
        lon32, lat32 = np.float32(lon), np.float32(lat)
        central = np.mean(lon32)
        proj = crs.Mercator(central_longitude=central, min_latitude=lat32.min(), max_latitude=lat32.max())
        want = proj.transform_points(crs.PlateCarree(), lon32, lat32)
        x, y = pp.mercator_xy(lon32, lat32, central)
        for got, ref in ((x, want[:, 0]), (y, want[:, 1])):
            worst = max(worst, float((np.abs(got - ref) / (MERCATOR_REL * np.abs(ref) + MERCATOR_ABS_M)).max()))
    return worst


def main():
    try:
        import cartopy  # noqa: F401
    except ImportError:
        sys.exit("diff_cartopy_geometry: cartopy is not installed; nothing compared")
    g, m = geodesic_difference(), mercator_difference()
    print(f"geodesic: largest |definition - cartopy| = {g:.3e} m (limit {GEODESIC_LIMIT_M} m)")
    print(f"mercator: largest difference = {m:.3e} of the limit ({MERCATOR_REL} relative + {MERCATOR_ABS_M} m)")
    sys.exit(0 if g <= GEODESIC_LIMIT_M and m <= 1.0 else 1)


if __name__ == "__main__":
    main()
