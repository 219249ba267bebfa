"""CPU, skipped until cartopy is importable: the two definitions that stand in for cartopy's calls in the pair geometry
-- postprocess.geodesic_distance_m for Geodesic().inverse and postprocess.mercator_xy for crs.Mercator -- against cartopy
itself (tools/diff_cartopy_geometry.py).  Until this has run somewhere, mercator_xy is restated from PROJ's documentation
and verified against Snyder's worked example only (tests/test_template_geometry_definition.py)."""
import os
import sys

import pytest

pytest.importorskip("cartopy")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import diff_cartopy_geometry as dcg  # noqa: E402


def test_geodesic_equals_cartopy_to_a_millimetre():
    assert dcg.geodesic_difference() <= dcg.GEODESIC_LIMIT_M


def test_mercator_equals_cartopy():
    assert dcg.mercator_difference() <= 1.0
