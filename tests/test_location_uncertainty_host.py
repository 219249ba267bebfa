"""CPU: the host side of the batched location uncertainties -- postprocess.rectangular_domain against the
reference's own Beamformer._rectangular_domain (tests/golden/rectangular_domain.npz, written by
tests/golden/make_rectangular_domain_golden.py; with BPMF_RECORD_REFERENCE=<reference source tree> the reference is
imported and asked again, live), the per-source table of its latitude scale, workflow.location_uncertainties_host
against direct calls of the pinned pieces, and the argument checks that must not need a device."""
import importlib.util
import os
import types
from unittest.mock import MagicMock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rectangular_domain.npz")
RECORD = os.environ.get("BPMF_RECORD_REFERENCE")


def load_generator():
    spec = importlib.util.spec_from_file_location(
        "make_rectangular_domain_golden", os.path.join(HERE, "golden", "make_rectangular_domain_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def stored_cases():
    """[(longitudes, latitudes, lon0, lat0, side_km, mask)] of the fixture."""
    z = np.load(GOLDEN)
    out = []
    for j, g in enumerate(z["grid"]):
        lon, lat = z[f"longitudes_{g}"], z[f"latitudes_{g}"]
        mask = np.unpackbits(z[f"mask_{j}"])[:lon.shape[0]].astype(bool)
        out.append((lon, lat, z["lon0"][j], z["lat0"][j], float(z["side_km"][j]), mask))
    return out


def test_rectangular_domain_equals_the_reference_fixture():
    from seismic_bpmf_amd import postprocess as pp
    cases = stored_cases()
    assert len(cases) >= 300
    sizes = set()
    for j, (lon, lat, lon0, lat0, side, want) in enumerate(cases):
        got = pp.rectangular_domain(lon0, lat0, lon, lat, side_km=side)
        assert got.dtype == bool and got.shape == lon.shape
        assert np.array_equal(got, want), (j, side, int(got.sum()), int(want.sum()))
        sizes.add((int(want.sum()), lon.shape[0]))
    # the centre's own epicentre alone, partial and whole-grid domains are all there
    assert min(n for n, _ in sizes) <= 3 and any(n == K for n, K in sizes) and len(sizes) > 20
    assert any(lat.min() < -30 for _, lat, *_ in cases) and any(np.abs(lat).max() > 80 for _, lat, *_ in cases)


def test_fixture_holds_the_cases_its_generator_states_with_columns_on_the_boundary():
    """The fixture's inputs are the generator's (pure NumPy, no reference needed), and the on-boundary sides do
    what they were built for: the side fails the strict `<` for its column or row, its nextafter passes."""
    gen = load_generator()
    grids = gen.rectangular_domain_grids()
    cases = list(gen.rectangular_domain_cases(grids))
    stored = stored_cases()
    assert len(cases) == len(stored)
    flips = 0
    for (g, lon0, lat0, side), (lon, lat, slon0, slat0, sside, _) in zip(cases, stored):
        assert np.array_equal(grids[g][0], lon) and np.array_equal(grids[g][1], lat)
        assert (lon0, lat0, side) == (slon0, slat0, sside)
    for a, b in zip(stored[:-1], stored[1:]):
        if b[4] == np.nextafter(a[4], np.inf) and np.array_equal(a[0], b[0]):
            assert not (a[5] & ~b[5]).any()                                  # a larger side loses nobody
            flips += int((b[5] & ~a[5]).sum() > 0)
    assert flips >= 20                                    # sources exactly on the boundary: out at side, in one ulp on


@pytest.fixture(scope="module")
def live_masks():
    """None -- or, with BPMF_RECORD_REFERENCE=<reference source tree>, the masks the imported reference gives for
    the generator's cases now (the live twin, as tests/test_reference_live.py has them)."""
    if not RECORD:
        yield None
        return
    import sys
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "golden", "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.REF = RECORD
    cwd, path0, mods0 = os.getcwd(), list(sys.path), set(sys.modules)
    try:
        mg.import_reference()                        # chdir()s into a scratch directory
    finally:
        os.chdir(cwd)
    from BPMF import template_search
    yield load_generator().reference_masks(template_search)
    for name in set(sys.modules) - mods0:
        if isinstance(sys.modules[name], MagicMock) or name == "BPMF" or name.startswith("BPMF."):
            del sys.modules[name]
    sys.path[:] = path0


def test_live_reference_gives_the_fixture_masks(live_masks):
    """With the reference tree present: its answers now are the fixture's, and rectangular_domain's.  Without it
    the recorded answers stand in, as in tests/test_reference_live.py."""
    from seismic_bpmf_amd import postprocess as pp
    stored = stored_cases()
    answers = live_masks if live_masks is not None else [c[5] for c in stored]
    assert len(answers) == len(stored)
    for j, ((lon, lat, lon0, lat0, side, kept), want) in enumerate(zip(stored, answers)):
        assert np.array_equal(kept, want), j
        assert np.array_equal(pp.rectangular_domain(lon0, lat0, lon, lat, side_km=side), want), j


def test_domain_scale_table_equals_the_scalar_of_the_function():
    """table[k] must be bit-equal to the dist_per_lat the reference's expression gives for the scalar
    lat0 = latitudes[k] (NumPy's vector and scalar sin are asserted equal here, not assumed)."""
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(7)
    lat = np.concatenate([rng.uniform(-90.0, 90.0, 20_000), [0.0, 90.0, -90.0, 45.0, -33.4, 84.5]])
    table = pp.domain_scale_per_latitude(lat)
    assert table.dtype == np.float64 and table.shape == lat.shape
    for k in range(lat.shape[0]):
        lat0 = lat[k]                                             # np.float64 scalar, as .iloc[] hands it out
        Rlat = 6371.0 * np.sin(np.deg2rad(90.0 - lat0))
        assert table[k] == 2.0 * np.pi * (1.0 / 360.0) * Rlat, k
    assert pp.domain_scale_per_longitude() == 2.0 * np.pi * (1.0 / 360.0) * 6371.0
    # the table in use: the mask from the table's value is the function's mask
    lon = rng.uniform(10.0, 12.0, lat.shape[0])
    lat = rng.uniform(-41.0, -39.0, lat.shape[0])
    table = pp.domain_scale_per_latitude(lat)
    for k in (0, 17, 4000):
        mask = (np.abs(lon - lon[k]) * pp.domain_scale_per_longitude() < 50.0) & (np.abs(lat - lat[k]) * table[k] < 50.0)
        assert np.array_equal(mask, pp.rectangular_domain(lon[k], lat[k], lon, lat, side_km=100.0))


def small_grid(seed=3, origin=(30.0, 40.0)):
    rng = np.random.default_rng(seed)
    lon = origin[0] + np.repeat(np.linspace(0.0, 1.2, 13), 11 * 3)
    lat = origin[1] + np.tile(np.repeat(np.linspace(0.0, 0.9, 11), 3), 13)
    dep = np.tile(np.array([1.0, 8.0, 15.0]), 13 * 11)
    return rng, lon, lat, dep


@pytest.mark.parametrize("origin", [(30.0, 40.0), (-71.0, -34.0)])
def test_host_loop_is_the_pinned_pieces_event_by_event(origin):
    """location_uncertainties_host adds no arithmetic of its own: bit for bit the direct calls of
    rectangular_domain / gibbs_weights / compute_location_uncertainty on seeded likelihood rows and max-beams."""
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    rng, lon, lat, dep = small_grid(origin=origin)
    K, E, N, off = lon.shape[0], 6, 400, 1000
    like = rng.random((E, K)).astype(np.float32)
    like[2] = np.nan                                                # a constant column's likelihood
    like[3] = 0.0
    src = rng.integers(0, K, E)
    for side in (100.0, 20.0, 5.0):
        got = location_uncertainties_host({"src_idx": src, "likelihood": like}, lon, lat, dep, "spatial",
                                          restricted_domain_side_km=side)
        assert got["n_domain"].dtype == np.int64 and got["hunc"].dtype == np.float64
        for e in range(E):
            k = src[e]
            dom = pp.rectangular_domain(lon[k], lat[k], lon, lat, side_km=side)
            with np.errstate(invalid="ignore"):
                h, v = pp.compute_location_uncertainty(lon[k], lat[k], dep[k], like[e][dom], lon[dom], lat[dom], dep[dom])
            assert np.array_equal(got["domain"][e], dom) and got["n_domain"][e] == dom.sum()
            assert np.array_equal([got["hunc"][e], got["vunc"][e]], [h, v], equal_nan=True), (side, e)
            assert (got["longitude"][e], got["latitude"][e], got["depth"][e]) == (lon[k], lat[k], dep[k])
        assert np.isnan(got["hunc"][2]) and np.isnan(got["vunc"][3])
        assert np.isfinite(got["hunc"][[0, 1, 4, 5]]).all()
        assert (got["hunc"][[0, 1, 4, 5]] > 0).all() or side == 5.0        # (5 km: the epicentre's own column)
    maxbeam = (2.0 * np.abs(rng.standard_normal((E, N)))).astype(np.float32)
    sources = rng.integers(0, K, (E, N)).astype(np.int32) + off
    res = {"src_idx": np.array([sources[e, maxbeam[e].argmax()] for e in range(E)]), "maxbeam": maxbeam,
           "maxbeam_sources": sources}
    for kT, cut in ((0.33, 0.25), (1.0, 0.5)):
        got = location_uncertainties_host(res, lon, lat, dep, "temporal", source_id_offset=off, effective_kT=kT,
                                          gibbs_cutoff=cut)
        assert "domain" not in got
        for e in range(E):
            k = res["src_idx"][e] - off
            w = pp.gibbs_weights(maxbeam[e], kT)
            assert w.dtype == np.float32
            m = w > cut
            dom = sources[e][m] - off
            h, v = pp.compute_location_uncertainty(lon[k], lat[k], dep[k], w[m], lon[dom], lat[dom], dep[dom])
            assert (got["hunc"][e], got["vunc"][e], got["n_domain"][e]) == (h, v, m.sum()), (kT, e)
            assert m.sum() >= 1 and (got["longitude"][e], got["depth"][e]) == (lon[k], dep[k])


def test_source_coordinate_checks_need_no_device():
    from seismic_bpmf_amd import BeamformerGPU, postprocess as pp
    from seismic_bpmf_amd.beampower import source_coordinate_tables
    _, lon, lat, dep = small_grid()
    K = lon.shape[0]
    tables = source_coordinate_tables(lon, lat, dep, K)
    assert tables.shape == (6, K) and tables.dtype == np.float64 and tables.flags.c_contiguous
    assert np.array_equal(tables[:3], [lon, lat, dep])
    assert np.array_equal(tables[3], pp.domain_scale_per_latitude(lat))
    u = np.arctan((1.0 - pp.WGS84_F) * np.tan(np.deg2rad(lat)))
    assert np.array_equal(tables[4], np.sin(u)) and np.array_equal(tables[5], np.cos(u))
    bf = BeamformerGPU.__new__(BeamformerGPU)                      # no plan, no device: the checks come first
    bf.K = K
    bad = lon.copy()
    bad[5] = np.nan
    for args in ((lon[:-1], lat, dep), (lon, lat.reshape(1, -1), dep), (lon, lat, dep[:3]), (bad, lat, dep),
                 (lon, np.where(np.arange(K) == 2, np.inf, lat), dep), (lon, lat, -bad), (lon, lat + 60.0, dep)):
        with pytest.raises(ValueError):
            bf.set_source_coordinates(*args)
        with pytest.raises(ValueError):
            source_coordinate_tables(*args, K)
    assert bf._coord_tables is None


def test_relocate_events_uncertainty_checks_need_no_device():
    from seismic_bpmf_amd.workflow import relocate_events
    f = np.zeros((2, 4, 3, 50), np.float32)
    wp = np.zeros((4, 3, 2), np.float32)
    bare = types.SimpleNamespace(S=4, P=2, K=10, _coord_tables=None)
    with pytest.raises(ValueError, match="set_source_coordinates"):
        relocate_events(bare, f, wp, uncertainties=True)
    with pytest.raises(ValueError, match="set_source_coordinates"):
        relocate_events(bare, f, wp, "temporal", uncertainties=True)
    have = types.SimpleNamespace(S=4, P=2, K=10, _coord_tables=object())
    for kw in (dict(restricted_domain_side_km=0.0), dict(restricted_domain_side_km=np.nan),
               dict(uncertainty_method="temporal", effective_kT=0.0),
               dict(uncertainty_method="temporal", gibbs_cutoff=np.inf),
               dict(uncertainty_method="temporal", domain_mask=True)):
        with pytest.raises(ValueError):
            relocate_events(have, f, wp, uncertainties=True, **kw)
