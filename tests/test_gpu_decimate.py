"""GPU: grid decimation against golden vectors from the reference's own libc.c and the pinned oracle; the edges
(roundings, cell edges, batch seams, stale working sets, input forms, refusals) on the cases of decimate_cases.py."""
import os

import numpy as np
import pytest

import decimate_cases as dc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("method", ["closest", "smallest"])
@pytest.mark.parametrize("ndiff", [5, 9])
def test_matches_reference_goldens(method, ndiff):
    from seismic_bpmf_amd.decimate import find_similar_sources
    g = np.load(os.path.join(GOLD, "similar_sources.npz"))
    red = find_similar_sources(g["moveouts"], g["lon"], g["lat"], g["cell_lon"], g["cell_lat"],
                               float(g[f"thr_{method}_{ndiff}"]), num_stations_for_diff=ndiff, method=method)
    assert red.dtype == bool and np.array_equal(red, g[f"red_{method}_{ndiff}"])


@pytest.mark.parametrize("method", ["closest", "smallest"])
def test_larger_grid_matches_oracle(oracle_lib, method):
    """Several batches of 256 kept sources, several cells, ties in the moveouts."""
    from seismic_bpmf_amd.decimate import find_similar_sources
    rng = np.random.default_rng(12)
    K, S = 3000, 11
    lon, lat = rng.uniform(0, 1, K).astype(np.float32), rng.uniform(0, 1, K).astype(np.float32)
    sta = rng.uniform(0, 1, (S, 2))
    mv = (np.hypot(lon[:, None] - sta[None, :, 0], lat[:, None] - sta[None, :, 1]) * 20).astype(np.float32)
    mv = np.round(mv, 1)                      # quantised -> ties in the argsort and in the sums
    cl = np.linspace(-0.01, 1.01, 4).astype(np.float32)
    for thr, nd in [(0.25, 6), (0.6, 11)]:
        red = find_similar_sources(mv, lon, lat, cl, cl, thr, num_stations_for_diff=nd, method=method)
        want = oracle_lib.find_similar_sources(mv, lon, lat, cl, cl, thr, nd, method)
        assert np.array_equal(red, want), (method, thr, (red != want).sum())
        assert 0.05 * K < red.sum() < 0.98 * K


# ---- the edges: the cases of decimate_cases.py, whose expected answers are the reference's own recorded ones
# (tests/golden/similar_sources_edges.npz; tests/test_decimate_definition.py holds the NumPy definition to the same file)
@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLD, "similar_sources_edges.npz")) as g:
        out = {}
        for case in dc.named_cases() + dc.random_cases():
            for method in dc.METHODS:
                flags = np.unpackbits(g[f"{case['name']}/{method}"])[:len(case["lon"])].astype(bool)
                flags.setflags(write=False)
                out[case["name"], method] = flags
        return out


def _device(case, method, **kw):
    from seismic_bpmf_amd.decimate import find_similar_sources
    mv, lon, lat, clon, clat, thr, n_diff = dc.args_of(case)
    return find_similar_sources(mv, lon, lat, clon, clat, thr, num_stations_for_diff=n_diff, method=method, **kw)


def _assert_same(got, want, label):
    assert got.dtype == bool and got.shape == want.shape, label
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (f"{label}: {diff.size} of {want.size} flags differ, first at sources {diff[:8].tolist()} "
                            f"(device {got[diff[:8]].astype(int).tolist()}, reference {want[diff[:8]].astype(int).tolist()})")


@pytest.mark.parametrize("method", dc.METHODS)
@pytest.mark.parametrize("name", dc.NAMED)
def test_named_case_equals_the_recorded_reference(recorded, name, method):
    case = dc.named_case(name)
    _assert_same(_device(case, method), recorded[name, method], f"{name} {method} ({case['why'] or ', '.join(case['reason'])})")


def test_random_cases_equal_the_recorded_reference(recorded):
    for case in dc.random_cases():
        for method in dc.METHODS:
            K, S = case["moveouts"].shape
            _assert_same(_device(case, method), recorded[case["name"], method],
                         f"{case['name']} {method} K={K} S={S} n_diff={case['n_diff']} thr={case['threshold']}")


@pytest.fixture(scope="module")
def big_grid():
    return dc.big_grid()


@pytest.mark.parametrize("method", dc.METHODS)
def test_back_to_back_calls_on_one_context(oracle_lib, recorded, big_grid, method):
    """bpmf_find_similar_sources takes its tables from the per-device working set and fills only `red` and `close`
    itself: each case runs directly behind a call of the OTHER method on a larger grid, and once more behind a small
    beamform host call on the same device."""
    from seismic_bpmf_amd import beamform
    other = dc.METHODS[1 - dc.METHODS.index(method)]
    rng = np.random.default_rng(32)
    f = np.abs(rng.standard_normal((3, 2, 400))).astype(np.float32)
    tau = rng.integers(0, 50, (20, 3, 2)).astype(np.int32)
    wp, ws = rng.random((3, 2, 2)).astype(np.float32), rng.random((20, 3)).astype(np.float32)
    want_beam = oracle_lib.beamform(f, tau, wp, ws, "strict", "max")
    big_first = None
    for name in ("chain_across_batches", "chain_in_one_cell", "batch_257", "S256_some", "nan_moveouts"):
        big = _device(big_grid, other)
        if big_first is None:
            big_first = big
            assert 2 * dc.FS_BATCH < (~big).sum() and 0.02 * big.size < big.sum()
            if other == "closest":
                _assert_same(big, oracle_lib.find_similar_sources(*dc.args_of(big_grid), other), "big grid")
        _assert_same(big, big_first, f"big grid {other}, repeated before {name}")
        case = dc.named_case(name)
        _assert_same(_device(case, method), recorded[name, method], f"{name} {method} behind a {other} call on 3000 x 40")
        mb, ma = beamform(f, tau, wp, ws, device="gpu", reduce="max", out_of_bounds="strict", device_id=0)
        assert np.array_equal(mb, want_beam[0]) and np.array_equal(ma, want_beam[1]), name
        _assert_same(_device(case, method), recorded[name, method], f"{name} {method} behind a beamform host call")


@pytest.mark.parametrize("method", dc.METHODS)
def test_input_forms_give_the_same_flags(recorded, method):
    from seismic_bpmf_amd.decimate import find_similar_sources
    case = dc.named_case("cells_change_answer")
    mv, lon, lat, clon, clat, thr, n_diff = dc.args_of(case)
    want = recorded[case["name"], method]
    kw = dict(num_stations_for_diff=n_diff, method=method)
    assert n_diff == mv.shape[1] and 0.05 < want.mean() < 0.95
    _assert_same(find_similar_sources(mv, lon, lat, clon, clat, thr, **kw), want, "float32, contiguous")
    _assert_same(find_similar_sources(mv.astype(np.float64), lon.astype(np.float64), lat.astype(np.float64),
                                      clon.astype(np.float64), clat.astype(np.float64), np.float64(thr), **kw), want, "float64")
    wide = np.full((mv.shape[0], 2 * mv.shape[1]), np.nan, np.float32)
    wide[:, ::2] = mv
    assert not wide[:, ::2].flags.c_contiguous
    _assert_same(find_similar_sources(wide[:, ::2], lon, lat, clon, clat, thr, **kw), want, "non-contiguous view")
    fortran = np.asfortranarray(mv)
    assert not fortran.flags.c_contiguous
    _assert_same(find_similar_sources(fortran, lon, lat, clon, clat, thr, **kw), want, "Fortran order")
    _assert_same(find_similar_sources(mv, lon.tolist(), lat.tolist(), clon.tolist(), clat.tolist(), thr, **kw), want, "lists")
    _assert_same(find_similar_sources(mv, lon, lat, clon, clat, thr, num_threads=3, **kw), want, "num_threads given")
    _assert_same(find_similar_sources(mv, lon, lat, clon, clat, thr, method=method), want, "num_stations_for_diff=None")
    # integer-typed moveouts (the reference only prints a warning): the same table in float32 is the same call.  The one
    # expected answer of this file that is not a recorded one: the definition's, which test_decimate_definition.py
    # holds to the reference's recorded flags on every case
    whole = np.random.default_rng(33).integers(0, 12, mv.shape)
    want = dc.definition(whole, lon, lat, clon, clat, 1.5, 4, method)
    assert 0.05 < want.mean() < 0.95
    for dtype in (np.int64, np.int32, np.float32):
        _assert_same(find_similar_sources(whole.astype(dtype), lon, lat, clon, clat, 1.5, num_stations_for_diff=4,
                                          method=method), want, f"whole seconds as {np.dtype(dtype).name}")


def test_refusals_come_before_any_device_work(recorded):
    import ctypes as C
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd.decimate import find_similar_sources
    case = dc.named_case("one_cell")
    mv, lon, lat, clon, clat, thr, n_diff = dc.args_of(case)
    K, S = mv.shape
    want = recorded[case["name"], "closest"]

    def valid_call_is_correct(label):
        _assert_same(_device(case, "closest"), want, f"valid call behind the refusal of {label}")

    # the Python surface raises where it checks, the rest is the library's refusal
    for label, exc, call in (
            ("method", ValueError, lambda: find_similar_sources(mv, lon, lat, clon, clat, thr, method="nearest")),
            ("1-D moveouts", ValueError, lambda: find_similar_sources(mv[:, 0], lon, lat, clon, clat, thr)),
            ("longitudes", ValueError, lambda: find_similar_sources(mv, lon[:-1], lat, clon, clat, thr)),
            ("latitudes", ValueError, lambda: find_similar_sources(mv, lon, lat[:-1], clon, clat, thr)),
            ("bad argument: n_stations must", _lib.BpmfHipError, lambda: find_similar_sources(np.zeros((4, 257), np.float32), lon[:4], lat[:4], clon, clat, thr)),
            ("bad argument: n_stations_for_diff must", _lib.BpmfHipError, lambda: find_similar_sources(mv, lon, lat, clon, clat, thr, num_stations_for_diff=0)),
            ("bad argument: n_stations_for_diff must", _lib.BpmfHipError, lambda: find_similar_sources(mv, lon, lat, clon, clat, thr, num_stations_for_diff=S + 1))):
        with pytest.raises(exc, match=label if exc is _lib.BpmfHipError else None):
            call()
        valid_call_is_correct(label)

    # the C ABI: -1, a message that names the argument, the output array untouched
    lib = _lib.lib()
    f, i = _lib._f, _lib._i
    wide = np.zeros((K, 257), np.float32)
    ptr = dict(moveouts=mv.ctypes.data_as(f), source_longitude=lon.ctypes.data_as(f), source_latitude=lat.ctypes.data_as(f),
               cell_longitude=clon.ctypes.data_as(f), cell_latitude=clat.ctypes.data_as(f))
    red = np.full(K, 7, np.int32)

    def call(n_stations=S, n_diff=n_diff, method=1, **null):
        p = {**ptr, **null}
        if n_stations == 257:
            p["moveouts"] = wide.ctypes.data_as(f)
        out = null.get("redundant_sources", red.ctypes.data_as(i))
        return lib.bpmf_find_similar_sources(p["moveouts"], p["source_longitude"], p["source_latitude"], p["cell_longitude"],
                                             p["cell_latitude"], C.c_float(thr), K, n_stations, clon.size - 1, clat.size - 1,
                                             n_diff, method, 0, out)

    for names_it, kw in (("n_stations ", dict(n_stations=257, n_diff=6)), ("n_stations_for_diff", dict(n_diff=0)),
                         ("n_stations_for_diff", dict(n_diff=S + 1)), ("method", dict(method=2)), ("method", dict(method=-1)),
                         ("moveouts is null", dict(moveouts=None)), ("source_longitude is null", dict(source_longitude=None)),
                         ("source_latitude is null", dict(source_latitude=None)), ("cell_longitude is null", dict(cell_longitude=None)),
                         ("cell_latitude is null", dict(cell_latitude=None)), ("redundant_sources is null", dict(redundant_sources=None))):
        assert call(**kw) == -1, kw
        msg = _lib.last_error()
        assert "bpmf_find_similar_sources" in msg and f"bad argument: {names_it}" in msg, (kw, msg)
        assert (red == 7).all(), kw
        valid_call_is_correct(str(kw))
    assert call() == 0, _lib.last_error()
    _assert_same(red.astype(bool), want, "the C ABI call itself")
    assert set(np.unique(red)) <= {0, 1}
