"""CPU: the host definitions around the deep-learning picker (postprocess.normalize_batch_host, find_picks_host,
get_picks_host) against the reference's own answers (BPMF/utils.py: normalize_batch, find_picks, get_picks) recorded
in tests/golden/picker.npz by tests/golden/make_picker_golden.py -- and, with BPMF_RECORD_REFERENCE=<reference source
tree> (and SciPy and pandas installed), against the live reference functions; every refusal; and the power of the
cases of tests/picker_cases.py to reject planted defects."""
import importlib.util
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picker_cases as pc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "picker.npz")
REFERENCE = os.environ.get("BPMF_RECORD_REFERENCE")
NORM_ALL = pc.NORM_CASES + pc.NORM_CASES_LARGE


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_picker_golden", os.path.join(HERE, "golden",
                                                                                     "make_picker_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def live_utils():
    """BPMF.utils of the live reference, imported with stub modules; skipped where it is not available."""
    if not REFERENCE:
        pytest.skip("BPMF_RECORD_REFERENCE is not set: no live reference")
    pytest.importorskip("scipy")
    pytest.importorskip("pandas")
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "golden", "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.REF = REFERENCE
    cwd, path0, mods0 = os.getcwd(), list(sys.path), set(sys.modules)
    try:
        mg.import_reference()                        # chdir()s into a scratch directory: BPMF reads its cfg from the CWD
    finally:
        os.chdir(cwd)
    from BPMF import utils
    yield utils
    for name in set(sys.modules) - mods0:
        if isinstance(sys.modules[name], MagicMock) or name == "BPMF" or name.startswith("BPMF."):
            del sys.modules[name]
    sys.path[:] = path0


def _golden_picks(golden, k):
    return tuple(golden[f"pick_{name}_{k}"] for name in ("value", "mean", "std", "index"))


def host_norm(k):
    n, W, overlap = NORM_ALL[k]
    return pp.normalize_batch_host(pc.norm_rows(n, k), W, overlap)


# ---- the definitions against the reference's recorded answers ----

@pytest.mark.parametrize("k", range(len(NORM_ALL)))
def test_normalize_batch_host_equals_the_reference(golden, k):
    n = NORM_ALL[k][0]
    got = host_norm(k)
    assert got.dtype == np.float64 and got.shape == (3, 3, n)
    pc.check(got.reshape(9, n)[golden[f"norm_rows_{k}"]], golden[f"norm_{k}"], str(NORM_ALL[k]))


def test_the_normalisation_cases_meet_every_class():
    met = set()
    for k, (n, W, overlap) in enumerate(pc.NORM_CASES):
        met |= pc.norm_classes_met(pc.norm_rows(n, k), W, overlap)
    assert met == pc.NORM_CLASSES, pc.NORM_CLASSES - met


def test_find_picks_host_equals_the_reference(golden):
    met, total = set(), 0
    for k, (label, series, thr) in enumerate(pc.pick_cases()):
        got = pp.find_picks_host(series, thr, return_index=True)
        assert got[0].dtype == np.float32 and got[1].dtype == np.float64 and got[2].dtype == np.float64
        pc.check_picks(got, _golden_picks(golden, k), label)
        assert np.array_equal(series[got[3]], got[0])
        met |= pc.pick_classes_met(series, thr, got)
        total += len(got[0])
    assert met == pc.PICK_CLASSES, pc.PICK_CLASSES - met
    assert total > 150 and pc.ALL_CLASSES == pc.NORM_CLASSES | pc.PICK_CLASSES


def test_get_picks_host_equals_the_reference(golden):
    for k, (label, *args) in enumerate(pc.selection_cases()):
        got = pp.get_picks_host(*args)
        assert got.dtype == np.float32 and got.shape == (len(args[3]), 6)
        pc.check(got, golden[f"select_{k}"], label)
    # the designed table: what every station is there for
    want = golden["select_0"]
    assert np.isnan(want[0, 3:]).all() and want[0, 1] == np.float32(300.5)          # no S: the best P stays
    assert np.isnan(want[1, :3]).all() and want[1, 4] == np.float32(500.25)         # no P
    assert np.isnan(want[2, :3]).all() and want[2, 4] == 600.                       # every P after the best S
    assert want[3, 1] == 201. and want[3, 4] == 450.                                # a pick AT buffer_length goes
    assert want[4, 1] == 300. and want[4, 4] == 350. and golden["select_1"][4, 1] == 420. \
        and golden["select_1"][4, 4] == 640.                                        # the prior changes both winners
    assert want[5, 1] == 250. and want[5, 4] == 400.                                # ties: the first
    assert np.isnan(want[6]).all() and np.isnan(want[7]).all()


# ---- the same against the live reference ----

def test_live_normalize_batch(live_utils):
    with np.errstate(all="ignore"):
        for k, (n, W, overlap) in enumerate(NORM_ALL):
            ref = live_utils.normalize_batch(pc.norm_rows(n, k), normalization_window_sample=W, overlap=overlap)
            pc.check(host_norm(k), ref, str(NORM_ALL[k]))


def test_live_find_picks(live_utils, maker):
    for label, series, thr in pc.pick_cases():
        ref = maker.reference_find_picks(live_utils, series, thr)
        pc.check_picks(pp.find_picks_host(series, thr, return_index=True), ref, label)


def test_live_get_picks(live_utils, maker):
    for label, *args in pc.selection_cases():
        pc.check(pp.get_picks_host(*args), maker.reference_get_picks(live_utils, *args), label)


# ---- refusals ----

def test_normalize_batch_refusals():
    x = np.zeros((1, 3, 600), np.float32)
    for kw, what in ((dict(normalization_window_sample=1), "at least 2"),
                     (dict(normalization_window_sample=200, overlap=0.999), "shift of 0"),
                     (dict(normalization_window_sample=1000, overlap=0.3), "fold more than once"),   # shift 700 > 599
                     (dict(normalization_window_sample=8193), "at most 8192"),
                     (dict(normalization_window_sample=8192, overlap=0.95), "window")):              # shift 409: 1 window
        with pytest.raises(ValueError, match=what):
            pp.normalize_batch_host(x, **kw)
    with pytest.raises(ValueError, match=r"\(R, C, n\)"):
        pp.normalize_batch_host(x[0])
    # the smallest shapes that pass: two windows, shift n - 1
    assert pp.normalize_batch_host(np.ones((1, 1, 3), np.float32), 4, 0.5).shape == (1, 1, 3)
    assert pp.normalize_batch_plan(3, 4, 0.5) == (2, 2)
    assert pp.normalize_batch_plan(6001, 3000, 0.5) == (1500, 5) and pp.normalize_batch_plan(6000, 3000, 0.5)[1] == 5


def test_find_picks_and_get_picks_refusals():
    with pytest.raises(ValueError, match="one series"):
        pp.find_picks_host(np.zeros((2, 10), np.float32), 0.5)
    v, m, s, c = pc.selection_cases()[0][1:5]
    with pytest.raises(ValueError, match="max_picks"):
        pp.get_picks_host(v, m[:, :, :2], s, c, 0)
    with pytest.raises(ValueError, match="picks were dropped"):
        pp.get_picks_host(v, m, s, c + 10, 0)
    with pytest.raises(ValueError, match="prior must be"):
        pp.get_picks_host(v, m, s, c, 0, prior=np.zeros((2, 2)), search_win_samp=10)
    half = np.zeros((len(c), 2))
    half[0, 0] = np.nan
    with pytest.raises(ValueError, match="all NaN"):
        pp.get_picks_host(v, m, s, c, 0, prior=half, search_win_samp=10)
    with pytest.raises(ValueError, match="search_win_samp"):
        pp.get_picks_host(v, m, s, c, 0, prior=np.zeros((len(c), 2)))
    for starts in (np.zeros((2, 2)), np.zeros((2, 4), np.int64), np.zeros((1, 2, 3), np.int64), np.array([2**41])):
        with pytest.raises(ValueError, match="starts"):
            pp.picker_starts(starts, 3)
    # no event: an empty table of the right shape, whichever form the starts have
    assert pp.picker_starts(np.zeros((0,), np.int64), 3).shape == (0, 3)
    assert pp.picker_starts(np.zeros((0, 3), np.int64), 3).shape == (0, 3)
    assert pp.picker_starts([5, -7], 3).tolist() == [[5, 5, 5], [-7, -7, -7]]


def test_picker_windows_host_pads_with_zeros_in_place():
    data, starts, per_station = pc.day_case(100)
    N = data.shape[-1]
    w = pp.picker_windows_host(data, per_station, 100)
    assert w.shape == (4, 3, 3, 100) and w.dtype == np.float32
    for e in range(4):
        for s in range(3):
            for i in (0, 37, 99):
                t = per_station[e, s] + i
                want = data[s, :, t] if 0 <= t < N else np.zeros(3, np.float32)
                assert pc.same_bits(w[e, s, :, i], want)


# ---- the power of the cases: each planted defect is rejected, by exactly these cases ----

def _rejecting_norm_cases(golden):
    out = []
    for k in range(len(pc.NORM_CASES)):
        n = pc.NORM_CASES[k][0]
        try:
            pc.check(host_norm(k).reshape(9, n)[golden[f"norm_rows_{k}"]], golden[f"norm_{k}"])
        except AssertionError:
            out.append(pc.NORM_CASES[k])
    return out


def _rejecting_pick_cases(golden):
    out = []
    for k, (label, series, thr) in enumerate(pc.pick_cases()):
        try:
            pc.check_picks(pp.find_picks_host(series, thr, return_index=True), _golden_picks(golden, k))
        except AssertionError:
            out.append(label)
    return out


def test_defect_edge_windows_not_replaced(golden, monkeypatch):
    monkeypatch.setattr(pp, "_normalize_batch_replace_edges", lambda std, mean: None)
    assert _rejecting_norm_cases(golden) == list(pc.NORM_CASES)


def test_defect_true_centres_as_nodes(golden, monkeypatch):
    """The windows' centres in the row are k * shift + W / 2 - shift; the reference's nodes are a linspace."""
    def centres(n, shift, n_windows, W=None):
        return shift * np.arange(n_windows, dtype=np.float64) + centres.W / 2 - shift
    rejecting = []
    for k, (n, W, overlap) in enumerate(pc.NORM_CASES):
        centres.W = W
        monkeypatch.setattr(pp, "normalize_batch_nodes", centres)
        try:
            pc.check(host_norm(k).reshape(9, n)[golden[f"norm_rows_{k}"]], golden[f"norm_{k}"])
        except AssertionError:
            rejecting.append((n, W, overlap))
    assert rejecting == EXPECTED_TRUE_CENTRES


def test_std_zero_before_the_replacement_is_no_defect(golden, monkeypatch):
    """`std == 0 -> 1` commutes with the replacement of the edge windows: both copy or rewrite single elements, so
    doing it first gives the same bits on every case (the half-constant row holds an edge window of std 0 that the
    replacement hides and a middle one that becomes 1).  A device kernel may therefore fix each window as it is
    computed."""
    replace = pp._normalize_batch_replace_edges

    def zero_first(std, mean):
        std[std == 0] = 1
        replace(std, mean)
    monkeypatch.setattr(pp, "_normalize_batch_replace_edges", zero_first)
    assert _rejecting_norm_cases(golden) == []
    met = set()
    for k, (n, W, overlap) in enumerate(pc.NORM_CASES):
        met |= pc.norm_classes_met(pc.norm_rows(n, k), W, overlap)
    assert {"edge_std0_hidden", "middle_std0_becomes_1"} <= met


def test_defect_std_zero_never_fixed(golden, monkeypatch):
    """What the half-constant and constant rows are for: without std == 0 -> 1 they divide by zero."""
    real = pp.np.std

    def std_tiny(*a, **kw):
        out = real(*a, **kw)
        out[out == 0] = np.float32(2.0)              # so that the definition's own fix-up no longer sees a zero
        return out
    monkeypatch.setattr(pp.np, "std", std_tiny)
    rejecting = _rejecting_norm_cases(golden)
    monkeypatch.undo()
    # (where all nodes are equal nothing is interpolated: a zero or constant row gives 0 / 2 = 0 / 1 there)
    assert rejecting == [case for case in pc.NORM_CASES if case != (3000, 3000, .5)]


def test_defect_plateau_midpoint_off_by_one(golden, monkeypatch):
    monkeypatch.setattr(pp, "_plateau_midpoint", lambda left, right: (left + right + 1) // 2)
    assert _rejecting_pick_cases(golden) == EXPECTED_MIDPOINT


def test_defect_probability_sum_in_float64(golden, monkeypatch):
    def moments(samples, prob):
        total = prob.astype(np.float64).sum()
        mean = np.sum(samples * prob) / total
        return mean, np.sqrt(np.sum((samples - mean) ** 2) / total)
    monkeypatch.setattr(pp, "_pick_moments", moments)
    assert _rejecting_pick_cases(golden) == EXPECTED_FLOAT64_SUM


def test_defect_strictly_above_the_threshold(golden, monkeypatch):
    monkeypatch.setattr(pp, "_reaches", lambda value, threshold: value > threshold)
    assert _rejecting_pick_cases(golden) == ["value_equals_threshold"]


# which cases reject what (asserted above, so that the case list cannot quietly lose its teeth)
EXPECTED_TRUE_CENTRES = [case for case in pc.NORM_CASES if case != (3000, 3000, .5)]   # (equal nodes: no abscissa used)
EXPECTED_MIDPOINT = ["plateau_even", "one_sample_wide", "quantised", "quantised_low_threshold"] + \
    [f"random_{k}" for k in (3, 6, 9, 11, 14, 15, 16, 18, 20, 21, 23, 24)]
EXPECTED_FLOAT64_SUM = ["separated_gaussians", "saddle_above_floor", "saddle_below_floor", "plateau_even", "plateau_odd",
                        "one_sample_wide", "wider_than_128", "wider_than_128_odd", "forty_picks", "nan_on_flank"] + \
    [f"random_{k}" for k in (1, 2, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17, 19, 20, 22, 23, 25)]
