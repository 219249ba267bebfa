"""CPU: the case table of threshold_cases.py before it is run on the device (test_gpu_threshold_seams.py).

* the NumPy definition of the RMS threshold equals the C oracle (tdt_rms_cpu) on every case, and both equal the
  reference's own output recorded in golden/tdt_rms_small.npz wherever the reference stays inside its window array;
  the other cases rest on the documented clamp of tdt_window_of and are listed in the file (`clamped`);
* the mirrors of the kernels' decomposition equal the definitions on every case;
* every planted defect is rejected by named cases (printed with -s: the catch matrix of profiles/threshold_seams.txt);
* the zero-placement cases hold their zero where their name says.

What a case cannot see (asserted below, so the list stays true):
  tail_dropped, tail_not_replaced       nothing where window % 32 == 0 (there is no tail); tail_not_replaced only where
                                        a zero lies in a tail
  remainder_steps_skipped               nothing where the number of steps is a multiple of 6 (windows 2, 30, 192, 194,
                                        384, 386)
  clamped_reload_accumulated            nothing where the window is shorter than one step (2, 30)
  gauss_without_g0                      only windows that start at a multiple of 500 (window 0 of every row)
  zero_step_by_min_not_abs              a step whose zero is its smallest value (no negative sample beside it)
  count_includes_zeros, dev_includes_zeros   rows without a zero in their whole global windows; one zero among 700
                                        samples moves the deviation too little to move a window value
  glob_takes_remainder                  n % window == 0
  smooth_skipped_below_3_windows        every case but those of exactly two windows
  expand_tail_gt                        every shape but shift = window + 1 with n + 1 a multiple of the shift: elsewhere
                                        i / shift of sample n - shift is the last window already (after the clamp)
  expand_unclamped                      the shapes the reference itself stays in bounds on
  group_window_from_first_only          shift >= 4 with every window edge on a multiple of 4
  group_tail_dropped                    n % 4 == 0, or no sample above the threshold among the last n % 4
  mad_head_window_zero                  half < shift (the head's window is window 0 anyway); the rms kind
  nan_threshold_falls_to_cap            no NaN threshold, or no finite cap on its row"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import golden_npz
import threshold_cases as tc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdt_rms_small.npz")
TDT_NAMES = [c.name for c in tc.tdt_cases()]
EXTRACT_NAMES = [c.name for c in tc.extract_cases()]
_f = C.POINTER(C.c_float)


@functools.lru_cache(maxsize=None)
def definition(name):
    c = tc.tdt_case(name)
    return tc.tdt_rms_definition(c.x, c.gauss, c.num_dev, c.half, c.shift)


def oracle_rows(oracle, case):
    """tdt_rms_cpu by (half_window, shift) on every row: the expanded threshold (rows, n)."""
    lib = oracle.load()
    full = np.zeros((case.rows, case.n), np.float32)
    gauss = np.ascontiguousarray(case.gauss, np.float32)
    for r in range(case.rows):
        x, scratch = np.ascontiguousarray(case.x[r]), np.empty(case.n, np.float32)
        rc = lib.tdt_rms_cpu(x.ctypes.data_as(_f), gauss.ctypes.data_as(_f), float(case.num_dev), case.n, case.half,
                             case.shift, scratch.ctypes.data_as(_f), full[r].ctypes.data_as(_f))
        assert rc == case.sizes[2], (case.name, rc)
    return full


@functools.lru_cache(maxsize=None)
def golden():
    return golden_npz.load(GOLD)


# ------------------------------------------------------------------------------- definition, oracle, reference ---
def test_the_table_holds_the_shapes_it_promises():
    cases = tc.tdt_cases()
    stream = [c for c in cases if c.group == "stream"]
    assert sorted({2 * c.half for c in stream}) == list(tc.STREAM_WINDOWS)
    assert [w // 32 for w in tc.STREAM_WINDOWS] == [0, 0, 1, 1, 1, 2, 5, 5, 6, 6, 7, 11, 12, 12, 13, 13]
    assert {w % 32 for w in tc.STREAM_WINDOWS} == {0, 2, 30}
    for w in tc.STREAM_WINDOWS:
        shifts = {c.shift for c in stream if 2 * c.half == w}
        assert {1, w, w + 1} <= shifts and any(s % 4 == 2 for s in shifts), w
        assert any(s % 2 == 1 and abs(s - 0.75 * w) <= 1.5 for s in shifts), w
    for c in stream:
        assert c.n % 2 == 1 and c.rows == 4 and {r * c.n % 4 for r in range(4)} == {0, 1, 2, 3}, c.name
        assert (c.x == 0).any() and np.signbit(c.x[c.x == 0]).any(), c.name
    lanes = [c for c in cases if c.group == "lanes"]
    want = {1, 63, 64, 65, 127, 128, 129}
    assert {c.rows * c.sizes[2] for c in lanes} == want and {c.rows * c.sizes[1] for c in lanes} >= want
    assert {c.sizes[2] for c in cases if c.group == "smooth"} >= {1, 2, 3}
    assert {c.in_bounds for c in cases if c.group == "expand"} == {True, False}
    ex = tc.extract_cases()
    for kind in ("rms", "mad"):
        mine = [c for c in ex if c.kind == kind]
        assert {c.x.shape[1] % 4 for c in mine} == {0, 1, 2, 3}
        assert {4095, 4096, 4097, 8193} <= {c.x.shape[1] for c in mine} and {1, 2, 3, 5} <= {c.shift for c in mine}
        assert all(np.unique(c.thr[~np.isnan(c.thr)]).size == np.count_nonzero(~np.isnan(c.thr)) for c in mine)


@pytest.mark.parametrize("name", TDT_NAMES)
def test_definition_equals_the_oracle_and_the_recorded_reference(oracle_lib, name):
    case = tc.tdt_case(name)
    thr_win, full = definition(name)
    assert full.dtype == np.float32 and thr_win.shape == (case.rows, case.sizes[2])
    orc = oracle_rows(oracle_lib, case)
    assert tc.same_values(full, orc), name
    g = golden()
    if case.in_bounds:
        ref = g["thr__" + name]
        assert tc.same_values(full, ref) and tc.same_values(orc, ref), name
    else:
        assert name in set(g["clamped"].tolist()) and "thr__" + name not in g.files


def test_the_recorded_reference_covers_the_table_and_nothing_else():
    g = golden()
    recorded = {k[len("thr__"):] for k in g.files if k.startswith("thr__")}
    clamped = set(g["clamped"].tolist())
    assert recorded == {c.name for c in tc.tdt_cases() if c.in_bounds}
    assert clamped == {c.name for c in tc.tdt_cases() if not c.in_bounds}
    assert len(recorded) >= 50
    # every window length and every group is pinned to the reference at least once
    assert {2 * tc.tdt_case(n).half for n in recorded} >= set(tc.STREAM_WINDOWS)
    assert {tc.tdt_case(n).group for n in recorded} == {"stream", "lanes", "zeros", "smooth", "expand"}


@pytest.mark.parametrize("name", TDT_NAMES)
def test_the_mirror_without_a_defect_equals_the_definition(name):
    c = tc.tdt_case(name)
    thr_win, full = definition(name)
    m_win, m_full = tc.tdt_rms_mirror(c.x, c.gauss, c.num_dev, c.half, c.shift)
    assert tc.same_bits(m_win, thr_win) and tc.same_bits(m_full, full), name


@pytest.mark.parametrize("name", EXTRACT_NAMES)
def test_extraction_mirror_equals_its_definition_and_the_probes_decide(name):
    c = tc.extract_case(name)
    want = tc.extract_definition(c.x, c.thr, c.kind, c.window_or_half, c.shift, c.row_cap)
    for capacity in (1, max(1, want.size), want.size + 1):
        got = tc.extract_mirror(c.x, c.thr, c.kind, c.window_or_half, c.shift, c.row_cap, capacity=capacity)
        assert tc.same_records(got, want), (name, capacity)
    found = set(zip(want["row"].tolist(), want["index"].tolist()))
    for r, i, how in c.probes:                     # on the threshold: no candidate; one ulp above: a candidate
        assert ((r, i) in found) == (how == "ulp"), (name, r, i, how)
    if "nothing_above" in name:
        assert want.size == 0
    elif "n_equals_window" not in name:
        assert {"eq", "ulp"} == {p[2] for p in c.probes} and want.size >= sum(p[2] == "ulp" for p in c.probes)
    if "nan_threshold_row" in name:
        assert np.isnan(c.thr[0]).all() and not (want["row"] == 0).any() and (c.x[0] > c.row_cap[0]).any()


def test_smoothing_cases_hold_their_sign_patterns():
    for c in tc.tdt_cases():
        if c.group == "smooth":
            assert tc.smooth_pattern_holds(c), c.name


# ------------------------------------------------------------------------------------------ zero placement ---
def test_zero_cases_hold_their_zero_where_the_name_says():
    W, n = tc.ZW, tc.ZN
    for c in tc.tdt_cases():
        if c.group != "zeros":
            continue
        e, row = c.expect, c.x[c.zero_row]
        zeros = np.flatnonzero(row == 0)
        assert zeros.size and not (c.x[0] == 0).any() and not (c.x[2] == 0).any(), c.name
        window, n_glob, n_win = c.sizes
        trace = []
        tc.tdt_rms_mirror(c.x, c.gauss, c.num_dev, c.half, c.shift, trace=trace)
        on_g = np.stack([g for _, g in trace])[:, c.zero_row * n_win:(c.zero_row + 1) * n_win]   # (step, window of the row)
        assert [b for b, _ in trace] == [0, 1, 2]
        if "j" in e:                               # one zero, shift = window: sample j of one window
            assert zeros.tolist() == [e["window"] * W + e["j"]] and c.shift == W, c.name
            if e.get("tail"):
                assert e["j"] >= (W // tc.STEP) * tc.STEP and not on_g.any(), c.name
                assert e["j"] in (96, 97)
            else:
                assert e["j"] // tc.STEP == e["step"] and e["j"] % tc.STEP in ((0, 31) if "step_" in c.name else range(32))
                want = np.zeros_like(on_g)
                want[e["step"], e["window"]] = True                 # one lane, one step
                assert np.array_equal(on_g, want), c.name
            if "gauss" in e:
                assert (e["window"] * c.shift) % tc.GAUSS_LEN != 0 and zeros[0] % tc.GAUSS_LEN == e["gauss"]
            assert np.signbit(row[zeros[0]]) == bool(e.get("negative")), c.name
            if e.get("negative_step"):
                step = row[e["window"] * W + 32:e["window"] * W + 64]
                assert np.count_nonzero(step == 0) == 1 and (step[step != 0] < 0).all()
        if "all_zero_sliding" in e:
            q = e["all_zero_sliding"]
            assert zeros.tolist() == list(range(q * c.shift, q * c.shift + W)) and on_g[:, q].all(), c.name
        if "all_zero_global" in e:
            q = e["all_zero_global"]
            assert zeros.tolist() == list(range(q * W, (q + 1) * W)), c.name
        if e.get("remainder_only"):
            assert zeros.min() == n_glob * W and zeros.max() == n - 1 and (n_win - 1) * c.shift + W > zeros.min()
        if e.get("lanes") == 64:                   # every lane of one wave takes `g` in some step
            lanes = np.arange(64 * e["wave"], 64 * e["wave"] + 64)
            assert (lanes // n_win == c.zero_row).all()
            assert on_g[:, lanes % n_win].any(0).all() and zeros.size == 1, c.name
        if e.get("nan_row"):
            thr_win, full = definition(c.name)
            assert np.isnan(thr_win[1]).all() and np.isfinite(thr_win[[0, 2]]).all(), c.name
            assert (row[:n_glob * W] == 0).all()
        else:
            assert np.isfinite(definition(c.name)[0]).all(), c.name


# -------------------------------------------------------------------------------------------- catch matrix ---
# defect -> cases that MUST reject it, cases that CANNOT (see the module docstring)
TDT_CATCH = {
    "tail_dropped": (["stream_w34_s34", "stream_w30_s30", "stream_w418_s1", "zero_tail_first"],
                     ["stream_w32_s32", "stream_w384_s1", "stream_w64_s65"]),
    "tail_not_replaced": (["zero_tail_first", "zero_tail_last"],
                          ["stream_w32_s32", "stream_w192_s1", "zero_step_last", "zero_one_lane"]),
    "gauss_without_g0": (["zero_gauss_index_499", "zero_gauss_index_0", "zero_step_first", "stream_w34_s1"],
                         ["lanes_1_as_1x1", "smooth_1_windows"]),
    "zero_step_by_min_not_abs": (["zero_in_negative_step", "zero_step_first"], ["zero_tail_first", "stream_w30_s30"]),
    "clamped_reload_accumulated": (["stream_w32_s32", "stream_w64_s1", "stream_w192_s193", "stream_w418_s418"],
                                   ["stream_w2_s1", "stream_w30_s31"]),
    "remainder_steps_skipped": (["stream_w32_s1", "stream_w160_s160", "stream_w224_s225", "stream_w352_s1",
                                 "stream_w416_s416", "zero_step_last"],
                                ["stream_w192_s192", "stream_w194_s1", "stream_w384_s385", "stream_w30_s1"]),
    "count_includes_zeros": (["zero_one_lane", "zero_negative_zero", "zero_run_over_a_global_window"],
                             ["zero_only_in_the_remainder", "smooth_8_windows"]),
    "dev_includes_zeros": (["zero_run_over_a_global_window", "zero_run_over_a_sliding_window"],
                           ["zero_only_in_the_remainder", "smooth_8_windows"]),
    "glob_takes_remainder": (["stream_w34_s34", "lanes_64_as_8x8", "zero_step_first"],
                             ["expand_one_window_n_equals_window"]),
    "smooth_skipped_below_3_windows": (["smooth_2_windows", "expand_n_minus_shift_below_shift"],
                                       ["smooth_1_windows", "smooth_3_windows", "smooth_8_windows"]),
    "expand_tail_gt": (["expand_tail_decides"], ["stream_w34_s34", "expand_clamp_idle", "smooth_2_windows"]),
    "expand_unclamped": (["expand_clamp_acts", "expand_clamp_acts_by_one", "stream_w64_s1"],
                         ["expand_clamp_idle", "stream_w34_s34"]),
}
EXTRACT_CATCH = {
    "group_window_from_first_only": (["extract_rms_n4096_s1", "extract_rms_n41_s3", "extract_mad_n4097_s5",
                                      "extract_mad_n4096_s2"], []),
    "group_tail_dropped": (["extract_rms_n41_s1", "extract_rms_n4097_s2", "extract_mad_n8193_s3", "extract_mad_n43_s5"],
                           ["extract_rms_n40_s1", "extract_rms_n4096_s5", "extract_mad_n4096_s1"]),
    "ge_instead_of_gt": (["extract_rms_n4095_s1", "extract_mad_n4096_s3", "extract_rms_no_cap"],
                         ["extract_rms_nothing_above"]),
    "cap_ignored": (["extract_rms_n4096_s2", "extract_mad_n42_s1"], ["extract_rms_no_cap", "extract_mad_no_cap"]),
    "mad_head_window_zero": (["extract_mad_n4096_s1", "extract_mad_n40_s2", "extract_mad_n8193_s3",
                              "extract_mad_wide_window"],
                             ["extract_mad_n4096_s5", "extract_rms_n4096_s1"]),
    "nan_threshold_falls_to_cap": (["extract_rms_nan_threshold_row", "extract_mad_nan_threshold_row"],
                                   ["extract_rms_n4096_s1"]),
}


def test_every_defect_is_listed():
    assert set(TDT_CATCH) == tc.TDT_DEFECTS and set(EXTRACT_CATCH) == tc.EXTRACT_DEFECTS


@pytest.mark.parametrize("defect", sorted(tc.TDT_DEFECTS))
def test_planted_threshold_defect_is_rejected_by_named_cases(defect):
    must, cannot = TDT_CATCH[defect]
    caught = []
    for c in tc.tdt_cases():
        thr_win, full = definition(c.name)
        m_win, m_full = tc.tdt_rms_mirror(c.x, c.gauss, c.num_dev, c.half, c.shift, drop=defect)
        if not (tc.same_bits(m_win, thr_win) and tc.same_bits(m_full, full)):
            caught.append(c.name)
    print(f"CATCH {defect}: {len(caught)} of {len(tc.tdt_cases())} cases: " + " ".join(caught))
    assert caught and set(must) <= set(caught), sorted(set(must) - set(caught))
    assert not set(cannot) & set(caught), sorted(set(cannot) & set(caught))


@pytest.mark.parametrize("defect", sorted(tc.EXTRACT_DEFECTS))
def test_planted_extraction_defect_is_rejected_by_named_cases(defect):
    must, cannot = EXTRACT_CATCH[defect]
    caught = []
    for c in tc.extract_cases():
        want = tc.extract_definition(c.x, c.thr, c.kind, c.window_or_half, c.shift, c.row_cap)
        got = tc.extract_mirror(c.x, c.thr, c.kind, c.window_or_half, c.shift, c.row_cap, drop=defect)
        if not tc.same_records(got, want):
            caught.append(c.name)
    print(f"CATCH {defect}: {len(caught)} of {len(tc.extract_cases())} cases: " + " ".join(caught))
    assert caught and set(must) <= set(caught), sorted(set(must) - set(caught))
    assert not set(cannot) & set(caught), sorted(set(cannot) & set(caught))


def test_window_params_reach_the_admitted_edge():
    """A handful of (sliding window, overlap) pairs of the Python entry: an odd window with overlap 0 gives
    shift = window + 1 (tdt_sizes admits it on purpose)."""
    from seismic_bpmf_amd.threshold import window_params
    got = [window_params(w, ov) for w, ov in tc.OVERLAP_CASES]
    assert got[0] == (17, 35) and got[1] == (32, 48) and got[3] == (50, 50)
    for (half, shift), (w, _) in zip(got, tc.OVERLAP_CASES):
        assert tc.tdt_sizes(3 * w + 5, half, shift) is not None
