"""csrc/day_rows.h, the library's single statement of a row of day windows, against the host definitions.  Runs on CPU:
the host C++ compiler builds tests/day_rows_check.cpp, a stand-alone program that includes nothing of the library but
that header, and its row decomposition, clamped starts, `inside` and clipped samples are compared exactly with
postprocess.picker_starts, _clipped_windows and multiband_windows_host; its refusals with the conditions the four entry
points wrote out one by one before the header."""
import os
import subprocess

import numpy as np
import pytest

from seismic_bpmf_amd import postprocess as pp
from test_np_order import ROOT, _host_cxx

S, C, N, n = 3, 2, 50, 8
LIMIT = 2**40
STARTS = [-2**41, -2**40, -9, -8, -3, 0, 42, 43, 50, 2**40, 2**41]
MOST = 0x7fffffff
# (whole_events, S, C, N, windows) in the order of day_rows_check.cpp
REFUSAL_CASES = [(False, 3, 2, 50, 7), (True, 3, 2, 50, 7), (True, 3, 2, 50, 6), (False, 0, 2, 50, 6),
                 (False, 3, 0, 50, 6), (False, 3, 2, 0, 6), (False, 3, 2, LIMIT, 6), (False, 3, 2, LIMIT + 1, 6),
                 (False, 3, 2, 50, MOST // 2), (False, 3, 2, 50, MOST // 2 + 1), (False, MOST // 2 + 1, 2, 50, 6),
                 (True, MOST // 2 + 1, 2, 50, MOST // 2 + 1), (False, MOST // 2, 2, 50, 6), (True, 3, 2, 50, 0),
                 (True, 0, 0, 0, 0)]
N_NULL_CASES = 2                                         # then two cases with a null pointer: that comes first


def _refused_before(whole, S_, C_, N_, windows):
    """The conditions of the entry points before day_rows.h: picker.hip / resample.hip, and the two spectrum files."""
    if S_ == 0 or C_ == 0 or N_ == 0 or N_ > LIMIT or windows > MOST // C_:
        return True
    return windows % S_ != 0 if whole else S_ > MOST // C_


def test_rows_of_day_windows_equal_the_host_definitions(tmp_path):
    exe = tmp_path / "day_rows_check"
    cmd = [_host_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "seismic_bpmf_amd", "csrc"),
           "-o", str(exe), os.path.join(ROOT, "tests", "day_rows_check.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]

    rng = np.random.default_rng(20261021)
    day = rng.standard_normal((S, C, N)).astype(np.float32)
    day[1, 0, 0], day[2, 1, N - 1], day[0, 1, 45] = np.nan, -0.0, np.inf
    # event e starts at STARTS[e] on station 0 and one and two samples later on the next two: (E, S)
    starts = np.array(STARTS, dtype=np.int64)[:, None] + np.arange(S, dtype=np.int64)
    E = len(STARTS)
    records = [(item, 1, int(starts.reshape(-1)[item // C])) for item in range(E * S * C)]
    records += [(item, 0, 12345) for item in range(2 * S * C)]          # no starts: every window begins at 0
    with open(tmp_path / "rows.bin", "wb") as f:
        f.write(np.array([S, C, N, n], dtype=np.int64).tobytes())
        f.write(day.tobytes())
        f.write(np.array(records, dtype=np.int64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "rows.bin")], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == len(records) + len(REFUSAL_CASES) + N_NULL_CASES

    # what the host says: starts beyond +-2^40 are refused there and clamped on the device, all others pass unchanged
    for v in (-2**40 - 1, 2**40 + 1):
        with pytest.raises(ValueError, match="within"):
            pp.picker_starts(np.array([v]), S)
    clamped = np.clip(starts, -LIMIT, LIMIT)
    assert np.array_equal(pp.picker_starts(clamped, S), clamped)
    assert np.array_equal(pp.picker_starts(clamped[:, 0], S), np.repeat(clamped[:, :1], S, axis=1))
    want = pp._clipped_windows(day, np.broadcast_to(clamped[:, :, None], (E, S, C)), n)
    assert np.array_equal(want.view(np.uint32), pp.picker_windows_host(day, clamped, n).view(np.uint32))
    mb_windows, valid = pp.multiband_windows_host(day, clamped, n)
    zero_want = pp._clipped_windows(day, np.zeros((2, S, C), dtype=np.int64), n)

    seen_inside = set()
    for (item, has_start, _), line in zip(records, lines):
        word = line.split()
        got = [int(w) for w in word[:7]]
        samples = np.array([int(w, 16) for w in word[7:]], dtype=np.uint32)
        win, c = divmod(item, C)
        s = win % S
        e = win // S
        start = int(clamped[e, s]) if has_start else 0
        inside = start >= 0 and start + n <= N
        assert got == [item, win, c, s, (s * C + c) * N, start, int(inside)], line
        rows = want if has_start else zero_want
        assert np.array_equal(samples, rows[e, s, c].view(np.uint32)), line
        if has_start:
            assert inside == bool(valid[e, s])
            seen_inside.add(inside)
            if inside:                                   # (the spectra read a window that lies inside as it is)
                assert np.array_equal(samples, mb_windows[e, s, c].view(np.uint32))
            if abs(int(starts[e, s])) > LIMIT:
                assert not samples.any()                 # +0.0 throughout
    assert seen_inside == {True, False}
    assert valid[STARTS.index(42)].tolist() == [True, False, False] and valid[STARTS.index(0)].all()

    assert lines[-N_NULL_CASES:] == ["refused 1 entry: null pointer"] * N_NULL_CASES
    for case, line in zip(REFUSAL_CASES, lines[len(records):]):
        word = line.split(" ", 2)
        assert word[0] == "refused" and int(word[1]) == int(_refused_before(*case)), (case, line)
        text = word[2] if len(word) > 2 else ""
        if int(word[1]):
            assert text.startswith("entry: bad argument (S=%d C=%d N=%d " % case[1:4]), line
            assert ("whole number of events" in text) == case[0] and (f"windows={case[4]}" in text) == case[0], line
            assert case[0] or f"rows={case[4]})" in text, line
        else:
            assert text == "", line
