"""csrc/np_order.h, the library's single statement of NumPy's summation order, against NumPy itself.  Runs on CPU: the
host C++ compiler builds tests/np_order_check.cpp, a stand-alone program that includes nothing of the library but that
header, and the program's sums are compared bit for bit with np.sum in float32 and in float64."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(1, 301)) + [1000, 8191, 8192, 8193, 16384, 16385, 24633, 40000]


def _host_cxx():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = cand and shutil.which(cand)
        if path:
            return path
    raise AssertionError("no host C++ compiler (set CXX)")


def test_one_thread_sums_equal_numpy_bit_for_bit(tmp_path):
    exe = tmp_path / "np_order_check"
    cmd = [_host_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "seismic_bpmf_amd", "csrc"),
           "-o", str(exe), os.path.join(ROOT, "tests", "np_order_check.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]

    rng = np.random.default_rng(20261020)
    base = (rng.standard_normal(max(LENGTHS)) * 10.0 ** rng.uniform(-3, 3, max(LENGTHS))).astype(np.float32)
    rows = [base[:m] for m in LENGTHS]
    for bad in (np.inf, np.nan):                         # one row with an Inf in it, one with a NaN
        row = base[:8193].copy()
        row[4321] = bad
        rows.append(row)
    with open(tmp_path / "rows.bin", "wb") as f:
        for row in rows:
            f.write(np.int32(row.size).tobytes())
            f.write(row.tobytes())

    res = subprocess.run([str(exe), str(tmp_path / "rows.bin")], capture_output=True, text=True)
    lines = res.stdout.splitlines()
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    # the walk against the descent for every chunk length, inside the program: at most 128 leaves, none deeper than 15
    assert lines[-1].split()[:2] == ["walk", "ok"], lines[-1]
    most_leaves, deepest = map(int, lines[-1].split()[2:])
    assert most_leaves <= 128 and deepest <= 15

    assert len(lines) == len(rows) + 1
    for row, line in zip(rows, lines):
        m, b32, b64 = line.split()
        assert int(m) == row.size
        got32 = np.array([int(b32, 16)], np.uint32).view(np.float32)[0]
        got64 = np.array([int(b64, 16)], np.uint64).view(np.float64)[0]
        with np.errstate(invalid="ignore"):
            want32 = np.sum(row)
            want64 = np.sum(np.arange(row.size) * row.astype(np.float64))
        assert want32.dtype == np.float32 and want64.dtype == np.float64
        for got, want in ((got32, want32), (got64, want64)):
            if np.isnan(want):                           # (a NaN's sign and payload are not NumPy's promise)
                assert np.isnan(got), (m, got, want)
            else:
                assert got.tobytes() == want.tobytes(), (m, got, want)
