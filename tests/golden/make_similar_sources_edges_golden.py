#!/usr/bin/env python3
"""Generate tests/golden/similar_sources_edges.npz from the REAL reference's clib.find_similar_sources
(BPMF/clib.py:104-221 -> BPMF/libc.c:55-387); runs only where the reference tree is (make_goldens.py:import_reference).

The inputs are not stored: they are the named and random cases of tests/decimate_cases.py, rebuilt from their seeds
wherever the file is read.  Stored are only the reference's flags, packed (np.packbits), one array per case and
method under the key "<case>/<method>", always from a single-threaded run (num_threads=1: the reference's OpenMP loops
race).

The archive is written with fixed member times, so that a second run reproduces the file byte for byte:
`python tests/golden/make_similar_sources_edges_golden.py --check` compares instead of writing.

Before writing, the recorded answers alone are checked for what keeps the cases from being trivial: every named case
outside decimate_cases.DEGENERATE has between 5 % and 95 % of its sources redundant under at least one method, and the
random set has more than 10 000 flags of each value.

Usage: python tests/golden/make_similar_sources_edges_golden.py [--check]
"""
import ctypes as C
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "similar_sources_edges.npz")
sys.path.insert(0, os.path.dirname(HERE))
import decimate_cases as dc  # noqa: E402


def key(case, method):
    return f"{case['name']}/{method}"


def reference_flags(clib, case, method):
    """The reference's own answer, single-threaded, with its progress prints sent nowhere."""
    mv, lon, lat, clon, clat, thr, n_diff = dc.args_of(case)
    sys.stdout.flush()
    keep, null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        red = clib.find_similar_sources(mv.copy(), lon.copy(), lat.copy(), clon.copy(), clat.copy(), thr,
                                        num_threads=1, num_stations_for_diff=n_diff, method=method)
    finally:
        C.CDLL(None).fflush(None)                                  # the C library's buffered prints go nowhere too
        os.dup2(keep, 1)
        os.close(keep)
        os.close(null)
    return np.asarray(red, bool)


def check_not_trivial(flags):
    """`flags`: key -> bool array.  The conditions of the module docstring, on recorded answers alone."""
    for case in dc.named_cases():
        if case["name"] in dc.DEGENERATE:
            continue
        shares = [flags[key(case, m)].mean() for m in dc.METHODS]
        assert any(0.05 <= s <= 0.95 for s in shares), (case["name"], shares)
    ones = sum(int(flags[key(c, m)].sum()) for c in dc.random_cases() for m in dc.METHODS)
    zeros = sum(int((~flags[key(c, m)]).sum()) for c in dc.random_cases() for m in dc.METHODS)
    assert ones > 10_000 and zeros > 10_000, (ones, zeros)
    return ones, zeros


def archive_bytes(arrays):
    """An .npz (np.load reads it) whose bytes depend on the arrays alone: fixed member times, one compression."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue())
    return buf.getvalue()


def main():
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    cases = dc.named_cases() + dc.random_cases()                   # built before import_reference changes directory
    _, clib = mg.import_reference()
    flags = {key(c, m): reference_flags(clib, c, m) for c in cases for m in dc.METHODS}
    ones, zeros = check_not_trivial(flags)
    data = archive_bytes({k: np.packbits(v) for k, v in flags.items()})
    assert len(data) < 256 * 1024, len(data)
    if "--check" in sys.argv[1:]:
        with open(OUT, "rb") as f:
            same = f.read() == data
        print(f"{OUT}: {'reproduced byte for byte' if same else 'DIFFERS from this run'}")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"{OUT}: {len(cases)} cases x {len(dc.METHODS)} methods, {sum(len(v) for v in flags.values())} flags, "
          f"random set {ones} redundant / {zeros} kept, {len(data)} bytes")


if __name__ == "__main__":
    main()
