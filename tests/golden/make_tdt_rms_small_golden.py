#!/usr/bin/env python3
"""Generate tests/golden/tdt_rms_small.npz: the output of the REAL reference's time_dependent_threshold
(BPMF/libc.c:516-673, compiled where it lies by oracle.build_ref() into oracle/_ref/libc.so) on the short shapes of
tests/threshold_cases.py; runs only where the reference tree is.

The C function is called directly with (half_window, shift), single-threaded (its OpenMP loops race), on a copy of
every row (it fills the zeros in place).  Only the cases on which the reference stays inside its own window array are
recorded (threshold_cases.reference_in_bounds, the condition make_goldens.py asserts on the long shapes); the others
rest on the documented clamp and are listed under `clamped`.  The inputs are not stored: threshold_cases builds them
from integer arithmetic alone.  Only arrays are written: per case the (rows, n) float32 threshold.

Usage: python tests/golden/make_tdt_rms_small_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
import golden_npz  # noqa: E402
import threshold_cases as tc  # noqa: E402

OUT = os.path.join(HERE, "tdt_rms_small.npz")


def main():
    from oracle import oracle
    path = oracle.build_ref()
    assert path, "the reference tree is not here"
    lib = C.CDLL(path)
    f = C.POINTER(C.c_float)
    lib.time_dependent_threshold.argtypes = [f, f, C.c_float, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, f]
    lib.time_dependent_threshold.restype = None
    out, clamped = {}, []
    for case in tc.tdt_cases():
        if not case.in_bounds:
            clamped.append(case.name)
            continue
        thr = np.zeros((case.rows, case.n), np.float32)
        gauss = np.ascontiguousarray(case.gauss, np.float32)
        for r in range(case.rows):
            row = np.array(case.x[r], np.float32)                  # a copy: the reference writes into it
            lib.time_dependent_threshold(row.ctypes.data_as(f), gauss.ctypes.data_as(f), float(case.num_dev), case.n,
                                         case.half, case.shift, 1, thr[r].ctypes.data_as(f))
        out["thr__" + case.name] = thr
    written = golden_npz.save(OUT, **out, clamped=np.array(clamped))
    print(f"{len(out)} cases recorded, {len(clamped)} rest on the clamp; "
          + ", ".join(f"{os.path.basename(p)} {os.path.getsize(p)} bytes" for p in written))


if __name__ == "__main__":
    main()
