#!/usr/bin/env python3
"""Generate tests/golden/resample.npz with scipy.signal.resample_poly itself (the call of Event.pick_PS_phases,
BPMF/dataset.py:1801-1804); runs only where SciPy is.

Only SciPy's answers are stored, as arrays; the inputs are regenerated from their seeds by tests/resample_cases.py:

* `up<u>_down<d>_n<n>`: resample_poly(rows(n), u, d, axis=-1)[golden_selection(n_out)] for every case of cases(): a
  short case whole, of a longer one the head, the middle (where the NaN of the last row spreads) and the tail of four
  rows (the file stays small: the rows are independent of each other);
* `taps_r<r>`: firwin(20 r + 1, 1 / r, window=("kaiser", 5.0)).astype(float32) for the rates of GOLDEN_RATES, the
  taps before the float32 multiplication by `up` (the test with a live SciPy goes through every rate 2 .. 64);
* `scipy_version`, `numpy_version`.

Usage: python tests/golden/make_resample_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resample.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import scipy
    from scipy.signal import firwin, resample_poly
    import resample_cases as rc
    out = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    with np.errstate(all="ignore"):
        for up, down, n in rc.cases():
            ref = resample_poly(rc.rows(n), up, down, axis=-1)
            assert ref.dtype == np.float32
            rows, samples = rc.golden_selection(ref.shape[-1])
            out[rc.golden_key(up, down, n)] = ref[np.ix_(rows, samples)]
        for r in rc.GOLDEN_RATES:
            out[f"taps_r{r}"] = firwin(20 * r + 1, 1.0 / r, window=("kaiser", 5.0)).astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
