#!/usr/bin/env python3
"""Generate tests/golden/picker.npz from the REAL reference (BPMF/utils.py: normalize_batch, find_picks, get_picks);
runs only where the reference tree, SciPy and pandas are (make_goldens.py:import_reference).

Only the reference's answers are stored, as arrays; the inputs are regenerated from their seeds by
tests/picker_cases.py:

* `norm_<k>`: utils.normalize_batch on the nine rows of norm_rows(n) for NORM_CASES + NORM_CASES_LARGE[k]; of the
  longer cases only the rows `norm_rows_<k>` are kept (the file stays small: the rows are independent of each other);
* `pick_value_<k>`, `pick_mean_<k>`, `pick_std_<k>`: utils.find_picks on pick_cases()[k], and `pick_index_<k>`: the
  peak indices that its scipy.signal.find_peaks call returned on the way;
* `select_<k>`: utils.get_picks on selection_cases()[k], the table written as Event.pick_PS_phases writes it
  (BPMF/dataset.py:1855-1865) and the prior as a pandas table of the stations that have one.

Usage: python tests/golden/make_picker_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "picker.npz")
sys.path.insert(0, os.path.dirname(HERE))


def kept_rows(n):
    """The rows (of nine) whose answers are stored for a case of n samples."""
    if n <= 300:
        return np.arange(9)
    if n <= 1203:
        return np.arange(7)
    if n <= 6001 and n != 6000:
        return np.array([0, 3, 4])
    return np.array([0])


def reference_find_picks(utils, series, threshold):
    """utils.find_picks and, beside its three results, the peak indices its find_peaks call returned."""
    seen = []
    find_peaks = utils.find_peaks

    def spy(*args, **kwargs):
        out = find_peaks(*args, **kwargs)
        seen.append(np.asarray(out[0], dtype=np.int64))
        return out
    utils.find_peaks = spy
    try:
        value, mean, std = utils.find_picks(series, threshold)
    finally:
        utils.find_peaks = find_peaks
    return value, mean, std, seen[0]


def reference_get_picks(utils, values, means, stds, counts, buffer_length, prior, search_win_samp):
    import pandas as pd
    S = len(counts)
    stations = [f"STA{s}" for s in range(S)]
    picks = pd.DataFrame(index=stations, columns=["P_probas", "P_picks", "P_unc", "S_probas", "S_picks", "S_unc"])
    for s, sta in enumerate(stations):
        for ph, name in enumerate("PS"):
            k = counts[s, ph]
            picks.loc[sta, [f"{name}_probas", f"{name}_picks", f"{name}_unc"]] = (
                values[s, ph, :k].copy(), means[s, ph, :k].copy(), stds[s, ph, :k].copy())
    kw = {}
    if prior is not None:
        table = pd.DataFrame(columns=["P", "S"])
        for s, sta in enumerate(stations):
            if not np.isnan(prior[s, 0]):
                table.loc[sta, "P"], table.loc[sta, "S"] = prior[s, 0], prior[s, 1]
        kw = {"prior_knowledge": table, "search_win_samp": search_win_samp}
    out = utils.get_picks(picks, buffer_length=buffer_length, **kw)
    return np.stack([np.asarray(out[c], dtype=np.float32) for c in
                     ["P_probas", "P_picks", "P_unc", "S_probas", "S_picks", "S_unc"]], axis=1)


def main():
    import picker_cases as pc
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF import utils
    out = {}
    with np.errstate(all="ignore"):
        for k, (n, W, overlap) in enumerate(pc.NORM_CASES + pc.NORM_CASES_LARGE):
            rows = kept_rows(n)
            ref = utils.normalize_batch(pc.norm_rows(n, k), normalization_window_sample=W, overlap=overlap)
            assert ref.dtype == np.float64
            out[f"norm_{k}"] = ref.reshape(9, n)[rows]
            out[f"norm_rows_{k}"] = rows
        for k, (label, series, threshold) in enumerate(pc.pick_cases()):
            value, mean, std, index = reference_find_picks(utils, series, threshold)
            out[f"pick_index_{k}"] = index
            out[f"pick_value_{k}"] = np.asarray(value, dtype=np.float32)
            out[f"pick_mean_{k}"] = np.asarray(mean, dtype=np.float64)
            out[f"pick_std_{k}"] = np.asarray(std, dtype=np.float64)
        for k, (label, values, means, stds, counts, buffer_length, prior, win) in enumerate(pc.selection_cases()):
            out[f"select_{k}"] = reference_get_picks(utils, values, means, stds, counts, buffer_length, prior, win)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
