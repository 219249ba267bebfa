#!/usr/bin/env python3
"""Generate tests/golden/svdwf.npz from the REAL reference (BPMF/utils.py: SVDWF, bandpass_filter; the stack of
BPMF/dataset.py:4331-4334) and SciPy; runs only where the reference tree and SciPy are
(make_goldens.py:import_reference).

Only recorded results are stored; the inputs are regenerated from their seeds by tests/svdwf_cases.py:

* `filtered_<k>`, `stack_<k>`, `k_<k>`: utils.SVDWF on REFERENCE_CASES[k] (of the larger cases only the rows
  svdwf_cases.kept_rows of `filtered`), the reference's normalised stack of it, and the reference's n_singular_values;
* `limit_ref`: 4 x the worst deviation of postprocess.svdwf_host / svdwf_stack_host from these, relative to the
  channel's largest |filtered| (|stack|) -- float32 LAPACK answers move with the BLAS build and its thread count;
* `bandpass_<k>`: utils.bandpass_filter on BANDPASS_CASES[k]; `bandpass_limit`: 8 x the worst relative deviation of
  postprocess.bandpass_filter_host from these (least squares there, closed form here);
* `butter_<k>`: iirfilter + zpk2sos on BUTTER_CASES[k]; `butter_coef_dev`: the worst coefficient deviation of
  postprocess.butter_bandpass_sos.

Usage: python tests/golden/make_svdwf_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "svdwf.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def reference_svdwf(utils, a, expl_var, kmax, w, bandpass, sc):
    """utils.SVDWF, the reference's stack of it, and the n_singular_values it selected."""
    from scipy.linalg import svd
    with np.errstate(all="ignore"):
        filtered = utils.SVDWF(a, expl_var=expl_var, max_singular_values=kmax, wiener_filter_colsize=w,
                               freqmin=sc.FREQMIN, freqmax=sc.FREQMAX,
                               sampling_rate=sc.SAMPLING_RATE if bandpass else None)
    filtered32 = np.zeros_like(a)
    filtered32[...] = filtered                                       # filtered_data[:, s, c, :] = utils.SVDWF(...)
    stack = np.mean(filtered32, axis=0)
    norm = np.max(stack, axis=-1)
    stack = stack / (1.0 if norm == 0.0 else norm)
    s = svd(a, full_matrices=False)[1]
    var = np.cumsum(s ** 2)
    k = 0 if var[-1] == 0.0 else min(kmax, int(np.min(np.where(var / var[-1] >= expl_var)[0])) + 1)
    return filtered32, stack.astype(np.float32), k


def main():
    import svdwf_cases as sc
    from scipy.signal import iirfilter, zpk2sos
    from seismic_bpmf_amd import postprocess as pp
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF import utils
    out, worst = {}, 0.0
    sos = sc.sos_table()
    for k, (label, kind, n, m, expl_var, kmax, w, bandpass) in enumerate(sc.REFERENCE_CASES):
        a = sc.reference_matrix(k)
        filtered, stack, rank = reference_svdwf(utils, a, expl_var, kmax, w, bandpass, sc)
        mine, mine_stack, mine_rank = pp.svdwf_stack_host(a[:, None, None, :], expl_var=expl_var,
                                                          max_singular_values=kmax, wiener_filter_colsize=w,
                                                          sos=sos if bandpass else None)
        assert mine_rank[0, 0, 0] == rank, (label, mine_rank, rank)
        dev = np.abs(mine[:, 0, 0] - filtered).max() / sc.scale(filtered)
        dev_stack = np.abs(mine_stack[0, 0, 0] - stack).max() / sc.scale(stack)
        print(f"{label}: k {rank}, filtered {dev:.2e}, stack {dev_stack:.2e}")
        worst = max(worst, dev, dev_stack)
        out[f"filtered_{k}"], out[f"stack_{k}"], out[f"k_{k}"] = filtered[sc.kept_rows(n)], stack, np.int32(rank)
    assert worst < 1e-4, worst                                      # beyond that the restatement is wrong
    out["limit_ref"] = np.float64(4 * worst)
    worst_bp = 0.0
    for k, (rows, m, order, lo, hi) in enumerate(sc.BANDPASS_CASES):
        x = sc.bandpass_rows(k)
        ref = utils.bandpass_filter(x, filter_order=order, freqmin=lo, freqmax=hi, f_Nyq=sc.SAMPLING_RATE / 2)
        mine = pp.bandpass_filter_host(x, freqmin=lo, freqmax=hi, f_Nyq=sc.SAMPLING_RATE / 2, filter_order=order)
        dev = np.abs(mine - ref).max() / sc.scale(ref)
        print(f"band-pass {(rows, m, order, lo, hi)}: {dev:.2e}")
        worst_bp = max(worst_bp, dev)
        out[f"bandpass_{k}"] = ref
    out["bandpass_limit"] = np.float64(8 * worst_bp)
    worst_coef = 0.0
    for k, (order, lo, hi) in enumerate(sc.BUTTER_CASES):
        nyq = sc.SAMPLING_RATE / 2
        ref = zpk2sos(*iirfilter(order, [lo / nyq, hi / nyq], btype="bandpass", ftype="butter", output="zpk"))
        worst_coef = max(worst_coef, float(np.abs(pp.butter_bandpass_sos(order, lo / nyq, hi / nyq) - ref).max()))
        out[f"butter_{k}"] = ref
    out["butter_coef_dev"] = np.float64(worst_coef)
    np.savez_compressed(OUT, **out)
    print(f"limit_ref {out['limit_ref']:.3e}, bandpass_limit {out['bandpass_limit']:.3e}, butter_coef_dev "
          f"{worst_coef:.3e}")
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
