#!/usr/bin/env python3
"""Generate tests/golden/spectral_fit.npz from the REAL reference (BPMF/spectrum.py: Spectrum.fit_average_spectrum
:729-849 with the module's brune / boatwright, and the gates and averages of compute_moment_magnitude :1907-1990 redone
with the reference's own arithmetic on the recorded fits); runs only where the reference tree and SciPy are
(make_goldens.py:import_reference).

fit_average_spectrum runs on duck-typed averages: a Spectrum whose `average_p_spectrum` is a dict of a masked array,
the frequencies and the number of valid channels.  scipy.optimize.curve_fit is wrapped for the run so that popt and
pcov are seen even where the method returns before it stores them (the below-fc gate).  For every group <g> of
tests/spectral_fit_cases.py:RECORDED (model, weighted, F) with E events each:

* `average_<g>`, `mask_<g>`, `numvalid_<g>` (E, F), `freq_<g>` (F,): the inputs, as sfc.recorded_inputs makes them;
* `popt_<g>` (E, 2), `pcov_<g>` (E, 2, 2): curve_fit's answer (NaN where the method returned before the fit or the fit
  raised), `called_<g>` (E,) bool: curve_fit was reached, `success_<g>` (E,) bool: inversion_success;
* `cost_<g>` (E,): 1/2 sum (w (y - model(x, *popt)))^2 with the reference's model function and the weights it handed
  to curve_fit (NaN where there is no popt);
* `scipy_version`, `numpy_version`.

Usage: python tests/golden/make_spectral_fit_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "spectral_fit.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import scipy
    import scipy.optimize
    import spectral_fit_cases as sfc
    spec_ = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mg)
    mg.import_reference()
    from BPMF import spectrum as ref
    warnings.simplefilter("ignore")
    real_curve_fit, seen = scipy.optimize.curve_fit, {}

    def capture(f, x, y, **kw):
        seen.update(called=True, x=np.array(x), y=np.array(y), sigma=kw.get("sigma"))
        popt, pcov = real_curve_fit(f, x, y, **kw)
        seen.update(popt=np.array(popt), pcov=np.array(pcov))
        return popt, pcov

    scipy.optimize.curve_fit = capture
    out = {}
    try:
        for group, (model, weighted, F, E, _) in sfc.RECORDED.items():
            x = sfc.recorded_inputs(group)
            popt, pcov = np.full((E, 2), np.nan), np.full((E, 2, 2), np.nan)
            cost, called, success = np.full(E, np.nan), np.zeros(E, bool), np.zeros(E, bool)
            for e in range(E):
                spec = ref.Spectrum()
                spec.average_spectra = ["p"]
                spec.average_p_spectrum = {
                    "spectrum": np.ma.masked_array(np.array(x["average"][e]), mask=np.array(x["mask"][e])),
                    "freq": np.array(x["frequencies"]), "num_valid_channels": np.array(x["num_valid"][e])}
                seen.clear()
                with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    spec.fit_average_spectrum("p", model=model, weighted=weighted)
                called[e], success[e] = bool(seen.get("called")), bool(spec.inversion_success)
                if "popt" in seen:
                    popt[e], pcov[e] = seen["popt"], seen["pcov"]
                    with np.errstate(all="ignore"):
                        residual = seen["y"] - getattr(ref, model)(seen["x"], *seen["popt"], log=True)
                        if seen["sigma"] is not None:
                            residual = residual / seen["sigma"]
                        cost[e] = 0.5 * np.sum(residual**2)
            for key, value in (("average", x["average"]), ("mask", x["mask"]), ("numvalid", x["num_valid"]),
                               ("freq", x["frequencies"]), ("popt", popt), ("pcov", pcov), ("cost", cost),
                               ("called", called), ("success", success)):
                out[f"{key}_{group}"] = value
            print(group, int(called.sum()), int(success.sum()))
    finally:
        scipy.optimize.curve_fit = real_curve_fit
    out["scipy_version"] = np.array(scipy.__version__)
    out["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
