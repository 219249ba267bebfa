"""GPU: the error of the three device library functions that csrc/source_spectra.hip calls -- exp, log10, pow -- measured
one by one, bit for bit, through bpmf_source_spectra_dev, against correctly rounded values computed with mpmath
(tests/golden/source_spectra_ulp.npz, tests/golden/make_source_spectra_ulp_golden.py).  The allowances of
source_spectra_cases (ULP_EXP, ULP_LOG10, ULP_POW) rest on these figures.

 exp    flags 2, S = C = F = 1, signal = 1, dist_km = 1, geometry_constant = 0.125, radiation = 125: g = 1 exactly, and
        with f = q = 1 corrected[e] = exp(fl(pi tt[e])).
 log10  flags 8, snr = 16 > threshold 8, corrected = x[e], one station at distance 1, weight_max = 1,
        max_num_bad_measurements = 0: the weight is exactly 1.0f and log10_M0[e] = log10(x[e]).
 pow    the same call with snr = 1 and first_high_band = 0: measured_disp[e] = pow(10, log10(x[e])) of the device's own
        log10, which the fixture is searched for.

Each figure is |device - correctly rounded| in units of the float64 spacing at the correctly rounded value."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_spectra_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "source_spectra_ulp.npz")


def run(arrays, flags, **params):
    """One call with E = ULP_N, S = C = F = 1: {output: array} of the stages asked for."""
    import torch
    from seismic_bpmf_amd import _lib
    E = sc.ULP_N
    used, written = sc.touched(flags)
    specs = sc.output_specs(E, 1, 1, 1)
    tensors = {k: torch.as_tensor(np.ascontiguousarray(v), device="cuda") for k, v in arrays.items()}
    for k in used - set(arrays):
        shape, dtype = specs[k]
        tensors[k] = torch.as_tensor(np.zeros(shape, dtype), device="cuda")
    p = {k: C.c_void_p(t.data_ptr()) for k, t in tensors.items()}
    rc = sc.c_call(_lib.lib(), p, E, 1, 1, 1, flags, C.c_void_p(torch.cuda.current_stream().cuda_stream), **params)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().bpmf_last_error()
    return {k: tensors[k].cpu().numpy() for k in written}


def test_exp_log10_and_pow_lie_within_the_ulps_the_allowances_assume():
    with np.load(GOLDEN) as g:
        exp_cr, log10_cr, pow_cr = g["exp_cr"], g["log10_cr"], g["pow_cr"]
    tt, x = sc.ulp_arguments()
    E = sc.ULP_N
    assert len(tt) == len(x) == E >= 4096 and exp_cr.shape == (E,) and pow_cr.shape == (E, 2 * sc.ULP_NEIGHBOURS + 1)
    assert (np.pi * tt).max() >= 60.0 and x.min() <= 1e-13 and x.max() >= 1e3 and sc.ULP_NEIGHBOURS >= sc.ULP_LOG10
    ones, valid = np.ones(E), np.ones((E, 1), np.uint8)

    got = run({"signal": ones.reshape(E, 1, 1), "valid": valid, "dist": ones.reshape(E, 1), "tt": tt.reshape(E, 1),
               "frequencies": np.ones(1), "q": np.ones(1)}, 2, geometry_constant=0.125, radiation=125.0)
    exp_ulp = sc.ulps_from(got["corrected"].ravel(), exp_cr).max()

    stage4 = dict(snr_threshold=8.0, bands=1, weight_max=1.0, max_bad=0)
    tables = {"valid": valid, "epi": ones.reshape(E, 1), "corrected": x.reshape(E, 1, 1)}
    got = run({**tables, "snr": np.full((E, 1, 1), 16.0)}, 8, first_high=1, **stage4)
    assert (got["weights"] == np.float32(1.0)).all() and np.array_equal(got["measured_disp"].ravel(), x)
    log10_dev = got["log10_M0"]
    log10_ulp = sc.ulps_from(log10_dev, log10_cr).max()

    got = run({**tables, "snr": np.ones((E, 1, 1))}, 8, first_high=0, **stage4)
    assert (got["measurement_snr"] == np.float32(1.0)).all()
    column = np.full(E, -1)
    for k in range(-sc.ULP_NEIGHBOURS, sc.ULP_NEIGHBOURS + 1):
        column[sc.stepped(log10_cr, k) == log10_dev] = k + sc.ULP_NEIGHBOURS
    print(f"device library, worst error in ulp over {E} arguments: exp {exp_ulp:g} (allowed {sc.ULP_EXP}), "
          f"log10 {log10_ulp:g} (allowed {sc.ULP_LOG10})", end="")
    assert (column >= 0).all(), "the device's log10 lies outside the neighbours the fixture holds"
    pow_ulp = sc.ulps_from(got["measured_disp"].ravel(), pow_cr[np.arange(E), column]).max()
    print(f", pow {pow_ulp:g} (allowed {sc.ULP_POW})")
    assert exp_ulp <= sc.ULP_EXP and log10_ulp <= sc.ULP_LOG10 and pow_ulp <= sc.ULP_POW, (exp_ulp, log10_ulp, pow_ulp)
