#!/usr/bin/env python3
"""Generate tests/golden/source_spectra_ulp.npz: correctly rounded exp, log10 and 10 ** y at the arguments of
tests/test_gpu_source_spectra_ulp.py, computed with mpmath at 200 bits and rounded once, to nearest, to float64.

The arguments are regenerated from a seed (source_spectra_cases.ulp_arguments); the file holds
* `exp_cr` (N,): the correctly rounded exp(z) of z = fl(pi * tt), the argument the device's exp receives;
* `log10_cr` (N,): the correctly rounded log10(x);
* `pow_cr` (N, 2 * ULP_NEIGHBOURS + 1): the correctly rounded 10 ** y for y = the correctly rounded log10(x) stepped
  by -ULP_NEIGHBOURS .. +ULP_NEIGHBOURS float64 neighbours (the device's pow receives the device's own log10(x), which
  the test looks up among these);
* `mpmath_version`.

Usage: python tests/golden/make_source_spectra_ulp_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "source_spectra_ulp.npz")
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import mpmath
    import source_spectra_cases as sc
    mpmath.mp.prec = 200

    def rounded(value):
        return float(mpmath.mpf(value, prec=53, rounding="n"))

    tt, x = sc.ulp_arguments()
    z = np.pi * tt                                          # one rounded product, as the kernel forms it
    exp_cr = np.array([rounded(mpmath.exp(mpmath.mpf(float(v)))) for v in z])
    log10_cr = np.array([rounded(mpmath.log10(mpmath.mpf(float(v)))) for v in x])
    pow_cr = np.empty((len(x), 2 * sc.ULP_NEIGHBOURS + 1))
    for k in range(-sc.ULP_NEIGHBOURS, sc.ULP_NEIGHBOURS + 1):
        y = sc.stepped(log10_cr, k)
        pow_cr[:, k + sc.ULP_NEIGHBOURS] = [rounded(mpmath.power(10, mpmath.mpf(float(v)))) for v in y]
    np.savez_compressed(OUT, exp_cr=exp_cr, log10_cr=log10_cr, pow_cr=pow_cr,
                        mpmath_version=np.array(mpmath.__version__))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
