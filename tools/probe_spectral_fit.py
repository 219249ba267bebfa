#!/usr/bin/env python3
"""Brune / Boatwright fits of a day's network-average spectra (workflow.fit_source_spectra, csrc/spectral_fit.hip) at the
shape of a day:

    2500 events x 25 log-spaced bins from 0.5 to 45 Hz, 0.15 decades of noise, P and S, sigmoid weights.

Three ways to the fits on one box:

    device     workflow.fit_source_spectra on averages that lie in HBM (as network_average_spectra leaves them), one
               call per phase, the Python call on a host clock and synchronised; and moment_magnitudes behind them;
    host       the NumPy definition (postprocess.fit_source_spectra_host) on --host-events events, scaled to all;
    SciPy      where SciPy is present: scipy.optimize.curve_fit with the reference's arguments (first guesses, bounds,
               sigma = 1 / w; BPMF/spectrum.py:794-824) on --host-events events, scaled to all, with the share of its
               fits whose cost exceeds the definition's by more than 1e-9.

Medians (min, max) of --calls behind --warmup calls.  The worst err / allowance of the device against the definition
(tests/spectral_fit_cases.py) is listed for this shape too.  Nothing is asserted on time.

    python tools/probe_spectral_fit.py [--calls 20] [--warmup 3] [--events 2500] [--host-events 200]
                                       [--out profiles/spectral_fit.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = 25


def summary(times):
    return f"median {statistics.median(times):9.3f} ms  (min {min(times):9.3f}, max {max(times):9.3f})"


def day_of_averages(E, model, rng):
    import spectral_fit_cases as sfc
    from seismic_bpmf_amd import postprocess as pp
    f = np.logspace(np.log10(0.5), np.log10(45.0), F)
    omega0, fc = 10.0 ** rng.uniform(11.0, 15.0, (E, 1)), np.exp(rng.uniform(np.log(1.5), np.log(15.0), (E, 1)))
    average = sfc.spectrum(f[None], omega0, fc, pp.FIT_MODELS[model]) * 10.0 ** (0.15 * rng.normal(size=(E, F)))
    return {"average": average, "mask": rng.random((E, F)) < 0.15, "num_valid": rng.integers(2, 25, (E, F)).astype(np.int32),
            "frequencies": f}


def scipy_fits(x, model, events):
    """curve_fit as the reference calls it; returns (seconds, costs)."""
    from scipy.optimize import curve_fit
    from seismic_bpmf_amd import postprocess as pp
    n = pp.FIT_MODELS[model]

    def log_model(freqs, omega0, fc):
        return np.log10(omega0) - (2.0 / n) * np.log10(1.0 + (freqs / fc) ** n)

    weights = pp.fit_weights(x["num_valid"], True)
    costs, start = np.full(events, np.nan), time.perf_counter()
    for e in range(events):
        keep = ~x["mask"][e]
        if keep.sum() / F < 0.5:
            continue
        xs, y, w = x["frequencies"][keep], np.log10(x["average"][e][keep]), weights[e][keep]
        fc0 = pp.fc_circular_crack(pp.moment_to_magnitude(x["average"][e][keep][0]))
        try:
            popt, _ = curve_fit(log_model, xs, y, p0=np.array([x["average"][e][keep][0], fc0]),
                                bounds=(np.array([0.0, 0.0]), np.array([np.inf, 1.0e3 * fc0])), sigma=1.0 / w)
        except (RuntimeError, ValueError):
            continue
        costs[e] = 0.5 * np.sum((w * (y - log_model(xs, *popt))) ** 2)
    return time.perf_counter() - start, costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2500)
    ap.add_argument("--host-events", type=int, default=200)
    ap.add_argument("--model", default="brune")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_fit.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_spectral_fit: needs a HIP device (nothing is timed without one)")
    import spectral_fit_cases as sfc
    import seismic_bpmf_amd as sb
    from seismic_bpmf_amd import postprocess as pp, workflow
    E, H = args.events, min(args.host_events, args.events)
    rng = np.random.default_rng(2500)
    days = {ph: day_of_averages(E, args.model, rng) for ph in ("p", "s")}
    dev = {ph: {k: torch.as_tensor(v, device="cuda") for k, v in x.items() if k != "frequencies"} for ph, x in days.items()}
    f = days["p"]["frequencies"]

    def device_call():
        fits = {ph: workflow.fit_source_spectra(d["average"], d["mask"], d["num_valid"], frequencies=f, phase=ph,
                                                model=args.model, weighted=True) for ph, d in dev.items()}
        return fits, workflow.moment_magnitudes(fits["p"], fits["s"])

    times = []
    for i in range(args.warmup + args.calls):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fits, mw = device_call()
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append(1000.0 * (time.perf_counter() - start))
    lines = [f"Brune / Boatwright fits at the shape of a day -- {sb.device_info(0)['name']}, model {args.model}, weighted",
             f"{E} events x {F} bins x 2 phases; {args.calls} calls behind {args.warmup}",
             "", f"device  fit_source_spectra (P, S) + moment_magnitudes, host clock, synchronised: {summary(times)}"]
    reasons = np.bincount(fits["p"]["reason"].cpu().numpy(), minlength=6)
    lines.append(f"        reasons of the P fits {dict(zip(pp.FIT_REASONS, reasons.tolist()))}; "
                 f"events with Mw {int((~torch.isnan(mw['Mw'])).sum())}")
    host_seconds, worst = 0.0, {}
    for ph, x in days.items():
        part = {k: (v[:H] if k != "frequencies" else v) for k, v in x.items()}
        start = time.perf_counter()
        want = pp.fit_source_spectra_host(part["average"], part["mask"], part["num_valid"], f, ph, model=args.model,
                                          weighted=True)
        host_seconds += time.perf_counter() - start
        got = {k: v[:H].cpu().numpy() for k, v in fits[ph].items()}
        discrete, ratios = sfc.check(got, want, part, args.model, True)
        worst[ph] = (discrete, ratios)
        days[ph]["want"] = want
    lines.append(f"host    the NumPy definition, {H} events per phase: {1000.0 * host_seconds / (2 * H):.3f} ms per fit, "
                 f"{host_seconds / (2 * H) * 2 * E:.2f} s scaled to {2 * E} fits")
    for ph, (discrete, ratios) in worst.items():
        lines.append(f"        device against it, phase {ph}: discrete outputs {'equal' if discrete else 'DIFFER'}; worst "
                     "err / allowance " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    try:
        seconds, above, fitted = 0.0, 0, 0
        for ph, x in days.items():
            t, costs = scipy_fits(x, args.model, H)
            seconds += t
            ok = np.isfinite(costs)
            fitted += int(ok.sum())
            above += int((costs[ok] > x["want"]["cost"][ok] * (1.0 + 1.0e-9)).sum())
        import scipy
        lines.append(f"SciPy   curve_fit {scipy.__version__} with the reference's arguments, {H} events per phase: "
                     f"{1000.0 * seconds / (2 * H):.3f} ms per fit, {seconds / (2 * H) * 2 * E:.2f} s scaled to {2 * E} "
                     f"fits; cost above the definition's by more than 1e-9 in {above} of {fitted} fits")
    except ImportError:
        lines.append("SciPy   not installed here: curve_fit not timed")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if os.path.exists(args.out) else "w") as out:
        out.write(text)


if __name__ == "__main__":
    main()
