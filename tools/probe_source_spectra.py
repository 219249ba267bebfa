#!/usr/bin/env python3
"""Propagation corrections, network-average spectra and Mw* of a day's events (workflow.source_spectra,
csrc/source_spectra.hip) at the shape of a day:

    2500 events x 20 stations x 25 log-spaced targets from 0.5 to 45 Hz, multi_component spectra (E, S, F), P and S.

Three ways to the same numbers on one box:

    device     workflow.source_spectra on spectra that lie in HBM (as fft_spectra leaves them): two calls per phase,
               the whole Python call on a host clock, synchronised; and each of the two calls alone;
    host       the NumPy definitions (postprocess.source_spectra_host, approximate_moment_magnitude_host) on all events;
    reference  where pandas is present: a reference-style loop per event -- a dict of per-station spectra, pandas
               Series for the distances, np.ma for the average -- restated here from the definitions' pieces on
               --loop-events events (the reference itself is not part of this repository), scaled to all events.

Medians (min, max) of --calls behind --warmup calls.  The worst err / allowance of the device against the definitions
(tests/source_spectra_cases.py) is listed for this shape too.  Nothing is asserted on time.

    python tools/probe_source_spectra.py [--calls 20] [--warmup 3] [--events 2500] [--loop-events 50]
                                         [--out profiles/source_spectra.txt]
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

S, F = 20, 25
THRESHOLD = 8.0


def summary(times):
    return f"median {statistics.median(times):9.3f} ms  (min {min(times):9.3f}, max {max(times):9.3f})"


def day_of_spectra(E, rng):
    f = np.logspace(np.log10(0.5), np.log10(45.0), F)
    plateau = 10.0 ** rng.uniform(-9.0, -6.0, size=(E, 1, 1))
    corner = rng.uniform(2.0, 15.0, size=(E, 1, 1))
    signal = plateau / (1.0 + (f / corner) ** 2) * np.exp(rng.normal(0.0, 0.4, size=(E, S, F)))
    noise = signal / np.exp(rng.normal(np.log(THRESHOLD), 1.0, size=(E, S, F)))
    dist = rng.uniform(5.0, 60.0, size=(E, S))
    return dict(frequencies=f, p=signal, s=1.3 * signal, noise=noise, dist=dist, epi=0.95 * dist, tt_p=dist / 6.0,
                tt_s=dist / 3.5, err=rng.uniform(0.2, 3.0, size=E), valid=rng.random((E, S)) < 0.95)


def reference_style_event(pd, pp, x, e, phase, k, which, q_rows, constants, medium):
    """One event as the reference walks it: dicts per station, pandas for the distances, np.ma for the average."""
    names = [f"ST{s:02d}" for s in range(S)]
    dist = pd.Series(x["dist"][e], index=names)
    epi = pd.Series(x["epi"][e], index=names)
    tt = pd.Series(x["tt_" + which[k]][e], index=names)
    spectra, snr = {}, {}
    for s, name in enumerate(names):
        if not x["valid"][e, s]:
            continue
        signal, noise = np.abs(x[phase][e, s]), np.abs(x["noise"][e, s])
        ratio = np.zeros(F)
        keep = ~((signal == 0) & (noise == 0))
        ratio[keep] = signal[keep] / noise[keep]
        value = x[phase][e, s] * (constants[k] * (1000.0 * dist.loc[name]) / (pp.RADIATION_P, pp.RADIATION_S)[k])
        value = value * np.exp(np.pi * tt.loc[name] * x["frequencies"] / q_rows[k])
        spectra[name], snr[name] = value, ratio
    keep = [n for n in spectra if not 100.0 * (x["err"][e] / dist.loc[n]) > 25.0]
    if keep:
        stack = np.ma.masked_array(np.stack([spectra[n] for n in keep]), np.stack([snr[n] < THRESHOLD for n in keep]))
        np.exp(np.ma.mean(np.ma.log10(stack), axis=0) * np.log(10.0))
        np.ma.std(np.ma.log10(stack), axis=0)
    table = pd.DataFrame({n: spectra[n] for n in spectra}, index=x["frequencies"])
    ratios = pd.DataFrame({n: snr[n] for n in snr}, index=x["frequencies"])
    measured = pd.Series(index=list(table.columns), dtype=np.float64)
    for name in measured.index:
        column = ratios.loc[:, name]
        bands = column.loc[column > THRESHOLD].index
        if len(bands):
            measured.loc[name] = table.loc[np.sort(bands)[:1], name].values[0]
        else:
            high = ratios.index > 2.0
            w, p = column.loc[high], table.loc[high, name]
            measured.loc[name] = 10.0 ** ((w * np.log10(p)).sum() / (w.sum() or 1.0))
    if len(epi):
        np.clip(epi, a_min=np.percentile(epi, 25.0), a_max=np.percentile(epi, 75.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2500)
    ap.add_argument("--loop-events", type=int, default=50)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import source_spectra_cases as sc
    from seismic_bpmf_amd import postprocess as pp, workflow
    assert torch.cuda.is_available(), "the probe needs a GPU"
    E = args.events
    x = day_of_spectra(E, np.random.default_rng(7))
    dev = {k: torch.as_tensor(x[k], device="cuda") for k in ("p", "s", "noise")}
    tables = dict(dist_km=x["dist"], tt_p_sec=x["tt_p"], tt_s_sec=x["tt_s"], location_err_km=x["err"],
                  frequencies=x["frequencies"], medium=sc.MEDIUM, q_phase_prefactor=sc.PREFACTOR)
    sync = torch.cuda.synchronize

    def both():
        return workflow.source_spectra(p=dev["p"], s=dev["s"], noise=dev["noise"], valid_p=x["valid"],
                                       valid_s=x["valid"], epicentral_dist_km=x["epi"], snr_threshold=THRESHOLD,
                                       **tables)

    def average(phase):
        return workflow.network_average_spectra(dev[phase], dev["noise"], phase=phase, valid=x["valid"],
                                                snr_threshold=THRESHOLD, **tables)

    first = average("p")

    def magnitude():
        return workflow.approximate_moment_magnitudes(first["corrected"], first["snr"], valid=x["valid"],
                                                      frequencies=x["frequencies"], epicentral_dist_km=x["epi"],
                                                      snr_threshold=THRESHOLD)

    def timed(fn):
        out = []
        for i in range(args.warmup + args.calls):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= args.warmup:
                out.append(1e3 * (time.perf_counter() - t0))
        return out

    lines = [f"source spectra: {E} events x {S} stations x {F} targets, multi_component, P + S; "
             f"{torch.cuda.get_device_name(0)}", ""]
    lines.append(f"device  source_spectra (P + S, 4 calls)        {summary(timed(both))}")
    lines.append(f"device  network_average_spectra (one phase)    {summary(timed(lambda: average('p')))}")
    lines.append(f"device  approximate_moment_magnitudes (one)    {summary(timed(magnitude))}")

    which, q_rows = pp.attenuation_plan(x["frequencies"], sc.MEDIUM, sc.PREFACTOR)
    constants = pp.geometry_constants(sc.MEDIUM)
    got = {ph: {k: v.cpu().numpy() for k, v in r.items()} for ph, r in both().items()}
    t0 = time.perf_counter()
    worst = {}
    for k, phase in enumerate(("p", "s")):
        want = pp.source_spectra_host(x[phase], x["noise"], x["valid"], None, x["dist"], x["tt_" + which[k]], x["err"],
                                      x["frequencies"], q_rows[k], constants[k], (pp.RADIATION_P, pp.RADIATION_S)[k],
                                      snr_threshold=THRESHOLD)
        want_mw = pp.approximate_moment_magnitude_host(want["corrected"], want["snr"], x["valid"], x["frequencies"],
                                                       x["epi"], snr_threshold=THRESHOLD)
        if k == 0:
            host_ms = 1e3 * (time.perf_counter() - t0)
        discrete, r_avg, r_std = sc.check_average(got[phase], want, (True, "mean", 0, 25.0))
        d2, r_disp, r_m0, r_mw = sc.check_mw(got[phase], want_mw, F)
        worst[phase] = (discrete and d2, r_avg, r_std, r_disp, r_m0, r_mw)
    lines.append(f"host    the NumPy definitions (one phase)          {host_ms:9.1f} ms")
    try:
        import pandas as pd
        n = min(args.loop_events, E)
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            for e in range(n):
                reference_style_event(pd, pp, x, e, "p", 0, which, q_rows, constants, sc.MEDIUM)
        per_event = 1e3 * (time.perf_counter() - t0) / n
        lines.append(f"loop    reference-style, per event (pandas {pd.__version__})  {per_event:9.3f} ms an event, "
                     f"{per_event * E:9.1f} ms for {E} (one phase, from {n} events)")
    except ImportError:
        lines.append("loop    reference-style: pandas is not installed")
    lines.append("")
    for phase, w in worst.items():
        lines.append(f"{phase}: discrete outputs equal: {w[0]}; worst err / allowance: average {w[1]:.3e}, std {w[2]:.3e}, "
                     f"measured_disp {w[3]:.3e}, log10_M0 {w[4]:.3e}, Mw_star {w[5]:.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(report + "\n")


if __name__ == "__main__":
    main()
