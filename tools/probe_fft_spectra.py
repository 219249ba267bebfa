#!/usr/bin/env python3
"""The FFT-method spectra of a day's events (workflow.fft_spectra, csrc/fft_spectrum.hip) at the shape of a day:

    2500 events x 20 stations x 3 components x 3 windows (noise, P, S) of 1500 samples at 100 Hz, 25 log-spaced
    targets from 0.5 to 45 Hz (Spectrum.set_target_frequencies), Tukey taper of alpha = 0.05.

Three ways to the same numbers, the two device paths alternating in one process:

    fused      one workflow.fft_spectra call per window kind (E = 2500), and one call on the concatenated starts of
               the three (E = 7500): a DFT pruned to the ~50 bins next to a target, the day read once, no spectrum
               stored.  "kernels" is the entry point alone between two device events, its plan uploaded and its
               workspace allocated beforehand; "call" is the whole Python call on a host clock, synchronised;
    composed   the same result from existing pieces: a torch gather of the windows into float64, times the taper,
               torch.fft.rfft, times delta, abs, and np.interp's formula written in torch;
    host       postprocess.fft_spectrum_host (np.fft.rfft, np.interp) on --host-events events of the same box, per row.

The float64 rate is the useful work, rows x n x bins x 4 flop, over the kernels' time, against the nominal
78.6 TFLOP/s of the chip's float64 pipes.  Medians (min, max) of --calls behind --warmup calls.  The deviations are
in units of the allowance of tests/fft_spectrum_cases.py (sqrt(2) B delta + 8 * 2^-53 |want|); the worst err /
allowance of every case of the tests is listed too.  Nothing is asserted on time.

    python tools/probe_fft_spectra.py [--json] [--calls 30] [--warmup 3] [--events 2500] [--host-events 2]
                                      [--out profiles/fft_spectra.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, Cc, N_SAMPLES, SR = 20, 3, 1500, 100.0
DAY_SAMPLES = 8_640_000
WINDOW_OFFSETS = {"noise": -3000, "p": 0, "s": 1200}                  # samples from the event's start
NOMINAL_F64_TFLOPS = 78.6


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2500)
    ap.add_argument("--host-events", type=int, default=2)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import fft_spectrum_cases as fc
    from seismic_bpmf_amd import _lib, postprocess as pp, workflow
    assert torch.cuda.is_available(), "the probe needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(7)
    day = 1e-6 * torch.randn((S, Cc, DAY_SAMPLES), generator=gen, device="cuda") + 3e-5
    rng = np.random.default_rng(7)
    E = args.events
    origin = rng.integers(3000, DAY_SAMPLES - 3000 - N_SAMPLES, (E, 1)) + rng.integers(0, 800, (E, S))
    starts = {k: (origin + off).astype(np.int64) for k, off in WINDOW_OFFSETS.items()}
    starts["all three"] = np.concatenate([starts[k] for k in WINDOW_OFFSETS])
    frequencies = workflow.target_frequencies(0.5, 45.0, 25)
    plan = pp.fft_spectrum_plan(N_SAMPLES, SR, frequencies)
    K_b, F = len(plan["bins"]), len(frequencies)
    lib = _lib.lib()
    sync = torch.cuda.synchronize
    dev = {k: torch.as_tensor(np.ascontiguousarray(plan[k]), device="cuda")
           for k in ("taper", "bins", "pair", "dx", "span", "flags", "exact", "outside")}
    dev["twiddles"] = torch.as_tensor(np.array(pp.dft_twiddles(N_SAMPLES)), device="cuda")

    def fused(kind):
        return workflow.fft_spectra(day, starts[kind], N_SAMPLES, sr=SR, frequencies=frequencies)[0]

    def kernels_only(kind):
        """(call, out): the entry point alone on buffers made beforehand."""
        st = torch.as_tensor(starts[kind].reshape(-1), device="cuda")
        rows = st.numel() * Cc
        n_bytes = int(lib.bpmf_fft_spectrum_workspace_size(rows, N_SAMPLES, K_b, F))
        ws = torch.empty((n_bytes,), dtype=torch.uint8, device="cuda")
        out = torch.empty((st.numel(), Cc, F), dtype=torch.float64, device="cuda")
        valid = torch.empty((st.numel(),), dtype=torch.uint8, device="cuda")
        ptr = {k: C.c_void_p(v.data_ptr()) for k, v in dev.items()}

        def call():
            rc = lib.bpmf_fft_spectrum_dev(
                C.c_void_p(day.data_ptr()), S, Cc, DAY_SAMPLES, st.numel(), C.c_void_p(st.data_ptr()), N_SAMPLES,
                ptr["taper"], ptr["twiddles"], plan["delta"], ptr["bins"], K_b, ptr["pair"], ptr["dx"], ptr["span"],
                ptr["flags"], F, 0, C.c_void_p(ws.data_ptr()), n_bytes,
                C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(out.data_ptr()),
                C.c_void_p(valid.data_ptr()))
            _lib.check(rc, "bpmf_fft_spectrum_dev")
        return call, out, (st, ws, valid)

    lo_bin = torch.as_tensor(plan["bins"][plan["pair"]].astype(np.int64), device="cuda")
    offsets = torch.arange(N_SAMPLES, device="cuda")

    def composed(kind):
        st = torch.as_tensor(starts[kind], device="cuda")                               # (E, S)
        index = st[:, :, None, None] + offsets                                         # (E, S, 1, n)
        windows = torch.gather(day[None].expand(st.shape[0], -1, -1, -1), 3, index.expand(-1, -1, Cc, -1))
        spectrum = torch.fft.rfft(windows.double() * dev["taper"]) * plan["delta"]
        modulus = spectrum.abs()
        lo, hi = modulus[..., lo_bin], modulus[..., lo_bin + 1]
        out = torch.where(dev["exact"], lo, ((hi - lo) / dev["span"]) * dev["dx"] + lo)
        return torch.where(dev["outside"], torch.zeros_like(out), out)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        return a.elapsed_time(b)

    def clock_ms(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    report = {"shape": {"events": E, "stations": S, "components": Cc, "samples": N_SAMPLES, "targets": F, "bins": K_b,
                        "sr": SR, "calls": args.calls, "warmup": args.warmup}, "times": {}}
    for kind in list(WINDOW_OFFSETS) + ["all three"]:
        call, _, keep = kernels_only(kind)
        times = {"fused kernels": [], "fused call": [], "composed": []}
        for i in range(args.warmup + args.calls):                      # the paths alternate, call by call
            t = {"fused kernels": event_ms(call), "fused call": clock_ms(lambda: fused(kind)),
                 "composed": clock_ms(lambda: composed(kind))}
            if i >= args.warmup:
                for k, v in t.items():
                    times[k].append(v)
        rows = starts[kind].size * Cc
        entry = {k: summary(v) for k, v in times.items()}
        entry["rows"] = rows
        entry["tflops"] = rows * N_SAMPLES * K_b * 4.0 / (entry["fused kernels"]["median_ms"] * 1e-3) / 1e12
        report["times"][kind] = entry
        del keep
        torch.cuda.empty_cache()

    # the three against each other on the first events, in units of the allowance
    few = max(1, args.host_events)
    st = starts["p"][:few]
    windows = np.stack([np.stack([day[s, :, st[e, s]:st[e, s] + N_SAMPLES].cpu().numpy() for s in range(S)])
                        for e in range(few)])
    t0 = time.perf_counter()
    want, _ = pp.fft_spectrum_host(windows, sr=SR, frequencies=frequencies)
    host_ms = (time.perf_counter() - t0) * 1e3
    allow = fc.allowance(windows, plan["taper"], want)
    got = workflow.fft_spectra(day, st, N_SAMPLES, sr=SR, frequencies=frequencies)[0].cpu().numpy()
    starts["few"] = st
    other = composed("few").cpu().numpy()
    report["host"] = {"rows": int(windows[..., 0].size), "ms": host_ms, "ms_per_row": host_ms / windows[..., 0].size}
    report["deviation"] = {"fused vs host": fc.deviation(got, want, allow),
                           "composed vs host": fc.deviation(other, want, allow),
                           "smallest |value| / allowance": float((np.abs(want) / allow)[want != 0].min())}

    # every case of the tests
    cases = {}
    for index in range(len(fc.CASES)):
        n, key, _ = fc.CASES[index]
        x = fc.windows(index)
        d, s = fc.day_of(x)
        f = fc.targets(key, n)
        for multi in (False, True):
            w, _ = pp.fft_spectrum_host(x, sr=SR, frequencies=f, multi_component=multi)
            g = workflow.fft_spectra(torch.as_tensor(d, device="cuda"), s, n, sr=SR, frequencies=f,
                                     multi_component=multi)[0].cpu().numpy()
            cases[fc.label(index) + (" multi" if multi else "")] = fc.deviation(
                g, w, fc.allowance(x, pp.tukey_window(n, 0.05), w, multi))
    report["cases"] = cases

    lines = [f"FFT-method spectra: {E} events x {S} stations x {Cc} components, windows of {N_SAMPLES} samples at "
             f"{SR:g} Hz, {F} targets ({K_b} bins); medians (min, max) of {args.calls} calls behind {args.warmup}, "
             "the paths alternating call by call in one process", ""]
    for kind, entry in report["times"].items():
        lines.append(f"{kind}: {entry['rows']} rows")
        for k in ("fused kernels", "fused call", "composed"):
            v = entry[k]
            lines.append(f"    {k:14s} {v['median_ms']:9.3f} ms ({v['min_ms']:.3f}, {v['max_ms']:.3f})")
        lines.append(f"    float64 rate of the kernels: {entry['tflops']:.2f} TFLOP/s useful = "
                     f"{100 * entry['tflops'] / NOMINAL_F64_TFLOPS:.1f} % of the nominal {NOMINAL_F64_TFLOPS}; "
                     f"composed / fused call = {entry['composed']['median_ms'] / entry['fused call']['median_ms']:.2f}")
    h = report["host"]
    lines += ["", f"host definition: {h['rows']} rows in {h['ms']:.1f} ms = {h['ms_per_row']:.4f} ms per row "
                  f"({h['ms_per_row'] * report['times']['all three']['rows'] / 1e3:.1f} s for the rows of all three)",
              "", "worst err / allowance on the first events: " +
              ", ".join(f"{k} {v:.3e}" for k, v in report["deviation"].items()), "",
              "worst err / allowance of every case of tests/fft_spectrum_cases.py (device against the definition):"]
    lines += [f"    {k:34s} {v:.3e}" for k, v in cases.items()]
    text = "\n".join(lines)
    print(json.dumps(report) if args.json else text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
