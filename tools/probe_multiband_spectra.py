#!/usr/bin/env python3
"""The multi-band spectra of a day's events (workflow.multiband_spectra, csrc/spectrum.hip) at the shape of a day:

    2500 events x 20 stations x 3 components x 3 windows (noise, P, S) of 1500 samples at 100 Hz, buffers of 2.5 s,
    eight octave bands from 0.39 Hz (the eighth, 49.92-99.84 Hz, lies beyond Nyquist and is skipped, as the reference
    skips it), corners = 4.

Three ways to the same numbers, alternating in one process:

    fused      one workflow.multiband_spectra call per window kind (E = 2500), and one call on the concatenated starts
               of the three (E = 7500); the day stays where it is, only the (E, S, C, B) maxima are stored;
    composed   what the library allowed before: the windows cut with torch indexing into a float64 tensor, mean, line
               and taper with torch operations, one workflow.bandpass_filter call per band (one thread per row over
               row-major memory, a full filtered tensor per band), abs, amax -- on --compose-events events, scaled
               per row;
    host       postprocess.multiband_spectrum_host on --host-events events of the same box, per row.

Times: a host clock around the call and a device synchronise; medians (min, max) of --calls behind --warmup calls.
The deviations among the three (fused, composed, host) on the first events are reported in the measure of
tests/multiband_cases.py:deviation -- they belong to THIS band set: the round-off of a cascade grows as its band
narrows, and these bands start lower (0.39 Hz) than those of the tests, whose limit is for their own.  Nothing is
asserted on time.

    python tools/probe_multiband_spectra.py [--json] [--calls 30] [--warmup 3] [--events 2500] [--compose-events 500]
                                            [--host-events 1] [--out profiles/multiband_spectra.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, C, N_SAMPLES, SR, BUFFER_SECONDS, CORNERS = 20, 3, 1500, 100.0, 2.5, 4
DAY_SAMPLES = 8_640_000
BANDS = {f"octave{k}": [0.39 * 2.0 ** k, 0.78 * 2.0 ** k] for k in range(8)}
WINDOW_OFFSETS = {"noise": -3000, "p": 0, "s": 1200}                  # samples from the event's start


def timed(fn, sync):
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2500)
    ap.add_argument("--compose-events", type=int, default=500)
    ap.add_argument("--host-events", type=int, default=1)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import multiband_cases as mc
    from seismic_bpmf_amd import postprocess as pp, workflow
    assert torch.cuda.is_available(), "the probe needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(7)
    day = 1e-6 * torch.randn((S, C, DAY_SAMPLES), generator=gen, device="cuda") + 3e-5
    rng = np.random.default_rng(7)
    E = args.events
    origin = rng.integers(3000, DAY_SAMPLES - 3000 - N_SAMPLES, (E, 1)) + rng.integers(0, 800, (E, S))
    starts = {k: (origin + off).astype(np.int64) for k, off in WINDOW_OFFSETS.items()}
    all_starts = np.concatenate([starts[k] for k in WINDOW_OFFSETS])
    plan = pp.multiband_plan(N_SAMPLES, BANDS, SR, BUFFER_SECONDS, CORNERS)
    live = np.flatnonzero(~plan["skip"])
    sync = torch.cuda.synchronize
    kw = dict(sr=SR, buffer_seconds=BUFFER_SECONDS, corners=CORNERS)

    def fused(st):
        return workflow.multiband_spectra(day, st, N_SAMPLES, BANDS, **kw)[0]

    Ec = min(args.compose_events, E)
    t_axis = torch.arange(N_SAMPLES, device="cuda", dtype=torch.float64) - (N_SAMPLES - 1) / 2.0
    taper = torch.ones(N_SAMPLES, device="cuda", dtype=torch.float64)
    w, buf = plan["taper"], plan["buffer"]
    side = 0.5 * (1.0 - torch.cos(torch.pi * torch.arange(w, device="cuda", dtype=torch.float64) / w))
    taper[:w], taper[N_SAMPLES - w:] = side, side.flip(0)
    d_starts_c = torch.as_tensor(starts["p"][:Ec], device="cuda")
    s_index = torch.arange(S, device="cuda")[None, :, None, None]
    c_index = torch.arange(C, device="cuda")[None, None, :, None]
    bandwidth = torch.as_tensor(plan["bandwidth"][live], device="cuda")

    def cut(d_st):
        return day[s_index, c_index, d_st[:, :, None, None] + torch.arange(N_SAMPLES, device="cuda")]

    def composed():
        x = cut(d_starts_c).double()                                  # (Ec, S, C, n) float64
        x = x - x.mean(dim=-1, keepdim=True)
        slope = (x * t_axis).sum(dim=-1, keepdim=True) / (t_axis * t_axis).sum()
        x = (x - (slope * t_axis + x.mean(dim=-1, keepdim=True))) * taper
        out = torch.zeros(x.shape[:-1] + (len(BANDS),), dtype=torch.float64, device="cuda")
        for i, b in enumerate(live):
            y = workflow.bandpass_filter(x, plan["sos"][b], detrend=False, taper_alpha=None)
            out[..., b] = y[..., buf:N_SAMPLES - buf].abs().amax(dim=-1) / bandwidth[i]
        return out

    calls = {"fused noise": lambda: fused(starts["noise"]), "fused p": lambda: fused(starts["p"]),
             "fused s": lambda: fused(starts["s"]), "fused three windows": lambda: fused(all_starts),
             "composed p": composed}
    times = {k: [] for k in calls}
    out = {}
    for i in range(args.warmup + args.calls):
        for k, fn in calls.items():                                   # alternating
            ms, out[k] = timed(fn, sync)
            if i >= args.warmup:
                times[k].append(ms)
    rows_window, rows_composed = E * S * C, Ec * S * C
    res = {"shape": {"events": E, "stations": S, "components": C, "windows": 3, "samples": N_SAMPLES,
                     "sampling_rate": SR, "buffer_seconds": BUFFER_SECONDS, "bands": len(BANDS),
                     "active_bands": int(len(live)), "corners": CORNERS},
           "calls": args.calls, "warmup": args.warmup, "workspace_bytes": workflow.MULTIBAND_WORKSPACE_BYTES,
           "rows_per_window": rows_window, "rows_composed": rows_composed}
    for k in calls:
        res[k] = summary(times[k])
    per_window = statistics.median([res[f"fused {k}"]["median_ms"] for k in WINDOW_OFFSETS])
    res["fused_ms_per_window"] = per_window
    res["fused_ms_per_event_three_windows"] = res["fused three windows"]["median_ms"] / E
    res["fused_us_per_row"] = 1e3 * per_window / rows_window
    res["fused_three_windows_us_per_row"] = 1e3 * res["fused three windows"]["median_ms"] / (3 * rows_window)
    res["composed_us_per_row"] = 1e3 * res["composed p"]["median_ms"] / rows_composed
    res["composed_over_fused_per_row"] = res["composed_us_per_row"] / res["fused_us_per_row"]
    res["composed_scaled_ms_per_window"] = res["composed_us_per_row"] * rows_window / 1e3

    # agreement on the first events: fused against composed, and against the definition on the host
    Ea = min(Ec, 20)
    Eh = min(args.host_events, Ea)
    got = out["fused p"].cpu().numpy()
    windows = cut(torch.as_tensor(starts["p"][:Ea], device="cuda")).cpu().numpy()
    prepared = pp.multiband_prepare_host(windows.reshape(-1, N_SAMPLES), w).reshape(windows.shape)
    scale = mc.row_scale(windows, prepared)
    res["fused_vs_composed_deviation"] = mc.deviation(got[:Ea], out["composed p"][:Ea].cpu().numpy(), scale, BANDS)
    if Eh > 0:
        t0 = time.perf_counter()
        want, _ = pp.multiband_spectrum_host(windows[:Eh], BANDS, **kw)
        host_ms = (time.perf_counter() - t0) * 1e3
        res["host_rows"] = Eh * S * C
        res["host_us_per_row"] = 1e3 * host_ms / (Eh * S * C)
        res["host_over_fused_per_row"] = res["host_us_per_row"] / res["fused_us_per_row"]
        res["fused_vs_host_deviation"] = mc.deviation(got[:Eh], want, scale[:Eh], BANDS)
        res["composed_vs_host_deviation"] = mc.deviation(out["composed p"][:Eh].cpu().numpy(), want, scale[:Eh], BANDS)
    text = json.dumps(res) if args.json else "\n".join(f"{k}: {v}" for k, v in res.items())
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
