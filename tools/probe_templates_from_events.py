#!/usr/bin/env python3
"""Templates of a day's located events at the channel layout of BASELINE configs[1]: 20 stations x 3 components,
windows of 256 samples (and noise windows of 500 for the SNR) cut from a day of 8 640 000 samples, 500 and 2500
events -- the device call (workflow.templates_from_events: upload of origins and moveouts, one launch, download of the
flags, norms and SNRs; the templates stay on the device) and its kernel alone (events around the launch of
bpmf_templates_from_events_dev) against the definition's NumPy code on the host of the same box
(postprocess.templates_from_events_host), and against the bytes moved -- windows read and templates written,
2 * E * S * C * L * 4, plus the noise windows -- over the 6.3 TB/s a stream gets from HBM.

    python tools/probe_templates_from_events.py [--json] [--calls 30] [--host-runs 3] [--events 500 2500]

Device figures: median (min, max) of --calls calls behind 3 warm-up calls.  --host-runs 0 skips the host side."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from seismic_bpmf_amd import _lib, postprocess as pp, workflow  # noqa: E402

HBM_STREAM_BYTES_PER_S = 6.3e12


def kernel_ms(data_dev, origin, moveouts, L, noise_offset, noise_samples, calls):
    """The launch alone, between two events on the stream (the entry point's check of the origins -- a copy of 8 E
    bytes and a synchronisation -- lies before the first event's kernel and is part of the figure)."""
    S, Cc, N = (int(v) for v in data_dev.shape)
    E = len(origin)
    d_origin, d_mv = torch.as_tensor(origin, device="cuda"), torch.as_tensor(moveouts, device="cuda")
    tp = torch.empty((E, S, Cc, L), dtype=torch.float32, device="cuda")
    norm = torch.empty((E, S, Cc), dtype=torch.float32, device="cuda")
    snr = torch.empty((E, S, Cc), dtype=torch.float32, device="cuda")
    flags = torch.empty((E, S, Cc), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for i in range(calls + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = _lib.lib().bpmf_templates_from_events_dev(
            C.c_void_p(data_dev.data_ptr()), S, Cc, N, E, C.c_void_p(d_origin.data_ptr()), C.c_void_p(d_mv.data_ptr()),
            L, 1, noise_offset, noise_samples, stream, C.c_void_p(tp.data_ptr()), C.c_void_p(norm.data_ptr()),
            C.c_void_p(flags.data_ptr()), C.c_void_p(snr.data_ptr()))
        b.record()
        _lib.check(rc, "bpmf_templates_from_events_dev")
        torch.cuda.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="print one JSON line per event count instead of text")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--events", type=int, nargs="+", default=[500, 2500])
    ap.add_argument("--samples", type=int, default=8_640_000)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: the median wants at least 20 calls")
    S, Cc, N, L = 20, 3, args.samples, 256
    noise_offset, noise_samples = 600, 500            # 5 s of noise ending 1 s before the origin, at 100 Hz
    gen = torch.Generator(device="cuda").manual_seed(1)
    data_dev = torch.randn((S, Cc, N), generator=gen, dtype=torch.float32, device="cuda")
    data = data_dev.cpu().numpy() if args.host_runs > 0 else None
    for E in args.events:
        rng = np.random.default_rng(E)
        origin = np.sort(rng.integers(1000, N - 4000, E)).astype(np.int64)
        moveouts = rng.integers(-100, 1501, (E, S, Cc)).astype(np.int32)

        def call():
            return workflow.templates_from_events(data_dev, origin, moveouts, L, noise_offset=noise_offset,
                                                  noise_samples=noise_samples)
        for _ in range(3):
            got = call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        kern = kernel_ms(data_dev, origin, moveouts, L, noise_offset, noise_samples, args.calls)
        moved = 2 * E * S * Cc * L * 4 + E * S * Cc * noise_samples * 4
        res = {"shape": {"events": E, "stations": S, "components": Cc, "samples": N, "window": L,
                         "noise_window": noise_samples},
               "bytes_moved": moved, "hbm_bound_ms": moved / HBM_STREAM_BYTES_PER_S * 1e3, "calls": args.calls,
               "device_call_ms_median": statistics.median(times), "device_call_ms_min": min(times),
               "device_call_ms_max": max(times), "launch_ms_median": statistics.median(kern),
               "launch_ms_min": min(kern), "launch_ms_max": max(kern)}
        res["launch_over_hbm_bound"] = res["launch_ms_median"] / res["hbm_bound_ms"]
        if args.host_runs > 0:
            host = []
            for _ in range(args.host_runs):
                t0 = time.perf_counter()
                want = pp.templates_from_events_host(data, origin, moveouts, L, "rms", noise_offset, noise_samples)
                host.append((time.perf_counter() - t0) * 1e3)
            res["host_definition_ms_median"] = statistics.median(host)
            res["host_runs"] = args.host_runs
            tp = got["templates"].cpu().numpy()
            res["identical"] = bool(np.array_equal(tp.view(np.uint32), want["templates"].view(np.uint32)) and
                                    np.array_equal(got["norm"].view(np.uint32), want["norm"].view(np.uint32)) and
                                    np.array_equal(got["snr"].view(np.uint32), want["snr"].view(np.uint32)) and
                                    np.array_equal(got["available"], want["available"]) and
                                    np.array_equal(got["complete"], want["complete"]))
            res["host_over_device"] = res["host_definition_ms_median"] / res["device_call_ms_median"]
        if args.json:
            print(json.dumps(res))
        else:
            for k, v in res.items():
                print(f"{k}: {v}")
            print()


if __name__ == "__main__":
    main()
