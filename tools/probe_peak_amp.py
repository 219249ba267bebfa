#!/usr/bin/env python3
"""Peak amplitudes of a day's detections at the shape of BASELINE configs[1]: 2500 detections of 500 templates,
20 stations x 3 components, windows of 300 samples in a day of 8 640 000 -- the device call
(workflow.peak_amplitudes: upload of the records and the moveout table, one launch, download of D * S * C floats)
against the host mirror (postprocess.peak_amplitudes_host, the reference's loop) on the same box.

    python tools/probe_peak_amp.py [--json] [--calls 30] [--host-runs 3] [--detections 2500] [--samples 8640000]

The device figure is the median of --calls calls behind 3 warm-up calls, a host clock around a call that ends in
the download.  --host-runs 0 skips the host mirror (a rocprofv3 --kernel-trace --stats run wants only the kernel)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from seismic_bpmf_amd import postprocess as pp, workflow  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of text")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--detections", type=int, default=2500)
    ap.add_argument("--samples", type=int, default=8_640_000)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: the median wants at least 20 calls")
    T, S, C, N, D = 500, 20, 3, args.samples, args.detections
    offset, duration = 100, 300                       # 1.0 s and 3.0 s at 100 Hz
    gen = torch.Generator(device="cuda").manual_seed(1)
    data_dev = torch.randn((S, C, N), generator=gen, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    rows = np.sort(rng.integers(0, T, D)).astype(np.int32)
    samples = rng.integers(0, N - 256, D).astype(np.int64)
    moveouts = rng.integers(0, 1501, (T, S, C)).astype(np.int32)
    data_norm = rng.uniform(0.5, 2.0, (S, C)).astype(np.float32)

    def call():
        return workflow.peak_amplitudes(data_dev, rows, samples, moveouts, offset=offset, duration=duration,
                                        data_norm=data_norm)
    for _ in range(3):
        got = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        got = call()
        times.append((time.perf_counter() - t0) * 1e3)
    res = {"shape": {"detections": D, "templates": T, "stations": S, "components": C, "samples": N,
                     "window": duration},
           "window_bytes": D * S * C * duration * 4, "calls": args.calls,
           "device_call_ms_median": statistics.median(times), "device_call_ms_min": min(times),
           "device_call_ms_max": max(times)}
    if args.host_runs > 0:
        data = data_dev.cpu().numpy()
        host = []
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            want = pp.peak_amplitudes_host(data, rows, samples, moveouts, offset, duration, data_norm)
            host.append((time.perf_counter() - t0) * 1e3)
        res["host_mirror_ms_median"] = statistics.median(host)
        res["host_runs"] = args.host_runs
        res["identical"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        res["host_over_device"] = res["host_mirror_ms_median"] / res["device_call_ms_median"]
    if args.json:
        print(json.dumps(res))
    else:
        for k, v in res.items():
            print(f"{k}: {v}")


if __name__ == "__main__":
    main()
