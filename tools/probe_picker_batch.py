#!/usr/bin/env python3
"""The picker's surroundings for a day's events: 20 stations x 3 components, windows of 6000 samples (60 s at 100 Hz)
cut from a day of 8 640 000 samples and normalised in windows of 3000, 512 and 2500 events -- the device calls
(workflow.picker_batch: upload of the starts and nodes, one launch, the batch stays on the device; workflow.find_picks
on (E, S, 2, 6000) probabilities: one launch and the download of the pick tables) and their kernels alone (events
around the launches) against the host definitions on the same box (postprocess.picker_windows_host +
normalize_batch_host, find_picks_host: the reference's arithmetic bit for bit), timed at --host-events events and
reported per event -- ASSUMING the host side scales linearly with the events, which is what its per-event loop in the
reference does.  The normalisation streams: bytes written (E * S * C * n * 4) over the launch time is set against the
6.3 TB/s a stream gets from HBM.

The probabilities are synthetic (the model is out of scope): a P and an S bump per station over a noise floor.

    python tools/probe_picker_batch.py [--json] [--calls 30] [--host-events 64] [--events 512 2500]

Device figures: median (min, max) of --calls calls behind 3 warm-up calls, one process.  --host-events 0 skips the
host side."""
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


def timed(call, calls):
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def launch_ms(launch, calls):
    """The launch alone, between two events on the stream."""
    times = []
    for i in range(calls + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = launch()
        b.record()
        _lib.check(rc, "launch")
        torch.cuda.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b))
    return times


def synthetic_probabilities(E, S, n, seed):
    """(E, S, 2, n) float32 on the device: a P and an S bump per series over a floor of 0.02."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float32)
    centre = torch.rand((E, S, 2, 1), generator=gen, device="cuda") * (n - 800) + 400
    width = torch.rand((E, S, 2, 1), generator=gen, device="cuda") * 20 + 5
    amp = torch.rand((E, S, 2, 1), generator=gen, device="cuda") * 0.7 + 0.3
    floor = torch.rand((E, S, 2, n), generator=gen, device="cuda") * 0.02
    return (floor + amp * torch.exp(-0.5 * ((t - centre) / width) ** 2)).clamp_(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="print one JSON line per event count instead of text")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--host-events", type=int, default=64)
    ap.add_argument("--events", type=int, nargs="+", default=[512, 2500])
    ap.add_argument("--samples", type=int, default=8_640_000)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: the median wants at least 20 calls")
    S, Cc, N, n, W, overlap = 20, 3, args.samples, 6000, 3000, 0.5
    gen = torch.Generator(device="cuda").manual_seed(1)
    data_dev = torch.randn((S, Cc, N), generator=gen, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shift, n_windows = pp.normalize_batch_plan(n, W, overlap)
    nodes = torch.as_tensor(pp.normalize_batch_nodes(n, shift, n_windows), device="cuda")
    for E in args.events:
        rng = np.random.default_rng(E)
        starts = np.sort(rng.integers(0, N - n, E)).astype(np.int64)
        batch, t_batch = timed(lambda: workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W,
                                                             overlap=overlap), args.calls)
        d_start = torch.as_tensor(np.repeat(starts, S), device="cuda")
        k_batch = launch_ms(lambda: _lib.lib().bpmf_normalize_batch_dev(
            C.c_void_p(data_dev.data_ptr()), S, Cc, N, E * S, C.c_void_p(d_start.data_ptr()), n, W, shift,
            C.c_void_p(nodes.data_ptr()), n_windows, 0, stream, C.c_void_p(batch.data_ptr())), args.calls)
        written = E * S * Cc * n * 4
        del batch
        proba = synthetic_probabilities(E, S, n, E)
        picks, t_picks = timed(lambda: workflow.find_picks(proba, 0.3, 0.3), args.calls)
        outs = [torch.empty((E * S * 2,) + tail, dtype=dt, device="cuda") for tail, dt in
                (((), torch.int32), ((32,), torch.float32), ((32,), torch.float64), ((32,), torch.float64),
                 ((32,), torch.int32))]
        k_picks = launch_ms(lambda: _lib.lib().bpmf_find_picks_dev(
            C.c_void_p(proba.data_ptr()), E * S * 2, n, 0.3, 0.3, 32, stream,
            *(C.c_void_p(o.data_ptr()) for o in outs)), args.calls)
        res = {"shape": {"events": E, "stations": S, "components": Cc, "day_samples": N, "window_samples": n,
                         "normalization_window": W, "overlap": overlap},
               "calls": args.calls, "batch_bytes_written": written,
               "picker_batch_call_ms_median": statistics.median(t_batch), "picker_batch_call_ms_min": min(t_batch),
               "picker_batch_call_ms_max": max(t_batch), "normalize_launch_ms_median": statistics.median(k_batch),
               "normalize_launch_ms_min": min(k_batch), "normalize_launch_ms_max": max(k_batch),
               "find_picks_call_ms_median": statistics.median(t_picks), "find_picks_call_ms_min": min(t_picks),
               "find_picks_call_ms_max": max(t_picks), "find_picks_launch_ms_median": statistics.median(k_picks),
               "find_picks_launch_ms_min": min(k_picks), "find_picks_launch_ms_max": max(k_picks),
               "picks_found": int(picks["count"].sum())}
        res["normalize_launch_share_of_call"] = res["normalize_launch_ms_median"] / res["picker_batch_call_ms_median"]
        res["find_picks_launch_share_of_call"] = res["find_picks_launch_ms_median"] / res["find_picks_call_ms_median"]
        res["normalize_written_TB_per_s"] = written / (res["normalize_launch_ms_median"] * 1e-3) / 1e12
        res["normalize_written_over_hbm_stream"] = res["normalize_written_TB_per_s"] * 1e12 / HBM_STREAM_BYTES_PER_S
        res["device_ms_per_event"] = (res["picker_batch_call_ms_median"] + res["find_picks_call_ms_median"]) / E
        if args.host_events > 0:
            He = min(args.host_events, E)
            data = data_dev.cpu().numpy()
            t0 = time.perf_counter()
            want = pp.normalize_batch_host(pp.picker_windows_host(data, starts[:He], n).reshape(He * S, Cc, n), W,
                                           overlap).astype(np.float32)
            t_norm = (time.perf_counter() - t0) * 1e3
            del data
            host_proba = proba[:He].cpu().numpy()
            t0 = time.perf_counter()
            host_counts = np.array([[[len(pp.find_picks_host(host_proba[e, s, ph], 0.3)[0]) for ph in range(2)]
                                     for s in range(S)] for e in range(He)])
            t_find = (time.perf_counter() - t0) * 1e3
            got = workflow.picker_batch(data_dev, starts[:He], n, normalization_window_sample=W, overlap=overlap)
            res.update({"host_events": He, "host_normalize_ms_per_event": t_norm / He,
                        "host_find_picks_ms_per_event": t_find / He,
                        "host_ms_per_event": (t_norm + t_find) / He,
                        "identical": bool(np.array_equal(got.cpu().numpy().reshape(want.shape).view(np.uint32),
                                                         want.view(np.uint32)) and
                                          np.array_equal(host_counts, picks["count"][:He]))})
            res["host_over_device_per_event"] = res["host_ms_per_event"] / res["device_ms_per_event"]
            del got
        del proba
        if args.json:
            print(json.dumps(res))
        else:
            for k, v in res.items():
                print(f"{k}: {v}")
            print()


if __name__ == "__main__":
    main()
