#!/usr/bin/env python3
"""Polyphase resampling in front of the picker at the tutorial's settings: a 25 Hz day of 20 stations x 3 components,
windows of 3000 samples (120 s) of 2500 events, up by 4 to the 100 Hz of the picker (12 000 samples a row, 150 000
rows).  Timed in one process, the three device figures ALTERNATING call by call so that clocks and neighbours on the
box touch them alike:

* the resampling kernel alone (bpmf_resample_poly_dev between two events on the stream, into a buffer kept);
* workflow.picker_batch(upsampling=4): upload of the starts, the tap table and the nodes, the resampling into a
  temporary, the normalisation of the 12 000-sample rows; the batch stays on the device;
* workflow.picker_batch without resampling on the same windows (3000-sample rows): what the call cost before;

and scipy.signal.resample_poly on the host of the same box for --host-rows of the same windows (skipped where SciPy is
not installed), whose answer the device must equal bit for bit.

    python tools/probe_resample_poly.py [--calls 20] [--events 2500] [--host-rows 60] [--out profiles/resample_poly.txt]

Medians (min, max) of --calls rounds behind 3 warm-up rounds.  The text goes to --out and to the standard output."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seismic_bpmf_amd import _lib, postprocess as pp, workflow  # noqa: E402


def wall_ms(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--events", type=int, default=2500)
    ap.add_argument("--host-rows", type=int, default=60)
    ap.add_argument("--samples", type=int, default=2_160_000, help="samples of the day (25 Hz)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_poly.txt"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: the median wants at least 20 rounds")
    S, Cc, N, n, up, down, W, overlap, E = 20, 3, args.samples, 3000, 4, 1, 3000, 0.5, args.events
    gen = torch.Generator(device="cuda").manual_seed(1)
    data_dev = torch.randn((S, Cc, N), generator=gen, dtype=torch.float32, device="cuda")
    starts = np.sort(np.random.default_rng(E).integers(0, N - n, E)).astype(np.int64)
    _, n_out, _, n_pre_remove, _, table = pp.resample_poly_plan(n, up, down)
    hp = len(table) // up
    d_start = torch.as_tensor(np.repeat(starts, S), device="cuda")
    d_table = torch.as_tensor(table, device="cuda")
    kept = torch.empty((E * S, Cc, n_out), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = _lib.lib().bpmf_resample_poly_dev(
            C.c_void_p(data_dev.data_ptr()), S, Cc, N, E * S, C.c_void_p(d_start.data_ptr()), n, up, down,
            C.c_void_p(d_table.data_ptr()), hp, n_pre_remove, n_out, stream, C.c_void_p(kept.data_ptr()))
        b.record()
        _lib.check(rc, "bpmf_resample_poly_dev")
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    times = {"kernel": [], "with": [], "without": []}
    for i in range(args.calls + 3):
        t_kernel = kernel()
        out, t_with = wall_ms(lambda: workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W,
                                                            overlap=overlap, upsampling=up, downsampling=down))
        del out
        out, t_without = wall_ms(lambda: workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W,
                                                               overlap=overlap))
        del out
        if i >= 3:
            times["kernel"].append(t_kernel)
            times["with"].append(t_with)
            times["without"].append(t_without)

    def line(name, t):
        return f"{name}: median {statistics.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f})"

    rows = E * S * Cc
    read_written = rows * (n + n_out) * 4
    k_med = statistics.median(times["kernel"]) * 1e-3
    text = [f"polyphase resampling up {up} down {down}: {E} events x {S} stations x {Cc} components, windows of {n} "
            f"samples of a day of {N} -> {rows} rows of {n_out} samples, {hp} taps per output",
            f"device: {torch.cuda.get_device_name()}; {args.calls} rounds behind 3 warm-up rounds, the three calls "
            "alternating",
            line("bpmf_resample_poly_dev, launch alone", times["kernel"]),
            f"  {rows * n_out * 4 / 1e9:.2f} GB written, {read_written / k_med / 1e12:.2f} TB/s read + written, "
            f"{2 * hp * rows * n_out / k_med / 1e12:.2f} Tflop/s of rounded multiplies and adds",
            line("workflow.picker_batch(upsampling=4), the call", times["with"]),
            line("workflow.picker_batch without resampling (rows of 3000), the call", times["without"])]
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
        text.append("scipy.signal.resample_poly: SciPy is not installed on this box")
    if resample_poly is not None and args.host_rows > 0:
        k = min(args.host_rows, E * S * Cc)
        events = -(-k // (S * Cc))
        windows = pp.picker_windows_host(data_dev.cpu().numpy(), starts[:events], n).reshape(-1, n)[:k]
        host = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            want = resample_poly(windows, up, down, axis=-1)
            host.append((time.perf_counter() - t0) * 1e3)
        got = workflow.resample_poly(torch.as_tensor(windows, device="cuda"), up, down).cpu().numpy()
        same = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        same &= bool(np.array_equal(kept.view(-1, n_out)[:k].cpu().numpy().view(np.uint32), want.view(np.uint32)))
        text.append(line(f"scipy.signal.resample_poly on the host, {k} rows of {n}", host))
        text.append(f"  per row: host {statistics.median(host) / k * 1e3:.1f} us, kernel {k_med / rows * 1e9:.1f} ns; "
                    f"device and SciPy identical bit for bit: {same}")
    text = "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
