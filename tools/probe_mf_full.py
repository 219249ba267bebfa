#!/usr/bin/env python3
"""What the matched filter's full normalisation (flag BPMF_MF_NORMALIZE_FULL) costs at the layout of BASELINE
configs[1]: 20 stations x 3 components, a day of 8 640 000 samples, templates of 256 samples, 500 templates.

  (a) the per-day preparation, short (bpmf_mf_prepare_data_dev) against full (bpmf_mf_prepare_data_full_dev): events
      around each call on the stream;
  (b) the main-kernel launches, short against full, on two workspaces that each hold their prepared day: the library's
      own event pair around the main kernel (bpmf_profile_*), and events around the whole bpmf_mf_run_dev call (in full
      mode it also centres the templates).  Both modes launch the SAME kernel on arrays of the same sizes: a difference
      beyond the spread of repeated identical runs would be a finding to explain;
  (c) the bytes the full-mode preparation moves beyond short mode's, over the 6.3 TB/s a stream gets from HBM.

The two modes ALTERNATE in one process; every figure is the median (min, max) of --calls measurements behind 3 warm-up
rounds, and `spread` is (max - min) / median of those repeated identical runs.

    python tools/probe_mf_full.py [--json] [--calls 30] [--templates 500] [--samples 8640000]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from seismic_bpmf_amd import _lib  # noqa: E402

HBM_STREAM_BYTES_PER_S = 6.3e12
FLAG_PREPARED, FLAG_FULL = 1, 4


def stats(xs):
    med = statistics.median(xs)
    return {"median_ms": med, "min_ms": min(xs), "max_ms": max(xs), "spread": (max(xs) - min(xs)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of text")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--templates", type=int, default=500)
    ap.add_argument("--samples", type=int, default=8_640_000)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: the median wants at least 20 calls")
    lib = _lib.lib()
    S, Cc, N, L, T = 20, 3, args.samples, 256, args.templates
    n_ch, n_corr = S * Cc, N - L + 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((S, Cc, N), generator=gen, dtype=torch.float32, device="cuda")
    data += torch.linspace(-50.0, 50.0, n_ch, device="cuda").reshape(S, Cc, 1)        # (full mode's use case: offsets)
    tp = torch.randn((T, S, Cc, L), generator=gen, dtype=torch.float32, device="cuda")
    mv = torch.randint(0, 1501, (T, S, Cc), generator=gen, dtype=torch.int32, device="cuda")
    w = torch.full((T, S, Cc), 1.0 / n_ch, dtype=torch.float32, device="cuda")
    out = torch.empty((T, n_corr), dtype=torch.float32, device="cuda")
    size = {"short": lib.bpmf_mf_workspace_bytes(L, N, T, S, Cc), "full": lib.bpmf_mf_full_workspace_bytes(L, N, T, S, Cc)}
    ws = {m: torch.empty(size[m], dtype=torch.uint8, device="cuda") for m in size}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prepare_fn = {"short": lib.bpmf_mf_prepare_data_dev, "full": lib.bpmf_mf_prepare_data_full_dev}

    def timed(f, what):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = f()
        b.record()
        _lib.check(rc, what)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def prepare(m):
        return timed(lambda: prepare_fn[m](data.data_ptr(), L, N, S, Cc, ws[m].data_ptr(), ws[m].numel(), stream),
                     f"prepare {m}")

    def run(m):
        flags = FLAG_PREPARED | (FLAG_FULL if m == "full" else 0)
        return timed(lambda: lib.bpmf_mf_run_dev(tp.data_ptr(), mv.data_ptr(), w.data_ptr(), data.data_ptr(), 1, L, N, T, S,
                                                 Cc, n_corr, 1, flags, ws[m].data_ptr(), ws[m].numel(), stream,
                                                 out.data_ptr()), f"run {m}")

    # (a) the preparations, alternating
    prep = {"short": [], "full": []}
    for i in range(args.calls + 3):
        for m in ("short", "full"):
            t = prepare(m)
            if i >= 3:
                prep[m].append(t)
    # (b) the launches on the two prepared days, alternating
    call = {"short": [], "full": []}
    kern = {"short": [], "full": []}
    for i in range(args.calls + 3):
        for m in ("short", "full"):
            _lib.profile_enable(True)
            t = run(m)
            _lib.profile_enable(False)
            k = _lib.profile_times_ms(_lib.KERNEL_MF_MAIN)
            assert len(k) == 1, k
            if i >= 3:
                call[m].append(t)
                kern[m].append(k[0])
    # (c) bytes: short reads d and writes the square prefix sums, then reads two of them per window and writes a norm;
    # full reads d twice (the mean, then the pass), writes d', two prefix arrays and the count, reads two of each per window
    nwin = n_corr
    moved = {"short": n_ch * (N * (4 + 8) + nwin * (2 * 8 + 4)),
             "full": n_ch * (N * (4 + 4 + 4 + 8 + 8 + 4) + nwin * (2 * (8 + 8 + 4) + 4))}
    added = moved["full"] - moved["short"]
    res = {"shape": {"stations": S, "components": Cc, "samples": N, "template_samples": L, "templates": T},
           "calls": args.calls, "workspace_bytes": size,
           "prepare": {m: stats(prep[m]) for m in prep}, "main_kernel": {m: stats(kern[m]) for m in kern},
           "run_dev_call": {m: stats(call[m]) for m in call},
           "prepare_bytes": moved, "prepare_added_bytes": added,
           "prepare_added_hbm_bound_ms": added / HBM_STREAM_BYTES_PER_S * 1e3}
    res["prepare_full_over_short"] = res["prepare"]["full"]["median_ms"] / res["prepare"]["short"]["median_ms"]
    res["prepare_added_ms"] = res["prepare"]["full"]["median_ms"] - res["prepare"]["short"]["median_ms"]
    res["main_kernel_full_over_short"] = res["main_kernel"]["full"]["median_ms"] / res["main_kernel"]["short"]["median_ms"]
    res["run_dev_call_full_minus_short_ms"] = res["run_dev_call"]["full"]["median_ms"] - res["run_dev_call"]["short"]["median_ms"]
    if args.json:
        print(json.dumps(res))
        return
    print(f"shape: {res['shape']}, medians of {args.calls} alternating calls (min, max; spread = (max - min) / median)")
    print(f"workspace bytes: short {size['short']}, full {size['full']}")
    for name in ("prepare", "main_kernel", "run_dev_call"):
        for m in ("short", "full"):
            s = res[name][m]
            print(f"{name:13s} {m:5s}: {s['median_ms']:9.3f} ms ({s['min_ms']:.3f}, {s['max_ms']:.3f}; spread {s['spread']:.4f})")
    print(f"prepare: full / short = {res['prepare_full_over_short']:.3f}, + {res['prepare_added_ms']:.3f} ms per day")
    print(f"main kernel: full / short = {res['main_kernel_full_over_short']:.4f}")
    print(f"run_dev call (full mode also centres the templates): full - short = {res['run_dev_call_full_minus_short_ms']:.3f} ms")
    print(f"prepare bytes: short {moved['short']}, full {moved['full']}; added {added} = "
          f"{res['prepare_added_hbm_bound_ms']:.3f} ms at {HBM_STREAM_BYTES_PER_S / 1e12:.1f} TB/s")


if __name__ == "__main__":
    main()
