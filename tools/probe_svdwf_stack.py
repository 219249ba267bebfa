#!/usr/bin/env python3
"""The SVD-Wiener stack of a template's detections (workflow.svdwf_stack, csrc/svdwf.hip) at two workloads of
20 stations x 3 components:

    A: 100 groups x 100 events x 256 samples   (Gram matrix over the events, 100 x 100)
    B:  20 groups x 1000 events x 200 samples  (Gram matrix over the samples, 200 x 200)

with the reference's defaults (expl_var 0.4, five singular values, Wiener window = the group, band-pass 2-12 Hz at
25 Hz).  For each: the whole call (host clock around the call and a device synchronise; the workspace for all channels
allocated once outside), the host definition postprocess.svdwf_host per channel on the same box, timed on
--host-channels channels, and -- where BPMF_RECORD_REFERENCE names the reference tree and SciPy is installed --
utils.SVDWF per channel; the worst deviation of the device from the definition on those channels, in units of the
limits of tests/test_gpu_svdwf.py.  Nothing is asserted on time.

Kernel times come from a run of their own under the profiler, which this tool does not start:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/probe_svdwf_stack.py --calls 3 --host-channels 0

and `--kernel-stats <csv>` condenses the *_kernel_stats.csv it wrote (the sv_* kernels: calls, total and mean time).

    python tools/probe_svdwf_stack.py [--json] [--calls 20] [--host-channels 3] [--workloads A B]

Device figures: median (min, max) of --calls calls behind 2 warm-up calls, one process."""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"A": (100, 100, 256), "B": (20, 1000, 200)}           # groups, events per group, samples
S, C = 20, 3
SAMPLING_RATE, FREQMIN, FREQMAX = 25.0, 2.0, 12.0


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "sv_" in name:
                rows.append((name.split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6,
                             float(r["AverageNs"]) / 1e6))
    total = sum(r[2] for r in rows)
    for name, calls, ms, mean in sorted(rows, key=lambda r: -r[2]):
        print(f"{name}: calls {calls}, total {ms:.3f} ms ({100 * ms / total:.1f} %), mean {mean:.3f} ms")


def waveforms(G, n, m, seed):
    """(G n, S, C, m) float32 on the device: per channel two wavelets with random amplitudes per event, plus noise."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(m, device="cuda", dtype=torch.float32)
    w1 = torch.exp(-0.5 * ((t - 0.4 * m) / (0.03 * m + 1)) ** 2) * torch.cos(0.5 * t)
    w2 = torch.exp(-0.5 * ((t - 0.6 * m) / (0.05 * m + 1)) ** 2) * torch.sin(0.3 * t)
    a1 = torch.rand((G * n, S, C, 1), generator=gen, device="cuda") * 1.5 + 0.5
    a2 = torch.rand((G * n, S, C, 1), generator=gen, device="cuda") * 2 - 1
    return a1 * w1 + a2 * w2 + 0.3 * torch.randn((G * n, S, C, m), generator=gen, device="cuda")


def live_reference():
    ref = os.environ.get("BPMF_RECORD_REFERENCE")
    if not ref:
        return None
    try:
        import scipy  # noqa: F401
        spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(ROOT, "tests", "golden",
                                                                                   "make_goldens.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        mg.REF = ref
        cwd = os.getcwd()
        try:
            mg.import_reference()
        finally:
            os.chdir(cwd)
        from BPMF import utils
        return utils
    except Exception as e:  # noqa: BLE001
        print(f"reference not available: {e}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="print one JSON line per workload instead of text")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-channels", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["A", "B"], choices=sorted(WORKLOADS))
    ap.add_argument("--kernel-stats", help="condense a rocprofv3 *_kernel_stats.csv and exit")
    args = ap.parse_args()
    if args.kernel_stats is not None:
        return kernel_stats(args.kernel_stats)
    import torch
    from seismic_bpmf_amd import _lib, postprocess as pp, workflow
    sos = pp.butter_bandpass_sos(4, FREQMIN / (SAMPLING_RATE / 2), FREQMAX / (SAMPLING_RATE / 2))
    utils = live_reference() if args.host_channels > 0 else None
    for name in args.workloads:
        G, n, m = WORKLOADS[name]
        x = waveforms(G, n, m, G)
        off = np.arange(G + 1, dtype=np.int64) * n
        n_bytes = _lib.lib().bpmf_svdwf_workspace_bytes(G, n, m, G * S * C)
        ws = torch.empty((n_bytes,), dtype=torch.uint8, device="cuda")
        call = lambda: workflow.svdwf_stack(x, off, sos=sos, workspace=ws)  # noqa: E731
        for _ in range(2):
            out = call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        stack, filtered, rank, status = out
        res = {"workload": name, "shape": {"groups": G, "events_per_group": n, "stations": S, "components": C,
                                           "samples": m}, "channels": G * S * C, "calls": args.calls,
               "workspace_bytes": int(n_bytes), "call_ms_median": statistics.median(times), "call_ms_min": min(times),
               "call_ms_max": max(times), "not_converged": int((status != 0).sum()),
               "n_singular_histogram": np.bincount(rank.ravel(), minlength=9).tolist()}
        res["device_ms_per_channel"] = res["call_ms_median"] / (G * S * C)
        if args.host_channels > 0:
            picks = [(g, s, c) for g, s, c in ((0, 0, 0), (G - 1, S - 1, C - 1), (G // 2, S // 2, 1),
                                               (1, 3, 2), (G - 2, 7, 0))][:args.host_channels]
            t_host, t_ref, worst_f, worst_s = [], [], 0.0, 0.0
            for g, s, c in picks:
                a = x[off[g]:off[g + 1], s, c].cpu().numpy()
                t0 = time.perf_counter()
                hf, hs, hk = pp.svdwf_stack_host(a[:, None, None, :], sos=sos)
                t_host.append((time.perf_counter() - t0) * 1e3)
                df = np.abs(filtered[off[g]:off[g + 1], s, c].cpu().numpy() - hf[:, 0, 0]).max() / np.abs(hf).max()
                ds = np.abs(stack[g, s, c].cpu().numpy() - hs[0, 0, 0]).max() / np.abs(hs).max()
                worst_f, worst_s = max(worst_f, df * 2.0 ** 22), max(worst_s, ds * 2.0 ** 21)
                assert hk[0, 0, 0] == rank[g, s, c]
                if utils is not None:
                    t0 = time.perf_counter()
                    utils.SVDWF(a, freqmin=FREQMIN, freqmax=FREQMAX, sampling_rate=SAMPLING_RATE)
                    t_ref.append((time.perf_counter() - t0) * 1e3)
            res.update({"host_channels": len(picks), "host_definition_ms_per_channel": statistics.median(t_host),
                        "reference_ms_per_channel": statistics.median(t_ref) if t_ref else None,
                        "worst_filtered_in_units_of_2^-22": worst_f, "worst_stack_in_units_of_2^-21": worst_s})
            res["host_definition_over_device_per_channel"] = (res["host_definition_ms_per_channel"]
                                                              / res["device_ms_per_channel"])
        del x, ws, out, stack, filtered
        if args.json:
            print(json.dumps(res))
        else:
            for k, v in res.items():
                print(f"{k}: {v}")
            print()


if __name__ == "__main__":
    main()
