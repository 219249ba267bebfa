#!/usr/bin/env python3
"""Time the multiples flagging (workflow.flag_multiples, csrc/multiples.hip) beside its host definition
(postprocess.flag_multiples): 20 000 and 10^6 events at T = 500 and 5000 templates, as one sparse day (events in small
clusters all over 86 400 s: many short segments) and as one swarm (no gap of dt_criterion: ONE segment, walked by one
wave).  Per case: the host definition, the whole workflow call (stable sort, uploads, the library call, scatter) and
the library call alone on arrays already on the device (span kernel + flag kernel + its one synchronisation), each the
median of `--repeats` runs after one warm-up; the results are compared first.  Writes profiles/flag_multiples.txt.

Usage: python tools/probe_flag_multiples.py [--out FILE] [--repeats 3] [--small]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def catalog(kind, n, T, rng, dt):
    if kind == "sparse day":
        centres = rng.uniform(0.0, 86400.0, max(1, n // 4))
        t = centres[rng.integers(0, len(centres), n)] + rng.exponential(0.5 * dt, n)
    else:                                        # swarm: mean gap dt / 40, the largest gap far below dt
        t = np.cumsum(rng.uniform(0.0, dt / 20.0, n))
    ok = rng.random((T, T)) < 0.2
    ok |= ok.T
    np.fill_diagonal(ok, True)
    return t, rng.integers(0, T, n), rng.random(n).astype(np.float32), ok


def median_ms(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flag_multiples.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="20 000 events only")
    args = ap.parse_args()
    import torch
    from seismic_bpmf_amd import _lib, postprocess as pp, workflow
    dt = 4.0
    lines = [f"flag_multiples on {torch.cuda.get_device_name(0)}; dt_criterion {dt} s; ms, median of {args.repeats}",
             f"{'catalog':<11} {'events':>8} {'T':>5} {'flagged':>8} {'segments':>9} {'host def.':>10} {'workflow':>9} "
             f"{'library':>8}"]
    print("\n".join(lines), flush=True)
    rng = np.random.default_rng(1)
    lib = _lib.lib()
    for kind in ("sparse day", "swarm"):
        for n in (20_000,) if args.small else (20_000, 1_000_000):
            for T in (500, 5000):
                t, rows, cc, ok = catalog(kind, n, T, rng, dt)
                t0 = time.perf_counter()
                want = pp.flag_multiples(t, rows, cc, ok, dt)
                host_ms = (time.perf_counter() - t0) * 1e3               # (one run: seconds at 10^6 events)
                got = workflow.flag_multiples(t, rows, cc, ok, dt)
                assert np.array_equal(got, want), (kind, n, T)
                call_ms = median_ms(lambda: workflow.flag_multiples(t, rows, cc, ok, dt), args.repeats)
                order = np.argsort(t, kind="stable")
                ts = t[order]
                d = [torch.as_tensor(a, device="cuda") for a in (ts, rows[order].astype(np.int32), cc[order],
                                                                  ok.view(np.uint8))]
                ws = torch.empty(lib.bpmf_flag_multiples_workspace_bytes(n), dtype=torch.uint8, device="cuda")
                out = torch.empty(n, dtype=torch.uint8, device="cuda")
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def library():
                    rc = lib.bpmf_flag_multiples_dev(C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()),
                                                     C.c_void_p(d[2].data_ptr()), n, C.c_void_p(d[3].data_ptr()), T, dt,
                                                     C.c_void_p(ws.data_ptr()), ws.numel(), stream,
                                                     C.c_void_p(out.data_ptr()))
                    _lib.check(rc, "bpmf_flag_multiples_dev")
                lib_ms = median_ms(library, args.repeats)
                segments = 1 + int((~(np.diff(ts) < dt)).sum())
                lines.append(f"{kind:<11} {n:>8} {T:>5} {int((~want).sum()):>8} {segments:>9} {host_ms:>10.1f} "
                             f"{call_ms:>9.2f} {lib_ms:>8.2f}")
                print(lines[-1], flush=True)
    lines.append("host def. = postprocess.flag_multiples (NumPy loop, one run); workflow = workflow.flag_multiples from "
                 "host arrays; library = bpmf_flag_multiples_dev on device arrays (both kernels and its synchronisation).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
