#!/usr/bin/env python3
"""Time the pair geometry on the device beside its host definitions and write profiles/template_geometry.txt:

  workflow.template_geometry at T = 2000, 5000 and 10 000 templates, workflow.template_pair_masks on its result, and
  workflow.compute_distances at K x R = 50 000 x 60 -- medians of 30 calls after 3 warm-up calls, each call timed by a
  host clock around the call and a device synchronise (so the host's projection and the uploads are inside) and by
  device events around the library call alone;
  postprocess.template_geometry_host / compute_distances_host on the same box (once each; the T^2 host loop is run up to
  --host-max templates, 5000 by default);
  the kernels' registers, scratch and occupancy as the compiler reports them (-Rpass-analysis=kernel-resource-usage).

Needs a GPU; without one it fails.  Usage: python tools/probe_template_geometry.py [--out FILE] [--host-max T]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, WARMUP = 30, 3


def templates(T, seed=1):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 1.5, (T, 3, 3))
    return (rng.uniform(-120.0, -118.0, T), rng.uniform(35.0, 37.0, T), rng.uniform(1.0, 25.0, T),
            a @ a.transpose(0, 2, 1), rng.random(T) < 0.8)


def timed(torch, call):
    """(median wall ms around call + synchronise, median device ms between events around the call)."""
    wall, dev = [], []
    for k in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            wall.append(1e3 * (time.perf_counter() - t0))
            dev.append(a.elapsed_time(b))
    return statistics.median(wall), statistics.median(dev), min(wall), max(wall)


def resource_usage():
    from seismic_bpmf_amd import build
    src = os.path.join(build.CSRC, "geometry.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.find_hipcc(), f"--offload-arch={build.ARCH}"] + [f for f in build.FLAGS if f != "-shared"] + \
              ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "geometry.o")]
        log = subprocess.run(cmd, capture_output=True, text=True).stderr
    lines, name = [], None
    for line in log.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = re.sub(r".*?(\d+)([a-z_]+_kernel).*", r"\2", m.group(1))
            lines.append([name])
        elif lines:
            lines[-1].append(f"{m.group(2)} {m.group(3)}")
    return ["  " + row[0] + ": " + ", ".join(row[1:]) for row in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_geometry.txt"))
    ap.add_argument("--host-max", type=int, default=5000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[2000, 5000, 10000])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("probe_template_geometry: no GPU")
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    out = [f"pair geometry (csrc/geometry.hip); device {torch.cuda.get_device_name(0)}; medians of {REPEATS} calls after "
           f"{WARMUP} warm-up calls; wall = host clock around the Python call and a synchronise, alone = device events around the library call on resident tables"]
    import ctypes as C
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for T in args.sizes:
        lon, lat, dep, cov, has = templates(T)
        wall, _, lo, hi = timed(torch, lambda: workflow.template_geometry(lon, lat, dep, cov, has))
        geo = workflow.template_geometry(lon, lat, dep, cov, has)
        # the library call alone, on tables that are already resident
        l32, a32, d32, xyz, c64, h = pp.template_geometry_arguments(lon, lat, dep, cov, has)
        d_geo = torch.as_tensor(workflow._geo_table(l32.astype(np.float64), a32.astype(np.float64), d32), device="cuda")
        d_xyz = torch.as_tensor(np.ascontiguousarray(xyz.T), device="cuda")
        d_cov = torch.as_tensor(np.ascontiguousarray(np.where(h[:, None, None], c64, 0.0).reshape(T, 9).T), device="cuda")
        d_has = torch.as_tensor(h.view(np.uint8), device="cuda")
        o = [torch.empty((T, T), dtype=torch.float32, device="cuda") for _ in range(3)]
        _, dev, _, _ = timed(torch, lambda: lib.bpmf_template_geometry_dev(ptr(d_geo), ptr(d_xyz), ptr(d_cov), ptr(d_has),
                                                                           T, stream(), ptr(o[0]), ptr(o[1]), ptr(o[2]), None))
        assert all(torch.equal(o[j], geo[k]) for j, k in enumerate(("intertemplate_dist", "dir_errors", "ellipsoid_dist")))
        mw, md, _, _ = timed(torch, lambda: workflow.template_pair_masks(geo["ellipsoid_dist"], distance_criterion=15.0,
                                                                         distance_threshold=5.0))
        line = (f"T={T}: template_geometry wall {wall:.3f} ms (min {lo:.3f}, max {hi:.3f}); bpmf_template_geometry_dev "
                f"alone {dev:.3f} ms = {T * T / (dev * 1e-3):.3g} pairs/s; template_pair_masks (both masks) wall "
                f"{mw:.3f} ms, between events {md:.3f} ms")
        del o
        if T <= args.host_max:
            t0 = time.perf_counter()
            host = pp.template_geometry_host(lon, lat, dep, cov, has)
            th = time.perf_counter() - t0
            same = {k: float((geo[k].cpu().numpy().view(np.int32) != host[k].view(np.int32)).mean()) for k in host}
            line += (f" | template_geometry_host {th:.2f} s = {1e3 * th / wall:.0f} x wall; elements that differ from "
                     f"the definition: " + ", ".join(f"{k} {v:.3%}" for k, v in same.items()))
        else:
            line += " | template_geometry_host: not run at this size"
        print(line, flush=True)
        out.append(line)
        del geo
    K, R = 50000, 60
    rng = np.random.default_rng(2)
    src = (rng.uniform(-120.0, -118.0, K), rng.uniform(35.0, 37.0, K), rng.uniform(0.0, 30.0, K))
    rcv = (rng.uniform(-120.0, -118.0, R), rng.uniform(35.0, 37.0, R), rng.uniform(-3.0, 0.0, R))
    wall, _, lo, hi = timed(torch, lambda: workflow.compute_distances(*src, *rcv, return_epicentral_distances=True))
    d_src = torch.as_tensor(workflow._geo_table(*src), device="cuda")
    d_rcv = torch.as_tensor(workflow._geo_table(*rcv), device="cuda")
    hypo, epi = (torch.empty((K, R), dtype=torch.float32, device="cuda") for _ in range(2))
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    _, dev, _, _ = timed(torch, lambda: lib.bpmf_geo_distances_dev(ptr(d_src), K, ptr(d_rcv), R, 1, stream(), ptr(hypo),
                                                                   ptr(epi), None, ptr(count)))
    t0 = time.perf_counter()
    pp.compute_distances_host(*src, *rcv, return_epicentral_distances=True)
    th = time.perf_counter() - t0
    line = (f"K x R = {K} x {R}: compute_distances (nonconverged='raise', reads the count) wall {wall:.3f} ms (min "
            f"{lo:.3f}, max {hi:.3f}); bpmf_geo_distances_dev alone {dev:.3f} ms = {K * R / (dev * 1e-3):.3g} pairs/s | "
            f"compute_distances_host {th:.2f} s = {1e3 * th / wall:.0f} x wall")
    print(line, flush=True)
    out.append(line)
    out.append("kernel resource use (-Rpass-analysis=kernel-resource-usage, gfx950):")
    out += resource_usage()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
