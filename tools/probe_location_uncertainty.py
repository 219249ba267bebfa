"""Location uncertainties of a batch of relocated events, on the host against on the device: cfg3 grid, windows of
N = 3000 samples taken from one resident synthetic day (the `starts` form), E = 512 and E = 2500.  Per event:
(a) the route without the device stage: workflow.relocate_events, then workflow.location_uncertainties_host -- the
    download of the (E, K) likelihood rows, the rectangular domain and the float64 Vincenty lengths in NumPy;
(b) relocate_events(uncertainties=True): the same, the last stage on the device (csrc/bp_uncertainty.hip);
(c) relocate_events alone (uncertainties=False: the launches of the call as it was before the stage existed).
n_domain of (a) and (b) must be equal and hunc / vunc within the tolerances of tests/test_gpu_location_uncertainty.py
before any time is printed.  (b) and (c) are timed alternately, each to a device synchronise; (a)'s host loop once.
The report goes to profiles/location_uncertainty.txt (--out), and to the terminal.

--kernels: only three calls of (b) at E = 512, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/probe_location_uncertainty.py --kernels)."""
import argparse, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
from seismic_bpmf_amd.workflow import location_uncertainties_host, relocate_events

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "location_uncertainty.txt"))
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--events", type=int, nargs="*", default=[512, 2500])
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


cfg = syn.BP_CONFIGS["cfg3"]
geo = syn.make_bp_geometry(cfg["grid"], cfg["S"], cfg["P"], cfg["sr"])
tau, ws = geo["moveouts"], geo["weights_sources"]
K, S, C = tau.shape[0], cfg["S"], cfg["C"]
coords = syn.geographic_coordinates(geo["sources"], (30.0, 40.0))
wp = syn.phase_weights(S, C, cfg["P"])
N, N_DAY, SIDE = 3000, 400_000, 100.0
feat, _ = syn.make_bp_features(tau, S, C, N_DAY, sr=cfg["sr"], n_events=60)
day = torch.as_tensor(feat, device="cuda")
bf = BeamformerGPU(tau, ws)
bf.set_source_coordinates(*coords)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if args.kernels:
    starts = np.sort(np.random.default_rng(512).integers(0, N_DAY - N, 512))
    for _ in range(3):
        relocate_events(bf, day, wp, starts=starts, n_samples=N, uncertainties=True, restricted_domain_side_km=SIDE)
    torch.cuda.synchronize()
    bf.close()
    sys.exit(0)

say(f"cfg3: K={K} sources on a {cfg['grid']} lattice over 100 km x 100 km, {S} stations, N={N}, day of {N_DAY} samples, "
    f"`starts` form, side {SIDE:g} km; device {torch.cuda.get_device_name(0)}")
for E in args.events:
    starts = np.sort(np.random.default_rng(E).integers(0, N_DAY - N, E))

    def alone():
        return relocate_events(bf, day, wp, starts=starts, n_samples=N)

    def on_device():
        return relocate_events(bf, day, wp, starts=starts, n_samples=N, uncertainties=True, restricted_domain_side_km=SIDE)

    def host_stage(res):
        return location_uncertainties_host(res, *coords, "spatial", restricted_domain_side_km=SIDE)

    res = on_device()                                                   # warm-up, and the check
    t_host, host = sync_time(lambda: host_stage(res))
    rel = 4 * K * 2.0 ** -53
    assert np.array_equal(res["n_domain"], host["n_domain"])
    assert (np.abs(res["vunc"] - host["vunc"]) <= rel * host["vunc"]).all()
    assert (np.abs(res["hunc"] - host["hunc"]) <= rel * host["hunc"] + 1e-9).all()
    say(f"E={E}: n_domain equal ({res['n_domain'].min()} to {res['n_domain'].max()} sources, median "
        f"{int(np.median(res['n_domain']))}); max |hunc - host| {np.abs(res['hunc'] - host['hunc']).max():.2e} km, "
        f"max |vunc - host| {np.abs(res['vunc'] - host['vunc']).max():.2e} km")
    del res, host
    alone()
    t_b, t_c = [], []
    for _ in range(3):
        t_c.append(sync_time(alone)[0])
        t_b.append(sync_time(on_device)[0])
    a, b, c = (min(t_c) + t_host) / E * 1e3, min(t_b) / E * 1e3, min(t_c) / E * 1e3
    say(f"E={E}: (a) relocate_events + host loop {a:.3f} ms/event (host stage {t_host / E * 1e3:.3f})"
        f" | (b) relocate_events(uncertainties=True) {b:.3f} ms/event"
        f" | (c) relocate_events alone {c:.3f} ms/event"
        f" | (a) / (b) = {a / b:.1f}, (b) / (c) = {b / c:.3f}, the stage (b) - (c) = {(b - c) * 1e3:.1f} us/event"
        f"   [runs, ms/event: (b) {[round(x / E * 1e3, 4) for x in t_b]}, (c) {[round(x / E * 1e3, 4) for x in t_c]}]")
    assert b < a and b <= 2.0 * c, "the device stage must not dominate the call it completes"
    torch.cuda.empty_cache()
bf.close()
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
