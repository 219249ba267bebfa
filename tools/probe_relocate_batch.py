"""Event relocation, one call per event against one call per batch (workflow.relocate_events): cfg3 grid, windows of
N = 3000 samples taken from one resident synthetic day.  (a) the loop over workflow.relocation_likelihood -- the
(K, N) volume, its arg-max and the likelihood of one column per event, two host synchronisations each; (b)
relocate_events on the same windows, as `starts` into the day and as an explicit (E, S, C, N) batch.  src_idx,
time_idx and every likelihood row of (a) and (b) are compared before any time is printed; then the two are timed
alternately in this process, each to a device synchronise."""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
from seismic_bpmf_amd.workflow import relocate_events, relocation_likelihood

cfg = syn.BP_CONFIGS["cfg3"]
geo = syn.make_bp_geometry(cfg["grid"], cfg["S"], cfg["P"], cfg["sr"])
tau, ws = geo["moveouts"], geo["weights_sources"]
K, S, C = tau.shape[0], cfg["S"], cfg["C"]
wp = syn.phase_weights(S, C, cfg["P"])
N, N_DAY = 3000, 400_000
feat, _ = syn.make_bp_features(tau, S, C, N_DAY, sr=cfg["sr"], n_events=60)
day = torch.as_tensor(feat, device="cuda")
bf = BeamformerGPU(tau, ws)
print(f"cfg3: K={K} sources, {S} stations ({int((ws[0] != 0).sum())} weighted), N={N}, day of {N_DAY} samples; "
      f"plan {bf.plan_info()['n_groups']} groups")


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for E in (64, 512, 2500):
    starts = np.sort(np.random.default_rng(E).integers(0, N_DAY - N, E))
    batch = torch.stack([day[:, :, s:s + N] for s in starts])

    def loop():
        return [relocation_likelihood(bf, day[:, :, s:s + N], wp) for s in starts]

    def by_starts():
        return relocate_events(bf, day, wp, starts=starts, n_samples=N)

    def by_batch():
        return relocate_events(bf, batch, wp)

    # warm-up of both paths, and the check: equal results before any time is reported
    ref = loop()
    for name, fn in (("starts", by_starts), ("batch", by_batch)):
        res = fn()
        like = res["likelihood"]
        assert np.array_equal(res["src_idx"], [r[0] for r in ref]), name
        assert np.array_equal(res["time_idx"], [r[1] for r in ref]), name
        for e, r in enumerate(ref):
            assert np.array_equal(like[e].cpu().numpy(), r[2], equal_nan=True), (name, e)
        del res, like
    del ref
    print(f"E={E}: src_idx, time_idx and {E} likelihood rows of the loop and of relocate_events (starts, batch) are equal")
    t_loop, t_starts, t_batch = [], [], []
    for _ in range(2):
        t_loop.append(sync_time(loop)[0])
        t_starts.append(sync_time(by_starts)[0])
        t_batch.append(sync_time(by_batch)[0])
    a, b, c = min(t_loop) / E * 1e3, min(t_starts) / E * 1e3, min(t_batch) / E * 1e3
    print(f"E={E}: (a) loop over relocation_likelihood {a:.3f} ms/event"
          f" | (b) relocate_events, starts form {b:.3f} ms/event (x {a / b:.1f})"
          f" | (b) relocate_events, explicit batch {c:.3f} ms/event (x {a / c:.1f})"
          f"   [runs, ms/event: loop {[round(x / E * 1e3, 3) for x in t_loop]},"
          f" starts {[round(x / E * 1e3, 3) for x in t_starts]}, batch {[round(x / E * 1e3, 3) for x in t_batch]}]")
    del batch
    torch.cuda.empty_cache()
bf.close()
