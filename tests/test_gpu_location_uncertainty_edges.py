"""GPU: the location-uncertainty stage alone (csrc/bp_uncertainty.hip through BeamformerGPU.location_uncertainty,
no beamforming) against workflow.location_uncertainties_host on the same arrays, at the domain sizes, grid lengths
and geometries where its kernels change path.  The inputs are those of tests/uncertainty_cases.py; the conditions
they must meet, and the proof that the bit-equality below rejects a denominator summed in another order, are
asserted without a device in tests/test_location_uncertainty_edges_host.py.

Tolerances (derived, none measured).
  vunc of A / B: bit for bit.  Every weighted |dz| is exactly 2 and the float32 weights are multiples of 2^-24 in
    [0.5, 1): the float64 numerator sum w 2 is exact in any order (fewer than 2^17 multiples of 2^-23 below 2,
    17 + 1 + 24 bits < 53), so vunc = exact numerator / (double) float32 denominator equals the host's exactly if,
    and only if, the denominator is np.sum's float32.
  hunc of A / B: relative 4 K 2^-53 plus 1e-9 km, as in tests/test_gpu_location_uncertainty.py.
  C, one geodesic per event (a likelihood row that is 1 at one source, 0 elsewhere, on a side of 1e6 km):
    convergent pairs |hunc - d_host / 1000| <= 1e-9 km + 4 K 2^-53 d; pairs the iteration gives up on return
    pi (a + b) / 2 / 1000 from the host's own float64 operations, 2^-52 relative; vunc = |dz| exactly.
  Temporal: check_temporal of tests/test_gpu_location_uncertainty.py (1e-6 relative, no sample near the cut-off).
n_domain, the domain mask and the coordinates are exact everywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uncertainty_cases as uc  # noqa: E402
import test_gpu_location_uncertainty as base  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("hunc", "vunc", "longitude", "latitude", "depth")


def stage_plan(K, offset=0):
    """A plan that supplies only K and the id offset: a (K, 2, 2) moveout table of zeros, unit source weights."""
    from seismic_bpmf_amd import BeamformerGPU
    return BeamformerGPU(np.zeros((K, 2, 2), np.int32), np.ones((K, 2), np.float32), source_id_offset=offset)


def run_stage(bf, method, src_idx, **kw):
    """One call of the stage on device tensors; outputs handed in full of junk.  Returns the dict
    relocate_events(uncertainties=True) would: hunc, vunc, longitude, latitude, depth, n_domain (host arrays) and
    for "spatial" the (E, K) domain mask, all downloaded."""
    import torch
    dev, E = bf.device, len(src_idx)
    dv = {k: torch.as_tensor(v, device=dev) for k, v in kw.items() if k in ("likelihood", "maxbeam", "maxbeam_sources")}
    n_terms = bf.K if method == "spatial" else dv["maxbeam"].shape[1]
    out = torch.full((5, E), 12345.0, dtype=torch.float64, device=dev)
    n_dom = torch.full((E,), 12345, dtype=torch.int32, device=dev)
    work = torch.empty(bf.uncertainty_workspace_bytes(E, n_terms), dtype=torch.uint8, device=dev)
    opts = {k: v for k, v in kw.items() if k in ("side_km", "effective_kT", "gibbs_cutoff")}
    res = {"src_idx": np.asarray(src_idx, np.int64)}
    src = torch.as_tensor(res["src_idx"].astype(np.int32), device=dev)
    if method == "spatial":
        mask = torch.full((E, bf.K), 7, dtype=torch.uint8, device=dev)
        bf.location_uncertainty("spatial", E, 1, src, work, out, n_dom, likelihood=dv["likelihood"], domain_mask=mask,
                                **opts)
        res["likelihood"], res["domain"] = dv["likelihood"], mask.cpu().numpy()
        assert set(np.unique(res["domain"])) <= {0, 1}
    else:
        dv["max_beam"] = dv["maxbeam"].max(dim=1).values.contiguous()
        bf.location_uncertainty("temporal", E, n_terms, src, work, out, n_dom, **dv, **opts)
        res["maxbeam"], res["maxbeam_sources"] = dv["maxbeam"], dv["maxbeam_sources"]
    got = out.cpu().numpy()
    res.update({k: got[i] for i, k in enumerate(KEYS)})
    res["n_domain"] = n_dom.cpu().numpy().astype(np.int64)
    return res


def check_exact_vunc(res, host, plan, n, what):
    """The checks of one spatial call of A / B; returns the worst |d hunc| in km."""
    K = plan["lon"].shape[0]
    E = res["hunc"].shape[0]
    assert (res["n_domain"] == n).all() and np.array_equal(res["n_domain"], host["n_domain"]), (what, res["n_domain"])
    assert np.array_equal(res["domain"], host["domain"]), what
    for key, table in (("longitude", "lon"), ("latitude", "lat"), ("depth", "dep")):
        assert np.array_equal(res[key], np.full(E, plan[table][plan["event"]])), (what, key)
    assert np.array_equal(res["vunc"], host["vunc"], equal_nan=True), (what, res["vunc"], host["vunc"])
    assert np.isfinite(host["vunc"]).all() == (n > 1), what            # (n = 1: the event alone, weight 0: 0 / 0)
    assert base.close(res["hunc"], host["hunc"], 4 * K * 2.0 ** -53, 1e-9), (what, res["hunc"], host["hunc"])
    return float(np.nanmax(np.abs(res["hunc"] - host["hunc"]), initial=0.0))


def test_denominator_order_over_a_sweep_of_the_domain_size():
    """A.  K = 24 800 rows on one parallel, 97 workgroups; per size n one call of E = 4 events whose domain is the n
    rows of lowest rank, scattered over the workgroups.  vunc bit for bit: the float32 denominator takes NumPy's
    path at n < 8, n % 8 != 0, 128 / 129, the lengths 129 .. 144 whose first half is a 64-element leaf, 8192 / 8193,
    odd numbers of chunks and last chunks shorter than 8."""
    plan, like = uc.sweep_case()
    bf = stage_plan(uc.SWEEP_K)
    try:
        bf.set_source_coordinates(plan["lon"], plan["lat"], plan["dep"])
        src = np.full(uc.SWEEP_E, plan["event"])
        worst = 0.0
        for n in uc.SWEEP_SIZES:
            side = uc.side_for(plan, n)
            res = run_stage(bf, "spatial", src, likelihood=like, side_km=side)
            worst = max(worst, check_exact_vunc(res, uc.spatial_host(plan, like, side), plan, n, ("sweep", n)))
        print(f"A: {len(uc.SWEEP_SIZES)} calls x {uc.SWEEP_E} events, K = {uc.SWEEP_K}, vunc bit-equal in all; "
              f"worst |d hunc| = {worst:.3e} km; sizes swept:", list(uc.SWEEP_SIZES))
    finally:
        bf.close()


@pytest.mark.parametrize("K, blocks, seg", uc.LONG_GRIDS)
def test_spatial_grids_of_more_than_65536_sources(K, blocks, seg):
    """B.  More than 256 workgroups per event: the scan takes `seg` counts per thread (and at 547 workgroups its
    last threads none).  Domains of 1, 300, 65 537 and K scattered rows, and one whose members are the rows of the
    first and of the last, partly filled, workgroup alone."""
    plan = uc.parallel_plan(K, uc.LONG_SEED)
    like = uc.likelihood_rows(plan, uc.LONG_E, uc.LONG_SEED + 100)
    ends = uc.parallel_plan(K, uc.LONG_SEED + 1, first_and_last=True)
    like_ends = uc.likelihood_rows(ends, uc.LONG_E, uc.LONG_SEED + 101)
    bf = stage_plan(K)
    try:
        worst, sizes = 0.0, []
        for p, lk, ns in ((plan, like, (1, 300, 65_537, K)), (ends, like_ends, (ends["n_ends"],))):
            bf.set_source_coordinates(p["lon"], p["lat"], p["dep"])
            src = np.full(uc.LONG_E, p["event"])
            for n in ns:
                side = uc.side_for(p, n)
                res = run_stage(bf, "spatial", src, likelihood=lk, side_km=side)
                worst = max(worst, check_exact_vunc(res, uc.spatial_host(p, lk, side), p, n, (K, n)))
                sizes.append(n)
        inside = np.flatnonzero(res["domain"][0]) // 256
        assert set(inside) == {0, blocks - 1} and 0 < (inside == blocks - 1).sum() < 256
        print(f"B spatial: K = {K}, {blocks} workgroups, {seg} counts per thread of the scan, {len(sizes)} calls x "
              f"{uc.LONG_E} events, vunc bit-equal in all; worst |d hunc| = {worst:.3e} km; sizes:", sizes)
    finally:
        bf.close()


TEMPORAL_K, TEMPORAL_OFFSET = 864, 300


def temporal_plan():
    """The K = 864 grid of the existing file as a shard with source_id_offset = 300."""
    from seismic_bpmf_amd import BeamformerGPU
    tau, ws, _, coords = base.small_setup(5)
    assert tau.shape[0] == TEMPORAL_K
    bf = BeamformerGPU(tau, ws, source_id_offset=TEMPORAL_OFFSET)
    bf.set_source_coordinates(*coords)
    return bf, coords


@pytest.mark.parametrize("kT, cutoff, share", [(1.0, 0.25, 1.0), (0.33, 0.97, 0.01)])
def test_temporal_stream_of_more_than_65536_samples(kT, cutoff, share):
    """B.  N = 70 001 samples, 274 workgroups per event, with a cut-off that admits every sample and one that
    admits about 1 %."""
    E, N = 3, 70_001
    mb, ids, src = uc.temporal_stream(E, N, TEMPORAL_K, TEMPORAL_OFFSET, 23, kT, cutoff)
    bf, coords = temporal_plan()
    try:
        res = run_stage(bf, "temporal", src, maxbeam=mb, maxbeam_sources=ids, effective_kT=kT, gibbs_cutoff=cutoff)
        host = base.check_temporal(res, coords, TEMPORAL_K, ("temporal", N, kT, cutoff), offset=TEMPORAL_OFFSET,
                                   effective_kT=kT, gibbs_cutoff=cutoff)
        assert (np.abs(res["n_domain"] / N - share) <= 0.3 * share).all() and (res["n_domain"] <= N).all()
        assert (res["n_domain"] == N).all() == (share == 1.0)
        assert np.isfinite(res["hunc"]).all() and (res["hunc"] > 0).all() and (res["vunc"] > 0).all()
        print(f"B temporal: N = {N}, cut-off {cutoff} at kT {kT}, n_domain {res['n_domain'].tolist()}; worst "
              f"|d hunc| = {np.abs(res['hunc'] - host['hunc']).max():.3e} km")
    finally:
        bf.close()


def test_an_id_outside_the_plan_in_the_temporal_stream():
    """D.  An admitted sample whose maxbeam_sources is offset + K makes its event NaN (and is still counted); an id
    of offset - 1 at a sample below the cut-off changes nothing; every other event keeps the bits of the same call
    without the bad ids."""
    E, N, kT, cutoff = 4, 1500, 0.33, 0.25
    mb, ids, src = uc.temporal_stream(E, N, TEMPORAL_K, TEMPORAL_OFFSET, 24, kT, cutoff)
    top = mb.max(axis=1)
    t1 = (int(mb[1].argmax()) + 700) % N
    t2 = (int(mb[2].argmax()) + 700) % N
    mb[1, t1] = top[1] - np.float32(0.1)                   # weight exp(-0.1 / 0.33) = 0.74: admitted
    mb[2, t2] = top[2] - np.float32(1.0)                   # weight exp(-1 / 0.33) = 0.05: below the cut-off
    bad = ids.copy()
    bad[1, t1] = TEMPORAL_OFFSET + TEMPORAL_K
    bad[2, t2] = TEMPORAL_OFFSET - 1
    bf, coords = temporal_plan()
    try:
        kw = dict(maxbeam=mb, effective_kT=kT, gibbs_cutoff=cutoff)
        clean = run_stage(bf, "temporal", src, maxbeam_sources=ids, **kw)
        base.check_temporal(clean, coords, TEMPORAL_K, "clean ids", offset=TEMPORAL_OFFSET, effective_kT=kT,
                            gibbs_cutoff=cutoff)
        got = run_stage(bf, "temporal", src, maxbeam_sources=bad, **kw)
        assert np.isnan(got["hunc"][1]) and np.isnan(got["vunc"][1])
        assert np.array_equal(got["n_domain"], clean["n_domain"]) and got["n_domain"][1] > 1
        keep = [0, 2, 3]
        for k in KEYS:
            assert np.array_equal(got[k][keep], clean[k][keep]) and np.isfinite(clean[k]).all(), k
        for k in ("longitude", "latitude", "depth"):
            assert got[k][1] == clean[k][1]
        print("D: n_domain", got["n_domain"].tolist(), "hunc", got["hunc"].tolist())
    finally:
        bf.close()


def test_every_branch_of_the_geodesic_one_pair_per_event():
    """C.  Coincident points, the equator (sin alpha = +-1 exactly), the date line, meridians, the poles, pairs a
    nanodegree apart and astride the equator, regional to nearly antipodal lengths, and the pairs Vincenty's
    iteration gives up on after 200 rounds."""
    from seismic_bpmf_amd import postprocess as pp
    case = uc.geodesic_case()
    lon, lat, dep, s, d = case["lon"], case["lat"], case["dep"], case["src"], case["dst"]
    K, E = lon.shape[0], s.shape[0]
    bf = stage_plan(K)
    try:
        bf.set_source_coordinates(lon, lat, dep)
        res = run_stage(bf, "spatial", s, likelihood=case["likelihood"], side_km=1e6)
    finally:
        bf.close()
    assert (res["n_domain"] == K).all() and (res["domain"] == 1).all()
    assert np.array_equal(res["longitude"], lon[s]) and np.array_equal(res["latitude"], lat[s])
    assert np.array_equal(res["depth"], dep[s])
    assert np.array_equal(res["vunc"], np.abs(dep[s] - dep[d]))
    d_km = np.array([pp.geodesic_distance_m(lon[a], lat[a], lon[b], lat[b], nonconverged="antipodal")[0]
                     for a, b in zip(s, d)]) / 1000.0
    conv = case["cls"] != uc.NOT_CONVERGENT
    err = np.abs(res["hunc"] - d_km)
    for name in sorted(set(case["cls"])):
        m = case["cls"] == name
        print(f"C {name}: {int(m.sum())} events, lengths {d_km[m].min():.6g} .. {d_km[m].max():.6g} km, worst "
              f"|d hunc| = {err[m].max():.3e} km")
    print(f"C: {E} events on a plan of {K} points")
    assert np.isfinite(res["hunc"]).all()
    late = err > 1e-9 + 4 * K * 2.0 ** -53 * d_km
    assert not (late & conv).any(), [(case["cls"][e], lon[s[e]], lat[s[e]], lon[d[e]], lat[d[e]], res["hunc"][e],
                                      d_km[e]) for e in np.flatnonzero(late & conv)]
    fallback = np.pi * (pp.WGS84_A + (1.0 - pp.WGS84_F) * pp.WGS84_A) / 2.0 / 1000.0
    assert (d_km[~conv] == fallback).all()
    assert (np.abs(res["hunc"][~conv] - fallback) <= 2.0 ** -52 * fallback).all(), res["hunc"][~conv]
    # and the whole call against the host loop: the same lengths, masks and sizes
    from seismic_bpmf_amd.workflow import location_uncertainties_host
    host = location_uncertainties_host({"src_idx": s, "likelihood": case["likelihood"]}, lon, lat, dep, "spatial",
                                       restricted_domain_side_km=1e6)
    assert np.array_equal(host["hunc"], d_km) and np.array_equal(host["vunc"], res["vunc"])
    assert np.array_equal(host["n_domain"], res["n_domain"]) and np.array_equal(host["domain"], res["domain"])
