"""GPU: workflow.compute_distances, template_geometry and template_pair_masks (bpmf_geo_distances_dev,
bpmf_template_geometry_dev, bpmf_pair_mask_dev; csrc/geometry.hip) against their host definitions, through the checks
of tests/geometry_cases.py -- whose docstring derives every tolerance, and which tests/test_template_geometry_definition.py
shows to be sharp against eleven planted defects:

  distances   K x R = 1 x 1, 1 x 300, 300 x 7, 257 x 3, both depth dtypes, with and without the optional outputs, and
              every named class of uncertainty_cases.geodesic_pairs.  float64 metres within 1e-9 km + 8 * 2^-53 d of the
              host's operations on the same tables; float32 outputs bit for bit the definition's two roundings of the
              device's own metres; regional case never more than 1 ulp from the whole definition, at most 2 % of the
              elements different; the fallback and the count of the pairs that do not converge; "raise" raises.
  geometry    T = 1, 2, 3, 65, 257: coincident templates, equal epicentres at different depths, mixed has_cov, zero and
              indefinite covariances, both depth units.  dir_errors bit for bit; ellipsoid_dist bit for bit from the
              device's own matrices; the diagonal of dist exactly 0.
  masks       both modes bit for bit, on the device's ellipsoid_dist, the golden's and a synthetic matrix, NaN included.
  plumbing    each entry point once between guard bands with junk in its outputs; flag_multiples and intertemplate_cc
              with a device mask against the host copy of it; every refusal, without a launch."""
import ctypes as C
import os

import numpy as np
import pytest

import geometry_cases as gc
import uncertainty_cases as uc
from arena import Arena

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


class Device:
    """The device entry points as a backend of geometry_cases."""

    def distances(self, src, rcv):
        import torch
        from seismic_bpmf_amd import workflow
        count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        hypo, epi, metres = workflow.compute_distances(*src, *rcv, return_epicentral_distances=True,
                                                       nonconverged="antipodal", return_metres=True, count_out=count)
        return hypo.cpu().numpy(), epi.cpu().numpy(), metres.cpu().numpy(), int(count.item())

    def geometry(self, case):
        from seismic_bpmf_amd import workflow
        got = workflow.template_geometry(case["longitude"], case["latitude"], case["depth"], case["cov_mat"],
                                         case["has_cov"], case["depth_unit"])
        return {k: v.cpu().numpy() for k, v in got.items()}

    def masks(self, ellipsoid, criterion, cc, similarity, threshold):
        import torch
        from seismic_bpmf_amd import workflow
        got = workflow.template_pair_masks(torch.as_tensor(ellipsoid, device="cuda"), distance_criterion=criterion,
                                           intertemplate_cc=cc, similarity_criterion=similarity,
                                           distance_threshold=threshold)
        assert got["pair_ok"].dtype == got["pair_mask"].dtype == torch.uint8
        ok, mask = got["pair_ok"].cpu().numpy(), got["pair_mask"].cpu().numpy()
        assert ok.max(initial=0) <= 1 and mask.max(initial=0) <= 1
        return ok.astype(bool), mask.astype(bool)


@pytest.fixture(scope="module")
def definitions():
    """{case name: template_geometry_host of it}, computed once."""
    return {c["name"]: gc.geometry_definition(c) for c in gc.template_cases()}


# -------------------------------------------------------------------------------------------- distances ---
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_distances_shapes(dtype):
    for name, src, rcv in gc.shape_cases(dtype):
        gc.check_distances(Device(), f"{name} {np.dtype(dtype).name}", src, rcv)
    gc.check_regional(Device(), dtype)


@pytest.mark.parametrize("case", gc.class_cases(), ids=lambda c: c[0])
def test_distances_named_class(case):
    gc.check_distances(Device(), *case)


def test_distances_without_the_optional_outputs_and_raise():
    from seismic_bpmf_amd import workflow
    name, src, rcv = gc.shape_cases(np.float32)[3]
    hypo, epi = workflow.compute_distances(*src, *rcv, return_epicentral_distances=True)
    alone = workflow.compute_distances(*src, *rcv)
    assert alone.shape == (257, 3) and alone.is_cuda
    assert np.array_equal(alone.cpu().numpy().view(np.int32), hypo.cpu().numpy().view(np.int32))
    _, _, metres = workflow.compute_distances(*src, *rcv, return_epicentral_distances=True, return_metres=True)
    want_hypo, want_epi = gc.pp.hypocentral_from_metres(metres.cpu().numpy(), src[2], rcv[2])
    assert np.array_equal(epi.cpu().numpy().view(np.int32), want_epi.view(np.int32))
    assert np.array_equal(hypo.cpu().numpy().view(np.int32), want_hypo.view(np.int32))
    name, src, rcv = next(c for c in gc.class_cases() if c[0] == uc.NOT_CONVERGENT)
    with pytest.raises(ValueError, match="convergence"):
        workflow.compute_distances(*src, *rcv)
    got = workflow.compute_distances(*src, *rcv, nonconverged="antipodal").cpu().numpy()
    assert np.isfinite(got).all()
    empty = workflow.compute_distances(*(x[:0] for x in src), *rcv)
    assert empty.shape == (0, rcv[0].size)


# ---------------------------------------------------------------------------------------------- geometry ---
@pytest.mark.parametrize("case", gc.template_cases(), ids=lambda c: c["name"])
def test_template_geometry(case, definitions):
    got = gc.check_geometry(Device(), case, definitions[case["name"]])
    # dist goes through the same device functions as compute_distances: the same bits
    lon, lat, dep = (np.float32(case[k]) for k in ("longitude", "latitude", "depth"))
    hypo, _, _, _ = Device().distances((lon, lat, dep), (lon, lat, dep))
    assert np.array_equal(got["intertemplate_dist"].view(np.int32), hypo.view(np.int32)), case["name"]
    if case["name"] in ("T65_reference", "T3_reference"):
        gc.check_masks(Device(), case["name"], *gc.mask_inputs(got["ellipsoid_dist"]))


def test_masks_on_the_golden_and_a_synthetic_matrix():
    gc.check_masks(Device(), "synthetic", *gc.synthetic_mask_case())
    with np.load(os.path.join(HERE, "golden", "template_geometry.npz")) as z:
        for g in range(int(z["n_groups"])):
            gc.check_masks(Device(), f"golden {g}", *gc.mask_inputs(z[f"ellipsoid_dist_{g}"], seed=g))
    # a host array is uploaded; one mask alone
    from seismic_bpmf_amd import workflow
    ell, cc = gc.synthetic_mask_case(T=3)
    got = workflow.template_pair_masks(ell, distance_threshold=5.0)
    assert list(got) == ["pair_mask"]
    assert np.array_equal(got["pair_mask"].cpu().numpy().astype(bool), gc.pp.intertemplate_pair_mask(ell, 5.0))


# ------------------------------------------------------------------------------- guard bands and plumbing ---
def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_in_arena(inputs, outputs, call):
    """The call between guard bands, outputs holding 0xFF junk; returns {output: value} after the guards held."""
    import torch
    arena = Arena()
    for name, value in inputs.items():
        arena.add_input(name, value)
    for name, (shape, dtype) in outputs.items():
        arena.add_output(name, shape, dtype)
    arena.commit()
    rc = call({r.name: C.c_void_p(r.ptr) for r in arena.regions})
    torch.cuda.synchronize()
    assert rc == 0
    assert arena.check() == []
    return {name: arena[name].value() for name in outputs}


def test_entry_points_between_guard_bands():
    import torch
    from seismic_bpmf_amd import _lib, workflow
    from seismic_bpmf_amd import postprocess as pp
    lib = _lib.lib()
    # distances, 65 x 3
    name, src, rcv = gc.regional_case(np.float64)
    src, rcv = tuple(x[:65] for x in src), tuple(x[:3] for x in rcv)
    got = _run_in_arena(
        {"src": workflow._geo_table(*src), "rcv": workflow._geo_table(*rcv)},
        {"hypo": ((65, 3), np.float32), "epi": ((65, 3), np.float32), "metres": ((65, 3), np.float64),
         "count": ((1,), np.int32)},
        lambda p: lib.bpmf_geo_distances_dev(p["src"], 65, p["rcv"], 3, 1, _stream(), p["hypo"], p["epi"], p["metres"],
                                             p["count"]))
    hypo, epi, metres = workflow.compute_distances(*src, *rcv, return_epicentral_distances=True, return_metres=True)
    assert got["count"][0] == 0
    assert np.array_equal(got["metres"], metres.cpu().numpy())
    assert np.array_equal(got["hypo"].view(np.int32), hypo.cpu().numpy().view(np.int32))
    assert np.array_equal(got["epi"].view(np.int32), epi.cpu().numpy().view(np.int32))
    # geometry, T = 65
    case = next(c for c in gc.template_cases() if c["name"] == "T65_reference")
    lon, lat, dep, xyz, cov, has = pp.template_geometry_arguments(case["longitude"], case["latitude"], case["depth"],
                                                                  case["cov_mat"], case["has_cov"])
    keys = ("intertemplate_dist", "dir_errors", "ellipsoid_dist")
    got = _run_in_arena(
        {"geo": workflow._geo_table(lon.astype(np.float64), lat.astype(np.float64), dep),
         "xyz": np.ascontiguousarray(xyz.T), "cov": np.ascontiguousarray(np.where(has[:, None, None], cov, 0.0).reshape(65, 9).T),
         "has": has.view(np.uint8)},
        {k: ((65, 65), np.float32) for k in keys},
        lambda p: lib.bpmf_template_geometry_dev(p["geo"], p["xyz"], p["cov"], p["has"], 65, _stream(),
                                                 p["intertemplate_dist"], p["dir_errors"], p["ellipsoid_dist"], None))
    want = Device().geometry(case)
    for k in keys:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    # masks, T = 65
    ell, cc = gc.mask_inputs(want["ellipsoid_dist"])
    for mode, crit, sim, with_cc in ((0, 15.0, 0.5, True), (0, 1.0, -1.0, False), (1, 5.0, -1.0, False)):
        got = _run_in_arena({"ell": ell, "cc": cc}, {"mask": ((65, 65), np.uint8)},
                            lambda p: lib.bpmf_pair_mask_dev(p["ell"], p["cc"] if with_cc else None, 65, mode, crit, sim,
                                                             _stream(), p["mask"]))
        want_mask = pp.multiples_pair_mask(ell, crit, cc, sim) if mode == 0 else pp.intertemplate_pair_mask(ell, crit)
        assert np.array_equal(got["mask"], want_mask.astype(np.uint8)), mode


def test_c_abi_refusals_launch_nothing():
    import torch
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    table = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    junk = lambda dtype: torch.full((4,), 77, dtype=dtype, device="cuda")
    f32, f64, i32, u8 = junk(torch.float32), junk(torch.float64), junk(torch.int32), junk(torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    refused = {
        "distances: null sources": lambda: lib.bpmf_geo_distances_dev(None, 2, p(table), 2, 0, _stream(), p(f32), None, None, p(i32)),
        "distances: null receivers": lambda: lib.bpmf_geo_distances_dev(p(table), 2, None, 2, 0, _stream(), p(f32), None, None, p(i32)),
        "distances: null output": lambda: lib.bpmf_geo_distances_dev(p(table), 2, p(table), 2, 0, _stream(), None, None, None, p(i32)),
        "distances: null count": lambda: lib.bpmf_geo_distances_dev(p(table), 2, p(table), 2, 0, _stream(), p(f32), None, None, None),
        "distances: K = 0": lambda: lib.bpmf_geo_distances_dev(p(table), 0, p(table), 2, 0, _stream(), p(f32), None, None, p(i32)),
        "distances: R = 0": lambda: lib.bpmf_geo_distances_dev(p(table), 2, p(table), 0, 0, _stream(), p(f32), None, None, p(i32)),
        "geometry: null geo": lambda: lib.bpmf_template_geometry_dev(None, p(table), None, None, 2, _stream(), p(f32), p(f32), p(f32), None),
        "geometry: null xyz": lambda: lib.bpmf_template_geometry_dev(p(table), None, None, None, 2, _stream(), p(f32), p(f32), p(f32), None),
        "geometry: null output": lambda: lib.bpmf_template_geometry_dev(p(table), p(table), None, None, 2, _stream(), p(f32), None, p(f32), None),
        "geometry: T = 0": lambda: lib.bpmf_template_geometry_dev(p(table), p(table), None, None, 0, _stream(), p(f32), p(f32), p(f32), None),
        "mask: null input": lambda: lib.bpmf_pair_mask_dev(None, None, 2, 0, 1.0, -1.0, _stream(), p(u8)),
        "mask: null output": lambda: lib.bpmf_pair_mask_dev(p(f32), None, 2, 0, 1.0, -1.0, _stream(), None),
        "mask: T = 0": lambda: lib.bpmf_pair_mask_dev(p(f32), None, 0, 0, 1.0, -1.0, _stream(), p(u8)),
        "mask: unknown mode": lambda: lib.bpmf_pair_mask_dev(p(f32), None, 2, 2, 1.0, -1.0, _stream(), p(u8)),
        "mask: cc in mode intertemplate": lambda: lib.bpmf_pair_mask_dev(p(f32), p(f32), 2, 1, 1.0, -1.0, _stream(), p(u8)),
    }
    for name, call in refused.items():
        rc = call()
        err = _lib.last_error()
        entry = {"distances": "bpmf_geo_distances_dev", "geometry": "bpmf_template_geometry_dev",
                 "mask": "bpmf_pair_mask_dev"}[name.split(":")[0]]
        assert rc == -1 and entry in err, (name, rc, err)
    torch.cuda.synchronize()
    for t in (f32, f64, i32, u8):
        assert (t == 77).all()


def test_python_refusals():
    import torch
    from seismic_bpmf_amd import workflow
    ell = torch.zeros((3, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        workflow.template_pair_masks(ell.double(), distance_criterion=1.0)
    with pytest.raises(ValueError):
        workflow.template_pair_masks(ell[:, :2], distance_criterion=1.0)
    with pytest.raises(ValueError):
        workflow.template_pair_masks(ell, distance_criterion=1.0, similarity_criterion=0.5,
                                     intertemplate_cc=np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        workflow.compute_distances([0.0], [0.0], [0.0], [1.0], [1.0], [0.0],
                                   count_out=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        workflow.flag_multiples([0.0, 1.0], [0, 1], [0.5, 0.6], torch.ones((2, 2), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        workflow.flag_multiples([0.0, 1.0], [0, 2], [0.5, 0.6], torch.ones((2, 2), dtype=torch.uint8, device="cuda"))


def test_device_masks_feed_flag_multiples_and_intertemplate_cc():
    import torch
    import guard_cases
    import multiples_cases as mc
    from seismic_bpmf_amd import workflow
    named = {c[0]: c for c in mc.named_cases()}
    for name in ("n2_multiples", "sliding_chain", "asymmetric", "false_diagonal"):
        _, t, rows, cc, ok, dt = named[name]
        want = workflow.flag_multiples(t, rows, cc, ok, dt)
        for dtype in (torch.uint8, torch.bool):
            got = workflow.flag_multiples(t, rows, cc, torch.as_tensor(ok, device="cuda").to(dtype), dt)
            assert np.array_equal(got, want), (name, dtype)
    # a mask made on the device from a device ellipsoid_dist, end to end
    case = next(c for c in gc.template_cases() if c["name"] == "T3_reference")
    geo = workflow.template_geometry(case["longitude"], case["latitude"], case["depth"], case["cov_mat"], case["has_cov"])
    masks = workflow.template_pair_masks(geo["ellipsoid_dist"], distance_criterion=-5.0, distance_threshold=-5.0)
    t, rows, cc = [0.0, 1.0, 2.0, 2.5], [0, 1, 2, 1], [0.4, 0.9, 0.5, 0.7]
    assert np.array_equal(workflow.flag_multiples(t, rows, cc, masks["pair_ok"], 4.0),
                          workflow.flag_multiples(t, rows, cc, masks["pair_ok"].cpu().numpy().astype(bool), 4.0))
    T, S, Cc, Lw, max_lag = guard_cases.INTERTP_SHAPES[0]
    wf, base, mask = guard_cases.intertp_inputs(T, S, Cc, Lw, 0)
    want = workflow.intertemplate_cc(wf, base, max_lag=max_lag, pair_mask=mask, symmetrise=False)
    for dtype in (torch.uint8, torch.bool):
        got = workflow.intertemplate_cc(wf, base, max_lag=max_lag, pair_mask=torch.as_tensor(mask, device="cuda").to(dtype),
                                        symmetrise=False)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), dtype
