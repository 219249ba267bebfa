"""GPU: every backprojection kernel family on features that hold NaN, +Inf and -Inf, judged by the written rule of
tests/bp_nonfinite_cases.py (float64 classes, exact floors and +Inf maxima, finite beams inside their bounds) and by
bit-equality with the oracle, NaN positions included.

The shapes are those of tests/test_gpu_f64_anchor.py -- the smallest at which each family is selected, asserted with
plan_info() -- planted with isolated bad samples on the seams of every tile, a +Inf and a -Inf that meet in one beam, a
zero phase weight over a NaN, a NaN gap over every station and a NaN-filled station.  The session runs with
debug.poison_output on (tests/conftest.py): an element no kernel writes shows as NaN or -1 where the rule says +0 or
(0, id_offset).  Every check prints its class counts (pytest -rP shows them)."""
import ctypes as C

import numpy as np
import pytest

import bp_nonfinite_cases as bn

pytestmark = pytest.mark.gpu

OOBS = ("strict", "flexible")


def _oracle(oracle_lib, case, oob, reduce, fc=False):
    with oracle_lib.compat(oracle_lib.COMPAT_FIRST_COMPUTED if fc else 0):
        return oracle_lib.beamform(*case.args, oob, reduce)


def _counts(x):
    c = bn.classify(x)
    return [int((c == k).sum()) for k in range(4)]


def _family(oracle_lib, label, shape, expect=None, with_beam=True, fc=False, id_offset=0):
    """One family on one shape: both regimes, strict and flexible, reduce="max" (and "none")."""
    from seismic_bpmf_amd import BeamformerGPU
    for regime in bn.REGIMES:
        case = bn.case(shape, regime)
        f, tau, wp, ws = case.args
        bf = BeamformerGPU(tau, ws, source_id_offset=id_offset)
        try:
            if expect is not None:
                expect(bf.plan_info())
            for oob in OOBS:
                r = bn.refs(shape, regime, oob)
                r.require()
                what = f"{label}: {r.name}" + (" first_computed" if fc else "")
                m, a = (x.cpu().numpy() for x in bf.run(f, wp, "max", oob))
                print(f"bp-nonfinite {what}: max-beam finite / NaN / +Inf / -Inf {_counts(m)}, floors "
                      f"{int(((m == 0) & (a == id_offset)).sum())}")
                bn.check_max(m, a, r, fc, oracle=_oracle(oracle_lib, case, oob, "max", fc), id_offset=id_offset, what=what)
                if with_beam:
                    beam = bf.run(f, wp, "none", oob).cpu().numpy()
                    print(f"bp-nonfinite {what}: beams finite / NaN / +Inf / -Inf {_counts(beam)}")
                    bn.check_none(beam, r, oracle=_oracle(oracle_lib, case, oob, "none"), what=what + " reduce=none")
        finally:
            bf.close()


# ------------------------------------------------------------------------------------ the kernel families ---
@pytest.mark.parametrize("tile", [512, 256, 128])
@pytest.mark.parametrize("uniform", [True, False])
def test_fast_classes(oracle_lib, hip_opts, tile, uniform):
    hip_opts("bp.fast_tile", tile)

    def expect(info):
        assert info["n_classes"] == 1 and info["class_tile"][0] == tile, info

    _family(oracle_lib, f"fast tile {tile}", "fast uniform" if uniform else "fast per-station", expect, with_beam=False)


def test_multi_residency_class(oracle_lib, hip_opts):
    hip_opts("bp.halves", 1)
    hip_opts("bp.fast_tile", 256)

    def expect(info):
        assert info["n_classes"] == 1 and info["class_tile"][0] == 256 and info["gather_bytes"] == 8, info

    _family(oracle_lib, "multi-residency", "multi-residency", expect, with_beam=False)


@pytest.mark.parametrize("shape", ["fast per-station", "wide moveouts"])
def test_general_kernels_alone(oracle_lib, hip_opts, shape):
    hip_opts("bp.fast", 0)

    def expect(info):
        assert info["n_classes"] == 0 and info["n_groups"] >= 1, info

    _family(oracle_lib, "bp.fast=0", shape, expect)


def test_direct_kernel(oracle_lib, hip_opts):
    hip_opts("bp.direct", 1)

    def expect(info):
        assert info["n_groups"] == 0 and info["n_classes"] == 0 and info["tile"] == 1024, info

    _family(oracle_lib, "bp.direct=1", "fast per-station", expect)


def test_grid_without_an_lds_plan(oracle_lib):
    def expect(info):
        assert info["n_groups"] == 0, info

    _family(oracle_lib, "no LDS plan", "no-LDS grid", expect)


@pytest.mark.parametrize("shape", ["default", "two stations"])
def test_default_plan_and_full_beams(oracle_lib, shape):
    _family(oracle_lib, "default plan", shape)


@pytest.mark.parametrize("shape", ["default", "fast per-station"])
def test_first_computed_scan(oracle_lib, hip_opts, shape):
    hip_opts("bp.compat_first_computed", 1)
    _family(oracle_lib, "bp.compat_first_computed", shape, with_beam=False, fc=True)


def test_floor_names_the_source_id_offset(oracle_lib, hip_opts):
    _family(oracle_lib, "source_id_offset=1000", "default", with_beam=False, id_offset=1000)
    hip_opts("bp.compat_first_computed", 1)
    _family(oracle_lib, "source_id_offset=1000", "default", with_beam=False, fc=True, id_offset=1000)


def test_split_rows_merge_to_the_same_bits(oracle_lib, hip_opts):
    """bp.split 1 and 3: a sample's maximum does not depend on which split row met the NaN first."""
    from seismic_bpmf_amd import BeamformerGPU
    for regime in bn.REGIMES:
        case = bn.case("fast per-station", regime)
        f, tau, wp, ws = case.args
        for oob in OOBS:
            want = _oracle(oracle_lib, case, oob, "max")
            for split in (1, 3):
                hip_opts("bp.split", split)
                bf = BeamformerGPU(tau, ws)
                try:
                    m, a = (x.cpu().numpy() for x in bf.run(f, wp, "max", oob))
                finally:
                    bf.close()
                    hip_opts.reset("bp.split")
                assert np.array_equal(m, want[0]) and np.array_equal(a, want[1]), (regime, oob, split)
            bn.check_max(m, a, bn.refs("fast per-station", regime, oob), what=f"bp.split: {case.name} {oob}")


def test_host_pointer_call_in_pieces(oracle_lib, hip_opts):
    """beamform(..., device="gpu") with the day uploaded in more than one piece."""
    from seismic_bpmf_amd import beamform
    hip_opts("bp.host_piece_samples", 1024)
    for shape in ("fast per-station", "default"):
        case = bn.case(shape, "signed")
        for oob in OOBS:
            r = bn.refs(shape, "signed", oob)
            m, a = beamform(*case.args, device="gpu", out_of_bounds=oob, device_id=0)
            bn.check_max(m, a, r, oracle=_oracle(oracle_lib, case, oob, "max"), what=f"host pieces: {r.name}")
            if shape == "default":
                beam = beamform(*case.args, device="gpu", out_of_bounds=oob, reduce="none", device_id=0)
                bn.check_none(beam, r, oracle=_oracle(oracle_lib, case, oob, "none"), what=f"host pieces: {r.name}")


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("fc", [False, True])
def test_virtual_devices_merge_to_the_one_device_result(oracle_lib, hip_opts, k, fc):
    """The per-device maxima travel through the packed keys (-Inf floors under first_computed included): the merged
    result does not depend on which device met the NaN, and equals the one-device result bit for bit."""
    from seismic_bpmf_amd import beamform
    hip_opts("bp.compat_first_computed", int(fc))
    runs = [(regime, oob) for regime in bn.REGIMES for oob in OOBS]
    one = {(regime, oob): beamform(*bn.case("default", regime).args, device="gpu", out_of_bounds=oob, device_id=0)
           for regime, oob in runs}
    hip_opts("debug.virtual_devices", k)
    for regime, oob in runs:
        case = bn.case("default", regime)
        multi = beamform(*case.args, device="gpu", out_of_bounds=oob, device_id=None)
        assert np.array_equal(multi[0], one[regime, oob][0]) and np.array_equal(multi[1], one[regime, oob][1]), (regime, oob)
        bn.check_max(*multi, bn.refs("default", regime, oob), fc, oracle=_oracle(oracle_lib, case, oob, "max", fc),
                     what=f"{k} virtual devices: {case.name} {oob} first_computed={fc}")


# ----------------------------------------------------------------------------------------- packed keys ---
def _total_order(x):
    """uint32 whose unsigned order is the total order of float32 (-Inf < ... < -0 < +0 < ... < +Inf)."""
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


@pytest.mark.parametrize("as_signed", [0, 1])
def test_packed_keys_round_trip_and_order(as_signed):
    import torch
    from seismic_bpmf_amd import _lib, parallel
    fmax, den = np.finfo(np.float32).max, np.float32(1e-45)
    vals = np.array([0.0, -0.0, den, -den, 1.0, -1.0, fmax, -fmax, np.inf, -np.inf], dtype=np.float32)
    args = np.array([0, 1, 2 ** 31 - 1], dtype=np.int32)
    beam, arg = (np.ascontiguousarray(x.ravel()) for x in np.meshgrid(vals, args, indexing="ij"))
    n = beam.size
    d_beam, d_arg = torch.as_tensor(beam, device="cuda"), torch.as_tensor(arg, device="cuda")
    packed = torch.empty(n, dtype=torch.int64, device="cuda")
    b2, a2 = torch.empty_like(d_beam), torch.empty_like(d_arg)
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.bpmf_bp_pack_max_dev(d_beam.data_ptr(), d_arg.data_ptr(), n, as_signed, stream, packed.data_ptr()),
               "bpmf_bp_pack_max_dev")
    _lib.check(lib.bpmf_bp_unpack_max_dev(packed.data_ptr(), n, as_signed, stream, b2.data_ptr(), a2.data_ptr()),
               "bpmf_bp_unpack_max_dev")
    assert np.array_equal(b2.cpu().numpy().view(np.uint32), beam.view(np.uint32)) and np.array_equal(a2.cpu().numpy(), arg)
    keys = packed.cpu().numpy()
    keys = keys if as_signed else keys.view(np.uint64)
    # the key order is "larger beam, then lower arg": every pair compared
    # (64-bit unsigned range: Python integers)
    rank = _total_order(beam).astype(object) * 2 ** 32 + (2 ** 32 - 1 - arg.astype(object))
    assert np.array_equal(keys[:, None] > keys[None, :], rank[:, None] > rank[None, :])
    assert np.unique(keys).size == n
    if as_signed:
        assert np.array_equal(parallel.pack_max_keys(d_beam, d_arg).cpu().numpy(), keys)
        pb, pa = parallel.unpack_max_keys(packed)
        assert np.array_equal(pb.cpu().numpy().view(np.uint32), beam.view(np.uint32)) and np.array_equal(pa.cpu().numpy(), arg)


# ------------------------------------------------------------------------------------------ relocation ---
def _judge_events(oracle_lib, res, per_event, f, tau, wp, ws, oob, method, what):
    from seismic_bpmf_amd import postprocess as pp
    for e in range(f.shape[0]):
        w = (what, e)
        vol = oracle_lib.beamform(f[e], tau, wp, ws, oob, "none")
        wm, wa = oracle_lib.beamform(f[e], tau, wp, ws, oob, "max")
        if method == "temporal":
            mb, ma = res["maxbeam"][e].cpu().numpy(), res["maxbeam_sources"][e].cpu().numpy()
            assert not np.isnan(mb).any(), w
            assert np.array_equal(mb, wm) and np.array_equal(ma, wa), w
            ti = int(mb.argmax())
            assert (res["time_idx"][e], res["src_idx"][e], res["max_beam"][e]) == (ti, ma[ti], mb[ti]), w
            src, t1, mbeam = per_event[e]
            assert (src, t1) == (res["src_idx"][e], res["time_idx"][e]) and np.array_equal(mbeam, mb), w
            continue
        src, ti, M = pp.focus_from_max(wm, wa)                       # rule 3 on the max-beams
        if not M > 0:
            src, ti = bn.focus_of_volume(vol)                        # (redone on its volume)
        assert (res["src_idx"][e], res["time_idx"][e]) == (src, ti), w
        col = res["columns"][e].cpu().numpy()
        assert np.array_equal(col, vol[:, ti], equal_nan=True), w    # rule 2: the oracle's column, NaNs in place
        with np.errstate(invalid="ignore"):
            want = pp.likelihood(vol[:, ti])
        like = res["likelihood"][e].cpu().numpy()
        assert np.array_equal(like, want, equal_nan=True), w
        if np.isnan(col).any():
            assert np.isnan(like).all(), w
        elif col.max() == np.inf:
            assert np.array_equal(np.isnan(like), np.isinf(col)) and not like[np.isfinite(col)].any(), w
        k1, t1, like1 = per_event[e]
        assert (k1, t1) == (src, ti) and np.array_equal(like1, like, equal_nan=True), w
        if e in (0, 3):
            assert res["max_beam"][e] == np.inf, w


def _relocation(oracle_lib, hip_opts, splits, expect=None):
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events, relocation_focus, relocation_likelihood
    for regime in bn.REGIMES:
        f, tau, wp, ws = bn.relocation_events(regime)
        bf = BeamformerGPU(tau, ws)
        try:
            if expect is not None:
                expect(bf.plan_info())
            for oob in OOBS:
                alone = {"spatial": [relocation_likelihood(bf, f[e], wp, oob) for e in range(f.shape[0])],
                         "temporal": [relocation_focus(bf, f[e], wp, "temporal", oob) for e in range(f.shape[0])]}
                # event 0's focus column holds NaN beams, event 2 is nothing but NaN
                assert np.isnan(alone["spatial"][0][2]).all() and np.isnan(alone["spatial"][2][2]).all()
                for method in ("temporal", "spatial"):
                    for split in splits:
                        if split is not None:
                            hip_opts("bp.split", split)
                        try:
                            res = relocate_events(bf, f, wp, method, oob, columns=method == "spatial")
                        finally:
                            if split is not None:
                                hip_opts.reset("bp.split")
                        _judge_events(oracle_lib, res, alone[method], f, tau, wp, ws, oob, method,
                                      (regime, oob, method, split))
        finally:
            bf.close()


def test_relocate_events_on_non_finite_windows(oracle_lib, hip_opts):
    _relocation(oracle_lib, hip_opts, (None, 3))


def test_relocate_events_on_non_finite_windows_without_lds_plan(oracle_lib, hip_opts):
    hip_opts("bp.direct", 1)

    def expect(info):
        assert info["n_groups"] == 0, info

    _relocation(oracle_lib, hip_opts, (None,), expect)


def test_per_event_focus_returns_the_column_of_the_batch(oracle_lib):
    """relocation_focus("spatial") on each event alone: the focus of relocation_likelihood and the raw column."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocation_focus, relocation_likelihood
    f, tau, wp, ws = bn.relocation_events("signed")
    bf = BeamformerGPU(tau, ws)
    try:
        for oob in OOBS:
            for e in range(f.shape[0]):
                k, ti, col = relocation_focus(bf, f[e], wp, "spatial", oob)
                vol = oracle_lib.beamform(f[e], tau, wp, ws, oob, "none")
                assert (k, ti) == bn.focus_of_volume(vol) == relocation_likelihood(bf, f[e], wp, oob)[:2], (oob, e)
                assert np.array_equal(col, vol[:, ti], equal_nan=True), (oob, e)
    finally:
        bf.close()
