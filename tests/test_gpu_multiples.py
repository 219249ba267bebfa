"""GPU: workflow.flag_multiples (bpmf_flag_multiples_dev, csrc/multiples.hip) against its host definition,
postprocess.flag_multiples -- np.array_equal on every case of multiples_cases.py: the named edge cases (windows of
63 / 64 / 65 / 130 neighbours, one segment, one segment per event, the sliding chain, ties in time and in cc, a window
that closes exactly at dt_criterion, accumulated sum against direct difference, asymmetric pair_ok, ...) and 200 seeded
random catalogs.  The output buffer is prefilled with 2: a flag the kernels do not write fails the comparison."""
import numpy as np
import pytest

import multiples_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wanted():
    """{name: the host definition's flags}, computed once."""
    from seismic_bpmf_amd import postprocess as pp
    return {name: pp.flag_multiples(*args) for name, *args in mc.named_cases() + mc.random_cases()}


def _check(case, wanted):
    import torch
    from seismic_bpmf_amd import workflow
    name, t, rows, cc, ok, dt = case
    out = torch.full((len(t),), 2, dtype=torch.uint8, device="cuda")
    got = workflow.flag_multiples(t, rows, cc, ok, dt, out=out)
    assert got.dtype == bool and got.shape == t.shape, name
    assert np.array_equal(got, wanted[name]), (name, np.flatnonzero(got != wanted[name])[:10])
    # the library's own buffer: 0 / 1 everywhere, in sorted order
    order = np.argsort(t, kind="stable")
    assert np.array_equal(out.cpu().numpy(), wanted[name][order].astype(np.uint8)), name


@pytest.mark.parametrize("case", mc.named_cases(), ids=lambda c: c[0])
def test_named_case(case, wanted):
    _check(case, wanted)


def test_random_cases(wanted):
    cases = mc.random_cases()
    assert len(cases) == 200 and max(len(c[1]) for c in cases) <= 2000 and max(c[4].shape[0] for c in cases) <= 40
    for case in cases:
        _check(case, wanted)
    assert sum(int((~wanted[c[0]]).sum()) for c in cases) > 10000


def test_without_out_and_on_a_side_stream(wanted):
    import torch
    from seismic_bpmf_amd import workflow
    case = mc.random_cases(count=3)[2]
    with torch.cuda.stream(torch.cuda.Stream()):
        got = workflow.flag_multiples(*case[1:], device="cuda:0")
    assert np.array_equal(got, wanted[case[0]])


def test_row_out_of_range_raises_and_reads_nothing_out_of_bounds():
    """The Python surface refuses the row; the library refuses it too (its own check, on the device) and names the event."""
    import ctypes as C
    import torch
    from seismic_bpmf_amd import _lib, workflow
    ok = np.ones((3, 3), bool)
    for rows in ([0, 3, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="outside"):
            workflow.flag_multiples([0.0, 1.0, 2.0], rows, [0.5, 0.6, 0.7], ok, 4.0)
        lib = _lib.lib()
        d_t = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device="cuda")
        d_rows = torch.tensor(rows, dtype=torch.int32, device="cuda")
        d_cc = torch.tensor([0.5, 0.6, 0.7], dtype=torch.float32, device="cuda")
        d_ok = torch.ones(9, dtype=torch.uint8, device="cuda")
        ws = torch.empty(lib.bpmf_flag_multiples_workspace_bytes(3), dtype=torch.uint8, device="cuda")
        out = torch.full((3,), 2, dtype=torch.uint8, device="cuda")
        rc = lib.bpmf_flag_multiples_dev(C.c_void_p(d_t.data_ptr()), C.c_void_p(d_rows.data_ptr()),
                                         C.c_void_p(d_cc.data_ptr()), 3, C.c_void_p(d_ok.data_ptr()), 3, 4.0,
                                         C.c_void_p(ws.data_ptr()), ws.numel(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(out.data_ptr()))
        assert rc != 0 and "event 1" in _lib.last_error() and "outside" in _lib.last_error()
    # n == 0 returns 0 and touches nothing
    out = torch.full((4,), 2, dtype=torch.uint8, device="cuda")
    assert lib.bpmf_flag_multiples_dev(None, None, None, 0, None, 3, 4.0, None, 0, None, C.c_void_p(out.data_ptr())) == 0
    assert (out == 2).all()


def test_detections_unique_on_the_device():
    from seismic_bpmf_amd import workflow
    rng = np.random.default_rng(11)
    det = {}
    for t in range(6):
        idx = np.unique(rng.integers(0, 500, 60)) * 10
        det[t] = (idx.astype(np.int64), rng.random(len(idx)).astype(np.float32), np.ones(len(idx), np.float32))
    ok = rng.random((6, 6)) < 0.6
    kw = dict(sr=25.0, step=2, pair_ok=ok, dt_criterion=4.0, t0_sec=3600.0)
    got, want = workflow.detections_unique(det, **kw), workflow.detections_unique(det, on_host=True, **kw)
    assert all(np.array_equal(got[t], want[t]) for t in det) and sum(int((~want[t]).sum()) for t in det) > 20
