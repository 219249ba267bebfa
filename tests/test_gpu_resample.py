"""GPU: the polyphase resampling on the device (csrc/resample.hip; workflow.resample_poly and
picker_batch(upsampling=, downsampling=)) against the definition on the host (postprocess.resample_poly_host, itself
pinned to scipy.signal.resample_poly in tests/test_resample_host.py): bit patterns through view(uint32), NaNs at the
same positions (tests/picker_cases.py: check -- whose power to reject a fused multiply-add, another summation order, a
shifted tap table and skipped padding taps on these inputs is shown in the CPU test).  The session runs with
debug.poison_output on (tests/conftest.py): an element the kernel does not write comes back as 0xFF bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picker_cases as pc  # noqa: E402
import resample_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_view(data, pad=3):
    """`data` as a device tensor that is a VIEW with a non-zero storage offset (4-byte aligned only)."""
    import torch
    buf = torch.full((data.size + pad + 5,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + data.size] = torch.as_tensor(data.reshape(-1), device="cuda")
    return buf[pad:pad + data.size].view(data.shape)


def _plan(n, up, down):
    """(reduced up, reduced down, hp, n_pre_remove, n_out, table, tile) of rows of n samples."""
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    up, down = pp.resample_poly_factors(up, down)
    _, n_out, _, n_pre_remove, _, table = pp.resample_poly_plan(n, up, down)
    hp = len(table) // up
    return up, down, hp, n_pre_remove, n_out, table, workflow.resample_poly_tile(up, down, hp)


def _resample_day(data_dev, starts, n, up, down, out=None, override=()):
    """bpmf_resample_poly_dev called directly on the windows of a day: (status, out (rows, C, n_out)).  `override`
    replaces arguments of the call by name."""
    import ctypes as C
    import torch
    from seismic_bpmf_amd import _lib
    S, Cc, N = (int(v) for v in data_dev.shape)
    up, down, hp, n_pre_remove, n_out, table, _ = _plan(n, up, down)
    a = dict(S=S, C=Cc, N=N, n_rows=np.asarray(starts).size if starts is not None else S, n_in=n, up=up, down=down, hp=hp,
             n_pre_remove=n_pre_remove, n_out=n_out)
    a.update(dict(override))
    d_start = None if starts is None else torch.as_tensor(np.asarray(starts, np.int64).reshape(-1), device="cuda")
    d_table = torch.as_tensor(table, device="cuda")
    if out is None:
        out = torch.empty((a["n_rows"], Cc, n_out), dtype=torch.float32, device="cuda")
    rc_ = _lib.lib().bpmf_resample_poly_dev(
        C.c_void_p(data_dev.data_ptr()), a["S"], a["C"], a["N"], a["n_rows"],
        None if d_start is None else C.c_void_p(d_start.data_ptr()), a["n_in"], a["up"], a["down"],
        C.c_void_p(d_table.data_ptr()), a["hp"], a["n_pre_remove"], a["n_out"],
        C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return rc_, out


@pytest.fixture(scope="module")
def host():
    """resample_poly_host of every case of the CPU test, computed once."""
    from seismic_bpmf_amd import postprocess as pp
    return {(up, down, n): pp.resample_poly_host(rc.rows(n), up, down) for up, down, n in rc.cases()}


def test_poison_is_on():
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1


@pytest.mark.parametrize("up,down", rc.FACTORS)
def test_resample_poly_equals_the_definition_on_every_case(host, up, down):
    """Every length of the CPU test, the input a view with a storage offset."""
    import torch
    from seismic_bpmf_amd import workflow
    for n in rc.lengths(up, down):
        x = rc.rows(n)
        x_dev = _device_view(x)
        got = workflow.resample_poly(x_dev, up, down)
        want = host[up, down, n]
        assert got.dtype == torch.float32 and got.device == x_dev.device and got.is_contiguous()
        assert got.data_ptr() != x_dev.data_ptr()
        pc.check(got.cpu().numpy(), want, f"up {up} down {down} n {n}")
    assert np.isnan(want[11]).any() and not np.isnan(want[:11]).any()


@pytest.mark.parametrize("up,down", [f for f in rc.FACTORS if f[0] != f[1]])
def test_output_lengths_around_the_tile(up, down):
    """n_out at one tile - 1, one tile, one tile + 1 and two tiles + 1 of the tile the host chooses."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    u, d, hp, _, _, _, tile = _plan(3000, up, down)
    assert tile % 64 == 0 and 64 <= tile <= 1024
    counts = []
    for n in rc.tile_lengths(tile, u, d):
        x = rc.rows(n, seed=1)[[0, 7, 10, 11]]
        got = workflow.resample_poly(torch.as_tensor(x, device="cuda"), up, down)
        pc.check(got.cpu().numpy(), pp.resample_poly_host(x, up, down), f"up {up} down {down} n {n}")
        counts.append(int(got.shape[-1]))
    step = -(-u // d)                                                # counts a length apart differ by at most this
    assert tile - step <= counts[0] < tile and tile - step < counts[1] <= tile, (tile, counts)
    assert tile < counts[2] <= tile + step and 2 * tile < counts[3] <= 2 * tile + step, (tile, counts)


def test_a_4d_input_a_single_row_and_a_side_stream(host):
    import torch
    from seismic_bpmf_amd import workflow
    x = rc.rows(257)
    got = workflow.resample_poly(_device_view(x.reshape(2, 3, 2, 257)), 5, 2)
    assert tuple(got.shape) == (2, 3, 2, 643)
    pc.check(got.cpu().numpy(), host[5, 2, 257].reshape(2, 3, 2, 643), "4-D")
    got = workflow.resample_poly(_device_view(x)[3], 5, 2)
    pc.check(got.cpu().numpy(), host[5, 2, 257][3], "1-D")
    strided = _device_view(np.repeat(x, 2, axis=1))[:, ::2]          # not contiguous
    pc.check(workflow.resample_poly(strided, 5, 2).cpu().numpy(), host[5, 2, 257], "strided")
    empty = workflow.resample_poly(torch.zeros((0, 3, 40), device="cuda"), 5, 2)
    assert tuple(empty.shape) == (0, 3, 100) and empty.dtype == torch.float32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    x_dev = _device_view(x)
    with torch.cuda.stream(side):
        out = workflow.resample_poly(x_dev, 5, 2)
        doubled = out * 2                                            # consumed on the same stream, no synchronisation
    side.synchronize()
    pc.check(doubled.cpu().numpy(), host[5, 2, 257] * np.float32(2), "side stream, consumed")


def test_a_long_row_crosses_many_tiles():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    x = rc.rows(200000, seed=2)[[3]]
    x[0, 123456] = np.nan
    got = workflow.resample_poly(torch.as_tensor(x, device="cuda"), 1, 4)
    assert tuple(got.shape) == (1, 50000) and 50000 > 40 * _plan(200000, 1, 4)[6]
    want = pp.resample_poly_host(x, 1, 4)
    pc.check(got.cpu().numpy(), want, "200000 samples down 4")
    assert 0 < np.isnan(want).sum() < 50


@pytest.mark.parametrize("up,down", [(4, 1), (2, 5)])
def test_the_day_form_cuts_the_window_first(up, down):
    """Windows inside the day, cut by its end, wholly past it and cut by its start; starts per event and per (event,
    station).  The wanted answer filters the zero-padded CUT windows: a kernel that reads the day's samples beside a
    window fails."""
    from seismic_bpmf_amd import postprocess as pp
    n = 1203
    data, starts, per_station = pc.day_case(n)
    data_dev = _device_view(data)
    for label, st in (("per event", starts), ("per event and station", per_station)):
        st = pp.picker_starts(st, 3)
        windows = pp.picker_windows_host(data, st, n)                # (E, S, C, n)
        assert not windows[2].any() and windows[0].all(axis=-1).any()
        want = pp.resample_poly_host(windows, up, down)
        status, got = _resample_day(data_dev, st, n, up, down)
        assert status == 0
        pc.check(got.cpu().numpy().reshape(want.shape), want, f"{label} up {up} down {down}")
    # the window inside the day has neighbours in the day that would change its ends
    e0 = int(starts[0])
    wider = pp.resample_poly_host(data[:, :, e0 - 60: e0 + n + 60], up, down)
    k = 60 * up // down
    assert not pc.same_bits(wider[0, 0, k: k + 8], want[0, 0, 0, :8])
    assert pc.same_bits(wider[0, 0, k + 100: k + 108], want[0, 0, 0, 100: 108])


def _composed(data, starts, n, up, down, W, overlap):
    from seismic_bpmf_amd import postprocess as pp
    windows = pp.resample_poly_host(pp.picker_windows_host(data, starts, n), up, down)
    E, S, C, n_out = windows.shape
    return pp.normalize_batch_host(windows.reshape(E * S, C, n_out), W, overlap).reshape(E, S, C, n_out)


@pytest.mark.parametrize("up,down,n", [(4, 1, 300), (2, 5, 3000)])
def test_picker_batch_resamples_between_the_cut_and_the_normalisation(up, down, n):
    """W = 400, overlap 0.5; starts per event and per (event, station); float32 and float64.  Down by 5 / 2 the
    windows hold 3000 input samples: 300 would leave 120, fewer than the shift of 200 that the normalisation needs
    (that refusal is tested below)."""
    import torch
    from seismic_bpmf_amd import workflow
    W, overlap = 400, .5
    data, starts, per_station = pc.day_case(n)
    data_dev = _device_view(data)
    n_out = -(-n * up // down)
    for label, st in (("per event", starts), ("per event and station", per_station)):
        want64 = _composed(data, st, n, up, down, W, overlap)
        assert want64.shape == (4, 3, 3, n_out)
        got = workflow.picker_batch(data_dev, st, n, normalization_window_sample=W, overlap=overlap, upsampling=up,
                                    downsampling=down)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, 3, n_out) and got.is_contiguous()
        pc.check(got.cpu().numpy(), want64.astype(np.float32), label)
        got64 = workflow.picker_batch(data_dev, st, n, normalization_window_sample=W, overlap=overlap, upsampling=up,
                                      downsampling=down, dtype=torch.float64)
        pc.check(got64.cpu().numpy(), want64, label + " float64")
    none = workflow.picker_batch(data_dev, np.zeros((0,), np.int64), n, normalization_window_sample=W,
                                 upsampling=up, downsampling=down)
    assert tuple(none.shape) == (0, 3, 3, n_out) and none.device == data_dev.device and none.dtype == torch.float32


def test_picker_batch_with_equal_factors_is_the_call_without_them():
    import torch
    from seismic_bpmf_amd import workflow
    n, W = 300, 100
    data, starts, _ = pc.day_case(n)
    data_dev = _device_view(data)
    plain = workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W)
    same = workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W, upsampling=3, downsampling=3)
    assert tuple(same.shape) == (4, 3, 3, n) and torch.equal(plain.view(torch.int32), same.view(torch.int32))


def test_refusals_come_before_any_device_work():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    x = torch.zeros((2, 3, 600), device="cuda")
    for call in (lambda: workflow.resample_poly(np.zeros((2, 600), np.float32), 4, 1),
                 lambda: workflow.resample_poly(torch.zeros((2, 600)), 4, 1)):
        with pytest.raises(ValueError, match="no CPU path; the definition on the host is postprocess.resample_poly_host"):
            call()
    for up, down in ((0, 1), (1, 0), (2.5, 1), (65, 1), (1, 130)):
        with pytest.raises(ValueError, match="resample_poly"):
            workflow.resample_poly(x, up, down)
        with pytest.raises(ValueError, match="resample_poly"):
            workflow.picker_batch(x, [0], 300, normalization_window_sample=100, upsampling=up, downsampling=down)
    with pytest.raises(ValueError, match="float32"):
        workflow.resample_poly(x.double(), 4, 1)
    with pytest.raises(ValueError, match="at least 1 sample"):
        workflow.resample_poly(torch.zeros((2, 0), device="cuda"), 4, 1)
    with pytest.raises(ValueError, match="at least 1 sample"):
        workflow.picker_batch(x, [0], 0, upsampling=4)
    with pytest.raises(ValueError, match="2\\^31 tiles"):            # 2^25 rows (never materialised) x 64 tiles
        workflow.resample_poly(torch.zeros(1, device="cuda").expand(2**25, 1024), 64, 1)
    # the refusals of the normalisation count in resampled samples, and come before the resampling is launched
    data, starts, _ = pc.day_case(300)
    with pytest.raises(ValueError, match="shift"):                   # 300 samples down 5 / 2 leave 120; the shift is 200
        workflow.picker_batch(torch.as_tensor(data, device="cuda"), starts, 300, normalization_window_sample=400,
                              upsampling=2, downsampling=5)
    with pytest.raises(ValueError, match="shift"):
        pp.normalize_batch_host(pp.resample_poly_host(pp.picker_windows_host(data, starts, 300), 2, 5)[0], 400, .5)
    with pytest.raises(ValueError, match="LDS"):                     # 9000 x 4 = 36000 samples do not fit
        workflow.picker_batch(x, [0], 9000, upsampling=4)
    workflow.picker_batch(x, [0], 9000, normalization_window_sample=3000)       # ... 9000 do
    with pytest.raises(ValueError, match="dtype"):
        workflow.picker_batch(x, [0], 300, normalization_window_sample=100, upsampling=4, dtype=torch.float16)


def test_c_abi_refuses_with_a_status_and_leaves_the_output_untouched():
    import torch
    from seismic_bpmf_amd import _lib
    n = 600
    data_dev = torch.ones((2, 3, n), device="cuda")
    out = torch.full((2, 3, 4 * n), 7.0, device="cuda")             # poisoned by the session only if a call gets through
    for override, word in ((dict(up=0), "up"), (dict(down=0), "up"), (dict(up=65), "up"), (dict(up=4, down=2), "gcd"),
                           (dict(up=1, down=1), "both 1"), (dict(n_in=0), "n_in"), (dict(n_in=2**38), "2^40"),
                           (dict(n_out=4 * n - 1), "n_out"), (dict(hp=0), "plan"), (dict(hp=600), "plan"),
                           (dict(n_pre_remove=10**6), "plan"), (dict(S=0), "bad argument"),
                           (dict(N=0), "bad argument"), (dict(n_rows=2**31), "bad argument")):
        status, _ = _resample_day(data_dev, None, n, 4, 1, out=out, override=override)
        assert status == -1 and word in _lib.last_error(), (override, _lib.last_error())
    assert _lib.lib().bpmf_resample_poly_tile(65, 1, 21) == 0 and _lib.lib().bpmf_resample_poly_tile(4, 1, 0) == 0
    status, _ = _resample_day(data_dev, None, n, 4, 1, out=out, override=dict(n_rows=0))
    assert status == 0                                               # no rows: nothing is launched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    status, got = _resample_day(data_dev, None, n, 4, 1, out=out)
    assert status == 0 and not bool((got == 7.0).any())
