"""GPU: what surrounds the deep-learning picker, on the device (csrc/picker.hip; workflow.normalize_batch,
picker_batch, find_picks, pick_events) against the definitions on the host (postprocess.normalize_batch_host,
find_picks_host, get_picks_host, themselves pinned to the reference in tests/test_picker_host.py): bit patterns
through view(uint32 / uint64), NaNs at the same positions (tests/picker_cases.py: check -- whose power to reject is
shown in the CPU test).  The session runs with debug.poison_output on (tests/conftest.py): an element the kernels do
not write comes back as 0xFF bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picker_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_view(data, pad=3):
    """`data` as a device tensor that is a VIEW with a non-zero storage offset (4-byte aligned only)."""
    import torch
    buf = torch.full((data.size + pad + 5,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + data.size] = torch.as_tensor(data.reshape(-1), device="cuda")
    return buf[pad:pad + data.size].view(data.shape)


def _host_norm(x, W, overlap):
    from seismic_bpmf_amd import postprocess as pp
    want64 = pp.normalize_batch_host(x, W, overlap)
    return want64, want64.astype(np.float32)


@pytest.fixture(scope="module")
def host_picks():
    """find_picks_host of every pick case, computed once."""
    from seismic_bpmf_amd import postprocess as pp
    return [pp.find_picks_host(series, thr, return_index=True) for _, series, thr in pc.pick_cases()]


def test_poison_is_on():
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1           # outputs are handed over full of junk


def test_normalize_batch_equals_the_definition_on_every_case():
    import torch
    from seismic_bpmf_amd import workflow
    met = set()
    for k, (n, W, overlap) in enumerate(pc.NORM_CASES):
        x = pc.norm_rows(n, k)
        want64, want32 = _host_norm(x, W, overlap)
        x_dev = _device_view(x)
        got32 = workflow.normalize_batch(x_dev, W, overlap)
        got64 = workflow.normalize_batch(x_dev, W, overlap, dtype=torch.float64)
        assert got32.dtype == torch.float32 and got64.dtype == torch.float64 and got32.device == x_dev.device
        pc.check(got64.cpu().numpy(), want64, f"float64 {(n, W, overlap)}")
        pc.check(got32.cpu().numpy(), want32, f"float32 {(n, W, overlap)}")
        assert np.isnan(want64).any() and not np.isnan(want64[0]).any()
        met |= pc.norm_classes_met(x, W, overlap)
    assert met == pc.NORM_CLASSES, pc.NORM_CLASSES - met


def test_picker_batch_equals_normalize_batch_of_the_cut_windows():
    """Starts per event and per (event, station); windows inside the day, cut by its end, wholly past it and cut by
    its start; the day is a view with a storage offset."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    n, W, overlap = 1203, 400, .5
    data, starts, per_station = pc.day_case(n)
    data_dev = _device_view(data)
    for label, st in (("per event", starts), ("per event and station", per_station),
                      ("as a tensor", torch.as_tensor(per_station))):
        windows = pp.picker_windows_host(data, np.asarray(st), n)              # (E, S, C, n)
        assert windows.shape == (4, 3, 3, n)
        assert not windows[2].any() and not windows[1, :, :, -n // 3:].any() and not windows[3, :, :, : n // 4].any()
        want64 = pp.normalize_batch_host(windows.reshape(12, 3, n), W, overlap).reshape(4, 3, 3, n)
        got = workflow.picker_batch(data_dev, st, n, normalization_window_sample=W, overlap=overlap)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, 3, n) and got.is_contiguous()
        pc.check(got.cpu().numpy(), want64.astype(np.float32), label)
        got64 = workflow.picker_batch(data_dev, st, n, normalization_window_sample=W, overlap=overlap,
                                      dtype=torch.float64)
        pc.check(got64.cpu().numpy(), want64, label + " float64")
        # and the tensor form on the cut windows gives the same bits
        again = workflow.normalize_batch(torch.as_tensor(windows.reshape(12, 3, n), device="cuda"), W, overlap)
        pc.check(again.cpu().numpy().reshape(4, 3, 3, n), want64.astype(np.float32), label + " tensor form")
    none = workflow.picker_batch(data_dev, np.zeros((0,), np.int64), n, normalization_window_sample=W)
    assert tuple(none.shape) == (0, 3, 3, n) and none.device == data_dev.device


def test_launches_go_to_the_current_stream_and_are_consumed_there():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    n, W = 777, 256
    data, starts, _ = pc.day_case(n, seed=5)
    want = pp.normalize_batch_host(pp.picker_windows_host(data, starts, n).reshape(12, 3, n), W, .75)
    want = want.astype(np.float32).reshape(4, 3, 3, n)
    data_dev = _device_view(data)
    _, series, thr = pc.pick_cases()[0]
    proba = torch.as_tensor(np.stack([series, series[::-1].copy()])[None], device="cuda")     # (1, 2, n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = workflow.picker_batch(data_dev, starts, n, normalization_window_sample=W, overlap=.75)
        doubled = out * 2                                            # consumed on the same stream, no synchronisation
        picks = workflow.find_picks(proba * 1, thr, thr)
    side.synchronize()
    pc.check(out.cpu().numpy(), want, "side stream")
    pc.check(doubled.cpu().numpy(), want * np.float32(2), "side stream, consumed")
    host = pp.find_picks_host(series, thr, return_index=True)
    k = len(host[0])
    assert picks["count"].tolist() == [[k, k]] and np.array_equal(picks["index"][0, 0, :k], host[3])
    assert np.array_equal(picks["index"][0, 1, :k], (len(series) - 1 - host[3])[::-1])


def test_find_picks_equals_the_definition_on_every_case(host_picks):
    import torch
    from seismic_bpmf_amd import workflow
    met = set()
    max_picks = 72
    for (label, series, thr), want in zip(pc.pick_cases(), host_picks):
        n = len(series)
        # the series as the S row of one station and as the P row of another, beside a row of noise below threshold
        quiet = np.full(n, np.float32(0.01))
        proba = np.stack([np.stack([quiet, series]), np.stack([series, quiet])])           # (2, 2, n)
        got = workflow.find_picks(_device_view(proba), thr, thr, max_picks=max_picks)
        k = len(want[0])
        assert got["count"].tolist() == [[0, k], [k, 0]], label
        for where in ((0, 1), (1, 0)):
            pc.check_picks(tuple(got[key][where][:k] for key in ("value", "mean", "std", "index")), want, label)
            assert np.isnan(got["value"][where][k:]).all() and np.isnan(got["mean"][where][k:]).all(), label
            assert np.isnan(got["std"][where][k:]).all() and (got["index"][where][k:] == -1).all(), label
        assert np.isnan(got["value"][0, 0]).all() and (got["index"][1, 1] == -1).all(), label
        assert got["value"].dtype == np.float32 and got["mean"].dtype == np.float64 and \
            got["std"].dtype == np.float64 and got["index"].dtype == np.int32 and got["count"].dtype == np.int32
        met |= pc.pick_classes_met(series, thr, want)
    assert met == pc.PICK_CLASSES, pc.PICK_CLASSES - met
    assert sum(len(w[0]) for w in host_picks) > 150


def test_thresholds_differ_between_p_and_s():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    _, series, _ = pc.pick_cases()[0]                               # peaks of 0.9, 0.7 and 0.4
    proba = torch.as_tensor(np.stack([series, series])[None, None], device="cuda")         # (1, 1, 2, n)
    got = workflow.find_picks(proba, threshold_P=0.3, threshold_S=0.6)
    assert got["count"].shape == (1, 1, 2) and got["value"].shape == (1, 1, 2, 32)
    assert got["count"][0, 0].tolist() == [len(pp.find_picks_host(series, 0.3)[0]),
                                           len(pp.find_picks_host(series, 0.6)[0])] == [3, 2]


def test_capacity_rule_of_find_picks(host_picks):
    """More picks than max_picks: count is the true number, the first max_picks records are kept; the call raises
    unless truncate=True."""
    import torch
    from seismic_bpmf_amd import workflow
    cases = pc.pick_cases()
    k = [label for label, _, _ in cases].index("forty_picks")
    _, series, thr = cases[k]
    want = host_picks[k]
    assert len(want[0]) == 40
    proba = torch.as_tensor(np.stack([series, series])[None], device="cuda")
    with pytest.raises(RuntimeError, match="40 picks, more than max_picks = 8"):
        workflow.find_picks(proba, thr, thr, max_picks=8)
    got = workflow.find_picks(proba, thr, thr, max_picks=8, truncate=True)
    assert got["count"].tolist() == [[40, 40]]
    pc.check_picks(tuple(got[key][0, 1] for key in ("value", "mean", "std", "index")),
                   tuple(w[:8] for w in want), "truncated")
    full = workflow.find_picks(proba, thr, thr, max_picks=40)       # exactly full: no slot left over, no raise
    pc.check_picks(tuple(full[key][0, 0] for key in ("value", "mean", "std", "index")), want, "exactly full")


def test_the_documented_caps():
    """n = 16384 with W = 3000 (120 s at 100 Hz): a handful of rows through both kernels, a pick wider than the 8192
    samples NumPy sums in one piece among them."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    n = 16384
    x = pc.norm_rows(n, 40)[:2]                                     # six rows: noise, zero, constant, half, NaN, tiny
    want64 = pp.normalize_batch_host(x, 3000, .5)
    got = workflow.normalize_batch(torch.as_tensor(x, device="cuda"), 3000, .5, dtype=torch.float64)
    pc.check(got.cpu().numpy(), want64, "n = 16384")
    t = np.arange(n, dtype=np.float64)
    wide = (0.9 * np.exp(-0.5 * ((t - 8000.3) / 5000.0) ** 2)).astype(np.float32)
    wide[:3] = 0.0
    wide[-3:] = 0.0
    # 81 peaks that grow towards the middle of the series: every prominence walk ends at the next peak or at an end
    many = (0.5 + (0.3 + 0.15 * (1.0 - np.abs(t - 8192.0) / 8192.0)) * np.sin(t / 32.0)).astype(np.float32)
    proba = np.stack([np.stack([wide, many]), np.stack([many, wide])])
    got = workflow.find_picks(torch.as_tensor(proba, device="cuda"), 0.3, 0.3, max_picks=100)
    want = {"wide": pp.find_picks_host(wide, 0.3, return_index=True),
            "many": pp.find_picks_host(many, 0.3, return_index=True)}
    assert len(want["wide"][0]) == 1 and len(want["many"][0]) > 70
    for name, where in (("wide", (0, 0)), ("many", (0, 1)), ("many", (1, 0)), ("wide", (1, 1))):
        k = len(want[name][0])
        assert got["count"][where] == k
        pc.check_picks(tuple(got[key][where][:k] for key in ("value", "mean", "std", "index")), want[name], name)
    lip_rip = pp.find_peaks_host(wide, 0.3)
    assert int(lip_rip[2][0]) - int(lip_rip[1][0]) + 1 > 8192


def test_pick_events_equals_get_picks_of_the_host_picks():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    rng = np.random.default_rng(5)
    E, S, n = 3, 4, 1500
    t = np.arange(n)
    proba = 0.02 * rng.random((E, S, 2, n))
    for e in range(E):
        for s in range(S):
            for ph in range(2):
                for _ in range(int(rng.integers(0, 4))):             # some series without a pick
                    proba[e, s, ph] += rng.uniform(.4, 1.) * np.exp(-0.5 * ((t - rng.uniform(50, n - 50)) /
                                                                           rng.uniform(4, 25)) ** 2)
    proba = np.clip(proba, 0, 1).astype(np.float32)
    prior = rng.uniform(200, 1300, (S, 2))
    prior[1] = np.nan
    for kw in ({}, {"prior": prior, "search_win_samp": 150}, {"sr": 100.0}):
        got = workflow.pick_events(torch.as_tensor(proba, device="cuda"), threshold_P=0.5, threshold_S=0.4,
                                   buffer_length=200, **kw)
        assert got.shape == (E, S, 6) and got.dtype == np.float32
        for e in range(E):
            values = np.full((S, 2, 32), np.nan, np.float32)
            means, stds = np.full((S, 2, 32), np.nan), np.full((S, 2, 32), np.nan)
            counts = np.zeros((S, 2), np.int32)
            for s in range(S):
                for ph, thr in enumerate((0.5, 0.4)):
                    v, m, d = pp.find_picks_host(proba[e, s, ph], thr)
                    counts[s, ph] = len(v)
                    values[s, ph, :len(v)], means[s, ph, :len(v)], stds[s, ph, :len(v)] = v, m, d
            want = pp.get_picks_host(values, means, stds, counts, 200, kw.get("prior"), kw.get("search_win_samp"))
            if "sr" in kw:
                want[:, [1, 2, 4, 5]] = want[:, [1, 2, 4, 5]] / np.float32(100.0)
            pc.check(got[e], want, f"event {e} {sorted(kw)}")
        assert np.isnan(got).any() and not np.isnan(got).all()


def test_refusals_come_before_any_device_work():
    import torch
    from seismic_bpmf_amd import workflow
    x = torch.zeros((2, 3, 600), device="cuda")
    host = np.zeros((2, 3, 600), np.float32)
    for call in (lambda: workflow.normalize_batch(host, 200), lambda: workflow.picker_batch(host, [0], 300),
                 lambda: workflow.find_picks(host[:, :2]), lambda: workflow.normalize_batch(torch.zeros((2, 3, 600))),
                 lambda: workflow.pick_events(torch.zeros((1, 2, 2, 60)), threshold_P=.5, threshold_S=.5,
                                              buffer_length=0)):
        with pytest.raises(ValueError, match="no CPU path; the definition"):
            call()
    for kw in (dict(normalization_window_sample=1), dict(normalization_window_sample=8193),
               dict(normalization_window_sample=200, overlap=0.999), dict(normalization_window_sample=2000),
               dict(normalization_window_sample=200, overlap=-3.0), dict(normalization_window_sample=200, dtype=torch.float16)):
        with pytest.raises(ValueError, match="normalize_batch"):
            workflow.normalize_batch(x, **kw)
    with pytest.raises(ValueError, match="LDS"):
        workflow.normalize_batch(torch.zeros((1, 1, 36000), device="cuda"), 3000)
    with pytest.raises(ValueError, match="starts"):
        workflow.picker_batch(x, np.zeros((2, 3), np.int64), 300, normalization_window_sample=100)
    with pytest.raises(ValueError, match="starts"):
        workflow.picker_batch(x, np.array([0.5]), 300, normalization_window_sample=100)
    with pytest.raises(ValueError, match="2\\^40"):
        workflow.picker_batch(x, np.array([2**41]), 300, normalization_window_sample=100)
    with pytest.raises(ValueError, match=r"\(\.\.\., 2, n\)"):
        workflow.find_picks(x)
    with pytest.raises(ValueError, match="16384"):
        workflow.find_picks(torch.zeros((1, 2, 16385), device="cuda"))
    with pytest.raises(ValueError, match="max_picks"):
        workflow.find_picks(x[:, :2], max_picks=0)
    with pytest.raises(ValueError, match="numbers"):
        workflow.find_picks(x[:, :2], threshold_P=float("nan"))


def test_c_abi_refuses_with_a_status_and_a_message():
    import ctypes as C
    import torch
    from seismic_bpmf_amd import _lib
    x = torch.zeros((1, 1, 40000), device="cuda")
    nodes = torch.zeros(25, dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 1, 40000), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().bpmf_normalize_batch_dev(C.c_void_p(x.data_ptr()), 1, 1, 40000, 1, None, 36000, 3000, 1500,
                                             C.c_void_p(nodes.data_ptr()), 25, 0, stream, C.c_void_p(out.data_ptr()))
    assert rc == -1 and "LDS" in _lib.last_error()
    rc = _lib.lib().bpmf_normalize_batch_dev(C.c_void_p(x.data_ptr()), 1, 1, 40000, 1, None, 6000, 3000, 1500,
                                             C.c_void_p(nodes.data_ptr()), 4, 0, stream, C.c_void_p(out.data_ptr()))
    assert rc == -1 and "5 windows" in _lib.last_error()
    rc = _lib.lib().bpmf_find_picks_dev(C.c_void_p(x.data_ptr()), 1, 20000, 0.5, 0.5, 4, stream,
                                        *(C.c_void_p(out.data_ptr()),) * 5)
    assert rc == -1 and "16384" in _lib.last_error()
    torch.cuda.synchronize()
    assert not out.any()                                             # nothing was launched
