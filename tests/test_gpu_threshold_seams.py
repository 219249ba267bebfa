"""GPU: the RMS threshold's streaming kernels and the candidate extraction (csrc/post.hip) on the case table of
threshold_cases.py -- windows shorter than a step and around 1, 2, 6 and 12 steps, shifts of 1, window, window + 1,
odd and = 2 mod 4, rows at every dword alignment, rows x windows on either side of 64 and 128, zeros planted at step
edges, in the tail, at the wrap of the gauss index, as -0.0, as whole windows and whole rows, 1 to 3 windows through
the smoothing, the clamp of the expansion, the extraction's groups of four at n = 4k .. 4k + 3 and around 4096 with
samples on and one ulp above the threshold, caps, capacities, NaN rows; the workspace dirty, every refusal.

Against the NumPy definition of threshold_cases.py and the C oracle, bit for bit (NaN equal to NaN).
test_threshold_cases_host.py shows on the CPU that definition, oracle and the reference's own recorded output agree on
the table and that each case rejects the planted defects named there.

Every call goes through the C entry points by (half_window, shift), with a workspace of exactly the size asked for,
filled with 0xFF, and outputs filled with 0xFF that are one row longer than needed: the extra row is where the idle
lanes of the last wave would store, and must stay untouched.

Out of scope: n >= 2^31 and windows near 2^31 (gigabytes per case), non-finite CC values other than the NaN rows that
zeros produce, the medians of the MAD threshold (test_gpu_threshold.py)."""
import ctypes as C

import numpy as np
import pytest

import threshold_cases as tc

pytestmark = pytest.mark.gpu
_f = C.POINTER(C.c_float)


def _lib():
    from seismic_bpmf_amd import _lib
    return _lib.lib()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _ff(shape, dtype=None):
    """A device tensor with every byte 0xFF."""
    import torch
    t = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _untouched(t):
    import torch
    return t.numel() == 0 or bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all().item())


def run_tdt(x, gauss, num_dev, half, shift, expand=True):
    """bpmf_tdt_rms_dev on x (rows, n): (thr_win, full or None) as NumPy arrays; the sentinel rows are checked."""
    import torch
    lib = _lib()
    rows, n = x.shape
    n_win = lib.bpmf_tdt_num_windows(n, half, shift)
    need = lib.bpmf_tdt_workspace_bytes(rows, n, half, shift)
    assert n_win == tc.tdt_sizes(n, half, shift)[2] and need > 0
    xd, gd, ws = _dev(x), _dev(gauss), _ff(need, torch.uint8)
    tw = _ff((rows + 1, n_win))
    full = _ff((rows + 1, n)) if expand else None
    rc = lib.bpmf_tdt_rms_dev(xd.data_ptr(), gd.data_ptr(), float(num_dev), rows, n, half, shift, ws.data_ptr(), need,
                              _stream(), tw.data_ptr(), full.data_ptr() if expand else None)
    torch.cuda.synchronize()
    assert rc == 0, lib.bpmf_last_error()
    assert _untouched(tw[rows]) and (full is None or _untouched(full[rows])), "the row behind the output was written"
    return tw[:rows].cpu().numpy(), full[:rows].cpu().numpy() if expand else None


def oracle_rows(oracle, case):
    lib = oracle.load()
    full = np.zeros((case.rows, case.n), np.float32)
    gauss = np.ascontiguousarray(case.gauss, np.float32)
    for r in range(case.rows):
        x, scratch = np.ascontiguousarray(case.x[r]), np.empty(case.n, np.float32)
        rc = lib.tdt_rms_cpu(x.ctypes.data_as(_f), gauss.ctypes.data_as(_f), float(case.num_dev), case.n, case.half,
                             case.shift, scratch.ctypes.data_as(_f), full[r].ctypes.data_as(_f))
        assert rc == case.sizes[2]
    return full


def run_extract(kind, x, thr, window_or_half, shift, row_cap, capacity, slack=2):
    """One call of the extraction's C entry point: (count, the first min(count, capacity) records sorted, whether the
    record buffer behind `capacity` is untouched)."""
    import torch
    lib = _lib()
    rows, n = x.shape
    xd, td = _dev(x), _dev(thr)
    cd = _dev(np.asarray(row_cap, np.float32)) if row_cap is not None else None
    count = _ff(2, torch.int32)
    rec = _ff((capacity + slack, 4), torch.int32)
    fn = lib.bpmf_extract_candidates_dev if kind == "rms" else lib.bpmf_extract_candidates_mad_dev
    rc = fn(xd.data_ptr(), td.data_ptr(), cd.data_ptr() if cd is not None else None, rows, n, window_or_half, shift,
            capacity, _stream(), count.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.bpmf_last_error()
    found = int(count[0].item())
    assert int(count[1].item()) == -1
    got = rec[:min(found, capacity)].cpu().numpy().view(tc.candidate_dtype).reshape(-1)
    return found, got[np.lexsort((got["index"], got["row"]))], _untouched(rec[min(found, capacity):])


def check_tdt_case(oracle, case):
    """Device == definition == oracle on thr_win and full; thr_win the same without the expansion; the extraction of
    the device's own thresholds == the samples above the definition's expanded threshold."""
    d_win, d_full = tc.tdt_rms_definition(case.x, case.gauss, case.num_dev, case.half, case.shift)
    tw, full = run_tdt(case.x, case.gauss, case.num_dev, case.half, case.shift)
    bad = []
    if not tc.same_values(tw, d_win):
        bad.append(f"{case.name}: thr_win differs in {np.count_nonzero(~((tw == d_win) | (np.isnan(tw) & np.isnan(d_win))))} "
                   f"of {tw.size} windows")
    if not tc.same_values(full, d_full):
        bad.append(f"{case.name}: expanded threshold differs from the definition")
    if not tc.same_values(full, oracle_rows(oracle, case)):
        bad.append(f"{case.name}: expanded threshold differs from the oracle")
    tw2, _ = run_tdt(case.x, case.gauss, case.num_dev, case.half, case.shift, expand=False)
    if not tc.same_bits(tw, tw2):
        bad.append(f"{case.name}: thr_win changes with the expansion")
    want = tc.extract_definition(case.x, d_win, "rms", case.half, case.shift, None)
    found, got, clean = run_extract("rms", case.x, tw, case.half, case.shift, None, max(1, want.size))
    if found != want.size or not tc.same_records(got, want) or not clean:
        bad.append(f"{case.name}: {found} candidates, {want.size} samples above the threshold")
    return bad


# ------------------------------------------------------------------------------------------ the case table ---
@pytest.mark.parametrize("window", tc.STREAM_WINDOWS)
def test_stream_cases(oracle_lib, window):
    """One window length through its five shifts (1, window, window + 1, odd near 3/4, = 2 mod 4), four rows of odd
    length with zeros of both signs."""
    bad = []
    for case in tc.tdt_cases():
        if case.group == "stream" and 2 * case.half == window:
            bad += check_tdt_case(oracle_lib, case)
    assert bad == []


@pytest.mark.parametrize("group", ["lanes", "smooth", "expand"])
def test_lane_smoothing_and_expansion_cases(oracle_lib, group):
    """lanes: rows x n_win and rows x n_glob at 1, 63, 64, 65, 127, 128, 129 (the row behind the outputs stays
    untouched: run_tdt).  smooth: 1, 2, 3 and 8 windows rising, falling, alternating, flat.  expand: the clamp acting
    and idle, n - shift < shift, n = window, the one shape where the tail test decides."""
    bad = []
    for case in tc.tdt_cases():
        if case.group == group:
            bad += check_tdt_case(oracle_lib, case)
    assert bad == []


def test_zero_cases_and_their_neighbouring_rows(oracle_lib):
    """Zeros by construction (step edges, tail, gauss index 499 / 0, -0.0, a negative step, whole windows, the
    remainder only, one lane, all 64 lanes, a whole row): right, and every row bit-equal to the same row run alone."""
    bad = []
    for case in tc.tdt_cases():
        if case.group != "zeros":
            continue
        bad += check_tdt_case(oracle_lib, case)
        tw, full = run_tdt(case.x, case.gauss, case.num_dev, case.half, case.shift)
        for r in range(case.rows):
            tw1, full1 = run_tdt(case.x[r:r + 1], case.gauss, case.num_dev, case.half, case.shift)
            if not (tc.same_bits(tw1[0], tw[r]) and tc.same_bits(full1[0], full[r])):
                bad.append(f"{case.name}: row {r} alone differs from row {r} among its neighbours")
        if case.expect.get("nan_row"):
            assert np.isnan(tw[1]).all() and np.isfinite(tw[[0, 2]]).all()
    assert bad == []


def _py_params(case):
    """(sliding_window_samp, overlap) that ThresholdGPU turns into the case's (window, shift)."""
    from seismic_bpmf_amd.threshold import window_params
    w = case.window + 1 if case.kind == "rms" and case.shift == case.window + 1 else case.window
    overlap = 1.0 - (case.shift + 0.5) / w if case.shift < w else 0.0
    assert window_params(w, overlap) == (case.window // 2 if case.kind == "rms" else w // 2, case.shift)
    return w, overlap


@pytest.mark.parametrize("kind", ["rms", "mad"])
def test_extraction_cases(kind):
    """Synthetic, pairwise distinct window values: n = 4k .. 4k + 3, 4095 .. 4097, 8193, shifts 1, 2, 3, 5, samples on
    and one ulp above the threshold at the ends of the head, the tail and an interior window, caps below / equal /
    above / +inf per row, no cap, no candidate, a NaN row; through ThresholdGPU.extract_candidates with a capacity of
    1, of exactly the count and of count + 1, and through the C entry point with a sentinel behind the records."""
    from seismic_bpmf_amd.threshold import ThresholdGPU
    th = ThresholdGPU()
    bad = []
    for case in tc.extract_cases():
        if case.kind != kind:
            continue
        want = tc.extract_definition(case.x, case.thr, kind, case.window_or_half, case.shift, case.row_cap)
        w, overlap = _py_params(case)
        xd, td = _dev(case.x), _dev(case.thr)
        for capacity in (1, max(1, want.size), want.size + 1):
            got = th.extract_candidates(xd, td, w, overlap=overlap, row_cap=case.row_cap, capacity=capacity, kind=kind)
            if not tc.same_records(got, want):
                bad.append(f"{case.name} capacity {capacity}: {got.size} records, {want.size} wanted")
            found, first, clean = run_extract(kind, case.x, case.thr, case.window_or_half, case.shift, case.row_cap,
                                              capacity)
            if found != want.size or not clean or first.size != min(found, capacity):
                bad.append(f"{case.name} capacity {capacity}: count {found} of {want.size}, buffer behind clean: {clean}")
            if capacity >= want.size and not tc.same_records(first, want):
                bad.append(f"{case.name} capacity {capacity}: records of the single call differ")
            if capacity < want.size and not all(r in want.tolist() for r in first.tolist()):
                bad.append(f"{case.name} capacity {capacity}: a stored record is no candidate")
    assert bad == []


# ------------------------------------------------------------------------------------- Python entry point ---
def test_threshold_gpu_by_window_and_overlap_with_a_dirty_kept_workspace(oracle_lib):
    """ThresholdGPU.time_dependent_threshold by (sliding window, overlap) -- an odd window with overlap 0 among them,
    which gives shift = window + 1 -- each call after a larger one has left the kept workspace behind, filled with
    0xFF before the call under test."""
    from seismic_bpmf_amd.threshold import ThresholdGPU, window_params
    th = ThresholdGPU()
    big = tc.live_rows(99, 8, 6001)
    th.time_dependent_threshold(_dev(big), 64, 8.0, overlap=0.9, white_noise=tc.gauss_sample(1))
    kept = th._ws
    for k, (w, overlap) in enumerate(tc.OVERLAP_CASES):
        half, shift = window_params(w, overlap)
        x, gauss = tc.live_rows(200 + k, 3, 3 * w + 5), tc.gauss_sample(200 + k)
        kept.fill_(0xFF)
        tw, full = th.time_dependent_threshold(_dev(x), w, 8.0, overlap=overlap, white_noise=gauss, expand=True)
        assert th._ws is kept                       # (the larger workspace is reused, not replaced)
        d_win, d_full = tc.tdt_rms_definition(x, gauss, 8.0, half, shift)
        assert tc.same_values(tw.cpu().numpy(), d_win) and tc.same_values(full.cpu().numpy(), d_full), (w, overlap)
        for r in range(3):
            assert tc.same_values(d_full[r], oracle_lib.time_dependent_threshold(x[r], w, 8.0, overlap, gauss)), (w, r)


# ------------------------------------------------------------------------------------------------ refusals ---
def _valid_call_is_still_right():
    case = tc.tdt_case("stream_w34_s25")
    tw, full = run_tdt(case.x, case.gauss, case.num_dev, case.half, case.shift)
    d_win, d_full = tc.tdt_rms_definition(case.x, case.gauss, case.num_dev, case.half, case.shift)
    assert tc.same_values(tw, d_win) and tc.same_values(full, d_full)
    want = tc.extract_definition(case.x, d_win, "rms", case.half, case.shift, None)
    found, got, _ = run_extract("rms", case.x, tw, case.half, case.shift, None, want.size + 1)
    assert found == want.size and tc.same_records(got, want)


@pytest.mark.parametrize("name,n_rows,n,half,shift,expand,short_ws", tc.TDT_REFUSALS, ids=[r[0] for r in tc.TDT_REFUSALS])
def test_threshold_refusals_write_nothing(name, n_rows, n, half, shift, expand, short_ws):
    """-1 with a message, outputs and workspace untouched (every buffer has the size a valid call of these arguments
    would need, so nothing could be written out of bounds either), and a valid call afterwards is right."""
    import torch
    lib = _lib()
    alloc_rows = max(n_rows, 1)
    sizes = tc.tdt_sizes(n, half, shift)
    n_win = sizes[2] if sizes else 8
    need = lib.bpmf_tdt_workspace_bytes(alloc_rows, n, half, shift) if sizes else 4096
    assert (sizes is None) == (name in ("n_below_window", "shift_zero", "shift_above_window_plus_1"))
    xd = torch.full((alloc_rows, max(n, 2 * half)), 0.25, dtype=torch.float32, device="cuda")
    gd = _dev(tc.gauss_sample(3))
    ws, tw, full = _ff(need, torch.uint8), _ff((alloc_rows, n_win)), _ff((alloc_rows, n))
    rc = lib.bpmf_tdt_rms_dev(xd.data_ptr(), gd.data_ptr(), 8.0, n_rows, n, half, shift, ws.data_ptr(),
                              need - 1 if short_ws else need, _stream(), tw.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    msg = lib.bpmf_last_error().decode()
    assert rc == -1 and "bpmf_tdt_rms_dev" in msg, (rc, msg)
    if name == "65536_rows_expanded":
        assert "65535" in msg
    assert _untouched(tw) and _untouched(full) and _untouched(ws), name
    if name == "65536_rows_expanded":              # without the expansion any number of rows goes
        rc = lib.bpmf_tdt_rms_dev(xd.data_ptr(), gd.data_ptr(), 8.0, n_rows, n, half, shift, ws.data_ptr(), need,
                                  _stream(), tw.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0 and (tw[[0, n_rows - 1]].cpu().numpy() == np.float32(0.25)).all()
    _valid_call_is_still_right()


@pytest.mark.parametrize("name,kind,n_rows,n,window,shift", tc.EXTRACT_REFUSALS, ids=[r[0] for r in tc.EXTRACT_REFUSALS])
def test_extraction_refusals_write_nothing(name, kind, n_rows, n, window, shift):
    import torch
    lib = _lib()
    alloc_rows = max(n_rows, 1)
    xd = torch.ones((alloc_rows, max(n, window)), dtype=torch.float32, device="cuda")
    td = torch.zeros((alloc_rows, 64), dtype=torch.float32, device="cuda")
    count, rec = _ff(2, torch.int32), _ff((64, 4), torch.int32)
    fn = lib.bpmf_extract_candidates_dev if kind == "rms" else lib.bpmf_extract_candidates_mad_dev
    rc = fn(xd.data_ptr(), td.data_ptr(), None, n_rows, n, window // 2 if kind == "rms" else window, shift, 64,
            _stream(), count.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    msg = lib.bpmf_last_error().decode()
    assert rc == -1 and "bpmf_extract_candidates" in msg, (rc, msg)
    assert _untouched(count) and _untouched(rec), name
    _valid_call_is_still_right()
