"""GPU: the feature stages past their first slab of rows and at their argument ceilings -- the envelope in several
batches, more than 65535 rows through the saturated envelopes, the row median / MAD, the row kurtosis and the running
kurtosis, the MAD threshold in slabs that reuse one workspace, the running kurtosis at the largest window it accepts.
Cases and checks: seam_cases.py (test_batch_seams_host.py shows that each check rejects a planted slab defect).

Every output here comes from torch.empty / torch.zeros inside a wrapper, and the caching allocator hands back the
block the previous, identical call filled with the right answer.  So the call that crosses a seam is the FIRST call on
its input, and just before it `_junk` allocates and frees 0xFF-filled tensors shaped like the wrapper's outputs and
workspace: a slab that no kernel writes then holds junk, not answers.  Calls used for comparison come afterwards.

Lines starting with "SEAM" are the measurements profiles/batch_seams.txt records (pytest -s)."""
import numpy as np
import pytest

import seam_cases as sc

pytestmark = pytest.mark.gpu


def _junk(*specs):
    """Allocate tensors of the given (shape, dtype), fill them with 0xFF bytes, free them."""
    import torch
    held = []
    for shape, dtype in specs:
        t = torch.empty(shape, dtype=dtype, device="cuda")
        if t.numel():
            t.view(torch.uint8).fill_(0xFF)
        held.append(t)
    del held


def _envelope_junk(n, per_batch, real):
    import torch
    cplx = torch.complex128 if real == torch.float64 else torch.complex64
    _junk(((5, n), torch.float32), ((per_batch, n), real), ((per_batch, n // 2 + 1), cplx), ((per_batch, n), real),
          ((per_batch, n), real))


# -------------------------------------------------------------------------- envelope ---
@pytest.mark.parametrize("n", sc.ENVELOPE_N)
def test_envelope_in_several_batches(n):
    """envelope() over 5 channels in 5, 2 + 2 + 1 and 1 batches, on float32 traces (the fused kernels on slices of the
    trace and the output) and on a float64 copy (the tensor expressions); envelope_c2c in batches of 2.  Each result
    within 1.0001 ulp of the float64 SciPy envelope rounded to float32.  Bit equality between batch counts is printed,
    not asserted: the FFT library may plan another kernel for another batch count."""
    import torch
    from seismic_bpmf_amd.features import envelope, envelope_c2c
    tr = sc.envelope_traces(n)
    for name, make in (("float32 fused", lambda: torch.as_tensor(tr, device="cuda")),
                       ("float64 tensor", lambda: torch.as_tensor(tr, device="cuda").double())):
        outs = {}
        for per_batch in (2, 1, 5):                       # (the one-batch call, the comparison, comes last)
            x = make()
            _envelope_junk(n, per_batch, torch.float64)
            outs[per_batch] = envelope(x, channels_per_batch=per_batch).cpu().numpy()
            assert sc.check_envelope(outs[per_batch], tr, per_batch) == [], (name, n, per_batch)
        print(f"SEAM envelope n={n} {name}: batches of 1 / 2 equal the single batch bit for bit: "
              f"{np.array_equal(outs[1], outs[5])} / {np.array_equal(outs[2], outs[5])}")
    x = torch.as_tensor(tr, device="cuda")
    _junk(((5, n), torch.float32), ((2, n), torch.float64), ((2, n), torch.complex128), ((2, n), torch.complex128))
    got = envelope_c2c(x, channels_per_batch=2).cpu().numpy()
    assert sc.check_envelope(got, tr, 2) == [], n


@pytest.mark.parametrize("n", sc.ENVELOPE_F32_N)
def test_envelope_float32_precision_against_the_reference_route(n):
    """envelope(precision="float32"), never called by a test before, in batches of 2 and in one: per channel within
    max(4 x the error of the reference's own float32 route, 4 ulp of the channel maximum) of the float64 envelope
    (seam_cases.check_envelope_f32 says where the 4s come from).  The reference route's error is measured here, on
    the host: up to 2.3 ulp of the channel maximum at n = 16, 8.4 at 1001, 10.8 at 20 000, 25.5 at 131 071, the
    channel with the offset being the worst."""
    import torch
    from seismic_bpmf_amd.features import envelope
    tr = sc.envelope_traces(n)
    for per_batch in (2, None):
        x = torch.as_tensor(tr, device="cuda")
        _envelope_junk(n, per_batch or 5, torch.float32)
        got = envelope(x, channels_per_batch=per_batch, precision="float32").cpu().numpy()
        dev, ref = sc.envelope_f32_errors(got, tr)
        print(f"SEAM envelope float32 n={n} batches of {per_batch or 5}: device error per channel "
              f"{np.array2string(dev, precision=2)} ulp of the channel maximum, reference route "
              f"{np.array2string(ref, precision=2)}")
        assert sc.check_envelope_f32(got, tr, per_batch or 5) == [], (n, per_batch, dev, ref)


# ---------------------------------------------------------------- saturated envelopes ---
def test_saturated_envelopes_over_more_than_65535_channels():
    """(21 846, 3, 16): 65 538 channels -- two batches of the envelope, two slabs of the row statistics'
    one-workgroup launch's rows and of bpmf_saturate_rows_dev -- with gapped, all-zero, mostly missing and
    below-threshold channels on both sides of row 65 535.  Sampled channels against the reference's restatement, the
    availability over all stations, and every sample against the element-wise float32 formulation in torch."""
    import torch
    from seismic_bpmf_amd.features import envelope, row_median_mad, saturated_envelopes
    tr = sc.saturated_traces()
    rows, n = sc.SAT_ROWS, sc.SAT_SHAPE[2]
    x = torch.as_tensor(tr, device="cuda")
    _junk(((rows, n), torch.float32), ((rows,), torch.float32), ((rows,), torch.float32), ((rows,), torch.int64),
          ((rows,), torch.int32), ((rows,), torch.bool), ((256,), torch.uint8),
          ((sc.ROW_LIMIT, n), torch.float64), ((sc.ROW_LIMIT, n // 2 + 1), torch.complex128))
    feat, avail = saturated_envelopes(x, max_dynamic_range=1.0e5)
    feat_h = feat.cpu().numpy()
    assert sc.check_saturated(feat_h, avail, tr, sc.ROW_LIMIT) == []
    # (the comparison calls, after the one under test)
    env = envelope(x).reshape(rows, n)
    median, mad, n_missing = row_median_mad(env, skip_zeros=True)
    dead = (n_missing.to(torch.float64) > n / 2) | ~(mad.to(torch.float64) >= 1.0e-11)
    std = (env - median[:, None]) / mad[:, None]
    std = torch.where(env == 0.0, torch.zeros((), device=env.device), std)
    want = torch.where(dead[:, None], torch.zeros((), device=env.device),
                       torch.minimum(std, torch.tensor(1.0e5, dtype=torch.float32, device=env.device)))
    bad = ~np.all(np.equal(feat_h.reshape(rows, n), want.cpu().numpy()), axis=1)
    assert not bad.any(), np.flatnonzero(bad)[:10]
    assert np.array_equal(avail, (~dead).reshape(-1, 3).sum(dim=1).cpu().numpy())
    assert sc.check_envelope(env.cpu().numpy()[sc.saturated_sample()], tr.reshape(rows, n)[sc.saturated_sample()], sc.ROW_LIMIT) == []


# ------------------------------------------------------------------- row median / MAD ---
@pytest.mark.parametrize("route", ["one_workgroup", "two_read"])
@pytest.mark.parametrize("skip_zeros", [False, True])
def test_row_median_mad_over_more_than_65535_rows(hip_opts, skip_zeros, route):
    """(65 538, 64) with zeros, ties, a -0.0 and a NaN row on both sides of row 65 535.  As is, rows of 64 take the
    one-workgroup route: a single launch, no seam, here for the row count.  With stats.row_grid_min_n = 0 they take
    the two-read route, whose loop over slabs of 65 535 rows -- one workspace carved again for the last 3 rows, the
    outputs advanced by r0 -- is the one under test."""
    import torch
    from seismic_bpmf_amd import _lib, features
    x = sc.stats_rows()
    rows, n = x.shape
    if route == "two_read":
        hip_opts("stats.row_grid_min_n", 0)
    ws_bytes = int(_lib.lib().bpmf_row_median_mad_workspace_bytes(rows, n))
    if route == "two_read":
        # 6.45 GB (65 535 rows x (4096 + 16384 floats of collection buffers + a 4096-bin histogram)): 2 % of the card
        assert 5.0e9 < ws_bytes < 8.0e9, ws_bytes
    else:
        assert ws_bytes == 256
    xd = torch.as_tensor(x, device="cuda")
    _junk(((rows,), torch.float32), ((rows,), torch.float32), ((rows,), torch.int64), ((ws_bytes,), torch.uint8))
    med, mad, nz = (t.cpu().numpy() for t in features.row_median_mad(xd, skip_zeros))
    assert sc.check_row_stats(med, mad, nz, x, skip_zeros, sc.ROW_LIMIT) == []
    # every row, against the vectorised host formulation (which the sample above holds against np.median)
    wm, wd, wz = sc.stats_definition(x, skip_zeros)
    assert np.array_equal(med, wm, equal_nan=True) and np.array_equal(mad, wd, equal_nan=True) and np.array_equal(nz, wz)


# ----------------------------------------------------------------------- row kurtosis ---
def test_row_excess_kurtosis_over_more_than_65535_rows():
    """(65 538, 40) with a constant row (NaN) on each side of row 65 535: two calls of the library on one workspace.
    SciPy one series at a time on the sampled rows, bit for bit; every row against the host mirror."""
    import torch
    from seismic_bpmf_amd import _lib, workflow
    x = sc.rowkurt_rows()
    rows, n = x.shape
    ws_bytes = int(_lib.lib().bpmf_row_kurtosis_workspace_bytes(sc.ROW_LIMIT, n))
    xd = torch.as_tensor(x, device="cuda")
    _junk(((rows, 3), torch.float32), ((ws_bytes,), torch.uint8))
    got = workflow.row_excess_kurtosis(xd)
    assert sc.check_row_kurtosis(got, x, sc.ROW_LIMIT) == []
    assert np.array_equal(got, sc.rowkurt_definition(x), equal_nan=True)


# ---------------------------------------------------------------------- MAD threshold ---
@pytest.mark.parametrize("route", ["default", "tables_from_row_statistics"])
@pytest.mark.parametrize("n,W,overlap", sc.MAD_CASES)
def test_mad_threshold_in_slabs(hip_opts, n, W, overlap, route):
    """7 rows in slabs of 1, 2, 3 (3 + 3 + 1) and 7 rows, by a mad_workspace_limit of so many times the library's
    bytes per row: window values and expanded threshold equal the host mirror row by row, bit for bit, and so do the
    candidates extracted from them.  One ThresholdGPU per slab size, and one kept across all sizes, whose workspace
    stays as large as the largest call made it and holds the previous slabs' rank tables under the last, differently
    carved slab.  On the default statistics route (tdt_mad_count_kernel fills the zero-rank tables) and with
    stats.row_grid_min_n = 4096 (rm_hist_kernel<true> fills them: the tables_done branch, zc + r0 * n_fill)."""
    import torch
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd.threshold import ThresholdGPU, mad_rows_per_call
    if route == "tables_from_row_statistics":
        hip_opts("stats.row_grid_min_n", 4096)
    lib = _lib.lib()
    x, wn = sc.mad_rows(n)
    shift = sc.mad_shift(W, overlap)
    n_win = int(lib.bpmf_tdt_mad_num_windows(n, W, shift))
    per_row = int(lib.bpmf_tdt_mad_workspace_bytes(64, n, W, shift)) // 64
    want_full = sc.mad_definition(x, W, overlap, wn)[1]
    kept = ThresholdGPU()
    for th, slabs in [(None, (3, 1, 2, 7)), (kept, (3, 7, 1, 2, 3))]:
        for slab in slabs:
            t = th or ThresholdGPU()
            t.mad_workspace_limit = sc.mad_limit(per_row, slab)
            assert mad_rows_per_call(sc.MAD_ROWS, per_row, t.mad_workspace_limit) == slab
            xd = torch.as_tensor(x, device="cuda")
            ws_bytes = int(lib.bpmf_tdt_mad_workspace_bytes(slab, n, W, shift))
            _junk(((sc.MAD_ROWS, n_win), torch.float32), ((sc.MAD_ROWS, n), torch.float32), ((ws_bytes,), torch.uint8))
            thr_win, full = t.time_dependent_threshold_mad(xd, W, sc.MAD_NUM_DEV, overlap=overlap, white_noise=wn)
            what = (n, W, overlap, route, slab, "kept" if th else "fresh")
            assert sc.check_mad_threshold(thr_win.cpu().numpy(), full.cpu().numpy(), x, wn, W, overlap, slab) == [], what
            assert t._ws.numel() >= ws_bytes
            cand = t.extract_candidates(xd, thr_win, W, overlap=overlap, row_cap=sc.MAD_ROW_CAP, kind="mad", capacity=64)
            assert sc.check_mad_candidates(cand, x, want_full, slab) == [], what
    assert kept._ws.numel() >= int(lib.bpmf_tdt_mad_workspace_bytes(7, n, W, shift))


# ------------------------------------------------------------------- running kurtosis ---
@pytest.mark.parametrize("W", sc.KURT_CEILING_W)
def test_running_kurtosis_at_its_window_ceiling(W):
    """W = 16 128 (64 KB of dynamic LDS exactly), 16 129 (the first window above 64 KB) and 32 768 (the largest the
    library accepts: 132 096 bytes): (1, 2, W + 300) with channel scales 1 and 30 and a flat stretch longer than W;
    one output sample (length W + 1); none (length W: the caller's zeros stay).  The oracle, bit for bit."""
    import torch
    from seismic_bpmf_amd.features import kurtosis
    for length in (None, W + 1, W):
        x = sc.kurt_ceiling_signal(W, length)
        assert x.shape[-1] == (length or W + 300)
        xd = torch.as_tensor(x, device="cuda")
        _junk((x.shape, torch.float32))
        got = kurtosis(xd, W).cpu().numpy()
        assert sc.check_running_kurtosis(got, x, W, 1) == [], (W, length)
        written = int((got[..., W:] != 0).sum())          # (the flat windows, and one with too small a variance, stay 0)
        assert written == 2 if length == W + 1 else written == 0 if length == W else 540 <= written < 600


def test_running_kurtosis_refuses_a_window_above_its_ceiling():
    """W = 32 769 is one more than include/bpmf_hip.h allows: an error from the argument check, nothing launched, the
    output left at its zeros."""
    import torch
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd.features import kurtosis
    W = sc.KURT_W_MAX + 1
    x = torch.ones((1, 1, W + 8), device="cuda")
    with pytest.raises(_lib.BpmfHipError, match=f"W={W}"):
        kurtosis(x, W)
    torch.cuda.synchronize()


def test_running_kurtosis_over_more_than_65535_channels():
    """(21 846, 3, 40), W = 5: features.kurtosis hands the library 65 535 channels and then 3.  The oracle on every
    channel, bit for bit."""
    import torch
    from seismic_bpmf_amd.features import kurtosis
    x = sc.kurt_many_signal()
    xd = torch.as_tensor(x, device="cuda")
    _junk((x.shape, torch.float32))
    got = kurtosis(xd, sc.KURT_MANY_W).cpu().numpy()
    assert sc.check_running_kurtosis(got, x, sc.KURT_MANY_W, sc.ROW_LIMIT) == []
    assert (got[..., sc.KURT_MANY_W:] != 0).all()
