"""GPU: the SVD-Wiener stack on the device (csrc/svdwf.hip; workflow.svdwf_stack, workflow.bandpass_filter) against
the definitions on the host (postprocess.svdwf_stack_host, bandpass_filter_host, themselves pinned to the reference
in tests/test_svdwf_host.py).

The limits are derived, not measured.  The device works in float64 on the Gram matrix of float32 data; under the
conditions tests/svdwf_cases.py:conditions asserts (retained sigma_j^2 separated by 1e-4 sigma_1^2, var away from
expl_var) its float64 result differs from the definition's by parts in 1e12, so what shows is the float32 rounding of
the stored values: two float64 numbers that close round to the same float32 or to neighbours, at most
2^-23 |value| <= 2^-23 of the channel's largest |filtered| apart -- the limit is 2^-22.  The stack adds the rounding of
the quotient and of the maximum it divides by: 2^-21 of the channel's largest |stack| (1 where the maximum is the
largest magnitude).  n_singular must be equal.  The worst figures seen are printed (profiles/svdwf_stack.txt).

The session runs with debug.poison_output on (tests/conftest.py) and the workspace is handed over full of junk."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svdwf_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

LIMIT_FILTERED = 2.0 ** -22
LIMIT_STACK = 2.0 ** -21
SECOND = [(0.4, 5, None, True), (0.8, 5, 4, False)]


def sweep(n):
    return [(ev, kmax, w, bp) for w in sc.window_sizes(n) for ev in sc.EXPL_VARS for kmax in sc.MAX_SINGULAR_VALUES
            for bp in (False, True)]


def single_group_cases():
    """(n, m, seed, S, C, [(expl_var, max_singular_values, w, band-pass), ...]) of every single-group test."""
    out = [(n, m, 3, 1, 1, sweep(n)) for n, m in sc.SMALL_SHAPES]
    out += [(n, m, 5, 1, 2, SECOND) for n, m in sc.MORE_SHAPES + [sc.LONG_SHAPE]]
    out += [(n, m, 7, 1, 1, SECOND[:1]) for n, m in sc.CAP_SHAPES]
    return out


def junk_workspace(n_bytes):
    import torch
    return torch.full((int(n_bytes),), 0xA5, dtype=torch.uint8, device="cuda")


def compare(got, want, off, label):
    """Device (stack, filtered, n_singular) against the host's; returns the worst (filtered, stack) deviations in
    units of their limits."""
    stack, filtered, rank = got
    want_filtered, want_stack, want_rank = want
    assert np.array_equal(rank, want_rank), (label, rank.ravel(), want_rank.ravel())
    worst_f = worst_s = 0.0
    G, S, Cc, m = want_stack.shape
    for g in range(G):
        for s in range(S):
            for c in range(Cc):
                hf = want_filtered[off[g]:off[g + 1], s, c]
                df = np.abs(filtered[off[g]:off[g + 1], s, c] - hf).max() / sc.scale(hf) if hf.size else 0.0
                ds = np.abs(stack[g, s, c] - want_stack[g, s, c]).max() / sc.scale(want_stack[g, s, c])
                assert df <= LIMIT_FILTERED, (label, g, s, c, df / LIMIT_FILTERED)
                assert ds <= LIMIT_STACK, (label, g, s, c, ds / LIMIT_STACK)
                worst_f, worst_s = max(worst_f, df / LIMIT_FILTERED), max(worst_s, ds / LIMIT_STACK)
    return worst_f, worst_s


def device(x, off=None, **kw):
    import torch
    from seismic_bpmf_amd import workflow
    from seismic_bpmf_amd import _lib
    sizes = np.diff(off) if off is not None else np.array([len(x)])
    n_bytes = _lib.lib().bpmf_svdwf_workspace_bytes(len(sizes), int(sizes.max()), x.shape[-1],
                                                    len(sizes) * x.shape[1] * x.shape[2])
    assert n_bytes > 0
    stack, filtered, rank, status = workflow.svdwf_stack(torch.as_tensor(x, device="cuda"), off,
                                                         workspace=junk_workspace(n_bytes), **kw)
    assert stack.dtype == torch.float32 and filtered.dtype == torch.float32 and stack.is_cuda and filtered.is_cuda
    assert not status.any()
    return stack.cpu().numpy(), filtered.cpu().numpy(), rank


def test_poison_is_on():
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1


@pytest.mark.parametrize("case", single_group_cases(), ids=lambda c: f"{c[0]}x{c[1]}")
def test_single_group_is_within_the_derived_limits(case):
    from seismic_bpmf_amd import postprocess as pp
    n, m, seed, S, Cc, params = case
    x = sc.group(n, m, seed, S, Cc)
    sos = sc.sos_table()
    off = np.array([0, n])
    worst = (0.0, 0.0)
    for expl_var, kmax, w, bandpass in params:
        kw = dict(expl_var=expl_var, max_singular_values=kmax, wiener_filter_colsize=w, sos=sos if bandpass else None)
        want = pp.svdwf_stack_host(x, **kw)
        if n == 1:
            assert np.abs(want[0]).max() > 0.1                       # (one event is not filtered away)
        worst = np.maximum(worst, compare(device(x, **kw), want, off, (n, m, expl_var, kmax, w, bandpass)))
    print(f"({n}, {m}): worst filtered {worst[0]:.3f} x 2^-22, stack {worst[1]:.3f} x 2^-21 of the channel scale")


def test_keywords_of_the_reference_call_and_no_filtered():
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    x = sc.group(7, 200, 9, 1, 2)
    want = pp.svdwf_stack_host(x, sos=sc.sos_table())
    x_dev = torch.as_tensor(x, device="cuda")
    stack, filtered, rank, status = workflow.svdwf_stack(x_dev, freqmin=sc.FREQMIN, freqmax=sc.FREQMAX,
                                                         sampling_rate=sc.SAMPLING_RATE, return_filtered=False)
    assert filtered is None
    full = device(x, sos=sc.sos_table())
    assert np.array_equal(stack.cpu().numpy().view(np.uint32), full[0].view(np.uint32))
    compare(full, want, np.array([0, 7]), "keywords")
    none = workflow.svdwf_stack(x_dev[:0], [0])
    assert tuple(none[0].shape) == (0, 1, 2, 200) and tuple(none[1].shape) == (0, 1, 2, 200)


@pytest.mark.parametrize("bandpass", [False, True])
def test_ragged_batch_equals_the_single_group_calls_bit_for_bit(bandpass):
    import torch
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    x, off = sc.ragged_batch()
    G, (N, S, Cc, m) = len(off) - 1, x.shape
    kw = dict(sos=sc.sos_table() if bandpass else None)
    want = pp.svdwf_stack_host(x, off, **kw)
    got = device(x, off, **kw)
    compare(got, want, off, "ragged")
    stack, filtered, rank = got
    g, s, c = sc.RAGGED_ZERO
    assert rank[g, s, c] == 0 and not stack[g, s, c].any() and not filtered[off[g]:off[g + 1], s, c].any()
    assert rank[2].tolist() == [[0] * Cc] * S and not stack[2].any()                     # the empty group
    g, s, c = sc.RAGGED_ZERO_COLUMNS
    assert not filtered[off[g]:off[g + 1], s, c, 10:13].any() or bandpass
    if not bandpass:
        g, s, c = sc.RAGGED_NEGATIVE
        assert (want[1][g, s, c] > 0).all() and (filtered[off[g]:off[g + 1], s, c] < 0).all()
        assert stack[g, s, c].min() == 1.0                                               # divided by the SIGNED maximum
    # every group on its own gives the same bits
    for g in range(G):
        alone = device(x[off[g]:off[g + 1]], **kw)
        assert np.array_equal(alone[0][0].view(np.uint32), stack[g].view(np.uint32)), g
        assert np.array_equal(alone[1].view(np.uint32), filtered[off[g]:off[g + 1]].view(np.uint32)), g
        assert np.array_equal(alone[2][0], rank[g])
    # a workspace of 8 slots: 24 channels in three slabs, handed over full of junk
    lib = _lib.lib()
    small = junk_workspace(lib.bpmf_svdwf_workspace_bytes(G, max(sc.RAGGED_SIZES), m, 8))
    assert lib.bpmf_svdwf_workspace_bytes(G, max(sc.RAGGED_SIZES), m, 9) > small.numel()
    again = workflow.svdwf_stack(torch.as_tensor(x, device="cuda"), off, workspace=small, **kw)
    assert np.array_equal(again[0].cpu().numpy().view(np.uint32), stack.view(np.uint32))
    assert np.array_equal(again[1].cpu().numpy().view(np.uint32), filtered.view(np.uint32))
    assert np.array_equal(again[2], rank) and not again[3].any()
    one = junk_workspace(lib.bpmf_svdwf_workspace_bytes(G, max(sc.RAGGED_SIZES), m, 1))
    again = workflow.svdwf_stack(torch.as_tensor(x, device="cuda"), off, workspace=one, **kw)
    assert np.array_equal(again[0].cpu().numpy().view(np.uint32), stack.view(np.uint32))


def test_launches_go_to_the_current_stream():
    import torch
    from seismic_bpmf_amd import workflow
    x = sc.group(7, 64, 11, 1, 2)
    want = device(x, sos=sc.sos_table())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x_dev = torch.as_tensor(x, device="cuda") * 1
        stack, filtered, _, _ = workflow.svdwf_stack(x_dev, sos=sc.sos_table())
        doubled = stack * 2
    side.synchronize()
    assert np.array_equal(stack.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(doubled.cpu().numpy(), want[0] * np.float32(2))


def test_a_sweep_cap_of_one_reports_not_converged(hip_opts):
    import torch
    from seismic_bpmf_amd import workflow
    x = sc.group(7, 64, 13, 1, 2)
    x[:, 0, 1] = 0.0                                                 # a zero matrix is diagonal already
    x_dev = torch.as_tensor(x, device="cuda")
    hip_opts("svdwf.max_sweeps", 1)
    with pytest.raises(RuntimeError, match="did not converge"):
        workflow.svdwf_stack(x_dev)
    stack, filtered, rank, status = workflow.svdwf_stack(x_dev, strict=False)
    assert status.tolist() == [[[1, 0]]] and rank.tolist() == [[[0, 0]]]
    assert not stack.cpu().numpy().any() and not filtered.cpu().numpy().any()
    hip_opts.reset("svdwf.max_sweeps")
    stack, _, rank, status = workflow.svdwf_stack(x_dev)
    assert status.tolist() == [[[0, 0]]] and rank[0, 0, 0] >= 1 and stack.cpu().numpy()[0, 0, 0].max() == 1.0


# ---- the band-pass on its own ----
@pytest.fixture(scope="module")
def tables():
    from seismic_bpmf_amd import postprocess as pp
    return {n: pp.butter_bandpass_sos(n, 0.1, 0.4) for n in range(1, 9)}


ROWS, DISTINCT = 70_000, 64


@pytest.mark.parametrize("m", [1, 2, 33, 257, 4097])
def test_plain_cascade_equals_the_definition_bit_for_bit(m, tables):
    """70 000 float64 rows (64 distinct ones, repeated: the rows are independent), 1 .. 8 sections, both zerophase
    settings: every row of the device result has the bits of the definition's."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    base = np.random.default_rng(m).standard_normal((DISTINCT, m))
    index = torch.arange(ROWS, device="cuda") % DISTINCT
    x_dev = torch.as_tensor(base, device="cuda")[index]
    for n_sections, sos in tables.items():
        for zerophase in (False, True):
            want = pp.bandpass_filter_host(base, sos, detrend=False, taper_alpha=None, zerophase=zerophase)
            got = workflow.bandpass_filter(x_dev, sos, detrend=False, taper_alpha=None, zerophase=zerophase)
            assert got.dtype == torch.float64 and tuple(got.shape) == (ROWS, m)
            want_dev = torch.as_tensor(want, device="cuda")[index]
            assert torch.equal(got.view(torch.int64), want_dev.view(torch.int64)), (m, n_sections, zerophase)
            del want_dev
            again = workflow.bandpass_filter(x_dev, sos, detrend=False, taper_alpha=None, zerophase=zerophase)
            for r in (1, ROWS // 2, ROWS - 1):
                assert np.array_equal(again[r].cpu().numpy().view(np.int64), want[r % DISTINCT].view(np.int64))


def test_full_bandpass_is_within_the_recorded_limit():
    """Mean, line, taper and cascade against bandpass_filter_host, within the limit the generator recorded for the
    definition against utils.bandpass_filter (8 x the measured deviation); float32 in and out; any leading shape."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd import workflow
    limit = float(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svdwf.npz"))
                  ["bandpass_limit"])
    for index, (rows, m, order, lo, hi) in enumerate(sc.BANDPASS_CASES):
        x = sc.bandpass_rows(index)
        kw = dict(freqmin=lo, freqmax=hi, f_Nyq=sc.SAMPLING_RATE / 2, filter_order=order)
        want = pp.bandpass_filter_host(x, **kw)
        got = workflow.bandpass_filter(torch.as_tensor(x, device="cuda"), **kw).cpu().numpy()
        dev = np.abs(got - want).max() / sc.scale(want)
        print(f"band-pass {sc.BANDPASS_CASES[index]}: {dev:.3e} (limit {limit:.3e})")
        assert dev <= limit
        x32 = x.astype(np.float32).reshape(rows, 1, m)
        want32 = pp.bandpass_filter_host(x32, **kw).astype(np.float32)
        got32 = workflow.bandpass_filter(torch.as_tensor(x32, device="cuda"), dtype=torch.float32, **kw)
        assert got32.dtype == torch.float32 and tuple(got32.shape) == (rows, 1, m)
        assert np.abs(got32.cpu().numpy() - want32).max() <= 2.0 ** -22 * sc.scale(want32)
        for zerophase in (False, True):
            for alpha in (None, 0.3):
                kw2 = dict(kw, zerophase=zerophase, taper_alpha=alpha, detrend=alpha is None)
                got = workflow.bandpass_filter(torch.as_tensor(x, device="cuda"), **kw2).cpu().numpy()
                want = pp.bandpass_filter_host(x, **kw2)
                assert np.abs(got - want).max() <= limit * sc.scale(want)


# ---- every refusal of the header ----
def test_refusals():
    import torch
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    n, m, S, Cc = 4, 32, 1, 2
    x = torch.zeros((n, S, Cc, m), dtype=torch.float32, device="cuda")
    sos = torch.as_tensor(sc.sos_table(), device="cuda")
    ws = junk_workspace(lib.bpmf_svdwf_workspace_bytes(1, n, m, 2))
    stack = torch.empty((1, S, Cc, m), dtype=torch.float32, device="cuda")
    filtered = torch.empty_like(x)
    rank = torch.empty((1, S, Cc), dtype=torch.int32, device="cuda")
    status = torch.empty_like(rank)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(off=(0, n), G=1, S_=S, C_=Cc, m_=m, ev=0.4, kmax=5, w=0, sos_=sos, n_sec=4, alpha=0.01, ws_=ws,
             ws_bytes=None, x_=x, stack_=stack, rank_=rank, status_=status):
        o = (C.c_int64 * len(off))(*off)
        return lib.bpmf_svdwf_stack_dev(p(x_), o, G, S_, C_, m_, ev, kmax, w, p(sos_), n_sec, alpha, p(ws_),
                                        ws_.numel() if ws_bytes is None and ws_ is not None else (ws_bytes or 0), None,
                                        p(filtered), p(stack_), p(rank_), p(status_))

    assert call() == 0
    torch.cuda.synchronize()
    assert call(G=0) == 0
    bad = [dict(x_=None), dict(stack_=None), dict(rank_=None), dict(status_=None), dict(ws_=None), dict(m_=0),
           dict(S_=0), dict(C_=0), dict(kmax=0), dict(kmax=9), dict(ev=0.0), dict(ev=1.01), dict(ev=float("nan")),
           dict(n_sec=9), dict(n_sec=0), dict(alpha=float("nan")), dict(w=65537), dict(off=(1, n)),
           dict(off=(0, 3, 2, 4), G=3), dict(off=(0, 513), m_=600), dict(off=(0, 600), m_=513),
           dict(off=(0, 16385), m_=8), dict(off=(0, 8), m_=16385), dict(S_=2**16, C_=2**15),
           dict(off=tuple(16384 * g for g in range(2**16 + 1)), G=2**16, m_=8),      # 2^30 events x 2 channels
           dict(ws_bytes=256)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "bpmf_svdwf_stack_dev" in _lib.last_error(), kw
    assert lib.bpmf_svdwf_workspace_bytes(1, 513, 600, 1) == 0 and lib.bpmf_svdwf_workspace_bytes(1, 8, 0, 1) == 0
    assert lib.bpmf_svdwf_workspace_bytes(1, 16385, 8, 1) == 0 and lib.bpmf_svdwf_workspace_bytes(2**31, 8, 8, 1) == 0
    assert lib.bpmf_svdwf_workspace_bytes(1, 512, 600, 1) > 0 and lib.bpmf_svdwf_workspace_bytes(1, 600, 512, 1) > 0

    rows = torch.zeros((3, m), dtype=torch.float64, device="cuda")
    out = torch.empty_like(rows)

    def filt(x_=rows, rows_=3, m_=m, sos_=sos, n_sec=4, alpha=0.01, zp=1, f64=1, ws_=None, ws_bytes=0, out_=out):
        return lib.bpmf_bandpass_rows_dev(p(x_), 1, rows_, m_, p(sos_), n_sec, 1, alpha, zp, f64, p(ws_), ws_bytes,
                                          None, p(out_))

    assert filt() == 0 and filt(rows_=0) == 0
    for kw in [dict(x_=None), dict(out_=None), dict(sos_=None), dict(m_=0), dict(m_=2**24 + 1), dict(rows_=2**31),
               dict(n_sec=0), dict(n_sec=9), dict(alpha=float("nan")), dict(f64=0), dict(f64=0, ws_=ws, ws_bytes=8)]:
        assert filt(**kw) == -1, kw
        assert "bpmf_bandpass_rows_dev" in _lib.last_error(), kw
    torch.cuda.synchronize()


def test_python_refusals():
    import torch
    from seismic_bpmf_amd import workflow
    x = torch.zeros((4, 1, 2, 32), dtype=torch.float32, device="cuda")
    for kw in (dict(expl_var=0.0), dict(max_singular_values=9), dict(wiener_filter_colsize=0),
               dict(offsets=[0, 3]), dict(offsets=[0, 3, 2, 4]), dict(sampling_rate=25.0),
               dict(workspace=torch.zeros(8, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            workflow.svdwf_stack(x, **kw)
    with pytest.raises(ValueError):
        workflow.svdwf_stack(x.cpu())
    with pytest.raises(ValueError):
        workflow.svdwf_stack(torch.zeros((513, 1, 1, 600), device="cuda"))
    with pytest.raises(ValueError):
        workflow.bandpass_filter(x.cpu(), sc.sos_table())
    with pytest.raises(ValueError):
        workflow.bandpass_filter(x)
    with pytest.raises(ValueError):
        workflow.bandpass_filter(x, np.ones((9, 6)))
