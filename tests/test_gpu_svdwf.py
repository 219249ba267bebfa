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

The limits hold for any spectrum that meets the conditions, not only the generic one of svdwf_cases.matrix: the
degenerate cases (zero and duplicated events, exact low rank, one event 1e4 x the others, scales of 1e-9 and 1e15,
constant traces) go through the same comparison, and the eigen-solve must converge on them in the sweeps its
definition (svdwf_cases.jacobi_reference) takes, + 2.  Two equal singular values carry the limits only where the
result is the projector onto their plane; elsewhere invariants.

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


def device(x, off=None, slots=None, workspace=None, **kw):
    """(stack, filtered, n_singular) of workflow.svdwf_stack in a workspace of `slots` channels (default: all) that is
    handed over full of junk; every status 0."""
    import torch
    from seismic_bpmf_amd import workflow
    from seismic_bpmf_amd import _lib
    sizes = np.diff(off) if off is not None else np.array([len(x)])
    n_bytes = _lib.lib().bpmf_svdwf_workspace_bytes(len(sizes), int(sizes.max()), x.shape[-1],
                                                    slots or len(sizes) * x.shape[1] * x.shape[2])
    assert n_bytes > 0
    workspace = junk_workspace(n_bytes) if workspace is None else workspace
    assert workspace.numel() == n_bytes
    stack, filtered, rank, status = workflow.svdwf_stack(torch.as_tensor(x, device="cuda"), off, workspace=workspace,
                                                         **kw)
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


# ---- degenerate spectra: rank-deficient, duplicated, badly scaled and clustered matrices (svdwf_cases.py) ----
# tests/test_svdwf_host.py asserts of every case that it meets `conditions` (so the derived limits hold unchanged), that
# the definition is stable on it and what the documented solver needs for it.
DEGENERATE = sc.degenerate_cases()
DEGENERATE_SOLVED = [case for case in DEGENERATE if min(case[1].shape) <= sc.JACOBI_REFERENCE_MAX_K]


def keywords(params):
    expl_var, kmax, w, bandpass = params
    return dict(expl_var=expl_var, max_singular_values=kmax, wiener_filter_colsize=w,
                sos=sc.sos_table() if bandpass else None)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint32), np.ascontiguousarray(v).view(np.uint32))
               for u, v in zip(a, b))


def solver_sweeps(workspace, n, m):
    """The sweeps the eigen-solve of the first slot took, read from the workspace of a single-group, single-channel
    call.  This restates the layout of csrc/svdwf.hip -- the 256-byte head of the offsets, the tables of sv_sizes in
    front of o_small, SM_SWEEPS = 27 -- and goes wrong silently when that changes: the figure is printed for
    profiles/svdwf_stack.txt and never asserted."""
    import torch
    Kp = min(n, m) + (min(n, m) & 1)
    o_small = 2 * Kp * Kp + 3 * 8 * n + 8 * m + 2 * n * m + m
    return int(workspace[256:].view(torch.float64)[o_small + 27].item())


@pytest.mark.parametrize("case", [c for c in DEGENERATE if c[0] != sc.EQUAL_SIGMA], ids=lambda c: c[0])
def test_degenerate_spectra_within_the_derived_limits(case):
    from seismic_bpmf_amd import postprocess as pp
    label, a, params = case
    x = a[:, None, None, :]
    off = np.array([0, len(a)])
    worst, ranks = (0.0, 0.0), []
    for p in params:
        want = pp.svdwf_stack_host(x, **keywords(p))
        got = device(x, **keywords(p))                                # (asserts status 0 at the default cap)
        worst = np.maximum(worst, compare(got, want, off, (label, p)))
        ranks.append(int(got[2][0, 0, 0]))
        if label.startswith("one event") and p[2] != 1:
            # each event against its own largest |filtered|: the second pass's running sums carry the large event
            # through every window.  No limit is derived for this figure; it is printed only.
            hf = want[0][:, 0, 0].astype(np.float64)
            rows = np.abs(got[1][:, 0, 0] - hf).max(axis=1) / np.abs(hf).max(axis=1)
            print(f"{label} {p}: worst per-row deviation {rows.max() / LIMIT_FILTERED:.2e} x 2^-22 of the row's scale "
                  f"(row {int(rows.argmax())})")
    print(f"{label}: worst filtered {worst[0]:.3f} x 2^-22, stack {worst[1]:.3f} x 2^-21 of the channel scale, "
          f"n_singular {ranks}")


def test_clustered_singular_values():
    """sigma_1 = sigma_2 exactly.  With both retained and no Wiener filter the result is the projector onto their
    plane: unique, the derived limits hold (svdwf_cases.conditions_subspace).  Cut by k, or filtered projection by
    projection, the definition depends on the vectors a solver happens to return from that plane (two routes on the
    host differ by the whole channel scale, tests/test_svdwf_host.py): status, n_singular, finiteness and
    repeatability are what is left to assert."""
    from seismic_bpmf_amd import postprocess as pp
    a = sc.equal_sigma_matrix()
    x = a[:, None, None, :]
    off = np.array([0, len(a)])
    seen = set()
    for p in sc.degenerate_params(len(a)):
        want = pp.svdwf_stack_host(x, **keywords(p))
        got = device(x, **keywords(p))                                # (asserts status 0)
        if p[0] == 0.8 and p[2] == 1:
            assert sc.conditions_subspace(a, p[0], p[1]) == 2
            worst = compare(got, want, off, (sc.EQUAL_SIGMA, p))
            print(f"{sc.EQUAL_SIGMA} {p}: worst filtered {worst[0]:.3f} x 2^-22, stack {worst[1]:.3f} x 2^-21 of the "
                  f"channel scale, n_singular {int(got[2][0, 0, 0])}")
            seen.add("unique")
            continue
        assert np.array_equal(got[2], want[2]), (p, got[2].ravel(), want[2].ravel())
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), p
        again = device(x, **keywords(p))
        assert same_bits(got[:2], again[:2]) and np.array_equal(got[2], again[2]), p
        seen.add("cut" if p[0] == 0.4 else "one by one")
    assert seen == {"unique", "cut", "one by one"}


@pytest.mark.parametrize("case", DEGENERATE_SOLVED, ids=lambda c: c[0])
def test_sweeps_follow_the_definition(case, hip_opts):
    """With the cap at the sweeps of svdwf_cases.jacobi_reference (the header's solver in float64 NumPy) + 2 the
    channel converges, to the bits it has at the default cap.  The 2 are for the last confirming sweeps, whose
    rotations at rounding level depend on the order the Gram matrix was summed in."""
    from seismic_bpmf_amd import _lib
    label, a, params = case
    n, m = a.shape
    x = a[:, None, None, :]
    kw = keywords(params[0])
    sweeps, status, _ = sc.jacobi_reference(sc.gram(a))
    assert status == 0
    n_bytes = _lib.lib().bpmf_svdwf_workspace_bytes(1, n, m, 1)
    workspace = junk_workspace(n_bytes)
    want = device(x, workspace=workspace, **kw)
    took = solver_sweeps(workspace, n, m)
    print(f"{label}: the definition takes {sweeps} sweeps, the device {took}")
    hip_opts("svdwf.max_sweeps", sweeps + 2)
    got = device(x, **kw)                                             # (asserts status 0)
    assert same_bits(want[:2], got[:2]) and np.array_equal(want[2], got[2])


def degenerate_batch():
    """Five groups, S x C = 1 x 2: events without data, duplicated events, no events, one event x 1e4, seven identical
    events; the second channel holds the first one's samples in reverse.  Returns (x, offsets)."""
    by_label = {label: a for label, a, _ in DEGENERATE}
    groups = [by_label["zero rows 40x200"], by_label["duplicated rows 40x200"], np.zeros((0, 200), np.float32),
              by_label["one event x 1e4 40x200"], by_label["identical rows 7x200"]]
    x = np.concatenate([np.stack([a, a[:, ::-1]], axis=1)[:, None] for a in groups], axis=0)
    return np.ascontiguousarray(x), np.concatenate(([0], np.cumsum([len(a) for a in groups]))).astype(np.int64)


def test_degenerate_groups_in_a_ragged_batch():
    x, off = degenerate_batch()
    G = len(off) - 1
    assert x.shape == (127, 1, 2, 200) and G == 5
    kw = keywords(sc.degenerate_params(40)[0])
    whole = device(x, off, **kw)
    assert (whole[2][[0, 1, 3, 4]] > 0).all() and not whole[2][2].any() and not whole[0][2].any()
    for g in range(G):
        alone = device(x[off[g]:off[g + 1]], **kw)
        assert same_bits((alone[0][0], alone[1]), (whole[0][g], whole[1][off[g]:off[g + 1]])), g
        assert np.array_equal(alone[2][0], whole[2][g]), g
    for slots in (3, 1):
        again = device(x, off, slots=slots, **kw)
        assert same_bits(again[:2], whole[:2]) and np.array_equal(again[2], whole[2]), slots


def test_a_non_finite_channel_stays_in_its_channel():
    """One NaN, then one +Inf, in one channel of a batch: its Gram matrix has a diagonal element that is not finite,
    the channel is not solved and reports status 1 with zero outputs; every other channel has the bits it has without
    the bad sample.  Tried in the 7-event group and in the 2-event one, whose only pair of rows the rotation
    criterion would skip with an Inf on the diagonal (|Inf| <= 2^-52 sqrt(Inf) sqrt(g_qq)) and call converged."""
    import torch
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd import workflow
    sizes = (7, 2)
    off = np.array([0, 7, 9])
    x = np.concatenate([sc.group(n, 64, 60 + g, 1, 2) for g, n in enumerate(sizes)], axis=0)
    kw = dict(sos=sc.sos_table())
    clean = device(x, off, **kw)
    n_bytes = _lib.lib().bpmf_svdwf_workspace_bytes(2, 7, 64, 4)

    def run(bad_value, row, g_bad, c_bad):
        bad = x.copy()
        bad[row, 0, c_bad, 10] = bad_value
        bad_dev = torch.as_tensor(bad, device="cuda")
        stack, filtered, rank, status = workflow.svdwf_stack(bad_dev, off, strict=False,
                                                             workspace=junk_workspace(n_bytes), **kw)
        stack, filtered = stack.cpu().numpy(), filtered.cpu().numpy()
        for g in range(2):
            rows = slice(off[g], off[g + 1])
            for c in range(2):
                if (g, c) == (g_bad, c_bad):
                    assert status[g, 0, c] == 1 and rank[g, 0, c] == 0, (bad_value, row)
                    assert not stack[g, 0, c].any() and not filtered[rows, 0, c].any(), (bad_value, row)
                    continue
                assert status[g, 0, c] == 0 and rank[g, 0, c] == clean[2][g, 0, c], (bad_value, row, g, c)
                assert same_bits((stack[g, 0, c], filtered[rows, 0, c]),
                                 (clean[0][g, 0, c], clean[1][rows, 0, c])), (bad_value, row, g, c)
        with pytest.raises(RuntimeError, match="did not converge"):
            workflow.svdwf_stack(bad_dev, off, **kw)

    run(np.nan, 3, 0, 1)
    run(np.inf, 3, 0, 1)
    run(np.nan, 8, 1, 0)
    run(np.inf, 7, 1, 0)
    run(-np.inf, 8, 1, 1)


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
