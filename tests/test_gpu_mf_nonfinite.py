"""GPU: the matched filter on non-finite samples (a NaN-filled gap, a clipped +-Inf, a 3e38) -- every kernel family,
selected as tests/test_gpu_f64_anchor.py selects them and asserted through bpmf_mf_launch_info, against the written rule
of tests/nonfinite_cases.py (tests/test_nonfinite_host.py holds the oracle to that rule and the checkers to planted
defects).

* exact families: equal to the oracle on the poisoned day (NaN-ness compared) except within R samples in front of a bad
  sample, where a kernel may return NaN; every channel without a bad sample, and every CLEAN lag of one with it, has the
  bits of the cleaned day.
* full mode: the float64 definition on CLEAN windows (evaluated on the cleaned day: zeros add nothing to the sum of the
  finite samples, so its constant c IS the poisoned day's, and its input conditions hold on every window), exactly 0 on
  every other class, the cleaned day's bits where nothing bad is near.
* mf.split16 = 2 at one, two and three segments: exact classes exact, the bar on CLEAN, never an Inf, the cleaned day's bits.
* the acceptance test: one NaN in one of nine channels in counts does not cost the detection.
The suite's poisoned outputs make an unwritten element NaN: NEAR is the only place where a skipped store could hide.
Every family prints its observed reach and NaN count (pytest -rP; profiles/mf_nonfinite.txt).
"""
import functools

import numpy as np
import pytest

import mf_full_definition as mfd
import nonfinite_cases as nc
from mf_launch import assert_takes

pytestmark = pytest.mark.gpu

FULL = 4


# ------------------------------------------------------------------------------------------- plumbing ---
def _host(case, ns, **kw):
    from seismic_bpmf_amd import matched_filter
    return matched_filter(*case.args, case.step, arch="gpu", check_zeros=False, network_sum=ns, device=0, **kw)


def _host_full(case, ns):
    import seismic_bpmf_amd as sb
    return sb.matched_filter_full(*case.args, case.step, arch="gpu", check_zeros=False, network_sum=ns, device=0)


def _resident(case, ns, **kw):
    from seismic_bpmf_amd import MatchedFilterGPU
    eng = MatchedFilterGPU(device=0)
    eng.set_data(case.data)
    first = eng.run(case.tp, case.mv, case.w, case.step, network_sum=ns, **kw).cpu().numpy()
    again = eng.run(case.tp, case.mv, case.w, case.step, network_sum=ns, **kw).cpu().numpy()      # on the prepared day
    assert np.array_equal(first, again, equal_nan=True), case.name
    return again


@functools.lru_cache(maxsize=None)
def _want(oracle_lib, L, step, T, align, flags):
    """The oracle on every poisoned case of a shape, both output forms: computed once, shared, never changed."""
    out = {}
    for case in nc.cases(L, step, T=T, align=align):
        with oracle_lib.compat(flags):
            out[case.name] = tuple(oracle_lib.matched_filter(*case.args, step, network_sum=ns) for ns in (True, False))
        for a in out[case.name]:
            a.setflags(write=False)
    return out


def _exact_family(oracle_lib, label, L, step, takes, run=_host, T=2, align=False, oracle_flags=0, launch_flags=0, **run_kw):
    """Every case of the shape through one exact family; R from the family the launch is asserted to take."""
    R = nc.reach("direct" if takes.get("family") == "direct" else "mfma", L)
    assert R < nc.R_LIMIT
    want = _want(oracle_lib, L, step, T, align, oracle_flags)
    n_near = n_nan = worst = 0
    for case in nc.cases(L, step, T=T, align=align):
        assert min(case.valid_lags()) >= nc.MIN_LAGS, case.name
        cls = case.classes(R)
        for ns in (True, False):
            assert_takes(case.tp.shape, case.N, step, ns, flags=launch_flags,
                         **{k: v(ns) if callable(v) else v for k, v in takes.items()})
            got = run(case, ns, **run_kw)
            what = f"{label}: {case.name} network_sum={ns}"
            k = nc.check_exact(got, want[case.name][0 if ns else 1], cls, R, what)
            if not ns:
                n_nan += k
                n_near += int((cls == nc.NEAR).sum())
                worst = max(worst, nc.observed_reach(got, want[case.name][1], case, R))
                nc.check_invariance(got, run(nc.cleaned(case), ns, **run_kw), cls, what)
    assert worst <= R
    print(f"mf-nonfinite {label} L={L} step={step}: R = {R}, largest observed reach {worst}, "
          f"{n_nan} of {n_near} NEAR entries came back NaN")


# ------------------------------------------------------------------------------------- exact families ---
@pytest.mark.parametrize("ntile", [1, 2, 4])
def test_wave_kernel_tiles(oracle_lib, hip_opts, ntile):
    hip_opts("mf.tiles_per_wave", ntile)
    takes = dict(family="wave", ntile=ntile)
    _exact_family(oracle_lib, f"wave ntile={ntile}", 200, 1, takes, align=True)         # Kpad - L = 24
    _exact_family(oracle_lib, f"wave ntile={ntile}", 64, 3, takes)                      # 16


@pytest.mark.parametrize("fused", [1, 0])
def test_wave_kernel_fused_and_separate_prologue(oracle_lib, hip_opts, fused):
    hip_opts("mf.tiles_per_wave", 1)
    hip_opts("mf.fused_prologue", fused)
    takes = dict(family="wave", ntile=1, fused=bool(fused), prologue=not fused)
    _exact_family(oracle_lib, f"wave fused={fused}", 64, 3, takes)
    _exact_family(oracle_lib, f"wave fused={fused}", 257, 1, takes)                     # Kpad - L = 15, the least


def test_wave_kernel_channel_split(oracle_lib, hip_opts):
    hip_opts("mf.channel_split", 1 << 20)
    hip_opts("mf.tiles_per_wave", 1)
    takes = dict(family="wave", ntile=1, fused=True, csplit=lambda ns: ns)
    _exact_family(oracle_lib, "wave channel split", 200, 1, takes, align=True)
    _exact_family(oracle_lib, "wave channel split resident", 200, 1, takes, run=_resident, align=True)


@pytest.mark.parametrize("L,step,maxr,maxt", [(300, 1, 20, 5), (1100, 3, 24, 9)])
def test_workgroup_kernel(oracle_lib, L, step, maxr, maxt):
    _exact_family(oracle_lib, f"workgroup maxr={maxr}", L, step, dict(family="workgroup", maxr=maxr, maxt=maxt),
                  align=L == 300)                                                       # Kpad - L = 20 and 20


def test_workgroup_kernel_on_short_templates(oracle_lib, hip_opts):
    hip_opts("mf.wave_kernel", 0)
    _exact_family(oracle_lib, "workgroup L=242", 242, 1, dict(family="workgroup", maxr=20, maxt=5))   # Kpad - L = 30, the most


def test_generic_kernel(oracle_lib, hip_opts):
    _exact_family(oracle_lib, "generic L > 2065", 2100, 1, dict(family="direct"))
    hip_opts("mf.max_mfma_step", 0)                    # every step is a large step: the generic kernel at an MFMA length
    _exact_family(oracle_lib, "generic, step beyond mf.max_mfma_step", 64, 3, dict(family="direct"))


def test_host_call_in_small_batches_and_pieces(oracle_lib, hip_opts):
    hip_opts("mf.host_batch_kb", 1)
    hip_opts("mf.host_piece_kb", 1)
    _exact_family(oracle_lib, "host batches 1 KB pieces 1 KB", 64, 3, dict(), T=3)
    hip_opts("mf.host_batch_kb", 64)
    hip_opts("mf.host_piece_kb", 16)
    _exact_family(oracle_lib, "host batches 64 KB pieces 16 KB", 200, 1, dict(), T=3)


def test_resident_engine_twice_on_the_prepared_day(oracle_lib):
    _exact_family(oracle_lib, "resident", 200, 1, dict(), run=_resident, align=True)
    _exact_family(oracle_lib, "resident", 1100, 3, dict(family="workgroup"), run=_resident)


def test_compat_sqrt_norm(oracle_lib, hip_opts):
    hip_opts("mf.compat_sqrt_norm", 1)
    for L, step in ((200, 1), (64, 3)):
        _exact_family(oracle_lib, "mf.compat_sqrt_norm", L, step, dict(), oracle_flags=oracle_lib.COMPAT_SQRT_NORM,
                      align=L == 200)


# ------------------------------------------------------------------------------------------ full mode ---
def _lags_of(case, n_random=400):
    """Lags to evaluate the float64 definition at: around every bad sample (windows that end up to 2 L + 150 samples in
    front of it to windows behind it), the ends of every template's range, the chunk and block seams, random ones."""
    near = []
    for s, c, i, _ in case.bad:
        for t in range(case.tp.shape[0]):
            lo = (i - 2 * case.L - 150 - int(case.mv[t, s, c])) // case.step
            near.append(np.arange(lo, lo + (3 * case.L + 300) // case.step + 2))
    return mfd.mf_full_lags(nc.cleaned(case).args, case.step, seed=case.L, n_random=n_random, extra=np.concatenate(near))


def _full_family(label, case, run, takes, flags=FULL):
    R = nc.reach("direct" if takes.get("family") == "direct" else "mfma", case.L)
    cls = case.classes(R)
    cl = nc.cleaned(case)
    lags = _lags_of(case)
    with np.errstate(invalid="ignore"):                 # (a template channel that holds NaN / Inf: the definition gives 0, B = 0)
        ref = mfd.mf_full_f64(*cl.args, step=case.step, lags=lags)
    k = cls[:, lags]
    by_form = {}
    for ns in (True, False):
        assert_takes(case.tp.shape, case.N, case.step, ns, flags=flags,
                     **{key: v(ns) if callable(v) else v for key, v in takes.items()})
        got_all = by_form[ns] = run(case, ns)
        got = got_all[:, lags]
        what = f"full mode {label}: {case.name} network_sum={ns}"
        want, B = (ref.net, ref.B_net) if ns else (ref.cc, ref.B)
        with np.errstate(invalid="ignore"):
            err = np.abs(got.astype(np.float64) - want)
        if ns:
            # (a lag with a channel of any other class is judged per channel only: the reference is the cleaned day's)
            near = (k == nc.NEAR).any(axis=(2, 3)) & np.isin(k, (nc.CLEAN, nc.NEAR, nc.OFF)).all(axis=(2, 3))
            clean = np.isin(k, (nc.CLEAN, nc.OFF)).all(axis=(2, 3))
            zero = np.isin(k, nc.ZERO_CLASSES_FULL).all(axis=(2, 3))
        else:
            near, clean, zero = k == nc.NEAR, np.isin(k, (nc.CLEAN, nc.OFF)), np.isin(k, nc.ZERO_CLASSES_FULL)
        bad = clean & ~(err <= B)
        assert not bad.any(), nc._first(bad, what, k, got, want, "outside the definition's bound")
        bad = near & ~np.isnan(got) & ~(err <= B)
        assert not bad.any(), nc._first(bad, what, k, got, want, "NEAR: neither NaN nor within the bound")
        bad = zero & (got.view(np.uint32) != 0)
        assert not bad.any(), nc._first(bad, what, k, got, want, "must be exactly +0")
        assert not np.isinf(got_all).any(), what
        if not ns:
            # nothing but NEAR may be NaN in full mode, and nothing that is CLEAN depends on the bad sample
            other = (cls != nc.NEAR) & (cls != nc.TOUCH_BIG) & np.isnan(got_all)
            assert not other.any(), nc._first(other, what, cls, got_all, got_all, "NaN outside NEAR")
            nc.check_invariance(got_all, run(cl, ns), cls, what)
    # the network sum IS the float32 chain over the per-channel values, at every lag (the mixed ones, unjudged above, too)
    assert np.array_equal(by_form[True], nc.network_sum32(by_form[False], case.w), equal_nan=True), label + ": " + case.name
    print(f"mf-nonfinite full mode {label}: {case.name}: {int(np.isin(k, (nc.CLEAN,)).sum())} CLEAN entries judged")


@pytest.mark.parametrize("ntile", [1, 2, 4])
def test_full_mode_wave_kernel(hip_opts, ntile):
    hip_opts("mf.tiles_per_wave", ntile)
    for case in nc.cases(100, 1, align=False, big=False):
        _full_family(f"wave ntile={ntile}", case, _host_full, dict(family="wave", ntile=ntile))


def test_full_mode_workgroup_and_generic_kernels(hip_opts):
    for case in nc.cases(300, 3, align=False, big=False):
        _full_family("workgroup", case, _host_full, dict(family="workgroup", maxr=20, maxt=5))
    hip_opts("mf.max_mfma_step", 0)
    for case in nc.cases(64, 3, align=False, big=False):
        _full_family("generic", case, _host_full, dict(family="direct"))


def test_full_mode_at_the_seam_of_the_partial_sums():
    """N = 70 000: two partial sums of 65 536 samples; bad samples on both sides of the seam.  A bad sample that
    reached the constant c would make the whole channel 0 -- 65 000 CLEAN lags in front of it included."""
    case = nc.full_seam_case()
    assert min(case.valid_lags()) >= nc.MIN_LAGS
    _full_family("SUM_PART seam", case, _host_full, dict())
    _full_family("SUM_PART seam, resident", case, lambda c, ns: _resident(c, ns, normalize="full"), dict())


# ------------------------------------------------------------------------------------------ mf.split16 ---
@functools.lru_cache(maxsize=None)
def _want_split(oracle_lib, L, align):
    return {case.name: tuple(oracle_lib.matched_filter(*case.args, 1, network_sum=ns) for ns in (True, False))
            for case in nc.cases(L, 1, align=align, big=False)}


@pytest.mark.parametrize("L", [200, 400, 800])
def test_split16_segments(oracle_lib, hip_opts, L):
    """One, two and three segments.  The scale exponent of a channel comes from its FINITE samples: a bad sample costs the
    lags of the rule and nothing else -- a day in counts keeps every CLEAN lag within the bar, with the cleaned day's bits."""
    hip_opts("mf.split16", 2)
    assert nc.split_geometry(L)[0] == {200: 1, 400: 2, 800: 3}[L]
    want = _want_split(oracle_lib, L, L == 200)
    worst = reach = n_nan = n_near = 0
    for n, case in enumerate(nc.cases(L, 1, align=L == 200, big=False)):
        R = nc.reach("split", L, case.mv)
        assert R[case.w != 0].max() < nc.R_LIMIT and min(case.valid_lags()) >= nc.MIN_LAGS, case.name
        cls = case.classes(R)
        cl = nc.cleaned(case)
        by_form = {}
        for ns in (True, False):
            got, got_cleaned = _host(case, ns), _host(cl, ns)
            by_form[ns] = got
            what = f"split16 L={L}: {case.name} network_sum={ns}"
            w_or = want[case.name][0 if ns else 1]
            if n == 0:      # (the split kernel ran: the exact kernel returns the oracle's bits)
                assert not np.array_equal(got_cleaned, oracle_lib.matched_filter(*cl.args, 1, network_sum=ns)), what
            worst = max(worst, nc.check_split(got, w_or, got_cleaned, cls, R, case.w if ns else 1.0, what))
            if not ns:
                nc.check_invariance(got, got_cleaned, cls, what)
                hit = (cls == nc.NEAR) & np.isnan(got)
                n_nan, n_near = n_nan + int(hit.sum()), n_near + int((cls == nc.NEAR).sum())
                reach = max(reach, nc.observed_reach(got, w_or, case, R))
        # the network sum is the float32 chain over the per-channel values at every lag
        assert np.array_equal(by_form[True], nc.network_sum32(by_form[False], case.w), equal_nan=True), case.name
    print(f"mf-nonfinite split16 L={L}: R = {nc.reach('split', L)} - (moveout mod 8), largest observed reach {reach}, "
          f"{n_nan} of {n_near} NEAR entries came back NaN, worst |d cc| / bar on finite entries {worst:.3e}")


def test_one_nan_in_a_day_of_counts_does_not_cost_the_detection(oracle_lib, hip_opts):
    """As a user meets it: nine channels in counts, a template cut from the day, one NaN in one channel far from the
    event.  Under mf.split16 the detection must stand where the oracle has it, at the oracle's value."""
    from seismic_bpmf_amd import matched_filter
    rng = np.random.default_rng(20)
    S, C, L, N, lag0 = 3, 3, 200, 20_000, 12_345
    d = (rng.standard_normal((S, C, N)) * 3.0e5).astype(np.float32)
    mv = rng.integers(-50, 300, (1, S, C)).astype(np.int32)
    tp = np.stack([np.stack([d[s, c, lag0 + mv[0, s, c]: lag0 + mv[0, s, c] + L] for c in range(C)]) for s in range(S)])[None]
    w = np.full((1, S, C), 1.0 / (S * C), np.float32)
    d[1, 2, 18_000] = np.nan            # BEHIND the event: in front of it the channel's norms are NaN and it counts 0 anyway
    want = oracle_lib.matched_filter(tp, mv, w, d, 1, True)
    assert int(np.nan_to_num(want)[0].argmax()) == lag0
    hip_opts("mf.split16", 2)
    got = matched_filter(tp, mv, w, d, 1, check_zeros=False, device=0)
    scrubbed = np.nan_to_num(got, nan=0.0)
    print(f"acceptance: arg-max {int(scrubbed[0].argmax())} (event at {lag0}), value {scrubbed[0, lag0]!r}, oracle {want[0, lag0]!r}, "
          f"{int(np.isnan(got).sum())} NaN lags of {got.size}")
    assert int(scrubbed[0].argmax()) == lag0
    assert abs(float(scrubbed[0, lag0]) - float(want[0, lag0])) <= nc.TOL_CC * float(np.abs(w).sum())
