"""CPU: the C oracle of the two hot paths against the float64 DEFINITION, within a derived bound.

The oracle is "parity unpinned" and the GPU suite proves the kernels equal to it bit for bit -- which says
nothing if oracle and kernels share a mistake (a lag-range rule, a moveout sign, a dropped station, a tie rule,
a normalisation guard).  Here the oracle is judged by tests/f64_anchor.py: float64 definitions written from the
documented conventions, an a priori forward-error bound computed from the same inputs (no tolerance is a
literal: each is that bound, 7u, or exact equality), exact zeros wherever the definition computes nothing, and
an arg-max rule that judges every sample.  Shapes cross what tests/test_oracle_hotpaths.py does not: several
1024-sample prefix-sum chunks, L in {1, 40, 256, 257, 1100, 2100}, steps {1, 3, 7}, moveouts of both signs with
first valid lags off the step grid, zero-weight channels / stations that carry the extreme moveouts; value
regimes: noise, per-channel scales with a glitch, DC offset, sinusoid, signed scaled features, exact integers.
Every compat switch alone and the two profiles.  The checker itself is tested on oracle results from mutated
inputs, which it must reject.  tests/test_gpu_f64_anchor.py holds the kernels to the same rules.
"""
import numpy as np
import pytest

import f64_anchor as fa

LENGTHS = [1, 40, 256, 257, 1100, 2100]
STEPS = [1, 3, 7]

MF_SWITCHES = {          # name -> (oracle flag name, definition parameters)
    "exclusive_last_lag": ("COMPAT_EXCLUSIVE_LAST_LAG", dict(exclusive_last_lag=True)),
    "sqrt_norm": ("COMPAT_SQRT_NORM", dict()),                      # rounding only: the same definition
    "range_all_channels": ("COMPAT_RANGE_ALL_CHANNELS", dict(range_all_channels=True)),
    "sequential_csum": ("COMPAT_SEQUENTIAL_CSUM", dict(sequential_csum=True)),
}
BP_SWITCHES = {
    "first_computed": ("COMPAT_FIRST_COMPUTED", dict(), True),
    "strict_upper_only": ("COMPAT_STRICT_UPPER_ONLY", dict(strict_upper_only=True), False),
    "range_all_stations": ("COMPAT_RANGE_ALL_STATIONS", dict(range_all_stations=True), False),
}


def _flags(oracle_lib, names, table):
    out = 0
    for n in names:
        out |= getattr(oracle_lib, table[n][0])
    return out


def _mf_kw(names):
    kw = {}
    for n in names:
        kw.update(MF_SWITCHES[n][1])
    return kw


def _mf_check(oracle_lib, args, step, kw, flags, what, exact=False):
    ref = fa.mf_f64(*args, step=step, exact=exact, **kw)
    worst = 0.0
    for ns in (True, False):
        with oracle_lib.compat(flags):
            got = oracle_lib.matched_filter(*args, step, ns)
        worst = max(worst, fa.mf_compare(got, ref, ns, f"oracle {what} network_sum={ns}").require())
    return ref, worst


@pytest.mark.parametrize("regime", fa.MF_REGIMES + ("int",))
@pytest.mark.parametrize("L", LENGTHS)
def test_mf_oracle_within_the_bound_of_the_definition(oracle_lib, L, regime):
    i = LENGTHS.index(L) + (fa.MF_REGIMES + ("int",)).index(regime)
    step = STEPS[i % 3]
    N = L + 2300 + 311 * (i % 4)                     # 2.3 to 5.2 chunks of the 1024-sample prefix sum
    args = fa.mf_case(regime, L, N, step, seed=100 * L + i)
    ref, _ = _mf_check(oracle_lib, args, step, {}, 0, f"MF L={L} {regime} step={step}", exact=regime == "int")
    # the case does hold what it is there for
    first = [fa.mf_lag_range(args[1][t], args[2][t], N, L, step) for t in range(2)]
    assert all(r is not None and r[0] > 0 and r[1] < ref.lags.size - 1 for r in first)
    assert step == 1 or any((-int(args[1][t][args[2][t] != 0].min())) % step for t in range(2))
    assert (ref.cc[ref.valid][:, ref.active[0]] != 0).any() and not ref.valid.all()
    # a dead (all-zero) template on a weighted channel inside the lag range, and the data gap: exact 0, B = 0
    assert fa.mf_dead_channels(args[0], ref) >= 1
    assert ref.zero_windows >= 1                                 # windows inside the data gap: exact 0, B = 0


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("switches", [(n,) for n in MF_SWITCHES] + [(), tuple(MF_SWITCHES)],
                         ids=list(MF_SWITCHES) + ["profile-build", "profile-upstream-recollected"])
def test_mf_oracle_switches_against_their_definitions(oracle_lib, switches, step):
    """Each mf.compat_* switch alone, then the two profiles of compat_profile(): "build" (none) and
    "upstream-recollected" (all four MF switches).  The range switches are judged by their own definition, which
    must differ from the default's on these inputs."""
    L, N = 40, 3500 + step
    for regime in ("noise", "scaled"):
        args = fa.mf_case(regime, L, N, step, seed=7 + step)
        ref, _ = _mf_check(oracle_lib, args, step, _mf_kw(switches), _flags(oracle_lib, switches, MF_SWITCHES),
                           f"MF {'+'.join(switches) or 'build'} {regime} step={step}")
        base = fa.mf_f64(*args, step=step)
        if "range_all_channels" in switches:
            assert (base.valid & ~ref.valid).sum() >= 2 * (300 // step)   # 333 samples per template
        elif "exclusive_last_lag" in switches and step == 1:
            assert (base.valid & ~ref.valid).sum(axis=1).tolist() == [1, 1]
        elif not switches:
            assert np.array_equal(base.valid, ref.valid)


BP_SHAPES = [(2, 1), (5, 2), (9, 3), (40, 2)]         # S * P = 2, 10, 27, 80
# the integer regime keeps its moveouts inside its stretches of negative and of zero features, so that whole
# samples sit on the (0, 0) floor; the general regime spreads them over [-700, 1200]
INT_TAU = dict(tau_lo=-70, tau_hi=120)


def _bp_check(oracle_lib, args, oob, kw, flags, first_computed, what, exact=False):
    ref = fa.bp_f64(*args, out_of_bounds=oob, exact=exact, **kw)
    with oracle_lib.compat(flags):
        beam = oracle_lib.beamform(*args, oob, "none")
        m, a = oracle_lib.beamform(*args, oob, "max")
    fa.bp_compare_beam(beam, ref, f"oracle {what} {oob} reduce=none").require()
    fa.bp_compare_max(m, a, ref, first_computed, f"oracle {what} {oob} reduce=max").require()
    if exact:
        wm, wa = fa.bp_max_f64(ref, first_computed)
        assert np.array_equal(beam, ref.beam) and np.array_equal(m, wm) and np.array_equal(a, wa), what
    return ref, (m, a)


@pytest.mark.parametrize("regime", ["signed", "int"])
@pytest.mark.parametrize("oob", ["strict", "flexible"])
@pytest.mark.parametrize("S,P", BP_SHAPES)
def test_bp_oracle_within_the_bound_of_the_definition(oracle_lib, S, P, oob, regime):
    K, N = 40, 4000
    args = fa.bp_case(regime, K, S, P, N, seed=10 * S + P, **(INT_TAU if regime == "int" else {}))
    ref, (m, a) = _bp_check(oracle_lib, args, oob, {}, 0, False, f"BP S={S} P={P} {regime}", exact=regime == "int")
    assert (args[1] < 0).any() and (args[1] > 0).any() and not args[3][3].any()
    assert not ref.computed[3].any() and ref.computed[0].any()
    if oob == "strict":
        assert (~ref.computed[ref.computed.any(axis=1)]).any(axis=1).all()     # every source has uncomputed samples
    if regime == "int":
        # hundreds of samples whose maximum several sources share (the lowest-index rule, pinned by the definition
        # alone), and samples on the (0, 0) floor although beams are computed there
        n_tied, n_floor = fa.bp_tie_and_floor_counts(ref)
        assert n_tied >= fa.MIN_TIED and n_floor >= fa.MIN_FLOOR, (n_tied, n_floor)
        assert ((m == 0) & (a == 0) & ref.computed.any(axis=0)).sum() == n_floor


@pytest.mark.parametrize("oob", ["strict", "flexible"])
@pytest.mark.parametrize("switches", [(n,) for n in BP_SWITCHES] + [(), ("first_computed",)],
                         ids=list(BP_SWITCHES) + ["profile-build", "profile-upstream-recollected"])
def test_bp_oracle_switches_against_their_definitions(oracle_lib, switches, oob):
    """Each bp.compat_* switch alone and the two profiles ("upstream-recollected" sets bp.compat_first_computed on
    this path).  A source without a weighted station computes nothing under every switch: the option texts speak
    of "its stations" for the range only, and a beam of no term is not a computed beam."""
    kw, fc = {}, False
    for n in switches:
        kw.update(BP_SWITCHES[n][1])
        fc = fc or BP_SWITCHES[n][2]
    for regime in ("signed", "int"):
        args = fa.bp_case(regime, 40, 6, 2, 4000, seed=3, **(INT_TAU if regime == "int" else {}))
        ref, (m, a) = _bp_check(oracle_lib, args, oob, kw, _flags(oracle_lib, switches, BP_SWITCHES), fc,
                                f"BP {'+'.join(switches) or 'build'} {regime}", exact=regime == "int")
        base = fa.bp_f64(*args, out_of_bounds=oob)
        if oob == "strict" and "range_all_stations" in switches:
            assert (base.computed & ~ref.computed).sum() > 1000
        if oob == "strict" and "strict_upper_only" in switches:
            assert (ref.computed & ~base.computed).sum() > 1000
        if fc and regime == "int":
            assert (m < 0).any() and ((m <= 0) & (a != 0)).any()      # where the default returns (0, 0)


# ------------------------------------------------------------------ the checker rejects what it must ---
def _mf_mutants(oracle_lib, args, step):
    tp, mv, w, d = args
    tp0 = tp.copy()
    tp0[..., -1] = 0.0
    yield "last template sample zeroed", lambda ns: oracle_lib.matched_filter(tp0, mv, w, d, step, ns)
    yield "every moveout + 1", lambda ns: oracle_lib.matched_filter(tp, mv + 1, w, d, step, ns)
    w0 = w.copy()
    w0[:, 1, 1] = 0.0
    yield "one weighted channel dropped", lambda ns: oracle_lib.matched_filter(tp, mv, w0, d, step, ns)


@pytest.mark.parametrize("L", [40, 2100])
def test_checker_rejects_mutated_matched_filters(oracle_lib, L):
    """Oracle results from mutated inputs, judged against the definition of the ORIGINAL inputs: outside the bound
    on most of the valid samples (per-channel layout: most samples of the channels the mutation touches)."""
    step, N = 1, L + 3000
    args = fa.mf_case("noise", L, N, step, seed=L)
    ref = fa.mf_f64(*args, step=step)
    assert fa.mf_compare(oracle_lib.matched_filter(*args, step, True), ref, True).n_bad == 0
    for name, run in _mf_mutants(oracle_lib, args, step):
        rep = fa.mf_compare(run(True), ref, True, name)
        frac = rep.bad[ref.valid].mean()
        print(f"mutation '{name}' L={L}: {frac:.3f} of the valid network sums rejected, worst err/B {rep.worst:.1f}")
        assert frac > 0.5, (name, frac)
        rep = fa.mf_compare(run(False), ref, False, name)
        frac = max(rep.bad[t, ref.valid[t]].mean(axis=0).max() for t in range(2))   # the channel it shows in most
        print(f"    per-channel layout: {frac:.3f} of the valid samples of that channel")
        assert frac > 0.5, (name, frac)


def test_checker_rejects_a_lag_range_off_by_one(oracle_lib):
    """The last valid lag removed (the oracle under mf.compat_exclusive_last_lag judged by the default definition)
    and added (the default oracle judged by the switch's definition): the one lag per template that differs is
    rejected -- a regular value against an exact zero."""
    args = fa.mf_case("noise", 40, 3300, 1, seed=12)
    for kw, flags, what in ((dict(), oracle_lib.COMPAT_EXCLUSIVE_LAST_LAG, "removed"),
                            (dict(exclusive_last_lag=True), 0, "added")):
        ref = fa.mf_f64(*args, step=1, **kw)
        for ns in (True, False):
            with oracle_lib.compat(flags):
                got = oracle_lib.matched_filter(*args, 1, ns)
            rep = fa.mf_compare(got, ref, ns, f"last lag {what}")
            assert rep.bad.reshape(2, ref.lags.size, -1).any(axis=2).sum(axis=1).tolist() == [1, 1], what


def test_checker_rejects_mutated_backprojections(oracle_lib):
    args = fa.bp_case("signed", 40, 6, 2, 4000, seed=5)
    f, tau, wp, ws = args
    ws0 = ws.copy()
    ws0[:, 0] = 0.0
    for oob in ("strict", "flexible"):
        ref = fa.bp_f64(*args, out_of_bounds=oob)
        anyc = ref.computed.any(axis=0)
        for name, mut in (("every moveout + 1", (f, tau + 1, wp, ws)), ("one weighted station dropped", (f, tau, wp, ws0))):
            rep = fa.bp_compare_beam(oracle_lib.beamform(*mut, oob, "none"), ref, name)
            frac = rep.bad[ref.computed & (ws[:, 0] != 0)[:, None]].mean()
            print(f"mutation '{name}' {oob}: {frac:.3f} of the computed beams rejected")
            assert frac > 0.9, (name, oob, frac)
            rep = fa.bp_compare_max(*oracle_lib.beamform(*mut, oob, "max"), ref, False, name)
            assert rep.bad[anyc].mean() > 0.5, (name, oob, rep.bad[anyc].mean())
    # strict evaluated as flexible: beams where the strict definition computes nothing
    ref = fa.bp_f64(*args, out_of_bounds="strict")
    rep = fa.bp_compare_beam(oracle_lib.beamform(*args, "flexible", "none"), ref, "strict as flexible")
    outside = ~ref.computed & (ws != 0).any(axis=1)[:, None]
    assert rep.bad[outside].mean() > 0.9 and not rep.bad[ref.computed].any()
    rep = fa.bp_compare_max(*oracle_lib.beamform(*args, "flexible", "max"), ref, False, "strict as flexible")
    assert rep.bad[~ref.computed.any(axis=0)].mean() > 0.5


def test_checker_rejects_ties_given_to_the_highest_index(oracle_lib):
    """Integer regime: the oracle run on the sources in REVERSED order gives every tie to the highest index of the
    original order; equal values, so only the exact arg-max comparison can reject it -- at every tied maximum."""
    f, tau, wp, ws = fa.bp_case("int", 40, 6, 2, 4000, seed=3, **INT_TAU)
    ref = fa.bp_f64(f, tau, wp, ws, out_of_bounds="flexible", exact=True)
    wm, wa = fa.bp_max_f64(ref)
    m, a = oracle_lib.beamform(f, tau[::-1], wp, ws[::-1], "flexible", "max")
    a = np.where(m > 0, 39 - a, 0).astype(np.int32)
    assert np.array_equal(m, wm)
    assert fa.bp_compare_max(m, a, ref).n_bad == 0          # values and maxima are right ...
    n_tied, _ = fa.bp_tie_and_floor_counts(ref)
    assert n_tied >= fa.MIN_TIED and (a != wa).sum() == n_tied      # ... the tie rule is not, at every tied sample
