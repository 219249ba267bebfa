"""CPU: the float64 definition of option mf.split16 (tests/f64_anchor.py: mf_split_f64, B_split, mf_split_exact_ok) judged on
its own, and the SENSITIVITY of the GPU checks that rest on it (tests/test_gpu_split16_anchor.py).

  * in the three exact regimes the predicate holds and the split numerators equal the plain ones, exactly;
  * in the general regimes the split form lies within B_split of the true correlation everywhere;
  * for every shape, step and regime the GPU tests run, the definition with a planted defect -- a product left out
    ("hi_lo", "lo_hi") or the data's lo halves scaled by 2^10 against the 2^-11 of their partner ("lo_scale") -- FAILS the
    check the GPU test applies to the kernel: in the exact regimes its numerators differ from the integer numerators
    (so its CC from the oracle's) on at least 90 % of the valid lags of every live channel the defect can reach; in the
    general regimes its rms error against the true correlation is at least 8 x the rms limit, K x the rms error of the
    exact float32 path (the oracle's) on the same lags, per channel and for the network sums.
"""
import functools

import numpy as np
import pytest

import f64_anchor as fa

N = fa.SPLIT_N
DEFINITION_LENGTHS = (8, 100, 378, 379, 753, 2040)
MIN_DIFFERING = 0.9
MIN_RMS_FACTOR = 8.0


def _live(args, ref):
    """(template, channel) pairs that are weighted and hold a template."""
    return ref.active & np.asarray(args[0]).any(axis=-1)


@functools.lru_cache(maxsize=None)
def _evaluated(regime, L, step, n_random=2400):
    """One case of the GPU tests, evaluated once for all the tests here: (args, the plain definition, its variants)."""
    exact = regime in fa.SPLIT_EXACT_REGIMES
    args = fa.mf_split_case(regime, L, N, step, seed=fa.split_exact_seed(L) if exact else fa.split_general_seed(L))
    lags = fa.mf_split_lags(args, step, seed=L, n_random=n_random, extra=() if exact else fa.split_glitch_lags(L, step))
    first = fa.mf_split_f64(*args, step=step, lags=lags, exact="split" if exact else False, drop="hi_lo")
    variants = {"hi_lo": first}
    variants.update({k: fa.mf_split_f64(*args, step=step, lags=lags, drop=k, _true=first.true) for k in ("lo_hi", "lo_scale")})
    sref = fa.mf_split_f64(*args, step=step, lags=lags, _true=first.true)
    for x in (first.true, sref, *variants.values()):                 # (what no test here reads)
        for name in ("split_terms", "split_den", "B_split"):
            x.__dict__.pop(name, None)
    return args, sref, variants


# ------------------------------------------------------------------------------ the pieces ---
def test_scale_exponents_and_planes():
    for x, s in ((3.0, 13), (2.0 ** 14, 0), (2.0 ** 15 - 1, 0), (2.0 ** 15, -1), (1e-30, 60), (0.0, 0)):
        assert fa.split_planes(np.array([x, -x / 2, 0.0]), 1.0).s == s, x
    with pytest.raises(AssertionError, match="beyond fp16"):          # (beyond the clamp: an input condition)
        fa.split_planes(np.array([1e30]), 1.0)
    p = fa.split_planes(np.array([8195.0, -4099.0, 3.0, 0.0]), fa.SPLIT_LO_SCALE)
    assert p.s == 1 and np.array_equal(p.hi, [16384.0, -8200.0, 6.0, 0.0]) and np.array_equal(p.rho, [6.0, 2.0, 0.0, 0.0])
    assert np.array_equal(p.lo, p.rho * 2048)
    assert fa._quantum([12.0, -0.75, 0.0]) == 0.25 and fa._quantum([0.0]) == 1.0 and fa._quantum([2.0 ** -30, 1.0]) == 2.0 ** -30
    assert fa.split_n_segments(376) == 1 and fa.split_n_segments(377) == 2 and fa.split_n_segments(2049) == 6
    assert fa.split_nks(376) == 26 and fa.split_nks(8) == 3 and fa.split_nks(377) == (192 + 53) // 16


def test_exact_predicate_refuses_what_is_not_exact():
    rng = np.random.default_rng(1)
    tp, mv, w, d = fa.mf_split_case("int_wide_data", 100, 5000, 1, seed=1)
    assert fa.mf_split_exact_ok(tp, d)
    assert not fa.mf_split_exact_ok(tp, rng.standard_normal(d.shape).astype(np.float32))        # lo halves that round
    assert not fa.mf_split_exact_ok(rng.standard_normal(tp.shape).astype(np.float32), d)
    # a window whose sum of |products| reaches 2^24 quanta: |t| = 3 against |d| = 2 * 4096 + 3 over 700 samples
    tp_big = np.full((1, 1, 1, 700), 3.0, np.float32)
    d_big = np.full((1, 1, 5000), 8195.0, np.float32)
    assert not fa.mf_split_exact_ok(tp_big, d_big) and fa.mf_split_exact_ok(tp_big[..., :600], d_big)


# ------------------------------------------------------------------------------ the definition ---
@pytest.mark.parametrize("L", DEFINITION_LENGTHS)
def test_exact_regimes_hold_the_predicate_and_give_the_integer_numerators(L):
    for regime in fa.SPLIT_EXACT_REGIMES:
        args, sref, _ = _evaluated(regime, L, 1)
        assert fa.mf_split_exact_ok(args[0], args[3]), (regime, L)
        live = _live(args, sref)
        assert sref.valid.any() and live.sum() == 16 and sref.zero_windows >= 1
        assert np.array_equal(sref.num, sref.true.num), (regime, L)
        assert np.array_equal(sref.cc, sref.true.cc) and np.array_equal(sref.net, sref.true.net)
        # ... and the regime reaches the plane it is named after: lo halves that are not zero
        n_lo_d = np.mean([(fa.split_planes(x, 1.0).rho != 0).mean() for x in args[3].reshape(-1, N)])
        n_lo_t = np.mean([(fa.split_planes(x, 1.0).rho != 0).mean() for x, l in zip(args[0].reshape(-1, L), live.ravel()) if l])
        print(f"{regime} L={L}: {n_lo_d:.0%} of the data samples and {n_lo_t:.0%} of the template samples have a lo half")
        assert (n_lo_d >= 0.4) == (regime == "int_wide_data") and (n_lo_d > 0) == (regime == "int_wide_data")
        assert (n_lo_t >= 0.25) == (regime == "int_wide_templates") and (n_lo_t > 0) == (regime == "int_wide_templates")


@pytest.mark.parametrize("L", DEFINITION_LENGTHS)
def test_general_regimes_lie_within_b_split_of_the_true_correlation(L):
    for regime in fa.SPLIT_GENERAL_REGIMES:
        args, sref, _ = _evaluated(regime, L, 1)
        assert not fa.mf_split_exact_ok(args[0][:1], args[3])
        for ns in (True, False):
            got, want, B = (sref.net, sref.true.net, sref.B_net) if ns else (sref.cc, sref.true.cc, sref.B)
            err = np.abs(got - want)
            assert (err <= B).all(), (regime, L, ns)
            assert not got[B == 0].any()
            print(f"definition {regime} L={L} network_sum={ns}: worst |split - f64| / B_split = {fa._worst(err, B):.4f}")
        # the bound is not vacuous: B_split is a small multiple of the float32 chain's own bound
        pos = sref.true.B > 0
        assert np.median(sref.B[pos] / sref.true.B[pos]) < 40


def test_b_split_holds_where_a_window_holds_the_unit_sample_of_a_quiet_channel():
    """The "glitch" regime keeps the sample that sets the quiet channel's scale at the end of the trace; here it lies
    inside the valid windows: quiet samples 2^-23 of the channel's maximum next to the maximum itself."""
    L = 100
    tp, mv, w, d = fa.mf_split_case("glitch", L, N, 1, seed=7)
    d[1, 1, N - 1], d[1, 1, N // 4] = d[1, 1, N - 2], 1.0
    lags = fa.mf_split_lags((tp, mv, w, d), 1, seed=L, extra=range(N // 4 - 2 * L, N // 4 + L, 7))
    sref = fa.mf_split_f64(tp, mv, w, d, lags=lags)
    err = np.abs(sref.cc - sref.true.cc)
    assert (err <= sref.B).all() and (np.abs(sref.net - sref.true.net) <= sref.B_net).all()
    # the data's lo halves stored plain would be fp16 subnormals here and lose their bits: the scaled ones do not
    quiet = fa.split_planes(d[1, 1], fa.SPLIT_LO_SCALE)
    plain = (quiet.rho).astype(np.float16).astype(np.float64)
    assert 10 * np.abs(quiet.lo / fa.SPLIT_LO_SCALE - quiet.rho).max() < np.abs(plain - quiet.rho).max() <= 2.0 ** -25


# ------------------------------------------------------------------------------ sensitivity ---
def _cases_of(L):
    return [c for c in fa.split_gpu_cases() if c[1] == L]


@pytest.mark.parametrize("L", fa.SPLIT_LENGTHS)
def test_a_planted_defect_fails_the_checks_of_the_gpu_tests(oracle_lib, L):
    assert _cases_of(L)
    for regime, _, step in _cases_of(L):
        exact = regime in fa.SPLIT_EXACT_REGIMES
        # (the GPU tests compare the exact regimes with the oracle at EVERY lag: a smaller sample estimates the fraction)
        args, sref, variants = _evaluated(regime, L, step) if not exact or (L in DEFINITION_LENGTHS and step == 1) else \
            _evaluated(regime, L, step, 500)
        live = _live(args, sref)
        where = sref.valid[:, :, None, None] & live[:, None]
        assert live.sum() == 16 and where.sum() >= 16 * 300
        if exact:
            assert np.array_equal(sref.num, sref.true.num)
            for drop in fa.SPLIT_DROPS:
                differs = variants[drop].num != sref.true.num
                worst = min(differs[t, sref.valid[t], s, c].mean() for t, s, c in np.argwhere(live))
                if drop in fa.SPLIT_EXACT_DROPS[regime]:
                    print(f"sensitivity {regime} L={L} step={step} drop={drop}: differs on {worst:.1%} of the valid lags (worst channel)")
                    assert worst >= MIN_DIFFERING, (regime, L, step, drop, worst)
                else:
                    assert not differs.any()           # (the regime does not reach that plane: nothing to lose)
            continue
        K = fa.SPLIT_RMS_K[L]
        for ns in (True, False):
            exact_path = fa.mf_full(oracle_lib.matched_filter(*args, step, ns), sref)
            own, rms_exact = fa.mf_rms_ratio(sref.net if ns else sref.cc, exact_path, sref, ns)
            judged = np.isfinite(own) & (live.any(axis=(1, 2)) if ns else live)
            assert judged.sum() >= (3 if ns else 12), (regime, L, ns, int(judged.sum()))
            assert np.nanmax(own[judged]) <= K                 # the definition itself, without accumulation error, passes
            for drop in fa.SPLIT_DROPS:
                ratio, _ = fa.mf_rms_ratio(variants[drop].net if ns else variants[drop].cc, exact_path, sref, ns)
                factor = float((ratio[judged] / K).min())
                print(f"sensitivity {regime} L={L} step={step} network_sum={ns} drop={drop}: rms error >= {factor:.1f} x the limit "
                      f"(K = {K}; the definition itself: {np.nanmax(own[judged]):.2f})")
                assert factor >= MIN_RMS_FACTOR, (regime, L, step, ns, drop, factor)
