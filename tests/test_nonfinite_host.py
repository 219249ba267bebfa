"""CPU: the non-finite contract of the matched filter (tests/nonfinite_cases.py) held against the oracle, and the
checkers of the GPU tests held against planted defects.

* mf_cpu against the written rule on every case, under the default conventions and under mf.compat_sqrt_norm: AFTER,
  TOUCH_NAN and a NaN template channel are exactly 0, TOUCH_INF is NaN, CLEAN (and NEAR: the oracle has no reach) carries
  the cleaned day's bits.  The normative convention, in words, so that it no longer merely happens.
* premises: every class occurs somewhere; every family's R stays below 64 on every case and every template keeps 2000
  valid lags (the excepted lags stay under 4 % of a channel).
* eight planted defects, each rejected by the checkers on every case that names it.
* the full-mode definition under its new channel constant (the sum of the FINITE samples over N) equals its old self bit
  for bit on every finite case it has.
"""
import functools

import numpy as np
import pytest

import mf_full_definition as mfd
import nonfinite_cases as nc
import test_mf_full_definition as tmfd

SHAPES = ((200, 1), (64, 3))                     # (L, step) of the oracle checks; every case of nc.cases at each
SPLIT_LENGTHS = (200, 400, 800)
MFMA_LENGTHS = (40, 64, 100, 128, 200, 256, 257, 300, 800, 1100)


def _all_cases():
    return [c for L, step in SHAPES for c in nc.cases(L, step)]


@functools.lru_cache(maxsize=None)
def _oracle(oracle_lib, L, step, flags):
    out = []
    for case in nc.cases(L, step):
        with oracle_lib.compat(flags):
            want = oracle_lib.matched_filter(*case.args, step, network_sum=False)
            want_net = oracle_lib.matched_filter(*case.args, step, network_sum=True)
            cl = nc.cleaned(case)
            want_cleaned = oracle_lib.matched_filter(*cl.args, step, network_sum=False)
        out.append((case, want, want_net, want_cleaned))
    return out


@pytest.mark.parametrize("compat", ["default", "sqrt_norm"])
@pytest.mark.parametrize("L,step", SHAPES)
def test_oracle_obeys_the_written_rule(oracle_lib, L, step, compat):
    flags = oracle_lib.COMPAT_SQRT_NORM if compat == "sqrt_norm" else 0
    for case, want, want_net, want_cleaned in _oracle(oracle_lib, L, step, flags):
        cls = case.classes(0)
        what = f"{case.name} [{compat}]"
        assert not np.isinf(want).any(), what
        zero = np.isin(cls, nc.ZERO_CLASSES)
        assert not want[zero].any(), nc._first(zero & (want != 0), what, cls, want, want, "the oracle is not 0")
        plus = np.isin(cls, (nc.OFF, nc.TOUCH_NAN, nc.AFTER, nc.DEAD_T_NAN))
        assert not want[plus].view(np.uint32).any(), what + ": a -0 where the guard writes +0"
        ti = cls == nc.TOUCH_INF
        assert np.isnan(want[ti]).all(), nc._first(ti & ~np.isnan(want), what, cls, want, want, "the oracle is not NaN")
        tb = cls == nc.TOUCH_BIG
        assert (np.isnan(want[tb]) | (want[tb] == 0)).all(), what
        keep = np.isin(cls, (nc.CLEAN, nc.NEAR))
        same = want.view(np.uint32) == want_cleaned.view(np.uint32)
        assert same[keep].all(), nc._first(keep & ~same, what, cls, want, want_cleaned, "differs from the cleaned day")
        assert np.isfinite(want[keep]).all(), what
        dt = cls == nc.DEAD_T_INF
        assert np.array_equal(np.isnan(want[dt]), np.isnan(want_cleaned[dt])), what
        # the network sum is the float32 chain over the weighted channels of those values
        assert np.array_equal(want_net, nc.network_sum32(want, case.w), equal_nan=True), what
        # and the checkers accept the oracle itself
        nc.check_exact(want, want, cls, 0, what)
        nc.check_invariance(want, want_cleaned, cls, what, near_too=True)


def test_premises_every_class_occurs_and_the_excepted_lags_stay_few():
    seen = set()
    for case in _all_cases() + [nc.full_seam_case()]:
        assert min(case.valid_lags()) >= nc.MIN_LAGS, (case.name, case.valid_lags())
        cls = case.classes(nc.reach("mfma", case.L))
        seen |= {int(k) for k in np.unique(cls)}
        live = cls != nc.OFF
        near = (cls == nc.NEAR).sum(axis=1) / np.maximum(live.sum(axis=1), 1)
        assert near.max() < 0.04, case.name
    assert seen == set(range(len(nc.CLASS_NAMES))), [nc.CLASS_NAMES[k] for k in set(range(10)) - seen]
    for L in MFMA_LENGTHS:
        assert 15 <= nc.reach("mfma", L) <= 30 < nc.R_LIMIT and nc.reach("mfma", L) == -(-(L + 15) // 16) * 16 - L
    assert nc.reach("direct", 2100) == 0
    assert [nc.reach("split", L) for L in SPLIT_LENGTHS] == [40, 40, 64]
    assert [nc.split_geometry(L)[0] for L in SPLIT_LENGTHS] == [1, 2, 3]
    for L in SPLIT_LENGTHS:
        for case in nc.cases(L, 1, align=False, big=False):
            R = nc.reach("split", L, case.mv)
            assert R[case.w != 0].max() < nc.R_LIMIT and R.min() >= 0, (case.name, int(R.max()))
            assert min(case.valid_lags()) >= nc.MIN_LAGS, case.name
    # every remainder of a moveout mod 8 (the split kernel's r) occurs among the weighted channels at L = 200
    rem = {int(m) % 8 for case in nc.cases(200, 1) for m in case.mv[case.w != 0]}
    assert rem == set(range(8))


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("family", ["direct", "mfma", "split"])
@pytest.mark.parametrize("defect", nc.DEFECTS)
def test_planted_defects_are_rejected(oracle_lib, defect, family):
    """Each defect planted into the oracle's per-channel result (and its network sum): the family's checkers must
    refuse it on every case that names it, in both output forms, and must accept the unplanted result."""
    named = 0
    L, step = SHAPES[0]
    for case, want, want_net, want_cleaned in _oracle(oracle_lib, L, step, 0):
        if family == "split" and case.exact_only:
            continue
        R = nc.reach(family, L, case.mv)
        cls = case.classes(R)
        planted = nc.plant(defect, case, want, want_cleaned, R)
        if planted is None:
            continue
        named += 1
        planted_net = nc.network_sum32(planted, case.w)
        cleaned_net = nc.network_sum32(want_cleaned, case.w)
        what = f"{defect} in {case.name} [{family}]"
        if family == "split":
            nc.check_split(want, want, want_cleaned, cls, R, 1.0, what)
            nc.check_split(want_net, want_net, cleaned_net, cls, R, case.w, what)
            per_channel = _rejected(lambda: nc.check_split(planted, want, want_cleaned, cls, R, 1.0, what))
            net = _rejected(lambda: nc.check_split(planted_net, want_net, cleaned_net, cls, R, case.w, what))
        else:
            per_channel = _rejected(lambda: nc.check_exact(planted, want, cls, R, what))
            net = _rejected(lambda: nc.check_exact(planted_net, want_net, cls, R, what))
        assert per_channel, what + ": accepted per channel"
        if defect != "neighbour":
            # (a NaN moved into a neighbouring channel of the same lag leaves the network sum NaN as before)
            assert net, what + ": accepted as a network sum"
        if defect in ("channel_poisoned", "channel_silenced", "neighbour", "reach_plus_one"):
            assert _rejected(lambda: nc.check_invariance(planted, want_cleaned, cls, what)), what + ": invariance accepted it"
    assert named >= 2, (defect, family, named)


def test_full_mode_constant_is_the_mean_on_finite_channels():
    """c = float32((sum of the finite samples) / N) is float32(float64 mean) bit for bit on every finite case the
    definition's own tests use -- so the definition, its emulation and its bounds are what they were -- and ignores a
    bad sample exactly as if it were +0."""
    for name, (regime, L, N, step) in tmfd.CASES.items():
        tp, mv, w, d = mfd.mf_full_case(regime, L, N, step, seed=L + 7)
        for row in d.reshape(-1, N):
            old = np.float32(row.astype(np.float64).mean())
            assert mfd.channel_constant(row).view(np.uint32) == old.view(np.uint32), name
    case = nc.full_seam_case()
    cl = nc.cleaned(case)
    for s, c, _, _ in case.bad:
        got = mfd.channel_constant(case.data[s, c])
        assert np.isfinite(got) and got.view(np.uint32) == mfd.channel_constant(cl.data[s, c]).view(np.uint32)
    assert mfd.channel_constant(np.full(10, np.nan, np.float32)) == 0


def test_full_mode_emulation_obeys_the_rule():
    """The float32 emulation of full mode's prescribed computation on a poisoned day: every class but CLEAN / NEAR is
    exactly 0 (a window that holds +-Inf too: E_c = Inf - Inf), CLEAN carries the cleaned day's bits."""
    for case in nc.cases(64, 3, align=False, big=False):
        cls = case.classes(0)
        lags = np.unique(np.concatenate([np.arange(0, case.n_corr, 37)] +
                                        [np.clip(np.arange((i - 500) // 3, (i + 200) // 3), 0, case.n_corr - 1)
                                         for _, _, i, _ in case.bad]))
        got = mfd.mf_full_emulate(*case.args, step=case.step, lags=lags)
        ref = mfd.mf_full_emulate(*nc.cleaned(case).args, step=case.step, lags=lags)
        k = cls[:, lags]
        zero = np.isin(k, nc.ZERO_CLASSES_FULL)
        assert not got[zero].view(np.uint32).any(), nc._first(zero & (got != 0), case.name, k, got, ref, "full mode: not +0")
        keep = np.isin(k, (nc.CLEAN, nc.NEAR))
        assert (got.view(np.uint32) == ref.view(np.uint32))[keep].all(), case.name
