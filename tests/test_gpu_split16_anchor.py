"""GPU: option mf.split16 against its float64 definition (tests/f64_anchor.py: mf_split_f64, B_split, mf_split_exact_ok).

tests/test_gpu_split16.py holds the path to the north star's bar, 2e-5 -- a hundred times what it delivers, so a lost lo
plane in one segment, one alignment remainder or one band copy passes there.  Here:
  exact regimes    on inputs where every fp16 operand is exact and every partial sum stays below 2^24 quanta the split
                   numerator IS the integer numerator: the output equals the oracle's bit for bit at every lag, and lies
                   within the exact-regime bound of the float64 definition.  "int" reaches hi * hi only, "int_wide_data"
                   hi_t * lo_d, "int_wide_templates" lo_t * hi_d.  A canary -- one more template, weighted only on one
                   more channel of Gaussian data -- rides in the same launch and must NOT equal the oracle: the split
                   kernel ran.
  general regimes  |kernel - cc| <= B_split per channel (B_net for the sums) with cc the TRUE correlation, exact zeros
                   where the definition computes nothing, and the sharp one: per channel, the rms of kernel - cc over the
                   sampled lags at most K times the rms of the exact float32 path's error (the oracle's, on the same
                   lags); K per template length in f64_anchor.SPLIT_RMS_K (3 x the ratio measured on an MI355X).
tests/test_split16_definition.py shows on the CPU that the definition with a planted defect fails these very checks on
these very inputs.  Shapes: 3 templates x 2 x 3 channels, N = 20 011 (three lag blocks of 8192, a partial last q-chunk),
moveouts of every remainder mod 8 with both signs, one to six segments.  Every check prints its figures (pytest -rP).
"""
import numpy as np
import pytest

import f64_anchor as fa

pytestmark = pytest.mark.gpu

N = fa.SPLIT_N
LENGTHS = fa.SPLIT_LENGTHS


@pytest.fixture
def split16(hip_opts):
    hip_opts("mf.split16", 2)              # the split kernel for every launch, however small
    return hip_opts


def _host(args, step, ns):
    from seismic_bpmf_amd import matched_filter
    return matched_filter(*args, step, arch="gpu", check_zeros=False, network_sum=ns)


def _resident(args, step, ns):
    from seismic_bpmf_amd import MatchedFilterGPU
    eng = MatchedFilterGPU(device=0)
    eng.set_data(args[3])
    first = eng.run(args[0], args[1], args[2], step, network_sum=ns).cpu().numpy()
    again = eng.run(args[0], args[1], args[2], step, network_sum=ns).cpu().numpy()    # on the prepared day
    assert np.array_equal(first, again)
    return again


def _with_canary(args, seed):
    """One more station whose first component is Gaussian, and one more template weighted on that channel alone."""
    tp, mv, w, d = args
    T, S, C, L = tp.shape
    rng = np.random.default_rng(seed)
    tp2, mv2, w2 = np.zeros((T + 1, S + 1, C, L), np.float32), np.zeros((T + 1, S + 1, C), np.int32), np.zeros((T + 1, S + 1, C), np.float32)
    d2 = np.zeros((S + 1, C, d.shape[-1]), np.float32)
    tp2[:T, :S], mv2[:T, :S], w2[:T, :S], d2[:S] = tp, mv, w, d
    tp2[T, S, 0] = rng.standard_normal(L)
    d2[S, 0] = rng.standard_normal(d.shape[-1])
    mv2[T, S, 0], w2[T, S, 0] = 5, 1.0
    return tp2, mv2, w2, d2


def _exact_case(oracle_lib, label, regime, L, step, run=_host):
    """One exact-regime case with its canary: bit-equality with the oracle at every lag, the canary apart; the exact
    templates within the exact-regime bound of the definition at the sampled lags."""
    args = fa.mf_split_case(regime, L, N, step, seed=fa.split_exact_seed(L))
    T, S = args[0].shape[:2]
    lags = fa.mf_split_lags(args, step, seed=L)
    ref = fa.mf_f64(*args, step=step, lags=lags, exact="split")           # (asserts mf_split_exact_ok)
    assert ref.valid.any() and not ref.valid.all() and ref.zero_windows >= 1 and fa.mf_dead_channels(args[0], ref) == 1
    full = _with_canary(args, seed=L)
    for ns in (True, False):
        what = f"kernel MF split16 {label} L={L} step={step} {regime} network_sum={ns}"
        got = run(full, step, ns)
        want = oracle_lib.matched_filter(*full, step, ns)
        canary_got, canary_want = (got[T], want[T]) if ns else (got[T, :, S, 0], want[T, :, S, 0])
        n_diff = int((canary_got != canary_want).sum())
        print(f"f64-anchor {what}: canary differs from the oracle at {n_diff} of {canary_got.size} lags")
        assert n_diff > 0, what + ": the canary equals the oracle -- the split kernel did not run"
        exact_got, exact_want = (got[:T], want[:T]) if ns else (got[:T, :, :S], want[:T, :, :S])
        differ = exact_got != exact_want
        if differ.any():
            i = tuple(int(x) for x in np.argwhere(differ)[0])
            where = f"first at template {i[0]}, index {i[1]} (data offset {i[1] * step}, offset mod 8192 = {i[1] * step % 8192})"
            if not ns:
                where += f", channel {i[2:]}, moveout {int(args[1][i[0], i[2], i[3]])} (remainder {int(args[1][i[0], i[2], i[3]]) % 8})"
            raise AssertionError(f"{what}: {int(differ.sum())} of {differ.size} values differ from the oracle; {where}: "
                                 f"got {exact_got[i]!r}, oracle {exact_want[i]!r}")
        if not ns:      # the canary's template writes nothing but its own channel
            assert np.array_equal(got[T, :, :S], want[T, :, :S]) and np.array_equal(got[T, :, S, 1:], want[T, :, S, 1:])
        fa.mf_compare(fa.mf_full(exact_got, ref), ref, ns, what).require()


def _general_case(oracle_lib, label, regime, L, step, run=_host, kw=None, flags=0):
    """One general-regime case: B_split and B_net, exact zeros, and the rms ratio against the exact path's error."""
    args = fa.mf_split_case(regime, L, N, step, seed=fa.split_general_seed(L))
    range_kw = {k: v for k, v in (kw or {}).items() if k != "sequential_csum"}
    lags = fa.mf_split_lags(args, step, seed=L, extra=fa.split_glitch_lags(L, step), **range_kw)
    sref = fa.mf_split_f64(*args, step=step, lags=lags, **(kw or {}))
    anchor = fa.mf_split_anchor(sref)
    assert sref.valid.any() and not sref.valid.all() and sref.zero_windows >= 1
    worst = 0.0
    for ns in (True, False):
        what = f"kernel MF split16 {label} L={L} step={step} {regime} network_sum={ns}"
        got = fa.mf_full(run(args, step, ns), sref)
        with oracle_lib.compat(flags):
            exact_path = fa.mf_full(oracle_lib.matched_filter(*args, step, ns), sref)
        fa.mf_compare(got, anchor, ns, what).require()
        worst = max(worst, fa.mf_rms_require(got, exact_path, sref, ns, fa.SPLIT_RMS_K[L], what))
    return worst


_step_of = fa.split_step_of


@pytest.mark.parametrize("L", LENGTHS)
def test_split16_exact_regimes_equal_the_oracle_bit_for_bit(oracle_lib, split16, L):
    for regime in fa.SPLIT_EXACT_REGIMES:
        _exact_case(oracle_lib, "host call", regime, L, _step_of(L))


@pytest.mark.parametrize("L", LENGTHS)
def test_split16_general_regimes_within_b_split_and_the_rms_ratio(oracle_lib, split16, L):
    worst = max(_general_case(oracle_lib, "host call", regime, L, _step_of(L)) for regime in fa.SPLIT_GENERAL_REGIMES)
    print(f"split16 anchor summary: L = {L}, step {_step_of(L)}: worst rms ratio {worst:.3f}, K = {fa.SPLIT_RMS_K[L]}")


@pytest.mark.parametrize("L", fa.SPLIT_RESIDENT_LENGTHS)
def test_split16_resident_engine_on_a_prepared_day(oracle_lib, split16, L):
    step = 4 - _step_of(L)                  # (the other step than the host call's at this length)
    _exact_case(oracle_lib, "resident", "int_wide_data", L, step, run=_resident)
    _exact_case(oracle_lib, "resident", "int_wide_templates", L, step, run=_resident)
    _general_case(oracle_lib, "resident", "glitch", L, step, run=_resident)


MF_SWITCHES = {"mf.compat_exclusive_last_lag": (dict(exclusive_last_lag=True), "COMPAT_EXCLUSIVE_LAST_LAG"),
               "mf.compat_sqrt_norm": (dict(), "COMPAT_SQRT_NORM"),
               "mf.compat_range_all_channels": (dict(range_all_channels=True), "COMPAT_RANGE_ALL_CHANNELS"),
               "mf.compat_sequential_csum": (dict(sequential_csum=True), "COMPAT_SEQUENTIAL_CSUM")}


@pytest.mark.parametrize("switch", list(MF_SWITCHES))
def test_split16_under_each_compat_switch(oracle_lib, split16, switch):
    """Each mf.compat_* switch with mf.split16 on: the definition under the same switch, B_split and the rms ratio (the
    exact path: the oracle under the same switch).  No bit-equality here: mf.compat_sqrt_norm changes the epilogue."""
    split16(switch, 1)
    kw, flag = MF_SWITCHES[switch]
    for L, step in fa.SPLIT_SWITCH_SHAPES:
        for regime in ("noise", "scaled"):
            _general_case(oracle_lib, switch, regime, L, step, kw=kw, flags=getattr(oracle_lib, flag))


def test_split16_template_length_limit(oracle_lib, split16):
    """The limit stated in include/bpmf_hip.h: the longest template the MFMA kernels take is the longest one mf.split16
    takes (the canary differs from the oracle); one sample more and the exact generic kernel answers, canary included."""
    from seismic_bpmf_amd import matched_filter
    L = fa.SPLIT_MAX_L
    assert LENGTHS[-1] == L                  # (the exact and general tests above run at the limit itself, canary and all)
    args = _with_canary(fa.mf_split_case("int_wide_data", L + 1, N, 1, seed=1), seed=2)
    for ns in (True, False):
        got = matched_filter(*args, 1, arch="gpu", check_zeros=False, network_sum=ns)
        assert np.array_equal(got, oracle_lib.matched_filter(*args, 1, ns)), f"L = {L + 1}, network_sum={ns}"
