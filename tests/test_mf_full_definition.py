"""CPU: the float64 definition of the matched filter's full normalisation (tests/mf_full_definition.py) judged on its own,
the SENSITIVITY of the GPU checks that rest on it (tests/test_gpu_mf_full.py), and the call surface of the feature that
needs no device.

  * the definition is np.corrcoef on random windows;
  * with N == L (one lag) the CPU oracle's short mode on the centred template and the centred window lies within B_full;
  * the float32 emulation of the prescribed computation passes the checker in every regime;
  * every planted defect FAILS the checker in the regimes listed in CATCHES -- which defect each regime catches:
        noise     data_mean template uncentred p_lo p_hi pp_div     (window sums of unit noise are ~ sqrt(L), far above B)
        offset    ... and c_neighbour   (the neighbour's offset is another one: d' keeps 2^12 .. 2^14, the float32 numerator
                                         chain loses 12 bits)
        drift     data_mean template uncentred p_lo p_hi pp_div     (large local means)
        step      data_mean template uncentred p_lo p_hi pp_div
        scaled    data_mean template uncentred p_lo p_hi pp_div
        gaps      flat_short   (the window whose last sample leaves the run), and what noise catches
        int0      data_mean uncentred p_lo p_hi pp_div   (template: zero-sum templates ARE centred -- nothing to catch)
        periodic  p_lo p_hi    (every other defect changes nothing where every window sum is 0: the regime is bit-equal
                                to short mode, data_mean included)
  * both input conditions fire on inputs built to violate them;
  * the new symbols, the flag and the launch information; the call surface.
"""
import functools

import numpy as np
import pytest

import f64_anchor as fa
import mf_full_definition as mfd

# (regime, L, N, step) of the checks here: the shapes of the GPU tests' regimes
CASES = {"noise": ("noise", 100, 3100, 1), "offset": ("offset", 100, 3100, 1), "drift": ("drift", 100, 3100, 1),
         "step": ("step", 100, 3100, 1), "scaled": ("scaled", 100, 3100, 1), "gaps": ("gaps", 100, 3100, 1),
         "gaps L=3": ("gaps", 3, 700, 1), "int0": ("int0", 100, 3100, 1), "periodic": ("periodic", 48, 3072, 1),
         "offset step 3": ("offset", 33, 1025, 3), "noise L=2": ("noise", 2, 700, 1), "noise L=1": ("noise", 1, 700, 1)}
_COMMON = ("data_mean", "template", "uncentred", "p_lo", "p_hi", "pp_div")
CATCHES = {"noise": _COMMON, "offset": _COMMON + ("c_neighbour",), "drift": _COMMON, "step": _COMMON, "scaled": _COMMON,
           "gaps": _COMMON + ("flat_short",), "gaps L=3": _COMMON + ("flat_short",),
           "int0": ("data_mean", "uncentred", "p_lo", "p_hi", "pp_div"), "periodic": ("p_lo", "p_hi"),
           "offset step 3": _COMMON + ("c_neighbour",), "noise L=2": _COMMON + ("flat_short",), "noise L=1": ("data_mean",)}
MIN_CAUGHT = 5


@functools.lru_cache(maxsize=None)
def _evaluated(name):
    regime, L, N, step = CASES[name]
    args = mfd.mf_full_case(regime, L, N, step, seed=L + 7)
    lags = mfd.mf_full_lags(args, step, seed=L, extra=mfd.gap_lags(args, step) if regime == "gaps" else ())
    ref = mfd.mf_full_f64(*args, step=step, lags=lags, exact=regime if regime in mfd.EXACT_REGIMES else False)
    return args, lags, ref


def test_definition_is_the_pearson_correlation():
    rng = np.random.default_rng(3)
    L, N = 37, 400
    tp = (rng.standard_normal((2, 1, 2, L)) + 3.0).astype(np.float32)
    d = (rng.standard_normal((1, 2, N)) * 2.0 - 11.0).astype(np.float32)
    mv = np.array([[[0, 5]], [[-3, 2]]], dtype=np.int32)
    w = np.ones((2, 1, 2), np.float32)
    ref = mfd.mf_full_f64(tp, mv, w, d)
    assert ref.valid.sum() > 600
    for t in range(2):
        for c in range(2):
            for i in np.flatnonzero(ref.valid[t])[::7]:
                x = d[0, c, i + mv[t, 0, c]: i + mv[t, 0, c] + L].astype(np.float64)
                want = np.corrcoef(tp[t, 0, c].astype(np.float64), x)[0, 1]
                assert abs(ref.cc[t, i, 0, c] - want) <= 1e-12


@pytest.mark.parametrize("offset", (0.0, 40.0))
def test_oracle_short_mode_on_centred_inputs_lies_within_the_bound(oracle_lib, offset):
    """One lag (N == L): c is the window's own mean, so short mode on (t', d') is the prescribed computation up to
    P^2 / L, P the rounding residue of the centring."""
    rng = np.random.default_rng(5)
    L = 200
    tp = (rng.standard_normal((3, 2, 3, L)) + 2.5).astype(np.float32)
    d = (rng.standard_normal((2, 3, L)) + offset).astype(np.float32)
    mv = np.zeros((3, 2, 3), np.int32)
    w = rng.uniform(0.2, 1.0, (3, 2, 3)).astype(np.float32)
    ref = mfd.mf_full_f64(tp, mv, w, d)
    t_k = (tp - tp.astype(np.float64).mean(axis=-1, keepdims=True).astype(np.float32)).astype(np.float32)
    d_k = (d - d.astype(np.float64).mean(axis=-1, keepdims=True).astype(np.float32)).astype(np.float32)
    got = oracle_lib.matched_filter(t_k, mv, w, d_k, 1, network_sum=False)
    assert fa.mf_compare(got, ref, False, "oracle short mode on centred inputs").require() > 0
    got = oracle_lib.matched_filter(t_k, mv, w, d_k, 1)
    fa.mf_compare(got, ref, True, "oracle short mode on centred inputs, network sum").require()
    # ... and short mode on the inputs as they are is NOT the correlation (the offsets of template and data)
    raw = oracle_lib.matched_filter(tp, mv, w, d, 1, network_sum=False)
    assert fa.mf_compare(raw, ref, False).n_bad > 0.9 * ref.B.size


@pytest.mark.parametrize("name", sorted(CASES))
def test_correct_emulation_passes(name):
    args, lags, ref = _evaluated(name)
    regime, L, N, step = CASES[name]
    assert ref.valid.any() and not ref.valid[1].any()              # (template 1 has no weight at all)
    got = mfd.mf_full_emulate(*args, step=step, lags=lags)
    fa.mf_compare(got, ref, False, f"emulation {name}").require()
    fa.mf_compare(mfd.network_sum32(got, args[2]), ref, True, f"emulation {name}, network sum").require()
    assert not got[ref.flat].any() and not np.signbit(got[ref.flat]).any()
    if regime == "gaps":
        assert ref.flat.sum() >= 20 and (ref.B > 0).sum() > ref.flat.sum()
    if L == 1:
        assert not ref.cc.any() and ref.flat.sum() == (ref.valid[:, :, None, None] & ref.active[:, None]).sum()
    if regime in mfd.EXACT_REGIMES:
        live = ref.B > 0
        assert (ref.B[live] <= 8 * fa.U * np.abs(ref.cc[live])).all()      # a few u |cc|: seven roundings and a double's worth


@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_defects_are_caught(name):
    args, lags, ref = _evaluated(name)
    step = CASES[name][3]
    for drop in CATCHES[name]:
        got = mfd.mf_full_emulate(*args, step=step, lags=lags, drop=drop)
        rep = fa.mf_compare(got, ref, False)
        assert rep.n_bad >= MIN_CAUGHT, (name, drop, rep.n_bad)
    assert set(d for v in CATCHES.values() for d in v) == set(mfd.DROPS)


def test_periodic_regime_is_short_mode(oracle_lib):
    """Every window sum is exactly 0: the emulation of full mode equals the oracle's short mode bit for bit."""
    args, lags, ref = _evaluated("periodic")
    assert not ref.P.any()
    got = mfd.mf_full_emulate(*args, lags=lags)
    want = oracle_lib.matched_filter(*args, 1, network_sum=False)[:, lags]
    assert np.array_equal(got, want) and np.abs(want).max() > 0.05
    for drop in ("p_lo", "p_hi"):
        assert not np.array_equal(mfd.mf_full_emulate(*args, lags=lags, drop=drop), want)


def test_input_conditions_fire():
    rng = np.random.default_rng(11)
    L, N = 16, 600
    tp = rng.standard_normal((1, 1, 1, L)).astype(np.float32)
    mv, w = np.zeros((1, 1, 1), np.int32), np.ones((1, 1, 1), np.float32)
    # E_t' E_c ~ 1e-6: inside the guard window
    t_c = tp[0, 0, 0].astype(np.float64) - tp[0, 0, 0].astype(np.float64).mean()
    d = rng.standard_normal((1, 1, N))
    d *= np.sqrt(1e-6 / (float(t_c @ t_c) * L))
    with pytest.raises(AssertionError, match="inside the guard window"):
        mfd.mf_full_f64(tp, mv, w, d.astype(np.float32))
    # a window that is not flat but whose centred energy drowns in the prefix sums' roundings: one sample of a
    # constant stretch off by one ulp, next to samples 1e8 times larger elsewhere in the channel
    d = rng.standard_normal((1, 1, N)) * 1e4
    d[0, 0, 200:260] = 1.0
    d[0, 0, 230] = np.nextafter(np.float32(1.0), np.float32(2.0))
    tp_big = (tp * 1e7).astype(np.float32)                            # (E_t' E_c above the guard)
    with pytest.raises(AssertionError, match="prefix-sum error bound"):
        mfd.mf_full_f64(tp_big, mv, w, d.astype(np.float32), lags=np.arange(205, 240))
    # ... while the FLAT windows of the same stretch are fine: exact zeros
    d[0, 0, 230] = 1.0
    ref = mfd.mf_full_f64(tp_big, mv, w, d.astype(np.float32), lags=np.arange(205, 240))
    assert ref.flat.all() and not ref.B.any()
    # the exact regimes refuse inputs that are not theirs
    args = mfd.mf_full_case("noise", 48, 3072, 1, seed=1)
    with pytest.raises(AssertionError):
        mfd.mf_full_f64(*args, exact="periodic")


# --------------------------------------------------------------------------- ABI, launch information ---
@pytest.fixture(scope="module")
def built():
    from seismic_bpmf_amd import build
    return build.build_lib()


def test_abi_has_the_new_symbols_and_the_flag(built):
    import ctypes
    import os
    import re
    import importlib
    from seismic_bpmf_amd import _lib
    mfmod = importlib.import_module("seismic_bpmf_amd.matched_filter")
    handle = ctypes.CDLL(built)
    for name in ("bpmf_mf_full_workspace_bytes", "bpmf_mf_prepare_data_full_dev"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bpmf_hip.h")).read()
    assert re.search(r"#define\s+BPMF_MF_NORMALIZE_FULL\s+4\b", header)
    assert re.search(r"#define\s+BPMF_MF_LAUNCH_INFO_FIELDS\s+13\b", header)
    assert mfmod.FLAG_NORMALIZE_FULL == 4
    lib = _lib.lib()
    # short mode keeps its size; full mode adds the per-day extras (d', a second prefix array, the count: 16 bytes a
    # sample) and t'
    L, N, T, S, C = 256, 100_000, 7, 4, 3
    short, full = lib.bpmf_mf_workspace_bytes(L, N, T, S, C), lib.bpmf_mf_full_workspace_bytes(L, N, T, S, C)
    extra = full - short
    assert 16 * S * C * N + 4 * T * S * C * L <= extra <= 16 * S * C * N + 4 * T * S * C * L + (1 << 16)
    # the per-day part precedes everything that depends on T
    grow = lib.bpmf_mf_full_workspace_bytes(L, N, T + 64, S, C) - full
    assert 0 < grow <= lib.bpmf_mf_workspace_bytes(L, N, T + 64, S, C) - short + 4 * 64 * S * C * L + 256
    with _lib.options(**{"mf.split16": 2}):
        assert lib.bpmf_mf_full_workspace_bytes(L, N, T, S, C) == full
        assert lib.bpmf_mf_workspace_bytes(L, N, T, S, C) > short


def test_launch_info_of_full_mode(built):
    from seismic_bpmf_amd import _lib
    shapes = ((1, 100, 20011), (1, 1040, 20011), (3, 33, 3100), (1, 257, 700))
    with _lib.options(**{"mf.split16": 2}):
        for step, L, N in shapes:
            assert _lib.mf_launch_info(step, L, N, 3, 2, 3)["family"] == "split16"
            info = _lib.mf_launch_info(step, L, N, 3, 2, 3, flags=4)
            assert info["family"] in ("direct", "workgroup", "wave") and info["refusal"] is None
        assert _lib.mf_launch_info(1, 100, 20011, 3, 2, 3, flags=4 | 2)["family"] == "direct"
    for step, L, N in shapes:                # the same kernel as short mode
        assert _lib.mf_launch_info(step, L, N, 3, 2, 3, flags=4) == _lib.mf_launch_info(step, L, N, 3, 2, 3)
    for opt in ("mf.compat_sqrt_norm", "mf.compat_sequential_csum"):
        with _lib.options(**{opt: 1}):
            _lib.mf_launch_info(1, 100, 20011, 3, 2, 3)
            with pytest.raises(_lib.BpmfHipError, match=f"status -1.*not defined under option {opt}"):
                _lib.mf_launch_info(1, 100, 20011, 3, 2, 3, flags=4)
    with _lib.options(**{"mf.compat_exclusive_last_lag": 1, "mf.compat_range_all_channels": 1}):
        assert _lib.mf_launch_info(1, 100, 20011, 3, 2, 3, flags=4)["family"] == "wave"


def test_call_surface():
    import seismic_bpmf_amd as sb
    tp = np.zeros((1, 1, 1, 8), np.float32)
    d = np.zeros((1, 1, 64), np.float32)
    mv, w = np.zeros((1, 1, 1), np.int32), np.ones((1, 1, 1), np.float32)
    with pytest.raises(NotImplementedError, match="matched_filter_full"):
        sb.matched_filter(tp, mv, w, d, 1, normalize="full")
    with pytest.raises(ValueError, match="no CPU implementation"):
        sb.matched_filter_full(tp, mv, w, d, 1, arch="cpu")
    with pytest.raises(ValueError):
        sb.matched_filter_full(tp, mv, w, np.zeros((2, 1, 64), np.float32), 1)       # station count mismatch
    import inspect
    assert inspect.signature(sb.MatchedFilterGPU.run).parameters["normalize"].default == "short"
    assert inspect.signature(sb.workflow.matched_filter_detections).parameters["normalize"].default == "short"
