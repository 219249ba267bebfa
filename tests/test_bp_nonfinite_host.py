"""CPU: the non-finite contract of the backprojection (tests/bp_nonfinite_cases.py) held against the oracle, and the
checkers of the GPU tests held against planted defects.

* bp_cpu against the written rule on every case: both value regimes, strict and flexible, reduce="none" and "max", the
  build's scan and oracle.compat(COMPAT_FIRST_COMPUTED) -- and the conditions every case must hold (the generator's
  floors on finite share, class counts, all-NaN samples and tied +Inf maxima).
* nine planted defects, each rejected by the checkers on a named case; the unplanted definition accepted.
* postprocess.focus_from_max and postprocess.likelihood on the relocation case (rule 4).
"""
import numpy as np
import pytest

import bp_nonfinite_cases as bn

OOBS = ("strict", "flexible")
DEFECT_CASES = (("default", "signed"), ("default", "int"))     # the named cases of the defect table


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("regime", bn.REGIMES)
@pytest.mark.parametrize("shape", list(bn.SHAPES))
def test_oracle_obeys_the_written_rule(oracle_lib, shape, regime):
    case = bn.case(shape, regime)
    for oob in OOBS:
        r = bn.refs(shape, regime, oob)
        counts = r.require()
        print(f"bp-nonfinite {r.name}: finite share {counts['finite_share']:.2f}, computed beams finite / NaN / +Inf / "
              f"-Inf {counts['per_class']}, all-NaN samples {counts['all_nan_samples']}, tied +Inf maxima "
              f"{counts['tied_inf_samples']}")
        vol = oracle_lib.beamform(*case.args, oob, "none")
        vol_clean = oracle_lib.beamform(*case.clean, oob, "none")
        bn.check_none(vol, r, oracle=vol, what=r.name + " oracle")
        # a finite beam has the bits of the same call on the cleaned features
        fin = r.ref.computed & (r.vol_class == bn.FINITE)
        assert np.array_equal(vol[fin].view(np.uint32), vol_clean[fin].view(np.uint32)), r.name
        for fc in (False, True):
            with oracle_lib.compat(oracle_lib.COMPAT_FIRST_COMPUTED if fc else 0):
                m, a = oracle_lib.beamform(*case.args, oob, "max")
            bn.check_max(m, a, r, fc, oracle=(m, a), what=f"{r.name} oracle first_computed={fc}")
            # the rule's scan over the oracle's own beams, in NumPy, gives the oracle's maximum bit for bit
            sm, sa = bn.scan_max(vol, r.ref.computed, fc)
            assert np.array_equal(m, sm) and np.array_equal(a, sa), r.name
            # ... and the source-id offset moves the floor with every other id
            bn.check_max(m, a + np.int32(1000), r, fc, oracle=(m, a), id_offset=1000, what=r.name + " id_offset")


@pytest.mark.parametrize("defect", bn.DEFECTS)
def test_planted_defects_are_rejected(oracle_lib, defect):
    """Each defect planted into the definition: the checkers refuse it on at least one named case, in every output form
    it changes, and accept the unplanted result of the same case."""
    named = []
    for shape, regime in DEFECT_CASES:
        case = bn.case(shape, regime)
        for oob in OOBS:
            r = bn.refs(shape, regime, oob)
            vol = oracle_lib.beamform(*case.args, oob, "none")
            comp = r.ref.computed
            for fc in (False, True):
                what = f"{defect} in {r.name} first_computed={fc}"
                if defect in bn.DEFECTS_MAX:
                    m, a, hit = bn.scan_max(vol, comp, fc, defect)
                    if not hit:
                        continue
                else:
                    bad_vol = bn.defective(defect, r, oracle_lib)
                    if bad_vol is None:
                        continue
                    if not fc:
                        assert _rejected(lambda: bn.check_none(bad_vol, r, what=what)), what + ": accepted as beams"
                    m, a = bn.scan_max(bad_vol, np.ones_like(comp) if defect == "strict_uncomputed_leaks" else comp, fc)
                    wm, wa = bn.scan_max(vol, comp, fc)
                    if np.array_equal(m, wm) and np.array_equal(a, wa):
                        continue                     # (the changed beams never reach the maximum here)
                bn.check_max(*bn.scan_max(vol, comp, fc), r, fc, what=what + " (unplanted)")
                assert _rejected(lambda: bn.check_max(m, a, r, fc, what=what)), what + ": accepted as a maximum"
                named.append(what)
    print(f"bp-nonfinite defect {defect}: rejected on {len(named)} (case, bounds, scan) combinations")
    assert named, f"{defect}: no named case holds it"


def test_strict_mask_of_the_cases_is_the_definitions():
    for shape in ("two stations", "default"):
        f, tau, wp, ws = bn.case(shape, "signed").clean
        want = bn.fa.bp_f64(f, tau, wp, ws, "strict").computed
        assert np.array_equal(bn.strict_computed(tau, ws, f.shape[-1]), want) and want.any() and not want.all()


def test_focus_and_likelihood_obey_rule_4(oracle_lib):
    from seismic_bpmf_amd import postprocess as pp
    for regime in bn.REGIMES:
        f, tau, wp, ws = bn.relocation_events(regime)
        for oob in OOBS:
            for e in range(f.shape[0]):
                what = (regime, oob, e)
                vol = oracle_lib.beamform(f[e], tau, wp, ws, oob, "none")
                m, a = oracle_lib.beamform(f[e], tau, wp, ws, oob, "max")
                assert not np.isnan(m).any()
                src, ti, M = pp.focus_from_max(m, a)
                assert M == m.max() and m[ti] == M and a[ti] == src, what
                if e in (0, 3):
                    assert M == np.inf, what                       # the planted +Inf is the maximum, no NaN is
                if e == 2:
                    # nothing but NaN beams (and +0 where strict computes none): an all-floor row, sample 0
                    assert (src, ti, M) == (0, 0, 0) and not m.any() and not a.any(), what
                if M > 0:
                    assert (src, ti) == bn.focus_of_volume(vol), what
                col = vol[:, ti]
                with np.errstate(invalid="ignore"):
                    like = pp.likelihood(col)
                assert like.dtype == np.float32
                if np.isnan(col).any():
                    assert np.isnan(like).all(), what
                elif col.max() == np.inf:
                    assert np.array_equal(np.isnan(like), np.isinf(col)) and not like[np.isfinite(col)].any(), what
                elif e == 1:
                    assert np.isfinite(like).all() and like.min() == 0 and like.max() == 1, what
            # event 0's column holds NaN beams (the dead station), event 3's is clean but for its +Inf
            vol0 = oracle_lib.beamform(f[0], tau, wp, ws, oob, "none")
            assert np.isnan(vol0[:, pp.focus_from_max(*oracle_lib.beamform(f[0], tau, wp, ws, oob, "max"))[1]]).any()


def test_first_maximum_of_a_volume_ignores_nan_in_every_block(monkeypatch):
    """workflow._first_maximum (the per-event focus) on host tensors: the first maximum in source-major order among the
    entries that are not NaN, whatever the block size; np.argmax's answer on a volume without NaN."""
    import torch
    from seismic_bpmf_amd import workflow
    rng = np.random.default_rng(3)
    base = np.round(rng.standard_normal((37, 101)) * 2).astype(np.float32)          # (many ties)
    vols = {"finite": base, "all NaN": np.full_like(base, np.nan)}
    v = base.copy()
    v[0, 0] = v[5, 7] = v[36, 100] = np.nan
    vols["NaN first, in the middle, last"] = v
    v = v.copy()
    v[20, 3] = v[20, 50] = v[30, 1] = np.inf
    vols["+Inf behind NaN"] = v
    v = np.full_like(base, np.nan)
    v[11, 13] = -np.inf
    vols["-Inf alone among NaN"] = v
    for block in (1, 101, 5 * 101, 1 << 22):
        monkeypatch.setattr(workflow, "_FOCUS_BLOCK", block)
        for name, vol in vols.items():
            got = workflow._first_maximum(torch.from_numpy(vol))
            assert tuple(int(x) for x in got) == bn.focus_of_volume(vol), (name, block)
    assert bn.focus_of_volume(base) == np.unravel_index(base.argmax(), base.shape)
    assert bn.focus_of_volume(vols["all NaN"]) == (0, 0) and bn.focus_of_volume(vols["+Inf behind NaN"]) == (20, 3)
