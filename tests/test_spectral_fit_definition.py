"""CPU: the definition of the Brune / Boatwright fit (postprocess.fit_source_spectra_host), the gates and the P-S average
(moment_magnitudes_host) and the resampling of multi-band spectra (resample_spectra_host).

Against the reference (tests/golden/spectral_fit.npz: Spectrum.fit_average_spectrum under SciPy's curve_fit on the
groups of spectral_fit_cases.RECORDED) the definition is held to what a minimiser can be held to:
 1. its cost is never above the reference's (a theorem, with 1e-12 for the rounding of two evaluations);
 2. where the reference reached the minimum (its cost within 1 + 1e-12 of the definition's: 88 of the 139 recorded
    fits, so 0.37 is left out and the cap is one half) the parameters lie in the sublevel set of that excess under a
    quadratic model of P, times MARGIN;
 3. there the errors agree with SciPy's pcov, which comes from a 2-point Jacobian at popt.
The worst ratios of 2 and 3 on the fixture are recorded in profiles/spectral_fit.txt; -rP prints them.
Then the cases with known answers, the defects that the comparison with the device must reject, and the two small
definitions.  No GPU."""
import os
import re

import numpy as np
import pytest

import spectral_fit_cases as sfc
from seismic_bpmf_amd import postprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = 1.0e-12                  # the reference "converged": cost_reference <= cost_definition (1 + CUT)
MARGIN = 4.0                   # on the quadratic model's width: it is loose on flat minima (worst measured: 0.88)
PCOV_TOLERANCE = 4.0 * 4.76e-7  # relative, on M0_err and fc_err: 4 x the worst measured on the fixture


@pytest.fixture(scope="module")
def recorded():
    g = sfc.golden()
    rows = []
    for group, (model, weighted, F, E, _) in sfc.RECORDED.items():
        x = {"average": g[f"average_{group}"], "mask": g[f"mask_{group}"], "num_valid": g[f"numvalid_{group}"],
             "frequencies": g[f"freq_{group}"]}
        fresh = sfc.recorded_inputs(group)
        assert all(np.array_equal(x[k], fresh[k]) for k in x), group       # the fixture holds what the cases make
        fit = pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], "p", model=model,
                                         weighted=weighted)
        for e in range(E):
            rows.append({"group": group, "e": e, "x": x, "model": model, "weighted": weighted, "F": F,
                         "fit": {k: v[e] for k, v in fit.items()}, "called": bool(g[f"called_{group}"][e]),
                         "ref_success": bool(g[f"success_{group}"][e]), "popt": g[f"popt_{group}"][e],
                         "pcov": g[f"pcov_{group}"][e], "ref_cost": float(g[f"cost_{group}"][e])})
    return rows


def converged(rows):
    return [r for r in rows if np.isfinite(r["ref_cost"]) and not r["fit"]["at_bound"] and r["fit"]["reason"] in (0, 3)
            and r["ref_cost"] <= r["fit"]["cost"] * (1.0 + CUT)]


def test_constants_are_the_header_s():
    header = open(os.path.join(ROOT, "include", "bpmf_hip.h")).read()
    for name, value in (("SCAN_POINTS", pp.FIT_SCAN_POINTS), ("ZOOM_ROUNDS", pp.FIT_ZOOM_ROUNDS),
                        ("ZOOM_POINTS", pp.FIT_ZOOM_POINTS), ("NEWTON_STEPS", pp.FIT_NEWTON_STEPS),
                        ("BOUND_FACTOR", pp.FIT_BOUND_FACTOR)):
        found = re.search(rf"#define BPMF_FIT_{name} (\S+)", header)
        assert found and float(found.group(1)) == float(value), name
    assert pp.FIT_SCAN_POINTS >= 1024


def test_the_reference_is_fitted_where_the_definition_is(recorded):
    """curve_fit is reached exactly where the definition passes the first two gates, and it never raised."""
    for r in recorded:
        assert r["called"] == (r["fit"]["reason"] not in (1, 2)), (r["group"], r["e"])
        assert not r["called"] or np.isfinite(r["popt"]).all(), (r["group"], r["e"])
    assert sum(r["called"] for r in recorded) >= 130


def test_cost_is_never_above_the_reference_s(recorded):
    worst = -np.inf
    for r in recorded:
        if r["called"]:
            assert r["fit"]["reason"] != 5
            worst = max(worst, r["fit"]["cost"] / r["ref_cost"] - 1.0)
            assert r["fit"]["cost"] <= r["ref_cost"] * (1.0 + 1.0e-12), (r["group"], r["e"], r["fit"]["cost"], r["ref_cost"])
    print(f"cost_definition / cost_reference - 1, worst: {worst:.3g}")


def test_parameters_where_the_reference_converged(recorded):
    rows, fitted = converged(recorded), [r for r in recorded if r["called"]]
    share = len(rows) / len(fitted)
    print(f"reference within 1 + {CUT:g} of the minimum and not at a bound: {len(rows)} of {len(fitted)} ({share:.2f})")
    assert 1.0 - share <= 0.5
    worst_u = worst_a = 0.0
    for r in rows:
        ln_x, y, w2, n = sfc.event_terms(r["x"], r["e"], r["model"], r["weighted"])
        u = np.log(r["fit"]["fc"])
        _, p2, _, _ = pp.fit_profile_derivatives(u, ln_x, y, w2, n)
        a1 = abs((w2 * (-(2.0 / sfc.LN10) / (1.0 + np.exp(-n * (ln_x - u))))).sum() / w2.sum())
        excess = CUT * r["fit"]["cost"]
        assert p2 > 0.0
        width_u = np.sqrt(2.0 * excess / p2)
        width_a = np.sqrt(2.0 * excess / w2.sum()) + a1 * width_u
        # (what two roundings of a parameter leave when the cost, and with it the width, is all but 0)
        ratio_u = abs(np.log(r["popt"][1]) - u) / (width_u + 8 * sfc.EPS * max(1.0, abs(u)))
        ratio_a = abs(np.log10(r["popt"][0]) - np.log10(r["fit"]["M0"])) / (width_a + 8 * sfc.EPS * 16.0)
        worst_u, worst_a = max(worst_u, ratio_u), max(worst_a, ratio_a)
        assert ratio_u <= MARGIN and ratio_a <= MARGIN, (r["group"], r["e"], ratio_u, ratio_a)
    print(f"worst |d ln fc| / width {worst_u:.3g}, worst |d log10 Omega_0| / width {worst_a:.3g} (margin {MARGIN:g})")


def test_errors_against_pcov_where_the_reference_converged(recorded):
    worst, count, degenerate = 0.0, 0, 0
    for r in converged(recorded):
        if r["fit"]["n_valid"] <= 2:
            assert np.isinf(r["fit"]["M0_err"]) and np.isinf(r["fit"]["fc_err"]) and np.isinf(r["pcov"]).all()
            continue
        ref_m0_err, ref_fc_err = np.sqrt(np.diag(r["pcov"]))
        if not ref_m0_err / r["popt"][0] > 1.0e-20:                 # SciPy's SVD cut dropped the Omega_0 column
            degenerate += 1
            continue
        if r["fit"]["cost"] < 1.0e-20:                              # an exact fit: both errors are roundings of 0
            continue
        count += 1
        for got, want in ((r["fit"]["M0_err"], ref_m0_err), (r["fit"]["fc_err"], ref_fc_err)):
            worst = max(worst, abs(got / want - 1.0))
            assert abs(got / want - 1.0) <= PCOV_TOLERANCE, (r["group"], r["e"], got, want)
    print(f"errors against pcov on {count} fits, worst relative difference {worst:.3g} (allowed {PCOV_TOLERANCE:g}); "
          f"{degenerate} fits with the reference's M0_err / M0 <= 1e-20 left out")
    assert count >= 40


# ---- cases with known answers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    cases = sfc.exact_cases()
    return {name: (c, pp.fit_source_spectra_host(c[0]["average"], c[0]["mask"], c[0]["num_valid"], c[0]["frequencies"],
                                                 "p", model=c[1], weighted=c[2], **c[3])) for name, c in cases.items()}


def test_noise_free_spectra_return_what_was_planted(exact):
    """A noise-free spectrum has P(u*) = 0 up to rounding: the planted parameters come back within the allowance that
    the rounding of y, g and the sums leaves through P'' (spectral_fit_cases.allowance: delta P' / P'')."""
    seen = 0
    for name, ((x, model, weighted, _, expect), fit) in exact.items():
        if "M0" not in expect:
            continue
        seen += 1
        assert fit["reason"][0] == expect["reason"] and fit["success"][0] and not fit["at_bound"][0], name
        ln_x, y, w2, n = sfc.event_terms(x, 0, model, weighted)
        B = sfc.allowance(ln_x, y, w2, n, np.log(expect["fc"]), weighted, False)
        assert not B["flat"]
        assert abs(np.log(fit["fc"][0] / expect["fc"])) <= B["u"], (name, fit["fc"][0])
        assert abs(np.log10(fit["M0"][0] / expect["M0"])) <= B["a"], (name, fit["M0"][0])
        assert fit["cost"][0] <= B["cost"], (name, fit["cost"][0])
        assert fit["Mw"][0] == pp.moment_to_magnitude(fit["M0"][0])
        assert fit["stress_drop_pa"][0] == pp.stress_drop_circular_crack(fit["Mw"][0], fit["fc"][0], "p")
    assert seen == 6
    x = exact["equal_num_valid"][0][0]
    assert np.array_equal(pp.fit_weights(x["num_valid"], True), np.full((1, 25), 0.5))


def test_the_stress_drop_takes_the_phase_and_the_first_guess_does_not(exact):
    x, model, weighted, _, _ = exact["planted_brune"][0]
    p = exact["planted_brune"][1]
    s = pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], "s", model=model)
    assert all(np.array_equal(p[k], s[k]) for k in p if k != "stress_drop_pa")
    assert np.isclose(s["stress_drop_pa"][0] / p["stress_drop_pa"][0], (2.23 / 1.47) ** 3, rtol=1e-14)


def test_few_valid_bins(exact):
    for M in range(4):
        (_, _, _, _, expect), fit = exact[f"M{M}"]
        assert fit["reason"][0] == expect["reason"] and fit["n_valid"][0] == M, M
        if M < 2:
            assert all(np.isnan(fit[k][0]) for k in pp.FIT_KEYS) and not fit["success"][0]
        else:
            assert np.isfinite([fit[k][0] for k in ("M0", "fc", "Mw", "cost", "stress_drop_pa")]).all()
            assert np.isinf(fit["M0_err"][0]) == (M == 2) and np.isinf(fit["fc_err"][0]) == (M == 2)


def test_a_corner_outside_the_interval_ends_at_the_bound(exact):
    fc0 = float(pp.fc_circular_crack(pp.moment_to_magnitude(1.0e13)))
    for name, factor in (("fc_above_band", 1.0e3), ("fc_below_band", 1.0e-3)):
        (x, _, _, _, _), fit = exact[name]
        own = float(pp.fc_circular_crack(pp.moment_to_magnitude(x["average"][0, 0])))
        assert fit["at_bound"][0] and fit["reason"][0] == 4 and not fit["success"][0], name
        assert np.isfinite(fit["M0"][0]) and abs(np.log(fit["fc"][0] / (own * factor))) <= 4 * sfc.EPS * 8.0, name
    assert abs(np.log(fc0 / float(pp.fc_circular_crack(pp.moment_to_magnitude(exact["fc_above_band"][0][0]["average"][0, 0]))))) < 1e-3


def test_the_global_basin_is_found(exact):
    """Two local minima of P with a clear gap: a dense scan of the whole interval names the lower one, and the answer
    lies in it."""
    for name in ("two_basins_high", "two_basins_low"):
        (x, model, weighted, _, _), fit = exact[name]
        ln_x, y, w2, n = sfc.event_terms(x, 0, model, weighted)
        fc0 = float(pp.fc_circular_crack(pp.moment_to_magnitude(x["average"][0, 0])))
        u = np.linspace(np.log(fc0 * 1e-3), np.log(fc0 * 1e3), 20001)
        cost = pp.fit_profile_cost(u, ln_x, y, w2, n)[0]
        inner = np.flatnonzero((cost[1:-1] < cost[:-2]) & (cost[1:-1] < cost[2:])) + 1
        assert len(inner) >= 2, "the case must have two basins"
        depths = np.sort(cost[inner])
        assert depths[1] > 1.05 * depths[0], "with a clear gap"
        best = u[inner[np.argmin(cost[inner])]]
        assert (best > np.median(u[inner])) == (name == "two_basins_high") or len(inner) > 2
        assert abs(np.log(fit["fc"][0]) - best) <= 2 * (u[1] - u[0]) and fit["cost"][0] <= depths[0], name
        assert not fit["at_bound"][0]


def test_exact_ties_go_to_the_lowest_index(exact):
    """A flat spectrum: wherever every 1 + s rounds to 1 the cost is exactly 0, over hundreds of scan points up to the
    upper end.  The lowest index wins each round, so the answer is inside the interval, not at its end."""
    (x, model, weighted, _, _), fit = exact["flat_plateau_ties"]
    assert fit["cost"][0] == 0.0 and not fit["at_bound"][0] and fit["reason"][0] == 0
    ln_x, y, w2, n = sfc.event_terms(x, 0, model, weighted)
    u = np.log(fit["fc"][0])
    fc0 = float(pp.fc_circular_crack(pp.moment_to_magnitude(1.0e13)))
    step = 2.0 * np.log(1.0e3) / (pp.FIT_SCAN_POINTS - 1)
    assert pp.fit_profile_cost(u - step, ln_x, y, w2, n)[0][0] > 0.0 and u < np.log(fc0 * 1.0e3) - 50 * step


def test_the_below_fc_gate_counts_over_all_bins(exact):
    (x, _, _, _, _), fit = exact["below_fc_over_F"]
    below = int((x["frequencies"][~x["mask"][0]] < fit["fc"][0]).sum())
    assert fit["reason"][0] == 3 and not fit["success"][0] and np.isfinite(fit["M0"][0])
    assert below / 25 < 0.1 <= below / fit["n_valid"][0]


def test_values_that_are_not_finite(exact):
    for name in ("bad_nan", "bad_inf", "bad_zero", "bad_negative"):
        fit = exact[name][1]
        assert fit["reason"][0] == 5 and not fit["success"][0] and all(np.isnan(fit[k][0]) for k in pp.FIT_KEYS), name
    x = exact["bad_nan"][0][0]
    masked = x["mask"].copy()
    masked[0, 7] = True                                             # the same bin masked: fitted
    assert pp.fit_source_spectra_host(x["average"], masked, x["num_valid"], x["frequencies"], "p")["reason"][0] == 0
    zero = np.zeros_like(x["num_valid"])                            # a mean of 0: the weights are 0 / 0
    fine = exact["planted_brune"][0][0]
    assert pp.fit_source_spectra_host(fine["average"], fine["mask"], zero, fine["frequencies"], "p",
                                      weighted=True)["reason"][0] == 5


def test_refusals_of_the_definition():
    x = sfc.exact_cases()["planted_brune"][0]
    with pytest.raises(ValueError, match="model"):
        pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], "p", model="haskell")
    with pytest.raises(ValueError, match="phase"):
        pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], "x")


# ---- the comparison that the device is held to: loose for a correct second implementation, sharp on defects ----
SENSITIVITY_CASES = [("planted_weighted_brune",), ("planted_weighted_boatwright",), ("flat_plateau_ties",),
                     ("below_fc_over_F",), ("fc_below_band",), ("low_corner",)]


def _noisy(model, weighted):
    x = sfc.gpu_inputs(3, 25, model, 77)
    x["mask"][:] = False
    if weighted:                                                    # masked bins whose counts move the mean
        x["mask"][:, [2, 9, 10, 20]] = True
        x["num_valid"][:, [2, 9, 10, 20]] = 60
    return x


def sensitivity_inputs():
    cases = sfc.exact_cases()
    sets = [(cases[n][0], cases[n][1], cases[n][2]) for (n,) in SENSITIVITY_CASES]
    sets += [(_noisy(model, weighted), model, weighted) for model in sfc.MODELS for weighted in (False, True)]
    return sets


def test_the_check_passes_the_model_and_rejects_every_planted_defect():
    failed = {d: set() for d in [None] + sfc.DEFECTS}
    for x, model, weighted in sensitivity_inputs():
        want = pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], "p", model=model,
                                          weighted=weighted)
        for defect in failed:
            got = sfc.model_fit(x, "p", model, weighted, defect=defect)
            discrete, worst = sfc.check(got, want, x, model, weighted)
            if not discrete:
                failed[defect].add("discrete")
            failed[defect].update(k for k, v in worst.items() if not v <= 1.0)
    for defect, checks in failed.items():
        print(f"{defect or 'no defect'}: fails {sorted(checks) or 'nothing'}")
    assert failed[None] == set()
    assert len(sfc.DEFECTS) >= 10
    for defect in sfc.DEFECTS:
        assert failed[defect], defect


# ---- the gates and the P-S average ---------------------------------------------------------------------------
def test_moment_magnitudes_host_on_the_recorded_fits(recorded):
    """The reference's arithmetic (BPMF/spectrum.py:1907-1946, :1965-1990) event by event in Python floats, on the
    recorded popt and pcov of two groups taken as P and S: equal bit for bit."""
    g = sfc.golden()
    for gp, gs in (("brune_u_25", "brune_w_25"), ("boatwright_w_16", "boatwright_u_16"), ("brune_u_3", "brune_w_3")):
        fits = {}
        for ph, group in (("p", gp), ("s", gs)):
            popt, pcov = g[f"popt_{group}"], g[f"pcov_{group}"]
            with np.errstate(all="ignore"):
                fits[ph] = {"M0": popt[:, 0], "fc": popt[:, 1], "Mw": pp.moment_to_magnitude(popt[:, 0]),
                            "M0_err": np.sqrt(pcov[:, 0, 0]), "fc_err": np.sqrt(pcov[:, 1, 1]),
                            "success": g[f"success_{group}"]}
        for limits in ((33.0, 33.0), (5.0, 100.0), (1.0e9, 2.0)):
            got = pp.moment_magnitudes_host(fits["p"], fits["s"], max_rel_m0_err_pct=limits[0],
                                            max_rel_fc_err_pct=limits[1])
            for e in range(len(fits["p"]["M0"])):
                total = total_err = norm = 0.0
                for ph in ("p", "s"):
                    f = {k: float(v[e]) for k, v in fits[ph].items()}
                    if not fits[ph]["success"][e]:
                        assert not got["accepted"][ph][e]
                        continue
                    with np.errstate(all="ignore"):
                        rel_m0, rel_fc = 100.0 * np.float64(f["M0_err"]) / f["M0"], 100.0 * np.float64(f["fc_err"]) / f["fc"]
                    ok = not (rel_m0 > limits[0] or f["fc"] < 0.0 or rel_fc > limits[1])
                    assert got["accepted"][ph][e] == ok
                    if ok:
                        total += f["Mw"]
                        total_err += 2.0 / 3.0 * f["M0_err"] / f["M0"]
                        norm += 1
                if norm:
                    assert got["Mw"][e] == total / norm and got["Mw_err"][e] == total_err / norm
                else:
                    assert np.isnan(got["Mw"][e]) and np.isnan(got["Mw_err"][e])
    one = pp.moment_magnitudes_host(fit_s=fits["s"])
    assert set(one["accepted"]) == {"s"}
    with pytest.raises(ValueError):
        pp.moment_magnitudes_host()


# ---- Spectrum.resample ---------------------------------------------------------------------------------------
def test_resample_spectra_host_is_np_interp_and_the_099_rule():
    rng = np.random.default_rng(5)
    bands = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0])
    targets = np.concatenate([[0.1, 0.5, 0.75, 1.0, 29.0, 0.99 * 30.0, np.nextafter(0.99 * 30.0, 0.0), 30.0, 45.0],
                              rng.uniform(0.2, 35.0, 200)])
    spectra = rng.normal(size=(4, 3, len(bands))) * 10.0 ** rng.uniform(-9, -3, (4, 3, 1))
    got = pp.resample_spectra_host(spectra, bands, targets)
    assert got.shape == (4, 3, len(targets))
    for i in np.ndindex(4, 3):
        want = np.interp(targets, bands, np.abs(spectra[i]))
        want[targets >= 0.99 * np.max(bands)] = 0.0
        assert np.array_equal(got[i], want)
    assert (got[..., targets >= 0.99 * 30.0] == 0.0).all() and (got[..., 6] > 0.0).all()
    assert np.array_equal(got[..., 0], np.abs(spectra[..., 0]))     # below the first band: its value
    with pytest.raises(ValueError):
        pp.resample_spectra_host(spectra, bands[::-1], targets)
