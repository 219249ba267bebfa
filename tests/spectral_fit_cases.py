"""Cases, allowances and an independent model for the Brune / Boatwright fit (postprocess.fit_source_spectra_host,
bpmf_fit_spectra_dev); shared by tests/test_spectral_fit_definition.py, tests/test_gpu_spectral_fit.py,
tests/golden/make_spectral_fit_golden.py and tools/probe_spectral_fit.py.

THE ALLOWANCES (written before the first run on a GPU; `allowance`).  The device and the host run the same operations in
the same order; they differ in the rounding of exp, log10, pow and log.  profiles/source_spectra_edges.txt measured the
device's exp and log10 at 1 ulp and pow at 1 ulp (2 allowed); log is not measured there and gets OpenCL's 3 ulp.  With
eps = 2^-53 and an ulp <= 2 eps relative, through the M terms of an event, for d = ln x - u, s = exp(n d), t = s/(1+s):
  delta(n d)  = n (2 U_LOG eps |ln x| + eps |d|)
  delta s / s = delta(n d) + 2 U_EXP eps
  delta g     = (2 / n) (2 U_LOG10 eps |log10(1 + s)| + (t delta s / s + eps) / ln 10)
  delta y     = 2 U_LOG10 eps |y|;   delta w^2 / w^2 = KAPPA_W eps = (4 U_EXP + 8) eps (weighted) or 0
  delta z     = delta y + delta g + eps |z|
  delta a     = max delta z + (M + 2) eps sum w^2 |z| / sum w^2 + 2 KAPPA_W eps sum w^2 |z - a| / sum w^2
  delta rho   = delta z + delta a + eps |rho|
  delta P     = sum w^2 (|rho| + delta rho) delta rho + (KAPPA_W + M + 3) eps P
  delta g'    = (2 / ln 10) (t (1 - t) (delta(n d) + 2 U_EXP eps) + 2 eps t) + eps |g'|
  delta c     = 2 max delta g' + (KAPPA_W + M + 2) eps max |g'|              (c = g' - a')
  delta P'    = sum w^2 (delta rho |c| + (|rho| + delta rho) delta c) + (KAPPA_W + M + 3) eps sum w^2 |rho c|
Both sides may err, so  B_cost = 2 delta P + P'' B_u^2 / 2,  B_u = 2 delta P' / P'' + BOUND_ULPS eps max(1, |u|) (the
second term: the interval's ends go through two pow and a log),  B_a = 2 delta a + |a'| B_u.  An event at a bound has
u* equal to the end on both sides: B_u is the second term alone.  An event with P'' <= FLAT_FLOOR sum w^2 is FLAT: the
minimum is not located by its curvature and it is judged on the cost only.  The errors and the stress drop follow from
these (`check`).
"""
import os

import numpy as np

from seismic_bpmf_amd import postprocess as pp

EPS = 2.0**-53
U_EXP, U_LOG10, U_POW, U_LOG = 1, 1, 2, 3
KAPPA_W = 4 * U_EXP + 8
BOUND_ULPS = 256
FLAT_FLOOR = 1.0e-8
LN10 = np.log(10.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_fit.npz")

MODELS = ("brune", "boatwright")
# group -> (model, weighted, F, E, seed): what tests/golden/make_spectral_fit_golden.py runs the reference on
RECORDED = {f"{model}_{'w' if weighted else 'u'}_{F}": (model, weighted, F, 6, 1000 * i + 10 * F + weighted)
            for i, model in enumerate(MODELS) for weighted in (False, True) for F in (3, 5, 8, 16, 25, 40, 64)}


# decades of noise of a group's six events: from what a sparse network leaves down to a smooth average, where
# curve_fit's own termination (ftol = 1e-8) more often ends on the minimum itself
RECORDED_NOISE = (0.15, 0.05, 0.03, 0.02, 0.02, 0.15)


def spectrum(f, omega0, fc, n):
    """omega0 / (1 + (f / fc)^n)^(2 / n): Brune (n = 2) or Boatwright (n = 4)."""
    return omega0 / (1.0 + (f / fc) ** n) ** (2.0 / n)


def recorded_inputs(group):
    """Six synthetic averages of F bins over 0.5 .. 40 Hz with RECORDED_NOISE decades of noise, a corner inside the
    band, bins masked at random (event 0: none; event 5: more than half, the reference's 'not enough valid points')."""
    model, weighted, F, E, seed = RECORDED[group]
    rng = np.random.default_rng(seed)
    f = np.geomspace(0.5, 40.0, F)
    omega0 = 10.0 ** rng.uniform(11.0, 15.0, E)
    fc = np.exp(rng.uniform(np.log(1.5), np.log(15.0), E))
    noise = np.array(RECORDED_NOISE)[:, None] * rng.normal(size=(E, F))
    average = spectrum(f[None], omega0[:, None], fc[:, None], pp.FIT_MODELS[model]) * 10.0**noise
    mask = rng.random((E, F)) < (0.2 if F >= 8 else 0.0)
    mask[0] = False
    mask[5] = rng.permutation(F) < (F // 2 + 1)
    num_valid = rng.integers(2, 25, (E, F)).astype(np.int32)
    return {"average": average, "mask": mask, "num_valid": num_valid, "frequencies": f}


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- cases with known answers -------------------------------------------------------------------------------
def exact_cases():
    """{name: (inputs, model, weighted, options, expectation)}: one event each, noise-free unless said."""
    f25 = np.geomspace(0.5, 40.0, 25)
    cases = {}

    def put(name, average, mask, num_valid, f, model="brune", weighted=False, expect=None, **options):
        x = {"average": np.atleast_2d(average).astype(np.float64), "mask": np.atleast_2d(mask).astype(bool),
             "num_valid": np.atleast_2d(num_valid).astype(np.int32), "frequencies": np.asarray(f, dtype=np.float64)}
        cases[name] = (x, model, weighted, options, expect or {})

    ones = np.full(25, 7)
    for model in MODELS:
        n = pp.FIT_MODELS[model]
        put(f"planted_{model}", spectrum(f25, 3.0e13, 4.0, n), np.zeros(25, bool), ones, f25, model,
            expect={"reason": 0, "M0": 3.0e13, "fc": 4.0})
        put(f"planted_weighted_{model}", spectrum(f25, 2.0e12, 9.0, n), np.zeros(25, bool), 2 + np.arange(25) % 11, f25,
            model, True, expect={"reason": 0, "M0": 2.0e12, "fc": 9.0})
    f3 = np.array([1.0, 4.0, 16.0])
    for M in range(4):
        mask = np.arange(3) >= M
        put(f"M{M}", spectrum(f3, 1.0e13, 3.0, 2.0) * np.array([1.0, 1.1, 0.9]), mask, [5, 6, 7], f3,
            expect={"reason": (1, 2, 0, 0)[M], "n_valid": M, "inf_errors": M == 2})
    put("equal_num_valid", spectrum(f25, 5.0e12, 6.0, 2.0), np.zeros(25, bool), ones, f25, "brune", True,
        expect={"reason": 0, "M0": 5.0e12, "fc": 6.0, "weights": 0.5})
    late = np.zeros(25, bool)
    late[:3] = True
    put("first_unmasked_not_0", spectrum(f25, 4.0e13, 5.0, 2.0), late, ones, f25, expect={"reason": 0, "M0": 4.0e13,
                                                                                          "fc": 5.0})
    fc0 = float(pp.fc_circular_crack(pp.moment_to_magnitude(1.0e13)))
    put("fc_above_band", spectrum(f25, 1.0e13, fc0 * 3.0e4, 2.0), np.zeros(25, bool), ones, f25,
        expect={"reason": 4, "at_bound": True, "fc": fc0 * 1.0e3})
    steep = spectrum(f25, 1.0e13 * (f25[0] / (fc0 * 3.0e-5)) ** 2, fc0 * 3.0e-5, 2.0)          # first value ~ 1e13
    put("fc_below_band", steep, np.zeros(25, bool), ones, f25, expect={"reason": 4, "at_bound": True})
    # two basins of P with a clear gap (found by a search over scattered four-bin spectra): the lower one at the higher
    # corner in the first, at the lower corner in the second
    f4 = np.geomspace(0.5, 40.0, 4)
    put("two_basins_high", 10.0 ** np.array([13.674, 10.568, 11.772, 11.91]), np.zeros(4, bool), [5, 6, 7, 8], f4,
        "boatwright", expect={"global": True})
    put("two_basins_low", 10.0 ** np.array([13.0, 13.675, 10.935, 11.985]), np.zeros(4, bool), [5, 6, 7, 8], f4,
        "boatwright", expect={"global": True})
    # (frequencies so far below the interval's upper end that there every 1 + s rounds to 1: exact ties at cost 0)
    put("flat_plateau_ties", np.full(25, 1.0e13), np.zeros(25, bool), ones, np.geomspace(1.0e-6, 1.0e-5, 25),
        expect={"at_bound": False})
    below = np.ones(25, bool)
    below[[3, 5, 8, 10, 12, 14, 16, 17, 18, 19, 20, 21, 22]] = False                            # M = 13 of F = 25
    put("below_fc_over_F", spectrum(f25, 1.0e13, 0.5 * (f25[5] + f25[8]), 2.0), below, ones, f25,
        expect={"reason": 3})
    for name, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("negative", -1.0e12)):
        bad = spectrum(f25, 1.0e13, 4.0, 2.0)
        bad[7] = value
        put(f"bad_{name}", bad, np.zeros(25, bool), ones, f25, expect={"reason": 5})
    put("low_corner", spectrum(f25, 1.0e13, fc0 * 0.03, 2.0) * (1.0 + 0.02 * np.cos(np.arange(25))), np.zeros(25, bool),
        ones, f25, expect={})
    return cases


def stack(names, cases=None):
    """The events of several one-event cases of equal F, model and options in one batch."""
    cases = cases or exact_cases()
    xs = [cases[n][0] for n in names]
    return {"average": np.concatenate([x["average"] for x in xs]), "mask": np.concatenate([x["mask"] for x in xs]),
            "num_valid": np.concatenate([x["num_valid"] for x in xs]), "frequencies": xs[0]["frequencies"]}


# ---- shapes of the GPU test ---------------------------------------------------------------------------------
GPU_SHAPES = [(1, 3), (3, 25), (65, 64), (3, 65), (3, 1024), (65, 25)]


def gpu_inputs(E, F, model, seed):
    """E events of F bins: event e has M = (0, 1, 2, 3, F)[e % 5] valid bins when E >= 3 (F for E == 1), a corner
    inside the band and 0.1 decades of noise."""
    rng = np.random.default_rng(seed)
    f = np.geomspace(0.5, 40.0, F)
    omega0 = 10.0 ** rng.uniform(11.0, 15.0, E)
    fc = np.exp(rng.uniform(np.log(1.5), np.log(15.0), E))
    average = spectrum(f[None], omega0[:, None], fc[:, None], pp.FIT_MODELS[model]) * 10.0 ** (0.1 * rng.normal(size=(E, F)))
    mask = np.zeros((E, F), bool)
    for e in range(E):
        M = F if E == 1 else (F, 3, 0, 1, 2)[e % 5]
        M = min(M, F)
        keep = np.sort(rng.permutation(F)[:M]) if e % 2 else np.arange(M)
        mask[e] = True
        mask[e, keep] = False
    if E == 65:                                                     # the rest of a day: random masks, mostly fitted
        mask[5:] = rng.random((E - 5, F)) < 0.25
    return {"average": average, "mask": mask, "num_valid": rng.integers(2, 25, (E, F)).astype(np.int32),
            "frequencies": f}


# ---- the allowances -----------------------------------------------------------------------------------------
def event_terms(x, e, model, weighted):
    """(ln_x, y, w2, n) of event e as the definition forms them, or None without unmasked bins."""
    keep = ~x["mask"][e]
    if not keep.any():
        return None
    with np.errstate(all="ignore"):
        y = np.log10(x["average"][e][keep])
        w = pp.fit_weights(x["num_valid"][e:e + 1], weighted)[0][keep]
    return np.log(x["frequencies"][keep]), y, w * w, pp.FIT_MODELS[model]


def allowance(ln_x, y, w2, n, u, weighted, at_bound):
    """{"cost", "u", "a", "flat", "p2", "centred", "plain"} for one fitted event at the definition's u (module docstring)."""
    M = len(y)
    kw = KAPPA_W if weighted else 0
    d = ln_x - u
    s = np.exp(n * d)
    t = 1.0 / (1.0 + np.exp(-n * d))
    L = np.log10(1.0 + s)
    g = (2.0 / n) * L
    z = y + g
    sw = w2.sum()
    a = (w2 * z).sum() / sw
    rho = z - a
    d_nd = n * (2 * U_LOG * EPS * np.abs(ln_x) + EPS * np.abs(d))
    d_s = d_nd + 2 * U_EXP * EPS
    d_g = (2.0 / n) * (2 * U_LOG10 * EPS * np.abs(L) + (t * d_s + EPS) / LN10)
    d_z = 2 * U_LOG10 * EPS * np.abs(y) + d_g + EPS * np.abs(z)
    d_a = d_z.max() + (M + 2) * EPS * (w2 * np.abs(z)).sum() / sw + 2 * kw * EPS * (w2 * np.abs(rho)).sum() / sw
    d_rho = d_z + d_a + EPS * np.abs(rho)
    P = 0.5 * (w2 * rho * rho).sum()
    d_P = (w2 * (np.abs(rho) + d_rho) * d_rho).sum() + (kw + M + 3) * EPS * P
    g1 = -(2.0 / LN10) * t
    a1 = (w2 * g1).sum() / sw
    c = g1 - a1
    d_g1 = (2.0 / LN10) * (t * (1.0 - t) * (d_nd + 2 * U_EXP * EPS) + 2 * EPS * t) + EPS * np.abs(g1)
    d_c = 2 * d_g1.max() + (kw + M + 2) * EPS * np.abs(g1).max()
    d_P1 = (w2 * (d_rho * np.abs(c) + (np.abs(rho) + d_rho) * d_c)).sum() + (kw + M + 3) * EPS * (w2 * np.abs(rho * c)).sum()
    centred, plain = (w2 * c * c).sum(), (w2 * g1 * g1).sum()
    p2 = centred + (w2 * rho * (2.0 * n / LN10) * t * (1.0 - t)).sum()
    ends = BOUND_ULPS * EPS * max(1.0, abs(u))
    flat = not at_bound and not p2 > FLAT_FLOOR * sw
    b_u = ends if at_bound else (np.inf if flat else 2.0 * d_P1 / p2 + ends)
    b_cost = 2.0 * d_P + (0.0 if flat or at_bound else 0.5 * p2 * b_u * b_u)
    if at_bound:                                                    # the end itself moves by `ends`: P' need not vanish
        b_cost += abs((w2 * rho * c).sum()) * ends
    return {"cost": b_cost, "u": b_u, "a": 2.0 * d_a + abs(a1) * (0.0 if flat else b_u), "flat": flat, "p2": p2,
            "centred": centred, "plain": plain, "P": P}


DISCRETE = ("n_valid", "success", "at_bound", "reason")


def check(got, want, x, model, weighted):
    """Compares a dict of (E,) arrays with the definition's.  Returns (discrete equal, {quantity: worst err / B}) over
    the events the definition reports values for; the quantities are cost, ln_fc, log10_M0, errors, stress_drop.  Events
    without values (reasons 1, 2, 5) must hold NaN in every float output."""
    discrete = all(np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64))
                   for k in DISCRETE)
    worst = {"cost": 0.0, "ln_fc": 0.0, "log10_M0": 0.0, "errors": 0.0, "stress_drop": 0.0}
    for e in range(len(want["reason"])):
        if want["reason"][e] in (1, 2, 5):
            discrete = discrete and all(np.isnan(got[k][e]) for k in pp.FIT_KEYS)
            continue
        ln_x, y, w2, n = event_terms(x, e, model, weighted)
        u = np.log(want["fc"][e])
        B = allowance(ln_x, y, w2, n, u, weighted, bool(want["at_bound"][e]))
        with np.errstate(all="ignore"):
            worst["cost"] = max(worst["cost"], abs(got["cost"][e] - want["cost"][e]) / B["cost"])
            if B["flat"]:
                continue
            err_u = abs(np.log(got["fc"][e]) - u)
            err_a = abs(np.log10(got["M0"][e]) - np.log10(want["M0"][e]))
            worst["ln_fc"] = max(worst["ln_fc"], err_u / (B["u"] + 4 * EPS * max(1.0, abs(u))))
            worst["log10_M0"] = max(worst["log10_M0"], err_a / (B["a"] + 2 * (U_POW + U_LOG10 + 1) * EPS * 16.0))
            # stress drop ~ M0 / fc^-3: 3 B_u + ln 10 (B_a + what pow and log10 add to Mw and back) + the two pow
            b_stress = 3.0 * B["u"] + LN10 * (B["a"] + 64 * EPS) + 16 * (U_POW + 2) * EPS
            worst["stress_drop"] = max(worst["stress_drop"],
                                       abs(got["stress_drop_pa"][e] / want["stress_drop_pa"][e] - 1.0) / b_stress)
            if len(y) > 2 and want["cost"][e] > 0.0 and B["centred"] > 0.0:
                # fc_err = fc sqrt(s^2 / D), M0_err = M0 ln 10 sqrt(s^2 sum w^2 g'^2 / (sum w^2 D)); |dD/du| <= 2 n
                # sqrt(D sum w^2 g'^2) (Cauchy-Schwarz, |g''| <= n |g'|), D centred with a cancellation of plain / D
                ratio = B["plain"] / B["centred"]
                b_err = (B["cost"] / want["cost"][e] + (1.0 + 2.0 * n * np.sqrt(ratio) + 2.0 * n) * B["u"] + LN10 * B["a"]
                         + 16 * (len(y) + 8 + (KAPPA_W if weighted else 0)) * EPS * ratio)
                for k in ("M0_err", "fc_err"):
                    if np.isfinite(want[k][e]) and want[k][e] > 0.0:
                        worst["errors"] = max(worst["errors"], abs(got[k][e] / want[k][e] - 1.0) / b_err)
                    else:
                        discrete = discrete and (got[k][e] == want[k][e] or (np.isnan(got[k][e]) and np.isnan(want[k][e])))
            else:
                discrete = discrete and all(got[k][e] == want[k][e] or (np.isnan(got[k][e]) and np.isnan(want[k][e]))
                                            or (want["cost"][e] == 0.0 and len(y) > 2) for k in ("M0_err", "fc_err"))
    return discrete, worst


# ---- an independent model, with the defects the checks must reject ---------------------------------------------
DEFECTS = ["weights dropped", "1 / w for w", "mean of num_valid over valid bins", "Brune's exponent in Boatwright",
           "M - 1 for M - 2", "natural log for log10 in J", "scan without the lowest-index tie rule",
           "no Newton finish", "bounds asymmetric", "below-fc fraction over M"]


def model_fit(x, phase, model, weighted, min_fraction_valid_points=0.5, min_fraction_valid_points_below_fc=0.1,
              defect=None):
    """The fit written a second time, from the issue's text and in other formulas (f / fc raised to n, NumPy's own sums,
    uncentred derivatives); `defect` plants one of DEFECTS."""
    n = pp.FIT_MODELS[model]
    if defect == "Brune's exponent in Boatwright":
        n = 2.0
    f = x["frequencies"]
    E, F = x["average"].shape
    out = {k: np.full(E, np.nan) for k in pp.FIT_KEYS}
    out.update(n_valid=np.zeros(E, np.int32), success=np.zeros(E, bool), at_bound=np.zeros(E, bool),
               reason=np.zeros(E, np.uint8))

    def parts(u, xs, y, w2):
        r = xs[None, :] / np.exp(np.atleast_1d(u))[:, None]
        g = (2.0 / n) * np.log10(1.0 + r**n)
        a = ((y + g) * w2).sum(axis=1) / w2.sum()
        rho = y + g - a[:, None]
        return 0.5 * (w2 * rho**2).sum(axis=1), a, rho, r

    with np.errstate(all="ignore"):
        for e in range(E):
            keep = ~x["mask"][e]
            M = out["n_valid"][e] = int(keep.sum())
            if M == 0 or M / F < min_fraction_valid_points:
                out["reason"][e] = 1 if M == 0 else 2
                continue
            nv = x["num_valid"][e].astype(np.float64)
            mean = nv[keep].mean() if defect == "mean of num_valid over valid bins" else nv.mean()
            w = 1.0 / (1.0 + np.exp(-(nv - mean) / mean))[keep] if weighted and defect != "weights dropped" else np.ones(M)
            if defect == "1 / w for w":
                w = 1.0 / w
            y, xs = np.log10(x["average"][e][keep]), f[keep]
            if not (np.isfinite(y).all() and np.isfinite(w).all()):
                out["reason"][e] = 5
                continue
            w2 = w**2
            fc0 = pp.fc_circular_crack(pp.moment_to_magnitude(x["average"][e][keep][0]))
            lo = np.log(fc0 * (1.0e-1 if defect == "bounds asymmetric" else 1.0e-3))
            hi = np.log(fc0 * 1.0e3)
            a_, b_, count = lo, hi, pp.FIT_SCAN_POINTS
            for _ in range(1 + pp.FIT_ZOOM_ROUNDS):
                grid = np.linspace(a_, b_, count)
                grid[0], grid[-1] = a_, b_
                cost = parts(grid, xs, y, w2)[0]
                cost = np.where(np.isnan(cost), np.inf, cost)
                i = int(np.argmin(cost))
                if defect == "scan without the lowest-index tie rule":
                    i = int(np.flatnonzero(cost == cost[i])[-1])
                a_, b_, u = grid[max(i - 1, 0)], grid[min(i + 1, count - 1)], grid[i]
                count = pp.FIT_ZOOM_POINTS
            for _ in range(0 if defect == "no Newton finish" else pp.FIT_NEWTON_STEPS):
                _, _, rho, r = parts(u, xs, y, w2)
                t = (r**n / (1.0 + r**n))[0]
                g1, g2 = -2.0 / LN10 * t, 2.0 * n / LN10 * t * (1.0 - t)
                a1 = (w2 * g1).sum() / w2.sum()
                p1 = (w2 * rho[0] * g1).sum()
                p2 = (w2 * g1 * g1).sum() - a1 * a1 * w2.sum() + (w2 * rho[0] * g2).sum()
                if p2 > 0.0 and np.isfinite(p1 / p2):
                    u = min(max(u - p1 / p2, a_), b_)
            cost, a, rho, r = parts(u, xs, y, w2)
            cost, a = cost[0], a[0]
            M0, fc = 10.0**a, np.exp(u)
            Mw = pp.moment_to_magnitude(M0)
            stress = pp.stress_drop_circular_crack(Mw, fc, phase)
            if not np.isfinite([M0, fc, cost, Mw, stress]).all():
                out["reason"][e] = 5
                continue
            # the covariance in the reference's own coordinates (Omega_0, fc)
            t = (r**n / (1.0 + r**n))[0]
            J = np.stack([w / (M0 * (1.0 if defect == "natural log for log10 in J" else LN10)),
                          -w * (-2.0 / LN10 * t) / fc], axis=1)
            scale = np.array([M0, fc])[None, :]                                        # (conditioning only)
            dof = M - 1 if defect == "M - 1 for M - 2" else M - 2
            if M > 2:
                pcov = 2.0 * cost / dof * np.linalg.inv((J * scale).T @ (J * scale)) * np.outer(scale[0], scale[0])
                errs = np.sqrt(np.diag(pcov))
            else:
                errs = np.array([np.inf, np.inf])
            out["M0"][e], out["fc"][e], out["Mw"][e], out["cost"][e], out["stress_drop_pa"][e] = M0, fc, Mw, cost, stress
            out["M0_err"][e], out["fc_err"][e] = errs
            out["at_bound"][e] = u == lo or u == hi
            over = M if defect == "below-fc fraction over M" else F
            if out["at_bound"][e]:
                out["reason"][e] = 4
            elif (xs < fc).sum() / over < min_fraction_valid_points_below_fc:
                out["reason"][e] = 3
    out["success"] = out["reason"] == 0
    return out
