"""Inputs, options and the comparison's own checks for the propagation corrections, network-average spectra and the
approximate moment magnitude (postprocess.source_spectra_host, network_average_spectrum_host,
approximate_moment_magnitude_host; csrc/source_spectra.hip).  Everything is regenerated from seeds; only the
reference's recorded answers live in tests/golden/source_spectra.npz (tests/golden/make_source_spectra_golden.py).

An event's spectra are a Brune plateau times a lognormal factor; the noise is the signal divided by a ratio, so that
the SNR is that ratio: powers of two (exact quotients: 1, 4, THRESHOLD itself, 16, 32 -- so `<`, `>` and `>=` at the
threshold are all exercised) or a continuous value kept 1 % away from THRESHOLD.  Events cycle through the numbers
of stations that hold a band above the threshold (0, 1, 5, 6, 7, all: the max_num_bad_measurements edge), through 1 .. 4
such bands per station, and through location errors that drop none, some and all stations."""
import numpy as np

THRESHOLD = 8.0                      # exactly representable, in float32 too
WEIGHT_MAX = 3.0
MAX_BAD = 6
MEDIUM = {"rho_source_kgm3": 2700.0, "rho_receiver_kgm3": 2600.0, "vp_source_ms": 6000.0, "vp_receiver_ms": 5500.0,
          "vs_source_ms": 3500.0, "vs_receiver_ms": 3200.0, "Q_1HZ": 33.0, "attenuation_n": 0.75}
PREFACTOR = {"p": 2.25, "s": 1.0}
SCALING = 2.0 / 3.0
PHASES = ("p", "s")

# name: (seed, E, S, C (0: (E, S, F) spectra), F, special)
CASES = {
    "small": (11, 3, 5, 0, 4, ()),
    "edge": (12, 12, 9, 0, 12, ("zeros", "nan", "missing_noise", "absent")),
    "components": (13, 6, 4, 3, 7, ("zeros", "absent", "missing_noise")),
    "one_station": (14, 3, 1, 0, 5, ()),
    "two_stations": (15, 4, 2, 0, 6, ("absent",)),
    "c63": (16, 2, 21, 3, 63, ("nan",)),
    "c64": (17, 2, 64, 0, 64, ("zeros",)),
    "c65": (18, 2, 13, 5, 65, ("absent",)),
    "batch": (19, 70, 6, 0, 9, ("zeros", "absent", "missing_noise")),
    "ceiling": (20, 1, 256, 0, 1024, ()),
}
RECORDED = ("small", "edge", "components", "one_station", "two_stations")      # in the golden file
GPU_CASES = tuple(CASES)

# (average_log, reduce, min_num_valid_channels_per_freq_bin, max_relative_distance_err_pct)
AVERAGE_OPTIONS = [(True, "mean", 0, 25.0), (True, "median", 0, 25.0), (False, "mean", 0, 25.0),
                   (False, "median", 0, 25.0), (True, "mean", 3, 25.0), (True, "median", 3, 1e9),
                   (False, "mean", 10 ** 6, 25.0), (True, "mean", 0, 0.0)]
# (num_averaging_bands, low_snr_freq_min_hz)
MW_OPTIONS = [(1, 2.0), (2, 2.0), (3, 0.0), (1, 1e9)]


def average_kwargs(option):
    return dict(snr_threshold=THRESHOLD, average_log=option[0], reduce=option[1],
                min_num_valid_channels_per_freq_bin=option[2], max_relative_distance_err_pct=option[3])


def mw_kwargs(option):
    return dict(snr_threshold=THRESHOLD, num_averaging_bands=option[0], low_snr_freq_min_hz=option[1],
                magnitude_log_moment_scaling=SCALING, weight_max=WEIGHT_MAX, max_num_bad_measurements=MAX_BAD)


_cache = {}


def inputs(name):
    """The case's inputs as a dict of read-only arrays; computed once."""
    if name in _cache:
        return _cache[name]
    seed, E, S, C, F, special = CASES[name]
    rng = np.random.default_rng(seed)
    lead = (E, S) if C == 0 else (E, S, C)
    f = np.logspace(np.log10(0.5), np.log10(20.0), F)
    plateau = 10.0 ** rng.uniform(-9.0, -6.0, size=(E,) + (1,) * len(lead[1:]) + (1,))
    corner = rng.uniform(2.0, 15.0, size=plateau.shape)
    signal = plateau / (1.0 + (f / corner) ** 2) * np.exp(rng.normal(0.0, 0.4, size=lead + (F,)))
    # the SNR: low everywhere, then 1 .. 4 bands above the threshold at the stations the event's turn names
    exact = np.array([1.0, 4.0, THRESHOLD, 0.5])
    ratio = np.where(rng.random(lead + (F,)) < 0.4, exact[rng.integers(0, 4, size=lead + (F,))],
                     rng.uniform(0.3, 0.99 * THRESHOLD, size=lead + (F,)))
    n_good = [0, 1, 5, 6, 7, S]
    for e in range(E):
        good = rng.permutation(S)[:min(n_good[e % 6], S)]
        for s in good:
            for c in range(max(C, 1)):
                bands = rng.permutation(F)[:1 + (e + s + c) % 4]
                high = np.where(rng.random(len(bands)) < 0.5, np.array([16.0, 32.0])[rng.integers(0, 2, len(bands))],
                                rng.uniform(1.01 * THRESHOLD, 50.0, len(bands)))
                ratio[(e, s, bands) if C == 0 else (e, s, c, bands)] = high
    noise = signal / ratio
    present = np.ones((E, S), dtype=bool)
    noise_present = np.ones((E, S), dtype=bool)
    dist = rng.uniform(5.0, 60.0, size=(E, S))
    epi = np.sqrt(np.maximum(dist ** 2 - rng.uniform(1.0, 4.5, size=(E, 1)) ** 2, 1.0))
    hmax = np.array([0.3, 4.0, 400.0])[np.arange(E) % 3] * rng.uniform(0.9, 1.1, E)      # none, some, all dropped
    vmax = 0.5 * hmax
    if E == 1:
        hmax, vmax = np.array([0.3]), np.array([0.2])
    if "zeros" in special:
        signal[0, 0, ..., 1] = 0.0                       # x / noise: SNR 0, log10's domain
        noise[0, 0, ..., 1] = 0.0                        # 0 / 0
        noise[0, max(S - 2, 0), ..., 0] = 0.0            # x / 0: inf
        signal[E - 1, 0] = 0.0                           # a station of zeros: measurement 0, SNR 0
    if "nan" in special:                                 # in an event whose stations are all there and all used
        signal[3 % E, 0, ..., 2] = np.nan
        noise[3 % E, S - 1, ..., 0] = np.nan
        signal[3 % E, 1 % S, ..., 3] = 0.0               # 0 / NaN: an SNR that is not masked on a value log10 masks
        noise[3 % E, 1 % S, ..., 3] = np.nan
    if "missing_noise" in special:
        noise_present[0, 1 % S] = False
        noise_present[E - 1, :] = False
    if "absent" in special:
        present[0, S - 1] = False
        present[1 % E, :] = False                        # an event without a station
        if E > 2:
            present[2, 0] = False
    signal[~present] = 0.0                               # what fft_spectra leaves for a window that is not valid
    noise[~noise_present] = 0.0
    out = dict(frequencies=f, signal=signal, noise=noise, present=present, noise_present=noise_present, dist=dist,
               epi=epi, tt_p=dist / 6.0 + rng.uniform(0.0, 0.2, size=(E, S)),
               tt_s=dist / 3.5 + rng.uniform(0.0, 0.3, size=(E, S)), hmax=hmax, vmax=vmax,
               location_err=np.sqrt(hmax ** 2 + vmax ** 2))
    for a in out.values():
        a.setflags(write=False)
    _cache[name] = out
    return out


def phase_arguments(name, phase, attenuation="reference"):
    """What source_spectra_host and the device call take for one phase of a case, beside the options."""
    from seismic_bpmf_amd import postprocess as pp
    x = inputs(name)
    k = PHASES.index(phase)
    which, q_rows = pp.attenuation_plan(x["frequencies"], MEDIUM, PREFACTOR, attenuation)
    return dict(signal=x["signal"] * (1.0 + 0.25 * k), noise=x["noise"], present=x["present"],
                noise_present=x["noise_present"], dist_km=x["dist"], tt_sec=x["tt_" + which[k]],
                location_err_km=x["location_err"], frequencies=x["frequencies"], q_row=q_rows[k],
                geometry_constant=pp.geometry_constants(MEDIUM)[k], radiation=(pp.RADIATION_P, pp.RADIATION_S)[k])


# ---- the comparison's own checks: what the GPU tests apply to the device, and the host test to planted defects ----
U = 2.0 ** -53
LN10 = float(np.log(10.0))
# Allowances per call of a device function against the correctly rounded value, in ulp (2 U relative).  ASSUMPTION: no
# accuracy statement of the ROCm device library is installed beside it; these are the figures of HIP's published
# math-API table for double (exp, log10: 1 ulp; pow: 1 ulp, taken as 2; sqrt and division: correctly rounded, taken as
# 1).  The host's own functions are allowed 1 ulp each.
ULP_EXP, ULP_LOG10, ULP_POW, ULP_SQRT_DIV = 1, 1, 2, 1
CORRECTED_ULP = 2 * (ULP_EXP + 1) + 2      # exp on both sides, then two roundings: relative 2 U each
EXP_STEPS = ULP_EXP + 1                    # how far the device's attenuation factor may lie from the host's, in ulp


def same_discrete(got, want, keys):
    for k in keys:
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return False
    return True


def corrected_ok(got, signal, geometry, att, present):
    """The device's corrected spectrum is fl(fl(x g) a') for an a' within EXP_STEPS ulp of the host's attenuation
    factor: two roundings, geometry first -- the structure itself, which a bound in ulp could not tell from
    fl(x fl(g a)).  NaN and 0 must agree exactly.  Returns the fraction of elements that fail."""
    first = signal * geometry
    ok = np.zeros(got.shape, dtype=bool)
    with np.errstate(all="ignore"):
        a = att.copy()
        for _ in range(EXP_STEPS):
            a = np.nextafter(a, -np.inf)
        for _ in range(2 * EXP_STEPS + 1):
            ok |= (got == first * a) | (np.isnan(got) & np.isnan(first * a))
            a = np.nextafter(a, np.inf)
    wide = (slice(None), slice(None)) + (None,) * (got.ndim - 2)
    ok = np.where(np.broadcast_to(present[wide], got.shape), ok, got == 0.0)
    return 1.0 - ok.mean()


def average_allowance(want, n_channels, average_log, largest):
    """|got - want| allowed for `average` and `std` of one call, (E, F) each, from the operation count: the inputs (the
    corrected spectra) within CORRECTED_ULP ulp; with average_log a log10 on both sides and exp(mean log(10)) on
    both sides; n adds and a division; `largest` (E, F): the largest |value averaged| of the bin (|log10| or the
    value itself).  See DESIGN.md section 4."""
    n = n_channels
    if average_log:
        each = (CORRECTED_ULP * 2 * U) / LN10 + (ULP_LOG10 + 1) * 2 * U * largest          # one log10 value
        centre = each + (n + 2) * U * largest                                               # mean or median of them
        average = np.abs(want["average"]) * (LN10 * centre + 2 * U * LN10 * largest + (ULP_EXP + 1) * 2 * U + 2 * U)
    else:
        each = CORRECTED_ULP * 2 * U * largest
        centre = each + (n + 2) * U * largest
        average = centre + 0.0 * want["average"]
    delta = each + centre                                    # of one deviation from the mean
    s = np.nan_to_num(want["std"], nan=0.0, posinf=0.0)
    var_err = 2.0 * delta * s + delta * delta + (n + 3) * 2 * U * s * s
    std = var_err / np.maximum(s, np.sqrt(var_err) + 1e-300) + 2 * ULP_SQRT_DIV * 2 * U * s
    return average, std


def worst_ratio(got, want, allow):
    """max |got - want| / allow over the elements where want is finite; inf where NaN / inf patterns differ."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    finite = np.isfinite(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(got[~finite & ~np.isnan(want)],
                                                                                want[~finite & ~np.isnan(want)]):
        return np.inf
    if not finite.any():
        return 0.0
    err = np.abs(got[finite] - want[finite])
    a = np.broadcast_to(allow, want.shape)[finite]
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(a, 1e-320))
    return float(ratio.max())


def largest_averaged(corrected, snr, used, option, C):
    """(E, F): the largest |value| that enters a bin's average, and the number of used channels (E,)."""
    E = corrected.shape[0]
    x = corrected.reshape(E, -1, corrected.shape[-1])
    with np.errstate(all="ignore"):
        v = np.abs(np.log10(x)) if option[0] else np.abs(x)
    keep = np.repeat(used, C, axis=1)[:, :, None] & np.isfinite(v)
    return np.where(keep, v, 0.0).max(axis=1), np.repeat(used, C, axis=1).sum(axis=1)


def check_average(got, want, option, C=1):
    """The comparison of stages 1-3: (discrete outputs equal, worst err / allowance of average, of std, fraction of
    `corrected` that fails corrected_ok is left to the caller).  `got`, `want`: dicts as source_spectra_host returns."""
    discrete = same_discrete(got, want, ("mask", "num_valid", "used"))
    largest, n = largest_averaged(want["corrected"], want["snr"], want["used"], option, C)
    a_avg, a_std = average_allowance(want, n[:, None], option[0], largest)
    return discrete, worst_ratio(got["average"], want["average"], a_avg), worst_ratio(got["std"], want["std"], a_std)


def mw_allowance(want, n_bands):
    """Allowances of stage 4, given the same corrected spectra and SNR on both sides.  measurement_snr and the
    weights are sums, products and quotients of equal inputs in a stated order, each correctly rounded on both sides:
    they must be EQUAL.  measured_disp: a value of the input itself, or their half-sum (equal), or
    10 ** (sum(w log10 p) / sum(w)): relative ln(10) (n_bands + 2 ULP_LOG10 + 4) 2 U max(1, |log10|) + pow's ulp on
    both sides + CORRECTED_ULP (stage 4 may run on the device's own corrected spectra).  log10_M0: that error through log10, a log10 on both sides, n adds and a division."""
    with np.errstate(all="ignore"):
        lg = np.abs(np.log10(want["measured_disp"]))
    lg = np.where(np.isfinite(lg), lg, 0.0)
    relative = (LN10 * (n_bands + 2 * ULP_LOG10 + 4) * 2 * U * np.maximum(lg, 1.0) + (ULP_POW + 1) * 2 * U
                + CORRECTED_ULP * 2 * U)
    n = want["weights"].shape[1]
    m0 = relative.max(axis=1) / LN10 + (lg.max(axis=1) + 1.0) * (n + 2 * ULP_LOG10 + 4) * 2 * U
    return np.abs(want["measured_disp"]) * relative, m0


def check_mw(got, want, n_bands):
    """(weights, measurement_snr and the NaN patterns equal; worst ratios of measured_disp, log10_M0, Mw_star)."""
    discrete = (np.array_equal(got["weights"], want["weights"])
                and np.array_equal(got["measurement_snr"], want["measurement_snr"])
                and np.array_equal(np.isnan(got["measured_disp"]), np.isnan(want["measured_disp"]))
                and np.array_equal(np.isnan(got["Mw_star"]), np.isnan(want["Mw_star"])))
    measured, m0 = mw_allowance(want, n_bands)
    return (discrete, worst_ratio(got["measured_disp"], want["measured_disp"], measured),
            worst_ratio(got["log10_M0"], want["log10_M0"], m0),
            worst_ratio(got["Mw_star"], want["Mw_star"], SCALING * m0 + 4 * U * np.abs(want["Mw_star"])))
