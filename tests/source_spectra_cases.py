"""Inputs, options and the comparison's own checks for the propagation corrections, network-average spectra and the
approximate moment magnitude (postprocess.source_spectra_host, network_average_spectrum_host,
approximate_moment_magnitude_host; csrc/source_spectra.hip).  Everything is regenerated from seeds; only the
reference's recorded answers live in tests/golden/source_spectra.npz (tests/golden/make_source_spectra_golden.py).

An event's spectra are a Brune plateau times a lognormal factor; the noise is the signal divided by a ratio, so that
the SNR is that ratio: powers of two (exact quotients: 1, 4, THRESHOLD itself, 16, 32 -- so `<`, `>` and `>=` at the
threshold are all exercised) or a continuous value kept 1 % away from THRESHOLD.  Events cycle through the numbers
of stations that hold a band above the threshold (0, 1, 5, 6, 7, all: the max_num_bad_measurements edge), through 1 .. 4
such bands per station, and through location errors that drop none, some and all stations.

Case `tables` adds zero and non-finite table entries for stages 1-3.  The STAGE4_CASES are built directly as corrected
spectra, SNR and epicentral distances (stage4_inputs): 0 .. 10 valid bands per channel, tied / zero / non-finite
distances at S = 2, 3, 4, 5, 9, and tied non-zero measurement SNRs across the weight cut-off.  The same module holds
the pointer order of the C entry point (c_call), used by the stage-subset, ulp and guard-band tests."""
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
    "tables": (21, 8, 6, 0, 9, ("tables",)),
    "guard_15x65": (22, 3, 5, 3, 65, ("zeros", "absent")),       # tests/guard_cases.py: nothing a multiple of 64
    "guard_129x3": (23, 2, 43, 3, 3, ("absent",)),              # 129 channels: 129 x 64 x 8 bytes of LDS for the median
}
RECORDED = ("small", "edge", "components", "one_station", "two_stations")      # in the golden file
GUARD_CASES = ("guard_15x65", "guard_129x3")
GPU_CASES = tuple(n for n in CASES if n != "tables" and n not in GUARD_CASES)
STAGES_1_TO_3_CASES = GPU_CASES + ("tables",)           # `tables`: non-finite and zero table entries, stages 1-3 only

# (average_log, reduce, min_num_valid_channels_per_freq_bin, max_relative_distance_err_pct)
AVERAGE_OPTIONS = [(True, "mean", 0, 25.0), (True, "median", 0, 25.0), (False, "mean", 0, 25.0),
                   (False, "median", 0, 25.0), (True, "mean", 3, 25.0), (True, "median", 3, 1e9),
                   (False, "mean", 10 ** 6, 25.0), (True, "mean", 0, 0.0)]
# (num_averaging_bands, low_snr_freq_min_hz)
MW_OPTIONS = [(1, 2.0), (2, 2.0), (3, 0.0), (1, 1e9), (4, 2.0), (5, 2.0), (6, 0.0), (7, 2.0), (8, 2.0)]


def average_kwargs(option):
    return dict(snr_threshold=THRESHOLD, average_log=option[0], reduce=option[1],
                min_num_valid_channels_per_freq_bin=option[2], max_relative_distance_err_pct=option[3])


def mw_kwargs(option, max_bad=MAX_BAD):
    return dict(snr_threshold=THRESHOLD, num_averaging_bands=option[0], low_snr_freq_min_hz=option[1],
                magnitude_log_moment_scaling=SCALING, weight_max=WEIGHT_MAX, max_num_bad_measurements=max_bad)


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
    tt_p = dist / 6.0 + rng.uniform(0.0, 0.2, size=(E, S))
    tt_s = dist / 3.5 + rng.uniform(0.0, 0.3, size=(E, S))
    if "tables" in special:                              # one event each; events 0, 3, 6 keep every station
        dist[0, 2] = 0.0                                 # error percentage inf: the station is not used
        hmax[1] = np.nan                                 # location_err NaN: not (NaN > max), every station used
        hmax[2], vmax[2], dist[2, 1] = 0.0, 0.0, 0.0     # 0 / 0: NaN again, and a geometrical factor of 0
        tt_p[3, 4], tt_s[3, 4] = np.inf, np.inf          # an attenuation factor of inf
        signal[4, 0], signal[4, 3, ::2] = -signal[4, 0], -signal[4, 3, ::2]      # negative values: |x| in the SNR only
        ratio[6, :, :3] = 1.0                            # bins 0, 1, 2 of event 6: num_valid 2, 3, 4 (min_num = 3)
        for b, n in enumerate((2, 3, 4)):
            ratio[6, :n, b] = 16.0
        noise = signal / ratio
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
               epi=epi, tt_p=tt_p, tt_s=tt_s, hmax=hmax, vmax=vmax,
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


# ---- bpmf_source_spectra_dev through the C ABI: the pointers in the header's order, and what each stage touches ----
POINTER_INPUTS = ("signal", "noise", "valid", "noise_valid", "dist", "epi", "tt", "location_err", "frequencies", "q")
POINTER_OUTPUTS = ("corrected", "snr", "average", "mask", "std", "num_valid", "used", "Mw_star", "log10_M0",
                   "measured_disp", "weights", "measurement_snr")
# bit: (what the stage reads, what it writes); `corrected` and `snr` are read by stages 4 and 8
STAGE_READS_WRITES = {1: (("signal", "noise", "valid", "noise_valid"), ("snr",)),
                      2: (("signal", "valid", "dist", "tt", "frequencies", "q"), ("corrected",)),
                      4: (("valid", "dist", "location_err", "corrected", "snr"),
                          ("average", "mask", "std", "num_valid", "used")),
                      8: (("valid", "epi", "corrected", "snr"),
                          ("Mw_star", "log10_M0", "measured_disp", "weights", "measurement_snr"))}


def output_specs(E, S, C, F):
    """{output: (shape, dtype)} of bpmf_source_spectra_dev (include/bpmf_hip.h)."""
    NC = S * C
    return {"corrected": ((E, NC, F), np.float64), "snr": ((E, NC, F), np.float64), "average": ((E, F), np.float64),
            "mask": ((E, F), np.uint8), "std": ((E, F), np.float64), "num_valid": ((E, F), np.int32),
            "used": ((E, S), np.uint8), "Mw_star": ((E,), np.float64), "log10_M0": ((E,), np.float64),
            "measured_disp": ((E, NC), np.float64), "weights": ((E, NC), np.float32),
            "measurement_snr": ((E, NC), np.float32)}


def touched(flags):
    """(pointers that the stages of `flags` read or write, outputs that they write)."""
    used, written = set(), set()
    for bit, (reads, writes) in STAGE_READS_WRITES.items():
        if flags & bit:
            used |= set(reads) | set(writes)
            written |= set(writes)
    return used, written


def c_call(lib, p, E, S, C, F, flags, stream=None, *, geometry_constant=0.0, radiation=1.0, snr_threshold=THRESHOLD,
           max_err_pct=25.0, min_num_valid=0, average_log=1, median=0, bands=1, first_high=0, scaling=SCALING,
           weight_max=WEIGHT_MAX, max_bad=MAX_BAD):
    """bpmf_source_spectra_dev with the pointers of the dict `p` (a missing name is passed as null)."""
    return lib.bpmf_source_spectra_dev(*[p.get(k) for k in POINTER_INPUTS], E, S, C, F, flags, geometry_constant,
                                       radiation, snr_threshold, max_err_pct, min_num_valid, average_log, median,
                                       bands, first_high, scaling, weight_max, max_bad, stream,
                                       *[p.get(k) for k in POINTER_OUTPUTS])


def c_inputs(name, phase):
    """({pointer name: contiguous array}, parameters of c_call) of stages 1-3 of a case, as the Python surface passes
    them."""
    x, a = inputs(name), phase_arguments(name, phase)
    arrays = {"signal": a["signal"], "noise": x["noise"], "valid": x["present"].astype(np.uint8),
              "noise_valid": x["noise_present"].astype(np.uint8), "dist": x["dist"], "epi": x["epi"], "tt": a["tt_sec"],
              "location_err": x["location_err"], "frequencies": x["frequencies"], "q": a["q_row"]}
    return ({k: np.ascontiguousarray(v) for k, v in arrays.items()},
            dict(geometry_constant=float(a["geometry_constant"]), radiation=float(a["radiation"])))


# ---- the arguments at which the device's exp, log10 and pow are measured (tests/test_gpu_source_spectra_ulp.py) ----
ULP_N = 4096
ULP_NEIGHBOURS = 2        # the fixture holds 10 ** y for the correctly rounded log10 and this many neighbours each side


def ulp_arguments():
    """(tt, x), ULP_N each: travel times with pi tt in 0 .. 60 (what exp receives with f = q = 1), and x in
    1e-13 .. 1e3 with the powers of ten, their neighbours and the neighbours of 1 among them."""
    rng = np.random.default_rng(77)
    tt = rng.uniform(0.0, 60.0 / np.pi, ULP_N)
    tt[:8] = [0.0, 2.0 ** -60, 1.0 / np.pi, 1.0, np.log(2.0) / np.pi, 10.0, 19.0, 60.0 / np.pi]
    x = 10.0 ** rng.uniform(-13.0, 3.0, ULP_N)
    powers = np.array([float(f"1e{k}") for k in range(-13, 4)])
    x[:17] = powers
    near_one = [1.0]
    for step in range(1, 9):
        near_one += [1.0 + step * 2.0 ** -52, 1.0 - step * 2.0 ** -53]
    x[17:17 + len(near_one)] = near_one
    x[40:57] = np.nextafter(powers, 0.0)
    x[57:74] = np.nextafter(powers, np.inf)
    return tt, x


def stepped(v, k):
    """v moved by k float64 neighbours (k < 0: down)."""
    v = np.array(v, dtype=np.float64)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def ulps_from(got, correctly_rounded):
    """|got - cr| in units of the spacing of cr (measured at cr, towards got)."""
    got, cr = np.asarray(got, dtype=np.float64), np.asarray(correctly_rounded, dtype=np.float64)
    with np.errstate(all="ignore"):
        step = np.abs(np.nextafter(cr, got) - cr)
        return np.where(got == cr, 0.0, np.abs(got - cr) / step)


# ---- stage-4 cases built directly: corrected spectra, SNR, epicentral distances ----
# name: (seed, E, S, C (0: (E, S, F) spectra), F).  What the real reference confirms (tests/golden/source_spectra.npz):
#   bands                 every event and option (the reference's np.median and np.percentile);
#   distances_S2 .. S9    every event but those with a NaN distance (event 6: np.percentile's NaN is confirmed, but the
#                         all-NaN weights that follow are compared as NaN patterns) -- recorded as they come;
#   snr_ties_*            NOT recorded: the reference's np.argsort (quicksort) leaves the order of equal SNRs open, and
#                         from 17 values on does not keep index order; the rule "ties by index" of
#                         postprocess.snr_based_weights_host and include/bpmf_hip.h stands alone there.
STAGE4_CASES = {
    "bands": (31, 12, 7, 0, 20),
    "distances_S2": (32, 12, 2, 0, 6),
    "distances_S3": (33, 12, 3, 0, 6),
    "distances_S4": (34, 12, 4, 0, 6),
    "distances_S5": (35, 12, 5, 0, 6),
    "distances_S9": (36, 12, 9, 0, 6),
    "snr_ties_S9": (37, 4, 9, 0, 8),
    "snr_ties_S20": (38, 4, 20, 0, 8),
    "snr_ties_S20_C2": (39, 4, 20, 2, 8),
}
STAGE4_RECORDED = ("bands", "distances_S2", "distances_S3", "distances_S4", "distances_S5", "distances_S9")
BANDS_MAX = 10                       # channels of `bands` cycle through 0 .. 10 bands above THRESHOLD
# the events of a distances case, in order
DISTANCE_EVENTS = ("distinct", "all_equal", "tie_on_the_interpolated_ranks", "tie_elsewhere", "ascending", "descending",
                   "nan", "inf", "zero", "minus_zero", "extremes_not_valid", "smallest_not_valid")


def TIES_MAX_BAD(n_channels):
    """The max_num_bad_measurements that an snr_ties case with n_channels present channels is run with."""
    return (0, 1, 6, n_channels - 1, n_channels, n_channels + 1)


def _spectra(rng, E, NC, F, n_valid):
    """(corrected, snr) (E, NC, F): lognormal values that are not monotone in frequency; n_valid[e, ch] bands above
    THRESHOLD scattered over the axis, the others below it or on it."""
    corrected = 10.0 ** rng.uniform(-9.0, -6.0, size=(E, NC, 1)) * np.exp(rng.normal(0.0, 0.6, size=(E, NC, F)))
    exact = np.array([1.0, 4.0, THRESHOLD, 0.5])
    snr = np.where(rng.random((E, NC, F)) < 0.3, exact[rng.integers(0, 4, size=(E, NC, F))],
                   rng.uniform(0.3, 0.99 * THRESHOLD, size=(E, NC, F)))
    for e in range(E):
        for ch in range(NC):
            bands = rng.permutation(F)[:n_valid[e, ch]]
            snr[e, ch, bands] = np.where(rng.random(len(bands)) < 0.5,
                                         np.array([16.0, 32.0])[rng.integers(0, 2, len(bands))],
                                         rng.uniform(1.01 * THRESHOLD, 50.0, len(bands)))
    return corrected, snr


def percentile_ranks(S):
    """[(lo, hi, t)] for q = 0.25, 0.75: the two ranks np.percentile (linear) interpolates between, and the fraction."""
    out = []
    for q in (0.25, 0.75):
        vi = q * (S - 1)
        lo = int(np.floor(vi))
        out.append((lo, min(lo + 1, S - 1), vi - lo))
    return out


def stage4_inputs(name):
    """A stage-4 case as a dict of read-only arrays: corrected, snr ((E, S, F) or (E, S, C, F)), present (E, S),
    frequencies (F,), epi (E, S); computed once."""
    if name in _cache:
        return _cache[name]
    seed, E, S, C, F = STAGE4_CASES[name]
    rng = np.random.default_rng(seed)
    Cc = max(C, 1)
    NC = S * Cc
    f = np.logspace(np.log10(0.5), np.log10(20.0), F)
    present = np.ones((E, S), dtype=bool)
    epi = rng.uniform(5.0, 60.0, size=(E, S))
    if name == "bands":
        n_valid = (np.arange(E * NC) % (BANDS_MAX + 1)).reshape(E, NC)
        corrected, snr = _spectra(rng, E, NC, F, n_valid)
        valid = [[np.flatnonzero(snr[e, ch] > THRESHOLD) for ch in range(NC)] for e in range(E)]
        for ch in range(NC):                             # event 8: two equal chosen values (k = 1 .. 7)
            if len(valid[8][ch]) >= 2:
                corrected[8, ch, valid[8][ch][1]] = corrected[8, ch, valid[8][ch][0]]
        for ch in (0, 5):                                # event 9: a NaN among the chosen bands (k = 8 and k = 2)
            corrected[9, ch, valid[9][ch][0]] = np.nan
        for ch in range(NC):                             # event 10: a NaN in the ninth valid band, beyond any nab
            if len(valid[10][ch]) > 8:
                corrected[10, ch, valid[10][ch][8]] = np.nan
        for ch in (1, 3):                                # event 11: a chosen value of +inf (k = 1 and k = 3)
            corrected[11, ch, valid[11][ch][0]] = np.inf
        present[1, 2] = False
    elif name.startswith("distances"):
        corrected, snr = _spectra(rng, E, NC, F, (np.arange(E * NC) % 4).reshape(E, NC))
        (lo, hi, _), (lo75, hi75, _) = percentile_ranks(S)
        for e, kind in enumerate(DISTANCE_EVENTS):
            ordered = np.sort(epi[e])
            if kind == "all_equal":
                ordered[:] = ordered[0]
            elif kind == "tie_on_the_interpolated_ranks":
                ordered[hi] = ordered[lo]
            elif kind == "tie_elsewhere":
                free = [r for r in range(S - 1) if not {r, r + 1} & {lo, hi, lo75, hi75}]
                r = free[-1] if free else S - 2
                ordered[r + 1] = ordered[r]
            if kind == "ascending":
                epi[e] = ordered
            elif kind == "descending":
                epi[e] = ordered[::-1]
            else:
                epi[e] = ordered[rng.permutation(S)]
            if kind == "nan":
                epi[e, rng.integers(S)] = np.nan
            elif kind == "inf":
                epi[e, rng.integers(S)] = np.inf
            elif kind == "zero":
                epi[e, rng.integers(S)] = 0.0
            elif kind == "minus_zero":
                epi[e, rng.integers(S)] = -0.0
            elif kind == "extremes_not_valid":
                present[e, [np.argmin(epi[e]), np.argmax(epi[e])]] = False
            elif kind == "smallest_not_valid":           # (at S = 3 the extremes leave one station: its own percentiles)
                present[e, np.argmin(epi[e])] = False
    else:
        # snr_ties: no channel has a valid band, so the float32 measurement SNR of a channel is sum(r r) / sum(r) of
        # its row, below THRESHOLD and not 0.  Rows are copied so that, by rank among the n channels of the event,
        # ranks 0-1, ranks n-7 .. n-5 and ranks n-2 .. n-1 are tied groups: the cuts `rank < n - max_bad` of
        # max_bad = n - 1, 6 and 1 fall inside them.  The copies are scattered over the channel indices.
        corrected, snr = _spectra(rng, E, NC, F, np.zeros((E, NC), dtype=int))
        snr = np.where(snr == THRESHOLD, 2.0, snr)
        if E > 1:
            present[1, S // 2] = False                   # n = (S - 1) C channels in event 1
        high = f > 2.0
        for e in range(E):
            ch = np.flatnonzero(np.repeat(present[e], Cc))
            n = len(ch)
            proxy = (snr[e, ch][:, high] ** 2).sum(axis=1) / snr[e, ch][:, high].sum(axis=1)
            by_rank = ch[np.argsort(proxy)]              # the rows in ascending order of their measurement SNR
            rows_x, rows_r = corrected[e, by_rank].copy(), snr[e, by_rank].copy()
            for group in ((0, 1), (n - 7, n - 6, n - 5), (n - 2, n - 1)):
                for r in group[1:]:
                    rows_x[r], rows_r[r] = rows_x[group[0]], rows_r[group[0]]
            scatter = ch[rng.permutation(n)]
            corrected[e, scatter], snr[e, scatter] = rows_x, rows_r
    shape = (E, S, F) if C == 0 else (E, S, C, F)
    out = dict(corrected=corrected.reshape(shape), snr=snr.reshape(shape), present=present, frequencies=f, epi=epi)
    for a in out.values():
        a.setflags(write=False)
    _cache[name] = out
    return out


def stage4_runs(name):
    """[(index into MW_OPTIONS, max_num_bad_measurements)]: the calls of stage 4 that a stage-4 case is run with."""
    if name.startswith("snr_ties"):
        seed, E, S, C, F = STAGE4_CASES[name]
        return [(0, b) for b in TIES_MAX_BAD(S * max(C, 1))] + [(0, b) for b in TIES_MAX_BAD((S - 1) * max(C, 1))[3:]]
    return [(o, MAX_BAD) for o in range(len(MW_OPTIONS))]


# ---- the comparison's own checks: what the GPU tests apply to the device, and the host test to planted defects ----
U = 2.0 ** -53
LN10 = float(np.log(10.0))
# Allowances per call of a device function against the correctly rounded value, in ulp (2 U relative): the figures of
# HIP's published math-API table for double (exp, log10: 1 ulp; pow: 1 ulp, taken as 2; sqrt and division: correctly
# rounded, taken as 1).  MEASURED on an MI355X at 4096 arguments each, through the entry point, against mpmath
# (tests/test_gpu_source_spectra_ulp.py, which asserts these constants): exp 1, log10 1, pow 1 ulp at the worst.  The
# host's own functions are allowed 1 ulp each.
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
    with np.errstate(invalid="ignore"):
        return _average_allowance(want, n, average_log, largest)


def _average_allowance(want, n, average_log, largest):
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
    """max |got - want| / allow over the elements where want is finite; inf where NaN / inf patterns differ.  Where
    the allowance itself is NaN or inf (it was computed from inputs that are not finite) the element must be EQUAL:
    a difference there gives inf, never "anything goes" (inf) and never "always fails" (NaN)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    finite = np.isfinite(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(got[~finite & ~np.isnan(want)],
                                                                                want[~finite & ~np.isnan(want)]):
        return np.inf
    if not finite.any():
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got[finite] - want[finite])
        a = np.broadcast_to(allow, want.shape)[finite]
        ratio = np.where(err == 0.0, 0.0, np.where(np.isfinite(a), err / np.maximum(a, 1e-320), np.inf))
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
    """(weights, measurement_snr and the NaN patterns equal; worst ratios of measured_disp, log10_M0, Mw_star).  A
    percentile that is NaN (a NaN distance) makes every weight of the event NaN: there the NaN pattern must be the
    same, and every other element equal as before."""
    discrete = (np.array_equal(got["weights"], want["weights"], equal_nan=True)
                and np.array_equal(got["measurement_snr"], want["measurement_snr"], equal_nan=True)
                and np.array_equal(np.isnan(got["measured_disp"]), np.isnan(want["measured_disp"]))
                and np.array_equal(np.isnan(got["Mw_star"]), np.isnan(want["Mw_star"])))
    measured, m0 = mw_allowance(want, n_bands)
    return (discrete, worst_ratio(got["measured_disp"], want["measured_disp"], measured),
            worst_ratio(got["log10_M0"], want["log10_M0"], m0),
            worst_ratio(got["Mw_star"], want["Mw_star"], SCALING * m0 + 4 * U * np.abs(want["Mw_star"])))
