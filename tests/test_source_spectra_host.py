"""CPU: the host definitions of the propagation corrections, the network-average spectrum and the approximate moment
magnitude (postprocess.propagation_factors_host, source_spectra_host, network_average_spectrum_host,
approximate_moment_magnitude_host) against what the REAL reference recorded (tests/golden/source_spectra.npz, written by
tests/golden/make_source_spectra_golden.py with NumPy and pandas of the versions named in the file).

Every float is demanded bit for bit: the definitions restate the same NumPy calls in the same order.  (Measured worst
relative difference: 0 -- nothing needed the 4 x allowance the plan provided for.)

The cases built directly for stage 4 (4 to 8 averaging bands, tied and non-finite distances, tied SNRs) and case
`tables` come with assertions, on the definition, that each reaches what it is there for: without them the device
comparison could pass vacuously.

Then: the input conditions under which the GPU tests may demand equal discrete outputs for every event; the planted
defects, each of which must fail the GPU comparison's own check (source_spectra_cases.check_average, corrected_ok,
check_mw); and the refusals of the Python and C surfaces that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_spectra_cases as sc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "source_spectra.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def chain(name, phase, o=0, attenuation="reference"):
    return pp.source_spectra_host(**sc.phase_arguments(name, phase, attenuation),
                                  **sc.average_kwargs(sc.AVERAGE_OPTIONS[o]))


def magnitude(name, phase, o, **kw):
    x, c = sc.inputs(name), chain(name, phase)
    return pp.approximate_moment_magnitude_host(c["corrected"], c["snr"], x["present"], x["frequencies"], x["epi"],
                                                **{**sc.mw_kwargs(sc.MW_OPTIONS[o]), **kw})


# ---- the definitions against the recorded answers ----
def test_golden_file_names_its_versions(golden):
    assert str(golden["numpy_version"]) and str(golden["pandas_version"])
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", sc.RECORDED)
def test_propagation_factors_equal_the_reference(golden, name):
    x = sc.inputs(name)
    for attenuation, key in (("reference", "att_reference"), ("physical", "att_physical")):
        geometry, att = pp.propagation_factors_host(x["frequencies"], x["dist"], x["tt_p"], x["tt_s"], sc.MEDIUM,
                                                    sc.PREFACTOR, attenuation)
        assert geometry.shape == x["dist"].shape + (2,) and att.shape == x["dist"].shape + (2, len(x["frequencies"]))
        for k, phase in enumerate(sc.PHASES):
            assert same(geometry[..., k], golden[f"geometry_{name}_{phase}"])
            assert same(att[:, :, k], golden[f"{key}_{name}_{phase}"])
    # the reference's pairing: both phases with the S travel time, P with Q_s and S with Q_p
    which, q = pp.attenuation_plan(x["frequencies"], sc.MEDIUM, sc.PREFACTOR, "reference")
    Q = sc.MEDIUM["Q_1HZ"] * np.power(x["frequencies"], sc.MEDIUM["attenuation_n"])
    assert which == ("s", "s") and same(q[0], Q * sc.PREFACTOR["s"]) and same(q[1], Q * sc.PREFACTOR["p"])
    assert pp.attenuation_plan(x["frequencies"], sc.MEDIUM, sc.PREFACTOR, "physical")[0] == ("p", "s")


@pytest.mark.parametrize("name", sc.RECORDED)
def test_snr_corrections_and_averages_equal_the_reference(golden, name):
    C = max(sc.CASES[name][3], 1)
    for phase in sc.PHASES:
        k = f"{name}_{phase}"
        for o in range(len(sc.AVERAGE_OPTIONS)):
            got = chain(name, phase, o)
            assert same(got["snr"], golden[f"snr_{k}"]) and same(got["corrected"], golden[f"corrected_{k}"])
            assert same(got["average"], golden[f"avg_{k}_{o}"]), (k, o)
            assert same(got["std"], golden[f"std_{k}_{o}"]), (k, o)
            assert same(got["mask"], golden[f"mask_{k}_{o}"]) and got["mask"].dtype == bool
            assert same(got["num_valid"], golden[f"nvalid_{k}_{o}"]) and got["num_valid"].dtype == np.int32
            assert same(got["used"].sum(axis=1) * C, golden[f"nused_{k}_{o}"])
            assert not got["mask"][~got["used"].any(axis=1)].size or got["mask"][~got["used"].any(axis=1)].all()


def test_the_recorded_cases_hold_what_the_issue_lists(golden):
    edge = {o: chain("edge", "p", o) for o in range(len(sc.AVERAGE_OPTIONS))}
    x = sc.inputs("edge")
    assert edge[6]["mask"].all() and edge[7]["mask"].all()                       # min_num above S * C; every station cut
    assert edge[5]["used"].sum() > edge[0]["used"].sum() > edge[7]["used"].sum() == 0      # none, some, all dropped
    assert (edge[0]["snr"] == sc.THRESHOLD).any() and np.isnan(edge[0]["snr"]).any() and np.isinf(edge[0]["snr"]).any()
    assert (edge[0]["corrected"][x["present"]] == 0).any() and not x["noise_present"].all() and not x["present"].all()
    assert (np.isnan(edge[3]["average"]) & ~edge[3]["mask"]).any()               # a median of a NaN is not masked,
    assert (edge[2]["mask"] & (edge[2]["std"] == 0)).any()                       # a NaN mean is, and its std is 0;
    assert not np.isnan(edge[1]["average"][~edge[1]["mask"]]).any()              # log10 masks NaN itself


@pytest.mark.parametrize("name", [n for n in sc.RECORDED if sc.CASES[n][3] == 0])
def test_approximate_moment_magnitude_equals_the_reference(golden, name):
    x = sc.inputs(name)
    for phase in sc.PHASES:
        k = f"{name}_{phase}"
        for o, option in enumerate(sc.MW_OPTIONS):
            got = magnitude(name, phase, o)
            ran = ~golden[f"mwraised_{k}_{o}"]
            assert same(got["Mw_star"][ran], golden[f"mw_{k}_{o}"][ran]), (k, o)
            assert same(got["measurement_snr"][ran], golden[f"msnr_{k}_{o}"][ran]), (k, o)
            assert same((got["weights"] > 0)[ran], (golden[f"rawweights_{k}_{o}"] > 0)[ran]), (k, o)
            assert same(got["log10_M0"], got["Mw_star"] / sc.SCALING + 9.1) or np.allclose(
                got["log10_M0"], got["Mw_star"] / sc.SCALING + 9.1, rtol=1e-14, equal_nan=True)
            assert got["weights"].dtype == np.float32 and got["measurement_snr"].dtype == np.float32
            # the reference raises for an event without a spectrum, and (its unused argmax) for an empty selection of
            # bands at a station without a valid band; the definition states 1 and 0 there
            stations = x["present"].any(axis=1)
            if option[1] < 1e8:
                assert same(ran, stations)
            else:
                assert np.isnan(got["Mw_star"][~stations]).all() and not ran[~stations].any()
                fallback = x["present"] & (got["measurement_snr"] == 0)
                assert (got["measured_disp"][fallback] == 1.0).all() and (fallback.any() or name != "edge")


def test_the_magnitude_cases_hold_what_the_issue_lists():
    counts = set()
    for name in ("edge", "batch"):
        for o in (0, 1, 2):
            got = magnitude(name, "p", o)
            good = (got["measurement_snr"] >= np.float32(sc.THRESHOLD)).sum(axis=1)
            counts |= set(good.tolist())
    assert {0, 1, 5, 6, 7} <= counts                                             # the max_num_bad_measurements edge
    snr = chain("edge", "p")["snr"]
    valid_bands = (snr > sc.THRESHOLD).sum(axis=-1)
    assert {0, 1, 2, 3, 4} <= set(valid_bands.ravel().tolist())
    assert sorted({sc.CASES[n][2] for n in sc.RECORDED})[:2] == [1, 2]           # the percentile edge cases


# ---- the input conditions of the GPU comparison ----
@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_input_conditions_of_the_gpu_cases(name):
    """Discrete outputs can be demanded equal for EVERY event: among the float32 measurement SNRs of an event, those
    below the threshold and not 0 are distinct (equal values order by index; zeros weigh 0 wherever they fall, and
    the values at the threshold are all kept, being fewer than max_num_bad_measurements where the order decides),
    and none lies within 2 float32 ulp of snr_threshold, 1.001 snr_threshold or weight_max unless it is equal."""
    x = sc.inputs(name)
    C = max(sc.CASES[name][3], 1)
    present = np.repeat(x["present"], C, axis=1)
    for phase in sc.PHASES:
        for o in range(len(sc.MW_OPTIONS)):
            msnr = magnitude(name, phase, o)["measurement_snr"]
            for e in range(len(msnr)):
                v = msnr[e][present[e]]
                low = v[(v > 0) & (v < np.float32(sc.THRESHOLD))]
                assert len(np.unique(low)) == len(low), (name, phase, o, e)
                for edge in (sc.THRESHOLD, 1.001 * sc.THRESHOLD, sc.WEIGHT_MAX):
                    edge = np.float32(edge)
                    near = np.abs(v - edge) <= 2 * np.spacing(edge)
                    assert (v[near] == edge).all(), (name, phase, o, e)
        # stages 1-3: the SNR is one correctly rounded division on both sides, so `<` decides equally
        snr = chain(name, phase)["snr"]
        assert np.array_equal(snr, pp.spectral_snr_host(sc.phase_arguments(name, phase)["signal"], x["noise"],
                                                         x["noise_present"]) * present.reshape(
            present.shape[0], -1, C).reshape(snr.shape[:-1])[..., None], equal_nan=True)


@pytest.mark.parametrize("name", [n for n in sc.STAGE4_CASES if not n.startswith("snr_ties")])
def test_input_conditions_of_the_stage_4_cases(name):
    """As above for the cases built directly (the snr_ties cases tie on purpose: there the rule "by index" is what is
    tested)."""
    x = sc.stage4_inputs(name)
    for o, max_bad in sc.stage4_runs(name):
        msnr = stage4_definition(name, o, max_bad)["measurement_snr"]
        for e in range(len(msnr)):
            v = msnr[e][x["present"][e]]
            low = v[(v > 0) & (v < np.float32(sc.THRESHOLD))]
            assert len(np.unique(low)) == len(low), (name, o, e)
            for edge in (sc.THRESHOLD, 1.001 * sc.THRESHOLD, sc.WEIGHT_MAX):
                edge = np.float32(edge)
                near = np.abs(v - edge) <= 2 * np.spacing(edge)
                assert (v[near] == edge).all(), (name, o, e)


# ---- planted defects: each must fail the GPU comparison's own check ----
def defective_average(arguments, option, defect=None):
    """source_spectra_host restated with one defect planted (None: it must equal the definition)."""
    a = dict(arguments)
    signal, present = np.asarray(a["signal"]), a["present"]
    dist, f, q = a["dist_km"], a["frequencies"], a["q_row"]
    tt = sc.inputs(defect[1])["tt_p"] if isinstance(defect, tuple) and defect[0] == "tt_p" else a["tt_sec"]
    wide = (slice(None), slice(None)) + (None,) * (signal.ndim - 2)
    average_log, reduce, min_num, max_err = option
    with np.errstate(all="ignore"):
        snr = pp.spectral_snr_host(signal, a["noise"], a["noise_present"])
        geometry = (a["geometry_constant"] * (1000.0 * dist) / a["radiation"])[wide]
        att = np.exp(np.pi * tt[..., None] * f / q)
        att = att if signal.ndim == 3 else att[:, :, None, :]
        corrected = signal * (geometry * att) if defect == "one_rounding" else signal * geometry * att
        corrected[~present], snr[~present] = 0.0, 0.0
        E, S = present.shape
        C = 1 if signal.ndim == 3 else signal.shape[2]
        F = signal.shape[-1]
        x, r = corrected.reshape(E, S * C, F), snr.reshape(E, S * C, F)
        used = present & ~(100.0 * (a["location_err_km"][:, None] / dist) > max_err)
        out = {"average": np.full((E, F), np.nan), "std": np.full((E, F), np.nan), "mask": np.ones((E, F), bool),
               "num_valid": np.zeros((E, F), np.int32), "used": used, "corrected": corrected, "snr": snr}
        for e in range(E):
            ch = np.flatnonzero(np.repeat(used[e], C))
            if not len(ch):
                continue
            v = x[e, ch]
            m = r[e, ch] <= sc.THRESHOLD if defect == "<=" else r[e, ch] < sc.THRESHOLD
            count_before = (~m).sum(axis=0)
            if defect == "count_after_domain" and average_log:
                count_before = (~(m | (v <= 0.0) | ~np.isfinite(np.log10(v)))).sum(axis=0)
            out["num_valid"][e] = count_before
            m = m | (count_before < min_num)[None, :]
            if average_log:
                m = m | (v <= 0.0) | ~np.isfinite(np.log10(v))
                v = np.log(v) if defect == "ln" else np.log10(v)
            count = (~m).sum(axis=0)
            mean = np.add.reduce(np.where(m, 0.0, v), axis=0) * 1.0 / count
            centre = mean
            if reduce == "median":
                ordered = np.sort(np.where(m, np.inf, v), axis=0)
                hi = np.minimum(count // 2, len(ch) - 1)
                lo = hi if defect == "upper_middle" else np.where(count % 2 == 1, hi, np.maximum(hi - 1, 0))
                centre = (np.take_along_axis(ordered, lo[None], 0)[0] + np.take_along_axis(ordered, hi[None], 0)[0]) / 2
                centre[(np.isnan(v) & ~m).any(axis=0)] = np.nan
            d = np.where(m, 0.0, v - mean)
            variance = np.add.reduce(d * d, axis=0) / (count - 1 if defect == "ddof" else count)
            out["mask"][e] = (count == 0) | (~np.isfinite(mean) if reduce == "mean" else False)
            out["average"][e] = np.where(out["mask"][e], np.nan, np.exp(centre * np.log(10.0)) if average_log else centre)
            out["std"][e] = np.where((count == 0) | ~np.isfinite(variance), np.nan, np.sqrt(variance))
            out["std"][e][(count > 0) & ~np.isfinite(mean)] = 0.0
    return out


def gpu_check_of_stages_1_to_3(got, want, arguments, option, C):
    """What tests/test_gpu_source_spectra.py:assert_average demands, as one bool."""
    with np.errstate(all="ignore"):
        geometry = arguments["geometry_constant"] * (1000.0 * arguments["dist_km"]) / arguments["radiation"]
        att = np.exp(np.pi * arguments["tt_sec"][..., None] * arguments["frequencies"] / arguments["q_row"])
    wide = (slice(None), slice(None)) + (None,) * (want["corrected"].ndim - 2)
    failed = sc.corrected_ok(got["corrected"], arguments["signal"], geometry[wide],
                             att if want["corrected"].ndim == 3 else att[:, :, None, :], arguments["present"])
    discrete, r_avg, r_std = sc.check_average(got, want, option, C)
    return same(got["snr"], want["snr"]) and failed == 0.0 and discrete and r_avg <= 1.0 and r_std <= 1.0


AVERAGE_DEFECTS = [("<=", 0), ("count_after_domain", 0), ("ddof", 0), ("upper_middle", 1), (("tt_p", "edge"), 0),
                   ("one_rounding", 0), ("ln", 0)]


@pytest.mark.parametrize("o", range(len(sc.AVERAGE_OPTIONS)))
def test_the_restated_definition_is_the_definition(o):
    for name in ("edge", "components", "tables"):
        arguments = sc.phase_arguments(name, "s")
        got, want = defective_average(arguments, sc.AVERAGE_OPTIONS[o]), chain(name, "s", o)
        assert all(same(got[k], want[k]) for k in want), [k for k in want if not same(got[k], want[k])]
        assert gpu_check_of_stages_1_to_3(got, want, arguments, sc.AVERAGE_OPTIONS[o], max(sc.CASES[name][3], 1))


@pytest.mark.parametrize("defect,o", AVERAGE_DEFECTS, ids=[str(d[0]) for d in AVERAGE_DEFECTS])
def test_a_planted_defect_in_stages_1_to_3_fails_the_gpu_check(defect, o):
    arguments = sc.phase_arguments("edge", "p")
    got = defective_average(arguments, sc.AVERAGE_OPTIONS[o], defect)
    assert not gpu_check_of_stages_1_to_3(got, chain("edge", "p", o), arguments, sc.AVERAGE_OPTIONS[o], 1)


SLOT_LEFT = 0.0        # what a slot of the sorted distances holds when no entry was ranked into it


def rank_sorted(v, defect=None):
    """The distances in np.sort's order as the device builds it: every entry is stored at its rank, NaN last, equal
    entries by index.  Defects: 'ties_by_value' (equal entries share a rank: one slot is written twice, another keeps
    SLOT_LEFT), 'nan_first'."""
    def before(a, b):
        if defect == "nan_first":
            return (np.isnan(a) and not np.isnan(b)) or a < b
        return (not np.isnan(a)) if np.isnan(b) else a < b
    out = np.full(len(v), SLOT_LEFT)
    for s in range(len(v)):
        rank = sum(before(v[j], v[s]) or (defect != "ties_by_value" and not before(v[s], v[j]) and j < s)
                   for j in range(len(v)))
        out[rank] = v[s]
    return out


def percentile_linear(ordered, q, defect=None):
    """np.percentile(method="linear") of sorted values: NaN if the last is NaN, else NumPy's two-sided lerp."""
    n = len(ordered)
    vi = n * q + (1.0 - q) - 1.0
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    t, a, b = vi - lo, ordered[lo], ordered[hi]
    diff = b - a
    value = b - diff * (1.0 - t) if t >= 0.5 and defect != "one_sided_lerp" else a + diff * t
    return np.nan if np.isnan(ordered[-1]) else value


def median_of_chosen(chosen, defect=None):
    ordered, n = np.sort(chosen), len(chosen)
    if n == 1:
        return chosen[0]
    if np.isnan(chosen).any():
        return np.nan
    if defect == "upper_middle_of_even" and n % 2 == 0 and n >= 4:
        return ordered[n // 2]
    return (ordered[(n - 1) // 2] + ordered[n // 2]) / 2.0


def weights_by_rank(m, thr, weight_max, max_bad, defect=None):
    """snr_based_weights_host restated: ties by index ('ties_last_index_first': the other way round)."""
    w = np.minimum(np.minimum(m, np.float32(1.001 * thr)), np.float32(weight_max))
    if (m >= np.float32(thr)).sum() >= max_bad:
        w[m < np.float32(thr)] = 0.0
        return w
    index = np.arange(len(m))
    order = np.lexsort((-index if defect == "ties_last_index_first" else index, m))
    w[order[:max(len(m) - max_bad, 0)]] = 0.0
    return w


def restated_magnitude(corrected, snr, present, f, epi, kw, defect=None):
    """approximate_moment_magnitude_host restated, its sorts, percentiles, medians and SNR ranks written out, with one
    defect planted (None: it must equal the definition)."""
    thr, nab, max_bad = kw["snr_threshold"], kw["num_averaging_bands"], kw["max_num_bad_measurements"]
    high = f > kw["low_snr_freq_min_hz"]
    E, S = present.shape
    F = corrected.shape[-1]
    x, r_all = np.asarray(corrected).reshape(E, -1, F), np.asarray(snr).reshape(E, -1, F)
    NC = x.shape[1]
    C = NC // S
    out = {"measured_disp": np.full((E, NC), np.nan), "measurement_snr": np.zeros((E, NC), np.float32),
           "weights": np.zeros((E, NC), np.float32), "log10_M0": np.full(E, np.nan)}
    log = np.log if defect == "ln" else np.log10
    with np.errstate(all="ignore"):
        for e in range(E):
            ch = np.flatnonzero(np.repeat(present[e], C))
            if not len(ch):
                continue
            disp = np.zeros(len(ch))
            m = np.zeros(len(ch), dtype=np.float64 if defect == "float64_snr" else np.float32)
            for j, s in enumerate(ch):
                r, v = r_all[e, s], x[e, s]
                valid = np.flatnonzero(r >= thr if defect == ">=" else r > thr)
                if len(valid):
                    pick = valid[::-1][:nab] if defect == "highest" else valid[:nab]
                    disp[j] = median_of_chosen(v[pick], defect)
                    m[j] = thr
                else:
                    total = pp._skipna_sum(r[high])
                    total = 1.0 if total == 0.0 else total
                    disp[j] = 10.0 ** (pp._skipna_sum(r[high] * np.log10(v[high])) / total)
                    m[j] = pp._skipna_sum(r[high] * r[high]) / total
            m[disp == 0.0] = 0.0
            if defect == "float64_snr":
                w = np.minimum(np.minimum(m, 1.001 * thr), sc.WEIGHT_MAX)
                if (m >= thr).sum() >= max_bad:
                    w[m < thr] = 0.0
                else:
                    w[np.argsort(m, kind="stable")[:max(len(m) - max_bad, 0)]] = 0.0
            elif defect == "strict_good":
                w = np.minimum(np.minimum(m, np.float32(1.001 * thr)), np.float32(sc.WEIGHT_MAX))
                if (m > np.float32(thr)).sum() >= max_bad:
                    w[m < np.float32(thr)] = 0.0
                else:
                    w[np.argsort(m, kind="stable")[:max(len(m) - max_bad, 0)]] = 0.0
            else:
                w = weights_by_rank(m, thr, sc.WEIGHT_MAX, max_bad, defect)
            of_valid = defect == "percentiles_of_used" or (defect == "percentiles_of_valid_at_3" and S == 3)
            ordered = rank_sorted(epi[e][present[e]] if of_valid else epi[e], defect)
            low, up = percentile_linear(ordered, 0.25, defect), percentile_linear(ordered, 0.75, defect)
            wd = np.repeat(1.0 / np.minimum(np.maximum(epi[e], low), up), C)
            w = (w * wd[ch]).astype(np.float32)
            peaks = np.zeros(len(ch))
            peaks[w > 0.0] = log(disp[w > 0.0]) * w[w > 0.0]
            out["log10_M0"][e] = peaks.sum() / w.sum()
            out["measured_disp"][e, ch], out["measurement_snr"][e, ch], out["weights"][e, ch] = disp, m, w
    out["Mw_star"] = kw["magnitude_log_moment_scaling"] * (out["log10_M0"] - 9.1)
    return out


def defective_magnitude(name, phase, o, defect):
    x, c = sc.inputs(name), chain(name, phase)
    return restated_magnitude(c["corrected"], c["snr"], x["present"], x["frequencies"], x["epi"],
                              sc.mw_kwargs(sc.MW_OPTIONS[o]), defect)


def stage4_definition(name, o, max_bad=sc.MAX_BAD):
    x = sc.stage4_inputs(name)
    return pp.approximate_moment_magnitude_host(x["corrected"], x["snr"], x["present"], x["frequencies"], x["epi"],
                                                **sc.mw_kwargs(sc.MW_OPTIONS[o], max_bad))


def stage4_restated(name, o, max_bad=sc.MAX_BAD, defect=None):
    x = sc.stage4_inputs(name)
    return restated_magnitude(x["corrected"], x["snr"], x["present"], x["frequencies"], x["epi"],
                              sc.mw_kwargs(sc.MW_OPTIONS[o], max_bad), defect)


def gpu_check_of_stage_4(got, want, n_bands):
    discrete, r_disp, r_m0, r_mw = sc.check_mw(got, want, n_bands)
    return discrete and r_disp <= 1.0 and r_m0 <= 1.0 and r_mw <= 1.0


MW_DEFECTS = ["float64_snr", "percentiles_of_used", "highest", "ln", ">=", "strict_good"]


@pytest.mark.parametrize("o", range(len(sc.MW_OPTIONS)))
def test_the_restated_magnitude_is_the_definition(o):
    got, want = defective_magnitude("edge", "s", o, None), magnitude("edge", "s", o)
    assert all(same(got[k], want[k]) for k in want), [k for k in want if not same(got[k], want[k])]
    assert gpu_check_of_stage_4(got, want, sc.CASES["edge"][4])


@pytest.mark.parametrize("defect", MW_DEFECTS)
def test_a_planted_defect_in_stage_4_fails_the_gpu_check(defect):
    name = "edge" if defect == "strict_good" else "batch"       # 9 stations: 7 at the threshold, 6 kept by the order
    got, want = defective_magnitude(name, "p", 1, defect), magnitude(name, "p", 1)
    assert not gpu_check_of_stage_4(got, want, sc.CASES[name][4])


def test_the_tables_case_reaches_what_it_is_there_for():
    x = sc.inputs("tables")
    got = {o: chain("tables", "p", o) for o in range(len(sc.AVERAGE_OPTIONS))}
    with np.errstate(all="ignore"):
        pct = 100.0 * (x["location_err"][:, None] / x["dist"])
    assert np.isposinf(pct[0, 2]) and not got[0]["used"][0, 2] and not got[5]["used"][0, 2] and got[0]["used"][0].sum() == 5
    assert np.isnan(pct[1]).all() and got[0]["used"][1].all() and got[7]["used"][1].all()      # not (NaN > max)
    assert np.isnan(pct[2, 1]) and (np.delete(pct[2], 1) == 0).all() and got[7]["used"][2].all()
    assert (got[0]["corrected"][2, 1] == 0).all()                                # a geometrical factor of 0
    assert np.isposinf(got[0]["corrected"][3, 4]).all()                          # an attenuation factor of inf
    assert (got[2]["mask"][3] & (got[2]["std"][3] == 0)).any()                   # an infinite mean: masked, std 0
    negative = got[0]["corrected"][4] < 0
    assert negative[0].all() and negative[3, ::2].all() and (got[0]["snr"][4][negative] > 0).all()
    assert not same(got[0]["average"][4], got[2]["average"][4])                  # average_log masks them, the mean takes them
    for o in (4, 5):                                                             # min_num_valid 3 on num_valid 2, 3, 4
        assert got[o]["num_valid"][6, :3].tolist() == [2, 3, 4] and got[o]["mask"][6, :3].tolist() == [True, False, False]
    assert not got[0]["mask"][6, :3].any()


# ---- the stage-4 cases: recorded answers, what they reach, the restated definition, planted defects ----
def finite_distance_events(name):
    return np.isfinite(sc.stage4_inputs(name)["epi"]).all(axis=1)


@pytest.mark.parametrize("name", sc.STAGE4_RECORDED)
def test_stage_4_cases_equal_the_reference(golden, name):
    """Bit for bit, for every event whose distances are finite.  With a NaN or inf distance a percentile is NaN, and
    the definition (np.clip on arrays: NaN everywhere) stands alone: the reference clips a pandas Series, which takes
    a NaN bound as no bound."""
    x = sc.stage4_inputs(name)
    finite = finite_distance_events(name)
    assert finite.sum() >= len(finite) - 2
    for o in range(len(sc.MW_OPTIONS)):
        got = stage4_definition(name, o)
        ran = ~golden[f"mwraised_{name}_{o}"] & finite
        if sc.MW_OPTIONS[o][1] < 1e8:          # (an empty selection of bands: the reference's unused argmax raises)
            assert ran[x["present"].any(axis=1) & finite].all()
        assert same(got["Mw_star"][ran], golden[f"mw_{name}_{o}"][ran]), (name, o)
        assert same(got["measurement_snr"][ran], golden[f"msnr_{name}_{o}"][ran]), (name, o)
        assert same((got["weights"] > 0)[ran], (golden[f"rawweights_{name}_{o}"] > 0)[ran]), (name, o)


def test_the_bands_case_reaches_every_count_of_averaging_bands():
    """For every num_averaging_bands 1 .. 8: channels with more valid bands, with as many, and (from 3 on: there is no
    whole number between 1 and 2) with fewer but more than one; and an answer that differs from that of one band
    fewer.  The chosen bands are not a contiguous block and their values not sorted."""
    x = sc.stage4_inputs("bands")
    k = (x["snr"] > sc.THRESHOLD).sum(axis=-1)[x["present"]]
    assert set(k.tolist()) == set(range(sc.BANDS_MAX + 1))
    by_nab = {option[0]: stage4_definition("bands", o) for o, option in enumerate(sc.MW_OPTIONS) if option[1] < 1e8}
    assert sorted(by_nab) == list(range(1, 9))
    for nab in range(1, 9):
        assert (k > nab).any() and (k == nab).any() and (nab < 3 or ((k > 1) & (k < nab)).any())
        if nab > 1:
            a, b = by_nab[nab]["measured_disp"], by_nab[nab - 1]["measured_disp"]
            assert not same(a, b), nab
            assert not same(by_nab[nab]["Mw_star"], by_nab[nab - 1]["Mw_star"]), nab
    scattered = unsorted = 0
    for e, s in zip(*np.nonzero(x["present"])):
        valid = np.flatnonzero(x["snr"][e, s] > sc.THRESHOLD)[:8]
        scattered += len(valid) > 1 and (np.diff(valid) > 1).any()
        unsorted += len(valid) > 2 and (np.diff(x["corrected"][e, s, valid]) < 0).any()
    assert scattered > 20 and unsorted > 20
    # the four events with a property of their own
    first = [np.flatnonzero(x["snr"][8, s] > sc.THRESHOLD)[:2] for s in range(1, 7)]
    assert all(x["corrected"][8, s + 1, v[0]] == x["corrected"][8, s + 1, v[1]] for s, v in enumerate(first))
    for nab in range(1, 9):
        assert np.isnan(by_nab[nab]["measured_disp"][9, [0, 5]]).all() and np.isnan(by_nab[nab]["Mw_star"][9])
        assert np.isnan(x["corrected"][10]).any() and not np.isnan(by_nab[nab]["measured_disp"][10]).any()
        assert np.isfinite(by_nab[nab]["Mw_star"][10])
        assert np.isposinf(by_nab[nab]["measured_disp"][11, 1])
    # k = 3: +inf is the value, then half of a half-sum, then the last of three, not their median
    assert np.isposinf(by_nab[1]["measured_disp"][11, 3]) and np.isposinf(by_nab[2]["measured_disp"][11, 3])
    assert np.isfinite(by_nab[3]["measured_disp"][11, 3])


def test_the_distance_cases_reach_both_lerp_branches_every_fraction_and_a_nan():
    fractions = set()
    for name in sc.STAGE4_CASES:
        if not name.startswith("distances"):
            continue
        x = sc.stage4_inputs(name)
        S = x["epi"].shape[1]
        fractions |= {t for _, _, t in sc.percentile_ranks(S)}
        events = dict(zip(sc.DISTANCE_EVENTS, range(len(sc.DISTANCE_EVENTS))))
        epi = x["epi"]
        with np.errstate(all="ignore"):
            assert np.isnan(np.percentile(epi[events["nan"]], 25.0))
        assert len(set(epi[events["distinct"]].tolist())) == S and len(set(epi[events["all_equal"]].tolist())) == 1
        (lo, hi, _), _ = sc.percentile_ranks(S)
        tied = np.sort(epi[events["tie_on_the_interpolated_ranks"]])
        assert tied[lo] == tied[hi]
        assert len(set(epi[events["tie_elsewhere"]].tolist())) == S - 1
        assert (np.diff(epi[events["ascending"]]) > 0).all() and (np.diff(epi[events["descending"]]) < 0).all()
        assert np.isposinf(epi[events["inf"]]).sum() == 1
        assert (epi[events["zero"]] == 0).sum() == 1 and not np.signbit(epi[events["zero"]]).any()
        assert (epi[events["minus_zero"]] == 0).sum() == 1 and np.signbit(epi[events["minus_zero"]]).sum() == 1
        e = events["extremes_not_valid"]
        assert not x["present"][e, np.argmin(epi[e])] and not x["present"][e, np.argmax(epi[e])]
    assert fractions == {0.0, 0.25, 0.5, 0.75}                    # t < 0.5 and t >= 0.5: both sides of the lerp


def straddled(result, present_channels):
    """Events in which channels of one non-zero measurement SNR got both a zero and a positive weight."""
    events = 0
    for e in range(len(result["weights"])):
        m, w = result["measurement_snr"][e][present_channels[e]], result["weights"][e][present_channels[e]]
        events += any((w[m == v] == 0).any() and (w[m == v] > 0).any() for v in np.unique(m[m > 0]))
    return events


@pytest.mark.parametrize("name", [n for n in sc.STAGE4_CASES if n.startswith("snr_ties")])
def test_a_tied_group_straddles_the_cut_for_each_max_bad(name):
    """The cut `rank < n - max_bad` applies only when fewer than max_bad SNRs reach the threshold, and is empty from
    max_bad = n on; max_bad = 0 zeroes everything below the threshold by the other rule.  So a tied group can
    straddle the cut for 1 <= max_bad <= n - 1, and must, for 1, 6 and n - 1; for 0, n and n + 1 the weights are all
    0, or all positive, whatever the order."""
    x = sc.stage4_inputs(name)
    C = max(sc.STAGE4_CASES[name][3], 1)
    channels = np.repeat(x["present"], C, axis=1)
    n_all = channels.shape[1]
    assert n_all in (9, 20, 40) and (channels.sum(axis=1) < n_all).any()
    for o, max_bad in sc.stage4_runs(name):
        got = stage4_definition(name, o, max_bad)
        assert (got["measurement_snr"][channels] > 0).all()
        assert (got["measurement_snr"][channels] < np.float32(sc.THRESHOLD)).all()
        n = channels.sum(axis=1)
        positive = ((got["weights"] > 0) & channels).sum(axis=1)
        assert np.array_equal(positive, np.minimum(n, max_bad))
        if max_bad in (1, 6, n_all - 1):
            assert straddled(got, channels) >= 1, (name, max_bad)
        else:
            assert max_bad in (0, n_all, n_all + 1) or max_bad >= n.min() - 1


@pytest.mark.parametrize("name", list(sc.STAGE4_CASES))
def test_the_restated_magnitude_is_the_definition_on_the_stage_4_cases(name):
    F = sc.STAGE4_CASES[name][4]
    for o, max_bad in sc.stage4_runs(name):
        got, want = stage4_restated(name, o, max_bad), stage4_definition(name, o, max_bad)
        assert all(same(got[k], want[k]) for k in want), (o, max_bad, [k for k in want if not same(got[k], want[k])])
        assert gpu_check_of_stage_4(got, want, F)


# (defect, case, index into MW_OPTIONS, max_num_bad_measurements)
STAGE4_DEFECTS = [("ties_by_value", "distances_S4", 0, sc.MAX_BAD), ("ties_by_value", "distances_S9", 0, sc.MAX_BAD),
                  ("nan_first", "distances_S5", 0, sc.MAX_BAD), ("nan_first", "distances_S9", 0, sc.MAX_BAD),
                  ("percentiles_of_valid_at_3", "distances_S3", 0, sc.MAX_BAD),
                  ("one_sided_lerp", "distances_S2", 0, sc.MAX_BAD), ("one_sided_lerp", "distances_S3", 0, sc.MAX_BAD),
                  ("upper_middle_of_even", "bands", 4, sc.MAX_BAD), ("upper_middle_of_even", "bands", 6, sc.MAX_BAD),
                  ("upper_middle_of_even", "bands", 8, sc.MAX_BAD),
                  ("ties_last_index_first", "snr_ties_S9", 0, 6), ("ties_last_index_first", "snr_ties_S20", 0, 1),
                  ("ties_last_index_first", "snr_ties_S20_C2", 0, 39)]


@pytest.mark.parametrize("defect,name,o,max_bad", STAGE4_DEFECTS, ids=[f"{d[0]}-{d[1]}-{d[2]}-{d[3]}" for d in STAGE4_DEFECTS])
def test_a_planted_defect_fails_the_gpu_check_on_the_stage_4_cases(defect, name, o, max_bad):
    """The one-sided lerp a + diff t differs from NumPy's two-sided one by an ulp of a float64 bound, which the
    float32 weights do not show; it shows where a distance is +inf: inf - inf 0.25 is NaN, a + inf 0.75 is inf."""
    got, want = stage4_restated(name, o, max_bad, defect), stage4_definition(name, o, max_bad)
    assert not gpu_check_of_stage_4(got, want, sc.STAGE4_CASES[name][4])


def test_the_checks_demand_equal_bits_where_their_allowance_is_not_finite():
    want = np.array([1.0, 2.0, np.nan, np.inf])
    for allow in (np.inf, np.nan):
        assert sc.worst_ratio(want, want, allow) == 0.0
        assert sc.worst_ratio(np.array([1.0, np.nextafter(2.0, 3.0), np.nan, np.inf]), want, allow) == np.inf
    mixed = np.array([1.0, np.inf, 0.0, 0.0])
    assert sc.worst_ratio(np.array([1.5, 2.0, np.nan, np.inf]), want, mixed) == 0.5
    assert sc.worst_ratio(np.array([1.5, 2.5, np.nan, np.inf]), want, mixed) == np.inf
    assert sc.worst_ratio(np.array([1.0, 2.0, 0.0, np.inf]), want, 1.0) == np.inf        # the NaN pattern differs
    assert sc.worst_ratio(np.array([1.0, 2.0, np.nan, -np.inf]), want, 1.0) == np.inf


# ---- refusals and shapes that need no device ----
def test_refusals_of_the_definitions():
    x = sc.inputs("small")
    with pytest.raises(ValueError, match="attenuation"):
        pp.attenuation_plan(x["frequencies"], sc.MEDIUM, None, "both")
    with pytest.raises(ValueError, match="frequencies"):
        pp.attenuation_plan(np.ones(pp.SOURCE_SPECTRA_MAX_FREQUENCIES + 1), sc.MEDIUM)
    with pytest.raises(ValueError, match="reduce"):
        pp.network_average_spectrum_host(x["signal"], x["signal"], x["present"], x["dist"], snr_threshold=1.0,
                                         reduce="mode")
    with pytest.raises(ValueError):
        pp.network_average_spectrum_host(x["signal"], x["signal"][:, :, :2], x["present"], x["dist"], snr_threshold=1.0)
    for bands in (0, pp.SOURCE_SPECTRA_MAX_AVERAGING_BANDS + 1):
        with pytest.raises(ValueError, match="num_averaging_bands"):
            pp.approximate_moment_magnitude_host(x["signal"], x["signal"], x["present"], x["frequencies"], x["epi"],
                                                 num_averaging_bands=bands)
    with pytest.raises(ValueError, match="ascend"):
        pp.approximate_moment_magnitude_host(x["signal"], x["signal"], x["present"], x["frequencies"][::-1], x["epi"])


def test_refusals_of_the_python_surface_come_before_any_device_call():
    import torch
    from seismic_bpmf_amd import workflow
    x = sc.inputs("small")
    signal = torch.as_tensor(np.array(x["signal"]))
    tables = dict(dist_km=x["dist"], tt_p_sec=x["tt_p"], tt_s_sec=x["tt_s"], location_err_km=x["location_err"],
                  medium=sc.MEDIUM, snr_threshold=sc.THRESHOLD)
    kw = dict(phase="p", valid=x["present"], frequencies=x["frequencies"], **tables)
    with pytest.raises(ValueError, match="no CPU path"):
        workflow.network_average_spectra(signal, signal, **kw)
    with pytest.raises(ValueError, match="phase"):
        workflow.network_average_spectra(signal, signal, **{**kw, "phase": "sv"})
    with pytest.raises(ValueError, match="reduce"):
        workflow.network_average_spectra(signal, signal, reduce="mode", **kw)
    with pytest.raises(ValueError, match="attenuation"):
        workflow.network_average_spectra(signal, signal, attenuation="none", **kw)
    with pytest.raises(ValueError, match="float64"):
        workflow.network_average_spectra(signal.float(), signal.float(), **kw)
    with pytest.raises(ValueError, match="equal in shape"):
        workflow.network_average_spectra(signal, signal[:2], **kw)
    with pytest.raises(ValueError, match="frequencies"):
        workflow.network_average_spectra(signal, signal, **{**kw, "frequencies": x["frequencies"][:-1]})
    with pytest.raises(ValueError, match="valid"):
        workflow.network_average_spectra(signal, signal, **{**kw, "valid": x["present"][:, :2]})
    wide = torch.zeros((1, pp.SOURCE_SPECTRA_MAX_CHANNELS + 1, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="channels"):
        workflow.network_average_spectra(wide, wide, **{**kw, "valid": np.ones(wide.shape[:2], bool)})
    long = torch.zeros((1, 2, pp.SOURCE_SPECTRA_MAX_FREQUENCIES + 1), dtype=torch.float64)
    with pytest.raises(ValueError, match="frequencies"):
        workflow.network_average_spectra(long, long, **{**kw, "valid": np.ones((1, 2), bool),
                                                        "frequencies": np.arange(1.0, long.shape[-1] + 1)})
    mw = dict(valid=x["present"], frequencies=x["frequencies"], epicentral_dist_km=x["epi"])
    with pytest.raises(ValueError, match="no CPU path"):
        workflow.approximate_moment_magnitudes(signal, signal, **mw)
    for bands in (0, 9):
        with pytest.raises(ValueError, match="num_averaging_bands"):
            workflow.approximate_moment_magnitudes(signal, signal, num_averaging_bands=bands, **mw)
    with pytest.raises(ValueError, match="ascending"):
        workflow.approximate_moment_magnitudes(signal, signal, **{**mw, "frequencies": x["frequencies"][::-1]})
    with pytest.raises(ValueError, match="max_num_bad_measurements"):
        workflow.approximate_moment_magnitudes(signal, signal, max_num_bad_measurements=-1, **mw)
    with pytest.raises(ValueError, match="at least one phase"):
        workflow.source_spectra(noise=signal, epicentral_dist_km=x["epi"], frequencies=x["frequencies"], **tables)
    with pytest.raises(ValueError, match="valid_s"):
        workflow.source_spectra(s=signal, noise=signal, epicentral_dist_km=x["epi"], frequencies=x["frequencies"],
                                **tables)
    with pytest.raises(ValueError, match="GPU"):
        workflow.integrate_spectra(signal, x["frequencies"])
    with pytest.raises(ValueError, match="GPU"):
        workflow.differentiate_spectra(signal, x["frequencies"])


def test_the_c_entry_point_refuses_what_the_header_says():
    """Every call is refused before anything is launched (or, with no event, returns 0): no pointer is read."""
    import ctypes as C
    from seismic_bpmf_amd import _lib, build
    build.build_lib()
    lib = _lib.lib()
    one = C.c_void_p(8)

    def call(E=1, S=1, Cc=1, F=1, flags=8, bands=1, first=0, bad=6, valid=one, corrected=one, snr=one, signal=None):
        return lib.bpmf_source_spectra_dev(signal, None, valid, None, None, one, None, None, None, None, E, S, Cc, F,
                                           flags, 0.0, 1.0, 8.0, 0.0, 0, 0, 0, bands, first, 1.0, 3.0, bad, None,
                                           corrected, snr, None, None, None, None, None, one, one, one, one, one)
    assert call(E=0) == 0
    # (d_corrected and d_snr are needed by the stages that read or write them: 2, 4, 8 and 1, 4, 8)
    for kw in (dict(flags=0), dict(flags=16), dict(valid=None), dict(S=257), dict(S=43, Cc=6), dict(F=1025),
               dict(bands=0), dict(bands=9), dict(first=2), dict(bad=-1), dict(flags=4), dict(E=2**31, F=2),
               dict(corrected=None), dict(snr=None), dict(flags=1, snr=None, signal=one),
               dict(flags=2, corrected=None, signal=one)):
        assert call(**kw) == -1, kw
        assert b"bpmf_source_spectra_dev" in lib.bpmf_last_error()
