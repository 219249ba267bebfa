"""GPU: propagation corrections, network-average spectra and Mw* on the device (csrc/source_spectra.hip;
workflow.network_average_spectra, approximate_moment_magnitudes, source_spectra, integrate_spectra,
differentiate_spectra) against the definitions on the host (postprocess.source_spectra_host,
approximate_moment_magnitude_host, themselves pinned to the reference bit for bit in tests/test_source_spectra_host.py).

The checks are source_spectra_cases.check_average / corrected_ok / check_mw, written down before
the first run on a GPU: masks, num_valid, used, the float32 measurement SNRs and weights (so the set of weighted
channels), the all-masked events and every NaN pattern must be EQUAL for every event -- no event is excluded; the input
conditions that make this a fair demand are asserted on the definition in the host test.  `snr` must be equal (one
correctly rounded division), `corrected` must be fl(fl(x g) a') for an a' within 2 ulp of the host's attenuation
factor, and `average`, `std`, `measured_disp`, `log10_M0`, `Mw_star` lie within allowances from the operation count.
Every test prints its worst err / allowance (-rP); the planted defects of the host test fail these same checks.

The session runs with debug.poison_output on (tests/conftest.py): every output is filled with 0xFF bytes before the
kernels run, and the calls are the first use of allocations that were filled with junk and given back."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_spectra_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host_average(name, phase, o, attenuation="reference"):
    from seismic_bpmf_amd import postprocess as pp
    want = pp.source_spectra_host(**sc.phase_arguments(name, phase, attenuation),
                                  **sc.average_kwargs(sc.AVERAGE_OPTIONS[o]))
    for a in want.values():
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def host_mw(name, phase, o):
    from seismic_bpmf_amd import postprocess as pp
    x, chain = sc.inputs(name), host_average(name, phase, 0)
    want = pp.approximate_moment_magnitude_host(chain["corrected"], chain["snr"], x["present"], x["frequencies"],
                                                x["epi"], **sc.mw_kwargs(sc.MW_OPTIONS[o]))
    for a in want.values():
        a.setflags(write=False)
    return want


def junk(n_bytes):
    """Allocations of about the call's size filled with 0xA5 bytes and handed back to the caching allocator."""
    import torch
    for size in (n_bytes, n_bytes // 2, 1 << 20, 1 << 12):
        torch.full((max(int(size), 1),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()


def up(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def down(result):
    return {k: v.cpu().numpy() for k, v in result.items()}


def device_average(name, phase, o, attenuation="reference", events=slice(None)):
    from seismic_bpmf_amd import workflow
    x, option = sc.inputs(name), sc.AVERAGE_OPTIONS[o]
    signal = sc.phase_arguments(name, phase)["signal"]
    junk(4 * signal.nbytes)
    return down(workflow.network_average_spectra(
        up(signal[events]), up(x["noise"][events]), phase=phase, valid=x["present"][events],
        noise_valid=x["noise_present"][events], dist_km=x["dist"][events], tt_p_sec=x["tt_p"][events],
        tt_s_sec=x["tt_s"][events], location_err_km=x["location_err"][events], frequencies=x["frequencies"],
        medium=sc.MEDIUM, q_phase_prefactor=sc.PREFACTOR, attenuation=attenuation, **sc.average_kwargs(option)))


def device_mw(name, corrected, snr, o, events=slice(None)):
    from seismic_bpmf_amd import workflow
    x = sc.inputs(name)
    junk(4 * corrected.nbytes)
    return down(workflow.approximate_moment_magnitudes(
        up(corrected[events]), up(snr[events]), valid=x["present"][events], frequencies=x["frequencies"],
        epicentral_dist_km=x["epi"][events], **sc.mw_kwargs(sc.MW_OPTIONS[o])))


def assert_average(label, got, want, arguments, option, C):
    assert got["corrected"].shape == want["corrected"].shape and got["average"].dtype == np.float64
    assert got["mask"].dtype == bool and got["used"].dtype == bool and got["num_valid"].dtype == np.int32
    assert np.array_equal(got["snr"], want["snr"], equal_nan=True), label
    with np.errstate(all="ignore"):
        geometry = arguments["geometry_constant"] * (1000.0 * arguments["dist_km"]) / arguments["radiation"]
        att = np.exp(np.pi * arguments["tt_sec"][..., None] * arguments["frequencies"] / arguments["q_row"])
    wide = (slice(None), slice(None)) + (None,) * (want["corrected"].ndim - 2)
    failed = sc.corrected_ok(got["corrected"], arguments["signal"], geometry[wide],
                             att if want["corrected"].ndim == 3 else att[:, :, None, :], arguments["present"])
    discrete, r_avg, r_std = sc.check_average(got, want, option, C)
    print(f"{label}: corrected outside fl(fl(x g) a') {failed:.3e}; worst err / allowance: average {r_avg:.3e}, "
          f"std {r_std:.3e}")
    assert failed == 0.0, (label, failed)
    assert discrete, label
    assert np.array_equal(np.isnan(got["average"]), want["mask"] | np.isnan(want["average"])), label
    assert r_avg <= 1.0 and r_std <= 1.0, (label, r_avg, r_std)


def assert_mw(label, got, want, n_bands):
    discrete, r_disp, r_m0, r_mw = sc.check_mw(got, want, n_bands)
    print(f"{label}: worst err / allowance: measured_disp {r_disp:.3e}, log10_M0 {r_m0:.3e}, Mw_star {r_mw:.3e}")
    assert got["weights"].dtype == np.float32 and got["measurement_snr"].dtype == np.float32
    assert discrete, label
    assert r_disp <= 1.0 and r_m0 <= 1.0 and r_mw <= 1.0, (label, r_disp, r_m0, r_mw)


# every shape of the issue: E = 3 with S = 5, C = 1, F = 4; 63 / 64 / 65 channels and bins; the ceilings; (E, S, F)
# and (E, S, C, F); events without a station, bins without a channel, even and odd counts, zeros, NaN, missing noise
@pytest.mark.parametrize("name", sc.STAGES_1_TO_3_CASES)
def test_stages_1_to_3_equal_the_definition(name):
    C = max(sc.CASES[name][3], 1)
    options = range(len(sc.AVERAGE_OPTIONS)) if name != "ceiling" else (0, 1)
    for phase in sc.PHASES:
        for o in options:
            want = host_average(name, phase, o)
            got = device_average(name, phase, o)
            assert_average(f"{name} {phase} {sc.AVERAGE_OPTIONS[o]}", got, want, sc.phase_arguments(name, phase),
                           sc.AVERAGE_OPTIONS[o], C)


def test_the_cases_reach_every_path():
    """An event with no station left, a bin with no valid channel, even and odd median counts, all-masked events by
    the distance cut-off, and masks by the least count -- on the definition, so that the comparison above means it."""
    want = host_average("edge", "p", 1)
    count = np.where(want["mask"], -1, want["num_valid"])
    assert (~want["used"]).all(axis=1).any() and want["used"].all(axis=1).any()
    assert (want["used"].any(axis=1) & ~want["used"].all(axis=1)).any()
    assert (want["mask"] & want["used"].any(axis=1)[:, None]).any()
    assert (count > 0).any() and (count[count > 0] % 2 == 0).any() and (count[count > 0] % 2 == 1).any()
    least = host_average("edge", "p", 4)
    assert (least["mask"] & (least["num_valid"] > 0)).any()
    assert host_average("edge", "p", 6)["mask"].all() and host_average("edge", "p", 7)["mask"].all()


@pytest.mark.parametrize("attenuation", ["reference", "physical"])
def test_both_attenuation_pairings(attenuation):
    for phase in sc.PHASES:
        want = host_average("edge", phase, 0, attenuation)
        got = device_average("edge", phase, 0, attenuation)
        assert_average(f"edge {phase} {attenuation}", got, want, sc.phase_arguments("edge", phase, attenuation),
                       sc.AVERAGE_OPTIONS[0], 1)
    assert not np.array_equal(host_average("edge", "p", 0, "physical")["corrected"],
                              host_average("edge", "p", 0, "reference")["corrected"])


@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_stage_4_equals_the_definition(name):
    F = sc.CASES[name][4]
    for phase in sc.PHASES:
        chain = host_average(name, phase, 0)
        for o in range(len(sc.MW_OPTIONS)):
            got = device_mw(name, chain["corrected"], chain["snr"], o)
            assert_mw(f"{name} {phase} {sc.MW_OPTIONS[o]}", got, host_mw(name, phase, o), F)


@pytest.mark.parametrize("name", list(sc.STAGE4_CASES))
def test_stage_4_equals_the_definition_on_the_cases_built_directly(name):
    """4 to 8 averaging bands, tied, zero and non-finite distances at S = 2, 3, 4, 5 and 9, and tied SNRs across the
    weight cut-off at 9, 20 and 40 channels (source_spectra_cases.stage4_inputs; what each case reaches is asserted on
    the definition in tests/test_source_spectra_host.py).  No event is excluded."""
    from seismic_bpmf_amd import postprocess as pp, workflow
    x = sc.stage4_inputs(name)
    F = sc.STAGE4_CASES[name][4]
    junk(4 * x["corrected"].nbytes)
    corrected, snr = up(x["corrected"]), up(x["snr"])
    for o, max_bad in sc.stage4_runs(name):
        kw = sc.mw_kwargs(sc.MW_OPTIONS[o], max_bad)
        with np.errstate(all="ignore"):
            want = pp.approximate_moment_magnitude_host(x["corrected"], x["snr"], x["present"], x["frequencies"],
                                                        x["epi"], **kw)
        got = down(workflow.approximate_moment_magnitudes(corrected, snr, valid=x["present"],
                                                          frequencies=x["frequencies"], epicentral_dist_km=x["epi"],
                                                          **kw))
        assert_mw(f"{name} {sc.MW_OPTIONS[o]} max_bad={max_bad}", got, want, F)


@pytest.mark.parametrize("name", ["small", "edge", "components", "c65"])
def test_source_spectra_runs_both_stages_for_both_phases(name):
    from seismic_bpmf_amd import workflow
    x = sc.inputs(name)
    C, F = max(sc.CASES[name][3], 1), sc.CASES[name][4]
    got = workflow.source_spectra(
        p=up(sc.phase_arguments(name, "p")["signal"]), s=up(sc.phase_arguments(name, "s")["signal"]),
        noise=up(x["noise"]), valid_p=x["present"], valid_s=x["present"], noise_valid=x["noise_present"],
        dist_km=x["dist"], epicentral_dist_km=x["epi"], tt_p_sec=x["tt_p"], tt_s_sec=x["tt_s"],
        location_err_km=x["location_err"], frequencies=x["frequencies"], medium=sc.MEDIUM,
        q_phase_prefactor=sc.PREFACTOR, **sc.average_kwargs(sc.AVERAGE_OPTIONS[0]),
        **{k: v for k, v in sc.mw_kwargs(sc.MW_OPTIONS[1]).items() if k != "snr_threshold"})
    assert sorted(got) == ["p", "s"]
    for phase in sc.PHASES:
        result = down(got[phase])
        assert_average(f"{name} {phase}", result, host_average(name, phase, 0), sc.phase_arguments(name, phase),
                       sc.AVERAGE_OPTIONS[0], C)
        assert_mw(f"{name} {phase}", result, host_mw(name, phase, 1), F)


def test_an_event_gives_the_same_bits_alone_and_in_a_batch_of_70():
    assert sc.CASES["batch"][1] == 70
    for o in (0, 1):
        whole = device_average("batch", "s", o)
        for e in (0, 37, 69):
            alone = device_average("batch", "s", o, events=slice(e, e + 1))
            for key in whole:
                assert np.array_equal(alone[key][0], whole[key][e], equal_nan=True), (o, e, key)
    whole_mw = device_mw("batch", whole["corrected"], whole["snr"], 1)
    for e in (0, 37, 69):
        alone = device_mw("batch", whole["corrected"], whole["snr"], 1, events=slice(e, e + 1))
        for key in whole_mw:
            assert np.array_equal(alone[key][0], whole_mw[key][e], equal_nan=True), (e, key)


def test_one_over_each_ceiling_is_refused():
    import torch
    from seismic_bpmf_amd import postprocess as pp, workflow
    kw = dict(phase="p", dist_km=None, tt_p_sec=None, tt_s_sec=None, location_err_km=None, medium=sc.MEDIUM,
              snr_threshold=sc.THRESHOLD)
    S, F = pp.SOURCE_SPECTRA_MAX_CHANNELS + 1, 4
    x = torch.zeros((1, S, F), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="channels"):
        workflow.network_average_spectra(x, x, valid=np.ones((1, S), bool), frequencies=np.arange(1.0, F + 1), **kw)
    x = torch.zeros((1, 43, 6, F), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="channels"):
        workflow.approximate_moment_magnitudes(x, x, valid=np.ones((1, 43), bool), frequencies=np.arange(1.0, F + 1),
                                               epicentral_dist_km=np.ones((1, 43)))
    F = pp.SOURCE_SPECTRA_MAX_FREQUENCIES + 1
    x = torch.zeros((1, 2, F), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="frequencies"):
        workflow.network_average_spectra(x, x, valid=np.ones((1, 2), bool), frequencies=np.arange(1.0, F + 1), **kw)
    with pytest.raises(ValueError, match="frequencies"):
        workflow.approximate_moment_magnitudes(x, x, valid=np.ones((1, 2), bool), frequencies=np.arange(1.0, F + 1),
                                               epicentral_dist_km=np.ones((1, 2)))


def test_integrate_and_differentiate():
    from seismic_bpmf_amd import workflow
    x = sc.inputs("components")
    spectra, f = up(x["signal"]), x["frequencies"]
    assert np.array_equal(workflow.integrate_spectra(spectra, f).cpu().numpy(), x["signal"] / f)
    assert np.array_equal(workflow.differentiate_spectra(spectra, up(f)).cpu().numpy(), x["signal"] * f)
    with pytest.raises(ValueError):
        workflow.integrate_spectra(spectra, f[:-1])


@pytest.mark.parametrize("multi", [True, False])
def test_the_output_of_fft_spectra_fed_straight_in(multi):
    """A small day: noise, P and S windows through workflow.fft_spectra, their tensors handed to source_spectra as they
    are; the definition runs on the downloaded spectra.  One window leaves the day: its station is absent."""
    import torch
    from seismic_bpmf_amd import postprocess as pp, workflow
    rng = np.random.default_rng(5)
    S, C, N, E, n, sr = 4, 3, 6000, 3, 256, 50.0
    t = np.arange(N) / sr
    day = rng.normal(0.0, 1.0, size=(S, C, N))
    p_starts = rng.integers(1500, 4000, size=(E, S))
    for e in range(E):
        for s in range(S):
            k = p_starts[e, s]
            day[s, :, k:k + 2 * n] += 30.0 * rng.normal(0.0, 1.0, size=(C, 2 * n)) * np.exp(-(t[:2 * n]) / 2.0)
    day = torch.as_tensor(day.astype(np.float32), device="cuda")
    s_starts = p_starts + n
    noise_starts = p_starts - 2 * n
    s_starts[1, 2] = N - n + 1                                       # not wholly inside the day
    f = workflow.target_frequencies(1.0, 20.0, 9)
    spectra = {k: workflow.fft_spectra(day, st, n, sr=sr, frequencies=f, multi_component=multi)
               for k, st in (("noise", noise_starts), ("p", p_starts), ("s", s_starts))}
    assert not bool(spectra["s"][2][1, 2]) and bool(spectra["p"][2].all())
    dist = rng.uniform(5.0, 40.0, size=(E, S))
    tables = dict(dist_km=dist, tt_p_sec=dist / 6.0, tt_s_sec=dist / 3.5, location_err_km=np.full(E, 0.5))
    got = workflow.source_spectra(
        p=spectra["p"][0], s=spectra["s"][0], noise=spectra["noise"][0], valid_p=spectra["p"][2],
        valid_s=spectra["s"][2], noise_valid=spectra["noise"][2], epicentral_dist_km=0.9 * dist, frequencies=f,
        medium=sc.MEDIUM, snr_threshold=3.0, q_phase_prefactor=sc.PREFACTOR, reduce="median", num_averaging_bands=2,
        **tables)
    option = (True, "median", 0, 25.0)
    for k, phase in enumerate(sc.PHASES):
        signal, valid = spectra[phase][0].cpu().numpy(), spectra[phase][2].cpu().numpy()
        which, q_rows = pp.attenuation_plan(f, sc.MEDIUM, sc.PREFACTOR)
        arguments = dict(signal=signal, noise=spectra["noise"][0].cpu().numpy(), present=valid,
                         noise_present=spectra["noise"][2].cpu().numpy(), dist_km=dist,
                         tt_sec=tables["tt_" + which[k] + "_sec"], location_err_km=tables["location_err_km"],
                         frequencies=f, q_row=q_rows[k], geometry_constant=pp.geometry_constants(sc.MEDIUM)[k],
                         radiation=(pp.RADIATION_P, pp.RADIATION_S)[k])
        want = pp.source_spectra_host(**arguments, snr_threshold=3.0, average_log=True, reduce="median")
        result = down(got[phase])
        assert_average(f"fft {phase} multi={multi}", result, want, arguments, option, 1 if multi else C)
        assert (~want["mask"]).any()
        want_mw = pp.approximate_moment_magnitude_host(want["corrected"], want["snr"], valid, f, 0.9 * dist,
                                                       snr_threshold=3.0, num_averaging_bands=2)
        # stage 4 ran on the device's own corrected spectra: the host's, within CORRECTED_ULP (in the allowance)
        assert_mw(f"fft {phase} multi={multi}", result, want_mw, len(f))
