"""GPU: the Brune / Boatwright fit on the device (bpmf_fit_spectra_dev, workflow.fit_source_spectra), the gates and the
P-S average (workflow.moment_magnitudes), source_spectra(fit=...) and workflow.resample_spectra.

The entry point runs through the C ABI between guard bands (tests/arena.py) on outputs filled with 0xFF bytes, and is
compared with postprocess.fit_source_spectra_host by spectral_fit_cases.check: the discrete outputs equal, the cost,
ln fc, log10 M0, the errors and the stress drop inside the allowances that the rounding of exp, log10, pow and log
leaves (written in spectral_fit_cases.py before the first run on a GPU).  -rP prints the worst err / B per family."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import source_spectra_cases as sc
import spectral_fit_cases as sfc
from seismic_bpmf_amd import postprocess as pp

pytestmark = pytest.mark.gpu

OUTPUTS = [(k, np.float64) for k in pp.FIT_KEYS] + [("n_valid", np.int32), ("success", np.uint8), ("at_bound", np.uint8),
                                                    ("reason", np.uint8)]
_HOST = {}


def host_fit(key, x, model, weighted, phase="p", **options):
    """The definition's answer, computed once per case."""
    if key not in _HOST:
        _HOST[key] = pp.fit_source_spectra_host(x["average"], x["mask"], x["num_valid"], x["frequencies"], phase,
                                                model=model, weighted=weighted, **options)
    return _HOST[key]


def fit_between_guards(x, model, weighted, phase="p", min_fraction_valid_points=0.5,
                       min_fraction_valid_points_below_fc=0.1):
    """One call of bpmf_fit_spectra_dev on an arena: status 0, no guard byte changed, no input written."""
    import torch
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    E, F = x["average"].shape
    a = ar.Arena("torch")
    a.add_input("average", x["average"].astype(np.float64))
    a.add_input("mask", x["mask"].astype(np.uint8))
    a.add_input("num_valid", x["num_valid"].astype(np.int32))
    a.add_input("frequencies", x["frequencies"].astype(np.float64))
    for name, dtype in OUTPUTS:
        a.add_output(name, (E,), dtype)
    a.commit()
    p = {r.name: C.c_void_p(r.ptr) for r in a.regions}
    rc = lib.bpmf_fit_spectra_dev(p["average"], p["mask"], p["num_valid"], p["frequencies"], E, F,
                                  sfc.MODELS.index(model), ("p", "s").index(phase), int(weighted),
                                  min_fraction_valid_points, min_fraction_valid_points_below_fc,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream), *(p[name] for name, _ in OUTPUTS))
    torch.cuda.synchronize()
    assert rc == 0, lib.bpmf_last_error()
    assert a.check() == []
    assert not any(r.changed() for r in a.regions if r.kind == "input")
    out = {name: a[name].value() for name, _ in OUTPUTS}
    assert not (out["success"] > 1).any() and not (out["at_bound"] > 1).any()
    return out


def up(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def down(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def report(label, discrete, worst):
    print(f"{label}: discrete {'equal' if discrete else 'DIFFER'}; worst err / B " +
          ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert discrete and all(v <= 1.0 for v in worst.values()), (label, discrete, worst)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("model", sfc.MODELS)
@pytest.mark.parametrize("E,F", sfc.GPU_SHAPES, ids=[f"E{E}_F{F}" for E, F in sfc.GPU_SHAPES])
def test_device_against_the_definition(E, F, model, weighted):
    x = sfc.gpu_inputs(E, F, model, 100 * E + F)
    # unweighted: no least fraction, so that the events of 1, 2 and 3 valid bins are fitted too (under weights a
    # single bin's cost is the rounding of w^2 z / w^2 - z, and its minimum nobody's)
    options = {} if weighted else {"min_fraction_valid_points": 0.0}
    want = host_fit((E, F, model, weighted), x, model, weighted, **options)
    if E >= 5:
        assert set(want["n_valid"][:5].tolist()) == {0, 1, 2, 3, F} and (want["reason"] == 0).sum() >= 1
    got = fit_between_guards(x, model, weighted, **options)
    report(f"E={E} F={F} {model} {'weighted' if weighted else 'unweighted'}", *sfc.check(got, want, x, model, weighted))


def exact_groups():
    """The cases with known answers, stacked by (F, model, weighted) where they share the frequencies."""
    groups = {}
    for name, (x, model, weighted, options, _) in sfc.exact_cases().items():
        key = (x["frequencies"].tobytes(), model, weighted)
        groups.setdefault(key, []).append(name)
    return sorted(groups.values())


@pytest.mark.parametrize("names", exact_groups(), ids=lambda names: names[0])
def test_cases_with_known_answers(names):
    cases = sfc.exact_cases()
    x, (_, model, weighted, _, _) = sfc.stack(names, cases), cases[names[0]]
    want = host_fit(tuple(names), x, model, weighted)
    got = fit_between_guards(x, model, weighted)
    report(" ".join(names), *sfc.check(got, want, x, model, weighted))
    for e, name in enumerate(names):
        expect = cases[name][4]
        for k in ("reason", "at_bound", "n_valid"):
            if k in expect:
                assert got[k][e] == expect[k], (name, k, got[k][e])


def test_the_phase_and_the_fractions_reach_the_kernel():
    x = sfc.gpu_inputs(65, 25, "brune", 4242)
    options = dict(min_fraction_valid_points=0.7, min_fraction_valid_points_below_fc=0.3)
    want = host_fit("fractions", x, "brune", True, phase="s", **options)
    assert len(set(want["reason"].tolist())) >= 3
    got = fit_between_guards(x, "brune", True, phase="s", **options)
    report("phase s, fractions 0.7 / 0.3", *sfc.check(got, want, x, "brune", True))


@pytest.mark.parametrize("F", [25, 64])
def test_an_event_alone_gives_the_bits_of_the_batch(F):
    from seismic_bpmf_amd import workflow
    x = sfc.gpu_inputs(65, F, "boatwright", 9000 + F)
    f = x["frequencies"]
    batch = down(workflow.fit_source_spectra(up(x["average"]), up(x["mask"]), up(x["num_valid"]), frequencies=f,
                                             phase="p", model="boatwright", weighted=True))
    via_abi = fit_between_guards(x, "boatwright", True)
    for k in batch:
        assert batch[k].tobytes() == via_abi[k].astype(batch[k].dtype).tobytes(), k    # the wrapper adds nothing
    for e in (0, 1, 4, 5, 17, 33, 63, 64):
        alone = down(workflow.fit_source_spectra(up(x["average"][e:e + 1]), up(x["mask"][e:e + 1]),
                                                 up(x["num_valid"][e:e + 1]), frequencies=f, phase="p",
                                                 model="boatwright", weighted=True))
        for k in batch:
            assert alone[k].tobytes() == batch[k][e:e + 1].tobytes(), (e, k)


def source_spectra_arguments(name):
    x = sc.inputs(name)
    return dict(p=up(sc.phase_arguments(name, "p")["signal"]), s=up(sc.phase_arguments(name, "s")["signal"]),
                noise=up(x["noise"]), valid_p=x["present"], valid_s=x["present"], noise_valid=x["noise_present"],
                dist_km=x["dist"], epicentral_dist_km=x["epi"], tt_p_sec=x["tt_p"], tt_s_sec=x["tt_s"],
                location_err_km=x["location_err"], frequencies=x["frequencies"], medium=sc.MEDIUM,
                q_phase_prefactor=sc.PREFACTOR, **sc.average_kwargs(sc.AVERAGE_OPTIONS[0]),
                **{k: v for k, v in sc.mw_kwargs(sc.MW_OPTIONS[1]).items() if k != "snr_threshold"})


def test_source_spectra_with_a_fit_equals_the_separate_calls():
    from seismic_bpmf_amd import workflow
    arguments = source_spectra_arguments("edge")
    f = arguments["frequencies"]
    plain = workflow.source_spectra(**arguments)
    assert workflow.source_spectra(**arguments, fit=None).keys() == plain.keys()
    fit_keys = set(pp.FIT_KEYS) | {"n_valid", "success", "at_bound", "reason"}
    for on in ("average", "integrated"):
        got = workflow.source_spectra(**arguments, fit="boatwright", fit_weighted=True, fit_on=on,
                                      min_fraction_valid_points=0.3)
        for ph in ("p", "s"):
            assert set(got[ph]) == set(plain[ph]) | fit_keys and not fit_keys & set(plain[ph])
            for k in plain[ph]:
                assert down({k: got[ph][k]})[k].tobytes() == down({k: plain[ph][k]})[k].tobytes(), (ph, k)
            spectrum = plain[ph]["average"] if on == "average" else workflow.integrate_spectra(plain[ph]["average"], f)
            separate = workflow.fit_source_spectra(spectrum, plain[ph]["mask"], plain[ph]["num_valid"], frequencies=f,
                                                   phase=ph, model="boatwright", weighted=True,
                                                   min_fraction_valid_points=0.3)
            for k in fit_keys:
                assert down({k: got[ph][k]})[k].tobytes() == down({k: separate[k]})[k].tobytes(), (on, ph, k)
        both = workflow.moment_magnitudes(got["p"], got["s"])
        host = pp.moment_magnitudes_host(down({k: got["p"][k] for k in fit_keys}), down({k: got["s"][k] for k in fit_keys}))
        assert np.array_equal(both["Mw"].cpu().numpy(), host["Mw"], equal_nan=True)
        assert np.array_equal(both["Mw_err"].cpu().numpy(), host["Mw_err"], equal_nan=True)
        for ph in ("p", "s"):
            assert np.array_equal(both["accepted"][ph].cpu().numpy(), host["accepted"][ph])


def test_moment_magnitudes_gates_and_averages():
    from seismic_bpmf_amd import workflow
    x = sfc.gpu_inputs(65, 25, "brune", 31)
    y = sfc.gpu_inputs(65, 25, "brune", 32)
    fits = [workflow.fit_source_spectra(up(v["average"]), up(v["mask"]), up(v["num_valid"]), frequencies=v["frequencies"],
                                        phase=ph, weighted=True) for ph, v in (("p", x), ("s", y))]
    for limits in ((33.0, 33.0), (9.0, 100.0), (1.0e9, 8.0)):
        got = workflow.moment_magnitudes(*fits, max_rel_m0_err_pct=limits[0], max_rel_fc_err_pct=limits[1])
        want = pp.moment_magnitudes_host(down(fits[0]), down(fits[1]), max_rel_m0_err_pct=limits[0],
                                         max_rel_fc_err_pct=limits[1])
        assert np.array_equal(got["Mw"].cpu().numpy(), want["Mw"], equal_nan=True)
        assert np.array_equal(got["Mw_err"].cpu().numpy(), want["Mw_err"], equal_nan=True)
        assert all(np.array_equal(got["accepted"][ph].cpu().numpy(), want["accepted"][ph]) for ph in ("p", "s"))
    assert 0 < want["accepted"]["p"].sum() < down(fits[0])["success"].sum()         # the last limits cut through the fits
    one = workflow.moment_magnitudes(fit_s=fits[1])
    assert set(one["accepted"]) == {"s"}


def test_resample_spectra_bit_for_bit():
    from seismic_bpmf_amd import workflow
    rng = np.random.default_rng(6)
    bands = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0])
    targets = np.concatenate([[0.1, 0.5, 0.75, 1.0, 16.0, 29.0, np.nextafter(0.99 * 30.0, 0.0), 0.99 * 30.0, 30.0, 45.0],
                              rng.uniform(0.2, 35.0, 300)])
    spectra = rng.normal(size=(5, 7, 3, len(bands))) * 10.0 ** rng.uniform(-9, -3, (5, 7, 3, 1))
    want = pp.resample_spectra_host(spectra, bands, targets)
    got = workflow.resample_spectra(up(spectra), bands, targets)
    assert got.is_cuda and got.cpu().numpy().dtype == want.dtype and tuple(got.shape) == want.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert (want[..., 7:10] == 0.0).all() and (want[..., 6] > 0.0).all()
    assert np.array_equal(want[..., 0], np.abs(spectra[..., 0])) and np.array_equal(want[..., 4], np.abs(spectra[..., 5]))
    again = workflow.resample_spectra(up(spectra), up(bands), up(targets))
    assert again.cpu().numpy().tobytes() == want.tobytes()


def test_refusals_come_before_any_device_call(monkeypatch):
    from seismic_bpmf_amd import _lib, workflow

    def never(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "call", never)
    x = sfc.gpu_inputs(3, 25, "brune", 1)
    good = dict(average=up(x["average"]), mask=up(x["mask"]), num_valid=up(x["num_valid"]))
    f = x["frequencies"]

    def refused(match, frequencies=f, phase="p", **change):
        kw = {**good, **{k: v for k, v in change.items() if k in good}}
        other = {k: v for k, v in change.items() if k not in good}
        with pytest.raises(ValueError, match=match):
            workflow.fit_source_spectra(kw["average"], kw["mask"], kw["num_valid"], frequencies=frequencies, phase=phase,
                                        **other)

    refused("model", model="haskell")
    refused("phase", phase="x")
    refused("frequencies", frequencies=f[::-1])
    refused("frequencies", frequencies=np.where(np.arange(25) == 3, np.nan, f))
    refused("frequencies", frequencies=np.concatenate([[0.0], f[1:]]))
    refused("frequencies", frequencies=f[:-1])
    refused("average", average=good["average"].float())
    refused("num_valid", num_valid=good["num_valid"].long())
    refused("mask", mask=good["mask"].double())
    refused("(E, F)", average=good["average"][:2])
    refused("average", average=good["average"][0])
    refused("one GPU", average=good["average"].cpu())
    refused("one GPU", mask=good["mask"].cpu())
    wide = 1025
    refused("1024", average=up(np.ones((1, wide))), mask=up(np.zeros((1, wide), bool)),
            num_valid=up(np.ones((1, wide), np.int32)), frequencies=np.arange(1.0, wide + 1.0))
    with pytest.raises(ValueError, match="fit must be"):
        workflow.source_spectra(**source_spectra_arguments("small"), fit="haskell")
    with pytest.raises(ValueError, match="fit_on"):
        workflow.source_spectra(**source_spectra_arguments("small"), fit="brune", fit_on="differentiated")
    with pytest.raises(ValueError):
        workflow.moment_magnitudes()
    with pytest.raises(ValueError):
        workflow.resample_spectra(good["average"], f[::-1], f)
    with pytest.raises(ValueError, match="GPU"):
        workflow.resample_spectra(good["average"].cpu(), f, f)


def test_the_c_entry_point_refuses_what_the_header_says():
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(8)
    outs = [one] * 11

    def call(E=1, F=3, model=0, phase=0, pointers=None, null=None):
        args = [one] * 4
        o = list(outs)
        if null is not None:
            (args if null < 4 else o)[null if null < 4 else null - 4] = None
        return lib.bpmf_fit_spectra_dev(*args, E, F, model, phase, 0, 0.5, 0.1, None, *o)

    assert call(E=0) == 0
    for kw in (dict(F=0), dict(F=1025), dict(model=2), dict(model=-1), dict(phase=2), dict(E=2**31, F=1),
               dict(null=0), dict(null=3), dict(null=4), dict(null=14)):
        assert call(**kw) == -1, kw
        assert b"bpmf_fit_spectra_dev" in lib.bpmf_last_error()
