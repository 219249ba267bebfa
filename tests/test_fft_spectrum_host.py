"""Host: the definition of the FFT-method spectra (postprocess.fft_spectrum_host, fft_spectrum_plan, dft_twiddles,
fft_windows_host) against the reference's recorded answers (tests/golden/fft_spectrum.npz, made by
tests/golden/make_fft_spectrum_golden.py from BPMF/spectrum.py itself), and the sharpness of the allowance the device
is held to (fft_spectrum_cases.allowance): a NumPy model of the device's pruned DFT passes it, and each of twelve
planted defects fails it on at least one case of a quick subset (-rP prints the matrix).

The recorded spectra hold NumPy's own FFT and np.interp to the last bit; the file names the NumPy that made it."""
import importlib.util
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fft_spectrum_cases as fc  # noqa: E402
import golden_npz  # noqa: E402
from seismic_bpmf_amd import postprocess as pp  # noqa: E402

SR = fc.SAMPLING_RATE
GOLDEN = os.path.join(HERE, "golden", "fft_spectrum.npz")
REFERENCE = os.environ.get("BPMF_RECORD_REFERENCE")


@pytest.fixture(scope="module")
def golden():
    return golden_npz.load(GOLDEN)


def definition(index, dtype, alpha, multi, **kw):
    n, key, _ = fc.CASES[index]
    x = fc.windows(index).astype(np.float32 if dtype == "f32" else np.float64)
    return pp.fft_spectrum_host(x, sr=SR, frequencies=fc.targets(key, n), alpha=alpha, multi_component=multi, **kw)


# ---- the definition against the reference's recorded answers ----

@pytest.mark.parametrize("index,dtype,alpha", fc.RECORDED,
                         ids=[f"{fc.label(k)} {d} alpha={a}" for k, d, a in fc.RECORDED])
def test_definition_equals_the_recorded_reference_bit_for_bit(golden, index, dtype, alpha):
    n, key, (E, S, C) = fc.CASES[index]
    for multi in (False, True):
        got, freq = definition(index, dtype, alpha, multi)
        want = golden[fc.recorded_key(index, dtype, alpha, multi)]
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want, equal_nan=True), (fc.label(index), multi, str(golden["numpy_version"]))
        if key is None:
            assert np.array_equal(freq, np.fft.rfftfreq(n, d=1.0 / SR))
            assert got.dtype == (np.float64 if multi else np.complex128)
        else:
            assert freq.dtype == np.float64 and np.array_equal(freq, fc.targets(key, n))
        if (E, S, C) == fc.SMALL:
            nan = got[fc.NAN_ROW[:2]] if multi else got[fc.NAN_ROW]
            zero = np.zeros(got.shape[-1], bool) if key is None else pp.fft_spectrum_plan(n, SR, freq)["outside"]
            assert np.isnan(fc.as_reals(nan[~zero])).all() and not nan[zero].any()
            if not multi:
                assert not got[fc.ZERO_ROW].any()


def test_float32_and_float64_traces_give_the_same_bits(golden):
    """trace * taper is float64 for both: the recorded pairs agree, and so does the definition."""
    pairs = [(k, a) for k, d, a in fc.RECORDED if d == "f64"]
    assert len(pairs) >= 5
    for index, alpha in pairs:
        for multi in (False, True):
            assert np.array_equal(golden[fc.recorded_key(index, "f32", alpha, multi)],
                                  golden[fc.recorded_key(index, "f64", alpha, multi)], equal_nan=True)


def test_recorded_set_covers_both_alphas_modes_and_complex_spectra(golden):
    assert {a for _, _, a in fc.RECORDED} == {0.05, 0.15} and {d for _, d, _ in fc.RECORDED} == {"f32", "f64"}
    complex_keys = [k for k in golden.files if k.startswith("single_") and np.iscomplexobj(golden[k])]
    assert len(complex_keys) >= 6
    assert not np.array_equal(golden[fc.recorded_key(fc.CASES.index((64, "log25", fc.SMALL)), "f32", 0.05, False)],
                              golden[fc.recorded_key(fc.CASES.index((64, "log25", fc.SMALL)), "f32", 0.15, False)],
                              equal_nan=True)
    assert str(golden["numpy_version"])


@pytest.fixture(scope="module")
def live_spectrum():
    """BPMF.spectrum.Spectrum of the live reference, imported with stub modules; skipped where it is not available."""
    if not REFERENCE:
        pytest.skip("BPMF_RECORD_REFERENCE is not set: no live reference")
    pytest.importorskip("scipy")
    pytest.importorskip("pandas")
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "golden", "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.REF = REFERENCE
    cwd, path0, mods0 = os.getcwd(), list(sys.path), set(sys.modules)
    try:
        mg.import_reference()                        # chdir()s into a scratch directory: BPMF reads its cfg from the CWD
    finally:
        os.chdir(cwd)
    from BPMF.spectrum import Spectrum
    yield Spectrum
    for name in set(sys.modules) - mods0:
        if isinstance(sys.modules[name], MagicMock) or name == "BPMF" or name.startswith("BPMF."):
            del sys.modules[name]
    sys.path[:] = path0


def test_definition_equals_the_live_reference(live_spectrum):
    spec = importlib.util.spec_from_file_location("make_fft_spectrum_golden",
                                                  os.path.join(HERE, "golden", "make_fft_spectrum_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    for index in fc.QUICK:
        n, key, _ = fc.CASES[index]
        for dtype in (np.float32, np.float64):
            x = fc.windows(index).astype(dtype)
            for multi in (False, True):
                want = maker.reference_case(live_spectrum, x, SR, 0.15, multi, fc.targets(key, n))
                got, _ = pp.fft_spectrum_host(x, sr=SR, frequencies=fc.targets(key, n), alpha=0.15,
                                              multi_component=multi)
                assert np.array_equal(got, want, equal_nan=True), (fc.label(index), dtype, multi)


def test_snr_of_the_definition_equals_the_recorded_one(golden):
    n, key, (E, S, C) = fc.CASES[fc.SNR_CASE]
    valid = np.ones((E, S), dtype=bool)
    valid[fc.SNR_MISSING] = False
    for multi in (False, True):
        signal, _ = definition(fc.SNR_CASE, "f32", 0.05, multi)
        want = golden["snr_multi" if multi else "snr"]
        got = pp.spectral_snr_host(signal, signal[fc.SNR_NOISE_EVENTS], valid)
        # the recorded NaN rows hold what the reference's FFT made of them: NaN at every target it does not zero, too
        assert np.array_equal(got, want, equal_nan=True)
        assert np.isnan(want).any() and not want[fc.SNR_MISSING].any()
        assert np.isinf(want).any() == (not multi)                      # x / 0: the zero row as noise
        assert (want == 0).any()


# ---- the parts ----

def test_taper_is_scipys_tukey_bit_for_bit():
    tukey = pytest.importorskip("scipy.signal.windows").tukey
    for n in sorted({c[0] for c in fc.CASES}):
        for alpha in (0.0, 0.05, 0.15, 0.5, 0.999):
            assert np.array_equal(pp.fft_spectrum_plan(n, SR, alpha=alpha)["taper"], tukey(n, alpha)), (n, alpha)
    assert not pp.fft_spectrum_plan(2, SR)["taper"].any()                # n = 2: the window is all zero
    own = np.linspace(0.5, 1.5, 17)
    assert np.array_equal(pp.fft_spectrum_plan(17, SR, taper=own)["taper"], own)


def test_twiddles_are_within_2_to_the_minus_52():
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble is no wider than float64 here")
    pi = np.longdouble("3.14159265358979323846264338327950288")
    rng = np.random.default_rng(52)
    worst = 0.0
    for n in sorted({c[0] for c in fc.CASES} | {int(v) for v in rng.integers(1, fc.CAP + 1, 200)}):
        table = pp.dft_twiddles(n)
        assert table.shape == (n, 2) and table.dtype == np.float64 and not np.signbit(table[table == 0]).any()
        m = np.arange(n, dtype=np.longdouble)
        # the angle reduced below 2 pi in integers; what long double leaves of error is below 2^-60
        truth = np.stack([np.cos(2 * pi * m / n), -np.sin(2 * pi * m / n)], axis=1)
        worst = max(worst, float(np.abs(table.astype(np.longdouble) - truth).max()))
        assert table[0, 0] == 1.0 and table[0, 1] == 0.0
        if n % 4 == 0:
            assert table[n // 4, 0] == 0.0 and table[n // 4, 1] == -1.0 and table[n // 2, 0] == -1.0
    print(f"worst twiddle error: {worst * 2.0 ** 52:.3f} x 2^-52")
    assert worst <= 2.0 ** -52


def test_plan_pairs_reproduce_np_interp_exactly_on_the_recorded_spectra(golden):
    tried = 0
    for index, dtype, alpha in fc.RECORDED:
        n, key, _ = fc.CASES[index]
        if key is not None or n < 3:
            continue
        for multi in (False, True):
            fp = np.abs(golden[fc.recorded_key(index, dtype, alpha, multi)])
            fp = fp.reshape(-1, fp.shape[-1])
            fp = fp[np.isfinite(fp).all(axis=1)]
            for targets in ("log25", "single", "bins", "low", "duplicates", "straddle", "1024"):
                f = fc.targets(targets, n)
                plan = pp.fft_spectrum_plan(n, SR, f)
                bins, p = plan["bins"], plan["pair"]
                assert (np.diff(bins) > 0).all() and bins[0] >= 0 and bins[-1] <= n // 2
                assert (bins[p + 1] == bins[p] + 1).all() and len(bins) <= 2 * len(f)
                freq = plan["freq"]
                assert np.array_equal(plan["dx"], f - freq[bins[p]]) and (plan["span"] > 0).all()
                assert np.array_equal(plan["outside"], f >= 0.99 * freq.max())
                lo, hi = fp[:, bins[p]], fp[:, bins[p + 1]]
                got = np.where(plan["exact"], lo, ((hi - lo) / plan["span"]) * plan["dx"] + lo)
                got[:, plan["outside"]] = 0.0
                want = np.stack([np.interp(f, freq, row) for row in fp])
                want[:, plan["outside"]] = 0.0
                assert np.array_equal(got, want), (fc.label(index), targets, multi)
                tried += 1
    assert tried >= 50
    plan = pp.fft_spectrum_plan(1500, SR, fc.targets("straddle", 1500))
    assert list(plan["outside"]) == [False, False, True, True, True, True, True, False]
    plan = pp.fft_spectrum_plan(17, SR, fc.targets("bins", 17))           # (the last bin is `outside`: its pair is K - 2)
    assert plan["exact"][:-1].all() and plan["outside"][-1] and list(plan["bins"]) == list(range(9))
    assert np.array_equal(pp.fft_spectrum_plan(16, SR)["bins"], np.arange(9))


def test_windows_are_the_multiband_ones():
    rng = np.random.default_rng(3)
    day = rng.standard_normal((3, 2, 300)).astype(np.float32)
    starts = np.array([[0, -1, 236], [237, 7, 236]], dtype=np.int64)
    got, valid = pp.fft_windows_host(day, starts, 64)
    want, want_valid = pp.multiband_windows_host(day, starts, 64)
    assert np.array_equal(got, want) and np.array_equal(valid, want_valid)
    assert list(valid.reshape(-1)) == [True, False, True, False, True, True] and not got[~valid].any()


def test_refusals():
    x = np.zeros((1, 1, 1, 64), np.float32)
    for kw, match in [(dict(n_samples=1), "2 .. 16384"), (dict(n_samples=16385), "2 .. 16384"),
                      (dict(sr=0.0), "sr > 0"), (dict(sr=np.nan), "sr > 0"), (dict(alpha=1.0), "alpha"),
                      (dict(alpha=-0.1), "alpha"), (dict(taper=np.ones(63)), "taper"),
                      (dict(frequencies=np.zeros(0)), "frequencies"), (dict(frequencies=np.ones(1025)), "frequencies"),
                      (dict(frequencies=np.ones((2, 2))), "frequencies"),
                      (dict(frequencies=np.array([1.0, np.nan])), "frequencies"),
                      (dict(frequencies=np.array([np.inf])), "frequencies")]:
        with pytest.raises(ValueError, match=match):
            pp.fft_spectrum_plan(**{**dict(n_samples=64, sr=SR), **kw})
    with pytest.raises(ValueError, match=r"\(E, S, C, n\)"):
        pp.fft_spectrum_host(x[0], sr=SR)
    with pytest.raises(ValueError, match="2 .. 16384"):
        pp.fft_spectrum_host(x[..., :1], sr=SR)
    for n in (0, 16385):
        with pytest.raises(ValueError, match="dft_twiddles"):
            pp.dft_twiddles(n)
    assert pp.fft_spectrum_host(x, sr=SR, frequencies=np.ones(1024))[0].shape == (1, 1, 1, 1024)


def test_size_function_refuses_what_the_entry_point_refuses():
    from seismic_bpmf_amd import _lib
    size = _lib.lib().bpmf_fft_spectrum_workspace_size
    assert size(64, 1500, 50, 25) == size(1, 1500, 50, 25) == size(0, 1500, 50, 25) > 64 * 50 * 16
    assert size(65, 1500, 50, 25) == size(128, 1500, 50, 25) > size(64, 1500, 50, 25)
    for args in [(64, 1, 1, 0), (64, 16385, 50, 25), (64, 1500, 0, 25), (64, 1500, 752, 0), (64, 1500, 50, 1025),
                 (2 ** 31, 1500, 50, 25), (2 ** 31 // 100 + 1, 1500, 50, 25), (2 ** 31 // 1024 + 1, 1500, 2, 1024)]:
        assert size(*args) == 0, args
    assert size(64, 1500, 751, 0) > 0 and size(64, 2, 2, 1024) > 0 and size(2 ** 31 // 100 - 64, 1500, 50, 25) > 0


def test_size_function_returns_the_recorded_bytes():
    """tests/golden/fft_spectrum_workspace_size.json: what the layout gave when it was written, refused sizes (0)
    included -- a change of the carve-up shows here as tests/test_workspace_layout.py shows it for the older ones."""
    import json
    from seismic_bpmf_amd import _lib
    size = _lib.lib().bpmf_fft_spectrum_workspace_size
    with open(os.path.join(HERE, "golden", "fft_spectrum_workspace_size.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 25 and sum(1 for _, want in recorded if want == 0) >= 8
    wrong = [(args, int(size(*args)), want) for args, want in recorded if int(size(*args)) != want]
    assert not wrong, wrong


def test_entry_point_refuses_before_any_launch():
    """Every argument check comes before the first device call: on a machine without a GPU, with addresses that are
    no memory at all, the entry point answers -1 and names what it refuses."""
    import ctypes as C
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    good = dict(S=2, C=3, N=5000, n_windows=4, n=1500, delta=0.01, n_bins=50, n_targets=25, multi=0, ws=1 << 20)

    def call(**kw):
        a = {**good, **kw}
        return lib.bpmf_fft_spectrum_dev(fake, a["S"], a["C"], a["N"], a["n_windows"], fake, a["n"], fake, fake,
                                         a["delta"], fake, a["n_bins"], a.get("pair", fake), fake, fake, fake,
                                         a["n_targets"], a["multi"], fake, a["ws"], None, fake, fake)

    least = lib.bpmf_fft_spectrum_workspace_size(64, 1500, 50, 25)
    for kw, word in [(dict(n=1), "samples"), (dict(n=16385), "samples"), (dict(n_bins=0), "bins"),
                     (dict(n_bins=752), "bins"), (dict(n_targets=1025), "targets"), (dict(ws=least - 1), "workspace"),
                     (dict(n_windows=3), "whole number of events"), (dict(S=0), "bad argument"),
                     (dict(pair=None), "null pointer"), (dict(delta=float("nan")), "delta"),
                     (dict(C=65, multi=1), "64 components"),
                     (dict(S=1, C=1, n_windows=2 ** 31 // 100 + 1), r"2^31")]:
        assert call(**kw) == -1, kw
        assert word in lib.bpmf_last_error().decode(), (kw, lib.bpmf_last_error())
    assert call(n_windows=0) == 0                                        # nothing to do: nothing is launched


# ---- the allowance: loose for correct code, sharp against defects ----

DEFECTS = ["alpha 0.05 for 0.15", "asymmetric taper", "delta missing", "conjugate sign", "index wrapped one late",
           "last sample dropped", "bin pair shifted by one", "nearest bin", "> for >= at 0.99 f_max",
           "components summed as moduli", "components summed after interpolation", "row of the next station"]


def model(x, frequencies, taper, multi, defect=None):
    """The device's arithmetic in NumPy: the taper, the DFT pruned to the plan's bins with twiddles from the table at
    (j k) mod n, delta, the modulus, the components, np.interp's formula on the plan's pairs -- with one planted
    defect."""
    n = x.shape[-1]
    plan = pp.fft_spectrum_plan(n, SR, frequencies, taper=taper)
    w = plan["taper"].copy()
    if defect == "alpha 0.05 for 0.15" and np.array_equal(w, pp.tukey_window(n, 0.15)):
        w = pp.tukey_window(n, 0.05)
    if defect == "asymmetric taper":
        w[n // 2:] = 1.0
    if defect == "row of the next station":
        x = np.roll(x, -1, axis=1)
    bad = ~np.isfinite(x).all(axis=-1)
    v = np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * w
    if defect == "last sample dropped":
        v[..., n - 1] = 0.0
    table = np.concatenate([pp.dft_twiddles(n), np.zeros((1, 2))])       # (what lies behind the table: not a twiddle)
    k = plan["bins"].astype(np.int64)
    idx = (np.arange(n, dtype=np.int64)[:, None] * k[None, :]) % n
    if defect == "index wrapped one late":                               # `>` for `>=` in the conditional subtract
        idx = np.where((idx == 0) & (np.arange(n)[:, None] * k[None, :] > 0), n, idx)
    W = table[idx, 0] + (-1j if defect == "conjugate sign" else 1j) * table[idx, 1]
    X = v @ W
    if defect != "delta missing":
        X = X * plan["delta"]
    X[bad] = complex(np.nan, np.nan)
    after = defect == "components summed after interpolation" and frequencies is not None
    if multi and not after:
        fp = np.abs(X).sum(axis=2) if defect == "components summed as moduli" else np.sqrt((np.abs(X) ** 2).sum(axis=2))
    else:
        fp = np.abs(X)
    if frequencies is None:
        return fp if multi else X
    p = plan["pair"].copy()
    if defect == "bin pair shifted by one":
        p = np.minimum(p + 1, len(k) - 2)
    lo, hi = fp[..., p], fp[..., p + 1]
    out = np.where(plan["exact"], lo, ((hi - lo) / plan["span"]) * plan["dx"] + lo)
    if defect == "nearest bin":
        out = np.where(plan["dx"] < 0.5 * plan["span"], lo, hi)
    outside = plan["frequencies"] > 0.99 * plan["freq"].max() if defect == "> for >= at 0.99 f_max" else plan["outside"]
    out[..., outside] = 0.0
    if multi and after:
        out = np.sqrt((out ** 2).sum(axis=2))
    return out


def test_allowance_passes_the_model_and_rejects_every_planted_defect():
    rng = np.random.default_rng(77)
    columns = [(index, None) for index in fc.QUICK] + [(fc.QUICK[0], "array"), (fc.QUICK[6], "array")]
    worst = {d: [] for d in [None] + DEFECTS}
    for index, taper_mode in columns:
        n, key, _ = fc.CASES[index]
        x, f = fc.windows(index), fc.targets(key, n)
        taper = pp.tukey_window(n, 0.15) if taper_mode is None else 0.5 + 0.5 * rng.random(n)
        for d in worst:
            dev = 0.0
            for multi in (False, True):
                want, _ = pp.fft_spectrum_host(x, sr=SR, frequencies=f, taper=taper, multi_component=multi)
                allow = fc.allowance(x, taper, want, multi)
                with np.errstate(all="ignore"):
                    dev = max(dev, fc.deviation(model(x, f, taper, multi, d), want, allow))
            worst[d].append(dev)
    print("columns: " + ", ".join(f"{fc.label(k)}{' taper=' if t else ''}{t or ''}" for k, t in columns))
    for d, row in worst.items():
        print(f"{d or 'no defect':40s} " + " ".join(f"{v:9.2e}" for v in row))
    assert max(worst[None]) <= 0.1, worst[None]                          # correct code: far inside
    for d in DEFECTS:
        assert max(worst[d]) > 1.0, (d, worst[d])
