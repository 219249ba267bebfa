"""CPU: the definition of the multi-band spectra (postprocess.multiband_spectrum_host, multiband_windows_host,
spectral_snr_host) against what the reference recorded (tests/golden/multiband.npz, made by
tests/golden/make_multiband_golden.py from BPMF/spectrum.py on duck-typed traces whose detrend / taper / filter are the
SciPy statements obspy documents -- obspy itself was not at hand; tests/test_multiband_obspy_live.py settles that part).

`limit` and `limit_f32` are recorded by the maker: 8 x / 4 x the worst deviation of the definition from the reference on
float64 copies / on the float32 windows themselves, in the measure of multiband_cases.deviation.  The planted defects
show that the case list can tell the definition from its near misses: each must deviate by more than 1000 x limit."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_npz  # noqa: E402
import multiband_cases as mc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

SR = mc.SAMPLING_RATE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiband.npz")
SNR_CASE, SNR_NOISE_EVENTS, SNR_MISSING = 3, [1, 1, 2, 4, 3], (4, 2)        # as the maker has them


@functools.lru_cache(maxsize=None)
def golden():
    return golden_npz.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def definition(index):
    """(windows, spectra, freq, scale) of CASES[index]; computed once."""
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    x, bands = mc.windows(index), mc.BANDS[band_key]
    spectra, freq = pp.multiband_spectrum_host(x, bands, sr=SR, buffer_seconds=buffer_seconds, corners=corners)
    plan = pp.multiband_plan(n, bands, SR, buffer_seconds, corners)
    prepared = pp.multiband_prepare_host(x.reshape(-1, n), plan["taper"]).reshape(x.shape)
    return x, spectra, freq, mc.row_scale(x, prepared)


def station_scale(x, scale):
    """row_scale of a station's components taken together (multi_component)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(scale).any(axis=-1), np.nan, np.nan_to_num(scale).max(axis=-1))


def combine(spectra):
    total = np.zeros(spectra.shape[:2] + spectra.shape[3:])
    for c in range(spectra.shape[2]):
        total += spectra[:, :, c] * spectra[:, :, c]
    return np.sqrt(total)


@pytest.mark.parametrize("index", range(len(mc.CASES)), ids=[c[0] for c in mc.CASES])
def test_definition_equals_the_reference(index):
    g = golden()
    bands = mc.BANDS[mc.CASES[index][4]]
    x, spectra, freq, scale = definition(index)
    dev64 = mc.deviation(spectra, g[f"spectrum_f64_{index}"], scale, bands)
    dev32 = mc.deviation(spectra, g[f"spectrum_f32_{index}"], scale, bands)
    multi = combine(spectra)
    m64 = mc.deviation(multi, g[f"multi_f64_{index}"], station_scale(x, scale), bands)
    m32 = mc.deviation(multi, g[f"multi_f32_{index}"], station_scale(x, scale), bands)
    print(f"{mc.CASES[index][0]}: float64 run {dev64:.2e} / {m64:.2e}, float32 run {dev32:.2e} / {m32:.2e}")
    assert max(dev64, m64) <= float(g["limit"]), (dev64, m64)
    assert max(dev32, m32) <= float(g["limit_f32"]), (dev32, m32)
    assert float(g["limit"]) < 1e-9 and float(g["limit_f32"]) < 1e-4


def test_multi_component_is_the_sum_in_component_order():
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[1]
    x, spectra, _, _ = definition(1)
    multi, _ = pp.multiband_spectrum_host(x, mc.BANDS[band_key], sr=SR, buffer_seconds=buffer_seconds,
                                          corners=corners, multi_component=True)
    assert multi.shape == spectra.shape[:2] + spectra.shape[3:]
    assert np.array_equal(multi, combine(spectra), equal_nan=True)


def test_freq_skipped_bands_and_special_rows():
    g = golden()
    for index in (0, 3, 10):
        x, spectra, freq, _ = definition(index)
        bands = pp.multiband_bands(mc.BANDS[mc.CASES[index][4]])
        assert freq.dtype == np.float32 and np.array_equal(freq, g[f"freq_{index}"])
        assert np.array_equal(freq, (0.5 * (bands[:, 0] + bands[:, 1])).astype(np.float32))
        skip = bands[:, 1] >= SR / 2
        assert skip.any() and not skip.all()
        assert not spectra[..., skip].any() and not np.signbit(spectra[..., skip]).any()
        for row in (mc.ZERO_ROW, mc.CONSTANT_ROW):
            assert not spectra[row].any() and not np.signbit(spectra[row]).any()
        assert np.isnan(spectra[mc.NAN_ROW][~skip]).all() and not spectra[mc.NAN_ROW][skip].any()
        live = mc.live_rows(x)
        assert (spectra[live][:, ~skip] > 0).all()
    octave = pp.multiband_plan(401, mc.OCTAVES, SR, 1.0)
    assert list(octave["skip"]) == [False] * 6 + [True, True]          # hi == sr / 2 exactly is skipped (>=)
    assert (octave["taper"], octave["buffer"]) == (100, 100)
    assert (pp.multiband_plan(1000, mc.OCTAVES, SR, 2.0)["taper"], pp.multiband_plan(257, mc.OCTAVES, SR, 0.01)["taper"],
            pp.multiband_plan(1024, mc.OCTAVES, SR, 2.56)["taper"]) == (200, 1, 256)
    assert pp.multiband_plan(100, mc.OCTAVES, SR, 0.29)["buffer"] == 28        # int(0.29 * 100.0), as Python has it


def test_snr_equals_the_reference_exactly():
    g = golden()
    x, spectra, _, _ = definition(SNR_CASE)
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[SNR_CASE]
    # the recorded SNR is made of the reference's own spectra: feed spectral_snr_host the same
    signal, noise = g[f"spectrum_f64_{SNR_CASE}"], g[f"spectrum_f64_{SNR_CASE}"][SNR_NOISE_EVENTS]
    valid = np.ones(signal.shape[:2], dtype=bool)
    valid[SNR_MISSING] = False
    # (the reference never saw the NaN row: there its noise spectrum is missing, its signal spectrum absent)
    nan_signal = np.isnan(signal)
    noise_valid = np.broadcast_to(valid[:, :, None], signal.shape[:3]) & ~np.isnan(noise).any(axis=-1)
    snr = pp.spectral_snr_host(np.where(nan_signal, 0.0, signal), np.where(np.isnan(noise), 0.0, noise), noise_valid)
    assert np.array_equal(snr, g["snr"])
    assert np.isinf(snr).any() and (snr == 0).any() and (snr[np.isfinite(snr)] > 0).any()
    multi, multi_noise = g[f"multi_f64_{SNR_CASE}"], g[f"multi_f64_{SNR_CASE}"][SNR_NOISE_EVENTS]
    # a station of which one component held the NaN: the reference summed the other two
    keep = ~np.isnan(multi).any(axis=-1) & ~np.isnan(multi_noise).any(axis=-1)
    got = pp.spectral_snr_host(np.nan_to_num(multi), np.nan_to_num(multi_noise), valid)
    assert np.array_equal(got[keep], g["snr_multi"][keep])
    # the definition's own answers: NaN / x = NaN, x / 0 = inf, 0 / 0 = 0, missing noise = 0
    mine = pp.spectral_snr_host(spectra, spectra[SNR_NOISE_EVENTS], valid)
    assert np.isnan(mine[mc.NAN_ROW][:6]).all() and not mine[SNR_MISSING].any()
    assert np.isinf(mine[0, 0, 1, :6]).all() and not mine[mc.ZERO_ROW].any()
    with pytest.raises(ValueError, match="shape"):
        pp.spectral_snr_host(np.zeros((2, 3)), np.zeros((2, 4)))


def test_windows_host():
    rng = np.random.default_rng(5)
    data = rng.standard_normal((3, 2, 50)).astype(np.float32)
    starts = np.array([0, 40, -1, 41, 17], dtype=np.int64)
    windows, valid = pp.multiband_windows_host(data, starts, 10)
    assert windows.shape == (5, 3, 2, 10) and windows.dtype == np.float32 and valid.shape == (5, 3)
    assert list(valid[:, 0]) == [True, True, False, False, True]
    assert np.array_equal(windows[1], data[:, :, 40:50]) and np.array_equal(windows[4], data[:, :, 17:27])
    assert not windows[2].any() and not windows[3].any()
    per_station = np.array([[0, 1, 2], [40, 41, 39]], dtype=np.int64)
    windows, valid = pp.multiband_windows_host(data, per_station, 10)
    assert np.array_equal(valid, [[True, True, True], [True, False, True]])
    assert np.array_equal(windows[0, 2], data[2, :, 2:12]) and not windows[1, 1].any()
    with pytest.raises(ValueError):
        pp.multiband_windows_host(data[0], starts, 10)
    with pytest.raises(ValueError):
        pp.multiband_windows_host(data, starts.astype(np.float64), 10)


@pytest.mark.parametrize("kwargs, match", [
    (dict(buffer_seconds=0.001), "empty"),                              # buf == 0
    (dict(buffer_seconds=2.0), "empty"),                                # n <= 2 buf (400 <= 400)
    (dict(frequency_bands=np.zeros((0, 2))), "frequency bands"),
    (dict(frequency_bands=np.tile([1.0, 2.0], (65, 1))), "frequency bands"),
    (dict(frequency_bands=[1.0, 2.0]), "frequency_bands must be"),
    (dict(corners=0), "corners"),
    (dict(corners=9), "corners"),
    (dict(frequency_bands={"a": [0.0, 2.0]}), "0 < lo < hi"),
    (dict(frequency_bands={"a": [2.0, 2.0]}), "0 < lo < hi"),
    (dict(frequency_bands={"a": [3.0, 2.0]}), "0 < lo < hi"),
    (dict(frequency_bands={"a": [1.0, 50.0 * (1 - 5e-7)]}), "high-pass"),
])
def test_refusals(kwargs, match):
    args = dict(frequency_bands=mc.OCTAVES, sr=SR, buffer_seconds=1.0, corners=4)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        pp.multiband_spectrum_host(np.zeros((2, 400), np.float32), args.pop("frequency_bands"), **args)


def test_a_band_just_clear_of_nyquist_is_served():
    plan = pp.multiband_plan(400, {"a": [20.0, 50.0 * (1 - 2e-6)]}, SR, 1.0)
    assert not plan["skip"][0] and np.isfinite(plan["sos"]).all()


# ---- planted defects: a copy of the definition with one switch each ----
def cascade(sos, x, z=None):
    """postprocess.sosfilt_rows with the state handed in and out."""
    y = np.array(x, dtype=np.float64)
    rows, m = y.shape
    z = np.zeros((sos.shape[0], 2, rows)) if z is None else z.copy()
    coef = [[float(v) for v in row] for row in sos]
    for t in range(m):
        cur = y[:, t].copy()
        for s in range(sos.shape[0]):
            b0, b1, b2, _, a1, a2 = coef[s]
            new = b0 * cur + z[s, 0]
            z[s, 0] = (b1 * cur - a1 * new) + z[s, 1]
            z[s, 1] = b2 * cur - a2 * new
            cur = new
        y[:, t] = cur
    return y, z


def definition_copy(x, band_table, buffer_seconds, corners, defect=None):
    """postprocess.multiband_spectrum_host restated, with one planted defect."""
    n = x.shape[-1]
    bands = pp.multiband_bands(band_table)
    nyq = SR / 2.0
    buf = int(buffer_seconds * SR)
    w = max(0, min(int(0.25 * n), buf) + {"taper + 1": 1, "taper - 1": -1}.get(defect, 0))
    v = np.array(x.reshape(-1, n), dtype=np.float64)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    den = math.fsum(t * t)
    for r in range(len(v)):
        v[r] -= math.fsum(v[r]) / n
        if defect != "no linear detrend":
            slope = math.fsum(v[r] * t) / den if den > 0 else 0.0
            v[r] -= slope * t + math.fsum(v[r]) / n
    if w:
        g = 0.5 * (1.0 - np.cos(np.pi * np.arange(w, dtype=np.float64) / w))
        v[:, :w] *= g
        v[:, n - w:] *= g[::-1]
    out = np.zeros((len(v), len(bands)))
    lo_k, hi_k = buf - (defect == "trim starts early"), n - buf + (defect == "trim ends late")
    for b, (lo, hi) in enumerate(bands):
        if (hi > nyq) if defect == "> in the skip rule" else (hi >= nyq):
            continue
        d = (b + 1) % len(bands) if defect == "band table shifted" else b
        try:
            sos = pp.butter_bandpass_sos(corners, bands[d, 0] / nyq, bands[d, 1] / nyq)
        except ValueError:                                             # (the design refuses what the defect lets through)
            out[:, b] = np.nan
            continue
        y, z = cascade(sos, v)
        if defect != "forward only":
            y = cascade(sos, y[:, ::-1], z if defect == "state carried over" else None)[0][:, ::-1]
        y = y[:, lo_k:hi_k]
        if defect == "max without abs":
            top = np.max(y, axis=1)
        elif defect == "maximum drops NaN":
            top = np.fmax.reduce(np.abs(y), axis=1, initial=0.0)         # (a running fmax from 0, as a kernel would)
        else:
            top = np.max(np.abs(y), axis=1)
        out[:, b] = top / (0.5 * (lo + hi) if defect == "centre frequency" else hi - lo)
    return out.reshape(x.shape[:-1] + (len(bands),))


DEFECTS = ["trim starts early", "trim ends late", "taper + 1", "taper - 1", "no linear detrend", "max without abs",
           "forward only", "state carried over", "band table shifted", "centre frequency", "> in the skip rule",
           "maximum drops NaN"]


def test_the_copy_is_the_definition():
    for index in (0, 2):
        _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
        x, spectra, _, _ = definition(index)
        assert np.array_equal(definition_copy(x, mc.BANDS[band_key], buffer_seconds, corners), spectra, equal_nan=True)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_seen(defect):
    g = golden()
    worst = 0.0
    for index in [0] + mc.QUICK:
        _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
        x, _, _, scale = definition(index)
        with np.errstate(all="ignore"):
            got = definition_copy(x, mc.BANDS[band_key], buffer_seconds, corners, defect)
        worst = max(worst, mc.deviation(got, g[f"spectrum_f64_{index}"], scale, mc.BANDS[band_key]))
        if worst > 1000 * float(g["limit"]):
            break
    print(f"{defect}: {worst:.2e} against 1000 x limit = {1000 * float(g['limit']):.2e}")
    assert worst > 1000 * float(g["limit"]), (defect, worst)
