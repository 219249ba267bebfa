"""GPU: the multi-band spectra on the device (csrc/spectrum.hip; workflow.multiband_spectra, workflow.multiband_snr)
against the definition on the host (postprocess.multiband_spectrum_host of multiband_windows_host, itself pinned to the
reference in tests/test_multiband_host.py).

The limit is the recorded one (tests/golden/multiband.npz: 8 x the worst deviation of the definition from the reference's
float64 run), in the measure of multiband_cases.deviation -- the error relative to the largest sample that went into
the filter.  The device and the definition run the same cascade in the same operation order; what differs is the last
bit of the mean, the slope and the cosine, which is what the reference's own least-squares detrend differs by too.
The zero row, the constant row and the skipped bands must be exactly +0, the live bands of the NaN row NaN.

The session runs with debug.poison_output on (tests/conftest.py): both outputs are filled with 0xFF bytes before the
kernels run, so an element that no kernel writes comes back as NaN / True-from-255 and fails its comparison."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_npz  # noqa: E402
import multiband_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SR = mc.SAMPLING_RATE
LIMIT = float(golden_npz.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiband.npz"))["limit"])
LARGE_CASE = 12
SNR_NOISE_EVENTS, SNR_MISSING = [1, 1, 2, 4, 3], (4, 2)


@functools.lru_cache(maxsize=None)
def host(index):
    """(windows, day, starts, spectra, scale) of CASES[index] on the host; computed once and left unchanged."""
    from seismic_bpmf_amd import postprocess as pp
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    x, bands = mc.windows(index), mc.BANDS[band_key]
    day, starts = mc.day_of(x)
    cut, valid = pp.multiband_windows_host(day, starts, n)
    assert valid.all() and np.array_equal(cut, x, equal_nan=True)
    spectra, freq = pp.multiband_spectrum_host(x, bands, sr=SR, buffer_seconds=buffer_seconds, corners=corners)
    plan = pp.multiband_plan(n, bands, SR, buffer_seconds, corners)
    prepared = pp.multiband_prepare_host(x.reshape(-1, n), plan["taper"]).reshape(x.shape)
    for a in (x, day, starts, spectra, freq, prepared):
        a.setflags(write=False)
    return x, day, starts, spectra, freq, mc.row_scale(x, prepared), prepared


def device(day, starts, n, bands, **kw):
    import torch
    from seismic_bpmf_amd import workflow
    day = day if isinstance(day, torch.Tensor) else torch.as_tensor(np.array(day), device="cuda")
    spectra, freq, valid = workflow.multiband_spectra(day, starts, n, bands, sr=SR, **kw)
    assert spectra.is_cuda and freq.is_cuda and valid.is_cuda
    assert spectra.dtype == torch.float64 and freq.dtype == torch.float32 and valid.dtype == torch.bool
    return spectra.cpu().numpy(), freq.cpu().numpy(), valid.cpu().numpy()


def run_case(index, **kw):
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    _, day, starts, _, _, _, _ = host(index)
    return device(day, starts, n, mc.BANDS[band_key], buffer_seconds=buffer_seconds, corners=corners, **kw)


def check_special_rows(index, got):
    from seismic_bpmf_amd import postprocess as pp
    bands = pp.multiband_bands(mc.BANDS[mc.CASES[index][4]])
    skip = bands[:, 1] >= SR / 2
    for part in (got[..., skip], got[mc.ZERO_ROW], got[mc.CONSTANT_ROW]):
        assert not part.any() and not np.signbit(part).any()                      # exactly +0
    assert np.isnan(got[mc.NAN_ROW][~skip]).all()


# every length of the issue at 45 rows, corners 2 / 4 / 8, B = 1 / 8 / 64, and 195 rows
@pytest.mark.parametrize("index", range(len(mc.CASES)), ids=[c[0] for c in mc.CASES])
def test_device_equals_the_definition(index):
    x, _, _, want, want_freq, scale, _ = host(index)
    got, freq, valid = run_case(index)
    assert got.shape == want.shape and valid.shape == x.shape[:2] and valid.all()
    assert np.array_equal(freq, want_freq)
    dev = mc.deviation(got, want, scale, mc.BANDS[mc.CASES[index][4]])
    print(f"{mc.CASES[index][0]}: {dev:.2e} ({dev / LIMIT:.3f} of the limit)")
    assert dev <= LIMIT, dev / LIMIT
    check_special_rows(index, got)


@pytest.mark.parametrize("index", [1, 3, 10])
def test_multi_component(index):
    from seismic_bpmf_amd import postprocess as pp
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    x, _, _, _, _, scale, _ = host(index)
    want, _ = pp.multiband_spectrum_host(x, mc.BANDS[band_key], sr=SR, buffer_seconds=buffer_seconds,
                                         corners=corners, multi_component=True)
    got, _, _ = run_case(index, multi_component=True)
    assert got.shape == want.shape == x.shape[:2] + (len(mc.BANDS[band_key]),)
    with np.errstate(invalid="ignore"):
        station = np.where(np.isnan(scale).any(axis=-1), np.nan, np.nan_to_num(scale).max(axis=-1))
    dev = mc.deviation(got, want, station, mc.BANDS[band_key])
    assert dev <= LIMIT, dev / LIMIT


def test_window_edges_and_both_forms_of_starts():
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(11)
    S, C, N, n = 3, 2, 300, 64
    day = (1e-6 * rng.standard_normal((S, C, N)) + 3e-5).astype(np.float32)
    kw = dict(buffer_seconds=0.1, corners=4)
    flat = np.array([0, N - n, -1, N - n + 1, 50, -n, N], dtype=np.int64)              # (E,)
    per_station = np.array([[0, -1, N - n], [N - n + 1, 7, N - n], [3, 4, -5]], dtype=np.int64)   # (E, S)
    for starts in (flat, per_station):
        windows, want_valid = pp.multiband_windows_host(day, starts, n)
        want, _ = pp.multiband_spectrum_host(windows, mc.OCTAVES, sr=SR, **kw)
        got, _, valid = device(day, starts, n, mc.OCTAVES, **kw)
        assert np.array_equal(valid, want_valid) and not want_valid.all() and want_valid.any()
        assert not got[~valid].any() and not np.signbit(got[~valid]).any()
        plan = pp.multiband_plan(n, mc.OCTAVES, SR, 0.1)
        prepared = pp.multiband_prepare_host(windows.reshape(-1, n), plan["taper"]).reshape(windows.shape)
        dev = mc.deviation(got, want, mc.row_scale(windows, prepared), mc.OCTAVES)
        assert dev <= LIMIT, dev / LIMIT
        assert (got[valid][:, :, :6] > 0).all()                                   # the neighbours are untouched
    assert list(device(day, flat, n, mc.OCTAVES, **kw)[2][:, 0]) == [True, True, False, False, True, False, False]
    empty, freq, valid = device(day, np.zeros((0,), np.int64), n, mc.OCTAVES, **kw)
    assert empty.shape == (0, S, C, 8) and valid.shape == (0, S) and freq.shape == (8,)


def test_other_days_go_through_as_picker_batch_takes_them():
    import torch
    index = 3
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    _, day, starts, _, _, _, _ = host(index)
    plain, _, _ = run_case(index)
    kw = dict(buffer_seconds=buffer_seconds, corners=corners)
    wide = torch.full(day.shape[:2] + (2 * day.shape[2],), 7.0, dtype=torch.float32, device="cuda")
    wide[:, :, ::2] = torch.as_tensor(day, device="cuda")
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    assert np.array_equal(device(strided, starts, n, mc.BANDS[band_key], **kw)[0], plain, equal_nan=True)
    double = torch.as_tensor(day, device="cuda").double()
    assert np.array_equal(device(double, starts, n, mc.BANDS[band_key], **kw)[0], plain, equal_nan=True)
    as_tensor = torch.as_tensor(starts, device="cuda")
    assert np.array_equal(device(day, as_tensor, n, mc.BANDS[band_key], **kw)[0], plain, equal_nan=True)


def test_slabs_batches_and_repeats_give_the_same_bits():
    import torch
    _, n, buffer_seconds, corners, band_key, (E, S, C) = mc.CASES[LARGE_CASE]
    _, day, starts, _, _, _, _ = host(LARGE_CASE)
    one_slab, _, _ = run_case(LARGE_CASE)
    assert np.array_equal(run_case(LARGE_CASE)[0], one_slab, equal_nan=True)     # two identical calls
    row_bytes = (4 + (1 + 6) * n) * 8                                             # six active bands
    four_slabs, _, valid = run_case(LARGE_CASE, workspace_bytes=64 * row_bytes + 100)
    assert E * S * C == 195 and valid.all()
    assert np.array_equal(four_slabs, one_slab, equal_nan=True)
    d_day = torch.as_tensor(day, device="cuda")
    kw = dict(buffer_seconds=buffer_seconds, corners=corners)
    for e, s, c in ((0, 0, 0), (6, 2, 1), (12, 4, 2), (4, 1, 1)):                 # rows 0, 97, 194 and 64 of the batch
        alone, _, _ = device(d_day[s:s + 1, c:c + 1], starts[e:e + 1, s:s + 1], n, mc.BANDS[band_key], **kw)
        assert np.array_equal(alone[0, 0, 0], one_slab[e, s, c], equal_nan=True), (e, s, c)


def test_the_cascade_is_the_anchored_one():
    """workflow.bandpass_filter (bit for bit SciPy's sosfilt, tests/test_gpu_svdwf.py) on the definition's prepared
    rows, trimmed and maximised on the host, against the fused call."""
    import torch
    from seismic_bpmf_amd import postprocess as pp, workflow
    index = 3
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    x, _, _, _, _, scale, prepared = host(index)
    got, _, _ = run_case(index)
    plan = pp.multiband_plan(n, mc.BANDS[band_key], SR, buffer_seconds, corners)
    rows = torch.as_tensor(np.nan_to_num(prepared), device="cuda")
    composed = np.zeros_like(got)
    for b in np.flatnonzero(~plan["skip"]):
        y = workflow.bandpass_filter(rows, plan["sos"][b], detrend=False, taper_alpha=None).cpu().numpy()
        composed[..., b] = np.abs(y[..., plan["buffer"]:n - plan["buffer"]]).max(axis=-1) / plan["bandwidth"][b]
    live = mc.live_rows(x)
    dev = mc.deviation(got[live], composed[live], scale[live], mc.BANDS[band_key])
    assert dev <= LIMIT, dev / LIMIT


def test_sample_cap():
    with pytest.raises(ValueError, match="16384"):
        device(np.zeros((1, 1, 20000), np.float32), np.zeros((1,), np.int64), 16385, mc.OCTAVES, buffer_seconds=1.0)
    got, _, valid = device(np.zeros((1, 1, 20000), np.float32), np.array([3616], np.int64), 16384, mc.ONE_BAND,
                           buffer_seconds=1.0)
    assert valid.all() and not got.any()


def test_refusals_come_before_the_library(monkeypatch):
    import torch
    from seismic_bpmf_amd import _lib, workflow

    class SizesOnly:       # the workspace refusal asks the library's pure size function for a row's bytes; nothing else
        bpmf_multiband_workspace_bytes = staticmethod(_lib.lib().bpmf_multiband_workspace_bytes)

        def __getattr__(self, name):
            raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", SizesOnly)
    day = torch.zeros((2, 3, 500), dtype=torch.float32, device="cuda")
    starts = np.zeros((4,), np.int64)
    good = dict(data_dev=day, starts=starts, n_samples=400, frequency_bands=mc.OCTAVES, sr=SR, buffer_seconds=1.0)
    with pytest.raises(AssertionError, match="library was reached"):
        workflow.multiband_spectra(**good)                              # (what is not refused does reach it)
    for change, match in [
            (dict(data_dev=day.cpu()), "on the GPU"),
            (dict(data_dev=np.zeros((2, 3, 500), np.float32)), "on the GPU"),
            (dict(data_dev=day[0]), r"\(S, C, N\)"),
            (dict(n_samples=16385), "16384"),
            (dict(buffer_seconds=0.001), "empty"),
            (dict(buffer_seconds=2.0), "empty"),
            (dict(frequency_bands=np.zeros((0, 2))), "frequency bands"),
            (dict(frequency_bands=np.tile([1.0, 2.0], (65, 1))), "frequency bands"),
            (dict(corners=0), "corners"),
            (dict(corners=9), "corners"),
            (dict(frequency_bands={"a": [0.0, 1.0]}), "0 < lo < hi"),
            (dict(frequency_bands={"a": [2.0, 1.0]}), "0 < lo < hi"),
            (dict(frequency_bands={"a": [1.0, 50.0 * (1 - 5e-7)]}), "high-pass"),
            (dict(data_dev=day[:1, :1], starts=np.broadcast_to(np.int64(0), (2 ** 25,)),
                  frequency_bands=mc.MANY_BANDS), r"2\^31"),
            (dict(workspace_bytes=1000), "workspace_bytes"),
            (dict(starts=np.zeros((4, 3), np.int64)), "starts"),
    ]:
        with pytest.raises(ValueError, match=match):
            workflow.multiband_spectra(**{**good, **change})


def test_snr_equals_its_definition_exactly():
    import torch
    from seismic_bpmf_amd import postprocess as pp, workflow
    index = 3
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    _, day, starts, _, _, _, _ = host(index)
    kw = dict(sr=SR, buffer_seconds=buffer_seconds, corners=corners)
    d_day = torch.as_tensor(day, device="cuda")
    valid = np.ones(starts.shape, dtype=bool)
    valid[SNR_MISSING] = False
    for multi in (False, True):
        signal = workflow.multiband_spectra(d_day, starts, n, mc.BANDS[band_key], multi_component=multi, **kw)[0]
        noise = signal[torch.as_tensor(SNR_NOISE_EVENTS, device="cuda")]
        got = workflow.multiband_snr(signal, noise, torch.as_tensor(valid, device="cuda"))
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == signal.shape
        want = pp.spectral_snr_host(signal.cpu().numpy(), noise.cpu().numpy(), valid)
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
        assert np.isinf(want).any() == (not multi) and np.isnan(want).any() and not want[SNR_MISSING].any()
        free = workflow.multiband_snr(signal, noise).cpu().numpy()
        assert np.array_equal(free, pp.spectral_snr_host(signal.cpu().numpy(), noise.cpu().numpy()), equal_nan=True)
