"""GPU: the FFT-method spectra on the device (csrc/fft_spectrum.hip; workflow.fft_spectra, workflow.spectral_snr)
against the definition on the host (postprocess.fft_spectrum_host of fft_windows_host, itself pinned to the reference
bit for bit in tests/test_fft_spectrum_host.py).

Every value the device returns must lie within fft_spectrum_cases.allowance of the definition:
sqrt(2) B delta + 8 * 2^-53 |want|, B = (n + 16) 2^-53 sum_j |x_j taper_j| -- a bound written down before the kernel
was (n rounded multiply-adds in any order, a twiddle within 2^-52, the definition's own FFT error), about 1e7 times
below the smallest modulus of the cases, and which every planted defect of the host test exceeds.  Where it is 0 or NaN
(a row of zeros, a row with a NaN, n = 2 with its all-zero window) the two must agree exactly.  Every test prints its
worst err / allowance (-rP).

The session runs with debug.poison_output on (tests/conftest.py): both outputs are filled with 0xFF bytes before the
kernels run, so an element that no kernel writes comes back as NaN / True-from-255 and fails its comparison; and the
calls of the main test are the first after allocations that were filled with junk and given back, so the workspace
starts from junk as well."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_spectrum_cases as fc  # noqa: E402
import golden_npz  # noqa: E402

pytestmark = pytest.mark.gpu

SR = fc.SAMPLING_RATE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_spectrum.npz")


@functools.lru_cache(maxsize=None)
def inputs(index):
    """(windows, day, starts) of CASES[index]; computed once and left unchanged."""
    from seismic_bpmf_amd import postprocess as pp
    n = fc.CASES[index][0]
    x = fc.windows(index)
    day, starts = fc.day_of(x)
    cut, valid = pp.fft_windows_host(day, starts, n)
    assert valid.all() and np.array_equal(cut, x, equal_nan=True)
    for a in (x, day, starts):
        a.setflags(write=False)
    return x, day, starts


@functools.lru_cache(maxsize=None)
def host(index, multi=False, alpha=0.05):
    """(want, freq, allowance) of CASES[index] from the definition; computed once and left unchanged."""
    from seismic_bpmf_amd import postprocess as pp
    n, key, _ = fc.CASES[index]
    x = inputs(index)[0]
    want, freq = pp.fft_spectrum_host(x, sr=SR, frequencies=fc.targets(key, n), alpha=alpha, multi_component=multi)
    allow = fc.allowance(x, pp.tukey_window(n, alpha), want, multi)
    for a in (want, freq, allow):
        a.setflags(write=False)
    return want, freq, allow


def junk(n_bytes):
    """Allocations of about the call's size filled with 0xA5 bytes and handed back to the caching allocator."""
    import torch
    for size in (n_bytes, n_bytes // 2, 1 << 20, 1 << 12):
        torch.full((max(int(size), 1),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()


def device(day, starts, n, frequencies=None, **kw):
    import torch
    from seismic_bpmf_amd import workflow
    day = day if isinstance(day, torch.Tensor) else torch.as_tensor(np.array(day), device="cuda")
    spectra, freq, valid = workflow.fft_spectra(day, starts, n, sr=SR, frequencies=frequencies, **kw)
    assert spectra.is_cuda and freq.is_cuda and valid.is_cuda and freq.dtype == torch.float64
    assert valid.dtype == torch.bool
    complex_out = frequencies is None and not kw.get("multi_component")
    assert spectra.dtype == (torch.complex128 if complex_out else torch.float64)
    return spectra.cpu().numpy(), freq.cpu().numpy(), valid.cpu().numpy()


def least_workspace(index):
    from seismic_bpmf_amd import _lib, postprocess as pp
    n, key, _ = fc.CASES[index]
    f = fc.targets(key, n)
    return int(_lib.lib().bpmf_fft_spectrum_workspace_size(64, n, len(pp.fft_spectrum_plan(n, SR, f)["bins"]),
                                                            0 if f is None else len(f)))


def run_case(index, **kw):
    n, key, _ = fc.CASES[index]
    _, day, starts = inputs(index)
    return device(day, starts, n, fc.targets(key, n), **kw)


def check_special_rows(index, got, multi):
    from seismic_bpmf_amd import postprocess as pp
    n, key, shape = fc.CASES[index]
    if shape not in (fc.SMALL, fc.LARGE):
        return
    zero = np.zeros(got.shape[-1], bool) if key is None else pp.fft_spectrum_plan(n, SR, fc.targets(key, n))["outside"]
    nan = got[fc.NAN_ROW[:2]] if multi else got[fc.NAN_ROW]
    assert np.isnan(fc.as_reals(nan[~zero])).all()
    assert not got[..., zero].any() and not np.signbit(fc.as_reals(got[..., zero])).any()      # exactly +0
    if not multi:
        assert not got[fc.ZERO_ROW].any()


# every length, target set and row count of the issue; 195 rows on the least workspace: four slabs
@pytest.mark.parametrize("index", range(len(fc.CASES)), ids=[fc.label(k) for k in range(len(fc.CASES))])
def test_device_equals_the_definition(index):
    n, key, shape = fc.CASES[index]
    x = inputs(index)[0]
    want, want_freq, allow = host(index)
    kw = dict(workspace_bytes=least_workspace(index)) if shape == fc.LARGE else {}
    junk(want.nbytes + least_workspace(index) * (x[..., 0].size // 64 + 1))
    got, freq, valid = run_case(index, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype and valid.shape == x.shape[:2] and valid.all()
    assert np.array_equal(freq, want_freq)
    dev = fc.deviation(got, want, allow)
    print(f"{fc.label(index)}: worst err / allowance {dev:.3e}")
    assert dev <= 1.0, dev
    check_special_rows(index, got, False)


MULTI = list(range(len(fc.CASES)))             # every case again with multi_component


@pytest.mark.parametrize("index", MULTI, ids=[fc.label(k) for k in MULTI])
def test_multi_component(index):
    n, key, shape = fc.CASES[index]
    want, _, allow = host(index, True)
    kw = dict(workspace_bytes=least_workspace(index)) if shape == fc.LARGE else {}   # 63 rows = 21 windows per slab
    got, _, valid = run_case(index, multi_component=True, **kw)
    assert got.shape == want.shape == shape[:2] + want.shape[-1:] and valid.all()
    dev = fc.deviation(got, want, allow)
    print(f"{fc.label(index)} multi: worst err / allowance {dev:.3e}")
    assert dev <= 1.0, dev
    check_special_rows(index, got, True)


def test_window_edges_and_both_forms_of_starts():
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(11)
    S, C, N, n = 3, 2, 300, 64
    day = (1e-6 * rng.standard_normal((S, C, N)) + 3e-5).astype(np.float32)
    f = fc.targets("log25", n)
    flat = np.array([0, N - n, -1, N - n + 1, 50, -n, N, -5000, 5000], dtype=np.int64)             # (E,)
    per_station = np.array([[0, -1, N - n], [N - n + 1, 7, N - n], [3, 4, -5]], dtype=np.int64)      # (E, S)
    worst = 0.0
    for starts in (flat, per_station):
        for frequencies in (f, None):
            for multi in (False, True):
                windows, want_valid = pp.fft_windows_host(day, starts, n)
                want, _ = pp.fft_spectrum_host(windows, sr=SR, frequencies=frequencies, multi_component=multi)
                got, _, valid = device(day, starts, n, frequencies, multi_component=multi)
                assert np.array_equal(valid, want_valid) and not want_valid.all() and want_valid.any()
                assert not got[~valid].any() and not np.signbit(fc.as_reals(got[~valid])).any()
                worst = max(worst, fc.deviation(got, want, fc.allowance(windows, pp.tukey_window(n, 0.05), want, multi)))
                assert (np.abs(got[valid][..., :3]) > 0).all()               # the neighbours are untouched
    print(f"window edges: worst err / allowance {worst:.3e}")
    assert worst <= 1.0
    assert list(device(day, flat, n, f)[2][:, 0]) == [True, True, False, False, True, False, False, False, False]
    empty, freq, valid = device(day, np.zeros((0,), np.int64), n, f)
    assert empty.shape == (0, S, C, 25) and valid.shape == (0, S) and freq.shape == (25,)


def test_slabs_batches_orders_and_repeats_give_the_same_bits():
    import torch
    index = fc.LARGE_CASE
    n, key, (E, S, C) = fc.CASES[index]
    _, day, starts = inputs(index)
    for frequencies in (fc.targets(key, n), None):
        for multi in (False, True):
            kw = dict(multi_component=multi)
            ample, _, _ = device(day, starts, n, frequencies, **kw)
            assert np.array_equal(device(day, starts, n, frequencies, **kw)[0], ample, equal_nan=True)   # twice
            from seismic_bpmf_amd import _lib, postprocess as pp
            bins = len(pp.fft_spectrum_plan(n, SR, frequencies)["bins"])
            least = int(_lib.lib().bpmf_fft_spectrum_workspace_size(64, n, bins,
                                                                     0 if frequencies is None else len(frequencies)))
            for size in (least, least + 100, 2 * least + 17):
                slabs, _, valid = device(day, starts, n, frequencies, workspace_bytes=size, **kw)
                assert E * S * C == 195 and valid.all()
                assert np.array_equal(slabs, ample, equal_nan=True), size
            order = np.random.default_rng(5).permutation(E)
            shuffled, _, _ = device(day, starts[order], n, frequencies, **kw)
            assert np.array_equal(shuffled, ample[order], equal_nan=True)
            d_day = torch.as_tensor(np.array(day), device="cuda")
            for e, s, c in ((0, 0, 0), (6, 2, 1), (12, 4, 2), (4, 1, 1)):     # rows 0, 97, 194 and 64 of the batch
                if multi:
                    alone, _, _ = device(d_day[s:s + 1], starts[e:e + 1, s:s + 1], n, frequencies, **kw)
                    assert np.array_equal(alone[0, 0], ample[e, s], equal_nan=True), (e, s)
                else:
                    alone, _, _ = device(d_day[s:s + 1, c:c + 1], starts[e:e + 1, s:s + 1], n, frequencies, **kw)
                    assert np.array_equal(alone[0, 0, 0], ample[e, s, c], equal_nan=True), (e, s, c)


def test_taper_as_an_array_and_another_alpha():
    from seismic_bpmf_amd import postprocess as pp
    index = fc.CASES.index((257, "log25", fc.SMALL))
    n, key, _ = fc.CASES[index]
    x, day, starts = inputs(index)
    own = 0.5 + 0.5 * np.random.default_rng(9).random(n)                   # no zero at either end
    worst = 0.0
    for frequencies in (fc.targets(key, n), None):
        for kw, taper in ((dict(taper=own), own), (dict(alpha=0.15), pp.tukey_window(n, 0.15))):
            want, _ = pp.fft_spectrum_host(x, sr=SR, frequencies=frequencies, **kw)
            got, _, _ = device(day, starts, n, frequencies, **kw)
            worst = max(worst, fc.deviation(got, want, fc.allowance(x, taper, want)))
    print(f"taper array / alpha 0.15: worst err / allowance {worst:.3e}")
    assert worst <= 1.0
    assert not np.array_equal(device(day, starts, n, None, taper=own)[0], run_case(index)[0], equal_nan=True)


def test_other_days_go_through_as_float32():
    import torch
    index = fc.CASES.index((257, "log25", fc.SMALL))
    n, key, _ = fc.CASES[index]
    _, day, starts = inputs(index)
    f = fc.targets(key, n)
    plain, _, _ = run_case(index)
    wide = torch.full(day.shape[:2] + (2 * day.shape[2],), 7.0, dtype=torch.float32, device="cuda")
    wide[:, :, ::2] = torch.as_tensor(np.array(day), device="cuda")
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    assert np.array_equal(device(strided, starts, n, f)[0], plain, equal_nan=True)
    double = torch.as_tensor(np.array(day), device="cuda").double() * (1.0 + 2.0 ** -40)   # rounds back to the float32
    assert np.array_equal(device(double, starts, n, f)[0], plain, equal_nan=True)
    as_tensor = torch.as_tensor(np.array(starts), device="cuda")
    assert np.array_equal(device(day, as_tensor, n, f)[0], plain, equal_nan=True)


def test_inf_rows_are_nan_too():
    index = fc.CASES.index((64, "log25", fc.SMALL))
    n, key, _ = fc.CASES[index]
    x = fc.windows(index)
    x[0, 0, 0, 0], x[0, 1, 1, n - 1], x[4, 2, 2, 5] = np.inf, -np.inf, np.inf     # (the ends are zeroed by the taper)
    day, starts = fc.day_of(x)
    from seismic_bpmf_amd import postprocess as pp
    for frequencies in (fc.targets(key, n), None):
        want, _ = pp.fft_spectrum_host(x, sr=SR, frequencies=frequencies)
        got, _, _ = device(day, starts, n, frequencies)
        assert fc.deviation(got, want, fc.allowance(x, pp.tukey_window(n, 0.05), want)) <= 1.0
        for row in ((0, 0, 0), (0, 1, 1), (4, 2, 2), fc.NAN_ROW):
            assert np.isnan(fc.as_reals(got[row][:3])).all(), row


def test_spectral_snr_against_the_recorded_one():
    import torch
    from seismic_bpmf_amd import workflow
    assert workflow.spectral_snr is workflow.multiband_snr
    golden = golden_npz.load(GOLDEN)
    index = fc.SNR_CASE
    n, key, (E, S, C) = fc.CASES[index]
    _, day, starts = inputs(index)
    valid = np.ones((E, S), dtype=bool)
    valid[fc.SNR_MISSING] = False
    d_day = torch.as_tensor(np.array(day), device="cuda")
    for multi in (False, True):
        signal = workflow.fft_spectra(d_day, starts, n, sr=SR, frequencies=fc.targets(key, n), multi_component=multi)[0]
        noise = signal[torch.as_tensor(fc.SNR_NOISE_EVENTS, device="cuda")]
        got = workflow.spectral_snr(signal, noise, torch.as_tensor(valid, device="cuda"))
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == signal.shape
        got, want = got.cpu().numpy(), golden["snr_multi" if multi else "snr"]
        # a ratio of two values, each inside its allowance: the relative errors add (and one rounding of the division)
        spectrum, _, allow = host(index, multi)
        with np.errstate(all="ignore"):
            relative = allow / np.abs(spectrum)
            bound = np.abs(want) * (1.01 * (relative + relative[fc.SNR_NOISE_EVENTS]) + 2.0 ** -52)
        bound[~np.isfinite(want) | (want == 0)] = 0.0                    # 0, inf and NaN: exactly
        dev = fc.deviation(got, want, bound)
        print(f"snr {'multi' if multi else 'single'}: worst err / allowance {dev:.3e}")
        assert dev <= 1.0
        assert np.isnan(want).any() and (want == 0).any() and not got[fc.SNR_MISSING].any()


def test_sample_limits():
    day = np.zeros((1, 1, 20000), np.float32)
    for n in (1, 16385):
        with pytest.raises(ValueError, match="2 .. 16384"):
            device(day, np.zeros((1,), np.int64), n, fc.targets("log25", 64))
    got, _, valid = device(day, np.array([3616], np.int64), 16384, fc.targets("log25", 16384))
    assert valid.all() and not got.any()


def test_refusals_come_before_the_library(monkeypatch):
    import torch
    from seismic_bpmf_amd import _lib, workflow

    class SizesOnly:       # the workspace refusal asks the library's pure size function for a row's bytes; nothing else
        bpmf_fft_spectrum_workspace_size = staticmethod(_lib.lib().bpmf_fft_spectrum_workspace_size)

        def __getattr__(self, name):
            raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", SizesOnly)
    day = torch.zeros((2, 3, 500), dtype=torch.float32, device="cuda")
    starts = np.zeros((4,), np.int64)
    good = dict(data_dev=day, starts=starts, n_samples=400, sr=SR, frequencies=fc.targets("log25", 400))
    with pytest.raises(AssertionError, match="library was reached"):
        workflow.fft_spectra(**good)                                    # (what is not refused does reach it)
    for change, match in [
            (dict(data_dev=day.cpu()), "on the GPU"),
            (dict(data_dev=np.zeros((2, 3, 500), np.float32)), "on the GPU"),
            (dict(data_dev=day[0]), r"\(S, C, N\)"),
            (dict(n_samples=16385), "2 .. 16384"),
            (dict(n_samples=1), "2 .. 16384"),
            (dict(sr=0.0), "sr > 0"),
            (dict(alpha=1.0), "alpha"),
            (dict(taper=np.ones(399)), "taper"),
            (dict(frequencies=np.ones(1025)), "frequencies"),
            (dict(frequencies=np.zeros(0)), "frequencies"),
            (dict(frequencies=np.array([1.0, np.nan])), "frequencies"),
            (dict(data_dev=torch.zeros((1, 65, 500), device="cuda"), multi_component=True), "64 components"),
            (dict(data_dev=day[:1, :1], starts=np.broadcast_to(np.int64(0), (2 ** 22,)),
                  frequencies=np.linspace(1.0, 40.0, 1024)), r"2\^31"),
            (dict(workspace_bytes=1000), "workspace_bytes"),
            (dict(starts=np.zeros((4, 3), np.int64)), "starts"),
    ]:
        with pytest.raises(ValueError, match=match):
            workflow.fft_spectra(**{**good, **change})
