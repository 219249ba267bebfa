"""GPU: the four entry points that cut rows of day windows (csrc/day_rows.h; DESIGN.md, "Rows of day windows") on the
SAME tiny day and the SAME starts, each against its definition on the host, so that a drift between them shows:
workflow.picker_batch without and with resampling (bpmf_normalize_batch_dev, bpmf_resample_poly_dev: +0.0 outside the
day, bit for bit), workflow.multiband_spectra and workflow.fft_spectra (`valid` exactly; the values under the limit of
tests/test_gpu_multiband.py and within the bound of fft_spectra's docstring, fft_spectrum_cases.allowance).

The session runs with debug.poison_output on (tests/conftest.py): an element that no kernel writes comes back as NaN /
True-from-255 and fails its comparison."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_spectrum_cases as fc  # noqa: E402
import golden_npz  # noqa: E402
import multiband_cases as mc  # noqa: E402
import picker_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

S, C, N, n = 3, 2, 96, 32
W, OVERLAP = 16, 0.5
SR = mc.SAMPLING_RATE
BUFFER_SECONDS = 4 / SR
MB_LIMIT = float(golden_npz.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiband.npz"))["limit"])
# wholly before the day, straddling its start, inside, ending exactly at N, straddling the end, wholly past, the limits
VALUES = [-40, -5, 10, 64, 70, 96, -2**40, 2**40]
FORMS = {"(E,)": np.array(VALUES, dtype=np.int64),
         "(E, S)": np.array([[VALUES[(e + 3 * s) % len(VALUES)] for s in range(S)] for e in range(len(VALUES))],
                            dtype=np.int64)}


@functools.lru_cache(maxsize=None)
def day():
    rng = np.random.default_rng(20261021)
    x = (rng.standard_normal((S, C, N)) * 3.0 + 0.5).astype(np.float32)
    x[1, 0, 20] = np.nan                                     # inside the windows from -5 and from 10 of station 1
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def host(form):
    """The definitions on the host for one form of the starts; computed once and left unchanged."""
    from seismic_bpmf_amd import postprocess as pp
    starts = FORMS[form]
    cut = pp.picker_windows_host(day(), starts, n)
    E = len(starts)
    with np.errstate(invalid="ignore"):
        out = {"cut": cut,
               "picker": pp.normalize_batch_host(cut.reshape(E * S, C, n), W, OVERLAP).reshape(E, S, C, n),
               "resampled": pp.resample_poly_host(cut, 2, 1)}
        out["picker_up"] = pp.normalize_batch_host(out["resampled"].reshape(E * S, C, 2 * n), W,
                                                   OVERLAP).reshape(E, S, C, 2 * n)
        out["windows"], out["valid"] = pp.multiband_windows_host(day(), starts, n)
        out["multiband"], _ = pp.multiband_spectrum_host(out["windows"], mc.ONE_BAND, sr=SR,
                                                         buffer_seconds=BUFFER_SECONDS)
        out["fft"], _ = pp.fft_spectrum_host(out["windows"], sr=SR)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_four_entry_points_cut_the_same_rows(form):
    import torch
    from seismic_bpmf_amd import _lib, postprocess as pp, workflow
    assert _lib.get_option("debug.poison_output")[0] == 1
    starts, want = FORMS[form], host(form)
    E = len(starts)
    d_day = torch.as_tensor(np.array(day()), device="cuda")
    # the premises: every kind of window is there, and a window inside the day holds the NaN
    st = pp.picker_starts(starts, S)
    assert want["valid"].any() and not want["valid"].all() and np.isnan(want["windows"]).any()
    assert np.array_equal(want["valid"], (st >= 0) & (st + n <= N)) and want["valid"][VALUES.index(64), 0]

    got = workflow.picker_batch(d_day, starts, n, normalization_window_sample=W, overlap=OVERLAP, dtype=torch.float64)
    pc.check(got.cpu().numpy(), want["picker"], "picker_batch")          # every bit: +0.0 outside the day, not -0.0
    got = workflow.picker_batch(d_day, starts, n, normalization_window_sample=W, overlap=OVERLAP, dtype=torch.float64,
                                upsampling=2, downsampling=1)
    assert got.shape == (E, S, C, 2 * n)
    pc.check(got.cpu().numpy(), want["picker_up"], "picker_batch(upsampling=2)")
    # the resampled windows themselves: the rows of the day, cut by bpmf_resample_poly_dev
    x = d_day.contiguous()
    got = workflow._resample_rows("picker_batch", x, E * S, torch.as_tensor(st.reshape(-1), device="cuda"), n, 2, 1)
    pc.check(got.cpu().numpy().reshape(E, S, C, 2 * n), want["resampled"], "resampled windows")

    got, _, valid = workflow.multiband_spectra(d_day, starts, n, mc.ONE_BAND, sr=SR, buffer_seconds=BUFFER_SECONDS)
    assert np.array_equal(valid.cpu().numpy(), want["valid"])
    plan = pp.multiband_plan(n, mc.ONE_BAND, SR, BUFFER_SECONDS)
    assert plan["buffer"] == 4 and not plan["skip"].any()
    prepared = pp.multiband_prepare_host(want["windows"].reshape(-1, n), plan["taper"]).reshape(want["windows"].shape)
    dev = mc.deviation(got.cpu().numpy(), want["multiband"], mc.row_scale(want["windows"], prepared), mc.ONE_BAND)
    print(f"{form} multiband: {dev:.2e} ({dev / MB_LIMIT:.3f} of the limit)")
    assert dev <= MB_LIMIT, dev / MB_LIMIT
    outside = got.cpu().numpy()[~want["valid"]]
    assert not outside.any() and not np.signbit(outside).any()                    # exactly +0

    got, _, valid = workflow.fft_spectra(d_day, starts, n, sr=SR, frequencies=None)
    assert np.array_equal(valid.cpu().numpy(), want["valid"])
    got = got.cpu().numpy()
    assert got.shape == want["fft"].shape == (E, S, C, n // 2 + 1) and got.dtype == want["fft"].dtype
    dev = fc.deviation(got, want["fft"], fc.allowance(want["windows"], pp.tukey_window(n, 0.05), want["fft"]))
    print(f"{form} fft: worst err / allowance {dev:.3e}")
    assert dev <= 1.0, dev
    outside = fc.as_reals(got[~want["valid"]])
    assert not outside.any() and not np.signbit(outside).any()


@pytest.mark.parametrize("beyond", [-(2**40 + 1), 2**40 + 1])
def test_starts_beyond_the_limit_are_refused_by_all_four(beyond):
    import torch
    from seismic_bpmf_amd import workflow
    d_day = torch.as_tensor(np.array(day()), device="cuda")
    for starts in (np.array([10, beyond], dtype=np.int64), np.array([[10, 10, beyond]], dtype=np.int64)):
        for call in (lambda: workflow.picker_batch(d_day, starts, n, normalization_window_sample=W, overlap=OVERLAP),
                     lambda: workflow.picker_batch(d_day, starts, n, normalization_window_sample=W, overlap=OVERLAP,
                                                   upsampling=2),
                     lambda: workflow.multiband_spectra(d_day, starts, n, mc.ONE_BAND, sr=SR,
                                                        buffer_seconds=BUFFER_SECONDS),
                     lambda: workflow.fft_spectra(d_day, starts, n, sr=SR)):
            with pytest.raises(ValueError, match=r"within \+-2\^40"):
                call()
