"""GPU: bpmf_fft_spectrum_dev between guard bands (tests/arena.py), on workspaces of exactly the sizes its sibling
bpmf_fft_spectrum_workspace_size names -- the one-slab size and the 64-row least -- through the checks of
tests/test_gpu_guard_bands.py: the result inside the allowance of fft_spectrum_cases, no byte of any guard changed,
inputs unchanged, the same bits from a workspace of 0xFF bytes and one of 0x00 bytes and from both sizes, and one byte
under the least refused with nothing in the arena changed.

66 rows of n = 130 (two slabs on the least workspace; one window cut by the start of the day, one ending with the day's
last sample, which is the end of the input), with targets, with multi_component and without targets (complex); and 17
rows of the first n above the cut-over, where the twiddles are read from memory and not from LDS."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_spectrum_cases as fc  # noqa: E402
import guard_cases as gc  # noqa: E402
import test_gpu_guard_bands as bands  # noqa: E402

pytestmark = pytest.mark.gpu

SR = fc.SAMPLING_RATE


@functools.lru_cache(maxsize=None)
def inputs(E, S, Cc, n):
    """(day (S, C, N), starts (E, S)): one start -1, one N - n."""
    rng = np.random.default_rng([5100, E * S * Cc, n])
    N = E * n + 40
    day = (1e-6 * rng.standard_normal((S, Cc, N)) + 3e-5 + 2e-5 * rng.uniform(-1, 1, (S, Cc, 1)) * np.arange(N) / N)
    day = day.astype(np.float32)
    starts = 3 + np.arange(E, dtype=np.int64)[:, None] * n + np.arange(S, dtype=np.int64)[None, :]
    starts[0, 0] = -1                                   # cut by the start of the day: not processed
    starts[E - 1, S - 1] = N - n                        # ends with the day's last sample (of the input's last rows)
    return day, starts


def make_call(lib, name, E, S, Cc, n, key, multi):
    from seismic_bpmf_amd import postprocess as pp
    day, starts = inputs(E, S, Cc, n)
    frequencies = fc.targets(key, n)
    plan = pp.fft_spectrum_plan(n, SR, frequencies)
    windows, valid = pp.fft_windows_host(day, starts, n)
    want, _ = pp.fft_spectrum_host(windows, sr=SR, frequencies=frequencies, multi_component=multi)
    allow = fc.allowance(windows, plan["taper"], want, multi)
    K_b, F = len(plan["bins"]), 0 if frequencies is None else len(frequencies)
    rows = E * S * Cc
    one_slab = lib.bpmf_fft_spectrum_workspace_size(rows, n, K_b, F)
    least = lib.bpmf_fft_spectrum_workspace_size(64, n, K_b, F)
    assert 0 < least <= one_slab and (one_slab > least) == (rows > 64)
    arrays = {"day": day, "starts": starts.reshape(-1), "taper": plan["taper"],
              "twiddles": np.ascontiguousarray(pp.dft_twiddles(n)), "bins": plan["bins"]}
    if F:
        arrays.update({k: plan[k] for k in ("pair", "dx", "span", "flags")})

    def invoke(lib, p, nb, stream):
        return lib.bpmf_fft_spectrum_dev(
            p["day"], S, Cc, day.shape[2], E * S, p["starts"], n, p["taper"], p["twiddles"], plan["delta"], p["bins"],
            K_b, p.get("pair"), p.get("dx"), p.get("span"), p.get("flags"), F, int(multi), p["ws"], nb["ws"], stream,
            p["spectra"], p["valid"])

    def verify(out):
        got = out["spectra"].reshape(fc.as_reals(want).shape)
        assert np.array_equal(out["valid"].reshape(valid.shape), valid.astype(np.uint8))
        assert not valid[0, 0] and valid.sum() == valid.size - 1
        assert not got[~valid].any() and not np.signbit(got[~valid]).any()
        dev = fc.deviation(got, fc.as_reals(want), allow)
        assert dev <= 1.0, (name, dev)
        assert (np.abs(got[valid][..., 0]) > 0).all()                   # (im of bin 0 is 0)

    width = (F if F else K_b * (1 if multi else 2))
    shape = (E * S, width) if multi else (E * S, Cc, width)
    return gc.Call(name, "bpmf_fft_spectrum_dev", arrays,
                   {"spectra": (shape, np.float64), "valid": ((E * S,), np.uint8)},
                   invoke, verify, [{"ws": one_slab}, {"ws": least}], {"ws": least - 1})


CALLS = [("66_rows_n130_targets", 11, 2, 3, 130, "log25", False),
         ("66_rows_n130_multi", 11, 2, 3, 130, "log25", True),
         ("66_rows_n130_all_bins", 11, 2, 3, 130, None, False),
         ("17_rows_above_the_table_cut", 17, 1, 1, fc.TABLE_CUT + 1, "log25", False)]


@pytest.mark.parametrize("spec", CALLS, ids=[c[0] for c in CALLS])
def test_between_guard_bands(spec):
    from seismic_bpmf_amd import _lib
    bands.check_call(make_call(_lib.lib(), *spec))
