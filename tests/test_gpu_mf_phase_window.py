"""GPU: the four-phase window of the 4-tile wave kernel (mf_mfma_wave_kernel, NTILE == 4), bit for bit against the oracle.

Sample x of a wave's window sits at plane x & 3, index x >> 2, plane stride PH = 16 (ceil(Ww / 64) | 1) + 2 with
Ww = 1008 + Kpad, and the K loop reads it with 8-byte loads.  The template lengths stand on both sides of every Kpad boundary
(Kpad = 16, 32, 48, 64, 256, 272) and take every stride there is: 17 staging chunks (PH = 274: rounded up from 16 at L = 1,
Kpad = 16, the one length at which Ww / 64 is integral; 17 of themselves at Kpad = 32 .. 64), 19 (PH = 306: rounded up from
18 at L = 128, of themselves at L = 150) and 21 (PH = 338: rounded up from 20 at Kpad = 256 and 272).
Every case: 3 templates on 2 stations x 3 components, N = 2 * 4096 + 1500 + L (two full lag blocks and a partial one, all
four waves of a workgroup at work), moveouts that put windows before sample 0 and past the end of the trace -- the most
negative one of a template is -73, -70 or -71, none of them a multiple of 4 -- a channel without weight and a stretch of
zeros longer than a window."""
import numpy as np
import pytest

from mf_launch import assert_takes

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 16, 17, 18, 33, 49, 128, 150, 241, 242, 256, 257]


def _same(a, b, what):
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        raise AssertionError(f"{what}: {(a != b).sum()} of {a.size} differ, max |diff| "
                             f"{np.abs(a.astype(np.float64) - b).max():.3e}")


def _inputs(L):
    rng = np.random.default_rng(4000 + L)
    T, S, C = 3, 2, 3
    N = 2 * 4096 + 1500 + L
    tp = rng.standard_normal((T, S, C, L)).astype(np.float32)
    mv = rng.integers(-60, 900, (T, S, C)).astype(np.int32)
    mv[0, 0, 0], mv[1, 1, 1], mv[2, 0, 2] = -73, -70, -71
    mv[0, 1, 0], mv[2, 1, 2] = 1499, 1201                   # windows that run past the end of the trace
    w = rng.random((T, S, C)).astype(np.float32)
    w[1, 1, 2] = 0.0
    d = rng.standard_normal((S, C, N)).astype(np.float32)
    d[1, 0, 5000:5000 + L + 40] = 0.0                       # windows without energy
    return tp, mv, w, d, N


@pytest.mark.parametrize("L", LENGTHS)
def test_phase_window_lengths(oracle_lib, hip_opts, L):
    """Steps 1 and 3, the network sum and the per-channel output, both normalisations."""
    from seismic_bpmf_amd import matched_filter
    hip_opts("mf.tiles_per_wave", 4)
    tp, mv, w, d, N = _inputs(L)
    for sqrt_norm in (0, 1):
        hip_opts("mf.compat_sqrt_norm", sqrt_norm)
        for step in (1, 3):
            for ns in (True, False):
                assert_takes(tp.shape, N, step, ns, family="wave", ntile=4, maxr=20)
                if sqrt_norm:
                    with oracle_lib.compat(oracle_lib.COMPAT_SQRT_NORM):
                        want = oracle_lib.matched_filter(tp, mv, w, d, step, ns)
                else:
                    want = oracle_lib.matched_filter(tp, mv, w, d, step, ns)
                _same(matched_filter(tp, mv, w, d, step, check_zeros=False, network_sum=ns), want,
                      f"L={L} step={step} network_sum={ns} sqrt_norm={sqrt_norm}")


@pytest.mark.parametrize("L", [17, 256])
def test_phase_window_without_boundary_priority(oracle_lib, hip_opts, L):
    from seismic_bpmf_amd import matched_filter
    hip_opts("mf.tiles_per_wave", 4)
    hip_opts("mf.boundary_prio", 0)
    tp, mv, w, d, N = _inputs(L)
    assert_takes(tp.shape, N, 1, True, family="wave", ntile=4, maxr=20)
    _same(matched_filter(tp, mv, w, d, 1, check_zeros=False), oracle_lib.matched_filter(tp, mv, w, d, 1),
          f"L={L} boundary_prio=0")


@pytest.mark.parametrize("L", [49, 257])
def test_phase_window_is_refilled_in_place(oracle_lib, hip_opts, L):
    """Two runs on one prepared day: every channel, and every call, rewrites the whole window it reads."""
    from seismic_bpmf_amd import MatchedFilterGPU
    hip_opts("mf.tiles_per_wave", 4)
    tp, mv, w, d, N = _inputs(L)
    want = oracle_lib.matched_filter(tp, mv, w, d, 1)
    eng = MatchedFilterGPU(device=0)
    eng.set_data(d)
    assert_takes(tp.shape, N, 1, True, family="wave", ntile=4, maxr=20)
    _same(eng.run(tp, mv, w, 1).cpu().numpy(), want, f"L={L} first run")
    _same(eng.run(tp[::-1].copy(), mv[::-1].copy(), w[::-1].copy(), 1).cpu().numpy(), want[::-1], f"L={L} other templates")
    _same(eng.run(tp, mv, w, 1).cpu().numpy(), want, f"L={L} second run")
