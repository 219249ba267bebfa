"""CPU: the host definition of the polyphase resampling (postprocess.resample_poly_host / resample_poly_plan) against
scipy.signal.resample_poly -- live where SciPy is installed, and through its answers recorded in
tests/golden/resample.npz by tests/golden/make_resample_golden.py everywhere; the float32 taps against firwin; the
power of the cases of tests/resample_cases.py to reject planted defects; every refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picker_cases as pc  # noqa: E402
import resample_cases as rc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "resample.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def host():
    """resample_poly_host of every case, computed once: {(up, down, n): (12, n_out) float32}."""
    return {(up, down, n): pp.resample_poly_host(rc.rows(n), up, down) for up, down, n in rc.cases()}


def test_the_cases_are_those_of_the_issue():
    assert len(rc.FACTORS) == 12 and len(rc.cases()) == 12 * 8
    for up, down in rc.FACTORS:
        hp = rc.taps_per_phase(up, down)
        assert set(rc.lengths(up, down)) == {1, 2, 3, hp - 1, hp, hp + 1, 257, 3000}
    x = rc.rows(257)
    assert x.shape == (12, 257) and x.dtype == np.float32
    assert not x[9].any() and np.signbit(x[10]).sum() > 128 and (x[10] == 0).sum() > 128
    assert np.flatnonzero(np.isnan(x)).tolist() == [11 * 257 + 128]
    assert pp.resample_poly_factors(8, 2) == (4, 1) and pp.resample_poly_factors(4, 6) == (2, 3)
    assert pp.resample_poly_factors(3, 3) == (1, 1)


@pytest.mark.parametrize("up,down", rc.FACTORS)
def test_resample_poly_host_equals_scipy_live(host, up, down):
    signal = pytest.importorskip("scipy.signal")
    for n in rc.lengths(up, down):
        x = rc.rows(n)
        with np.errstate(all="ignore"):
            want = signal.resample_poly(x, up, down, axis=-1)
        got = host[up, down, n]
        assert got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(want)), (up, down, n)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], want.view(np.uint32)[~np.isnan(want)]), (up, down, n)
        pc.check(got, want, f"up {up} down {down} n {n}")
        if n == 3000:                                                # the NaN spreads over a part of its row only
            assert np.isnan(want[11]).any() and not np.isnan(want[11]).all() and not np.isnan(want[:11]).any()


@pytest.mark.parametrize("up,down", rc.FACTORS)
def test_resample_poly_host_equals_the_recorded_answers(golden, host, up, down):
    for n in rc.lengths(up, down):
        got = host[up, down, n]
        rows, samples = rc.golden_selection(got.shape[-1])
        pc.check(got[np.ix_(rows, samples)], golden[rc.golden_key(up, down, n)], f"up {up} down {down} n {n}")
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_a_copy_and_leading_axes(host):
    x = rc.rows(257)
    got = pp.resample_poly_host(x, 3, 3)
    assert got is not x and not np.shares_memory(got, x) and pc.same_bits(got, x)
    pc.check(pp.resample_poly_host(x.reshape(2, 3, 2, 257), 5, 2), host[5, 2, 257].reshape(2, 3, 2, -1), "4-D")
    pc.check(pp.resample_poly_host(x[3], 5, 2), host[5, 2, 257][3], "1-D")
    pc.check(pp.resample_poly_host(x, 8, 2), host[4, 1, 257], "reduced factors")
    pc.check(pp.resample_poly_host(x, np.int64(4), 1.0), host[4, 1, 257], "integer-valued factors of other types")


def test_the_plan():
    h, n_out, n_pre_pad, n_pre_remove, n_post_pad, table = pp.resample_poly_plan(3000, 4, 1)
    assert (len(h), n_out, n_pre_pad, n_pre_remove, n_post_pad, len(table)) == (81, 12000, 1, 41, 0, 84)
    assert h.dtype == np.float32 and table.dtype == np.float32
    assert pc.same_bits(table[1:82], h) and not table[0] and not table[82:].any()
    h, n_out, n_pre_pad, n_pre_remove, n_post_pad, table = pp.resample_poly_plan(3000, 2, 5)
    assert (len(h), n_out, n_pre_pad, n_pre_remove, len(table)) == (101, 1200, 5, 11, 106 + n_post_pad)
    for up, down, n in rc.cases():                                  # the plan's own inequality, and the smallest pad
        u, d = pp.resample_poly_factors(up, down)
        h, n_out, n_pre_pad, n_pre_remove, n_post_pad, table = pp.resample_poly_plan(n, up, down)
        length = len(h) + n_pre_pad + n_post_pad
        assert n_out == -(-n * u // d) and len(table) == -(-length // u) * u
        assert ((n - 1) * u + length - 1) // d + 1 >= n_out + n_pre_remove
        assert n_post_pad == 0 or ((n - 1) * u + length - 2) // d + 1 < n_out + n_pre_remove


def test_float32_taps_equal_firwin_live():
    signal = pytest.importorskip("scipy.signal")
    for r in range(2, 65):
        want = signal.firwin(20 * r + 1, 1.0 / r, window=("kaiser", 5.0)).astype(np.float32)
        for up, down in ((r, 1), (1, r), (r, r - 1)):
            got = pp.resample_poly_plan(100, up, down)[0]
            assert np.array_equal(got.view(np.uint32), (want * np.float32(up)).view(np.uint32)), (up, down)


def test_float32_taps_equal_the_recorded_firwin(golden):
    for r in rc.GOLDEN_RATES:
        want = golden[f"taps_r{r}"]
        assert want.dtype == np.float32 and want.shape == (20 * r + 1,)
        for up, down in ((r, 1), (1, r)):
            got = pp.resample_poly_plan(100, up, down)[0]
            assert np.array_equal(got.view(np.uint32), (want * np.float32(up)).view(np.uint32)), (up, down)


@pytest.mark.parametrize("defect", rc.DEFECTS)
def test_the_checker_rejects_a_planted_defect(host, defect):
    """On these inputs the checker of the GPU test tells a wrong kernel apart: a contracted multiply-add, a sum in
    descending order and a tap table read one phase further fail on the noise rows of every factor pair; a chain that
    skips the zero taps of the padding fails on the row with the NaN."""
    rejected = 0
    for up, down in rc.FACTORS:
        if pp.resample_poly_factors(up, down) == (1, 1):
            continue
        for n in (257, 3000):
            x = rc.rows(n)
            rows = [11] if defect == "skip_zero_taps" else list(range(9))
            wrong = rc.defective(x[rows], up, down, defect)
            want = host[up, down, n][rows]
            if defect == "skip_zero_taps":
                assert np.isnan(want).sum() >= np.isnan(wrong).sum()
                rejected += not pc.same_bits(wrong, want)
                continue
            differ = np.mean(wrong.view(np.uint32) != want.view(np.uint32))
            assert differ > 0.05, (defect, up, down, n, differ)
            with pytest.raises(AssertionError, match="differs at"):
                pc.check(wrong, want, defect)
            rejected += 1
    assert rejected >= (8 if defect == "skip_zero_taps" else 22), rejected
    if defect == "skip_zero_taps":
        x = rc.rows(3000)[[11]]
        with pytest.raises(AssertionError, match="differs at"):
            pc.check(rc.defective(x, 4, 1, defect), host[4, 1, 3000][[11]], defect)


def test_refusals():
    x = rc.rows(40)
    for up, down in ((0, 1), (1, 0), (-4, 1), (2.5, 1), (4, "1"), (None, 1), (True, 1), (65, 1), (1, 65), (130, 3)):
        with pytest.raises(ValueError, match="resample_poly"):
            pp.resample_poly_host(x, up, down)
        with pytest.raises(ValueError, match="resample_poly"):
            pp.resample_poly_plan(40, up, down)
    assert pp.resample_poly_factors(128, 2) == (64, 1)              # the limit counts after the reduction
    with pytest.raises(ValueError, match="at least 1 sample"):
        pp.resample_poly_plan(0, 4, 1)
    with pytest.raises(ValueError, match="at least 1 sample"):
        pp.resample_poly_host(np.zeros((3, 0), np.float32), 4, 1)
    with pytest.raises(ValueError, match="2\\^40"):
        pp.resample_poly_plan(2**38, 4, 1)
    with pytest.raises(ValueError, match="2\\^40"):
        pp.resample_poly_plan(2**34, 1, 64)
    pp.resample_poly_plan(2**34 - 1, 1, 64)
    with pytest.raises(ValueError, match="float32"):
        pp.resample_poly_host(x.astype(np.float64), 4, 1)
    with pytest.raises(ValueError, match=r"\(\.\.\., n\)"):
        pp.resample_poly_host(np.float32(1.0), 4, 1)
