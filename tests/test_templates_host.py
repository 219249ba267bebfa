"""CPU: the definition of the template builder (postprocess.templates_from_events_host, template_window_moveouts)
against what the REAL reference made of the same events (tests/golden/templates.npz, written by
tests/golden/make_templates_golden.py: utils.get_np_array, Event.set_availability, Family.normalize,
Template.moveouts_win / moveouts_arr called unbound on stand-in objects), bit for bit.  One part of the reference
cannot be driven without obspy even with stand-ins: Event.compute_snr deep-copies the event and reads its noise
windows through Event.read_waveforms, which builds an obspy.Stream; its two np.std lines (BPMF/dataset.py:1457-1461)
are pinned through NumPy alone, on the arrays the reference's get_np_array returned for the noise windows.

Then the checker itself (tests/templates_cases.py: check), which the GPU test relies on: it passes the definition's
answer and rejects each of seven planted defects applied to it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import templates_cases as tc  # noqa: E402

from seismic_bpmf_amd import postprocess as pp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "templates.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return [{k[:-len(f"_{j}")]: z[k] for k in z.files if k.endswith(f"_{j}")} for j in range(int(z["n_cases"]))]


def _host(g, normalize, noise=True):
    with np.errstate(invalid="ignore"):
        return pp.templates_from_events_host(g["data"], g["origin"], g["moveouts_arr"], int(g["n_samples"]), normalize,
                                             int(g["noise_offset"]) if noise else None,
                                             int(g["noise_samples"]) if noise else None)


def test_definition_equals_the_reference(golden):
    assert len(golden) == 3
    seen_cut = seen_past = 0
    for j, g in enumerate(golden):
        n = g["data"].shape[-1]
        start = g["origin"][:, None, None] + g["moveouts_arr"]
        assert start.min() >= 0                      # (windows cut by the start of the day: the stated departure)
        seen_cut += int(((start < n) & (start + int(g["n_samples"]) > n)).sum())
        seen_past += int((start >= n).sum())
        for mode in ("rms", "max", None):
            got = _host(g, mode)
            assert tc.same_bits(got["waveforms"], g["waveforms"]), (j, mode)
            assert got["available"].dtype == np.bool_ and np.array_equal(got["available"], g["available"]), (j, mode)
            want = g["waveforms"] if mode is None else g[f"templates_{mode}"]
            assert tc.same_bits(got["templates"], want), (j, mode)
            assert tc.same_bits(got["snr"], g["snr"]), (j, mode)
            # the norm the reference divided by, read back from its own arrays
            with np.errstate(invalid="ignore"):
                norm = {"rms": np.std(g["waveforms"], axis=-1), "max": np.max(np.abs(g["waveforms"]), axis=-1),
                        None: np.ones(g["snr"].shape, np.float32)}[mode]
            norm[norm == 0.0] = 1.0
            assert tc.same_bits(got["norm"], norm)
            assert np.array_equal(got["complete"], start + int(g["n_samples"]) <= n)
    assert seen_cut >= 5 and seen_past >= 5


def test_window_moveouts_equal_the_reference(golden):
    for g in golden:
        got = pp.template_window_moveouts(g["moveouts_sec"], g["offset_sec"], g["phase_of_component"], float(g["sr"]))
        assert got.dtype == np.int32 and np.array_equal(got, g["moveouts_arr"])
        assert (got < 0).any()                       # windows that start before the origin time


def test_weights_follow_availability(golden):
    g = golden[0]
    got = _host(g, "rms")
    w = pp.normalize_weights(pp.weights_channels_simple(got["available"] & got["complete"], 6, 3))
    assert w.dtype == np.float32 and w.shape == got["available"].shape
    for e in range(len(w)):
        present = got["available"][e] & got["complete"][e]
        if present.sum() >= 6 and present.any(axis=1).sum() >= 3:
            assert np.array_equal(w[e] != 0, present) and abs(w[e].sum() - 1.0) < 1e-6
        else:
            assert not w[e].any()
    assert not w[-1].any() and w[0].any()            # the last event lies at the very end of the day


def test_no_noise_window_means_no_snr():
    case = tc.make_case(1, 2, 3, 4, 50, noise=None)
    for kw in ({}, {"noise_samples": None}, {"noise_samples": 0}, {"noise_offset": 10, "noise_samples": 0},
               {"noise_offset": 10, "noise_samples": None}):
        with np.errstate(invalid="ignore"):
            out = pp.templates_from_events_host(case["data"], case["origin"], case["moveouts"], 50, **kw)
        assert out["snr"] is None and out["templates"].shape == (4, 2, 3, 50)
    # (E, S) moveouts are one moveout per station; no event gives empty arrays of the right shapes
    with np.errstate(invalid="ignore"):
        a = pp.templates_from_events_host(case["data"], case["origin"], case["moveouts"][:, :, 0], 50)
        b = pp.templates_from_events_host(case["data"], case["origin"],
                                          np.repeat(case["moveouts"][:, :, :1], 3, axis=2), 50)
    tc.check(a, b)
    empty = pp.templates_from_events_host(case["data"], np.zeros(0, np.int64), np.zeros((0, 2, 3), np.int32), 50,
                                          noise_offset=5, noise_samples=20)
    assert empty["templates"].shape == (0, 2, 3, 50) and empty["snr"].shape == (0, 2, 3)
    assert empty["available"].shape == (0, 2, 3) and empty["available"].dtype == np.bool_


def test_argument_validation_raises_before_any_device_work():
    from seismic_bpmf_amd import workflow
    import seismic_bpmf_amd as sb
    assert sb.templates_from_events is workflow.templates_from_events
    case = tc.make_case(2, 2, 3, 4, 50)
    d, o, m = case["data"], case["origin"], case["moveouts"]
    with pytest.raises(ValueError, match="tensor on the GPU"):
        workflow.templates_from_events(d, o, m, 50)                  # there is no CPU path
    bad = [dict(n_samples=0), dict(n_samples=8193), dict(n_samples=-1), dict(noise_samples=8193, noise_offset=1),
           dict(noise_samples=-1, noise_offset=1), dict(noise_samples=10), dict(normalize="l2"),
           dict(moveouts=m[:3]), dict(moveouts=m[:, :1]), dict(moveouts=m[:, :, :2]), dict(moveouts=m.astype(np.float32)),
           dict(origin_samples=o.astype(np.float64)), dict(origin_samples=o.reshape(2, 2)),
           dict(origin_samples=np.array([0, 1, 2, 2**40 + 1])), dict(origin_samples=np.array([0, 1, 2, -2**40 - 1])),
           dict(noise_samples=10, noise_offset=2**40 + 1), dict(data=d[0])]
    for kw in bad:
        args = dict(data=d, origin_samples=o, moveouts=m, n_samples=50)
        args.update(kw)
        with pytest.raises(ValueError, match="templates_from_events"):
            pp.templates_from_events_host(**args)
    pp.templates_from_events_host(d, np.array([0, 1, 2, 2**40]), m, 8192, noise_offset=-2**40, noise_samples=8192)


# ---------------------------------------------------------------------------------------- the checker
def _sequential_std(x):
    """np.std with running sums in place of pairwise ones."""
    count = np.float32(x.shape[-1])
    mean = np.cumsum(x, axis=-1, dtype=np.float32)[..., -1:] / count
    d = x - mean
    return np.sqrt(np.cumsum(d * d, axis=-1, dtype=np.float32)[..., -1] / count)


def _fused_std(x):
    """np.std with the squares of the deviations fused into the eight running sums of a leaf (x of up to 128
    samples): r[j] = fma(d, d, r[j]), one rounding where NumPy has two."""
    n = x.shape[-1]
    assert 16 <= n <= 128
    count = np.float32(n)
    d = (x - np.sum(x, axis=-1, keepdims=True) / count).astype(np.float64)
    r = (d[..., :8] * d[..., :8]).astype(np.float32)
    for i in range(8, n - n % 8, 8):
        r = (d[..., i:i + 8] * d[..., i:i + 8] + r.astype(np.float64)).astype(np.float32)   # (exact product, one rounding)
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for i in range(n - n % 8, n):
        res = (d[..., i] * d[..., i] + res.astype(np.float64)).astype(np.float32)
    return np.sqrt(res / count)


def _renormalised(want, std):
    out = dict(want)
    norm = std.astype(np.float32).copy()
    norm[norm == 0.0] = 1.0
    out["norm"] = norm
    out["templates"] = want["waveforms"] / norm[..., None]
    return out


def test_checker_rejects_planted_defects():
    rejected = []

    def rejects(got, want, name):
        tc.check(want, want, name)
        with pytest.raises(AssertionError, match=name):
            tc.check(got, want, name)
        rejected.append(name)

    with np.errstate(invalid="ignore", divide="ignore"):
        # 1. a sequential sum instead of the pairwise one
        case = tc.make_case(11, 1, 5, 3, 1000, "rms", placements=("inside",))
        want = tc.host_answer(case)
        rejects(_renormalised(want, _sequential_std(want["waveforms"])), want, "sequential sum")
        # 2. a fused multiply-add in the deviations
        case = tc.make_case(12, 20, 3, 30, 100, "rms", placements=("inside",))
        want = tc.host_answer(case)
        rejects(_renormalised(want, _fused_std(want["waveforms"])), want, "fused multiply-add")
        # 3. a window cut by sample 0, left-aligned as the reference does it
        case = tc.make_case(13, 1, 5, 3, 64, "rms", placements=("cut_by_start",))
        want = tc.host_answer(case)
        got = dict(want)
        got["templates"] = np.concatenate([want["templates"][..., 32:], want["templates"][..., :32]], axis=-1)
        rejects(got, want, "left-aligned")
        # 4. a zero norm left as 0 (an all-zero window: 0 / 0)
        case = tc.make_case(14, 1, 5, 3, 64, "rms", placements=("before_day", "inside"))
        want = tc.host_answer(case)
        got = dict(want)
        got["norm"] = np.where(want["available"], want["norm"], np.float32(0.0)).astype(np.float32)
        got["templates"] = want["waveforms"] / got["norm"][..., None]
        rejects(got, want, "zero norm")
        # 5. `available` taken from the normalised window of a NaN channel (all NaN: nothing compares greater than 0)
        case = tc.make_case(15, 1, 8, 3, 64, "max", placements=("at_start",))
        want = tc.host_answer(case)
        assert np.isnan(want["norm"]).any()
        got = dict(want)
        got["available"] = (np.abs(want["templates"]) > 0).any(axis=-1)
        rejects(got, want, "available from the normalised window")
        # 6. a clipped sample left as junk (here: the day's last sample, where a clamped load lands)
        case = tc.make_case(16, 1, 5, 3, 64, None, placements=("cut_by_end",))
        want = tc.host_answer(case)
        got = dict(want)
        got["templates"] = want["templates"].copy()
        got["templates"][..., -1] = case["data"][None, :, :, -1]
        rejects(got, want, "junk")
        # 7. the SNR taken from the normalised window
        case = tc.make_case(17, 1, 5, 3, 64, "rms", noise=(100, 80), placements=("inside",))
        want = tc.host_answer(case)
        got = dict(want)
        got["snr"] = (want["snr"] / want["norm"]).astype(np.float32)
        rejects(got, want, "snr of the normalised window")
    assert len(rejected) == 7


def test_cases_go_through_every_class():
    met = set()
    labels = [label for label, _ in tc.CASES]
    assert len(set(labels)) == len(labels)
    for label, kw in tc.CASES:
        case = tc.make_case(**kw)
        want = tc.host_answer(case)
        tc.check(want, want, label)
        met |= tc.classes_met(case, want)
    assert met == tc.ALL_CLASSES, (tc.ALL_CLASSES - met, met - tc.ALL_CLASSES)
    assert {kw["L"] for _, kw in tc.CASES} >= set(tc.LENGTHS)
    assert {kw["S"] * kw["C"] for _, kw in tc.CASES} >= {1, 5, 60} and {kw["E"] for _, kw in tc.CASES} >= {1, 3, 300}
