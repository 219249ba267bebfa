"""CPU: the detection stage behind the beamformer without a device -- the host half of workflow.beam_detections_device
(the floor, the tie fallback, the suppression on the list, the gathered windows, beam_slice) on the NumPy stand-in of
its device half (bp_detect_cases.StandIn), against its definition, postprocess.find_beam_detections on the series
(DESIGN.md s4 "Non-finite features", rule 3); and the case list the GPU test shares: every class met, every planted
defect caught, no case in the one excluded class of input."""
import numpy as np
import pytest

import bp_detect_cases as bc


@pytest.fixture(scope="module")
def pp():
    """postprocess, with the NumPy stand-in for its host suppression routine where the library is not built."""
    from seismic_bpmf_amd import _lib, postprocess
    try:
        _lib.lib()
    except Exception:
        original = postprocess._suppress
        postprocess._suppress = bc.suppress
        yield postprocess
        postprocess._suppress = original
        return
    yield postprocess


@pytest.fixture(scope="module")
def wanted(pp):
    return {case[0]: bc.definition(case) for case in bc.named_cases()}


def _threshold_kw(spec):
    if spec[0] == "nodes":
        return dict(window=spec[1], overlap=spec[2], n_dev=spec[3])
    return dict(threshold=spec[1])


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def test_stand_in_suppression_equals_the_library(pp):
    rng = np.random.default_rng(3)
    for trial in range(40):
        ind = np.unique(rng.integers(0, 400, int(rng.integers(1, 120))))
        h = rng.integers(0, 6, ind.size).astype(np.float64)
        rank = pp._tallest_first(h)
        mpd = int(rng.integers(2, 30))
        assert np.array_equal(bc.suppress(ind, rank, mpd), pp._suppress(ind, rank, mpd)), trial


def test_the_stage_on_the_stand_in_equals_the_definition(pp, wanted):
    """beam_detections_device(detector=StandIn()) == find_beam_detections, peaks and sources, on every case -- a -Inf
    threshold (scalar, in an array, a whole array) among them."""
    import torch
    from seismic_bpmf_amd.workflow import beam_detections_device
    differ = []
    for name, beam, src, spec, mpd in bc.named_cases():
        det = bc.StandIn()
        peaks, psrc, nodes = beam_detections_device(torch.from_numpy(beam.copy()), torch.from_numpy(src.copy()), mpd=mpd,
                                                    detector=det, **_threshold_kw(spec))
        assert peaks.dtype.kind == "i" and (nodes is None) == (spec[0] != "nodes"), name
        if not _same((peaks, psrc), wanted[name]):
            differ.append((name, peaks.tolist(), wanted[name][0].tolist()))
    assert not differ, differ
    assert sum(w[0].size > 0 for w in wanted.values()) >= len(wanted) // 2        # the cases detect something


def test_the_restated_stage_equals_the_definition(pp, wanted):
    for name, beam, src, spec, mpd in bc.named_cases():
        assert _same(bc.stage(beam, src, spec, mpd), wanted[name]), name


def test_the_extraction_rule_equals_detect_peaks_without_suppression(pp):
    """The differences rule of the stand-in and the (fixed) kernel == postprocess.detect_peaks at mpd 1 on every series."""
    for name, beam, src, spec, mpd in bc.named_cases():
        with np.errstate(invalid="ignore"):
            want = pp.detect_peaks(beam, mpd=1)
        assert np.array_equal(bc.extract_rule(beam, -np.inf), want), name


def test_the_four_series_of_the_issue_are_cases(pp):
    """[1, inf, inf, 1, 0, 3, 1] and its kin: the run of +Inf is no peak, the isolated +Inf is one."""
    series = {c[0]: c[1] for c in bc.named_cases()}
    want = ([5], [6], [5], [2, 5])
    for j, (x, peaks) in enumerate(zip(bc.TABLE, want)):
        x = np.asarray(x, np.float32)
        assert np.array_equal(series[f"table_{j + 1}"], x)
        assert bc.extract_rule(x, 0.5).tolist() == pp.detect_peaks(x, mpd=1).tolist() == peaks
    assert [bc.extract_rule(np.asarray(x, np.float32), 0.5, "values_compared").tolist() for x in bc.TABLE] == \
        [[1, 5], [1, 6], [2, 5], [2, 5]]


def test_every_class_is_met(pp):
    met = {}
    for case in bc.named_cases():
        classes = bc.census(case)
        assert classes <= set(bc.CLASSES), (case[0], classes - set(bc.CLASSES))
        for c in classes:
            met.setdefault(c, []).append(case[0])
    missing = [c for c in bc.CLASSES if c not in met]
    assert not missing, missing
    assert len(set(bc.CLASSES)) == len(bc.CLASSES)
    for c in bc.CLASSES:
        print(f"{len(met[c]):3d}  {c}")


def test_no_case_is_in_the_excluded_class(pp):
    """A NaN and two neighbouring equal infinities in one series: outside the contract (the reference's answer at the
    infinities depends on whether a NaN exists anywhere)."""
    assert not [c[0] for c in bc.named_cases() if bc.excluded(c[1])]
    assert bc.excluded(np.array([0, np.nan, 1, np.inf, np.inf, 0], np.float32))
    assert bc.excluded(np.array([-np.inf, -np.inf, np.nan], np.float32))
    assert not bc.excluded(np.array([0, np.nan, np.inf, -np.inf, np.inf, 0], np.float32))
    assert not bc.excluded(np.array([0, 1, np.inf, np.inf, 0], np.float32))
    # what the exclusion is about: the same run of +Inf is no peak without a NaN and one with a NaN far away
    x = np.array([1, np.inf, np.inf, 1, 0, 3, 1, 0, 0], np.float32)
    y = x.copy()
    y[-1] = np.nan
    assert pp.detect_peaks(x).tolist() == [5] and pp.detect_peaks(y).tolist() == [2, 5]


def test_series_are_short(pp):
    for name, beam, src, spec, mpd in bc.named_cases():
        assert beam.dtype == np.float32 and src.dtype == np.int32 and beam.shape == src.shape, name
        if spec[0] == "nodes":
            assert int(spec[1]) <= 8200 and beam.size <= 3 * 8200, name
        else:
            assert beam.size <= 1100, name


def _device_half(case, defect=None):
    """What the device half hands to the host for a case: the records above the scalar floor (what the GPU test holds
    against the kernel), or the window statistics."""
    name, beam, src, spec, mpd = case
    det = bc.StandIn(defect)
    if spec[0] == "scalar":
        return [det.extract_peaks(beam, src, spec[1])] if not np.isnan(spec[1]) else []
    return list(det.window_stats(beam, spec[1], spec[2])) if spec[0] == "nodes" else []


@pytest.mark.parametrize("defect", bc.DEFECTS)
def test_every_planted_defect_changes_a_case(pp, wanted, defect):
    """Each way of getting the stage wrong changes the result of at least one case: the detections -- or, for `>=`
    at the floor of the extraction, the records: the host tests `>` again in float64 at every survivor, and a record
    AT the floor is lower than every other one, so it can suppress none of them; that defect shows in the records,
    which is where the GPU test looks."""
    if defect == "floor_greater_equal":
        caught = [case[0] for case in bc.extraction_cases()
                  if not all(np.array_equal(a, b) for a, b in zip(_device_half(case, defect), _device_half(case)))]
    else:
        caught = [name for name, beam, src, spec, mpd in bc.named_cases()
                  if not _same(bc.stage(beam, src, spec, mpd, defect=defect), wanted[name])]
    print(f"{defect}: {len(caught)} cases differ: {' '.join(caught[:12])}{' ...' if len(caught) > 12 else ''}")
    assert caught, defect


@pytest.mark.parametrize("defect", bc.DEFECTS_DEVICE)
def test_every_device_defect_changes_what_the_device_half_returns(pp, defect):
    """Records and window statistics are what test_gpu_bp_detect.py holds against the kernels: each defect of the
    device half changes them on at least one case."""
    caught = [case[0] for case in bc.named_cases()
              if not all(bc.same_bits(a["beam"], b["beam"]) and np.array_equal(a["index"], b["index"]) if a.dtype.names
                         else bc.same_bits(a, b) for a, b in zip(_device_half(case, defect), _device_half(case)))]
    assert caught, defect


@pytest.mark.parametrize("defect", [d for d in bc.DEFECTS_DEVICE if d != "floor_greater_equal"])
def test_a_defective_device_half_shows_through_the_library(pp, wanted, defect):
    """The same for the device half behind the library's own host half: beam_detections_device on a defective
    stand-in differs from the definition on at least one case."""
    import torch
    from seismic_bpmf_amd.workflow import beam_detections_device
    caught = []
    for name, beam, src, spec, mpd in bc.named_cases():
        got = beam_detections_device(torch.from_numpy(beam.copy()), torch.from_numpy(src.copy()), mpd=mpd,
                                     detector=bc.StandIn(defect), **_threshold_kw(spec))
        if not _same(got[:2], wanted[name]):
            caught.append(name)
    assert caught, defect


def test_key_order_medians_equal_np_median_bit_for_bit(pp):
    """What the window kernel computes -- the order statistics by key (-0.0 in front of +0.0), the float32 mean of the
    two middle ones, + 0.0 (np.median ends in np.mean, whose sum starts from +0: no median is -0.0) -- == np.median of
    every window of the statistics cases, bit for bit (NaN for NaN)."""
    def by_keys(seg):
        if not seg.size or np.isnan(seg).any():
            return bc.NAN
        s = seg[np.argsort(bc.f32_key(seg), kind="stable")]
        with np.errstate(all="ignore"):
            m = s[s.size // 2] if s.size % 2 else (s[s.size // 2 - 1] + s[s.size // 2]) / np.float32(2.0)
            return m + np.float32(0.0)

    windows = 0
    for name, beam, src, spec, mpd in bc.statistics_cases():
        window, shift, nw = bc.bp_window_plan(beam.size, spec[1], spec[2])
        med, mad = bc.StandIn().window_stats(beam, window, spec[2])
        for q in range(1, nw + 1):
            seg = beam[q * shift:min(beam.size, q * shift + window)]
            m = by_keys(seg)
            with np.errstate(all="ignore"):
                d = by_keys(np.abs(seg - m)) if seg.size else bc.NAN
            assert bc.same_bits(m, med[q]) and bc.same_bits(d, mad[q]), (name, q)
            windows += 1
    assert windows >= 100


def test_a_shift_of_zero_samples_is_refused_by_name(pp):
    import torch
    from seismic_bpmf_amd.threshold import bp_window_plan
    from seismic_bpmf_amd.workflow import beam_detections_device
    assert int((1.0 - 0.9999) * 100) == 0
    with pytest.raises(ValueError, match="shift of 0 samples"):
        bp_window_plan(1000, 100, 0.9999)
    with pytest.raises(ValueError, match="shift of 0 samples"):
        bp_window_plan(1000, 1, 0.75)
    with pytest.raises(ValueError, match="shorter than the sliding window"):
        bp_window_plan(99, 100, 0.75)
    assert bp_window_plan(100, 100, 0.75) == (100, 25, 1)
    x = torch.zeros(1000)
    with pytest.raises(ValueError, match="shift of 0 samples"):
        beam_detections_device(x, torch.zeros(1000, dtype=torch.int32), mpd=5, window=100, overlap=0.9999,
                               detector=bc.StandIn())
