"""GPU: the detection stage behind the beamformer on the cases of tests/bp_detect_cases.py -- the seams of the extraction
kernel (wave, block, the ends of the series), +-Inf and NaN in the max-beam, the window lengths around the block and the
unrolled loop of the radix select, every form of the threshold.  Everything is exact:

* bpmf_bp_window_stats_dev == np.median / MAD of every window, bit for bit (the sign of a zero counts, NaN for NaN);
* bpmf_bp_extract_peaks_dev == the rule restated in NumPy (the reference's float64 differences), at a record capacity
  of 1, of the count minus one and of the count, the records sorted;
* workflow.beam_detections_device == postprocess.find_beam_detections on the series (DESIGN.md s4 "Non-finite features",
  rule 3), peaks and sources.

Every call is made on outputs filled with junk, twice with different junk (debug.poison_output is on for the session);
what a call is not to write must still hold the junk afterwards."""
import numpy as np
import pytest

import bp_detect_cases as bc

pytestmark = pytest.mark.gpu

JUNK = (0x7F7F7F7F, 0xFFC12345 - (1 << 32))          # as int32: a large finite float, a NaN with a payload


@pytest.fixture(scope="module")
def det():
    from seismic_bpmf_amd.threshold import BeamDetectorGPU
    return BeamDetectorGPU()


@pytest.fixture(scope="module")
def wanted():
    return {case[0]: bc.definition(case) for case in bc.named_cases()}


def _dev(a):
    import torch
    return torch.tensor(np.asarray(a), device="cuda")


def _junk(shape, value):
    import torch
    return torch.full(shape, value, dtype=torch.int32, device="cuda")


def _threshold_kw(spec):
    if spec[0] == "nodes":
        return dict(window=spec[1], overlap=spec[2], n_dev=spec[3])
    return dict(threshold=spec[1])


def test_window_statistics_equal_np_median_bit_for_bit(det):
    import torch
    from seismic_bpmf_amd import _lib
    windows = 0
    for name, beam, src, spec, mpd in bc.statistics_cases():
        window, shift, nw = bc.bp_window_plan(beam.size, spec[1], spec[2])
        want_med, want_mad = bc.StandIn().window_stats(beam, window, spec[2])
        assert det.lib.bpmf_bp_num_windows(beam.size, window, shift) == nw, name
        x = _dev(beam)
        for junk in JUNK:
            med, mad = _junk((nw + 2,), junk), _junk((nw + 2,), junk)
            _lib.call("bpmf_bp_window_stats_dev", x.device, x, beam.size, window, shift, _lib.STREAM,
                      med.view(torch.float32), mad.view(torch.float32))
            med, mad = med.cpu().numpy(), mad.cpu().numpy()
            assert med[0] == med[-1] == mad[0] == mad[-1] == junk, name          # the end entries are the caller's
            for q in range(1, nw + 1):
                assert bc.same_bits(med[q].view(np.float32), want_med[q]) and bc.same_bits(mad[q].view(np.float32), want_mad[q]), \
                    (name, q, med[q].view(np.float32), want_med[q], mad[q].view(np.float32), want_mad[q])
        got_med, got_mad = det.window_stats(x, window, spec[2])
        assert bc.same_bits(got_med[1:-1], want_med[1:-1]) and bc.same_bits(got_mad[1:-1], want_mad[1:-1]), name
        assert got_med[0] == got_med[-1] == got_mad[0] == got_mad[-1] == 0, name
        windows += nw
    assert windows >= 100


def test_extracted_records_equal_the_rule_at_every_capacity(det):
    import torch
    from seismic_bpmf_amd import _lib
    records = 0
    for name, beam, src, spec, mpd in bc.extraction_cases():
        floor = float(spec[1])
        want = bc.StandIn().extract_peaks(beam, src, floor)
        x, s = _dev(beam), _dev(src)
        count = want.size
        for capacity in sorted({1, count - 1, count} - {-1}):
            got = det.extract_peaks(x, s, floor, capacity=capacity)
            assert got.dtype == bc.peak_dtype and np.all(np.diff(got["index"]) > 0), (name, capacity)
            for field in ("index", "source"):
                assert np.array_equal(got[field], want[field]), (name, capacity, field, got[field][:8], want[field][:8])
            assert bc.same_bits(got["beam"], want["beam"]), (name, capacity)
        assert np.array_equal(det.extract_peaks(x, None, floor)["source"], np.zeros(count, np.int32)), name
        # the entry point itself on junk: the count is set (not added to), `capacity` records are written and no more
        for junk, capacity in zip(JUNK, (count, 1)):
            rec, found = _junk((capacity + 3, 4), junk), _junk((1,), junk)
            _lib.call("bpmf_bp_extract_peaks_dev", x.device, x, s, beam.size, floor, capacity, _lib.STREAM, found, rec)
            assert int(found.item()) == count, (name, capacity)
            rec = rec.cpu().numpy()
            stored = min(count, capacity)
            assert (rec[stored:] == junk).all(), (name, capacity)
            got = rec[:stored].view(bc.peak_dtype).reshape(-1)
            assert np.unique(got["index"]).size == stored and np.isin(got["index"], want["index"]).all(), (name, capacity)
            at = np.searchsorted(want["index"], got["index"])
            assert np.array_equal(got["source"], want["source"][at]) and bc.same_bits(got["beam"], want["beam"][at]), name
            assert (got["pad"] == 0).all(), name
        records += count
    assert records >= 2000


def test_detections_equal_the_definition_on_every_case(det, wanted):
    from seismic_bpmf_amd.workflow import beam_detections_device
    differ = []
    for name, beam, src, spec, mpd in bc.named_cases():
        x, s = _dev(beam), _dev(src)
        for repeat in range(2):
            peaks, psrc, nodes = beam_detections_device(x, s, mpd=mpd, **_threshold_kw(spec))
            assert peaks.dtype.kind == "i" and (nodes is None) == (spec[0] != "nodes"), name
            if not (np.array_equal(peaks, wanted[name][0]) and np.array_equal(psrc, wanted[name][1])):
                differ.append((name, repeat, peaks.tolist()[:12], wanted[name][0].tolist()[:12]))
        if spec[0] == "nodes":
            med, mad = bc.StandIn().window_stats(beam, spec[1], spec[2])
            with np.errstate(all="ignore"):
                from seismic_bpmf_amd import postprocess as pp
                centre, thr = pp.bp_threshold_nodes(beam.size, int(spec[1]), spec[2], med, mad, spec[3])
            assert np.array_equal(nodes[0], centre) and bc.same_bits(nodes[1], thr), name
    assert not differ, differ
    assert sum(w[0].size > 0 for w in wanted.values()) >= len(wanted) // 2


def test_a_shift_of_zero_samples_is_refused_by_name(det):
    import torch
    from seismic_bpmf_amd.workflow import beam_detections_device
    x = torch.zeros(1000, device="cuda")
    with pytest.raises(ValueError, match="shift of 0 samples"):
        det.window_stats(x, 100, 0.9999)
    with pytest.raises(ValueError, match="shift of 0 samples"):
        beam_detections_device(x, torch.zeros(1000, dtype=torch.int32, device="cuda"), mpd=5, window=100, overlap=0.9999)
    with pytest.raises(ValueError, match="shorter than the sliding window"):
        det.window_stats(x, 1001, 0.75)
