"""CPU: the host side of the peak amplitudes (BPMF/similarity_search.py:695-722) -- the host mirror against the
reference's three-level loop written out (tests/peak_amp_cases.py: literal_loop), on seeded cases that are first
shown to hold every class of window the unguarded slice produces; normalize_data(return_norm=True) against
set_data's three lines (:181-185); detection_aux_data against lines 715-722."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_amp_cases as pc  # noqa: E402


def _mirror(case):
    from seismic_bpmf_amd import postprocess as pp
    return pp.peak_amplitudes_host(case["data"], case["rows"], case["samples"], case["moveouts"], case["offset"],
                                   case["duration"], case["data_norm"])


def test_host_mirror_equals_the_literal_loop_on_every_class_of_window():
    cases = [pc.make_case(*p) for p in pc.CPU_CASES]
    with np.errstate(invalid="ignore"):
        got = [_mirror(c) for c in cases]
        counts = None
        for c, g in zip(cases, got):
            counts = pc.count_classes(c, g, counts)
        print(counts)
        assert set(counts) == set(pc.CLASSES)
        for name, n in counts.items():
            assert n >= 50, (name, counts)           # a condition of the test: the seeds must cover every class
        for p, c, g in zip(pc.CPU_CASES, cases, got):
            want = pc.literal_loop(c)
            assert g.dtype == np.float32 and g.shape == (len(c["rows"]),) + c["data"].shape[:2]
            assert np.array_equal(g, want, equal_nan=True), p
            assert pc.same_bits(g, want), p


def test_host_mirror_slice_rule_examples():
    """The three consequences of the unguarded slice, on a day of 10 samples."""
    from seismic_bpmf_amd import postprocess as pp
    data = np.arange(10, dtype=np.float32).reshape(1, 1, 10) - 4.0            # -4 .. 5
    mv = np.zeros((1, 1, 1), np.int32)

    def amp(k, duration, norm=None):
        return pp.peak_amplitudes_host(data, [0], [k], mv, 0, duration, norm)[0, 0, 0]
    assert amp(2, 3) == 0.0                      # [2, 5): -2, -1, 0
    assert amp(0, 3) == -2.0                     # a window of negative samples: max, not max |x|
    assert amp(-2, 5) == 0.0 and amp(-2, 2) == 0.0   # straddles sample 0 (or ends at it): data[8:3], data[8:0] are empty
    assert amp(-3, 2) == 4.0                     # wholly before sample 0: wraps to data[7:9]
    assert amp(8, 5) == 5.0                      # clipped at N
    assert amp(10, 5) == 0.0 and amp(25, 5) == 0.0   # wholly past N
    assert amp(-13, 5) == -3.0                   # i1 + N still negative: clipped to 0 -> data[0:2]
    assert amp(0, 20) == 5.0                     # duration > N
    assert amp(0, 3, np.array([[3.0]], np.float32)) == -6.0
    assert amp(3, -2) == 0.0                     # a negative duration: data[3:1]
    out = pp.peak_amplitudes_host(data, np.zeros(0, np.int32), np.zeros(0, np.int64), mv, 0, 3)
    assert out.shape == (0, 1, 1) and out.dtype == np.float32
    # moveouts given per station are those of every component
    d2 = np.stack([data[0, 0], data[0, 0, ::-1]]).reshape(1, 2, 10)
    got = pp.peak_amplitudes_host(d2, [0, 0], [1, 2], np.array([[3]], np.int32), 1, 2)
    assert np.array_equal(got[:, 0, 0], [0.0, 1.0]) and np.array_equal(got[:, 0, 1], [2.0, 1.0])


def test_normalize_data_return_norm_equals_set_data():
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(8)
    raw = (rng.standard_normal((5, 3, 4000)) * rng.uniform(1e-3, 1e4, (5, 3, 1))).astype(np.float32)
    raw[2, 1] = 0.0                              # a dead channel: norm 1, data untouched
    data_arr = raw.copy()
    norm = np.std(data_arr, axis=-1, keepdims=True)          # similarity_search.py:182-185
    norm[norm == 0.0] = 1.0
    data_norm = norm.squeeze()
    data_arr /= norm
    got, got_norm = pp.normalize_data(raw, return_norm=True)
    assert got.dtype == np.float32 and np.array_equal(got, data_arr)
    assert got_norm.dtype == np.float32 and got_norm.shape == (5, 3) and np.array_equal(got_norm, data_norm)
    assert got_norm[2, 1] == 1.0
    only = pp.normalize_data(raw)                # the default return is unchanged
    assert isinstance(only, np.ndarray) and np.array_equal(only, data_arr)


def test_detection_aux_data_equals_the_reference_lines():
    from seismic_bpmf_amd import workflow
    rng = np.random.default_rng(2)
    n_dev = 8.0
    det, amps = {}, {}
    for t, n in enumerate([3, 0, 5]):
        idx = np.sort(rng.choice(10_000, n, replace=False)).astype(np.int64)
        det[t] = (idx, rng.uniform(0.1, 0.9, n).astype(np.float32), rng.uniform(0.05, 0.3, n).astype(np.float32))
        amps[t] = rng.standard_normal((n, 4, 3)).astype(np.float32)
    got = workflow.detection_aux_data(det, amps, n_dev)
    assert sorted(got) == [0, 1, 2] and got[1] == []
    tids = [17, 4, 99]
    named = workflow.detection_aux_data(det, amps, n_dev, tids=tids)
    for t, (idx, cc, threshold) in det.items():
        assert len(got[t]) == len(idx)
        for i in range(len(idx)):
            aux_data = {}                                                    # similarity_search.py:715-722
            aux_data["cc"] = cc[i]
            aux_data["n_threshold"] = cc[i] / threshold[i]
            aux_data["n_dev"] = aux_data["n_threshold"] * np.float32(n_dev)
            aux_data["tid"] = t
            aux_data["peak_amplitudes"] = amps[t][i]
            g = got[t][i]
            assert sorted(g) == sorted(aux_data)
            for key in ("cc", "n_threshold", "n_dev"):
                assert type(g[key]) is np.float32 and g[key] == aux_data[key], key
            assert g["tid"] == t and named[t][i]["tid"] == tids[t]
            assert g["peak_amplitudes"].shape == (4, 3) and np.array_equal(g["peak_amplitudes"], amps[t][i])
    bare = workflow.detection_aux_data(det, None, n_dev)                     # extract_peak_amplitudes off
    assert "peak_amplitudes" not in bare[0][0] and bare[0][0]["cc"] == det[0][1][0]
