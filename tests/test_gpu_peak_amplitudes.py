"""GPU: the peak amplitudes of matched-filter detections gathered on the device (csrc/peak_amp.hip,
workflow.peak_amplitudes; BPMF/similarity_search.py:695-714) against the host mirror
(postprocess.peak_amplitudes_host, itself pinned to the reference's loop in tests/test_peak_amplitudes_host.py):
bit patterns, every NaN equal to every NaN.  The session runs with debug.poison_output on (tests/conftest.py), so an
element the kernel does not write is a NaN here."""
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_amp_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirror(case):
    from seismic_bpmf_amd import postprocess as pp
    with np.errstate(invalid="ignore"):
        return pp.peak_amplitudes_host(case["data"], case["rows"], case["samples"], case["moveouts"], case["offset"],
                                       case["duration"], case["data_norm"])


def _device_view(data, pad=3):
    """The day as a device tensor that is a VIEW with a non-zero storage offset (4-byte aligned only)."""
    import torch
    buf = torch.full((data.size + pad + 5,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + data.size] = torch.as_tensor(data.reshape(-1), device="cuda")
    view = buf[pad:pad + data.size].view(data.shape)
    assert view.storage_offset() == pad and view.is_contiguous()
    return view


def _device(case, data_dev=None):
    from seismic_bpmf_amd import workflow
    return workflow.peak_amplitudes(_device_view(case["data"]) if data_dev is None else data_dev, case["rows"],
                                    case["samples"], case["moveouts"], offset=case["offset"],
                                    duration=case["duration"], data_norm=case["data_norm"])


def _check(case, label):
    got, want = _device(case), _mirror(case)
    if not pc.same_bits(got, want):
        bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        q, s, c = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {got.size} differ; first at (q={q}, s={s}, c={c}): got "
                             f"{got[q, s, c]!r}, want {want[q, s, c]!r}, sample {case['samples'][q]}, moveout "
                             f"{case['moveouts'][case['rows'][q], s, c]}, offset {case['offset']}, duration "
                             f"{case['duration']}, N {case['data'].shape[-1]}")
    return want


# S * C in {1, 3, 7, 60}, each with its own N (never a multiple of 4), window and offset
SHAPES = [((1, 1), 5003, 10, 1), ((1, 3), 4999, -5, 37), ((7, 1), 2501, 0, 2600), ((20, 3), 6001, 100, 300)]


def test_device_equals_host_mirror_on_every_class_of_window():
    assert pc.make_case(0, 50, 1, 1, 1, 0, 0, 1)["rows"].size == 0
    counts = None
    seed = 100
    for (S, C), N, offset, duration in SHAPES:
        for D in (0, 1, 2500):
            for norm in (True, False):
                seed += 1
                case = pc.make_case(seed, N, S, C, 6, D, offset, duration, norm=norm)
                want = _check(case, f"S={S} C={C} N={N} D={D} norm={norm}")
                assert want.shape == (D, S, C)
                counts = pc.count_classes(case, want, counts)
    print(counts)
    for name, n in counts.items():                   # the comparison above went through every class
        assert n >= 50, (name, counts)


def test_long_windows_and_windows_longer_than_a_round_of_loads():
    """`duration` up to N and beyond is a loop, not a bound: windows of 511 .. 513 and 1025 samples (a wave reads 512
    per round) and the whole day."""
    N = 70_003
    for i, duration in enumerate((511, 512, 513, 1025, N - 1, N, N + 7)):
        case = pc.make_case(300 + i, N, 2, 3, 3, 40, 11, duration, norm=bool(i % 2), nan_every=40_000)
        case["samples"][8:16] = np.arange(8) + case["offset"]          # windows that start at the head of the day
        _check(case, f"duration={duration}")


def test_all_empty_windows_are_written_as_zero_under_the_poison_option():
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1
    case = pc.make_case(7, 3001, 4, 3, 5, 500, 50, 200)
    N = 3001
    case["moveouts"] = np.clip(case["moveouts"], -40, 40)
    half = len(case["samples"]) // 2
    case["samples"][:half] = N + 100 + np.arange(half)                 # wholly past N
    case["samples"][half:] = -100 + np.arange(len(case["samples"]) - half) % 100  # every window straddles sample 0
    want = _mirror(case)
    assert not want.any() and not np.signbit(want).any()
    got = _device(case)
    assert got.shape == want.shape and pc.same_bits(got, want)


def test_bad_arguments_raise_with_a_message():
    import ctypes as C
    import torch
    from seismic_bpmf_amd import _lib, workflow
    case = pc.make_case(9, 1001, 2, 3, 4, 20, 5, 30)
    data = _device_view(case["data"])
    for bad_row in (4, -1, 2**31 - 1):
        rows = case["rows"].copy()
        rows[11] = bad_row
        with pytest.raises(_lib.BpmfHipError, match=f"detection 11 names template row {bad_row}, outside"):
            workflow.peak_amplitudes(data, rows, case["samples"], case["moveouts"], offset=5, duration=30)
    with pytest.raises(ValueError, match="tensor on the GPU"):
        workflow.peak_amplitudes(case["data"], case["rows"], case["samples"], case["moveouts"], offset=5, duration=30)
    with pytest.raises(ValueError, match="moveouts must be"):
        workflow.peak_amplitudes(data, case["rows"], case["samples"], case["moveouts"][:, :1], offset=5, duration=30)
    with pytest.raises(ValueError, match="data_norm must be"):
        workflow.peak_amplitudes(data, case["rows"], case["samples"], case["moveouts"], offset=5, duration=30,
                                 data_norm=np.ones(3, np.float32))
    with pytest.raises(ValueError, match="one entry per detection"):
        workflow.peak_amplitudes(data, case["rows"][:5], case["samples"], case["moveouts"], offset=5, duration=30)
    # the C ABI itself: null pointers and S * C == 0 return -1 and leave a message
    lib = _lib.lib()
    d_rows = torch.as_tensor(case["rows"], device="cuda")
    d_samples = torch.as_tensor(case["samples"], device="cuda")
    d_mv = torch.as_tensor(case["moveouts"], device="cuda")
    out = torch.zeros((20, 2, 3), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [C.c_void_p(data.data_ptr()), 2, 3, 1001, 20, C.c_void_p(d_rows.data_ptr()),
            C.c_void_p(d_samples.data_ptr()), C.c_void_p(d_mv.data_ptr()), 4, 5, 30, None, stream,
            C.c_void_p(out.data_ptr())]
    assert lib.bpmf_peak_amplitudes_dev(*good) == 0
    for pos in (0, 5, 6, 7, 13):
        args = list(good)
        args[pos] = None
        assert lib.bpmf_peak_amplitudes_dev(*args) == -1
        assert "null pointer" in _lib.last_error()
    for pos in (1, 2):
        args = list(good)
        args[pos] = 0
        assert lib.bpmf_peak_amplitudes_dev(*args) == -1
        assert "bad argument" in _lib.last_error()
    args = list(good)
    args[4] = 0                                      # no detection: nothing to do, whatever the pointers
    args[13] = None
    assert lib.bpmf_peak_amplitudes_dev(*args) == 0


def test_fuzz_of_240_shapes():
    for seed in range(240):
        rng = np.random.default_rng(5000 + seed)
        N = int(rng.integers(5, 3000))
        S, C = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        T, D = int(rng.integers(1, 7)), int(rng.integers(0, 41))
        offset = int(rng.integers(-50, 200))
        duration = int(rng.choice([1, 2, 63, 64, 65, int(rng.integers(1, 2 * N + 2)), int(rng.integers(1, 400))]))
        case = pc.make_case(6000 + seed, N, S, C, T, D, offset, duration, norm=bool(seed % 2))
        _check(case, f"fuzz seed {seed}: N={N} S={S} C={C} T={T} D={D}")


def _planted_day():
    from seismic_bpmf_amd import synthetic as syn
    inp = syn.make_mf_inputs(T=4, S=6, C=3, L=64, N=150_000, seed=3, max_moveout=200, n_events=4)
    kw = dict(sr=100.0, threshold_window_dur=300.0, minimum_interevent_time=5.0, remove_edges=False,
              white_noise=np.random.default_rng(0).standard_normal(500).astype(np.float32))
    norm = np.random.default_rng(1).uniform(0.5, 3.0, (6, 3)).astype(np.float32)
    return inp, kw, norm


def _mirror_of_detections(inp, det, moveouts, norm, offset=100, duration=300, step=1):
    """{row: (n, S, C)} from the host mirror on the same day (1.0 s and 3.0 s at 100 Hz)."""
    from seismic_bpmf_amd import postprocess as pp
    return {t: pp.peak_amplitudes_host(inp["data"], np.full(len(det[t]), t), np.asarray(det[t]) * step, moveouts,
                                       offset, duration, norm) for t in det}


def test_matched_filter_detections_with_peak_amplitudes():
    import torch
    from seismic_bpmf_amd.workflow import matched_filter_detections
    inp, kw, norm = _planted_day()
    args = (inp["templates"], inp["moveouts"], inp["weights"], inp["data"])
    plain = matched_filter_detections(*args, **kw)
    assert len(plain) == 2
    det0, cc0 = plain
    det, cc, amp = matched_filter_detections(*args, extract_peak_amplitudes=True, data_norm=norm, **kw)
    assert sorted(det) == sorted(det0) == [0, 1, 2, 3]
    for t in det:
        assert np.array_equal(det[t], det0[t])
        assert set(i0 for tt, i0 in inp["planted"] if tt == t) <= set(det[t].tolist()), t    # real events, all of them
    assert len(inp["planted"]) == 16 and torch.equal(cc, cc0)
    want = _mirror_of_detections(inp, det, inp["moveouts"], norm)
    for t in det:
        assert amp[t].shape == (len(det[t]), 6, 3) and amp[t].dtype == np.float32
        assert pc.same_bits(amp[t], want[t]), t
        assert (amp[t] > 0).all()                    # maxima of 300 samples of noise and signal
    # other phases on the components, another window, no norm
    mv_amp = np.ascontiguousarray(inp["moveouts"][:, :, ::-1])
    _, _, amp2 = matched_filter_detections(*args, extract_peak_amplitudes=True, moveouts_peak_amp=mv_amp,
                                           offset_win_peak_amp_sec=0.5, duration_win_peak_amp_sec=1.27, **kw)
    want2 = _mirror_of_detections(inp, det, mv_amp, None, offset=50, duration=127)
    assert all(pc.same_bits(amp2[t], want2[t]) for t in det)
    # every row rejected by the kurtosis check: (0, S, C) arrays, nothing launched
    det3, _, amp3 = matched_filter_detections(*args, extract_peak_amplitudes=True, max_kurto=-10.0, **kw)
    assert all(len(det3[t]) == 0 and amp3[t].shape == (0, 6, 3) and amp3[t].dtype == np.float32 for t in range(4))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_worker(port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from seismic_bpmf_amd import _lib, workflow
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    _lib.set_option("debug.poison_output", 1)
    inp, kw, norm = _planted_day()
    det, info = workflow.sharded_matched_filter_detections(
        inp["templates"], inp["moveouts"], inp["weights"], inp["data"], data_src=0, device=0,
        extract_peak_amplitudes=True, data_norm=norm, **kw)
    q.put(({t: v[0].tolist() for t, v in det.items()}, info["peak_amplitudes"], info["records_gathered"]))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_matched_filter_detections_world_1_with_peak_amplitudes():
    import torch.multiprocessing as mp
    from seismic_bpmf_amd.workflow import matched_filter_detections
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_sharded_worker, args=(_free_port(), q))
    proc.start()
    try:
        det, amp, n_rec = q.get(timeout=300)
        proc.join(timeout=120)
        assert proc.exitcode == 0
    finally:
        if proc.is_alive():
            proc.kill()
    inp, kw, norm = _planted_day()
    det1, _, amp1 = matched_filter_detections(inp["templates"], inp["moveouts"], inp["weights"], inp["data"],
                                              extract_peak_amplitudes=True, data_norm=norm, **kw)
    want = _mirror_of_detections(inp, det1, inp["moveouts"], norm)
    assert sorted(amp) == sorted(det) == [0, 1, 2, 3] and n_rec == sum(len(v) for v in det1.values()) >= 16
    for t in range(4):
        assert det[t] == det1[t].tolist()
        assert amp[t].shape == (len(det[t]), 6, 3)
        assert pc.same_bits(amp[t], amp1[t]) and pc.same_bits(amp[t], want[t]), t
