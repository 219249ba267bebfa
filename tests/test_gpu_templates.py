"""GPU: matched-filter templates cut from the day on the device (csrc/templates.hip, workflow.templates_from_events)
against the definition on the host (postprocess.templates_from_events_host, itself pinned to the reference in
tests/test_templates_host.py): bit patterns through view(uint32), NaNs at the same positions
(tests/templates_cases.py: check -- whose power to reject is shown in the CPU test).  The session runs with
debug.poison_output on (tests/conftest.py): an element the kernel does not write comes back as 0xFF bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import templates_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_view(data, pad=3):
    """The day as a device tensor that is a VIEW with a non-zero storage offset (4-byte aligned only)."""
    import torch
    buf = torch.full((data.size + pad + 5,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + data.size] = torch.as_tensor(data.reshape(-1), device="cuda")
    return buf[pad:pad + data.size].view(data.shape)


def _device(case, data_dev=None, **kw):
    from seismic_bpmf_amd import workflow
    return workflow.templates_from_events(_device_view(case["data"]) if data_dev is None else data_dev, case["origin"],
                                          case["moveouts"], case["L"], normalize=case["normalize"],
                                          noise_offset=case["noise_offset"], noise_samples=case["noise_samples"], **kw)


def _to_host(out):
    got = dict(out)
    got["templates"] = out["templates"].cpu().numpy()
    return got


def test_device_equals_the_definition_on_every_case():
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1           # outputs are handed over full of junk
    met = set()
    for label, kw in tc.CASES:
        case = tc.make_case(**kw)
        want = tc.host_answer(case)
        out = _device(case)
        tc.check(_to_host(out), want, label)
        assert np.array_equal(out["moveouts"].cpu().numpy(), case["moveouts"]), label
        met |= tc.classes_met(case, want)
    assert met == tc.ALL_CLASSES, tc.ALL_CLASSES - met


def test_tensors_come_back_on_the_days_device_and_stream():
    """Called under a side stream, the launch goes to that stream and the tensors are usable on it at once; moveouts
    given per station, as a tensor, serve every component; the weights are the simple weights of the flags."""
    import torch
    from seismic_bpmf_amd import postprocess as pp
    case = tc.make_case(31, 4, 3, 5, 129, "rms", noise=(60, 50), placements=("inside", "cut_by_end"))
    case["moveouts"] = np.repeat(case["moveouts"][:, :, :1], 3, axis=2)
    want = tc.host_answer(case)
    data = _device_view(case["data"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = _device(dict(case, moveouts=torch.as_tensor(case["moveouts"][:, :, 0], device="cuda")), data,
                      min_channels=4, min_stations=2)
        doubled = out["templates"] * 2                               # consumed on the same stream, no synchronisation
    side.synchronize()
    for key, dtype, shape in (("templates", torch.float32, (5, 4, 3, 129)), ("moveouts", torch.int32, (5, 4, 3)),
                              ("weights", torch.float32, (5, 4, 3))):
        t = out[key]
        assert t.device == data.device and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(), key
    tc.check(_to_host(out), want, "side stream")
    assert tc.same_bits(doubled.cpu().numpy(), want["templates"] * np.float32(2))
    for require_complete in (True, False):
        w = _device(case, data, min_channels=4, min_stations=2, require_complete=require_complete)["weights"]
        present = want["available"] & want["complete"] if require_complete else want["available"]
        assert np.array_equal(w.cpu().numpy(), pp.normalize_weights(pp.weights_channels_simple(present, 4, 2)))
    assert not want["complete"].all() and want["available"][~want["complete"]].any()
    # no event: empty arrays of the right shapes, nothing launched
    none = _device(dict(case, origin=np.zeros(0, np.int64), moveouts=np.zeros((0, 4, 3), np.int32)), data)
    assert tuple(none["templates"].shape) == (0, 4, 3, 129) and none["templates"].device == data.device
    assert tuple(none["weights"].shape) == (0, 4, 3) and tuple(none["moveouts"].shape) == (0, 4, 3)
    assert none["available"].shape == none["complete"].shape == none["norm"].shape == none["snr"].shape == (0, 4, 3)


def test_refusals_come_before_any_device_work():
    import torch
    from seismic_bpmf_amd import _lib, workflow
    case = tc.make_case(32, 2, 3, 4, 50, "rms", noise=(30, 20))
    data = _device_view(case["data"])
    with pytest.raises(ValueError, match="tensor on the GPU"):
        workflow.templates_from_events(case["data"], case["origin"], case["moveouts"], 50)
    with pytest.raises(ValueError, match="moveouts must be"):
        workflow.templates_from_events(data, case["origin"], case["moveouts"][:, :, :2], 50)
    with pytest.raises(ValueError, match="n_samples must be"):
        workflow.templates_from_events(data, case["origin"], case["moveouts"], 8193)
    with pytest.raises(ValueError, match="noise_samples must be"):
        workflow.templates_from_events(data, case["origin"], case["moveouts"], 50, noise_offset=1, noise_samples=8193)
    with pytest.raises(ValueError, match=r"within \+-2\^40"):
        workflow.templates_from_events(data, case["origin"] + 2**41, case["moveouts"], 50)
    # the C ABI itself: -1, a message, and outputs that nobody touched
    lib = _lib.lib()
    n = case["data"].shape[-1]
    d_origin = torch.as_tensor(case["origin"], device="cuda")
    d_far = torch.as_tensor(np.array([0, 5, -2**40 - 1, 7], dtype=np.int64), device="cuda")
    d_mv = torch.as_tensor(case["moveouts"], device="cuda")
    tp = torch.full((4, 2, 3, 50), 7.0, dtype=torch.float32, device="cuda")
    norm = torch.full((4, 2, 3), 7.0, dtype=torch.float32, device="cuda")
    flags = torch.full((4, 2, 3), 7, dtype=torch.uint8, device="cuda")
    snr = torch.full((4, 2, 3), 7.0, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = [p(data), 2, 3, n, 4, p(d_origin), p(d_mv), 50, 1, 30, 20, stream, p(tp), p(norm), p(flags), p(snr)]

    def refused(what, **changes):
        args = list(good)
        for pos, value in changes.items():
            args[int(pos[1:])] = value
        assert lib.bpmf_templates_from_events_dev(*args) == -1, changes
        assert what in _lib.last_error(), (_lib.last_error(), changes)

    for pos in (0, 5, 6, 12, 13, 14):
        refused("null pointer", **{f"a{pos}": None})
    refused("d_snr goes with noise_samples", a15=None)               # a noise window and nowhere to put the SNR
    refused("d_snr goes with noise_samples", a10=0)                  # the reverse
    refused("n_samples <= 8192", a7=0)
    refused("n_samples <= 8192", a7=8193)
    refused("noise_samples <= 8192", a10=8193)
    for changes in (dict(a1=0), dict(a2=0), dict(a3=0), dict(a3=2**40 + 1), dict(a8=3), dict(a8=-1),
                    dict(a9=2**40 + 1), dict(a9=-2**40 - 1), dict(a1=2**31), dict(a1=2**20, a2=2**10)):
        refused("bad argument", **changes)
    refused("event 2 has origin sample -1099511627777", a5=p(d_far))
    torch.cuda.synchronize()
    for t in (tp, norm, flags, snr):
        assert bool((t == 7).all())
    empty = list(good)
    empty[4] = 0                                                     # no event: nothing to do, whatever the pointers
    empty[12] = None
    assert lib.bpmf_templates_from_events_dev(*empty) == 0
    assert lib.bpmf_templates_from_events_dev(*good) == 0           # and the call they were all derived from works
    torch.cuda.synchronize()
    want = tc.host_answer(case)
    got = {"templates": tp.cpu().numpy(), "norm": norm.cpu().numpy(), "snr": snr.cpu().numpy(),
           "available": (flags.cpu().numpy() & 1) != 0, "complete": (flags.cpu().numpy() & 2) != 0}
    tc.check(got, want, "C ABI")
    assert int(flags.max()) <= 3


def test_templates_cut_on_the_device_go_straight_into_the_matched_filter():
    """The chain of one day at the smallest honest shape: events planted in a synthetic day, templates cut on the
    device at the planted origins, MatchedFilterGPU.run on the same day with the tensors as returned.  A template
    correlated with the samples it was cut from has CC 1 on every channel: cc[e, origin[e]] = sum(w) within SURVEY
    Appendix C's 2e-5 * sum|w|; and the whole CC matrix equals, bit for bit, the run with the templates the
    definition builds on the host."""
    import torch
    from seismic_bpmf_amd import MatchedFilterGPU, synthetic
    from seismic_bpmf_amd import postprocess as pp
    inp = synthetic.make_mf_inputs(T=3, S=4, C=3, L=128, N=20000, max_moveout=200, n_events=2)
    first = {}
    for t, i0 in inp["planted"]:
        first.setdefault(t, i0)
    assert sorted(first) == [0, 1, 2]
    origin = np.array([first[t] for t in range(3)], dtype=np.int64)
    mf = MatchedFilterGPU()
    mf.set_data(inp["data"])
    out = _device(dict(data=None, origin=origin, moveouts=inp["moveouts"], L=128, normalize="rms", noise_offset=None,
                       noise_samples=None), mf.data)
    assert all(out[k].is_cuda for k in ("templates", "moveouts", "weights"))
    cc = mf.run(out["templates"], out["moveouts"], out["weights"], 1)
    w = out["weights"].cpu().numpy()
    assert out["available"].all() and out["complete"].all() and np.allclose(w.sum(axis=(1, 2)), 1.0)
    cc_host = cc.cpu().numpy()
    for e in range(3):
        at_origin = float(cc_host[e, origin[e]])
        total, bound = float(w[e].sum(dtype=np.float64)), 2e-5 * float(np.abs(w[e]).sum(dtype=np.float64))
        print(f"event {e}: cc at the origin {at_origin!r}, sum(w) {total!r}, |difference| {abs(at_origin - total):.3e}, "
              f"bound {bound:.3e}")
        assert abs(at_origin - total) <= bound
        assert int(cc_host[e].argmax()) == origin[e]
    want = pp.templates_from_events_host(inp["data"], origin, inp["moveouts"], 128, "rms")
    weights = pp.normalize_weights(pp.weights_channels_simple(want["available"] & want["complete"], 6, 3))
    cc_ref = MatchedFilterGPU()
    cc_ref.set_data(inp["data"])
    ref = cc_ref.run(want["templates"], want["moveouts"], weights, 1).cpu().numpy()
    assert cc_host.shape == ref.shape and np.array_equal(cc_host.view(np.uint32), ref.view(np.uint32))
    torch.cuda.synchronize()
