"""GPU: the matched filter's full normalisation (flag BPMF_MF_NORMALIZE_FULL, csrc/mf_full.hip) against its float64
definition (tests/mf_full_definition.py; tests/test_mf_full_definition.py shows which planted defect each regime catches).

Every kernel family the flag can take -- asserted with bpmf_mf_launch_info, flags = 4 -- over the sizes at which the
per-day preparation can go wrong (one 1024-sample chunk, the chunk seam, its successor, a partial last chunk, three lag
blocks; channels off 16-byte alignment; L from 1 to 1040) and the regimes of the definition: |kernel - f64| <= B_full per
channel and for the network sum, outputs poisoned, exact +0 (bit for bit) on flat windows, bit-equality with short mode
where every window sum is 0.  Then the resident engine, the C ABI's refusals, the host call on two (virtual) devices and
the detection workflow.  Every check prints its worst err / B (pytest -rP).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import f64_anchor as fa
import mf_full_definition as mfd
from mf_launch import assert_takes

pytestmark = pytest.mark.gpu

FULL = 4
WORST = {}


@functools.lru_cache(maxsize=None)
def _case(regime, L, N, step, **range_kw):
    args = mfd.mf_full_case(regime, L, N, step, seed=7000 + L + step)
    lags = mfd.mf_full_lags(args, step, seed=L, extra=mfd.gap_lags(args, step) if regime == "gaps" else ())
    ref = mfd.mf_full_f64(*args, step=step, lags=lags, exact=regime if regime in mfd.EXACT_REGIMES else False, **range_kw)
    assert ref.valid.any() and not ref.valid[1].any()               # (template 1 has no weight at all)
    assert (~ref.active[0]).sum() == 1                              # one zero-weight channel
    if regime == "gaps":
        assert ref.flat.sum() >= 20
    return args, ref


def _host(args, step, ns):
    import seismic_bpmf_amd as sb
    return sb.matched_filter_full(*args, step, arch="gpu", check_zeros=False, network_sum=ns, device=0)


def _resident(args, step, ns, **kw):
    from seismic_bpmf_amd import MatchedFilterGPU
    eng = MatchedFilterGPU(device=0)
    eng.set_data(args[3])
    first = eng.run(args[0], args[1], args[2], step, network_sum=ns, normalize="full", **kw).cpu().numpy()
    again = eng.run(args[0], args[1], args[2], step, network_sum=ns, normalize="full", **kw).cpu().numpy()   # prepared day
    assert np.array_equal(first, again, equal_nan=True)
    return again


def _judge(family, label, got, ref, ns):
    got = fa.mf_full(got, ref)
    worst = fa.mf_compare(got, ref, ns, f"kernel MF full {family}: {label} network_sum={ns}").require()
    WORST[family] = max(WORST.get(family, 0.0), worst)
    if not ns:
        # flat windows and flat template channels: +0 bit for bit
        assert not got[ref.flat].view(np.uint32).any(), label


def _check(family, regime, L, N, step=1, run=_host, takes=None, flags=FULL, **run_kw):
    args, ref = _case(regime, L, N, step)
    for ns in (True, False):
        assert_takes(args[0].shape, N, step, ns, flags=flags,
                     **{k: v(ns) if callable(v) else v for k, v in (takes or {}).items()})
        _judge(family, f"{regime} L={L} N={N} step={step}", run(args, step, ns, **run_kw), ref, ns)
    print(f"f64-anchor MF full, family {family}: worst err/B so far {WORST[family]:.4f}")
    return args, ref


# ----------------------------------------------------------------------------------- kernel families ---
@pytest.mark.parametrize("ntile", [1, 2, 4])
def test_wave_kernel_tiles(hip_opts, ntile):
    hip_opts("mf.tiles_per_wave", ntile)
    takes = dict(family="wave", ntile=ntile)
    fam = f"wave ntile={ntile}"
    _check(fam, "noise", 100, 20011, takes=takes)                   # three 8192-lag blocks
    _check(fam, "offset", 100, 3100, takes=takes)                   # short mode is off by orders of magnitude here
    _check(fam, "drift", 33, 1025, takes=takes)
    _check(fam, "step", 257, 3100, takes=takes)
    _check(fam, "gaps", 100, 3100, takes=takes)
    _check(fam, "int0", 100, 3100, takes=takes)
    _check(fam, "scaled", 8, 1024, 3, takes=takes)


def test_wave_kernel_short_templates_and_small_days():
    for L, N in ((1, 700), (2, 700), (3, 700), (8, 1025)):
        _check("wave default", "noise", L, N, takes=dict(family="wave"))
    _check("wave default", "gaps", 3, 700, takes=dict(family="wave"))
    _check("wave default", "scaled", 100, 3100, takes=dict(family="wave"))
    _check("wave default", "offset", 2, 1024, takes=dict(family="wave"))
    args, ref = _case("noise", 1, 700, 1)
    assert not ref.cc.any()                                         # L = 1: every window is flat


@pytest.mark.parametrize("fused", [1, 0])
def test_wave_kernel_fused_and_separate_prologue(hip_opts, fused):
    hip_opts("mf.tiles_per_wave", 1)
    hip_opts("mf.fused_prologue", fused)
    takes = dict(family="wave", ntile=1, fused=bool(fused), prologue=not fused)
    _check(f"wave fused={fused}", "offset", 33, 1025, 3, takes=takes)
    _check(f"wave fused={fused}", "int0", 257, 1025, takes=takes)


def test_wave_kernel_channel_split(hip_opts):
    hip_opts("mf.channel_split", 1 << 20)
    hip_opts("mf.tiles_per_wave", 1)
    takes = dict(family="wave", ntile=1, fused=True, csplit=lambda ns: ns)
    for regime, L, N in (("offset", 100, 3100), ("gaps", 33, 1025), ("int0", 100, 3100)):
        _check("wave channel split", regime, L, N, takes=takes)
        _check("wave channel split", regime, L, N, run=_resident, takes=takes)


def test_workgroup_kernel(hip_opts):
    _check("workgroup", "offset", 1040, 20011, takes=dict(family="workgroup", maxr=24, maxt=9))
    _check("workgroup", "gaps", 1040, 3100, takes=dict(family="workgroup", maxr=24, maxt=9))
    _check("workgroup", "noise", 1040, 3100, 3, takes=dict(family="workgroup", maxr=24, maxt=9))
    hip_opts("mf.wave_kernel", 0)
    takes = dict(family="workgroup", maxr=20, maxt=5)
    for regime, L, N in (("offset", 100, 3100), ("drift", 33, 1025), ("step", 257, 3100), ("int0", 100, 3100),
                         ("noise", 2, 700)):
        _check("workgroup", regime, L, N, takes=takes)


def test_generic_kernel(hip_opts):
    takes = dict(family="direct")
    for regime, L, N, step in (("offset", 33, 3100, 3), ("gaps", 100, 3100, 1), ("int0", 100, 3100, 1),
                               ("noise", 1040, 3100, 3), ("noise", 1, 700, 1)):
        _check("generic", regime, L, N, step, run=_resident, takes=takes, flags=FULL | 2, force_direct=True)
    hip_opts("mf.max_mfma_step", 0)
    _check("generic", "offset", 33, 3100, 3, takes=takes)
    _check("generic", "step", 257, 3100, 3, takes=takes)


def test_short_mode_is_wrong_on_an_offset_where_full_mode_is_right():
    import seismic_bpmf_amd as sb
    args, ref = _case("offset", 100, 3100, 1)
    short = sb.matched_filter(*args, 1, arch="gpu", check_zeros=False, network_sum=False, device=0)
    rep = fa.mf_compare(fa.mf_full(short, ref), ref, False)
    live = ref.B > 0
    err = np.abs(fa.mf_full(short, ref).astype(np.float64) - ref.cc)[live]
    assert rep.n_bad > 0.9 * live.sum() and np.median(err / ref.B[live]) > 1e3


@pytest.mark.parametrize("family", ["wave 1", "wave 2", "wave 4", "channel split", "workgroup", "generic"])
def test_periodic_regime_is_bit_equal_to_short_mode(oracle_lib, hip_opts, family):
    """Every window sum is exactly 0: full mode == short mode == the oracle, bit for bit, on the same arrays."""
    import seismic_bpmf_amd as sb
    L, N = mfd.PERIODIC_L, 64 * mfd.PERIODIC_L
    flags = FULL
    if family.startswith("wave"):
        hip_opts("mf.tiles_per_wave", int(family[-1]))
        takes = dict(family="wave", ntile=int(family[-1]))
    elif family == "channel split":
        hip_opts("mf.channel_split", 1 << 20)
        hip_opts("mf.tiles_per_wave", 1)
        takes = dict(family="wave", csplit=lambda ns: ns)
    elif family == "workgroup":
        hip_opts("mf.wave_kernel", 0)
        takes = dict(family="workgroup")
    else:
        hip_opts("mf.max_mfma_step", 0)
        takes = dict(family="direct")
    args, ref = _check(f"periodic {family}", "periodic", L, N, takes=takes, flags=flags)
    assert not ref.P.any()
    for ns in (True, False):
        full = _host(args, 1, ns)
        short = sb.matched_filter(*args, 1, arch="gpu", check_zeros=False, network_sum=ns, device=0)
        assert np.array_equal(full, short) and np.array_equal(full, oracle_lib.matched_filter(*args, 1, network_sum=ns))
        assert np.abs(full).max() > 0.05


# ------------------------------------------------------------------------------------- resident engine ---
def test_resident_short_full_short_on_one_object():
    from seismic_bpmf_amd import MatchedFilterGPU
    args, ref = _case("offset", 100, 3100, 1)

    def fresh(normalize, ns):
        eng = MatchedFilterGPU(device=0)
        eng.set_data(args[3])
        return eng.run(*args[:3], 1, network_sum=ns, normalize=normalize).cpu().numpy()

    eng = MatchedFilterGPU(device=0)
    eng.set_data(args[3])
    for ns in (True, False):
        want = {m: fresh(m, ns) for m in ("short", "full")}
        for mode in ("short", "full", "full", "short", "short", "full"):
            got = eng.run(*args[:3], 1, network_sum=ns, normalize=mode).cpu().numpy()
            assert np.array_equal(got, want[mode]), (mode, ns)
        _judge("resident", "short / full / short", want["full"], ref, ns)
    assert eng.workspace_bytes(100, 3, "full") > eng.workspace_bytes(100, 3) == eng.lib.bpmf_mf_workspace_bytes(100, 3100, 3, 2, 3)
    with pytest.raises(ValueError, match="normalize"):
        eng.run(*args[:3], 1, normalize="none")


def test_resident_two_template_lengths_on_one_object():
    from seismic_bpmf_amd import MatchedFilterGPU
    a33, r33 = _case("offset", 33, 3100, 3)
    a100, r100 = _case("offset", 100, 3100, 1)
    eng = MatchedFilterGPU(device=0)
    for (args, ref, step) in ((a100, r100, 1), (a33, r33, 3), (a100, r100, 1)):
        eng.set_data(args[3])
        for ns in (True, False):
            for _ in range(2):
                got = eng.run(*args[:3], step, network_sum=ns, normalize="full").cpu().numpy()
                _judge("resident", f"two lengths, L={args[0].shape[-1]}", got, ref, ns)
    # the same day, two lengths, the day prepared again for each
    short_tp = np.ascontiguousarray(a100[0][..., 20:53])
    eng.set_data(a100[3])
    for tp, step in ((a100[0], 1), (short_tp, 1), (a100[0], 1)):
        got = eng.run(tp, a100[1], a100[2], step, normalize="full").cpu().numpy()
        assert np.array_equal(got, _host((tp,) + a100[1:], step, True))


@pytest.mark.parametrize("switch,kw", [("mf.compat_exclusive_last_lag", dict(exclusive_last_lag=True)),
                                       ("mf.compat_range_all_channels", dict(range_all_channels=True))])
def test_lag_range_switches_compose(hip_opts, switch, kw):
    hip_opts(switch, 1)
    for regime, L, N, step in (("offset", 100, 3100, 1), ("drift", 33, 1025, 3)):
        args = mfd.mf_full_case(regime, L, N, step, seed=7000 + L + step)
        lags = mfd.mf_full_lags(args, step, seed=L)
        ref = mfd.mf_full_f64(*args, step=step, lags=lags, **kw)
        plain = _case(regime, L, N, step)[1]
        assert not np.array_equal(ref.valid, plain.valid)           # the switch moves an edge of some range
        for ns in (True, False):
            _judge("resident", f"{switch} {regime} L={L}", _resident(args, step, ns), ref, ns)
            _judge("host", f"{switch} {regime} L={L}", _host(args, step, ns), ref, ns)


def test_c_abi_refuses_stale_days_and_undefined_options(hip_opts):
    """BPMF_MF_DATA_PREPARED on a day prepared for the other normalisation (or on another day), and the two options
    full mode is not defined under: status -1 with a message, nothing launched (the output keeps its fill)."""
    import torch
    from seismic_bpmf_amd import _lib
    lib = _lib.lib()
    args, ref = _case("offset", 100, 3100, 1)
    tp, mv, w, d = (torch.as_tensor(a, device="cuda:0").contiguous() for a in args)
    other = d.clone()
    T, S, Cc, L = tp.shape
    N = d.shape[-1]
    n_corr = N - L + 1
    nbytes = lib.bpmf_mf_full_workspace_bytes(L, N, T, S, Cc)
    assert nbytes > lib.bpmf_mf_workspace_bytes(L, N, T, S, Cc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    out = torch.full((T, n_corr), 123.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(flags, data=d):
        rc = lib.bpmf_mf_run_dev(tp.data_ptr(), mv.data_ptr(), w.data_ptr(), data.data_ptr(), 1, L, N, T, S, Cc, n_corr, 1,
                                 flags, ws.data_ptr(), ws.numel(), stream, out.data_ptr())
        torch.cuda.synchronize()
        return rc, _lib.last_error()

    def untouched():
        return bool((out == 123.0).all())

    with torch.cuda.device(0):
        assert lib.bpmf_mf_prepare_data_dev(d.data_ptr(), L, N, S, Cc, ws.data_ptr(), ws.numel(), stream) == 0
        rc, msg = run(1 | FULL)
        assert rc == -1 and "prepared in short mode" in msg and untouched()
        assert lib.bpmf_mf_prepare_data_full_dev(d.data_ptr(), L, N, S, Cc, ws.data_ptr(), ws.numel(), stream) == 0
        rc, msg = run(1)
        assert rc == -1 and "bpmf_mf_prepare_data_full_dev" in msg and untouched()
        rc, msg = run(1 | FULL, other)                                  # another day
        assert rc == -1 and "another day" in msg and untouched()
        rc, msg = run(1 | FULL)
        assert rc == 0, msg
        full = out.cpu().numpy()
        _judge("C ABI", "prepared, then run", full, ref, True)
        rc, msg = run(0)                                                # short mode prepares its own day again ...
        assert rc == 0, msg
        short = out.cpu().numpy()
        assert not np.array_equal(short, full)
        rc, msg = run(1)                                                # ... which it may then reuse, full mode may not
        assert rc == 0 and np.array_equal(out.cpu().numpy(), short)
        out.fill_(123.0)
        rc, msg = run(1 | FULL)
        assert rc == -1 and untouched()
        small = lib.bpmf_mf_workspace_bytes(L, N, T, S, Cc)
        rc = lib.bpmf_mf_prepare_data_full_dev(d.data_ptr(), L, N, S, Cc, ws.data_ptr(), small, stream)
        assert rc == -1 and "workspace too small" in _lib.last_error()
        for opt in ("mf.compat_sqrt_norm", "mf.compat_sequential_csum"):
            hip_opts(opt, 1)
            rc, msg = run(FULL)
            assert rc == -1 and f"not defined under option {opt}" in msg and untouched()
            rc = lib.bpmf_mf_prepare_data_full_dev(d.data_ptr(), L, N, S, Cc, ws.data_ptr(), ws.numel(), stream)
            assert rc == -1 and opt in _lib.last_error()
            with pytest.raises(_lib.BpmfHipError, match=opt):
                _host(args, 1, True)
            hip_opts(opt, 0)
        torch.cuda.synchronize()


def test_plain_c_program_runs_full_mode(tmp_path):
    """tests/c_abi/abi_mf_full.c, built and run like tests/c_abi/abi_smoke.c (tests/test_gpu_c_abi.py)."""
    import os
    import subprocess
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "seismic_bpmf_amd", "lib")
    exe = str(tmp_path / "abi_mf_full")
    cmd = ["gcc", "-std=c99", "-O1", "-ffp-contract=off", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "c_abi", "abi_mf_full.c"), "-o", exe, "-L", libdir, "-lbpmf_hip", "-lm",
           "-Wl,--allow-shlib-undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([libdir, torch_lib, "/opt/rocm/lib", os.environ.get("LD_LIBRARY_PATH", "")]))
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.startswith("ok:"), run.stdout
    print(run.stdout)


# ------------------------------------------------------------------------------------------ host calls ---
def test_host_call_on_two_virtual_devices_equals_the_resident_result(hip_opts):
    import seismic_bpmf_amd as sb
    from seismic_bpmf_amd import _lib
    args, ref = _case("offset", 100, 20011, 1)
    hip_opts("mf.host_batch_kb", 64)                                # several template batches per device
    hip_opts("mf.host_piece_kb", 16)
    hip_opts("mf.host_piece_lags", 4096)                            # (no effect in full mode: the day goes up whole)
    want = {ns: _resident(args, 1, ns) for ns in (True, False)}
    one = _host(args, 1, True)
    hip_opts("debug.virtual_devices", 2)
    try:
        for ns in (True, False):
            got = sb.matched_filter_full(*args, 1, check_zeros=False, network_sum=ns, device=None)
            assert np.array_equal(got, want[ns])
            _judge("host", f"two virtual devices network_sum={ns}", got, ref, ns)
        assert np.array_equal(one, want[True])
        # short mode on the same devices, the same working sets, afterwards: its own bits
        short = sb.matched_filter(*args, 1, check_zeros=False, device=None)
    finally:
        _lib.release_device_memory(-1)
    hip_opts("debug.virtual_devices", 0)
    assert np.array_equal(short, sb.matched_filter(*args, 1, check_zeros=False, device=0))


# -------------------------------------------------------------------------------------------- workflow ---
def test_workflow_detections_with_full_normalisation(oracle_lib):
    """A short day whose channels carry offsets: the detections of matched_filter_detections(normalize="full") are those
    of the host selection (the oracle's RMS threshold, postprocess.select_cc_indexes) on the DEFINITION's CC -- which
    separates them from the threshold, and competing candidates from each other, by more than B_full."""
    from seismic_bpmf_amd import postprocess as pp, synthetic as syn, workflow
    T, S, Cc, L, N, sr, n_dev, overlap, window_dur, min_iet = 2, 2, 3, 64, 12_000, 100.0, 8.0, 0.25, 20.0, 2.0
    m = syn.make_mf_inputs(T=T, S=S, C=Cc, L=L, N=N, seed=77, max_moveout=100, n_events=3)
    data = (m["data"] + np.array([[50.0, -30.0, 8.0], [-400.0, 2.5, 1000.0]], np.float32)[:, :, None]).astype(np.float32)
    tp = (m["templates"] + np.float32(3.0)).astype(np.float32)
    wn = np.random.default_rng(0).standard_normal(500).astype(np.float32)
    kw = dict(sr=sr, threshold_window_dur=window_dur, minimum_interevent_time=min_iet, n_dev=n_dev, overlap=overlap,
              white_noise=wn, remove_edges=False)
    got, cc = workflow.matched_filter_detections(tp, m["moveouts"], m["weights"], data, normalize="full", **kw)
    ref = mfd.mf_full_f64(tp, m["moveouts"], m["weights"], data)
    _judge("workflow", "the CC matrix", cc.cpu().numpy(), ref, True)
    cc_def = ref.net.astype(np.float32)
    window = int(pp.sec_to_samp(window_dur, sr))
    w = m["weights"]
    n_found = 0
    for t in range(T):
        thr = oracle_lib.time_dependent_threshold(cc_def[t], window, n_dev, overlap, wn)
        thr = np.minimum(thr, np.float32((0.80 * w.reshape(T, -1).sum(axis=1))[t]))
        win = workflow.search_window(m["moveouts"][t].reshape(S, -1), int(pp.sec_to_samp(min_iet, sr)), 1)
        want = pp.select_cc_indexes(cc_def[t], thr, win, step=1, sr=sr, data_duration_sec=1e9, n_dev_threshold=n_dev,
                                    min_freq_hz=2.0, data_buffer_sec=0.0, remove_edges=False,
                                    anomalous_cdf_at_mean_plus_1sig=0.0)
        # the margins: a perturbation of the CC within B moves the threshold by at most (1 + n_dev) max B
        b_max = float(ref.B_net[t].max())
        margin = 2 * (2 + n_dev) * b_max
        assert np.abs(ref.net[t] - thr.astype(np.float64)).min() > margin
        cand = np.flatnonzero(cc_def[t] > thr)
        for a, b in zip(cand[:-1], cand[1:]):
            assert b - a >= win or abs(ref.net[t, a] - ref.net[t, b]) > 2 * b_max
        planted = sorted(i0 for tt, i0 in m["planted"] if tt == t)
        assert list(want) == planted and np.array_equal(got[t], want), (t, got[t], want, planted)
        n_found += len(want)
    assert n_found == 6
    # short mode on this day is not the correlation: the offsets drown it
    _, cc_short = workflow.matched_filter_detections(tp, m["moveouts"], m["weights"], data, **kw)
    assert np.abs(cc_short.cpu().numpy().astype(np.float64) - ref.net).max() > 0.3
