"""The case table of tests/test_gpu_guard_bands.py: one small call per device-pointer entry point, described so that
the test can cut every buffer of it from a fenced arena (tests/arena.py).

A case is a `Call`:
    inputs      {name: NumPy array}                         uploaded as they are
    outputs     {name: (shape, dtype)} or {name: (shape, dtype, initial body)}   (0xFF bytes without a body)
    variants    [{workspace name: bytes}, ...]              the workspace sizes the call must accept; [{}] for none
    refusal     {workspace name: bytes} or None             sizes the call must refuse (one byte under the smallest)
    invoke      f(lib, p, nbytes, stream) -> status         p: {region name: c_void_p}, nbytes: {workspace name: bytes}
    verify      f(out) -> None                              out: {output name: NumPy array}; asserts the entry point's
                                                            own comparison against its host definition or oracle
    options     {library option: value} set around the call
    before      f(lib) / after f(lib)                       host-side set-up that needs the device (a plan)

The shapes are the smallest at which each carve-up can go wrong; tests/test_arena_host.py asserts the premises that can
be computed without a device.  No tolerance is introduced here: every `verify` is the comparison the entry point's own
test already makes.  Inputs come from fixed seeds; definitions are computed once per case (functools.lru_cache)."""
import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HERE = os.path.dirname(os.path.abspath(__file__))


class Call:
    def __init__(self, name, entry, inputs, outputs, invoke, verify, variants=None, refusal=None, options=None,
                 before=None, after=None):
        self.name, self.entry, self.inputs, self.outputs = name, entry, inputs, outputs
        self.invoke, self.verify = invoke, verify
        self.variants = variants if variants is not None else [{}]
        self.refusal, self.options = refusal, dict(options or {})
        self.before, self.after = before, after
        self.refusal_invoke = None      # the call to refuse, where it is not `invoke` (a pair of calls: its second)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# =================================================================== tier 1: entry points with a caller's workspace ===
# ---- bpmf_tdt_rms_dev: two cases of threshold_cases.tdt_cases(), one of the lane group, one of the stream group ----
def tdt_rms_calls(lib):
    import threshold_cases as tc
    calls = []
    for group, name in (("lanes", "lanes_65_as_5x13"), ("stream", "stream_w194_s145")):
        case = tc.tdt_case(name)
        assert case.group == group
        rows, n = case.x.shape
        n_win = tc.tdt_sizes(n, case.half, case.shift)[2]
        need = lib.bpmf_tdt_workspace_bytes(rows, n, case.half, case.shift)
        want = tc.tdt_rms_definition(case.x, case.gauss, case.num_dev, case.half, case.shift)

        def invoke(lib, p, nb, stream, case=case, rows=rows, n=n):
            return lib.bpmf_tdt_rms_dev(p["x"], p["gauss"], float(case.num_dev), rows, n, case.half, case.shift, p["ws"],
                                        nb["ws"], stream, p["thr_win"], p["full"])

        def verify(out, want=want, tc=tc, name=case.name):
            assert tc.same_values(out["thr_win"], want[0]) and tc.same_values(out["full"], want[1]), name

        calls.append(Call(f"tdt_rms:{case.name}", "bpmf_tdt_rms_dev",
                          {"x": case.x, "gauss": np.ascontiguousarray(case.gauss, np.float32)},
                          {"thr_win": ((rows, n_win), np.float32), "full": ((rows, n), np.float32)},
                          invoke, verify, [{"ws": need}], {"ws": need - 1}))
    return calls


# ---- bpmf_multiband_spectrum_dev ----
MB_E, MB_S, MB_C, MB_N_SAMPLES, MB_BUFFER = 11, 2, 3, 130, 10
MB_TIME_TILE = 64                       # samples of one tile of mb_prepare_kernel (csrc/spectrum.hip)


@functools.lru_cache(maxsize=None)
def multiband_inputs():
    """(day (S, C, N), starts (E, S), plan, want spectra, want valid, scale): 66 rows, one start -1, one N - n."""
    import multiband_cases as mc
    from seismic_bpmf_amd import postprocess as pp
    E, S, Cc, n = MB_E, MB_S, MB_C, MB_N_SAMPLES
    rng = np.random.default_rng([4100, 66])
    N = E * n + 40
    day = (1e-6 * rng.standard_normal((S, Cc, N)) + 3e-5 + 2e-5 * rng.uniform(-1, 1, (S, Cc, 1)) * np.arange(N) / N)
    day = day.astype(np.float32)
    starts = 3 + np.arange(E, dtype=np.int64)[:, None] * n + np.arange(S, dtype=np.int64)[None, :]
    starts[0, 0] = -1                                   # cut by the start of the day: not processed
    starts[E - 1, S - 1] = N - n                        # ends with the day's last sample (of the input's last rows)
    buffer_seconds = MB_BUFFER / mc.SAMPLING_RATE
    windows, valid = pp.multiband_windows_host(day, starts, n)
    want, _ = pp.multiband_spectrum_host(windows, mc.OCTAVES, sr=mc.SAMPLING_RATE, buffer_seconds=buffer_seconds)
    plan = pp.multiband_plan(n, mc.OCTAVES, mc.SAMPLING_RATE, buffer_seconds, 4)
    prepared = pp.multiband_prepare_host(windows.reshape(-1, n), plan["taper"]).reshape(windows.shape)
    return day, starts, plan, want, valid, mc.row_scale(windows, prepared)


def multiband_calls(lib):
    import golden_npz
    import multiband_cases as mc
    day, starts, plan, want, valid, scale = multiband_inputs()
    limit = float(golden_npz.load(os.path.join(HERE, "golden", "multiband.npz"))["limit"])
    E, S, Cc, n = MB_E, MB_S, MB_C, MB_N_SAMPLES
    B, n_active = len(plan["bands"]), int((~plan["skip"]).sum())
    assert (B, n_active, plan["buffer"]) == (8, 6, MB_BUFFER)
    bandwidth = np.ascontiguousarray(plan["bandwidth"], np.float64)
    skip = np.ascontiguousarray(plan["skip"], np.uint8)
    sos = np.ascontiguousarray(plan["sos"], np.float64)
    one_slab = lib.bpmf_multiband_workspace_bytes(E * S * Cc, n, n_active)
    least = lib.bpmf_multiband_workspace_bytes(64, n, n_active)

    def invoke(lib, p, nb, stream):
        return lib.bpmf_multiband_spectrum_dev(
            p["day"], S, Cc, day.shape[2], E * S, p["starts"], n, int(plan["taper"]), int(plan["buffer"]), p["sos"], B,
            int(sos.shape[1]), bandwidth.ctypes.data_as(C.POINTER(C.c_double)), skip.ctypes.data_as(C.POINTER(C.c_uint8)),
            p["ws"], nb["ws"], stream, p["spectra"], p["valid"])

    def verify(out):
        got = out["spectra"].reshape(want.shape)
        assert np.array_equal(out["valid"].reshape(valid.shape), valid.astype(np.uint8))
        assert not valid[0, 0] and valid.sum() == valid.size - 1
        assert not got[~valid].any() and not np.signbit(got[~valid]).any()
        dev = mc.deviation(got, want, scale, mc.OCTAVES)
        assert dev <= limit, dev / limit
        assert not got[..., plan["skip"]].any() and (got[valid][..., ~plan["skip"]] > 0).all()

    return [Call("multiband:66_rows", "bpmf_multiband_spectrum_dev",
                 {"day": day, "starts": starts.reshape(-1), "sos": sos},
                 {"spectra": ((E * S, Cc, B), np.float64), "valid": ((E * S,), np.uint8)},
                 invoke, verify, [{"ws": one_slab}, {"ws": least}], {"ws": least - 1})]


# ---- bpmf_svdwf_stack_dev ----
SV_OFFSETS, SV_S, SV_C, SV_M = (0, 0, 5, 14), 1, 2, 48


@functools.lru_cache(maxsize=None)
def svdwf_inputs():
    import svdwf_cases as sc
    from seismic_bpmf_amd import postprocess as pp
    off = np.array(SV_OFFSETS, dtype=np.int64)
    x = np.concatenate([sc.group(int(n), SV_M, 60 + g, SV_S, SV_C) for g, n in enumerate(np.diff(off))], axis=0)
    sos = sc.sos_table()
    want = pp.svdwf_stack_host(x, off, sos=sos)
    return x, off, np.ascontiguousarray(sos, np.float64), want


def svdwf_calls(lib):
    import svdwf_cases as sc
    from seismic_bpmf_amd import postprocess as pp
    x, off, sos, want = svdwf_inputs()
    want_filtered, want_stack, want_rank = want
    G, N, S, Cc, m = len(off) - 1, len(x), SV_S, SV_C, SV_M
    n_max = int(np.diff(off).max())
    expl_var, kmax, w = pp.svdwf_arguments(N, m, 0.4, 5, None)
    all_slots = lib.bpmf_svdwf_workspace_bytes(G, n_max, m, G * S * Cc)
    one_slot = lib.bpmf_svdwf_workspace_bytes(G, n_max, m, 1)

    def invoke(lib, p, nb, stream):
        return lib.bpmf_svdwf_stack_dev(p["x"], off.ctypes.data_as(C.POINTER(C.c_int64)), G, S, Cc, m, expl_var, kmax,
                                        0 if w is None else w, p["sos"], sos.shape[0], 0.01, p["ws"], nb["ws"], stream,
                                        p["filtered"], p["stack"], p["n_singular"], p["status"])

    def verify(out):
        # the header's bounds, as tests/test_gpu_svdwf.py: compare applies them
        assert not out["status"].any()
        assert np.array_equal(out["n_singular"], want_rank)
        for g in range(G):
            for s in range(S):
                for c in range(Cc):
                    hf = want_filtered[off[g]:off[g + 1], s, c]
                    df = np.abs(out["filtered"][off[g]:off[g + 1], s, c] - hf).max() / sc.scale(hf) if hf.size else 0.0
                    ds = np.abs(out["stack"][g, s, c] - want_stack[g, s, c]).max() / sc.scale(want_stack[g, s, c])
                    assert df <= 2.0 ** -22 and ds <= 2.0 ** -21, (g, s, c, df * 2.0 ** 22, ds * 2.0 ** 21)
        assert not out["stack"][0].any() and not out["n_singular"][0].any()          # the empty group

    return [Call("svdwf:empty_group_n_below_m", "bpmf_svdwf_stack_dev", {"x": x, "sos": sos},
                 {"filtered": ((N, S, Cc, m), np.float32), "stack": ((G, S, Cc, m), np.float32),
                  "n_singular": ((G, S, Cc), np.int32), "status": ((G, S, Cc), np.int32)},
                 invoke, verify, [{"ws": all_slots}, {"ws": one_slot}], {"ws": one_slot - 1})]


# ---- bpmf_bandpass_rows_dev ----
BAND_ROWS, BAND_N, BAND_SECTIONS = 70, 100, 4


@functools.lru_cache(maxsize=None)
def bandpass_inputs():
    from seismic_bpmf_amd import postprocess as pp
    rng = np.random.default_rng(3100)
    x = (rng.standard_normal((BAND_ROWS, BAND_N)) + rng.uniform(-3, 3, (BAND_ROWS, 1))
         + rng.uniform(-.01, .01, (BAND_ROWS, 1)) * np.arange(BAND_N)).astype(np.float32)
    sos = np.ascontiguousarray(pp.butter_bandpass_sos(BAND_SECTIONS, 0.1, 0.4), np.float64)
    assert sos.shape == (BAND_SECTIONS, 6)
    want = pp.bandpass_filter_host(x, sos, detrend=True, taper_alpha=0.1, zerophase=True)
    return x, sos, want


def bandpass_calls(lib):
    import svdwf_cases as sc
    x, sos, want = bandpass_inputs()
    limit = float(np.load(os.path.join(HERE, "golden", "svdwf.npz"))["bandpass_limit"])
    calls = []
    for out_f64 in (0, 1):
        need = lib.bpmf_bandpass_rows_workspace_bytes(BAND_ROWS, BAND_N, 1, out_f64)
        assert (need == 0) == bool(out_f64)

        def invoke(lib, p, nb, stream, out_f64=out_f64):
            return lib.bpmf_bandpass_rows_dev(p["x"], 0, BAND_ROWS, BAND_N, p["sos"], BAND_SECTIONS, 1, 0.1, 1, out_f64,
                                              p.get("ws"), nb.get("ws", 0), stream, p["out"])

        def verify(out, out_f64=out_f64):
            # tests/test_gpu_svdwf.py::test_full_bandpass_is_within_the_recorded_limit: float64 within the recorded
            # limit, float32 within 2^-22 of the largest value
            if out_f64:
                assert np.abs(out["out"] - want).max() <= limit * sc.scale(want)
            else:
                want32 = want.astype(np.float32)
                assert np.abs(out["out"] - want32).max() <= 2.0 ** -22 * sc.scale(want32)

        calls.append(Call(f"bandpass:{'f64_null_workspace' if out_f64 else 'f32_zero_phase'}", "bpmf_bandpass_rows_dev",
                          {"x": x, "sos": sos}, {"out": ((BAND_ROWS, BAND_N), np.float64 if out_f64 else np.float32)},
                          invoke, verify, [{}] if out_f64 else [{"ws": need}], None if out_f64 else {"ws": need - 1}))
    return calls


# ---- bpmf_flag_multiples_dev ----
def multiples_calls(lib):
    import multiples_cases as mc
    from seismic_bpmf_amd import postprocess as pp
    calls = []
    named = {c[0]: c for c in mc.named_cases()}
    for name in ("neighbours_65", "time_ties"):
        _, t, rows, cc, ok, dt = named[name]
        n, T = len(t), ok.shape[0]
        assert n == {"neighbours_65": 130, "time_ties": 240}[name]
        order = np.argsort(t, kind="stable")
        want = pp.flag_multiples(t, rows, cc, ok, dt)[order].astype(np.uint8)
        need = lib.bpmf_flag_multiples_workspace_bytes(n)

        def invoke(lib, p, nb, stream, n=n, T=T, dt=dt):
            return lib.bpmf_flag_multiples_dev(p["t"], p["rows"], p["cc"], n, p["ok"], T, dt, p["ws"], nb["ws"], stream,
                                               p["unique"])

        def verify(out, want=want, name=name):
            assert np.array_equal(out["unique"], want), (name, np.flatnonzero(out["unique"] != want)[:10])

        calls.append(Call(f"multiples:{name}", "bpmf_flag_multiples_dev",
                          {"t": t[order], "rows": rows[order].astype(np.int32), "cc": cc[order],
                           "ok": np.ascontiguousarray(ok, np.uint8)},
                          {"unique": ((n,), np.uint8)}, invoke, verify, [{"ws": need}], {"ws": need - 1}))
    return calls


# ---- bpmf_intertemplate_cc_dev ----
INTERTP_SHAPES = [(9, 2, 1, 40, 0), (12, 3, 2, 1300, 12)]            # (T, S, C, Lw, max_lag)


def intertp_inputs(T, S, Cc, Lw, seed):
    """Waveforms, channel weights and the ragged pair mask of tests/test_gpu_workflow.py's batched test."""
    rng = np.random.default_rng([21, seed])
    wf = rng.standard_normal((T, S, Cc, Lw)).astype(np.float32)
    wf[1] = np.roll(wf[0], 2, axis=-1)
    wf[2, 1, 0] = 0.0                                   # dead template channel -> CC 0 there
    base = (rng.random((T, S, Cc)) > 0.3).astype(np.float32)
    base[:, 0, :] = 1.0
    base[3] = 0.0                                       # a template without any weighted channel
    base /= np.maximum(base.sum(axis=(1, 2), keepdims=True), 1.0)
    mask = rng.random((T, T)) > 0.4
    mask[np.arange(T), np.arange(T)] = True
    mask[4] = False                                     # a template with no partner at all
    return wf, base, mask


def intertemplate_calls(lib):
    calls = []
    for k, (T, S, Cc, Lw, max_lag) in enumerate(INTERTP_SHAPES):
        wf, base, mask = intertp_inputs(T, S, Cc, Lw, k)
        need = lib.bpmf_intertemplate_workspace_bytes(T, S, Cc, max_lag)
        want = {}

        def invoke(lib, p, nb, stream, T=T, S=S, Cc=Cc, Lw=Lw, max_lag=max_lag):
            return lib.bpmf_intertemplate_cc_dev(p["wf"], p["base"], p["mask"], T, S, Cc, Lw, max_lag, p["ws"], nb["ws"],
                                                 stream, p["out"])

        def verify(out, wf=wf, base=base, mask=mask, max_lag=max_lag, want=want):
            # the reference's per-template loop on the device's matched filter, as test_gpu_workflow.py compares
            if "m" not in want:
                from seismic_bpmf_amd import workflow
                full = base[:, None, :, :] * mask[:, :, None, None]
                want["m"] = workflow.intertemplate_cc_loop(wf, full, max_lag=max_lag, symmetrise=False)
            assert np.array_equal(out["out"], want["m"]), np.argwhere(out["out"] != want["m"])[:5]
            assert not out["out"][4].any() and not out["out"][3].any()

        calls.append(Call(f"intertemplate:T{T}_Lw{Lw}_lag{max_lag}", "bpmf_intertemplate_cc_dev",
                          {"wf": wf, "base": base, "mask": np.ascontiguousarray(mask, np.uint8)},
                          {"out": ((T, T), np.float32)}, invoke, verify, [{"ws": need}], {"ws": need - 1}))
    return calls


# ---- bpmf_row_median_mad_ws_dev ----
def median_rows(n):
    """The 16 rows of tests/test_gpu_threshold.py::test_row_median_mad_two_read_path_equals_the_one_workgroup_path."""
    rng = np.random.default_rng(n)
    rows = [rng.standard_normal(n) * 0.05, np.abs(rng.standard_normal(n)), np.full(n, 0.25), rng.choice([-0.5, 0.75], n),
            rng.standard_cauchy(n) * 0.01, rng.standard_normal(n) * 0.05 + np.linspace(-3.0, 3.0, n),
            np.round(rng.standard_normal(n) * 4) / 64, rng.standard_normal(n) * 1e-30, rng.standard_normal(n) * 0.05,
            rng.standard_normal(n) * 0.05, rng.standard_normal(n) * 0.05, rng.standard_normal(n) * 0.001 + 1000.0,
            rng.lognormal(0.0, 2.0, n), rng.standard_normal(n) * 0.05, np.zeros(n), rng.standard_normal(n) * 0.05]
    x = np.stack(rows).astype(np.float32)
    x[1, rng.random(n) < 0.55] = 0.0
    x[8, n // 3] = np.inf
    x[8, n // 2] = -np.inf
    x[9, n // 2] = np.nan
    x[10, : n // 2] = 0.0
    stride = max(1, n // 4096)
    x[13, ::stride] = 50.0 + rng.standard_normal(len(x[13, ::stride])).astype(np.float32)
    x[15, -1] = -0.0
    return x


def median_mad_calls(lib):
    import warnings
    from seismic_bpmf_amd import _lib
    calls = []
    for n, min_n in ((4096, 0), (5, None)):
        x = median_rows(n)
        rows = len(x)
        with _lib.options(**({"stats.row_grid_min_n": min_n} if min_n is not None else {})):
            need = lib.bpmf_row_median_mad_workspace_bytes(rows, n)       # (the size depends on the option)
        assert (need > 256) == (min_n == 0)
        for skip in (0, 1):
            want_med, want_mad = np.empty(rows, np.float32), np.empty(rows, np.float32)
            for r in range(rows):
                v = x[r][x[r] != 0] if skip else x[r]
                with np.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    m = np.median(v) if v.size else np.float32(np.nan)
                    want_mad[r] = np.median(np.abs(v - m)) if v.size else np.float32(np.nan)
                    want_med[r] = m
            want_nz = (x == 0).sum(axis=1).astype(np.int64)

            def invoke(lib, p, nb, stream, rows=rows, n=n, skip=skip):
                return lib.bpmf_row_median_mad_ws_dev(p["x"], rows, n, skip, p["ws"], nb["ws"], stream, p["median"],
                                                      p["mad"], p["n_zero"])

            def verify(out, want_med=want_med, want_mad=want_mad, want_nz=want_nz, label=(n, skip)):
                assert np.array_equal(out["median"], want_med, equal_nan=True), label
                assert np.array_equal(out["mad"], want_mad, equal_nan=True), label
                assert np.array_equal(out["n_zero"], want_nz), label

            calls.append(Call(f"median_mad:n{n}_skip{skip}", "bpmf_row_median_mad_ws_dev", {"x": x},
                              {"median": ((rows,), np.float32), "mad": ((rows,), np.float32), "n_zero": ((rows,), np.int64)},
                              invoke, verify, [{"ws": need}], None,
                              options={"stats.row_grid_min_n": min_n} if min_n is not None else None))
    return calls


# ---- bpmf_tdt_mad_dev ----
MAD_ROWS, MAD_N, MAD_W, MAD_SHIFT, MAD_OVERLAP = 3, 7777, 500, 50, 0.899


def tdt_mad_calls(lib):
    from seismic_bpmf_amd import postprocess as pp
    rows, n, W, shift = MAD_ROWS, MAD_N, MAD_W, MAD_SHIFT
    assert int((1.0 - MAD_OVERLAP) * W) == shift
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((rows, n)) * 0.05).astype(np.float32)
    x[rng.random((rows, n)) < 0.02] = 0.0
    x[0, 1000:1400] = 0.0
    x[2, -300:] = 0.0
    wn = rng.standard_normal(int((x == 0).sum(axis=1).max())).astype(np.float32)
    assert wn.size < n                                    # (the call checks the rows' zeros against it)
    want = np.stack([pp.time_dependent_threshold_mad(x[r], W, 8.0, overlap=MAD_OVERLAP, white_noise=wn)
                     for r in range(rows)]).astype(np.float32)
    n_win = lib.bpmf_tdt_mad_num_windows(n, W, shift)
    need = lib.bpmf_tdt_mad_workspace_bytes(rows, n, W, shift)
    half = W // 2
    seen = np.arange(half, n - (W - half))                # the samples of the expansion that show a window's value
    windows = {}
    calls = []
    for expand in (1, 0):
        def invoke(lib, p, nb, stream, expand=expand):
            return lib.bpmf_tdt_mad_dev(p["x"], p["wn"], wn.size, 8.0, rows, n, W, shift, p["ws"], nb["ws"], stream,
                                        p["thr_win"], p["full"] if expand else None, p["n_zero"])

        def verify(out, expand=expand):
            assert np.array_equal(out["n_zero"], (x == 0).sum(axis=1))
            if expand:
                assert np.array_equal(out["full"], want), np.argwhere(out["full"] != want)[:5]
                which = np.minimum(seen // shift, n_win - 1)
                assert np.array_equal(out["thr_win"][:, which], want[:, seen])
                windows["with"] = out["thr_win"]
            else:                                         # the same window values without the expansion
                assert same_bits(out["thr_win"], windows["with"])

        outputs = {"thr_win": ((rows, n_win), np.float32), "n_zero": ((rows,), np.int64)}
        if expand:
            outputs["full"] = ((rows, n), np.float32)
        calls.append(Call(f"tdt_mad:{'expanded' if expand else 'windows_only'}", "bpmf_tdt_mad_dev", {"x": x, "wn": wn},
                          outputs, invoke, verify, [{"ws": need}], {"ws": need - 1}))
    return calls


# ---- bpmf_row_kurtosis_dev / bpmf_row_kurtosis_parts_dev ----
def kurtosis_calls(lib):
    from seismic_bpmf_amd import postprocess as pp
    calls = []
    for n in (129, 8193):
        rows = 3
        rng = np.random.default_rng([11, n])
        x = (rng.standard_normal((rows, n)) * rng.uniform(0.01, 2.0, (rows, 1)) + rng.uniform(-1, 1, (rows, 1)))
        x = x.astype(np.float32)
        x[1, : n // 2] = 0.0
        x[2] = x[2, 0]                                    # a constant row: NaN
        with np.errstate(all="ignore"):
            want = np.array([pp.excess_kurtosis_f32(r) for r in x], dtype=np.float32)
            # the same expression on ARRAYS (the exact square), which is what bpmf_row_kurtosis_dev itself stores
            mean = np.mean(x, axis=1, keepdims=True)
            s2 = (x - mean) ** 2
            m2, m4 = np.mean(s2, axis=1), np.mean(s2 ** 2, axis=1)
            want_array = np.where(m2 <= (np.finfo(np.float32).eps * mean[:, 0]) ** 2, np.float32(np.nan),
                                  m4 / m2 ** 2.0 - np.float32(3)).astype(np.float32)
        assert np.isfinite(want[:2]).all()
        need = lib.bpmf_row_kurtosis_workspace_bytes(rows, n)
        for parts in (0, 1):
            def invoke(lib, p, nb, stream, parts=parts, rows=rows, n=n):
                if parts:
                    return lib.bpmf_row_kurtosis_parts_dev(p["x"], rows, n, p["ws"], nb["ws"], stream, p["kurtosis"],
                                                           p["parts"])
                return lib.bpmf_row_kurtosis_dev(p["x"], rows, n, p["ws"], nb["ws"], stream, p["kurtosis"])

            def verify(out, parts=parts, want=want, want_array=want_array, n=n):
                assert np.array_equal(out["kurtosis"], want_array, equal_nan=True), (n, out["kurtosis"], want_array)
                if parts:
                    got = pp.kurtosis_from_moments_rows(out["parts"])
                    assert np.array_equal(got, want, equal_nan=True), (n, got, want)

            outputs = {"kurtosis": ((rows,), np.float32)}
            if parts:
                outputs["parts"] = ((rows, 3), np.float32)
            calls.append(Call(f"kurtosis:n{n}{'_parts' if parts else ''}",
                              "bpmf_row_kurtosis_dev", {"x": x}, outputs, invoke, verify, [{"ws": need}], None))
    return calls


# ---- bpmf_mf_run_dev (and bpmf_mf_prepare_data_full_dev) ----
MF_L = 17
MF_FORCE_DIRECT, MF_PREPARED, MF_FULL = 2, 1, 4
MF_SPLIT_TOL = 2e-5                       # tests/test_gpu_split16.py: TOL_CC, per unit of sum |w| / per channel


def oracle_module():
    from oracle import oracle
    if not os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "liboracle.so")):
        oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def mf_inputs():
    from test_gpu_mf_phase_window import _inputs
    return _inputs(MF_L)


@functools.lru_cache(maxsize=None)
def mf_oracle(step, ns):
    tp, mv, w, d, N = mf_inputs()
    return oracle_module().matched_filter(tp, mv, w, d, step, ns)


@functools.lru_cache(maxsize=None)
def mf_full_reference(step):
    import mf_full_definition as mfd
    tp, mv, w, d, N = mf_inputs()
    lags = mfd.mf_full_lags((tp, mv, w, d), step, seed=MF_L)
    return mfd.mf_full_f64(tp, mv, w, d, step=step, lags=lags)


def mf_calls(lib):
    import f64_anchor as fa
    from mf_launch import assert_takes
    from seismic_bpmf_amd import _lib
    tp, mv, w, d, N = mf_inputs()
    T, S, Cc, L = tp.shape
    calls = []
    # (label, flags, options, family asserted, comparison)
    families = [("direct", MF_FORCE_DIRECT, {}, "direct", "oracle"),
                ("wave", 0, {}, "wave", "oracle"),
                ("split16", 0, {"mf.split16": 2}, "split16", "split16"),
                ("full", MF_FULL, {}, "wave", "full"),
                ("full_prepared", MF_FULL | MF_PREPARED, {}, "wave", "full")]
    for label, flags, opts, family, comparison in families:
        with _lib.options(**opts):
            need = (lib.bpmf_mf_full_workspace_bytes if flags & MF_FULL else lib.bpmf_mf_workspace_bytes)(L, N, T, S, Cc)
            for step in (1, 3):
                for ns in (1, 0):
                    assert_takes(tp.shape, N, step, bool(ns), flags=flags & ~MF_PREPARED, family=family)
        for step in (1, 3):
            n_corr = (N - L) // step + 1
            for ns in (1, 0):
                def invoke(lib, p, nb, stream, flags=flags, step=step, ns=ns, n_corr=n_corr, prepare=True):
                    if flags & MF_PREPARED and prepare:          # the pair shares one workspace
                        rc = lib.bpmf_mf_prepare_data_full_dev(p["data"], L, N, S, Cc, p["ws"], nb["ws"], stream)
                        if rc:
                            return rc
                    return lib.bpmf_mf_run_dev(p["tp"], p["mv"], p["w"], p["data"], step, L, N, T, S, Cc, n_corr, ns,
                                               flags if prepare else flags & ~MF_PREPARED, p["ws"], nb["ws"], stream,
                                               p["cc"])

                def verify(out, comparison=comparison, step=step, ns=ns, label=label):
                    got = out["cc"]
                    if comparison == "oracle":
                        want = mf_oracle(step, bool(ns))
                        assert np.array_equal(got, want), (label, step, ns, int((got != want).sum()))
                    elif comparison == "split16":               # tests/test_gpu_split16.py: _check
                        want = mf_oracle(step, bool(ns))
                        assert np.isfinite(got).all()
                        odd = (got == 0.0) != (want == 0.0)
                        assert not odd.any() or np.abs(got[odd]).max() < 1e-30
                        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
                        if ns:
                            diff = diff / np.maximum(np.abs(w).reshape(T, -1).sum(axis=1)[:, None], 1e-30)
                        assert diff.max() <= MF_SPLIT_TOL, (label, step, ns, diff.max())
                    else:                                       # tests/test_gpu_mf_full.py: _judge
                        ref = mf_full_reference(step)
                        got = fa.mf_full(got, ref)
                        fa.mf_compare(got, ref, bool(ns), f"guard bands MF {label} step={step} network_sum={ns}").require()
                        if not ns:
                            assert not got[ref.flat].view(np.uint32).any()

                call = Call(f"mf:{label}_step{step}_ns{ns}", "bpmf_mf_run_dev",
                            {"tp": tp, "mv": mv, "w": w, "data": d},
                            {"cc": ((T, n_corr) if ns else (T, n_corr, S, Cc), np.float32)},
                            invoke, verify, [{"ws": need}], {"ws": need - 1}, options=opts)
                # the refused call is the run alone (it implies the preparation, and checks the size first)
                call.refusal_invoke = functools.partial(invoke, prepare=False)
                calls.append(call)
    return calls


# ---- bpmf_bp_run_dev ----
BP_GRID, BP_S, BP_P, BP_SR, BP_CLOSEST, BP_C, BP_N = (12, 12, 6), 9, 2, 50.0, 5, 3, 700
RELOC_E, RELOC_N = 3, 300


@functools.lru_cache(maxsize=None)
def bp_geometry():
    from seismic_bpmf_amd import synthetic as syn
    geo = syn.make_bp_geometry(BP_GRID, BP_S, BP_P, BP_SR, n_closest=BP_CLOSEST)
    return (np.ascontiguousarray(geo["moveouts"], np.int32), np.ascontiguousarray(geo["weights_sources"], np.float32),
            syn.phase_weights(BP_S, BP_C, BP_P), syn.geographic_coordinates(geo["sources"], (30.0, 40.0)))


def make_plan(lib, tau, ws):
    import torch
    from seismic_bpmf_amd import _lib
    plan = C.c_void_p()
    K, S, P = tau.shape
    _lib.check(lib.bpmf_bp_plan_create(tau.ctypes.data_as(_lib._i), ws.ctypes.data_as(_lib._f), K, S, P,
                                       torch.cuda.current_device(), 0, C.byref(plan)), "bpmf_bp_plan_create")
    return plan


def destroy_plans(plans):
    def after(lib, state):
        while plans:
            lib.bpmf_bp_plan_destroy(plans.pop())
    return after


def bp_run_calls(lib):
    from seismic_bpmf_amd import _lib, synthetic as syn
    tau, ws, wp, _ = bp_geometry()
    K = tau.shape[0]
    f, _ = syn.make_bp_features(tau, BP_S, BP_C, BP_N, sr=BP_SR)
    plans, calls = [], []
    cases = [(reduce, oob, {}) for reduce in ("max", "none") for oob in ("strict", "flexible")]
    cases.append(("max", "strict", {"bp.direct": 1}))
    for reduce, oob, opts in cases:
        with _lib.options(**opts):
            plan = make_plan(lib, tau, ws)                # (a plan keeps the variant it was built with)
            plans.append(plan)
            need = lib.bpmf_bp_workspace_bytes(plan, BP_N, BP_C)
            info = _lib.bp_launch_info(tau, ws, BP_N, reduce)
        assert need == info["schedule"]["total"] and (info["shape"]["direct"] == "bp.direct") == bool(opts)

        def invoke(lib, p, nb, stream, plan=plan, reduce=reduce, oob=oob):
            return lib.bpmf_bp_run_dev(plan, p["f"], p["wp"], BP_N, BP_C, {"strict": 0, "flexible": 1}[oob],
                                       {"max": 0, "none": 1}[reduce], p["ws"], nb["ws"], stream, p["beam"], p.get("arg"))

        def verify(out, reduce=reduce, oob=oob):
            want = oracle_module().beamform(f, tau, wp, ws, oob, reduce)
            if reduce == "max":
                assert np.array_equal(out["beam"], want[0]) and np.array_equal(out["arg"], want[1]), (reduce, oob)
            else:
                assert np.array_equal(out["beam"], want), (reduce, oob)

        outputs = {"beam": ((BP_N,), np.float32), "arg": ((BP_N,), np.int32)} if reduce == "max" \
            else {"beam": ((K, BP_N), np.float32)}
        calls.append(Call(f"bp_run:{reduce}_{oob}{'_direct' if opts else ''}", "bpmf_bp_run_dev", {"f": f, "wp": wp},
                          outputs, invoke, verify, [{"ws": need}], {"ws": need - 1}, options=opts))
    calls[-1].after = destroy_plans(plans)
    return calls


# ---- bpmf_bp_relocate_batch_dev, then bpmf_bp_location_uncertainty_dev on its outputs where they lie ----
def relocate_events_input(tau):
    """(E, S, C, N): an event of rounded features (exact ties), one with a planted arrival, an all-zero one -- events
    0, 3 and 2 of tests/test_gpu_relocate_batch.py: make_events."""
    from test_gpu_relocate_batch import make_events
    return np.ascontiguousarray(make_events(tau, RELOC_N, seed=RELOC_N, n_events=4)[[0, 3, 2]])


def relocate_calls(lib):
    from seismic_bpmf_amd import beampower, postprocess as pp, workflow
    tau, ws, wp, coords = bp_geometry()
    K, E, N = tau.shape[0], RELOC_E, RELOC_N
    f = relocate_events_input(tau)
    assert f.shape == (E, BP_S, BP_C, N) and not f[2].any()
    tables = beampower.source_coordinate_tables(*coords, K)
    plan = make_plan(lib, tau, ws)
    plans = [plan]
    need = lib.bpmf_bp_relocate_workspace_bytes(plan, E, N, BP_C)
    kT, cutoff, side = 0.33, 0.25, 100.0
    calls = []
    for method, n_terms in (("spatial", K), ("temporal", N)):
        need_unc = lib.bpmf_bp_location_uncertainty_workspace_bytes(E, n_terms)
        spatial = method == "spatial"

        def invoke(lib, p, nb, stream, spatial=spatial):
            rc = lib.bpmf_bp_relocate_batch_dev(
                plan, p["f"], BP_S * BP_C * N, N, None, p["wp"], p["tau"] if spatial else None,
                p["w_sources"] if spatial else None, E, N, BP_C, 1, 0 if spatial else 1, p["ws"], nb["ws"], stream,
                p["time_idx"], p["src_idx"], p["max_beam"], p.get("likelihood"), p.get("columns"), p.get("maxbeam"),
                p.get("maxbeam_sources"))
            if rc:
                return rc
            return lib.bpmf_bp_location_uncertainty_dev(
                plan, 0 if spatial else 1, E, N, p["src_idx"], p.get("likelihood"), p.get("maxbeam"),
                p.get("maxbeam_sources"), p["max_beam"], p["tables"], pp.domain_scale_per_longitude(), side / 2.0, kT,
                cutoff, p["ws_unc"], nb["ws_unc"], stream, p["hunc"], p["vunc"], p["n_domain"], p["longitude"],
                p["latitude"], p["depth"], p.get("domain"))

        def verify(out, spatial=spatial, method=method):
            from test_gpu_location_uncertainty import close, no_sample_near_the_cutoff
            oracle = oracle_module()
            lon, lat, dep = coords
            for e in range(E):                            # tests/test_gpu_relocate_batch.py, np.array_equal throughout
                if spatial:
                    vol = oracle.beamform(f[e], tau, wp, ws, "flexible", "none")
                    k, t = np.unravel_index(vol.argmax(), vol.shape)
                    assert (out["src_idx"][e], out["time_idx"][e]) == (k, t) and out["max_beam"][e] == vol.max(), e
                    assert np.array_equal(out["columns"][e], vol[:, t]), e
                    with np.errstate(invalid="ignore"):
                        assert np.array_equal(out["likelihood"][e], pp.likelihood(vol[:, t]), equal_nan=True), e
                else:
                    mb, ma = oracle.beamform(f[e], tau, wp, ws, "flexible", "max")
                    assert np.array_equal(out["maxbeam"][e], mb) and np.array_equal(out["maxbeam_sources"][e], ma), e
                    assert out["time_idx"][e] == mb.argmax() and out["src_idx"][e] == ma[mb.argmax()]
                    assert out["max_beam"][e] == mb.max()
            # tests/test_gpu_location_uncertainty.py: check_spatial / check_temporal, with their derived tolerances
            res = {k: out[k] for k in ("src_idx", "likelihood", "maxbeam", "maxbeam_sources") if k in out}
            if not spatial:
                assert no_sample_near_the_cutoff(out["maxbeam"], kT, cutoff)
            host = workflow.location_uncertainties_host(res, lon, lat, dep, method, restricted_domain_side_km=side,
                                                        effective_kT=kT, gibbs_cutoff=cutoff)
            assert np.array_equal(out["n_domain"], host["n_domain"])
            rows = out["src_idx"]
            assert np.array_equal(out["longitude"], lon[rows]) and np.array_equal(out["latitude"], lat[rows])
            assert np.array_equal(out["depth"], dep[rows])
            if spatial:
                assert np.array_equal(out["domain"].astype(bool), host["domain"])
                rel = 4 * K * 2.0 ** -53
                assert close(out["vunc"], host["vunc"], rel) and close(out["hunc"], host["hunc"], rel, 1e-9)
                assert np.isnan(out["hunc"][2]) and np.isfinite(out["hunc"][:2]).all()
            else:
                assert close(out["vunc"], host["vunc"], 1e-6) and close(out["hunc"], host["hunc"], 1e-6)
                assert out["n_domain"][2] == N and np.isfinite(out["hunc"]).all()

        inputs = {"f": f, "wp": wp, "tables": tables}
        outputs = {"time_idx": ((E,), np.int32), "src_idx": ((E,), np.int32), "max_beam": ((E,), np.float32)}
        if spatial:
            inputs.update(tau=tau, w_sources=ws)
            outputs.update(likelihood=((E, K), np.float32), columns=((E, K), np.float32), domain=((E, K), np.uint8))
        else:
            outputs.update(maxbeam=((E, N), np.float32), maxbeam_sources=((E, N), np.int32))
        for name in ("hunc", "vunc", "longitude", "latitude", "depth"):
            outputs[name] = ((E,), np.float64)
        outputs["n_domain"] = ((E,), np.int32)
        calls.append(Call(f"relocate:{method}", "bpmf_bp_relocate_batch_dev", inputs, outputs, invoke, verify,
                          [{"ws": need, "ws_unc": need_unc}], {"ws": need - 1}))
    calls[-1].after = destroy_plans(plans)
    return calls


# ============================================================ tier 2: entry points whose only risk is the output ===
def peak_amplitudes_calls(lib):
    import peak_amp_cases as pac
    from seismic_bpmf_amd import postprocess as pp
    case = pac.make_case(1, 1003, 4, 3, 5, 203, 20, 60, True)
    S, Cc, N = case["data"].shape
    D, T = len(case["rows"]), case["moveouts"].shape[0]
    with np.errstate(invalid="ignore"):
        want = pp.peak_amplitudes_host(case["data"], case["rows"], case["samples"], case["moveouts"], case["offset"],
                                       case["duration"], case["data_norm"])
    assert pac.same_bits(want, pac.literal_loop(case))

    def invoke(lib, p, nb, stream):
        return lib.bpmf_peak_amplitudes_dev(p["data"], S, Cc, N, D, p["rows"], p["samples"], p["moveouts"], T,
                                            case["offset"], case["duration"], p["norm"], stream, p["out"])

    def verify(out):
        assert pac.same_bits(out["out"], want)

    return [Call("peak_amplitudes:203_detections", "bpmf_peak_amplitudes_dev",
                 {"data": case["data"], "rows": case["rows"], "samples": case["samples"], "moveouts": case["moveouts"],
                  "norm": case["data_norm"]}, {"out": ((D, S, Cc), np.float32)}, invoke, verify)]


TEMPLATES_CASE = dict(seed=505, S=1, C=5, E=3, L=129, normalize="rms", noise=(140, 129), rotate=5)


def templates_calls(lib):
    import templates_cases as tpc
    from seismic_bpmf_amd import postprocess as pp
    case = tpc.make_case(**TEMPLATES_CASE)
    assert "cut_by_end" in case["placement"].ravel().tolist()
    S, Cc, N = case["data"].shape
    origin, mv, L, n_noise, offset = pp.template_arguments(S, Cc, case["origin"], case["moveouts"], case["L"],
                                                           case["normalize"], case["noise_offset"], case["noise_samples"])
    E = len(origin)
    want = tpc.host_answer(case)

    def invoke(lib, p, nb, stream):
        return lib.bpmf_templates_from_events_dev(p["data"], S, Cc, N, E, p["origin"], p["moveouts"], L, 1, offset,
                                                  n_noise, stream, p["templates"], p["norm"], p["flags"], p["snr"])

    def verify(out):
        assert not (out["flags"] & ~np.uint8(3)).any()
        got = {"templates": out["templates"], "norm": out["norm"], "snr": out["snr"],
               "available": (out["flags"] & 1) != 0, "complete": (out["flags"] & 2) != 0}
        tpc.check(got, want, "guard bands")

    return [Call("templates:L129_cut_by_end", "bpmf_templates_from_events_dev",
                 {"data": case["data"], "origin": np.ascontiguousarray(origin, np.int64),
                  "moveouts": np.ascontiguousarray(mv, np.int32)},
                 {"templates": ((E, S, Cc, L), np.float32), "norm": ((E, S, Cc), np.float32),
                  "flags": ((E, S, Cc), np.uint8), "snr": ((E, S, Cc), np.float32)}, invoke, verify)]


NORM_CASE = (300, 129, .5)


def normalize_batch_calls(lib):
    import picker_cases as pc
    from seismic_bpmf_amd import postprocess as pp
    n, W, overlap = NORM_CASE
    assert NORM_CASE in pc.NORM_CASES
    x = pc.norm_rows(n)
    R, Cc, _ = x.shape
    shift, n_windows = pp.normalize_batch_plan(n, normalization_window_sample=W, overlap=overlap)
    nodes = np.ascontiguousarray(pp.normalize_batch_nodes(n, shift, n_windows), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = pp.normalize_batch_host(x, W, overlap)
    assert want.dtype == np.float64
    calls = []
    for out_f64 in (0, 1):
        def invoke(lib, p, nb, stream, out_f64=out_f64):
            return lib.bpmf_normalize_batch_dev(p["x"], R, Cc, n, R, None, n, W, shift, p["nodes"], n_windows, out_f64,
                                                stream, p["out"])

        def verify(out, out_f64=out_f64):
            pc.check(out["out"], want if out_f64 else want.astype(np.float32), f"normalize_batch f64={out_f64}")

        calls.append(Call(f"normalize_batch:{'f64' if out_f64 else 'f32'}", "bpmf_normalize_batch_dev",
                          {"x": x, "nodes": nodes}, {"out": ((R, Cc, n), np.float64 if out_f64 else np.float32)},
                          invoke, verify))
    return calls


RESAMPLE_CASE = (5, 2, 257)              # up, down, n


def resample_calls(lib):
    import picker_cases as pc
    import resample_cases as rsc
    from seismic_bpmf_amd import postprocess as pp
    up, down, n = RESAMPLE_CASE
    assert RESAMPLE_CASE in list(rsc.cases())
    x = np.ascontiguousarray(rsc.rows(n))
    rows = len(x)
    _, n_out, _, n_pre_remove, _, table = pp.resample_poly_plan(n, up, down)
    table = np.ascontiguousarray(table, np.float32)
    hp = len(table) // up
    want = pp.resample_poly_host(x, up, down)

    def invoke(lib, p, nb, stream):
        return lib.bpmf_resample_poly_dev(p["x"], rows, 1, n, rows, None, n, up, down, p["table"], hp, n_pre_remove, n_out,
                                          stream, p["out"])

    def verify(out):
        pc.check(out["out"].reshape(want.shape), want, "resample_poly 5/2 n=257")

    return [Call("resample:5_2_n257", "bpmf_resample_poly_dev", {"x": x, "table": table},
                 {"out": ((rows, 1, n_out), np.float32)}, invoke, verify)]


PICKS_MAX = 8


def find_picks_calls(lib):
    import picker_cases as pc
    from seismic_bpmf_amd import postprocess as pp
    named = {label: (x, thr) for label, x, thr in pc.pick_cases()}
    series = [named["forty_picks"], named["separated_gaussians"]]
    x = np.stack([s[0] for s in series])
    thresholds = [s[1] for s in series]
    n_traces, n = x.shape
    want = [pp.find_picks_host(x[t], thresholds[t], return_index=True) for t in range(n_traces)]
    assert len(want[0][0]) == 40 and 0 < len(want[1][0]) < PICKS_MAX

    def invoke(lib, p, nb, stream):
        return lib.bpmf_find_picks_dev(p["proba"], n_traces, n, thresholds[0], thresholds[1], PICKS_MAX, stream,
                                       p["count"], p["value"], p["mean"], p["std"], p["index"])

    def verify(out):
        for t in range(n_traces):
            count = len(want[t][0])
            kept = min(count, PICKS_MAX)
            assert out["count"][t] == count                           # the TRUE number of picks
            got = tuple(out[k][t, :kept] for k in ("value", "mean", "std", "index"))
            pc.check_picks(got, tuple(np.asarray(w)[:kept] for w in want[t]), f"series {t}")
            assert np.isnan(out["value"][t, kept:]).all() and np.isnan(out["mean"][t, kept:]).all()
            assert np.isnan(out["std"][t, kept:]).all() and (out["index"][t, kept:] == -1).all()

    return [Call("find_picks:forty_picks_max_8", "bpmf_find_picks_dev", {"proba": x},
                 {"count": ((n_traces,), np.int32), "value": ((n_traces, PICKS_MAX), np.float32),
                  "mean": ((n_traces, PICKS_MAX), np.float64), "std": ((n_traces, PICKS_MAX), np.float64),
                  "index": ((n_traces, PICKS_MAX), np.int32)}, invoke, verify)]


WS_N, WS_WINDOW, WS_SHIFT = 1030, 257, 64


def window_stats_calls(lib):
    n, window, shift = WS_N, WS_WINDOW, WS_SHIFT
    rng = np.random.default_rng(8)
    x = np.round(np.abs(rng.standard_normal(n)) * (1 + 5 * (rng.random(n) > 0.99)), 2).astype(np.float32)
    x[::7] = -0.0
    nw = int(lib.bpmf_bp_num_windows(n, window, shift))
    assert nw == (n - window) // shift + 1 and nw * shift + window > n          # the last window is cut by the end
    init = np.full(4 * (nw + 2), 0xFF, np.uint8)
    init[:4] = init[-4:] = 0xA5                           # entries 0 and n_windows + 1 are the caller's
    init = init.view(np.float32)

    def invoke(lib, p, nb, stream):
        return lib.bpmf_bp_window_stats_dev(p["x"], n, window, shift, stream, p["median"], p["mad"])

    def verify(out):
        for q in range(1, nw + 1):
            seg = x[q * shift:min(n, q * shift + window)]
            m = np.median(seg)
            assert out["median"][q] == m and out["mad"][q] == np.median(np.abs(seg - m)), q
        for name in ("median", "mad"):
            ends = out[name].view(np.uint8).reshape(-1, 4)[[0, -1]]
            assert (ends == 0xA5).all(), (name, "an end entry was written")

    return [Call("window_stats:last_window_cut", "bpmf_bp_window_stats_dev", {"x": x},
                 {"median": ((nw + 2,), np.float32, init), "mad": ((nw + 2,), np.float32, init)}, invoke, verify)]


PEAKS_N, PEAKS_CAPACITY, PEAKS_FLOOR = 1003, 5, 1.0


def extract_peaks_calls(lib):
    from seismic_bpmf_amd import postprocess as pp
    from seismic_bpmf_amd.threshold import peak_dtype
    n = PEAKS_N
    rng = np.random.default_rng(12)
    x = np.round(np.abs(rng.standard_normal(n)), 1).astype(np.float32)          # ties and plateaus
    x[500] = np.nan
    x[-2] = 9.0                                           # a peak on the last sample that can be one
    src = rng.integers(0, 50_000, n).astype(np.int32)
    idx = pp.detect_peaks(x, 1)
    idx = idx[x[idx] > PEAKS_FLOOR]
    assert idx.size > 4 * PEAKS_CAPACITY and n - 2 in idx

    def invoke(lib, p, nb, stream):
        return lib.bpmf_bp_extract_peaks_dev(p["x"], p["src"], n, PEAKS_FLOOR, PEAKS_CAPACITY, stream, p["count"],
                                             p["records"])

    def verify(out):
        assert out["count"][0] == idx.size and out["count"][1] == -1            # the true number; its neighbour stays
        rec = out["records"].view(peak_dtype).reshape(-1)
        stored = rec[:PEAKS_CAPACITY]
        assert len(set(stored["index"].tolist())) == PEAKS_CAPACITY and np.isin(stored["index"], idx).all()
        assert np.array_equal(stored["beam"], x[stored["index"]]) and np.array_equal(stored["source"], src[stored["index"]])
        assert (out["records"][PEAKS_CAPACITY:] == -1).all(), "a record behind `capacity` was written"

    return [Call("extract_peaks:capacity_below_count", "bpmf_bp_extract_peaks_dev", {"x": x, "src": src},
                 {"count": ((2,), np.int32), "records": ((PEAKS_CAPACITY + 3, 4), np.int32)}, invoke, verify)]


SS_LANES = 64                            # lanes of a workgroup of csrc/source_spectra.hip: the median's column is (NC, 64) f64
SS_AVERAGE_OPTION, SS_MW_OPTION = 1, 1   # indices into source_spectra_cases.AVERAGE_OPTIONS (log, median) / MW_OPTIONS


def source_spectra_calls(lib):
    """All four stages in one call (flags 15), the median asked for: 15 channels x 65 bins (nothing a multiple of 64),
    and 129 channels x 3 bins (129 x 64 x 8 bytes of dynamic LDS: just over the 64 KB that need the opt-in).  Twelve
    outputs of four element widths, no workspace."""
    import source_spectra_cases as sc
    from seismic_bpmf_amd import postprocess as pp
    option, mw_option = sc.AVERAGE_OPTIONS[SS_AVERAGE_OPTION], sc.MW_OPTIONS[SS_MW_OPTION]
    calls = []
    for name in sc.GUARD_CASES:
        _, E, S, Cc, F, _ = sc.CASES[name]
        x, arguments = sc.inputs(name), sc.phase_arguments(name, "p")
        arrays, params = sc.c_inputs(name, "p")
        params.update(average_log=int(option[0]), median=int(option[1] == "median"), min_num_valid=option[2],
                      max_err_pct=option[3], bands=mw_option[0],
                      first_high=int(np.searchsorted(x["frequencies"], mw_option[1], side="right")))
        with np.errstate(all="ignore"):
            want = pp.source_spectra_host(**arguments, **sc.average_kwargs(option))
            want_mw = pp.approximate_moment_magnitude_host(want["corrected"], want["snr"], x["present"],
                                                           x["frequencies"], x["epi"], **sc.mw_kwargs(mw_option))
            geometry = arguments["geometry_constant"] * (1000.0 * x["dist"]) / arguments["radiation"]
            att = np.exp(np.pi * arguments["tt_sec"][..., None] * x["frequencies"] / arguments["q_row"])

        def invoke(lib, p, nb, stream, E=E, S=S, Cc=Cc, F=F, params=params):
            return sc.c_call(lib, p, E, S, Cc, F, 15, stream, **params)

        def verify(out, want=want, want_mw=want_mw, arguments=arguments, geometry=geometry, att=att, Cc=Cc, F=F):
            got = {k: out[k] for k in ("average", "std", "num_valid")}
            got.update(mask=out["mask"] != 0, used=out["used"] != 0, snr=out["snr"].reshape(want["snr"].shape),
                       corrected=out["corrected"].reshape(want["corrected"].shape))
            assert not (out["mask"] > 1).any() and not (out["used"] > 1).any()
            assert np.array_equal(got["snr"], want["snr"], equal_nan=True)
            assert sc.corrected_ok(got["corrected"], arguments["signal"], geometry[:, :, None, None],
                                   att[:, :, None, :], arguments["present"]) == 0.0
            discrete, r_avg, r_std = sc.check_average(got, want, option, Cc)
            assert discrete and r_avg <= 1.0 and r_std <= 1.0, (discrete, r_avg, r_std)
            got_mw = {k: out[k] for k in ("Mw_star", "log10_M0", "measured_disp", "weights", "measurement_snr")}
            discrete, r_disp, r_m0, r_mw = sc.check_mw(got_mw, want_mw, F)
            assert discrete and r_disp <= 1.0 and r_m0 <= 1.0 and r_mw <= 1.0, (discrete, r_disp, r_m0, r_mw)

        calls.append(Call(f"source_spectra:{name}", "bpmf_source_spectra_dev", arrays, sc.output_specs(E, S, Cc, F),
                          invoke, verify))
    return calls


TIER2 = [peak_amplitudes_calls, templates_calls, normalize_batch_calls, resample_calls, find_picks_calls,
         window_stats_calls, extract_peaks_calls, source_spectra_calls]

TIER1 = [tdt_rms_calls, multiband_calls, svdwf_calls, bandpass_calls, multiples_calls, intertemplate_calls,
         median_mad_calls, tdt_mad_calls, kurtosis_calls, mf_calls, bp_run_calls, relocate_calls]


def builders():
    """[(label, function(lib) -> [Call, ...])]: one per entry point; the test parametrises over these."""
    return [(f.__name__[:-len("_calls")], f) for f in TIER1 + TIER2]
