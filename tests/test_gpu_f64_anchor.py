"""GPU: the matched-filter and backprojection KERNELS against the float64 definition -- the oracle is not in
the loop.

Every other GPU test asserts bit-equality with oracle/bpmf_oracle.c, which the same understanding wrote; here each
kernel family (selected as tests/test_gpu_variants.py selects them) is judged by tests/f64_anchor.py: |kernel - f64|
within the a priori bound computed from the inputs, exact zeros wherever the definition computes nothing, the
arg-max rules on every sample, and -- on small-integer inputs, where float32 is exact -- bit-equality of beam,
max-beam and arg-max with float64 (the lowest-index tie rule and the (0, 0) floor, pinned independently).  Each
compat switch is judged by its own definition, and the two day-scale plans (cfg2's day of matched filter, cfg3's
50 000 sources over its day) at sampled lags / times that hold the first and last valid index, the strict tail,
the neighbours of multiples of 128, 256, 512, 2048 and 8192 spread over the day, and seeded random indices.
Every check prints its worst err / B (pytest -rP shows them).
"""
import numpy as np
import pytest

import f64_anchor as fa
from mf_launch import assert_takes

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ matched filter ---
def _mf_host(args, step, ns):
    from seismic_bpmf_amd import matched_filter
    return matched_filter(*args, step, arch="gpu", check_zeros=False, network_sum=ns)


def _mf_resident(args, step, ns):
    from seismic_bpmf_amd import MatchedFilterGPU
    eng = MatchedFilterGPU(device=0)
    eng.set_data(args[3])
    first = eng.run(args[0], args[1], args[2], step, network_sum=ns).cpu().numpy()
    again = eng.run(args[0], args[1], args[2], step, network_sum=ns).cpu().numpy()    # on the prepared day
    assert np.array_equal(first, again)
    return again


def _mf_family(label, L, step, N, run=_mf_host, regimes=("noise", "scaled", "int"), T=2, kw=None, takes=None):
    """`takes`: fields of bpmf_mf_launch_info the launches must show (a function of network_sum where it decides): the
    family the caller's options are meant to select is the one that runs."""
    for regime in regimes:
        args = fa.mf_case(regime, L, N, step, seed=1000 + L + step, T=T)
        for ns in (True, False):
            assert_takes(args[0].shape, N, step, ns, **{k: v(ns) if callable(v) else v for k, v in (takes or {}).items()})
        ref = fa.mf_f64(*args, step=step, exact=regime == "int", **(kw or {}))
        assert ref.valid.any() and not ref.valid.all()
        assert fa.mf_dead_channels(args[0], ref) >= 1              # a dead template, weighted, inside the lag range
        assert ref.zero_windows >= 1                               # windows inside the data gap
        for ns in (True, False):
            fa.mf_compare(run(args, step, ns), ref, ns, f"kernel MF {label} L={L} step={step} {regime} network_sum={ns}").require()


@pytest.mark.parametrize("wave_kernel", [1, 0])
def test_mf_wave_and_workgroup_kernels(hip_opts, wave_kernel):
    hip_opts("mf.wave_kernel", wave_kernel)
    takes = dict(family="wave") if wave_kernel else dict(family="workgroup", maxr=20, maxt=5)
    for L, step in ((200, 1), (257, 3), (1, 1)):
        _mf_family(f"wave_kernel={wave_kernel}", L, step, 9300, takes=takes)


@pytest.mark.parametrize("ntile", [1, 2, 4])
def test_mf_tiles_per_wave(hip_opts, ntile):
    hip_opts("mf.tiles_per_wave", ntile)
    _mf_family(f"tiles_per_wave={ntile}", 128, 1, 9100, takes=dict(family="wave", ntile=ntile))
    _mf_family(f"tiles_per_wave={ntile}", 40, 7, 5000, takes=dict(family="wave", ntile=ntile))


@pytest.mark.parametrize("fused", [1, 0])
def test_mf_fused_prologue(hip_opts, fused):
    hip_opts("mf.tiles_per_wave", 1)
    hip_opts("mf.fused_prologue", fused)
    takes = dict(family="wave", ntile=1, fused=bool(fused), prologue=not fused)
    _mf_family(f"fused_prologue={fused}", 100, 1, 2600, takes=takes)
    _mf_family(f"fused_prologue={fused}", 33, 3, 2500, takes=takes)


def test_mf_channel_split(hip_opts):
    hip_opts("mf.channel_split", 1 << 20)
    hip_opts("mf.tiles_per_wave", 1)
    takes = dict(family="wave", ntile=1, fused=True, csplit=lambda ns: ns)       # (the channel split is the network sum's)
    for L in (64, 256):
        _mf_family("channel_split", L, 1, 5200, takes=takes)
        _mf_family("channel_split resident", L, 1, 5200, run=_mf_resident, regimes=("noise", "int"), takes=takes)


@pytest.mark.parametrize("L", [300, 1100, 2065])
def test_mf_long_template_kernels(L):
    # (the workgroup kernel's two register variants; 2065 is beyond its 2049 samples: the generic kernel)
    takes = {300: dict(family="workgroup", maxr=20, maxt=5), 1100: dict(family="workgroup", maxr=24, maxt=9),
             2065: dict(family="direct")}[L]
    _mf_family("257 < L <= 2065", L, 1 if L != 1100 else 3, L + 7000, takes=takes)


def test_mf_generic_kernel_long_templates_and_large_steps(hip_opts):
    _mf_family("generic L > 2065", 2100, 1, 2100 + 5000, takes=dict(family="direct"))
    _mf_family("generic step > max_mfma_step", 64, 70, 64 + 70 * 1500, takes=dict(family="direct"))
    hip_opts("mf.max_mfma_step", 0)
    _mf_family("generic max_mfma_step=0", 200, 3, 6000, takes=dict(family="direct"))


def test_mf_host_call_small_batches_and_pieces(hip_opts):
    hip_opts("mf.host_batch_kb", 64)
    hip_opts("mf.host_piece_kb", 16)
    _mf_family("host batches 64 KB pieces 16 KB", 40, 1, 9000, T=5)
    hip_opts("mf.host_batch_kb", 1)
    hip_opts("mf.host_piece_kb", 1)
    _mf_family("host batches 1 KB pieces 1 KB", 128, 3, 7000, T=5, regimes=("scaled", "int"))


def test_mf_resident_engine():
    for L, step in ((256, 1), (1100, 1), (2100, 7)):
        _mf_family("resident", L, step, L + 6000, run=_mf_resident)


MF_SWITCHES = {"mf.compat_exclusive_last_lag": dict(exclusive_last_lag=True), "mf.compat_sqrt_norm": dict(),
               "mf.compat_range_all_channels": dict(range_all_channels=True),
               "mf.compat_sequential_csum": dict(sequential_csum=True)}


@pytest.mark.parametrize("switch", list(MF_SWITCHES))
def test_mf_switch_against_its_definition(hip_opts, switch):
    """Each mf.compat_* switch on the default kernels, judged by the float64 definition written from the option's
    description (the two range switches change which lags are exact zeros; the two others change rounding only)."""
    hip_opts(switch, 1)
    for step in (1, 3):
        _mf_family(switch, 200, step, 9000, regimes=("noise", "scaled", "dc", "sine", "int"), kw=MF_SWITCHES[switch])
    _mf_family(switch + " resident", 300, 1, 7000, run=_mf_resident, regimes=("scaled",), kw=MF_SWITCHES[switch])


def test_mf_default_kernels_in_every_value_regime():
    for L, step in ((256, 1), (40, 3)):
        _mf_family("default", L, step, 9000, regimes=fa.MF_REGIMES + ("int",))


# ------------------------------------------------------------------------------ backprojection ---
def _bp_run(args, oob, reduce, expect=None):
    from seismic_bpmf_amd import BeamformerGPU
    f, tau, wp, ws = args
    bf = BeamformerGPU(tau, ws)
    try:
        if expect is not None:
            expect(bf.plan_info())
        out = bf.run(f, wp, reduce, oob)
        return out.cpu().numpy() if reduce == "none" else tuple(x.cpu().numpy() for x in out)
    finally:
        bf.close()


def _bp_judge(label, args, oob, regime, m, a, first_computed=False, kw=None, beam=None):
    ref = fa.bp_f64(*args, out_of_bounds=oob, exact=regime == "int", **(kw or {}))
    what = f"kernel BP {label} {regime} {oob}"
    fa.bp_compare_max(m, a, ref, first_computed, what + " reduce=max").require()
    if beam is not None:
        fa.bp_compare_beam(beam, ref, what + " reduce=none").require()
    if regime == "int":
        # bit-equality pins the tie rule and the floor only where the inputs hold both
        n_tied, n_floor = fa.bp_tie_and_floor_counts(ref)
        print(f"f64-anchor {what}: {n_tied} tied maxima, {n_floor} floor samples")
        assert n_tied >= fa.MIN_TIED and n_floor >= fa.MIN_FLOOR, (what, n_tied, n_floor)
        wm, wa = fa.bp_max_f64(ref, first_computed)
        assert np.array_equal(m, wm), f"{what}: {(m != wm).sum()} max-beams differ from float64"
        assert np.array_equal(a, wa), f"{what}: {(a != wa).sum()} arg-max differ from float64"
        assert beam is None or np.array_equal(beam, ref.beam), what
    return ref


def _bp_family(label, expect=None, with_beam=False, first_computed=False, kw=None, oobs=("strict", "flexible"), **case):
    for regime in ("signed", "int"):
        args = fa.bp_case(regime, seed=len(label) + case["K"], **case)
        for oob in oobs:
            m, a = _bp_run(args, oob, "max", expect)
            beam = _bp_run(args, oob, "none") if with_beam else None
            _bp_judge(label, args, oob, regime, m, a, first_computed, kw, beam)


FAST = dict(K=480, S=18, P=2, N=6000, tau_lo=-40, tau_hi=160)


@pytest.mark.parametrize("tile", [512, 256, 128])
@pytest.mark.parametrize("uniform", [True, False])
def test_bp_fast_classes(hip_opts, tile, uniform):
    hip_opts("bp.fast_tile", tile)

    def expect(info):
        assert info["n_classes"] == 1 and info["class_tile"][0] == tile, info

    _bp_family(f"fast tile {tile} {'uniform' if uniform else 'per-station'} weights", expect, n_used=10,
               uniform=uniform, **FAST)


def test_bp_multi_residency_class(hip_opts):
    hip_opts("bp.halves", 1)
    hip_opts("bp.fast_tile", 256)

    def expect(info):
        assert info["n_classes"] == 1 and info["class_tile"][0] == 256 and info["gather_bytes"] == 8, info

    _bp_family("multi-residency 40 of 44 stations", expect, K=300, S=44, P=2, N=5000, tau_lo=-50, tau_hi=150,
               n_used=40, uniform=True)


def test_bp_general_kernels_alone(hip_opts):
    hip_opts("bp.fast", 0)

    def expect(info):
        assert info["n_classes"] == 0 and info["n_groups"] >= 1, info

    _bp_family("bp.fast=0", expect, n_used=10, **FAST)
    _bp_family("bp.fast=0 wide moveouts", expect, K=120, S=9, P=3, N=8000, tau_lo=-700, tau_hi=1200)


def test_bp_direct_kernel(hip_opts):
    hip_opts("bp.direct", 1)

    def expect(info):            # what bpmf_bp_plan_info reports of a plan without LDS windows
        assert info["n_groups"] == 0 and info["n_classes"] == 0 and info["tile"] == 1024, info

    _bp_family("bp.direct=1", expect, n_used=10, **FAST)


def test_bp_grid_without_an_lds_plan():
    def expect(info):
        assert info["n_groups"] == 0, info

    _bp_family("no LDS plan, 150 stations x 2 phases", expect, K=32, S=150, P=2, N=5000, tau_lo=-100, tau_hi=200)


def test_bp_full_beams_and_default_plan():
    _bp_family("default", None, with_beam=True, K=200, S=8, P=2, N=3000, tau_lo=-120, tau_hi=260, n_used=5)
    _bp_family("default two stations", None, with_beam=True, K=60, S=2, P=1, N=2500, tau_lo=-300, tau_hi=500)


def test_bp_batch_path_of_relocate_events():
    """workflow.relocate_events("temporal"): the (max-beam, arg-max) rows of a batch of events computed in shared
    launches (csrc/bp_relocate.hip), each event judged like a call of its own."""
    from seismic_bpmf_amd import BeamformerGPU
    from seismic_bpmf_amd.workflow import relocate_events
    E, K, S, P, N = 4, 300, 12, 2, 2500
    for regime in ("signed", "int"):
        events = [fa.bp_case(regime, K, S, P, N, seed=40 + e, tau_lo=-60, tau_hi=240, n_used=7) for e in range(E)]
        _, tau, wp, ws = events[0]
        f = np.stack([ev[0] for ev in events])
        bf = BeamformerGPU(tau, ws)
        try:
            for oob in ("flexible", "strict"):
                res = relocate_events(bf, f, wp, "temporal", oob)
                mb, ma = res["maxbeam"].cpu().numpy(), res["maxbeam_sources"].cpu().numpy()
                for e in range(E):
                    _bp_judge(f"relocate_events event {e}", (f[e], tau, wp, ws), oob, regime, mb[e], ma[e])
                    assert res["time_idx"][e] == int(mb[e].argmax()) and res["src_idx"][e] == ma[e, res["time_idx"][e]]
        finally:
            bf.close()


BP_SWITCHES = {"bp.compat_first_computed": (dict(), True), "bp.compat_strict_upper_only": (dict(strict_upper_only=True), False),
               "bp.compat_range_all_stations": (dict(range_all_stations=True), False)}


@pytest.mark.parametrize("switch", list(BP_SWITCHES))
def test_bp_switch_against_its_definition(hip_opts, switch):
    """Each bp.compat_* switch on the default plan, judged by the float64 definition written from the option's
    description.  A source without a weighted station computes nothing under every switch."""
    hip_opts(switch, 1)
    kw, fc = BP_SWITCHES[switch]
    _bp_family(switch, None, with_beam=True, first_computed=fc, kw=kw, n_used=10, K=200, S=18, P=2, N=4000,
               tau_lo=-70, tau_hi=120)


def test_upstream_recollected_profile_against_the_definitions():
    """compat_profile("upstream-recollected") -- what a user turns on to match upstream -- through the drop-in calls:
    the four MF switches and bp.compat_first_computed together, judged by the definitions (its other checks compare
    with the oracle under the same flags, or need upstream's packages)."""
    import seismic_bpmf_amd as sb
    try:
        assert sb.compat_profile("upstream-recollected") == "upstream-recollected"
        kw = dict(exclusive_last_lag=True, range_all_channels=True, sequential_csum=True)
        for step in (1, 3):
            _mf_family("profile upstream-recollected", 96, step, 9000, kw=kw)
        for regime in ("signed", "int"):
            args = fa.bp_case(regime, 150, 9, 2, 4000, seed=17, tau_lo=-70, tau_hi=120, n_used=6)
            for oob in ("strict", "flexible"):
                m, a = sb.beamform(*args, device="gpu", out_of_bounds=oob)
                _bp_judge("profile upstream-recollected", args, oob, regime, m, a, first_computed=True)
    finally:
        sb.compat_profile("build")
    _mf_family("profile build", 96, 1, 9000, regimes=("noise",))


# ------------------------------------------------------------------------------ day scale, sampled ---
def test_mf_cfg2_day_at_sampled_lags():
    """cfg2's day (20 x 3 channels, L = 256, 8.64 M samples), 4 templates with moveouts of both signs, the resident
    engine: a few thousand lags against the sampled float64 form."""
    import torch
    from seismic_bpmf_amd import MatchedFilterGPU
    S, C, L, N, T = 20, 3, 256, 8_640_000, 4
    g = torch.Generator(device="cuda")
    g.manual_seed(41)
    data = torch.randn((S, C, N), device="cuda", generator=g)
    rng = np.random.default_rng(43)
    tmpl = rng.standard_normal((T, S, C, L)).astype(np.float32)
    mv = rng.integers(-1500, 3001, (T, S, C)).astype(np.int32)
    mv[0, 3, 1], mv[1, 0, 0], mv[2, 5, 2] = -1499, -1022, -3
    w = rng.uniform(0.05, 1.0, (T, S, C)).astype(np.float32)
    w[3, :, 1] = 0.0
    mv[3, 2, 1], mv[3, 4, 1] = -9000, 12_000                     # zero-weight channels beyond every weighted moveout
    mf = MatchedFilterGPU()
    mf.set_data(data)
    cc = mf.run(tmpl, mv, w, 1)
    n_corr = N - L + 1
    assert tuple(cc.shape) == (T, n_corr)
    ranges = [fa.mf_lag_range(mv[t], w[t], N, L, 1) for t in range(T)]
    lags = fa.edge_sample(n_corr, [r[0] for r in ranges], [r[1] for r in ranges], n_random=2500, seed=5)
    assert all(r[0] in lags and r[1] in lags and r[0] > 0 and r[1] + 1 in lags for r in ranges)
    got = cc[:, torch.as_tensor(lags, device=cc.device)].cpu().numpy()
    ref = fa.mf_f64(tmpl, mv, w, data.cpu().numpy(), 1, lags=lags)
    assert ref.valid.any(axis=0).sum() > 2500 and (~ref.valid).sum() > 100
    fa.mf_compare(got, ref, True, f"kernel MF cfg2 day, {lags.size} sampled lags").require()


def test_bp_cfg3_full_grid_day_at_sampled_times():
    """cfg3 in full -- 50 000 sources, 20 stations x 3 components, 4.32 M samples -- at a few hundred sample times,
    all sources each: the first check of the full plan's max-beam and arg-max against anything independent."""
    import torch
    from seismic_bpmf_amd import BeamformerGPU, synthetic as syn
    cfg = syn.BP_CONFIGS["cfg3"]
    geo = syn.make_bp_geometry(cfg["grid"], cfg["S"], cfg["P"], cfg["sr"])
    tau, ws = geo["moveouts"], geo["weights_sources"]
    K, N = tau.shape[0], cfg["N"]
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    feat = torch.randn((cfg["S"], cfg["C"], N), device="cuda", generator=g).abs_()
    wp = syn.phase_weights(cfg["S"], cfg["C"], cfg["P"])
    tmax_used = np.where(ws[:, :, None] != 0, tau, -1).max(axis=(1, 2))
    last = N - 1 - int(tmax_used.min())                           # the last sample any source computes under strict
    times = fa.edge_sample(N, [0], [last], n_random=120, seed=9, per_multiple=6)
    assert 0 in times and last in times and last + 1 in times and N - 1 in times and 200 < times.size < 400
    bf = BeamformerGPU(tau, ws)
    try:
        beam, arg = bf.run(feat, wp, "max", "strict")
        idx = torch.as_tensor(times, device=beam.device)
        m, a = beam[idx].cpu().numpy(), arg[idx].cpu().numpy()
    finally:
        bf.close()
    ref = fa.bp_f64(feat.cpu().numpy(), tau, wp, ws, "strict", times=times)
    assert ref.computed[:, times <= last].any(axis=0).all() and not ref.computed[:, times > last].any()
    fa.bp_compare_max(m, a, ref, False, f"kernel BP cfg3 full grid, {times.size} sampled times").require()
    wm, wa = fa.bp_max_f64(ref)
    print(f"cfg3: arg-max equal to float64's at {(a == wa).sum()} of {times.size} sampled times")
    assert not m[times > last].any() and not a[times > last].any()
