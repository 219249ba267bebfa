"""CPU: the fenced arena of the guard-band tests (tests/arena.py) backed by a NumPy byte array through the same code
-- layout, fills, and for every kind of planted write the exact guard and offsets that check() names -- and the
premises of the case table (tests/guard_cases.py) that can be computed without a device: the library loads without a
GPU (tests/test_abi.py) and its bpmf_*_workspace_bytes functions are pure host code."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import guard_cases as gc

ROW_BYTES = 130 * 8                   # one float64 row of 130 samples: 64 of them are a slab


def small_arena():
    """An input, an output and -- last, so that a slab behind it lands in the slack -- a workspace."""
    a = ar.Arena("numpy")
    x = a.add_input("x", np.arange(75, dtype=np.float32))            # 300 bytes: the body ends off every alignment
    out = a.add_output("out", (7, 3), np.float64)
    ws = a.add_workspace("ws", 1000, 0x00)
    return a.commit(), x, out, ws


def poke(region, offset, values):
    """Write bytes at `offset` from the region's first byte THROUGH ITS ADDRESS, as a kernel would."""
    raw = np.ascontiguousarray(values, dtype=np.uint8)
    C.memmove(region.ptr + offset, raw.ctypes.data, raw.size)


# ---------------------------------------------------------------------------------------------- the arena ---
def test_layout_and_fills():
    a, x, out, ws = small_arena()
    image = a.read()
    for r in (x, out, ws):
        assert r.start % ar.ALIGN == 0 and r.ptr == a.base_ptr + r.start
        assert r.start - r.front >= ar.GUARD and r.behind_end - r.end >= ar.GUARD
    assert x.front == 0 and out.front == x.behind_end and ws.front == out.behind_end       # nothing between the regions
    assert ws.behind_end - ws.end >= ar.GUARD + ar.SLACK and ws.behind_end == image.size
    # guards of an input: NaN as float32 and float64, -1 as int32 and int64
    behind = image[x.end:x.behind_end]
    assert (behind == 0xFF).all() and (image[x.front:x.start] == 0xFF).all()
    whole = behind[(-x.end) % 8:][:64]
    assert np.isnan(whole.view(np.float32)).all() and np.isnan(whole.view(np.float64)).all()
    assert (whole.view(np.int32) == -1).all() and (whole.view(np.int64) == -1).all()
    # guards of workspace and outputs; the bodies
    for r in (out, ws):
        assert (image[r.front:r.start] == 0xA5).all() and (image[r.end:r.behind_end] == 0xA5).all()
    assert (out.raw() == 0xFF).all() and np.isnan(out.value()).all() and out.value().shape == (7, 3)
    assert (ws.raw() == 0x00).all() and ws.nbytes == 1000
    assert np.array_equal(x.value(), np.arange(75, dtype=np.float32))


def test_untouched_guards_give_an_empty_list():
    a, x, out, ws = small_arena()
    assert a.check() == [] and a.changed_bodies() == []
    # writes INSIDE the bodies, up to their last byte, are no finding
    poke(out, 0, [1] * out.nbytes)
    poke(ws, ws.nbytes - 1, [7])
    assert a.check() == [] and a.changed_bodies() == ["out", "ws"]
    a.reset()
    assert a.check() == [] and a.changed_bodies() == []


def test_one_byte_behind_an_output():
    a, x, out, ws = small_arena()
    poke(out, out.nbytes, [0])
    assert a.check() == [{"region": "out", "side": "behind", "first": 0, "last": 0, "bytes": 1}]


def test_one_element_in_front_of_a_workspace():
    a, x, out, ws = small_arena()
    poke(ws, -4, np.frombuffer(np.float32(1.5).tobytes(), np.uint8))
    assert a.check() == [{"region": "ws", "side": "front", "first": -4, "last": -1, "bytes": 4}]


def test_a_slab_of_64_rows_behind_a_workspace():
    a, x, out, ws = small_arena()
    slab = 64 * ROW_BYTES
    assert slab > ar.GUARD                                 # longer than a guard: this is what the slack is for
    poke(ws, ws.nbytes, np.zeros(slab, np.uint8))
    assert a.check() == [{"region": "ws", "side": "behind", "first": 0, "last": slab - 1, "bytes": slab}]
    # a slab that starts one row into the guard (the carve-up one row short), of which every other byte changes
    a.reset()
    rows = np.tile(np.array([0xA5, 0x11], np.uint8), slab // 2)
    poke(ws, ws.nbytes + ROW_BYTES, rows)
    assert a.check() == [{"region": "ws", "side": "behind", "first": ROW_BYTES + 1, "last": ROW_BYTES + slab - 1,
                          "bytes": slab // 2}]


def test_a_write_into_the_guard_of_an_input():
    a, x, out, ws = small_arena()
    poke(x, x.nbytes + 8, [0])
    assert a.check() == [{"region": "x", "side": "behind", "first": 8, "last": 8, "bytes": 1}]
    a.reset()
    poke(x, -1, [0])
    assert a.check() == [{"region": "x", "side": "front", "first": -1, "last": -1, "bytes": 1}]


def test_every_changed_guard_is_named_and_reset_puts_the_image_back():
    a, x, out, ws = small_arena()
    poke(out, -2, [0, 0])
    poke(out, out.nbytes + 5, [1])
    poke(ws, ws.nbytes + ar.GUARD + ar.SLACK - 1 + (-ws.end) % ar.ALIGN, [3])          # the last byte of the slack
    found = a.check()
    assert [(f["region"], f["side"], f["first"], f["last"]) for f in found] == [
        ("out", "front", -2, -1), ("out", "behind", 5, 5),
        ("ws", "behind", ws.behind_end - ws.end - 1, ws.behind_end - ws.end - 1)]
    a.reset(workspace_fill=0xFF)
    assert a.check() == [] and (ws.raw() == 0xFF).all() and a.changed_bodies() == []
    assert np.array_equal(a.read(), a.image)


def test_an_output_with_a_body_of_its_own():
    a = ar.Arena("numpy")
    init = np.full(5, np.nan, np.float32)
    init[[0, -1]] = 2.5
    out = a.add_output("out", (5,), np.float32, init=init)
    other = a.add_output("other", (3,), np.int32, fill=0x3C)
    a.commit()
    assert np.array_equal(out.value(), init, equal_nan=True) and (other.raw() == 0x3C).all()


# ---------------------------------------------------------------------------------- premises of the table ---
@pytest.fixture(scope="module")
def lib():
    from seismic_bpmf_amd import _lib
    return _lib.lib()


def test_66_rows_make_two_slabs_on_64_rows_worth_of_workspace(lib):
    n, active = gc.MB_N_SAMPLES, 6
    rows = gc.MB_E * gc.MB_S * gc.MB_C
    row_bytes = (4 + (1 + active) * n) * 8                 # include/bpmf_hip.h: what a row takes
    least, one_slab = lib.bpmf_multiband_workspace_bytes(64, n, active), lib.bpmf_multiband_workspace_bytes(rows, n, active)
    assert rows == 66 and least == 64 * row_bytes and one_slab == 128 * row_bytes
    slab = least // row_bytes // 64 * 64
    assert slab == 64 and -(-rows // slab) == 2 and (least - 1) // row_bytes // 64 * 64 == 0
    assert 63 // gc.MB_C == 64 // gc.MB_C == 65 // gc.MB_C == 21          # the slab boundary lies inside window 21
    # n = 130 is three time tiles, the last one partial
    assert -(-n // gc.MB_TIME_TILE) == 3 and n % gc.MB_TIME_TILE != 0
    day, starts, plan, want, valid, scale = gc.multiband_inputs()
    assert (starts == -1).sum() == 1 and (starts == day.shape[2] - n).sum() == 1 and plan["buffer"] == gc.MB_BUFFER
    assert int((~plan["skip"]).sum()) == active and int(plan["skip"].sum()) == 2


def test_one_svdwf_slot_makes_six_slabs(lib):
    off = np.array(gc.SV_OFFSETS)
    G, n_max, m = len(off) - 1, int(np.diff(off).max()), gc.SV_M
    channels = G * gc.SV_S * gc.SV_C
    head = lib.bpmf_svdwf_workspace_bytes(G, n_max, m, 0)
    one, every = lib.bpmf_svdwf_workspace_bytes(G, n_max, m, 1), lib.bpmf_svdwf_workspace_bytes(G, n_max, m, channels)
    slot = one - head
    assert channels == 6 and slot > 0 and every == head + channels * slot
    assert (one - head) // slot == 1 and -(-channels // 1) == 6 and (one - 1 - head) // slot == 0
    assert 0 in np.diff(off) and (np.diff(off) < m).all()              # an empty group; n < m everywhere


def test_the_svdwf_case_meets_the_conditions_of_its_bounds():
    import svdwf_cases as sc
    x, off, sos, want = gc.svdwf_inputs()
    for g in range(len(off) - 1):
        for s in range(gc.SV_S):
            for c in range(gc.SV_C):
                if off[g + 1] > off[g]:
                    assert sc.conditions(x[off[g]:off[g + 1], s, c], 0.4, 5) == want[2][g, s, c]


def test_each_tier_2_case_ends_in_a_partial_row_window_or_tile(lib):
    import picker_cases as pc
    import resample_cases as rsc
    import templates_cases as tpc
    from seismic_bpmf_amd import postprocess as pp
    for build in gc.TIER2:                                 # (the builders assert their own premises as well)
        assert build(lib)
    # resampling: the last tile of outputs is partial
    up, down, n = gc.RESAMPLE_CASE
    _, n_out, _, _, _, table = pp.resample_poly_plan(n, up, down)
    tile = lib.bpmf_resample_poly_tile(up, down, len(table) // up)
    assert tile > 0 and n_out % tile != 0 and (up, down, n) in list(rsc.cases())
    # normalisation: a trailing partial window is dropped, and 129 = one leaf of 128 and one sample
    n, W, overlap = gc.NORM_CASE
    shift, n_windows = pp.normalize_batch_plan(n, normalization_window_sample=W, overlap=overlap)
    assert (n + 2 * shift - W) % shift != 0 and W % 128 == 1 and "trailing_window_dropped" in pc.norm_classes_met(pc.norm_rows(n), W, overlap)
    # picks: more picks than slots
    forty = next(x for label, x, thr in pc.pick_cases() if label == "forty_picks")
    assert len(pp.find_picks_host(forty, 0.3)[0]) == 40 > gc.PICKS_MAX
    # templates: 129 samples, a window cut by the end of the day
    case = tpc.make_case(**gc.TEMPLATES_CASE)
    assert case["L"] % 128 == 1 and "cut_by_end" in case["placement"].ravel().tolist()
    # window statistics: the last window is cut by the end of the series; peaks: a partial last block of 256 samples
    nw = lib.bpmf_bp_num_windows(gc.WS_N, gc.WS_WINDOW, gc.WS_SHIFT)
    assert nw * gc.WS_SHIFT + gc.WS_WINDOW > gc.WS_N > nw * gc.WS_SHIFT
    assert gc.PEAKS_N % 256 != 0


def test_the_source_spectra_calls_miss_every_multiple_of_64_and_cross_the_lds_opt_in(lib):
    import source_spectra_cases as sc
    from seismic_bpmf_amd import postprocess as pp
    small, long_column = (sc.CASES[n][1:5] for n in sc.GUARD_CASES)
    assert small == (3, 5, 3, 65) and (small[1] * small[2]) % gc.SS_LANES == 15 and small[3] % gc.SS_LANES == 1
    E, S, Cc, F = long_column
    assert S * Cc == 129 and F == 3 and S * Cc <= pp.SOURCE_SPECTRA_MAX_CHANNELS
    assert S * Cc * gc.SS_LANES * 8 == 66048 > 64 * 1024 >= (S * Cc - 1) * gc.SS_LANES * 8       # the median's column
    assert sc.AVERAGE_OPTIONS[gc.SS_AVERAGE_OPTION][:2] == (True, "median")
    calls = gc.source_spectra_calls(lib)
    assert len(calls) == 2
    for call, name in zip(calls, sc.GUARD_CASES):
        assert sorted(call.outputs) == sorted(sc.POINTER_OUTPUTS) and call.variants == [{}] and call.refusal is None
        assert {np.dtype(spec[1]).itemsize for spec in call.outputs.values()} == {1, 4, 8}
        assert sorted(np.dtype(spec[1]).name for spec in call.outputs.values()).count("float32") == 2
        # the definition's own answer passes the call's verify
        want = pp.source_spectra_host(**sc.phase_arguments(name, "p"),
                                      **sc.average_kwargs(sc.AVERAGE_OPTIONS[gc.SS_AVERAGE_OPTION]))
        x = sc.inputs(name)
        with np.errstate(all="ignore"):
            mw = pp.approximate_moment_magnitude_host(want["corrected"], want["snr"], x["present"], x["frequencies"],
                                                      x["epi"], **sc.mw_kwargs(sc.MW_OPTIONS[gc.SS_MW_OPTION]))
        out = {**{k: want[k] for k in ("average", "std", "num_valid")}, **mw,
               "mask": want["mask"].astype(np.uint8), "used": want["used"].astype(np.uint8),
               "snr": want["snr"].reshape(call.outputs["snr"][0]),
               "corrected": want["corrected"].reshape(call.outputs["corrected"][0])}
        call.verify(out)
        assert (~want["mask"]).any() and np.isfinite(mw["Mw_star"]).any()
        out["num_valid"] = out["num_valid"] + 1
        with pytest.raises(AssertionError):
            call.verify(out)


def test_tier_1_cases_that_need_no_plan_build_on_the_host(lib):
    """Every builder but the two that create a backprojection plan: their workspace sizes come from pure host
    functions, their definitions from the host."""
    for build in gc.TIER1:
        if build in (gc.bp_run_calls, gc.relocate_calls):
            continue
        for call in build(lib):
            for sizes in call.variants:
                assert all(v > 0 for v in sizes.values()), call.name
            if call.refusal:
                (name, short), = call.refusal.items()
                assert short == min(v[name] for v in call.variants) - 1, call.name


# (function, arguments with `rows` first or None where nothing counts rows, index of the rows argument, a refused size)
def _size_functions(lib):
    return [
        ("bpmf_mf_workspace_bytes", (17, 9709, 3, 2, 3), 2, (0, 9709, 3, 2, 3)),
        ("bpmf_mf_workspace_bytes", (17, 9709, 3, 2, 3), 2, (17, 16, 3, 2, 3)),
        ("bpmf_mf_full_workspace_bytes", (17, 9709, 3, 2, 3), 2, (17, 9709, 3, 0, 3)),
        ("bpmf_intertemplate_workspace_bytes", (12, 3, 2, 12), 0, (12, 3, 2, 32)),
        ("bpmf_intertemplate_workspace_bytes", (12, 3, 2, 12), 0, (0, 3, 2, 12)),
        ("bpmf_tdt_workspace_bytes", (5, 447, 17, 34), 0, (5, 33, 17, 34)),
        ("bpmf_tdt_workspace_bytes", (5, 447, 17, 34), 0, (5, 447, 17, 0)),
        ("bpmf_row_median_mad_workspace_bytes", (16, 4096), 0, (0, 4096)),
        ("bpmf_row_median_mad_workspace_bytes", (16, 4096), 0, (16, 0)),
        ("bpmf_tdt_mad_workspace_bytes", (3, 7777, 500, 50), 0, (3, 499, 500, 50)),
        ("bpmf_tdt_mad_workspace_bytes", (3, 7777, 500, 50), 0, (65536, 7777, 500, 50)),
        ("bpmf_tdt_mad_workspace_bytes", (3, 7777, 500, 50), 0, (3, 7777, 500, 0)),
        ("bpmf_row_kurtosis_workspace_bytes", (3, 8193), 0, (65536, 8193)),
        ("bpmf_row_kurtosis_workspace_bytes", (3, 8193), 0, (3, 0)),
        ("bpmf_svdwf_workspace_bytes", (3, 9, 48, 1), 3, (3, 9, 0, 1)),
        ("bpmf_svdwf_workspace_bytes", (3, 9, 48, 1), 3, (3, 513, 600, 1)),
        ("bpmf_bandpass_rows_workspace_bytes", (70, 100, 1, 0), 0, (70, 2 ** 24 + 1, 1, 0)),
        ("bpmf_multiband_workspace_bytes", (66, 130, 6), 0, (66, 16385, 6)),
        ("bpmf_multiband_workspace_bytes", (66, 130, 6), 0, (66, 0, 6)),
        ("bpmf_flag_multiples_workspace_bytes", (130,), 0, (2 ** 31 - 1,)),
        ("bpmf_bp_location_uncertainty_workspace_bytes", (3, 864), 0, (65536, 864)),
        ("bpmf_bp_location_uncertainty_workspace_bytes", (3, 864), 0, (3, 0)),
    ]


def test_workspace_sizes_are_0_for_refused_sizes_and_never_shrink_with_the_rows(lib, hip_opts):
    for min_n in (None, 0):                                # the row statistics' two routes size differently
        if min_n is not None:
            hip_opts("stats.row_grid_min_n", min_n)
        for name, good, rows_at, refused in _size_functions(lib):
            fn = getattr(lib, name)
            assert fn(*refused) == 0, (name, refused)
            sizes = []
            for rows in (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 1000):
                args = list(good)
                args[rows_at] = rows
                sizes.append(fn(*args))
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (name, sizes)
            assert fn(*good) > 0, (name, good)

