"""The checks of seam_cases.py can fail: each is fed the host definition's own output with one defect of a slab loop
planted -- the second slab written at the first slab's offset, the last (partial) slab left at the junk fill, a
boundary off by one row, the per-row statistics of slab 2 taken from slab 1, the first output sample of a running
kurtosis row left zero -- and must reject it; the undamaged output must pass.  No GPU: test_gpu_batch_seams.py feeds
the same checks what the device wrote."""
import numpy as np
import pytest

import seam_cases as sc

SLAB_DEFECTS = sc.DEFECTS[:3]


def _stat_from_first_slab(rows, slab):
    """Row index whose statistics each row takes when the median / MAD pointers are not advanced from slab to slab."""
    return np.arange(rows) % slab


# ------------------------------------------------------------------------------ rows ---
@pytest.mark.parametrize("rows,slabs", [(5, sc.ENVELOPE_BATCHES), (sc.MAD_ROWS, sc.MAD_SLABS), (sc.SAT_ROWS, [sc.ROW_LIMIT]),
                                        (sc.STATS_SHAPE[0], [sc.ROW_LIMIT]), (sc.ROWKURT_SHAPE[0], [sc.ROW_LIMIT]),
                                        (200_000, [sc.ROW_LIMIT, 70_000])])
def test_sampled_rows_hold_the_rows_around_every_boundary(rows, slabs):
    sample = sc.sampled_rows(rows, slabs, seed=1)
    assert np.array_equal(sample, np.unique(sample)) and sample[0] == 0 and sample[-1] == rows - 1
    must = {0, rows - 1}
    for slab in slabs:
        starts = list(range(0, rows, slab))
        assert sc.slab_boundaries(rows, slab) == starts[1:] and sum(sc.slab_lengths(rows, slab)) == rows
        for c in starts[1:]:
            must |= {r for r in (c - 1, c, c + 1) if r < rows}
    assert must <= set(sample.tolist())
    assert sample.size == min(rows, len(must) + sc.N_SEEDED)
    assert np.array_equal(sample, sc.sampled_rows(rows, slabs, seed=1))         # seeded


def test_special_rows_lie_on_both_sides_of_the_seam_and_in_the_sample():
    for special, sample in ((sc.SAT_SPECIAL, sc.saturated_sample()), (sc.STATS_SPECIAL, sc.stats_sample()),
                            ([("constant", r) for r in sc.ROWKURT_CONSTANT], sc.rowkurt_sample())):
        rows = [r for _, r in special]
        assert set(rows) <= set(sample.tolist())
        assert min(rows) < sc.ROW_LIMIT <= max(rows)
        behind = {k for k, r in special if r >= sc.ROW_LIMIT}
        assert len(behind) == len([r for r in rows if r >= sc.ROW_LIMIT])       # every row behind the seam another kind
    assert {k for k, r in sc.SAT_SPECIAL if r < sc.ROW_LIMIT} == {"gapped", "all_zero", "mostly_missing", "below_threshold"}


def test_rows_carry_their_own_data():
    a = sc.row_noise(np.arange(1000), 64, seed=5)
    assert np.array_equal(a[[3, 998]], sc.row_noise([3, 998], 64, seed=5))      # a row can be drawn on its own
    assert np.unique(a.round(12), axis=0).shape[0] == 1000
    assert abs(a.mean()) < 0.02 and abs(a.std() - 1.0) < 0.02 and np.isfinite(a).all()
    assert not np.array_equal(a, sc.row_noise(np.arange(1000), 64, seed=6))
    scale, offset = sc.row_scale_offset(np.arange(1000), seed=5)
    assert np.unique(scale).size == 1000 and scale.min() >= 0.5 and np.abs(offset).max() <= 1.0


# -------------------------------------------------------------------------- envelope ---
@pytest.mark.parametrize("n", sc.ENVELOPE_N)
def test_envelope_check_passes_the_definition(n):
    tr = sc.envelope_traces(n)
    assert tr.shape == (5, 1, n) and tr.dtype == np.float32 and not tr[1].any() and tr[3].min() > 900
    assert sc.check_envelope(sc.envelope_definition(tr), tr, 2) == []


@pytest.mark.parametrize("defect", SLAB_DEFECTS)
@pytest.mark.parametrize("slab", [1, 2])
@pytest.mark.parametrize("n", sc.ENVELOPE_N)
def test_envelope_check_rejects(n, slab, defect):
    tr = sc.envelope_traces(n)
    out = sc.plant(sc.envelope_definition(tr), slab, defect)
    assert sc.check_envelope(out, tr, slab), (n, slab, defect)


@pytest.mark.parametrize("n", sc.ENVELOPE_F32_N)
def test_envelope_float32_check_passes_the_reference_route(n):
    """The reference's own float32 route passes (its error is the yardstick); 5 x its error does not."""
    from oracle.features_host import envelope_host
    tr = sc.envelope_traces(n)
    ref = np.stack([envelope_host(x) for x in tr.reshape(5, n)]).reshape(tr.shape)
    assert ref.dtype == np.float32 and sc.check_envelope_f32(ref, tr, 2) == []
    assert sc.check_envelope_f32(sc.envelope_definition(tr), tr, 2) == []
    dev, err = sc.envelope_f32_errors(ref, tr)
    assert np.array_equal(dev, err)
    exact = sc.envelope_f64(tr)
    ulp = np.spacing(exact.max(axis=-1, keepdims=True).astype(np.float32))
    worse = (exact + np.maximum(5.0 * err, 5.0).reshape(5, 1, 1) * ulp).astype(np.float32)
    assert sc.check_envelope_f32(worse, tr, 2), n


@pytest.mark.parametrize("defect", SLAB_DEFECTS)
@pytest.mark.parametrize("n", sc.ENVELOPE_F32_N)
def test_envelope_float32_check_rejects(n, defect):
    from oracle.features_host import envelope_host
    tr = sc.envelope_traces(n)
    ref = np.stack([envelope_host(x) for x in tr.reshape(5, n)]).reshape(tr.shape)
    assert sc.check_envelope_f32(sc.plant(ref, 2, defect), tr, 2), (n, defect)


# ---------------------------------------------------------------- saturated envelopes ---
@pytest.fixture(scope="module")
def saturated():
    tr = sc.saturated_traces()
    feat, avail, dead = sc.saturated_definition(tr)
    for a in (tr, feat, avail, dead):
        a.setflags(write=False)
    return tr, feat, avail, dead


def test_saturated_check_passes_the_definition(saturated):
    tr, feat, avail, dead = saturated
    assert tr.shape == sc.SAT_SHAPE and sc.SAT_ROWS == 65_538
    kinds = dict((r, k) for k, r in sc.SAT_SPECIAL)
    for r, k in kinds.items():
        assert dead[r] == (k in sc.SAT_DROPPED), (r, k)    # (the transform fills a gap: such a channel stays alive)
    assert dead.sum() == sum(k in sc.SAT_DROPPED for k in kinds.values())
    assert sc.check_saturated(feat, avail, tr, sc.ROW_LIMIT) == []


@pytest.mark.parametrize("defect", sc.DEFECTS)
def test_saturated_check_rejects(saturated, defect):
    tr, feat, avail, dead = saturated
    if defect == "stat_from_first_slab":
        out, _, _ = sc.saturated_definition(tr, stats_from=_stat_from_first_slab(sc.SAT_ROWS, sc.ROW_LIMIT))
    else:
        out = sc.plant(feat.reshape(sc.SAT_ROWS, -1), sc.ROW_LIMIT, defect).reshape(sc.SAT_SHAPE)
    assert sc.check_saturated(out, avail, tr, sc.ROW_LIMIT), defect


def test_saturated_check_rejects_an_availability_from_the_wrong_station(saturated):
    tr, feat, avail, dead = saturated
    wrong = avail.copy()
    wrong[-1] = avail[0]                                   # the last station: the three channels behind the seam
    assert avail[-1] != avail[0]
    assert sc.check_saturated(feat, wrong, tr, sc.ROW_LIMIT)


# ------------------------------------------------------------------- row median / MAD ---
@pytest.fixture(scope="module")
def stats_x():
    x = sc.stats_rows()
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("skip", [False, True])
def test_row_stats_check_passes_the_definition(stats_x, skip):
    x = stats_x
    assert x.shape == sc.STATS_SHAPE
    med, mad, nz = sc.stats_definition(x, skip)
    assert sc.check_row_stats(med, mad, nz, x, skip, sc.ROW_LIMIT) == []
    kinds = dict((r, k) for k, r in sc.STATS_SPECIAL)
    for r, k in kinds.items():
        assert np.isnan(med[r]) == (k == "nan" or (k == "all_zero" and skip)), (r, k)
        assert (nz[r] > 0) == (k in ("zeros", "neg_zero", "zeros_neg_zero", "all_zero") or (k == "ties" and (x[r] == 0).any()))


@pytest.mark.parametrize("defect", sc.DEFECTS)
@pytest.mark.parametrize("skip", [False, True])
def test_row_stats_check_rejects(stats_x, skip, defect):
    x = stats_x
    med, mad, nz = sc.stats_definition(x, skip)
    if defect == "stat_from_first_slab":
        src = _stat_from_first_slab(x.shape[0], sc.ROW_LIMIT)
        bad = (med[src], mad[src], nz[src])
    else:
        bad = tuple(sc.plant(a, sc.ROW_LIMIT, defect) for a in (med, mad, nz))
    assert sc.check_row_stats(*bad, x, skip, sc.ROW_LIMIT), defect
    for k in range(3):                                     # each output on its own
        one = [med, mad, nz]
        one[k] = bad[k]
        assert sc.check_row_stats(*one, x, skip, sc.ROW_LIMIT), (defect, k)


# ----------------------------------------------------------------------- row kurtosis ---
@pytest.fixture(scope="module")
def rowkurt():
    x = sc.rowkurt_rows()
    want = sc.rowkurt_definition(x)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def test_row_kurtosis_check_passes_the_definition(rowkurt):
    x, want = rowkurt
    assert x.shape == sc.ROWKURT_SHAPE
    assert np.isnan(want[list(sc.ROWKURT_CONSTANT)]).all() and np.isnan(want).sum() == 2
    assert sc.check_row_kurtosis(want, x, sc.ROW_LIMIT) == []


@pytest.mark.parametrize("defect", sc.DEFECTS)
def test_row_kurtosis_check_rejects(rowkurt, defect):
    x, want = rowkurt
    if defect == "stat_from_first_slab":
        out = sc.rowkurt_definition(x, mean_from=_stat_from_first_slab(x.shape[0], sc.ROW_LIMIT))
    else:
        out = sc.plant(want, sc.ROW_LIMIT, defect)
    assert sc.check_row_kurtosis(out, x, sc.ROW_LIMIT), defect


# ---------------------------------------------------------------------- MAD threshold ---
@pytest.fixture(scope="module", params=sc.MAD_CASES, ids=lambda c: f"n{c[0]}-W{c[1]}")
def mad_case(request):
    n, W, ov = request.param
    x, wn = sc.mad_rows(n)
    wins, full = sc.mad_definition(x, W, ov, wn)
    for a in (x, wn, wins, full):
        a.setflags(write=False)
    return n, W, ov, x, wn, wins, full


def test_mad_rows_are_the_rows_the_issue_names(mad_case):
    n, W, ov, x, wn, wins, full = mad_case
    nz = (x == 0).sum(axis=1)
    assert x.shape == (sc.MAD_ROWS, n) and wn.shape == (n,)
    assert nz[2] == 0 and nz[5] == 0 and len(set(nz[[0, 1, 3, 4, 6]].tolist())) == 5 and nz.max() <= n
    assert x[1, 700:-900].all() and nz[1] >= 1590        # zeros only at the ends (all but the peaks planted there)
    assert np.unique(x[4]).size < 60
    assert (x > np.minimum(full, sc.MAD_ROW_CAP[:, None])).sum(axis=1).min() > 0    # every row has candidates


def test_mad_check_passes_the_definition(mad_case):
    n, W, ov, x, wn, wins, full = mad_case
    assert sc.check_mad_threshold(wins, full, x, wn, W, ov, 3) == []


@pytest.mark.parametrize("defect", sc.DEFECTS)
@pytest.mark.parametrize("slab", [s for s in sc.MAD_SLABS if s < sc.MAD_ROWS])
def test_mad_check_rejects(mad_case, slab, defect):
    n, W, ov, x, wn, wins, full = mad_case
    if defect == "stat_from_first_slab":
        bw, bf = sc.mad_definition(x, W, ov, wn, stats_from=_stat_from_first_slab(sc.MAD_ROWS, slab))
    else:
        bw, bf = sc.plant(wins, slab, defect), sc.plant(full, slab, defect)
    assert sc.check_mad_threshold(bw, bf, x, wn, W, ov, slab)
    assert sc.check_mad_threshold(bw, full, x, wn, W, ov, slab)      # each output on its own
    assert sc.check_mad_threshold(wins, bf, x, wn, W, ov, slab)


def test_mad_candidates_check(mad_case):
    from seismic_bpmf_amd.threshold import candidate_dtype
    n, W, ov, x, wn, wins, full = mad_case
    t = np.minimum(full, sc.MAD_ROW_CAP[:, None])
    r, i = np.nonzero(x > t)
    cand = np.zeros(r.size, candidate_dtype)
    cand["row"], cand["index"], cand["cc"], cand["threshold"] = r, i, x[r, i], t[r, i]
    assert sc.check_mad_candidates(cand, x, full, 3) == []
    assert sc.check_mad_candidates(cand[1:], x, full, 3)
    moved = cand.copy()
    moved["row"][moved["row"] == 6] = 3                    # the last slab's records under another row
    assert sc.check_mad_candidates(moved, x, full, 3)


@pytest.mark.parametrize("n,W,ov", sc.MAD_CASES)
def test_mad_limits_give_the_slabs_they_are_meant_to(n, W, ov):
    """The limits the GPU test sets make ThresholdGPU take 1, 2, 3 and 7 rows per call -- slabs of 3 + 3 + 1 and
    1 x 7 among them -- with the library's own workspace size (host code)."""
    from seismic_bpmf_amd import _lib
    from seismic_bpmf_amd.threshold import mad_rows_per_call
    lib = _lib.lib()
    shift = sc.mad_shift(W, ov)
    for min_n in (None, 4096):
        if min_n is not None:
            _lib.set_option("stats.row_grid_min_n", min_n)
        try:
            per_row = int(lib.bpmf_tdt_mad_workspace_bytes(64, n, W, shift)) // 64
            assert per_row > 0
            got = {}
            for slab in sc.MAD_SLABS:
                chunk = mad_rows_per_call(sc.MAD_ROWS, per_row, sc.mad_limit(per_row, slab))
                got[slab] = sc.slab_lengths(sc.MAD_ROWS, chunk)
        finally:
            _lib.set_option("stats.row_grid_min_n", _lib.get_option("stats.row_grid_min_n")[1])
        assert got == {1: [1] * 7, 2: [2, 2, 2, 1], 3: [3, 3, 1], 7: [7]}, (min_n, got)
    assert mad_rows_per_call(70_000, 1, 4 << 30) == 65_535 and mad_rows_per_call(7, 100, 10) == 1


# ------------------------------------------------------------------- running kurtosis ---
def test_running_kurtosis_ceiling_signals():
    """The window ceilings are the first and the last whose LDS image exceeds 64 KB, and the signals hold what the
    issue asks for: both scales, outputs that stay zero (a flat window) beside finite non-zero ones."""
    lds = [(W + 256) * 4 for W in sc.KURT_CEILING_W]
    assert lds[0] == 64 * 1024 and lds[1] > 64 * 1024 and sc.KURT_CEILING_W[2] == sc.KURT_W_MAX and lds[2] == 132_096
    W = sc.KURT_CEILING_W[0]
    x = sc.kurt_ceiling_signal(W)
    assert x.shape == (1, 2, W + 300) and 20 < x[0, 1].std() < 40 and np.all(x[0, 0, 10:W + 60] == 0.5)
    want = sc.running_kurtosis_definition(x, W)
    assert not want[..., :W].any() and np.isfinite(want).all()
    assert (want[0, 1, W:] != 0).all() and (want[0, 0, W + 10:W + 61] == 0).all() and (want[0, 0, W:] != 0).sum() == 249
    assert sc.check_running_kurtosis(want, x, W, 1) == []
    assert sc.check_running_kurtosis(sc.plant_first_sample_zero(want, W, 1), x, W, 1)
    one = sc.kurt_ceiling_signal(W, W + 1)
    assert one.shape == (1, 2, W + 1) and np.array_equal(one, x[..., :W + 1])
    w1 = sc.running_kurtosis_definition(one, W)
    assert (w1[..., W] != 0).all() and sc.check_running_kurtosis(sc.plant_first_sample_zero(w1, W, 1), one, W, 1)
    none = sc.kurt_ceiling_signal(W, W)
    assert not sc.running_kurtosis_definition(none, W).any()


@pytest.fixture(scope="module")
def kurt_many():
    x = sc.kurt_many_signal()
    want = sc.running_kurtosis_definition(x, sc.KURT_MANY_W)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def test_running_kurtosis_check_passes_the_definition(kurt_many):
    x, want = kurt_many
    S, C, n = sc.KURT_MANY_SHAPE
    assert x.shape == (S, C, n) and S * C == 65_538
    assert (want[..., sc.KURT_MANY_W:] != 0).all() and not want[..., :sc.KURT_MANY_W].any()
    assert sc.check_running_kurtosis(want, x, sc.KURT_MANY_W, sc.ROW_LIMIT) == []


@pytest.mark.parametrize("defect", SLAB_DEFECTS + ("first_sample_zero",))
def test_running_kurtosis_check_rejects(kurt_many, defect):
    x, want = kurt_many
    S, C, n = sc.KURT_MANY_SHAPE
    if defect == "first_sample_zero":
        out = sc.plant_first_sample_zero(want, sc.KURT_MANY_W, sc.ROW_LIMIT)
    else:
        out = sc.plant(want.reshape(S * C, n), sc.ROW_LIMIT, defect).reshape(x.shape)
    found = sc.check_running_kurtosis(out, x, sc.KURT_MANY_W, sc.ROW_LIMIT)
    assert found, defect
    if defect == "first_sample_zero":
        assert "2 rows" in found[0] and "65535" in found[0]      # the first row of either slab
