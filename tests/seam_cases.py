"""Inputs and checks of the row-batch seams of the feature stages (envelope, saturated envelopes, row median / MAD,
row kurtosis, MAD threshold, running kurtosis), shared by test_gpu_batch_seams.py (which feeds the checks what the
device wrote) and test_batch_seams_host.py (which feeds them the host definition's output with one planted defect,
to show that each check can fail).  Not a test module; imports no torch.

Every check takes plain NumPy arrays -- the output of the call under test, its input, the slab size the call split
its rows by -- and returns a list of findings (empty: passed).  It compares with the host definition: everywhere
where that is cheap, on `sampled_rows` where the definition loops per row.  Every row carries its own data
(`row_noise`: the row index is part of the seed; its own scale and offset), so a slab written at another slab's
offset, or twice, differs on every row."""
import numpy as np

ROW_LIMIT = 65535                  # gridDim.y: the rows of one launch
N_SEEDED = 64
DEFECTS = ("second_slab_at_first_offset", "last_slab_junk", "boundary_off_by_one", "stat_from_first_slab")


# ------------------------------------------------------------------------------ rows ---
def slab_boundaries(rows, slab):
    """First rows of the second, third, ... slab."""
    return list(range(int(slab), int(rows), int(slab)))


def slab_lengths(rows, slab):
    return [min(int(slab), rows - r0) for r0 in range(0, rows, int(slab))]


def sampled_rows(rows, slabs, seed=0, extra=()):
    """The rows a per-row host definition is evaluated on: the first, the last, c-1, c, c+1 around every boundary c
    of every slab size in `slabs`, the rows of `extra`, and N_SEEDED seeded rows besides (as many as are left)."""
    must = {0, rows - 1} | {int(r) for r in extra}
    for slab in slabs:
        for c in slab_boundaries(rows, slab):
            must |= {c - 1, c, c + 1}
    must = {r for r in must if 0 <= r < rows}
    rest = np.setdiff1d(np.arange(rows), np.fromiter(must, dtype=np.int64, count=len(must)))
    rng = np.random.default_rng(seed)
    seeded = rng.choice(rest, size=min(N_SEEDED, rest.size), replace=False)
    return np.array(sorted(must | {int(r) for r in seeded}), dtype=np.int64)


def _mix(z):
    """splitmix64's finaliser on uint64 arrays (wraps silently)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _uniform(key):
    return ((key >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)


def row_noise(row_ids, n, seed):
    """(len(row_ids), n) float64 standard-normal values; element (r, j) is a function of (seed, r, j) alone, so
    any subset of rows can be drawn again on its own."""
    r = np.asarray(row_ids, dtype=np.uint64).reshape(-1, 1)
    j = np.arange(n, dtype=np.uint64).reshape(1, -1)
    base = _mix(r + np.uint64((int(seed) * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF))
    k1 = _mix(base + j * np.uint64(2) + np.uint64(1))
    k2 = _mix(base + j * np.uint64(2) + np.uint64(2))
    return np.sqrt(-2.0 * np.log(_uniform(k1))) * np.cos(2.0 * np.pi * _uniform(k2))


def row_scale_offset(row_ids, seed):
    """A scale in [0.5, 4) and an offset in [-1, 1) for every row, from the row index."""
    r = np.asarray(row_ids, dtype=np.uint64)
    u = _uniform(_mix(r * np.uint64(3) + np.uint64(seed) + np.uint64(0xABCDEF)))
    v = _uniform(_mix(r * np.uint64(5) + np.uint64(seed) + np.uint64(0x123457)))
    return 0.5 + 3.5 * u, 2.0 * v - 1.0


def _junk(a):
    """An array like `a` filled with 0xFF bytes: what the GPU tests leave in the allocator's next blocks."""
    out = np.empty_like(a)
    out.view(np.uint8)[...] = 0xFF
    return out


def plant(want, slab, defect):
    """`want (rows, ...)` with one of the first three DEFECTS of a slab loop planted."""
    out = np.array(want, copy=True)
    rows = out.shape[0]
    bounds = slab_boundaries(rows, slab)
    assert bounds, "one slab only: nothing to plant"
    junk = _junk(out)
    if defect == "second_slab_at_first_offset":
        c, e = bounds[0], min(rows, 2 * bounds[0])
        out[:e - c] = want[c:e]
        out[c:e] = junk[c:e]
    elif defect == "last_slab_junk":
        out[bounds[-1]:] = junk[bounds[-1]:]
    elif defect == "boundary_off_by_one":
        for c in bounds:
            out[c] = want[c - 1]
    else:
        raise ValueError(defect)
    return out


def _bad_rows(name, bad, slab):
    bad = np.flatnonzero(bad)
    if not bad.size:
        return []
    return [f"{name}: {bad.size} rows differ, first {bad[:6].tolist()} (slabs of {slab})"]


# -------------------------------------------------------------------------- envelope ---
ENVELOPE_N = (1, 2, 3, 16, 1001, 4096)
ENVELOPE_F32_N = ENVELOPE_N + (20_000, 131_071)
ENVELOPE_BATCHES = (1, 2, 5)               # channels per batch: 5, 2 + 2 + 1 and 1 batches of the 5 channels


def envelope_traces(n):
    """(5, 1, n) float32: a zero channel, a channel with a gap, a channel with a +1000 offset; all of them different."""
    scale = np.array([1.0, 1.0, 0.3, 2.0, 7.0])
    tr = (row_noise(np.arange(5), n, seed=n) * scale[:, None]).astype(np.float32)
    tr[1] = 0.0
    tr[2, n // 3: n // 2] = 0.0
    tr[3] += np.float32(1000.0)
    return tr.reshape(5, 1, n)


def envelope_f64(traces):
    from scipy.signal import hilbert
    return np.abs(hilbert(np.asarray(traces, dtype=np.float64), axis=-1))


def envelope_definition(traces):
    """The float64 envelope rounded to float32: what envelope() is within an ulp of."""
    return envelope_f64(traces).astype(np.float32)


def check_envelope(out, traces, slab):
    """The criterion of test_device_envelopes_against_float64_and_the_reference_output on every sample: within
    1.0001 ulp of the float64 SciPy envelope rounded to float32."""
    out = np.asarray(out)
    if out.dtype != np.float32 or out.shape != np.shape(traces):
        return [f"envelope: {out.dtype} {out.shape}"]
    exact = envelope_f64(traces)
    ok = np.abs(out - exact) <= np.spacing(np.float32(exact)) * 1.0001 + 1e-300
    n = out.shape[-1]
    return _bad_rows("envelope", ~ok.reshape(-1, n).all(axis=1), slab)


_F32_YARDSTICK = {}


def _envelope_f32_yardstick(traces):
    """(float64 envelope, ulp of the channel maximum, error of the reference's float32 route in those ulp) of the
    channels of `traces`, computed once per set of traces."""
    from oracle.features_host import envelope_host
    tr = np.ascontiguousarray(traces)
    key = (tr.shape, hash(tr.tobytes()))
    if key not in _F32_YARDSTICK:
        flat = tr.reshape(-1, tr.shape[-1])
        exact = envelope_f64(flat)
        ulp = np.spacing(exact.max(axis=1).astype(np.float32)).astype(np.float64)
        ref = np.stack([envelope_host(x) for x in flat]).astype(np.float64)
        _F32_YARDSTICK[key] = (exact, ulp, np.abs(ref - exact).max(axis=1) / ulp)
    return _F32_YARDSTICK[key]


def envelope_f32_errors(out, traces):
    """Per channel, in ulp of the channel's largest float64 envelope value: (error of `out`, error of the reference's
    own float32 route, oracle.features_host.envelope_host), both against the float64 envelope."""
    exact, ulp, ref_err = _envelope_f32_yardstick(traces)
    dev = np.asarray(out, dtype=np.float64).reshape(exact.shape)
    return np.abs(dev - exact).max(axis=1) / ulp, ref_err


def check_envelope_f32(out, traces, slab):
    """envelope(precision="float32"): per channel at most max(4 x the reference route's own error, 4 ulp of the
    channel maximum) from the float64 envelope.  4 x: another FFT factorisation changes the constant of an
    eps log n error, not its order; 4 ulp: channels on which the reference happens to be nearly exact."""
    out = np.asarray(out)
    if out.dtype != np.float32 or out.shape != np.shape(traces):
        return [f"envelope float32: {out.dtype} {out.shape}"]
    dev, ref = envelope_f32_errors(out, traces)
    return _bad_rows("envelope float32", ~(dev <= np.maximum(4.0 * ref, 4.0)), slab)


# ---------------------------------------------------------------- saturated envelopes ---
SAT_SHAPE = (21_846, 3, 16)                # 65 538 channels: slabs of 65 535 + 3
SAT_ROWS = SAT_SHAPE[0] * SAT_SHAPE[1]
# (kind, row) -- three rows lie behind the seam, so the far side holds three of the four kinds.  The one left out is
# the mostly missing channel: the Hilbert transform fills a gap of the trace, so its envelope has no zeros and it is
# a live channel like the gapped one; the channel of zeros (NaN statistics) and the one below the anomaly threshold
# are the two ways of being dropped
SAT_SPECIAL = (("gapped", 65_520), ("all_zero", 65_523), ("mostly_missing", 65_526), ("below_threshold", 65_529),
               ("mostly_missing", 65_534),
               ("gapped", 65_535), ("all_zero", 65_536), ("below_threshold", 65_537))
SAT_DROPPED = ("all_zero", "below_threshold")


def _sat_rows(row_ids):
    row_ids = np.asarray(row_ids, dtype=np.int64)
    n = SAT_SHAPE[2]
    scale, offset = row_scale_offset(row_ids, seed=3)
    x = (row_noise(row_ids, n, seed=3) * scale[:, None] + 0.1 * offset[:, None]).astype(np.float32)
    for kind, row in SAT_SPECIAL:
        at = np.flatnonzero(row_ids == row)
        if kind == "gapped":
            x[at, 5:9] = 0.0
        elif kind == "all_zero":
            x[at] = 0.0
        elif kind == "mostly_missing":
            x[at, :11] = 0.0
        elif kind == "below_threshold":
            x[at] *= np.float32(1.0e-14)
    return x


def saturated_traces():
    return _sat_rows(np.arange(SAT_ROWS)).reshape(SAT_SHAPE)


def masked_median(v, valid):
    """np.median of the valid entries of every row of a float32 matrix (NaN for a row without any): float32, the
    middle value or the float32 mean of the two middle values."""
    big = np.where(valid, v, np.float32(np.inf))
    s = np.sort(big, axis=1)
    k = valid.sum(axis=1)
    rows = np.arange(v.shape[0])
    lo, hi = s[rows, np.maximum(k - 1, 0) // 2], s[rows, k // 2 % v.shape[1]]
    with np.errstate(all="ignore"):
        med = np.where(lo == hi, lo, (lo + hi) / np.float32(2.0)).astype(np.float32)
    return np.where(k > 0, med, np.float32(np.nan))


def saturated_definition(traces, anomaly_threshold=1.0e-11, max_dynamic_range=1.0e5, stats_from=None):
    """The device's formulation of BPMF/template_search.py:1525-1572 on the host, all channels at once: the float64
    envelope rounded to float32, np.median / MAD of its non-zero samples, (x - median) / MAD in float32, 0 for
    missing samples and dead channels, capped.  Returns (features, availability, dead).  `stats_from`: row index
    per row whose (median, MAD, dead) to use instead of the row's own -- the planted defect."""
    tr = np.asarray(traces)
    S, C, n = tr.shape
    env = envelope_definition(tr).reshape(S * C, n)
    valid = env != 0.0
    med = masked_median(env, valid)
    with np.errstate(all="ignore"):
        mad = masked_median(np.abs(env - med[:, None]), valid)
    dead = ((~valid).sum(axis=1) > n / 2) | ~(mad.astype(np.float64) >= anomaly_threshold)
    availability = (~dead).reshape(S, C).sum(axis=1).astype(np.int32)
    if stats_from is not None:
        med, mad, dead = med[stats_from], mad[stats_from], dead[stats_from]
    with np.errstate(all="ignore"):
        std = (env - med[:, None]) / mad[:, None]
    std = np.where(env == 0.0, np.float32(0.0), std)
    feat = np.where(dead[:, None], np.float32(0.0), np.minimum(std, np.float32(max_dynamic_range)))
    return feat.astype(np.float32).reshape(S, C, n), availability, dead


def saturated_sample(slab=ROW_LIMIT):
    return sampled_rows(SAT_ROWS, [slab], seed=31, extra=[r for _, r in SAT_SPECIAL])


def check_saturated(features, availability, traces, slab):
    """Features of the sampled channels against oracle.features_host.saturated_envelopes_host with the bounds of
    test_device_envelopes_against_float64_and_the_reference_output (the reference's float32 FFT round-off, 40 ulp
    of the channel maximum in MAD units, plus 1e-5 relative -- 5e-2 where that noise is not small); the channels the
    reference drops dropped; the availability vector equal over all stations (host formulation of all channels,
    and the reference on the sampled stations)."""
    from scipy.stats import median_abs_deviation as scimad
    from oracle.features_host import envelope_host, saturated_envelopes_host
    tr = np.asarray(traces)
    S, C, n = tr.shape
    feat = np.asarray(features)
    if feat.dtype != np.float32 or feat.shape != tr.shape:
        return [f"saturated envelopes: {feat.dtype} {feat.shape}"]
    found = []
    _, avail_all, _ = saturated_definition(tr)
    availability = np.asarray(availability)
    if availability.shape != avail_all.shape or not np.array_equal(availability, avail_all):
        found += _bad_rows("availability (stations)", availability.reshape(-1) != avail_all.reshape(-1)
                           if availability.shape == avail_all.shape else np.ones(1, bool), slab)
    rows = saturated_sample(slab)
    flat, fflat = tr.reshape(S * C, n), feat.reshape(S * C, n)
    gold, gold_avail = saturated_envelopes_host(flat[rows].reshape(-1, 1, n).copy())
    gold = gold.reshape(-1, n)
    bad = np.zeros(rows.size, bool)
    for i, r in enumerate(rows):
        got = fflat[r]
        if not gold[i].any():
            bad[i] = bool(got.any()) or not np.all(got == got)
            continue
        gold_env = envelope_host(flat[r])
        ulp_max = np.spacing(np.abs(gold_env).max().astype(np.float32))
        noise = 40 * ulp_max / scimad(gold_env[gold_env != 0])
        rel = 1e-5 if noise < 1e-3 else 5e-2
        bad[i] = not np.all(np.abs(got.astype(np.float64) - gold[i]) <= noise + rel * np.abs(gold[i]))
    found += _bad_rows("features (sampled channels)", np.isin(np.arange(S * C), rows[bad]), slab)
    # the reference's own availability, on the stations all of whose channels are sampled
    sampled = np.zeros(S * C, bool)
    sampled[rows] = True
    live = np.zeros(S * C, np.int32)
    live[rows] = gold_avail
    whole = sampled.reshape(S, C).all(axis=1)
    if availability.shape == (S,):
        found += _bad_rows("availability (reference, sampled stations)",
                           whole & (availability != live.reshape(S, C).sum(axis=1)), slab)
    return found


# ------------------------------------------------------------------- row median / MAD ---
STATS_SHAPE = (65_538, 64)
# (kind, row): zeros and a -0.0 share a row behind the seam, where there are three rows for four kinds
STATS_SPECIAL = (("zeros", 65_510), ("ties", 65_513), ("neg_zero", 65_516), ("nan", 65_519), ("all_zero", 65_522),
                 ("ties", 65_534),
                 ("zeros_neg_zero", 65_535), ("ties", 65_536), ("nan", 65_537))


def stats_rows():
    rows, n = STATS_SHAPE
    ids = np.arange(rows)
    scale, offset = row_scale_offset(ids, seed=5)
    x = (row_noise(ids, n, seed=5) * scale[:, None] + offset[:, None]).astype(np.float32)
    for kind, r in STATS_SPECIAL:
        if kind in ("zeros", "zeros_neg_zero"):
            x[r, 3:40:3] = 0.0
        if kind in ("neg_zero", "zeros_neg_zero"):
            x[r, 1] = -0.0
        if kind == "ties":
            x[r] = np.round(x[r] * 2) / 2
        if kind == "nan":
            x[r, 7] = np.nan
        if kind == "all_zero":
            x[r] = 0.0
    return x


def stats_sample(slab=ROW_LIMIT):
    return sampled_rows(STATS_SHAPE[0], [slab], seed=53, extra=[r for _, r in STATS_SPECIAL])


def _median_mad(v):
    import warnings
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = np.median(v) if v.size else np.float32(np.nan)
        d = np.median(np.abs(v - m)) if v.size else np.float32(np.nan)
    return np.float32(m), np.float32(d)


def stats_definition(x, skip_zeros):
    """(median, MAD, n_zero) of every row, vectorised (NaN rows by np.median's rule: NaN); the check below holds it
    against np.median row by row on the sample."""
    x = np.asarray(x, dtype=np.float32)
    valid = (x != 0.0) if skip_zeros else np.ones(x.shape, bool)
    nan_row = np.isnan(x).any(axis=1)
    med = masked_median(x, valid)
    with np.errstate(all="ignore"):
        mad = masked_median(np.abs(x - med[:, None]), valid)
    med[nan_row] = np.nan
    mad[nan_row] = np.nan
    return med, mad, (x == 0.0).sum(axis=1).astype(np.int64)


def check_row_stats(med, mad, nz, x, skip_zeros, slab):
    """np.median / MAD of the sampled rows (over the non-zero samples when `skip_zeros`), bit for bit; the number of
    zeros of every row."""
    med, mad, nz = np.asarray(med), np.asarray(mad), np.asarray(nz)
    rows = x.shape[0]
    if med.shape != (rows,) or mad.shape != (rows,) or nz.shape != (rows,) or med.dtype != np.float32 or mad.dtype != np.float32:
        return [f"row statistics: shapes {med.shape} {mad.shape} {nz.shape}"]
    found = _bad_rows("n_zero", nz != (x == 0.0).sum(axis=1), slab)
    sample = stats_sample(slab)
    bad_m, bad_d = np.zeros(rows, bool), np.zeros(rows, bool)
    for r in sample:
        m, d = _median_mad(x[r][x[r] != 0] if skip_zeros else x[r])
        bad_m[r] = not np.array_equal(med[r], m, equal_nan=True)
        bad_d[r] = not np.array_equal(mad[r], d, equal_nan=True)
    return found + _bad_rows("median", bad_m, slab) + _bad_rows("MAD", bad_d, slab)


# ----------------------------------------------------------------------- row kurtosis ---
ROWKURT_SHAPE = (65_538, 40)
ROWKURT_CONSTANT = (65_530, 65_536)


def rowkurt_rows():
    rows, n = ROWKURT_SHAPE
    ids = np.arange(rows)
    scale, offset = row_scale_offset(ids, seed=7)
    x = (row_noise(ids, n, seed=7) * scale[:, None] + offset[:, None]).astype(np.float32)
    for r in ROWKURT_CONSTANT:
        x[r] = x[r, 0]
    return x


def rowkurt_sample(slab=ROW_LIMIT):
    return sampled_rows(ROWKURT_SHAPE[0], [slab], seed=71, extra=ROWKURT_CONSTANT)


def rowkurt_definition(x, mean_from=None):
    """postprocess.excess_kurtosis_f32 of every row: the moments by row reductions (NumPy sums a row of a C-ordered
    matrix as it sums the row alone), the last expression on scalars as SciPy evaluates it on one series.
    `mean_from`: row index per row whose mean to subtract instead of the row's own -- the planted defect."""
    from seismic_bpmf_amd.postprocess import kurtosis_from_moments_rows
    x = np.ascontiguousarray(x, dtype=np.float32)
    mean = np.mean(x, axis=1, keepdims=True)
    if mean_from is not None:
        mean = mean[mean_from]
    with np.errstate(all="ignore"):
        s2 = (x - mean) ** 2
        parts = np.stack([mean[:, 0], np.mean(s2, axis=1), np.mean(s2 ** 2, axis=1)], axis=1)
    return kurtosis_from_moments_rows(parts)


def check_row_kurtosis(out, x, slab):
    """scipy.stats.kurtosis one series at a time on the sampled rows, bit for bit (NaN for a constant row)."""
    from scipy.stats import kurtosis
    out = np.asarray(out)
    if out.shape != (x.shape[0],) or out.dtype != np.float32:
        return [f"row kurtosis: {out.dtype} {out.shape}"]
    import warnings
    bad = np.zeros(x.shape[0], bool)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (SciPy warns about the constant rows)
        for r in rowkurt_sample(slab):
            bad[r] = not np.array_equal(out[r], np.float32(kurtosis(x[r])), equal_nan=True)
    return _bad_rows("row kurtosis", bad, slab)


# ---------------------------------------------------------------------- MAD threshold ---
MAD_ROWS = 7
MAD_CASES = ((9_000, 4500, 0.5), (25_001, 1001, 0.25))          # (n, W, overlap)
MAD_SLABS = (1, 2, 3, 7)                                         # 7 x 1, 2 + 2 + 2 + 1, 3 + 3 + 1, 1 x 7
MAD_NUM_DEV = 8.0
MAD_ROW_CAP = np.array([10.0, 10.0, 0.3, 10.0, 10.0, 10.0, 10.0], np.float32)


def mad_rows(n):
    """7 rows as in test_mad_threshold_batched_rows_and_candidates: rows with different numbers of zeros sharing one
    noise vector, a row without zeros, zeros only at the ends, ties; peaks above the threshold.  Returns (x, noise)."""
    scale = np.array([0.09, 0.07, 0.06, 0.04, 0.05, 0.03, 0.02])
    offset = np.array([0.0, 0.03, -0.02, 0.04, 0.0, -0.03, 0.02])  # (its own centre and deviation for every row)
    z = row_noise(np.arange(MAD_ROWS + 2), n, seed=n)
    x = (z[:MAD_ROWS] * scale[:, None] + offset[:, None]).astype(np.float32)
    x[0, np.abs(z[MAD_ROWS]) < 0.06] = 0.0                       # ~5 % zeros, scattered
    x[1, :700] = 0.0
    x[1, -900:] = 0.0                                            # zeros only at the ends
    x[3, 5000:5600] = 0.0
    x[4] = np.round(x[4] * 50) / 50                              # ties (and the zeros rounding makes)
    x[6, 100:117] = 0.0
    x[:, ::977] += np.float32(0.6)                               # (row 2, 5: no zeros)
    return x, z[MAD_ROWS + 1].astype(np.float32)


def mad_shift(W, overlap):
    return int((1.0 - overlap) * W)


def mad_limit(per_row, slab):
    """The ThresholdGPU.mad_workspace_limit that makes it take `slab` rows per call; per_row =
    bpmf_tdt_mad_workspace_bytes(64, n, W, shift) // 64, as the wrapper computes it."""
    return int(per_row) * int(slab)


def mad_windows_definition(x, W, n_dev, overlap, white_noise, centre_dev=None):
    """BPMF/similarity_search.py:1079-1113 up to the window values (postprocess.time_dependent_threshold_mad's lines,
    which return the expanded series only).  `centre_dev`: (centre0, dev0) to fill the zeros with instead of the
    row's own -- the planted defect."""
    x = np.array(x, copy=True)
    shift = mad_shift(W, overlap)
    zeros = x == 0.0
    n_zeros = int(zeros.sum())
    centre0 = np.median(x[~zeros])
    dev0 = np.median(np.abs(x[~zeros] - centre0))
    if centre_dev is not None:
        centre0, dev0 = centre_dev
    x[zeros] = white_noise[:n_zeros] * dev0 + centre0
    wins = np.lib.stride_tricks.sliding_window_view(x, W)[::shift, :]
    centre = np.median(wins, axis=-1)
    dev = np.median(np.abs(wins - centre[:, None]), axis=-1)
    thr = centre + n_dev * dev
    thr[1:] = np.maximum(thr[:-1], thr[1:])
    thr[:-1] = np.maximum(thr[:-1], thr[1:])
    return thr, (centre0, dev0)


def mad_expand(thr, n, W, overlap):
    half, shift = W // 2, mad_shift(W, overlap)
    where = np.arange(half, n - (W - half)) // shift
    where[where >= thr.size] = thr.size - 1
    mid = thr[where]
    return np.hstack((mid[0] * np.ones(half, dtype=np.float32), mid, mid[-1] * np.ones(W - half, dtype=np.float32)))


def mad_definition(x, W, overlap, white_noise, stats_from=None):
    """(thr_windows (rows, n_win), full (rows, n)) of the host definition, row by row."""
    own = [mad_windows_definition(r, W, MAD_NUM_DEV, overlap, white_noise)[1] for r in x]
    wins, full = [], []
    for i, r in enumerate(x):
        cd = own[stats_from[i]] if stats_from is not None else None
        thr, _ = mad_windows_definition(r, W, MAD_NUM_DEV, overlap, white_noise, centre_dev=cd)
        wins.append(thr)
        full.append(mad_expand(thr, r.size, W, overlap))
    return np.stack(wins).astype(np.float32), np.stack(full).astype(np.float32)


def check_mad_threshold(thr_win, full, x, white_noise, W, overlap, slab):
    """Window values and expanded threshold equal postprocess.time_dependent_threshold_mad row by row, bit for bit
    (the window values through the same lines, mad_windows_definition)."""
    from seismic_bpmf_amd import postprocess as pp
    thr_win, full = np.asarray(thr_win), np.asarray(full)
    rows, n = x.shape
    if full.shape != (rows, n) or thr_win.ndim != 2 or thr_win.shape[0] != rows or full.dtype != np.float32:
        return [f"MAD threshold: shapes {thr_win.shape} {full.shape}"]
    bad_w, bad_f = np.zeros(rows, bool), np.zeros(rows, bool)
    for r in range(rows):
        want = pp.time_dependent_threshold_mad(x[r], W, MAD_NUM_DEV, overlap=overlap, white_noise=white_noise)
        wins, _ = mad_windows_definition(x[r], W, MAD_NUM_DEV, overlap, white_noise)
        assert np.array_equal(mad_expand(wins, n, W, overlap), want)        # (the two restatements agree)
        bad_f[r] = not np.array_equal(full[r], want)
        bad_w[r] = thr_win.shape[1] != wins.size or not np.array_equal(thr_win[r], wins.astype(np.float32))
    return _bad_rows("thr_windows", bad_w, slab) + _bad_rows("expanded threshold", bad_f, slab)


def check_mad_candidates(cand, x, full, slab):
    """extract_candidates(kind="mad", row_cap=MAD_ROW_CAP): every sample above min(threshold, cap), as the existing
    test compares them."""
    bad = np.zeros(x.shape[0], bool)
    for r in range(x.shape[0]):
        t_r = np.minimum(full[r], MAD_ROW_CAP[r])
        idx = np.flatnonzero(x[r] > t_r)
        mine = cand[cand["row"] == r]
        bad[r] = not (np.array_equal(mine["index"], idx) and np.array_equal(mine["threshold"], t_r[idx])
                      and np.array_equal(mine["cc"], x[r, idx]))
    return _bad_rows("candidates", bad, slab)


# ------------------------------------------------------------------- running kurtosis ---
KURT_W_MAX = 32_768                         # the limit include/bpmf_hip.h states
KURT_CEILING_W = (16_128, 16_129, 32_768)   # (W + 256) * 4 bytes of LDS: 65 536, 65 540 -- the first above 64 KB -- and 132 096
KURT_MANY_SHAPE = (21_846, 3, 40)
KURT_MANY_W = 5


def kurt_ceiling_signal(W, length=None):
    """(1, 2, W + 300) float32 with channel scales 1 and 30 and a flat stretch longer than W in channel 0 (outputs
    whose whole window is flat keep the caller's zeros); `length`: the first samples only."""
    n = W + 300
    x = row_noise(np.arange(2), n, seed=W) * np.array([1.0, 30.0])[:, None]
    x[0, 10:W + 60] = 0.5
    return x.astype(np.float32).reshape(1, 2, n)[..., :length].copy()


def kurt_many_signal():
    S, C, n = KURT_MANY_SHAPE
    ids = np.arange(S * C)
    scale, offset = row_scale_offset(ids, seed=9)
    return (row_noise(ids, n, seed=9) * scale[:, None] + offset[:, None]).astype(np.float32).reshape(S, C, n)


def running_kurtosis_definition(signal, W):
    from oracle import oracle
    return oracle.kurtosis(np.ascontiguousarray(signal, dtype=np.float32), int(W))


def plant_first_sample_zero(want, W, slab):
    """The first output sample (n = W) of the first row of every slab left zero."""
    out = np.array(want, copy=True)
    flat = out.reshape(-1, out.shape[-1])
    for r0 in range(0, flat.shape[0], int(slab)):
        flat[r0, W] = 0.0
    return out


def check_running_kurtosis(out, signal, W, slab):
    """The oracle's running kurtosis (oracle/adjacent_oracle.c, the reference's loop) on every channel, bit for bit."""
    out, signal = np.asarray(out), np.asarray(signal)
    if out.dtype != np.float32 or out.shape != signal.shape:
        return [f"running kurtosis: {out.dtype} {out.shape}"]
    want = running_kurtosis_definition(signal, W)
    n = signal.shape[-1]
    out = np.ascontiguousarray(out)
    same = (out.view(np.uint32) == want.view(np.uint32)) | ((out != out) & (want != want))
    return _bad_rows("running kurtosis", ~same.reshape(-1, n).all(axis=1), slab)
