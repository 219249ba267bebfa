"""The cases of the detection stage behind the beamformer (csrc/bp_detect.hip, threshold.BeamDetectorGPU,
workflow.beam_detections_device), shared by tests/test_bp_detect_host.py on the CPU and tests/test_gpu_bp_detect.py on
the device (TEST INFRASTRUCTURE, pure NumPy).

THE RULE (DESIGN.md s4 "Non-finite features", rule 3): postprocess.find_beam_detections on the downloaded series is the
definition of beam_detections_device, for every float32 series, +-Inf included, and every form of the threshold.

Every case is (name, beam float32, sources int32, threshold spec, mpd); a threshold spec is
    ("scalar", value)  |  ("array", (n,) values)  |  ("nodes", window, overlap, n_dev).
The series are short: the kernels go wrong where a wave (64), a block (256 threads of the extraction, 1024 of the window
statistics), the unrolled element loop (8 x 1024) or a window ends, not at the length of a day.

`StandIn` is the device half in NumPy (np.median and the extraction rule), `stage` the whole stage restated on top of
it; both take `defect`, one of DEFECTS, a way of getting it wrong.  `census` names the classes of CLASSES a case meets:
test_bp_detect_host.py demands every class from some case, every defect caught by some case, and no case in the one
class of input that stays outside the contract (`excluded`): a NaN and two neighbouring equal infinities in one series,
where the reference's answer at the infinities depends on whether a NaN exists anywhere.
"""
import functools
import warnings

import numpy as np

INF, NAN = np.float32(np.inf), np.float32(np.nan)
F32 = np.float32

peak_dtype = np.dtype([("index", np.int32), ("beam", np.float32), ("source", np.int32), ("pad", np.int32)])

SEAM_N = (0, 1, 2, 3, 4, 63, 64, 65, 66, 255, 256, 257, 258, 511, 512, 513, 514)
STAT_WINDOWS = (1, 2, 3, 1023, 1024, 1025, 8191, 8192, 8193)

DEFECTS_DEVICE = ("values_compared",        # x1 > x0 && x2 <= x1 on the values: the first +Inf of a run is a peak
                  "right_less",             # `<` for `<=` on the right neighbour: no flat top is a peak
                  "floor_greater_equal",    # `>=` for `>` at the floor
                  "first_left_out",         # t = 1 never looked at
                  "last_left_out",          # t = n - 2 never looked at
                  "arrival_order",          # the records as they arrive (wave by wave, last wave first), not sorted
                  "even_lo_only")           # the median of an even window is its lower middle value
DEFECTS_HOST = ("floor_no_ulp",             # the smallest node as the floor, without its float32 step down
                "no_tie_fallback",          # equal peaks closer than mpd ranked on the list above the floor
                "tie_test_strict",          # the tie test with `<` for `<= mpd`
                "clamped_window_read_as_cut",   # see stage(): what the guard of beam_slice is there to prevent
                "neg_inf_floor_blocks")     # a -Inf floor treated as "nothing passes"
DEFECTS = DEFECTS_DEVICE + DEFECTS_HOST


# ----------------------------------------------------------------------------------------- the device half ---
def bp_window_plan(n, window, overlap):
    from seismic_bpmf_amd.threshold import bp_window_plan as plan
    return plan(n, window, overlap)


def f32_key(a):
    """The order-preserving key of the radix select (csrc/select.h)."""
    u = np.asarray(a, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def same_bits(a, b):
    """float32 arrays equal bit for bit -- the sign of a zero counts -- with NaN equal to NaN (the payload and the sign
    of a NaN carry nothing: Inf - Inf has one sign on the host and the other on the device)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _quiet():
    ctx = warnings.catch_warnings()
    ctx.__enter__()
    warnings.simplefilter("ignore")
    return ctx


def median_f32(seg, lo_only=False):
    """np.median of a float32 window (NaN for an empty one), float32."""
    seg = np.asarray(seg, np.float32)
    ctx = _quiet()
    try:
        with np.errstate(all="ignore"):
            if lo_only and seg.size and seg.size % 2 == 0 and not np.isnan(seg).any():
                return np.sort(seg)[seg.size // 2 - 1]
            return np.float32(np.median(seg)) if seg.size else NAN
    finally:
        ctx.__exit__(None, None, None)


def extract_rule(x, floor, defect=None):
    """Sample indices, ascending, of the rising-edge local maxima above `floor`: the reference's differences in float64
    (dx > 0 on the left, dx <= 0 on the right), t = 1 .. n - 2."""
    x = np.asarray(x, np.float32)
    n = x.size
    if n < 3:
        return np.zeros(0, np.int64)
    v = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if defect == "values_compared":
            left, right = v[1:-1] > v[:-2], v[2:] <= v[1:-1]
        else:
            d = v[1:] - v[:-1]
            left, right = d[:-1] > 0, (d[1:] < 0 if defect == "right_less" else d[1:] <= 0)
        above = v[1:-1] >= floor if defect == "floor_greater_equal" else v[1:-1] > floor
    hit = left & right & above
    if defect == "first_left_out":
        hit[0] = False
    if defect == "last_left_out":
        hit[-1] = False
    return np.flatnonzero(hit).astype(np.int64) + 1


class StandIn:
    """What workflow.beam_detections_device asks of a threshold.BeamDetectorGPU, in NumPy on CPU tensors or arrays."""

    def __init__(self, defect=None):
        self.defect = defect
        self.calls = []

    @staticmethod
    def _np(a):
        return None if a is None else np.asarray(a.cpu() if hasattr(a, "cpu") else a).reshape(-1)

    def window_stats(self, beam, window, overlap=0.75):
        x = self._np(beam).astype(np.float32)
        n = x.size
        window, shift, nw = bp_window_plan(n, window, overlap)
        med, mad = np.zeros(nw + 2, np.float32), np.zeros(nw + 2, np.float32)
        lo_only = self.defect == "even_lo_only"
        with np.errstate(all="ignore"):
            for q in range(1, nw + 1):
                seg = x[q * shift:min(n, q * shift + window)]
                med[q] = median_f32(seg, lo_only)
                mad[q] = median_f32(np.abs(seg - med[q]), lo_only)
        self.calls.append(("window_stats", window, overlap))
        return med, mad

    def extract_peaks(self, beam, sources, floor):
        x = self._np(beam).astype(np.float32)
        src = self._np(sources)
        idx = extract_rule(x, float(floor), self.defect)
        if self.defect == "arrival_order":
            idx = np.concatenate([idx[idx // 64 == w] for w in np.unique(idx // 64)[::-1]]) if idx.size else idx
        rec = np.zeros(idx.size, peak_dtype)
        rec["index"], rec["beam"] = idx, x[idx]
        rec["source"] = src[idx] if src is not None else 0
        self.calls.append(("extract_peaks", float(floor)))
        return rec


# ------------------------------------------------------------------------------- the whole stage, restated ---
def suppress(ind, rank, mpd):
    """The tallest-first +-mpd suppression on ascending positions, as the library's host routine walks it (the
    neighbours of every kept peak): the stand-in for postprocess._suppress where the library is not built."""
    ind, rank = np.asarray(ind, np.int64), np.asarray(rank, np.int64)
    keep = np.ones(ind.size, bool)
    for i in rank:
        if not keep[i]:
            continue
        j = i - 1
        while j >= 0 and ind[j] >= ind[i] - mpd:
            keep[j] = False
            j -= 1
        j = i + 1
        while j < ind.size and ind[j] <= ind[i] + mpd:
            keep[j] = False
            j += 1
    return keep


def close_ties(index, height, mpd, strict=False):
    index, height = np.asarray(index, np.int64), np.asarray(height)
    for a in range(index.size):
        for b in range(a + 1, index.size):
            gap = abs(int(index[b]) - int(index[a]))
            if height[a] == height[b] and (gap < mpd if strict else gap <= mpd):
                return True
    return False


def stage(beam, sources, spec, mpd, defect=None):
    """beam_detections_device restated: (peaks, sources).  The threshold floor, the tie fallback, the suppression on the
    list, the float64 threshold test, the gathered windows and the snap; `defect` plants one of DEFECTS.

    "clamped_window_read_as_cut": the windows around the candidates are gathered at positions CLAMPED to the series, so
    that entry k of the window of candidate c is beam[c - half + k] wherever that sample exists, and a slice [i0, i1) of
    the series is read at offset i0 - (c - half).  The guard of beam_slice (`lo >= 0 and c + half < n`) sends the windows
    that touch an end to the download instead.  With clamped positions that guard protects nothing -- removing it
    alone changes no result, which is why it is not the planted defect; what it is there to prevent is reading such a
    window as if it had been CUT at the ends (its first entry sample max(0, c - half)), and that is planted."""
    from seismic_bpmf_amd import postprocess as pp
    x = np.asarray(beam, np.float32)
    src = np.asarray(sources, np.int32)
    n = x.size
    det = StandIn(defect if defect in DEFECTS_DEVICE else None)
    none = np.zeros(0, np.int64), np.zeros(0, np.int32)
    if spec[0] == "nodes":
        _, window, overlap, n_dev = spec
        med, mad = det.window_stats(x, window, overlap)
        with np.errstate(all="ignore"):
            centre, thr = pp.bp_threshold_nodes(n, int(window), overlap, med, mad, n_dev)
        real = thr[~np.isnan(thr)]
        floor = float("nan")
        if real.size:
            floor = float(real.min()) if defect == "floor_no_ulp" else float(np.nextafter(F32(real.min()), -INF))

        def threshold_at(s):
            with np.errstate(all="ignore"):
                return pp.interp_threshold(s, centre, thr)
    elif spec[0] == "scalar":
        floor = float(spec[1])

        def threshold_at(s):
            return np.full(len(s), float(spec[1]))
    else:
        arr = np.asarray(spec[1])
        real = arr[~np.isnan(arr)]
        floor = float(real.min()) if real.size else float("nan")

        def threshold_at(s):
            return arr[s]
    if np.isnan(floor) or floor == np.inf or (defect == "neg_inf_floor_blocks" and floor == -np.inf):
        return none
    rec = det.extract_peaks(x, src, floor)
    if mpd > 1 and defect != "no_tie_fallback" and close_ties(rec["index"], rec["beam"], mpd, defect == "tie_test_strict"):
        rec = det.extract_peaks(x, src, -np.inf)
    index, height = rec["index"].astype(np.int64), rec["beam"].astype(np.float64)
    if index.size and mpd > 1:
        keep = suppress(index, pp._tallest_first(height), mpd)
        index, height = index[keep], height[keep]
    with np.errstate(invalid="ignore"):
        cand = index[height > np.asarray(threshold_at(index), np.float64)]
    half = int(mpd) + 1
    windows = {int(c): x[np.clip(np.arange(c - half, c + half + 1), 0, n - 1)] for c in cand}

    def beam_slice(i0, i1):
        for c in sorted(windows):
            if i1 - 1 - half <= c <= i0 + half:
                lo = c - half
                if defect == "clamped_window_read_as_cut":
                    lo = max(0, lo)
                    return windows[c][i0 - lo:i1 - lo]
                if lo >= 0 and c + half < n:
                    return windows[c][i0 - lo:i1 - lo]
        return x[i0:i1]

    peaks = pp.snap_and_merge_peaks(cand, n, mpd, beam_slice)
    return peaks, src[peaks]


# -------------------------------------------------------------------------------------------- definition ---
def threshold_series(beam, spec):
    """The (n,) threshold of the definition (a scalar stays a scalar)."""
    from seismic_bpmf_amd import postprocess as pp
    if spec[0] == "nodes":
        ctx = _quiet()
        try:
            with np.errstate(all="ignore"):
                return pp.bp_time_dependent_threshold(np.asarray(beam, np.float32), int(spec[1]), spec[3], overlap=spec[2])
        finally:
            ctx.__exit__(None, None, None)
    return spec[1]


def definition(case):
    """postprocess.find_beam_detections on the series: (peaks, sources)."""
    from seismic_bpmf_amd import postprocess as pp
    name, beam, sources, spec, mpd = case
    with np.errstate(invalid="ignore"):
        peaks, src = pp.find_beam_detections(beam, sources, threshold_series(beam, spec), mpd)
    return np.asarray(peaks, np.int64), np.asarray(src, np.int32)


def excluded(beam):
    """The one class of input outside the contract: a NaN and two neighbouring equal infinities in one series."""
    x = np.asarray(beam, np.float32)
    return bool(np.isnan(x).any() and (np.isinf(x[1:]) & (x[1:] == x[:-1])).any())


# ------------------------------------------------------------------------------------------------- cases ---
def _sources(n, seed):
    return np.random.default_rng(1000 + seed).integers(0, 50_000, n).astype(np.int32)


def _case(cases, name, beam, spec, mpd):
    beam = np.asarray(beam, np.float32)
    if spec[0] == "array":
        spec = ("array", np.asarray(spec[1], np.float32))
        spec[1].setflags(write=False)
    src = _sources(beam.size, len(cases))
    beam.setflags(write=False)
    src.setflags(write=False)
    assert name not in [c[0] for c in cases], name
    cases.append((name, beam, src, spec, int(mpd)))


def _planted(n, peaks, first=0.0, last=0.0):
    x = np.zeros(n, np.float32)
    for p in peaks:
        if 0 <= p < n:
            x[p] = 2.0 + (p % 7)
    if n >= 1:
        x[0] = first
    if n >= 2:
        x[n - 1] = last
    return x


TABLE = ([1, INF, INF, 1, 0, 3, 1], [1, INF, INF, INF, 1, 0, 3, 1], [0, 1, INF, INF, 2, 3, 1], [1, 2, INF, 1, 0, 3, 1])


@functools.lru_cache(maxsize=None)
def named_cases():
    cases = []
    add = functools.partial(_case, cases)
    S = ("scalar", 0.5)
    # ---- extraction seams: the lengths around a wave, a block, two blocks ----
    for n in SEAM_N:
        # peaks at t = 1, t = n - 2 and every t = 63, 255 (mod 256)
        at = []
        for t in [1, n - 2] + [t for t in range(1, n - 1) if t % 256 in (63, 255)]:
            if 1 <= t <= n - 2 and not {t - 1, t, t + 1} & set(at):
                at.append(t)
        add(f"n{n}_edges", _planted(n, at), S, 1)
        # peaks at every t = 64, 0 (mod 256), maxima at t = 0 and t = n - 1 that do not count
        at = {t for t in range(2, n - 2) if t % 256 in (64, 0)}
        add(f"n{n}_ends", _planted(n, sorted(at), first=9.0, last=9.5), S, 2)
        # the densest series: every odd sample a peak (ties among them: the fallback at mpd 3)
        x = np.zeros(n, np.float32)
        x[1::2] = 1.0 + (np.arange(1, n, 2) % 5)
        add(f"n{n}_dense", x, S, 3)
    n = 300
    add("constant", np.full(n, 2.0), S, 1)
    add("rising", np.arange(n), S, 1)
    add("falling", np.arange(n)[::-1], S, 2)
    # ---- flat tops: 2, 3, 64 (over a wave), 65 (over a wave), 300 (over two blocks), one followed by a rise, one
    # that runs into the end of the series ----
    x = np.zeros(1100, np.float32)
    for start, length, value in ((10, 2, 3.0), (20, 3, 4.0), (40, 64, 5.0), (130, 65, 6.0), (230, 300, 7.0)):
        x[start:start + length] = value
    x[600:603], x[603] = 3.0, 5.0
    x[1090:] = 4.0
    add("flat_tops", x, S, 1)
    add("flat_tops_mpd40", x, S, 40)
    # ---- the floor: a peak exactly at it, one float32 step above and below; a float64 floor between two float32 ----
    f = F32(1.5)
    x = np.zeros(24, np.float32)
    x[3], x[8], x[13], x[18] = f, np.nextafter(f, INF), np.nextafter(f, -INF), 2.0
    add("at_the_floor", x, ("scalar", 1.5), 1)
    x = np.zeros(16, np.float32)
    x[3], x[8] = F32(0.1), np.nextafter(F32(0.1), -INF)           # float32(0.1) > 0.1 > the float32 below it
    add("floor_between_float32", x, ("scalar", 0.1), 1)
    # ---- infinities ----
    for j, series in enumerate(TABLE):
        add(f"table_{j + 1}", series, S, 1)
        add(f"table_{j + 1}_mpd2", series, S, 2)
    add("inf_isolated", [0, 1, INF, 1, 0, 2, 1, 0], S, 1)
    x = np.zeros(200, np.float32)
    x[10], x[40], x[150], x[180] = 3.0, 4.0, 5.0, 2.0
    x[60:130] = INF                                               # a run of 70 over two wave seams, then lower
    add("inf_run_70", x, S, 1)
    add("inf_run_70_mpd30", x, S, 30)
    add("inf_run_then_rise", [0, 1, INF, INF, INF, 2, 3, 4, 1, 0, INF, INF, 1, 0], S, 1)
    add("inf_at_0", [INF, 1, 2, 1, 0, 3, 0], S, 1)
    add("inf_at_1", [0, INF, 1, 2, 1, 0], S, 1)
    add("inf_at_n-2", [1, 2, 1, 0, INF, 0], S, 1)
    add("inf_at_n-1", [1, 2, 1, 0, 3, 1, INF], S, 1)
    add("inf_at_every_end", [INF, INF, 1, 2, 1, 0, INF, INF], S, 2)
    add("neg_inf_sample_and_gap", [1, 2, -INF, 3, 1, -INF, -INF, -INF, 2, 4, 1, -INF, 0], S, 1)
    add("neg_inf_everywhere", [-INF] * 9, ("scalar", -np.inf), 1)
    add("inf_next_to_neg_inf", [1, -INF, INF, -INF, 2, 1, 0, INF, -INF, 1, 0, -INF, INF, 1], S, 1)
    for gap, tag in ((3, "closer_than_mpd"), (5, "mpd_apart"), (6, "mpd_plus_1_apart")):
        x = np.zeros(30, np.float32)
        x[4], x[10], x[10 + gap], x[24] = 2.0, INF, INF, 3.0
        add(f"two_inf_{tag}", x, S, 5)
    x = np.zeros(40, np.float32)
    x[20], x[21], x[22:24], x[30] = 5.0, 1.0, INF, 2.0            # the snap (+-4) moves the peak at 20 onto the run
    add("finite_peak_next_to_inf_run", x, S, 8)
    # ---- NaN (hand-made input: the library's max-beam never holds one) ----
    add("nan_at_0", [NAN, 1, 3, 1, 0, 2, 0], S, 1)
    add("nan_at_1", [0, NAN, 3, 1, 0, 2, 0], S, 1)
    add("nan_at_n-2", [0, 2, 0, 1, 3, NAN, 0], S, 1)
    add("nan_at_n-1", [0, 2, 0, 1, 3, 1, NAN], S, 3)
    add("nan_next_to_peaks", [0, 1, 4, NAN, 0, 2, 0, NAN, 5, 1, 0, 3, 0, INF, 0, NAN, 0], S, 1)
    add("nan_next_to_peaks_mpd4", [0, 1, 4, NAN, 0, 2, 0, NAN, 5, 1, 0, 3, 0, INF, 0, NAN, 0, 2, 1, 0], S, 4)
    add("nan_runs", [0, 3, 1, NAN, NAN, 2, 4, 1, NAN, NAN, NAN, 5, 0, 2, 0], S, 2)
    add("all_nan", [NAN] * 10, S, 1)
    # ---- threshold forms on one small series ----
    rng = np.random.default_rng(20261021)
    x = np.round(np.abs(rng.standard_normal(60)) * 3.0).astype(np.float32)
    x[17], x[41] = INF, 9.0
    for tag, value in (("pos_inf", np.inf), ("neg_inf", -np.inf), ("nan", np.nan), ("finite", 2.0)):
        add(f"scalar_{tag}", x, ("scalar", value), 1)
        add(f"scalar_{tag}_mpd4", x, ("scalar", value), 4)
    thr = np.full(60, 2.0, np.float32)
    peaks = extract_rule(x, 2.0)
    for tag, value in (("nan", NAN), ("pos_inf", INF), ("neg_inf", -INF)):
        t = thr.copy()
        t[peaks[::2]] = value
        add(f"array_with_{tag}", x, ("array", t), 1)
        add(f"array_with_{tag}_mpd4", x, ("array", t), 4)
    add("array_all_neg_inf", x, ("array", np.full(60, -INF)), 1)
    add("array_all_neg_inf_mpd4", x, ("array", np.full(60, -INF)), 4)
    add("array_all_nan", x, ("array", np.full(60, NAN)), 2)
    # ---- mpd and the gathered windows ----
    x = rng.integers(0, 10, 50).astype(np.float32)                # ties; peaks right at both ends
    x[:4], x[-4:] = (0, 9, 1, 8), (8, 1, 9, 0)
    for mpd in (1, 2, 3, 6, 7, 50, 80):
        add(f"ties_mpd{mpd}", x, ("scalar", 2.5), mpd)
    for mpd in (4, 5):
        x = np.zeros(60, np.float32)
        x[10], x[10 + mpd], x[30], x[30 + mpd + 1], x[50] = 5.0, 5.0, 6.0, 6.0, 3.0
        add(f"equal_peaks_mpd{mpd}", x, S, mpd)
    # chains of equal peaks exactly mpd apart above the floor, among many lower maxima with ties: which of a chain
    # survive depends on where the sort puts the equal heights in the list of ALL local maxima -- the tie fallback
    # must see that a gap of exactly mpd counts (several series: the order of equal heights is the sort's business)
    for k in range(6):
        r = np.random.default_rng(500 + k)
        x = np.zeros(400, np.float32)
        x[1::2] = r.integers(1, 4, 200)
        for start, links in ((100, 3), (200, 4), (301, 5)):
            for p in range(start, start + 6 * links, 6):
                x[p - 1:p + 2] = (0.0, 7.0, 0.0)
        add(f"tie_chain_{k}", x, ("scalar", 4.5), 6)
    # ---- window statistics: the window lengths around a block and the unrolled loop; cut last windows ----
    def noise(n, seed, spikes=6):
        r = np.random.default_rng(seed)
        y = np.abs(r.standard_normal(n)).astype(np.float32)
        for p in r.integers(2, max(3, n - 2), spikes):
            y[p] += np.float32(r.uniform(8, 30))
        return y

    add("w1", noise(7, 1, 2), ("nodes", 1, 0.0, 3.0), 1)
    add("w2", noise(9, 2, 2), ("nodes", 2, 0.5, 3.0), 1)
    add("w3", noise(11, 3, 2), ("nodes", 3, 0.5, 3.0), 2)
    for w in STAT_WINDOWS[3:]:
        add(f"w{w}", noise(2 * w + 300, w), ("nodes", w, 0.75, 6.0), 25)
    add("w1024_last_cut_to_1", noise(2 * 1024 + 1, 11), ("nodes", 1024, 0.0, 6.0), 10)
    add("w1025_last_cut_to_2", noise(2 * 1025 + 2, 12), ("nodes", 1025, 0.0, 6.0), 10)
    add("w8192_last_cut_to_1", noise(2 * 8192 + 1, 13), ("nodes", 8192, 0.0, 6.0), 50)
    add("window_is_n", noise(1100, 14), ("nodes", 1100, 0.75, 6.0), 10)
    add("window_is_n-1", noise(1100, 15), ("nodes", 1099, 0.75, 6.0), 10)
    add("rounded_ties", np.round(noise(3000, 16, 10), 1), ("nodes", 1000, 0.9, 4.0), 7)
    # ---- windows designed one by one: 64 samples each, no overlap (window 0 belongs to no node) ----
    w = 64
    r = np.random.default_rng(77)
    blocks = {
        "unused": np.abs(r.standard_normal(w)),
        "half 1 half 1e10": r.permutation(np.r_[np.full(w // 2, 1.0), np.full(w // 2, 1e10)]),
        "half -1 half +1": r.permutation(np.r_[np.full(w // 2, -1.0), np.full(w // 2, 1.0)]),
        "zeros in the middle": r.permutation(np.r_[np.full(w // 2 - 1, -2.0), [-0.0, 0.0], np.full(w // 2 - 1, 3.0)]),
        "all -0.0": np.full(w, -0.0),
        "constant": np.full(w, 2.5),
        "heavy ties": r.choice([1.0, 2.0, 3.0, 4.0], w),
        "second level": r.permutation(np.r_[np.full(w // 2, 1.0), np.full(w // 2, 1.0005)]),
        "minority inf": r.permutation(np.r_[np.abs(r.standard_normal(w - 15)), np.full(10, np.inf), np.full(5, -np.inf)]),
        "inf both sides": r.permutation(np.r_[r.uniform(1, 2, w // 2), np.full(w // 4, np.inf), np.full(w // 4, -np.inf)]),
        "half +inf": r.permutation(np.r_[r.uniform(1, 2, w // 2), np.full(w // 2, np.inf)]),
        "majority +inf": r.permutation(np.r_[r.uniform(1, 2, 20), np.full(w - 20, np.inf)]),
        "all -inf": np.full(w, -np.inf),
        "plain": np.abs(r.standard_normal(w)),
        "plain with peaks": np.abs(r.standard_normal(w)) + 40.0 * (np.arange(w) % 16 == 7),
        "tail": np.abs(r.standard_normal(9)) + 30.0 * (np.arange(9) == 4),
    }
    add("designed_windows", np.concatenate(list(blocks.values())), ("nodes", w, 0.0, 5.0), 3)
    odd = np.concatenate([np.abs(r.standard_normal(63)), r.permutation(np.r_[np.full(31, -1.0), [-0.0], np.full(31, 2.0)]),
                          r.permutation(np.r_[np.full(33, np.inf), r.uniform(0, 1, 30)]), np.abs(r.standard_normal(70))])
    add("designed_odd_windows", odd, ("nodes", 63, 0.0, 5.0), 2)
    # ---- nodes: all NaN; one NaN among finite ones; two equal nodes with peaks of exactly their height between ----
    x = noise(48, 21, 3)
    x[::4] = NAN
    add("nodes_all_nan", x, ("nodes", 8, 0.5, 3.0), 2)
    x = noise(400, 22, 12)
    x[150] = NAN
    add("nodes_one_nan", x, ("nodes", 40, 0.5, 3.0), 5)
    # period 6, windows of 12 every 6 samples: every window holds {0 0 1 1 1 1 2 2 2 2 4 4}: median 1.5, MAD 0.5, and
    # with n_dev 5 every node is 4.0 -- the height of the peaks; between two centres 6 apart the interpolation weights
    # are multiples of fl(1/6) and do not always add up to 1
    x = np.tile(np.array([1, 2, 4, 2, 1, 0], np.float32), 20)
    add("peaks_as_high_as_equal_nodes", x, ("nodes", 12, 0.5, 5.0), 1)
    add("peaks_as_high_as_equal_nodes_mpd4", x, ("nodes", 12, 0.5, 5.0), 4)
    return tuple(cases)


def extraction_cases():
    """The cases whose threshold is a scalar: the floor of the extraction is that scalar, no window is involved."""
    return tuple(c for c in named_cases() if c[3][0] == "scalar")


def statistics_cases():
    return tuple(c for c in named_cases() if c[3][0] == "nodes")


# ------------------------------------------------------------------------------------------------ census ---
def _runs(mask):
    """[(start, stop)] of the maximal runs of True."""
    m = np.r_[False, np.asarray(mask, bool), False]
    d = np.flatnonzero(m[1:] != m[:-1])
    return list(zip(d[::2], d[1::2]))


def _flat_runs(x):
    """[(start, stop)] of the maximal runs of equal values at least 2 long."""
    if x.size < 2:
        return []
    with np.errstate(invalid="ignore"):
        return [(a, b + 1) for a, b in _runs(x[1:] == x[:-1])]


CLASSES = tuple(
    [f"n = {n}" for n in SEAM_N]
    + ["peak at t = 1", "peak at t = n - 2"]
    + [f"a peak at every t = {r} (mod 256)" for r in (63, 64, 0, 255)]
    + ["maximum at t = 0 does not count", "maximum at t = n - 1 does not count", "every odd sample a peak",
       "constant", "rising", "falling"]
    + [f"flat top of {k}" for k in (2, 3, 64, 65, 300)]
    + ["flat top over a wave seam", "flat top over a block seam", "flat top followed by a rise",
       "flat top into the end of the series", "peak exactly at the floor", "peak one float32 above the floor",
       "peak one float32 below the floor", "float64 floor between two float32", "three records or more"]
    + ["isolated +Inf", "+Inf run of 2", "+Inf run of 3", "+Inf run of 70", "+Inf run, then lower", "+Inf run, then a rise",
       "+Inf at t = 0", "+Inf at t = 1", "+Inf at t = n - 2", "+Inf at t = n - 1", "-Inf sample", "-Inf gap",
       "+Inf next to -Inf", "two +Inf peaks closer than mpd", "two +Inf peaks mpd apart", "two +Inf peaks mpd + 1 apart",
       "detection snapped onto the first +Inf of a run"]
    + ["NaN at t = 0", "NaN at t = 1", "NaN at t = n - 2", "NaN at t = n - 1", "NaN left of a local maximum",
       "NaN right of a local maximum", "NaN run", "all NaN"]
    + [f"window of {w}" for w in STAT_WINDOWS]
    + ["window == n", "window == n - 1", "last window cut to 1", "last window cut to 2",
       "middle values part at the first radix level", "middle values part at the second radix level",
       "half 1.0, half 1e10", "half -1, half +1", "middle values -0.0 and +0.0", "window of -0.0 only", "odd window, -0.0 in the middle", "constant window",
       "heavy ties", "minority of Inf, finite median", "finite median, Inf MAD", "exactly half +Inf in an even window",
       "majority of +Inf", "all -Inf window", "median Inf, NaN node"]
    + ["all nodes NaN", "one NaN node among finite ones", "peak as high as two equal neighbouring nodes",
       "scalar +Inf", "scalar -Inf", "scalar NaN", "array with a NaN", "array with a +Inf", "array with a -Inf",
       "array all -Inf"]
    + ["mpd = 1", "mpd = 2", "mpd = 3", "mpd even, above 3", "mpd odd, above 3", "mpd >= n",
       "candidate closer than mpd + 1 to the start", "candidate closer than mpd + 1 to the end",
       "equal finite peaks mpd apart", "equal finite peaks mpd + 1 apart"])


def census(case):
    """The set of the CLASSES that `case` meets, read from its data."""
    name, x, src, spec, mpd = case
    n = x.size
    met = set()
    kind = spec[0]
    v = x.astype(np.float64)
    nan, pinf, ninf = np.isnan(x), x == np.inf, x == -np.inf
    floor = float(spec[1]) if kind == "scalar" else -np.inf
    local = extract_rule(x, -np.inf)                      # every local maximum of the rule
    rec = extract_rule(x, floor) if not np.isnan(floor) else local[:0]
    if kind == "scalar":
        if n in SEAM_N:
            met.add(f"n = {n}")
        if 1 in rec:
            met.add("peak at t = 1")
        if n >= 3 and n - 2 in rec:
            met.add("peak at t = n - 2")
        for r in (63, 64, 0, 255):
            want = [t for t in range(2, n - 2) if t % 256 == r]
            if n > 256 + 2 and want and np.isin(want, rec).all():
                met.add(f"a peak at every t = {r} (mod 256)")
        if n >= 3 and v[0] > v[1] and 1 not in rec:
            met.add("maximum at t = 0 does not count")
        if n >= 3 and v[-1] > v[-2]:
            met.add("maximum at t = n - 1 does not count")
        if n >= 258 and np.array_equal(rec, np.arange(1, n - 1, 2)):
            met.add("every odd sample a peak")
        if n >= 3 and not nan.any():
            d = np.diff(v)
            for tag, ok in (("constant", (d == 0).all()), ("rising", (d > 0).all()), ("falling", (d < 0).all())):
                if ok:
                    met.add(tag)
        for a, b in _flat_runs(x):
            if not np.isfinite(x[a]) or a == 0 or not x[a] > x[a - 1]:
                continue
            if b == n:
                met.add("flat top into the end of the series")
            elif x[b] > x[a]:
                met.add("flat top followed by a rise")
            elif b - a in (2, 3, 64, 65, 300):
                met.add(f"flat top of {b - a}")
            if b < n and a // 64 != (b - 1) // 64:
                met.add("flat top over a wave seam")
            if b < n and a // 256 != (b - 1) // 256:
                met.add("flat top over a block seam")
        if np.isfinite(floor):
            f32 = F32(floor)
            if float(f32) == floor:
                for tag, h in (("peak exactly at the floor", f32), ("peak one float32 above the floor", np.nextafter(f32, INF)),
                               ("peak one float32 below the floor", np.nextafter(f32, -INF))):
                    if (x[local] == h).any():
                        met.add(tag)
            else:
                lo, hi = (np.nextafter(f32, -INF), f32) if float(f32) > floor else (f32, np.nextafter(f32, INF))
                if (x[local] == lo).any() and (x[local] == hi).any():
                    met.add("float64 floor between two float32")
        if rec.size >= 3:
            met.add("three records or more")
        if np.isinf(floor) or np.isnan(floor):
            met.add({np.inf: "scalar +Inf", -np.inf: "scalar -Inf"}.get(floor, "scalar NaN"))
    # ---- infinities ----
    inf_peaks = [t for t in local if pinf[t]]
    for a, b in _runs(pinf):
        if b - a == 1 and 1 <= a <= n - 2:
            met.add("isolated +Inf")
        if b - a in (2, 3, 70):
            met.add(f"+Inf run of {b - a}")
        if b - a >= 2 and b + 1 < n and np.isfinite(x[b]) and np.isfinite(x[b + 1]):
            met.add("+Inf run, then a rise" if x[b + 1] > x[b] else "+Inf run, then lower")
    for t, tag in ((0, "t = 0"), (1, "t = 1"), (n - 2, "t = n - 2"), (n - 1, "t = n - 1")):
        if n >= 4 and pinf[t]:
            met.add(f"+Inf at {tag}")
        if n >= 4 and nan[t] and not nan.all():
            met.add(f"NaN at {tag}")
    for a, b in _runs(ninf):
        if 0 < a and b < n:
            met.add("-Inf sample" if b - a == 1 else "-Inf gap")
    if n >= 2 and ((pinf[1:] & ninf[:-1]) | (ninf[1:] & pinf[:-1])).any():
        met.add("+Inf next to -Inf")
    for a in inf_peaks:
        for b in inf_peaks:
            if b > a and mpd > 1:
                gap = b - a
                if gap < mpd:
                    met.add("two +Inf peaks closer than mpd")
                elif gap <= mpd + 1:
                    met.add("two +Inf peaks mpd apart" if gap == mpd else "two +Inf peaks mpd + 1 apart")
    want, _ = definition(case)
    if any(t + 1 < n and pinf[t] and pinf[t + 1] and not (t > 0 and pinf[t - 1]) for t in want):
        met.add("detection snapped onto the first +Inf of a run")
    # ---- NaN ----
    with np.errstate(invalid="ignore"):
        for t in range(1, n - 1):
            if np.isfinite(x[t]) and x[t] > floor:
                if nan[t - 1] and not nan[t + 1] and x[t + 1] <= x[t]:
                    met.add("NaN left of a local maximum")
                if nan[t + 1] and not nan[t - 1] and x[t] > x[t - 1]:
                    met.add("NaN right of a local maximum")
    if any(b - a >= 2 for a, b in _runs(nan)) and not nan.all():
        met.add("NaN run")
    if n >= 3 and nan.all():
        met.add("all NaN")
    # ---- the window statistics and the nodes ----
    if kind == "nodes":
        met |= _census_windows(case)
    if kind == "array":
        arr = np.asarray(spec[1])
        some = lambda m: m.any() and not m.all()
        for tag, m in (("array with a NaN", np.isnan(arr)), ("array with a +Inf", arr == np.inf), ("array with a -Inf", arr == -np.inf)):
            if some(m):
                met.add(tag)
        if (arr == -np.inf).all():
            met.add("array all -Inf")
    # ---- mpd ----
    met.add("mpd = %d" % mpd if mpd <= 3 else "mpd >= n" if mpd >= n else f"mpd {'even' if mpd % 2 == 0 else 'odd'}, above 3")
    for c in _survivors(case):
        if c - (mpd + 1) < 0:
            met.add("candidate closer than mpd + 1 to the start")
        if c + (mpd + 1) >= n:
            met.add("candidate closer than mpd + 1 to the end")
    if mpd > 1:
        fin = [t for t in rec if np.isfinite(x[t])]
        for a in fin:
            for b in fin:
                if b > a and x[a] == x[b] and b - a in (mpd, mpd + 1):
                    met.add("equal finite peaks mpd apart" if b - a == mpd else "equal finite peaks mpd + 1 apart")
    return met


def _survivors(case):
    """The peaks of the definition in front of the snap."""
    from seismic_bpmf_amd import postprocess as pp
    name, x, src, spec, mpd = case
    with np.errstate(invalid="ignore"):
        peaks = pp.detect_peaks(x, mpd=mpd)
        thr = np.broadcast_to(np.asarray(threshold_series(x, spec)), (x.size,))
        return peaks[x[peaks] > thr[peaks]]


def _census_windows(case):
    from seismic_bpmf_amd import postprocess as pp
    name, x, src, spec, mpd = case
    _, window, overlap, n_dev = spec
    n = x.size
    met = set()
    window, shift, nw = bp_window_plan(n, window, overlap)
    if window in STAT_WINDOWS:
        met.add(f"window of {window}")
    if window == n:
        met.add("window == n")
    if window == n - 1:
        met.add("window == n - 1")
    last = min(n, nw * shift + window) - nw * shift
    if last in (1, 2):
        met.add(f"last window cut to {last}")
    med, mad = StandIn().window_stats(x, window, overlap)
    for q in range(1, nw + 1):
        seg = x[q * shift:min(n, q * shift + window)]
        m, d, size = med[q], mad[q], seg.size
        if size == 0 or np.isnan(seg).any():
            continue
        order = np.sort(f32_key(seg))
        n_inf, n_pinf = int(np.isinf(seg).sum()), int((seg == np.inf).sum())
        if size % 2 == 0 and size >= 2:
            lo, hi = order[size // 2 - 1], order[size // 2]
            if lo >> 21 != hi >> 21:
                met.add("middle values part at the first radix level")
            elif lo >> 10 != hi >> 10:
                met.add("middle values part at the second radix level")
            values = set(seg.tolist())
            if values == {1.0, float(F32(1e10))} and (seg == 1.0).sum() * 2 == size:
                met.add("half 1.0, half 1e10")
            if values == {-1.0, 1.0} and (seg == 1.0).sum() * 2 == size:
                met.add("half -1, half +1")
            zeros = seg[seg == 0]
            if zeros.size == 2 and np.signbit(zeros).sum() == 1 and (seg < 0).sum() == size // 2 - 1:
                met.add("middle values -0.0 and +0.0")
            if n_pinf * 2 == size and n_inf == n_pinf:
                met.add("exactly half +Inf in an even window")
        # (np.median ends in np.mean, whose sum starts from +0: a median of -0.0 comes out as +0.0)
        if size >= 2 and (seg == 0).all() and np.signbit(seg).all() and not np.signbit(m):
            met.add("window of -0.0 only")
        if size % 2 and f32_key(np.float32(-0.0)) == order[size // 2] and (seg == 0).sum() == 1 and not np.signbit(m):
            met.add("odd window, -0.0 in the middle")
        if size >= 8 and (seg == seg[0]).all() and d == 0 and np.isfinite(m):
            met.add("constant window")
        if size >= 64 and 1 < np.unique(seg).size <= size // 8 and n_inf == 0:
            met.add("heavy ties")
        if n_inf and np.isfinite(m):
            met.add("minority of Inf, finite median" if np.isfinite(d) else "finite median, Inf MAD")
        if n_pinf * 2 > size and n_pinf < size:
            met.add("majority of +Inf")
        if (seg == -np.inf).all() and size >= 2:
            met.add("all -Inf window")
        if np.isinf(m) and np.isnan(d):
            met.add("median Inf, NaN node")
    with np.errstate(all="ignore"):
        centre, thr = pp.bp_threshold_nodes(n, window, overlap, med, mad, n_dev)
    bad = np.isnan(thr)
    if bad.all():
        met.add("all nodes NaN")
    if bad[1:-1].sum() == 1 and np.isfinite(thr[~bad]).all() and nw >= 3:
        met.add("one NaN node among finite ones")
    local = extract_rule(x, -np.inf)
    for q in range(1, nw):
        if np.isfinite(thr[q]) and thr[q] == thr[q + 1]:
            between = local[(local > centre[q]) & (local < centre[q + 1])]
            if (x[between] == thr[q]).any():
                met.add("peak as high as two equal neighbouring nodes")
    return met
