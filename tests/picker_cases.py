"""Cases and the checkers of the picker batch (csrc/picker.hip; workflow.normalize_batch / picker_batch / find_picks /
pick_events; postprocess.normalize_batch_host / find_picks_host / get_picks_host), shared by
tests/test_picker_host.py (CPU), tests/test_gpu_picker_batch.py (GPU) and tests/golden/make_picker_golden.py.

Normalisation: NORM_CASES lists (n, W, overlap); every case normalises the same nine rows (three "stations" of three
channels), one per ROW_CLASSES plus two more of noise.  Picks: pick_cases() lists (label, series, threshold).
Selection: selection_cases() lists station tables.  Everything is regenerated from fixed seeds.

The checkers compare bit for bit through view(uint32 / uint64); NaNs must sit at the same positions, their payloads
are not compared."""
import numpy as np

# (n, W, overlap): what it exercises
NORM_CASES = (
    (20, 6, .5),          # a sum under 8 elements
    (90, 40, .5),         # the 8-way leaf
    (300, 128, .5),       # the 8-way leaf, full
    (300, 129, .5),       # the first split of the pairwise tree
    (1203, 400, .5),      # a larger window
    (1000, 300, .66),     # shift 102; nodes off the integers
    (777, 256, .75),      # overlap .75
    (6001, 3000, .5),     # a trailing window dropped
    (3000, 3000, .5),     # n = W, three windows, all nodes equal
    (64, 8, .875),        # shift 1
)
# the shapes the reference was first compared on (the golden file holds them too)
NORM_CASES_LARGE = ((6000, 3000, .5), (12000, 3000, .5))
ROW_CLASSES = ("noise100", "zero", "constant", "half_constant", "nan", "tiny20", "negative_zero")
PLACEMENTS = ("inside", "cut_by_end", "past_day", "cut_by_start")


def norm_rows(n, seed=0):
    """(3, 3, n) float32: a row of every class of ROW_CLASSES, then two of plain noise."""
    rng = np.random.default_rng(20261019 + seed)
    x = rng.standard_normal((9, n)).astype(np.float32)
    x[0] *= np.float32(100.0)
    x[1] = 0.0
    x[2] = np.float32(-2.5)
    x[3, : (3 * n) // 4] = np.float32(1.25)      # windows 0 and 1 (and more) constant where 3n/4 >= W
    x[4, n // 3::97] = np.nan
    x[5] *= np.float32(1e-20)
    x[6, ::3] = -0.0
    x[6, : n // 2] = -0.0
    return x.reshape(3, 3, n)


def window_stats(x, W, shift):
    """np.std / np.mean of the reference's windows BEFORE the edges are replaced (for classes_met only)."""
    padded = np.pad(x, ((0, 0), (0, 0), (shift, shift)), mode="reflect")
    win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(padded, W, axis=-1)[:, :, ::shift, :])
    with np.errstate(invalid="ignore"):
        return np.std(win, axis=-1), np.mean(win, axis=-1)


def norm_classes_met(x, W, overlap):
    """The special situations a normalisation case goes through (a set of names)."""
    n = x.shape[-1]
    shift = int((1.0 - overlap) * W)
    std, _ = window_stats(x, W, shift)
    nw = std.shape[-1]
    met = {"row:" + c for c in ROW_CLASSES[: min(len(ROW_CLASSES), x.shape[0] * x.shape[1])]}
    if W < 8:
        met.add("sum_under_8")
    elif W <= 128:
        met.add("one_leaf")
    else:
        met.add("split_tree")
    if np.any((std[..., 0] == 0) & (std[..., 1] != 0)) or np.any((std[..., -1] == 0) & (std[..., -2] != 0)):
        met.add("edge_std0_hidden")
    if nw > 2 and np.any(std[..., 1:-1] == 0):
        met.add("middle_std0_becomes_1")
    if np.isnan(std).any() and not np.isnan(std).all():
        met.add("nan_window")
    if (n + 2 * shift - W) % shift:
        met.add("trailing_window_dropped")
    nodes = np.linspace(shift, n - shift, nw)
    if np.any(nodes != np.round(nodes)):
        met.add("nodes_off_integers")
    if nodes[0] == nodes[-1]:
        met.add("nodes_all_equal")
    if shift == 1:
        met.add("shift_1")
    if np.any((std > 0) & (std < 1e-19)):
        met.add("tiny_std")
    return met


NORM_CLASSES = ({"row:" + c for c in ROW_CLASSES} |
                {"sum_under_8", "one_leaf", "split_tree", "edge_std0_hidden", "middle_std0_becomes_1", "nan_window",
                 "trailing_window_dropped", "nodes_off_integers", "nodes_all_equal", "shift_1", "tiny_std"})


def day_case(n=1203, seed=3):
    """A day (3, 3, N) of the row classes and E = 4 windows of n samples, one per PLACEMENTS, as starts (E,) and as
    starts (E, S) (every station its own shift)."""
    N = 2 * n + 61
    data = norm_rows(N, seed)
    starts = np.array([n // 3, N - n // 2, N + 20, -(n // 3)], dtype=np.int64)
    per_station = starts[:, None] + np.array([0, 7, -11], dtype=np.int64)[None, :]
    return data, starts, per_station


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def check(got, want, label=""):
    """AssertionError unless the float array `got` equals `want` in dtype, shape and every bit, NaNs at the same
    positions."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{label}: got {got.dtype} {got.shape}, want {want.dtype} {want.shape}"
    if not same_bits(got, want):
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        bad = np.argwhere(~((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))
        i = tuple(bad[0])
        raise AssertionError(f"{label}: differs at {len(bad)} of {want.size} elements, first at {i}: got {got[i]!r}, "
                             f"want {want[i]!r}")


def check_picks(got, want, label=""):
    """`got` and `want`: (values float32, means float64, stds float64[, index]) of one series."""
    assert len(got[0]) == len(want[0]), f"{label}: {len(got[0])} picks, want {len(want[0])}"
    for name, g, w, dt in zip(("value", "mean", "std"), got, want, (np.float32, np.float64, np.float64)):
        check(np.asarray(g, dtype=dt), np.asarray(w, dtype=dt), f"{label}: {name}")
    if len(got) > 3 and len(want) > 3:
        assert np.array_equal(np.asarray(got[3], np.int64), np.asarray(want[3], np.int64)), f"{label}: index"


# ---- picks ----

def _gauss(n, centre, sigma, amp):
    t = np.arange(n, dtype=np.float64)
    return amp * np.exp(-0.5 * ((t - centre) / sigma) ** 2)


def pick_cases():
    """[(label, series float32, threshold)]: the designed series and 26 model-like random ones, n from 50 to 3000."""
    out = []
    x = _gauss(3000, 500, 20, .9) + _gauss(3000, 1500, 12, .7) + _gauss(3000, 2400, 30, .4)
    out.append(("separated_gaussians", x, 0.3))
    # two peaks: the lower one's prominence is 0.1 (saddle 0.6) / 0.5 (saddle 0.2); the floor is 0.27
    for name, saddle in (("saddle_above_floor", 0.6), ("saddle_below_floor", 0.2)):
        x = np.interp(np.arange(400), [0, 100, 150, 200, 250, 399], [0, 0, .8, saddle, .7, 0])
        out.append((name, x, 0.3))
    for name, length in (("plateau_even", 10), ("plateau_odd", 11)):
        x = np.zeros(300)
        x[100:100 + length] = 1.0
        x[90:100] = np.linspace(0.05, .95, 10)
        x[100 + length:110 + length] = np.linspace(.95, 0.05, 10)
        out.append((name, x, 0.6))
    x = _gauss(500, 250, 15, .8)
    x[:12] = 1.0
    x[-9:] = 0.9
    out.append(("plateaus_touching_both_ends", x, 0.6))
    x = np.zeros(200)
    x[20:30] = np.linspace(0, 1, 10)
    x[30:40] = np.linspace(1, .5, 10)
    x[40:80] = 0.5
    x[80], x[81:] = 0.9, 0.1                       # 0.5 | 0.9 | 0.1: width 0.75 at half prominence
    x[60] = 0.9
    x[61:80] = 0.5                                 # and a symmetric one: width exactly 1
    out.append(("one_sample_wide", x, 0.3))
    x = np.interp(np.arange(120), [0, 40, 60, 80, 119], [0, 0, .5, 0, 0])
    out.append(("value_equals_threshold", x, 0.5))
    rng = np.random.default_rng(77)
    x = np.convolve(rng.random(1200), np.ones(25) / 25, mode="same")
    x = np.round((x - x.min()) / (x.max() - x.min()) * 16) / 16
    out.append(("quantised", x, 0.6))
    out.append(("quantised_low_threshold", x, 0.1))
    out.append(("wider_than_128", _gauss(2000, 900, 150, .95), 0.6))
    out.append(("wider_than_128_odd", _gauss(1999, 901.3, 97, .77) + _gauss(1999, 300, 60, .5), 0.1))
    out.append(("empty", np.zeros(50), 0.6))
    out.append(("below_threshold", _gauss(777, 300, 10, .55), 0.6))
    x = np.zeros(3000)
    for k in range(40):                            # 40 triangles
        x[50 + 70 * k: 50 + 70 * k + 21] = np.concatenate([np.linspace(0, .5 + .01 * k, 11),
                                                             np.linspace(.5 + .01 * k, 0, 11)[1:]])
    out.append(("forty_picks", x, 0.3))
    x = _gauss(600, 300, 25, .9)
    x[240] = np.nan                                # a NaN on the flank: the walks stop there
    out.append(("nan_on_flank", x, 0.3))
    for k in range(26):
        n = int(rng.integers(50, 3001))
        x = np.zeros(n)
        for _ in range(int(rng.integers(1, 6))):
            x += _gauss(n, rng.uniform(0, n), rng.uniform(2, 60), rng.uniform(.2, 1.3))
        x += 0.03 * rng.random(n)
        x = np.clip(x, 0.0, 1.0)                   # clipped plateaus
        if k % 3 == 0:
            x = np.round(x * 64) / 64
        out.append((f"random_{k}", x, (0.1, 0.3, 0.6)[k % 3]))
    return [(label, np.ascontiguousarray(x, dtype=np.float32), thr) for label, x, thr in out]


def pick_classes_met(series, threshold, host_picks):
    """Names of the situations one pick case goes through; host_picks = find_picks_host(series, threshold,
    return_index=True)."""
    x = series.astype(np.float64)
    met = set()
    values, means, stds, index = host_picks
    if len(values) == 0:
        met.add("no_pick")
    if len(values) > 32:
        met.add("more_than_32")
    if np.any(values.astype(np.float64) == threshold):
        met.add("value_equals_threshold")
    d = np.diff(x)
    rises = np.flatnonzero(d[:-1] > 0) + 1         # i with x[i-1] < x[i]
    candidates = 0
    for i in rises:
        j = i
        while j + 1 < len(x) and x[j + 1] == x[i]:
            j += 1
        if j + 1 < len(x) and x[j + 1] < x[i]:
            if x[i] >= threshold:
                candidates += 1
            if j > i and x[i] >= threshold:
                met.add("plateau_even" if (j - i + 1) % 2 == 0 else "plateau_odd")
        elif j + 1 == len(x) and j > i:
            met.add("plateau_touching_end")
    if len(x) > 1 and x[0] == x[1] and x[0] >= threshold:
        met.add("plateau_touching_start")
    if candidates > len(values):
        met.add("candidate_dropped")               # by prominence or by width
    if len(values) and np.any(stds > 0):
        # window wider than 128 samples: the sums split
        from seismic_bpmf_amd import postprocess as pp
        _, lip, rip = pp.find_peaks_host(series, threshold)
        if np.any(rip.astype(np.int64) - lip.astype(np.int64) + 1 > 128):
            met.add("window_over_128")
        if np.any(rip.astype(np.int64) - lip.astype(np.int64) + 1 < 8):
            met.add("window_under_8")
    if np.isnan(x).any():
        met.add("nan_sample")
    if len(np.unique(x)) < len(x) // 8 and len(values):
        met.add("ties")
    return met


PICK_CLASSES = {"no_pick", "more_than_32", "value_equals_threshold", "plateau_even", "plateau_odd",
                "plateau_touching_end", "plateau_touching_start", "candidate_dropped", "window_over_128",
                "window_under_8", "nan_sample", "ties"}
ALL_CLASSES = NORM_CLASSES | PICK_CLASSES


# ---- selection ----

def _table(rows, max_picks=6):
    """rows: per station ([(proba, pick, unc) ...] for P, [...] for S) -> values, means, stds, counts."""
    S = len(rows)
    values = np.full((S, 2, max_picks), np.nan, dtype=np.float32)
    means = np.full((S, 2, max_picks), np.nan, dtype=np.float64)
    stds = np.full((S, 2, max_picks), np.nan, dtype=np.float64)
    counts = np.zeros((S, 2), dtype=np.int32)
    for s, phases in enumerate(rows):
        for ph, picks in enumerate(phases):
            counts[s, ph] = len(picks)
            for k, (proba, pick, unc) in enumerate(picks):
                values[s, ph, k], means[s, ph, k], stds[s, ph, k] = proba, pick, unc
    return values, means, stds, counts


def selection_cases():
    """[(label, values, means, stds, counts, buffer_length, prior or None, search_win_samp or None)]."""
    designed = [
        ([(.8, 300.5, 2.)], []),                                           # no S
        ([], [(.7, 500.25, 3.)]),                                          # no P
        ([(.9, 700., 2.), (.6, 650., 1.)], [(.95, 600., 2.), (.5, 900., 4.)]),   # every P after the best S
        ([(.9, 200., 2.), (.5, 201., 1.)], [(.8, 200., 2.), (.6, 450., 2.)]),    # picks exactly at buffer_length
        ([(.9, 300., 2.), (.8, 420., 1.)], [(.9, 350., 2.), (.85, 640., 2.)]),   # a prior changes the winner
        ([(.7, 250., 2.), (.7, 260., 1.)], [(.6, 400., 2.), (.6, 500., 2.)]),    # ties: the first wins
        ([], []),                                                          # nothing at all
        ([(.9, 100., 2.)], [(.9, 150., 2.)]),                              # everything inside the buffer
    ]
    prior = np.full((len(designed), 2), np.nan)
    prior[4] = (425., 650.)
    prior[2] = (640., 880.)
    out = [("designed", *_table(designed), 200, None, None),
           ("designed_prior", *_table(designed), 200, prior, 40),
           ("designed_float_buffer", *_table(designed), 200.9, None, None)]
    rng = np.random.default_rng(99)
    for k in range(5):
        rows = []
        for _ in range(7):
            rows.append(tuple([(float(np.float32(rng.uniform(.3, 1))), float(rng.uniform(0, 1000)),
                                float(rng.uniform(.5, 8))) for _ in range(int(rng.integers(0, 6)))]
                              for _ph in range(2)))
        pr = rng.uniform(100, 900, (7, 2))
        pr[rng.random(7) < 0.3] = np.nan
        out.append((f"random_{k}", *_table(rows), int(rng.integers(0, 400)), pr if k % 2 else None,
                    int(rng.integers(20, 400)) if k % 2 else None))
    return out
