"""Inputs of the multi-band spectrum tests, regenerated from seeds (tests/test_multiband_host.py,
tests/test_gpu_multiband.py, tests/golden/make_multiband_golden.py, tools/diff_obspy_multiband.py): the windows of E
events x S stations x C components -- noise of 1e-6 on an offset of 3e-5 and a ramp, float32, so that both detrends
matter --, with one all-zero row, one constant row and one row that holds a NaN; the frequency bands; the day such
windows are cut from; and the measure every comparison uses."""
import numpy as np

SAMPLING_RATE = 100.0
# the octaves [0.5 2^k, 2^k], k = 0 .. 6, and [25, 50], in the order Spectrum.set_frequency_bands gives them (by
# centre frequency): [25, 50] has hi == sr / 2 exactly and [32, 64] lies beyond it -- both are skipped (`>=`)
OCTAVES = {**{f"octave{k}": [0.5 * 2.0 ** k, 2.0 ** k] for k in range(6)}, "half": [25.0, 50.0], "octave6": [32.0, 64.0]}
ONE_BAND = {"one": [2.0, 4.0]}
MANY_BANDS = {f"b{j}": [0.4 * 1.08 ** j, 0.8 * 1.08 ** j] for j in range(64)}     # the last ten reach past sr / 2
HIGH_OCTAVES = {f"octave{k}": [0.5 * 2.0 ** k, 2.0 ** k] for k in range(2, 6)}   # 2 Hz and up
BANDS = {"octaves": OCTAVES, "one": ONE_BAND, "many": MANY_BANDS, "high": HIGH_OCTAVES}

# (n, buffer_seconds): one trimmed sample; a short row; w = 1 (the taper only zeroes the ends); an odd length;
# max_length wins (200 < 250); both limits 256; a usual window; the cap
LENGTHS = [(3, 0.01), (64, 0.1), (257, 0.01), (401, 1.0), (1000, 2.0), (1024, 2.56), (3000, 5.0), (16384, 10.0)]

SMALL = (5, 3, 3)                         # E, S, C: 45 rows
LARGE = (13, 5, 3)                        # 195 rows: four slabs of 64
ZERO_ROW, CONSTANT_ROW, NAN_ROW = (1, 0, 1), (2, 1, 0), (3, 2, 2)      # (e, s, c)

# (label, n, buffer_seconds, corners, bands, (E, S, C)): every case the golden file records
CASES = [(f"n={n} buffer={b}", n, b, 4, "octaves", SMALL) for n, b in LENGTHS] + [
    ("corners=2", 401, 1.0, 2, "octaves", SMALL),
    ("corners=8", 401, 1.0, 8, "high", SMALL),
    ("64 bands", 257, 0.01, 4, "many", SMALL),
    ("one band", 257, 0.01, 4, "one", SMALL),
    ("195 rows", 401, 1.0, 4, "octaves", LARGE),
]
QUICK = [1, 2, 3, 8, 9, 11]              # the cases the planted defects are tried on (a few hundred samples each)


def windows(index):
    """The (E, S, C, n) float32 windows of CASES[index]."""
    _, n, _, _, _, (E, S, C) = CASES[index]
    rng = np.random.default_rng([4000, index])
    x = 1e-6 * rng.standard_normal((E, S, C, n)) + 3e-5
    x += rng.uniform(-1.0, 1.0, (E, S, C, 1)) * 2e-5 * np.arange(n) / n
    x = x.astype(np.float32)
    x[ZERO_ROW] = 0.0
    x[CONSTANT_ROW] = np.float32(3e-5)
    x[NAN_ROW + (n // 2,)] = np.nan
    return x


def day_of(x, lead=0, gap=7):
    """A day the windows `x` (E, S, C, n) are cut from, and their starts: (day (S, C, N) float32, starts (E, S) int64).
    The windows of a channel lie one behind the other from sample `lead` + s on, the day ends `gap` - s samples behind
    the last; the samples around them are junk (1.0)."""
    E, S, C, n = x.shape
    assert gap >= S - 1
    N = lead + E * n + gap
    day = np.ones((S, C, N), dtype=np.float32)
    starts = lead + np.arange(E, dtype=np.int64)[:, None] * n + np.arange(S, dtype=np.int64)[None, :]
    for e in range(E):
        for s in range(S):
            day[s, :, starts[e, s]:starts[e, s] + n] = x[e, s]
    return day, starts


def live_rows(x):
    """(E, S, C) bool: the rows that are neither zero, constant nor hold a NaN."""
    live = np.ones(x.shape[:3], dtype=bool)
    for row in (ZERO_ROW, CONSTANT_ROW, NAN_ROW):
        live[row] = False
    return live


def row_scale(x, prepared):
    """What a row's deviations are measured against: max_k |v_k| of the row after the taper (`prepared`), or -- where
    that is 0: a constant row, of which the reference leaves the rounding residue of its mean -- the largest |x| of the
    row itself.  0 for a row of zeros, NaN for a row that holds one."""
    with np.errstate(invalid="ignore"):
        top, raw = np.abs(prepared).max(axis=-1), np.abs(np.asarray(x, dtype=np.float64)).max(axis=-1)
        return np.where(top > 0, top, raw)


def deviation(got, want, scale, bands):
    """The worst |got - want| (hi - lo) / scale over rows (..., B) and bands, `scale` (...) from row_scale: the error
    relative to what went into the filter, so that a quiet band is not judged by its own small value.  Where the scale
    is 0 or NaN (a row of zeros, a row with a NaN) the two must agree exactly: a difference there is infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bw = np.array([hi - lo for lo, hi in (bands.values() if isinstance(bands, dict) else bands)])
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64)[..., None], got.shape)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.where(same, 0.0, np.abs(got - want) * bw / scale)
    dev[~same & ~(scale > 0)] = np.inf
    dev[np.isnan(dev)] = np.inf
    return float(dev.max()) if dev.size else 0.0
