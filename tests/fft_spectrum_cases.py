"""Inputs of the FFT-method spectrum tests, regenerated from seeds (tests/test_fft_spectrum_host.py,
tests/test_gpu_fft_spectrum.py, tests/test_gpu_fft_spectrum_guard.py, tests/golden/make_fft_spectrum_golden.py,
tools/probe_fft_spectra.py): the windows of E events x S stations x C components -- noise of 1e-6 on an offset of 3e-5
and a ramp, float32 --, with one all-zero row, one constant row and one row that holds a NaN where the shape has room
for them; the target sets; the allowance of the device and the measure every comparison uses."""
import numpy as np

SAMPLING_RATE = 100.0
TABLE_CUT = 8064                          # FS_TABLE_LDS_MAX of csrc/fft_spectrum.hip: up to here the twiddles lie in LDS
CAP = 16384

SMALL = (5, 3, 3)                         # E, S, C: 45 rows, no multiple of 16
LARGE = (13, 5, 3)                        # 195 rows: four slabs of 64 on the least workspace
ONE = (1, 1, 1)
THREE = (1, 1, 3)
ZERO_ROW, CONSTANT_ROW, NAN_ROW = (1, 0, 1), (2, 1, 0), (3, 2, 2)      # (e, s, c), in shapes that hold them


def targets(key, n):
    """The target frequencies of the set `key` for windows of n samples at SAMPLING_RATE (None: every bin, complex)."""
    freq = np.fft.rfftfreq(n, d=1.0 / SAMPLING_RATE)
    top, K = freq.max(), len(freq)
    if key is None:
        return None
    if key == "log25":                                                # Spectrum.set_target_frequencies(0.5, 45, 25)
        return np.logspace(np.log10(0.5), np.log10(45.0), 25)
    if key == "single":
        return np.array([3.7])
    if key == "bins":                                                 # exactly the frequencies of bins, the last two too
        return freq[np.unique(np.clip([0, 1, K // 3, K // 2, K - 3, K - 2, K - 1], 0, K - 1))].copy()
    if key == "low":                                                  # between bin 0 and bin 1, and below bin 0
        return freq[1] * np.array([0.5, 1e-9, 0.999999, 0.25, -0.5])
    if key == "duplicates":
        return np.array([2.0, 5.0, 2.0, 11.0, 5.0, 5.0, 2.0])
    if key == "straddle":                                             # around 0.99 f_max: one equal to it, one to f_max
        edge = 0.99 * top
        return np.array([0.5 * top, np.nextafter(edge, 0.0), edge, np.nextafter(edge, np.inf), 0.995 * top, top,
                         1.2 * top, 0.9 * top])
    if key == "1024":
        return np.linspace(0.01, 55.0, 1024)
    raise KeyError(key)


LENGTHS = [2, 3, 15, 16, 17, 64, 257, 1000, 1024, 1500, TABLE_CUT, TABLE_CUT + 1]

# (n, target set, (E, S, C)): every case the device is held to
CASES = [(n, "log25", SMALL) for n in LENGTHS] + [(CAP, "log25", THREE)] + \
        [(n, key, SMALL) for n in (17, 1500) for key in ("single", "bins", "low", "duplicates", "straddle")] + \
        [(257, "1024", SMALL), (1500, "1024", SMALL)] + \
        [(n, None, SMALL) for n in (2, 3, 15, 16, 17, 64, 257, 1500)] + [(CAP, None, THREE)] + \
        [(257, "log25", LARGE), (1500, "log25", ONE), (3, None, ONE), (TABLE_CUT + 1, "bins", ONE)] + \
        [(n, None, SMALL) for n in (1000, 1024)]
LARGE_CASE = CASES.index((257, "log25", LARGE))
QUICK = [CASES.index(c) for c in [(17, "log25", SMALL), (64, "log25", SMALL), (257, "log25", SMALL),
                                  (17, "bins", SMALL), (17, "straddle", SMALL), (1500, "straddle", SMALL),
                                  (64, None, SMALL)]]
# what tests/golden/fft_spectrum.npz records: (case, dtype of the traces, alpha), both component modes each; the
# spectra of the short cases are complex
RECORDED = [(k, "f32", 0.05) for k, (n, key, shape) in enumerate(CASES)
            if key != "1024" and (key is not None or n <= 64)] + \
           [(CASES.index(c), "f64", 0.05) for c in [(64, "log25", SMALL), (257, "log25", SMALL), (1500, "log25", SMALL),
                                                     (17, None, SMALL)]] + \
           [(CASES.index(c), dtype, 0.15) for c in [(64, "log25", SMALL), (1500, "log25", SMALL), (64, None, SMALL)]
            for dtype in ("f32", "f64")]
SNR_CASE = CASES.index((257, "log25", SMALL))
SNR_NOISE_EVENTS = [1, 1, 2, 4, 3]        # the event whose windows serve as the noise of event e
SNR_MISSING = (4, 2)                      # (event, station): no noise traces


def label(index):
    n, key, (E, S, C) = CASES[index]
    return f"n={n} {key or 'all bins'} {E}x{S}x{C}"


def recorded_key(index, dtype, alpha, multi):
    return f"{'multi' if multi else 'single'}_{index}_{dtype}_{int(round(100 * alpha)):02d}"


def windows(index):
    """The (E, S, C, n) float32 windows of CASES[index]."""
    n, _, (E, S, C) = CASES[index]
    rng = np.random.default_rng([5000, index])
    x = 1e-6 * rng.standard_normal((E, S, C, n)) + 3e-5
    x += rng.uniform(-1.0, 1.0, (E, S, C, 1)) * 2e-5 * np.arange(n) / n
    x = x.astype(np.float32)
    if (E, S, C) in (SMALL, LARGE):
        x[ZERO_ROW] = 0.0
        x[CONSTANT_ROW] = np.float32(3e-5)
        x[NAN_ROW + (n // 2,)] = np.nan
    return x


def day_of(x, lead=0, gap=7):
    """multiband_cases.day_of: a day the windows are cut from, junk (1.0) around them, and their (E, S) starts."""
    import multiband_cases as mc
    return mc.day_of(x, lead, gap)


def allowance(x, taper, want, multi=False, delta=1.0 / SAMPLING_RATE):
    """What a value of the device may differ from the definition's `want` by: sqrt(2) B delta + 8 * 2^-53 |want|, with
    B = (n + 16) 2^-53 sum_j |x_j taper_j| of the row -- n rounded multiply-adds in any order, a twiddle within 2^-52
    and the definition's own FFT error, on each of re and im, so sqrt(2) B on the modulus; the second term is for the
    modulus, the sum over the components and the interpolation, a convex combination that does not enlarge B.
    With `multi` B is the root of the sum of the components' B^2: |sqrt(sum a_c^2) - sqrt(sum b_c^2)| <= the l2 norm
    of a - b.  A complex `want` is compared as its re and im, each with 8 * 2^-53 of its own size.  0 for a row of
    zeros or a taper of zeros, NaN for a row with a NaN: there the two must agree exactly."""
    n = x.shape[-1]
    with np.errstate(invalid="ignore"):
        B = (n + 16) * 2.0 ** -53 * np.abs(x.astype(np.float64) * taper).sum(axis=-1)
        if multi:
            B = np.sqrt((B * B).sum(axis=-1))
        want = as_reals(want)
        return np.sqrt(2.0) * B[..., None] * delta + 8 * 2.0 ** -53 * np.abs(want)


def as_reals(a):
    """A complex (..., K) array as float64 (..., 2 K), re and im interleaved; a real one as it is."""
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.float64) if np.iscomplexobj(a) else np.asarray(a, dtype=np.float64)


def deviation(got, want, allowance):
    """The worst |got - want| / allowance over every value.  Equal values (NaN equal to NaN) deviate by 0 whatever the
    allowance; where the allowance is 0 or NaN the two must agree exactly: a difference there is infinite.  No value
    is left out."""
    got, want = as_reals(got), as_reals(want)
    assert got.shape == want.shape == allowance.shape, (got.shape, want.shape, allowance.shape)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.where(same, 0.0, np.abs(got - want) / allowance)
    dev[~same & ~(allowance > 0)] = np.inf
    dev[np.isnan(dev)] = np.inf
    return float(dev.max()) if dev.size else 0.0
