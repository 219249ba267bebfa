"""Inputs of the SVD-Wiener stack tests, regenerated from seeds (tests/test_svdwf_host.py, tests/test_gpu_svdwf.py,
tests/golden/make_svdwf_golden.py): the (n, m) matrices of one channel's detections -- two Gaussian wavelets with
random amplitudes per event plus white noise, float32 --, the parameter sets, the ragged batch, and the conditions
every case must meet before a device result is compared with the definition within limits that are derived and not
measured: `conditions` asserts them on the CPU.  `degenerate_cases` are the spectra that generator never gives --
rank-deficient, duplicated, badly scaled, clustered -- and `jacobi_reference` the device's eigen-solver restated."""
import numpy as np

SAMPLING_RATE = 25.0
FREQMIN, FREQMAX = 2.0, 12.0

# (n, m) of one group; the Gram matrix is formed over the events for n <= m, over the samples otherwise
SMALL_SHAPES = [(1, 64), (2, 33), (3, 64), (7, 200), (40, 200)]
MORE_SHAPES = [(64, 64), (70, 48), (300, 96), (129, 128), (128, 129)]
CAP_SHAPES = [(512, 600), (600, 512)]
LONG_SHAPE = (12, 2048)

EXPL_VARS = (0.4, 0.8, 1.0)
MAX_SINGULAR_VALUES = (1, 5, 8)

# the committed cases of the reference comparison: (label, kind, n, m, expl_var, max_singular_values, w, band-pass)
REFERENCE_CASES = [
    ("3x64", "wavelets", 3, 64, 0.4, 5, None, True),
    ("3x64 w=1", "wavelets", 3, 64, 0.8, 5, 1, True),
    ("1x64", "wavelets", 1, 64, 0.4, 5, None, True),
    ("1x64 w=4", "wavelets", 1, 64, 0.4, 5, 4, False),
    ("7x200", "wavelets", 7, 200, 0.4, 5, None, True),
    ("7x200 w=5 0.8", "wavelets", 7, 200, 0.8, 5, 5, True),
    ("7x200 w=4 0.8 cap 2", "wavelets", 7, 200, 0.8, 2, 4, False),
    ("7x200 w=4 all", "wavelets", 7, 200, 1.0, 5, 4, True),
    ("rank one 3x64 all", "rank one", 3, 64, 1.0, 5, None, False),
    ("negative 7x100 raw", "negative", 7, 100, 0.4, 5, None, False),
    ("40x200", "wavelets", 40, 200, 0.4, 5, None, True),
    ("40x200 w=4 0.8", "wavelets", 40, 200, 0.8, 5, 4, True),
    ("40x200 w=1 0.8 raw", "wavelets", 40, 200, 0.8, 8, 1, False),
    ("300x200 0.8", "wavelets", 300, 200, 0.8, 5, None, True),
    ("200x1000", "wavelets", 200, 1000, 0.4, 5, 5, True),
]
REFERENCE_ROWS_KEPT = 8                   # of the larger cases only these rows of `filtered` are recorded
BANDPASS_CASES = [(5, 200, 4, 2.0, 12.0), (3, 1000, 4, 0.5, 1.0), (4, 33, 2, 1.0, 5.0), (2, 4097, 4, 2.0, 12.0)]  # (rows, m, order, band)
BUTTER_CASES = [(order, lo, hi) for order in (2, 4) for lo, hi in ((2.0, 12.0), (0.5, 1.0), (5.0, 12.4))]  # Hz at 25 Hz


def reference_matrix(index):
    """The (n, m) float32 matrix of REFERENCE_CASES[index]."""
    _, kind, n, m = REFERENCE_CASES[index][:4]
    if kind == "wavelets":
        return matrix(n, m, 1000 + index)
    rng = np.random.default_rng(2000 + index)
    if kind == "rank one":                # exactly rank one in float32: small integers; var[0] = 1 = expl_var
        return np.outer(np.arange(1, n + 1), rng.integers(-8, 9, m)).astype(np.float32)
    assert kind == "negative"             # every sample negative: the stack is negative throughout
    bump = 1.0 + np.exp(-0.5 * ((np.arange(m) - 0.45 * m) / 6.0) ** 2)
    return (-(rng.uniform(2.0, 3.0, (n, 1)) * bump) + 0.05 * rng.standard_normal((n, m))).astype(np.float32)


def kept_rows(n):
    """The rows of `filtered` the golden file records for a case of n events."""
    return np.arange(n) if n <= REFERENCE_ROWS_KEPT else np.linspace(0, n - 1, REFERENCE_ROWS_KEPT).astype(np.int64)


def bandpass_rows(index):
    """The (rows, m) float64 input of BANDPASS_CASES[index]: noise on an offset and a slope."""
    rows, m = BANDPASS_CASES[index][:2]
    rng = np.random.default_rng(3000 + index)
    return rng.standard_normal((rows, m)) + rng.uniform(-3, 3, (rows, 1)) + rng.uniform(-.01, .01, (rows, 1)) * np.arange(m)


def window_sizes(n):
    """wiener_filter_colsize of the parameter sweep: the default, none, even, odd, longer than the group."""
    return (None, 1, 4, 5, n + 3)


def matrix(n, m, seed, noise=0.3):
    """(n, m) float32: two Gaussian wavelets with random amplitudes per event plus white noise."""
    rng = np.random.default_rng([seed, n, m])
    t = np.arange(m, dtype=np.float64)
    w1 = np.exp(-0.5 * ((t - 0.4 * m) / (0.03 * m + 1.0)) ** 2) * np.cos(0.5 * t)
    w2 = np.exp(-0.5 * ((t - 0.6 * m) / (0.05 * m + 1.0)) ** 2) * np.sin(0.3 * t)
    x = rng.uniform(0.5, 2.0, (n, 1)) * w1 + rng.uniform(-1.0, 1.0, (n, 1)) * w2 + noise * rng.standard_normal((n, m))
    return x.astype(np.float32)


def group(n, m, seed, S=1, C=1):
    """(n, S, C, m) float32: one group, every channel a matrix of its own."""
    x = np.empty((n, S, C, m), dtype=np.float32)
    for s in range(S):
        for c in range(C):
            x[:, s, c] = matrix(n, m, seed + 101 * s + 11 * c)
    return x


def sos_table():
    """The band-pass of the reference call (order 4, 2-12 Hz at 25 Hz)."""
    from seismic_bpmf_amd import postprocess as pp
    return pp.butter_bandpass_sos(4, FREQMIN / (SAMPLING_RATE / 2), FREQMAX / (SAMPLING_RATE / 2))


RAGGED_SIZES = (1, 7, 0, 40)
RAGGED_M = 100
RAGGED_ZERO = (1, 0, 0)                  # (group, station, component): all zeros
RAGGED_ZERO_COLUMNS = (3, 0, 1)          # samples 10 .. 12 are zero in every event
RAGGED_NEGATIVE = (3, 1, 2)              # every sample negative: the stack is negative throughout (no band-pass)


def ragged_batch():
    """G = 4 groups of 1, 7, 0 and 40 events, S x C = 2 x 3, with the three special channels.  Returns (x, offsets)."""
    off = np.concatenate(([0], np.cumsum(RAGGED_SIZES))).astype(np.int64)
    x = np.concatenate([group(n, RAGGED_M, 40 + g, 2, 3) for g, n in enumerate(RAGGED_SIZES)], axis=0)
    g, s, c = RAGGED_ZERO
    x[off[g]:off[g + 1], s, c] = 0.0
    g, s, c = RAGGED_ZERO_COLUMNS
    x[off[g]:off[g + 1], s, c, 10:13] = 0.0
    g, s, c = RAGGED_NEGATIVE
    n = RAGGED_SIZES[g]
    rng = np.random.default_rng(77)
    t = np.arange(RAGGED_M)
    bump = 1.0 + np.exp(-0.5 * ((t - 45.0) / 6.0) ** 2)
    x[off[g]:off[g + 1], s, c] = (-(rng.uniform(2.0, 3.0, (n, 1)) * bump)
                                   + 0.05 * rng.standard_normal((n, RAGGED_M))).astype(np.float32)
    return x, off


def conditions(a, expl_var, max_singular_values):
    """Assert what the derived limits rest on, for one channel's matrix: finite input; every retained sigma_j^2
    separated from the next by at least 1e-4 sigma_1^2; no var[j] within 1e-4 of expl_var (expl_var = 1: the rank
    exceeds max_singular_values, so that the cap decides).  Returns k (0 for a zero matrix)."""
    a = np.asarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    s = np.linalg.svd(a, compute_uv=False)
    s2 = s ** 2
    if s2.sum() == 0.0:
        return 0
    var = np.cumsum(s2) / s2.sum()
    if expl_var >= 1.0:
        rank = int((s2 > 1e-4 * s2[0]).sum())
        assert rank > max_singular_values or rank == len(s2), (rank, max_singular_values)
        k = min(max_singular_values, len(s2))
        if rank > max_singular_values:
            assert (var[:max_singular_values] < 1.0 - 1e-4).all()
    else:
        assert (np.abs(var[:max_singular_values] - expl_var) > 1e-4).all(), (var[:8], expl_var)
        k = min(max_singular_values, int(np.flatnonzero(var >= expl_var)[0]) + 1)
    nxt = np.append(s2, 0.0)
    assert (s2[:k] - nxt[1:k + 1] >= 1e-4 * s2[0]).all(), (s2[:k + 1] / s2[0])
    return k


def conditions_subspace(a, expl_var, max_singular_values):
    """`conditions` for a matrix whose retained singular values may be equal among themselves: finite input, var away
    from expl_var by 1e-4, and sigma_k^2 - sigma_(k+1)^2 >= 1e-4 sigma_1^2 for the LAST retained value only.  What is
    then unique is the projector onto the retained subspace, not the vectors.  Returns k."""
    a = np.asarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    s2 = np.linalg.svd(a, compute_uv=False) ** 2
    assert s2.sum() > 0.0 and expl_var < 1.0
    var = np.cumsum(s2) / s2.sum()
    assert (np.abs(var[:max_singular_values] - expl_var) > 1e-4).all(), (var[:8], expl_var)
    k = min(max_singular_values, int(np.flatnonzero(var >= expl_var)[0]) + 1)
    nxt = np.append(s2, 0.0)
    assert s2[k - 1] - nxt[k] >= 1e-4 * s2[0], (k, s2[:k + 1] / s2[0])
    return k


# ---- degenerate spectra: rank-deficient, duplicated, badly scaled and clustered matrices ----
EQUAL_SIGMA = "equal sigma 6x200"
JACOBI_REFERENCE_MAX_K = 128             # jacobi_reference is a test helper: about a second at this order


def degenerate_params(n):
    """(expl_var, max_singular_values, w, band-pass) of the degenerate cases."""
    return [(0.4, 5, None, True), (0.8, 5, 4, False), (0.8, 5, 1, False), (0.8, 8, n + 3, True)]


def fixed_wavelets(r, m):
    """(r, m) float64: r linearly independent Gaussian wavelets, the same for every event."""
    t = np.arange(m, dtype=np.float64)
    return np.stack([np.exp(-0.5 * ((t - (j + 1.0) / (r + 1.0) * m) / (0.04 * m + 1.0)) ** 2) * np.cos((0.2 + 0.15 * j) * t)
                     for j in range(r)])


def low_rank(n, m, r, seed):
    """(n, m) float32 without noise: random amplitudes on r fixed wavelets (rank r up to the float32 rounding)."""
    rng = np.random.default_rng([seed, n, m, r])
    amplitudes = rng.uniform(0.5, 2.0, (n, r)) * rng.choice([-1.0, 1.0], (n, r))
    return (amplitudes @ fixed_wavelets(r, m)).astype(np.float32)


def equal_sigma_matrix():
    """6 x 200 float32, sigma_1 = sigma_2 exactly: rows 0-2 carry one wavelet on samples 0 .. 99, rows 3-5 the same
    wavelet moved to samples 100 .. 199 (same float32 values: equal norm), with the same three amplitudes."""
    t = np.arange(100, dtype=np.float64)
    w = (np.exp(-0.5 * ((t - 50.0) / 9.0) ** 2) * np.cos(0.5 * t)).astype(np.float32)
    x = np.zeros((6, 200), dtype=np.float32)
    for i, amplitude in enumerate((1.0, 2.0, 0.5)):
        x[i, :100] = np.float32(amplitude) * w
        x[3 + i, 100:] = np.float32(amplitude) * w
    return x


def degenerate_cases():
    """[(label, (n, m) float32 matrix, [(expl_var, max_singular_values, w, band-pass), ...])]: the spectra real groups
    have and `matrix` does not -- events without data, duplicated detections, noise-free stacks, one event far above
    the others, physical units, constant traces, and two equal singular values (EQUAL_SIGMA: conditions_subspace)."""
    out = []

    def add(label, x, first_only=False):
        assert x.dtype == np.float32
        params = degenerate_params(len(x))
        out.append((f"{label} {x.shape[0]}x{x.shape[1]}", x, params[:1] if first_only else params))

    x = matrix(40, 200, 501)
    x[np.random.default_rng(502).choice(40, 15, replace=False)] = 0.0
    add("zero rows", x)
    x = matrix(8, 200, 503)
    x[4:] = 0.0
    add("zero rows", x)
    for n, m, seed in ((40, 200, 504), (512, 600, 505)):
        x = matrix(n, m, seed)
        x[n // 2:] = x[:n // 2]
        add("duplicated rows", x, first_only=n == 512)
    add("identical rows", np.repeat(matrix(1, 200, 506), 7, axis=0))
    for r, n, m in ((3, 40, 200), (2, 7, 200), (5, 300, 96), (2, 512, 600)):
        add(f"low rank {r}", low_rank(n, m, r, 507), first_only=n == 512)
    x = matrix(40, 200, 508)
    x[17] *= np.float32(1e4)
    add("one event x 1e4", x)
    add("scaled by 1e-9", matrix(40, 200, 509) * np.float32(1e-9))
    add("scaled by 1e15", matrix(40, 200, 510) * np.float32(1e15))
    add("constant rows", np.repeat(np.random.default_rng(511).uniform(-2.0, 2.0, (7, 1)).astype(np.float32), 200, axis=1))
    out.append((EQUAL_SIGMA, equal_sigma_matrix(), degenerate_params(6)))
    return out


def gram(a):
    """The float64 Gram matrix the device diagonalises: over the events for n <= m, over the samples otherwise."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    return a @ a.T if a.shape[0] <= a.shape[1] else a.T @ a


def jacobi_reference(G, max_sweeps=60, defect=None):
    """The eigen-solve of csrc/svdwf.hip's header restated in float64 NumPy, one round-robin step at a time: the (K, K)
    matrix padded with a zero row and column to even order Kp; step `step` of a sweep pairs a = (step + i) % (Kp - 1)
    with b = Kp - 1 (i = 0) or (step + Kp - 1 - i) % (Kp - 1), i < Kp / 2; a pair with
    |g_pq| <= 2^-52 sqrt|g_pp| sqrt|g_qq| is skipped; tau = (g_qq - g_pp) / 2 g_pq,
    t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; the columns are rotated, then the rows,
    and the rotated element is set to zero; the solve ends with the first sweep that rotates nothing.  Returns
    (sweeps, status, eigenvalues (K,) in index order): status 1 at the cap, and with no sweep at all where a diagonal
    element is not finite (a NaN or an Inf in the channel), as in the kernel.  `defect` plants one for the tests."""
    G = np.asarray(G, dtype=np.float64)
    K = len(G)
    Kp = K + (K & 1)
    A = np.zeros((Kp, Kp))
    A[:K, :K] = G
    M1, i = Kp - 1, np.arange(Kp // 2)
    eps = 2.0 ** -52
    sweeps, status = 0, 1
    if not np.isfinite(np.diag(G)).all():
        return 0, 1, np.diag(G).copy()
    with np.errstate(all="ignore"):
        for sweep in range(max_sweeps):
            rotated = False
            for step in range(M1):
                a, b = (step + i) % M1, np.where(i == 0, M1, (step + M1 - i) % M1)
                p, q = np.minimum(a, b), np.maximum(a, b)
                gpp, gqq, gpq = A[p, p], A[q, q], A[p, q]
                skip = np.abs(gpq) <= eps * (np.sqrt(np.abs(gpp)) * np.sqrt(np.abs(gqq)))
                if defect == "a pair whose g_pp is 0 or below skipped":
                    skip = skip | (gpp <= 0.0) | (gqq <= 0.0)
                tau = (gqq - gpp) / (2.0 * gpq)
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = np.where(skip, 0.0, t * c)
                on = s != 0.0                                      # (the kernel leaves a pair with s = 0 untouched)
                if not on.any():
                    continue
                rotated = True
                p, q, c, s = p[on], q[on], c[on], s[on]
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * x - s * y, s * x + c * y
                x, y = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
                A[p, q] = A[q, p] = 0.0
            sweeps = sweep + 1
            if not rotated:
                status = 0
                break
    return sweeps, status, np.diag(A)[:Kp if defect == "padded index taken for a real one" else K].copy()


def scale(values):
    """The scale a channel's deviations are measured against: its largest magnitude (1 for a zero channel)."""
    top = float(np.abs(values).max()) if np.size(values) else 0.0
    return top if top > 0 else 1.0
