"""Cases of the polyphase resampling (csrc/resample.hip; workflow.resample_poly / picker_batch(upsampling=,
downsampling=); postprocess.resample_poly_host / resample_poly_plan), shared by tests/test_resample_host.py (CPU),
tests/test_gpu_resample.py (GPU) and tests/golden/make_resample_golden.py.

FACTORS lists (up, down); lengths(up, down) the row lengths of a pair; rows(n) the twelve rows every case resamples.
Everything is regenerated from fixed seeds.  The checker is picker_cases.check: bit for bit through view(uint32), NaNs
at the same positions.  defective() is the definition with one planted defect: the CPU test shows that the checker
rejects each of them on these inputs."""
import numpy as np

FACTORS = (
    (4, 1), (1, 4), (2, 1), (5, 2), (2, 5), (3, 7), (7, 3),
    (8, 2),               # reduces to (4, 1)
    (4, 6),               # reduces to (2, 3)
    (64, 1), (1, 64),     # the largest rates
    (3, 3),               # a copy
)
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1.0, 1e1, 1e2, 1e3, 3e-3)
N_ROWS = len(SCALES) + 3
DEFECTS = ("fma", "descending", "phase_shift", "skip_zero_taps")
GOLDEN_KEEP = 128                                # samples kept at the head, around the middle and at the tail
GOLDEN_ROWS = (0, 7, len(SCALES) + 1, len(SCALES) + 2)       # ... of these rows, for the long cases
GOLDEN_RATES = (2, 3, 4, 5, 7, 49, 64)             # the rates whose float32 taps the golden file keeps
GOLDEN_ALL = 1536                                # a case of at most this many output samples is kept whole


def taps_per_phase(up, down):
    """hp of the plan for rows of 3000 samples (it is the same for every length from hp + 1 on)."""
    from seismic_bpmf_amd import postprocess as pp
    up, down = pp.resample_poly_factors(up, down)
    return len(pp.resample_poly_plan(3000, up, down)[5]) // up


def lengths(up, down):
    hp = taps_per_phase(up, down)
    return tuple(sorted({1, 2, 3, hp - 1, hp, hp + 1, 257, 3000} - {0}))


def rows(n, seed=0):
    """(12, n) float32: nine rows of noise at the SCALES, a zero row, a row with -0.0 samples, a row with one NaN in
    the middle."""
    rng = np.random.default_rng(20261019 + 1000 * seed + n)
    x = rng.standard_normal((N_ROWS, n)).astype(np.float32)
    for k, s in enumerate(SCALES):
        x[k] *= np.float32(s)
    x[len(SCALES)] = 0.0
    x[len(SCALES) + 1, ::3] = -0.0
    x[len(SCALES) + 1, : n // 2] = -0.0
    x[len(SCALES) + 2, n // 2] = np.nan
    return x


def cases():
    """[(up, down, n)] of every factor pair and length."""
    return [(up, down, n) for up, down in FACTORS for n in lengths(up, down)]


def golden_selection(n_out):
    """(rows, samples) of a case that the golden file keeps: everything of a short case; of a long one the head, the
    middle (where the NaN spreads) and the tail of four rows."""
    if N_ROWS * n_out <= GOLDEN_ALL:
        return np.arange(N_ROWS), np.arange(n_out)
    if n_out <= 3 * GOLDEN_KEEP:
        return np.asarray(GOLDEN_ROWS), np.arange(n_out)
    mid = n_out // 2 - GOLDEN_KEEP // 2
    keep = np.concatenate([np.arange(GOLDEN_KEEP), mid + np.arange(GOLDEN_KEEP),
                           n_out - GOLDEN_KEEP + np.arange(GOLDEN_KEEP)])
    return np.asarray(GOLDEN_ROWS), keep


def golden_key(up, down, n):
    return f"up{up}_down{down}_n{n}"


def defective(x, up, down, defect):
    """resample_poly_host with one planted defect: "fma" (the product enters the sum unrounded, as a contracted
    multiply-add computes it), "descending" (input index descending), "phase_shift" (the tap table read one phase
    further) or "skip_zero_taps" (the zero taps of the padding do not multiply)."""
    from seismic_bpmf_amd import postprocess as pp
    assert defect in DEFECTS
    x = np.asarray(x, dtype=np.float32)
    up, down = pp.resample_poly_factors(up, down)
    n_in = x.shape[-1]
    _, n_out, _, n_pre_remove, _, table = pp.resample_poly_plan(n_in, up, down)
    hp = len(table) // up
    m = np.arange(n_out, dtype=np.int64) + n_pre_remove
    j_hi, t = m * down // up, m * down % up
    if defect == "phase_shift":
        t = (t + 1) % up if up > 1 else t
        j_hi = j_hi + (1 if up == 1 else 0)
    acc = np.zeros(x.shape[:-1] + (n_out,), dtype=np.float32)
    order = range(hp) if defect == "descending" else range(hp - 1, -1, -1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in order:
            j = j_hi - k
            ok = (j >= 0) & (j < n_in)
            if defect == "skip_zero_taps":
                ok &= table[t + k * up] != 0
            q = np.flatnonzero(ok)
            if not len(q):
                continue
            if defect == "fma":
                exact = x[..., j[q]].astype(np.float64) * table[t[q] + k * up].astype(np.float64)
                acc[..., q] = (acc[..., q].astype(np.float64) + exact).astype(np.float32)
            else:
                acc[..., q] = acc[..., q] + x[..., j[q]] * table[t[q] + k * up]
    return acc


def tile_lengths(tile, up, down):
    """Row lengths that put n_out = ceil(n up / down) just under one tile (tile - 1, or the largest count below it that
    a length gives), at one tile (or the largest count up to it), just over one tile and just over two tiles
    (tile + 1 and 2 tile + 1, or the smallest counts from there on)."""
    def count(n):
        return -(-n * up // down)

    def largest_up_to(want):
        n = max(1, want * down // up)
        while count(n + 1) <= want:
            n += 1
        return n

    def smallest_from(want):
        n = max(1, want * down // up)
        while count(n) < want:
            n += 1
        return n
    return [largest_up_to(tile - 1), largest_up_to(tile), smallest_from(tile + 1), smallest_from(2 * tile + 1)]
