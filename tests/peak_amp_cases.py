"""Seeded inputs for the peak-amplitude tests (CPU and GPU): detections whose windows data[s, c, i1:i2] fall in
every class of the reference's unguarded NumPy slice (BPMF/similarity_search.py:706-714), the literal loop they are
compared with, and the classifier that counts the classes.  Not a test module."""
import numpy as np

CLASSES = ("interior", "clipped_at_N", "empty_straddle_0", "wrapped", "past_N", "nan", "all_negative",
           "duration_1", "duration_gt_N")


def make_case(seed, N, S, C, T, D, offset, duration, norm=True, nan_every=None):
    """dict(data, rows, samples, moveouts, offset, duration, data_norm).  The detection samples are drawn from zones
    that put the window start i1 = k + moveout - offset inside the day, across its end, across sample 0, wholly
    before sample 0 (wrapping), one whole day before that, past the end, and far outside on both sides."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((S, C, N)).astype(np.float32)
    flat = data.reshape(S * C, N)
    for ch in range(S * C):
        if ch % 3 == 1:                                   # a channel below zero throughout
            flat[ch] = -np.abs(flat[ch]) - np.float32(0.125)
        else:                                             # a stretch below zero on every other channel
            lo = int(rng.integers(0, max(1, N // 2)))
            flat[ch, lo:lo + N // 4] = -np.abs(flat[ch, lo:lo + N // 4]) - np.float32(0.125)
        gap = int(rng.integers(0, max(1, N - 8)))
        flat[ch, gap:gap + 5] = 0.0                       # a gap filled with zeros
    n_nan = N // (nan_every or max(4, 3 * max(1, min(abs(duration), N)))) + 1
    for ch in range(S * C):
        flat[ch, rng.integers(0, N, n_nan)] = np.nan
        flat[ch, rng.integers(0, N, 2)] = np.inf
        flat[ch, rng.integers(0, N, 2)] = -np.inf
    M = max(1, min(50, N // 10))
    moveouts = rng.integers(-M, M + 1, (T, S, C)).astype(np.int32)
    moveouts[rng.random((T, S, C)) < 0.01] = np.int32(3 * N)          # a moveout longer than the day
    dur = int(duration)
    zones = [(M, N - dur - M), (N - dur, N), (-dur, 0), (-N, -dur - M), (-N - dur, -N), (N, 2 * N),
             (2 * N, 1 << 40), (-(1 << 40), -2 * N)]
    weights = np.array([4, 2, 2, 2, 1, 2, 0.5, 0.5])
    zone = rng.choice(len(zones), size=D, p=weights / weights.sum())
    samples = np.empty(D, dtype=np.int64)
    for q in range(D):
        lo, hi = sorted(zones[zone[q]])
        samples[q] = int(rng.integers(lo, hi + 1)) + int(offset)
    if D >= 8:
        samples[:4] = [(1 << 62) + 11, -(1 << 62) - 11, np.iinfo(np.int64).max, np.iinfo(np.int64).min]
    rows = rng.integers(0, T, D).astype(np.int32)
    data_norm = rng.uniform(0.5, 2.0, (S, C)).astype(np.float32) if norm else None
    return dict(data=data, rows=rows, samples=samples, moveouts=moveouts, offset=int(offset), duration=dur,
                data_norm=data_norm)


def literal_loop(case):
    """The reference's three-level loop, lines 695-714, on the arrays of a case."""
    data, data_norm = case["data"], case["data_norm"]
    S, C, _ = data.shape
    out = np.zeros((len(case["rows"]), S, C), dtype=np.float32)
    for q in range(len(case["rows"])):
        for s in range(S):
            for c in range(C):
                mv_sc = int(case["moveouts"][case["rows"][q], s, c])
                time_idx1 = int(case["samples"][q]) + mv_sc - case["offset"]
                time_idx2 = time_idx1 + case["duration"]
                win_peak_amp = data[s, c, time_idx1:time_idx2]
                if len(win_peak_amp) > 0:
                    out[q, s, c] = win_peak_amp.max() * data_norm[s, c] if data_norm is not None else win_peak_amp.max()
    return out


def count_classes(case, amplitudes, counts=None):
    """Adds the windows of a case to `counts` {class: windows}; `amplitudes` is what the host mirror returned for it
    (the NaN and all-negative classes are read off its values, with the norm taken out by its sign)."""
    counts = {k: 0 for k in CLASSES} if counts is None else counts
    N = case["data"].shape[-1]
    i1 = (case["samples"].astype(object)[:, None, None] + case["moveouts"][case["rows"]].astype(object)
          - case["offset"])
    i2 = i1 + case["duration"]
    nonempty = np.zeros(i1.shape, bool)
    for idx in np.ndindex(i1.shape):
        a, b, _ = slice(i1[idx], i2[idx]).indices(N)
        nonempty[idx] = b > a
    counts["interior"] += int(((i1 >= 0) & (i1 < i2) & (i2 <= N)).sum())
    counts["clipped_at_N"] += int(((i1 >= 0) & (i1 < N) & (i2 > N)).sum())
    counts["empty_straddle_0"] += int(((i1 < 0) & (i2 >= 0) & ~nonempty).sum())
    counts["wrapped"] += int(((i1 >= -N) & (i1 < i2) & (i2 < 0) & nonempty).sum())
    counts["past_N"] += int(((i1 >= N) & (i2 >= N)).sum())
    sign = 1.0 if case["data_norm"] is None else np.sign(case["data_norm"])[None]
    counts["nan"] += int((nonempty & np.isnan(amplitudes)).sum())
    counts["all_negative"] += int((nonempty & (amplitudes * sign < 0)).sum())
    if case["duration"] == 1:
        counts["duration_1"] += i1.size
    if case["duration"] > N:
        counts["duration_gt_N"] += i1.size
    return counts


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# (seed, N, S, C, T, D, offset, duration, with data_norm): N not a multiple of 4 in most
CPU_CASES = [(1, 1000, 4, 3, 5, 200, 20, 60, True), (2, 1003, 1, 1, 3, 600, 10, 1, True),
             (3, 997, 7, 1, 4, 100, 0, 1500, False), (4, 1001, 20, 3, 6, 40, 100, 300, True),
             (5, 1002, 1, 3, 2, 300, -5, 37, False), (6, 350, 2, 3, 3, 60, 7, 351, True)]
