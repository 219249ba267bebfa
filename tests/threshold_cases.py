"""The RMS time-dependent threshold and the candidate extraction (csrc/post.hip) at their seams: a plain definition, a
mirror of the kernels' decomposition that takes planted defects by name, and the table of the smallest shapes at
which each seam exists.  test_threshold_cases_host.py shows on the CPU that definition, C oracle and the reference's
own output agree on the table and that every planted defect is rejected by a named case;
test_gpu_threshold_seams.py runs the same table on the device.  Every comparison is bit for bit.

Definition (tdt_rms_definition, extract_definition): NumPy float32 written from BPMF/libc.c:516-673 and the header
comments of post.hip -- vectorised ACROSS windows, a Python loop ALONG the window, so every float accumulation is the
reference's sequential one.  It does not call the oracle.

Mirror (tdt_rms_mirror, extract_mirror): what the kernels do instead -- steps of 32 samples with six steps of loads
in flight and a clamped reload, the unrolled loop, its remainder and the scalar tail, the hot path `f` or the
replacement path `g` chosen per lane and step by min |v| == 0, the gauss index from g0 = i0 % 500, partial sums per
global window, the three loops of the smoothing kernel, the expansion; in the extraction the groups of four samples
that look their window up at their two ends.  `drop` names the defects to plant (TDT_DEFECTS, EXTRACT_DEFECTS).

Out of scope: n >= 2^31 and windows near 2^31 (gigabytes per case), non-finite CC values other than the NaN rows that
zeros produce, the medians of the MAD threshold (test_gpu_threshold.py)."""
import functools
from dataclasses import dataclass, field

import numpy as np

f32, f64 = np.float32, np.float64
STEP, DEPTH, GAUSS_LEN = 32, 6, 500
ROW_LIMIT = 65535
candidate_dtype = np.dtype([("row", np.int32), ("index", np.int32), ("cc", np.float32), ("threshold", np.float32)])

TDT_DEFECTS = frozenset([
    "tail_dropped", "tail_not_replaced", "gauss_without_g0", "zero_step_by_min_not_abs", "clamped_reload_accumulated",
    "remainder_steps_skipped", "count_includes_zeros", "dev_includes_zeros", "glob_takes_remainder",
    "smooth_skipped_below_3_windows", "expand_tail_gt", "expand_unclamped"])
EXTRACT_DEFECTS = frozenset([
    "group_window_from_first_only", "group_tail_dropped", "ge_instead_of_gt", "cap_ignored", "mad_head_window_zero",
    "nan_threshold_falls_to_cap"])


def _drop(drop, known):
    drop = frozenset([drop] if isinstance(drop, str) else (drop or ()))
    assert drop <= known, sorted(drop - known)
    return drop


def noise(seed, shape):
    """float32 values in (-1, 1), bell-shaped (the mean of two uniforms), from 64-bit integer arithmetic alone
    (splitmix64): the same bits under every NumPy and libm, so recorded outputs stay valid."""
    count = int(np.prod(shape))
    z = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z = z + np.full(count, seed, np.uint64) * np.uint64(0xD1B54A32D192ED03)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    a = (z >> np.uint64(40)).astype(f64)
    b = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(f64)
    return ((a + b + 1.0) / 2.0 ** 24 - 1.0).astype(f32).reshape(shape)


def gauss_sample(seed):
    """500 values standing in for the standard-normal sample (any 500 floats serve: distinct, both signs)."""
    return (noise(seed, GAUSS_LEN) * f32(2.5)).astype(f32)


def tdt_sizes(n, half_window, shift):
    """(window, n_glob, n_win) of libc.c:527-528 / :553, None where the library refuses.  shift == window + 1 (an
    odd Python window with overlap 0) is admitted: the reference's size_t difference wraps to (n + 1) / shift."""
    window = 2 * half_window
    if window == 0 or window > 0x7FFFFFFF or shift == 0 or shift > window + 1 or n < window:
        return None
    return window, n // window, (n - window + shift) // shift


def reference_in_bounds(n, half_window, shift):
    """The reference's own expansion reads threshold_win[i / shift] without a clamp (libc.c:666): it stays inside
    its array iff the last interior sample does -- the condition make_goldens.py asserts on its shapes."""
    _, _, n_win = tdt_sizes(n, half_window, shift)
    return n - shift - 1 < shift or (n - shift - 1) // shift <= n_win - 1


def _delay_the_jump(w, min_windows=2):
    """libc.c:631-651 on every row of w (rows, n_win), in place: three loops along the windows."""
    n_win = w.shape[1]
    if n_win < min_windows:
        return w
    d = w[:, 1:] - w[:, :-1]
    for q in range(1, n_win):
        neg = d[:, q - 1] < 0
        w[:, q] = np.where(neg, w[:, q] - d[:, q - 1], w[:, q])
        d[:, q - 1] = w[:, q] - w[:, q - 1]
    for q in range(n_win - 1):
        w[:, q] = np.where(d[:, q] > 0, w[:, q] + d[:, q], w[:, q])
    return w


def rms_window_of(n, shift, n_win):
    """Window of every sample (libc.c:656-667 with the clamp of tdt_window_of): the first `shift` samples take
    window 0, the samples from n - shift on the last one, the others min(i / shift, n_win - 1)."""
    i = np.arange(n)
    q = np.minimum(i // shift, n_win - 1)
    if n - shift >= 0:                                   # (size_t: n - shift wraps to a huge value otherwise)
        q[i >= n - shift] = n_win - 1
    q[i < shift] = 0
    return q


def mad_window_of(n, window, shift, n_win):
    """min(clamp(i, half, n - (window - half) - 1) / shift, n_win - 1)   (similarity_search.py:1100-1112)."""
    half = window // 2
    i = np.clip(np.arange(n), half, n - (window - half) - 1)
    return np.minimum(i // shift, n_win - 1)


def tdt_rms_parts(x, gauss, num_dev, half_window, shift):
    """Everything the definition computes, by name: centre, dev, raw (window values before the smoothing),
    thr_win, full."""
    x = np.atleast_2d(np.asarray(x, f32))
    rows, n = x.shape
    window, n_glob, n_win = tdt_sizes(n, half_window, shift)
    g = np.asarray(gauss, f32)[:GAUSS_LEN]
    with np.errstate(all="ignore"):
        G = x[:, :n_glob * window].reshape(rows, n_glob, window)
        part = np.zeros((rows, n_glob), f32)
        cnt = np.zeros((rows, n_glob), np.int64)
        for j in range(window):
            v = G[:, :, j]
            nz = v != 0
            part = np.where(nz, part + v, part)
            cnt += nz
        centre = np.zeros(rows, f32)
        for q in range(n_glob):
            centre = centre + part[:, q]
        total = cnt.sum(1).astype(f32)
        centre = centre / total
        part = np.zeros((rows, n_glob), f32)
        for j in range(window):
            v = G[:, :, j]
            d = (v - centre[:, None]).astype(f64)
            part = np.where(v != 0, (part.astype(f64) + d * d).astype(f32), part)
        dev = np.zeros(rows, f32)
        for q in range(n_glob):
            dev = dev + part[:, q]
        dev = np.sqrt(dev / total)
        fill = g[np.arange(n) % GAUSS_LEN][None, :] * dev[:, None]
        scratch = np.where(x == 0, centre[:, None] + fill, x)
        starts = np.arange(n_win) * shift
        acc = np.zeros((rows, n_win), f32)
        for j in range(window):
            acc = acc + scratch[:, starts + j]
        mean = acc / f32(window)
        ss = np.zeros((rows, n_win), f32)
        for j in range(window):
            d = (scratch[:, starts + j] - mean).astype(f64)
            ss = (ss.astype(f64) + d * d).astype(f32)
        raw = mean + f32(num_dev) * np.sqrt(ss / f32(window))
        thr_win = _delay_the_jump(raw.copy())
    assert raw.dtype == f32 and thr_win.dtype == f32 and centre.dtype == f32 and dev.dtype == f32
    full = thr_win[:, rms_window_of(n, shift, n_win)]
    return {"centre": centre, "dev": dev, "raw": raw, "thr_win": thr_win, "full": full}


def tdt_rms_definition(x, gauss, num_dev, half_window, shift):
    """(thr_win (rows, n_win), full (rows, n)) of the RMS threshold for every row of x."""
    p = tdt_rms_parts(x, gauss, num_dev, half_window, shift)
    return p["thr_win"], p["full"]


def _records(x, t):
    with np.errstate(invalid="ignore"):
        rr, ii = np.nonzero(x > t)
    out = np.zeros(rr.size, candidate_dtype)
    out["row"], out["index"], out["cc"], out["threshold"] = rr, ii, x[rr, ii], t[rr, ii]
    return out


def extract_definition(x, thr_windows, kind, window_or_half, shift, row_cap):
    """Records (row, index, cc, threshold) of every sample with cc > np.minimum(threshold, row_cap[row])
    (similarity_search.py:629 and :231-232; a NaN threshold stays NaN and nothing exceeds it), sorted by row and
    index.  kind "rms": window_or_half is the half window; "mad": the window."""
    x = np.atleast_2d(np.asarray(x, f32))
    tw = np.atleast_2d(np.asarray(thr_windows, f32))
    rows, n = x.shape
    n_win = tw.shape[1]
    if kind == "rms":
        assert tdt_sizes(n, window_or_half, shift)[2] == n_win
        w = rms_window_of(n, shift, n_win)
    else:
        assert (n - window_or_half) // shift + 1 == n_win
        w = mad_window_of(n, window_or_half, shift, n_win)
    cap = np.full(rows, np.inf, f32) if row_cap is None else np.asarray(row_cap, f32)
    with np.errstate(invalid="ignore"):
        t = np.minimum(tw[:, w], cap[:, None])
    return _records(x, t)


# ------------------------------------------------------------------------------------------------ mirrors ---
def _stream(flat, starts, window, drop, trace=None):
    """tdt_stream2 for the lanes whose windows start at flat[starts]: yields (values, j, use_g) in the order a lane
    accumulates them -- the value of every lane at sample j of its window, and whether the lane is on the replacement
    path `g`.  `slots` holds WHICH step each of the DEPTH register slots has loaded: a step accumulates what its slot
    holds, whatever that is, then reloads the slot with step b + DEPTH clamped to the last one."""
    nstep = window // STEP
    last = max(nstep - 1, 0)
    slots = [min(d, last) for d in range(DEPTH)] if nstep else []
    e32 = np.arange(STEP)

    def step(b, sl):
        vals = flat[starts[:, None] + (slots[sl] * STEP + e32)[None, :]]
        slots[sl] = min(b + DEPTH, last)
        lo = vals.min(1) if "zero_step_by_min_not_abs" in drop else np.abs(vals).min(1)
        use_g = lo == 0
        if trace is not None:
            trace.append((b, use_g))
        for e in range(STEP):
            yield vals[:, e], b * STEP + e, use_g

    b = 0
    while b + DEPTH <= nstep:
        for sl in range(DEPTH):
            yield from step(b + sl, sl)
        b += DEPTH
    if "remainder_steps_skipped" not in drop:
        for sl in range(DEPTH - 1):
            if b < nstep:
                yield from step(b, sl)
                b += 1
    if "clamped_reload_accumulated" in drop and nstep:
        assert all(s == last for s in slots) or "remainder_steps_skipped" in drop
        yield from step(last, 0)                         # the extra read of the last step is not dropped
    if "tail_dropped" not in drop:
        on_g = np.full(starts.size, "tail_not_replaced" not in drop)
        for j in range(nstep * STEP, window):
            yield flat[starts + j], j, on_g


def tdt_rms_mirror(x, gauss, num_dev, half_window, shift, drop=None, trace=None):
    """(thr_win, full) the way the seven kernels of bpmf_tdt_rms_dev compute them.  `trace`, a list, receives
    (step, use_g per lane) of the window kernel's first pass; lane = row * n_win + window."""
    drop = _drop(drop, TDT_DEFECTS)
    x = np.atleast_2d(np.asarray(x, f32))
    rows, n = x.shape
    window, n_glob, n_win = tdt_sizes(n, half_window, shift)
    g = np.asarray(gauss, f32)[:GAUSS_LEN]
    flat = x.ravel()
    offs = [q * window for q in range(n_glob)]
    if "glob_takes_remainder" in drop and n % window:
        offs.append(n - window)
    ng = len(offs)
    gstart = (np.arange(rows)[:, None] * n + np.array(offs, np.int64)[None, :]).ravel()
    grow = np.repeat(np.arange(rows), ng)
    with np.errstate(all="ignore"):
        # (1) tdt_glob_sum_kernel: zeros are added too (x + -0 = x), only the count tests
        acc = np.zeros(gstart.size, f32)
        cnt = np.zeros(gstart.size, np.int64)
        for v, _, _ in _stream(flat, gstart, window, drop):
            acc = acc + v
            cnt += 1 if "count_includes_zeros" in drop else (v != 0)
        # (2) tdt_glob_centre_kernel
        part, cnt = acc.reshape(rows, ng), cnt.reshape(rows, ng)
        centre = np.zeros(rows, f32)
        for q in range(ng):
            centre = centre + part[:, q]
        total = cnt.sum(1).astype(f32)
        centre = centre / total
        # (3) tdt_glob_dev_kernel
        acc = np.zeros(gstart.size, f32)
        c = centre[grow]
        for v, _, _ in _stream(flat, gstart, window, drop):
            d = (v - c).astype(f64)
            new = (acc.astype(f64) + d * d).astype(f32)
            acc = new if "dev_includes_zeros" in drop else np.where(v != 0, new, acc)
        # (4) tdt_glob_std_kernel
        part = acc.reshape(rows, ng)
        dev = np.zeros(rows, f32)
        for q in range(ng):
            dev = dev + part[:, q]
        dev = np.sqrt(dev / total)
        # (5) tdt_window_kernel: two passes, zeros replaced where they are read, on the path `g` only
        lane = np.arange(rows * n_win)
        row, q = lane // n_win, lane % n_win
        i0 = q * shift
        start = row * n + i0
        g0 = np.zeros_like(i0) if "gauss_without_g0" in drop else i0 % GAUSS_LEN
        c, dv = centre[row], dev[row]

        def filled(v, j, use_g):
            return np.where(use_g & (v == 0), c + g[(g0 + j) % GAUSS_LEN] * dv, v)

        acc = np.zeros(lane.size, f32)
        for v, j, use_g in _stream(flat, start, window, drop, trace):
            acc = acc + filled(v, j, use_g)
        mean = acc / f32(window)
        ss = np.zeros(lane.size, f32)
        for v, j, use_g in _stream(flat, start, window, drop):
            d = (filled(v, j, use_g) - mean).astype(f64)
            ss = (ss.astype(f64) + d * d).astype(f32)
        thr_win = (mean + f32(num_dev) * np.sqrt(ss / f32(window))).reshape(rows, n_win)
        # (6) tdt_smooth_kernel
        thr_win = _delay_the_jump(thr_win, 3 if "smooth_skipped_below_3_windows" in drop else 2)
    assert thr_win.dtype == f32
    # (7) tdt_expand_kernel (tdt_window_of); one float past the end stands for whatever lies behind the array
    i = np.arange(n)
    wq = i // shift if "expand_unclamped" in drop else np.minimum(i // shift, n_win - 1)
    head = i < shift
    tail = (i > n - shift if "expand_tail_gt" in drop else i >= n - shift) if n - shift >= 0 else np.zeros(n, bool)
    wq = np.where(head, 0, np.where(tail, n_win - 1, wq))
    behind = np.concatenate([thr_win.ravel(), np.full(n, np.nan, f32)])
    full = behind[np.arange(rows)[:, None] * n_win + wq[None, :]]
    return thr_win, full


def extract_mirror(x, thr_windows, kind, window_or_half, shift, row_cap, drop=None, capacity=1 << 20):
    """The records of cand_extract_kernel behind its two entry points and the regrowing loop of
    ThresholdGPU.extract_candidates: groups of four samples, the window looked up at both ends of a group and per
    sample only where the ends differ, head and tail regions from the entry point's four numbers."""
    drop = _drop(drop, EXTRACT_DEFECTS)
    x = np.atleast_2d(np.asarray(x, f32))
    tw = np.atleast_2d(np.asarray(thr_windows, f32))
    rows, n = x.shape
    n_win = tw.shape[1]
    u32 = 0xFFFFFFFF
    if kind == "rms":
        head_len, head_win, tail_start, tail_win = shift, 0, (n - shift) & u32, n_win - 1
    else:
        half = window_or_half // 2
        tail_start = n - (window_or_half - half)
        head_len, head_win = half, min(half // shift, n_win - 1)
        tail_win = min((tail_start - 1) // shift, n_win - 1)
        if "mad_head_window_zero" in drop:
            head_win = 0

    def window_of(i):
        return np.where(i < head_len, head_win, np.where(i >= tail_start, tail_win, np.minimum(i // shift, n_win - 1)))

    i = np.arange(n)
    i0 = i // 4 * 4
    cnt = np.minimum(n - i0, 4)
    w_first, w_last = window_of(i0), window_of(i0 + cnt - 1)
    w = w_first if "group_window_from_first_only" in drop else np.where(w_first == w_last, w_first, window_of(i))
    cap = np.full(rows, np.inf, f32) if row_cap is None or "cap_ignored" in drop else np.asarray(row_cap, f32)
    th = tw[:, w]
    with np.errstate(invalid="ignore"):
        t = np.fmin(cap[:, None], th)
        if "nan_threshold_falls_to_cap" not in drop:
            t = np.where(np.isnan(th), th, t)
        hit = (x >= t) if "ge_instead_of_gt" in drop else (x > t)
    if "group_tail_dropped" in drop:
        hit &= (cnt == 4)[None, :]
    rr, ii = np.nonzero(hit)
    while rr.size > capacity:                            # count > capacity: the buffer is regrown, the call repeated
        capacity = rr.size
    out = np.zeros(rr.size, candidate_dtype)
    out["row"], out["index"], out["cc"], out["threshold"] = rr, ii, x[rr, ii], t[rr, ii]
    return out


# --------------------------------------------------------------------------------------------- case table ---
@dataclass
class TdtCase:
    name: str
    x: np.ndarray
    half: int
    shift: int
    gauss: np.ndarray
    num_dev: float = 8.0
    group: str = "stream"
    zero_row: int = None          # zero cases: the row that holds the planted zeros
    expect: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.x.shape[1]

    @property
    def rows(self):
        return self.x.shape[0]

    @property
    def sizes(self):
        return tdt_sizes(self.n, self.half, self.shift)

    @property
    def in_bounds(self):
        return reference_in_bounds(self.n, self.half, self.shift)


STREAM_WINDOWS = (2, 30, 32, 34, 62, 64, 160, 190, 192, 194, 224, 352, 384, 386, 416, 418)


def stream_shifts(window):
    """1, window, window + 1, an odd shift near 3/4 window, a shift = 2 mod 4 near half a window."""
    two_mod_4 = max(2, (window // 2 - 2) // 4 * 4 + 2)
    return sorted({1, window, window + 1, (3 * window // 4) | 1, two_mod_4})


def live_rows(seed, rows, n, zeros=True):
    """CC-like rows: small values of both signs, a few spikes, and (zeros=True) exact zeros of both signs sprinkled
    over ~3 % of the samples so that the replacement path runs in most windows."""
    x = noise(seed, (rows, n)) * f32(0.05)
    pick = noise(seed + 7919, (rows, n))
    x[pick > f32(0.93)] += f32(0.6)
    if zeros:
        x[np.abs(pick) < f32(0.012)] = 0.0
        x[(pick > f32(0.3)) & (pick < f32(0.303))] = -0.0
        x[:, n // 3], x[:, 2 * n // 3] = 0.0, -0.0          # (at least one of each in every row, however short)
    return x.astype(f32)


def _stream_cases():
    out = []
    for window in STREAM_WINDOWS:
        n = 3 * window + 5                               # odd: four rows start at the four alignments of a dword
        for shift in stream_shifts(window):
            seed = 1000 * window + shift
            out.append(TdtCase(f"stream_w{window}_s{shift}", live_rows(seed, 4, n), window // 2, shift,
                               gauss_sample(seed)))
    return out


def _lane_cases():
    out = []
    window = 34
    for total, rows in ((1, 1), (63, 7), (64, 8), (65, 5), (127, 1), (128, 8), (129, 3)):
        n_glob = total // rows                           # shift = window: n_win = n_glob, both products hit `total`
        n = n_glob * window + 5
        c = TdtCase(f"lanes_{total}_as_{rows}x{n_glob}", live_rows(50_000 + total, rows, n), window // 2, window,
                    gauss_sample(total), group="lanes")
        assert c.sizes == (window, n_glob, n_glob)
        out.append(c)
    for total, rows, shift in ((63, 3, 5), (64, 2, 5), (65, 1, 3), (129, 3, 1)):   # n_win apart from n_glob
        n_win = total // rows
        n = window - shift + n_win * shift
        c = TdtCase(f"lanes_win_{total}_as_{rows}x{n_win}_s{shift}", live_rows(51_000 + total, rows, n), window // 2,
                    shift, gauss_sample(total + 1), group="lanes")
        assert c.sizes[2] == n_win
        out.append(c)
    return out


ZW, ZN = 98, 743                                         # zero cases: 3 steps + a tail of 2; 7 windows + 57 samples


def _zero_case(name, shift, place, expect, seed):
    """Three rows: live, the row `place` plants zeros in (no other zero in it), live.  The middle row has no spikes,
    and the window named in `expect` is four times as loud as the others: its value is a local maximum, which the
    smoothing leaves as it is (a window below its neighbours takes THEIR value and would hide what happened in it)."""
    x = live_rows(60_000 + seed, 3, ZN, zeros=False)
    x[1] = noise(61_000 + seed, ZN) * f32(0.05)
    if "window" in expect:
        x[1, expect["window"] * ZW:(expect["window"] + 1) * ZW] *= f32(4.0)
    for r in (0, 2, 1):
        x[r][x[r] == 0] = f32(0.01)
    place(x[1])
    return TdtCase("zero_" + name, x, ZW // 2, shift, gauss_sample(600 + seed), group="zeros", zero_row=1,
                   expect=expect)


def _zero_cases():
    def at(*idx, value=0.0):
        def place(r):
            r[list(idx)] = value
        return place

    def negative_step(r):
        r[2 * ZW + 32:2 * ZW + 64] = -np.abs(r[2 * ZW + 32:2 * ZW + 64]) - f32(1e-3)
        r[2 * ZW + 40] = 0.0

    def run(a, b):
        def place(r):
            r[a:b] = 0.0
        return place

    W = ZW
    out = [
        # shift = window: sample i is sample i % W of window i // W, and of no other
        _zero_case("step_first", W, at(W + 32), {"window": 1, "j": 32, "step": 1}, 1),
        _zero_case("step_last", W, at(W + 63), {"window": 1, "j": 63, "step": 1}, 2),
        _zero_case("tail_first", W, at(W + 96), {"window": 1, "j": 96, "tail": True}, 3),
        _zero_case("tail_last", W, at(W + 97), {"window": 1, "j": 97, "tail": True}, 4),
        # window 5 starts at 490 (i0 % 500 = 490): its samples 9 and 10 take gauss[499] and gauss[0]
        _zero_case("gauss_index_499", W, at(499), {"window": 5, "j": 9, "step": 0, "gauss": 499}, 5),
        _zero_case("gauss_index_0", W, at(500), {"window": 5, "j": 10, "step": 0, "gauss": 0}, 6),
        _zero_case("negative_zero", W, at(3 * W + 17, value=-0.0), {"window": 3, "j": 17, "step": 0, "negative": True}, 7),
        _zero_case("in_negative_step", W, negative_step, {"window": 2, "j": 40, "step": 1, "negative_step": True}, 8),
        _zero_case("one_lane", W, at(4 * W + 5), {"window": 4, "j": 5, "step": 0, "lanes": 1}, 9),
        # shift = 49: sliding window 3 is [147, 245), global window 2 is [196, 294)
        _zero_case("run_over_a_sliding_window", 49, run(147, 245), {"all_zero_sliding": 3}, 10),
        _zero_case("run_over_a_global_window", 49, run(196, 294), {"all_zero_global": 2}, 11),
        _zero_case("only_in_the_remainder", 49, run(7 * W, ZN), {"remainder_only": True}, 12),
        # shift = 1: row 1 starts at lane 646; the wave of lanes 704 .. 767 holds its windows 58 .. 121, which all
        # hold sample 130
        _zero_case("all_64_lanes", 1, at(130), {"wave": 11, "lanes": 64}, 13),
        _zero_case("row_between_live_rows", 49, run(0, ZN), {"nan_row": True}, 14),
        _zero_case("live_only_in_the_remainder", 49, run(0, 7 * W), {"nan_row": True}, 15),
    ]
    return out


SMOOTH_PATTERNS = ("rise", "fall", "alternate", "plateau")


def _smooth_cases():
    """Rows whose amplitude is scaled per window (shift = window = 34) so that the raw window values rise, fall,
    alternate or repeat exactly (every window of the plateau row holds the same 34 samples)."""
    out = []
    window = 34
    for n_win in (1, 2, 3, 8):
        n = n_win * window + 3
        base = noise(70_000 + n_win, (4, n)) * f32(0.05)   # no spikes: the scale alone orders the window values
        q = np.minimum(np.arange(n) // window, n_win - 1)
        scale = {"rise": 2.0 ** q, "fall": 2.0 ** (n_win - 1 - q), "alternate": 1.0 + 2.0 * (q % 2),
                 "plateau": np.where((q >= (n_win + 1) // 2) & (n_win > 2), 2.0, 1.0)}
        x = np.stack([base[r] * scale[p].astype(f32) for r, p in enumerate(SMOOTH_PATTERNS)])
        pattern = np.tile(base[3, :window], n_win + 1)[:n]
        x[3] = pattern * scale["plateau"].astype(f32)    # x 2: exact, the two plateaus are flat bit for bit
        out.append(TdtCase(f"smooth_{n_win}_windows", x.astype(f32), window // 2, window, gauss_sample(70 + n_win),
                           group="smooth"))
    return out


def smooth_pattern_holds(case):
    """The intended sign pattern of the raw window values' differences, on the definition."""
    raw = tdt_rms_parts(case.x, case.gauss, case.num_dev, case.half, case.shift)["raw"]
    d = np.diff(raw, axis=1)
    sign = np.sign(d)
    n_win = raw.shape[1]
    if n_win == 1:
        return d.size == 0
    alt = np.all(sign[2, 1:] == -sign[2, :-1]) and np.all(sign[2] != 0)
    flat = np.count_nonzero(d[3] == 0) == n_win - 1 - (n_win > 2)        # one step up between two plateaus
    return bool(np.all(d[0] > 0) and np.all(d[1] < 0) and alt and flat)


def _expand_cases():
    mk = lambda name, n, half, shift, seed: TdtCase(name, live_rows(80_000 + seed, 3, n), half, shift,  # noqa: E731
                                                    gauss_sample(80 + seed), group="expand")
    out = [mk("expand_clamp_acts", 100, 17, 5, 1),                  # n_win 14, (n - shift - 1) / shift = 18
           mk("expand_clamp_acts_by_one", 106, 17, 12, 2),         # n_win 7, samples 84 .. 93 have i / shift = 7
           mk("expand_clamp_idle", 107, 17, 34, 3),
           mk("expand_n_minus_shift_below_shift", 69, 17, 35, 4),  # n_win 2; sample 34 is head AND tail: head wins
           mk("expand_one_window_n_equals_window", 34, 17, 35, 5),  # n - shift wraps
           # shift = window + 1 and n + 1 a multiple of it: the one family in which sample n - shift (69) does not
           # have the last window as its i / shift already -- the tail test decides
           mk("expand_tail_decides", 104, 17, 35, 6)]
    assert out[5].sizes[2] == 3 and (out[5].n - 35) // 35 == 1
    assert not out[0].in_bounds and not out[1].in_bounds and (out[1].n - 13) // 12 == out[1].sizes[2]
    assert out[2].in_bounds and out[3].in_bounds and out[4].in_bounds
    assert out[3].sizes[2] == 2 and out[3].n - out[3].shift < out[3].shift
    return out


OVERLAP_CASES = ((35, 0.0), (64, 0.25), (194, 0.66), (100, 0.5), (386, 0.9))   # (sliding_window_samp, overlap)


@functools.lru_cache(maxsize=None)
def tdt_cases():
    cases = _stream_cases() + _lane_cases() + _zero_cases() + _smooth_cases() + _expand_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        c.x.setflags(write=False)
        assert c.x.dtype == f32 and c.sizes is not None, c.name
    return tuple(cases)


def tdt_case(name):
    return next(c for c in tdt_cases() if c.name == name)


@dataclass
class ExtractCase:
    name: str
    kind: str                    # "rms" / "mad"
    x: np.ndarray
    thr: np.ndarray              # (rows, n_win) synthetic window values, all distinct
    window: int                  # the sliding window (rms: 2 * half)
    shift: int
    row_cap: np.ndarray = None
    probes: list = field(default_factory=list)   # (row, index, "eq" / "ulp"): samples set on / one ulp above

    @property
    def window_or_half(self):
        return self.window // 2 if self.kind == "rms" else self.window

    @property
    def n_win(self):
        return self.thr.shape[1]


def extract_n_win(kind, n, window, shift):
    return tdt_sizes(n, window // 2, shift)[2] if kind == "rms" else (n - window) // shift + 1


def make_extract_case(name, kind, n, window, shift, caps="mixed", sprinkle=True, nan_row=None, rows=4, seed=0,
                      probe=True):
    n_win = extract_n_win(kind, n, window, shift)
    thr = (f32(0.5) + f32(2.0 ** -12) * np.arange(rows * n_win, dtype=f32)).reshape(rows, n_win)   # exact, distinct
    assert np.unique(thr).size == thr.size
    wof = rms_window_of(n, shift, n_win) if kind == "rms" else mad_window_of(n, window, shift, n_win)
    x = np.full((rows, n), -1.0, f32)
    if sprinkle:
        pick = noise(90_000 + seed, (rows, n))
        x = np.where(pick > f32(0.9), thr[:, wof] * (f32(1.0) + pick - f32(0.93)), x).astype(f32)
    cap = None
    if caps == "mixed":      # below every threshold, equal to the threshold of an interior window, above, +inf
        cap = np.array([0.25, thr[1 % rows, n_win // 2], 10.0, np.inf][:rows], f32)
    if nan_row is not None:
        thr[nan_row] = np.nan
    # samples exactly on the threshold and one ulp above it: first and last sample of the head region, of the tail
    # region and of an interior window (where the regions are empty or coincide the probes coincide too)
    if kind == "rms":
        head_end, tail_start = min(shift, n), max(n - shift, 0)
    else:
        head_end, tail_start = window // 2, n - (window - window // 2)
    mid = (n // 2) // shift * shift
    places = sorted({0, head_end - 1, head_end, tail_start - 1, tail_start, n - 1, mid, min(mid + shift - 1, n - 1)})
    probes = []
    for r in range(rows):
        for k, i in enumerate(p for p in places if 0 <= p < n and probe):
            how = ("eq", "ulp")[(k + r) % 2]
            t = thr[r, wof[i]] if cap is None else np.minimum(thr[r, wof[i]], cap[r])
            if np.isfinite(t):
                x[r, i] = t if how == "eq" else np.nextafter(t, f32(np.inf))
                probes.append((r, i, how))
    return ExtractCase(name, kind, x, thr, window, shift, cap, probes)


EXTRACT_N = (40, 41, 42, 43, 4095, 4096, 4097, 8193)
EXTRACT_SHIFTS = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def extract_cases():
    out = []
    for kind, window in (("rms", 6), ("mad", 7)):
        for n in EXTRACT_N:
            for shift in EXTRACT_SHIFTS:
                out.append(make_extract_case(f"extract_{kind}_n{n}_s{shift}", kind, n, window, shift, seed=n + shift))
        out += [
            make_extract_case(f"extract_{kind}_wide_window", kind, 4097, 34 + (kind == "mad"), 5, seed=1),
            make_extract_case(f"extract_{kind}_shift_is_window_plus_1" if kind == "rms" else f"extract_{kind}_shift_is_window",
                              kind, 4099, 34 + (kind == "mad"), 35, seed=2),
            make_extract_case(f"extract_{kind}_no_cap", kind, 4097, window, 3, caps=None, seed=3),
            make_extract_case(f"extract_{kind}_nothing_above", kind, 4097, window, 3, caps=None, sprinkle=False, probe=False,
                              seed=4),
            make_extract_case(f"extract_{kind}_nan_threshold_row", kind, 4097, window, 3, nan_row=0, seed=5),
        ]
    out.append(make_extract_case("extract_rms_n_equals_window", "rms", 34, 34, 35, seed=6))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        c.x.setflags(write=False)
        c.thr.setflags(write=False)
    return tuple(out)


def extract_case(name):
    return next(c for c in extract_cases() if c.name == name)


# (name, n_rows, n, half_window, shift, expand, short_workspace): every one returns -1 with a message and writes nothing
TDT_REFUSALS = (
    ("n_below_window", 2, 33, 17, 5, True, False),
    ("shift_zero", 2, 100, 17, 0, True, False),
    ("shift_above_window_plus_1", 2, 100, 17, 36, True, False),
    ("zero_rows", 0, 100, 17, 5, True, False),
    ("workspace_too_small", 2, 100, 17, 5, True, True),
    ("65536_rows_expanded", ROW_LIMIT + 1, 64, 17, 5, True, False),
)
# (name, kind, n_rows, n, window, shift)
EXTRACT_REFUSALS = (
    ("rms_65536_rows", "rms", ROW_LIMIT + 1, 64, 34, 5),
    ("mad_65536_rows", "mad", ROW_LIMIT + 1, 64, 35, 5),
    ("rms_zero_rows", "rms", 0, 64, 34, 5),
    ("mad_zero_rows", "mad", 0, 64, 35, 5),
    ("rms_n_below_window", "rms", 2, 33, 34, 5),
    ("mad_n_below_window", "mad", 2, 34, 35, 5),
    ("rms_shift_zero", "rms", 2, 64, 34, 0),
    ("mad_shift_zero", "mad", 2, 64, 35, 0),
)


def same_bits(a, b):
    """Bit equality of two float32 arrays (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_values(a, b):
    """Equality of the values, NaN equal to NaN (what a comparison across compilers can ask of a NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_records(a, b):
    return a.shape == b.shape and all(same_values(a[k], b[k]) for k in candidate_dtype.names)
