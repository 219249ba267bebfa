"""Non-finite samples in the matched filter: the written rule, the cases and the checkers (TEST INFRASTRUCTURE, pure
NumPy; shared by tests/test_nonfinite_host.py on the CPU and tests/test_gpu_mf_nonfinite.py on the device).

The data are whatever the network recorded: a NaN-filled gap or a clipped +-Inf is ordinary input, and the caller only
scrubs NaN from the RESULT (similarity_search.py:540).  DESIGN.md s3 states per path what one bad sample may cost; this
module is that statement in NumPy.

THE RULE (short mode, the oracle's conventions).  The window norm comes from a double prefix sum of data^2, so a NaN or
+-Inf sample at index p of a channel makes csum[k] non-finite for every k > p.  Per (template, lag, station, component)
inside the template's valid lag range, with the window [j, j + L), j = lag * step + moveout:

    CLEAN       the window ends before the channel's first bad sample, by more than R samples: the bits of the cleaned day
    NEAR        the window ends within R samples before a bad sample: the oracle's value (= the cleaned day's), or NaN in a
                kernel whose K range runs R samples past the window and multiplies band zeros with the bad sample
    TOUCH_NAN   the window holds a NaN and does not start behind the first NaN / Inf: E_d = NaN, the guard fails, cc = +0
    TOUCH_INF   ... holds +-Inf and no NaN: E_d = Inf, r_d = 0, cc = num * 0 = NaN
    TOUCH_BIG   ... holds a finite sample whose square overflows float32 (3e38) and nothing worse: (float)E_d = Inf,
                r_d = 0, cc = num * 0: 0, or NaN where the numerator overflowed
    AFTER       the window starts behind the first NaN / Inf: csum[j] is non-finite, E_d = NaN (Inf - Inf, NaN - x): cc = +0
    AFTER_BIG   the window starts behind a BIG sample (and no NaN / Inf): both prefix values carry 9e76 and their
                difference is 0 or a multiple of its ulp, (float)E_d is 0 or Inf: cc = 0 (of either sign)
    DEAD_T_NAN  the template channel holds a NaN: r_t = NaN, the guard fails, cc = +0 at every lag
    DEAD_T_INF  the template channel holds +-Inf and no NaN: r_t = 0, cc = num * 0 = NaN wherever the window norm is a
                finite number, 0 elsewhere.  (Not 0: only a NaN norm fails the guard.  Judged by NaN-ness against the oracle.)
    OFF         outside the valid lag range, or a zero-weight channel: nothing is computed, exactly 0

Under mf.compat_sqrt_norm the same classes hold with E_t * E_d > 1e-6 as the guard (NaN fails it; num / sqrtf(Inf) is
NaN or 0 exactly where num * 0 is).  In FULL mode (mf_full_definition) E_c = Q - P P / L is NaN for a window that holds
+-Inf as well (Inf - Inf), and t - tbar is NaN for a template channel that holds one: every class but CLEAN / NEAR /
TOUCH_BIG is exactly 0 there.

R, THE REACH, per family -- derived from the tile algebra (DESIGN.md s3 repeats the derivations), never measured:
    direct        0: one thread per lag reads its own window.
    fp32 MFMA     (mf_mfma_wave_kernel at 1, 2 and 4 tiles per wave, four-phase window included, and mf_mfma_kernel): band
                  row b of a 16-lag tile multiplies tmpl[m - b] with window sample m for EVERY m in [0, Kpad), Kpad =
                  16 ceil((L + 15) / 16) (mf_kpad: the K loop runs whole trips of 16); the lag's own window is m in
                  [b, b + L), so the zeros of the band meet the b samples in front of it (those windows start behind the bad
                  sample: AFTER, 0 by the guard) and the Kpad - L - b samples behind it:  R = Kpad - L, 15 .. 30.
    split16       row b of a 32-lag tile and the moveout's remainder r = moveout mod 8 (the window starts on a multiple of
                  8): segment g multiplies tmpl[g seg + m - b - r] with sample m of its window for m in [0, 16 nks),
                  nks = nks_of(seg); the last segment ends 16 nks + (n_seg - 1) seg - L - b - r samples behind the window:
                  R = 16 nks_of(seg) + (n_seg - 1) seg - L - r, per template channel: 40 - r at L = 200 and 400,
                  64 - r at L = 800 (seg = 272).
"""
import functools

import numpy as np

import f64_anchor as fa

OFF, CLEAN, NEAR, TOUCH_NAN, TOUCH_INF, TOUCH_BIG, AFTER, AFTER_BIG, DEAD_T_NAN, DEAD_T_INF = range(10)
CLASS_NAMES = ("OFF", "CLEAN", "NEAR", "TOUCH_NAN", "TOUCH_INF", "TOUCH_BIG", "AFTER", "AFTER_BIG", "DEAD_T_NAN", "DEAD_T_INF")
ZERO_CLASSES = (OFF, TOUCH_NAN, AFTER, AFTER_BIG, DEAD_T_NAN)          # exactly 0 in short mode
ZERO_CLASSES_FULL = ZERO_CLASSES + (TOUCH_INF, DEAD_T_INF)              # ... and in full mode

TOL_CC = 2e-5                      # the bar of tests/test_gpu_split16.py, per unit of sum |w|
BIG = np.float32(3e38)
BIG_MIN = 2.0 ** 64                # |x| >= this: x^2 overflows float32
R_LIMIT = 64                       # premise: R < 64 for every family ...
MIN_LAGS = 2000                    # ... and at least 2000 valid lags per template: the excepted lags stay under 4 %
AMPLITUDES = (1.0, 3.0e5, 1.0e-9)  # per channel: unit noise, counts, and what fp16 flushes to zero
N_DEFAULT = 9000
FAMILIES = ("direct", "mfma", "split")


# ------------------------------------------------------------------------------------------------ reach ---
def mf_kpad(L):
    return (L + 15 + 15) // 16 * 16


def split_geometry(L):
    """(n_seg, seg_len, nks) of mf_split.h: n_segments_of, segment_len_of, nks_of(seg_len)."""
    max_seg = (16 * 26 - 38) // 8 * 8
    n_seg = (L + max_seg - 1) // max_seg
    seg = ((L + n_seg - 1) // n_seg + 7) // 8 * 8
    return n_seg, seg, (seg + 38 + 15) // 16


def reach(family, L, moveouts=None):
    """R of a family at template length L: a number, or (T, S, C) for "split" when the moveouts are given (R depends on
    moveout mod 8 there; without them the largest, r = 0)."""
    assert family in FAMILIES
    if family == "direct":
        return 0
    if family == "mfma":
        return mf_kpad(L) - L
    n_seg, seg, nks = split_geometry(L)
    base = 16 * nks + (n_seg - 1) * seg - L
    return base if moveouts is None else base - np.mod(np.asarray(moveouts, dtype=np.int64), 8)


# ------------------------------------------------------------------------------------------------- rule ---
def bad_mask(x):
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(x) | (np.abs(x) >= BIG_MIN)


def classify(data, moveouts, L, step, n_corr, weights=None, templates=None, R=0):
    """The class of every (t, lag, s, c): int8 (T, n_corr, S, C).  R: a number or (T, S, C)."""
    data = np.asarray(data, dtype=np.float32)
    S, C, N = data.shape
    mv = np.asarray(moveouts, dtype=np.int64)
    T = mv.shape[0]
    mv = np.broadcast_to(mv.reshape(T, S, -1), (T, S, C))
    w = np.ones((T, S, C)) if weights is None else np.broadcast_to(np.asarray(weights, np.float64).reshape(T, S, -1), (T, S, C))
    Rr = np.broadcast_to(np.asarray(R, dtype=np.int64), (T, S, C))
    out = np.full((T, n_corr, S, C), OFF, dtype=np.int8)
    lags = np.arange(n_corr, dtype=np.int64)
    for s in range(S):
        for c in range(C):
            x = data[s, c]
            is_nan, is_inf = np.isnan(x), np.isinf(x)
            with np.errstate(invalid="ignore"):
                is_big = np.isfinite(x) & (np.abs(x) >= BIG_MIN)
            cn, ci, cb = (np.concatenate([[0], np.cumsum(m)]) for m in (is_nan, is_inf, is_big))
            hard = np.flatnonzero(is_nan | is_inf)
            p0 = int(hard[0]) if hard.size else N                     # the first NaN / Inf: csum is non-finite behind it
            bigs = np.flatnonzero(is_big)
            pb = int(bigs[0]) if bigs.size else N
            first_bad = min(p0, pb)
            for t in range(T):
                if w[t, s, c] == 0:
                    continue
                rng_t = fa.mf_lag_range(mv[t], w[t], N, L, step)
                if rng_t is None:
                    continue
                sel = lags[rng_t[0]:rng_t[1] + 1]
                j = sel * step + mv[t, s, c]
                assert j.min() >= 0 and j.max() + L <= N
                n_nan, n_inf, n_big = cn[j + L] - cn[j], ci[j + L] - ci[j], cb[j + L] - cb[j]
                gap = first_bad - (j + L - 1)                          # samples from the window's last to the first bad one
                cls = np.where(gap > Rr[t, s, c], CLEAN, NEAR)
                cls = np.where(j > pb, AFTER_BIG, cls)
                cls = np.where(n_big > 0, TOUCH_BIG, cls)
                cls = np.where(n_inf > 0, TOUCH_INF, cls)
                cls = np.where(n_nan > 0, TOUCH_NAN, cls)
                cls = np.where(j > p0, AFTER, cls)
                if templates is not None:
                    tc = np.asarray(templates)[t, s, c]
                    if np.isnan(tc).any():
                        cls[:] = DEAD_T_NAN
                    elif np.isinf(tc).any():
                        cls[:] = DEAD_T_INF
                out[t, sel, s, c] = cls
    return out


# ------------------------------------------------------------------------------------------------ cases ---
class Case:
    """name, templates, moveouts, weights, data (poisoned), L, N, step, bad: ((s, c, index, value), ...) of the data,
    bad_t: ((t, s, c, index, value), ...) of the templates, exact_only: holds a 3e38 (the exact families only)."""

    def __init__(self, name, tp, mv, w, d, step, bad, bad_t=()):
        self.name, self.tp, self.mv, self.w, self.step = name, tp, mv, w, step
        self.bad, self.bad_t = tuple(bad), tuple(bad_t)
        self.L, self.N = tp.shape[-1], d.shape[-1]
        self.n_corr = (self.N - self.L) // step + 1
        self.clean_data = d
        self.data = d.copy()
        for s, c, i, v in self.bad:
            self.data[s, c, i] = v
        for t, s, c, i, v in self.bad_t:
            self.tp[t, s, c, i] = v
        self.exact_only = any(np.isfinite(v) for _, _, _, v in self.bad)
        self.clean_data.setflags(write=False)
        self.data.setflags(write=False)
        self.tp.setflags(write=False)

    @property
    def args(self):
        return self.tp, self.mv, self.w, self.data

    def classes(self, R=0):
        return classify(self.data, self.mv, self.L, self.step, self.n_corr, self.w, self.tp, R)

    def valid_lags(self):
        out = []
        for t in range(self.tp.shape[0]):
            r = fa.mf_lag_range(self.mv[t], self.w[t], self.N, self.L, self.step)
            out.append(0 if r is None else r[1] - r[0] + 1)
        return out


def cleaned(case):
    """The same case with every bad DATA sample replaced by +0.0 (a bad template sample stays)."""
    d = case.data.copy()
    d[bad_mask(d)] = 0.0
    out = Case.__new__(Case)
    out.__dict__.update(case.__dict__)
    out.name, out.data, out.bad = case.name + " (cleaned)", d, ()
    d.setflags(write=False)
    return out


def _base(seed, T, L, N, step, S=3, C=3):
    """Finite inputs: per-channel amplitudes 1 / 3e5 / 1e-9 (templates scaled the other way, so that E_t E_d stays
    far above the guard), signed moveouts whose remainders mod 8 differ, station 0 dead (zero weights), a zero gap of 3 L
    samples on channel (S - 1, 0)."""
    rng = np.random.default_rng(seed)
    amp = np.array([[AMPLITUDES[(s + c) % 3] for c in range(C)] for s in range(S)])
    d = rng.standard_normal((S, C, N)) * amp[:, :, None]
    tp = rng.standard_normal((T, S, C, L)) / amp[None, :, :, None]
    mv = rng.integers(-70, 401, (T, S, C))
    if reach("split", L) >= R_LIMIT:
        # three segments of 272 at L = 800: R = 64 - (moveout mod 8).  The premise R < 64 holds for every remainder but
        # 0, which these moveouts avoid (every remainder, 0 included, occurs at L = 200 and 400, where R <= 40)
        mv[mv % 8 == 0] += 1
    w = rng.uniform(0.1, 1.0, (T, S, C))
    w[:, 0, :] = 0.0
    g0 = N // 3
    d[S - 1, 0, g0:g0 + 3 * L] = 0.0
    return tp.astype(np.float32), mv.astype(np.int32), w.astype(np.float32), d.astype(np.float32), g0


NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)


@functools.lru_cache(maxsize=None)
def cases(L, step, T=2, N=None, big=True, align=True):
    """Every case at template length L and this step: seeded, regenerated on first use, read-only afterwards.
    Channels (station, component) and their amplitudes: (1,0) counts, (1,1) 1e-9, (1,2) unit, (2,0) 1e-9 with the
    gap, (2,1) unit, (2,2) counts; station 0 is dead."""
    N = N or max(N_DEFAULT, L + 7200)
    out = []

    def add(name, bad, bad_t=(), seed=0):
        tp, mv, w, d, _ = _base(91_000 + 7 * L + step + seed, T, L, N, step)
        out.append(Case(f"{name} L={L} step={step}", tp, mv, w, d, step, bad, bad_t))

    mid = N // 2
    g0 = N // 3
    add("one NaN mid-day, counts", [(1, 0, mid, NAN)])
    add("one NaN mid-day, 1e-9", [(1, 1, mid + 1, NAN)])
    add("+Inf, -Inf and NaN in three channels", [(1, 2, mid + 2, PINF), (2, 2, mid + 3, NINF), (2, 1, mid - 300, NAN)])
    if big:
        add("3e38 alone in its channel", [(2, 1, mid + 4, BIG), (1, 0, mid + 700, -BIG)])
    if align:
        for k in range(16):                              # every alignment inside a 16-lag tile
            add(f"NaN at {mid + 100 + k} (alignment {k})", [(1, 0, mid + 100 + k, NAN), (2, 1, mid + 116 + k, PINF)], seed=k)
    add("index 0: a dead channel", [(1, 0, 0, NAN), (2, 2, 0, PINF)])
    add("index N - 1", [(1, 2, N - 1, NAN), (2, 1, N - 1, PINF), (1, 1, N - 1, NINF)])
    add("NaN inside the zero gap", [(2, 0, g0 + L, NAN)])
    add("Inf inside the zero gap", [(2, 0, g0 + L + 5, PINF)])
    add("the prefix-sum chunk seam, 1023", [(1, 0, 1023, NAN), (1, 2, 1023, PINF)])
    add("the prefix-sum chunk seam, 1024", [(1, 0, 1024, NAN), (2, 2, 1024, NINF)])
    add("two kinds in one channel", [(1, 0, mid - 1500, PINF), (1, 0, mid + 1500, NAN),      # Inf, then NaN far behind
                                     (2, 1, mid - 1000, NAN), (2, 1, mid - 900, NINF),       # NaN, then Inf
                                     (1, 2, mid, PINF), (1, 2, mid + 10, NAN)])              # Inf and NaN in one window
    add("two channels of one station", [(1, 0, mid - 500, NAN), (1, 1, mid - 400, PINF)])
    add("NaN and Inf in template channels", [(2, 2, mid, NAN)],
        bad_t=[(0, 1, 0, L // 2, NAN), (T - 1, 2, 1, min(3, L - 1), PINF)])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def full_seam_case():
    """Full mode's partial sums of the channel constant: 65 536 samples each."""
    tp, mv, w, d, _ = _base(65_536, 1, 64, 70_000, 1)
    return Case("SUM_PART seam N=70000 L=64", tp, mv, w, d, 1,
                [(1, 0, 65_535, NAN), (1, 2, 65_536, NAN), (2, 1, 65_535, PINF), (2, 2, 65_536, NINF)])


# --------------------------------------------------------------------------------------------- checkers ---
def _first(mask, case_name, classes, got, want, why):
    i = tuple(int(x) for x in np.argwhere(mask)[0])
    if len(i) == 4:
        t, lag, s, c = i
        return (f"{case_name}: {why}: template {t}, channel ({s}, {c}), lag {lag}, class {CLASS_NAMES[classes[i]]}: "
                f"got {got[i]!r}, want {want[i]!r} ({int(mask.sum())} entries)")
    t, lag = i
    cl = sorted({CLASS_NAMES[k] for k in np.unique(classes[t, lag])})
    return (f"{case_name}: {why}: template {t}, lag {lag}, channel classes {cl}: got {got[i]!r}, want {want[i]!r} "
            f"({int(mask.sum())} lags)")


def _same(a, b):
    """Equal as np.array_equal(..., equal_nan=True) judges it, element by element: NaN-ness, not payload."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _network(classes):
    return classes.ndim == 4


def check_exact(got, want, classes, R, what=""):
    """A bit-exact family against the oracle on the poisoned day.  Outside NEAR equality (NaN-ness compared); inside
    NEAR the oracle's value or NaN.  got / want: (T, n_corr, S, C), or (T, n_corr) -- then a lag is NEAR if any
    weighted channel is.  Returns the number of NEAR entries that came back NaN where the oracle has a number."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    near = classes == NEAR
    if got.ndim == 2:
        near = near.any(axis=(2, 3))
    same = _same(got, want)
    bad = ~same & ~(near & np.isnan(got))
    assert not bad.any(), _first(bad, what, classes, got, want, f"differs from the oracle (R = {np.max(R)})")
    return int((near & ~same).sum())


def check_split(got, want, got_cleaned, classes, R, weights, what=""):
    """mf.split16 against the oracle on the poisoned day: the classes that no numerator decides are exact (0, NaN),
    CLEAN is within TOL_CC (times sum |w| for the network sum) and carries the cleaned day's bits, NEAR is that or NaN;
    nothing is ever +-Inf.  Returns the worst |d cc| over the bar on the finite entries."""
    got, want, got_cleaned = np.asarray(got), np.asarray(want), np.asarray(got_cleaned)
    assert got.shape == want.shape == got_cleaned.shape and got.dtype == np.float32, what
    assert not np.isinf(got).any(), _first(np.isinf(got), what, classes, got, want, "an Inf in the result")
    w = np.abs(np.asarray(weights, np.float64))
    with np.errstate(invalid="ignore"):
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if got.ndim == 4:
        zero = np.isin(classes, ZERO_CLASSES)
        bad = zero & (got.view(np.uint32) != 0)
        assert not bad.any(), _first(bad, what, classes, got, want, "must be exactly +0")
        bad = (classes == TOUCH_INF) & ~np.isnan(got)
        assert not bad.any(), _first(bad, what, classes, got, want, "must be NaN")
        dead = classes == DEAD_T_INF
        bad = dead & (np.isnan(got) != np.isnan(want))
        assert not bad.any(), _first(bad, what, classes, got, want, "NaN-ness of a template channel that holds Inf")
        clean, near = classes == CLEAN, classes == NEAR
        bad = clean & (got.view(np.uint32) != got_cleaned.view(np.uint32))
        assert not bad.any(), _first(bad, what, classes, got, got_cleaned, "CLEAN differs from the cleaned day's bits")
        bar = TOL_CC
    else:
        must_nan = np.isnan(want)                           # a TOUCH_INF / DEAD_T_INF channel: the weighted sum is NaN
        bad = must_nan & ~np.isnan(got)
        assert not bad.any(), _first(bad, what, classes, got, want, "must be NaN")
        near = (classes == NEAR).any(axis=(2, 3)) & ~must_nan
        clean = ~near & ~must_nan
        quiet = np.isin(classes, (CLEAN, OFF)).all(axis=(2, 3))       # every channel as on the cleaned day
        bad = quiet & (got.view(np.uint32) != got_cleaned.view(np.uint32))
        assert not bad.any(), _first(bad, what, classes, got, got_cleaned, "differs from the cleaned day's bits")
        bar = TOL_CC * w.reshape(w.shape[0], -1).sum(axis=1)[:, None]
    bar = np.broadcast_to(bar, got.shape)
    bad = clean & ~(diff <= bar)
    assert not bad.any(), _first(bad, what, classes, got, want, f"outside {TOL_CC:.0e} * sum |w|")
    bad = near & ~np.isnan(got) & ~(diff <= bar)
    assert not bad.any(), _first(bad, what, classes, got, want, f"NEAR: neither NaN nor within the bar (R = {np.max(R)})")
    sel = (clean | near) & ~np.isnan(got)
    return float((diff[sel] / bar[sel]).max(initial=0.0))


def check_invariance(got, got_cleaned, classes, what="", near_too=False):
    """network_sum=False: a channel without a bad sample has the cleaned day's bits at every lag, and so has every CLEAN
    lag of a channel with one (and OFF entries: nothing is computed there on either day).  No reference needed."""
    got, got_cleaned = np.asarray(got), np.asarray(got_cleaned)
    assert got.ndim == 4 and got.shape == got_cleaned.shape == classes.shape, what
    sel = np.isin(classes, (CLEAN, OFF, NEAR) if near_too else (CLEAN, OFF))
    bad = sel & (got.view(np.uint32) != got_cleaned.view(np.uint32))
    assert not bad.any(), _first(bad, what, classes, got, got_cleaned, "differs from the cleaned day's bits")
    return int(sel.sum())


def observed_reach(got, want, case, R):
    """The largest distance (window end -> bad sample) at which a lag came back NaN where the oracle has a number, per
    call; 0 when none did.  For profiles/mf_nonfinite.txt -- R is derived, this only reports how much of it shows."""
    got, want = np.asarray(got), np.asarray(want)
    if got.ndim != 4:
        return 0
    classes = case.classes(R)
    hit = (classes == NEAR) & np.isnan(got) & ~np.isnan(want)
    worst = 0
    for t, lag, s, c in np.argwhere(hit):
        j = lag * case.step + int(case.mv[t, s, c])
        first_bad = int(np.flatnonzero(bad_mask(case.data[s, c]))[0])
        worst = max(worst, first_bad - (j + case.L - 1))
    return worst


# ---------------------------------------------------------------------------------------- planted defects ---
DEFECTS = ("inverted_guard", "nan_scrubbed", "live_tail", "channel_poisoned", "channel_silenced", "neighbour",
           "reach_plus_one", "cleaned_returned")


def plant(defect, case, want, want_cleaned, R):
    """A per-channel result (T, n_corr, S, C) with the defect planted into the oracle's, or None when the case does not
    name it (it holds nothing of what the defect changes)."""
    assert defect in DEFECTS
    classes = case.classes(R)
    out = np.array(want, dtype=np.float32, copy=True)
    if defect == "inverted_guard":               # nrm >= 1000 ? 0 : num * nrm -- a NaN norm yields NaN
        hit = np.isin(classes, (AFTER, TOUCH_NAN, DEAD_T_NAN))
        out[hit] = np.nan
    elif defect == "nan_scrubbed":               # a NaN scrubbed to 0 inside the kernel
        hit = np.isnan(out)
        out[hit] = 0.0
    elif defect == "live_tail":                  # AFTER from a direct window sum (no prefix sum carries the NaN on)
        hit = classes == AFTER
        out[hit] = want_cleaned[hit]
        hit = hit & (want_cleaned != 0)
    elif defect == "channel_poisoned":           # the whole day of the bad channel is NaN
        hit = (classes == CLEAN) & _bad_channels(case)[None, None]
        out[hit] = np.nan
    elif defect == "channel_silenced":           # the halves of an unscaled 1e-9 channel flush to zero: finite and wrong
        tiny = np.zeros(classes.shape[2:], bool)
        for s, c, _, _ in case.bad:
            tiny[s, c] |= AMPLITUDES[(s + c) % 3] == 1.0e-9
        hit = (classes == CLEAN) & tiny[None, None] & (np.abs(want) > 2 * TOL_CC)
        out[hit] = 0.0
    elif defect == "neighbour":                  # the channel behind a bad one takes its NaNs
        hit = np.zeros(classes.shape, bool)
        S, C = classes.shape[2:]
        for s, c, _, _ in case.bad:
            n = (s * C + c + 1) % (S * C)
            touched = np.isin(classes[..., s, c], (TOUCH_NAN, TOUCH_INF, TOUCH_BIG))
            hit[..., n // C, n % C] |= touched & (classes[..., n // C, n % C] == CLEAN)
        out[hit] = np.nan
    elif defect == "reach_plus_one":             # the K range one sample longer than derived
        hit = np.zeros(classes.shape, bool)
        Rr = np.broadcast_to(np.asarray(R), classes.shape[:1] + classes.shape[2:])
        for s, c, _, _ in case.bad:
            first_bad = int(np.flatnonzero(bad_mask(case.data[s, c]))[0])
            if not (np.isnan(case.data[s, c, first_bad]) or np.isinf(case.data[s, c, first_bad])):
                continue                          # (0 * 3e38 is 0: a BIG sample has no reach)
            for t in range(classes.shape[0]):
                j_end = first_bad - int(Rr[t, s, c]) - 1             # the window's last sample, R + 1 in front
                num = j_end - (case.L - 1) - int(case.mv[t, s, c])
                if num % case.step == 0 and 0 <= num // case.step < case.n_corr and classes[t, num // case.step, s, c] == CLEAN:
                    hit[t, num // case.step, s, c] = True
        out[hit] = np.nan
    else:                                        # the cleaned day's result returned for the poisoned day
        out = np.array(want_cleaned, dtype=np.float32, copy=True)
        hit = ~_same(out, want)
    return out if hit.any() else None


def _bad_channels(case):
    m = np.zeros(case.data.shape[:2], bool)
    for s, c, _, _ in case.bad:
        m[s, c] = True
    return m


def network_sum32(cc, weights):
    """The float32 fmaf chain over the weighted channels, in channel order (zero-weight channels are skipped)."""
    T, n, S, C = cc.shape
    w = np.asarray(weights, np.float32).reshape(T, S * C)
    flat = cc.reshape(T, n, S * C)
    acc = np.zeros((T, n), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for ch in range(S * C):
            use = w[:, ch] != 0
            nxt = (acc.astype(np.float64) + w[:, None, ch].astype(np.float64) * flat[..., ch].astype(np.float64)).astype(np.float32)
            acc = np.where(use[:, None], nxt, acc)
    return acc
