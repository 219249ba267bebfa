"""Float64 definitions of the two hot paths with a priori error bounds, and the checker that judges
a float32 result (the C oracle's or a kernel's) against them.  TEST INFRASTRUCTURE, pure NumPy.

Nothing here is read off oracle/bpmf_oracle.c: the definitions follow SURVEY.md s8a / App. C and, for the
seven convention switches, the option texts in csrc/util.hip and the table in DESIGN.md s3.  Every
tolerance is derived (DESIGN.md "Float64 anchor"), with u = 2^-24 and gamma_n = n u / (1 - n u):

MF, per channel and lag
    cc = sum_l t_l d_l / sqrt(E_t E_d),   0 where E_t E_d <= 1e-6
    B  = gamma_L (A + |cc|) + 7u |cc| + E_term
    A      = sum_l |t_l d_l| / sqrt(E_t E_d): the L-term float32 numerator chain (its error is at most
             gamma_L sum |t_l d_l|) and the L-term chain of E_t (relative error gamma_L on E_t, at most that
             on cc);
    7u|cc|   the normalisation: float cast of the window energy, two sqrtf, two divides, two multiplies
             (or multiply, sqrtf, divide under mf.compat_sqrt_norm), one rounding each;
    E_term = 0.5 |cc| c_N 2^-53 csum_total / E_d: E_d is the difference of two double prefix sums, each
             carrying at most c_N roundings of a running sum <= csum_total; c_N = 1024 + ceil(N / 1024) for
             the 1024-sample hierarchy, N for the one chain of mf.compat_sequential_csum.
MF network sum:  sum_ch |w| B_ch + gamma_SC sum_ch |w cc|   (an S*C-term fmaf chain)
BP, per beam:    gamma_(n_terms + C) sum |beta| |alpha| |f|  (a C-term chain inside an n_terms-term chain)

In the exact regime (small integers, every partial sum below 2^24) numerators, energies and beams are exact
in float32: BP must equal float64 bit for bit and the MF bound shrinks to 7u |cc|.

The build zeroes r_t r_d >= 1000 and the definition E_t E_d <= 1e-6: the same threshold up to rounding, so
the definitions ASSERT that no active window has E_t E_d in [2.5e-7, 4e-6] -- a condition on the inputs.
"""
import numpy as np

U = 2.0 ** -24
NORM_ROUNDINGS = 7
GUARD = 1e-6
GUARD_WINDOW = (2.5e-7, 4e-6)
CSUM_CHUNK = 1024
EXACT_LIMIT = 2 ** 24
# what an exact-regime backprojection case must hold before its bit-equality means anything for the tie rule and
# the floor: "hundreds" of tied maxima, and floor samples well beyond a stray one
MIN_TIED, MIN_FLOOR = 200, 50


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------- matched filter ---
def mf_lag_range(mv, w, N, L, step, exclusive_last_lag=False, range_all_channels=False):
    """(first, last) valid lag of one template, or None.  Lag i reads data[i*step + mv : i*step + mv + L]
    of every channel that counts: the weighted ones, all of them under range_all_channels.  Inclusive end
    i*step + mv_max + L <= N; under exclusive_last_lag i*step < N - L - mv_max."""
    mv, w = np.asarray(mv).ravel(), np.asarray(w).ravel()
    if not (w != 0).any() or N < L:
        return None
    sel = np.ones(w.shape, bool) if range_all_channels else (w != 0)
    lo, hi = int(mv[sel].min()), int(mv[sel].max())
    n_corr = (N - L) // step + 1
    first = 0 if lo >= 0 else -(lo // step)                 # ceil(-lo / step)
    room = N - L - hi - (1 if exclusive_last_lag else 0)
    if room < 0:
        return None
    last = min(room // step, n_corr - 1)
    return (first, last) if first <= last else None


class MFRef:
    """cc, B: (T, n_lags, S, C) per-channel values and bounds (0 where the definition computes nothing);
    net, B_net: (T, n_lags); valid: (T, n_lags) lag inside the template's range; active: (T, S, C);
    zero_windows: how many valid entries read a window of exact zeros."""


def mf_f64(templates, moveouts, weights, data, step=1, lags=None, exclusive_last_lag=False,
           range_all_channels=False, sequential_csum=False, exact=False):
    """The definition at `lags` (all n_corr of them when None): O(len(lags) * L) per template-channel."""
    tp32 = np.asarray(templates)
    T, S, C, L = tp32.shape
    mv = np.broadcast_to(np.asarray(moveouts).reshape(T, S, -1), (T, S, C)).astype(np.int64)
    w = np.broadcast_to(np.asarray(weights).reshape(T, S, -1), (T, S, C)).astype(np.float64)
    data = np.asarray(data)
    N = data.shape[-1]
    n_corr = (N - L) // step + 1
    lags = np.arange(n_corr) if lags is None else np.asarray(lags, dtype=np.int64)
    assert lags.size and lags.min() >= 0 and lags.max() < n_corr
    c_N = N if sequential_csum else CSUM_CHUNK + -(-N // CSUM_CHUNK)
    if exact:
        assert np.abs(data).max() <= 3 and np.abs(tp32).max() <= 3 and 9 * L < EXACT_LIMIT
        assert np.array_equal(data, np.round(data)) and np.array_equal(tp32, np.round(tp32))
    ref = MFRef()
    ref.lags, ref.step, ref.w = lags, step, w
    ref.active = w != 0
    ref.cc = np.zeros((T, lags.size, S, C))
    ref.B = np.zeros((T, lags.size, S, C))
    ref.valid = np.zeros((T, lags.size), dtype=bool)
    ref.zero_windows = 0            # valid entries whose data window is all exact zeros (a data gap): cc = B = 0
    idx_l = np.arange(L)
    for s in range(S):
        for c in range(C):
            if not ref.active[:, s, c].any():
                continue
            d = data[s, c]
            csum_total = sum(float(np.dot(x, x)) for x in (d[i:i + (1 << 22)].astype(np.float64)
                                                           for i in range(0, N, 1 << 22)))
            for t in range(T):
                if not ref.active[t, s, c]:
                    continue
                rng_t = mf_lag_range(mv[t], w[t], N, L, step, exclusive_last_lag, range_all_channels)
                if rng_t is None:
                    continue
                ok = (lags >= rng_t[0]) & (lags <= rng_t[1])
                ref.valid[t] = ok
                tmpl = tp32[t, s, c].astype(np.float64)
                E_t = float(tmpl @ tmpl)
                sel = np.flatnonzero(ok)
                for j0 in range(0, sel.size, 2048):
                    j = sel[j0:j0 + 2048]
                    starts = lags[j] * step + mv[t, s, c]
                    assert starts.min() >= 0 and starts.max() + L <= N
                    win = d[starts[:, None] + idx_l[None, :]].astype(np.float64)
                    E_d = (win * win).sum(axis=1)
                    prod = E_t * E_d
                    ref.zero_windows += int((E_d == 0).sum())
                    in_window = (prod >= GUARD_WINDOW[0]) & (prod <= GUARD_WINDOW[1])
                    assert not in_window.any(), \
                        f"input condition: E_t*E_d = {prod[in_window][0]:.3e} inside the guard window (t={t}, s={s}, c={c})"
                    keep = prod > GUARD
                    den = np.sqrt(np.where(keep, prod, 1.0))
                    cc = np.where(keep, (win @ tmpl) / den, 0.0)
                    if exact:
                        B = NORM_ROUNDINGS * U * np.abs(cc)
                    else:
                        A = np.where(keep, (np.abs(win) @ np.abs(tmpl)) / den, 0.0)
                        E_term = 0.5 * np.abs(cc) * c_N * 2.0 ** -53 * csum_total / np.where(keep, E_d, 1.0)
                        B = np.where(keep, gamma(L) * (A + np.abs(cc)) + NORM_ROUNDINGS * U * np.abs(cc) + E_term, 0.0)
                    ref.cc[t, j, s, c] = cc
                    ref.B[t, j, s, c] = B
    aw = np.abs(w)[:, None]
    ref.net = (ref.cc * w[:, None]).sum(axis=(2, 3))
    ref.B_net = (ref.B * aw).sum(axis=(2, 3)) + gamma(S * C) * (np.abs(ref.cc) * aw).sum(axis=(2, 3))
    return ref


class Report:
    def __init__(self, what, bad, ratio, detail=""):
        self.what, self.n, self.n_bad = what, int(bad.size), int(bad.sum())
        self.bad, self.worst, self.detail = bad, float(ratio), detail

    @property
    def frac_bad(self):
        return self.n_bad / max(1, self.n)

    def require(self):
        print(f"f64-anchor {self.what}: worst err/B = {self.worst:.4f}, {self.n_bad} of {self.n} outside")
        assert self.n_bad == 0, f"{self.what}: {self.n_bad} of {self.n} outside the bound or a zero rule; {self.detail}"
        return self.worst


def _worst(err, B):
    pos = B > 0
    return float((err[pos] / B[pos]).max()) if pos.any() else 0.0


def mf_compare(got, ref, network_sum, what="MF"):
    """`got`: the float32 result AT ref.lags -- (T, n_lags) or (T, n_lags, S, C).  |got - f64| <= B element by
    element; B is 0 wherever the definition computes nothing, so those outputs must be exactly 0."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    want, B = (ref.net, ref.B_net) if network_sum else (ref.cc, ref.B)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= B)                                      # (NaN fails)
    detail = ""
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        detail = f"first at {i} (lag {int(ref.lags[i[1]])}): got {got[i]!r}, f64 {want[i]!r}, B {B[i]:.3e}"
    return Report(what, bad, _worst(err, B), detail)


def mf_full(got, ref):
    """A whole result restricted to ref.lags."""
    return np.asarray(got)[:, ref.lags]


# ----------------------------------------------------------------------------- backprojection ---
class BPRef:
    """beam, B: (K, n_times) float64 (0 where not computed); computed: (K, n_times) bool."""


def bp_f64(features, moveouts, w_phases, w_sources, out_of_bounds="strict", times=None,
           strict_upper_only=False, range_all_stations=False, exact=False):
    """b_k(t) = sum_{s,p} beta[k,s] sum_c alpha[s,c,p] f[s,c,t + tau[k,s,p]] over the stations with beta != 0, at
    `times` (all N when None), over all K sources.  strict: computed where 0 <= t + tau_min and t + tau_max < N
    (tau_min / tau_max over the weighted stations; over all stations under range_all_stations; the lower test
    dropped, and terms in front of sample 0 with it, under strict_upper_only); flexible: everywhere, terms outside
    the trace dropped.  A source without any weighted station computes nothing."""
    f = np.asarray(features)
    S, C, N = f.shape
    tau = np.asarray(moveouts).astype(np.int64)
    K, _, P = tau.shape
    alpha = np.asarray(w_phases).astype(np.float64)
    beta = np.asarray(w_sources).astype(np.float64)
    times = np.arange(N) if times is None else np.asarray(times, dtype=np.int64)
    used = beta != 0
    ref = BPRef()
    ref.times, ref.K, ref.N = times, K, N
    has = used.any(axis=1)
    if out_of_bounds == "strict":
        sel = np.ones_like(used) if range_all_stations else used
        lo = np.where(sel[:, :, None], tau, np.iinfo(np.int64).max).min(axis=(1, 2))
        hi = np.where(sel[:, :, None], tau, np.iinfo(np.int64).min).max(axis=(1, 2))
        lo, hi = np.where(has, lo, 0), np.where(has, hi, 0)
        comp = times[None, :] + hi[:, None] < N
        if not strict_upper_only:
            comp &= times[None, :] + lo[:, None] >= 0
    else:
        assert out_of_bounds == "flexible"
        comp = np.ones((K, times.size), dtype=bool)
    comp &= has[:, None]
    beam = np.zeros((K, times.size))
    mag = np.zeros((K, times.size))
    for s in range(S):
        ks = np.flatnonzero(used[:, s])
        if not ks.size:
            continue
        for p in range(P):
            Usp = np.zeros(N)
            Uabs = np.zeros(N)
            for c in range(C):
                fc = f[s, c].astype(np.float64)
                Usp += alpha[s, c, p] * fc
                Uabs += abs(alpha[s, c, p]) * np.abs(fc)
            x = times[None, :] + tau[ks, s, p][:, None]
            inb = (x >= 0) & (x < N)
            np.clip(x, 0, N - 1, out=x)
            beam[ks] += np.where(inb, beta[ks, s, None] * Usp[x], 0.0)
            mag[ks] += np.where(inb, np.abs(beta[ks, s, None]) * Uabs[x], 0.0)
    n_terms = P * used.sum(axis=1)
    ref.computed = comp
    ref.beam = np.where(comp, beam, 0.0)
    ref.mag = np.where(comp, mag, 0.0)
    if exact:
        assert all(np.array_equal(a, np.round(a)) for a in (f, alpha, beta)), "exact regime: integers only"
        assert np.abs(f).max() <= 3 and np.abs(alpha).max() <= 2 and beta.min() >= 0 and beta.max() <= 2
        assert ref.mag.max() < EXACT_LIMIT, "exact regime: a partial sum could reach 2^24"
        ref.B = np.zeros_like(ref.beam)
    else:
        ref.B = gamma(n_terms + C)[:, None] * ref.mag
    return ref


def bp_max_f64(ref, first_computed=False):
    """The definition's (max-beam, arg-max): scan the computed beams from (0, source 0), strictly greater
    replaces (lowest index on ties); under first_computed from the first computed beam, (0, 0) where none is."""
    masked = np.where(ref.computed, ref.beam, -np.inf)
    best, arg = masked.max(axis=0), masked.argmax(axis=0)
    keep = np.isfinite(best) if first_computed else best > 0
    return np.where(keep, best, 0.0), np.where(keep, arg, 0).astype(np.int32)


def bp_tie_and_floor_counts(ref):
    """What an exact-regime case must hold, counted on the definition alone: the samples whose positive maximum
    several sources share (the lowest-index rule) and the samples that compute beams, none of them positive (the
    (0, 0) floor of the default scan)."""
    masked = np.where(ref.computed, ref.beam, -np.inf)
    best = masked.max(axis=0)
    tied = ((masked == best).sum(axis=0) > 1) & (best > 0)
    floor = ref.computed.any(axis=0) & (best <= 0)
    return int(tied.sum()), int(floor.sum())


def bp_compare_beam(got, ref, what="BP beam"):
    """reduce="none": (K, n_times) at ref.times; |got - b| <= B, exactly 0 where nothing is computed."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.beam.shape, (got.dtype, got.shape, ref.beam.shape)
    err = np.abs(got.astype(np.float64) - ref.beam)
    bad = ~(err <= ref.B)
    detail = ""
    if bad.any():
        k, j = (int(x) for x in np.argwhere(bad)[0])
        detail = f"first at source {k}, t {int(ref.times[j])}: got {got[k, j]!r}, f64 {ref.beam[k, j]!r}, B {ref.B[k, j]:.3e}"
    return Report(what, bad, _worst(err, ref.B), detail)


def bp_compare_max(m, a, ref, first_computed=False, what="BP max"):
    """reduce="max" at ref.times, every sample judged.  With b the float64 beams, B their bounds, k* the float64
    arg-max over the computed beams:  |m - b_a| <= B_a;  b_a >= b_k* - B_a - B_k*;  source a computed at t.
    Default scan: m > 0 or (m, a) == (0, 0), and (0, 0) only if b_k* <= B_k* (or nothing is computed).
    first_computed: (0, 0) exactly where nothing is computed, else the three rules (m of any sign)."""
    m, a = np.asarray(m), np.asarray(a)
    assert m.dtype == np.float32 and a.dtype == np.int32 and m.shape == a.shape == ref.times.shape
    nt = ref.times.size
    j = np.arange(nt)
    masked = np.where(ref.computed, ref.beam, -np.inf)
    k_star = masked.argmax(axis=0)
    b_star, B_star = masked[k_star, j], ref.B[k_star, j]
    in_range = (a >= 0) & (a < ref.K)
    a_ = np.where(in_range, a, 0)
    b_a, B_a, comp_a = ref.beam[a_, j], ref.B[a_, j], ref.computed[a_, j]
    m64 = m.astype(np.float64)
    err = np.abs(m64 - b_a)
    rules = in_range & comp_a & (err <= B_a) & (b_a >= b_star - B_a - B_star)
    floor = (m == 0) & (a == 0)
    if first_computed:
        any_comp = ref.computed.any(axis=0)
        ok = np.where(any_comp, rules, floor)
    else:
        ok = np.where(floor, b_star <= B_star, rules & (m > 0))
    bad = ~ok
    detail = ""
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        detail = (f"first at t {int(ref.times[i])}: got ({m[i]!r}, {int(a[i])}), b_a {b_a[i]!r} +- {B_a[i]:.3e}, "
                  f"f64 max ({b_star[i]!r} +- {B_star[i]:.3e}, {int(k_star[i])})")
    judged = ~floor & in_range & comp_a
    return Report(what, bad, _worst(err[judged], B_a[judged]), detail)


# ----------------------------------------------------------------------------- sampled indices ---
EDGE_MULTIPLES = (128, 256, 512, 2048, 8192)


def edge_sample(n, firsts, lasts, n_random, seed, per_multiple=12, tail=24):
    """Sorted unique indices in [0, n): 0 and n - 1; every `firsts` / `lasts` index (first / last valid lag or
    sample) with its neighbours, and `tail` indices behind each `lasts` (the strict tail); the neighbours
    -1, 0, +1 of `per_multiple` multiples of 128, 256, 512, 2048 and 8192 spread over the axis; seeded random."""
    idx = [0, n - 1]
    for x in list(firsts) + list(lasts):
        idx += [x - 1, x, x + 1]
    for x in lasts:
        idx += list(range(x + 1, x + 1 + tail)) + [(x + n) // 2]
    for m in EDGE_MULTIPLES:
        n_mult = (n - 1) // m
        for q in np.unique(np.linspace(1, max(1, n_mult), per_multiple).astype(np.int64)):
            idx += [q * m - 1, q * m, q * m + 1]
    idx += list(np.random.default_rng(seed).integers(0, n, n_random))
    idx = np.unique(np.asarray(idx, dtype=np.int64))
    return idx[(idx >= 0) & (idx < n)]


# ----------------------------------------------------------------------------- inputs ---
MF_REGIMES = ("noise", "scaled", "dc", "sine")


def mf_case(regime, L, N, step, seed, T=2, S=2, C=3, mv_lo=-70, mv_hi=400):
    """Inputs of one matched-filter case: moveouts of both signs whose most negative one is not a multiple of the
    step, one zero-weight channel per template that carries moveouts beyond every weighted one (what
    range_all_channels is about), a data gap of exact zeros, a dead (all-zero) template channel.
    Regimes: unit noise; per-channel scales 1e-6..1e4 with a glitch of 3e4 sigma; DC offset (data + 50, template
    + 5); a sinusoid (|cc| ~ 1); "int": the exact regime (integers in -3..3)."""
    rng = np.random.default_rng(seed)
    n_ch = S * C

    def noise(shape):
        x = rng.standard_normal(shape)
        # (a window of one or a few samples can have any energy: keep the samples away from 0 so that the
        # energy-guard condition holds whatever the seed)
        return np.sign(x) * (0.5 + np.abs(x)) if L < 8 else x

    if regime == "int":
        tp = rng.integers(-3, 4, (T, S, C, L)).astype(np.float64)
        d = rng.integers(-3, 4, (S, C, N)).astype(np.float64)
        if L < 8:
            tp[tp == 0] = 1
    elif regime == "sine":
        om = 2 * np.pi / 23.0
        ph = rng.uniform(0, 2 * np.pi, (S, C, 1))
        d = np.sin(om * np.arange(N) + ph) + 0.01 * rng.standard_normal((S, C, N))
        tp = np.sin(om * np.arange(L) + rng.uniform(0, 2 * np.pi, (T, S, C, 1))) + 1.5 * (L < 8)
        if L < 8:
            d = d + 1.5
    else:
        tp, d = noise((T, S, C, L)), noise((S, C, N))
        if regime == "dc":
            tp, d = tp + 5.0, d + 50.0
        elif regime == "scaled":
            sd = np.resize([1e-6, 1e-3, 1e-1, 1.0, 1e2, 1e4], n_ch).reshape(S, C, 1)
            st = np.resize([1e-3, 1e3, 1e1, 1.0, 1e-2, 1e-4], n_ch).reshape(1, S, C, 1)
            d[S - 1, C - 1, N // 3] = 3e4                      # the glitch
            d, tp = d * sd, tp * st
        else:
            assert regime == "noise"
    mv = rng.integers(mv_lo, mv_hi + 1, (T, S, C))
    w = rng.uniform(0.1, 1.0, (T, S, C))
    if regime == "int":
        w = rng.integers(1, 3, (T, S, C)).astype(np.float64)
    for t in range(T):
        mv.reshape(T, -1)[t, (t + 1) % n_ch] = mv_lo - (mv_lo % step == 0)   # first valid lag off the step grid
        z = (2 * t + 3) % n_ch
        if n_ch > 2 and z != (t + 1) % n_ch:
            w.reshape(T, -1)[t, z] = 0.0
            mv.reshape(T, -1)[t, z] = mv_hi + 333 if t % 2 else mv_lo - 333
    g0 = N // 2
    d[0, 0, g0:g0 + 2 * L + 50] = 0.0                         # a data gap
    if T > 1 and n_ch > 1:
        # a dead template channel: the first one of template T - 1 that is weighted, after channel (0, 0),
        # which holds the data gap
        dead = 1 + int(np.flatnonzero(w.reshape(T, -1)[T - 1, 1:] != 0)[0])
        tp.reshape(T, n_ch, L)[T - 1, dead] = 0.0
    return (tp.astype(np.float32), mv.astype(np.int32), w.astype(np.float32), d.astype(np.float32))


def mf_dead_channels(templates, ref):
    """Number of (template, channel) pairs that are weighted, all-zero in the template, and inside the valid lag
    range somewhere -- after asserting that the definition gives exact 0 with a zero bound on every one of them."""
    tp = np.asarray(templates)
    dead = ref.active & ~tp.any(axis=-1) & ref.valid.any(axis=1)[:, None, None]
    for t, s, c in np.argwhere(dead):
        assert not ref.cc[t, :, s, c].any() and not ref.B[t, :, s, c].any()
    return int(dead.sum())


def bp_case(regime, K, S, P, N, seed, C=3, tau_lo=-700, tau_hi=1200, n_used=None, uniform=False):
    """Inputs of one backprojection case: moveouts of both signs, a zero-weight source, zero-weight stations that
    carry the extreme moveouts (what range_all_stations is about).  Regimes: "signed" -- signed features with
    per-channel scales 1e-3..1e3, signed phase weights; "int": the exact regime -- features in -3..3, phase
    weights in -2..2, source weights in 0..2, stretches of negative and of zero features (the (0, 0) floor),
    duplicated sources and few distinct values (maxima shared by several sources)."""
    rng = np.random.default_rng(seed)
    tau = rng.integers(tau_lo, tau_hi + 1, (K, S, P))
    n_used = S if n_used is None else n_used
    ws = np.zeros((K, S))
    for k in range(K):
        sel = rng.choice(S, min(S, n_used), replace=False) if n_used < S else np.arange(S)
        ws[k, sel] = 1.0
    if regime == "int":
        f = rng.integers(-3, 4, (S, C, N)).astype(np.float64)
        # a stretch of negative and one of zero features, each longer than the span of the moveouts, so that
        # whole samples see nothing else (the zero stretch: beams of exact 0, the floor)
        n_flat = tau_hi - tau_lo + 110
        assert N // 2 + n_flat <= N
        f[:, :, N // 4: N // 4 + n_flat] = -np.abs(f[:, :, N // 4: N // 4 + n_flat])
        f[:, :, N // 2: N // 2 + n_flat] = 0.0
        wp = rng.integers(0, 3, (S, C, P)).astype(np.float64)
        wp[0, 0, 0] = -1.0
        ws *= 1.0 if uniform else rng.integers(1, 3, (K, S))
        if K >= 8:
            tau[K // 2: K // 2 + K // 8] = tau[K // 4: K // 4 + K // 8]      # identical sources: exact ties
            ws[K // 2: K // 2 + K // 8] = ws[K // 4: K // 4 + K // 8]
    else:
        assert regime == "signed"
        scale = 10.0 ** rng.uniform(-3, 3, (S, C, 1))
        f = rng.standard_normal((S, C, N)) * scale
        wp = rng.uniform(-1.0, 1.0, (S, C, P))
        ws *= 0.25 if uniform else rng.uniform(0.1, 1.0, (K, S))
    if K > 3:
        ws[3] = 0.0                                            # a source without any station
    if S > 2 and n_used >= S:
        ws[::2, S - 1] = 0.0                                   # zero-weight stations with the extreme moveouts
        tau[::2, S - 1, 0] = tau_lo - 150
        tau[::2, S - 1, P - 1] = tau_hi + 250
    elif S > n_used:
        for k in range(0, K, 2):
            s = int(np.flatnonzero(ws[k] == 0)[0])
            tau[k, s, 0], tau[k, s, P - 1] = tau_lo - 150, tau_hi + 250
    return f.astype(np.float32), tau.astype(np.int32), wp.astype(np.float32), ws.astype(np.float32)
