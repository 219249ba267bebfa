"""Float64 definition of the matched filter's FULL normalisation (flag BPMF_MF_NORMALIZE_FULL: the window mean removed,
the Pearson correlation) with an a priori bound per value, a float32 emulation of the prescribed computation with
planted defects, and the inputs of the tests that rest on them.  TEST INFRASTRUCTURE, pure NumPy; extends
tests/f64_anchor.py (mf_f64 / MFRef / mf_compare), which it imports and does not change.

Written from DESIGN.md s3 "full normalisation" and the header text of the flag, not from csrc/mf_full.hip.

Definition, per template t, channel ch with w != 0 and valid lag i (x the window, tp the template channel):
    cc = sum (tp - mean tp)(x - mean x) / sqrt(E_t' E_c),   E_t' = sum (tp - mean tp)^2,   E_c = sum (x - mean x)^2
    exactly +0 where the window is flat (all L samples compare equal), where the template channel is flat, and where
    E_t' E_c <= 1e-6.  Lag ranges, weights and the network sum are those of mf_f64.

Prescribed computation (what B_full bounds; u = 2^-24):
    c = float32(float64 mean of the channel), d' = fl32(d - c);  tbar32 = float32(float64 mean tp), t' = fl32(tp - tbar32)
    num = the L-term float32 fmaf chain of t' d';  E_t'' = the float32 chain of t'^2
    P, Q = window sums of d', d'^2 from double prefix sums in the 1024-sample hierarchy;  E_c^ = Q - P P / L in double
    cc^ = num * ((1 / sqrtf(E_t'')) * (1 / sqrtf((float)E_c^)))

B_full.  With the REAL-arithmetic values of the rounded operands  N_k = sum t' d',  E_tk = sum t'^2,
E_ck = sum (d' - mean d')^2,  P_k = sum d',  den = sqrt(E_t' E_c),  Delta = tbar32 - mean tp,  e_t / e_d the rounding of
each t' / d' (evaluated exactly from the inputs: a subtraction of two floats within a factor of two of each other is
exact, so an offset costs nothing here):
    B1 = gamma_L A_k                                        the numerator chain,  A_k = sum |t' d'| / den
       + (|Delta| |P_k| + sum |e_t d'| + sum |t_c e_d|) / den   the mean of the template rounded to float32 (it multiplies
                                                            the window sum of d': a large LOCAL mean costs precision), and
                                                            one rounding of each t' and each d' in the numerator
       + |cc| (gamma_L + 7u)                                the chain of E_t'' and the seven normalisation roundings of mf_f64
       + |cc| / 2 (|E_tk - E_t'| / E_t' + |E_ck - E_c| / E_c)   the roundings of t' and d' in the two energies (L Delta^2 included)
       + |cc| / 2 E_err / E_c                               E_term over BOTH prefix arrays:
    E_err = dQ + (2 |P_k| dP + dP^2) / L + 4 * 2^-53 Q_k,   dQ = 2 c_N 2^-53 sum_channel d'^2,  dP = 2 c_N 2^-53 sum_channel |d'|
            (a prefix value carries at most c_N = 1024 + ceil(N / 1024) roundings of running sums that never exceed the
            channel's sum of d'^2, resp. of |d'|; a window sum is the difference of two; P P, / L and the subtraction round
            once more each, relative to at most Q_k)
    B_full = B1 (1 + 2 r),   r = gamma_L + 7u + |E_tk - E_t'| / E_t' + |E_ck - E_c| / E_c + E_err / E_c   (second order:
            the relative errors of the denominators multiply those of the numerator; r < 2^-5 is asserted)
Input conditions (asserted, like GUARD_WINDOW in mf_f64): no active window has E_t' E_c in [2.5e-7, 4e-6]; no window
that is not flat has E_c below 2^10 E_err.

Exact regimes (numerators, E_t'' and both window sums exact; c = 0, tbar = 0, so d' = d and t' = tp):
    "int0"      integers |x| <= 3 whose channel sums and template sums are exactly 0.  P P is an exact double, P P / L
                rounds once, Q - P P / L once more; then the seven float32 roundings:
                B = |cc| (7u + 2^-54 (P^2 / L + E_c) / E_c) (1 + 2 r)
    "periodic"  data = a sum of zero-sum integer sequences whose periods (3, 4, 6, 8, 12, 16) divide L = 48, N a multiple of
                L: every window sum is exactly 0 (asserted), E_c^ = Q, and full mode is bit-equal to short mode.
"""
import numpy as np

import f64_anchor as fa

U = fa.U
COND_E_FACTOR = 2.0 ** 10
R_LIMIT = 2.0 ** -5
DROPS = ("data_mean", "template", "uncentred", "p_lo", "p_hi", "c_neighbour", "flat_short", "pp_div")
PERIODS = (3, 4, 6, 8, 12, 16)
PERIODIC_L = 48
REGIMES = ("noise", "offset", "drift", "step", "scaled", "gaps", "int0", "periodic")
EXACT_REGIMES = ("int0", "periodic")
OFFSET = 2.0 ** 13


def _is_flat(rows):
    return (rows == rows[..., :1]).all(axis=-1)


def channel_constant(d):
    """c of one channel: float32((float64 sum of its finite samples) / N), 0 when none is finite.  On a finite channel
    this is float32(float64 mean) bit for bit (a bad sample adds +0 to the same summation); a NaN or +-Inf sample must
    not reach c, or d' = d - c is NaN for the whole day of the channel."""
    d64 = np.asarray(d).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.float32(np.where(np.isfinite(d64), d64, 0.0).sum() / d64.size)


def mf_full_f64(templates, moveouts, weights, data, step=1, lags=None, exclusive_last_lag=False,
                range_all_channels=False, exact=False):
    """The definition at `lags` (all of them when None): an fa.MFRef with cc, B (T, n_lags, S, C), net, B_net, valid,
    active, and `flat` (T, n_lags, S, C): valid entries of weighted channels whose window or template channel is flat
    (cc and B exactly 0).  exact: False, "int0" or "periodic"."""
    tp32 = np.asarray(templates, dtype=np.float32)
    T, S, C, L = tp32.shape
    mv = np.broadcast_to(np.asarray(moveouts).reshape(T, S, -1), (T, S, C)).astype(np.int64)
    w = np.broadcast_to(np.asarray(weights).reshape(T, S, -1), (T, S, C)).astype(np.float64)
    data = np.asarray(data, dtype=np.float32)
    N = data.shape[-1]
    n_corr = (N - L) // step + 1
    lags = np.arange(n_corr) if lags is None else np.asarray(lags, dtype=np.int64)
    assert lags.size and lags.min() >= 0 and lags.max() < n_corr
    c_N = fa.CSUM_CHUNK + -(-N // fa.CSUM_CHUNK)
    gL = float(fa.gamma(L))
    if exact:
        assert exact in EXACT_REGIMES
        assert np.array_equal(data, np.round(data)) and np.array_equal(tp32, np.round(tp32))
        assert np.abs(tp32).max() <= 3 and float(np.abs(data).max()) * 3 * L < fa.EXACT_LIMIT
        assert (data.astype(np.float64).sum(axis=-1) == 0).all(), "exact regime: every channel sums to exactly 0"
        assert (tp32.astype(np.float64).sum(axis=-1) == 0).all(), "exact regime: every template channel sums to exactly 0"
        if exact == "int0":
            assert np.abs(data).max() <= 3
        else:
            assert L == PERIODIC_L and N % L == 0
    ref = fa.MFRef()
    ref.lags, ref.step, ref.w = lags, step, w
    ref.active = w != 0
    shape = (T, lags.size, S, C)
    ref.cc, ref.B = np.zeros(shape), np.zeros(shape)
    ref.flat = np.zeros(shape, dtype=bool)
    ref.P = np.zeros(shape)
    ref.valid = np.zeros((T, lags.size), dtype=bool)
    ref.r_max = 0.0
    for s in range(S):
        for c in range(C):
            if not ref.active[:, s, c].any():
                continue
            d64 = data[s, c].astype(np.float64)
            c32 = channel_constant(data[s, c])
            y_all = d64 - float(c32)                               # d - c (the difference of two floats: exact in double)
            dp_all = (data[s, c] - c32).astype(np.float32).astype(np.float64)      # d' = fl32(d - c)
            rows_raw = np.lib.stride_tricks.sliding_window_view(data[s, c], L)
            rows_y = np.lib.stride_tricks.sliding_window_view(y_all, L)
            rows_dp = np.lib.stride_tricks.sliding_window_view(dp_all, L)
            dQ = 2 * c_N * 2.0 ** -53 * float(dp_all @ dp_all)
            dP = 2 * c_N * 2.0 ** -53 * float(np.abs(dp_all).sum())
            for t in range(T):
                if not ref.active[t, s, c]:
                    continue
                rng_t = fa.mf_lag_range(mv[t], w[t], N, L, step, exclusive_last_lag, range_all_channels)
                if rng_t is None:
                    continue
                ok = (lags >= rng_t[0]) & (lags <= rng_t[1])
                ref.valid[t] = ok
                t64 = tp32[t, s, c].astype(np.float64)
                tbar = t64.mean()
                tbar32 = np.float32(tbar)
                delta = float(tbar32) - tbar
                t_c = t64 - tbar                                    # the centred template of the definition
                flat_t = bool(_is_flat(tp32[t, s, c]))
                t_k = np.zeros(L) if flat_t else (tp32[t, s, c] - tbar32).astype(np.float32).astype(np.float64)
                e_t = np.abs(t_k - (t64 - float(tbar32)))
                E_t, E_tk = float(t_c @ t_c), float(t_k @ t_k)
                rel_t = abs(E_tk - E_t) / E_t if E_t > 0 else 0.0
                sel = np.flatnonzero(ok)
                for j0 in range(0, sel.size, 256):
                    j = sel[j0:j0 + 256]
                    starts = lags[j] * step + mv[t, s, c]
                    assert starts.min() >= 0 and starts.max() + L <= N
                    flat_w = _is_flat(rows_raw[starts])
                    y, dp = rows_y[starts], rows_dp[starts]
                    yc = y - y.mean(axis=1, keepdims=True)
                    E_c = np.einsum("ij,ij->i", yc, yc)
                    dpc = dp - dp.mean(axis=1, keepdims=True)
                    E_ck = np.einsum("ij,ij->i", dpc, dpc)
                    P_k, Q_k = dp.sum(axis=1), np.einsum("ij,ij->i", dp, dp)
                    E_err = dQ + (2 * np.abs(P_k) * dP + dP * dP) / L + 4 * 2.0 ** -53 * Q_k
                    zero = flat_w | flat_t
                    prod = np.where(zero, 0.0, E_t * E_c)
                    in_window = (prod >= fa.GUARD_WINDOW[0]) & (prod <= fa.GUARD_WINDOW[1])
                    assert not in_window.any(), \
                        f"input condition: E_t'*E_c = {prod[in_window][0]:.3e} inside the guard window (t={t}, s={s}, c={c})"
                    keep = prod > fa.GUARD
                    thin = keep & (E_c < COND_E_FACTOR * E_err)
                    assert not thin.any(), \
                        (f"input condition: E_c = {E_c[thin][0]:.3e} below 2^10 x the prefix-sum error bound "
                         f"{E_err[thin][0]:.3e} (t={t}, s={s}, c={c})")
                    den = np.sqrt(np.where(keep, prod, 1.0))
                    E_c1 = np.where(keep, E_c, 1.0)
                    cc = np.where(keep, (y @ t_c) / den, 0.0)
                    acc = np.abs(cc)
                    if exact:
                        if exact == "periodic":
                            assert (P_k[keep] == 0).all(), "periodic regime: every window sum is exactly 0"
                        r = fa.NORM_ROUNDINGS * U + 2.0 ** -53 * (P_k * P_k / L + E_c1) / E_c1
                        B1 = acc * (fa.NORM_ROUNDINGS * U + 2.0 ** -54 * (P_k * P_k / L + E_c1) / E_c1)
                    else:
                        A_k = (np.abs(dp) @ np.abs(t_k)) / den
                        num_ops = (abs(delta) * np.abs(P_k) + np.abs(dp) @ e_t + np.abs(dp - y) @ np.abs(t_c)) / den
                        rel_c = np.abs(E_ck - E_c) / E_c1
                        r = gL + fa.NORM_ROUNDINGS * U + rel_t + rel_c + E_err / E_c1
                        B1 = gL * A_k + num_ops + acc * (gL + fa.NORM_ROUNDINGS * U + 0.5 * (rel_t + rel_c + E_err / E_c1))
                    r = np.where(keep, r, 0.0)
                    assert r.max(initial=0.0) < R_LIMIT, f"input condition: relative error of the norms {r.max():.3e} (t={t}, s={s}, c={c})"
                    ref.r_max = max(ref.r_max, float(r.max(initial=0.0)))
                    ref.cc[t, j, s, c] = cc
                    ref.B[t, j, s, c] = np.where(keep, B1 * (1 + 2 * r), 0.0)
                    ref.flat[t, j, s, c] = zero
                    ref.P[t, j, s, c] = P_k
    ref.net, ref.B_net = fa._mf_network(ref.cc, ref.cc, ref.B, w)
    return ref


# --------------------------------------------------------------------- float32 emulation, planted defects ---
def _chain32(a, b):
    """The float32 fmaf chain sum_l a[l] * b[..., l], l ascending (products exact in double, one rounding per step)."""
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), dtype=np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for l in range(a.shape[-1]):
        acc = (acc.astype(np.float64) + a64[..., l] * b64[..., l]).astype(np.float32)
    return acc


def mf_full_emulate(templates, moveouts, weights, data, step=1, lags=None, drop=None, exclusive_last_lag=False,
                    range_all_channels=False):
    """The prescribed computation in float32 NumPy at `lags`: per-channel values (T, n_lags, S, C) float32 (0 where
    nothing is computed).  `drop`: one of DROPS, a planted defect --
        data_mean    the data mean not removed (the short-mode value: raw template, raw data, uncentred energy)
        template     the template not centred
        uncentred    E_c left uncentred (Q alone)
        p_lo, p_hi   the window of P one sample short at its start / its end
        c_neighbour  c taken from the neighbouring channel
        flat_short   flatness decided for L - 1 samples
        pp_div       P P divided by L - 1."""
    assert drop is None or drop in DROPS
    tp32 = np.asarray(templates, dtype=np.float32)
    T, S, C, L = tp32.shape
    mv = np.broadcast_to(np.asarray(moveouts).reshape(T, S, -1), (T, S, C)).astype(np.int64)
    w = np.broadcast_to(np.asarray(weights).reshape(T, S, -1), (T, S, C)).astype(np.float64)
    data = np.asarray(data, dtype=np.float32)
    N = data.shape[-1]
    n_ch = S * C
    n_corr = (N - L) // step + 1
    lags = np.arange(n_corr) if lags is None else np.asarray(lags, dtype=np.int64)
    out = np.zeros((T, lags.size, S, C), dtype=np.float32)
    flat_data = data.reshape(n_ch, N)
    with np.errstate(all="ignore"):
        for ch in range(n_ch):
            s, c = divmod(ch, C)
            d = flat_data[ch]
            src = flat_data[(ch + 1) % n_ch] if drop == "c_neighbour" else d
            c32 = channel_constant(src)
            dp = d.copy() if drop == "data_mean" else (d - c32).astype(np.float32)
            dp64 = dp.astype(np.float64)
            csP = np.concatenate([[0.0], np.cumsum(dp64)])
            csQ = np.concatenate([[0.0], np.cumsum(dp64 * dp64)])
            eq = np.concatenate([[0], np.cumsum(np.concatenate([[0], (d[1:] == d[:-1]).astype(np.int64)]))])   # eq[n]: pairs among samples < n
            rows = np.lib.stride_tricks.sliding_window_view(dp, L)
            for t in range(T):
                if w[t, s, c] == 0:
                    continue
                rng_t = fa.mf_lag_range(mv[t], w[t], N, L, step, exclusive_last_lag, range_all_channels)
                if rng_t is None:
                    continue
                sel = np.flatnonzero((lags >= rng_t[0]) & (lags <= rng_t[1]))
                if not sel.size:
                    continue
                j = lags[sel] * step + mv[t, s, c]
                x = tp32[t, s, c]
                if drop in ("template", "data_mean"):
                    tk = x.copy()
                elif _is_flat(x):
                    tk = np.zeros(L, np.float32)
                else:
                    tk = (x - np.float32(x.astype(np.float64).mean())).astype(np.float32)
                r_t = np.float32(1.0) / np.sqrt(_chain32(tk, tk))
                P = csP[j + L] - csP[j]
                if drop == "p_lo":
                    P = csP[j + L] - csP[j + 1]
                elif drop == "p_hi":
                    P = csP[j + L - 1] - csP[j]
                Q = csQ[j + L] - csQ[j]
                if drop in ("uncentred", "data_mean"):
                    E = Q
                elif drop == "pp_div":
                    E = Q - P * P / max(L - 1, 1)
                else:
                    E = Q - P * P / L
                if drop == "flat_short" and L > 1:
                    is_flat = (eq[j + L - 1] - eq[j + 1]) == L - 2
                elif drop == "data_mean":
                    is_flat = np.zeros(j.shape, bool)
                else:
                    is_flat = (eq[j + L] - eq[j + 1]) == L - 1
                r_c = np.where(is_flat, np.float32(np.inf), np.float32(1.0) / np.sqrt(E.astype(np.float32))).astype(np.float32)
                num = _chain32(tk[None, :], rows[j])
                nrm = (r_t * r_c).astype(np.float32)
                out[t, sel, s, c] = np.where(nrm < np.float32(1000.0), (num * nrm).astype(np.float32), np.float32(0.0))
    return out


def network_sum32(cc, weights):
    """The float32 fmaf chain over the channels of per-channel values (T, n_lags, S, C) -> (T, n_lags)."""
    T, n, S, C = cc.shape
    w = np.broadcast_to(np.asarray(weights, dtype=np.float32).reshape(T, S, -1), (T, S, C)).reshape(T, 1, S * C)
    acc = np.zeros((T, n), dtype=np.float32)
    flat = cc.reshape(T, n, S * C)
    for ch in range(S * C):
        acc = (acc.astype(np.float64) + w[..., ch].astype(np.float64) * flat[..., ch].astype(np.float64)).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------- inputs ---
def _zero_sum_ints(rng, shape, bound):
    """Integers in [-bound, bound] whose sums over the last axis are exactly 0 (length 1: zeros)."""
    x = rng.integers(-bound, bound + 1, shape).astype(np.int64)
    flat = x.reshape(-1, shape[-1])
    for row in flat:
        s = int(row.sum())
        while s != 0:
            k = int(rng.integers(0, row.size))
            step = -1 if s > 0 else 1
            if abs(row[k] + step) <= bound:
                row[k] += step
                s += step
    return flat.reshape(shape)


def run_of(regime, L, N):
    """(start, length) of the flat runs of regime "gaps": a zero-filled one and a constant one, each longer than L."""
    n = L + 37
    return ((N // 8, n), (N // 8 + n + max(L // 2, 9), n))


GAP_VALUE = 7.5


def mf_full_case(regime, L, N, step, seed, T=3, S=2, C=3, mv_lo=-40, mv_hi=60):
    """Inputs of one case: (templates, moveouts, weights, data).  Moveouts of both signs, one zero-weight channel per
    weighted template, template 1 without any weight, templates that carry an offset of their own (except in the exact
    regimes).  Data regimes: unit noise; noise on per-channel offsets of +-2^13 and +-2^12; a linear drift; an offset step
    in mid-trace; per-channel scales between 1e-4 and 1e4 (one channel under the energy guard); noise with a zero-filled and
    a constant run on channels 0 and 1; the two exact regimes.  Below L = 8 the noise lives on a lattice of 1/4, so that a
    window is either flat or has an energy far above the guard."""
    assert regime in REGIMES
    rng = np.random.default_rng(seed)
    n_ch = S * C

    def noise(shape):
        x = rng.standard_normal(shape)
        return np.round(x * 4) / 4 if L < 8 else x

    if regime == "int0":
        tp = _zero_sum_ints(rng, (T, S, C, L), 3).astype(np.float64)
        d = _zero_sum_ints(rng, (S, C, N), 3).astype(np.float64)
    elif regime == "periodic":
        assert L == PERIODIC_L and N % L == 0
        tp = _zero_sum_ints(rng, (T, S, C, L), 3).astype(np.float64)
        d = np.zeros((S, C, N))
        for p in PERIODS:
            d += np.tile(_zero_sum_ints(rng, (S, C, p), 2), N // p)
    else:
        tp = noise((T, S, C, L)) + np.resize([5.0, -2.0, 0.5], n_ch).reshape(1, S, C, 1)
        if L >= 2 and L < 8:
            tp[..., 0] += 1.0                                   # (never flat)
            tp[..., 1] -= 1.0
        d = noise((S, C, N))
        n = np.arange(N)
        if regime == "offset":
            d = d + (OFFSET * np.resize([1.0, -1.0, 0.5, 1.0, -0.5, 1.0], n_ch)).reshape(S, C, 1)
        elif regime == "drift":
            d = d + np.resize([200.0, -120.0, 60.0], n_ch).reshape(S, C, 1) * (2.0 * n / N - 1.0) + 20.0
        elif regime == "step":
            d = d + np.resize([300.0, -150.0], n_ch).reshape(S, C, 1) * (n >= N // 2)
        elif regime == "scaled":
            sd = np.resize([1e-3, 1e4, 1e-4, 1.0, 1e4, 1e-3], n_ch).reshape(S, C, 1)
            st = np.resize([1e3, 1e-2, 1e-3, 1.0, 1e-4, 1e4], n_ch).reshape(1, S, C, 1)
            d, tp = d * sd, tp * st
        elif regime == "gaps":
            (z0, zn), (k0, kn) = run_of(regime, L, N)
            assert k0 + kn < N
            d.reshape(n_ch, N)[0, z0:z0 + zn] = 0.0
            d.reshape(n_ch, N)[0, k0:k0 + kn] = GAP_VALUE
            d.reshape(n_ch, N)[1, z0:z0 + zn] = -GAP_VALUE
            d.reshape(n_ch, N)[1, k0:k0 + kn] = 0.0
    mv = rng.integers(mv_lo, mv_hi + 1, (T, S, C))
    w = rng.uniform(0.1, 1.0, (T, S, C))
    if regime in EXACT_REGIMES:
        w = rng.integers(1, 3, (T, S, C)).astype(np.float64)
    for t in range(T):
        mv.reshape(T, -1)[t, (t + 2) % n_ch] = mv_lo - (mv_lo % step == 0)      # first valid lag off the step grid
        z = (2 * t + 3) % n_ch
        if z != (t + 2) % n_ch and z > 1:                                      # (channels 0 and 1 hold the flat runs)
            w.reshape(T, -1)[t, z] = 0.0
            mv.reshape(T, -1)[t, z] = mv_hi + 77 if t % 2 else mv_lo - 77
    if T > 2:
        w[1] = 0.0                                                             # a template without any weight
    return tp.astype(np.float32), mv.astype(np.int32), w.astype(np.float32), d.astype(np.float32)


def mf_full_lags(args, step, seed, n_random=300, extra=()):
    """Lags to evaluate: the edges of every template's range, block and chunk seams, random ones, and `extra`."""
    tp, mv, w, d = args
    T, S, C, L = tp.shape
    N = d.shape[-1]
    n_corr = (N - L) // step + 1
    firsts, lasts = [], []
    for t in range(T):
        r = fa.mf_lag_range(mv[t], w[t], N, L, step)
        if r is not None:
            firsts.append(r[0])
            lasts.append(r[1])
    idx = fa.edge_sample(n_corr, firsts, lasts, n_random, seed, per_multiple=4, tail=6, multiples=(256, 1024, 4096, 8192))
    extra = np.asarray([e for e in extra if 0 <= e < n_corr], dtype=np.int64)
    return np.unique(np.concatenate([idx, extra]))


def gap_lags(args, step):
    """Lags whose windows straddle, touch or lie inside the flat runs of regime "gaps" on channels 0 and 1, for every
    template's moveout there."""
    tp, mv, w, d = args
    T, S, C, L = tp.shape
    N = d.shape[-1]
    out = []
    for (g0, gn) in run_of("gaps", L, N):
        for t in range(T):
            for ch in (0, 1):
                m = int(mv.reshape(T, -1)[t, ch])
                for start in (g0 - L, g0 - L + 1, g0 - 1, g0, g0 + 1, g0 + (gn - L) // 2, g0 + gn - L - 1, g0 + gn - L,
                              g0 + gn - L + 1, g0 + gn - 1, g0 + gn):
                    if (start - m) % step == 0:
                        out.append((start - m) // step)
    return out
