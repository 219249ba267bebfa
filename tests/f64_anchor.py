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

MF under mf.split16 (mf_split_f64: what the split kernel computes, in float64; B_split bounds |kernel - cc|, cc the
TRUE correlation above, not the split form).  With x' = x 2^s the scaled samples, hi = fp16(x'), rho = x' - hi,
lo_t = fp16(rho_t), lo'_d = fp16(rho_d 2^11), hs = fp16(hi_t 2^-11), num = sum (hi_t hi_d + hs lo'_d + lo_t hi_d):
    B_split = (E_rep + E_abs + E_acc) (1 + rho) + rho |cc|,   rho = gamma_L + 7u + E_term / |cc|
    E_rep = (3 + 2^-10) 2^-22 A              the two fp16 roundings of each kept lo half and the lo_t lo_d term left out
    E_abs = (1 + 2^-11) (2 * 2^-25 sum |d'| + 2^-36 sum |t'|) / (2^(s_t + s_d) sqrt(E_t E_d))
                                             fp16 operands that are subnormal: lo_t, hs (absolute error 2^-25 each) and lo'_d
    E_acc = gamma'_n_acc (1 + 2^-11)^2 (1 + 2^-10) A      [sum (|hi_t hi_d| + |hs lo'_d| + |lo_t hi_d|) is at most that]
            n_acc = 3 * 16 * nks * n_seg exact products into one float32 accumulator in ANY order, 2u per addition
            (gamma'_n = 2 n u / (1 - 2 n u)): the matrix pipe's summation order and rounding mode are not documented,
            and truncation cannot be excluded
    rho      the unchanged part of B: the chain of E_t, the normalisation, the prefix sums of E_d.
Exact regime of the split (mf_split_exact_ok): every fp16 operand exact and zero or normal, every window's
sum of |products| below 2^24 quanta -> the three products and every partial sum in any order are exact in float32.

The build zeroes r_t r_d >= 1000 and the definition E_t E_d <= 1e-6: the same threshold up to rounding, so
the definitions ASSERT that no active window has E_t E_d in [2.5e-7, 4e-6] -- a condition on the inputs.

Inter-template CC (intertp_f64: written from TemplateGroup.compute_intertemplate_cc of the reference, the header comment
of csrc/intertp.hip and DESIGN.md, not from the kernel body).  m = max_lag, L = Lw - 2m, w (T, n_ch) the base weights:
    per ordered pair (t, u) inside the mask, channel ch with w[t, ch] != 0, lag j = 0 .. 2m:
        cc_j, B_j   the MF definition above: template wf[u, ch, m : Lw - m], data wf[t, ch], moveout 0, step 1, N = Lw
                    (c_N = 1024 + ceil(Lw / 1024); 0 under the energy guard; the guard-window condition asserted)
        best = max_j cc_j  (max, not max |x|),   Bb = max_j B_j           [|max a - max b| <= max |a - b|]
    raw[t, u] = sum_ch w[t, ch] best
    B_raw     = sum_ch |w| Bb + gamma_(n_ch + 1) sum_ch |w| (|best| + Bb)
                one rounding of each product and an n_ch-term float32 sum in ANY order (the kernels sum in NumPy's
                pairwise order; the bound does not use it)
    sym   = (raw + raw^T) / 2
    B_sym = (B_raw + B_raw^T) / 2 + u (|sym| + (B_raw + B_raw^T) / 2)     the one float32 addition; halving is exact
raw is exactly +0 (compared bitwise) wherever B_raw = 0: pairs outside the mask, rows whose template has no weighted
channel, and pairs all of whose weighted channels are dead (all-zero) on either side or under the energy guard.  A dead
channel among live ones contributes an exact 0 with a zero bound.  Integer regime (waveforms in -3..3): B_j = 7u |cc_j|,
the rest of the bound unchanged (cc is no integer, the products w * best round).
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
    """The definition at `lags` (all n_corr of them when None): O(len(lags) * L) per template-channel.
    exact=True: integers of magnitude <= 3 (float32 exact throughout, B = 7u |cc|); exact="split": the wider
    exact regime of mf_split_exact_ok (numerators exact on both paths; the float32 chain of E_t is not exact for wide
    templates and keeps its term: B = (7u + gamma_L) |cc| there)."""
    return _mf_eval(templates, moveouts, weights, data, step, lags, exclusive_last_lag, range_all_channels,
                    sequential_csum, exact, None)


def _mf_eval(templates, moveouts, weights, data, step, lags, exclusive_last_lag, range_all_channels,
             sequential_csum, exact, split):
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
    if exact == "split":
        assert mf_split_exact_ok(tp32, data), "exact regime of the split: see mf_split_exact_ok"
    elif exact:
        assert np.abs(data).max() <= 3 and np.abs(tp32).max() <= 3 and 9 * L < EXACT_LIMIT
        assert np.array_equal(data, np.round(data)) and np.array_equal(tp32, np.round(tp32))
    ref = MFRef()
    ref.lags, ref.step, ref.w = lags, step, w
    ref.active = w != 0
    ref.cc = np.zeros((T, lags.size, S, C))
    ref.B = np.zeros((T, lags.size, S, C))
    ref.num = np.zeros((T, lags.size, S, C))            # the unscaled numerators sum_l t_l d_l
    if split is not None:
        # the three products of the split numerator, unscaled (hl: hs * lo'_d; hl_half: the same with lo'_d scaled by
        # 2^10, the planted defect "lo_scale"), and B_split
        ref.split_terms = {k: np.zeros_like(ref.cc) for k in ("hh", "lh", "hl", "hl_half")}
        ref.split_den, ref.B_split = np.full_like(ref.cc, np.inf), np.zeros_like(ref.cc)
    ref.valid = np.zeros((T, lags.size), dtype=bool)
    ref.zero_windows = 0            # valid entries whose data window is all exact zeros (a data gap): cc = B = 0
    for s in range(S):
        for c in range(C):
            if not ref.active[:, s, c].any():
                continue
            d = data[s, c]
            rows = np.lib.stride_tricks.sliding_window_view(d, L)          # rows[i] = d[i : i + L]
            if split is not None:
                sd = split_planes(d, SPLIT_LO_SCALE)
                # (lo'_d scaled by 2^10 instead: the planted defect "lo_scale")
                lo_half = (sd.rho * (SPLIT_LO_SCALE / 2)).astype(np.float16).astype(np.float64)
                # (fp16 values: float32 holds them exactly and halves the bytes the windows are gathered from)
                rows_hi, rows_lo, rows_lo_half = (np.lib.stride_tricks.sliding_window_view(x.astype(np.float32), L)
                                                  for x in (sd.hi, sd.lo, lo_half))
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
                if exact == "split" and E_t / _quantum(tmpl) ** 2 >= EXACT_LIMIT:
                    exact_B = (NORM_ROUNDINGS * U + gamma(L))          # (the float32 chain of E_t rounds)
                else:
                    exact_B = NORM_ROUNDINGS * U
                if split is not None:
                    st = split_planes(tmpl, 1.0)
                    hs = (st.hi * (1.0 / SPLIT_LO_SCALE)).astype(np.float16).astype(np.float64)
                    unscale = 2.0 ** -(st.s + sd.s)
                    n_acc = 3 * 16 * split_nks(L) * split_n_segments(L)
                sel = np.flatnonzero(ok)
                for j0 in range(0, sel.size, 256):
                    j = sel[j0:j0 + 256]
                    starts = lags[j] * step + mv[t, s, c]
                    assert starts.min() >= 0 and starts.max() + L <= N
                    win = rows[starts].astype(np.float64)
                    E_d = np.einsum("ij,ij->i", win, win)
                    prod = E_t * E_d
                    ref.zero_windows += int((E_d == 0).sum())
                    in_window = (prod >= GUARD_WINDOW[0]) & (prod <= GUARD_WINDOW[1])
                    assert not in_window.any(), \
                        f"input condition: E_t*E_d = {prod[in_window][0]:.3e} inside the guard window (t={t}, s={s}, c={c})"
                    keep = prod > GUARD
                    den = np.sqrt(np.where(keep, prod, 1.0))
                    num = win @ tmpl
                    cc = np.where(keep, num / den, 0.0)
                    a_sum, d_sum = (np.abs(win) @ np.stack([np.abs(tmpl), np.ones(L)], axis=1)).T
                    A = np.where(keep, a_sum / den, 0.0)
                    E_rel = 0.5 * c_N * 2.0 ** -53 * csum_total / np.where(keep, E_d, 1.0)
                    if exact:
                        B = exact_B * np.abs(cc)
                    else:
                        B = np.where(keep, gamma(L) * (A + np.abs(cc)) + (NORM_ROUNDINGS * U + E_rel) * np.abs(cc), 0.0)
                    ref.cc[t, j, s, c] = cc
                    ref.B[t, j, s, c] = B
                    ref.num[t, j, s, c] = num
                    if split is not None:
                        w_hi, w_lo = rows_hi[starts].astype(np.float64), rows_lo[starts].astype(np.float64)
                        hh, lh = (w_hi @ np.stack([st.hi, st.lo], axis=1)).T
                        hl = w_lo @ hs
                        hl_half = rows_lo_half[starts].astype(np.float64) @ hs if split == "defects" else hl
                        # sum of |products|: |hi| <= (1 + 2^-11) |x'|, |lo_t| and |hs lo'_d| / |hi_t| <= (1 + 2^-11) 2^-11 |x'|
                        p_abs = (1 + 2.0 ** -11) ** 2 * (1 + 2.0 ** -10) * a_sum / unscale
                        e_abs = (1 + 2.0 ** -11) * (2 * 2.0 ** -25 * d_sum * 2.0 ** -st.s
                                                   + 2.0 ** -36 * np.abs(tmpl).sum() * 2.0 ** -sd.s)
                        rho = gamma(L) + NORM_ROUNDINGS * U + E_rel
                        e_num = SPLIT_C_REP * A + (e_abs + gamma(2 * n_acc) * p_abs * unscale) / den
                        for k, v in (("hh", hh), ("lh", lh), ("hl", hl), ("hl_half", hl_half)):
                            ref.split_terms[k][t, j, s, c] = v * unscale
                        ref.split_den[t, j, s, c] = np.where(keep, den, np.inf)
                        ref.B_split[t, j, s, c] = np.where(keep, e_num * (1 + rho) + rho * np.abs(cc), 0.0)
    ref.net, ref.B_net = _mf_network(ref.cc, ref.cc, ref.B, w)
    return ref


def _mf_network(cc, cc_true, B, w):
    """The weighted sum of `cc` and the bound of a float32 fmaf chain over the S * C channels on per-channel values
    that lie within B of cc_true."""
    S, C = w.shape[1:]
    aw = np.abs(w)[:, None]
    return ((cc * w[:, None]).sum(axis=(2, 3)),
            (B * aw).sum(axis=(2, 3)) + gamma(S * C) * (np.abs(cc_true) * aw).sum(axis=(2, 3)))


# ----------------------------------------------------------- matched filter under mf.split16 ---
# Written from the header comment of csrc/mf_split.h and DESIGN.md s4 "MF, split precision", not from the kernel.
SPLIT_S_TARGET, SPLIT_S_CLAMP = 14, 60          # a channel's largest magnitude scaled into [2^14, 2^15); |s| <= 60
SPLIT_LO_SCALE = 2.0 ** 11                      # the data's lo halves are stored times 2^11, paired with fp16(hi_t 2^-11)
SPLIT_SEGMENT = 376                             # samples one band image holds; longer templates in equal segments
SPLIT_C_REP = (3 + 2.0 ** -10) * 2.0 ** -22     # E_rep / A (module docstring)
SPLIT_DROPS = ("hi_lo", "lo_hi", "lo_scale")


def split_n_segments(L):
    return -(-L // SPLIT_SEGMENT)


def split_nks(L):
    """k-steps of 16 per segment: segments of equal length, a multiple of 8, each with a band of seg_len + 38."""
    seg_len = -(-(-(-L // split_n_segments(L))) // 8) * 8
    return (seg_len + 38 + 15) // 16


class SplitPlanes:
    """s: the scale exponent; hi = fp16(x 2^s); lo = fp16((x 2^s - hi) * lo_scale); rho = x 2^s - hi, as float64."""


def split_planes(x, lo_scale):
    x = np.asarray(x, dtype=np.float64)
    p = SplitPlanes()
    m = float(np.abs(x).max(initial=0.0))
    p.s = 0
    if m > 0 and np.isfinite(m):
        p.s = int(np.clip(SPLIT_S_TARGET - (np.frexp(m)[1] - 1), -SPLIT_S_CLAMP, SPLIT_S_CLAMP))
    p.scaled = x * 2.0 ** p.s
    with np.errstate(over="ignore"):
        p.hi = p.scaled.astype(np.float16).astype(np.float64)
    assert np.isfinite(p.hi).all(), "input condition: a scaled sample beyond fp16 (the clamp |s| <= 60 is active)"
    p.rho = p.scaled - p.hi
    p.lo = (p.rho * lo_scale).astype(np.float16).astype(np.float64)
    return p


def mf_split_f64(templates, moveouts, weights, data, step=1, lags=None, exclusive_last_lag=False,
                 range_all_channels=False, sequential_csum=False, exact=False, drop=None, _true=None):
    """What mf.split16 computes, in float64: .cc / .net / .num the split form (norms, guard, lag ranges and the
    weighted sum as in mf_f64), .B / .B_net = B_split, the bound of |kernel - TRUE cc| (module docstring), .true the
    mf_f64 result at the same lags.  `drop` plants a defect IN THIS DEFINITION for the sensitivity tests: "hi_lo" /
    "lo_hi" leave a product out, "lo_scale" scales the data's lo halves by 2^10 against the 2^-11 of hs (pass the
    result's .true of a call with a `drop` as `_true` and the next variant costs nothing)."""
    assert drop is None or drop in SPLIT_DROPS
    true = _true or _mf_eval(templates, moveouts, weights, data, step, lags, exclusive_last_lag, range_all_channels,
                             sequential_csum, exact, "defects" if drop else "plain")
    terms = true.split_terms
    ref = MFRef()
    ref.true, ref.lags, ref.step, ref.w, ref.active, ref.valid = true, true.lags, step, true.w, true.active, true.valid
    ref.zero_windows = true.zero_windows
    ref.num = terms["hh"] + (0.0 if drop == "lo_hi" else terms["lh"]) + \
        (0.0 if drop == "hi_lo" else terms["hl_half" if drop == "lo_scale" else "hl"])
    ref.cc, ref.B = ref.num / true.split_den, true.B_split
    ref.net, ref.B_net = _mf_network(ref.cc, true.cc, ref.B, true.w)
    return ref


def mf_split_anchor(sref):
    """The reference mf_compare judges a split16 KERNEL by: the true correlation with B_split around it."""
    ref = MFRef()
    ref.lags, ref.step, ref.w, ref.active, ref.valid = sref.lags, sref.step, sref.w, sref.active, sref.valid
    ref.cc, ref.net, ref.B, ref.B_net = sref.true.cc, sref.true.net, sref.B, sref.B_net
    return ref


def mf_split_lags(args, step, seed, n_random=2400, extra=(), **range_kw):
    """The sampled lags of a split16 case: first and last valid lag of every template with their neighbours and the
    tail behind, the neighbours of multiples of 1024, 2048 and 8192 (tile, wave and workgroup of the split kernel),
    `extra`, and seeded random ones -- more than 2000 in all."""
    tp, mv, w, d = args
    N, L = d.shape[-1], tp.shape[-1]
    rg = [mf_lag_range(mv[t], w[t], N, L, step, **range_kw) for t in range(tp.shape[0])]
    lags = edge_sample((N - L) // step + 1, [r[0] for r in rg] + list(extra), [r[1] for r in rg], n_random, seed,
                       multiples=(1024, 2048, 8192))
    assert lags.size >= min(2000, n_random)
    return lags


def mf_rms_ratio(got, exact_path, sref, network_sum, what="MF split16"):
    """The sharp check of a split16 result: per channel (per template row for network sums), over the sampled valid
    lags, rms(got - cc) / rms(exact_path - cc) with cc the true float64 correlation and `exact_path` the float32
    chain's result (the oracle's) at the same lags.  Returns the ratios (NaN where the exact path's error is 0:
    there `got` must have none either, which is asserted)."""
    true = sref.true
    want = true.net if network_sum else true.cc
    got, exact_path = np.asarray(got, np.float64), np.asarray(exact_path, np.float64)
    assert got.shape == want.shape == exact_path.shape, (got.shape, want.shape, exact_path.shape)
    valid = sref.valid if network_sum else sref.valid[:, :, None, None] & np.ones(want.shape, bool)
    n = np.maximum(valid.sum(axis=1), 1)
    rms_got = np.sqrt((np.where(valid, got - want, 0.0) ** 2).sum(axis=1) / n)
    rms_exact = np.sqrt((np.where(valid, exact_path - want, 0.0) ** 2).sum(axis=1) / n)
    assert not rms_got[rms_exact == 0].any(), f"{what}: an error where the exact path has none"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(rms_exact > 0, rms_got / rms_exact, np.nan)
    return ratio, rms_exact


def mf_rms_require(got, exact_path, sref, network_sum, K, what):
    ratio, _ = mf_rms_ratio(got, exact_path, sref, network_sum, what)
    worst = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else 0.0
    print(f"f64-anchor {what}: rms(kernel - f64) / rms(exact path - f64) worst {worst:.3f}, "
          f"median {float(np.nanmedian(ratio)) if worst else 0.0:.3f} (K = {K})")
    assert worst <= K, f"{what}: rms ratio {worst:.3f} > K = {K}"
    return worst


def _quantum(x):
    """The largest power of two that divides every non-zero element (1 for none)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[x != 0]
    if not x.size:
        return 1.0
    m, e = np.frexp(x)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.frexp((mi & -mi).astype(np.float64))[1] - 1
    return 2.0 ** int((e - 53 + tz).min())


FP16_MIN_NORMAL = 2.0 ** -14


def mf_split_exact_ok(templates, data):
    """The exact regime of mf.split16.  Per template channel and data channel: hi + lo reproduce the scaled sample
    (nothing is left for an error term), hs = hi_t 2^-11 exactly, every fp16 operand is zero or normal, and with q_t,
    q_d the quanta of the two channels every window -- at every offset of the trace -- has
    sum_l (|hi_t hi_d| + |hs lo'_d| + |lo_t hi_d|) < 2^24 q_t q_d: every product and every partial sum in any order is
    an integer multiple of q_t q_d below 2^24 of them, exact in float32.  Also sum d^2 < 2^53 q_d^2 (the prefix sums)."""
    tp = np.asarray(templates)
    d = np.asarray(data)
    T, S, C, L = tp.shape
    N = d.shape[-1]
    nfft = 1 << int(np.ceil(np.log2(N + L)))

    def normal(*planes):
        return all(((x == 0) | (np.abs(x) >= FP16_MIN_NORMAL)).all() for x in planes)

    for s in range(S):
        for c in range(C):
            sd = split_planes(d[s, c], SPLIT_LO_SCALE)
            if not (np.array_equal(sd.lo, sd.rho * SPLIT_LO_SCALE) and normal(sd.hi, sd.lo)):
                return False
            q_d = _quantum(np.concatenate([sd.hi, sd.rho]))
            if float((sd.scaled / q_d) @ (sd.scaled / q_d)) >= 2.0 ** 53:
                return False
            f_hi, f_lo = (np.fft.rfft(np.abs(x) / q_d, nfft) for x in (sd.hi, sd.rho))
            for t in range(T):
                st = split_planes(tp[t, s, c], 1.0)
                hs = (st.hi / SPLIT_LO_SCALE).astype(np.float16).astype(np.float64)
                if not (np.array_equal(st.lo, st.rho) and np.array_equal(hs * SPLIT_LO_SCALE, st.hi)
                        and normal(st.hi, st.lo, hs)):
                    return False
                q_t = _quantum(np.concatenate([st.hi, st.rho]))
                # sum_l a_l b_(i + l) at every offset i, in quanta (integers: the FFT's rounding is rounded away, and
                # one quantum of margin is left for it)
                a_hi, a_lo = np.abs(st.hi) / q_t, np.abs(st.rho) / q_t
                corr = np.fft.irfft(f_hi * np.conj(np.fft.rfft(a_hi + a_lo, nfft))
                                    + f_lo * np.conj(np.fft.rfft(a_hi, nfft)), nfft)[:N - L + 1]
                if np.round(corr).max(initial=0.0) + 1 >= EXACT_LIMIT:
                    return False
    return True


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


# ----------------------------------------------------------------------------- inter-template CC ---
INTERTP_MAX_LAG = 31                             # the batched kernel holds 2 * 31 + 1 = 63 lags per pair
INTERTP_LDS_FLOATS = 64 * 1024 // 4              # the batched launch's LDS budget
INTERTP_TILE = 8                                 # templates u per workgroup
INTERTP_DROPS = ("first_lag", "last_lag", "trim", "tail", "abs_max", "w_u", "mask_T", "last_channel", "lds_chunk",
                 "no_sym")


def intertp_lds_chunk(n_ch, Lw, max_lag):
    """Channels of one template the batched launch stages per LDS pass: the largest c <= n_ch with
    c * Lw + 8 * c * n_lag + 8 * n_ch floats within 64 KB (the data rows, the CCs of a tile of 8 templates, their
    weighted maxima); 0 where one channel does not fit (workflow.intertemplate_cc then takes the per-template loop)."""
    n_lag = 2 * max_lag + 1
    room = INTERTP_LDS_FLOATS - INTERTP_TILE * n_ch
    return int(max(0, min(n_ch, room // (Lw + INTERTP_TILE * n_lag))))


class IntertpRef:
    """raw, B_raw: (T, T) the un-symmetrised matrix and its bound; sym, B_sym: the symmetrised ones; zero: (T, T) where
    raw must be exactly +0; live: (T, T, n_ch) the (pair, channel) entries the definition computes; best, Bb: (T, T, n_ch)
    max over the lags and its bound; arg: (T, T, n_ch) the lag of the maximum."""


def intertp_f64(waveforms, base_weights, pair_mask, max_lag, exact=False, drop=None):
    """The definition of the module docstring, vectorised over pairs, channels and lags.  exact=True: the integer regime.
    `drop` plants a defect IN THIS DEFINITION for the sensitivity tests: "first_lag" / "last_lag" leave that lag out,
    "trim" cuts the templates at m + 1 (the three need max_lag >= 1 and change nothing at 0), "tail" leaves the last L % 8
    samples out of the numerators, "abs_max" takes max |cc|, "w_u" weights pair (t, u) with w[u], "mask_T" transposes the
    mask, "last_channel" leaves the last channel out of the sum, "lds_chunk" every channel behind the first
    intertp_lds_chunk ones, "no_sym" returns raw as sym."""
    assert drop is None or drop in INTERTP_DROPS
    wf32 = np.asarray(waveforms)
    T, S, C, Lw = wf32.shape
    n_ch, m = S * C, int(max_lag)
    L, n_lag = Lw - 2 * m, 2 * m + 1
    assert m >= 0 and L >= 1
    wf = wf32.reshape(T, n_ch, Lw).astype(np.float64)
    w = np.asarray(base_weights).reshape(T, n_ch).astype(np.float64)
    mask = np.asarray(pair_mask, dtype=bool).reshape(T, T)
    if drop == "mask_T":
        mask = mask.T
    if exact:
        assert np.abs(wf).max() <= 3 and 9 * L < EXACT_LIMIT and np.array_equal(wf, np.round(wf))
    c_N = CSUM_CHUNK + -(-Lw // CSUM_CHUNK)
    t0 = m + (1 if drop == "trim" and m else 0)
    tp = wf[:, :, t0:t0 + L]                                                           # (u, ch, l)
    win = np.lib.stride_tricks.sliding_window_view(wf, L, axis=-1)                     # (t, ch, lag, l)
    assert win.shape[2] == n_lag
    win_c = np.ascontiguousarray(win.transpose(1, 0, 2, 3)).reshape(n_ch, T * n_lag, L)
    tp_c = np.ascontiguousarray(tp.transpose(1, 2, 0))                                 # (ch, l, u)
    n_num = L - L % 8 if drop == "tail" else L

    def pairs(x):                                                                      # (ch, t * lag, u) -> (t, u, ch, lag)
        return x.reshape(n_ch, T, n_lag, T).transpose(1, 3, 0, 2)

    num = pairs(np.matmul(win_c[:, :, :n_num], tp_c[:, :n_num]))
    a_sum = pairs(np.matmul(np.abs(win_c), np.abs(tp_c)))
    E_d = np.einsum("cil,cil->ci", win_c, win_c).reshape(n_ch, T, n_lag).transpose(1, 0, 2)      # (t, ch, lag)
    E_t = np.einsum("ucl,ucl->uc", tp, tp)                                             # (u, ch)
    csum_total = np.einsum("tcn,tcn->tc", wf, wf)
    prod = E_t[None, :, :, None] * E_d[:, None, :, :]
    w_pair = np.broadcast_to(w[None, :, :] if drop == "w_u" else w[:, None, :], (T, T, n_ch))
    live = mask[:, :, None] & (w_pair != 0)
    in_window = live[..., None] & (prod >= GUARD_WINDOW[0]) & (prod <= GUARD_WINDOW[1])
    assert not in_window.any(), \
        f"input condition: E_t*E_d = {prod[in_window][0]:.3e} inside the guard window at (t, u, ch, lag) {np.argwhere(in_window)[0]}"
    keep = prod > GUARD
    den = np.sqrt(np.where(keep, prod, 1.0))
    cc = np.where(keep, num / den, 0.0)
    if exact:
        B = NORM_ROUNDINGS * U * np.abs(cc)
    else:
        A = np.where(keep, a_sum / den, 0.0)
        E_rel = 0.5 * c_N * 2.0 ** -53 * csum_total[:, None, :, None] / np.where(keep, E_d[:, None], 1.0)
        B = np.where(keep, gamma(L) * (A + np.abs(cc)) + (NORM_ROUNDINGS * U + E_rel) * np.abs(cc), 0.0)
    lags = slice(1 if drop == "first_lag" and m else 0, n_lag - (1 if drop == "last_lag" and m else 0))
    pick = np.abs(cc[..., lags]) if drop == "abs_max" else cc[..., lags]
    ref = IntertpRef()
    ref.live = live
    ref.arg = np.where(live, pick.argmax(axis=-1) + lags.start, -1)
    ref.best = np.where(live, pick.max(axis=-1), 0.0)
    ref.Bb = np.where(live, B[..., lags].max(axis=-1), 0.0)
    summed = np.ones(n_ch, dtype=bool)
    if drop == "last_channel":
        summed[n_ch - 1] = False
    elif drop == "lds_chunk":
        summed[intertp_lds_chunk(n_ch, Lw, m):] = False
    aw = np.abs(w_pair) * summed
    ref.raw = (w_pair * summed * ref.best).sum(axis=-1)
    ref.B_raw = (aw * ref.Bb).sum(axis=-1) + gamma(n_ch + 1) * (aw * (np.abs(ref.best) + ref.Bb)).sum(axis=-1)
    ref.zero = ref.B_raw == 0
    half = (ref.B_raw + ref.B_raw.T) / 2
    ref.sym = ref.raw if drop == "no_sym" else (ref.raw + ref.raw.T) / 2
    ref.B_sym = half + U * (np.abs(ref.sym) + half)
    return ref


def intertp_compare(got, ref, raw=None, what="inter-template CC"):
    """`got`: the float32 symmetrised matrix, |got - sym| <= B_sym entry by entry; `raw` (optional): the float32 matrix
    before the symmetrisation, |raw - f64| <= B_raw and bitwise +0 wherever ref.zero."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.sym.shape, (got.dtype, got.shape, ref.sym.shape)
    err, B = np.abs(got.astype(np.float64) - ref.sym), ref.B_sym
    bad = ~(err <= B)                                      # (NaN fails)
    detail = ""
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        detail = f"first at {i}: got {got[i]!r}, f64 {ref.sym[i]!r}, B_sym {B[i]:.3e}"
    worst = _worst(err, B)
    if raw is not None:
        raw = np.ascontiguousarray(raw)
        assert raw.dtype == np.float32 and raw.shape == ref.raw.shape
        err_r = np.abs(raw.astype(np.float64) - ref.raw)
        bad_r = ~(err_r <= ref.B_raw) | (ref.zero & (raw.view(np.uint32) != 0))
        if bad_r.any() and not detail:
            i = tuple(int(x) for x in np.argwhere(bad_r)[0])
            detail = f"first (before the symmetrisation) at {i}: got {raw[i]!r}, f64 {ref.raw[i]!r}, B_raw {ref.B_raw[i]:.3e}"
        bad, worst = np.concatenate([bad.ravel(), bad_r.ravel()]), max(worst, _worst(err_r, ref.B_raw))
    return Report(what, bad, worst, detail)


# ----------------------------------------------------------------------------- sampled indices ---
EDGE_MULTIPLES = (128, 256, 512, 2048, 8192)


def edge_sample(n, firsts, lasts, n_random, seed, per_multiple=12, tail=24, multiples=EDGE_MULTIPLES):
    """Sorted unique indices in [0, n): 0 and n - 1; every `firsts` / `lasts` index (first / last valid lag or
    sample) with its neighbours, and `tail` indices behind each `lasts` (the strict tail); the neighbours
    -1, 0, +1 of `per_multiple` multiples of 128, 256, 512, 2048 and 8192 (or of `multiples`) spread over the axis;
    seeded random."""
    idx = [0, n - 1]
    for x in list(firsts) + list(lasts):
        idx += [x - 1, x, x + 1]
    for x in lasts:
        idx += list(range(x + 1, x + 1 + tail)) + [(x + n) // 2]
    for m in multiples:
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


SPLIT_EXACT_REGIMES = ("int", "int_wide_data", "int_wide_templates")
SPLIT_GENERAL_REGIMES = ("noise", "scaled", "glitch")
# which planted defect (mf_split_f64's `drop`) each exact regime exposes: "int" has no lo halves at all
SPLIT_EXACT_DROPS = {"int": (), "int_wide_data": ("hi_lo", "lo_scale"), "int_wide_templates": ("lo_hi",)}
WIDE_MAX_L = 682                                 # 3 * (2 * 4096 + 3) * L < 2^24


def mf_split_case(regime, L, N, step, seed, T=3, S=2, C=3):
    """Inputs of one mf.split16 case (T * S * C = 18 template channels): 16 live ones whose moveouts hold every
    remainder mod 8 with both signs, one zero-weight channel with a moveout beyond every weighted one, one dead
    (all-zero) weighted template channel, a data gap of exact zeros; the most negative weighted moveout of every
    template is no multiple of the step.
    Exact regimes (mf_split_exact_ok), every channel times its own power of two (data 2^7, 1, 2^-9; templates 2^-9, 1,
    2^11): "int" integers in -3..3 (hi * hi only); "int_wide_data" data 4096 a + b, b in -3..3, a in -2..2 and
    templates in -3..3 -- a in -1..1 and templates in -1..1 beyond L = 682 -- (hi_t * lo_d); "int_wide_templates" its
    mirror image (lo_t * hi_d).
    General regimes: "noise"; "scaled" (mf_case's: per-channel scales 1e-6..1e4, a glitch of 3e4 sigma); "glitch" (a
    sample of 3e4 sigma in unit noise, and a channel at 1e-7 whose last sample is 1 -- every other sample of it 2^-23 of
    the channel's maximum, lo halves in fp16's subnormal range unless stored scaled -- with its templates at 1e6)."""
    assert T * S * C == 18 and L >= 8
    rng = np.random.default_rng(seed)
    n_ch = S * C
    if regime in SPLIT_EXACT_REGIMES:
        small, a_max = (3, 2) if L <= WIDE_MAX_L else (1, 1)

        def ints(shape, wide):
            b = rng.integers(-3, 4, shape) if wide else rng.integers(-small, small + 1, shape)
            return (4096 * rng.integers(-a_max, a_max + 1, shape) * wide + b).astype(np.float64)

        if regime == "int":
            small = 3
        tp = ints((T, S, C, L), regime == "int_wide_templates")
        d = ints((S, C, N), regime == "int_wide_data")
        d *= np.resize([2.0 ** 7, 1.0, 2.0 ** -9], n_ch).reshape(S, C, 1)
        tp *= np.resize([2.0 ** -9, 1.0, 2.0 ** 11], n_ch).reshape(1, S, C, 1)
        w = rng.integers(1, 3, (T, S, C)).astype(np.float64)
    else:
        tp, d = rng.standard_normal((T, S, C, L)), rng.standard_normal((S, C, N))
        w = rng.uniform(0.1, 1.0, (T, S, C))
        if regime == "scaled":
            d[S - 1, C - 1, N // 3] = 3e4
            d *= np.resize([1e-6, 1e-3, 1e-1, 1.0, 1e2, 1e4], n_ch).reshape(S, C, 1)
            tp *= np.resize([1e-3, 1e3, 1e1, 1.0, 1e-2, 1e-4], n_ch).reshape(1, S, C, 1)
        elif regime == "glitch":
            d[0, 1, N // 3] = 3e4
            d[1, 1] *= 1e-7
            d[1, 1, N - 1] = 1.0        # (the last sample: the prefix sums in front of it, and so the exact path's window
                                        #  norms, stay accurate -- what the rms ratio is measured against)
            tp[:, 1, 1] *= 1e6
        else:
            assert regime == "noise"
    # the 16 live moveouts: remainder r = 0..7, one positive (8 k + r) and one negative (-8 k + r) each, the negative
    # ones dealt over the templates
    pos = list(rng.permutation([8 * int(rng.integers(1, 50)) + r for r in range(8)]))
    neg = list(rng.permutation([-8 * int(rng.integers(2, 10)) + r for r in range(8)]))
    mv = np.zeros((T, n_ch), dtype=np.int64)
    flat_w = w.reshape(-1)
    zero_w, dead = 0 * n_ch + 3 % n_ch, (T - 1) * n_ch + 1            # (template 0, channel 3), (template T - 1, channel 1)
    for t in range(T):
        live = [i for i in range(n_ch) if t * n_ch + i not in (zero_w, dead)]
        n_neg = -(-(len(neg) * len(live)) // (len(neg) + len(pos)))
        vals = [neg.pop() for _ in range(n_neg)] + [pos.pop() for _ in range(len(live) - n_neg)]
        mv[t, live] = rng.permutation(vals)
        k = live[int(np.argmin(mv[t, live]))]
        if mv[t, k] % step == 0:                                 # first valid lag off the step grid (same remainder mod 8)
            mv[t, k] -= 8
    assert not pos and not neg
    mv.reshape(-1)[dead] = 17
    flat_w[zero_w] = 0.0
    mv.reshape(-1)[zero_w] = mv.min() - 333
    g0 = N // 2
    d[0, 0, g0:g0 + L + 50] = 0.0                                # a data gap: 51 windows of exact zeros
    tp.reshape(T * n_ch, L)[dead] = 0.0
    mv = mv.reshape(T, S, C)
    res = set((int(m) % 8, bool(m < 0)) for i, m in enumerate(mv.ravel()) if i not in (zero_w, dead))
    assert len(res) == 16, "every remainder mod 8 with both signs among the live moveouts"
    return (tp.astype(np.float32), mv.astype(np.int32), w.astype(np.float32), d.astype(np.float32))


# The shapes of tests/test_gpu_split16_anchor.py, which tests/test_split16_definition.py walks on the CPU.
SPLIT_N = 20011                                  # > 8192 + L: three lag blocks; no multiple of 8: a partial last q-chunk
SPLIT_MAX_L = 2049                               # the longest template of the MFMA kernels (include/bpmf_hip.h)
SPLIT_LENGTHS = (8, 32, 100, 257, 376, 377, 379, 752, 753, 1040, 2040, SPLIT_MAX_L)
SPLIT_STEP3_LENGTHS = (32, 257, 379, 1040)       # step 3 in the host-call tests (1 at the other lengths)
SPLIT_RESIDENT_LENGTHS = (376, 753)              # MatchedFilterGPU on a prepared day, with the other step
SPLIT_SWITCH_SHAPES = ((100, 1), (379, 3))       # (L, step) of the mf.compat_* tests, regimes "noise" and "scaled"
# Allowed rms(kernel - f64) / rms(exact float32 path - f64) per template length: K = 3 x SPLIT_RMS_MEASURED, the worst
# ratio of any channel, regime, step and entry point at that length on an MI355X (DESIGN.md s3,
# profiles/split16_anchor.txt); the factor 3 covers the spread of an rms over ~2000 samples from seed to seed and an
# accumulation order that changes with the k-step and segment counts.  tests/test_split16_definition.py holds K to the
# sensitivity condition: every planted defect of the definition exceeds K by a factor of 8 at least.
SPLIT_RMS_MEASURED = {8: 2.268, 32: 1.218, 100: 0.954, 257: 0.887, 376: 0.862, 377: 0.828, 379: 0.876, 752: 0.863,
                      753: 0.801, 1040: 0.814, 2040: 0.787, 2049: 0.815}
SPLIT_RMS_K = {L: round(3 * r, 1) for L, r in SPLIT_RMS_MEASURED.items()}
assert tuple(SPLIT_RMS_K) == SPLIT_LENGTHS


def split_exact_seed(L):
    return 2000 + L


def split_general_seed(L):
    return 3000 + L


def split_step_of(L):
    return 3 if L in SPLIT_STEP3_LENGTHS else 1


def split_gpu_cases():
    """(regime, L, step) of every case the GPU tests run (the compat switches add lag-range rules, not inputs)."""
    cases = [(r, L, split_step_of(L)) for L in SPLIT_LENGTHS for r in SPLIT_EXACT_REGIMES + SPLIT_GENERAL_REGIMES]
    cases += [(r, L, 4 - split_step_of(L)) for L in SPLIT_RESIDENT_LENGTHS
              for r in ("int_wide_data", "int_wide_templates", "glitch")]
    cases += [(r, L, step) for L, step in SPLIT_SWITCH_SHAPES for r in ("noise", "scaled")]
    return sorted(set(cases), key=lambda x: (x[1], x[2], x[0]))


def split_glitch_lags(L, step):
    """Lags whose windows hold the sample of 3e4 sigma of the "scaled" and "glitch" regimes (at N // 3)."""
    return ((SPLIT_N // 3 - L // 2) // step, (SPLIT_N // 3 - L) // step, (SPLIT_N // 3) // step)


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


# ----------------------------------------------------------------------------- inter-template CC: inputs ---
INTERTP_REGIMES = MF_REGIMES + ("int",)
INTERTP_SCALES = (1.0, 1e-3, 1e-1, 1e2, 1e4)     # "scaled": (L sigma^2)^2 is ~1e-8 at 1e-3 and >= 0.4 at 1e-1 for L >= 64


def intertp_case(regime, T, S, C, Lw, max_lag, seed):
    """Inputs of one inter-template case: (waveforms (T, S, C, Lw), base weights (T, S, C), pair mask (T, T)), float32 / bool.
    As many of these as T holds:  template 1 = template 0 rolled by +max_lag and template 2 by -max_lag (the best lag of
    the pairs with template 0 is the last / the first one);  template 3 = minus template 0 rolled by max_lag // 2 (max
    and max |x| differ by about 1);  template 4 without any weighted channel;  a dead (all-zero) channel 1 of template 5
    (of the last template below T = 6, where there are two channels);  row 6 of the mask empty.  Base weights differ from
    row to row, with zeros from 3 channels on.  The mask holds every pair among templates 0..3 that involves template 0
    and the diagonal, is random elsewhere and not symmetric: (1, 2), (3, 1), (2, 3) are set and their transposes are not.
    Regimes as mf_case; "scaled": one scale per channel, INTERTP_SCALES in turn (the channels at 1e-3 fall under the energy
    guard); "int": waveforms in -3..3 and weights in 0..2."""
    rng = np.random.default_rng(seed)
    n_ch, m = S * C, int(max_lag)
    L = Lw - 2 * m
    if regime == "int":
        wf = rng.integers(-3, 4, (T, n_ch, Lw)).astype(np.float64)
        if L < 8:
            wf[wf == 0] = 1
    elif regime == "sine":
        om = 2 * np.pi / 23.0
        wf = np.sin(om * np.arange(Lw) + rng.uniform(0, 2 * np.pi, (T, n_ch, 1))) + 0.01 * rng.standard_normal((T, n_ch, Lw))
        if L < 8:
            wf = wf + 1.5
    else:
        wf = rng.standard_normal((T, n_ch, Lw))
        if L < 8:                                                # (keep a window of a few samples away from zero energy)
            wf = np.sign(wf) * (0.5 + np.abs(wf))
        if regime == "dc":
            wf = wf + 50.0
        elif regime == "scaled":
            assert L >= 64
            wf = wf * np.resize(INTERTP_SCALES, n_ch).reshape(1, n_ch, 1)
        else:
            assert regime == "noise"
    if T > 1:
        wf[1] = np.roll(wf[0], m, axis=-1)
    if T > 2:
        wf[2] = np.roll(wf[0], -m, axis=-1)
    if T > 3:
        wf[3] = -np.roll(wf[0], m // 2, axis=-1)
    if regime == "int":
        w = rng.integers(1, 3, (T, n_ch)).astype(np.float64)
    else:
        w = rng.uniform(0.1, 1.0, (T, n_ch))
    if n_ch >= 3:
        w[rng.random((T, n_ch)) < 0.25] = 0.0
        w[:, :2] = np.where(w[:, :2] == 0, 1.0, w[:, :2])        # channels 0 and 1 stay weighted
        w[0, n_ch - 1] = 1.0                                     # ... and the last one in row 0
    if T > 4:
        w[4] = 0.0                                               # a template without any weighted channel
    if n_ch >= 2 or T > 5:
        wf[5 if T > 5 else T - 1, 1 % n_ch] = 0.0                # a dead channel
    mask = rng.random((T, T)) < 0.6
    mask[np.arange(T), np.arange(T)] = True
    k = min(T, 4)
    mask[0, :k] = mask[:k, 0] = True
    for a, b in ((1, 2), (3, 1), (2, 3)):
        if a < T and b < T:
            mask[a, b], mask[b, a] = True, False
    if T > 6:
        mask[6] = False                                          # a template without any partner
    return (wf.reshape(T, S, C, Lw).astype(np.float32), w.reshape(T, S, C).astype(np.float32), mask)


# The shapes of tests/test_gpu_intertp_anchor.py, which tests/test_intertp_definition.py walks on the CPU:
# name -> (T, S, C, Lw, max_lag).
INTERTP_ROWS = {
    "1 63 lags, L=3": (9, 1, 1, 65, 31),
    "2 L=8, one full tile, 7 channels": (8, 1, 7, 70, 31),
    "3 L=17, 8 channels": (7, 2, 4, 79, 31),
    "4 33 lags, 9 channels, three tiles": (17, 3, 3, 96, 16),
    "5 129 channels": (16, 43, 3, 96, 5),
    "6 136 channels": (5, 34, 4, 96, 5),
    "7 137 channels": (3, 137, 1, 96, 5),
    "8 84 channels = 2 chunks of 42": (3, 28, 3, 200, 10),
    "9 Lw=1054 across the first prefix-sum chunk": (4, 1, 2, 1054, 20),
    "10 Lw=2078 across the second prefix-sum chunk": (3, 1, 2, 2078, 31),
    "11a Lw=1": (3, 1, 1, 1, 0),
    "11b T=1": (1, 2, 3, 40, 4),
}
INTERTP_ROWS.update({f"12 m={m} L={L}": (9, 2, 3, L + 2 * m, m) for m in (3, 4, 7, 8, 28) for L in (7, 9, 15, 16)})
INTERTP_ALL_REGIME_ROWS = ("4 33 lags, 9 channels, three tiles", "6 136 channels")
# (n_ch, Lw, max_lag) -> the LDS passes of the batched launch, by intertp_lds_chunk
INTERTP_CHUNKS = {"5 129 channels": (83, 46), "7 137 channels": (83, 54), "8 84 channels = 2 chunks of 42": (42, 42)}


def intertp_regimes_of(row):
    return INTERTP_REGIMES if row in INTERTP_ALL_REGIME_ROWS else ("noise", "int")


def intertp_seed(row):
    return 5000 + list(INTERTP_ROWS).index(row)


def intertp_features(args, ref, max_lag):
    """What a case holds of the list in intertp_case, counted on the definition: a dict of booleans."""
    wf, w, mask = args
    T = wf.shape[0]
    n_ch = w[0].size
    m, n_lag = int(max_lag), 2 * int(max_lag) + 1
    ch0 = ref.live[..., 0]
    dead = ~np.asarray(wf).reshape(T, n_ch, -1).any(axis=-1)                         # (T, n_ch)
    dead_live = ref.live & (dead[:, None, :] | dead[None, :, :])
    assert not ref.best[dead_live].any() and not ref.Bb[dead_live].any()
    return {
        "last_lag_best": T > 1 and bool(ch0[1, 0]) and ref.arg[1, 0, 0] == n_lag - 1 and ref.best[1, 0, 0] > 0.999,
        "first_lag_best": T > 2 and bool(ch0[2, 0]) and ref.arg[2, 0, 0] == 0 and ref.best[2, 0, 0] > 0.999,
        "negated": T > 3 and bool(ch0[3, 0]) and ref.best[3, 0, 0] < 0.9,
        "dead_channel": bool(dead_live.any()),
        "unweighted_row": bool((~(np.asarray(w).reshape(T, n_ch) != 0).any(axis=1) & mask.any(axis=1)).any()),
        "empty_mask_row": bool((~mask.any(axis=1)).any()),
        "asymmetric_mask": int((mask & ~mask.T).sum()),
        "rows_differ": T > 1 and len({tuple(r) for r in np.asarray(w).reshape(T, n_ch)}) > 1,
    }
