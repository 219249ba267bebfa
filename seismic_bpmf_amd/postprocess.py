"""Host-side steps right before / after the two hot paths (SURVEY.md section 8a rows
MF-4, MF-5, MF-6, BP-3, BP-4, BP-6), restated from the reference so that detection *indices*
come out identical.  Every function is pinned against golden vectors produced by the reference
itself (tests/golden/, tests/test_postprocess.py).

These are small integer / NumPy routines in the reference too (Python loops in
BPMF/similarity_search.py and BPMF/template_search.py); the heavy part of the post-CC step, the
RMS sliding threshold of BPMF/libc.c:516-673, has a device version in threshold.py.
"""
import functools

import numpy as np


# ----------------------------------------------------------------- time conversion ---
def sec_to_samp(t, sr, epsilon=0.2):
    """Seconds -> samples, BPMF/utils.py:1258-1271: truncate |t*sr| + epsilon, restore the sign."""
    t = np.asarray(t, dtype=np.float64)
    return np.int64(np.sign(t) * np.int64(np.abs(t * sr) + epsilon))


def moveouts_to_samples(travel_times_sec, sr, relative_to_first=True):
    """(K,S,P) travel times -> integer moveout table (BP-3).

    BPMF/template_search.py:145-168 (sec_to_samp) and :212-214 (minus the per-source minimum over
    stations and phases).  Returns (moveouts int32, moveout_to_tt int64 per source) -- the second is
    what find_detections adds back to the origin time (:635-639)."""
    tau = sec_to_samp(travel_times_sec, sr)
    first = np.zeros(tau.shape[0], dtype=np.int64)
    if relative_to_first:
        first = tau.reshape(tau.shape[0], -1).min(axis=1)
        tau = tau - first[:, None, None]
    return tau.astype(np.int32), first


# ------------------------------------------------------------------- input conditioning ---
def normalize_data(data_arr, return_norm=False):
    """MatchedFilter.set_data conditioning, BPMF/similarity_search.py:181-185: each channel is
    divided by its standard deviation (channels with zero std are left untouched).  With `return_norm`:
    (data / std, std.squeeze()) -- the second is the reference's `self.data_norm`, which turns the peak
    amplitudes of the normalised day back into those of the recorded one (:713)."""
    d = np.array(data_arr, dtype=np.float32, copy=True)
    std = d.std(axis=-1, keepdims=True)
    std[std == 0.0] = 1.0
    if return_norm:
        return d / std, std.squeeze()
    return d / std


def peak_amplitudes_host(data, rows, samples, moveouts, offset, duration, data_norm=None):
    """Host mirror of bpmf_peak_amplitudes_dev: the loop of MatchedFilter._find_detections_t
    (BPMF/similarity_search.py:695-714) over the detections (template row rows[q], DATA sample samples[q]), with the
    reference's own unguarded NumPy slice -- a window that straddles sample 0 is empty, one wholly before it wraps to
    the end of the day, one past the end is clipped.  data (S, C, N) float32, moveouts (T, S, C) in samples,
    `offset` / `duration` in samples, data_norm (S, C) or None (the maximum is then stored as it is).
    Returns (D, S, C) float32."""
    data = np.asarray(data, dtype=np.float32)
    S, C = data.shape[:2]
    rows = np.asarray(rows).reshape(-1)
    samples = np.asarray(samples).reshape(-1)
    moveouts = np.asarray(moveouts)
    moveouts = np.broadcast_to(moveouts.reshape(moveouts.shape[0], S, -1), (moveouts.shape[0], S, C))
    norm = None if data_norm is None else np.asarray(data_norm, dtype=np.float32).reshape(S, C)
    out = np.zeros((len(rows), S, C), dtype=np.float32)
    for q in range(len(rows)):
        mv = moveouts[int(rows[q])]
        for s in range(S):
            for c in range(C):
                time_idx1 = int(samples[q]) + int(mv[s, c]) - int(offset)
                time_idx2 = time_idx1 + int(duration)
                win_peak_amp = data[s, c, time_idx1:time_idx2]
                if len(win_peak_amp) > 0:
                    out[q, s, c] = win_peak_amp.max() if norm is None else win_peak_amp.max() * norm[s, c]
    return out


DAY_INDEX_LIMIT = 2**40          # N and |start|, |origin|, |offset| of the device entry points (csrc/day_rows.h)
TEMPLATE_MAX_SAMPLES = 8192      # np.std sums a longer row in buffers of 8192 samples: another summation tree


def _clipped_windows(data, start, length):
    """(E, S, C, length) float32: data[s, c, start[e, s, c] + l] where that sample exists, +0.0 elsewhere."""
    S, C, N = data.shape
    idx = start[..., None] + np.arange(length, dtype=np.int64)
    inside = (idx >= 0) & (idx < N)
    out = data[np.arange(S)[None, :, None, None], np.arange(C)[None, None, :, None], np.where(inside, idx, 0)]
    out[~inside] = 0.0
    return out


def template_window_moveouts(moveouts_sec, offset_phase_sec, phase_of_component, sr):
    """The (E, S, C) int32 moveouts of the template WINDOWS, Template.moveouts_win / moveouts_arr
    (BPMF/dataset.py:3451-3475): sec_to_samp(moveout - offset) of the phase each component is cut around.
    `moveouts_sec` (E, S, P) float64 seconds after the origin time, `offset_phase_sec` (P,) the time the window
    starts before the arrival (aux_data["offset_<phase>"]), `phase_of_component` (C,) the phase index of every
    component (aux_data["phase_on_comp<cp>"])."""
    mv = np.asarray(moveouts_sec, dtype=np.float64)
    win = mv - np.asarray(offset_phase_sec, dtype=np.float64)[None, None, :]
    return sec_to_samp(win[:, :, np.asarray(phase_of_component, dtype=np.int64)], sr).astype(np.int32)


def templates_from_events_host(data, origin_samples, moveouts, n_samples, normalize="rms", noise_offset=None,
                               noise_samples=None):
    """The DEFINITION of bpmf_templates_from_events_dev (csrc/templates.hip), in NumPy's own np.std / np.max / `/`:
    matched-filter templates cut from the day `data` (S, C, N) float32 at the located events.  For event e and channel
    (s, c), i0 = origin_samples[e] + moveouts[e, s, c] (`moveouts` (E, S[, C]) int32 WINDOW moveouts, any sign) and

    * waveforms[e, s, c, l] = data[s, c, i0 + l] where 0 <= i0 + l < N, else +0.0 -- Event.read_waveforms(
      time_shifted=True) + utils.get_np_array (BPMF/dataset.py:1929-2069, BPMF/utils.py:1653-1657), whose zero padding
      this is for a window cut by the END of the day.  DEPARTURE: a window cut by the START of the day keeps its
      alignment here (zeros in front); the reference left-aligns the samples it could read and pads behind them;
    * complete = the window lies wholly inside [0, N);  available = np.any(window != 0), Event.set_availability's test
      (:2592; a NaN counts as data);
    * norm = np.std(window) ("rms") | np.max(np.abs(window)) ("max") | 1 (None); 0 becomes 1; templates = waveforms /
      norm in float32 (TemplateGroup.normalize, :4160-4165);
    * snr (only with `noise_samples`) = np.std(window) / np.std(noise window) in float32, a noise std of 0 taken as 1,
      always on the un-normalised window (Event.compute_snr, :1457-1461).  The noise window is the `noise_samples`
      samples from origin_samples[e] - noise_offset, the same for every channel (time_shifted=False), clipped in place.
      DEPARTURE: the reference hands int(noise_window_sec * sr) to an argument read as seconds; here the length is in
      samples and says what it is.

    n_samples and noise_samples stop at 8192 (TEMPLATE_MAX_SAMPLES).  Returns a dict: waveforms, templates
    (E, S, C, L) float32; norm (E, S, C) float32; available, complete (E, S, C) bool; moveouts (E, S, C) int32; snr
    (E, S, C) float32 or None."""
    data = np.asarray(data, dtype=np.float32)
    if data.ndim != 3:
        raise ValueError("templates_from_events: data must be (S, C, N)")
    S, C, N = data.shape
    origin, mv, L, n_noise, offset = template_arguments(S, C, origin_samples, moveouts, n_samples, normalize,
                                                        noise_offset, noise_samples)
    E = len(origin)
    start = origin[:, None, None] + mv.astype(np.int64)
    waveforms = _clipped_windows(data, start, L)
    out = {"waveforms": waveforms, "moveouts": mv, "complete": (start >= 0) & (start + L <= N),
           "available": np.any(waveforms != 0.0, axis=-1), "snr": None}
    if normalize == "rms":
        norm = np.std(waveforms, axis=-1, keepdims=True)
    elif normalize == "max":
        norm = np.max(np.abs(waveforms), axis=-1, keepdims=True)
    else:
        norm = np.ones((E, S, C, 1), dtype=np.float32)
    norm[norm == 0.0] = 1.0
    out["templates"] = waveforms / norm
    out["norm"] = norm[..., 0]
    if n_noise:
        noise = _clipped_windows(data, np.broadcast_to((origin - offset)[:, None, None], (E, S, C)), n_noise)
        noise_std = np.std(noise, axis=-1)
        noise_std[noise_std == 0.0] = 1.0
        out["snr"] = np.std(waveforms, axis=-1) / noise_std
    return out


def template_arguments(S, C, origin_samples, moveouts, n_samples, normalize, noise_offset, noise_samples):
    """The arguments of templates_from_events (host definition and device call alike), checked and in their final
    types: (origin int64 (E,), moveouts int32 (E, S, C), L, noise_samples or 0, noise_offset).  Raises ValueError."""
    origin = np.asarray(origin_samples)
    mv = np.asarray(moveouts)
    if origin.ndim != 1 or (origin.size and origin.dtype.kind not in "iu"):
        raise ValueError("templates_from_events: origin_samples must be (E,) integers")
    origin = origin.astype(np.int64)
    E = len(origin)
    if mv.ndim not in (2, 3) or mv.shape[:2] != (E, S) or (mv.ndim == 3 and mv.shape[2] not in (1, C)):
        raise ValueError(f"templates_from_events: moveouts must be ({E}, {S}) or ({E}, {S}, {C}); got {mv.shape}")
    if mv.size and mv.dtype.kind not in "iu":
        raise ValueError("templates_from_events: moveouts must be integers (samples)")
    if mv.size and (mv.min() < -2**31 or mv.max() >= 2**31):
        raise ValueError("templates_from_events: moveouts must fit int32")
    mv = np.array(np.broadcast_to(mv.reshape(E, S, 1 if mv.ndim == 2 else mv.shape[2]), (E, S, C)), dtype=np.int32,
                  order="C")
    if normalize not in ("rms", "max", None):
        raise ValueError("templates_from_events: normalize must be 'rms', 'max' or None")
    L = int(n_samples)
    if not 1 <= L <= TEMPLATE_MAX_SAMPLES:
        raise ValueError(f"templates_from_events: n_samples must be 1 .. {TEMPLATE_MAX_SAMPLES}; got {L}")
    n_noise = 0 if noise_samples is None else int(noise_samples)
    if not 0 <= n_noise <= TEMPLATE_MAX_SAMPLES:
        raise ValueError(f"templates_from_events: noise_samples must be 0 .. {TEMPLATE_MAX_SAMPLES}; got {n_noise}")
    if n_noise and noise_offset is None:
        raise ValueError("templates_from_events: noise_samples needs noise_offset (samples before the origin)")
    offset = 0 if noise_offset is None else int(noise_offset)
    if np.any(np.abs(origin) > DAY_INDEX_LIMIT) or abs(offset) > DAY_INDEX_LIMIT:
        raise ValueError("templates_from_events: origin_samples and noise_offset must lie within +-2^40")
    return origin, mv, L, n_noise, offset


# ---- the deep-learning picker's surroundings: utils.normalize_batch, find_picks, get_picks (BPMF/utils.py:1966-2200) ----

PICKER_MAX_WINDOW = 8192                     # one NumPy sum is one pairwise tree up to here (csrc/np_sums.h)
PICK_COLUMNS = ("P_probas", "P_picks", "P_unc", "S_probas", "S_picks", "S_unc")


def normalize_batch_plan(n_samples, normalization_window_sample=3000, overlap=0.5):
    """(shift, n_windows) of utils.normalize_batch for rows of `n_samples`: shift = int((1 - overlap) * W), windows
    at the multiples of shift in the row reflect-padded by shift, a trailing partial window dropped.  ValueError for
    what the reference cannot do (fewer than 2 windows: its IndexError; shift > n - 1: np.pad reflects more than once)
    or what the device does not do (W > 8192)."""
    n, W = int(n_samples), int(normalization_window_sample)
    if W < 2:
        raise ValueError(f"normalize_batch: normalization_window_sample must be at least 2; got {W}")
    if W > PICKER_MAX_WINDOW:
        raise ValueError(f"normalize_batch: normalization_window_sample must be at most {PICKER_MAX_WINDOW}; got {W}")
    shift = int((1.0 - overlap) * W)
    if shift < 1:
        raise ValueError(f"normalize_batch: overlap {overlap} leaves a shift of {shift} samples; need at least 1")
    if shift > n - 1:
        raise ValueError(f"normalize_batch: the shift ({shift}) must be at most n_samples - 1 ({n - 1}): the reflect "
                         "padding would fold more than once")
    n_windows = (n + 2 * shift - W) // shift + 1 if n + 2 * shift >= W else 0
    if n_windows < 2:
        raise ValueError(f"normalize_batch: {n} samples hold {n_windows} window(s) of {W}; need at least 2")
    return shift, n_windows


def normalize_batch_nodes(n_samples, shift, n_windows):
    """The abscissae the reference interpolates the window statistics from (BPMF/utils.py:2005) -- not the centres of
    the windows."""
    return np.linspace(shift, n_samples - shift, n_windows)


def _normalize_batch_replace_edges(std, mean):
    """BPMF/utils.py:2007-2014: the last window takes the statistics of the last but one, then the first those of the
    second."""
    std[..., -1], mean[..., -1] = std[..., -2], mean[..., -2]
    std[..., 0], mean[..., 0] = std[..., 1], mean[..., 1]


def normalize_batch_host(seismogram, normalization_window_sample=3000, overlap=0.5):
    """The DEFINITION of bpmf_normalize_batch_dev (csrc/picker.hip): utils.normalize_batch (BPMF/utils.py:1966-2036),
    the running Z-score in front of the deep-learning picker, bit for bit and without SciPy.  `seismogram`
    (R, C, n) float32; returns float64 (R, C, n).  Per row: reflect-pad by shift = int((1 - overlap) * W); np.std and
    np.mean (float32) of the windows at the multiples of shift; the edge windows take their neighbours' statistics;
    std == 0 becomes 1; both are interpolated to every sample with np.interp (float64) from the nodes
    np.linspace(shift, n - shift, n_windows); out = (x - mean) / std in float64.  Refusals: normalize_batch_plan."""
    x = np.asarray(seismogram, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError("normalize_batch: seismogram must be (R, C, n)")
    R, C, n = x.shape
    W = int(normalization_window_sample)
    shift, n_windows = normalize_batch_plan(n, W, overlap)
    padded = np.pad(x, ((0, 0), (0, 0), (shift, shift)), mode="reflect")
    windows = np.ascontiguousarray(
        np.lib.stride_tricks.sliding_window_view(padded, W, axis=-1)[:, :, ::shift, :])
    assert windows.shape[2] == n_windows
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        std = np.std(windows, axis=-1)
        mean = np.mean(windows, axis=-1)
        _normalize_batch_replace_edges(std, mean)
        std[std == 0] = 1
        nodes = normalize_batch_nodes(n, shift, n_windows)
        t = np.arange(n)
        std_t = np.stack([np.interp(t, nodes, row, left=row[0], right=row[-1])
                          for row in std.reshape(-1, n_windows)]).reshape(R, C, n)
        mean_t = np.stack([np.interp(t, nodes, row, left=row[0], right=row[-1])
                           for row in mean.reshape(-1, n_windows)]).reshape(R, C, n)
        return (x - mean_t) / std_t


def picker_windows_host(data, starts, n_samples):
    """(E, S, C, n_samples) float32: the windows data[s, c, starts[e(, s)] + i] of the (S, C, N) day, +0.0 outside it
    -- what picker_batch normalises without ever storing it."""
    data = np.asarray(data, dtype=np.float32)
    S, C, N = data.shape
    starts = picker_starts(starts, S)
    return _clipped_windows(data, np.broadcast_to(starts[:, :, None], starts.shape + (C,)), int(n_samples))


def picker_starts(starts, S):
    """`starts` (E,) or (E, S) integers as (E, S) int64, within +-2^40.  Raises ValueError."""
    st = np.asarray(starts)
    if st.ndim not in (1, 2) or (st.ndim == 2 and st.shape[1] != S) or (st.size and st.dtype.kind not in "iu"):
        raise ValueError(f"picker_batch: starts must be (E,) or (E, {S}) integers (samples); got {st.dtype} {st.shape}")
    st = st.astype(np.int64)
    if np.any(np.abs(st) > DAY_INDEX_LIMIT):
        raise ValueError("picker_batch: starts must lie within +-2^40")
    return np.array(np.broadcast_to(st[:, None] if st.ndim == 1 else st, (len(st), S)), dtype=np.int64, order="C")


RESAMPLE_MAX_RATE = 64                       # max(up, down) after the reduction by their gcd
RESAMPLE_INDEX_LIMIT = DAY_INDEX_LIMIT        # n_in * max(up, down) stays below it


def resample_poly_factors(up, down):
    """`up` and `down` of scipy.signal.resample_poly as Python ints divided by their gcd.  ValueError for factors that
    are no integers or under 1, or a reduced max(up, down) over 64."""
    factors = []
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            if not isinstance(v, (float, np.floating)) or v != int(v):
                raise ValueError(f"resample_poly: {name} must be an integer; got {v!r}")
        if int(v) < 1:
            raise ValueError(f"resample_poly: {name} must be at least 1; got {v!r}")
        factors.append(int(v))
    g = int(np.gcd(factors[0], factors[1]))
    up, down = factors[0] // g, factors[1] // g
    if max(up, down) > RESAMPLE_MAX_RATE:
        raise ValueError(f"resample_poly: the reduced factors {up} / {down} exceed {RESAMPLE_MAX_RATE}")
    return up, down


def resample_poly_plan(n_in, up, down):
    """What scipy.signal.resample_poly(x, up, down) (default window and padtype) does to a row of `n_in` float32
    samples, restated without SciPy: (h, n_out, n_pre_pad, n_pre_remove, n_post_pad, table) for `up` and `down`
    reduced by their gcd.  With r = max(up, down) and half = 10 r: `h` (2 half + 1,) float32 =
    firwin(2 half + 1, 1 / r, window=("kaiser", 5.0)).astype(float32) * float32(up); `n_out` = ceil(n_in up / down);
    upfirdn runs the filter with `n_pre_pad` zeros in front and `n_post_pad` behind and the first `n_pre_remove` of its
    outputs are dropped; `table` (hp up,) float32 is that padded filter, zero-extended to hp = ceil(len / up) taps per
    phase: output q reads table[t + k up], k = 0 .. hp - 1, for its phase t.  The float32 taps equal SciPy's bit for
    bit for every r from 2 to 64 (the float64 ones do not: np.i0 and SciPy's i0 differ in the last bits).
    Refusals (ValueError): resample_poly_factors; n_in < 1; n_in max(up, down) >= 2^40."""
    up, down = resample_poly_factors(up, down)
    n_in = int(n_in)
    if n_in < 1:
        raise ValueError(f"resample_poly: rows of at least 1 sample; got {n_in}")
    r = max(up, down)
    if n_in * r >= RESAMPLE_INDEX_LIMIT:
        raise ValueError(f"resample_poly: n_in * max(up, down) = {n_in * r} must stay below 2^40")
    half = 10 * r
    m = (np.arange(2 * half + 1) - half).astype(np.float64)
    cutoff = 1.0 / r                         # firwin forms cutoff * m, not m / r: the two differ in the last bit
    h64 = cutoff * np.sinc(cutoff * m) * (np.i0(5.0 * np.sqrt(1.0 - (m / half) ** 2)) / np.i0(5.0))
    h64 = h64 / h64.sum()
    h = h64.astype(np.float32) * np.float32(up)
    n_out = n_in * up // down + bool(n_in * up % down)
    n_pre_pad = down - half % down
    n_pre_remove = (half + n_pre_pad) // down
    n_post_pad = 0
    while ((n_in - 1) * up + len(h) + n_pre_pad + n_post_pad - 1) // down + 1 < n_out + n_pre_remove:
        n_post_pad += 1
    length = len(h) + n_pre_pad + n_post_pad
    hp = -(-length // up)
    table = np.zeros(hp * up, dtype=np.float32)
    table[n_pre_pad:n_pre_pad + len(h)] = h
    return h, n_out, n_pre_pad, n_pre_remove, n_post_pad, table


def resample_poly_host(x, up, down):
    """The DEFINITION of bpmf_resample_poly_dev (csrc/resample.hip): scipy.signal.resample_poly(x, up, down, axis=-1)
    of float32 rows, bit for bit and without SciPy -- the up- and down-sampling between the cut windows and the picker
    in Event.pick_PS_phases (BPMF/dataset.py:1801-1804, 5596-5599).  `x` (..., n_in) float32; returns (..., n_out)
    float32.  With the plan of resample_poly_plan, output q has m = q + n_pre_remove, j_hi = m down // up,
    t = m down % up and is the float32 chain
        acc = +0;   for k = hp - 1 .. 0:   j = j_hi - k;   acc = fl(acc + fl(x[j] * table[t + k up]))   where 0 <= j < n_in
    -- input index ascending, one rounded multiply and one rounded add per tap, never fused, samples outside the row
    skipped.  The zero taps of the padding do multiply: a NaN sample spreads as far as SciPy spreads it.  up == down
    after the reduction returns a copy.  Refusals: resample_poly_plan."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"resample_poly: x must be float32; got {x.dtype}")
    if x.ndim < 1:
        raise ValueError("resample_poly: x must be (..., n)")
    up, down = resample_poly_factors(up, down)
    n_in = x.shape[-1]
    _, n_out, _, n_pre_remove, _, table = resample_poly_plan(n_in, up, down)
    if up == down:
        return x.copy()
    hp = len(table) // up
    m = np.arange(n_out, dtype=np.int64) + n_pre_remove
    j_hi, t = m * down // up, m * down % up
    acc = np.zeros(x.shape[:-1] + (n_out,), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(hp - 1, -1, -1):
            j = j_hi - k
            q = np.flatnonzero((j >= 0) & (j < n_in))
            if len(q):
                acc[..., q] = acc[..., q] + x[..., j[q]] * table[t[q] + k * up]
    return acc


def _plateau_midpoint(left, right):
    return (left + right) // 2


def _reaches(value, threshold):
    """find_peaks(height=threshold) keeps value >= threshold."""
    return value >= threshold


def _pick_moments(samples, prob):
    """BPMF/utils.py:2083-2084 as written: np.sum(samples * prob) in float64, prob.sum() in float32, and a spread that
    the probabilities do not weight."""
    mean = np.sum(samples * prob) / prob.sum()
    std = np.sqrt(np.sum((samples - mean) ** 2) / prob.sum())
    return mean, std


def find_peaks_host(phase_probability, threshold):
    """scipy.signal.find_peaks(x, height=threshold, prominence=0.9 * threshold, width=1) restated without SciPy:
    (peaks, left_ips, right_ips).  Local maxima are the midpoints of plateaus that a rise opens and a fall closes (one
    touching either end of the series is none); height: x[peak] >= threshold; prominence over the whole series
    (wlen=None): x[peak] - max(lowest value on either side before a higher sample); width at half prominence between
    linearly interpolated crossings, kept when >= 1.  The series is compared as float64, as SciPy casts it."""
    x = np.ascontiguousarray(phase_probability, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("find_picks: phase_probability must be one series")
    n = len(x)
    min_prominence = 0.9 * threshold
    peaks, left_ips, right_ips = [], [], []
    i = 1
    while i < n - 1:
        if x[i - 1] < x[i]:
            ahead = i + 1
            while ahead < n - 1 and x[ahead] == x[i]:
                ahead += 1
            if x[ahead] < x[i]:
                pk = _plateau_midpoint(i, ahead - 1)
                if _reaches(x[pk], threshold):
                    # prominence: walk out while the samples are not higher than the peak, keep the lowest
                    j, left_min, left_base = pk, x[pk], pk
                    while j >= 0 and x[j] <= x[pk]:
                        if x[j] < left_min:
                            left_min, left_base = x[j], j
                        j -= 1
                    j, right_min, right_base = pk, x[pk], pk
                    while j <= n - 1 and x[j] <= x[pk]:
                        if x[j] < right_min:
                            right_min, right_base = x[j], j
                        j += 1
                    prominence = x[pk] - max(left_min, right_min)
                    if min_prominence <= prominence:
                        height = x[pk] - prominence * 0.5
                        j = pk
                        while left_base < j and height < x[j]:
                            j -= 1
                        left_ip = float(j)
                        if x[j] < height:
                            left_ip += (height - x[j]) / (x[j + 1] - x[j])
                        j = pk
                        while j < right_base and height < x[j]:
                            j += 1
                        right_ip = float(j)
                        if x[j] < height:
                            right_ip -= (height - x[j]) / (x[j - 1] - x[j])
                        if 1 <= right_ip - left_ip:
                            peaks.append(pk)
                            left_ips.append(left_ip)
                            right_ips.append(right_ip)
                i = ahead
        i += 1
    return np.array(peaks, dtype=np.int64), np.array(left_ips, dtype=np.float64), np.array(right_ips, dtype=np.float64)


def find_picks_host(phase_probability, threshold, return_index=False):
    """The DEFINITION of bpmf_find_picks_dev (csrc/picker.hip): utils.find_picks (BPMF/utils.py:2039-2094) with its
    default keywords, bit for bit and without SciPy.  Returns (values float32, means float64, stds float64) [and the
    peak indices int64]: per peak of find_peaks_host, over the samples int(left_ip) .. int(right_ip), the moments
    of _pick_moments on the float32 series.  Other find_peaks keywords are out of scope."""
    prob_series = np.ascontiguousarray(phase_probability, dtype=np.float32)
    peaks, left_ips, right_ips = find_peaks_host(prob_series, threshold)
    means, stds = np.zeros(len(peaks), dtype=np.float64), np.zeros(len(peaks), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(len(peaks)):
            samples = np.arange(int(left_ips[k]), int(right_ips[k]) + 1)
            means[k], stds[k] = _pick_moments(samples, prob_series[samples])
    values = prob_series[peaks]
    return (values, means, stds, peaks) if return_index else (values, means, stds)


def _best_pick(probas, picks, prior, search_win_samp):
    if prior is None:
        return int(np.argmax(probas))
    return int(np.argmax(probas * np.exp(-((picks - prior) ** 2) / (2.0 * search_win_samp**2))))


def get_picks_host(values, means, stds, counts, buffer_length, prior=None, search_win_samp=None):
    """utils.get_picks (BPMF/utils.py:2097-2200) on arrays instead of a pandas table: one P and one S pick per
    station.  `values` (S, 2, max_picks) float32, `means`, `stds` (S, 2, max_picks) float64 and `counts` (S, 2): the
    picks of find_picks, phase 0 = P, phase 1 = S.  Picks > int(buffer_length) only; the best S first (argmax of the
    probability, or of probability * exp(-(pick - prior)^2 / (2 win^2)) where `prior` (S, 2), in samples, is not NaN
    for the station: a station has both priors or none); then the P picks strictly before that S; a station without
    an S keeps its best P.  `buffer_length` is explicit: the reference binds int(2 * cfg.SAMPLING_RATE_HZ) when it is
    imported.  Returns (S, 6) float32 in the order of PICK_COLUMNS, NaN where there is no pick."""
    values, means, stds = np.asarray(values, np.float32), np.asarray(means, np.float64), np.asarray(stds, np.float64)
    counts = np.asarray(counts)
    if values.ndim != 3 or values.shape[1] != 2 or means.shape != values.shape or stds.shape != values.shape or \
            counts.shape != values.shape[:2]:
        raise ValueError("get_picks: values, means, stds must be (S, 2, max_picks) and counts (S, 2)")
    if counts.size and (counts.min() < 0 or counts.max() > values.shape[2]):
        raise ValueError("get_picks: counts must lie in 0 .. max_picks (picks were dropped: raise max_picks)")
    S = values.shape[0]
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float64)
        if prior.shape != (S, 2) or np.any(np.isnan(prior[:, 0]) != np.isnan(prior[:, 1])):
            raise ValueError(f"get_picks: prior must be ({S}, 2), a row being all NaN (no prior) or not at all")
        if search_win_samp is None:
            raise ValueError("get_picks: prior needs search_win_samp (the width of the Gaussian, in samples)")
    out = np.full((S, 6), np.nan, dtype=np.float32)
    for s in range(S):
        station_prior = None if prior is None or np.isnan(prior[s, 0]) else prior[s]
        cols = []
        for ph in range(2):
            k = int(counts[s, ph])
            valid = means[s, ph, :k] > int(buffer_length)
            cols.append([values[s, ph, :k][valid], means[s, ph, :k][valid], stds[s, ph, :k][valid]])
        (p_probas, p_picks, p_unc), (s_probas, s_picks, s_unc) = cols
        if len(s_picks):
            best = _best_pick(s_probas, s_picks, None if station_prior is None else station_prior[1], search_win_samp)
            out[s, 3:] = s_probas[best], s_picks[best], s_unc[best]
            before = p_picks < s_picks[best]
            p_probas, p_picks, p_unc = p_probas[before], p_picks[before], p_unc[before]
        if len(p_picks):
            best = _best_pick(p_probas, p_picks, None if station_prior is None else station_prior[0], search_win_samp)
            out[s, :3] = p_probas[best], p_picks[best], p_unc[best]
    return out


def normalize_weights(weights):
    """Sum of channel weights = 1 per template, BPMF/similarity_search.py:469-472."""
    w = np.array(weights, dtype=np.float32, copy=True)
    norm = w.sum(axis=(1, 2), keepdims=True)
    norm[norm == 0.0] = 1.0
    return w / norm


def normalize_templates(waveforms, method="rms"):
    """TemplateGroup.normalize, BPMF/dataset.py:4152-4166: every (template, station, channel)
    window divided by its standard deviation ("rms") or its peak amplitude ("max"); all-zero
    windows stay zero."""
    w = np.array(waveforms, dtype=np.float32, copy=True)
    if method == "rms":
        norm = np.std(w, axis=-1, keepdims=True)
    elif method == "max":
        norm = np.max(np.abs(w), axis=-1, keepdims=True)
    else:
        raise ValueError("method must be 'rms' or 'max'")
    norm[norm == 0.0] = 1.0
    w /= norm
    return w


def network_to_template_map(waveforms, selected_stations=None):
    """TemplateGroup.set_network_to_template_map, BPMF/dataset.py:4977-5008: channel (t, s, c) is
    used when (1) its samples do not sum to 0 (:5001) AND (2) station s is one of the stations
    selected on template t (`tp.stations`, :5003-5007 -- what n_closest_stations /
    n_best_SNR_stations leave on a template).

    `selected_stations`: a (T, S) boolean array, or one sequence of network station indexes per
    template (the reference's `network.station_indexes.loc[tp.stations]`); None = every station of
    every template is selected (templates that carry the whole network)."""
    present = ~(np.sum(np.asarray(waveforms), axis=-1) == 0.0)
    if selected_stations is None:
        return present
    T, S = present.shape[:2]
    if isinstance(selected_stations, np.ndarray) and selected_stations.dtype == bool:
        sel = selected_stations
        if sel.shape != (T, S):
            raise ValueError(f"selected_stations must have shape {(T, S)}, got {sel.shape}")
    else:
        if len(selected_stations) != T:
            raise ValueError("selected_stations needs one entry per template")
        sel = np.zeros((T, S), dtype=bool)
        for t, idx in enumerate(selected_stations):
            sel[t, np.asarray(idx, dtype=np.int64)] = True
    return present & sel[:, :, None]


def station_density_weights(interstation_distances, cutoff_dist=None, lower_percentile=0.0,
                            upper_percentile=100.0):
    """Per-station weights that balance station density (BPMF/template_search.py:898-949, same
    text at similarity_search.py:371-421): w_s = 1 / sum_j exp(-D_sj^2 / cutoff^2), cutoff = median
    non-zero inter-station distance unless given, optionally clipped to percentiles.  Float64 sums
    stored as float32, like the reference."""
    D = np.asarray(interstation_distances, dtype=np.float64)
    if cutoff_dist is None:
        cutoff_dist = np.median(D[D != 0.0])
    w = np.zeros(D.shape[0], dtype=np.float32)
    for s in range(D.shape[0]):
        w[s] = 1.0 / np.sum(np.exp(-(D[s] ** 2) / cutoff_dist ** 2))
    if lower_percentile > 0.0:
        w = np.clip(w, np.percentile(w, lower_percentile), w.max())
    if upper_percentile < 100.0:
        w = np.clip(w, w.min(), np.percentile(w, upper_percentile))
    return w


def _kth_smallest(mv, k):
    """Largest of the k smallest values of every row (the reference's np.partition cut-off)."""
    return np.partition(mv, k - 1, axis=1)[:, :k].max(axis=1, keepdims=True)


def weights_sources_closest(moveouts, n_closest, online=None):
    """Source weights of BP-4, BPMF/template_search.py:779-798: 1 for the stations whose
    first-phase moveout is not larger than the `n_closest`-th smallest one *among the operational
    stations* of each source (ties at the cut-off included), 0 for offline stations.  With
    `n_closest` 0 or >= the number of stations every operational station keeps weight 1."""
    first = np.asarray(moveouts)[:, :, 0]
    K, S = first.shape
    online = np.ones(S, dtype=bool) if online is None else np.asarray(online, dtype=bool)
    w = np.ones((K, S), dtype=np.float32)
    n = min(int(online.sum()), int(n_closest))
    if 0 < n < S:
        w[first > _kth_smallest(first[:, online], n)] = 0.0
    w[:, ~online] = 0.0
    return w


def weights_sources_max_moveout(moveouts, max_moveout, online=None):
    """BPMF/template_search.py:800-814: 1 where the earliest phase of a station arrives less than
    `max_moveout` samples after the source's first arrival, 0 for offline stations."""
    earliest = np.min(np.asarray(moveouts), axis=-1)
    w = np.zeros(earliest.shape, dtype=np.float32)
    w[earliest < max_moveout] = 1.0
    if online is not None:
        w[:, ~np.asarray(online, dtype=bool)] = 0.0
    return w


def set_weights_sources(moveouts, method="closest_stations", n_min_stations=0, normalize=False,
                        online=None, density_weights=None, **kwargs):
    """Beamformer.set_weights_sources (BP-4), BPMF/template_search.py:816-895.

    `online` replaces `data.availability_per_sta`; `density_weights` (S,) replaces the
    `weight_station_density=True` branch (build it with station_density_weights)."""
    if method == "closest_stations":
        if kwargs.get("num_closest_stations") is None:
            raise TypeError("method 'closest_stations' needs num_closest_stations")
        w = weights_sources_closest(moveouts, kwargs["num_closest_stations"], online)
    elif method == "max_moveout":
        if kwargs.get("max_moveout") is None:
            raise TypeError("method 'max_moveout' needs max_moveout")
        w = weights_sources_max_moveout(moveouts, kwargs["max_moveout"], online)
    else:
        raise ValueError("method must be 'closest_stations' or 'max_moveout'")
    if n_min_stations > 0:
        w[np.sum(w > 0.0, axis=-1) < n_min_stations, :] = 0.0
    if density_weights is not None:
        w *= np.asarray(density_weights)[None, :]
    if normalize:
        norm = np.sum(w, axis=1, keepdims=True)
        norm[norm == 0.0] = 1.0
        w /= norm
    return w


def weights_channels_simple(present, min_channels=6, min_stations=3):
    """MatchedFilter._weights_channels_simple, BPMF/similarity_search.py:288-296: weight 1 on
    every present template channel; templates with fewer than `min_channels` channels or
    `min_stations` stations get all-zero weights."""
    w = np.float32(present)
    too_few = (np.sum(w != 0.0, axis=(1, 2)) < min_channels) | \
              (np.sum(np.sum(w, axis=2) > 0.0, axis=1) < min_stations)
    w[too_few] = 0.0
    return w


def _operational(availability, data_channels_ok):
    ok = np.asarray(availability, dtype=bool)
    if data_channels_ok is not None:
        ok = np.logical_and(ok, np.asarray(data_channels_ok, dtype=bool)[None, :, :])
    return ok


def weights_channels_closest(moveouts, availability, num_closest_stations, data_channels_ok=None):
    """MatchedFilter._weights_channels_closest, BPMF/similarity_search.py:298-332.  Stations
    without any operational channel are pushed to the end of the ranking; the cut-off is the
    `num_closest_stations`-th smallest first-phase moveout; offline channels get 0."""
    mv_all = np.asarray(moveouts)
    T, S = mv_all.shape[:2]
    ok = _operational(availability, data_channels_ok)
    w = np.ones(ok.shape, dtype=np.float32)
    first = np.array(mv_all[..., 0], copy=True)
    first[~np.any(ok, axis=-1)] = np.iinfo(np.int32).max
    n = min(S, int(num_closest_stations))
    if 0 < n < S:
        w[mv_all[:, :, 0] > _kth_smallest(first, n), :] = 0.0
    w[~ok] = 0.0
    return w


def weights_channels_max_moveout(moveouts, availability, max_moveout_sec, sr, n_min_stations=0,
                                 max_moveout2_sec=None, data_channels_ok=None):
    """MatchedFilter._weights_channels_max_moveout, BPMF/similarity_search.py:334-367 (including
    its fall-back: when fewer than `n_min_stations` (template, station) pairs qualify in total,
    the second radius is applied without the availability mask)."""
    ok = _operational(availability, data_channels_ok)
    w = np.zeros(ok.shape, dtype=np.float32)
    earliest = np.min(np.asarray(moveouts), axis=-1)
    valid = (earliest < int(max_moveout_sec * sr)) & np.any(ok, axis=-1)
    if np.sum(valid) < n_min_stations and max_moveout2_sec is not None:
        valid = earliest < int(max_moveout2_sec * sr)
    w[valid, :] = 1.0
    w[~ok] = 0.0
    return w


def set_weights_channels(method="simple", n_min_stations=0, normalize=True, density_weights=None,
                         *, present=None, moveouts=None, availability=None, sr=None,
                         min_channels=6, min_stations=3, data_channels_ok=None, **kwargs):
    """MatchedFilter.set_weights_channels (MF-6), BPMF/similarity_search.py:423-474.  The
    template-group attributes the reference reads are passed explicitly: `present` =
    network_to_template_map, `moveouts` = moveouts_arr (T,S,P), `availability` =
    availability_arr (T,S,C), `sr` = template sampling rate."""
    if method == "simple":
        w = weights_channels_simple(present, min_channels, min_stations)
    elif method == "closest_stations":
        if kwargs.get("num_closest_stations") is None:
            raise TypeError("method 'closest_stations' needs num_closest_stations")
        w = weights_channels_closest(moveouts, availability, kwargs["num_closest_stations"],
                                     data_channels_ok)
    elif method == "max_moveout":
        if kwargs.get("max_moveout_sec") is None:
            raise TypeError("method 'max_moveout' needs max_moveout_sec")
        w = weights_channels_max_moveout(moveouts, availability, kwargs["max_moveout_sec"], sr,
                                         n_min_stations, kwargs.get("max_moveout2_sec"),
                                         data_channels_ok)
    else:
        raise ValueError("method must be 'simple', 'closest_stations' or 'max_moveout'")
    if n_min_stations > 0:
        w[np.sum(np.any(w > 0.0, axis=-1), axis=1) < n_min_stations, :] = 0.0
    if density_weights is not None:
        w *= np.asarray(density_weights)[None, :, None]
    if normalize:
        norm = np.sum(w, axis=(1, 2), keepdims=True)
        norm[norm == 0.0] = 1.0
        w /= norm
    return w


# ------------------------------------------------------------------------ peak picking ---
def detect_peaks(x, mpd=1):
    """Indices of local maxima of `x` at least `mpd` samples apart (tallest first wins).

    Restates the path of BPMF/utils.py:2203-2354 that BPMF uses (edge="rising", no height or
    prominence threshold, kpsh=False): a peak is a sample strictly above its left neighbour and
    not below its right one; the first and last sample never qualify; peaks are then visited in
    decreasing height and every other peak within +-mpd of a kept one is dropped.
    """
    x = np.atleast_1d(np.asarray(x)).astype(np.float64)
    if x.size < 3:
        return np.array([], dtype=int)
    dx = np.diff(x)
    nan = np.flatnonzero(np.isnan(x))
    if nan.size:
        x = x.copy()
        x[nan] = np.inf
        dx[np.isnan(dx)] = np.inf
    rising = np.flatnonzero((np.append(dx, 0.0) <= 0) & (np.insert(dx, 0, 0.0) > 0))
    ind = np.unique(rising)
    if ind.size and nan.size:
        bad = np.unique(np.concatenate((nan, nan - 1, nan + 1)))
        ind = ind[~np.isin(ind, bad)]
    if ind.size and ind[0] == 0:
        ind = ind[1:]
    if ind.size and ind[-1] == x.size - 1:
        ind = ind[:-1]
    if ind.size and mpd > 1:
        rank = _tallest_first(x[ind])
        ind = ind[_suppress(ind, rank, mpd)]
    return ind


def _tallest_first(height):
    """Visiting order of the suppression, the reference's own expression
    `np.argsort(x[ind])[::-1]` (BPMF/utils.py:2335).  NumPy's default sort is not stable (for
    float64 a SIMD sort): the order of EXACTLY equal heights depends on the whole array, so it
    can only be reproduced by sorting the same full list of local maxima -- which is what
    detect_peaks does, and what the device path falls back to when two equal peaks closer than mpd
    exist among its candidates (has_close_ties)."""
    return np.argsort(np.asarray(height))[::-1]


def has_close_ties(index, height, mpd):
    """True if two peaks of exactly equal height lie within mpd samples of each other -- the only
    case in which the visiting order of equal heights changes which peaks survive."""
    index = np.asarray(index, dtype=np.int64)
    height = np.asarray(height)
    if index.size < 2:
        return False
    order = np.lexsort((index, height))
    h, i = height[order], index[order]
    return bool(np.any((h[1:] == h[:-1]) & (i[1:] - i[:-1] <= mpd)))


def _suppress(ind, rank, mpd):
    """Mask of the peaks `ind` (ascending) that survive the tallest-first +-mpd suppression of
    BPMF/utils.py:2334-2345, visited in the order `rank` (indices into `ind`).  The reference's
    loop is O(peaks^2) in NumPy -- hours for a day of beam; the library's host routine walks the
    neighbours of each kept peak instead (same order, same result)."""
    ind = np.ascontiguousarray(ind, dtype=np.int64)
    rank = np.ascontiguousarray(rank, dtype=np.int64)
    from . import _lib
    lib = _lib.lib()                              # raises if the library has not been built
    keep = np.empty(ind.size, dtype=np.uint8)
    import ctypes as C
    rc = lib.bpmf_suppress_peaks(ind.ctypes.data_as(C.POINTER(C.c_int64)),
                                 rank.ctypes.data_as(C.POINTER(C.c_int64)), ind.size, float(mpd),
                                 keep.ctypes.data_as(C.POINTER(C.c_uint8)))
    _lib.check(rc, "bpmf_suppress_peaks")
    return keep.astype(bool)


def snap_and_merge_peaks(peaks, n, mpd, beam_slice):
    """The regrouping lines of Beamformer.find_detections, BPMF/template_search.py:612-624: every
    peak, in order, is moved to the largest sample within +-mpd/2 of its CURRENT position (first
    occurrence on ties, np.argmax), together with every other peak that currently sits on the same
    sample; duplicates are merged.  `beam_slice(i0, i1)` returns maxbeam[i0:i1] -- the only access
    to the series, so the same code runs on a host array and on windows fetched from the device."""
    peaks = np.array(peaks, copy=True)
    for q in range(peaks.size):
        lo = max(0, peaks[q] - mpd / 2)
        hi = min(peaks[q] + mpd / 2, n)
        win = np.arange(lo, hi).astype(np.int32)   # same float->int truncation as the reference
        seg = np.asarray(beam_slice(int(win[0]), int(win[-1]) + 1))
        snapped = np.argmax(seg[win - win[0]]) + win[0]
        peaks[peaks == peaks[q]] = snapped
    return np.unique(peaks)


def find_beam_detections(maxbeam, maxbeam_sources, threshold, mpd):
    """Peak logic of Beamformer.find_detections (BP-6), BPMF/template_search.py:604-627.

    Peaks of `maxbeam` at least `mpd` samples apart and above `threshold`, each snapped to the
    largest sample within +-mpd/2, duplicates merged.  Returns (peak sample indices, their source
    indices) -- the "detection sample indices" that must match the reference exactly."""
    maxbeam = np.asarray(maxbeam)
    n = maxbeam.size
    threshold = np.broadcast_to(np.asarray(threshold), (n,))
    peaks = detect_peaks(maxbeam, mpd=mpd)
    peaks = peaks[maxbeam[peaks] > threshold[peaks]]
    peaks = snap_and_merge_peaks(peaks, n, mpd, lambda i0, i1: maxbeam[i0:i1])
    return peaks, np.asarray(maxbeam_sources)[peaks]


def find_beam_detections_from_candidates(index, height, threshold_at, mpd, n, beam_slice):
    """find_beam_detections for a series that is not on the host: `index` (ascending) / `height`
    list every rising-edge local maximum above a floor that no threshold value undercuts (the
    device extraction, csrc/bp_detect.hip); `threshold_at(samples)` evaluates the threshold at a few
    samples.  The tallest-first suppression of BPMF/utils.py:2334-2345 runs on this list: the peaks
    it lacks are lower than every peak above the threshold, so they can neither remove one of those
    nor tie with one, and the survivors above the threshold are the reference's.  Exactly equal
    heights closer than mpd are the one exception (has_close_ties): the caller then passes the list
    of ALL local maxima, on which the order is the reference's (_tallest_first)."""
    index = np.asarray(index, dtype=np.int64)
    height = np.asarray(height).astype(np.float64)
    if index.size and mpd > 1:
        rank = _tallest_first(height)
        keep = _suppress(index, rank, mpd)
        index, height = index[keep], height[keep]
    above = height > np.asarray(threshold_at(index), dtype=np.float64)
    return snap_and_merge_peaks(index[above], n, mpd, beam_slice)


def bp_threshold_nodes(n, window, overlap, median, mad, n_dev):
    """Window centres and node values of template_search.time_dependent_threshold
    (BPMF/template_search.py:1452-1487) from the per-window medians / MADs: `median`, `mad` are
    float32 arrays of n_windows + 2 entries whose entries 1 .. n_windows are filled; the end fills
    are applied here.  Returns (centre float32, threshold float32), both n_windows + 2 long; the
    threshold at sample t is interp_threshold(t, centre, threshold), the end values outside."""
    shift = int((1.0 - overlap) * window)
    n_windows = int((n - window) // shift) + 1
    med = np.array(median, dtype=np.float32, copy=True)
    dev = np.array(mad, dtype=np.float32, copy=True)
    centre = np.zeros(n_windows + 2, dtype=np.float32)
    for q in range(1, n_windows + 1):
        i1 = q * shift
        centre[q] = (i1 + min(n, i1 + window)) / 2.0
    med[0], dev[0], centre[0] = med[1], dev[1], 0.0
    med[-1], dev[-1], centre[-1] = med[-2], dev[-2], n
    return centre, med + n_dev * dev


def interp_threshold(samples, centre, nodes):
    """The reference's interp1d(kind="slinear", bounds_error=False, fill_value=(first, last)) at
    `samples`, in float64 and in SciPy's own operation order, so that the threshold is bit-identical
    to the reference's (checked live against it in tests/test_reference_live.py): an order-1
    B-spline through the nodes, evaluated by de Boor's recursion -- on [xa, xb) with w = 1 / (xb - xa):
    ya * (w * (xb - x)) + yb * (w * (x - xa)).  (np.interp's ya + slope * (x - xa) differs from it in
    the last bit at a third of the samples.)"""
    x = np.asarray(samples, dtype=np.float64)
    t = np.asarray(centre, dtype=np.float64)
    y = np.asarray(nodes, dtype=np.float64)
    if t.size < 2 or np.any(np.diff(t) <= 0):
        # duplicate knots (the empty last window of bp_threshold_nodes): SciPy refuses them; keep the
        # piecewise-linear definition there
        return np.interp(x, t, y, left=nodes[0], right=nodes[-1])
    i = np.clip(np.searchsorted(t, x, side="right") - 1, 0, t.size - 2)
    xa, xb = t[i], t[i + 1]
    w = 1.0 / (xb - xa)
    out = 0.0 + y[i] * (w * (xb - x))
    out = out + y[i + 1] * (w * (x - xa))
    out = np.where(x < t[0], np.float64(nodes[0]), out)
    return np.where(x > t[-1], np.float64(nodes[-1]), out)


def select_cc_indexes(cc_t, threshold, search_win, *, step, sr, data_duration_sec,
                      n_dev_threshold, min_freq_hz, data_buffer_sec, threshold_type="rms",
                      remove_edges=True, anomalous_cdf_at_mean_plus_1sig=0.50,
                      window_for_validation_Tmax=100.0):
    """Peak list of one CC series (MF-4), BPMF/similarity_search.py:187-286.

    Explicit keyword arguments replace the reference's module-level config (`cfg.N_DEV_MF_THRESHOLD`,
    `cfg.MIN_FREQ_HZ`, `cfg.DATA_BUFFER_SEC`) and `self.data.sr / duration / step`.
    Returns CC indices (multiply by `step` for data samples)."""
    cc_t = np.asarray(cc_t)
    threshold = np.broadcast_to(np.asarray(threshold), cc_t.shape)
    idx = list(np.flatnonzero(cc_t > threshold))
    one_sigma = threshold / n_dev_threshold
    if threshold_type == "mad":
        one_sigma = one_sigma * 1.48
    # sequential pair-wise merge with the reference's own bookkeeping: after each removal the
    # comparison pointer stays on the survivor (:240-251)
    removed = 0
    for q in range(1, len(idx)):
        cur, prev = idx[q - removed], idx[q - removed - 1]
        if cur - prev < search_win:
            idx.remove(prev if cc_t[cur] > cc_t[prev] else cur)
            removed += 1
    idx = np.asarray(idx, dtype=np.int64)

    if anomalous_cdf_at_mean_plus_1sig > 0.0 and idx.size:
        win = int(1.0 / min_freq_hz * window_for_validation_Tmax)
        keep = np.ones(idx.size, dtype=bool)
        for q, i in enumerate(idx):
            i0 = max(0, i - win // 2)
            i1 = i0 + win
            if i1 >= cc_t.size:
                i1 = cc_t.size - 1
                i0 = i1 - win
            seg = cc_t[i0:i1]
            left, right = seg[: win // 2], seg[win // 2:]
            frac = min(np.sum(left < one_sigma[i]) / float(len(left)),
                       np.sum(right < one_sigma[i]) / float(len(right)))
            keep[q] = frac >= anomalous_cdf_at_mean_plus_1sig
        idx = idx[keep]

    if remove_edges:
        samples = idx * step
        idx = idx[samples >= sec_to_samp(data_buffer_sec, sr)]
        samples = idx * step
        idx = idx[samples < sec_to_samp(data_duration_sec + data_buffer_sec, sr)]
    return idx


def time_dependent_threshold_mad(time_series, sliding_window, n_dev, overlap=0.66,
                                 white_noise=None):
    """MAD variant of the MF detection threshold (MF-5), BPMF/similarity_search.py:1079-1113."""
    x = np.array(time_series, copy=True)
    n = x.size
    half = sliding_window // 2
    shift = int((1.0 - overlap) * sliding_window)
    zeros = x == 0.0
    n_zeros = int(zeros.sum())
    if white_noise is None:
        white_noise = np.random.normal(size=n_zeros).astype("float32")
    centre0 = np.median(x[~zeros])
    dev0 = np.median(np.abs(x[~zeros] - centre0))
    x[zeros] = white_noise[:n_zeros] * dev0 + centre0
    wins = np.lib.stride_tricks.sliding_window_view(x, sliding_window)[::shift, :]
    centre = np.median(wins, axis=-1)
    dev = np.median(np.abs(wins - centre[:, None]), axis=-1)
    thr = centre + n_dev * dev
    thr[1:] = np.maximum(thr[:-1], thr[1:])
    thr[:-1] = np.maximum(thr[:-1], thr[1:])
    where = np.arange(half, n - (sliding_window - half)) // shift
    where[where >= thr.size] = thr.size - 1
    thr = thr[where]
    return np.hstack((thr[0] * np.ones(half, dtype=np.float32), thr,
                      thr[-1] * np.ones(sliding_window - half, dtype=np.float32)))


def bp_time_dependent_threshold(network_response, window, n_dev, overlap=0.75):
    """Detection threshold on the maximum beam (BP side of row BP-6),
    BPMF/template_search.py:1418-1487: median + n_dev * MAD over sliding windows (float32
    per-window values), the first/last window repeated at the ends, linear interpolation
    between window centres."""
    x = np.asarray(network_response)
    n = x.size
    shift = int((1.0 - overlap) * window)
    n_windows = int((n - window) // shift) + 1
    med = np.zeros(n_windows + 2, dtype=np.float32)
    mad = np.zeros(n_windows + 2, dtype=np.float32)
    for q in range(1, n_windows + 1):
        i1 = q * shift
        seg = x[i1:min(n, i1 + window)]
        m = np.median(seg)
        med[q] = m
        mad[q] = np.median(np.abs(seg - m))
    centre, nodes = bp_threshold_nodes(n, window, overlap, med, mad, n_dev)
    return interp_threshold(np.arange(n, dtype=np.float64), centre, nodes)


def excess_kurtosis_f32(a):
    """scipy.stats.kurtosis(a) (Fisher, biased) of a 1-D float32 series exactly as SciPy evaluates it
    on a float32 array -- the `sanity_check` of MatchedFilter._find_detections_t
    (BPMF/similarity_search.py:633-642): float32 mean (NumPy's pairwise sum / count), float32
    powers of the zero-mean series, float32 means of those, m4 / m2**2 - 3; NaN when
    m2 <= (eps * mean)**2.  Restated without SciPy so that the device kernel
    (csrc/stats.hip, bpmf_row_kurtosis_dev) has a host mirror; tests compare both with SciPy."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    mean = np.mean(a, keepdims=True)
    d = a - mean
    s2 = d ** 2
    m2 = np.mean(s2)
    m4 = np.mean(s2 ** 2)
    return kurtosis_from_moments_f32(mean[0], m2, m4)


def kurtosis_from_moments_f32(mean, m2, m4):
    """The last expression of scipy.stats.kurtosis on ONE float32 series, `m4 / m2**2.0 - 3` (NaN when
    m2 <= (eps * mean)**2), on NumPy float32 SCALARS as SciPy evaluates it there.  Not a detail: a NumPy scalar
    `**` is the C library's powf, which glibc does not always round like the exact square an array `**` gives
    (one random row in 2500 ends 2 ulp apart), and BPMF passes one series (similarity_search.py:640).  The device
    hands out (mean, m2, m4) per row (bpmf_row_kurtosis_parts_dev) and the host finishes here, with whatever
    NumPy / libm the reference itself would run on."""
    with np.errstate(all="ignore"):
        return _kurtosis_from_moments(np.float32(mean), np.float32(m2), np.float32(m4))


_F32_EPS = np.finfo(np.float32).eps
_F32_NAN = np.float32(np.nan)
_F32_THREE = np.float32(3)


def _kurtosis_from_moments(mean, m2, m4):
    """(np.float32 scalars in, warnings handled by the caller: a row of a loop over a CC matrix)"""
    if m2 <= (_F32_EPS * mean) ** 2:
        return _F32_NAN
    return np.float32(m4 / m2 ** 2.0) - _F32_THREE


def kurtosis_from_moments_rows(parts):
    """kurtosis_from_moments_f32 for every row of a (rows, 3) float32 array of (mean, m2, m4)."""
    parts = np.asarray(parts, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.array([_kurtosis_from_moments(p[0], p[1], p[2]) for p in parts], dtype=np.float32)


# ---------------------------------------------------------------- event relocation ---
def likelihood(beam_column):
    """Beamformer._likelihood (BPMF/template_search.py:498-506): the beam over the grid at the time of
    maximum focusing, rescaled to [0, 1] -- (x - min) / (max - min), clipped."""
    x = np.asarray(beam_column)
    like = (x - x.min()) / (x.max() - x.min())
    return np.clip(like, a_min=0.0, a_max=1.0)


def focus_from_max(maxbeam, arg):
    """Host mirror of the focus kernel of the batched relocation (csrc/bp_relocate.hip): the point of maximum
    focusing of a (K, N) beam volume from its per-sample maximum over the sources alone -- `maxbeam` (N,) and
    `arg` (N,), the running maximum of the build (start (0, source 0), replaced on strictly greater, sources
    ascending: arg[t] is the LOWEST source that reaches maxbeam[t]).  With M = maxbeam.max(): among the samples
    with maxbeam == M the smallest arg, then the smallest such sample.  Returns (src_idx, time_idx, M).

    Equals np.unravel_index(vol.argmax(), vol.shape) -- the first maximum in source-major order -- whenever
    M > 0 or the whole volume is zero: the lowest source that reaches M anywhere is the smallest arg among the
    samples that reach M, and its first sample there is the smallest of them.  (M == 0 over a volume with negative
    beams hides where its zeros are; workflow.relocate_events redoes such an event on the volume.)"""
    mb = np.asarray(maxbeam)
    a = np.asarray(arg)
    m = mb.max()
    at_max = np.flatnonzero(mb == m)
    src = a[at_max].min()
    time_idx = at_max[a[at_max] == src][0]
    return int(src), int(time_idx), m


def gibbs_weights(maxbeam, effective_kT=0.33):
    """Likelihood of the "temporal" uncertainty method of Event.relocate_beam
    (BPMF/dataset.py:2224-2231): exp(-(max - maxbeam) / effective_kT)."""
    mb = np.asarray(maxbeam)
    return np.exp(-(mb.max() - mb) / effective_kT)


DOMAIN_EARTH_RADIUS_KM = 6371.0     # the sphere of Beamformer._rectangular_domain


def rectangular_domain(lon0, lat0, longitudes, latitudes, side_km=100.0):
    """Beamformer._rectangular_domain (BPMF/template_search.py:1232-1267), operation for operation in float64:
    the sources of a grid inside a rectangle of `side_km` centred on (lon0, lat0), on a sphere of 6371 km.
    `longitudes`, `latitudes`: (K,) coordinates of the grid.  Returns a (K,) bool array.  (The reference scales the
    LATITUDE differences by the length of a degree along the parallel of lat0 and the longitude differences by
    the length of a degree of a great circle; so does this.)"""
    lat0 = np.float64(lat0)
    lon0 = np.float64(lon0)
    R_earth_km = DOMAIN_EARTH_RADIUS_KM
    colat0 = 90.0 - lat0
    Rlat = R_earth_km * np.sin(np.deg2rad(colat0))
    dist_per_lat = 2.0 * np.pi * (1.0 / 360.0) * Rlat
    dist_per_lon = 2.0 * np.pi * (1.0 / 360.0) * R_earth_km
    longitudes = np.asarray(longitudes, dtype=np.float64)
    latitudes = np.asarray(latitudes, dtype=np.float64)
    return (np.abs(longitudes - lon0) * dist_per_lon < side_km / 2.0) & (
        np.abs(latitudes - lat0) * dist_per_lat < side_km / 2.0)


def domain_scale_per_latitude(latitudes):
    """`dist_per_lat` of rectangular_domain for every source of a grid as the centre: table[k] is the scalar
    the function computes for lat0 = latitudes[k] (same expression, evaluated on the vector)."""
    latitudes = np.asarray(latitudes, dtype=np.float64)
    colat0 = 90.0 - latitudes
    Rlat = DOMAIN_EARTH_RADIUS_KM * np.sin(np.deg2rad(colat0))
    return 2.0 * np.pi * (1.0 / 360.0) * Rlat


def domain_scale_per_longitude():
    """`dist_per_lon` of rectangular_domain: the length in km of a degree of a great circle of the 6371 km sphere."""
    return 2.0 * np.pi * (1.0 / 360.0) * DOMAIN_EARTH_RADIUS_KM


def reduced_latitude_sin_cos(latitudes):
    """(sin u, cos u) of the reduced latitudes u = atan((1 - f) tan(lat)) on WGS84, as geodesic_distance_m
    computes them for its end points."""
    lat = np.asarray(latitudes, dtype=np.float64)
    u = np.arctan((1.0 - WGS84_F) * np.tan(np.deg2rad(lat)))
    return np.sin(u), np.cos(u)


WGS84_A = 6378137.0                 # semi-major axis, m
WGS84_F = 1.0 / 298.257223563       # flattening


def geodesic_distance_m(lon0, lat0, lon, lat, max_iter=200, tol=1e-12, nonconverged="raise"):
    """Length in metres of the WGS84 geodesics from (lon0, lat0) to every (lon[i], lat[i]), degrees in --
    what ``cartopy.geodesic.Geodesic().inverse(...)[:, 0]`` returns in
    Beamformer._compute_location_uncertainty (BPMF/template_search.py:1310-1320; cartopy wraps
    GeographicLib on the same ellipsoid).  Vincenty's inverse iteration, vectorised: within a fraction of a
    millimetre of GeographicLib for every pair that is not nearly antipodal.  Vincenty's iteration does not
    converge for pairs within about half a degree of antipodal, where GeographicLib still returns a length:
    `nonconverged="raise"` (default) raises ValueError rather than return a wrong length;
    `nonconverged="antipodal"` gives those pairs pi (a + b) / 2 = 20 003.917 km and leaves every other pair exact.
    (pi b = 19 970.3, pi a = 20 037.5 km.)  Exact antipodes are joined over a pole by half a meridian,
    20 003.931 km: for them the value is 14 m short.  Any other pair the iteration gives up on has its second point
    within about 180 f = 0.6 degrees, some 70 km, of the antipode of its first, so by the triangle inequality its
    true length is within that of the half meridian, and the value within about 70 km (0.35 %) of the true length.
    Host code (float64 NumPy): a domain has a few thousand sources."""
    if nonconverged not in ("raise", "antipodal"):
        raise ValueError("nonconverged must be 'raise' or 'antipodal'")
    lon = np.atleast_1d(np.asarray(lon, dtype=np.float64))
    lat = np.atleast_1d(np.asarray(lat, dtype=np.float64))
    lon, lat = np.broadcast_arrays(lon, lat)
    f, a = WGS84_F, WGS84_A
    b = (1.0 - f) * a
    u1 = np.arctan((1.0 - f) * np.tan(np.deg2rad(float(lat0))))
    u2 = np.arctan((1.0 - f) * np.tan(np.deg2rad(lat)))
    su1, cu1, su2, cu2 = np.sin(u1), np.cos(u1), np.sin(u2), np.cos(u2)
    big_l = np.deg2rad((lon - float(lon0) + 180.0) % 360.0 - 180.0)     # longitude difference in [-180, 180)
    def at(lam):
        sl, cl = np.sin(lam), np.cos(lam)
        sin_sig = np.hypot(cu2 * sl, cu1 * su2 - su1 * cu2 * cl)
        cos_sig = su1 * su2 + cu1 * cu2 * cl
        sig = np.arctan2(sin_sig, cos_sig)
        sin_al = np.where(sin_sig > 0.0, cu1 * cu2 * sl / np.where(sin_sig > 0.0, sin_sig, 1.0), 0.0)
        cos2_al = 1.0 - sin_al * sin_al
        cos_2sm = np.where(cos2_al > 0.0, cos_sig - 2.0 * su1 * su2 / np.where(cos2_al > 0.0, cos2_al, 1.0), 0.0)
        return sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm

    lam = big_l.copy()
    done = np.zeros(lam.shape, dtype=bool)
    # (a point that has converged is left alone, and the lengths come from one evaluation at the final
    # longitudes: the result of a point does not depend on what else is in the call)
    for _ in range(max_iter):
        sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
        c = f / 16.0 * cos2_al * (4.0 + f * (4.0 - 3.0 * cos2_al))
        new = big_l + (1.0 - c) * f * sin_al * (
            sig + c * sin_sig * (cos_2sm + c * cos_sig * (-1.0 + 2.0 * cos_2sm * cos_2sm)))
        conv = np.abs(new - lam) < tol
        lam = np.where(done, lam, new)
        done = done | conv
        if done.all():
            break
    if not done.all() and nonconverged == "raise":
        raise ValueError("geodesic_distance_m: no convergence (nearly antipodal points)")
    sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm = at(lam)
    usq = cos2_al * (a * a - b * b) / (b * b)
    big_a = 1.0 + usq / 16384.0 * (4096.0 + usq * (-768.0 + usq * (320.0 - 175.0 * usq)))
    big_b = usq / 1024.0 * (256.0 + usq * (-128.0 + usq * (74.0 - 47.0 * usq)))
    d_sig = big_b * sin_sig * (cos_2sm + big_b / 4.0 * (
        cos_sig * (-1.0 + 2.0 * cos_2sm * cos_2sm)
        - big_b / 6.0 * cos_2sm * (-3.0 + 4.0 * sin_sig * sin_sig) * (-3.0 + 4.0 * cos_2sm * cos_2sm)))
    return np.where(done, b * big_a * (sig - d_sig), np.pi * (a + b) / 2.0)


def compute_location_uncertainty(event_longitude, event_latitude, event_depth, likelihood,
                                 source_longitude, source_latitude, source_depth):
    """Beamformer._compute_location_uncertainty (BPMF/template_search.py:1269-1333) without cartopy:
    (hunc, vunc) in km -- the likelihood-weighted mean geodesic distance of the domain's sources to the
    event and their mean absolute depth difference.  `source_*`: the coordinates of the sources OF THE
    DOMAIN (the reference indexes its grid with `domain`), `likelihood`: theirs.
    One limitation against cartopy / GeographicLib: a source within about half a degree of the event's
    ANTIPODE (never the case for a regional source grid) gets the length pi (a + b) / 2 = 20 003.917 km, within
    about 70 km (0.35 %) of its true geodesic distance (14 m for the antipode itself), instead of failing the whole
    relocation (geodesic_distance_m, nonconverged="antipodal"); every other distance is exact to a fraction of a millimetre."""
    d_km = geodesic_distance_m(event_longitude, event_latitude, source_longitude, source_latitude,
                               nonconverged="antipodal") / 1000.0
    depth_diff = np.abs(float(event_depth) - np.asarray(source_depth, dtype=np.float64))
    return location_uncertainty(likelihood, d_km, depth_diff)


def location_uncertainty(likelihood_domain, distances_km, depth_diff_km):
    """Beamformer._compute_location_uncertainty (BPMF/template_search.py:1269-1333) behind its geodesic
    call: likelihood-weighted mean epicentral distance and mean absolute depth difference of the
    sources of the domain.  `distances_km`: distance of every source of the domain to the event (the
    reference takes cartopy's Geodesic().inverse(...)[:, 0] / 1000); returns (hunc, vunc) in km."""
    like = np.asarray(likelihood_domain)
    hunc = np.sum(like * np.asarray(distances_km)) / np.sum(like)
    vunc = np.sum(like * np.asarray(depth_diff_km)) / np.sum(like)
    return hunc, vunc


def multiples_pair_mask(ellipsoid_dist, distance_criterion, intertemplate_cc=None, similarity_criterion=-1.0):
    """The template-pair test of ``TemplateGroup.remove_multiples`` (BPMF/dataset.py:5262-5274) for every pair at once:
    pair_ok[i, j] = ellipsoid_dist[i, j] < distance_criterion, and -- only when similarity_criterion > -1 --
    & (intertemplate_cc[i, j] >= similarity_criterion).  (T, T) arrays in, (T, T) bool out; the comparisons are
    NumPy's own on the arrays as given (a NaN fails both), so the flagging itself compares no matrix value."""
    dist = np.asarray(ellipsoid_dist)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError(f"multiples_pair_mask: ellipsoid_dist must be (T, T); got {dist.shape}")
    ok = dist < distance_criterion
    if similarity_criterion > -1.0:
        if intertemplate_cc is None:
            raise ValueError("multiples_pair_mask: similarity_criterion > -1 needs intertemplate_cc")
        sim = np.asarray(intertemplate_cc)
        if sim.shape != dist.shape:
            raise ValueError(f"multiples_pair_mask: intertemplate_cc must be {dist.shape}; got {sim.shape}")
        ok = ok & (sim >= similarity_criterion)
    return np.ascontiguousarray(ok)


def multiples_arguments(origin_time_sec, template_rows, cc, pair_ok, n_templates=None):
    """The arguments of flag_multiples, checked and typed: (t float64 (n,), rows int32 (n,), cc float32 (n,),
    pair_ok bool (T, T)).  ValueError for mismatched lengths, a pair_ok that is not square, a row outside [0, T)
    or a cc that is not finite (the keeper is the largest cc: a NaN has no order).  pair_ok=None with `n_templates`:
    the mask lives elsewhere (on the device) and only its size is known; None comes back in its place."""
    t = np.ascontiguousarray(np.asarray(origin_time_sec, dtype=np.float64).reshape(-1))
    rows = np.asarray(template_rows).reshape(-1)
    if rows.size and not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("flag_multiples: template_rows must be integers")
    c = np.ascontiguousarray(np.asarray(cc, dtype=np.float32).reshape(-1))
    if pair_ok is None and n_templates is not None:
        ok, T = None, int(n_templates)
    else:
        ok = np.asarray(pair_ok)
        if ok.ndim != 2 or ok.shape[0] != ok.shape[1]:
            raise ValueError(f"flag_multiples: pair_ok must be (T, T); got {ok.shape}")
        ok = np.ascontiguousarray(ok.astype(bool))
        T = ok.shape[0]
    if not (t.shape == rows.shape == c.shape):
        raise ValueError("flag_multiples: origin_time_sec, template_rows and cc must have one entry per event")
    if rows.size and (rows.min() < 0 or rows.max() >= T):
        raise ValueError(f"flag_multiples: a template row lies outside [0, {T})")
    if not np.isfinite(c).all():
        raise ValueError("flag_multiples: cc must be finite")
    return t, np.ascontiguousarray(rows.astype(np.int32)), c, ok


def flag_multiples(origin_time_sec, template_rows, cc, pair_ok, dt_criterion):
    """The loop of ``TemplateGroup.remove_multiples`` (BPMF/dataset.py:5214-5282) on plain arrays: which events of
    a catalog stay `unique_event` when several templates detect the same event.  `origin_time_sec` (n,) float64,
    `template_rows` (n,) rows of `pair_ok`, `cc` (n,) float32 and finite, `pair_ok` (T, T) bool
    (multiples_pair_mask), `dt_criterion` seconds.  Returns (n,) bool in the order of the input.

    The events are visited in the STABLE order of their origin times (equal times: input order -- the reference's
    pandas quicksort leaves that order to the platform).  A visited event n1 that is still unique gathers its
    neighbours -- itself and the following events n2 for as long as the float64 sum of the inter-event times
    ie[n1 + 1] + ... + ie[n2], accumulated left to right, stays < dt_criterion (the reference's running sum, not
    t[n2] - t[n1]) --, keeps those still unique, and of them the ones with pair_ok[row of n1, row of m].  Two or more
    of these are multiples: all are flagged False, then the one with the largest cc (equal cc: the earliest in the
    visiting order, np.argmax) is set True again.  This is the definition workflow.flag_multiples (csrc/multiples.hip)
    is tested against, element for element."""
    t, rows, c, ok = multiples_arguments(origin_time_sec, template_rows, cc, pair_ok)
    n = t.shape[0]
    dt_criterion = float(dt_criterion)
    order = np.argsort(t, kind="stable")
    ts, r, c = t[order], rows[order], c[order]
    ie = np.hstack(([0.0], ts[1:] - ts[:-1])).tolist() if n else []      # Python floats: the same float64 additions
    unique = np.ones(n, dtype=bool)
    for n1 in range(n - 1):
        if not unique[n1]:
            continue
        n2 = n1 + 1
        acc = ie[n2]
        while acc < dt_criterion:
            n2 += 1
            if n2 >= n:
                break
            acc += ie[n2]
        if n2 - n1 < 2:
            continue
        candidates = n1 + np.flatnonzero(unique[n1:n2])
        multiples = candidates[ok[r[n1], r[candidates]]]
        if len(multiples) >= 2:
            unique[multiples] = False
            unique[multiples[np.argmax(c[multiples])]] = True
    out = np.empty(n, dtype=bool)
    out[order] = unique
    return out


# ---- pair geometry (BPMF/utils.py: compute_distances :1419-1498; BPMF/dataset.py: compute_intertemplate_dist,
# ---- compute_dir_errors, compute_ellipsoid_dist :4568-4688, the weights of compute_intertemplate_cc :4787-4816) ----
DIR_ERROR_CHI2_68_3DF = 3.52          # s_68_3df of compute_dir_errors
DIR_ERROR_DEFAULT_KM = 15.0           # a template without cov_mat


def _coordinates(name, lon, lat, dep):
    """(lon, lat float64, dep as given) of one side of compute_distances, checked: 1-D, one length, finite, latitudes
    within [-90, 90]."""
    lon, lat, dep = (np.atleast_1d(np.asarray(x)) for x in (lon, lat, dep))
    if not (lon.ndim == lat.ndim == dep.ndim == 1 and lon.shape == lat.shape == dep.shape):
        raise ValueError(f"{name}: longitudes, latitudes and depths must be 1-D and of one length; got {lon.shape}, "
                         f"{lat.shape}, {dep.shape}")
    for what, x in (("longitudes", lon), ("latitudes", lat), ("depths", dep)):
        if x.dtype.kind not in "fiu":
            raise ValueError(f"{name}: {what} must be real numbers; got {x.dtype}")
    lon, lat = lon.astype(np.float64), lat.astype(np.float64)
    if dep.dtype != np.float32:
        dep = dep.astype(np.float64)
    if not (np.isfinite(lon).all() and np.isfinite(lat).all() and np.isfinite(dep).all()):
        raise ValueError(f"{name}: coordinates must be finite")
    if lat.size and (lat.min() < -90.0 or lat.max() > 90.0):
        raise ValueError(f"{name}: latitudes must lie in [-90, 90]")
    return lon, lat, dep


def distances_arguments(src_lon, src_lat, src_dep, rcv_lon, rcv_lat, rcv_dep):
    """The arguments of compute_distances_host, checked and typed: (source lon, lat, dep, receiver lon, lat, dep,
    depth_float64).  Longitudes and latitudes are widened to float64 as given.  depth_float64 is False when both depth
    arrays are float32 -- the hypocentral step then stays in float32, as NumPy's promotion has it in the reference --
    and True otherwise (the depths are then float64)."""
    s = _coordinates("compute_distances: sources", src_lon, src_lat, src_dep)
    r = _coordinates("compute_distances: receivers", rcv_lon, rcv_lat, rcv_dep)
    depth_float64 = not (s[2].dtype == np.float32 and r[2].dtype == np.float32)
    if depth_float64:
        s, r = (s[0], s[1], s[2].astype(np.float64)), (r[0], r[1], r[2].astype(np.float64))
    return s + r + (depth_float64,)


def hypocentral_from_metres(metres, src_dep, rcv_dep):
    """The two rounding steps of utils.compute_distances behind its geodesic call, on (K, R) float64 `metres`:
    epicentral = float32(metres / 1000.0); hypocentral = sqrt(epicentral ** 2 + (src_dep - rcv_dep[s]) ** 2) column by
    column in NumPy's promoted dtype -- float32 throughout for float32 depths, float64 from the sum on for float64
    depths -- stored as float32.  Returns (hypocentral, epicentral)."""
    metres = np.asarray(metres, dtype=np.float64)
    epicentral = np.zeros(metres.shape, dtype=np.float32)
    hypocentral = np.zeros(metres.shape, dtype=np.float32)
    for s in range(metres.shape[1]):
        epicentral[:, s] = metres[:, s] / 1000.0
        hypocentral[:, s] = np.sqrt(epicentral[:, s] ** 2 + (src_dep - rcv_dep[s]) ** 2)
    return hypocentral, epicentral


def compute_distances_host(src_lon, src_lat, src_dep, rcv_lon, rcv_lat, rcv_dep, return_epicentral_distances=False,
                           nonconverged="raise"):
    """utils.compute_distances (BPMF/utils.py:1419-1498) with geodesic_distance_m in place of
    ``cartopy.geodesic.Geodesic().inverse``: (K, R) float32 hypocentral distances in km between K sources and R
    receivers, and with `return_epicentral_distances` the (K, R) float32 epicentral distances as well.  Degrees and
    km in.  As in the reference the RECEIVER is the geodesic's first point, and the roundings are its own
    (hypocentral_from_metres).  `nonconverged`: what a nearly antipodal pair does (geodesic_distance_m).  This is the
    definition workflow.compute_distances (csrc/geometry.hip) is tested against."""
    slon, slat, sdep, rlon, rlat, rdep, _ = distances_arguments(src_lon, src_lat, src_dep, rcv_lon, rcv_lat, rcv_dep)
    if nonconverged not in ("raise", "antipodal"):
        raise ValueError("nonconverged must be 'raise' or 'antipodal'")
    metres = np.zeros((slon.shape[0], rlon.shape[0]), dtype=np.float64)
    for s in range(rlon.shape[0]):
        if slon.shape[0]:
            metres[:, s] = geodesic_distance_m(rlon[s], rlat[s], slon, slat, nonconverged=nonconverged)
    hypocentral, epicentral = hypocentral_from_metres(metres, sdep, rdep)
    return (hypocentral, epicentral) if return_epicentral_distances else hypocentral


def mercator_xy(lon, lat, central_longitude, a=WGS84_A, f=WGS84_F):
    """Ellipsoidal Mercator with k_0 = 1 (PROJ's `merc`, Snyder 1987 eq. 7-6 / 7-7), the projection
    ``cartopy.crs.Mercator(central_longitude, min_latitude, max_latitude)`` selects -- its two latitude arguments only
    set the map's bounds:  x = a dlon, dlon = lon - central_longitude wrapped to [-180, 180] degrees, in radians;
    y = a (asinh(tan phi) - e atanh(e sin phi)), e^2 = f (2 - f).  Degrees in, metres out (float64); a pole gives an
    infinite y.  Restated from the documentation of PROJ and Snyder's worked example, NOT verified against cartopy
    itself (tests/test_template_geometry_cartopy_live.py does that where cartopy is installed)."""
    lon = np.asarray(lon, dtype=np.float64)
    lat = np.asarray(lat, dtype=np.float64)
    e = np.sqrt(f * (2.0 - f))
    dlon = lon - np.float64(central_longitude)
    dlon = np.where(np.abs(dlon) > 180.0, (dlon + 180.0) % 360.0 - 180.0, dlon)
    phi = np.deg2rad(lat)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = a * (np.arcsinh(np.tan(phi)) - e * np.arctanh(e * np.sin(phi)))
    y = np.where(np.abs(lat) == 90.0, np.copysign(np.inf, lat), y)
    return a * np.deg2rad(dlon), y


def template_geometry_arguments(longitude, latitude, depth, cov_mat=None, has_cov=None, depth_unit="reference"):
    """The arguments of template_geometry_host, checked and typed as the reference types them: (lon, lat, dep float32
    (T,), xyz float64 (T, 3), cov float64 (T, 3, 3) or None, has_cov bool (T,)).  xyz: Mercator x, y in metres about
    the mean of the float32 longitudes, and the depth -- in km ("reference") or in metres ("metres")."""
    if depth_unit not in ("reference", "metres"):
        raise ValueError("template_geometry: depth_unit must be 'reference' or 'metres'")
    lon, lat, dep = _coordinates("template_geometry", longitude, latitude, depth)
    T = lon.shape[0]
    if T == 0:
        raise ValueError("template_geometry: no template")
    lon, lat, dep = np.float32(lon), np.float32(lat), np.float32(dep)
    if not np.isfinite(dep).all():
        raise ValueError("template_geometry: coordinates must be finite")
    cov = None
    if cov_mat is not None:
        cov = np.asarray(cov_mat, dtype=np.float64)
        if cov.shape != (T, 3, 3):
            raise ValueError(f"template_geometry: cov_mat must be ({T}, 3, 3); got {cov.shape}")
        cov = np.ascontiguousarray(cov)
    if has_cov is None:
        has = np.full(T, cov is not None)
    else:
        has = np.asarray(has_cov)
        if has.shape != (T,):
            raise ValueError(f"template_geometry: has_cov must be ({T},); got {has.shape}")
        has = has.astype(bool)
        if has.any() and cov is None:
            raise ValueError("template_geometry: has_cov names templates but cov_mat is None")
    if cov is not None and not np.isfinite(cov[has]).all():
        raise ValueError("template_geometry: cov_mat must be finite where has_cov is set")
    x, y = mercator_xy(lon, lat, np.mean(lon))
    z = dep.astype(np.float64) * 1000.0 if depth_unit == "metres" else dep.astype(np.float64)
    return lon, lat, dep, np.stack([x, y, z], axis=1), cov, has


def dir_errors_host(xyz, cov, has_cov):
    """compute_dir_errors (BPMF/dataset.py:4639-4660) behind its projection: (T, T) float32, row t the length of
    template t's uncertainty ellipsoid towards every template.  Per pair in float64: d = X[u] - X[t];
    n = sqrt((dx^2 + dy^2) + dz^2); d / n with NaN (u at t) replaced by 0; cov_dir = |sum_i (sum_j C_ij u_j) u_i| with
    j, then i, summed in index order, unfused (the reference's BLAS leaves that order open);
    float32(sqrt(3.52 cov_dir)).  A row without covariance is 15.0."""
    T = xyz.shape[0]
    out = np.zeros((T, T), dtype=np.float32)
    for t in range(T):
        if not has_cov[t]:
            out[t, :] = DIR_ERROR_DEFAULT_KM
            continue
        d = xyz - xyz[t, :]
        n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = d / n[:, np.newaxis]
        u[np.isnan(u)] = 0.0
        c = cov[t]
        rows = [(c[i, 0] * u[:, 0] + c[i, 1] * u[:, 1]) + c[i, 2] * u[:, 2] for i in range(3)]
        cov_dir = np.abs((rows[0] * u[:, 0] + rows[1] * u[:, 1]) + rows[2] * u[:, 2])
        out[t, :] = np.sqrt(DIR_ERROR_CHI2_68_3DF * cov_dir)
    return out


def template_geometry_host(longitude, latitude, depth, cov_mat=None, has_cov=None, depth_unit="reference"):
    """The pair matrices of a TemplateGroup (BPMF/dataset.py:4568-4688) without cartopy: a dict of
    `intertemplate_dist`, `dir_errors` and `ellipsoid_dist`, each (T, T) float32 in km.

    The coordinates are cast to float32 first, as the reference does.  intertemplate_dist =
    compute_distances_host(templates, templates) (a nearly antipodal pair gets pi (a + b) / 2);  dir_errors =
    dir_errors_host on the Mercator coordinates about central_longitude = np.mean of the float32 longitudes
    (mercator_xy: restated from the documentation, not verified against cartopy);  ellipsoid_dist =
    (intertemplate_dist - dir_errors) - dir_errors.T in float32.  `cov_mat` (T, 3, 3), `has_cov` (T,) bool (default:
    every template has one if cov_mat is given, none otherwise).

    Kept as the reference has it: the direction's X and Y are Mercator METRES (stretched by 1 / cos(latitude)) while Z
    is the depth in KILOMETRES, so every direction is nearly horizontal and dir_errors is essentially the horizontal
    extent of the ellipsoid.  depth_unit="metres" multiplies the depths by 1000 before the directions are formed: the
    consistent alternative, which the reference does not compute."""
    lon, lat, dep, xyz, cov, has = template_geometry_arguments(longitude, latitude, depth, cov_mat, has_cov, depth_unit)
    dist = compute_distances_host(lon, lat, dep, lon, lat, dep, nonconverged="antipodal")
    err = dir_errors_host(xyz, cov, has)
    return {"intertemplate_dist": dist, "dir_errors": err, "ellipsoid_dist": (dist - err) - err.T}


def intertemplate_pair_mask(ellipsoid_dist, distance_threshold):
    """The pairs compute_intertemplate_cc correlates (BPMF/dataset.py:4815-4816): mask[t, u] =
    not (ellipsoid_dist[u, t] > distance_threshold).  The reference reads COLUMN tids[t] of its frame, and the matrix is
    not bitwise symmetric; a NaN is not above the threshold and stays in.  (T, T) in, (T, T) bool out."""
    dist = np.asarray(ellipsoid_dist)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError(f"intertemplate_pair_mask: ellipsoid_dist must be (T, T); got {dist.shape}")
    return np.ascontiguousarray(~(dist.T > distance_threshold))


def intertemplate_station_weights(source_receiver_dist, availability, availability_per_cha, n_stations):
    """The channel weights of compute_intertemplate_cc (BPMF/dataset.py:4787-4814), (T, S, C) float32: per template the
    `n_stations` closest AVAILABLE stations -- filled up, when fewer are available, with the closest of the others --
    carry their per-channel availabilities as 0 / 1, and the whole is divided by its sum (no channel at all: 0 / 0,
    NaN, as the reference).  `source_receiver_dist` (T, S), `availability` (T, S) bool, `availability_per_cha`
    (T, S, C) bool.  Sorting is stable (equal distances: station order), where pandas' quicksort leaves ties to the
    platform; NaN distances sort last."""
    dist = np.asarray(source_receiver_dist)
    avail = np.asarray(availability).astype(bool)
    per_cha = np.asarray(availability_per_cha).astype(bool)
    if dist.ndim != 2 or avail.shape != dist.shape or per_cha.ndim != 3 or per_cha.shape[:2] != dist.shape:
        raise ValueError("intertemplate_station_weights: source_receiver_dist and availability must be (T, S) and "
                         f"availability_per_cha (T, S, C); got {dist.shape}, {avail.shape}, {per_cha.shape}")
    n_stations = int(n_stations)
    if n_stations < 0:
        raise ValueError("intertemplate_station_weights: n_stations must not be negative")
    T, S, C = per_cha.shape
    weights = np.zeros((T, S, C), dtype=np.float32)
    for t in range(T):
        pool = np.flatnonzero(avail[t])
        closest = pool[np.argsort(dist[t, pool], kind="stable")][:n_stations]
        if len(closest) < n_stations:
            others = np.setdiff1d(np.arange(S), closest)
            closest = np.hstack((closest, others[np.argsort(dist[t, others], kind="stable")][:n_stations - len(closest)]))
        weights[t, closest, :] = np.int32(per_cha[t, closest, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        weights /= np.sum(weights, axis=(1, 2), keepdims=True)
    return weights


# ---- SVD-Wiener stack of a template's detections (BPMF/utils.py: bandpass_filter :24-90, SVDWF :667-772;
# ---- BPMF/dataset.py: EventGroup.SVDWF_stack :4275-4374) ----
SVDWF_MAX_SMALL_SIDE = 512            # min(n, m) of one channel's (n, m) matrix (csrc/svdwf.hip)
SVDWF_MAX_LARGE_SIDE = 16384          # max(n, m)
SVDWF_MAX_SINGULAR_VALUES = 8
BANDPASS_MAX_SECTIONS = 8


def butter_bandpass_sos(order, low, high):
    """Second-order sections of a digital Butterworth band-pass of `order` corners between `low` and `high`, both as
    fractions of the Nyquist frequency: what scipy.signal.iirfilter(order, [low, high], btype="bandpass",
    ftype="butter", output="zpk") followed by zpk2sos makes, without SciPy -- the analogue prototype, the band-pass
    transform, the bilinear map, and the sections paired as zpk2sos pairs them (the pole pair closest to the unit circle
    goes last and takes the two zeros nearest to it; the gain goes to the first section).  Returns (order, 6) float64
    rows [b0, b1, b2, 1, a1, a2].  A band so wide that the transform makes real poles is refused."""
    order = int(order)
    low, high = float(low), float(high)
    if not 1 <= order <= BANDPASS_MAX_SECTIONS:
        raise ValueError(f"butter_bandpass_sos: order must be 1 .. {BANDPASS_MAX_SECTIONS}; got {order}")
    if not 0.0 < low < high < 1.0:
        raise ValueError(f"butter_bandpass_sos: need 0 < low < high < 1 (fractions of Nyquist); got {low}, {high}")
    steps = np.arange(-order + 1, order, 2)
    p = -np.exp(1j * np.pi * steps / (2 * order))                  # buttap
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * np.array([low, high]) / fs)
    bw, wo = warped[1] - warped[0], np.sqrt(warped[0] * warped[1])
    p_lp = p * bw / 2                                              # lp2bp_zpk
    root = np.sqrt(p_lp ** 2 - wo ** 2)
    p_bp = np.concatenate((p_lp + root, p_lp - root))
    k_bp = bw ** order
    fs2 = 2.0 * fs                                                 # bilinear_zpk
    p_z = (fs2 + p_bp) / (fs2 - p_bp)
    k_z = k_bp * np.real(1.0 / np.prod(fs2 - p_bp))                # (the zeros at s = 0 give prod(fs2 - 0) = fs2^order ...
    k_z *= fs2 ** order                                            # ... in the numerator)
    if np.any(np.abs(p_z.imag) <= 100 * np.finfo(float).eps * np.abs(p_z)):
        raise ValueError("butter_bandpass_sos: the band is so wide that the band-pass transform makes real poles")
    poles = p_z[p_z.imag > 0]
    poles = poles[np.lexsort((np.abs(poles.imag), poles.real))]    # _cplxreal's order
    if len(poles) != order:
        raise ValueError("butter_bandpass_sos: the poles do not come in conjugate pairs")
    zeros = [1.0] * order + [-1.0] * order                         # s = 0 -> z = 1; s = infinity -> z = -1
    zeros.sort()
    sos = np.zeros((order, 6))
    for si in range(order - 1, -1, -1):
        i = int(np.argmin(np.abs(1 - np.abs(poles))))
        p1 = poles[i]
        poles = np.delete(poles, i)
        pair = []
        for _ in range(2):
            j = int(np.argmin(np.abs(p1 - np.array(zeros))))
            pair.append(zeros.pop(j))
        z1, z2 = pair
        sos[si] = [1.0, -(z1 + z2), z1 * z2, 1.0, -2.0 * p1.real, p1.real * p1.real + p1.imag * p1.imag]
    sos[0, :3] *= k_z
    return sos


def sos_table(sos):
    """`sos` as the contiguous (n_sections, 6) float64 table the filters take: 1 .. 8 finite rows with a0 = 1."""
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= BANDPASS_MAX_SECTIONS:
        raise ValueError(f"sos must be (n_sections, 6) with 1 .. {BANDPASS_MAX_SECTIONS} sections; got {sos.shape}")
    if not np.isfinite(sos).all() or not (sos[:, 3] == 1.0).all():
        raise ValueError("sos must be finite with a0 = 1 in every section")
    return sos


def bandpass_sos(sos=None, freqmin=None, freqmax=None, f_Nyq=None, filter_order=4):
    """The section table of a band-pass call: `sos` itself, or butter_bandpass_sos(filter_order, freqmin / f_Nyq,
    freqmax / f_Nyq)."""
    if sos is not None:
        return sos_table(sos)
    if freqmin is None or freqmax is None or f_Nyq is None:
        raise ValueError("give either sos or freqmin, freqmax and f_Nyq")
    return butter_bandpass_sos(filter_order, float(freqmin) / float(f_Nyq), float(freqmax) / float(f_Nyq))


def sosfilt_rows(sos, x):
    """scipy.signal.sosfilt(sos, x) along the last axis of the (rows, m) float64 `x`, from zero state, in SciPy's
    operation order: per sample the sections run innermost, y = b0 x + z0; z0 = (b1 x - a1 y) + z1;
    z1 = b2 x - a2 y.  Bit for bit SciPy's result."""
    y = np.array(x, dtype=np.float64)
    rows, m = y.shape
    n_sec = sos.shape[0]
    z = np.zeros((n_sec, 2, rows))
    coef = [[float(v) for v in row] for row in sos]
    for t in range(m):
        cur = y[:, t].copy()
        for s in range(n_sec):
            b0, b1, b2, _, a1, a2 = coef[s]
            new = b0 * cur + z[s, 0]
            z[s, 0] = (b1 * cur - a1 * new) + z[s, 1]
            z[s, 1] = b2 * cur - a2 * new
            cur = new
        y[:, t] = cur
    return y


def tukey_window(m, alpha):
    """scipy.signal.windows.tukey(m, alpha) (symmetric), float64."""
    m = int(m)
    if m <= 1 or alpha <= 0:
        return np.ones(max(m, 0))
    alpha = min(float(alpha), 1.0)
    n = np.arange(m, dtype=np.float64)
    width = int(np.floor(alpha * (m - 1) / 2.0))
    w = np.ones(m)
    n1, n3 = n[:width + 1], n[m - width - 1:]
    w[:width + 1] = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / alpha / (m - 1))))
    w[m - width - 1:] = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * n3 / alpha / (m - 1))))
    return w


def bandpass_filter_host(x, sos=None, *, freqmin=None, freqmax=None, f_Nyq=None, filter_order=4, detrend=True,
                         taper_alpha=0.01, zerophase=True):
    """utils.bandpass_filter (BPMF/utils.py:24-90) along the last axis of `x` (..., m), float64, NumPy only.  Per row:
    the mean is subtracted, then the least-squares line (closed form: slope = sum((i - c) x) / sum((i - c)^2) about the
    middle index c, intercept = the mean that is left; the reference solves the same problem with lstsq) -- both only
    with `detrend` --, the row is multiplied by tukey(m, taper_alpha) (`taper_alpha` None: no taper), and the SOS
    cascade (sosfilt_rows) runs forward from zero state and, with `zerophase`, on the reversed row from zero state,
    reversed again.  No padding.  The sections are `sos` (n_sections, 6) or butter_bandpass_sos of the keywords."""
    table = bandpass_sos(sos, freqmin, freqmax, f_Nyq, filter_order)
    x = np.asarray(x)
    y = np.array(x.reshape(-1, x.shape[-1]) if x.ndim else x.reshape(1, 1), dtype=np.float64)
    m = y.shape[1]
    if detrend and m:
        y = y - y.mean(axis=1, keepdims=True)
        d = np.arange(m, dtype=np.float64) - (m - 1) / 2.0
        den = float((d * d).sum())
        slope = (y * d).sum(axis=1, keepdims=True) / den if den > 0 else np.zeros((y.shape[0], 1))
        y = y - (slope * d + y.mean(axis=1, keepdims=True))
    if taper_alpha is not None and m:
        y = y * tukey_window(m, taper_alpha)
    y = sosfilt_rows(table, y)
    if zerophase:
        y = sosfilt_rows(table, y[:, ::-1])[:, ::-1]
    return y.copy().reshape(x.shape)                               # (a copy: C order, no negative stride left)


def wiener_rows_host(p, w):
    """scipy.signal.wiener(p, [w, 1]) of the (n, m) float64 `p`: the local sums of row i run over the rows
    i - w // 2 .. i + (w - 1) // 2 that exist (zero padding: the divisor is always w); noise = the mean local variance
    of the whole matrix; where the local variance is below it the local mean, else
    (p - mean) (1 - noise / var) + mean."""
    n = p.shape[0]
    lo, hi = w // 2, (w - 1) // 2
    s1, s2 = np.zeros_like(p), np.zeros_like(p)
    p2 = p * p
    for d in range(-lo, hi + 1):
        a, b = max(0, -d), min(n, n - d)                           # rows i with 0 <= i + d < n
        if a < b:
            s1[a:b] += p[a + d:b + d]
            s2[a:b] += p2[a + d:b + d]
    mean = s1 / w
    var = s2 / w - mean ** 2
    noise = var.mean()
    with np.errstate(all="ignore"):
        res = (p - mean) * (1 - noise / var) + mean
        return np.where(var < noise, mean, res)


def svdwf_arguments(n, m, expl_var, max_singular_values, wiener_filter_colsize):
    """Checks shared by svdwf_host and workflow.svdwf_stack; returns (expl_var, max_singular_values, w or None)."""
    expl_var, k = float(expl_var), int(max_singular_values)
    if not 0.0 < expl_var <= 1.0:
        raise ValueError(f"svdwf: expl_var must be in (0, 1]; got {expl_var}")
    if not 1 <= k <= SVDWF_MAX_SINGULAR_VALUES:
        raise ValueError(f"svdwf: max_singular_values must be 1 .. {SVDWF_MAX_SINGULAR_VALUES}; got {k}")
    w = None if wiener_filter_colsize is None else int(wiener_filter_colsize)
    if w is not None and not 1 <= w < 2**31:
        raise ValueError(f"svdwf: wiener_filter_colsize must be at least 1; got {w}")
    if m < 1:
        raise ValueError("svdwf: the waveforms hold no samples")
    return expl_var, k, w


def svdwf_host(matrix, expl_var=0.4, max_singular_values=5, wiener_filter_colsize=None, sos=None, taper_alpha=0.01,
               return_rank=False):
    """utils.SVDWF (BPMF/utils.py:667-772) of one channel's (n, m) float32 matrix of detections, restated in float64
    with its quirks; NumPy only.  1. singular values of the matrix, var = cumsum(s^2) / sum(s^2); a zero matrix gives
    zeros (no band-pass); k = min(max_singular_values, 1 + first j with var[j] >= expl_var).  2. for j < min(n, k):
    the rank-one projection P_j = u_j (u_j^T A), left as it is when w = wiener_filter_colsize (default n) is 1, else
    wiener_rows_host(P_j, w); a projection whose filtered form holds a NaN is skipped whole.  3. their sum, passed
    through wiener_rows_host again (w != 1); NaN and +-Inf become 0.  4. with `sos`: bandpass_filter_host (mean, line,
    tukey(m, taper_alpha), zero phase).  5. the result rounded to float32.  Departure: where LAPACK fails the
    reference returns Gaussian noise; here the error is raised.  Returns (n, m) float32 (and k, 0 for a zero matrix,
    with `return_rank`)."""
    a = np.asarray(matrix, dtype=np.float32).astype(np.float64)
    if a.ndim != 2:
        raise ValueError("svdwf_host: matrix must be (n, m)")
    n, m = a.shape
    expl_var, kmax, w = svdwf_arguments(n, m, expl_var, max_singular_values, wiener_filter_colsize)
    out = np.zeros((n, m), dtype=np.float32)
    if n == 0:
        return (out, 0) if return_rank else out
    if w is None:
        w = n
    u, s, _ = np.linalg.svd(a, full_matrices=False)
    var = np.cumsum(s ** 2)
    if var[-1] == 0.0:
        return (out, 0) if return_rank else out
    var = var / var[-1]
    k = min(kmax, int(np.flatnonzero(var >= expl_var)[0]) + 1)
    d = np.zeros((n, m))
    for j in range(min(n, k)):
        proj = np.outer(u[:, j], u[:, j] @ a)
        f = proj if w == 1 else wiener_rows_host(proj, w)
        if np.isnan(f).any():
            continue
        d += f
    if w != 1:
        d = wiener_rows_host(d, w)
    d[~np.isfinite(d)] = 0.0
    if sos is not None:
        d = bandpass_filter_host(d, sos, taper_alpha=taper_alpha)
    out = d.astype(np.float32)
    return (out, k) if return_rank else out


def group_offsets(n_events, offsets=None):
    """`offsets` (G + 1,) int64 of a ragged batch of groups over `n_events` rows (None: one group), checked."""
    if offsets is None:
        return np.array([0, int(n_events)], dtype=np.int64)
    off = np.ascontiguousarray(np.asarray(offsets).astype(np.int64).reshape(-1))
    if off.size < 1 or off[0] != 0 or off[-1] != int(n_events) or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must ascend from 0 to the number of events ({int(n_events)}); got {off.tolist()}")
    return off


def svdwf_stack_host(x, offsets=None, *, expl_var=0.4, max_singular_values=5, wiener_filter_colsize=None, sos=None,
                     taper_alpha=0.01):
    """EventGroup.SVDWF_stack (BPMF/dataset.py:4313-4335) on plain arrays, for a ragged batch of groups: `x`
    (N, S, C, m) float32, group g = rows offsets[g] .. offsets[g + 1].  Every channel of every group goes through
    svdwf_host; the stack of a group is the float64 mean over its events of the float32 filtered values, divided by
    its SIGNED maximum over the samples (a maximum of 0 divides by 1), rounded to float32.  An empty group has a zero
    stack.  Returns (filtered (N, S, C, m) float32, stack (G, S, C, m) float32, n_singular (G, S, C) int32)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4:
        raise ValueError("svdwf_stack_host: x must be (N, S, C, m)")
    N, S, Cc, m = x.shape
    off = group_offsets(N, offsets)
    G = len(off) - 1
    filtered = np.zeros_like(x)
    stack = np.zeros((G, S, Cc, m), dtype=np.float32)
    rank = np.zeros((G, S, Cc), dtype=np.int32)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if a == b:
            continue
        for s in range(S):
            for c in range(Cc):
                filtered[a:b, s, c], rank[g, s, c] = svdwf_host(
                    x[a:b, s, c], expl_var, max_singular_values, wiener_filter_colsize, sos, taper_alpha,
                    return_rank=True)
        mean = filtered[a:b].astype(np.float64).mean(axis=0)
        norm = mean.max(axis=-1, keepdims=True)
        norm[norm == 0.0] = 1.0
        stack[g] = (mean / norm).astype(np.float32)
    return filtered, stack, rank


# ---- multi-band displacement spectra (BPMF/spectrum.py: Spectrum.compute_multi_band_spectrum :387-505,
# ---- compute_signal_to_noise_ratio :601-648) ----
# The reference runs three obspy operations on every trace and band.  obspy was not at hand when this was written: the
# three are RESTATED here from obspy's documented behaviour, and stay unverified against obspy itself until
# tools/diff_obspy_multiband.py (or tests/test_multiband_obspy_live.py) runs next to a real obspy:
#   tr.detrend("constant") / tr.detrend("linear")        = scipy.signal.detrend(data, type=...)
#   tr.taper(0.25, max_length=L, type="cosine")          = a half-Hann of w = min(int(0.25 npts), int(L sr)) samples on
#                                                          each side, 0.5 (1 - cos(pi i / w)), i < w
#   tr.filter("bandpass", corners=, zerophase=True)      = iirfilter -> zpk2sos -> sosfilt, forward and on the reversed
#                                                          output
MULTIBAND_MAX_SAMPLES = 16384
MULTIBAND_MAX_BANDS = 64
MULTIBAND_NYQUIST_MARGIN = 1e-6       # obspy turns a band whose upper corner is this close below Nyquist into a high-pass


def multiband_bands(frequency_bands):
    """The reference's `frequency_bands` -- a dict {name: [lo, hi]} in its order, or a (B, 2) array, in Hz -- as a
    (B, 2) float64 array.  Raises ValueError for anything else, for B outside 1 .. 64, and for a band with lo <= 0 or
    lo >= hi."""
    if isinstance(frequency_bands, dict):
        frequency_bands = [frequency_bands[k] for k in frequency_bands]
    try:
        bands = np.array(frequency_bands, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("multiband: frequency_bands must be a dict {name: [lo, hi]} or a (B, 2) array") from None
    if bands.ndim != 2 or bands.shape[1] != 2:
        raise ValueError(f"multiband: frequency_bands must be a dict {{name: [lo, hi]}} or a (B, 2) array; got the "
                         f"shape {bands.shape}")
    if not 1 <= len(bands) <= MULTIBAND_MAX_BANDS:
        raise ValueError(f"multiband: 1 .. {MULTIBAND_MAX_BANDS} frequency bands; got {len(bands)}")
    bad = ~((bands[:, 0] > 0) & (bands[:, 0] < bands[:, 1]) & np.isfinite(bands[:, 1]))
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"multiband: band {b} = [{bands[b, 0]}, {bands[b, 1]}] Hz; need 0 < lo < hi")
    return bands


def multiband_plan(n_samples, frequency_bands, sr, buffer_seconds, corners=4):
    """What a multi-band call works with, and its refusals.  Returns a dict: `bands` (B, 2) Hz; `taper` w =
    min(int(0.25 n), int(buffer_seconds sr)) and `buffer` = int(buffer_seconds sr) in samples, both int() as the
    reference and obspy take them; `skip` (B,) bool: hi >= sr / 2, the reference's `continue`; `sos` (B, corners, 6):
    butter_bandpass_sos of every band that is not skipped (a skipped band holds pass-through sections); `bandwidth`
    (B,) = hi - lo; `freq` (B,) float32 = 0.5 (lo + hi), skipped bands included.  Raises ValueError: bad bands
    (multiband_bands); corners outside 1 .. 8; buffer == 0 or n <= 2 buffer, where the reference's data[buf:-buf] is
    empty and it returns zeros; a band with (1 - 1e-6) sr / 2 < hi < sr / 2, which obspy silently turns into a
    high-pass (not restated here)."""
    n, sr = int(n_samples), float(sr)
    bands = multiband_bands(frequency_bands)
    corners = int(corners)
    if not 1 <= corners <= BANDPASS_MAX_SECTIONS:
        raise ValueError(f"multiband: corners must be 1 .. {BANDPASS_MAX_SECTIONS}; got {corners}")
    if not sr > 0 or not float(buffer_seconds) >= 0:
        raise ValueError(f"multiband: need sr > 0 and buffer_seconds >= 0; got {sr}, {buffer_seconds}")
    buf = int(buffer_seconds * sr)
    if buf == 0 or n <= 2 * buf:
        raise ValueError(f"multiband: windows of {n} samples with buffers of {buf}: the trimmed range data[buf:-buf] is "
                         "empty (the reference returns all zeros there); need buffer >= 1 sample and n > 2 buffer")
    w = min(int(0.25 * n), buf)
    nyq = sr / 2.0
    skip = bands[:, 1] >= nyq
    near = (bands[:, 1] > (1.0 - MULTIBAND_NYQUIST_MARGIN) * nyq) & ~skip
    if near.any():
        b = int(np.flatnonzero(near)[0])
        raise ValueError(f"multiband: band {b} ends at {bands[b, 1]} Hz, within 1e-6 below the Nyquist frequency "
                         f"{nyq} Hz: obspy silently turns such a band-pass into a high-pass, which is not served")
    sos = np.zeros((len(bands), corners, 6))
    sos[:, :, 0] = sos[:, :, 3] = 1.0
    for b, (lo, hi) in enumerate(bands):
        if not skip[b]:
            sos[b] = butter_bandpass_sos(corners, lo / nyq, hi / nyq)
    return {"bands": bands, "taper": w, "buffer": buf, "skip": skip, "sos": sos,
            "bandwidth": bands[:, 1] - bands[:, 0], "freq": (0.5 * (bands[:, 0] + bands[:, 1])).astype(np.float32)}


def multiband_prepare_host(windows, taper):
    """Steps 1-3 of the definition on (rows, n) float32 windows: float64 rows with the mean subtracted
    (v -= sum(v) / n), the least-squares line removed (with t_k = k - (n - 1) / 2: minus (sum(v t) / sum(t^2)) t_k +
    sum(v) / n, slope 0 where sum(t^2) = 0), and a half-Hann of `taper` samples, 0.5 (1 - cos(pi i / taper)), on each
    side (0: none).  The sums are exact (math.fsum), so that no summation order shows."""
    import math
    v = np.array(windows, dtype=np.float64)
    rows, n = v.shape
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    den = math.fsum(t * t)
    for r in range(rows):
        v[r] -= math.fsum(v[r]) / n
        slope = math.fsum(v[r] * t) / den if den > 0 else 0.0
        v[r] -= slope * t + math.fsum(v[r]) / n
    if taper:
        g = 0.5 * (1.0 - np.cos(np.pi * np.arange(taper, dtype=np.float64) / taper))
        v[:, :taper] *= g
        v[:, n - taper:] *= g[::-1]
    return v


def _sosfilt_bands(sos, x):
    """sosfilt_rows for several filters at once: `sos` (A, n_sections, 6), `x` (m, A, rows) time-major; element by
    element the same operations in the same order, so bit for bit sosfilt_rows(sos[a], x[:, a, :].T).T."""
    y = np.array(x, dtype=np.float64)
    m, A, rows = y.shape
    n_sec = sos.shape[1]
    z = np.zeros((n_sec, 2, A, rows))
    coef = [[np.ascontiguousarray(sos[:, s, j])[:, None] for j in range(6)] for s in range(n_sec)]
    for t in range(m):
        cur = y[t].copy()
        for s in range(n_sec):
            b0, b1, b2, _, a1, a2 = coef[s]
            new = b0 * cur + z[s, 0]
            z[s, 0] = (b1 * cur - a1 * new) + z[s, 1]
            z[s, 1] = b2 * cur - a2 * new
            cur = new
        y[t] = cur
    return y


def multiband_spectrum_host(windows, frequency_bands, *, sr, buffer_seconds, corners=4, multi_component=False):
    """The definition of the multi-band spectra: Spectrum.compute_multi_band_spectrum (BPMF/spectrum.py:387-505) on
    plain arrays, float64 throughout, NumPy only.  `windows` (..., n) float32, one trace each (noise, P or S window;
    (..., C, n) with `multi_component`).  Per window: multiband_prepare_host (detrend "constant", detrend "linear",
    the cosine taper of min(int(0.25 n), int(buffer_seconds sr)) samples); per band with hi < sr / 2 the Butterworth
    band-pass of `corners` corners (butter_bandpass_sos) forward from zero state and over the reversed result from
    zero state (as sosfilt_rows: SciPy's operation order); a = max |y[k]| over buf <= k < n - buf, buf =
    int(buffer_seconds sr), divided by hi - lo; a NaN in that range gives NaN.  A band with hi >= sr / 2 gives 0.
    `multi_component`: sqrt(sum over the components a^2), in component order.  Returns (spectra (..., B) float64,
    freq (B,) float32 = 0.5 (lo + hi)).  Refusals: multiband_plan.

    obspy's detrend, taper and filter are restated from their documented behaviour (see the section comment); the
    arithmetic around them is pinned to the reference in tests/test_multiband_host.py."""
    x = np.asarray(windows, dtype=np.float32)
    if x.ndim < (2 if multi_component else 1):
        raise ValueError("multiband_spectrum_host: windows must be (..., n), or (..., C, n) with multi_component")
    n = x.shape[-1]
    plan = multiband_plan(n, frequency_bands, sr, buffer_seconds, corners)
    buf, B = plan["buffer"], len(plan["bands"])
    lead = x.shape[:-1]
    out = np.zeros((int(np.prod(lead, dtype=np.int64)), B))
    live = np.flatnonzero(~plan["skip"])
    if out.shape[0] and len(live):
        v = multiband_prepare_host(x.reshape(-1, n), plan["taper"])
        y = _sosfilt_bands(plan["sos"][live], np.broadcast_to(v.T[:, None, :], (n, len(live), len(v))))
        y = _sosfilt_bands(plan["sos"][live], y[::-1])[::-1]
        out[:, live] = (np.max(np.abs(y[buf:n - buf]), axis=0) / plan["bandwidth"][live, None]).T
    out = out.reshape(lead + (B,))
    if multi_component:
        total = np.zeros(lead[:-1] + (B,))
        for c in range(lead[-1]):
            total += out[..., c, :] * out[..., c, :]
        out = np.sqrt(total)
    return out, plan["freq"]


def multiband_windows_host(data, starts, n_samples):
    """The windows a multi-band call works on: (windows (E, S, C, n_samples) float32, valid (E, S) bool).
    windows[e, s, c] = data[s, c, starts[e(, s)] : + n_samples] of the (S, C, N) day where that range lies wholly inside
    the day (valid); elsewhere zeros and valid = False -- the reference would go on with the shorter trace it managed
    to read, which is not served.  `starts` (E,) or (E, S) integers (picker_starts)."""
    data = np.asarray(data, dtype=np.float32)
    if data.ndim != 3:
        raise ValueError("multiband_windows_host: data must be (S, C, N)")
    S, C, N = data.shape
    n = int(n_samples)
    st = picker_starts(starts, S)
    valid = (st >= 0) & (st + n <= N)
    windows = _clipped_windows(data, np.broadcast_to(st[:, :, None], st.shape + (C,)), n)
    windows[~valid] = 0.0
    return windows, valid


def spectral_snr_host(signal, noise, noise_valid=None):
    """Spectrum.compute_signal_to_noise_ratio (BPMF/spectrum.py:601-648) on arrays of equal shape (..., B): 0 where
    signal and noise are both 0, |signal| / |noise| elsewhere (inf included), and 0 where the noise spectrum is missing:
    `noise_valid` (...) bool, the `valid` of the noise windows, broadcast over the trailing axes."""
    signal, noise = np.abs(np.asarray(signal, dtype=np.float64)), np.abs(np.asarray(noise, dtype=np.float64))
    if signal.shape != noise.shape:
        raise ValueError(f"spectral_snr_host: signal {signal.shape} and noise {noise.shape} differ in shape")
    snr = np.zeros(signal.shape)
    keep = ~((signal == 0.0) & (noise == 0.0))
    if noise_valid is not None:
        nv = np.asarray(noise_valid, dtype=bool)
        keep &= nv.reshape(nv.shape + (1,) * (signal.ndim - nv.ndim))
    with np.errstate(divide="ignore", invalid="ignore"):
        snr[keep] = signal[keep] / noise[keep]
    return snr


# ---- FFT-method displacement spectra (BPMF/spectrum.py: Spectrum.compute_spectrum :507-599, Spectrum.resample
# ---- :851-887; method "regular" of compute_moment_magnitude) ----
FFT_SPECTRUM_MIN_SAMPLES = 2
FFT_SPECTRUM_MAX_SAMPLES = 16384
FFT_SPECTRUM_MAX_TARGETS = 1024
FFT_SPECTRUM_EXACT, FFT_SPECTRUM_OUTSIDE = 1, 2        # bits of the plan's `flags`


def fft_spectrum_plan(n_samples, sr, frequencies=None, alpha=0.05, taper=None):
    """What an FFT-method call works with, and its refusals.  Returns a dict: `taper` (n,) float64 =
    scipy.signal.windows.tukey(n, alpha) (tukey_window, which equals it bit for bit for 0 <= alpha < 1), or the caller's
    (n,) `taper`; `delta` = 1.0 / sr; `freq` = np.fft.rfftfreq(n, d=delta) (K = n // 2 + 1 bins); `bins` (K_b,) int32,
    ascending: without `frequencies` every bin, with them the sorted unique j and j + 1 that np.interp uses for a
    target -- j the last bin with freq[j] <= f, kept inside 0 .. K - 2.  With `frequencies` (F,) also `frequencies`
    as float64; `pair` (F,) int32, the index of j in `bins` (that of j + 1 is one more); `dx` = f - freq[j] and `span`
    = freq[j + 1] - freq[j], float64; `exact`: f == freq[j], or f < freq[0], where np.interp returns fp[j]; `outside`:
    f >= 0.99 freq.max(), which the reference sets to 0; `flags` (F,) uint8 = exact | 2 outside.
    Raises ValueError: n outside 2 .. 16384; sr not a positive number; more than 1024 targets, none, or one that is not
    finite; alpha outside [0, 1); a `taper` that is not (n,)."""
    n = int(n_samples)
    if not FFT_SPECTRUM_MIN_SAMPLES <= n <= FFT_SPECTRUM_MAX_SAMPLES:
        raise ValueError(f"fft_spectrum: windows of {FFT_SPECTRUM_MIN_SAMPLES} .. {FFT_SPECTRUM_MAX_SAMPLES} samples; "
                         f"got {n}")
    sr = float(sr)
    if not (sr > 0 and np.isfinite(sr)):
        raise ValueError(f"fft_spectrum: need sr > 0; got {sr}")
    if taper is None:
        if not 0 <= float(alpha) < 1:
            raise ValueError(f"fft_spectrum: alpha must lie in [0, 1); got {alpha} (pass the window as taper=)")
        window = tukey_window(n, float(alpha))
    else:
        window = np.array(taper, dtype=np.float64)
        if window.shape != (n,):
            raise ValueError(f"fft_spectrum: taper must be ({n},); got the shape {window.shape}")
    delta = 1.0 / sr
    freq = np.fft.rfftfreq(n, d=delta)
    plan = {"taper": window, "delta": delta, "freq": freq}
    if frequencies is None:
        plan["bins"] = np.arange(len(freq), dtype=np.int32)
        return plan
    f = np.array(frequencies, dtype=np.float64)
    if f.ndim != 1 or not 1 <= len(f) <= FFT_SPECTRUM_MAX_TARGETS or not np.isfinite(f).all():
        raise ValueError(f"fft_spectrum: frequencies must be 1 .. {FFT_SPECTRUM_MAX_TARGETS} finite numbers in one "
                         f"dimension; got the shape {f.shape}")
    j = np.clip(np.searchsorted(freq, f, side="right") - 1, 0, len(freq) - 2)
    bins = np.unique(np.concatenate([j, j + 1]))
    plan.update(frequencies=f, bins=bins.astype(np.int32), pair=np.searchsorted(bins, j).astype(np.int32),
                dx=f - freq[j], span=freq[j + 1] - freq[j], exact=(f == freq[j]) | (f < freq[0]),
                outside=f >= 0.99 * freq.max())
    plan["flags"] = (plan["exact"] * FFT_SPECTRUM_EXACT + plan["outside"] * FFT_SPECTRUM_OUTSIDE).astype(np.uint8)
    return plan


def _two_prod(a, b):
    """a * b as the float64 product and what its rounding left out (Dekker's split; exact without an FMA)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


@functools.lru_cache(maxsize=8)
def _dft_twiddles(n):
    # sin and cos of a = pi t / (4 n) <= pi / 4, t = 0 .. n, from the angle as a float64 and what that leaves out:
    # q = t / (4 n) and pi each as a sum of two float64 (the remainder of the division exact), their product to
    # first order in the small parts (what is dropped is below 2^-100), then sin(hi + lo) = sin(hi) + lo cos(hi) and
    # cos(hi + lo) = cos(hi) - lo sin(hi): each value within 1.5 * 2^-53 with a libm good to one unit in the last place
    t = np.arange(n + 1, dtype=np.float64)
    d = 4.0 * n
    q = t / d
    p, e = _two_prod(q, np.full_like(q, d))
    q_lo = ((t - p) - e) / d
    pi_hi, pi_lo = 3.141592653589793, 1.2246467991473532e-16
    hi, e = _two_prod(q, np.full_like(q, pi_hi))
    lo = e + (pi_hi * q_lo + pi_lo * q)
    s, c = np.sin(hi), np.cos(hi)
    s, c = s + lo * c, c - lo * s
    # 2 pi m / n = (pi / 4) (o + rem / n): the octant o and what is left of it, in integers
    m = np.arange(n, dtype=np.int64)
    o, rem = np.divmod(8 * m, n)
    t = np.where(o % 2 == 0, rem, n - rem)
    cos = np.choose(o, [c[t], s[t], -s[t], -c[t], -c[t], -s[t], s[t], c[t]])
    sin = np.choose(o, [s[t], c[t], c[t], s[t], -s[t], -c[t], -c[t], -s[t]])
    table = np.stack([cos, -sin], axis=1) + 0.0                     # (no -0)
    table.setflags(write=False)
    return table


def dft_twiddles(n):
    """(n, 2) float64: cos(2 pi m / n) and -sin(2 pi m / n), m = 0 .. n - 1, every entry within 2^-52 of the true value
    for every n <= 16384: the argument is reduced to an octant in integers, and the angle left, at most pi / 4, goes
    into sin and cos as a float64 plus the remainder that the float64 leaves out.  (Read-only; cached.)"""
    n = int(n)
    if not 1 <= n <= FFT_SPECTRUM_MAX_SAMPLES:
        raise ValueError(f"dft_twiddles: 1 .. {FFT_SPECTRUM_MAX_SAMPLES} entries; got {n}")
    return _dft_twiddles(n)


def fft_spectrum_host(windows, *, sr, frequencies=None, alpha=0.05, taper=None, multi_component=False):
    """The definition of the FFT-method spectra: Spectrum.compute_spectrum (BPMF/spectrum.py:507-599) and
    Spectrum.resample (:851-887) on plain arrays, the reference's statements in the reference's order.  `windows`
    (E, S, C, n), float32 or float64 as given, one trace each.  Per trace np.fft.rfft(trace * taper) * delta, taper =
    tukey(n, alpha) or the caller's array, delta = 1 / sr.  Without `frequencies`: the complex spectrum (E, S, C, K),
    K = n // 2 + 1, or with `multi_component` sqrt(sum over the components |X_c|^2), summed in component order from 0,
    (E, S, K).  With `frequencies` (F,): np.interp(frequencies, freq, |spectrum|) with the targets at or beyond
    0.99 freq.max() set to 0: (E, S, C, F), or (E, S, F) float64.
    A trace that holds a NaN or an Inf is NaN at every bin (re and im) and at every target that is not set to 0; with
    `multi_component` so is its station.  This is the definition's own answer, whatever an FFT makes of such a trace.
    Returns (spectra, freq): freq = `frequencies` as float64, or np.fft.rfftfreq(n, d=delta).  Refusals:
    fft_spectrum_plan."""
    x = np.asarray(windows)
    if x.ndim != 4:
        raise ValueError("fft_spectrum_host: windows must be (E, S, C, n)")
    n = x.shape[-1]
    plan = fft_spectrum_plan(n, sr, frequencies, alpha, taper)
    spectrum = np.fft.rfft(x * plan["taper"]) * plan["delta"]
    bad = ~np.isfinite(x).all(axis=-1)
    spectrum[bad] = complex(np.nan, np.nan)
    if multi_component:
        total = np.zeros(x.shape[:2] + (spectrum.shape[-1],), dtype=np.float64)
        for c in range(x.shape[2]):
            total += np.abs(spectrum[:, :, c]) ** 2
        spectrum = np.sqrt(total)
    if frequencies is None:
        return spectrum, plan["freq"]
    modulus = np.abs(spectrum)
    out = np.empty(modulus.shape[:-1] + (len(plan["frequencies"]),), dtype=np.float64)
    for index in np.ndindex(out.shape[:-1]):
        out[index] = np.interp(plan["frequencies"], plan["freq"], modulus[index])
    out[..., plan["outside"]] = 0.0
    return out, plan["frequencies"]


def fft_windows_host(data, starts, n_samples):
    """The windows an FFT-method call works on, and `valid`: multiband_windows_host, which fits as it is."""
    return multiband_windows_host(data, starts, n_samples)


# ---- Propagation corrections, network-average spectra and the approximate moment magnitude (BPMF/spectrum.py:
# ---- set_Q_model :37-63, compute_correction_factor :97-198, correct_geometrical_spreading :200-227,
# ---- correct_attenuation :229-256 with update_attenuation_factor :78-95, compute_network_average_spectrum :258-386,
# ---- _snr_based_weights :1290-1338, approximate_moment_magnitude :1341-1496) ----
SOURCE_SPECTRA_MAX_CHANNELS = 256          # S * C of one event
SOURCE_SPECTRA_MAX_FREQUENCIES = 1024      # as fft_spectra
SOURCE_SPECTRA_MAX_AVERAGING_BANDS = 8
RADIATION_P, RADIATION_S = np.sqrt(4.0 / 15.0), np.sqrt(2.0 / 5.0)
MEDIUM_KEYS = ("rho_source_kgm3", "rho_receiver_kgm3", "vp_source_ms", "vp_receiver_ms", "vs_source_ms",
               "vs_receiver_ms", "Q_1HZ", "attenuation_n")


def geometry_constants(medium, radiation_p=RADIATION_P, radiation_s=RADIATION_S):
    """(c_p, c_s): 4 pi sqrt(rho_receiver) sqrt(rho_source) sqrt(v_receiver) v_source^2.5 of compute_correction_factor,
    multiplied in the reference's order, for P and S; the geometrical factor of a station at `dist` km is
    c * (1000 * dist) / radiation."""
    def constant(v_source, v_receiver):
        return (4.0 * np.pi * np.sqrt(medium["rho_receiver_kgm3"]) * np.sqrt(medium["rho_source_kgm3"])
                * np.sqrt(v_receiver) * v_source ** (5.0 / 2.0))
    return (constant(medium["vp_source_ms"], medium["vp_receiver_ms"]),
            constant(medium["vs_source_ms"], medium["vs_receiver_ms"]))


def attenuation_plan(frequencies, medium, q_phase_prefactor=None, attenuation="reference"):
    """Which travel time and which Q row a phase's attenuation factor exp(((pi tt) f) / Q_row) takes: returns
    (tt_phase, q_rows) with tt_phase = ("s", "s") or ("p", "s") for (P, S) and q_rows (2, F).  Q(f) = Q_1HZ f^n (the
    reference's interp1d of it at its own frequencies is the identity).  attenuation="reference" is what
    correct_attenuation does through update_attenuation_factor: BOTH phases take the S travel time, the P factor
    divides by Q * prefactor["s"] and the S factor by Q * prefactor["p"].  attenuation="physical" pairs tt_p with
    Q * prefactor["p"] and tt_s with Q * prefactor["s"]."""
    if attenuation not in ("reference", "physical"):
        raise ValueError(f"attenuation must be 'reference' or 'physical'; got {attenuation!r}")
    f = np.asarray(frequencies, dtype=np.float64)
    if f.ndim != 1 or not 1 <= len(f) <= SOURCE_SPECTRA_MAX_FREQUENCIES or not np.isfinite(f).all():
        raise ValueError(f"frequencies must be 1 .. {SOURCE_SPECTRA_MAX_FREQUENCIES} finite numbers in one dimension")
    prefactor = dict(q_phase_prefactor or {})
    Q = medium["Q_1HZ"] * np.power(f, medium["attenuation_n"])
    q_p, q_s = Q * prefactor.get("p", 1.0), Q * prefactor.get("s", 1.0)
    if attenuation == "reference":
        return ("s", "s"), np.stack([q_s, q_p])
    return ("p", "s"), np.stack([q_p, q_s])


def propagation_factors_host(frequencies, source_receiver_dist_km, tt_p_sec, tt_s_sec, medium, q_phase_prefactor=None,
                             attenuation="reference", radiation_p=RADIATION_P, radiation_s=RADIATION_S):
    """The factors that correct_geometrical_spreading and correct_attenuation multiply a spectrum by, in that order,
    each with its own rounding: `geometry` (E, S, 2) and `attenuation` (E, S, 2, F), phase 0 = P, 1 = S.
    geometry = c * (1000 * dist) / radiation (geometry_constants); attenuation = exp(((pi * tt) * f) / Q_row)
    (attenuation_plan, where the reference's pairing of travel times and Q rows is stated)."""
    dist = np.asarray(source_receiver_dist_km, dtype=np.float64)
    tt = {"p": np.asarray(tt_p_sec, dtype=np.float64), "s": np.asarray(tt_s_sec, dtype=np.float64)}
    if dist.ndim != 2 or tt["p"].shape != dist.shape or tt["s"].shape != dist.shape:
        raise ValueError("propagation_factors_host: distances and travel times must be (E, S) and equal in shape")
    f = np.asarray(frequencies, dtype=np.float64)
    which, q_rows = attenuation_plan(f, medium, q_phase_prefactor, attenuation)
    c = geometry_constants(medium)
    radiation = (radiation_p, radiation_s)
    geometry = np.stack([c[k] * (1000.0 * dist) / radiation[k] for k in range(2)], axis=-1)
    with np.errstate(all="ignore"):
        att = np.stack([np.exp(np.pi * tt[which[k]][..., None] * f / q_rows[k]) for k in range(2)], axis=2)
    return geometry, att


def _source_channels(spectra, n_stations):
    """(E, S, F) or (E, S, C, F) -> ((E, S * C, F) view, C)."""
    x = np.asarray(spectra, dtype=np.float64)
    if x.ndim not in (3, 4) or x.shape[1] != n_stations:
        raise ValueError(f"spectra must be (E, S, F) or (E, S, C, F) with S = {n_stations}; got {x.shape}")
    C = 1 if x.ndim == 3 else x.shape[2]
    return x.reshape(x.shape[0], n_stations * C, x.shape[-1]), C


def network_average_spectrum_host(spectra, snr, present, dist_err_pct, *, snr_threshold, average_log=True,
                                  min_num_valid_channels_per_freq_bin=0, max_relative_distance_err_pct=25.0,
                                  reduce="mean"):
    """Spectrum.compute_network_average_spectrum (:258-386) for E events at once, without np.ma: `spectra`, `snr`
    (E, S, F) or (E, S, C, F) float64 (a channel is (s, c), in that order), `present` (E, S) bool (False: the station
    has no spectrum, its window was not valid), `dist_err_pct` (E, S) = 100 sqrt(hmax^2 + vmax^2) / dist.

    A station is `used` if present and not dist_err_pct > max.  Per bin over the used channels: masked where
    snr < snr_threshold (a NaN SNR is not masked); num_valid counts the unmasked, BEFORE the two rules that follow:
    a bin with num_valid < min_num is masked in every channel, and with average_log np.ma.log10 also masks values
    <= 0 and every value whose log10 is not finite (NaN and inf: np.ma masks a non-finite result of a domained
    function, so a NaN reaches an average only with average_log=False).  Mean: the channels' values (0 where masked) added in channel order, times 1.0, divided by the
    count; median: NaN if an unmasked value is NaN, else the middle value or the half-sum of the two middle values;
    with average_log the average is exp(that * log(10)) of the log10 values.  std is np.ma.std, ddof = 0, about the
    MEAN in both cases: sqrt(sum((v - mean)^2) / count).  np.ma's division masks a quotient that is not finite: so a
    mean that is NaN or infinite is masked (a median is not: it can be an unmasked NaN), and std is then 0, unmasked
    (np.ma.var sums deviations that the masked mean has masked, and sets its own mask from the counts alone).  A bin without an unmasked channel is masked; an event without a used station is masked
    everywhere.  Returns a dict: `average`, `std` (E, F) float64, NaN where `mask`
    (E, F) bool; `num_valid` (E, F) int32; `used` (E, S) bool."""
    if reduce not in ("mean", "median"):
        raise ValueError(f"reduce must be 'mean' or 'median'; got {reduce!r}")
    present = np.asarray(present, dtype=bool)
    if present.ndim != 2:
        raise ValueError("present must be (E, S)")
    E, S = present.shape
    x, C = _source_channels(spectra, S)
    r, C2 = _source_channels(snr, S)
    err = np.asarray(dist_err_pct, dtype=np.float64)
    if r.shape != x.shape or err.shape != (E, S) or x.shape[0] != E:
        raise ValueError("spectra and snr must be equal in shape, dist_err_pct (E, S) as present")
    F = x.shape[-1]
    used = present & ~(err > max_relative_distance_err_pct)
    average, std = np.full((E, F), np.nan), np.full((E, F), np.nan)
    mask, num_valid = np.ones((E, F), dtype=bool), np.zeros((E, F), dtype=np.int32)
    log10 = np.log(10.0)
    with np.errstate(all="ignore"):
        for e in range(E):
            ch = np.flatnonzero(np.repeat(used[e], C))
            if len(ch) == 0:
                continue
            v, m = x[e, ch], r[e, ch] < snr_threshold
            num_valid[e] = (~m).sum(axis=0)
            m = m | (num_valid[e] < min_num_valid_channels_per_freq_bin)[None, :]
            if average_log:
                m = m | (v <= 0.0) | ~np.isfinite(np.log10(v))
                v = np.log10(v)
            count = (~m).sum(axis=0)
            filled = np.where(m, 0.0, v)
            mean = np.add.reduce(filled, axis=0) * 1.0 / count
            if reduce == "mean":
                centre = mean
            else:
                ordered = np.sort(np.where(m, np.inf, v), axis=0)           # NaN last, masked (inf) before it
                hi = np.minimum(count // 2, len(ch) - 1)
                lo = np.where(count % 2 == 1, hi, np.maximum(hi - 1, 0))
                centre = (np.take_along_axis(ordered, lo[None], 0)[0] + np.take_along_axis(ordered, hi[None], 0)[0]) / 2.0
                centre[(np.isnan(v) & ~m).any(axis=0)] = np.nan
            d = np.where(m, 0.0, v - mean)
            variance = np.add.reduce(d * d, axis=0) / count
            value = np.exp(centre * log10) if average_log else centre
            mask[e] = (count == 0) | (~np.isfinite(mean) if reduce == "mean" else False)
            average[e] = np.where(mask[e], np.nan, value)
            std[e] = np.where((count == 0) | ~np.isfinite(variance), np.nan, np.sqrt(variance))
            std[e][(count > 0) & ~np.isfinite(mean)] = 0.0
    return {"average": average, "mask": mask, "std": std, "num_valid": num_valid, "used": used}


def snr_based_weights_host(snr, snr_threshold, weight_max=3.0, max_num_bad_measurements=6):
    """_snr_based_weights (:1290-1338) on a float32 vector: min(snr, 1.001 threshold, weight_max), all in float32;
    with at least max_num_bad_measurements values >= threshold every value < threshold gets 0, otherwise all but the
    max_num_bad_measurements largest get 0.  Equal values are ordered by index: of a tied group across the cut, those
    of the lowest indices get 0.  The reference's np.argsort (quicksort) leaves their order open, and from 17 values
    on does not keep index order, so this rule is the definition's own; the device is held to it on non-zero ties
    that straddle the cut at 9, 20 and 40 channels (tests/source_spectra_cases.py: snr_ties_*)."""
    snr = np.asarray(snr, dtype=np.float32)
    thr = np.float32(snr_threshold)
    weights = np.minimum(np.minimum(snr, np.float32(1.001 * snr_threshold)), np.float32(weight_max))
    if np.sum(snr >= thr) >= max_num_bad_measurements:
        weights[snr < thr] = 0.0
    else:
        order = np.argsort(snr, kind="stable")
        weights[order[:len(order) - max_num_bad_measurements if len(order) > max_num_bad_measurements else 0]] = 0.0
    return weights


def _skipna_sum(values):
    """pandas' Series.sum: NaN counts as 0, then NumPy's sum of the contiguous row."""
    return np.where(np.isnan(values), 0.0, values).sum()


def approximate_moment_magnitude_host(corrected, snr, present, frequencies, epicentral_dist_km, *, snr_threshold=10.0,
                                      num_averaging_bands=1, low_snr_freq_min_hz=2.0,
                                      magnitude_log_moment_scaling=2.0 / 3.0, weight_max=3.0,
                                      max_num_bad_measurements=6):
    """approximate_moment_magnitude (:1341-1496) of one phase for E events, dtypes included.  `corrected`, `snr`
    (E, S, F) or (E, S, C, F) float64; `present` (E, S) bool; `frequencies` (F,); `epicentral_dist_km` (E, S).  The
    reference indexes the distances by spectrum id, so its code runs only with multi_component_spectrum=True; here a
    channel (s, c) takes the distance of its station s.

    Per channel of a present station: the valid bands are those with snr > snr_threshold (strict); with k > 0 of them
    the measurement is the value at the lowest one, or the median of the lowest min(k, num_averaging_bands) (in the
    order of `frequencies`, which must ascend), and its SNR is snr_threshold; with none, over the bands with
    frequency > low_snr_freq_min_hz, NaN terms counting as 0: 10 ** (sum(snr log10(value)) / sum(snr)) and
    sum(snr snr) / sum(snr), the sum replaced by 1.0 where it is 0 (so an empty selection gives 1 and 0, where the
    reference's unused argmax would raise).  The SNR is rounded to float32 and set to 0 where the measurement is 0.
    Weights: snr_based_weights_host, times (rounded to float32 from the float64 product) the reciprocal of the
    epicentral distance clipped to the 25th and 75th np.percentile (linear) of ALL S stations of the event.
    log10_M0 = sum(log10(measurement) * weight over weight > 0) in float64 / the float32 sum of the weights, both in
    NumPy's order over the present channels; Mw* = scaling * (log10_M0 - 9.1).
    Returns a dict: `Mw_star`, `log10_M0` (E,) float64 (NaN without a positive weight); `measured_disp` (E, S * C)
    float64 (NaN for an absent station); `weights`, `measurement_snr` (E, S * C) float32 (0 for an absent station)."""
    present = np.asarray(present, dtype=bool)
    E, S = present.shape
    x, C = _source_channels(corrected, S)
    r, _ = _source_channels(snr, S)
    f = np.asarray(frequencies, dtype=np.float64)
    epi = np.asarray(epicentral_dist_km, dtype=np.float64)
    nab = int(num_averaging_bands)
    if r.shape != x.shape or f.shape != (x.shape[-1],) or epi.shape != (E, S):
        raise ValueError("corrected and snr must be equal in shape, frequencies (F,), epicentral_dist_km (E, S)")
    if not 1 <= nab <= SOURCE_SPECTRA_MAX_AVERAGING_BANDS:
        raise ValueError(f"num_averaging_bands must be 1 .. {SOURCE_SPECTRA_MAX_AVERAGING_BANDS}; got {nab}")
    if np.any(np.diff(f) <= 0):
        raise ValueError("frequencies must ascend")
    NC = S * C
    high = f > low_snr_freq_min_hz
    measured = np.full((E, NC), np.nan)
    msnr = np.zeros((E, NC), dtype=np.float32)
    weights = np.zeros((E, NC), dtype=np.float32)
    log10_m0 = np.full(E, np.nan)
    with np.errstate(all="ignore"):
        for e in range(E):
            ch = np.flatnonzero(np.repeat(present[e], C))
            if len(ch) == 0:
                continue
            disp, m32 = np.zeros(len(ch)), np.zeros(len(ch), dtype=np.float32)
            for j, c in enumerate(ch):
                valid = np.flatnonzero(r[e, c] > snr_threshold)
                if len(valid):
                    chosen = x[e, c, valid[:min(len(valid), nab)]]
                    disp[j] = np.median(chosen) if len(chosen) > 1 else chosen[0]
                    m32[j] = snr_threshold
                else:
                    w_, p_ = r[e, c, high], x[e, c, high]
                    total = _skipna_sum(w_)
                    total = 1.0 if total == 0.0 else total
                    disp[j] = 10.0 ** (_skipna_sum(w_ * np.log10(p_)) / total)
                    m32[j] = _skipna_sum(w_ * w_) / total
            m32[disp == 0.0] = 0.0
            w = snr_based_weights_host(m32, snr_threshold, weight_max, max_num_bad_measurements)
            wd = 1.0 / np.clip(epi[e], a_min=np.percentile(epi[e], 25.0), a_max=np.percentile(epi[e], 75.0))
            w *= np.repeat(wd, C)[ch]
            peaks = np.zeros(len(ch))
            peaks[w > 0.0] = np.log10(disp[w > 0.0]) * w[w > 0.0]
            log10_m0[e] = peaks.sum() / w.sum()
            measured[e, ch], msnr[e, ch], weights[e, ch] = disp, m32, w
    return {"Mw_star": magnitude_log_moment_scaling * (log10_m0 - 9.1), "log10_M0": log10_m0, "measured_disp": measured,
            "weights": weights, "measurement_snr": msnr}


def source_spectra_host(signal, noise, present, noise_present, dist_km, tt_sec, location_err_km, frequencies, q_row,
                        geometry_constant, radiation, **average_options):
    """Stages 1-3 of one phase as the device call chains them: spectral_snr_host, the two corrections (the spectrum
    times the geometrical factor, rounded, times the attenuation factor) and network_average_spectrum_host with
    dist_err_pct = 100 * (location_err / dist).  A channel of an absent station has corrected = snr = 0.  `tt_sec` and
    `q_row` are the travel time and the (F,) Q row that attenuation_plan names for the phase.  Returns the dict of
    network_average_spectrum_host with `corrected` and `snr` (shaped as `signal`) added."""
    signal = np.asarray(signal, dtype=np.float64)
    present = np.asarray(present, dtype=bool)
    dist, tt = np.asarray(dist_km, dtype=np.float64), np.asarray(tt_sec, dtype=np.float64)
    f, q = np.asarray(frequencies, dtype=np.float64), np.asarray(q_row, dtype=np.float64)
    wide = (slice(None), slice(None)) + (None,) * (signal.ndim - 2)
    snr = spectral_snr_host(signal, noise, noise_present)
    with np.errstate(all="ignore"):
        geometry = geometry_constant * (1000.0 * dist) / radiation
        att = np.exp(np.pi * tt[..., None] * f / q)
        corrected = signal * geometry[wide]
        corrected = corrected * (att if signal.ndim == 3 else att[:, :, None, :])
        err_pct = 100.0 * (np.asarray(location_err_km, dtype=np.float64)[:, None] / dist)
    corrected[~present] = 0.0
    snr[~present] = 0.0
    out = network_average_spectrum_host(corrected, snr, present, err_pct, **average_options)
    out.update(corrected=corrected, snr=snr)
    return out


# ---- Spectrum.fit_average_spectrum :729-849 (log=True), the gates and the P-S average of compute_moment_magnitude
# :1895-1990, Spectrum.resample :851-887 ----
# The constants of the fit's operational definition; include/bpmf_hip.h holds the same numbers as BPMF_FIT_*
# (tests/test_spectral_fit_definition.py compares the two).
FIT_SCAN_POINTS = 1024                     # G: log-spaced corner frequencies over the closed interval
FIT_ZOOM_ROUNDS = 2
FIT_ZOOM_POINTS = 64                       # one per lane
FIT_NEWTON_STEPS = 4
FIT_BOUND_FACTOR = 1.0e3                   # fc0 / 1e3 .. fc0 * 1e3
FIT_MODELS = {"brune": 2.0, "boatwright": 4.0}          # n of g = (2 / n) log10(1 + (f / fc)^n)
FIT_REASONS = ("fitted", "all bins masked", "too few valid bins", "too few valid bins below fc", "fc at a bound",
               "a value that is not finite")
FIT_KEYS = ("M0", "fc", "Mw", "M0_err", "fc_err", "cost", "stress_drop_pa")
FIT_LOG_OF_10 = 2.302585092994046          # np.log(10.0)
CRACK_CONSTANT = {"p": 2.23, "s": 1.47}
CRACK_VR_M_PER_S = 0.9 * 3500.0            # vr_vs_ratio * vs_m_per_s, the reference's defaults


def moment_to_magnitude(M0):
    """BPMF/spectrum.py:1201-1203."""
    return 2.0 / 3.0 * (np.log10(M0) - 9.1)


def magnitude_to_moment(Mw):
    """BPMF/spectrum.py:1196-1198."""
    return 10.0 ** (3.0 / 2.0 * Mw + 9.1)


def fc_circular_crack(Mw, stress_drop_Pa=1.0e6, phase="p"):
    """BPMF/spectrum.py:1206-1246 with the reference's velocity defaults."""
    crack_radius = np.power((7.0 / 16.0) * (magnitude_to_moment(Mw) / stress_drop_Pa), 1.0 / 3.0)
    return (CRACK_CONSTANT[phase] * CRACK_VR_M_PER_S) / (2.0 * np.pi * crack_radius)


def stress_drop_circular_crack(Mw, fc, phase="p"):
    """BPMF/spectrum.py:1249-1287 with the reference's velocity defaults."""
    crack_radius = CRACK_CONSTANT[phase] * CRACK_VR_M_PER_S / (2.0 * np.pi * fc)
    return 7.0 / 16.0 * magnitude_to_moment(Mw) / crack_radius**3


def _ordered_sum(terms):
    """The sum of the last axis, one term after the other from the first (what a plain loop on the device does)."""
    return np.add.accumulate(terms, axis=-1)[..., -1]


def fit_profile_cost(u, ln_x, y, w2, n):
    """The profile cost P(u) = 1/2 sum w^2 (y + g - a)^2 and a(u) = sum w^2 (y + g) / sum w^2 at every u of a (K,)
    array, with g = (2 / n) log10(1 + exp(n (ln x - u))) and every sum in bin order.  Returns (P, a), each (K,)."""
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    with np.errstate(all="ignore"):
        g = (2.0 / n) * np.log10(1.0 + np.exp(n * (ln_x[None, :] - u[:, None])))
        z = y[None, :] + g
        a = _ordered_sum(w2[None, :] * z) / _ordered_sum(w2)
        rho = z - a[:, None]
        return 0.5 * _ordered_sum(w2[None, :] * rho * rho), a


def fit_profile_derivatives(u, ln_x, y, w2, n):
    """At one u: P'(u) = sum w^2 rho (g' - a'), P''(u) = sum w^2 (g' - a')^2 + sum w^2 rho g'', the centred second
    moment D = sum w^2 (g' - a')^2 and the plain one sum w^2 g'^2, with t = 1 / (1 + exp(-n (ln x - u))),
    g' = dg/du = -(2 / ln 10) t and g'' = (2 n / ln 10) t (1 - t).  Sums in bin order."""
    with np.errstate(all="ignore"):
        d = ln_x - u
        g = (2.0 / n) * np.log10(1.0 + np.exp(n * d))
        t = 1.0 / (1.0 + np.exp(-(n * d)))
        g1 = -(2.0 / FIT_LOG_OF_10) * t
        g2 = (2.0 * n / FIT_LOG_OF_10) * (t * (1.0 - t))
        sw = _ordered_sum(w2)
        z = y + g
        rho = z - _ordered_sum(w2 * z) / sw
        c1 = g1 - _ordered_sum(w2 * g1) / sw
        centred = _ordered_sum(w2 * c1 * c1)
        return (_ordered_sum(w2 * rho * c1), centred + _ordered_sum(w2 * rho * g2), centred,
                _ordered_sum(w2 * g1 * g1))


def _fit_lowest(cost):
    """The index of the lowest cost, ties to the lowest index; a NaN counts as +inf."""
    return int(np.argmin(np.where(np.isnan(cost), np.inf, cost)))


def _fit_grid(lo, hi, count):
    """`count` points from lo to hi, both ends exact: lo + i ((hi - lo) / (count - 1)), the last one hi itself."""
    u = lo + np.arange(count, dtype=np.float64) * ((hi - lo) / (count - 1))
    u[-1] = hi
    return u


def fit_minimise(ln_x, y, w2, n, lo, hi):
    """argmin of the profile cost on the closed interval [lo, hi] as the kernel finds it: FIT_SCAN_POINTS evenly spaced
    u, the lowest cost (ties to the lowest index), FIT_ZOOM_ROUNDS rounds of FIT_ZOOM_POINTS points on the bracket of
    its two neighbours, then FIT_NEWTON_STEPS Newton steps u - P' / P'' (taken where P'' > 0 and the step is finite)
    clamped to the last bracket.  Returns u*."""
    a, b, count = lo, hi, FIT_SCAN_POINTS
    for _ in range(1 + FIT_ZOOM_ROUNDS):
        u = _fit_grid(a, b, count)
        i = _fit_lowest(fit_profile_cost(u, ln_x, y, w2, n)[0])
        a, b, best = u[max(i - 1, 0)], u[min(i + 1, count - 1)], u[i]
        count = FIT_ZOOM_POINTS
    u = best
    for _ in range(FIT_NEWTON_STEPS):
        p1, p2 = fit_profile_derivatives(u, ln_x, y, w2, n)[:2]
        with np.errstate(all="ignore"):
            step = p1 / p2
        if p2 > 0.0 and step - step == 0.0:
            u = min(max(u - step, a), b)
    return u


def fit_weights(num_valid, weighted):
    """(E, F) weights of the fit: sigmoid((num_valid - mean) / mean) with the mean over ALL F bins of the event
    (BPMF/spectrum.py:796-799), or 1.  curve_fit's sigma = 1 / w multiplies the residuals by w."""
    nv = np.asarray(num_valid, dtype=np.float64)
    if not weighted:
        return np.ones_like(nv)
    with np.errstate(all="ignore"):
        mean = _ordered_sum(nv) / nv.shape[-1]
        return 1.0 / (1.0 + np.exp(-((nv - mean[..., None]) / mean[..., None])))


def fit_source_spectra_host(average, mask, num_valid, frequencies, phase, *, model="brune", weighted=False,
                            min_fraction_valid_points=0.5, min_fraction_valid_points_below_fc=0.1):
    """Spectrum.fit_average_spectrum (BPMF/spectrum.py:729-849, log=True) for E events, by DEFINITION the exact weighted
    least-squares minimum rather than where SciPy's curve_fit stops: `average`, `mask`, `num_valid` (E, F) as
    network_average_spectrum_host returns them, `frequencies` (F,) positive and ascending, `phase` "p" or "s" (it
    enters the stress drop only: the reference's first guess of fc is the P one for both phases).

    Per event: no unmasked bin -> reason 1; valid / F < min_fraction_valid_points -> reason 2.  Else y = log10(average),
    x = frequencies at the M unmasked bins, w = fit_weights; Omega_0's first guess is the first unmasked value,
    fc0 = fc_circular_crack(moment_to_magnitude(Omega_0)).  The model is m(f) = a - g(f / fc), a = log10 Omega_0,
    g = log10(1 + r^2) (Brune) or 0.5 log10(1 + r^4) (Boatwright).  a is linear, so with u = ln fc the problem is
    u* = argmin P(u) (fit_profile_cost) on [ln(fc0 / 1e3), ln(fc0 1e3)], found by fit_minimise.  The upper end is the
    reference's bound; the reference's lower bound is fc = 0, where P tends to a constant and no minimum is attained,
    so the symmetric lower end is a departure.  u* at either end -> at_bound, reason 4 (values reported).

    Covariance, exact (not SciPy's SVD cut, which in one fit of six drops the Omega_0 column and leaves
    M0_err ~ 1e-31 M0: that artefact is not reproduced): J = w [1 / (Omega_0 ln 10), -dg/dfc], pcov = (2 P / (M - 2))
    (J^T J)^-1, in the coordinates (a, u) where J = w [1, -g'], so that pcov_00 = (Omega_0 ln 10)^2 s^2 sum w^2 g'^2 /
    (sum w^2 D) and pcov_11 = fc^2 s^2 / D with D the centred moment of g'.  M <= 2: inf, SciPy's rule.
    sum(x < fc) / F < min_fraction_valid_points_below_fc -> reason 3 (values reported).  A y, w, M0, fc, cost, Mw or
    stress drop that is not finite -> reason 5, NaN outputs (the two errors may be inf).  Precedence 1, 2, 5, 4, 3.

    Returns a dict of (E,) arrays: FIT_KEYS float64 (NaN where nothing was fitted), `n_valid` int32, `success`
    (reason 0), `at_bound` bool, `reason` uint8 (FIT_REASONS)."""
    if model not in FIT_MODELS:
        raise ValueError(f"fit_source_spectra_host: model must be one of {sorted(FIT_MODELS)}; got {model!r}")
    if phase not in CRACK_CONSTANT:
        raise ValueError(f"fit_source_spectra_host: phase must be 'p' or 's'; got {phase!r}")
    n = FIT_MODELS[model]
    average, mask = np.asarray(average, dtype=np.float64), np.asarray(mask, dtype=bool)
    f = np.asarray(frequencies, dtype=np.float64)
    E, F = average.shape
    weights = fit_weights(num_valid, weighted)
    out = {k: np.full(E, np.nan) for k in FIT_KEYS}
    out.update(n_valid=np.zeros(E, np.int32), success=np.zeros(E, bool), at_bound=np.zeros(E, bool),
               reason=np.zeros(E, np.uint8))
    with np.errstate(all="ignore"):
        for e in range(E):
            keep = ~mask[e]
            M = int(keep.sum())
            out["n_valid"][e] = M
            if M == 0:
                out["reason"][e] = 1
                continue
            if M / float(F) < min_fraction_valid_points:
                out["reason"][e] = 2
                continue
            y, x, w = np.log10(average[e][keep]), f[keep], weights[e][keep]
            if not (np.isfinite(y).all() and np.isfinite(w).all()):
                out["reason"][e] = 5
                continue
            w2, ln_x = w * w, np.log(x)
            fc0 = fc_circular_crack(moment_to_magnitude(average[e][keep][0]))
            lo, hi = np.log(fc0 / FIT_BOUND_FACTOR), np.log(fc0 * FIT_BOUND_FACTOR)
            if not (np.isfinite(lo) and np.isfinite(hi)):
                out["reason"][e] = 5
                continue
            u = fit_minimise(ln_x, y, w2, n, lo, hi)
            cost, a = (v[0] for v in fit_profile_cost(u, ln_x, y, w2, n))
            _, _, centred, plain = fit_profile_derivatives(u, ln_x, y, w2, n)
            M0, fc = 10.0 ** a, np.exp(u)
            Mw = moment_to_magnitude(M0)
            stress = stress_drop_circular_crack(Mw, fc, phase)
            if not np.isfinite([M0, fc, cost, Mw, stress]).all():
                out["reason"][e] = 5
                continue
            if M > 2:
                s2 = 2.0 * cost / (M - 2)
                cov_a, cov_u = s2 * plain / (_ordered_sum(w2) * centred), s2 / centred
            else:
                cov_a = cov_u = np.inf
            out["M0"][e], out["fc"][e], out["Mw"][e], out["cost"][e], out["stress_drop_pa"][e] = M0, fc, Mw, cost, stress
            out["M0_err"][e] = (M0 * FIT_LOG_OF_10) * np.sqrt(cov_a)
            out["fc_err"][e] = fc * np.sqrt(cov_u)
            out["at_bound"][e] = u == lo or u == hi
            if out["at_bound"][e]:
                out["reason"][e] = 4
            elif int((x < fc).sum()) / float(F) < min_fraction_valid_points_below_fc:
                out["reason"][e] = 3
    out["success"] = out["reason"] == 0
    return out


def moment_magnitudes_host(fit_p=None, fit_s=None, *, max_rel_m0_err_pct=33.0, max_rel_fc_err_pct=33.0):
    """The acceptance tests and the P-S average of compute_moment_magnitude (BPMF/spectrum.py:1907-1946, :1965-1990)
    on the dicts of fit_source_spectra_host: a phase is accepted where its fit succeeded and NOT (100 M0_err / M0 >
    max_rel_m0_err_pct or fc < 0 or 100 fc_err / fc > max_rel_fc_err_pct); Mw is the sum of the accepted phases' Mw
    (P first) divided by their number, Mw_err that of 2 / 3 * M0_err / M0; NaN where no phase was accepted.  The
    reference computes a stress-drop gate and then overrides it to True (:1937-1940); it stays overridden here.
    Returns {"Mw", "Mw_err" (E,) float64, "accepted": {phase: (E,) bool}}."""
    given = [(ph, fit) for ph, fit in (("p", fit_p), ("s", fit_s)) if fit is not None]
    if not given:
        raise ValueError("moment_magnitudes_host: give the fit of at least one phase")
    E = len(given[0][1]["M0"])
    total, total_err, norm, accepted = np.zeros(E), np.zeros(E), np.zeros(E), {}
    with np.errstate(all="ignore"):
        for ph, fit in given:
            M0, fc = np.asarray(fit["M0"], dtype=np.float64), np.asarray(fit["fc"], dtype=np.float64)
            rel_m0 = 100.0 * np.asarray(fit["M0_err"], dtype=np.float64) / M0
            rel_fc = 100.0 * np.asarray(fit["fc_err"], dtype=np.float64) / fc
            ok = np.asarray(fit["success"], dtype=bool) & ~((rel_m0 > max_rel_m0_err_pct) | (fc < 0.0) |
                                                             (rel_fc > max_rel_fc_err_pct))
            accepted[ph] = ok
            total = total + np.where(ok, np.asarray(fit["Mw"], dtype=np.float64), 0.0)
            total_err = total_err + np.where(ok, 2.0 / 3.0 * np.asarray(fit["M0_err"], dtype=np.float64) / M0, 0.0)
            norm = norm + ok
        some = norm > 0
        return {"Mw": np.where(some, total / norm, np.nan), "Mw_err": np.where(some, total_err / norm, np.nan),
                "accepted": accepted}


def resample_plan(frequencies_in, frequencies_out):
    """What np.interp needs per target of Spectrum.resample (BPMF/spectrum.py:851-887), from the frequencies alone:
    `pair` j with xp[j] <= x < xp[j + 1] (clipped to 0 .. B - 2), `below` (x < xp[0]: fp[0]), `above` (x >= xp[-1]:
    fp[-1], before the zeroing), `on` (x == xp[j]: fp[j]) and `outside` (x >= 0.99 max(xp): 0)."""
    xp = np.asarray(frequencies_in, dtype=np.float64)
    x = np.asarray(frequencies_out, dtype=np.float64)
    if xp.ndim != 1 or x.ndim != 1 or len(xp) < 2 or not np.isfinite(xp).all() or not np.isfinite(x).all() or \
            np.any(np.diff(xp) <= 0):
        raise ValueError("resample_plan: frequencies_in must be (B >= 2,) finite and ascending, frequencies_out (T,) "
                         "finite")
    pair = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 2)
    return {"pair": pair, "below": x < xp[0], "above": x >= xp[-1], "on": x == xp[pair],
            "outside": x >= 0.99 * np.max(xp), "dx": x - xp[pair], "span": xp[pair + 1] - xp[pair]}


def resample_spectra_host(spectra, frequencies_in, frequencies_out):
    """Spectrum.resample (BPMF/spectrum.py:851-887) of (..., B) spectra onto (T,) targets: np.interp of |spectra| --
    ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) (x - xp[j]) + fp[j], one rounded operation each, fp[j] itself on a
    band's frequency, the end values outside the bands -- and +0 at and beyond 0.99 max(frequencies_in)."""
    plan = resample_plan(frequencies_in, frequencies_out)
    fp = np.abs(np.asarray(spectra, dtype=np.float64))
    j = plan["pair"]
    with np.errstate(all="ignore"):
        lo, hi = fp[..., j], fp[..., j + 1]
        slope = (hi - lo) / plan["span"]
        out = slope * plan["dx"] + lo
        # np.interp's own second thoughts on a NaN: from the pair's other end, then equal ends
        out = np.where(np.isnan(out), slope * (plan["dx"] - plan["span"]) + hi, out)
        out = np.where(np.isnan(out) & (lo == hi), lo, out)
    out = np.where(plan["on"], lo, out)
    out = np.where(plan["below"], fp[..., :1], out)
    out = np.where(plan["above"], fp[..., -1:], out)
    return np.where(plan["outside"], 0.0, out)
